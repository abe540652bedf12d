#!/usr/bin/env python3
"""Generates tests/golden/model_forward.npz from the REFERENCE's model-learning networks (rls.model.ac_network_model_multi_gumbel),
on the CPU.  Run from the repo root where a checkout of the reference exists:

    python tests/golden/make_model_golden.py <path of the reference checkout>

Critic, per case (N, D, heads) of tests/model_ref.py GOLDEN_CASES: the reference module's state_dict after its own default
initialisation under torch.manual_seed(seed), and both of its outputs (Q, r) in float32 and float64 on critic_ref.GOLDEN_ROWS input
rows (tests/critic_ref.py golden_inputs: the file carries their fingerprint, not the rows).  Actor, for ACTOR_CASES: its state_dict
and its float64 outputs (policy logits, predicted next observation) on the same observations.  Data only; the reference itself
never travels.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import critic_ref as cr  # noqa: E402
from tests import model_ref as mr  # noqa: E402


def main(reference_root):
    sys.path.insert(0, reference_root)
    from rls.model.ac_network_model_multi_gumbel import ActorNetwork, CriticNetwork
    arrays = {}
    for N, D, heads in mr.GOLDEN_CASES:
        name, seed = cr.golden_name(N, D, heads), 78000 + N
        torch.manual_seed(seed)
        net = CriticNetwork(D + sum(heads), 1).eval()
        obs, idx = cr.golden_inputs(N, D, heads)
        act = cr.one_hot(idx, heads)
        with torch.no_grad():
            q32, r32 = (t.numpy() for t in net(torch.from_numpy(obs), torch.from_numpy(act)))
            sd = {k: v.clone() for k, v in net.state_dict().items()}
            q64, r64 = (t.numpy() for t in net.double()(torch.from_numpy(obs).double(), torch.from_numpy(act).double()))
        for k, v in sd.items():
            arrays['%s/sd/%s' % (name, k)] = v.numpy()
        arrays[name + '/q32'], arrays[name + '/q64'], arrays[name + '/r32'], arrays[name + '/r64'] = q32, q64, r32, r64
        arrays[name + '/seed'] = np.array(seed)
        arrays[name + '/input_sum'] = np.array([obs.astype(np.float64).sum(), float(idx.sum())])   # fingerprint of golden_inputs
        print('critic %s: |q| <= %.3g, |r| <= %.3g, |q32 - q64| <= %.3g, |r32 - r64| <= %.3g' % (
            name, np.abs(q64).max(), np.abs(r64).max(), np.abs(q32 - q64).max(), np.abs(r32 - r64).max()))
        if (N, D, heads) in mr.ACTOR_CASES:
            torch.manual_seed(seed + 500)
            actor = ActorNetwork(D, heads[0] if len(heads) == 1 else list(heads)).eval()
            with torch.no_grad():
                asd = {k: v.clone() for k, v in actor.state_dict().items()}
                logits64, next64 = actor.double()(torch.from_numpy(obs).double())
            for k, v in asd.items():
                arrays['%s/actor_sd/%s' % (name, k)] = v.numpy()
            arrays[name + '/logits64'], arrays[name + '/next_state64'] = logits64.numpy(), next64.numpy()
            print('actor  %s: |logits| <= %.3g, |next_state| <= %.3g' % (name, np.abs(logits64.numpy()).max(), np.abs(next64.numpy()).max()))
    out = os.path.join(HERE, mr.GOLDEN_FILE)
    np.savez_compressed(out, **arrays)
    print('%s: %d bytes' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
