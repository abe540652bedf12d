#!/usr/bin/env python3
"""Generates tests/golden/bicnet_critic_forward.npz from the REFERENCE's BiCNet critic (rls.model.ac_network_multi_gumbel_BIC
CriticNetwork), on the CPU.  Run from the repo root where a checkout of the reference exists:

    python tests/golden/make_bicnet_golden.py <path of the reference checkout>

Per case (N, D, heads) of tests/critic_ref.py GOLDEN_CASES: the reference module's state_dict after its own default initialisation
under torch.manual_seed(seed), and the module's float32 and float64 outputs [GOLDEN_ROWS, N, 1] on the rows of
tests/critic_ref.py golden_inputs (drawn by the legacy NumPy generator, so the file carries their fingerprint, not the rows).
Data only; the reference itself never travels.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import critic_ref as cr  # noqa: E402


def main(reference_root):
    sys.path.insert(0, reference_root)
    from rls.model.ac_network_multi_gumbel_BIC import CriticNetwork
    arrays = {}
    for N, D, heads in cr.GOLDEN_CASES:
        name, seed = cr.golden_name(N, D, heads), 88000 + N
        torch.manual_seed(seed)
        net = CriticNetwork(D + sum(heads), 1).eval()
        obs, idx = cr.golden_inputs(N, D, heads)
        act = cr.one_hot(idx, heads)
        with torch.no_grad():
            q32 = net(torch.from_numpy(obs), torch.from_numpy(act)).numpy()
            sd = {k: v.clone() for k, v in net.state_dict().items()}
            q64 = net.double()(torch.from_numpy(obs).double(), torch.from_numpy(act).double()).numpy()
        for k, v in sd.items():
            arrays['%s/sd/%s' % (name, k)] = v.numpy()
        arrays[name + '/q32'], arrays[name + '/q64'] = q32, q64
        arrays[name + '/seed'] = np.array(seed)
        arrays[name + '/input_sum'] = np.array([obs.astype(np.float64).sum(), float(idx.sum())])   # fingerprint of golden_inputs
        print('%s: |q| <= %.3g, |q32 - q64| <= %.3g' % (name, np.abs(q64).max(), np.abs(q32 - q64).max()))
    out = os.path.join(HERE, 'bicnet_critic_forward.npz')
    np.savez_compressed(out, **arrays)
    print('%s: %d bytes' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
