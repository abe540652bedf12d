"""The learner's Gumbel-softmax sample in plain torch, in any dtype: what pw_gumbel_st_forward / pw_gumbel_st_backward compute
(multiagent_rl_amd/csrc/pw_kernels_sample.hpp), the stock expression they replace, and stand-ins with the signatures of
multiagent_rl_amd.sampling's launches for the CPU tests.  The noise is oracle/actor_oracle.py's restatement of the device's draw."""
import numpy as np
import torch

from oracle import actor_oracle


def noise(seed, step, rows, n):
    """float64 [rows, n]: log(-log u) of (seed; step, row 0 .. rows-1)."""
    return torch.from_numpy(actor_oracle.gumbel_noise(int(seed), int(step), np.arange(rows), n))


def forward(logits, nz, tau, hard):
    """-> (y, soft, idx): v = (logits - nz) / tau, the first maximum, softmax, (onehot - soft) + soft."""
    v = (logits - nz.to(logits.dtype)) / tau
    idx = torch.from_numpy(np.argmax(v.detach().cpu().numpy(), axis=-1))          # NumPy's argmax: the FIRST maximum
    soft = torch.softmax(v, dim=-1)
    onehot = torch.nn.functional.one_hot(idx.to(soft.device), v.shape[-1]).to(soft.dtype)
    return ((onehot - soft) + soft if hard else soft), soft, idx.to(torch.int32)


def backward(dY, soft, tau):
    return soft * (dY - (dY * soft).sum(dim=-1, keepdim=True)) / tau


def stock(logits, nz, tau, hard):
    """torch.nn.functional.gumbel_softmax's own lines with the gumbels given (gumbels = -nz): differentiable in ``logits``."""
    y_soft = ((logits - nz.to(logits.dtype)) / tau).softmax(-1)
    if not hard:
        return y_soft
    index = y_soft.max(-1, keepdim=True)[1]
    y_hard = torch.zeros_like(logits).scatter_(-1, index, 1.0)
    return y_hard - y_soft.detach() + y_soft


# ---- stand-ins of sampling.launch_forward / launch_backward / launch_advance (same signatures) ------------------------------------
def launch_forward(logits, tau, hard, seed, step, cell, keep, want_idx=False, want_noise=False):
    rows, n = logits.shape
    nz = noise(seed, int(step) + (int(cell[0]) if cell is not None else 0), rows, n).to(logits.dtype)
    y, soft, idx = forward(logits.detach(), nz, tau, hard)
    return y, (soft if keep else None), (idx if want_idx else None), (nz if want_noise else None)


def launch_backward(dY, soft, tau):
    return backward(dY, soft, tau)


def launch_advance(cell, delta):
    cell += int(delta)
