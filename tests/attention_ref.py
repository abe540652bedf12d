"""The attention block of CriticNetwork in plain torch, in any dtype: what pw_attention_pool_forward / pw_attention_pool_backward
compute, written from include/pworld.h and not from the kernels.

``forward``: scores against the last step, softmax over the steps (maximum subtracted), weighted sum, optional ReLU; ``backward``: the
gradient at ``Y`` by the formulas of the header.  ``launch_forward`` / ``launch_backward`` have the signatures of the two overridable
launch functions of multiagent_rl_amd.attention, so a CPU test can put them in their place.  ``stock``: the expression of
``critic.py`` itself (two ``bmm``s and a softmax), for autograd."""
import torch
import torch.nn.functional as F

SHAPES = [(1, 1), (5, 2), (17, 3), (33, 6), (16, 13), (3, 64)]   # (b, N): the one-direction entries of lstm_ref.SHAPES


def forward(Y, relu=True):
    """Y [b,N,H] -> out [b,H], weight [b,N]."""
    q = Y[:, -1]
    s = (Y * q.unsqueeze(1)).sum(dim=2)
    e = torch.exp(s - s.max(dim=1, keepdim=True).values)
    w = e / e.sum(dim=1, keepdim=True)
    c = torch.zeros_like(q)
    for t in range(Y.shape[1]):
        c = c + w[:, t:t + 1] * Y[:, t]
    return (c.clamp_min(0) if relu else c), w


def backward(dOut, Y, weight, out, relu=True):
    """-> dY [b,N,H]."""
    q = Y[:, -1]
    dc = dOut * (out > 0).to(dOut.dtype) if relu else dOut
    dw = (Y * dc.unsqueeze(1)).sum(dim=2)
    ds = weight * (dw - (weight * dw).sum(dim=1, keepdim=True))
    dY = weight.unsqueeze(2) * dc.unsqueeze(1) + ds.unsqueeze(2) * q.unsqueeze(1)
    dq = torch.zeros_like(q)
    for t in range(Y.shape[1]):
        dq = dq + ds[:, t:t + 1] * Y[:, t]
    dY[:, -1] = dY[:, -1] + dq
    return dY


# ---- stand-ins for multiagent_rl_amd.attention.launch_forward / launch_backward (any device, any dtype) --------------------------
def launch_forward(Y, relu, keep):
    out, w = forward(Y, relu)
    return out, (w if keep else None)


def launch_backward(dOut, Y, weight, out, relu):
    return backward(dOut, Y, weight, out, relu)


def stock(steps, relu=True):
    """critic.py:41-45 with h_n[-1] = steps[:, -1]."""
    score = torch.bmm(steps, steps[:, -1].unsqueeze(2)).squeeze(2)
    weight = F.softmax(score, dim=1)
    ctx = torch.bmm(steps.transpose(1, 2), weight.unsqueeze(2)).squeeze(2)
    return F.relu(ctx) if relu else ctx


def make_inputs(b, N, dtype, device='cpu', seed=1, H=64):
    """Y [b,N,H] of the size of an LSTM's output (|y| < 1) and a fixed NON-uniform dOut [b,H], from a CPU generator: the same numbers
    on every device, float32-representable."""
    g = torch.Generator().manual_seed(seed + 1000 * b + N)
    Y = torch.tanh(torch.randn(b, N, H, generator=g, dtype=torch.float64)).float()
    dOut = (torch.randn(b, H, generator=g, dtype=torch.float64) * torch.linspace(0.25, 2.0, H, dtype=torch.float64)).float()
    return Y.to(device=device, dtype=dtype), dOut.to(device=device, dtype=dtype)


def grads(fn, Y, loss):
    """{'out', 'dY'} of ``loss(fn(Y))`` by autograd."""
    Y = Y.detach().clone().requires_grad_(True)
    out = fn(Y)
    loss(out).backward()
    return {'out': out.detach(), 'dY': Y.grad.detach()}
