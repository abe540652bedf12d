"""A float64 restatement of the learner's output layers (multiagent_rl_amd.heads), written from the header comment of
csrc/pw_kernels_head.hpp, the stock float32 expression, and the inputs their tests share.

    A = relu ? max(X, 0) : X;   out_k = A W_k^T + b_k;
    dX = (sum_k dOut_k W_k) o (relu ? X > 0 : 1);   dW_k = dOut_k^T A;   db_k = sum over rows of dOut_k      (a head without dOut: nothing)

``make_inputs`` draws the parameters as ``nn.Linear(64, n)`` does and X ~ N(0, 1), with a few entries set to exactly +0.0, -0.0 and
tiny positive normal numbers: the mask's edge.  The mask is taken from the float32 X that both sides read, so float32 and float64
agree on it by construction and no row is drawn again.
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

HIDDEN = 64
TINY = 2.0 ** -100          # a positive float32 far above the denormals (2^-126): X > 0 holds, relu(X) = X


@functools.lru_cache(maxsize=None)
def make_inputs(rows, widths, seed=0):
    """-> (x [rows,64], (W_k), (b_k)) float32 CPU tensors.  Computed once per shape and left unchanged."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + sum(131 ** (i + 1) * n for i, n in enumerate(widths)))
    state = torch.random.get_rng_state()
    torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
    lins = [nn.Linear(HIDDEN, n) for n in widths]
    torch.random.set_rng_state(state)
    x = torch.randn(rows, HIDDEN, generator=g)
    flat = x.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:min(24, flat.numel() // 2)]
    for i, at in enumerate(where.tolist()):
        flat[at] = (0.0, -0.0, TINY)[i % 3]
    return x, tuple(lin.weight.detach().clone() for lin in lins), tuple(lin.bias.detach().clone() for lin in lins)


def forward(x, weights, biases, relu):
    """float64 -> [out_k]."""
    a = x.double().clamp_min(0.0) if relu else x.double()
    return [a @ w.double().t() + b.double() for w, b in zip(weights, biases)]


def backward(dOuts, x, weights, relu):
    """float64; ``dOuts``: per head a tensor or None -> dict: dx, and dW<k>, db<k> for the heads that have a dOut."""
    x = x.double()
    a = x.clamp_min(0.0) if relu else x
    out, dx = {}, torch.zeros_like(x)
    for k, (d, w) in enumerate(zip(dOuts, weights)):
        if d is None:
            continue
        d = d.double()
        dx = dx + d @ w.double()
        out['dW%d' % k], out['db%d' % k] = d.t() @ a, d.sum(0)
    out['dx'] = dx * (x > 0).double() if relu else dx
    return out


def stock(x, weights, biases, relu):
    """The stock expression in the dtype and on the device of its arguments: ``F.linear(F.relu(x), w, b)`` per head."""
    a = F.relu(x) if relu else x
    return [F.linear(a, w, b) for w, b in zip(weights, biases)]


def stock_grads(loss_of, x, weights, biases, relu):
    """``stock`` with autograd in every argument; ``loss_of(outs)`` is the scalar autograd sees -> (outs, dict as ``backward`` names it;
    a parameter that received no gradient is absent)."""
    leaf = lambda t: t.detach().clone().requires_grad_()  # noqa: E731
    x, weights, biases = leaf(x), [leaf(w) for w in weights], [leaf(b) for b in biases]
    outs = stock(x, weights, biases, relu)
    loss_of(outs).backward()
    res = dict(dx=x.grad)
    for k, (w, b) in enumerate(zip(weights, biases)):
        if w.grad is not None:
            res['dW%d' % k], res['db%d' % k] = w.grad, b.grad
    return [o.detach() for o in outs], res


# ---- stand-ins for the two launches (CPU tests) ----------------------------------------------------------------------------------
def launch_forward(x, weights, biases, relu):
    return [o.to(x.dtype) for o in forward(x, weights, biases, relu)]


def launch_backward(dOuts, x, weights, relu, want_dx):
    r = backward(dOuts, x, weights, relu)
    grab = lambda n: r[n].to(x.dtype).contiguous() if n in r else None  # noqa: E731
    return (grab('dx') if want_dx else None, [grab('dW%d' % k) for k in range(len(weights))], [grab('db%d' % k) for k in range(len(weights))])
