"""A float64 restatement of the dense front (multiagent_rl_amd.dense) and the inputs its tests share.

    hid = relu([x0 | x1] w1^T + b1);   G = hid [W_ih of direction 0; of direction 1]^T + (b_ih + b_hh)

``make_inputs`` draws the parameters as torch does by default (``nn.Linear(d0 + d1, 64)``, ``nn.LSTM(64, H, bidirectional=dirs == 2)``),
N(0, 1) observation rows and a one-hot action part.  The ReLU's mask is discontinuous: a row with a hidden unit whose float64
pre-activation lies within ``MARGIN`` = 1e-5 of zero is drawn again (the largest float32 error of that pre-activation is below 1e-6),
so that a float32 computation and the float64 one agree on the mask; ``redrawn`` reports the share of such rows.
"""
import functools

import torch
import torch.nn as nn
import torch.nn.functional as F

MARGIN = 1e-5
HIDDEN = 64


def pre_activation(x0, x1, w1, b1):
    x = x0 if x1 is None else torch.cat([x0, x1], dim=-1)
    return x.double() @ w1.double().t() + b1.double()


@functools.lru_cache(maxsize=None)
def make_inputs(rows, d0, d1, dirs, seed=0):
    """-> dict of float32 CPU tensors: x0 [rows,d0], x1 [rows,d1] or None, w1, b1, w_ih / b_ih / b_hh (tuples, one per direction), and
    ``redrawn`` (share of the rows drawn more than once).  Computed once per shape and left unchanged."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * rows + 131 * d0 + 17 * d1 + dirs)
    state = torch.random.get_rng_state()
    torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
    lin, lstm = nn.Linear(d0 + d1, HIDDEN), nn.LSTM(HIDDEN, 64 // dirs, num_layers=1, batch_first=True, bidirectional=dirs == 2)
    torch.random.set_rng_state(state)
    w1, b1 = lin.weight.detach().clone(), lin.bias.detach().clone()
    names = ['_l0'] + (['_l0_reverse'] if dirs == 2 else [])
    w_ih, b_ih, b_hh = (tuple(getattr(lstm, kind + n).detach().clone() for n in names) for kind in ('weight_ih', 'bias_ih', 'bias_hh'))

    def draw(n):
        x0 = torch.randn(n, d0, generator=g)
        x1 = F.one_hot(torch.randint(0, d1, (n,), generator=g), d1).float() if d1 else None
        return x0, x1
    x0, x1 = draw(rows)
    again = torch.zeros(rows, dtype=torch.bool)
    for _ in range(100):
        close = (pre_activation(x0, x1, w1, b1).abs() < MARGIN).any(dim=1)
        if not bool(close.any()):
            break
        again |= close
        n0, n1 = draw(int(close.sum()))
        x0[close] = n0
        if d1:
            x1[close] = n1
    else:
        raise AssertionError('rows keep landing on the ReLU\'s kink')
    return dict(x0=x0, x1=x1, w1=w1, b1=b1, w_ih=w_ih, b_ih=b_ih, b_hh=b_hh, redrawn=float(again.float().mean()))


def forward(x0, x1, w1, b1, w_ih, b_ih, b_hh):
    """float64 -> (hid [rows,64], G [rows,256])."""
    hid = pre_activation(x0, x1, w1, b1).clamp_min(0.0)
    w = torch.cat([t.double() for t in w_ih], dim=0)
    b = torch.cat([bi.double() + bh.double() for bi, bh in zip(b_ih, b_hh)], dim=0)
    return hid, hid @ w.t() + b


def backward(dG, x0, x1, h, w1, w_ih):
    """float64, from ``h`` (hid as the forward left it; ``h > 0`` is the mask) -> dict: dW1, db1, dW_ih0 (dW_ih1), db_gate0 (db_gate1),
    dx0, dx1 (with an x1)."""
    dG, h = dG.double(), h.double()
    x = (x0 if x1 is None else torch.cat([x0, x1], dim=-1)).double()
    w = torch.cat([t.double() for t in w_ih], dim=0)
    dhid = (dG @ w) * (h > 0).double()
    out = dict(dW1=dhid.t() @ x, db1=dhid.sum(0))
    rows_per = w.shape[0] // len(w_ih)
    for d in range(len(w_ih)):
        part = dG[:, d * rows_per:(d + 1) * rows_per]
        out['dW_ih%d' % d] = part.t() @ h
        out['db_gate%d' % d] = part.sum(0)
    dx = dhid @ w1.double()
    out['dx0'] = dx[:, :x0.shape[1]]
    if x1 is not None:
        out['dx1'] = dx[:, x0.shape[1]:]
    return out


def stock(x0, x1, w1, b1, w_ih, b_ih, b_hh):
    """The stock expression, in the dtype and on the device of its arguments, as the networks write it: the cat, dense1, the ReLU, and
    ``FusedLSTM.forward``'s one ``F.linear`` over the concatenated weights and summed biases -> G."""
    x = x0 if x1 is None else torch.cat([x0, x1], dim=-1)
    hid = F.relu(F.linear(x, w1, b1))
    if len(w_ih) == 2:
        w, b = torch.cat(list(w_ih), dim=0), torch.cat([b_ih[0] + b_hh[0], b_ih[1] + b_hh[1]], dim=0)
    else:
        w, b = w_ih[0], b_ih[0] + b_hh[0]
    return F.linear(hid, w, b)


def stock_grads(dG_of, x0, x1, w1, b1, w_ih, b_ih, b_hh):
    """``stock`` with autograd in every argument; ``dG_of(G)`` is the scalar autograd sees -> (G, dict as ``backward`` names it)."""
    leaf = lambda t: None if t is None else t.detach().clone().requires_grad_()  # noqa: E731
    x0, x1, w1, b1 = leaf(x0), leaf(x1), leaf(w1), leaf(b1)
    w_ih, b_ih, b_hh = [leaf(t) for t in w_ih], [leaf(t) for t in b_ih], [leaf(t) for t in b_hh]
    G = stock(x0, x1, w1, b1, w_ih, b_ih, b_hh)
    dG_of(G).backward()
    out = dict(dW1=w1.grad, db1=b1.grad, dx0=x0.grad)
    if x1 is not None:
        out['dx1'] = x1.grad
    for d in range(len(w_ih)):
        out['dW_ih%d' % d], out['db_gate%d' % d], out['db_hh%d' % d] = w_ih[d].grad, b_ih[d].grad, b_hh[d].grad
    return G.detach(), out
