"""The split form of a one-layer LSTM in plain torch, in any dtype: what pw_lstm_train_forward / pw_lstm_train_backward and
multiagent_rl_amd/lstm.py compute together, written from include/pworld.h and not from the kernels.

``forward``: the recurrence from the pre-activations ``G = x W_ih^T + b_ih + b_hh`` with the activations of every step kept;
``backward``: the backward recurrence (gradient at the pre-activations); ``whh_grads``: the two W_hh GEMMs.  ``launch_forward`` /
``launch_backward`` have the signatures of the two overridable launch functions of multiagent_rl_amd.lstm, so a CPU test can put
them in their place.  ``split_grads``: everything an ``nn.LSTM``'s autograd returns, from the pieces above."""
import torch
import torch.nn.functional as F


def _steps(N, d):
    """The time indices of direction ``d`` in its forward order."""
    return list(range(N - 1, -1, -1)) if d else list(range(N))


def forward(G, w_hh_fw, w_hh_bw=None):
    """G [b,N,dirs,4H] -> Y [b,N,dirs*H], saved [b,N,dirs,5,H] (i, f, g, o after activation, c)."""
    b, N, dirs, H = G.shape[0], G.shape[1], G.shape[2], G.shape[3] // 4
    Y = G.new_zeros(b, N, dirs * H)
    saved = G.new_zeros(b, N, dirs, 5, H)
    for d, W in enumerate((w_hh_fw, w_hh_bw)[:dirs]):
        h, c = G.new_zeros(b, H), G.new_zeros(b, H)
        for t in _steps(N, d):
            a = G[:, t, d] + h @ W.t()
            i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            Y[:, t, d * H:(d + 1) * H] = h
            saved[:, t, d] = torch.stack([i, f, g, o, c], dim=1)
    return Y, saved


def backward(dY, saved, w_hh_fw, w_hh_bw=None):
    """dY [b,N,dirs*H], saved -> dG [b,N,dirs,4H]."""
    b, N, dirs, _, H = saved.shape
    dG = saved.new_zeros(b, N, dirs, 4 * H)
    for d, W in enumerate((w_hh_fw, w_hh_bw)[:dirs]):
        order = _steps(N, d)
        dh, dc = saved.new_zeros(b, H), saved.new_zeros(b, H)
        for s in range(N - 1, -1, -1):
            t = order[s]
            i, f, g, o, c = saved[:, t, d].unbind(dim=1)
            c_prev = saved[:, order[s - 1], d, 4] if s > 0 else torch.zeros_like(c)
            tc = torch.tanh(c)
            dht = dY[:, t, d * H:(d + 1) * H] + dh
            d_o = dht * tc * o * (1 - o)
            dct = dc + dht * o * (1 - tc * tc)
            d_i = dct * g * i * (1 - i)
            d_f = dct * c_prev * f * (1 - f)
            d_g = dct * i * (1 - g * g)
            dG[:, t, d] = torch.cat([d_i, d_f, d_g, d_o], dim=1)
            dh = dG[:, t, d] @ W
            dc = dct * f
    return dG


def whh_grads(dG, Y):
    """-> (dW_hh forward [4H,H], dW_hh reverse or None): dG^T against the output of the direction's previous step."""
    H = dG.shape[3] // 4
    d_fw = dG[:, 1:, 0].reshape(-1, 4 * H).t() @ Y[:, :-1, :H].reshape(-1, H)
    d_bw = None
    if dG.shape[2] == 2:
        d_bw = dG[:, :-1, 1].reshape(-1, 4 * H).t() @ Y[:, 1:, H:].reshape(-1, H)
    return d_fw, d_bw


# ---- stand-ins for multiagent_rl_amd.lstm.launch_forward / launch_backward (any device, any dtype) ------------------------------
def launch_forward(G, w_hh_fw, w_hh_bw, keep):
    Y, saved = forward(G, w_hh_fw, w_hh_bw)
    return Y, (saved if keep else None)


def launch_backward(dY, saved, w_hh_fw, w_hh_bw):
    return backward(dY, saved, w_hh_fw, w_hh_bw)


def projection(lstm):
    """(W_ih of all directions stacked [dirs*4H, I], b_ih + b_hh stacked [dirs*4H], w_hh_fw, w_hh_bw or None) of a one-layer nn.LSTM."""
    if lstm.bidirectional:
        return (torch.cat([lstm.weight_ih_l0, lstm.weight_ih_l0_reverse]),
                torch.cat([lstm.bias_ih_l0 + lstm.bias_hh_l0, lstm.bias_ih_l0_reverse + lstm.bias_hh_l0_reverse]),
                lstm.weight_hh_l0, lstm.weight_hh_l0_reverse)
    return lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0, lstm.weight_hh_l0, None


@torch.no_grad()
def split_grads(lstm, x, dY):
    """Output and every gradient of ``(lstm(x)[0] * dY).sum()`` from the split form, in the dtype of ``lstm`` and ``x``:
    {'Y', 'G', 'dG', 'x', 'weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0' (+ '_reverse')}."""
    w_ih, bias, w_fw, w_bw = projection(lstm)
    dirs, H = (2 if lstm.bidirectional else 1), lstm.hidden_size
    b, N = x.shape[0], x.shape[1]
    G = F.linear(x, w_ih, bias).view(b, N, dirs, 4 * H)
    Y, saved = forward(G, w_fw, w_bw)
    dG = backward(dY, saved, w_fw, w_bw)
    d_fw, d_bw = whh_grads(dG, Y)
    flat = dG.reshape(b * N, dirs * 4 * H)
    d_wih, d_b = flat.t() @ x.reshape(b * N, -1), flat.sum(dim=0)
    out = {'Y': Y, 'G': G, 'dG': dG, 'x': (flat @ w_ih).view_as(x)}
    for d, sfx in enumerate(('', '_reverse')[:dirs]):
        out['weight_ih_l0' + sfx] = d_wih[d * 4 * H:(d + 1) * 4 * H]
        out['bias_ih_l0' + sfx] = out['bias_hh_l0' + sfx] = d_b[d * 4 * H:(d + 1) * 4 * H]
        out['weight_hh_l0' + sfx] = d_bw if d else d_fw
    return out


def autograd_grads(lstm, x, dY):
    """The same dictionary (without 'G' / 'dG') from torch's own autograd through ``lstm(x)``."""
    x = x.detach().clone().requires_grad_(True)
    for p in lstm.parameters():
        p.grad = None
    Y = lstm(x)[0]
    (Y * dY).sum().backward()
    out = {'Y': Y.detach(), 'x': x.grad}
    for n, p in lstm.named_parameters():
        out[n] = p.grad.clone()
        p.grad = None
    return out


SHAPES = [(1, 1, 1, 64), (5, 2, 2, 32), (17, 3, 1, 64), (33, 6, 2, 32), (16, 13, 1, 64), (3, 64, 1, 64), (3, 50, 2, 32)]   # (b, N, dirs, H)


def make_lstm(dirs, H, dtype, device='cpu', seed=0, input_size=64):
    torch.manual_seed(seed)
    return torch.nn.LSTM(input_size, H, num_layers=1, batch_first=True, bidirectional=dirs == 2).to(device=device, dtype=dtype)


def make_inputs(b, N, dirs, H, dtype, device='cpu', seed=1, input_size=64):
    """x [b,N,I] and a fixed NON-uniform dY [b,N,dirs*H] (from a CPU generator: the same numbers on every device)."""
    g = torch.Generator().manual_seed(seed + 1000 * b + N)
    x = torch.randn(b, N, input_size, generator=g, dtype=torch.float64)
    dY = torch.randn(b, N, dirs * H, generator=g, dtype=torch.float64) * torch.linspace(0.25, 2.0, dirs * H, dtype=torch.float64)
    return x.to(device=device, dtype=dtype), dY.to(device=device, dtype=dtype)


# ---- the four served networks: a scalar loss with fixed non-uniform weights, and every parameter gradient -----------------------
def make_network(name, seed=0):
    from multiagent_rl_amd.critic import BiCNetCritic, CriticNetwork
    from multiagent_rl_amd.policy import ActorNetwork
    torch.manual_seed(seed)
    return {'actor': lambda: ActorNetwork(10, 5), 'actor2': lambda: ActorNetwork(21, [5, 10]),
            'critic': lambda: CriticNetwork(15, 1), 'bicnet': lambda: BiCNetCritic(15, 1)}[name]()


NETWORKS = ('actor', 'actor2', 'critic', 'bicnet')


def network_inputs(name, b, N, dtype, device='cpu', seed=3):
    g = torch.Generator().manual_seed(seed + 100 * b + N)
    widths = {'actor': (10,), 'actor2': (21,), 'critic': (10, 5), 'bicnet': (10, 5)}[name]
    return tuple(torch.randn(b, N, w, generator=g, dtype=torch.float64).to(device=device, dtype=dtype) for w in widths)


def network_loss(net, inputs):
    out = net(*inputs)
    outs = list(out) if isinstance(out, (list, tuple)) else [out]
    return sum((o * torch.cos(torch.arange(o.numel(), device=o.device).to(o.dtype)).view_as(o)).sum() for o in outs)


def network_grads(net, inputs):
    for p in net.parameters():
        p.grad = None
    network_loss(net, inputs).backward()
    out = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    return out


def worst_ratio(kernel, stock, ref):
    """Over the quantities of three dictionaries (under test, stock float32, float64 reference): the largest
    error / max(e_stock, one float32 rounding of the largest entry), with its name -- the bound of the tests is 4."""
    worst = (0.0, None, 0.0, 0.0)
    for n, r in ref.items():
        if n not in kernel:
            continue
        r = r.detach().double().cpu()
        e_k = float((kernel[n].detach().double().cpu() - r).abs().max())
        e_s = float((stock[n].detach().double().cpu() - r).abs().max())
        ratio = e_k / max(e_s, 2.0 ** -23 * float(r.abs().max()), 1e-300)
        if ratio > worst[0]:
            worst = (ratio, n, e_k, e_s)
    return worst
