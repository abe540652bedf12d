"""GPU: pw_lstm_train_forward / pw_lstm_train_backward and their Python surface (multiagent_rl_amd.lstm: lstm_recurrence, FusedLSTM,
fuse_lstm, accelerate_trainer(lstm=True), the example learner's fused_lstm switch).

References: float64 nn.LSTM autograd, and tests/lstm_ref.py (the split form in float64, equal to that autograd to 1e-12:
tests/test_lstm_host.py).  Bounds:
  * the forward output: 2e-5, the project's bar for the actor's LSTM with these activations (v_exp_f32 / v_rcp_f32);
  * every gradient: 4 x max(e_stock, 2^-23 max|ref|), e_stock = the error of stock float32 nn.LSTM on the GPU against the same float64
    reference in the same run (the factor is tests/test_gpu_optim.py's for an equally long rounding chain; the second term is one
    float32 rounding of the largest entry, which keeps an exactly zero stock error from making the ratio meaningless).
At the kernel (dG, dW_hh from a given G) stock has no such entry point; it is given the SAME pre-activations through an identity
input projection (weight_ih = I, zero biases, x = G: a product with the identity is exact), and its dx is then its dG.

``PW_LSTM_F64_REPORT=<path>``: every case appends its figures there (profiles/lstm_train_vs_f64.txt is where such a run is kept).
"""
import copy
import functools
import os
import sys

import pytest

from tests import lstm_ref

torch = pytest.importorskip('torch')
nn, F = torch.nn, torch.nn.functional

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
IDS = ['b%d-N%d-%dx%d' % s for s in lstm_ref.SHAPES]


def _report(line):
    print(line)
    path = os.environ.get('PW_LSTM_F64_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _check(tag, kernel, stock, ref):
    """Every quantity of ``ref`` finite in ``kernel``; the output 'Y' within 2e-5 and every gradient within
    4 x max(e_stock, 2^-23 max|ref|); the figures go to the report."""
    for n in ref:
        assert n in kernel and bool(torch.isfinite(kernel[n]).all()), (tag, n)
    e_y = float((kernel['Y'].double().cpu() - ref['Y'].double().cpu()).abs().max()) if 'Y' in ref else 0.0
    grads = {n: r for n, r in ref.items() if n != 'Y'}
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(kernel, stock, grads)
    _report('%-58s Y %.3e  worst gradient %-22s kernel %.3e  stock %.3e  ratio %.2f' % (tag, e_y, worst, e_k, e_s, ratio))
    assert e_y <= 2e-5 and ratio <= 4.0, (tag, e_y, worst, e_k, e_s, ratio)


def _grads(lstm, x, loss):
    """{'Y', 'x', <parameter names>} of ``loss(lstm(x)[0])``."""
    x = x.detach().clone().requires_grad_(True)
    for p in lstm.parameters():
        p.grad = None
    Y = lstm(x)[0]
    loss(Y).backward()
    out = {'Y': Y.detach(), 'x': x.grad.detach()}
    out.update({n: p.grad.detach().clone() for n, p in lstm.named_parameters()})
    return out


@functools.lru_cache(maxsize=None)
def _case(b, N, dirs, H):
    """One shape's modules and inputs, made once: float64 on the CPU (the reference), stock float32 and fused float32 on the GPU, all
    three with the same (float32-representable) parameters and inputs."""
    from multiagent_rl_amd.lstm import fuse_lstm
    stock = lstm_ref.make_lstm(dirs, H, torch.float32, DEV)
    ref = copy.deepcopy(stock).cpu().double()
    fused = copy.deepcopy(stock)
    assert fuse_lstm(fused) == 1
    x, dY = lstm_ref.make_inputs(b, N, dirs, H, torch.float32)
    return stock, fused, ref, x, dY


def _three(shape, loss):
    stock, fused, ref, x, dY = _case(*shape)
    l64, l32 = (lambda Y: loss(Y, dY.double())), (lambda Y: loss(Y, dY.to(DEV)))
    return _grads(fused, x.to(DEV), l32), _grads(stock, x.to(DEV), l32), _grads(ref, x.double(), l64)


# ---- 1. forward -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', lstm_ref.SHAPES, ids=IDS)
def test_forward_against_float64(shape):
    stock, fused, ref, x, _ = _case(*shape)
    with torch.no_grad():
        want = ref(x.double())
        got, (h_n, c_n) = fused(x.to(DEV))
        base = stock(x.to(DEV))[0]
    err, e_s = float((got.double().cpu() - want[0]).abs().max()), float((base.double().cpu() - want[0]).abs().max())
    e_h = float((h_n.double().cpu() - want[1][0]).abs().max())
    e_c = float((c_n.double().cpu() - want[1][1]).abs().max())
    _report('forward %-50s Y %.3e (stock %.3e)  h_n %.3e  c_n %.3e   bound 2e-5' % (shape, err, e_s, e_h, e_c))
    assert err <= 2e-5 and e_h <= 2e-5 and e_c <= 2e-5 * max(1.0, float(want[1][1].abs().max()))


# ---- 2. / 3. gradients at the kernel ------------------------------------------------------------------------------------------------
def _identity_lstm(dirs, H, w_fw, w_bw):
    """Stock nn.LSTM that takes the pre-activations themselves: input [G of direction 0 | G of direction 1], weight_ih = the identity
    block of its direction, zero biases."""
    m = nn.LSTM(dirs * 4 * H, H, num_layers=1, batch_first=True, bidirectional=dirs == 2).to(DEV)
    eye = torch.eye(dirs * 4 * H, device=DEV)
    with torch.no_grad():
        for d, (sfx, w) in enumerate((('', w_fw), ('_reverse', w_bw))[:dirs]):
            getattr(m, 'weight_ih_l0' + sfx).copy_(eye[d * 4 * H:(d + 1) * 4 * H])
            getattr(m, 'weight_hh_l0' + sfx).copy_(w)
            getattr(m, 'bias_ih_l0' + sfx).zero_()
            getattr(m, 'bias_hh_l0' + sfx).zero_()
    return m


def _kernel_level(shape, g_scale=1.0, w_scale=1.0):
    from multiagent_rl_amd.lstm import lstm_recurrence
    b, N, dirs, H = shape
    lstm, _, _, x, dY = _case(*shape)
    with torch.no_grad():
        w_ih, bias, w_fw, w_bw = lstm_ref.projection(lstm)
        G = (F.linear(x.to(DEV), w_ih, bias) * g_scale).view(b, N, dirs, 4 * H).contiguous()
        ws = [(w * w_scale).clone() for w in (w_fw, w_bw) if w is not None]
    keys = ['weight_hh_l0', 'weight_hh_l0_reverse'][:dirs]
    # the kernels
    Gk, wk = G.clone().requires_grad_(True), [w.clone().requires_grad_(True) for w in ws]
    Y = lstm_recurrence(Gk, *wk)
    grads = torch.autograd.grad(Y, [Gk] + wk, dY.to(DEV))
    kernel = dict(zip(['Y', 'dG'] + keys, [Y.detach()] + list(grads)))
    # stock float32, fed the same G through the identity projection
    m = _identity_lstm(dirs, H, *(ws + [None])[:2])
    xs = G.reshape(b, N, dirs * 4 * H).clone().requires_grad_(True)
    Ys = m(xs)[0]
    Ys.backward(dY.to(DEV))
    stock = {'Y': Ys.detach(), 'dG': xs.grad.view(b, N, dirs, 4 * H)}
    stock.update({k: getattr(m, k).grad for k in keys})
    # the float64 restatement, fed the same G
    w64 = [w.double().cpu() for w in ws]
    Yr, saved = lstm_ref.forward(G.double().cpu(), *w64)
    dGr = lstm_ref.backward(dY.double(), saved, *w64)
    ref = dict(zip(['Y', 'dG'] + keys, [Yr, dGr] + [g for g in lstm_ref.whh_grads(dGr, Yr) if g is not None]))
    return kernel, stock, ref


@pytest.mark.parametrize('shape', lstm_ref.SHAPES, ids=IDS)
def test_kernel_gradients_against_the_float64_restatement(shape):
    _check('kernel dG, dW_hh %s' % (shape,), *_kernel_level(shape))


@pytest.mark.parametrize('shape', lstm_ref.SHAPES, ids=IDS)
def test_end_to_end_gradients_against_float64_autograd(shape):
    kernel, stock, ref = _three(shape, lambda Y, dY: (Y * dY).sum())
    assert len(ref) == 2 + 4 * shape[2]
    _check('FusedLSTM dx, dW_ih, dW_hh, db %s' % (shape,), kernel, stock, ref)


@pytest.mark.parametrize('shape', lstm_ref.SHAPES, ids=IDS)
def test_saturated_gates(shape):
    """G x 30 and W_hh x 4: sigmoids at 0 / 1 and tanh at +-1 in float32 (exp overflows to inf, 1 / inf = 0): nothing but finite numbers.

    This is the case the saved gates are made for (saved_sigmoid / saved_tanh, csrc/pw_kernels_lstm.hpp): the backward multiplies by
    o (1 - o), 1 - g^2 and 1 - tanh(c)^2, differences of numbers near 1 when the gates are saturated.  With the gates saved as
    fast_sigmoid / fast_tanh form them, b3-N64-1x64 had dG at 3.10e-06 against stock's 7.15e-07 (4.33 x) while the same backward fed
    exact gates was at 1.04 x (tools/lstm_saturation_split.py, profiles/lstm_train_saturated.txt)."""
    _check('saturated (G x 30, W_hh x 4) %s' % (shape,), *_kernel_level(shape, 30.0, 4.0))


@pytest.mark.parametrize('shape', [lstm_ref.SHAPES[1], lstm_ref.SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_small_outputs_keep_their_relative_accuracy(shape):
    """G x 0.05: tanh(g), tanh(c) and the output are a few hundredths.  The forward's Y is held to the gradients' bound here, 4 x
    max(e_stock, 2^-23 max|ref|): with the cell's tanh formed as 2 / (1 + e) - 1 (one rounding of 1, ~1e-7 absolute, whatever the value)
    Y missed it several times over, and in a whole update the critic's dense2.weight gradient stood at 4.97 x stock
    (tests/test_gpu_update_parity.py, two_head-b33).  The gradients are held as everywhere."""
    kernel, stock, ref = _kernel_level(shape, 0.05)
    assert float(ref['Y'].abs().max()) < 0.05
    ratio, _, e_k, e_s = lstm_ref.worst_ratio(kernel, stock, {'Y': ref['Y']})
    _report('small outputs (G x 0.05) %-34s Y kernel %.3e  stock %.3e  largest %.3e  ratio %.2f' % (shape, e_k, e_s, float(ref['Y'].abs().max()), ratio))
    assert ratio <= 4.0, (shape, e_k, e_s, ratio)
    _check('small outputs (G x 0.05) %s' % (shape,), kernel, stock, ref)


# ---- 4. gradient patterns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', lstm_ref.SHAPES, ids=IDS)
def test_gradient_patterns(shape):
    H = shape[3]
    _check('Y.sum() (expanded dY) %s' % (shape,), *_three(shape, lambda Y, dY: Y.sum()))
    _check('only Y[:, -1] (the h_n path) %s' % (shape,), *_three(shape, lambda Y, dY: (Y[:, -1] * dY[:, -1]).sum()))
    if shape[2] == 2:
        k, s, r = _three(shape, lambda Y, dY: (Y[:, :, H:] * dY[:, :, H:]).sum())
        assert float(k['weight_hh_l0'].abs().max()) == 0.0 and float(k['weight_ih_l0'].abs().max()) == 0.0
        _check('only direction 1 %s' % (shape,), k, s, r)


# ---- 5. exactness of the plumbing ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [lstm_ref.SHAPES[2], lstm_ref.SHAPES[3], lstm_ref.SHAPES[0]], ids=[IDS[2], IDS[3], IDS[0]])
def test_plumbing_is_exact(shape):
    from multiagent_rl_amd import lstm as L
    b, N, dirs, H = shape
    stock, _, _, x, dY = _case(*shape)
    with torch.no_grad():
        w_ih, bias, w_fw, w_bw = lstm_ref.projection(stock)
        G = F.linear(x.to(DEV), w_ih, bias).view(b, N, dirs, 4 * H).contiguous()
        w_fw = w_fw.detach().clone()
        w_bw = None if w_bw is None else w_bw.detach().clone()
    dYd = dY.to(DEV)
    bits = lambda t: t.view(torch.int32)   # noqa: E731
    Y0, none = L.launch_forward(G, w_fw, w_bw, False)
    Y1, saved = L.launch_forward(G, w_fw, w_bw, True)
    assert none is None and torch.equal(bits(Y0), bits(Y1))                           # saving changes nothing of Y
    dG1 = L.launch_backward(dYd, saved, w_fw, w_bw)
    Y2, saved2 = L.launch_forward(G, w_fw, w_bw, True)
    dG2 = L.launch_backward(dYd, saved2, w_fw, w_bw)
    assert torch.equal(bits(Y1), bits(Y2)) and torch.equal(bits(saved), bits(saved2)) and torch.equal(bits(dG1), bits(dG2))   # two runs
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Y3, saved3 = L.launch_forward(G, w_fw, w_bw, True)
        dG3 = L.launch_backward(dYd, saved3, w_fw, w_bw)
    torch.cuda.current_stream().wait_stream(side)
    assert torch.equal(bits(Y1), bits(Y3)) and torch.equal(bits(dG1), bits(dG3))        # a second stream
    views = []
    for w in (w_fw, w_bw):                                                                # weights one element into a larger storage
        if w is None:
            views.append(None)
            continue
        big = torch.full((w.numel() + 7,), float('nan'), device=DEV)
        big[1:1 + w.numel()] = w.reshape(-1)
        views.append(big[1:1 + w.numel()].view_as(w))
        assert views[-1].data_ptr() % 16 == 4 and views[-1].is_contiguous()
    Y4, saved4 = L.launch_forward(G, views[0], views[1], True)
    dG4 = L.launch_backward(dYd, saved4, views[0], views[1])
    assert torch.equal(bits(Y1), bits(Y4)) and torch.equal(bits(dG1), bits(dG4))


# ---- 6. the networks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,N', [(33, 6), (5, 13)])
@pytest.mark.parametrize('name', lstm_ref.NETWORKS)
def test_networks_against_float64(name, b, N):
    from multiagent_rl_amd.lstm import fuse_lstm
    stock = lstm_ref.make_network(name).to(DEV)
    fused, ref = copy.deepcopy(stock), copy.deepcopy(stock).double()
    assert fuse_lstm(fused) == 1
    inputs = lstm_ref.network_inputs(name, b, N, torch.float32, DEV)
    g_ref = lstm_ref.network_grads(ref, tuple(t.double() for t in inputs))
    _check('%s b=%d N=%d' % (name, b, N), lstm_ref.network_grads(fused, inputs), lstm_ref.network_grads(stock, inputs), g_ref)


def _sample(logits, seed):
    """F.gumbel_softmax(logits, hard=True) with the noise drawn in float32 from a reseeded torch, whatever the dtype of ``logits``: the
    float64 copies see the numbers the float32 networks see."""
    torch.manual_seed(seed)
    g = -torch.empty(logits.shape, dtype=torch.float32, device=logits.device).exponential_().log()
    soft = F.softmax(logits + g.to(logits.dtype), dim=-1)
    hard = torch.zeros_like(soft).scatter_(-1, soft.argmax(dim=-1, keepdim=True), 1.0)
    return hard - soft.detach() + soft


def _update_grads(actor, critic, batch, y):
    """One update's two losses as examples/madr_learner.py forms them, without the optimiser steps: every .grad of the critic after
    loss_critic.backward(), and of actor and critic after loss_actor.backward() (the critic's accumulate, as in the learner)."""
    s0, a0 = batch
    for p in list(actor.parameters()) + list(critic.parameters()):
        p.grad = None
    F.smooth_l1_loss(critic(s0, a0), y).backward()
    out = {'critic_loss/' + n: p.grad.detach().clone() for n, p in critic.named_parameters()}
    loss_actor = -critic(s0, _sample(actor(s0), 77)).mean()
    loss_actor.backward()
    out.update({'actor_loss/critic.' + n: p.grad.detach().clone() for n, p in critic.named_parameters()})
    out.update({'actor_loss/actor.' + n: p.grad.detach().clone() for n, p in actor.named_parameters()})
    return out


@pytest.mark.parametrize('b,N', [(33, 6), (5, 13)])
def test_one_update_of_the_learner_against_float64(b, N):
    from multiagent_rl_amd.lstm import fuse_lstm
    actor, critic = lstm_ref.make_network('actor').to(DEV), lstm_ref.make_network('critic', seed=1).to(DEV)
    s0, = lstm_ref.network_inputs('actor', b, N, torch.float32, DEV)
    g = torch.Generator().manual_seed(9)
    a0 = F.one_hot(torch.randint(0, 5, (b, N), generator=g), 5).float().to(DEV)
    y = torch.randn(b, 1, generator=g).to(DEV)
    nets = {'stock': (actor, critic), 'fused': (copy.deepcopy(actor), copy.deepcopy(critic)),
            'ref': (copy.deepcopy(actor).double(), copy.deepcopy(critic).double())}
    assert fuse_lstm(nets['fused'][0]) == 1 and fuse_lstm(nets['fused'][1]) == 1
    grads = {k: _update_grads(a, c, (s0.to(next(a.parameters()).dtype), a0.to(next(a.parameters()).dtype)), y.to(next(a.parameters()).dtype))
             for k, (a, c) in nets.items()}
    assert float(grads['ref']['actor_loss/actor.bilstm.weight_hh_l0'].abs().max()) > 0
    _check('one update (critic loss, actor loss) b=%d N=%d' % (b, N), grads['fused'], grads['stock'], grads['ref'])


# ---- 7. the entry points ------------------------------------------------------------------------------------------------------------
class _OneBatch(object):
    """What examples/madr_learner.py's Trainer asks of its memory, serving the batch it was last given."""
    batch = None

    def make_index(self, n):
        return None

    def sample_index(self, idx):
        return self.batch


def _batch(g, b=64, N=3, D=10):
    s0, s1 = torch.randn(b, N, D, generator=g), torch.randn(b, N, D, generator=g)
    a0 = F.one_hot(torch.randint(0, 5, (b, N), generator=g), 5).float()
    return s0.numpy(), a0.numpy(), torch.randn(b, generator=g).numpy(), s1.numpy(), (torch.rand(b, generator=g) < 0.1).float().numpy()


# lr: Adam's first step is lr g / (|g| + eps), which turns a last-bit difference of a gradient entry near eps into a parameter difference of
# up to lr -- the reason the networks above are compared by gradient.  loss_actor of the first call is formed after the critic's step, so
# at the learner's lr = 1e-2 a single such entry could move it by ~1e-4 with nothing wrong; at 1e-4 that effect is below 1e-6 and the
# 1e-5 bound checks what it is meant to check, that the switch changes the plumbing and not the losses.
LR = 1e-4


@pytest.mark.parametrize('how', ['accelerate_trainer', 'fused_lstm', 'targets+optimizer+lstm'])
def test_trainer_entry_points(how):
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import madr_learner
    finally:
        sys.path.pop(0)
    from multiagent_rl_amd.critic import CriticNetwork, accelerate_trainer
    from multiagent_rl_amd.lstm import FusedLSTM
    from multiagent_rl_amd.policy import ActorNetwork
    trainers = []
    for switch in (False, True):
        torch.manual_seed(11)
        trainers.append(madr_learner.Trainer(ActorNetwork(10, 5), CriticNetwork(15, 1), _OneBatch(), batch_size=64, lr=LR,
                                             fused_lstm=switch and how == 'fused_lstm'))
    plain, fused = trainers
    if how == 'accelerate_trainer':
        accelerate_trainer(fused, seed=3, lstm=True)
    elif how != 'fused_lstm':
        accelerate_trainer(fused, seed=3, targets=True, optimizer=True, lstm=True)
    assert type(plain.actor.bilstm) is nn.LSTM and type(plain.critic.lstm) is nn.LSTM
    assert type(fused.actor.bilstm) is FusedLSTM and type(fused.critic.lstm) is FusedLSTM
    if how != 'targets+optimizer+lstm':
        assert type(fused.target_actor.bilstm) is FusedLSTM and type(fused.target_critic.lstm) is FusedLSTM
    g = torch.Generator().manual_seed(6)
    for it in range(3):
        plain.memory.batch = fused.memory.batch = _batch(g)
        torch.manual_seed(200 + it)
        lp = plain.optimize()
        torch.manual_seed(200 + it)
        lf = fused.optimize()
        assert all(x == x and abs(x) != float('inf') for x in lp + lf), (lp, lf)
        if it == 0:
            _report('%-24s first optimize(): loss_actor %.8f / %.8f  loss_critic %.8f / %.8f (unpatched / switched)' % (
                how, lp[0], lf[0], lp[1], lf[1]))
            for a, c in zip(lp, lf):
                assert abs(a - c) <= 1e-5 * max(1.0, abs(a)), (how, lp, lf)
