"""GPU: pw_attention_pool_forward / pw_attention_pool_backward and their Python surface (multiagent_rl_amd.attention: attention_pool,
fuse_attention, accelerate_trainer(attention=True), the example learner's fused_attention switch).

Reference: tests/attention_ref.py in float64 (equal to float64 autograd of the stock expression to 1e-12: tests/test_attention_host.py).
Bound, the project's own (tests/test_gpu_lstm_train.py): every quantity within 4 x max(e_stock, 2^-23 max|ref|), e_stock = the error of the
stock float32 expression (bmm, softmax, bmm, relu under autograd) on the GPU against the same float64 reference in the same run; the
second term is one float32 rounding of the largest entry, which keeps an exactly zero stock error from making the ratio meaningless.

``PW_ATTN_F64_REPORT=<path>``: every case appends its figures there (profiles/attention_vs_f64.txt is where such a run is kept).
"""
import copy
import functools
import os
import sys

import pytest

from tests import attention_ref, lstm_ref

torch = pytest.importorskip('torch')
nn, F = torch.nn, torch.nn.functional

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
SHAPES = attention_ref.SHAPES
IDS = ['b%d-N%d' % s for s in SHAPES]


def _report(line):
    print(line)
    path = os.environ.get('PW_ATTN_F64_REPORT')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def _check(tag, kernel, stock, ref):
    for n in ref:
        assert n in kernel and bool(torch.isfinite(kernel[n]).all()), (tag, n)
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(kernel, stock, ref)
    _report('%-64s worst %-34s kernel %.3e  stock %.3e  ratio %.2f' % (tag, worst, e_k, e_s, ratio))
    assert ratio <= 4.0, (tag, worst, e_k, e_s, ratio)


@functools.lru_cache(maxsize=None)
def _inputs(b, N):
    return attention_ref.make_inputs(b, N, torch.float32)


# the three gradient patterns: (name, the loss autograd sees, the dOut it amounts to)
PATTERNS = (
    ('random dOut', lambda out, d: (out * d).sum(), lambda d: d),
    ('out.sum() (expanded dOut)', lambda out, d: out.sum(), lambda d: torch.ones_like(d)),
    ('only unit 5', lambda out, d: (out[:, 5] * d[:, 5]).sum(), lambda d: torch.zeros_like(d).index_copy_(1, torch.tensor([5]), d[:, 5:6])),
)


def _three(shape, relu, scale, loss, d_out):
    """{'out', 'dY'} of the kernels, of the stock float32 expression on the GPU, and of the float64 restatement, from the same numbers."""
    from multiagent_rl_amd.attention import attention_pool
    Y, dOut = _inputs(*shape)
    Y = Y * scale                                           # a power of two: exact
    Yd, dd = Y.to(DEV), dOut.to(DEV)
    kernel = attention_ref.grads(lambda y: attention_pool(y, relu), Yd, lambda o: loss(o, dd))
    stock = attention_ref.grads(lambda y: attention_ref.stock(y, relu), Yd, lambda o: loss(o, dd))
    Y64 = Y.double()
    out, w = attention_ref.forward(Y64, relu)
    ref = {'out': out, 'dY': attention_ref.backward(d_out(dOut.double()), Y64, w, out, relu)}
    return kernel, stock, ref


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_out_and_dY_against_float64(shape, relu):
    for name, loss, d_out in PATTERNS:
        _check('%s %s relu=%d' % (name, shape, relu), *_three(shape, relu, 1.0, loss, d_out))


@pytest.mark.parametrize('relu', [True, False], ids=['relu', 'linear'])
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_saturated_scores(shape, relu):
    """Y x 8: scores of the size of a thousand, so the softmax is one-hot in float32 and the other steps' exponentials underflow to
    zero.  Nothing but finite numbers, and the same bound (a one-hot softmax leaves no rounding: out is one step of Y and dY is dc
    at that step, exactly, for the kernels and for stock).  Two cases beside it, same bound: Y x 2, scores of the size of a hundred
    and weights from ~1 down to subnormal, none of them exactly 0 or 1; and Y x 0.25, scores below 2 and a flat softmax in which every
    step's weight counts (unscaled, the last step's score against itself, ~25, already leads the others by several units)."""
    name, loss, d_out = PATTERNS[0]
    _check('saturated (Y x 8) %s relu=%d' % (shape, relu), *_three(shape, relu, 8.0, loss, d_out))
    _check('peaked (Y x 2) %s relu=%d' % (shape, relu), *_three(shape, relu, 2.0, loss, d_out))
    _check('flat (Y x 0.25) %s relu=%d' % (shape, relu), *_three(shape, relu, 0.25, loss, d_out))


# ---- 2. exactness -------------------------------------------------------------------------------------------------------------------
bits = lambda t: t.view(torch.int32)   # noqa: E731


@pytest.mark.parametrize('b', [1, 5, 33])
def test_one_step_is_the_identity_bit_for_bit(b):
    """N = 1: w = 1 and ds = 0 exactly, so out = relu(Y[:, 0]) and dY = dOut [Y[:, 0] > 0] (dOut without the ReLU)."""
    from multiagent_rl_amd import attention as A
    Y, dOut = (t.to(DEV) for t in attention_ref.make_inputs(b, 1, torch.float32))
    for relu in (True, False):
        out, w = A.launch_forward(Y, relu, True)
        dY = A.launch_backward(dOut, Y, w, out, relu)
        assert torch.equal(w, torch.ones_like(w))
        want_out = torch.relu(Y[:, 0]) if relu else Y[:, 0]
        want_dY = dOut * (Y[:, 0] > 0) if relu else dOut
        assert torch.equal(out, want_out) and torch.equal(dY[:, 0], want_dY)


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3], SHAPES[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_all_negative_rows_give_zero_everywhere(shape):
    from multiagent_rl_amd import attention as A
    Y, dOut = (t.to(DEV) for t in _inputs(*shape))
    Y = -Y.abs() - 0.01
    out, w = A.launch_forward(Y, True, True)
    dY = A.launch_backward(dOut, Y, w, out, True)
    assert float(out.abs().max()) == 0.0 and float(dY.abs().max()) == 0.0


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[2], SHAPES[4], SHAPES[5]], ids=[IDS[0], IDS[2], IDS[4], IDS[5]])
def test_plumbing_is_exact(shape):
    from multiagent_rl_amd import attention as A
    Y, dOut = (t.to(DEV) for t in _inputs(*shape))
    for relu in (True, False):
        out0, none = A.launch_forward(Y, relu, False)
        out1, w1 = A.launch_forward(Y, relu, True)
        assert none is None and torch.equal(bits(out0), bits(out1))                          # saving changes nothing of out
        dY1 = A.launch_backward(dOut, Y, w1, out1, relu)
        out2, w2 = A.launch_forward(Y, relu, True)
        dY2 = A.launch_backward(dOut, Y, w2, out2, relu)
        assert torch.equal(bits(out1), bits(out2)) and torch.equal(bits(w1), bits(w2)) and torch.equal(bits(dY1), bits(dY2))   # two runs
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out3, w3 = A.launch_forward(Y, relu, True)
            dY3 = A.launch_backward(dOut, Y, w3, out3, relu)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(bits(out1), bits(out3)) and torch.equal(bits(w1), bits(w3)) and torch.equal(bits(dY1), bits(dY3))   # a second stream
        big = torch.full((Y.numel() + 7,), float('nan'), device=DEV)                        # Y one element into a larger storage
        big[1:1 + Y.numel()] = Y.reshape(-1)
        view = big[1:1 + Y.numel()].view_as(Y)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        out4, w4 = A.launch_forward(view, relu, True)
        assert torch.equal(bits(out1), bits(out4)) and torch.equal(bits(dY1), bits(A.launch_backward(dOut, view, w4, out4, relu)))


# ---- 3. the networks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_lstm', [False, True], ids=['attention', 'attention+lstm'])
@pytest.mark.parametrize('b,N', [(33, 6), (5, 13)])
def test_critic_against_float64(b, N, with_lstm):
    from multiagent_rl_amd.attention import FusedAttention, fuse_attention
    from multiagent_rl_amd.lstm import FusedLSTM, fuse_lstm
    stock = lstm_ref.make_network('critic').to(DEV)
    fused, ref = copy.deepcopy(stock), copy.deepcopy(stock).double()
    assert fuse_attention(fused) == 1 and isinstance(fused, FusedAttention)
    if with_lstm:
        assert fuse_lstm(fused) == 1 and type(fused.lstm) is FusedLSTM
    inputs = lstm_ref.network_inputs('critic', b, N, torch.float32, DEV)

    def grads(net, ins):
        ins = tuple(t.detach().clone().requires_grad_(True) for t in ins)
        out = lstm_ref.network_grads(net, ins)
        out.update({'input%d' % i: t.grad for i, t in enumerate(ins)})
        return out
    g_ref = grads(ref, tuple(t.double() for t in inputs))
    assert len(g_ref) == len(list(stock.parameters())) + 2
    _check('critic b=%d N=%d%s' % (b, N, ' + fuse_lstm' if with_lstm else ''), grads(fused, inputs), grads(stock, inputs), g_ref)


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
    """The pass in which the gradient runs through the critic's attention into the actor."""
    from multiagent_rl_amd.attention import fuse_attention
    actor, critic = lstm_ref.make_network('actor').to(DEV), lstm_ref.make_network('critic', seed=1).to(DEV)
    s0, = lstm_ref.network_inputs('actor', b, N, torch.float32, DEV)
    g = torch.Generator().manual_seed(9)
    a0 = F.one_hot(torch.randint(0, 5, (b, N), generator=g), 5).float().to(DEV)
    y = torch.randn(b, 1, generator=g).to(DEV)
    nets = {'stock': (actor, critic), 'fused': (copy.deepcopy(actor), copy.deepcopy(critic)),
            'ref': (copy.deepcopy(actor).double(), copy.deepcopy(critic).double())}
    assert fuse_attention(nets['fused'][1]) == 1 and fuse_attention(nets['fused'][0]) == 0
    grads = {k: _update_grads(a, c, (s0.to(next(a.parameters()).dtype), a0.to(next(a.parameters()).dtype)), y.to(next(a.parameters()).dtype))
             for k, (a, c) in nets.items()}
    assert float(grads['ref']['actor_loss/actor.bilstm.weight_hh_l0'].abs().max()) > 0
    _check('one update (critic loss, actor loss) b=%d N=%d' % (b, N), grads['fused'], grads['stock'], grads['ref'])


def test_the_no_gradient_critic_kernel_accepts_a_swapped_module():
    from multiagent_rl_amd.attention import fuse_attention
    from multiagent_rl_amd.critic import FusedCritic
    critic = lstm_ref.make_network('critic').to(DEV)
    obs, act = lstm_ref.network_inputs('critic', 33, 6, torch.float32, DEV)
    want = FusedCritic(critic).q(obs, act)
    assert fuse_attention(critic) == 1
    assert torch.equal(FusedCritic(critic).q(obs, act), want)


# ---- 4. the entry points ------------------------------------------------------------------------------------------------------------
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


LR = 1e-4   # as tests/test_gpu_lstm_train.py: at 1e-4 Adam's amplification of a last-bit gradient difference stays below the 1e-5 bound


@pytest.mark.parametrize('how', ['accelerate_trainer', 'fused_attention', 'targets+optimizer+lstm+attention'])
def test_trainer_entry_points(how):
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    try:
        import madr_learner
    finally:
        sys.path.pop(0)
    from multiagent_rl_amd.attention import FusedAttention
    from multiagent_rl_amd.critic import CriticNetwork, accelerate_trainer
    from multiagent_rl_amd.lstm import FusedLSTM
    from multiagent_rl_amd.policy import ActorNetwork
    trainers = []
    for switch in (False, True):
        torch.manual_seed(11)
        trainers.append(madr_learner.Trainer(ActorNetwork(10, 5), CriticNetwork(15, 1), _OneBatch(), batch_size=64, lr=LR,
                                             fused_attention=switch and how == 'fused_attention'))
    plain, fused = trainers
    if how == 'accelerate_trainer':
        accelerate_trainer(fused, seed=3, attention=True)
    elif how != 'fused_attention':
        accelerate_trainer(fused, seed=3, targets=True, optimizer=True, lstm=True, attention=True)
    assert type(plain.critic) is CriticNetwork and type(plain.target_critic) is CriticNetwork
    assert isinstance(fused.critic, FusedAttention) and isinstance(fused.critic, CriticNetwork)
    if how == 'targets+optimizer+lstm+attention':
        assert not isinstance(fused.target_critic, nn.Module) and type(fused.target_critic.module) is CriticNetwork   # the no-gradient kernel's
        assert type(fused.critic.lstm) is FusedLSTM and type(fused.actor.bilstm) is FusedLSTM
    else:
        assert type(fused.target_critic) is type(fused.critic) and type(fused.critic.lstm) is nn.LSTM
    g = torch.Generator().manual_seed(6)
    for it in range(3):
        plain.memory.batch = fused.memory.batch = _batch(g)
        torch.manual_seed(200 + it)
        lp = plain.optimize()
        torch.manual_seed(200 + it)
        lf = fused.optimize()
        assert all(x == x and abs(x) != float('inf') for x in lp + lf), (lp, lf)
        if it == 0:
            _report('%-34s first optimize(): loss_actor %.8f / %.8f  loss_critic %.8f / %.8f (unpatched / switched)' % (
                how, lp[0], lf[0], lp[1], lf[1]))
            for a, c in zip(lp, lf):
                assert abs(a - c) <= 1e-5 * max(1.0, abs(a)), (how, lp, lf)
