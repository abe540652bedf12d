"""CPU: the host side of pw_gumbel_st_forward / pw_gumbel_st_backward and of multiagent_rl_amd.sampling (no launch happens without a
GPU: every call into the library here is refused before one), the float64 restatement tests/sampling_ref.py against float64 autograd of
F.gumbel_softmax's own lines, and the Python plumbing (autograd function, GumbelSampler, the switches) with the launches replaced by
that restatement.

Bound.  Restatement in float64 against autograd in float64: 1e-12 (the same mathematics; sums of at most 16 numbers below 1)."""
import inspect
import os
import re
import sys
import types

import pytest

from multiagent_rl_amd import _lib
from tests import sampling_ref

torch = pytest.importorskip('torch')
nn = torch.nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _examples():
    if os.path.join(ROOT, 'examples') not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import madr_learner
    import train_batched
    return madr_learner, train_batched


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hard', [True, False], ids=['hard', 'soft'])
@pytest.mark.parametrize('rows,n,tau', [(3, 1, 1.0), (7, 5, 1.0), (5, 16, 0.5)])
def test_restatement_equals_float64_autograd_of_the_stock_lines(rows, n, tau, hard):
    g = torch.Generator().manual_seed(rows * 100 + n)
    logits = (2 * torch.randn(rows, n, generator=g, dtype=torch.float64)).requires_grad_()
    dY = torch.randn(rows, n, generator=g, dtype=torch.float64)
    nz = sampling_ref.noise(7, 3, rows, n)
    want = sampling_ref.stock(logits, nz, tau, hard)
    (want * dY).sum().backward()
    y, soft, idx = sampling_ref.forward(logits.detach(), nz, tau, hard)
    assert float((y - want.detach()).abs().max()) <= 1e-12
    assert float((sampling_ref.backward(dY, soft, tau) - logits.grad).abs().max()) <= 1e-12
    assert torch.equal(idx.long(), want.detach().argmax(-1)) or not hard
    if hard:
        assert float((y.sum(-1) - 1).abs().max()) <= 1e-12 and float(y.max(-1).values.sub(1).abs().max()) <= 1e-12


# ---- the plumbing, with stand-ins for the launches --------------------------------------------------------------------------------
@pytest.fixture
def standins(monkeypatch):
    from multiagent_rl_amd import sampling
    calls = []

    def fwd(logits, tau, hard, seed, step, cell, keep, want_idx=False, want_noise=False):
        calls.append(('forward', int(step), keep, tuple(logits.shape)))
        return sampling_ref.launch_forward(logits, tau, hard, seed, step, cell, keep, want_idx, want_noise)

    def bwd(dY, soft, tau):
        calls.append(('backward', dY.is_contiguous()))
        return sampling_ref.launch_backward(dY, soft, tau)

    def adv(cell, delta):
        calls.append(('advance', int(delta)))
        sampling_ref.launch_advance(cell, delta)
    monkeypatch.setattr(sampling, 'launch_forward', fwd)
    monkeypatch.setattr(sampling, 'launch_backward', bwd)
    monkeypatch.setattr(sampling, 'launch_advance', adv)
    sampling.calls = calls
    yield sampling
    del sampling.calls


@pytest.mark.parametrize('hard', [True, False], ids=['hard', 'soft'])
def test_gumbel_st_function(standins, hard):
    """Gradients flow and equal autograd of the stock lines; nothing is saved without a gradient; an expanded dY arrives contiguous;
    any leading shape is flattened row-major."""
    g = torch.Generator().manual_seed(1)
    logits = 2 * torch.randn(4, 3, 5, generator=g, dtype=torch.float64)
    dY = torch.randn(4, 3, 5, generator=g, dtype=torch.float64)
    cell = torch.tensor([32])
    nz = sampling_ref.noise(9, 34, 12, 5).reshape(4, 3, 5)
    x = logits.clone().requires_grad_()
    want = sampling_ref.stock(x, nz, 0.5, hard)
    (want * dY).sum().backward()
    xs = logits.clone().requires_grad_()
    got = standins.gumbel_st(xs, tau=0.5, hard=hard, seed=9, step=2, cell=cell)
    assert got.shape == (4, 3, 5) and got.requires_grad
    (got * dY).sum().backward()
    assert float((got - want).detach().abs().max()) <= 1e-12 and float((xs.grad - x.grad).abs().max()) <= 1e-12
    assert standins.calls == [('forward', 2, True, (12, 5)), ('backward', True)]
    del standins.calls[:]
    xs.grad = None
    standins.gumbel_st(xs, seed=9).sum().backward()                       # out.sum(): an expanded zero-stride dY
    assert standins.calls == [('forward', 0, True, (12, 5)), ('backward', True)] and float(xs.grad.abs().max()) <= 1e-12
    del standins.calls[:]
    with torch.no_grad():
        out = standins.gumbel_st(xs, seed=9)
    assert not out.requires_grad and out.grad_fn is None
    assert not standins.gumbel_st(logits, seed=9).requires_grad            # an input that needs no gradient
    assert [c[2] for c in standins.calls] == [False, False]                # ... and nothing was kept for a backward


def test_refusals_name_the_reason():
    from multiagent_rl_amd import sampling
    with pytest.raises(RuntimeError, match='no CPU fallback'):             # the real launch functions are in place
        sampling.gumbel_st(torch.zeros(2, 3, 5))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        sampling.launch_backward(torch.zeros(2, 5), torch.zeros(2, 5), 1.0)
    with pytest.raises(ValueError, match='1 to 16 logits'):
        sampling.gumbel_st(torch.zeros(2, 17))
    with pytest.raises(ValueError, match='1 to 16 logits'):
        sampling.gumbel_st(torch.zeros(2, 0))
    with pytest.raises(ValueError, match='tau'):
        sampling.gumbel_st(torch.zeros(2, 5), tau=0.0)
    with pytest.raises(ValueError, match='scalar'):
        sampling.gumbel_st(torch.zeros(()))
    with pytest.raises(ValueError, match='at least one row'):
        sampling.gumbel_st(torch.zeros(0, 5))
    assert sampling.default_seed(0) == sampling.LEARNER_STREAM and sampling.default_seed(5) != 5
    assert sampling.default_seed(2 ** 64 - 1) == sampling.LEARNER_STREAM - 1       # mod 2^64


def test_sampler_numbers_the_sites_of_an_update(standins):
    s = standins.GumbelSampler(seed=3, device='cpu')
    assert s.cell.dtype == torch.int64 and int(s.cell) == 0 and standins.SITES_PER_UPDATE == 16
    x = torch.randn(6, 2, 5, dtype=torch.float64)
    a = s.sample(x)
    b = s.sample([x, x[..., :3]])                                        # two heads: one site each, concatenated
    c = s.gumbel_softmax(x, hard=False)
    i = s.sample_index(x)
    assert a.shape == (6, 2, 5) and b.shape == (6, 2, 8) and i.shape == (6, 2) and i.dtype == torch.int32
    assert [k[1] for k in standins.calls] == [0, 1, 2, 3, 4]
    assert torch.equal(b[..., :5].argmax(-1), sampling_ref.forward(x.reshape(12, 5), sampling_ref.noise(3, 1, 12, 5), 1.0, True)[2].long().reshape(6, 2))
    assert float((c.sum(-1) - 1).abs().max()) <= 1e-12 and float(c.max()) < 1.0
    assert torch.equal(i.long(), sampling_ref.forward(x.reshape(12, 5), sampling_ref.noise(3, 4, 12, 5), 1.0, True)[2].long().reshape(6, 2))
    s.end_update()
    assert standins.calls[-1] == ('advance', 16) and int(s.cell) == 16 and s.site == 0 and s.updates == 1
    del standins.calls[:]
    a2 = s.sample(x)
    assert standins.calls == [('forward', 0, False, (12, 5))]             # the ordinal restarts; the cell carries the update
    assert not torch.equal(a, a2)
    assert torch.equal(a2, sampling_ref.forward(x.reshape(12, 5), sampling_ref.noise(3, 16, 12, 5), 1.0, True)[0].reshape(6, 2, 5))
    for _ in range(15):
        s.sample(x)
    with pytest.raises(ValueError, match='more than 16'):                  # the 17th site would be the next update's first
        s.sample(x)
    s.reset(0)
    assert int(s.cell) == 0 and torch.equal(s.sample(x), a)               # the same (seed, cell, site): the same sample
    with pytest.raises(ValueError, match=r'\[n, t, A\]'):
        s.gumbel_softmax(x[0])
    assert standins.GumbelSampler(device='cpu').seed == standins.default_seed(0)
    assert standins.GumbelSampler(device='cpu', exploration_seed=4).seed == standins.default_seed(4)


class _Shape(object):
    def __init__(self):
        self.actor, self.device, self.action_type = nn.Linear(4, 5), torch.device('cpu'), 'Discrete'


class _ReferenceShape(_Shape):
    """The reference Trainer's surface as far as the switch touches it: a gumbel_softmax method used twice per optimize()."""

    def gumbel_softmax(self, x, hard=True):
        return 'stock'

    def optimize(self):
        x = torch.zeros(2, 3, 5, dtype=torch.float64)
        return self.gumbel_softmax(x), self.gumbel_softmax(x)


class _ExampleShape(_Shape):
    """The example learner's: a static _sample that also takes a list of heads."""

    @staticmethod
    def _sample(logits):
        return 'stock'

    def optimize(self):
        x = torch.zeros(2, 3, 5, dtype=torch.float64)
        return self._sample(x), self._sample([x, x])


@pytest.fixture
def no_gpu_exploration(monkeypatch):
    from multiagent_rl_amd import policy
    monkeypatch.setattr(policy, 'FusedExploration', lambda actor, action_type, seed=0: types.SimpleNamespace(
        get_exploration_action=None, refresh=lambda: None))
    return policy


def test_accelerate_trainer_installs_the_sampler_on_either_surface(standins, no_gpu_exploration):
    accelerate_trainer = no_gpu_exploration.accelerate_trainer
    sig = inspect.signature(accelerate_trainer).parameters
    assert sig['sampling'].default is False and sig['sampling_seed'].default is None
    for cls in (_ReferenceShape, _ExampleShape):                           # the default leaves both alone
        t = cls()
        accelerate_trainer(t)
        assert 'gumbel_softmax' not in vars(t) and '_sample' not in vars(t) and t.optimize()[0] == 'stock'
        assert not hasattr(t._pw_accel, 'sampler')
    assert standins.calls == []
    t = _ReferenceShape()
    fx = accelerate_trainer(t, seed=11, sampling=True)
    assert isinstance(fx.sampler, standins.GumbelSampler) and fx.sampler.seed == standins.default_seed(11)
    assert t.gumbel_softmax == fx.sampler.gumbel_softmax and '_sample' not in vars(t)
    a, b = t.optimize()
    assert a.shape == (2, 3, 5) and not torch.equal(a, b)                  # two sites: other noise on equal logits
    assert [c[:2] for c in standins.calls] == [('forward', 0), ('forward', 1), ('advance', 16)]
    assert int(fx.sampler.cell) == 16 and fx.sampler.site == 0
    t.optimize()
    assert int(fx.sampler.cell) == 32
    del standins.calls[:]
    t = _ExampleShape()
    fx = accelerate_trainer(t, sampling=True, sampling_seed=99)
    assert fx.sampler.seed == 99 and t._sample == fx.sampler.sample and 'gumbel_softmax' not in vars(t)
    a, b = t.optimize()
    assert a.shape == (2, 3, 5) and b.shape == (2, 3, 10)
    assert [c[:2] for c in standins.calls] == [('forward', 0), ('forward', 1), ('forward', 2), ('advance', 16)]
    bare = types.SimpleNamespace(actor=nn.Linear(4, 5), optimize=lambda: None)
    with pytest.raises(ValueError, match='neither'):
        accelerate_trainer(bare, sampling=True)


class _Ring(object):
    device_index = True

    def __len__(self):
        return 64

    def make_index(self, b):
        return torch.arange(b)

    def sample_index(self, idx):
        g = torch.Generator().manual_seed(2)
        b = len(idx)
        return (torch.randn(b, 3, 10, generator=g), torch.eye(5)[torch.randint(0, 5, (b, 3), generator=g)], torch.randn(b, generator=g),
                torch.randn(b, 3, 10, generator=g), torch.zeros(b))


def test_example_learner_switch_is_an_instance_attribute_and_off_by_default(standins, no_gpu_exploration):
    madr_learner, train_batched = _examples()
    from multiagent_rl_amd.policy import ActorNetwork
    sig = inspect.signature(madr_learner.Trainer.__init__).parameters
    assert sig['fused_sampling'].default is False and sig['sampling_seed'].default is None
    make = lambda cls, **k: cls(ActorNetwork(10, 5), madr_learner.CriticNetwork(15), _Ring(), batch_size=8, device='cpu', **k)  # noqa: E731
    plain = make(madr_learner.Trainer)
    assert plain.sampler is None and '_sample' not in vars(plain)
    t = make(madr_learner.Trainer, fused_sampling=True, sampling_seed=5)
    assert isinstance(t.sampler, standins.GumbelSampler) and t.sampler.seed == 5 and vars(t)['_sample'] == t.sampler.sample
    assert '_sample' in vars(madr_learner.Trainer) and madr_learner.Trainer._sample is not t._sample     # the class keeps the stock one

    class Own(madr_learner.Trainer):
        _sample = staticmethod(lambda logits: torch.softmax(logits, -1))
    own = make(Own)
    assert own.sampler is None and own._sample is Own._sample
    own.optimize()
    assert standins.calls == []
    t.optimize()                                                           # one whole update through the stand-ins
    kinds = [c[0] for c in standins.calls]
    assert kinds == ['forward', 'forward', 'backward', 'advance']
    assert [c[1:3] for c in standins.calls[:2]] == [(0, False), (1, True)]   # site 0 under no_grad keeps nothing; site 1 is the actor loss
    assert int(t.sampler.cell) == 16 and t.sampler.site == 0
    fx = no_gpu_exploration.accelerate_trainer(t, sampling=True)           # the learner's own sampler counts: kept, and not closed twice
    assert fx.sampler is t.sampler and fx.owned_sampler is None
    t.optimize()
    assert int(t.sampler.cell) == 32
    with pytest.raises(SystemExit):                                        # the flag exists; an unknown one is refused by the same parser
        train_batched.main(['--fused-sampling', '--no-such-flag'])
    assert '--fused-sampling' in inspect.getsource(train_batched.main)


def test_graphed_update_closes_the_update_inside_the_region():
    """GraphedUpdate._update: body, then the sampler's end_update, then the in-place refresh -- all inside what gets captured."""
    from multiagent_rl_amd.graph import GraphedUpdate
    order = []
    g = GraphedUpdate.__new__(GraphedUpdate)
    g._body = lambda: order.append('body') or ('la', 'lc')
    g._sampler = types.SimpleNamespace(end_update=lambda: order.append('end_update'))
    g._target_actor = types.SimpleNamespace(refresh=lambda in_place: order.append('refresh in place %r' % in_place))
    assert g._update() == ('la', 'lc') and order == ['body', 'end_update', 'refresh in place True']
    g._sampler, order[:] = None, []
    g._update()
    assert order == ['body', 'refresh in place True']


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
P = [4096 + 1024 * k for k in range(7)]    # fake, aligned "device pointers": every call below is refused before a launch


def _fwd(logits=P[0], rows=8, n=5, tau=1.0, hard=1, seed=7, step=0, step_dev=None, y=P[1], soft=P[2], idx=P[3], noise=P[4]):
    return _lib.load().pw_gumbel_st_forward(logits, rows, n, tau, hard, seed, step, step_dev, y, soft, idx, noise, None)


def _bwd(dY=P[5], soft=P[2], rows=8, n=5, tau=1.0, dLogits=P[6]):
    return _lib.load().pw_gumbel_st_backward(dY, soft, rows, n, tau, dLogits, None)


def test_symbols_are_exported_and_declared():
    lib = _lib.load()
    header = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    for name in ('pw_gumbel_st_forward', 'pw_gumbel_st_backward'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r'\bint %s\(' % name, header)
    assert lib.pw_version() >= 117


@pytest.mark.parametrize('call', [_fwd, _bwd], ids=['forward', 'backward'])
@pytest.mark.parametrize('kw,word', [
    (dict(n=0), b'n must be in 1 .. 16'), (dict(n=-3), b'n must'), (dict(n=17), b'n must'), (dict(n=1 << 20), b'n must'),
    (dict(tau=0.0), b'tau must'), (dict(tau=-1.0), b'tau must'), (dict(tau=float('nan')), b'tau must'), (dict(tau=float('inf')), b'tau must'),
    (dict(rows=0), b'rows must'), (dict(rows=-4), b'rows must'), (dict(rows=1 << 40), b'rows:'),
    (dict(soft=P[2] + 2), b'soft must be 4-byte aligned'),
], ids=lambda v: str(v) if isinstance(v, dict) else '')
def test_both_entry_points_refuse_bad_shared_arguments(call, kw, word):
    assert call(**kw) == EINVAL
    assert word in _lib.load().pw_last_error(), _lib.load().pw_last_error()


def test_each_entry_point_refuses_its_bad_buffers():
    lib = _lib.load()
    for name in ('logits', 'y'):
        assert _fwd(**{name: None}) == EINVAL and name.encode() + b' is null' in lib.pw_last_error()
    for k, name in enumerate(('logits', 'y', 'idx', 'noise')):
        assert _fwd(**{name: P[k] + 1}) == EINVAL and name.encode() + b' must be 4-byte aligned' in lib.pw_last_error()
    assert _fwd(step_dev=P[5] + 4) == EINVAL and b'step_dev must be 8-byte aligned' in lib.pw_last_error()
    for name in ('dY', 'soft', 'dLogits'):
        assert _bwd(**{name: None}) == EINVAL and name.encode() + b' is null' in lib.pw_last_error()
    for name in ('dY', 'dLogits'):
        assert _bwd(**{name: P[5] + 2}) == EINVAL and name.encode() + b' must be 4-byte aligned' in lib.pw_last_error()


# ---- what the compiler made of the new unit ---------------------------------------------------------------------------------------
def test_sample_unit_carries_exactly_its_own_kernels():
    """Mirrors test_attention_unit_carries_exactly_its_own_kernels: the unit includes pw_common.hpp for its device functions and must
    not pick up a kernel with it; the two kernels are templates on ceil(n / 4) = 1 .. 4."""
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import code_object
    finally:
        sys.path.pop(0)
    if not code_object.tools_present():
        pytest.skip('ROCm LLVM binary tools not installed')
    from multiagent_rl_amd import build_native
    if not all(os.path.exists(o) for o in build_native.objects()):
        build_native.build(force=True)
    src = open(os.path.join(ROOT, 'multiagent_rl_amd', 'csrc', 'pw_kernels_sample.hpp')).read()
    defined = set(re.findall(r'__global__ void (?:__launch_bounds__\(\w+\) )?(pw_\w+_kernel)\(', src))
    assert defined == {'pw_gumbel_st_forward_kernel', 'pw_gumbel_st_backward_kernel'}
    names = code_object.per_unit_kernels()['pworld_sample']
    assert {re.match(r'(?:void )?(\w+)', n).group(1) for n in names} == defined
    assert sorted(re.match(r'(?:void )?(\w+<\d>)', n).group(1) for n in names) == sorted(
        '%s<%d>' % (k, nb) for k in defined for nb in (1, 2, 3, 4))
    assert os.path.join(build_native.HERE, 'csrc', 'pworld_sample.hip') in build_native.SRCS
    assert 'pworld_sample' in build_native.unit_sources.__doc__
    unit = [os.path.basename(f) for f in build_native.unit_sources('pworld_sample')]
    assert 'pw_kernels_sample.hpp' in unit
    families = {os.path.basename(f) for fam in build_native.KERNEL_FAMILIES.values() for f in fam}
    assert not (set(unit) & families) - {'pw_common.hpp', 'pw_params.hpp', 'pworld_math.h'}   # no kernel header of the env / actor families
