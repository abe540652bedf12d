"""CPU: what the captured update (multiagent_rl_amd/graph.py) rests on, as far as it can be checked without a GPU -- the batch draw of
pw_replay_sample and Adam's step-dependent scalars of pw_adam_step_dev against Python restatements, the refusals of the two entry points
(each before a launch), the refusals of GraphedUpdate / accelerate_trainer(graph=True), and the control flow of the entry path."""
import ctypes as C
import math
import os
import struct
import sys
import types

import numpy as np
import pytest
import torch

from multiagent_rl_amd import _lib
from oracle import actor_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

EINVAL = -1
TAG = 0x52504C59
M32 = 0xFFFFFFFF


@pytest.fixture(scope='module')
def lib():
    lib = _lib.load()
    global EINVAL
    assert lib.pw_replay_sample(None, 0, None, None, 1, None, None, None, None, None, None, None) != 0
    EINVAL = lib.pw_replay_sample(None, 0, None, None, 1, None, None, None, None, None, None, None)
    return lib


# ---- the draw rule ---------------------------------------------------------------------------------------------------------------
def draw_restated(seed, call, n, length):
    """Elements 0 .. n-1 of draw number `call`: word (e & 3) of Philox4x32-10(counter = (e >> 2, call lo, call hi, TAG), key = seed),
    scaled to [0, length) by the upper half of the 64-bit product."""
    e = np.arange(n, dtype=np.uint64)
    u = lambda v: np.full(n, v, dtype=np.uint64)  # noqa: E731
    w = ao.philox4x32_10(e >> np.uint64(2), u(call & M32), u((call >> 32) & M32), u(TAG), u(seed & M32), u((seed >> 32) & M32))
    word = np.choose((e & np.uint64(3)).astype(np.int64), [np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in w])
    return ((word * np.uint64(length)) >> np.uint64(32)).astype(np.int64)


@pytest.mark.parametrize('seed', [0, 12345678, 2 ** 63 + 5])
@pytest.mark.parametrize('call', [0, 1, 2 ** 32 + 7])
def test_draw_equals_the_restatement_over_the_oracles_philox(lib, seed, call):
    for length in (1, 2, 3, 64, 10 ** 6, 2 ** 20):
        got = np.array([lib.pw_replay_draw_host(seed, call, e, length) for e in range(1024)], dtype=np.int64)
        assert np.array_equal(got, draw_restated(seed, call, 1024, length)), (seed, call, length)
        assert got.min() >= 0 and got.max() < length
        if length == 1:
            assert not got.any()


def test_draw_clamps_the_length_and_is_uniform(lib):
    assert lib.pw_replay_draw_host(7, 3, 5, 0) == 0 and lib.pw_replay_draw_host(7, 3, 5, -9) == 0       # a length below 1 counts as 1
    seed, n = 12345678, 65536
    got = np.concatenate([draw_restated(seed, call, 1024, 64) for call in range(n // 1024)])           # 64 draws of a 1024-batch
    assert all(lib.pw_replay_draw_host(seed, 5, e, 64) == draw_restated(seed, 5, 1024, 64)[e] for e in range(0, 1024, 37))
    counts = np.bincount(got, minlength=64)
    chi2 = float(((counts - n / 64.0) ** 2 / (n / 64.0)).sum())
    assert chi2 < 103.4424, chi2          # the 99.9 % quantile of chi-square with 63 degrees of freedom; deterministic for this seed


# ---- Adam's bias scalars ---------------------------------------------------------------------------------------------------------
def f32(x):
    return struct.unpack('f', struct.pack('f', x))[0]


def pow_sqm(x, t):
    r = 1.0
    while t:
        if t & 1:
            r *= x
        x *= x
        t >>= 1
    return r


def scalars(lib, step, lr, b1, b2):
    out = (C.c_float * 2)()
    lib.pw_adam_bias_scalars(step, lr, b1, b2, out)
    return out[0], out[1]


SETTINGS = [(0.9, 0.999, 1e-2), (0.9, 0.999, 1e-3), (0.8, 0.99, 3e-4)]


@pytest.mark.parametrize('b1,b2,lr', SETTINGS)
def test_bias_scalars_equal_square_and_multiply_and_libm_pow(lib, b1, b2, lr):
    for t in range(1, 20001):
        got = scalars(lib, t, lr, b1, b2)
        assert got == (f32(math.sqrt(1.0 - pow_sqm(b2, t))), f32(lr / (1.0 - pow_sqm(b1, t)))), t
        # the host path of pw_adam_step: std::pow -- the same float32 numbers at every step, so the two kernels can be held to bit-identity
        assert got == (f32(math.sqrt(1.0 - math.pow(b2, t))), f32(lr / (1.0 - math.pow(b1, t)))), t


def test_bias_scalars_beyond_the_walked_range_and_below_step_one(lib):
    for t in (20001, 10 ** 6 + 3, 2 ** 40 + 1, 2 ** 62):
        assert scalars(lib, t, 1e-3, 0.9, 0.999) == (f32(math.sqrt(1.0 - pow_sqm(0.999, t))), f32(1e-3 / (1.0 - pow_sqm(0.9, t))))
    one = scalars(lib, 1, 1e-2, 0.9, 0.999)
    assert scalars(lib, 0, 1e-2, 0.9, 0.999) == one and scalars(lib, -5, 1e-2, 0.9, 0.999) == one


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_version_and_symbols(lib):
    assert lib.pw_version() >= 116
    hdr = open(os.path.join(ROOT, 'include', 'pworld.h')).read()
    for name in ('pw_replay_sample', 'pw_replay_draw_host', 'pw_adam_step_dev', 'pw_adam_bias_scalars'):
        assert name in _lib.SIGNATURES and (name + '(') in hdr, name


def _store(capacity=256):
    st = _lib.PwReplayStore()
    st.obs = st.next_obs = st.rew = st.done = st.act = 0x1000     # fake pointers: every call below is refused before a launch
    st.capacity, st.num_agents, st.obs_dim, st.act_heads = capacity, 3, 10, 1
    return st


def test_replay_sample_refusals_name_the_argument(lib):
    p = C.c_void_p(0x1000)

    def call(st=_store(), call_dev=p, len_dev=p, b=8, idx=p, obs=p):
        return lib.pw_replay_sample(None if st is None else C.byref(st), 1, call_dev, len_dev, b, idx, obs, None, None, None, None, None)
    for kw, word in ((dict(st=None), b'st is null'), (dict(call_dev=None), b'call_dev'), (dict(len_dev=None), b'len_dev'),
                     (dict(b=0), b'b must be'), (dict(b=-3), b'b must be'), (dict(idx=None, obs=None), b'out_idx'),
                     (dict(st=_store(2 ** 32 + 1)), b'capacity'), (dict(st=_store(0)), b'capacity'),
                     (dict(call_dev=C.c_void_p(0x1004)), b'aligned')):
        assert call(**kw) == EINVAL and word in lib.pw_last_error(), (kw, lib.pw_last_error())


def test_adam_step_dev_refusals_name_the_argument(lib):
    rows = [(0x1000, 0x2000, 0x3000, 0x4000, None, 64) for _ in range(3)]
    table = (_lib.PwOptTensor * 3)(*rows)
    p = C.c_void_p(0x1000)

    def call(table=table, count=3, step_dev=p, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, max_norm=0.5, tau=0.01):
        return lib.pw_adam_step_dev(table, count, step_dev, lr, b1, b2, eps, wd, max_norm, tau, None, None)
    for kw, word in ((dict(table=None), b'tensors'), (dict(step_dev=None), b'step_dev'), (dict(step_dev=C.c_void_p(0x1004)), b'step_dev'),
                     (dict(count=0), b'count'), (dict(count=33), b'count'), (dict(lr=-1.0), b'lr'), (dict(lr=float('nan')), b'lr'),
                     (dict(b1=1.0), b'beta'), (dict(b2=-0.1), b'beta'), (dict(eps=-1e-8), b'eps'), (dict(wd=-1.0), b'weight_decay'),
                     (dict(max_norm=float('nan')), b'max_norm')):
        assert call(**kw) == EINVAL and word in lib.pw_last_error(), (kw, lib.pw_last_error())
    bad = (_lib.PwOptTensor * 1)((0x1000, None, 0x3000, 0x4000, None, 64))
    assert call(table=bad, count=1) == EINVAL and b'grad' in lib.pw_last_error()
    tgt = (_lib.PwOptTensor * 1)((0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 64))
    assert call(table=tgt, count=1, tau=1.5) == EINVAL and b'tau' in lib.pw_last_error()


# ---- what GraphedUpdate refuses --------------------------------------------------------------------------------------------------
class _CounterRing(object):
    device_index = 'counter'

    def __init__(self, n=4096):
        self.n = n

    def __len__(self):
        return self.n


def _served_trainer(critic='attention', memory=None):
    """The example learner on the CPU with the three constructor switches on and the rest of the served configuration put on by hand
    (the HIP target wrappers need a GPU; their presence is what the checks read)."""
    import madr_learner
    from multiagent_rl_amd.critic import BiCNetCritic, CriticNetwork, _FusedTarget
    from multiagent_rl_amd.policy import ActorNetwork
    net = CriticNetwork(15) if critic == 'attention' else BiCNetCritic(15)
    cls = madr_learner.Trainer if critic == 'attention' else madr_learner.BiCNetTrainer
    t = cls(ActorNetwork(10, 5), net, _CounterRing() if memory is None else memory, batch_size=32, device='cpu', fused_optimizer=True,
            fused_lstm=True, fused_attention=True)
    for opt in (t.actor_optimizer, t.critic_optimizer):
        opt.graph_steps = True
    t.target_actor, t.target_critic = _FusedTarget(t.target_actor, lambda obs: None), _FusedTarget(t.target_critic, lambda o, a: None)
    t._pw_accel = types.SimpleNamespace(target_actor=object(), inner_optimize=t.optimize, refresh=lambda: None)
    return t


@pytest.mark.parametrize('critic', ['attention', 'bicnet'])
def test_the_served_configuration_is_accepted(critic):
    from multiagent_rl_amd.graph import GraphedUpdate, missing_for_graph
    t = _served_trainer(critic)
    assert missing_for_graph(t) == []
    g = GraphedUpdate(t, warmup=2)
    assert (g.warmup, g.replays, g.graph) == (2, 0, None)


def test_each_missing_piece_is_refused_by_name():
    from multiagent_rl_amd.attention import unfuse_attention
    from multiagent_rl_amd.graph import GraphedUpdate
    from multiagent_rl_amd.lstm import unfuse_lstm

    def refused(t, word):
        with pytest.raises(ValueError) as e:
            GraphedUpdate(t)
        assert word in str(e.value), str(e.value)
    t = _served_trainer()
    t.target_actor = t.target_actor.module
    refused(t, 'targets')
    t = _served_trainer()
    del t._pw_accel
    refused(t, 'targets')
    t = _served_trainer()
    t.critic_optimizer = torch.optim.Adam(t.critic.parameters())
    refused(t, 'optimizer: critic_optimizer is Adam')
    t = _served_trainer()
    t.actor_optimizer.graph_steps = False
    refused(t, 'graph_steps')
    t = _served_trainer()
    unfuse_lstm(t.actor)
    refused(t, 'lstm: actor')
    t = _served_trainer()
    unfuse_lstm(t.critic)
    refused(t, 'lstm: critic')
    t = _served_trainer()
    unfuse_attention(t.critic)
    refused(t, 'attention')
    t = _served_trainer('bicnet')          # no attention block: nothing to miss there, but the rest still counts
    unfuse_lstm(t.critic)
    refused(t, 'lstm: critic')
    for mode in (False, True):
        ring = _CounterRing()
        ring.device_index = mode
        refused(_served_trainer(memory=ring), "device_index='counter'")
    refused(_served_trainer(memory=[0] * 64), 'memory')
    # a ring that is too short is refused when an update is asked for, not at construction (train_batched builds the learner first)
    g = GraphedUpdate(_served_trainer(memory=_CounterRing(31)))
    with pytest.raises(ValueError, match='31 transitions, an update draws 32'):
        g()


def test_accelerate_trainer_graph_refuses_without_the_switches(monkeypatch):
    import inspect
    import madr_learner
    from multiagent_rl_amd import policy
    from multiagent_rl_amd.critic import CriticNetwork
    sig = inspect.signature(policy.accelerate_trainer).parameters
    assert sig['graph'].default is False and sig['graph_warmup'].default == 3
    monkeypatch.setattr(policy, 'FusedExploration', lambda actor, action_type, seed=0: types.SimpleNamespace(
        get_exploration_action=None, refresh=lambda: None))
    t = madr_learner.Trainer(policy.ActorNetwork(10, 5), CriticNetwork(15), _CounterRing(), batch_size=32, device='cpu')
    before = t.optimize
    with pytest.raises(ValueError) as e:
        policy.accelerate_trainer(t, graph=True)
    for word in ('targets', 'optimizer: actor_optimizer is Adam', 'optimizer: critic_optimizer is Adam', 'lstm: actor, critic', 'attention'):
        assert word in str(e.value), str(e.value)
    assert t.optimize == before            # nothing installed
    with pytest.raises(ValueError, match='critic_optimizer is Adam'):     # the constructor switch of the example learner says the same
        madr_learner.Trainer(policy.ActorNetwork(10, 5), CriticNetwork(15), _CounterRing(), batch_size=32, device='cpu', graph_update=True)
    with pytest.raises(ValueError, match="device_index='counter'"):
        madr_learner.Trainer(policy.ActorNetwork(10, 5), CriticNetwork(15), [0] * 64, batch_size=32, device='cpu', fused_optimizer=True,
                             fused_lstm=True, fused_attention=True, graph_update=True)


def test_replay_buffer_modes_and_fused_adam_bookkeeping():
    from multiagent_rl_amd.optim import FusedAdam
    from multiagent_rl_amd.replay_buffer import ReplayBuffer
    rb = ReplayBuffer(256, device_index='counter', index_seed=2 ** 64 + 9)
    assert rb.device_index == 'counter' and rb.index_seed == 9 and len(rb) == 0
    assert ReplayBuffer(256, device_index=True).device_index is True and ReplayBuffer(256).device_index is False
    with pytest.raises(ValueError):
        ReplayBuffer(2 ** 32 + 1, device_index='counter')
    with pytest.raises(ValueError):
        ReplayBuffer(256, device_index='device')
    with pytest.raises(ValueError, match='empty'):
        rb.make_index(4)
    st = rb.__getstate__()
    assert st['device_index'] == 'counter' and st['index_seed'] == 9 and st['draws'] == 0
    rb2 = ReplayBuffer.__new__(ReplayBuffer)
    rb2.__setstate__(dict(st, len=7, draws=12))
    assert rb2.device_index == 'counter' and len(rb2) == 7 and rb2._draws0 == 12
    # note_graph_steps: the host-side step of every parameter with state, and a state_dict that still loads into torch's Adam
    ps = [torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(3, 2))]
    opt = FusedAdam(ps, lr=1e-2, graph_steps=True)
    assert opt.graph_steps
    for p in ps:
        opt.state[p] = dict(step=torch.tensor(4.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
    opt.note_graph_steps(3)
    assert [float(opt.state[p]['step']) for p in ps] == [7.0, 7.0]
    ref = torch.optim.Adam(ps, lr=1e-2)
    ref.load_state_dict(opt.state_dict())
    assert [float(ref.state[p]['step']) for p in ps] == [7.0, 7.0]
    back = FusedAdam(ps, lr=1e-2, graph_steps=True)
    back.load_state_dict(ref.state_dict())
    assert float(back.state[ps[0]]['step']) == 7.0


# ---- the entry path --------------------------------------------------------------------------------------------------------------
def test_entry_script_refuses_graph_update_without_the_fused_flags(capsys):
    import train_batched as entry
    for flags in ([], ['--fused-targets', '--fused-optimizer', '--fused-lstm'], ['--fused-optimizer', '--fused-lstm', '--fused-attention']):
        with pytest.raises(SystemExit):
            entry.main(['--critic', 'attention', '--graph-update'] + flags)
        assert '--graph-update needs' in capsys.readouterr().err
    with pytest.raises(SystemExit):     # bicnet has no attention block: the first three are what it needs
        entry.main(['--critic', 'bicnet', '--graph-update', '--fused-targets', '--fused-lstm'])
    assert '--fused-optimizer' in capsys.readouterr().err


def test_train_batched_graph_update_passes_through_with_a_stub_learner():
    from multiagent_rl_amd.graph import GraphedUpdate
    from multiagent_rl_amd.train import train_batched
    from tests import test_train_entry as te

    class StubGraphed(GraphedUpdate):
        def __init__(self, trace, memory):
            self.trace, self.memory, self.replays = trace, memory, 0

        def __call__(self):
            self.replays += 1
            self.trace.append(('optimize', len(self.memory)))

    class Learner(te._StubTrainer):
        def __init__(self, actor, critic, memory, action_type='Discrete'):
            super().__init__(actor, critic, memory, action_type)
            self.optimize = StubGraphed(self.trace, memory)

    trace = []
    te._StubTrainer.trace = trace
    env, cfg = te._StubEnv(), te._Args()
    make = lambda e, actor, memory, seed: (te._StubFused(trace), te._StubRollout(e, memory, trace))  # noqa: E731
    hist = train_batched(env, 'actor', 'critic', Learner, 'simple_spread', 'Discrete', arglist=cfg, memory=te._StubMemory(), out_dir=None,
                         log=lambda *a: None, chunk=10, make_rollout=make, graph_update=True)
    st = hist['stats']
    assert st['updates_run'] == 6 and st['graph_replays'] == 6 and [e[0] for e in trace].count('optimize') == 6
    plain = train_batched(env, 'actor', 'critic', te._StubTrainer, 'simple_spread', 'Discrete', arglist=cfg, memory=te._StubMemory(),
                          out_dir=None, log=lambda *a: None, chunk=10, make_rollout=make)
    assert plain['stats']['graph_replays'] == 0
    with pytest.raises(ValueError, match='accelerate_trainer'):     # a learner nothing has prepared is refused, not silently run eagerly
        train_batched(env, 'actor', 'critic', te._StubTrainer, 'simple_spread', 'Discrete', arglist=cfg, memory=te._StubMemory(),
                      out_dir=None, log=lambda *a: None, chunk=10, make_rollout=make, graph_update=True)
