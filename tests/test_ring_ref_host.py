"""No GPU: the NumPy ring model of tests/ring_ref.py, the inputs the GPU ring tests run on, and the host refusals of the ring's base layer.

(a) The model is anchored to the reference: tests/golden/replay_buffer.json (written by the reference's own ReplayBuffer) replayed
    through ``RingModel.add`` gives the stored rewards, ``len``, ``_next_idx`` and the encoded batch of the reference.
(b) The inputs discriminate: on every shape and ring kind tests/test_gpu_replay_ring.py uses, each of eight deliberately wrong models
    gives other planes (or other gather outputs) than the true one.  A kernel with one of these mistakes therefore fails there.
(c) Every refusal of pw_replay_add / _tail / _rollout / _packed, pw_replay_gather, pw_replay_sample, pw_pack_transitions and pw_exchange
    is PW_EINVAL with its message, on fake aligned pointers: nothing launches.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from multiagent_rl_amd import _lib
from tests import ring_ref as rr
from tests.ring_ref import RingModel

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'replay_buffer.json')


# ---- (a) the anchor -------------------------------------------------------------------------------------------------------------
def test_the_model_replays_the_references_own_ring():
    g = json.load(open(GOLD))
    cap = g['size']
    first = g['transitions'][0]
    N, D = np.asarray(first['obs']).shape
    m = RingModel(np.zeros((cap, N, D)), np.zeros((cap, N, D)), np.zeros((cap, N)), np.zeros(cap), np.zeros(cap))
    for tr in g['transitions']:                     # ReplayBuffer.add(): one transition at the cursor
        f32 = lambda k: np.asarray(tr[k], np.float32)[None]
        m.add(m.next_idx, f32('obs'), np.argmax(np.asarray(tr['act']), -1)[None], f32('rew'), f32('next_obs'), done=f32('done'))
    assert m.len == g['len'] and m.next_idx == g['next_idx']
    assert rr.same(m.rew, np.asarray(g['storage_rewards'], np.float32))                     # the ring's overwrite order
    got = m.gather(g['make_index_seed0'])
    assert [list(a.shape) for a in got] == g['encode_shapes']
    for a, want in zip(got, g['encode']):
        assert rr.same(a, np.asarray(want, np.float32))


# ---- (b) the wrong models -------------------------------------------------------------------------------------------------------
class IgnoresTerminal(RingModel):
    """next_obs never comes from final_obs."""
    def add(self, start, obs, act, rew, next_obs, final_obs=None, terminal=None, done=None):
        RingModel.add(self, start, obs, act, rew, next_obs, None, terminal, done)

    def add_rollout(self, start, obs0, out):
        RingModel.add_rollout(self, start, obs0, dict(out, final_obs=None))

    def pack(self, out, act, sel_t, sel_e):
        return RingModel.pack(self, dict(out, final_obs=None), act, sel_t, sel_e)


class FinalObsEverywhere(RingModel):
    """next_obs comes from final_obs whether the env ended or not (where final_obs and terminal are given)."""
    def add(self, start, obs, act, rew, next_obs, final_obs=None, terminal=None, done=None):
        RingModel.add(self, start, obs, act, rew, next_obs, final_obs, None if terminal is None else np.ones_like(terminal), done)

    def add_rollout(self, start, obs0, out):
        RingModel.add_rollout(self, start, obs0, dict(out, terminal=np.ones_like(out['terminal'])))

    def pack(self, out, act, sel_t, sel_e):
        return RingModel.pack(self, dict(out, terminal=None if out.get('terminal') is None else np.ones_like(out['terminal'])), act, sel_t, sel_e)


class WritesNActionColumns(RingModel):
    """N of the N*H action bytes of a slot are written."""
    def store(self, slot, obs, act, rew, next_obs, done):
        before = self.act[slot].copy()
        RingModel.store(self, slot, obs, act, rew, next_obs, done)
        flat, old = self.act[slot].reshape(-1), before.reshape(-1)
        flat[self.N:] = old[self.N:]


class SwapsHeads(RingModel):
    """(movement, symbol) stored -- or decoded -- as (symbol, movement)."""
    def store(self, slot, obs, act, rew, next_obs, done):
        RingModel.store(self, slot, obs, np.asarray(act)[..., ::-1] if self.heads == 2 else act, rew, next_obs, done)

    def one_hot(self, stored):
        return RingModel.one_hot(self, stored[::-1] if self.heads == 2 else stored)


class RewardOfAgentZero(RingModel):
    """A per-agent ring reads the reward at [e, 0] for every agent c."""
    def store(self, slot, obs, act, rew, next_obs, done):
        RingModel.store(self, slot, obs, act, np.full(self.N, rew[0], np.float32) if self.per_agent else rew, next_obs, done)

    def gather(self, idx):
        o, a, r, n, d = RingModel.gather(self, idx)
        return o, a, (np.repeat(r[:, :1], self.N, axis=1) if self.per_agent else r), n, d


class DoesNotWrap(RingModel):
    def slot(self, start, k):
        return min(start + k, self.cap - 1)


class ObsOfTheSameStep(RingModel):
    """obs of step t taken from the chunk's obs[t] instead of obs[t-1] (obs0 for t = 0)."""
    def add_rollout(self, start, obs0, out):
        RingModel.add_rollout(self, start, obs0, out)
        T, B = out['obs'].shape[:2]
        for t in range(T):
            for e in range(B):
                self.obs[self.slot(start, t * B + e)] = out['obs'][t, e]

    def pack(self, out, act, sel_t, sel_e):
        rows = RingModel.pack(self, out, act, sel_t, sel_e)
        for r, (t, e) in enumerate(zip(sel_t, sel_e)):
            rows[r, :self.N * self.D] = out['obs'][t, e].reshape(-1)
        return rows


class DecodesHeadOneWithHeadZerosWidth(RingModel):
    def one_hot(self, stored):
        row = RingModel.one_hot(self, stored)
        if self.heads == 2:
            W0 = self.head_width[0] if self.head_width[0] > 0 else 5
            row[2 * W0:] = 0.0
        return row


WRITER_VARIANTS = (IgnoresTerminal, FinalObsEverywhere, WritesNActionColumns, SwapsHeads, RewardOfAgentZero, DoesNotWrap, ObsOfTheSameStep)


def _applies(variant, op, kind, N, transitions, cap, final):
    """Whether `variant` changes anything `op` does on a ring of `kind` at all; with the exemptions: the (variant, shape) pairs at
    which it coincides with the true model WHATEVER the inputs are."""
    k = rr.KINDS[kind]
    if variant in (IgnoresTerminal, FinalObsEverywhere):
        if op not in ('add', 'rollout', 'pack') or not final:
            return False
        # exempt: ONE transition whose terminal flag is set (the masks set the first and last env) -- final_obs everywhere IS the contract there
        return not (variant is FinalObsEverywhere and transitions == 1)
    if variant in (WritesNActionColumns, SwapsHeads):
        return k['heads'] == 2 and op in ('add', 'rollout')
    if variant is RewardOfAgentZero:
        # exempt: N = 1 -- agent c IS agent 0
        return k['per_agent'] and op in ('add', 'rollout') and N > 1
    if variant is DoesNotWrap:
        # exempt: a ring of one slot -- min(start + e, 0) and (start + e) % 1 are both 0
        return op in ('add', 'rollout', 'packed') and cap > 1
    if variant is ObsOfTheSameStep:
        return op in ('rollout', 'pack')
    raise AssertionError(variant)


def _differs(a, b):
    return any(not rr.same(x, y) for x, y in zip(a, b))


def _writer_cases():
    for kind in rr.KINDS:
        for cap, N, D, B, start in rr.ADD_SHAPES + (rr.ADD_WIDE,):
            for final in ('both', 'final_obs', 'terminal', 'neither'):
                if (cap, N, D, B, start) == rr.ADD_WIDE and final != 'both':
                    continue
                yield ('add', kind, (cap, N, D, B, start), final)
        for shape in rr.ROLLOUT_SHAPES + (rr.ROLLOUT_WIDE,):
            for final in (True, False):
                yield ('rollout', kind, shape, final)
    for shape in rr.TAIL_SHAPES:
        yield ('add', 'plain', shape, 'both')
    for shape in rr.PACK_SHAPES:
        for final in ('both', 'final_obs', 'terminal'):
            yield ('pack', 'plain', shape, final)
        yield ('packed', 'plain', shape, None)


def _run_writer(cls, op, kind, shape, final):
    """The planes (or rows) `cls` leaves after `op` on the inputs the GPU test of this case uses."""
    if op == 'add':
        cap, N, D, B, start = shape
        m = cls(**dict(rr.initial_planes(cap, N, D, kind), head_width=rr.KINDS[kind]['head_width']))
        a = rr.add_inputs(kind, N, D, B, final=final, done=True)
        m.add(start, a['obs'], a['act'], a['rew'], a['next_obs'], a['final_obs'], a['terminal'], a['done'])
        return list(m.planes().values())
    if op == 'rollout':
        cap, start, T, B, N, D = shape
        m = cls(**dict(rr.initial_planes(cap, N, D, kind), head_width=rr.KINDS[kind]['head_width']))
        obs0, out = rr.chunk(kind, T, B, N, D, final=final)
        m.add_rollout(start, obs0, out)
        return list(m.planes().values())
    T, B, N, D, R, _ = shape
    obs0, out = rr.chunk('plain', T, B, N, D, final=final in ('both', 'final_obs'), terminal=final in ('both', 'terminal'))
    sel_t, sel_e = rr.selection(T, B, R)
    cap, start = rr.packed_ring(R)
    m = cls(**rr.initial_planes(cap, N, D, 'plain'))
    if op == 'pack':
        return [m.pack(out, out['act'], sel_t, sel_e)]
    m.add_packed(start, rr.packed_rows(RingModel(**rr.initial_planes(cap, N, D, 'plain')), T, B, N, D, R))
    return list(m.planes().values())


@pytest.mark.parametrize('case', list(_writer_cases()), ids=lambda c: '%s-%s-%s-%s' % (c[0], c[1], 'x'.join(str(s) for s in c[2]), c[3]))
def test_every_wrong_writer_is_told_apart_on_the_inputs_the_gpu_tests_use(case):
    op, kind, shape, final = case
    if op == 'add':
        cap, N, transitions = shape[0], shape[1], shape[3]
    elif op == 'rollout':
        cap, N, transitions = shape[0], shape[4], shape[2] * shape[3]
    else:
        cap, N, transitions = rr.packed_ring(shape[4])[0], shape[2], shape[4]
    has_final = final in ('both', True)
    true = _run_writer(RingModel, op, kind, shape, final)
    for variant in WRITER_VARIANTS:
        if _applies(variant, op, kind, N, transitions, cap, has_final):
            assert _differs(true, _run_writer(variant, op, kind, shape, final)), variant.__name__
    if op == 'rollout' and final:       # the chunk's done plane reaches a per-agent ring and no other
        cap_, start, T, B, N_, D = shape
        m = rr.model_from(rr.initial_planes(cap_, N_, D, kind), kind)
        obs0, out = rr.chunk(kind, T, B, N_, D, done=None)
        m.add_rollout(start, obs0, out)
        assert _differs(true, list(m.planes().values())) == rr.KINDS[kind]['per_agent']


def _gather_cases():
    for kind in rr.KINDS:
        for cap, N, D in rr.GATHER_RINGS:
            for b in rr.GATHER_BATCHES:
                yield (kind, cap, N, D, b)
        yield (kind,) + rr.GATHER_WIDE


@pytest.mark.parametrize('case', list(_gather_cases()), ids=lambda c: '-'.join(str(s) for s in c))
def test_every_wrong_gather_is_told_apart_on_the_inputs_the_gpu_tests_use(case):
    kind, cap, N, D, b = case
    k = rr.KINDS[kind]
    idx = rr.gather_index(cap, b)
    true = rr.model_from(rr.ring_contents(cap, N, D, kind), kind).gather(idx)
    for variant in (SwapsHeads, DecodesHeadOneWithHeadZerosWidth, RewardOfAgentZero):
        if variant is RewardOfAgentZero and not (k['per_agent'] and N > 1):      # exempt at N = 1: agent c IS agent 0
            continue
        if variant is not RewardOfAgentZero and k['heads'] != 2:
            continue
        m = variant(**dict(rr.ring_contents(cap, N, D, kind), head_width=k['head_width']))
        assert _differs(true, m.gather(idx)), variant.__name__
    # a slot read through the wrong index: every slot of the ring holds other observations, rewards and done flags
    for plane in ('obs', 'next_obs', 'rew', 'done'):
        words = rr.bits(rr.ring_contents(cap, N, D, kind)[plane]).reshape(cap, -1)
        assert len({w.tobytes() for w in words}) == cap, plane


def test_the_generators_keep_their_promises():
    for shape, salt in (((7, 1, 2), 0), ((257, 3, 10), 1), ((331, 64, 104), 2), ((5, 130, 64, 104), 5)):
        v = rr.values(shape, salt)
        words = rr.bits(v).reshape(-1)
        assert len(np.unique(words)) == words.size                          # distinct, the special values included
        assert all(s in words for s in rr.SPECIALS)
    assert not set(rr.bits(rr.values((50,), 0)).tolist()) - set(rr.SPECIALS) & set(rr.bits(rr.values((50,), 1)).tolist())   # tensors of a case share nothing else
    for B in (1, 4, 7, 257):
        t = rr.terminal_mask((B,))
        assert t[0] == 1 and t[-1] == 1 and (B < 4 or (0 < t[1:-1].sum() < B - 2))
    t = rr.terminal_mask((9, 33))
    assert t[:, 0].all() and t[:, -1].all() and not np.array_equal(t[0], t[1])
    a = rr.actions((9, 33, 3), (5, 10))
    assert a[..., 0].min() == 0 and a[..., 0].max() == 4 and a[..., 1].min() == 0 and a[..., 1].max() == 9 and (a[..., 0] != a[..., 1]).any()
    for T, B, R in ((4, 5, 9), (3, 8, 80), (3, 8, 40)):
        st, se = rr.selection(T, B, R)
        pairs = list(zip(st.tolist(), se.tolist()))
        assert len(pairs) == R and st.min() >= 1 and len(set(pairs)) < R
        assert {1, T - 1} <= set(st.tolist()) and {0, B - 1} <= set(se.tolist()) and se.min() >= 0 and se.max() < B
    idx = rr.gather_index(1000, 257)
    assert {0, 999} <= set(idx.tolist()) and len(set(idx.tolist())) < 257 and idx.min() >= 0 and idx.max() < 1000
    assert idx[4:10].tolist() == [999, 998, 997, 996, 995, 994]
    d = rr.done_bytes((9, 33, 3))
    assert {0, 1, 255} <= set(d.reshape(-1).tolist())
    # the wide sizes take the second trip of their grid-stride loop: elements > cap of grid_blocks * 256 (csrc/pworld_replay.hip)
    cap, N, D, B, _ = rr.ADD_WIDE
    assert B * N * D > 8192 * 256 and rr.GATHER_WIDE[3] * N * D > 8192 * 256
    cap, _, T, B, N, D = rr.ROLLOUT_WIDE
    assert T * B * N * D > 16384 * 256 and T * B <= cap
    T, B, N, D, R, R_in = rr.PACK_SHAPES[-1]
    assert R * (2 * N * D + N + 2) > 4096 * 256 and R_in * (2 * N * D + N + 2) > 2048 * 256
    assert rr.RingModel.counter_add(5, 3, 0) == 8 and rr.RingModel.counter_add(8, 4, 10) == 2 and rr.RingModel.counter_add(2 ** 40, 1, 0) == 2 ** 40 + 1


def test_the_models_pack_is_the_stand_ins_pack():
    """tests/dist_standins.pack_reference (torch) and the model restate the same rows independently."""
    torch = pytest.importorskip('torch')
    from tests.dist_standins import pack_reference
    T, B, N, D, R, _ = rr.PACK_SHAPES[1]
    obs0, out = rr.chunk('plain', T, B, N, D)
    sel_t, sel_e = rr.selection(T, B, R)
    rows = RingModel(**rr.initial_planes(4, N, D, 'plain')).pack(out, out['act'], sel_t, sel_e)
    cpu = {k: torch.from_numpy(v) for k, v in out.items() if v is not None}
    cpu['terminal'] = cpu['terminal'].bool()
    want = pack_reference(cpu, torch.from_numpy(out['act']), torch.from_numpy(sel_t), torch.from_numpy(sel_e))
    assert rr.same(rows, want.numpy())


# ---- (c) the refusals -----------------------------------------------------------------------------------------------------------
P = [C.c_void_p(0x100000 + 0x10000 * i) for i in range(16)]          # fake, 256-byte aligned "device pointers"


def _ring(N=3, D=10, cap=100, **kw):
    st = _lib.PwReplayStore()
    st.obs, st.next_obs, st.rew, st.done, st.act, st.lm = 4096, 8192, 12288, 16384, 20480, 24576
    st.capacity, st.num_agents, st.obs_dim = cap, N, D
    for k, v in kw.items():
        if k == 'head_width':
            st.head_width[0], st.head_width[1] = v
        else:
            setattr(st, k, v)
    return st


def _io(**kw):
    io = _lib.PwStepIO()
    for k in ('obs', 'rew_shared', 'terminal', 'act_idx'):
        setattr(io, k, 0x900000 + 0x10000 * len(k))
    for k, v in kw.items():
        setattr(io, k, v)
    return io


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _refused(lib, rc, *words):
    msg = lib.pw_last_error()
    assert rc == -1 and all(w in msg for w in words), (rc, msg, words)       # PW_EINVAL


def _add(lib, st, start=0, B=4):
    return lib.pw_replay_add(C.byref(st), start, None, B, P[0], P[1], P[2], P[3], P[4], P[5], None, None)


def _tail(lib, st, start=0, B=4, start_dev=None, next_start_dev=None):
    return lib.pw_replay_add_tail(C.byref(st), start, start_dev, next_start_dev, B, P[0], P[1], P[2], P[3], P[4], P[5], None,
                                  P[6], P[7], P[8], None, None)


def _rollout(lib, st, start=0, B=4, T=3, io=None, book=(None, None, None, None)):
    return lib.pw_replay_add_rollout(C.byref(st), start, B, T, P[0], C.byref(io if io is not None else _io()), P[1], book[0], book[1],
                                     book[2], book[3], None)


def _packed(lib, st, start=0, R=4):
    return lib.pw_replay_add_packed(C.byref(st), start, R, P[0], None)


def _gather(lib, st, b=4):
    return lib.pw_replay_gather(C.byref(st), P[0], b, P[1], P[2], P[3], P[4], P[5], None)


def _sample(lib, st, b=4):
    return lib.pw_replay_sample(C.byref(st), 1, P[0], P[1], b, P[2], P[3], P[4], P[5], P[6], P[7], None)


def _exchange(lib, st, start=0, R_in=4, rows_in=P[0], io='chunk', N=3, D=10, R_out=4, rows_out=P[1]):
    io = _io() if io == 'chunk' else io
    return lib.pw_exchange(None if st is None else C.byref(st), start, R_in, rows_in, None if io is None else C.byref(io), 8, N, D,
                           P[2], P[3], R_out, rows_out, None)


def test_a_write_that_does_not_fit_the_ring_is_refused(lib):
    for call in (_add, _tail):
        for kw in (dict(B=0), dict(B=-1), dict(B=101), dict(start=-1)):
            _refused(lib, call(lib, _ring(), **kw), b'bad ring arguments')
    for kw in (dict(R=0), dict(R=101), dict(start=-1)):
        _refused(lib, _packed(lib, _ring(), **kw), b'bad ring arguments')
    for kw in (dict(B=0), dict(T=0), dict(B=34, T=3), dict(start=-1)):          # 34 * 3 = 102 > 100
        _refused(lib, _rollout(lib, _ring(), **kw), b'bad ring arguments', b'the chunk must fit the ring')
    _refused(lib, _exchange(lib, _ring(), R_in=101), b'bad ring arguments')
    _refused(lib, _exchange(lib, _ring(), start=-1), b'bad ring arguments')
    _refused(lib, _add(lib, _ring(cap=0), B=1), b'bad ring arguments')


def test_rows_too_short_for_the_kernels_index_split_are_refused(lib):
    _refused(lib, _add(lib, _ring(D=1)), b'obs_dim must be >= 2')
    _refused(lib, _gather(lib, _ring(D=1)), b'obs_dim must be >= 2')
    _refused(lib, _sample(lib, _ring(D=1)), b'pw_replay_sample', b'obs_dim must be >= 2')
    _refused(lib, _tail(lib, _ring(D=4)), b'obs_dim must be >= 5')
    _refused(lib, _rollout(lib, _ring(D=4)), b'obs_dim must be >= 5')


@pytest.mark.parametrize('bad', [dict(act_heads=3), dict(act_heads=-1), dict(act_heads=2, head_width=(5, 0)), dict(act_heads=2, head_width=(-1, 10))])
def test_an_action_layout_no_kernel_serves_is_refused_by_every_entry_point_that_reads_it(lib, bad):
    """pw_replay_add_rollout used to take act_heads = 3: its kernel then stores ONE index per agent where the gather reads two."""
    for call in (_add, _gather, _rollout):
        _refused(lib, call(lib, _ring(**bad)), b'bad act_heads / head_width')
    _refused(lib, _sample(lib, _ring(**bad)), b'pw_replay_sample', b'bad st->act_heads / st->head_width')


def test_the_action_layouts_the_kernels_serve_pass_the_same_checks(lib):
    """The refusals above are about the layout: the same calls with a served layout get past them (and stop at a LATER check, so
    still nothing launches)."""
    for good in (dict(), dict(act_heads=1), dict(act_heads=2, head_width=(0, 10)), dict(act_heads=2, head_width=(5, 1))):
        _refused(lib, _rollout(lib, _ring(**good), book=(P[6], None, None, None)), b'bookkeeping needs')


def test_the_plain_ring_entry_points_refuse_every_other_ring(lib):
    calls = ((_tail, b'pw_replay_add_tail'), (_packed, b'pw_replay_add_packed'), (_exchange, b'pw_exchange'))
    for call, who in calls:
        _refused(lib, call(lib, _ring(per_agent=1)), who, b'per-agent ring')
        _refused(lib, call(lib, _ring(act_heads=2, head_width=(5, 10))), who, b'two-head ring')
        _refused(lib, call(lib, _ring(D=10, state_rows=1, num_landmarks=3, scenario=_lib.PW_SIMPLE_SPREAD)), who, b'STATE ring')
    state = dict(D=10, state_rows=1, num_landmarks=3, scenario=_lib.PW_SIMPLE_SPREAD)
    _refused(lib, _add(lib, _ring(**state)), b'pw_replay_add', b'STATE ring')
    _refused(lib, _rollout(lib, _ring(**state)), b'pw_replay_add_rollout', b'STATE ring')


def test_the_tail_and_rollout_refuse_half_given_arguments(lib):
    _refused(lib, _tail(lib, _ring(), start_dev=P[9], next_start_dev=P[9]), b'must not alias')
    _refused(lib, _rollout(lib, _ring(per_agent=1), io=_io(rew=0)), b'pw_replay_add_rollout', b'per-agent rew')
    for book in ((P[6], None, P[8], P[9]), (P[6], P[7], None, P[9]), (P[6], P[7], P[8], None), (P[6], None, None, None)):
        _refused(lib, _rollout(lib, _ring(), book=book), b'bookkeeping needs')
    _refused(lib, _rollout(lib, _ring(), io=_io(terminal=0)), b'null argument')
    _refused(lib, lib.pw_replay_add(C.byref(_ring()), 0, None, 4, P[0], P[1], P[2], None, P[4], P[5], None, None), b'null argument')


def test_gather_pack_and_exchange_refuse_empty_and_mismatched_work(lib):
    _refused(lib, _gather(lib, _ring(), b=0), b'batch must be >= 1')
    _refused(lib, _gather(lib, _ring(), b=-5), b'batch must be >= 1')
    _refused(lib, _exchange(lib, None, io=None), b'nothing to do')
    _refused(lib, _exchange(lib, _ring(), R_in=0, R_out=0), b'nothing to do')
    _refused(lib, _exchange(lib, _ring(), rows_in=None, rows_out=None), b'nothing to do')
    _refused(lib, _exchange(lib, _ring(), N=4), b'row width mismatch')
    _refused(lib, _exchange(lib, _ring(), D=12), b'row width mismatch')
    _refused(lib, _exchange(lib, None, io=_io(obs=0)), b'chunk needs obs')

    def pack(io, R=4):
        return lib.pw_pack_transitions(C.byref(io), 8, 3, 10, P[2], P[3], R, P[1], None)
    _refused(lib, pack(_io(), R=0), b'bad sizes')
    _refused(lib, pack(_io(), R=-2), b'bad sizes')
    _refused(lib, pack(_io(obs=0)), b'chunk needs obs')
    _refused(lib, pack(_io(act_idx=0)), b'chunk needs obs')
    _refused(lib, lib.pw_counter_add(None, 1, 0, None), b'null counter')
