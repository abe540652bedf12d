"""GPU: the replay ring's base layer -- pw_replay_add, pw_replay_add_tail, pw_replay_add_rollout, pw_replay_gather, pw_replay_sample,
pw_pack_transitions, pw_replay_add_packed, pw_exchange, pw_counter_add -- against the plain NumPy ring model of tests/ring_ref.py.

Most of the suite's ring tests compare one launch of the library with another; these entry points are the other launch.  Here each is
called through ctypes on a hand-built ``pw_replay_store`` whose planes (and every output buffer) are guarded buffers (tests/guarded.py):
the model starts from the planes' bytes, and after the launch EVERY plane must equal the model's bit for bit -- the slots the launch did
not write included -- with the guard bands intact.  Inputs come from the generators of tests/ring_ref.py; tests/test_ring_ref_host.py
shows on the CPU that those inputs tell eight wrong models from the true one at every shape used here.  Everything is a copy, an
integer conversion or an index computation: every comparison is exact.

The "wide" shapes (N = 64, D = 104) have more elements than the launch's grid cap x 256 threads, so the second trip of each
grid-stride loop of csrc/pw_kernels_replay.hpp is taken.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from multiagent_rl_amd import _lib  # noqa: E402
from tests import ring_ref as rr  # noqa: E402
from tests.guarded import assert_guards_intact, assert_untouched, guarded  # noqa: E402

F32, U8, I64 = torch.float32, torch.uint8, torch.int64


def dev(a):
    """A NumPy array's bytes on the device (None stays None)."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to('cuda')


def host(t):
    return t.detach().cpu().numpy()


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return _lib.stream(torch.device('cuda', torch.cuda.current_device()))


def assert_same(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    g, w = rr.bits(got).reshape(-1), rr.bits(want).reshape(-1)
    bad = np.flatnonzero(g != w)
    assert not bad.size, '%s: %d of %d elements differ; the first at flat index %d: got 0x%X, want 0x%X' % (
        name, bad.size, g.size, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


def filled(shape, dtype, a):
    """A guarded buffer holding the array's bytes."""
    t = guarded(shape, dtype)
    t.copy_(dev(a).view(shape))
    return t


def cell(v):
    return filled((1,), I64, np.array([v], np.int64))


class Ring(object):
    """A pw_replay_store over guarded planes.  Without `contents` the planes keep the guard pattern (arbitrary words: NaNs, indices
    outside every head) -- the model is built from whatever they hold."""

    def __init__(self, cap, N, D, kind, head_width=None, contents=None):
        k = rr.KINDS[kind]
        self.kind, self.head_width = kind, tuple(k['head_width'] if head_width is None else head_width)
        rs = (cap, N) if k['per_agent'] else (cap,)
        self.t = dict(obs=guarded((cap, N, D), F32), next_obs=guarded((cap, N, D), F32),
                      act=guarded((cap, N, 2) if k['heads'] == 2 else (cap, N), U8), rew=guarded(rs, F32), done=guarded(rs, F32))
        if contents is not None:
            for name, t in self.t.items():
                t.copy_(dev(contents[name]))
        st = self.st = _lib.PwReplayStore()
        for name, t in self.t.items():
            setattr(st, name, t.data_ptr())
        st.capacity, st.num_agents, st.obs_dim = cap, N, D
        st.act_heads = 2 if k['heads'] == 2 else (1 if k['per_agent'] else 0)        # 0 and 1 both mean one head
        st.per_agent = int(k['per_agent'])
        st.head_width[0], st.head_width[1] = self.head_width

    def model(self):
        """The model of the ring as it is NOW (read back from the device)."""
        return rr.model_from({name: host(t) for name, t in self.t.items()}, self.kind, self.head_width)

    def check(self, model, what=''):
        for name, t in self.t.items():
            assert_same(host(t), model.planes()[name], '%s plane %s' % (what, name))
            assert_guards_intact(t, '%s plane %s' % (what, name))

    def ref(self):
        return C.byref(self.st)


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


# ---- pw_replay_add --------------------------------------------------------------------------------------------------------------
def _add(lib, kind, shape, final, done, cursor):
    cap, N, D, B, start = shape
    ring = Ring(cap, N, D, kind)
    model = ring.model()
    a = rr.add_inputs(kind, N, D, B, final=final, done=done)
    d = {k: dev(v) for k, v in a.items()}
    cur = cell(start) if cursor == 'start_dev' else None
    by_value = (start + 3) % cap if cur is not None else start               # with a cell, the by-value argument is ANOTHER position
    _lib.check(lib.pw_replay_add(ring.ref(), by_value, p(cur), B, p(d['obs']), p(d['act']), p(d['rew']), p(d['next_obs']), p(d['final_obs']),
                                 p(d['terminal']), p(d['done']), stream()))
    model.add(start, a['obs'], a['act'], a['rew'], a['next_obs'], a['final_obs'], a['terminal'], a['done'])
    what = 'add %s %s final=%s done=%s %s:' % (kind, shape, final, done, cursor)
    ring.check(model, what)
    if cur is not None:
        assert int(cur.item()) == start
        assert_guards_intact(cur, what + ' cursor cell')


@pytest.mark.parametrize('final', ['both', 'final_obs', 'terminal', 'neither'])
@pytest.mark.parametrize('shape', rr.ADD_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('kind', list(rr.KINDS))
def test_add_equals_the_model_on_every_ring_kind(lib, kind, shape, final):
    """final_obs / terminal both given, one NULL, both NULL; done NULL and given (non-zero values); the position by value and from a
    device cell that overrides another by-value position."""
    for done in (False, True):
        for cursor in ('start', 'start_dev'):
            _add(lib, kind, shape, final, done, cursor)


@pytest.mark.parametrize('kind', list(rr.KINDS))
def test_add_takes_the_second_trip_of_its_grid_stride_loop(lib, kind):
    _add(lib, kind, rr.ADD_WIDE, 'both', True, 'start_dev')


# ---- pw_replay_add_tail ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('done', [False, True], ids=['done_null', 'done_given'])
@pytest.mark.parametrize('shape', rr.TAIL_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_add_tail_fills_the_ring_as_the_model_and_publishes_the_next_position(lib, shape, done):
    """The ring half of the launch (the episode statistics: tests/test_gpu_episode_stats.py).  `done` is an input the Python wrapper
    never passes."""
    cap, N, D, B, start = shape
    for cursor in ('start', 'start_dev'):
        ring = Ring(cap, N, D, 'plain')
        model = ring.model()
        a = rr.add_inputs('plain', N, D, B, final='both', done=done)
        d = {k: dev(v) for k, v in a.items()}
        cur = cell(start) if cursor == 'start_dev' else None
        nxt, step = cell(-77), cell(41)
        ep_ret, fin_sum, fin_cnt = torch.zeros(B, device='cuda'), torch.zeros(1, dtype=torch.float64, device='cuda'), torch.zeros(1, dtype=I64, device='cuda')
        _lib.check(lib.pw_replay_add_tail(ring.ref(), (start + 3) % cap if cur is not None else start, p(cur), p(nxt), B, p(d['obs']), p(d['act']),
                                          p(d['rew']), p(d['next_obs']), p(d['final_obs']), p(d['terminal']), p(d['done']), p(ep_ret),
                                          p(fin_sum), p(fin_cnt), p(step), stream()))
        model.add(start, a['obs'], a['act'], a['rew'], a['next_obs'], a['final_obs'], a['terminal'], a['done'])
        what = 'add_tail %s done=%s %s:' % (shape, done, cursor)
        ring.check(model, what)
        assert start + B > cap and int(nxt.item()) == (start + B) % cap == model.next_idx      # across the ring's end
        assert int(step.item()) == 42
        for t, name in ((nxt, 'next_start_dev'), (step, 'step_counter')) + (((cur, 'start_dev'),) if cur is not None else ()):
            assert_guards_intact(t, what + ' ' + name)
        assert cur is None or int(cur.item()) == start


# ---- pw_replay_add_rollout ------------------------------------------------------------------------------------------------------
ROLLOUT_MODES = {'final_null': dict(final=False, done=None), 'done_null': dict(final=True, done=None), 'done_nonzero': dict(final=True, done='nonzero')}


def _rollout(lib, kind, shape, mode):
    cap, start, T, B, N, D = shape
    ring = Ring(cap, N, D, kind)
    model = ring.model()
    obs0, out = rr.chunk(kind, T, B, N, D, **ROLLOUT_MODES[mode])
    d = {k: dev(v) for k, v in out.items()}
    d_obs0 = dev(obs0)
    io = _lib.PwStepIO()
    for name in ('obs', 'final_obs', 'terminal', 'rew_shared', 'rew', 'done'):      # a plain ring is handed rew and done too: it must not read them
        if d[name] is not None:
            setattr(io, name, d[name].data_ptr())
    _lib.check(lib.pw_replay_add_rollout(ring.ref(), start, B, T, p(d_obs0), C.byref(io), p(d['act']), None, None, None, None, stream()))
    model.add_rollout(start, obs0, out)
    ring.check(model, 'add_rollout %s %s %s:' % (kind, shape, mode))


@pytest.mark.parametrize('mode', list(ROLLOUT_MODES))
@pytest.mark.parametrize('shape', rr.ROLLOUT_SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('kind', list(rr.KINDS))
def test_add_rollout_equals_the_model_on_every_ring_kind(lib, kind, shape, mode):
    """One transition in a ring of one slot; T*B = capacity with a wrap; 297 transitions of 30 numbers across a wrap.  final_obs NULL,
    io.done NULL, io.done with non-zero bytes (a per-agent ring stores them as floats, a plain one stores 0)."""
    _rollout(lib, kind, shape, mode)


@pytest.mark.parametrize('kind', list(rr.KINDS))
def test_add_rollout_takes_the_second_trip_of_its_grid_stride_loop(lib, kind):
    _rollout(lib, kind, rr.ROLLOUT_WIDE, 'done_nonzero')


# ---- pw_replay_gather -----------------------------------------------------------------------------------------------------------
OUTPUTS = ('obs', 'act', 'rew', 'next_obs', 'done')


def _out_shapes(ring, b):
    st, k = ring.st, rr.KINDS[ring.kind]
    N, D = st.num_agents, st.obs_dim
    W = (ring.head_width[0] if ring.head_width[0] > 0 else 5) + (ring.head_width[1] if k['heads'] == 2 else 0)
    rs = (b, N) if k['per_agent'] else (b,)
    return dict(obs=(b, N, D), act=(b, N, W), rew=rs, next_obs=(b, N, D), done=rs)


def _gather(lib, ring, idx, given=OUTPUTS):
    """One pw_replay_gather with guarded buffers for the outputs in `given` and NULL for the others."""
    shapes = _out_shapes(ring, len(idx))
    outs = {name: guarded(shapes[name], F32) for name in given}
    d_idx = dev(idx)
    _lib.check(lib.pw_replay_gather(ring.ref(), p(d_idx), len(idx), *([p(outs.get(name)) for name in OUTPUTS] + [stream()])))
    return outs


def _check_gather(outs, want, what):
    for name, t in outs.items():
        assert_same(host(t), want[OUTPUTS.index(name)], '%s out_%s' % (what, name))
        assert_guards_intact(t, '%s out_%s' % (what, name))


def _gather_case(lib, kind, cap, N, D, b):
    contents = rr.ring_contents(cap, N, D, kind)
    ring = Ring(cap, N, D, kind, contents=contents)          # the model's contents written straight into the planes, not through an add
    model = rr.model_from(contents, kind)
    idx = rr.gather_index(cap, b)
    what = 'gather %s cap %d N %d D %d b %d:' % (kind, cap, N, D, b)
    _check_gather(_gather(lib, ring, idx), model.gather(idx), what)
    ring.check(model, what)                                  # a gather writes nothing into the ring


@pytest.mark.parametrize('b', rr.GATHER_BATCHES)
@pytest.mark.parametrize('shape', rr.GATHER_RINGS, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('kind', list(rr.KINDS))
def test_gather_equals_the_model_on_every_ring_kind(lib, kind, shape, b):
    _gather_case(lib, kind, *(shape + (b,)))


@pytest.mark.parametrize('kind', list(rr.KINDS))
def test_gather_takes_the_second_trip_of_its_grid_stride_loop(lib, kind):
    _gather_case(lib, kind, *rr.GATHER_WIDE)


@pytest.mark.parametrize('kind', list(rr.KINDS))
def test_gather_with_each_output_null_on_its_own_and_each_output_alone(lib, kind):
    cap, N, D = rr.GATHER_RINGS[2]
    b = 257
    contents = rr.ring_contents(cap, N, D, kind)
    ring = Ring(cap, N, D, kind, contents=contents)
    model = rr.model_from(contents, kind)
    idx = rr.gather_index(cap, b)
    want = model.gather(idx)
    full = {name: host(t) for name, t in _gather(lib, ring, idx).items()}
    for i, name in enumerate(OUTPUTS):
        assert_same(full[name], want[i], 'full launch out_%s' % name)
    subsets = [tuple(n for n in OUTPUTS if n != skip) for skip in OUTPUTS] + [(only,) for only in OUTPUTS]
    for given in subsets:
        what = 'gather %s given %s:' % (kind, '+'.join(given))
        outs = _gather(lib, ring, idx, given)
        _check_gather(outs, want, what)
        for name, t in outs.items():
            assert_same(host(t), full[name], what + ' vs the full launch, out_%s' % name)
    ring.check(model, 'gather subsets %s:' % kind)


@pytest.mark.parametrize('kind,head_width', [('plain', (3, 0)), ('plain', (16, 0)), ('plain', (0, 0)), ('per_agent', (16, 0)), ('two_head', (0, 10)),
                                             ('per_agent_two_head', (3, 16))], ids=lambda v: str(v).replace(' ', ''))
def test_gather_action_encoding(lib, kind, head_width):
    """One-hot rows of width W0 (| W1); head_width[0] = 0 means 5; a stored index outside its head -- 200, and the head's own width --
    selects no column."""
    cap, N, D = rr.GATHER_RINGS[0]
    contents = rr.ring_contents(cap, N, D, kind, head_width=head_width)
    W0 = head_width[0] if head_width[0] > 0 else 5
    act = contents['act'].reshape(cap, N, -1)
    act[0, 0, 0], act[0, 1, 0] = 200, W0                     # slot 0: agent 0 far outside head 0, agent 1 one past its last index
    act[cap - 1, 1, -1] = 200                                # slot cap-1, agent 1: the last head
    if act.shape[2] == 2:
        act[cap - 1, 0, 1] = head_width[1]
    ring = Ring(cap, N, D, kind, head_width=head_width, contents=contents)
    model = rr.model_from(contents, kind, head_width)
    idx = rr.gather_index(cap, 5)                            # slots cap-1 and 0, each more than once
    want = model.gather(idx)
    k = rr.KINDS[kind]
    assert want[1].shape == (5, N, W0 + (head_width[1] if k['heads'] == 2 else 0))
    assert not want[1][1, 0, :W0].any() and not want[1][1, 1, :W0].any() and want[1][0, 0, :W0].sum() == 1     # the zero rows are in the batch
    what = 'gather %s head_width %s:' % (kind, head_width)
    _check_gather(_gather(lib, ring, idx), want, what)
    ring.check(model, what)


# ---- pw_replay_sample -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['plain', 'per_agent_two_head'])
def test_sample_on_a_row_ring_takes_the_second_trip_of_its_grid_stride_loop(lib, kind):
    cap, N, D, b = rr.GATHER_WIDE
    seed, call, length = 0x9E3779B97F4A7C15, 3, cap - 3
    contents = rr.ring_contents(cap, N, D, kind)
    ring = Ring(cap, N, D, kind, contents=contents)
    model = rr.model_from(contents, kind)
    shapes = _out_shapes(ring, b)
    outs = {name: guarded(shapes[name], F32) for name in OUTPUTS}
    out_idx, call_dev, len_dev = guarded((b,), I64), cell(call), cell(length)
    _lib.check(lib.pw_replay_sample(ring.ref(), seed, p(call_dev), p(len_dev), b, p(out_idx), *([p(outs[name]) for name in OUTPUTS] + [stream()])))
    idx = host(out_idx)
    want_idx = np.array([lib.pw_replay_draw_host(seed, call, e, length) for e in range(b)], np.int64)
    assert_same(idx, want_idx, 'sample %s out_idx' % kind)
    assert idx.min() >= 0 and idx.max() < length
    _check_gather(outs, model.gather(idx), 'sample %s:' % kind)
    assert_guards_intact(out_idx, 'out_idx')
    assert int(call_dev.item()) == call and int(len_dev.item()) == length           # the launch does not advance the counter
    ring.check(model, 'sample %s:' % kind)


# ---- pw_pack_transitions, pw_replay_add_packed, pw_exchange -----------------------------------------------------------------------
PACK_MODES = {'both': dict(final=True, terminal=True), 'final_null': dict(final=False, terminal=True), 'terminal_null': dict(final=True, terminal=False)}
PACK_IDS = ['N%d_D%d' % (s[2], s[3]) for s in rr.PACK_SHAPES]


def _chunk_io(d):
    io = _lib.PwStepIO()
    for name in ('obs', 'final_obs', 'terminal', 'rew_shared'):
        if d[name] is not None:
            setattr(io, name, d[name].data_ptr())
    io.act_idx = d['act'].data_ptr()
    return io


def _plain_model(N, D):
    return rr.model_from(rr.initial_planes(2, N, D, 'plain'), 'plain')       # pack() reads the chunk only


@pytest.mark.parametrize('mode', list(PACK_MODES))
@pytest.mark.parametrize('shape', rr.PACK_SHAPES, ids=PACK_IDS)
def test_pack_transitions_equals_the_model(lib, shape, mode):
    T, B, N, D, R, _ = shape
    obs0, out = rr.chunk('plain', T, B, N, D, **PACK_MODES[mode])
    sel_t, sel_e = rr.selection(T, B, R)
    d = {k: dev(v) for k, v in out.items()}
    d_t, d_e = dev(sel_t), dev(sel_e)
    rows = guarded((R, 2 * N * D + N + 2), F32)
    io = _chunk_io(d)
    _lib.check(lib.pw_pack_transitions(C.byref(io), B, N, D, p(d_t), p(d_e), R, p(rows), stream()))
    want = _plain_model(N, D).pack(out, out['act'], sel_t, sel_e)
    if mode == 'both':
        assert out['terminal'][sel_t, sel_e].any() and not out['terminal'][sel_t, sel_e].all()        # rows of both sources
    assert_same(host(rows), want, 'pack %s %s rows' % (shape, mode))
    assert_guards_intact(rows, 'rows')


@pytest.mark.parametrize('shape', rr.PACK_SHAPES, ids=PACK_IDS)
def test_add_packed_equals_the_model_across_a_wrap_with_a_done_column(lib, shape):
    T, B, N, D, R, _ = shape
    cap, start = rr.packed_ring(R)
    ring = Ring(cap, N, D, 'plain')
    model = ring.model()
    rows = rr.packed_rows(_plain_model(N, D), T, B, N, D, R)
    d_rows = dev(rows)
    _lib.check(lib.pw_replay_add_packed(ring.ref(), start, R, p(d_rows), stream()))
    model.add_packed(start, rows)
    ring.check(model, 'add_packed %s:' % (shape,))


@pytest.mark.parametrize('mode', ['ingest_only', 'pack_only', 'both', 'pack_only-final_null', 'pack_only-terminal_null', 'both-final_null',
                                  'both-terminal_null'])
@pytest.mark.parametrize('shape', rr.PACK_SHAPES, ids=PACK_IDS)
def test_exchange_ingests_and_packs_as_the_model_in_each_of_its_modes(lib, shape, mode):
    """Ingest alone (io NULL), pack alone (st NULL), both; the pack half with the chunk's final_obs or terminal NULL as well."""
    T, B, N, D, R, R_in = shape
    mode, chunk_mode = (mode.split('-') + ['both'])[:2]
    R_out = R_in if (N, D) == (rr.WIDE_N, rr.WIDE_D) else R                 # small shapes: R_in != R_out
    cap, start = rr.packed_ring(R_in)
    ring = Ring(cap, N, D, 'plain')
    model = ring.model()
    rows_in = rr.packed_rows(_plain_model(N, D), T, B, N, D, R_in)
    obs0, out = rr.chunk('plain', T, B, N, D, **PACK_MODES[chunk_mode])
    sel_t, sel_e = rr.selection(T, B, R_out)
    d = {k: dev(v) for k, v in out.items()}
    d_t, d_e, d_rows_in = dev(sel_t), dev(sel_e), dev(rows_in)
    rows_out = guarded((R_out, 2 * N * D + N + 2), F32)
    io = _chunk_io(d)
    ingest, pack = mode != 'pack_only', mode != 'ingest_only'
    # the disabled half is switched off by ITS struct being NULL alone: its rows and counts are still given.  Ingest-only: the row
    # width comes from the ring, not from the N / D arguments
    _lib.check(lib.pw_exchange(ring.ref() if ingest else None, start, R_in, p(d_rows_in), C.byref(io) if pack else None, B, N if pack else 0,
                               D if pack else 0, p(d_t), p(d_e), R_out, p(rows_out), stream()))
    what = 'exchange %s %s (chunk: %s):' % (shape, mode, chunk_mode)
    if ingest:
        model.add_packed(start, rows_in)
    ring.check(model, what)                                  # pack-only: the ring stays as it was
    if pack:
        assert_same(host(rows_out), _plain_model(N, D).pack(out, out['act'], sel_t, sel_e), what + ' rows_out')
        assert_guards_intact(rows_out, what + ' rows_out')
    else:
        assert_untouched(rows_out, what + ' rows_out')


# ---- pw_counter_add -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('v,delta,modulo,want', [(5, 3, 0, 8), (8, 4, 10, 2), (999, 1, 1000, 0), (2 ** 40, 1, 0, 2 ** 40 + 1), (7, 331, 400, 338), (3, 5, -1, 8)])
def test_counter_add(lib, v, delta, modulo, want):
    assert rr.RingModel.counter_add(v, delta, modulo) == want
    c = cell(v)
    _lib.check(lib.pw_counter_add(p(c), delta, modulo, stream()))
    assert int(c.item()) == want
    assert_guards_intact(c, 'counter')
