"""A plain NumPy model of the device replay ring, and the inputs the ring tests run on.  NumPy only: no torch, no library, no stand-in.

``RingModel`` holds the five planes of ``pw_replay_store`` as arrays and has one method per operation of the ring's base layer.  Each
restates the CONTRACT -- include/pworld.h ("device replay ring", "multi-GPU exchange") and the reference's rls/replay_buffer.py
(``add`` overwrites at ``_next_idx`` modulo ``_maxsize``; ``_encode_sample`` stacks the stored tuples) -- as a loop over transitions,
not the kernels' flat index arithmetic.  Everything is a copy, an integer conversion or an index computation: copies keep bits, so the
tests compare through ``bits()`` (a uint32 view), never with ``==`` on floats (NaN, -0.0).

The second half are the input generators (``values`` ... ``selection``) and the case tables.  tests/test_gpu_replay_ring.py feeds
them to the library; tests/test_ring_ref_host.py shows, without a GPU, that on exactly these inputs a set of deliberately wrong models
gives other planes than this one -- so a kernel with one of those mistakes cannot pass.
"""
import numpy as np

# ---- ring kinds (pw_replay_store.act_heads / per_agent / head_width) -------------------------------------------------------------
KINDS = {
    'plain': dict(heads=1, per_agent=False, head_width=(5, 0)),
    'two_head': dict(heads=2, per_agent=False, head_width=(5, 10)),
    'per_agent': dict(heads=1, per_agent=True, head_width=(5, 0)),
    'per_agent_two_head': dict(heads=2, per_agent=True, head_width=(5, 10)),
}


def bits(a):
    """The array's 32-bit words (float32) or the array itself (integers): what 'equal' means for a copy."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


class RingModel(object):
    """obs / next_obs [cap,N,D] f32, act [cap,N] or [cap,N,2] u8, rew / done [cap] or [cap,N] f32 -- constructed from the planes'
    initial contents (copied), so slots no operation wrote stay comparable.  head_width = (W0, W1) sizes the one-hot rows of gather;
    W0 = 0 means 5 (the header's legacy value)."""

    def __init__(self, obs, next_obs, act, rew, done, head_width=(5, 0)):
        self.obs, self.next_obs = np.array(obs, dtype=np.float32), np.array(next_obs, dtype=np.float32)
        self.act, self.rew, self.done = np.array(act, dtype=np.uint8), np.array(rew, dtype=np.float32), np.array(done, dtype=np.float32)
        self.cap, self.N, self.D = self.obs.shape
        self.heads = 2 if self.act.ndim == 3 else 1
        self.per_agent = self.rew.ndim == 2
        assert self.next_obs.shape == self.obs.shape and self.act.shape[:2] == (self.cap, self.N)
        assert self.rew.shape == self.done.shape == ((self.cap, self.N) if self.per_agent else (self.cap,))
        self.head_width = (int(head_width[0]), int(head_width[1]))
        self.next_idx, self.len = 0, 0        # ReplayBuffer._next_idx / __len__, kept by add() alone (the golden anchor reads them)

    def planes(self):
        return dict(obs=self.obs, next_obs=self.next_obs, act=self.act, rew=self.rew, done=self.done)

    # -- where transition number k of a write that begins at `start` goes (rls/replay_buffer.py:32-36: _next_idx = (_next_idx + 1) % _maxsize)
    def slot(self, start, k):
        return (start + k) % self.cap

    # -- what one stored transition is made of; the writers below differ only in where they take the five parts from
    def store(self, slot, obs, act, rew, next_obs, done):
        self.obs[slot] = obs
        self.next_obs[slot] = next_obs
        self.act[slot] = np.asarray(act).astype(np.int64).astype(np.uint8)      # an index 0..255; [N] or [N,2]
        self.rew[slot] = rew                                                    # a scalar, or [N] for a per-agent ring
        self.done[slot] = done

    # -- pw_replay_add (and the ring half of pw_replay_add_tail): ReplayBuffer.add() of B transitions
    def add(self, start, obs, act, rew, next_obs, final_obs=None, terminal=None, done=None):
        B = obs.shape[0]
        for e in range(B):
            pre_reset = final_obs is not None and terminal is not None and bool(terminal[e])
            self.store(self.slot(start, e), obs[e], act[e], rew[e], final_obs[e] if pre_reset else next_obs[e],
                       np.float32(0.0) if done is None else done[e])
        self.next_idx, self.len = self.slot(start, B), min(self.len + B, self.cap)

    # -- pw_replay_add_rollout: a T-step chunk, in the order of T add() calls
    def add_rollout(self, start, obs0, out):
        """out: obs [T,B,N,D], terminal [T,B] u8, rew_shared [T,B], act [T,B,N(,2)] i32; optional final_obs [T,B,N,D], rew [T,B,N],
        done [T,B,N] u8 (None or absent = not given)."""
        T, B = out['obs'].shape[:2]
        final_obs, chunk_done = out.get('final_obs'), out.get('done')
        for t in range(T):
            acted_on = obs0 if t == 0 else out['obs'][t - 1]
            for e in range(B):
                pre_reset = final_obs is not None and bool(out['terminal'][t, e])
                if self.per_agent:
                    rew = out['rew'][t, e]
                    done = np.zeros(self.N, np.float32) if chunk_done is None else chunk_done[t, e].astype(np.float32)
                else:
                    rew, done = out['rew_shared'][t, e], np.float32(0.0)
                self.store(self.slot(start, t * B + e), acted_on[e], out['act'][t, e], rew,
                           final_obs[t, e] if pre_reset else out['obs'][t, e], done)

    # -- pw_pack_transitions: rows [obs N*D | next_obs N*D | act N | rew | 0] of the selected transitions (t >= 1)
    def pack(self, out, act, sel_t, sel_e):
        N, D = out['obs'].shape[2:]
        final_obs, terminal = out.get('final_obs'), out.get('terminal')
        rows = np.zeros((len(sel_t), 2 * N * D + N + 2), np.float32)
        for r, (t, e) in enumerate(zip(sel_t, sel_e)):
            assert t >= 1
            pre_reset = final_obs is not None and terminal is not None and bool(terminal[t, e])
            rows[r, :N * D] = out['obs'][t - 1, e].reshape(-1)
            rows[r, N * D:2 * N * D] = (final_obs if pre_reset else out['obs'])[t, e].reshape(-1)
            rows[r, 2 * N * D:2 * N * D + N] = act[t, e].astype(np.float32)
            rows[r, 2 * N * D + N] = out['rew_shared'][t, e]
            rows[r, 2 * N * D + N + 1] = 0.0             # done: the reference's done_callback is None
        return rows

    # -- pw_replay_add_packed: ReplayBuffer.add() of R received rows (a plain ring)
    def add_packed(self, start, rows):
        N, D = self.N, self.D
        assert self.heads == 1 and not self.per_agent and rows.shape[1] == 2 * N * D + N + 2
        for r in range(rows.shape[0]):
            row = rows[r]
            self.store(self.slot(start, r), row[:N * D].reshape(N, D), row[2 * N * D:2 * N * D + N], row[2 * N * D + N],
                       row[N * D:2 * N * D].reshape(N, D), row[2 * N * D + N + 1])

    # -- the one-hot rows a gather returns for one stored agent action: [head 0 | head 1]; an index outside its head selects no column
    def one_hot(self, stored):
        W0 = self.head_width[0] if self.head_width[0] > 0 else 5
        W1 = self.head_width[1] if self.heads == 2 else 0
        row = np.zeros(W0 + W1, np.float32)
        a0 = int(stored[0]) if self.heads == 2 else int(stored)
        if a0 < W0:
            row[a0] = 1.0
        if self.heads == 2 and int(stored[1]) < W1:
            row[W0 + int(stored[1])] = 1.0
        return row

    # -- pw_replay_gather: sample_index() / _encode_sample()
    def gather(self, idx):
        idx = [int(i) for i in idx]
        assert all(0 <= i < self.cap for i in idx)
        act = np.stack([np.stack([self.one_hot(self.act[i, a]) for a in range(self.N)]) for i in idx])
        return (np.stack([self.obs[i] for i in idx]), act, np.stack([self.rew[i] for i in idx]),
                np.stack([self.next_obs[i] for i in idx]), np.stack([self.done[i] for i in idx]))

    # -- pw_counter_add
    @staticmethod
    def counter_add(v, delta, modulo):
        v = v + delta
        return v % modulo if modulo > 0 else v


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
SPECIALS = (0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC12345, 0x807FFFFF)   # -0.0, a subnormal, +inf, -inf, a NaN with a payload, the largest negative subnormal


def values(shape, salt):
    """float32 [shape]: element i is 2^(salt - 8) * (1 + i / 2^23) -- a distinct function of its flat index, and of the salt (one
    binade per salt, so two tensors of a case share no value) -- with a handful overwritten by SPECIALS at positions that move with
    the salt."""
    n = int(np.prod(shape))
    assert 0 <= salt < 64 and n < (1 << 23)
    word = (np.uint32(119 + salt) << np.uint32(23)) | np.arange(n, dtype=np.uint32)
    for k, s in enumerate(SPECIALS):
        word[((2 * k + 1) * n // 12 + salt) % n] = s
    return word.view(np.float32).reshape(shape)


def actions(shape, widths):
    """int32 [shape] ([shape, 2] for two widths): indices inside their head, a function of the flat index that differs between the
    heads and covers each head; the LAST element holds each head's last index (a gather of one slot still tells the heads apart)."""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    heads = [(w - 1 - ((n - 1 - i) * m) % w).astype(np.int32).reshape(shape) for w, m in zip(widths, (3, 7))]
    return heads[0] if len(widths) == 1 else np.stack(heads, axis=-1)


def terminal_mask(shape):
    """uint8 [B] or [T,B]: the first and the last env set (every step), a mix between that moves from step to step."""
    B = shape[-1]
    lead = int(np.prod(shape[:-1]))
    m = np.zeros((lead, B), np.uint8)
    for t in range(lead):
        m[t] = ((np.arange(B) + t) % 3 == 1)
        m[t, 0] = m[t, B - 1] = 1
    return m.reshape(shape)


def done_bytes(shape):
    """uint8 [shape]: a chunk's `done` with non-zero values (0, 1, 255 and others)."""
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((i * 37 + 1) % 256).astype(np.uint8).reshape(shape)


def initial_planes(cap, N, D, kind, salt=40):
    """What a ring holds before the operation under test (CPU tests; the GPU tests read the device planes' bytes back instead)."""
    k = KINDS[kind]
    rs = (cap, N) if k['per_agent'] else (cap,)
    i = np.arange(cap * N * k['heads'], dtype=np.int64)
    act = (101 + i * 13 % 150).astype(np.uint8).reshape((cap, N, 2) if k['heads'] == 2 else (cap, N))     # 101..250: outside every head
    return dict(obs=values((cap, N, D), salt), next_obs=values((cap, N, D), salt + 1), act=act, rew=values(rs, salt + 2), done=values(rs, salt + 3))


def model_from(planes, kind, head_width=None):
    return RingModel(planes['obs'], planes['next_obs'], planes['act'], planes['rew'], planes['done'],
                     KINDS[kind]['head_width'] if head_width is None else head_width)


def ring_contents(cap, N, D, kind, head_width=None):
    """A full ring for the gather tests: distinct observations, rewards and done flags, action indices inside their head."""
    k = KINDS[kind]
    hw = k['head_width'] if head_width is None else head_width
    p = initial_planes(cap, N, D, kind, salt=20)
    widths = [hw[0] if hw[0] > 0 else 5] + ([hw[1]] if k['heads'] == 2 else [])
    p['act'] = actions((cap, N), widths).astype(np.uint8)
    return p


def add_inputs(kind, N, D, B, final='both', done=True):
    """The arguments of one pw_replay_add.  final: 'both', 'final_obs' (terminal NULL), 'terminal' (final_obs NULL) or 'neither'."""
    k = KINDS[kind]
    rs = (B, N) if k['per_agent'] else (B,)
    return dict(obs=values((B, N, D), 0), next_obs=values((B, N, D), 1), act=actions((B, N), k['head_width'][:k['heads']]),
                rew=values(rs, 3), final_obs=values((B, N, D), 2) if final in ('both', 'final_obs') else None,
                terminal=terminal_mask((B,)) if final in ('both', 'terminal') else None, done=values(rs, 4) if done else None)


def chunk(kind, T, B, N, D, final=True, done='nonzero', terminal=True):
    """obs0 and the output tensors of a T-step rollout chunk -- synthetic: the ring's writers copy.  done: None or 'nonzero'."""
    k = KINDS[kind]
    out = dict(obs=values((T, B, N, D), 5), rew_shared=values((T, B), 8), rew=values((T, B, N), 9),
               act=actions((T, B, N), k['head_width'][:k['heads']]))
    out['final_obs'] = values((T, B, N, D), 6) if final else None
    out['terminal'] = terminal_mask((T, B)) if terminal else None
    out['done'] = done_bytes((T, B, N)) if done == 'nonzero' else None
    return values((B, N, D), 7), out


def selection(T, B, R):
    """sel_t, sel_e int32 [R] for pw_pack_transitions: t = 1 and t = T-1, e = 0 and e = B-1, a repeated (t, e); never t = 0."""
    assert T >= 2 and R >= 5
    base = [(1, 0), (T - 1, B - 1), (1, B - 1), (T - 1, 0), (1, 0)]
    r = np.arange(R - len(base), dtype=np.int64)
    sel_t = np.array([t for t, _ in base] + list(1 + (r * 5 + 2) % (T - 1)), np.int32)
    sel_e = np.array([e for _, e in base] + list((r * 7 + 3) % B), np.int32)
    assert sel_t.min() >= 1 and sel_t.max() == T - 1
    return sel_t, sel_e


def packed_ring(R):
    """(cap, start) of the ring R packed rows go into: it wraps."""
    return R + 3, R - 2


def packed_rows(model, T, B, N, D, R):
    """R received rows: the model's pack of the chunk, with the done column set to non-zero values."""
    obs0, out = chunk('plain', T, B, N, D)
    rows = model.pack(out, out['act'], *selection(T, B, R))
    rows[:, -1] = values((R,), 10)
    return rows


def gather_index(cap, b):
    """int64 [b]: cap-1 and 0 (each twice: repeats), a descending run from cap-1, then a spread; the first b of that."""
    run = [cap - 1 - j for j in range(min(cap, 6))]
    spread = [(j * 7919 + 13) % cap for j in range(b)]
    return np.array(([cap - 1, 0, 0, cap - 1] + run + spread)[:b], np.int64)


# ---- the cases the GPU tests run, and the CPU test checks for discrimination -----------------------------------------------------------
WIDE_N, WIDE_D = 64, 104                                  # N*D = 6656: with the sizes below every grid-stride loop takes its second trip
ADD_SHAPES = ((10, 2, 6, 4, 8), (7, 1, 2, 7, 3), (1000, 3, 10, 257, 900))            # (cap, N, D, B, start)
ADD_WIDE = (400, WIDE_N, WIDE_D, 331, 390)                                             # 331 * 6656 = 2 203 136 > 8192 * 256
TAIL_SHAPES = ((10, 1, 5, 10, 7), ADD_WIDE)
ROLLOUT_SHAPES = ((1, 0, 1, 1, 1, 5), (12, 5, 3, 4, 2, 6), (1000, 900, 9, 33, 3, 10))   # (cap, start, T, B, N, D); the second: T*B = cap and a wrap
ROLLOUT_WIDE = (700, 690, 5, 130, WIDE_N, WIDE_D)                                       # 650 * 6656 = 4 326 400 > 16384 * 256
GATHER_RINGS = ((10, 2, 6), (7, 1, 2), (1000, 3, 10))                                   # (cap, N, D)
GATHER_BATCHES = (1, 5, 257)
GATHER_WIDE = (400, WIDE_N, WIDE_D, 331)
PACK_SHAPES = ((4, 5, 1, 2, 9, 6), (4, 5, 3, 10, 9, 6), (3, 8, WIDE_N, WIDE_D, 80, 40))  # (T, B, N, D, R of pack / add_packed, R_in of exchange); 80 * 13378 = 1 070 240 > 4096 * 256
