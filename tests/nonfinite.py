"""Non-finite inputs of the network kernels: where the poison goes, the inputs it goes into, and the three things the tests ask of the
result (tests/test_nonfinite_host.py checks the float64 restatements with them, tests/test_gpu_nonfinite.py the kernels).

A NaN observation is a real input: two coincident agents give 0 / 0 in the environment, the rollout writes that row into the ring and the
learner samples it.  What a network kernel owes such a row:

(M) mask       ``~isfinite`` of every output equals ``~isfinite`` of the float64 restatement's, elementwise (NaN and +-Inf both count;
               the VALUES inside a poisoned row are not compared: float32 and float64 may differ in NaN against Inf there, and the
               backward masks of a ReLU at a NaN are F.relu's in one and clamp_min's in the other);
(I) isolation  every row-local output of every clean row has the bits of the same launch on the clean inputs -- the kernels pack 16
               rows into one matrix tile and park idle slots on row 0, so one ``0 * NaN`` in a padding or select trick would show here;
(R) range      an action index of a poisoned row lies in [0, n): which one is not pinned (NumPy's arg-max picks the NaN).

The poisoned rows of a batch of ``b``: row 0 (the row idle slots alias), a row in the middle of a tile, the last row; ``b`` is chosen so
that the last workgroup has idle slots.  Every builder computes its inputs once and leaves them unchanged (``poisoned`` copies).
"""
import functools

import numpy as np
import torch

NAN, INF = float('nan'), float('inf')
TILE = 16                                    # rows of one matrix tile in every network kernel


def rows_to_poison(b):
    """Row 0, a row in the middle of a tile (of the second tile where there is one), the last row."""
    mid = TILE + TILE // 2 - 1 if b > 2 * TILE else b // 2
    assert 0 < mid < b - 1
    return (0, mid, b - 1)


def poisoned(t, index, value=NAN):
    """A copy of tensor / array ``t`` with ``t[index] = value``."""
    out = t.clone() if isinstance(t, torch.Tensor) else np.array(t, copy=True)
    out[index] = value
    return out


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def nonfinite(t):
    return ~np.isfinite(_np(t))


def assert_same_mask(got, ref, what):
    """(M)"""
    g, r = nonfinite(got), nonfinite(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = np.argwhere(g != r)
    assert bad.size == 0, '%s: non-finite mask differs from the float64 reference at %d of %d entries (%d non-finite here, %d there), ' \
        'first %s: %r here' % (what, len(bad), g.size, int(g.sum()), int(r.sum()), tuple(bad[0]), _np(got)[tuple(bad[0])])


def assert_clean_rows_same_bits(got, clean, bad_rows, what, axis=0):
    """(I): along ``axis``, every index outside ``bad_rows`` holds the bits of ``clean``."""
    g, c = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(clean))
    assert g.shape == c.shape and g.dtype == c.dtype, (what, g.shape, c.shape)
    keep = np.setdiff1d(np.arange(g.shape[axis]), np.asarray(bad_rows))
    assert keep.size > 0
    g, c = np.take(g, keep, axis), np.take(c, keep, axis)
    if g.dtype == np.float32:
        g, c = g.view(np.int32), c.view(np.int32)
    bad = np.argwhere(g != c)
    assert bad.size == 0, '%s: %d entries of clean rows differ from the launch on clean inputs, first at clean row %d (%s)' % (
        what, len(bad), int(keep[bad[0][axis]]), tuple(bad[0]))
    assert np.isfinite(np.take(_np(clean), keep, axis)).all(), what


def assert_in_range(idx, n, what):
    """(R)"""
    a = _np(idx)
    assert a.size and a.min() >= 0 and a.max() < n, (what, int(a.min()), int(a.max()), n)


def rows_with(mask, axis=0):
    """The indices along ``axis`` that hold a True somewhere."""
    m = np.asarray(mask)
    other = tuple(i for i in range(m.ndim) if i != axis)
    return np.nonzero(m.any(axis=other))[0] if other else np.nonzero(m)[0]


# ---- the dense front ---------------------------------------------------------------------------------------------------------------
DENSE_ROWS = 35                              # two full tiles and a ragged one
DENSE_SHAPES = ((16, 5, 1), (21, 15, 2))     # (d0, d1, dirs)
DENSE_NAMES = ('x0', 'x1', 'w1', 'b1', 'w_ih', 'b_ih', 'b_hh')


@functools.lru_cache(maxsize=None)
def dense_inputs(d0, d1, dirs):
    """-> (dict of float32 CPU tensors as dense_ref.forward takes them, dG float32 [rows,256])."""
    from tests import dense_ref
    inp = dense_ref.make_inputs(DENSE_ROWS, d0, d1, dirs)
    dG = torch.randn(DENSE_ROWS, 256, generator=torch.Generator().manual_seed(d0 + dirs))
    return {k: inp[k] for k in DENSE_NAMES}, dG


def dense_poisons(d0, d1):
    """(which input, column): one observation column, the last action column."""
    return (('x0', 3), ('x1', d1 - 1))


def dense_f64(inp):
    f = lambda t: None if t is None else t.double()  # noqa: E731
    return {k: (tuple(f(t) for t in v) if isinstance(v, tuple) else f(v)) for k, v in inp.items()}


# ---- the LSTM recurrence -----------------------------------------------------------------------------------------------------------
LSTM_B, LSTM_N = 5, 3
LSTM_SHAPES = ((1, 64), (2, 32))             # (dirs, H)
LSTM_POISON = (1, 0, 7)                      # (step, direction, gate column): the input gate of unit 7 at step 1 of direction 0


@functools.lru_cache(maxsize=None)
def lstm_inputs(dirs, H):
    """-> (G [b,N,dirs,4H], w_hh_fw, w_hh_bw or None, dY [b,N,dirs*H]), float32 on the CPU."""
    from tests import lstm_ref
    net = lstm_ref.make_lstm(dirs, H, torch.float32)
    g = torch.Generator().manual_seed(10 * dirs + H)
    G = torch.randn(LSTM_B, LSTM_N, dirs, 4 * H, generator=g)
    dY = torch.randn(LSTM_B, LSTM_N, dirs * H, generator=g)
    w_bw = net.weight_hh_l0_reverse.detach().clone() if dirs == 2 else None
    return G, net.weight_hh_l0.detach().clone(), w_bw, dY


# ---- attention pooling -------------------------------------------------------------------------------------------------------------
ATTENTION_SHAPES = ((5, 3), (6, 64))         # (b, N)
ATTENTION_COLUMN = 7


def attention_inputs(b, N):
    from tests import attention_ref
    return attention_ref.make_inputs(b, N, torch.float32)      # Y [b,N,64], dOut [b,64]


def attention_poisons(N):
    """The step of the poisoned element: one that is not the query, and the query (the last step)."""
    return (0, N - 1)


# ---- the Gumbel sample -------------------------------------------------------------------------------------------------------------
SAMPLE_ROWS, SAMPLE_WIDTHS, SAMPLE_SEED, SAMPLE_STEP, SAMPLE_TAU = 5, (5, 15), 77, 3, 0.5


@functools.lru_cache(maxsize=None)
def sample_inputs(n):
    """-> (logits [rows,n], dY [rows,n]) float32 on the CPU."""
    g = torch.Generator().manual_seed(n)
    return 2 * torch.randn(SAMPLE_ROWS, n, generator=g), torch.randn(SAMPLE_ROWS, n, generator=g)


# ---- the no-gradient critics -------------------------------------------------------------------------------------------------------
CRITIC_B, CRITIC_N, CRITIC_D, CRITIC_A, CRITIC_GAMMA = 5, 3, 16, 5, 0.95
CRITIC_FORMS = ('attention', 'bicnet', 'model')
CRITIC_POISON = (1, 3)                       # (agent, observation column): the per-step critic's mask starts at agent 1


def critic_net(form, seed=5):
    from multiagent_rl_amd import critic as cr
    torch.manual_seed(seed)
    cls = dict(attention=cr.CriticNetwork, bicnet=cr.BiCNetCritic, model=cr.ModelCriticNetwork)[form]
    return cls(CRITIC_D + CRITIC_A, 1).eval()


@functools.lru_cache(maxsize=None)
def critic_inputs(form):
    """-> obs, next_obs float32 [b,N,D], act int32 [b,N], rew, done float32 ([b], the per-step critic: [b,N]); NumPy."""
    rng = np.random.RandomState(len(form))
    b, N = CRITIC_B, CRITIC_N
    shape = (b, N) if form == 'bicnet' else (b,)
    return dict(obs=rng.randn(b, N, CRITIC_D).astype(np.float32), next_obs=rng.randn(b, N, CRITIC_D).astype(np.float32),
                act=rng.randint(0, CRITIC_A, (b, N)).astype(np.int32), rew=rng.randn(*shape).astype(np.float32),
                done=(rng.rand(*shape) < 0.4).astype(np.float32))


def critic_f64(form, net, obs, act_idx):
    """-> dict of the float64 outputs of the form: q ([b], per step [b,N]) and, for the model form, r."""
    from tests import bicnet_ref, critic_ref, model_ref
    act = critic_ref.one_hot(act_idx, (CRITIC_A,))
    if form == 'attention':
        return dict(q=critic_ref.forward_f64(net, obs, act))
    if form == 'bicnet':
        return dict(q=bicnet_ref.forward_f64(net, obs, act))
    q, r = model_ref.critic_f64(net, obs, act)
    return dict(q=q, r=r)


# ---- the actor ---------------------------------------------------------------------------------------------------------------------
ACTOR_B, ACTOR_N, ACTOR_LOGITS = 19, 3, 5
ACTOR_ENVS = (5, 17)                         # the first workgroup; the ragged second one (19 = 16 + 3)
ACTOR_POISON = (1, 3)                        # (agent, observation column)
ACTOR_FORMS = {'actor16': 16, 'chain': 16, 'wide': 70, 'bf16x3': 16}     # form -> D


@functools.lru_cache(maxsize=None)
def actor_obs(D):
    return (np.random.RandomState(D).randn(ACTOR_B, ACTOR_N, D) * 2).astype(np.float32)
