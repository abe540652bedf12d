"""Float64 host reference of the actor and of its Gumbel sampling (test infrastructure; the product never imports it).

``forward_f64`` restates ``multiagent_rl_amd.policy.ActorNetwork`` (rls/model/ac_network_multi_gumbel.py:52-67):
H = relu(BiLSTM(relu(dense1(x)))) over the agent axis, then one or two linear heads, all in float64 NumPy.

The sampler restates the device's draw exactly: logit o of global row r (= env * N + agent) at Philox step s uses word
(o & 3) of Philox4x32-10 block (o >> 2), keyed

    counter = (r lo32, r hi32 | tag(blk), s lo32, s hi32),  key = (seed lo32, seed hi32),
    tag(blk) = ((blk & 1) << 31) | ((blk >> 1) << 30),

the logits of both heads concatenated [n_out0 | n_out1].  The uniform is formed in float32 as the device forms it
(``pw_gumbel_uniform``: (w >> 8) + 0.5, times 2^-24, clamped below 1); the noise log(-log u) is taken in float64, and the
action of a head is the first maximum of logit - noise.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
U_MAX = np.float32(np.nextafter(np.float32(1.0), np.float32(0.0)))   # 0x1.fffffep-1
TOP_WORD = (1 << 24) - 1                                             # w >> 8 of the word whose unclamped uniform is 1.0


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 (Salmon et al., SC'11): uint32-valued arrays (broadcast together) -> 4 uint64 arrays
    holding 32-bit words.  The 32 x 32 -> 64 products are exact in uint64."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK for v in (c0, c1, c2, c3, k0, k1))
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(c0, c1, c2, c3, k0, k1)
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
        k0 = (k0 + _W0) & _MASK
        k1 = (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def block_tag(blk):
    blk = np.asarray(blk, dtype=np.uint64)
    return ((blk & np.uint64(1)) << np.uint64(31)) | ((blk >> np.uint64(1)) << np.uint64(30))


def gumbel_words(seed, step, rows, n_out):
    """-> uint64 [len(rows), n_out]: the Philox word of every (row, logit).  ``step`` is a scalar or one per row."""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    step = np.broadcast_to(np.asarray(step, dtype=np.uint64), rows.shape)
    seed = int(seed)
    nb = (int(n_out) + 3) // 4
    out = np.empty((rows.size, 4 * nb), dtype=np.uint64)
    for b in range(nb):
        w = philox4x32_10(rows & _MASK, (rows >> _S32) | block_tag(b), step & _MASK, step >> _S32,
                          seed & 0xFFFFFFFF, seed >> 32)
        for q in range(4):
            out[:, 4 * b + q] = w[q]
    return out[:, :n_out]


def uniform_f32(words):
    """The device's uniform of a word, float32 operation for operation: min(((w >> 8) + 0.5f) * 2^-24f, 0x1.fffffep-1f)."""
    top = (np.asarray(words, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)    # < 2^24: exact
    u = (top + np.float32(0.5)) * np.float32(2.0 ** -24)
    return np.minimum(u, U_MAX)


def uniform_f32_unclamped(words):
    """The form before the clamp (the word 2^24 - 1 gives exactly 1.0)."""
    top = (np.asarray(words, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)
    return (top + np.float32(0.5)) * np.float32(2.0 ** -24)


def gumbel_noise(seed, step, rows, n_out):
    """log(-log u) in float64, [len(rows), n_out]; the perturbed logit is logit - noise."""
    u = uniform_f32(gumbel_words(seed, step, rows, n_out)).astype(np.float64)
    return np.log(-np.log(u))


def predict(logits64, seed, step, rows, heads):
    """logits64 [R, sum(heads)] (float64) -> (act int64 [R, len(heads)], margin float64 [R, len(heads)]).
    act = first maximum of logits - noise per head; margin = best perturbed value - the runner-up (inf for a 1-logit head)."""
    logits64 = np.asarray(logits64, dtype=np.float64)
    R, out = logits64.shape
    assert out == sum(heads)
    v = logits64 - gumbel_noise(seed, step, rows, out)
    acts, margins, lo = [], [], 0
    for n in heads:
        vh = v[:, lo:lo + n]
        a = np.argmax(vh, axis=1)
        if n > 1:
            top2 = np.sort(vh, axis=1)[:, -2:]
            m = top2[:, 1] - top2[:, 0]
        else:
            m = np.full(R, np.inf)
        acts.append(a)
        margins.append(m)
        lo += n
    return np.stack(acts, 1), np.stack(margins, 1)


def find_top_word_seed(row, step, start=0, chunk=1 << 20, limit=1 << 28):
    """Smallest seed >= start whose Philox block 0 at (row, step) holds a word with w >> 8 == 2^24 - 1.
    -> (seed, word index q): logit q of that row draws the top word."""
    row, step = int(row), int(step)
    for s0 in range(int(start), int(start) + limit, chunk):
        seeds = np.arange(s0, s0 + chunk, dtype=np.uint64)
        w = philox4x32_10(row & 0xFFFFFFFF, row >> 32, step & 0xFFFFFFFF, step >> 32, seeds & _MASK, seeds >> _S32)
        hits = [(int(i[0]), q) for q, i in enumerate(np.nonzero((wq >> np.uint64(8)) == np.uint64(TOP_WORD))[0] for wq in w)
                if i.size]
        if hits:
            i, q = min(hits)
            return s0 + i, q
    raise RuntimeError('no seed found')


# ------------------------------------------------------------------ the network
def actor_params(actor):
    """ActorNetwork -> dict of float64 NumPy arrays (weights as the module holds them, whatever device)."""
    g = lambda t: t.detach().cpu().double().numpy()  # noqa: E731
    lstm = actor.bilstm
    two = type(actor.out_dim) is list
    heads = [actor.dense2_1.module, actor.dense2_2.module] if two else [actor.dense2.module]
    return dict(w1=g(actor.dense1.module.weight), b1=g(actor.dense1.module.bias),
                wih=(g(lstm.weight_ih_l0), g(lstm.weight_ih_l0_reverse)),
                whh=(g(lstm.weight_hh_l0), g(lstm.weight_hh_l0_reverse)),
                b=(g(lstm.bias_ih_l0) + g(lstm.bias_hh_l0), g(lstm.bias_ih_l0_reverse) + g(lstm.bias_hh_l0_reverse)),
                w2=[g(h.weight) for h in heads], b2=[g(h.bias) for h in heads])


def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def forward_f64(actor, obs):
    """obs [B, N, D] -> (H [B, N, 64], [logits [B, N, n] per head]), float64.  PyTorch's LSTM: gates (i, f, g, o),
    c' = f c + i g, h' = o tanh(c'); the reverse direction runs agent N-1 .. 0; H = relu([h_fwd | h_rev])."""
    P = actor_params(actor) if not isinstance(actor, dict) else actor
    x = np.asarray(obs, dtype=np.float64)
    B, N, _ = x.shape
    x1 = np.maximum(x @ P['w1'].T + P['b1'], 0.0)
    hs = []
    for d in range(2):
        g_in = x1 @ P['wih'][d].T + P['b'][d]          # [B, N, 128]
        h = np.zeros((B, 32))
        c = np.zeros((B, 32))
        out = np.zeros((B, N, 32))
        for t in (range(N) if d == 0 else range(N - 1, -1, -1)):
            g = g_in[:, t] + h @ P['whh'][d].T
            i, f, gg, o = _sigmoid(g[:, :32]), _sigmoid(g[:, 32:64]), np.tanh(g[:, 64:96]), _sigmoid(g[:, 96:])
            c = f * c + i * gg
            h = o * np.tanh(c)
            out[:, t] = h
        hs.append(out)
    H = np.maximum(np.concatenate(hs, -1), 0.0)
    return H, [H @ w.T + b for w, b in zip(P['w2'], P['b2'])]
