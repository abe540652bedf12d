"""Pins oracle/actor_oracle.py, the float64 host reference the GPU actor tests compare with: its vectorised Philox
against the two scalar forms and Random123's answers, the block tags, the Gumbel uniform over every 24-bit word, the
sampler's distribution, and the float64 network against PyTorch's float32 one."""
import numpy as np
import pytest

from oracle import actor_oracle as ao
from oracle import c_oracle as co
from oracle import particle_oracle as po

torch = pytest.importorskip('torch')


def test_vector_philox_reproduces_random123_answers():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = ao.philox4x32_10(*ctr, *key)
        assert tuple(int(w) for w in got) == want


def test_vector_philox_equals_the_scalar_forms_on_tagged_wide_counters():
    """Rows >= 2^32, steps >= 2^32, seeds >= 2^32 and the tag bits of every block, through gumbel_words."""
    rng = np.random.RandomState(3)
    rows = np.concatenate([rng.randint(0, 1 << 20, 6), (1 << 32) + rng.randint(0, 1 << 20, 3), [(1 << 40) + 7]])
    for seed, step in [(0, 0), (9, 1), (2 ** 32 + 5, 2 ** 32 + 3), (0xfedcba9876543210, 0xffffffffffff)]:
        w = ao.gumbel_words(seed, step, rows, 16)
        for i, r in enumerate(rows.tolist()):
            for blk in range(4):
                tag = ((blk & 1) << 31) | ((blk >> 1) << 30)
                ctr = (r & 0xffffffff, (r >> 32) | tag, step & 0xffffffff, step >> 32)
                key = (seed & 0xffffffff, seed >> 32)
                want = po.philox4x32_10(ctr, key)
                assert co.philox4x32_10(ctr, key) == want
                assert tuple(int(x) for x in w[i, 4 * blk:4 * blk + 4]) == want, (seed, step, r, blk)


def test_block_tags_give_distinct_counters():
    tags = [int(ao.block_tag(b)) for b in range(4)]
    assert tags == [0, 0x80000000, 0x40000000, 0xC0000000]
    # below the tag bits (rows < 2^62) no two blocks of any row share a counter word 1
    r = np.array([0, 1, 5, (1 << 30) - 1], dtype=np.uint64)
    c1 = {(int(x) | t) for x in (r >> np.uint64(32)).tolist() for t in tags}
    assert len(c1) == 4
    w = ao.gumbel_words(7, 0, [3], 16)[0]
    assert len({tuple(w[4 * b:4 * b + 4].tolist()) for b in range(4)}) == 4


def test_uniform_lies_strictly_inside_the_unit_interval_for_every_word():
    words = np.arange(1 << 24, dtype=np.uint64) << np.uint64(8)
    u = ao.uniform_f32(words)
    assert u.dtype == np.float32
    assert (u > 0).all() and (u < 1).all()
    old = ao.uniform_f32_unclamped(words)
    assert old[-1] == np.float32(1.0)                       # the defect: 16777215.5f rounds half-to-even to 2^24
    assert np.array_equal(u[:-1], old[:-1])                  # every other word keeps its value
    assert u[-1] == ao.U_MAX and u[-1].view(np.uint32) == 0x3f7fffff
    assert np.isfinite(np.log(-np.log(u.astype(np.float64)))).all()
    assert np.all(np.diff(u) >= 0)


def test_top_word_seed_search():
    seed, q = ao.find_top_word_seed(5, 0, start=2 ** 32)
    w = ao.gumbel_words(seed, 0, [5], 4)[0]
    assert int(w[q]) >> 8 == ao.TOP_WORD
    assert ao.uniform_f32(w[q]) == ao.U_MAX


@pytest.mark.parametrize('heads', [(5,), (5, 10), (7, 9)])
def test_sampler_reproduces_softmax(heads):
    """10^6 draws (one row each, step fixed) of fixed logits: frequencies within 2e-3 of softmax per class; two heads
    draw independently (joint frequencies = product of the marginals)."""
    rng = np.random.RandomState(sum(heads))
    logits = rng.randn(sum(heads)) * 1.5
    R = 10 ** 6
    act, margin = ao.predict(np.broadcast_to(logits, (R, sum(heads))), 2 ** 32 + 11, 17, np.arange(R), heads)
    assert act.shape == (R, len(heads)) and (margin > 0).all()
    lo = 0
    for h, n in enumerate(heads):
        p = np.exp(logits[lo:lo + n] - logits[lo:lo + n].max())
        p /= p.sum()
        f = np.bincount(act[:, h], minlength=n) / R
        assert np.abs(f - p).max() < 2e-3, (heads, h, f, p)
        lo += n
    if len(heads) == 2:
        n0, n1 = heads
        joint = np.bincount(act[:, 0] * n1 + act[:, 1], minlength=n0 * n1).reshape(n0, n1) / R
        prod = np.outer(np.bincount(act[:, 0], minlength=n0), np.bincount(act[:, 1], minlength=n1)) / R ** 2
        assert np.abs(joint - prod).max() < 2e-3


def test_predict_is_first_maximum_and_margin():
    lg = np.zeros((4, 6))
    act, margin = ao.predict(lg, 1, 0, np.arange(4), (5, 1))
    noise = ao.gumbel_noise(1, 0, np.arange(4), 6)
    assert np.array_equal(act[:, 0], np.argmax(-noise[:, :5], 1))
    assert (act[:, 1] == 0).all() and np.isinf(margin[:, 1]).all()


@pytest.mark.parametrize('D,heads,N', [(16, 5, 6), (21, [5, 10], 2), (9, [7, 9], 13), (64, [1, 15], 31), (1, 16, 1)])
def test_forward_f64_agrees_with_pytorch_float32(D, heads, N):
    from multiagent_rl_amd.policy import ActorNetwork
    torch.manual_seed(D + N)
    net = ActorNetwork(D, heads).eval()
    obs = torch.randn(7, N, D) * 2
    with torch.no_grad():
        want = net(obs)
        hid = torch.relu(net.bilstm(torch.relu(net.dense1(obs)))[0])
    want = want if isinstance(want, list) else [want]
    H, lg = ao.forward_f64(net, obs.numpy())
    np.testing.assert_allclose(H, hid.numpy(), rtol=0, atol=1e-5)
    assert len(lg) == len(want)
    for a, b in zip(lg, want):
        np.testing.assert_allclose(a, b.numpy(), rtol=0, atol=1e-5)
