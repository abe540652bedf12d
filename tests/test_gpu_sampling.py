"""GPU: pw_gumbel_st_forward / pw_gumbel_st_backward and their Python surface (multiagent_rl_amd.sampling: gumbel_st, GumbelSampler, the
example learner's fused_sampling switch).

References.  The noise and the sampled index: oracle/actor_oracle.py (gumbel_noise / predict, the float64 restatement of the device's
Philox draw).  The forward: a float64 softmax of the device's own perturbed logits.  The backward: the float64 formula on the device's
own soft sample, and float64 autograd of F.gumbel_softmax's own lines (tests/sampling_ref.py stock) fed the device's noise.

Bounds (each stated where it is used):
  * idx: equal to the float64 prediction wherever the float64 margin exceeds MARGIN = 1e-4 (tests/test_gpu_actor_reference.py's figure for
    this noise function); at most 0.1 % of the rows may be left out (the oracle alone leaves out at most 0.02 % at these shapes and seeds);
  * noise: |device - float64| <= 1e-4;
  * soft: rtol 5e-5, atol 1e-7 -- one rounding in logit - noise and one in v - max at magnitude <= 64 (ulp 7.6e-6); tau = 1 and 0.5
    divide exactly;
  * y: bit-identical to (onehot(idx) - soft) + soft recomputed in float32 from the launch's own soft and idx; hard=False: y is soft;
  * dLogits against the float64 formula: 5e-6 max|dY| / tau (a 16-term ordered sum); against float64 autograd of the stock
    expression: 2e-4 max|dY| / tau (the forward's error in soft rides along);
  * 20 000 draws of one row: |freq - softmax| < 0.015 per class (test_fused_gumbel_sampling_distribution's bound).
"""
import copy
import functools

import numpy as np
import pytest
import torch

from oracle import actor_oracle as ao
from tests import sampling_ref

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
ROWS = (1, 257, 6144)
WIDTHS = (1, 3, 4, 5, 10, 16)
KEYS = ((7, 0), (7, 16), (2 ** 33 + 5, 2 ** 32 + 3))
TAUS = (1.0, 0.5)


@functools.lru_cache(maxsize=None)
def _logits(rows, n):
    g = torch.Generator().manual_seed(1000 * n + rows)
    return 2 * torch.randn(rows, n, generator=g)


@functools.lru_cache(maxsize=None)
def _oracle(rows, n, seed, step):
    """-> (noise float64 [rows,n], predicted idx [rows], float64 margin [rows]); computed once per case and left unchanged."""
    noise = ao.gumbel_noise(seed, step, np.arange(rows), n)
    act, margin = ao.predict(_logits(rows, n).double().numpy(), seed, step, np.arange(rows), (n,))
    return noise, act[:, 0], margin[:, 0]


def _forward(rows, n, seed, step, tau, hard=True, cell=None):
    from multiagent_rl_amd import sampling
    x = _logits(rows, n).cuda()
    y, soft, idx, noise = sampling.launch_forward(x, tau, hard, seed, step, cell, True, want_idx=True, want_noise=True)
    return x, y, soft, idx, noise


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize('seed,step', KEYS, ids=['s7_t0', 's7_t16', 's2p33_t2p32'])
@pytest.mark.parametrize('n', WIDTHS)
def test_keying_follows_the_oracle(n, seed, step):
    for rows in ROWS:
        want_noise, want_idx, margin = _oracle(rows, n, seed, step)
        for tau in TAUS:
            x, y, soft, idx, noise = _forward(rows, n, seed, step, tau)
            err = np.abs(noise.double().cpu().numpy() - want_noise).max()
            got = idx.cpu().numpy()
            ok = margin > MARGIN
            left_out = 1.0 - ok.mean()
            print('rows %d n %d tau %g: max |noise - float64| %.3e, rows left out %.4f %%, idx mismatches at margin %d' % (
                rows, n, tau, err, 100 * left_out, int((ok & (got != want_idx)).sum())))
            assert err <= 1e-4
            assert got.dtype == np.int32 and got.min() >= 0 and got.max() < n
            assert left_out <= 1e-3 and not (ok & (got != want_idx)).any()
        # the step by value plus the cell is the same draw as the sum by value alone
        cell = torch.tensor([step - 5 if step >= 5 else step], dtype=torch.int64, device='cuda')
        by_value = step - int(cell[0])
        again = _forward(rows, n, seed, by_value, TAUS[-1], cell=cell)
        for a, b in zip(again[1:], (y, soft, idx, noise)):
            assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)


@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('n', WIDTHS)
def test_forward_is_the_softmax_of_the_perturbed_logits(n, tau):
    from multiagent_rl_amd import sampling
    for rows in ROWS:
        for seed, step in KEYS[::2]:
            x, y, soft, idx, noise = _forward(rows, n, seed, step, tau)
            want = torch.softmax((x.double() - noise.double()) / tau, dim=-1)
            err = (soft.double() - want).abs()
            print('rows %d n %d tau %g: max |soft - float64| %.3e, max relative %.3e' % (
                rows, n, tau, float(err.max()), float((err / want.clamp_min(1e-30)).max())))
            assert bool((err <= 1e-7 + 5e-5 * want).all())
            v = (x - noise) / tau
            first = np.argmax((v == v.max(-1, keepdim=True).values).cpu().numpy(), axis=-1)         # NumPy: the FIRST maximum of the device's own v
            assert np.array_equal(idx.cpu().numpy(), first)
            onehot = torch.nn.functional.one_hot(idx.long(), n).float()
            assert torch.equal(_bits(y), _bits((onehot - soft) + soft))
            y_soft, soft2, _, _ = sampling.launch_forward(x, tau, False, seed, step, None, True)
            assert torch.equal(_bits(y_soft), _bits(soft)) and torch.equal(_bits(soft2), _bits(soft))
            y_only = sampling.launch_forward(x, tau, True, seed, step, None, False)                    # nothing optional stored
            assert y_only[1:] == (None, None, None) and torch.equal(_bits(y_only[0]), _bits(y))


@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('n', WIDTHS)
def test_backward_is_the_softmax_gradient(n, tau):
    from multiagent_rl_amd import sampling
    for rows in ROWS:
        seed, step = KEYS[1]
        x, y, soft, idx, noise = _forward(rows, n, seed, step, tau)
        dY = torch.randn(rows, n, generator=torch.Generator().manual_seed(rows + n)).cuda()
        got = sampling.launch_backward(dY, soft, tau).double()
        scale = float(dY.abs().max()) / tau
        want = sampling_ref.backward(dY.double(), soft.double(), tau)
        xs = x.double().requires_grad_()
        for hard in (True, False):                                     # the hard and the soft sample share the gradient
            xs.grad = None
            (sampling_ref.stock(xs, noise.double(), tau, hard) * dY.double()).sum().backward()
            e_formula, e_stock = float((got - want).abs().max()), float((got - xs.grad).abs().max())
            print('rows %d n %d tau %g hard %s: |dLogits - formula| %.3e (bound %.3e), |dLogits - stock autograd| %.3e (bound %.3e)' % (
                rows, n, tau, hard, e_formula, 5e-6 * scale, e_stock, 2e-4 * scale))
            assert e_formula <= 5e-6 * scale and e_stock <= 2e-4 * scale
        assert float(got.abs().max()) > 0 or n == 1


def test_autograd_surface_on_the_device():
    """gumbel_st end to end: any leading shape, a strided input, gradient equal to the launches', nothing kept under no_grad."""
    from multiagent_rl_amd import sampling
    x = _logits(257, 5).cuda().reshape(257, 1, 5).expand(257, 3, 5).transpose(0, 1)       # [3, 257, 5], strided
    xs = x.clone(memory_format=torch.contiguous_format).requires_grad_()
    y = sampling.gumbel_st(xs, tau=0.5, seed=7, step=3)
    flat = xs.detach().reshape(-1, 5)
    want_y, soft, _, _ = sampling.launch_forward(flat, 0.5, True, 7, 3, None, True)
    assert y.shape == (3, 257, 5) and torch.equal(_bits(y.detach()), _bits(want_y.reshape(3, 257, 5)))
    dY = torch.randn(3, 257, 5, device='cuda')
    g, = torch.autograd.grad(y, xs, dY)
    assert torch.equal(_bits(g), _bits(sampling.launch_backward(dY.reshape(-1, 5), soft, 0.5).reshape(3, 257, 5)))
    xt = x.detach().requires_grad_()                                                        # the strided tensor itself
    yt = sampling.gumbel_st(xt, tau=0.5, seed=7, step=3)
    assert torch.equal(_bits(yt.detach()), _bits(y.detach()))
    with torch.no_grad():
        assert sampling.gumbel_st(xs, seed=7).grad_fn is None
    for bad, word in ((torch.zeros(2, 5), 'no CPU fallback'), (torch.zeros(2, 5, device='cuda', dtype=torch.float64), 'float32'),
                      (torch.zeros(2, 17, device='cuda'), '1 to 16')):
        with pytest.raises((RuntimeError, ValueError), match=word):
            sampling.gumbel_st(bad)


def test_distribution_and_reproducibility():
    from multiagent_rl_amd.sampling import SITES_PER_UPDATE, GumbelSampler
    row = torch.tensor([0.3, -1.2, 1.1, 0.0, -0.4])
    p = torch.softmax(row.double(), -1).numpy()
    x = row.cuda().repeat(20000, 1)
    s = GumbelSampler(seed=123, device='cuda')
    a = s.sample_index(x)                                                  # site 0
    b = s.sample_index(x)                                                  # site 1
    freq = np.bincount(a.cpu().numpy(), minlength=5) / 20000.0
    print('freq %s softmax %s max diff %.4f' % (freq, p, np.abs(freq - p).max()))
    assert a.dtype == torch.int32 and np.abs(freq - p).max() < 0.015
    assert not torch.equal(a, b)                                           # another site: other noise
    hard0 = GumbelSampler(seed=123, device='cuda').sample(x)
    assert torch.equal(hard0.argmax(-1).int(), a) and int((hard0 != 0).sum()) == 20000      # one-hot: the sample_index of the same site
    s.end_update()
    c = s.sample_index(x)                                                  # site 0 of the next update: another cell value
    assert int(s.cell) == SITES_PER_UPDATE and not torch.equal(a, c)
    s.reset(0)
    assert torch.equal(s.sample_index(x), a) and torch.equal(s.sample_index(x), b)     # the same (seed, cell, site): the same bits
    s.reset(1)
    assert torch.equal(s.sample_index(x), c)
    other = GumbelSampler(seed=124, device='cuda')
    assert not torch.equal(other.sample_index(x), a)


def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]


def test_one_sample_is_one_kernel_forward_and_one_backward():
    from multiagent_rl_amd.sampling import GumbelSampler
    s = GumbelSampler(seed=1, device='cuda')
    x = _logits(6144, 5).cuda().requires_grad_()
    dY = torch.randn(6144, 5, device='cuda')
    torch.autograd.grad(s.sample(x), x, dY)                                # warm: the library is loaded, the allocator has its blocks
    torch.cuda.synchronize()
    y, fwd = _device_kernels(lambda: s.sample(x))
    _, bwd = _device_kernels(lambda: torch.autograd.grad(y, x, dY))
    print('forward: %r\nbackward: %r' % (fwd, bwd))
    assert len(fwd) == 1 and 'pw_gumbel_st_forward_kernel' in fwd[0]
    assert len(bwd) == 1 and 'pw_gumbel_st_backward_kernel' in bwd[0]


def test_a_captured_sample_draws_new_noise_every_replay():
    """The by-value site is what the capture records; the cell is read by the kernel and advanced inside the region."""
    from multiagent_rl_amd import sampling
    x = _logits(257, 10).cuda()
    s = sampling.GumbelSampler(seed=9, device='cuda')
    s.sample(x)
    s.end_update()                                                         # one eager update: cell = 16
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        first, second = s.sample(x), s.sample(x)
        s.end_update()
    for update in (1, 2, 3):
        g.replay()
        torch.cuda.synchronize()
        for site, got in enumerate((first, second)):
            want = sampling.launch_forward(x, 1.0, True, 9, 16 * update + site, None, False)[0]
            assert torch.equal(_bits(got), _bits(want)), (update, site)
    assert int(s.cell) == 64 and s.site == 0


# ---- the capability: graphed and eager updates with REAL noise, bit for bit --------------------------------------------------------
def _learner(ug, variant, nets, graph, sampler_seed):
    import madr_learner
    from multiagent_rl_amd.policy import accelerate_trainer
    cls_name, _, _, ring_kw, N, D = ug.VARIANTS[variant]
    actor, critic = copy.deepcopy(nets)
    t = getattr(madr_learner, cls_name)(actor, critic, ug._filled_memory(ring_kw, N, D),
                                        action_type='MultiDiscrete' if 'act_heads' in ring_kw else 'Discrete', batch_size=ug.BATCH,
                                        fused_optimizer=True, fused_lstm=True, fused_attention=True, graph_update=graph,
                                        fused_sampling=True, sampling_seed=sampler_seed)
    if not graph:
        accelerate_trainer(t, targets=True)
    return t


@pytest.mark.parametrize('variant', ['attention', 'two_head', 'bicnet', 'model'])
def test_graphed_updates_with_real_noise_equal_eager_updates_bit_for_bit(variant):
    """Learners A and B eager, C graphed, one sampler seed: A == B == C in every parameter, target, Adam moment and loss after each of 8
    updates and after a learning-rate change (a re-capture).  torch's generator is re-seeded differently before every learner's update:
    nothing in the update may draw from it.  A learner with another sampler seed differs."""
    import tests.test_gpu_update_graph as ug                              # the harness: VARIANTS, _filled_memory, _everything, _same
    from multiagent_rl_amd import critic as cr, policy as pol
    from multiagent_rl_amd.graph import GraphedUpdate
    torch.manual_seed(3)
    nets = (ug.VARIANTS[variant][1](pol, cr), ug.VARIANTS[variant][2](pol, cr))
    a, b, c = (_learner(ug, variant, nets, graph, 5) for graph in (False, False, True))
    d = _learner(ug, variant, nets, False, 6)
    assert isinstance(c.optimize, GraphedUpdate) and all('_sample' in vars(t) for t in (a, b, c, d))

    def step(t, k):
        torch.manual_seed(100 + k)
        sites_before = t.sampler.site
        out = tuple(float(x) for x in t.optimize())
        assert sites_before == 0 and t.sampler.site == 0
        return out
    for it in range(8):
        la, lb, lc = step(a, 0), step(b, 1), step(c, 2)
        sa, sb, sc = ug._everything(a), ug._everything(b), ug._everything(c)
        assert len(sa) == len(sc) > 20
        bad_b = [i for i, (x, y) in enumerate(zip(sa, sb)) if not ug._same(x, y)]
        bad_c = [i for i, (x, y) in enumerate(zip(sa, sc)) if not ug._same(x, y)]
        print('%s update %d: losses A %r B %r C %r; tensors differing A/B %r A/C %r' % (variant, it + 1, la, lb, lc, bad_b[:5], bad_c[:5]))
        assert la == lb and not bad_b, (variant, it)
        assert la == lc and not bad_c, (variant, it)
        assert int(a.sampler.cell) == int(c.sampler.cell) == 16 * (it + 1)
        if it == 0:
            ld = step(d, 3)
            assert ld != la and any(not ug._same(x, y) for x, y in zip(sa, ug._everything(d)))
    g = c.optimize
    assert (g.eager_calls, g.captures, g.replays) == (3, 1, 5) and a.sampler.updates == 8
    for t in (a, c):                                                       # a changed learning rate: captured again, still the eager learner's bits
        for opt in (t.actor_optimizer, t.critic_optimizer):
            opt.param_groups[0]['lr'] = 1e-3
    la, lc = step(a, 0), step(c, 2)
    assert g.captures == 2 and la == lc and all(ug._same(x, y) for x, y in zip(ug._everything(a), ug._everything(c)))
    assert int(a.sampler.cell) == int(c.sampler.cell) == 16 * 9
