"""GPU: pw_lstm_train_wgrad (the two W_hh gradients of the learner's LSTMs, csrc/pw_kernels_lstm_wgrad.hpp) and its Python surface
(multiagent_rl_amd.lstm: launch_wgrad, lstm_recurrence(wgrad=True), fuse_lstm(wgrad=True), the example learner's fused_wgrad).

Reference: tests/lstm_wgrad_ref.py, the float64 restatement of the two sums, applied to the float32 dG and Y that the device's own
forward and backward produced.  Stock: the torch expression the switch replaces (two sliced copies and a GEMM per direction), on the
GPU in the same run.  Bound, the project's own (tests/lstm_ref.worst_ratio <= 4): the error against float64 is at most
4 x max(the stock expression's error, one float32 rounding of the reference's largest entry).

Measured: ratios 0.00 - 0.58 at the kernel over all shapes and patterns, 1.00 - 1.21 for the networks; every case
prints its own.
"""
import copy
import functools

import pytest
import torch

from tests import lstm_ref, lstm_wgrad_ref

pytestmark = pytest.mark.gpu
F = torch.nn.functional
DEV = 'cuda'
LONG = [(1024, 6, 1, 64), (1024, 6, 2, 32), (300, 21, 1, 64), (300, 21, 2, 32)]
SHAPES = list(lstm_ref.SHAPES) + LONG
IDS = ['b%d-N%d-%dx%d' % s for s in SHAPES]
BOTH = [(1, 64), (2, 32)]
BOTH_IDS = ['1x64', '2x32']


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stock(dG, Y):
    """The expression of lstm._Recurrence.backward with the switch off."""
    H = dG.shape[3] // 4
    d_fw = dG[:, 1:, 0].reshape(-1, 4 * H).t() @ Y[:, :-1, :H].reshape(-1, H)
    d_bw = dG[:, :-1, 1].reshape(-1, 4 * H).t() @ Y[:, 1:, H:].reshape(-1, H) if dG.shape[2] == 2 else None
    return d_fw, d_bw


def _named(pair):
    return {k: v for k, v in zip(('weight_hh_l0', 'weight_hh_l0_reverse'), pair) if v is not None}


# the three gradient patterns of tests/test_gpu_lstm_train.py::test_gradient_patterns, as the dY they amount to
PATTERNS = (
    ('random dY', lambda dY: dY),
    ('Y.sum() (ones)', lambda dY: torch.ones_like(dY)),
    ('only Y[:, -1]', lambda dY: torch.cat([torch.zeros_like(dY[:, :-1]), dY[:, -1:]], dim=1)),
)


@functools.lru_cache(maxsize=None)
def _case(b, N, dirs, H):
    """One shape's G, weights and dY on the device and the device's own (Y, saved), made once and left unchanged."""
    from multiagent_rl_amd import lstm as L
    stock = lstm_ref.make_lstm(dirs, H, torch.float32, DEV)
    x, dY = lstm_ref.make_inputs(b, N, dirs, H, torch.float32)
    with torch.no_grad():
        w_ih, bias, w_fw, w_bw = lstm_ref.projection(stock)
        G = F.linear(x.to(DEV), w_ih, bias).view(b, N, dirs, 4 * H).contiguous()
        w_fw = w_fw.detach().clone()
        w_bw = None if w_bw is None else w_bw.detach().clone()
    Y, saved = L.launch_forward(G, w_fw, w_bw, True)
    return G, w_fw, w_bw, dY.to(DEV), Y, saved


def _dG(shape, pattern=PATTERNS[0][1]):
    from multiagent_rl_amd import lstm as L
    G, w_fw, w_bw, dY, Y, saved = _case(*shape)
    return L.launch_backward(pattern(dY).contiguous(), saved, w_fw, w_bw), Y


# ---- 1. accuracy ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_against_the_float64_restatement(shape):
    from multiagent_rl_amd import lstm as L
    dirs = shape[2]
    for name, pattern in PATTERNS:
        dG, Y = _dG(shape, pattern)
        kernel, stock = _named(L.launch_wgrad(dG, Y, True, dirs == 2)), _named(_stock(dG, Y))
        ref = _named(lstm_wgrad_ref.whh_grads(dG, Y))
        assert len(ref) == dirs and all(bool(torch.isfinite(v).all()) for v in kernel.values())
        ratio, worst, e_k, e_s = lstm_ref.worst_ratio(kernel, stock, ref)
        print('dW_hh %-22s %-16s worst %-22s kernel %.3e  stock %.3e  ratio %.2f' % (shape, name, worst, e_k, e_s, ratio))
        assert ratio <= 4.0, (shape, name, worst, e_k, e_s, ratio)


# ---- 2. indexing, exactly ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dirs,H', BOTH, ids=BOTH_IDS)
@pytest.mark.parametrize('b', [3, 17])
def test_one_row_of_dG_gives_one_outer_product(b, dirs, H):
    from multiagent_rl_amd import lstm as L
    N = 4
    g = torch.Generator().manual_seed(b + dirs)
    Y = torch.randn(b, N, dirs * H, generator=g).to(DEV)
    row = torch.randn(4 * H, generator=g).to(DEV)
    zero = torch.zeros(4 * H, H, device=DEV)
    for seq in sorted({0, b // 2, b - 1}):
        for d in range(dirs):
            for t in range(N):
                prev = t + 1 if d else t - 1
                dG = torch.zeros(b, N, dirs, 4 * H, device=DEV)
                dG[seq, t, d] = row
                got = L.launch_wgrad(dG, Y, True, dirs == 2)
                want = torch.outer(row, Y[seq, prev, d * H:(d + 1) * H]) if 0 <= prev < N else zero
                assert torch.equal(got[d], want), (seq, d, t)                  # as numbers: a zero of either sign is a zero
                if dirs == 2:
                    assert torch.equal(got[1 - d], zero), (seq, d, t)
    dG = torch.zeros(b, N, dirs, 4 * H, device=DEV)                             # only the rows that have no previous step
    dG[:, 0, 0] = torch.randn(b, 4 * H, generator=g).to(DEV)
    if dirs == 2:
        dG[:, N - 1, 1] = torch.randn(b, 4 * H, generator=g).to(DEV)
    for got in L.launch_wgrad(dG, Y, True, dirs == 2)[:dirs]:
        assert torch.equal(got, zero)


@pytest.mark.parametrize('dirs,H', BOTH, ids=BOTH_IDS)
def test_one_step_gives_zeros_and_a_skipped_direction_is_none(dirs, H):
    from multiagent_rl_amd import lstm as L
    g = torch.Generator().manual_seed(4)
    dG, Y = torch.randn(5, 1, dirs, 4 * H, generator=g).to(DEV), torch.randn(5, 1, dirs * H, generator=g).to(DEV)
    got = L.launch_wgrad(dG, Y, True, dirs == 2)
    for d in range(dirs):
        assert got[d].shape == (4 * H, H) and got[d].dtype == torch.float32 and float(got[d].abs().max()) == 0.0
    assert dirs == 2 or got[1] is None
    dG, Y = _dG((17, 3, dirs, H) if dirs == 1 else (33, 6, dirs, H))
    both = L.launch_wgrad(dG, Y, True, dirs == 2)
    only_fw = L.launch_wgrad(dG, Y, True, False)
    assert only_fw[1] is None and torch.equal(_bits(only_fw[0]), _bits(both[0]))
    if dirs == 2:
        only_bw = L.launch_wgrad(dG, Y, False, True)
        assert only_bw[0] is None and torch.equal(_bits(only_bw[1]), _bits(both[1]))


# ---- 3. non-finite ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dirs,H', BOTH, ids=BOTH_IDS)
@pytest.mark.parametrize('b,N', [(17, 3), (33, 6)])
def test_non_finite_inputs_reach_what_they_reach_in_the_stock_expression(b, N, dirs, H):
    from multiagent_rl_amd import lstm as L
    g = torch.Generator().manual_seed(b)
    dG0, Y0 = torch.randn(b, N, dirs, 4 * H, generator=g).to(DEV), torch.randn(b, N, dirs * H, generator=g).to(DEV)
    run = lambda dG, Y: L.launch_wgrad(dG, Y, True, dirs == 2)[:dirs]  # noqa: E731
    clean = run(dG0, Y0)
    nan = float('nan')

    def masks(dG, Y):
        got = run(dG, Y)
        ref = lstm_wgrad_ref.whh_grads(dG, Y)[:dirs]
        for a, r in zip(got, ref):
            assert torch.equal(~torch.isfinite(a).cpu(), ~torch.isfinite(r)), 'the non-finite mask is the restatement\'s'
        return got
    s, r0, k0 = b - 2, 4 * H - 3, H - 5
    dG = dG0.clone()                                                            # rows that have no previous step: nothing reaches the sums
    dG[s, 0, 0, r0] = nan
    dG[0, 0, 0, 1] = float('inf')
    if dirs == 2:
        dG[s, N - 1, 1, r0] = nan
    for a, c in zip(masks(dG, Y0), clean):
        assert bool(torch.isfinite(a).all()) and torch.equal(_bits(a), _bits(c))
    dG = dG0.clone()                                                            # a live row: exactly row r0 of d_fw
    dG[s, 1, 0, r0] = nan
    got = masks(dG, Y0)
    bad = ~torch.isfinite(got[0])
    assert bool(bad[r0].all()) and int(bad.sum()) == H
    keep = torch.arange(4 * H, device=DEV) != r0
    assert torch.equal(_bits(got[0][keep]), _bits(clean[0][keep]))
    if dirs == 2:
        assert torch.equal(_bits(got[1]), _bits(clean[1]))
    Y = Y0.clone()                                                              # the shifted operand: exactly column k0 of d_fw
    Y[s, 0, k0] = nan
    got = masks(dG0, Y)
    bad = ~torch.isfinite(got[0])
    assert bool(bad[:, k0].all()) and int(bad.sum()) == 4 * H
    if dirs == 2:
        assert torch.equal(_bits(got[1]), _bits(clean[1]))                      # column k0 < H is direction 0's alone
        Y = Y0.clone()                                                          # and the reverse direction's shifted operand
        Y[s, N - 1, H + k0] = nan
        got = masks(dG0, Y)
        bad = ~torch.isfinite(got[1])
        assert bool(bad[:, k0].all()) and int(bad.sum()) == 4 * H and torch.equal(_bits(got[0]), _bits(clean[0]))


# ---- 4. the same bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dirs,H', BOTH, ids=BOTH_IDS)
@pytest.mark.parametrize('b,N', [(1024, 6), (33, 6)])
def test_the_same_inputs_give_the_same_bits(b, N, dirs, H):
    from multiagent_rl_amd import lstm as L
    dG, Y = _dG((b, N, dirs, H))
    run = lambda: L.launch_wgrad(dG, Y, True, dirs == 2)[:dirs]  # noqa: E731
    first, second = run(), run()
    other = _dG((17, 3, 1, 64))                                                 # an unrelated launch of another shape in between
    L.launch_wgrad(other[0], other[1], True, False)
    third = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fourth = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    replays = []
    for _ in range(2):
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        replays.append([t.clone() for t in captured])
    torch.cuda.synchronize()
    for i, others in enumerate((second, third, fourth, replays[0], replays[1])):
        for d in range(dirs):
            assert torch.equal(_bits(first[d]), _bits(others[d])), (i, d)
    assert bool(torch.isfinite(first[0]).all()) and float(first[0].abs().max()) > 0


# ---- 5. kernel count --------------------------------------------------------------------------------------------------------------
def _device_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, [e.name for e in prof.events() if str(getattr(e, 'device_type', '')).endswith('CUDA')]


@pytest.mark.parametrize('dirs,H', BOTH, ids=BOTH_IDS)
def test_the_backward_of_the_recurrence_is_the_librarys_kernels_alone(dirs, H):
    from multiagent_rl_amd import lstm as L
    G, w_fw, w_bw, dY, _, _ = _case(1024, 6, dirs, H)
    leaves = [t.clone().requires_grad_(True) for t in (G, w_fw, w_bw) if t is not None]
    lists = {}
    for wgrad in (True, False):
        torch.autograd.grad(L.lstm_recurrence(*leaves, wgrad=wgrad), leaves, dY)   # warm: the allocator has its blocks
        torch.cuda.synchronize()
        Y = L.lstm_recurrence(*leaves, wgrad=wgrad)
        _, lists[wgrad] = _device_kernels(lambda: torch.autograd.grad(Y, leaves, dY))
    print('%d x %d backward with the switch:    %r\n%d x %d backward without the switch: %r' % (dirs, H, lists[True], dirs, H, lists[False]))
    on, off = lists[True], lists[False]
    assert all('pw_lstm_train' in k for k in on) and 'pw_lstm_train_backward_kernel' in on[0]
    assert 2 <= len(on) <= 3 and sum('pw_lstm_train_wgrad' in k for k in on) == len(on) - 1
    assert len(off) > len(on) and any('pw_lstm_train' not in k for k in off)


# ---- 6. the networks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b,N', [(33, 6), (5, 13)])
@pytest.mark.parametrize('name', lstm_ref.NETWORKS)
def test_networks_against_float64(name, b, N):
    from multiagent_rl_amd.lstm import fuse_lstm
    plain = lstm_ref.make_network(name).to(DEV)
    ref = copy.deepcopy(plain).double()
    stock, fused = copy.deepcopy(plain), copy.deepcopy(plain)
    assert fuse_lstm(stock) == 1 and fuse_lstm(fused, wgrad=True) == 1
    inputs = lstm_ref.network_inputs(name, b, N, torch.float32, DEV)
    g_ref = lstm_ref.network_grads(ref, tuple(t.double() for t in inputs))
    g_fused, g_stock = lstm_ref.network_grads(fused, inputs), lstm_ref.network_grads(stock, inputs)
    assert set(g_fused) == set(g_ref) and all(bool(torch.isfinite(v).all()) for v in g_fused.values())
    ratio, worst, e_k, e_s = lstm_ref.worst_ratio(g_fused, g_stock, g_ref)
    print('%s b=%d N=%d: worst %s  wgrad %.3e  fused without %.3e  ratio %.2f' % (name, b, N, worst, e_k, e_s, ratio))
    assert ratio <= 4.0, (name, worst, e_k, e_s, ratio)
    hh = [n for n in g_ref if 'weight_hh' in n]
    assert hh and all(float(g_fused[n].abs().max()) > 0 for n in hh)


# ---- 7. the capability: graphed and eager updates with the switch, bit for bit ----------------------------------------------------
def _learner(ug, variant, nets, graph, wgrad=True):
    import madr_learner
    from multiagent_rl_amd.policy import accelerate_trainer
    cls_name, _, _, ring_kw, N, D = ug.VARIANTS[variant]
    actor, critic = copy.deepcopy(nets)
    t = getattr(madr_learner, cls_name)(actor, critic, ug._filled_memory(ring_kw, N, D),
                                        action_type='MultiDiscrete' if 'act_heads' in ring_kw else 'Discrete', batch_size=ug.BATCH,
                                        fused_optimizer=True, fused_lstm=True, fused_attention=True, graph_update=graph,
                                        fused_sampling=True, sampling_seed=5, fused_front=True, fused_wgrad=wgrad)
    if not graph:
        accelerate_trainer(t, targets=True)
    return t


@pytest.mark.parametrize('variant', ['attention', 'two_head', 'bicnet', 'model'])
def test_graphed_updates_with_the_switch_equal_eager_updates_bit_for_bit(variant):
    """Learners A and B eager, C graphed, all with every switch and fused_wgrad: A == B == C in every parameter, target, Adam moment and
    loss after each of 8 updates and after a learning-rate change (a re-capture).  Learner D, graphed without the switch, starts from
    the same weights: after the first update both losses agree with A's to 1e-3 relative (only the summation order differs), after 8
    updates some parameter differs, and one of its replays holds more device kernels than one of C's."""
    import tests.test_gpu_update_graph as ug                              # the harness: VARIANTS, _filled_memory, _everything, _same
    from multiagent_rl_amd import critic as cr, policy as pol
    from multiagent_rl_amd.graph import GraphedUpdate
    from multiagent_rl_amd.lstm import FusedLSTM
    torch.manual_seed(3)
    nets = (ug.VARIANTS[variant][1](pol, cr), ug.VARIANTS[variant][2](pol, cr))
    a, b, c = (_learner(ug, variant, nets, graph) for graph in (False, False, True))
    d = _learner(ug, variant, nets, True, wgrad=False)
    assert isinstance(c.optimize, GraphedUpdate) and isinstance(d.optimize, GraphedUpdate)
    modes = lambda t: [getattr(m, 'wgrad', False) for n in (t.actor, t.critic) for m in n.modules() if type(m) is FusedLSTM]  # noqa: E731
    assert modes(a) == modes(b) == modes(c) == [True, True] and modes(d) == [False, False]

    def step(t, k):
        torch.manual_seed(100 + k)
        return tuple(float(x) for x in t.optimize())
    for it in range(8):
        la, lb, lc, ld = step(a, 0), step(b, 1), step(c, 2), step(d, 3)
        sa, sb, sc = ug._everything(a), ug._everything(b), ug._everything(c)
        assert len(sa) == len(sc) > 20
        bad_b = [i for i, (x, y) in enumerate(zip(sa, sb)) if not ug._same(x, y)]
        bad_c = [i for i, (x, y) in enumerate(zip(sa, sc)) if not ug._same(x, y)]
        print('%s update %d: losses A %r B %r C %r D %r; tensors differing A/B %r A/C %r' % (variant, it + 1, la, lb, lc, ld, bad_b[:5], bad_c[:5]))
        assert la == lb and not bad_b, (variant, it)
        assert la == lc and not bad_c, (variant, it)
        if it == 0:
            for x, y in zip(la, ld):
                assert abs(x - y) <= 1e-3 * abs(y), (la, ld)
    assert any(not ug._same(x, y) for x, y in zip(ug._everything(a), ug._everything(d)))
    g = c.optimize
    assert (g.eager_calls, g.captures, g.replays) == (3, 1, 5)
    for t in (a, c):                                                       # a changed learning rate: captured again, still the eager learner's bits
        for opt in (t.actor_optimizer, t.critic_optimizer):
            opt.param_groups[0]['lr'] = 1e-3
    la, lc = step(a, 0), step(c, 2)
    assert g.captures == 2 and la == lc and all(ug._same(x, y) for x, y in zip(ug._everything(a), ug._everything(c)))
    _, with_switch = _device_kernels(c.optimize)
    _, without = _device_kernels(d.optimize)
    print('%s: device kernels of one graphed update: with the switch %d, without %d' % (variant, len(with_switch), len(without)))
    assert 0 < len(with_switch) < len(without)
    assert sum('pw_lstm_train_wgrad' in k for k in with_switch) == 6 and not any('pw_lstm_train_wgrad' in k for k in without)


def test_accelerate_trainer_wgrad_switch():
    import tests.test_gpu_update_graph as ug                              # puts examples/ on sys.path
    import madr_learner
    from multiagent_rl_amd import critic as cr, policy as pol
    from multiagent_rl_amd.lstm import FusedLSTM
    _, mk_actor, mk_critic, ring_kw, N, D = ug.VARIANTS['attention']
    make = lambda **kw: madr_learner.Trainer(mk_actor(pol, cr), mk_critic(pol, cr), ug._filled_memory(ring_kw, N, D), batch_size=ug.BATCH, **kw)  # noqa: E731
    with pytest.raises(ValueError, match='no fused LSTM'):
        pol.accelerate_trainer(make(), wgrad=True)
    with pytest.raises(ValueError, match='fused_lstm'):
        make(fused_wgrad=True)
    t = make()
    fx = pol.accelerate_trainer(t, lstm=True, wgrad=True)
    assert fx.wgrad_lstms == 4 and all(m.wgrad for n in (t.actor, t.critic) for m in n.modules() if type(m) is FusedLSTM)
    la, lc = t.optimize()
    assert la == la and lc == lc
    t = make(fused_lstm=True)
    fx = pol.accelerate_trainer(t, targets=True, wgrad=True)                 # LSTMs fused already; the targets are wrappers: left alone
    assert fx.wgrad_lstms == 2 and t.critic.lstm.wgrad is True


# ---- 8. refusals on the device ----------------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from multiagent_rl_amd import _lib, lstm as L
    z = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    dG, Y = z(4, 3, 1, 256), z(4, 3, 64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        L.launch_wgrad(dG.cpu(), Y.cpu(), True, False)
    with pytest.raises(RuntimeError, match='float32'):
        L.launch_wgrad(dG.double(), Y, True, False)
    with pytest.raises(RuntimeError, match='contiguous'):
        L.launch_wgrad(z(4, 3, 1, 512)[..., ::2], Y, True, False)
    with pytest.raises(ValueError, match='dirs'):
        L.launch_wgrad(z(4, 3, 1, 128), z(4, 3, 32), True, False)
    with pytest.raises(ValueError, match='Y must be'):
        L.launch_wgrad(dG, z(4, 3, 32), True, False)
    with pytest.raises(ValueError, match='want_bw'):
        L.launch_wgrad(dG, Y, True, True)
    with pytest.raises(ValueError, match='neither'):
        L.launch_wgrad(dG, Y, False, False)
    # the entry point itself, with real device memory: PW_EINVAL surfaces as PworldError with the text of pw_last_error
    lib, p, s = _lib.load(), _lib.ptr, _lib.stream(dG.device)
    out, out2, scratch = z(256, 64), z(128, 32), z(lib.pw_lstm_train_wgrad_scratch_bytes(4, 3, 1, 64) // 4)
    odd = lambda t: _lib.C.c_void_p(t.data_ptr() + 2)  # noqa: E731
    cases = [
        ((p(dG), p(Y), 4, 3, 1, 64, p(out), p(out2), p(scratch), s), 'dw_hh_bw must be null with dirs = 1'),
        ((p(dG), p(Y), 4, 3, 1, 64, None, None, p(scratch), s), 'both null'),
        ((p(dG), p(Y), 4, 3, 2, 32, None, None, p(scratch), s), 'both null'),
        ((None, p(Y), 4, 3, 1, 64, p(out), None, p(scratch), s), 'dG is null'),
        ((p(dG), None, 4, 3, 1, 64, p(out), None, p(scratch), s), 'Y is null'),
        ((p(dG), p(Y), 4, 3, 1, 64, p(out), None, None, s), 'scratch is null'),
        ((p(dG), p(Y), 4, 3, 1, 64, odd(out), None, p(scratch), s), 'dw_hh_fw must be 4-byte aligned'),
        ((p(dG), p(Y), 4, 3, 2, 32, p(out2), odd(out2), p(scratch), s), 'dw_hh_bw must be 4-byte aligned'),
        ((odd(dG), p(Y), 4, 3, 1, 64, p(out), None, p(scratch), s), 'dG must be 4-byte aligned'),
        ((p(dG), p(Y), 4, 3, 1, 32, p(out), None, p(scratch), s), 'shapes served'),
        ((p(dG), p(Y), 4, 0, 1, 64, p(out), None, p(scratch), s), 'N must be'),
        ((p(dG), p(Y), 0, 3, 1, 64, p(out), None, p(scratch), s), 'b must be'),
    ]
    for args, text in cases:
        with pytest.raises(_lib.PworldError, match=text):
            _lib.check(lib.pw_lstm_train_wgrad(*args))
        assert text in lib.pw_last_error().decode()
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0 and float(out2.abs().max()) == 0.0      # nothing was launched
