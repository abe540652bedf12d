"""CPU: the critic's host side.

(a) tests/critic_ref.py (float64 NumPy, written from the architecture) reproduces the float64 outputs the REFERENCE's
    CriticNetwork gave on the fixture rows (tests/golden/critic_forward.npz, made by tests/golden/make_critic_golden.py) to 1e-12.
(b) ``multiagent_rl_amd.critic.CriticNetwork`` loads every fixture state_dict with ``strict=True`` (same keys, same shapes) and
    reproduces the reference's float32 outputs to 2e-6 on the CPU.
(c) ``pw_critic_forward`` is exported and refuses null / out-of-range arguments before anything is launched.
"""
import ctypes as C
import os

import numpy as np
import pytest

from tests import critic_ref as cr

torch = pytest.importorskip('torch')

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'critic_forward.npz'))
CASES = cr.GOLDEN_CASES
IDS = [cr.golden_name(*c) for c in CASES]


def fixture_state_dict(name):
    pre = name + '/sd/'
    return {k[len(pre):]: torch.from_numpy(G[k]) for k in G.files if k.startswith(pre)}


def test_fixture_holds_the_four_cases_and_the_reference_keys():
    for name in IDS:
        assert sorted(fixture_state_dict(name)) == sorted(cr.KEYS)
        assert G[name + '/q32'].shape == (cr.GOLDEN_ROWS, 1) and G[name + '/q32'].dtype == np.float32
        assert G[name + '/q64'].shape == (cr.GOLDEN_ROWS, 1) and G[name + '/q64'].dtype == np.float64
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), 'golden', 'critic_forward.npz')) < (1 << 20)


@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_inputs_are_the_rows_the_fixture_was_made_from(N, D, heads):
    obs, idx = cr.golden_inputs(N, D, heads)
    want = G[cr.golden_name(N, D, heads) + '/input_sum']
    assert obs.astype(np.float64).sum() == want[0] and float(idx.sum()) == want[1]


@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_float64_restatement_reproduces_the_reference(N, D, heads):
    name = cr.golden_name(N, D, heads)
    obs, idx = cr.golden_inputs(N, D, heads)
    q = cr.forward_f64(fixture_state_dict(name), obs, cr.one_hot(idx, heads))
    err = float(np.abs(q - G[name + '/q64'][:, 0]).max())
    print('%s: |q_f64 - reference float64| %.3g' % (name, err))
    assert err <= 1e-12


@pytest.mark.parametrize('N,D,heads', CASES, ids=IDS)
def test_host_module_loads_reference_state_dict_and_reproduces_float32(N, D, heads):
    from multiagent_rl_amd.critic import CriticNetwork
    name = cr.golden_name(N, D, heads)
    net = CriticNetwork(D + sum(heads), 1).eval()
    sd = fixture_state_dict(name)
    assert {k: tuple(v.shape) for k, v in net.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    net.load_state_dict(sd, strict=True)
    obs, idx = cr.golden_inputs(N, D, heads)
    act = cr.one_hot(idx, heads)
    with torch.no_grad():
        q = net(torch.from_numpy(obs), torch.from_numpy(act)).numpy()
        if len(heads) == 2:   # a list of per-head one-hots is concatenated as the reference does
            parts = [torch.from_numpy(act[..., :heads[0]]), torch.from_numpy(act[..., heads[0]:])]
            assert np.array_equal(net(torch.from_numpy(obs), parts).numpy(), q)
    assert q.shape == (cr.GOLDEN_ROWS, 1)
    err = float(np.abs(q - G[name + '/q32']).max())
    print('%s: |q - reference float32| %.3g' % (name, err))
    assert err <= 2e-6


def test_critic_forward_arguments_are_checked_on_the_host():
    """Null pointers, both / neither action form, bad widths and shapes, a half-given TD epilogue: PW_EINVAL with a text, nothing
    launched (no GPU needed; the pointers are fakes)."""
    from multiagent_rl_amd import _lib
    lib = _lib.load()
    assert 'pw_critic_forward' in _lib.SIGNATURES and hasattr(lib, 'pw_critic_forward')
    p = C.c_void_p(4096)
    w = [p] * 8

    def call(obs=p, idx=p, vec=None, n0=5, n1=0, weights=w, b=64, N=6, D=16, rew=None, done=None, q=p, y=None):
        return lib.pw_critic_forward(obs, idx, vec, n0, n1, *weights, b, N, D, rew, done, 0.95, q, y, None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        assert text in lib.pw_last_error(), (kw, lib.pw_last_error())

    refused(b'null', obs=None)
    refused(b'null', q=None)
    for i in range(8):
        refused(b'null', weights=[None if j == i else p for j in range(8)])
    refused(b'exactly one', idx=p, vec=p)
    refused(b'exactly one', idx=None, vec=None)
    refused(b'action widths', n0=0)
    refused(b'action widths', n1=-1)
    refused(b'action widths', n0=9, n1=8)
    refused(b'N must be', N=0)
    refused(b'N must be', N=65)
    refused(b'obs_dim', D=0)
    refused(b'obs_dim', D=105)
    refused(b'b must be', b=0)
    refused(b'b must be', b=1 << 31)
    refused(b'TD target', y=p)
    refused(b'TD target', rew=p, done=p)
    refused(b'TD target', rew=p, y=p)
    refused(b'TD target', done=p, y=p)
