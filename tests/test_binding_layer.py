"""The Python layer between torch and libpworld: the launch-argument helpers of ``_lib`` and the replay ring's cursor.  Host only."""
import glob
import os

import pytest
import torch

from multiagent_rl_amd import _lib, attention, lstm, optim, sampling
from multiagent_rl_amd.replay_buffer import ReplayBuffer

IO_FIELDS = [name for name, _ in _lib.PwStepIO._fields_]


def test_ptr():
    t = torch.zeros(3)
    assert _lib.ptr(None) is None
    assert _lib.ptr(t).value == t.data_ptr()


def test_step_io_fills_the_named_fields_that_are_present():
    out = dict(obs=torch.zeros(2, 4, 3), rew=torch.zeros(2, 4), done=None, coll=torch.zeros(2, 4))
    io = _lib.step_io(out, ('obs', 'rew', 'done', 'terminal'))   # done is None, terminal absent, coll not named
    want = dict(obs=out['obs'].data_ptr(), rew=out['rew'].data_ptr())
    for name in IO_FIELDS:
        assert (getattr(io, name) or 0) == want.get(name, 0), name
    act = torch.zeros(2, 4, dtype=torch.int32)
    io = _lib.step_io(out, ('obs',), lead=(2, 4), device=torch.device('cpu'), act_idx=act, act_comm=None)
    assert io.act_idx == act.data_ptr() and io.obs == out['obs'].data_ptr()
    assert [name for name in IO_FIELDS if getattr(io, name)] == ['act_idx', 'obs']


def test_step_io_refuses_what_a_kernel_must_not_get():
    with pytest.raises(ValueError, match='contiguous'):
        _lib.step_io(dict(obs=torch.zeros(2, 4, 3)[:, ::2]), ('obs',))
    with pytest.raises(ValueError, match='obs'):
        _lib.step_io(dict(obs=torch.zeros(2, 4, 3), rew=torch.zeros(2, 5)), ('rew', 'obs'), lead=(2, 5))
    with pytest.raises(ValueError, match='rew'):
        _lib.step_io(dict(rew=torch.zeros(2)), ('rew',), lead=(2, 4))      # shorter than the prefix
    with pytest.raises(ValueError, match='meta'):
        _lib.step_io(dict(obs=torch.zeros(2, 4, 3)), ('obs',), device=torch.device('meta'))


@pytest.mark.parametrize('family', [attention.FAMILY, lstm.FAMILY, sampling.FAMILY, optim.FAMILY])
def test_check_f32_names_the_family_for_a_cpu_tensor(family):
    assert 'no CPU fallback' in family
    with pytest.raises(RuntimeError) as err:
        _lib.check_f32(torch.zeros(3), 'x', family)
    assert 'no CPU fallback' in str(err.value) and family in str(err.value) and str(err.value).startswith('x is on cpu')


def test_the_ring_cursor_is_one_statement():
    for move in ('_advance', 'note_graph_adds'):
        rb = ReplayBuffer(10)
        getattr(rb, move)(7)
        assert (rb._next_idx, len(rb)) == (7, 7)
        getattr(rb, move)(7)
        assert (rb._next_idx, len(rb)) == (4, 10)
        rb.clear()
        assert (rb._next_idx, len(rb)) == (0, 0)


def test_only_lib_builds_launch_arguments_and_only_the_ring_moves_its_cursor():
    here = os.path.dirname(os.path.abspath(_lib.__file__))
    for path in sorted(glob.glob(os.path.join(here, '*.py'))):
        name, text = os.path.basename(path), open(path).read()
        if name == '_lib.py':
            continue
        assert 'cuda_stream' not in text and 'PwStepIO(' not in text, name
        if name != 'replay_buffer.py':
            assert '_next_idx =' not in text and '_next_idx, ' not in text, name
