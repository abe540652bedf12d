"""The learner's LSTMs WITH gradient on the HIP kernels: ``lstm_recurrence`` (an autograd function over ``pw_lstm_train_forward`` /
``pw_lstm_train_backward``), ``FusedLSTM`` (an ``nn.LSTM`` whose ``forward`` uses it) and ``fuse_lstm`` / ``unfuse_lstm``.

Each of the three passes with gradient of an update (``critic(s0, a0)``, ``actor(s0)``, ``critic(s0, actor(s0))``) runs an
``nn.LSTM`` over the agent axis; on MIOpen's RNN path that is ~45 small kernels per direction for a length-6 sequence, forward
alone.  Here the recurrent part is ONE launch forward and ONE backward; everything that is a GEMM stays a torch GEMM under
ordinary autograd: the input projection ``G = x W_ih^T + b_ih + b_hh`` (so ``x``, ``W_ih`` and both biases get their gradients from
``F.linear``) and the two ``W_hh`` gradients (``dG^T`` against the output shifted by one step).

``wgrad=True`` (``fuse_lstm``, ``lstm_recurrence``; off by default) takes those two ``W_hh`` gradients off torch as well: instead of two
strided copies and a rocBLAS GEMM per direction, ONE ``pw_lstm_train_wgrad`` (two device kernels for both directions) reads ``dG`` and
the shifted ``Y`` in place and sums in an order that depends on the shape alone -- another order than rocBLAS's, so the last bits of
``W_hh.grad`` differ across the switch.

Shapes served, the two the reference's networks have: one direction with 64 hidden units (``CriticNetwork.lstm``,
``BiCNetCritic.lstm``) and two directions with 32 (``ActorNetwork.bilstm``); one layer, ``batch_first``, zero initial state,
float32 on the GPU.  Anything else raises: there is no CPU fallback.  Gate activations are ``v_exp_f32`` / ``v_rcp_f32``
(``csrc/pw_lstm_math.hpp``), so results differ from MIOpen's in the last bits and a seeded run does not reproduce across the
switch -- which is why it is opt-in everywhere (``accelerate_trainer(trainer, lstm=True)``).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

SERVED = ((1, 64), (2, 32))   # (directions, hidden units)


def _served(dirs, H):
    return (int(dirs), int(H)) in SERVED


FAMILY = 'the LSTM kernels run on the GPU (no CPU fallback; unfuse_lstm restores nn.LSTM)'


def _shape(G, w_hh_fw, w_hh_bw):
    if G.dim() != 4 or G.shape[3] % 4:
        raise ValueError('G must be [b, N, dirs, 4 H] (got %r)' % (tuple(G.shape),))
    b, N, dirs, H = G.shape[0], G.shape[1], G.shape[2], G.shape[3] // 4
    if not _served(dirs, H):
        raise ValueError('dirs = %d, H = %d: the shapes served are %s' % (dirs, H, ' and '.join('dirs = %d, H = %d' % s for s in SERVED)))
    if b < 1 or N < 1:
        raise ValueError('G must hold at least one sequence of at least one step (got %r)' % (tuple(G.shape),))
    if (w_hh_bw is not None) != (dirs == 2):
        raise ValueError('w_hh_bw comes with dirs = 2 and only then')
    for w in (w_hh_fw, w_hh_bw):
        if w is not None and tuple(w.shape) != (4 * H, H):
            raise ValueError('W_hh must be [4 H, H] = %r (got %r)' % ((4 * H, H), tuple(w.shape)))
    return b, N, dirs, H


# ---- the overridable pieces: the launches.  A CPU test replaces them with torch stand-ins of the same signature. ------------
def launch_forward(G, w_hh_fw, w_hh_bw, keep):
    """G [b,N,dirs,4H] contiguous -> (Y [b,N,dirs*H], saved [b,N,dirs,5,H] or None when not ``keep``): one ``pw_lstm_train_forward``."""
    b, N, dirs, H = _shape(G, w_hh_fw, w_hh_bw)
    _lib.check_f32(G, 'G', FAMILY)
    _lib.check_f32(w_hh_fw, 'w_hh_fw', FAMILY, G.device, 'G')
    if w_hh_bw is not None:
        _lib.check_f32(w_hh_bw, 'w_hh_bw', FAMILY, G.device, 'G')
    Y = torch.empty((b, N, dirs * H), dtype=torch.float32, device=G.device)
    saved = torch.empty((b, N, dirs, 5, H), dtype=torch.float32, device=G.device) if keep else None
    p = _lib.ptr
    _lib.check(_lib.load().pw_lstm_train_forward(p(G), p(w_hh_fw), p(w_hh_bw), b, N, dirs, H, p(Y), p(saved), _lib.stream(G.device)))
    return Y, saved


def launch_backward(dY, saved, w_hh_fw, w_hh_bw):
    """dY [b,N,dirs*H] contiguous, saved as ``launch_forward`` returned it -> dG [b,N,dirs,4H]: one ``pw_lstm_train_backward``."""
    b, N, dirs, _, H = saved.shape
    _lib.check_f32(dY, 'dY', FAMILY)
    _lib.check_f32(saved, 'saved', FAMILY, dY.device, 'G')
    if tuple(dY.shape) != (b, N, dirs * H):
        raise ValueError('dY must be %r (got %r)' % ((b, N, dirs * H), tuple(dY.shape)))
    dG = torch.empty((b, N, dirs, 4 * H), dtype=torch.float32, device=dY.device)
    p = _lib.ptr
    _lib.check(_lib.load().pw_lstm_train_backward(p(dY), p(saved), p(w_hh_fw), p(w_hh_bw), b, N, dirs, H, p(dG), _lib.stream(dY.device)))
    return dG


def launch_wgrad(dG, Y, want_fw, want_bw):
    """dG [b,N,dirs,4H] as ``launch_backward`` returned it, Y [b,N,dirs*H] as ``launch_forward`` did -> (dW_hh forward [4H,H] or None,
    dW_hh reverse [4H,H] or None), each where wanted: one ``pw_lstm_train_wgrad``.  The scratch is a torch tensor: a graph capture
    sees an ordinary allocation."""
    if dG.dim() != 4 or dG.shape[3] % 4:
        raise ValueError('dG must be [b, N, dirs, 4 H] (got %r)' % (tuple(dG.shape),))
    b, N, dirs, H = dG.shape[0], dG.shape[1], dG.shape[2], dG.shape[3] // 4
    if not _served(dirs, H):
        raise ValueError('dirs = %d, H = %d: the shapes served are %s' % (dirs, H, ' and '.join('dirs = %d, H = %d' % s for s in SERVED)))
    if b < 1 or N < 1:
        raise ValueError('dG must hold at least one sequence of at least one step (got %r)' % (tuple(dG.shape),))
    if tuple(Y.shape) != (b, N, dirs * H):
        raise ValueError('Y must be %r (got %r)' % ((b, N, dirs * H), tuple(Y.shape)))
    if want_bw and dirs == 1:
        raise ValueError('want_bw comes with dirs = 2 and only then')
    if not (want_fw or want_bw):
        raise ValueError('launch_wgrad: neither direction is wanted')
    _lib.check_f32(dG, 'dG', FAMILY)
    _lib.check_f32(Y, 'Y', FAMILY, dG.device, 'dG')
    lib = _lib.load()
    d_fw = torch.empty((4 * H, H), dtype=torch.float32, device=dG.device) if want_fw else None
    d_bw = torch.empty((4 * H, H), dtype=torch.float32, device=dG.device) if want_bw else None
    scratch = torch.empty(lib.pw_lstm_train_wgrad_scratch_bytes(b, N, dirs, H) // 4, dtype=torch.float32, device=dG.device)
    p = _lib.ptr
    _lib.check(lib.pw_lstm_train_wgrad(p(dG), p(Y), b, N, dirs, H, p(d_fw), p(d_bw), p(scratch), _lib.stream(dG.device)))
    return d_fw, d_bw


# Sequence lengths at which ``wgrad=True`` still takes the two GEMMs, per (dirs, H): read from profiles/lstm_wgrad.txt
# (tools/lstm_wgrad_bench.py part (a): an N at which the GEMM path is ahead by more than the spread of its own repeats).
WGRAD_HANDED_BACK = {(1, 64): (), (2, 32): ()}


class _Recurrence(torch.autograd.Function):
    """(G, w_hh_fw, w_hh_bw or None, keep, wgrad) -> (Y, saved or None).  ``saved`` carries no gradient; it is kept when an input needs a
    gradient or the caller asks for it (``FusedLSTM`` reads ``c_n`` from it).  ``wgrad``: the W_hh gradients from ``launch_wgrad``."""

    @staticmethod
    def forward(ctx, G, w_hh_fw, w_hh_bw, keep, wgrad=False):
        ctx.wgrad = bool(wgrad)
        if ctx.wgrad:   # no gradient ever arrives for ``saved``: without this autograd fills a tensor of its size with zeros per backward
            ctx.set_materialize_grads(False)
        need = any(ctx.needs_input_grad[:3])
        Y, saved = launch_forward(G.contiguous(), w_hh_fw, w_hh_bw, need or keep)
        if need:
            ctx.save_for_backward(saved, Y, w_hh_fw, w_hh_bw)
        if saved is not None:
            ctx.mark_non_differentiable(saved)
        return Y, saved

    @staticmethod
    @once_differentiable
    def backward(ctx, dY, _):
        saved, Y, w_hh_fw, w_hh_bw = ctx.saved_tensors
        H = saved.shape[4]
        if dY is None:   # only with the switch on (gradients not materialised): nothing reached Y
            return None, None, None, None, None
        dG = launch_backward(dY.contiguous(), saved, w_hh_fw, w_hh_bw)   # autograd hands over expanded zero-stride gradients (Y.sum())
        d_fw = d_bw = None
        if ctx.wgrad and dG.shape[1] not in WGRAD_HANDED_BACK[(dG.shape[2], H)]:
            want_fw, want_bw = ctx.needs_input_grad[1], w_hh_bw is not None and ctx.needs_input_grad[2]
            if want_fw or want_bw:
                d_fw, d_bw = launch_wgrad(dG, Y, want_fw, want_bw)
            return (dG if ctx.needs_input_grad[0] else None), d_fw, d_bw, None, None
        # dW_hh = sum over the steps of dG_t^T h_prev: the forward direction's previous step is t - 1, the reverse direction's t + 1
        if ctx.needs_input_grad[1]:
            d_fw = dG[:, 1:, 0].reshape(-1, 4 * H).t() @ Y[:, :-1, :H].reshape(-1, H)
        if w_hh_bw is not None and ctx.needs_input_grad[2]:
            d_bw = dG[:, :-1, 1].reshape(-1, 4 * H).t() @ Y[:, 1:, H:].reshape(-1, H)
        return (dG if ctx.needs_input_grad[0] else None), d_fw, d_bw, None, None


def _recurrence(G, w_hh_fw, w_hh_bw, keep, wgrad=False):
    if not torch.is_grad_enabled():   # under no_grad the function still sees requires_grad inputs: detached, it stores nothing
        G, w_hh_fw, w_hh_bw = G.detach(), w_hh_fw.detach(), None if w_hh_bw is None else w_hh_bw.detach()
    return _Recurrence.apply(G, w_hh_fw, w_hh_bw, keep, wgrad)


def lstm_recurrence(G, w_hh_fw, w_hh_bw=None, wgrad=False):
    """The recurrent part of a one-layer LSTM from zero initial state, differentiable once in ``G`` and both ``W_hh``.

    ``G [b,N,dirs,4H] = x W_ih^T + b_ih + b_hh`` (gate order i, f, g, o; direction 1 walks the steps backwards), ``w_hh_* [4H,H]`` as
    ``nn.LSTM`` keeps them, ``w_hh_bw`` with ``dirs = 2`` only.  Returns ``Y [b,N,dirs*H] = [h_forward | h_reverse]``.  When no input
    needs a gradient the launch stores no activations.  ``wgrad``: the backward forms the ``W_hh`` gradients with ``launch_wgrad`` (one
    call for the directions that need one, none when neither does) instead of two sliced copies and a GEMM per direction."""
    return _recurrence(G, w_hh_fw, w_hh_bw, False, wgrad)[0]


# Sequence lengths that FusedLSTM.forward hands back to nn.LSTM.forward, per (dirs, H): read from profiles/lstm_train.txt (tools/lstm_train_bench.py
# part (a): an N at which stock is ahead by more than the spread of its own repeats).  Empty: no such N was measured.
HANDED_BACK = {(1, 64): (), (2, 32): ()}


class FusedLSTM(nn.LSTM):
    """``nn.LSTM`` whose ``forward(x, hx=None)`` computes ``G`` with ONE ``F.linear`` for both directions (weights and ``b_ih + b_hh``
    concatenated) and runs the recurrence on ``lstm_recurrence``.  Parameters, ``state_dict`` keys and everything but ``forward`` are
    ``nn.LSTM``'s, so instances come from ``fuse_lstm`` (a class swap) rather than from a constructor.

    Returns ``(Y, (h_n, c_n))``.  ``h_n`` is SLICED from ``Y`` (``Y[:, -1, :H]``, and ``Y[:, 0, H:]`` for the reverse direction), so
    a gradient through it reaches the recurrence (the attention critic scores every step against it).  ``c_n`` comes from the saved
    cell state and carries NO gradient: none of the served networks uses it.  (For that ``c_n`` the launch keeps the
    activations even under ``no_grad``; ``lstm_recurrence`` alone does not.)

    Raises for ``hx is not None``, a CPU tensor, a dtype other than float32, ``num_layers != 1``, ``proj_size``, dropout, no bias, not
    ``batch_first``, unbatched input, or a shape other than 1 x 64 / 2 x 32: there is no CPU fallback."""

    def _refuse(self):
        dirs = 2 if self.bidirectional else 1
        why = None
        if self.num_layers != 1:
            why = 'num_layers = %d' % self.num_layers
        elif getattr(self, 'proj_size', 0):
            why = 'proj_size = %d' % self.proj_size
        elif self.dropout:
            why = 'dropout = %g' % self.dropout
        elif not self.bias:
            why = 'bias = False'
        elif not self.batch_first:
            why = 'batch_first = False'
        elif not _served(dirs, self.hidden_size):
            why = '%d direction(s) of %d hidden units' % (dirs, self.hidden_size)
        return why

    def forward(self, x, hx=None):
        why = self._refuse()
        if why:
            raise ValueError('FusedLSTM serves one layer, batch_first, with bias, 1 x 64 or 2 x 32 hidden units: not %s' % why)
        if hx is not None:
            raise ValueError('FusedLSTM starts from the zero state: hx must be None')
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError('FusedLSTM takes x [b, N, %d]' % self.input_size)
        # (a CPU tensor is refused by launch_forward, the piece that would touch the GPU: "no CPU fallback; unfuse_lstm restores nn.LSTM")
        if x.dtype != torch.float32 or self.weight_hh_l0.dtype != torch.float32:
            raise RuntimeError('FusedLSTM is float32 (x %s, weights %s)' % (x.dtype, self.weight_hh_l0.dtype))
        dirs, H = (2 if self.bidirectional else 1), self.hidden_size
        b, N = x.shape[0], x.shape[1]
        if N in HANDED_BACK[(dirs, H)]:
            return nn.LSTM.forward(self, x, hx)
        if dirs == 2:
            w_ih = torch.cat([self.weight_ih_l0, self.weight_ih_l0_reverse], dim=0)
            bias = torch.cat([self.bias_ih_l0 + self.bias_hh_l0, self.bias_ih_l0_reverse + self.bias_hh_l0_reverse], dim=0)
            w_bw = self.weight_hh_l0_reverse
        else:
            w_ih, bias, w_bw = self.weight_ih_l0, self.bias_ih_l0 + self.bias_hh_l0, None
        return self._from_gates(F.linear(x, w_ih, bias).view(b, N, dirs, 4 * H), w_bw)

    def forward_gates(self, G):
        """The recurrence alone, on gates formed elsewhere (``dense.front_projection``): ``G [b, N, dirs, 4 H] = x W_ih^T + b_ih + b_hh``
        -> what ``forward(x)`` returns, ``(Y, (h_n, c_n))``.  ``W_ih`` and the biases are not read here."""
        why = self._refuse()
        if why:
            raise ValueError('FusedLSTM serves one layer, batch_first, with bias, 1 x 64 or 2 x 32 hidden units: not %s' % why)
        dirs, H = (2 if self.bidirectional else 1), self.hidden_size
        if not isinstance(G, torch.Tensor) or G.dim() != 4 or tuple(G.shape[2:]) != (dirs, 4 * H):
            raise ValueError('FusedLSTM.forward_gates takes G [b, N, %d, %d]' % (dirs, 4 * H))
        return self._from_gates(G, self.weight_hh_l0_reverse if dirs == 2 else None)

    def _from_gates(self, G, w_bw):
        dirs, H = G.shape[2], self.hidden_size
        Y, saved = _recurrence(G, self.weight_hh_l0, w_bw, True, getattr(self, 'wgrad', False))
        if dirs == 2:
            h_n = torch.stack([Y[:, -1, :H], Y[:, 0, H:]], dim=0)
            c_n = torch.stack([saved[:, -1, 0, 4], saved[:, 0, 1, 4]], dim=0)
        else:
            h_n, c_n = Y[:, -1, :H].unsqueeze(0), saved[:, -1, 0, 4].unsqueeze(0)
        return Y, (h_n, c_n)


def _modules(module):
    return module.modules() if isinstance(module, nn.Module) else ()


def fuse_lstm(module, wgrad=False):
    """Every plain ``nn.LSTM`` inside ``module`` that ``FusedLSTM`` serves becomes one, by a swap of ``__class__``: parameters and
    ``state_dict`` keys stay (saved ``*_actor.pt`` / ``*_critic.pt`` files load unchanged, ``FusedActor`` / ``FusedCritic`` keep
    reading the same tensors in place), and ``copy.deepcopy`` of the network keeps it -- an instance-level ``forward`` would not
    survive the deep copy a Trainer takes for its target networks.  Returns the number of modules swapped.

    ``wgrad=True``: the swapped LSTMs, and those ``module`` already holds fused, take their ``W_hh`` gradients from ``launch_wgrad``.
    The mode is a plain instance attribute (``m.wgrad``): a deep copy keeps it, ``state_dict`` does not hold it, ``unfuse_lstm`` removes
    it.  Those already fused are not counted."""
    n = 0
    for m in _modules(module):
        if type(m) is nn.LSTM:
            m.__class__ = FusedLSTM
            if m._refuse():
                m.__class__ = nn.LSTM
            else:
                n += 1
        if wgrad and type(m) is FusedLSTM:
            m.wgrad = True
    return n


def unfuse_lstm(module):
    """The reverse of ``fuse_lstm``.  Returns the number of modules swapped back."""
    n = 0
    for m in _modules(module):
        if type(m) is FusedLSTM:
            m.__class__ = nn.LSTM
            m.__dict__.pop('wgrad', None)
            n += 1
    return n


def fuse_trainer(trainer):
    """``fuse_lstm`` on ``trainer.actor``, ``trainer.critic`` and on the target networks that are still modules (``accelerate_trainer(
    targets=True)`` has replaced them by wrappers on the no-gradient kernels).  Returns the number of LSTMs swapped."""
    return sum(fuse_lstm(getattr(trainer, name, None)) for name in ('actor', 'critic', 'target_actor', 'target_critic'))


def wgrad_trainer(trainer, dry=False):
    """Every ``FusedLSTM`` of ``trainer.actor``, ``trainer.critic`` and the target networks that are still modules takes its ``W_hh``
    gradients from ``launch_wgrad`` (``fuse_lstm(wgrad=True)``'s mode, for LSTMs that are fused already).  Returns their number;
    ``ValueError`` when there is none.  ``dry``: only the check."""
    found = [m for name in ('actor', 'critic', 'target_actor', 'target_critic') for m in _modules(getattr(trainer, name, None))
             if type(m) is FusedLSTM]
    if not found:
        raise ValueError('wgrad=True: the trainer holds no fused LSTM (accelerate_trainer(..., lstm=True, wgrad=True) / fused_lstm=True); '
                         'the W_hh gradients of a plain nn.LSTM are MIOpen\'s')
    if not dry:
        for m in found:
            m.wgrad = True
    return len(found)
