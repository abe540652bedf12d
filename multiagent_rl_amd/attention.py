"""The attention block of the learner's critic WITH gradient on the HIP kernels: ``attention_pool`` (an autograd function over
``pw_attention_pool_forward`` / ``pw_attention_pool_backward``) and ``fuse_attention`` / ``unfuse_attention``.

``CriticNetwork.forward`` scores every LSTM step against the last one, takes a softmax over the agent axis, a weighted sum and a
ReLU (``critic.py``): ``bmm``, ``softmax``, ``bmm``, ``relu`` forward and about a dozen kernels backward, on N x 64 numbers per batch
row and without a parameter.  Both critic passes with gradient of an update run it (``critic(s0, a0)``, ``critic(s0, actor(s0))``).
Here the block is ONE launch forward and ONE backward; dense1, the LSTM and dense2 stay what they are.

Served: float32 on the GPU, 64 hidden units, an agent axis of 1 to ``MAX_STEPS``; the query is the last step of the LSTM's output
(``h_n[-1]`` of a one-direction LSTM).  ``attention_pool`` raises for anything else: there is no CPU fallback.  A fused critic hands an
agent axis the kernels do not serve (or one listed in ``HANDED_BACK``) to the forward of the class it was swapped from.  Sums run in
another order than rocBLAS's, so results differ from the stock expression in the last bits and a seeded run does not reproduce
across the switch -- which is why it is opt-in everywhere (``accelerate_trainer(trainer, attention=True)``).

The critic of the model-learning variant (``critic.ModelCriticNetwork``: the same block WITHOUT the ReLU, then two heads) is served by
``fuse_model_attention`` / ``unfuse_model_attention``: the same swap, ``attention_pool(steps, relu=False)``, a pair returned.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

HIDDEN = 64       # the hidden size served
MAX_STEPS = 64    # the longest agent axis served (pw_critic_forward's bound)

# Agent-axis lengths that a fused critic hands back to the stock expression: read from profiles/attention_train.txt
# (tools/attention_bench.py: an N at which stock is ahead by more than the spread of its own repeats).  Empty: no such N was measured.
HANDED_BACK = ()


def _check(t, what, device=None):
    if t.device.type != 'cuda':
        raise RuntimeError('%s is on %s: the attention kernels run on the GPU (no CPU fallback; unfuse_attention restores the stock '
                           'expression)' % (what, t.device))
    if device is not None and t.device != device:
        raise RuntimeError('%s is on %s, Y on %s' % (what, t.device, device))
    if t.dtype != torch.float32:
        raise RuntimeError('%s must be float32 (got %s)' % (what, t.dtype))
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % what)


def _shape(Y):
    if Y.dim() != 3 or Y.shape[2] != HIDDEN:
        raise ValueError('Y must be [b, N, %d] (got %r)' % (HIDDEN, tuple(Y.shape)))
    b, N = Y.shape[0], Y.shape[1]
    if b < 1 or not 1 <= N <= MAX_STEPS:
        raise ValueError('Y must hold at least one row of 1 to %d steps (got %r)' % (MAX_STEPS, tuple(Y.shape)))
    return b, N


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ---- the overridable pieces: the two launches.  A CPU test replaces them with torch stand-ins of the same signature. ------------
def launch_forward(Y, relu, keep):
    """Y [b,N,64] contiguous -> (out [b,64], weight [b,N] or None when not ``keep``): one ``pw_attention_pool_forward``."""
    b, N = _shape(Y)
    _check(Y, 'Y')
    out = torch.empty((b, HIDDEN), dtype=torch.float32, device=Y.device)
    weight = torch.empty((b, N), dtype=torch.float32, device=Y.device) if keep else None
    _lib.check(_lib.load().pw_attention_pool_forward(_p(Y), b, N, HIDDEN, int(bool(relu)), _p(out), _p(weight),
                                                     C.c_void_p(torch.cuda.current_stream(Y.device).cuda_stream)))
    return out, weight


def launch_backward(dOut, Y, weight, out, relu):
    """dOut [b,64] contiguous, Y as given to and weight, out as returned by ``launch_forward`` -> dY [b,N,64]: one
    ``pw_attention_pool_backward``."""
    b, N = _shape(Y)
    _check(Y, 'Y')
    for t, what, shape in ((dOut, 'dOut', (b, HIDDEN)), (weight, 'weight', (b, N)), (out, 'out', (b, HIDDEN))):
        _check(t, what, Y.device)
        if tuple(t.shape) != shape:
            raise ValueError('%s must be %r (got %r)' % (what, shape, tuple(t.shape)))
    dY = torch.empty((b, N, HIDDEN), dtype=torch.float32, device=Y.device)
    _lib.check(_lib.load().pw_attention_pool_backward(_p(dOut), _p(Y), _p(weight), _p(out), b, N, HIDDEN, int(bool(relu)), _p(dY),
                                                      C.c_void_p(torch.cuda.current_stream(Y.device).cuda_stream)))
    return dY


class _Pool(torch.autograd.Function):
    """(Y, relu) -> out.  (Y, weight, out) are kept only when Y needs a gradient."""

    @staticmethod
    def forward(ctx, Y, relu):
        need = ctx.needs_input_grad[0]
        Y = Y.contiguous()
        out, weight = launch_forward(Y, relu, need)
        if need:
            ctx.save_for_backward(Y, weight, out)
            ctx.relu = relu
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dOut):
        Y, weight, out = ctx.saved_tensors
        return launch_backward(dOut.contiguous(), Y, weight, out, ctx.relu), None   # autograd hands over expanded zero-stride gradients (out.sum())


def attention_pool(Y, relu=True):
    """``Y [b,N,64]`` (the LSTM's output) -> ``[b,64]``: ``s_t = <Y_t, Y_{N-1}>``, ``w = softmax_t(s)``, ``c = sum_t w_t Y_t``, and
    ``max(c, 0)`` with ``relu``.  Differentiable once in ``Y``; when ``Y`` needs no gradient the launch stores no weights."""
    if not torch.is_grad_enabled():   # under no_grad the function still sees a requires_grad input: detached, it stores nothing
        Y = Y.detach()
    return _Pool.apply(Y, bool(relu))


def stock_attention(steps, relu=True):
    """The same block as ``CriticNetwork.forward`` writes it (two ``bmm``s and a softmax): the expression the kernels replace."""
    score = torch.bmm(steps, steps[:, -1].unsqueeze(2)).squeeze(2)
    weight = F.softmax(score, dim=1)
    ctx = torch.bmm(steps.transpose(1, 2), weight.unsqueeze(2)).squeeze(2)
    return F.relu(ctx) if relu else ctx


# ---- the module surface ---------------------------------------------------------------------------------------------------------
class FusedAttention(object):
    """What ``fuse_attention`` mixes in front of a critic's class: ``CriticNetwork.forward`` with the three attention lines and the
    ReLU replaced by ``attention_pool(steps, relu=True)``.  Everything else, parameters and ``state_dict`` keys included, is the
    original class's (``_unfused``), to whose ``forward`` an agent axis that is not served (or is in ``HANDED_BACK``) goes."""
    _unfused = None

    def forward(self, obs, action):
        if not 1 <= obs.shape[-2] <= MAX_STEPS or obs.shape[-2] in HANDED_BACK:
            return self._unfused.forward(self, obs, action)
        parts = [obs] + (list(action) if isinstance(action, (list, tuple)) else [action])
        hid = F.relu(self.dense1(torch.cat(parts, dim=-1)))
        steps, _ = self.lstm(hid, None)   # the query is steps[:, -1] = h_n[-1] (nn.LSTM computes the same number; FusedLSTM slices it)
        return self.dense2(attention_pool(steps, relu=True))


class FusedModelAttention(object):
    """What ``fuse_model_attention`` mixes in front of a model-learning critic's class (``critic.ModelCriticNetwork`` or the reference's
    ``ac_network_model_multi_gumbel.CriticNetwork``): its ``forward`` with the attention lines replaced by
    ``attention_pool(steps, relu=False)`` -- that critic has no ReLU on the context -- and both heads on the result: ``(dense2(c),
    dense3(c))``.  Handing back as ``FusedAttention``."""
    _unfused = None

    def forward(self, obs, action):
        if not 1 <= obs.shape[-2] <= MAX_STEPS or obs.shape[-2] in HANDED_BACK:
            return self._unfused.forward(self, obs, action)
        parts = [obs] + (list(action) if isinstance(action, (list, tuple)) else [action])
        hid = F.relu(self.dense1(torch.cat(parts, dim=-1)))
        steps, _ = self.lstm(hid, None)
        ctx = attention_pool(steps, relu=False)
        return self.dense2(ctx), self.dense3(ctx)


_classes = {}   # (mixin, original class) -> its fused subclass


def _fused_class(cls, mixin=FusedAttention):
    if (mixin, cls) not in _classes:
        _classes[mixin, cls] = type(mixin.__name__ + cls.__name__, (mixin, cls), {'_unfused': cls, '__module__': cls.__module__})
    return _classes[mixin, cls]


def _is_attention_critic(m):
    """By structure, as ``FusedCritic`` reads it: ``dense1`` wrapping ``Linear(., 64)``, a one-layer one-direction batch_first ``lstm`` of 64
    hidden units, a plain ``Linear(64, .)`` ``dense2`` and no ``dense3`` (the model-learning variant: no ReLU, a second head --
    ``fuse_model_attention``'s)."""
    return not hasattr(m, 'dense3') and _has_attention_trunk(m)


def _has_attention_trunk(m):
    lin1 = getattr(getattr(m, 'dense1', None), 'module', None)
    lstm, lin2 = getattr(m, 'lstm', None), getattr(m, 'dense2', None)
    if not isinstance(lin1, nn.Linear) or not isinstance(lstm, nn.LSTM) or type(lin2) is not nn.Linear:
        return False
    return (lin1.out_features == HIDDEN and lstm.input_size == HIDDEN and lstm.hidden_size == HIDDEN and lstm.num_layers == 1
            and not lstm.bidirectional and lstm.batch_first and not getattr(lstm, 'proj_size', 0) and lin2.in_features == HIDDEN)


def _is_model_critic(m):
    """The model-learning critic by structure: the attention critic's trunk and, beside ``dense2``, a plain ``Linear(64, k)`` ``dense3`` of
    ``dense2``'s width (a ``dense3`` of another width is some other network: left alone)."""
    lin3 = getattr(m, 'dense3', None)
    return (type(lin3) is nn.Linear and _has_attention_trunk(m) and lin3.in_features == HIDDEN
            and lin3.out_features == m.dense2.out_features)


def _modules(module):
    return module.modules() if isinstance(module, nn.Module) else ()


def fuse_attention(module):
    """Every attention critic inside ``module`` (``module`` itself included) gets ``FusedAttention.forward`` by a swap of ``__class__``
    to a subclass of its own class: parameters and ``state_dict`` keys stay, ``isinstance`` checks keep holding, and ``copy.deepcopy``
    keeps the swap (the deep copy a Trainer takes for its target network).  The subclass is made at run time, so a swapped module is
    saved by ``state_dict`` (as the Trainers do), not pickled whole.  Returns the number of critics swapped."""
    n = 0
    for m in _modules(module):
        if not isinstance(m, FusedAttention) and _is_attention_critic(m):
            m.__class__ = _fused_class(type(m))
            n += 1
    return n


def unfuse_attention(module):
    """The reverse of ``fuse_attention``: every swapped critic gets the exact class it had.  Returns the number swapped back."""
    n = 0
    for m in _modules(module):
        if isinstance(m, FusedAttention):
            m.__class__ = type(m)._unfused
            n += 1
    return n


def fuse_model_attention(module):
    """``fuse_attention`` for the model-learning variant: every model critic inside ``module`` (``module`` itself included) gets
    ``FusedModelAttention.forward`` by the same swap of ``__class__``.  ``fuse_attention`` leaves such a critic alone and this function
    leaves an attention critic alone, so both may run over one container.  Returns the number of critics swapped."""
    n = 0
    for m in _modules(module):
        if not isinstance(m, (FusedAttention, FusedModelAttention)) and _is_model_critic(m):
            m.__class__ = _fused_class(type(m), FusedModelAttention)
            n += 1
    return n


def unfuse_model_attention(module):
    """The reverse of ``fuse_model_attention``.  Returns the number swapped back."""
    n = 0
    for m in _modules(module):
        if isinstance(m, FusedModelAttention):
            m.__class__ = type(m)._unfused
            n += 1
    return n


def fuse_trainer(trainer):
    """``fuse_attention`` and ``fuse_model_attention`` on ``trainer.critic``, and on ``trainer.target_critic`` while it is still a module
    (``accelerate_trainer(targets=True)`` replaces it by a wrapper on the no-gradient kernel, which has its own attention).  Returns the
    number swapped."""
    return sum(fuse_attention(getattr(trainer, name, None)) + fuse_model_attention(getattr(trainer, name, None))
               for name in ('critic', 'target_critic'))
