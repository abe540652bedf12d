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

What every critic of the family shares lives here too, once, and ``critic.py`` imports it (this module imports only ``_lib``): the trunk
``lstm_trunk``, the stock attention expression ``attend`` and the structural classifier ``critic_form``.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from .heads import output_layers

HIDDEN = 64       # the hidden size served
MAX_STEPS = 64    # the longest agent axis served (pw_critic_forward's bound)

# Agent-axis lengths that a fused critic hands back to the stock expression: read from profiles/attention_train.txt
# (tools/attention_bench.py: an N at which stock is ahead by more than the spread of its own repeats).  Empty: no such N was measured.
HANDED_BACK = ()


FAMILY = 'the attention kernels run on the GPU (no CPU fallback; unfuse_attention restores the stock expression)'


def _shape(Y):
    if Y.dim() != 3 or Y.shape[2] != HIDDEN:
        raise ValueError('Y must be [b, N, %d] (got %r)' % (HIDDEN, tuple(Y.shape)))
    b, N = Y.shape[0], Y.shape[1]
    if b < 1 or not 1 <= N <= MAX_STEPS:
        raise ValueError('Y must hold at least one row of 1 to %d steps (got %r)' % (MAX_STEPS, tuple(Y.shape)))
    return b, N


# ---- the overridable pieces: the two launches.  A CPU test replaces them with torch stand-ins of the same signature. ------------
def launch_forward(Y, relu, keep):
    """Y [b,N,64] contiguous -> (out [b,64], weight [b,N] or None when not ``keep``): one ``pw_attention_pool_forward``."""
    b, N = _shape(Y)
    _lib.check_f32(Y, 'Y', FAMILY)
    p = _lib.ptr
    out = torch.empty((b, HIDDEN), dtype=torch.float32, device=Y.device)
    weight = torch.empty((b, N), dtype=torch.float32, device=Y.device) if keep else None
    _lib.check(_lib.load().pw_attention_pool_forward(p(Y), b, N, HIDDEN, int(bool(relu)), p(out), p(weight), _lib.stream(Y.device)))
    return out, weight


def launch_backward(dOut, Y, weight, out, relu):
    """dOut [b,64] contiguous, Y as given to and weight, out as returned by ``launch_forward`` -> dY [b,N,64]: one
    ``pw_attention_pool_backward``."""
    b, N = _shape(Y)
    _lib.check_f32(Y, 'Y', FAMILY)
    p = _lib.ptr
    for t, what, shape in ((dOut, 'dOut', (b, HIDDEN)), (weight, 'weight', (b, N)), (out, 'out', (b, HIDDEN))):
        _lib.check_f32(t, what, FAMILY, Y.device, 'Y')
        if tuple(t.shape) != shape:
            raise ValueError('%s must be %r (got %r)' % (what, shape, tuple(t.shape)))
    dY = torch.empty((b, N, HIDDEN), dtype=torch.float32, device=Y.device)
    _lib.check(_lib.load().pw_attention_pool_backward(p(dOut), p(Y), p(weight), p(out), b, N, HIDDEN, int(bool(relu)), p(dY),
                                                      _lib.stream(Y.device)))
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


def attend(steps, query, relu):
    """The stock attention expression (two ``bmm``s and a softmax): every step scored against ``query``, softmax over the agent axis,
    weighted sum, ReLU if asked.  The critic modules pass ``h_n[-1]`` as the reference writes it; ``stock_attention`` the last step."""
    score = torch.bmm(steps, query.unsqueeze(2)).squeeze(2)
    weight = F.softmax(score, dim=1)
    ctx = torch.bmm(steps.transpose(1, 2), weight.unsqueeze(2)).squeeze(2)
    return F.relu(ctx) if relu else ctx


def stock_attention(steps, relu=True):
    """The same block as ``CriticNetwork.forward`` writes it, on the LSTM's output alone: the expression the kernels replace."""
    return attend(steps, steps[:, -1], relu)


# ---- what every critic of the family shares: the trunk and the question which form a module is ----------------------------------
def stock_trunk(m, obs, action):
    """The trunk as torch runs it: the cat, ``m.dense1``, the ReLU, ``m.lstm``."""
    parts = [obs] + (list(action) if isinstance(action, (list, tuple)) else [action])
    hid = F.relu(m.dense1(torch.cat(parts, dim=-1)))
    steps, (h_n, _) = m.lstm(hid, None)
    return steps, h_n


def lstm_trunk(m, obs, action):
    """``m.dense1`` on ``[obs, action...]`` (``action`` a tensor or a list of them), ReLU, ``m.lstm`` over the agent axis
    -> ``(steps [b,N,64], h_n [1,b,64])``.  ``m``: any module with the family's ``dense1`` and ``lstm``, this project's or not.  A
    module that ``dense.fuse_front`` has swapped carries its own trunk (``_front_trunk``: the same numbers from the dense-front
    kernels), whichever forward asks for it."""
    trunk = getattr(m, '_front_trunk', None)
    return stock_trunk(m, obs, action) if trunk is None else trunk(obs, action)


def _linear(m, wrapped=False):
    """``m`` (``wrapped``: ``m.module``, the TimeDistributed form) if it is a Linear, else None."""
    if wrapped:
        m = None if isinstance(m, nn.Linear) else getattr(m, 'module', None)
    return m if isinstance(m, nn.Linear) else None


def critic_form(m):
    """Which critic ``m`` is, by structure -> ``(form, head widths)``.  The trunk of all three: ``dense1`` wrapping ``Linear(., 64)`` and a
    one-layer one-direction batch_first ``lstm`` of 64 hidden units.  Then ``'attention'``: a plain ``Linear(64, k)`` ``dense2`` and no
    ``dense3``, widths ``(k,)``; ``'steps'``: ``dense2`` wraps its Linear in a ``.module`` (the per-step critic), no ``dense3``, ``(k,)``;
    ``'model'``: beside a plain ``dense2`` a plain ``Linear(64, k)`` ``dense3`` of the same width, ``(k, k)``.  Anything else (a wrapped
    ``dense3``, one beside a per-step ``dense2``, one of another width) is some other network: ``(None, ())``."""
    lin1, lstm = _linear(getattr(m, 'dense1', None), wrapped=True), getattr(m, 'lstm', None)
    if lin1 is None or lin1.out_features != HIDDEN or not isinstance(lstm, nn.LSTM):
        return None, ()
    if not (lstm.input_size == HIDDEN and lstm.hidden_size == HIDDEN and lstm.num_layers == 1 and not lstm.bidirectional
            and lstm.batch_first and not getattr(lstm, 'proj_size', 0)):
        return None, ()
    dense2, dense3 = getattr(m, 'dense2', None), getattr(m, 'dense3', None)
    plain, step = _linear(dense2), _linear(dense2, wrapped=True)
    lin2 = plain or step
    if lin2 is None or lin2.in_features != HIDDEN:
        return None, ()
    if dense3 is None:
        return ('attention' if plain else 'steps'), (lin2.out_features,)
    if plain and type(dense3) is nn.Linear and dense3.in_features == HIDDEN and dense3.out_features == lin2.out_features:
        return 'model', (lin2.out_features, dense3.out_features)
    return None, ()


# ---- the module surface ---------------------------------------------------------------------------------------------------------
class _Fused(object):
    """The one ``forward`` of the two mixins: the trunk, ``attention_pool`` in place of the attention lines, the head(s).  Everything
    else, parameters and ``state_dict`` keys included, is the original class's (``_unfused``), to whose ``forward`` an agent axis that
    is not served (or is in ``HANDED_BACK``) goes."""
    _unfused = None
    _model = False

    def forward(self, obs, action):
        if not 1 <= obs.shape[-2] <= MAX_STEPS or obs.shape[-2] in HANDED_BACK:
            return self._unfused.forward(self, obs, action)
        steps, _ = lstm_trunk(self, obs, action)   # the query is steps[:, -1] = h_n[-1] (nn.LSTM computes the same number; FusedLSTM slices it)
        ctx = attention_pool(steps, relu=not self._model)
        return output_layers(self, ctx, 'model' if self._model else 'attention')


class FusedAttention(_Fused):
    """What ``fuse_attention`` mixes in front of a critic's class: ``CriticNetwork.forward`` with the three attention lines and the
    ReLU replaced by ``attention_pool(steps, relu=True)``."""


class FusedModelAttention(_Fused):
    """What ``fuse_model_attention`` mixes in front of a model-learning critic's class (``critic.ModelCriticNetwork`` or the reference's
    ``ac_network_model_multi_gumbel.CriticNetwork``): its ``forward`` with the attention lines replaced by
    ``attention_pool(steps, relu=False)`` -- that critic has no ReLU on the context -- and both heads on the result: ``(dense2(c),
    dense3(c))``."""
    _model = True


_MIXIN = {'attention': FusedAttention, 'model': FusedModelAttention}   # the per-step form has no attention block
_classes = {}   # (mixin, original class) -> its fused subclass


def _fused_class(cls, mixin):
    if (mixin, cls) not in _classes:
        _classes[mixin, cls] = type(mixin.__name__ + cls.__name__, (mixin, cls), {'_unfused': cls, '__module__': cls.__module__})
    return _classes[mixin, cls]


def _without(cls, mixin):
    """``cls`` without the layer ``mixin`` put on it, wherever in a stack of swaps that layer sits: the class the module would have
    had if that swap had never run (the other swaps' layers are put back over what remains)."""
    made = [k for k, v in _classes.items() if v is cls]
    if not made:
        return cls
    mx, base = made[0]
    return base if issubclass(mx, mixin) else _fused_class(_without(base, mixin), mx)


def _reclass(module, new_class):
    """Every module inside ``module`` (itself included; nothing if it is no module) for which ``new_class(m)`` names a class gets it."""
    n = 0
    for m in (module.modules() if isinstance(module, nn.Module) else ()):
        cls = new_class(m)
        if cls is not None:
            m.__class__ = cls
            n += 1
    return n


def _swap(module, forms):
    """Critics of one of ``forms`` that are not swapped yet -> the fused subclass of their own class."""
    return _reclass(module, lambda m: _fused_class(type(m), _MIXIN[critic_form(m)[0]])
                    if not isinstance(m, _Fused) and critic_form(m)[0] in forms else None)


def _unswap(module, mixin):
    return _reclass(module, lambda m: _without(type(m), mixin) if isinstance(m, mixin) else None)


def fuse_attention(module):
    """Every attention critic inside ``module`` (``module`` itself included) gets ``FusedAttention.forward`` by a swap of ``__class__``
    to a subclass of its own class: parameters and ``state_dict`` keys stay, ``isinstance`` checks keep holding, and ``copy.deepcopy``
    keeps the swap (the deep copy a Trainer takes for its target network).  The subclass is made at run time, so a swapped module is
    saved by ``state_dict`` (as the Trainers do), not pickled whole.  Returns the number of critics swapped."""
    return _swap(module, ('attention',))


def unfuse_attention(module):
    """The reverse of ``fuse_attention``: every swapped critic gets the exact class it had.  Returns the number swapped back."""
    return _unswap(module, FusedAttention)


def fuse_model_attention(module):
    """``fuse_attention`` for the model-learning variant: every model critic inside ``module`` (``module`` itself included) gets
    ``FusedModelAttention.forward`` by the same swap of ``__class__``.  ``fuse_attention`` leaves such a critic alone and this function
    leaves an attention critic alone, so both may run over one container.  Returns the number of critics swapped."""
    return _swap(module, ('model',))


def unfuse_model_attention(module):
    """The reverse of ``fuse_model_attention``.  Returns the number swapped back."""
    return _unswap(module, FusedModelAttention)


def fuse_trainer(trainer):
    """``fuse_attention`` and ``fuse_model_attention`` on ``trainer.critic``, and on ``trainer.target_critic`` while it is still a module
    (``accelerate_trainer(targets=True)`` replaces it by a wrapper on the no-gradient kernel, which has its own attention).  Returns the
    number swapped."""
    return sum(_swap(getattr(trainer, name, None), _MIXIN) for name in ('critic', 'target_critic'))
