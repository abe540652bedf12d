"""The dense front of the learner's networks WITH gradient on the HIP kernels: ``front_projection`` (an autograd function over
``pw_front_train_forward`` / ``pw_front_train_backward``) and ``fuse_front`` / ``unfuse_front``.

All three passes with gradient of an update (``critic(s0, a0)``, ``actor(s0)``, ``critic(s0, sample(actor(s0)))``) begin with

    cat([obs, action]) -> dense1 (Linear(D + A, 64)) -> ReLU -> G = hid W_ih^T + (b_ih + b_hh)      [rows, 256]

which feeds the recurrence (``lstm.lstm_recurrence``).  On torch that is 5 to 9 kernels forward (the cat, the addmm, the relu, one or
two bias adds, two more cats for a BiLSTM's concatenated weights and biases, the second addmm) and 7 to 10 backward.  Here it is ONE
launch forward and TWO backward: the input row's two parts are read side by side, the weights and biases where ``nn.Linear`` and
``nn.LSTM`` keep them.  The four parameter gradients are sums over the rows, across workgroups: every workgroup leaves its partial sums
in a scratch tensor and a second kernel adds them in workgroup order -- no floating-point atomics, and the split is a function of
``rows`` alone, so the same inputs give the same bits on every launch, eager or replayed from a graph.

Served: float32 on the GPU, 64 hidden units, ``(dirs, H)`` = (1, 64) (the critics' LSTM) or (2, 32) (the actor's BiLSTM), an
observation part of 1 to 104 numbers, an action part of 0 to 16.  ``front_projection`` raises for anything else: there is no CPU
fallback.  Sums run in another order than rocBLAS's, so results differ from the stock expression in the last bits and a seeded run
does not reproduce across the switch -- which is why it is opt-in everywhere (``accelerate_trainer(trainer, front=True)``).
"""
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from . import attention as _attention
from .attention import _fused_class, _linear, _reclass, _without, attend, attention_pool, critic_form
from .heads import output_layers
from .lstm import SERVED, FusedLSTM

HIDDEN = 64       # dense1's width = the LSTM's input size
GATES = 256       # dirs * 4 H
MAX_D0 = 104      # the widest observation part
MAX_D1 = 16       # the widest action part

# Agent-axis lengths that a swapped network hands back to the stock front: read from profiles/front_train.txt
# (tools/front_train_bench.py: an N at which stock is ahead by more than the spread of its own repeats).  Empty: no such N was measured.
HANDED_BACK = ()

FAMILY = 'the dense-front kernels run on the GPU (no CPU fallback; unfuse_front restores the stock expression)'


def _seq(t):
    return [t] if isinstance(t, torch.Tensor) else list(t)


def _shape(x0, x1, w1, b1, w_ih, b_ih, b_hh):
    """-> (rows, d0, d1, dirs, H) of arguments that are consistent and served; ``ValueError`` otherwise."""
    dirs = len(w_ih)
    if not (len(b_ih) == len(b_hh) == dirs) or dirs < 1:
        raise ValueError('w_ih, b_ih and b_hh: one tensor per direction each (got %d, %d, %d)' % (dirs, len(b_ih), len(b_hh)))
    if w_ih[0].dim() != 2 or w_ih[0].shape[0] % 4:
        raise ValueError('w_ih must be [4 H, %d] (got %r)' % (HIDDEN, tuple(w_ih[0].shape)))
    H = w_ih[0].shape[0] // 4
    if (dirs, H) not in SERVED:
        raise ValueError('dirs = %d, H = %d: the shapes served are %s' % (dirs, H, ' and '.join('dirs = %d, H = %d' % s for s in SERVED)))
    if x0.dim() != 2 or (x1 is not None and x1.dim() != 2):
        raise ValueError('x0 and x1 must be [rows, d] (got %r and %r)' % (tuple(x0.shape), None if x1 is None else tuple(x1.shape)))
    rows, d0, d1 = x0.shape[0], x0.shape[1], 0 if x1 is None else x1.shape[1]
    if rows < 1:
        raise ValueError('x0 must hold at least one row (got %r)' % (tuple(x0.shape),))
    if not 1 <= d0 <= MAX_D0:
        raise ValueError('d0 = %d: the observation part holds 1 to %d numbers' % (d0, MAX_D0))
    if d1 > MAX_D1 or (x1 is not None and d1 < 1):
        raise ValueError('d1 = %d: the action part holds 1 to %d numbers, or x1 is None' % (d1, MAX_D1))
    if x1 is not None and x1.shape[0] != rows:
        raise ValueError('x1 must hold the %d rows of x0 (got %r)' % (rows, tuple(x1.shape)))
    if tuple(w1.shape) != (HIDDEN, d0 + d1) or tuple(b1.shape) != (HIDDEN,):
        raise ValueError('w1 must be %r and b1 %r (got %r and %r)' % ((HIDDEN, d0 + d1), (HIDDEN,), tuple(w1.shape), tuple(b1.shape)))
    for d in range(dirs):
        if tuple(w_ih[d].shape) != (4 * H, HIDDEN) or tuple(b_ih[d].shape) != (4 * H,) or tuple(b_hh[d].shape) != (4 * H,):
            raise ValueError('direction %d: w_ih must be %r, b_ih and b_hh %r (got %r, %r, %r)' % (
                d, (4 * H, HIDDEN), (4 * H,), tuple(w_ih[d].shape), tuple(b_ih[d].shape), tuple(b_hh[d].shape)))
    return rows, d0, d1, dirs, H


def _pair(tensors):
    """The ABI's ``const float *const [2]``: one address per direction (entry 1 null with one direction)."""
    arr = (_lib.C.c_void_p * 2)()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _check_all(named, anchor):
    for what, t in named:
        if t is not None:
            _lib.check_f32(t, what, FAMILY, anchor.device if t is not anchor else None, 'x0')


# ---- the overridable pieces: the two launches.  A CPU test replaces them with torch stand-ins of the same signature. ------------
def launch_forward(x0, x1, w1, b1, w_ih, b_ih, b_hh, keep):
    """x0 [rows,d0], x1 [rows,d1] or None, the parameters in place -> (G [rows,256], hid [rows,64] or None when not ``keep``): one
    ``pw_front_train_forward``."""
    rows, d0, d1, dirs, H = _shape(x0, x1, w1, b1, w_ih, b_ih, b_hh)
    _check_all([('x0', x0), ('x1', x1), ('w1', w1), ('b1', b1)] + [('w_ih', t) for t in w_ih] + [('b_ih', t) for t in b_ih] +
               [('b_hh', t) for t in b_hh], x0)
    G = torch.empty((rows, GATES), dtype=torch.float32, device=x0.device)
    hid = torch.empty((rows, HIDDEN), dtype=torch.float32, device=x0.device) if keep else None
    p = _lib.ptr
    _lib.check(_lib.load().pw_front_train_forward(p(x0), d0, p(x1), d1, p(w1), p(b1), _pair(w_ih), _pair(b_ih), _pair(b_hh), rows, dirs, H,
                                                  p(hid), p(G), _lib.stream(x0.device)))
    return G, hid


def launch_backward(dG, x0, x1, hid, w1, w_ih, want_dx0, want_dx1):
    """dG [rows,256] contiguous, the forward's inputs and its ``hid`` -> (dW1, db1, [dW_ih per direction], [db_gate per direction], dx0 or
    None, dx1 or None): one ``pw_front_train_backward`` (two kernels).  The scratch for the per-workgroup partial sums is a torch
    tensor: a graph capture sees an ordinary allocation."""
    dirs, H = len(w_ih), w_ih[0].shape[0] // 4
    rows, d0, d1 = x0.shape[0], x0.shape[1], 0 if x1 is None else x1.shape[1]
    _check_all([('x0', x0), ('dG', dG), ('x1', x1), ('hid', hid), ('w1', w1)] + [('w_ih', t) for t in w_ih], x0)
    if tuple(dG.shape) != (rows, GATES) or tuple(hid.shape) != (rows, HIDDEN):
        raise ValueError('dG must be %r and hid %r (got %r and %r)' % ((rows, GATES), (rows, HIDDEN), tuple(dG.shape), tuple(hid.shape)))
    lib, dev = _lib.load(), x0.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    dW1, db1 = new(HIDDEN, d0 + d1), new(HIDDEN)
    dW_ih, db_gate = [new(4 * H, HIDDEN) for _ in range(dirs)], [new(4 * H) for _ in range(dirs)]
    dx0 = new(rows, d0) if want_dx0 else None
    dx1 = new(rows, d1) if want_dx1 and x1 is not None else None
    nbytes = lib.pw_front_train_scratch_bytes(rows, d0, d1)
    scratch = new(nbytes // 4)
    p = _lib.ptr
    _lib.check(lib.pw_front_train_backward(p(dG), p(x0), d0, p(x1), d1, p(hid), p(w1), _pair(w_ih), rows, dirs, H, p(dW1), p(db1),
                                           _pair(dW_ih), _pair(db_gate), p(dx0), p(dx1), p(scratch), nbytes, _lib.stream(dev)))
    return dW1, db1, dW_ih, db_gate, dx0, dx1


class _Front(torch.autograd.Function):
    """(x0, x1 or None, w1, b1, dirs, w_ih..., b_ih..., b_hh...) -> G.  ``hid`` is kept only when an argument needs a gradient."""

    @staticmethod
    def forward(ctx, x0, x1, w1, b1, dirs, *params):
        w_ih, b_ih, b_hh = list(params[:dirs]), list(params[dirs:2 * dirs]), list(params[2 * dirs:])
        need = any(ctx.needs_input_grad)
        G, hid = launch_forward(x0, x1, w1, b1, w_ih, b_ih, b_hh, need)
        if need:
            ctx.save_for_backward(x0, x1, hid, w1, *w_ih)
            ctx.dirs = dirs
        return G

    @staticmethod
    @once_differentiable
    def backward(ctx, dG):
        x0, x1, hid, w1 = ctx.saved_tensors[:4]
        w_ih, dirs, need = list(ctx.saved_tensors[4:]), ctx.dirs, ctx.needs_input_grad
        # autograd hands over expanded zero-stride gradients (G.sum())
        dW1, db1, dW_ih, db_gate, dx0, dx1 = launch_backward(dG.contiguous(), x0, x1, hid, w1, w_ih, need[0], need[1] and x1 is not None)
        grads = [dx0, dx1, dW1 if need[2] else None, db1 if need[3] else None, None]
        grads += [g if need[5 + d] else None for d, g in enumerate(dW_ih)]
        grads += [g if need[5 + dirs + d] else None for d, g in enumerate(db_gate)]          # one vector per direction serves b_ih ...
        grads += [g if need[5 + 2 * dirs + d] else None for d, g in enumerate(db_gate)]      # ... and b_hh
        return tuple(grads)


def front_projection(x0, x1, w1, b1, w_ih, b_ih, b_hh):
    """``G = relu([x0 | x1] w1^T + b1) W_ih^T + (b_ih + b_hh)``, differentiable once in every tensor argument.

    ``x0 [rows, d0]`` (the observation rows) and ``x1 [rows, d1]`` or ``None`` (the action rows) are the two parts of the input row;
    ``w1 [64, d0 + d1]``, ``b1 [64]`` are dense1's; ``w_ih``, ``b_ih``, ``b_hh``: one tensor per direction each (a tensor, or a sequence
    of one or two) in ``nn.LSTM`` layout.  Returns ``G [rows, dirs * 4 H]``, direction 0's gate columns first: viewed as
    ``[b, N, dirs, 4 H]`` it is what ``lstm.lstm_recurrence`` takes.  ``dx0`` / ``dx1`` are formed only for a part that needs a
    gradient, and ``hid`` is stored only when some argument does."""
    w_ih, b_ih, b_hh = _seq(w_ih), _seq(b_ih), _seq(b_hh)
    _shape(x0, x1, w1, b1, w_ih, b_ih, b_hh)
    args = [x0, x1, w1, b1] + w_ih + b_ih + b_hh
    if not torch.is_grad_enabled():   # under no_grad the function still sees requires_grad inputs: detached, it stores nothing
        args = [None if t is None else t.detach() for t in args]
    args = [None if t is None else t.contiguous() for t in args[:2]] + args[2:]
    return _Front.apply(args[0], args[1], args[2], args[3], len(w_ih), *args[4:])


# ---- the module surface ---------------------------------------------------------------------------------------------------------
def _lstm_params(lstm):
    names = ['_l0'] + (['_l0_reverse'] if lstm.bidirectional else [])
    return tuple([getattr(lstm, kind + n) for n in names] for kind in ('weight_ih', 'bias_ih', 'bias_hh'))


def front_gates(lin, lstm, x0, x1):
    """``lin`` (dense1's Linear) and ``lstm`` (a ``FusedLSTM``) on ``x0 [b,N,d0]``, ``x1 [b,N,d1]`` or None -> what ``lstm`` returns for
    ``relu(lin(cat([x0, x1])))``: ``front_projection`` and ``FusedLSTM.forward_gates``."""
    if not isinstance(lstm, FusedLSTM):
        raise ValueError('the fused front feeds FusedLSTM.forward_gates: the network\'s LSTM is a plain nn.LSTM (lstm.fuse_lstm first, '
                         'or accelerate_trainer(lstm=True, front=True))')
    if x0.dim() != 3 or (x1 is not None and (x1.dim() != 3 or x1.shape[:2] != x0.shape[:2])):
        raise ValueError('the fused front takes obs [b, N, D] and actions [b, N, A] (got %r and %r)' % (
            tuple(x0.shape), None if x1 is None else tuple(x1.shape)))
    b, N = x0.shape[0], x0.shape[1]
    w_ih, b_ih, b_hh = _lstm_params(lstm)
    G = front_projection(x0.reshape(b * N, x0.shape[2]), None if x1 is None else x1.reshape(b * N, x1.shape[2]), lin.weight, lin.bias,
                         w_ih, b_ih, b_hh)
    return lstm.forward_gates(G.view(b, N, len(w_ih), GATES // len(w_ih)))


class FusedFront(object):
    """What ``fuse_front`` mixes in front of a network's class.  Everything but ``forward`` (and the trunk the critic family shares),
    parameters and ``state_dict`` keys included, is the original class's."""
    _unfused = None


class FusedFrontCritic(FusedFront):
    """A critic of the family ``attention.critic_form`` recognises: the trunk is ``front_gates``; what follows is the form's own --
    the attention (``attention_pool`` while the module is also a fused-attention critic, else the stock expression) and the head(s),
    or the per-step head."""

    def _front_trunk(self, obs, action):
        """``attention.lstm_trunk`` of a swapped critic -> ``(steps [b,N,64], h_n [1,b,64])``."""
        if obs.dim() == 3 and obs.shape[1] in HANDED_BACK:
            return _attention.stock_trunk(self, obs, action)
        rest = list(action) if isinstance(action, (list, tuple)) else [action]
        x1 = rest[0] if len(rest) == 1 else torch.cat(rest, dim=-1)
        steps, (h_n, _) = front_gates(_linear(self.dense1, wrapped=True), self.lstm, obs, x1)
        return steps, h_n

    def forward(self, obs, action):
        form = critic_form(self)[0]
        steps, h_n = self._front_trunk(obs, action)
        if form == 'steps':
            return output_layers(self, steps, 'steps')
        model = form == 'model'
        if isinstance(self, _attention._Fused) and 1 <= steps.shape[1] <= _attention.MAX_STEPS and steps.shape[1] not in _attention.HANDED_BACK:
            ctx = attention_pool(steps, relu=not model)
        else:
            ctx = attend(steps, h_n[-1], relu=not model)
        return output_layers(self, ctx, form)


class FusedFrontActor(FusedFront):
    """An actor recognised by ``actor_form``: ``front_gates`` on the observation alone, then the ReLU and the head(s) as
    ``policy.ActorNetwork`` / ``policy.ModelActorNetwork`` write them (``heads.output_layers``)."""

    def forward(self, obs):
        if obs.dim() == 3 and obs.shape[1] in HANDED_BACK:
            return self._unfused.forward(self, obs)
        hid, _ = front_gates(_linear(self.dense1, wrapped=True), self.bilstm, obs, None)
        return output_layers(self, hid, 'actor')


def actor_form(m):
    """The number of policy heads (1: ``dense2``; 2: ``dense2_1`` + ``dense2_2``) if ``m`` is an actor of the family by structure --
    ``dense1`` wrapping ``Linear(., 64)``, a one-layer batch_first ``bilstm`` of 2 x 32 hidden units, the head(s), an optional
    ``dense3`` -- else None."""
    lin1, lstm = _linear(getattr(m, 'dense1', None), wrapped=True), getattr(m, 'bilstm', None)
    if lin1 is None or lin1.out_features != HIDDEN or not isinstance(lstm, nn.LSTM):
        return None
    if not (lstm.input_size == HIDDEN and lstm.hidden_size == 32 and lstm.num_layers == 1 and lstm.bidirectional and lstm.batch_first
            and not getattr(lstm, 'proj_size', 0)):
        return None
    head = lambda name: _linear(getattr(m, name, None), wrapped=True) or _linear(getattr(m, name, None))  # noqa: E731
    ok = lambda lin: lin is not None and lin.in_features == HIDDEN  # noqa: E731
    if getattr(m, 'dense3', None) is not None and not ok(head('dense3')):
        return None
    if ok(head('dense2_1')) and ok(head('dense2_2')) and getattr(m, 'dense2', None) is None:
        return 2
    if ok(head('dense2')) and getattr(m, 'dense2_1', None) is None and getattr(m, 'dense2_2', None) is None:
        return 1
    return None


def _front_class(m):
    """The class ``fuse_front`` gives ``m``, or None if ``m`` is no network of the two families (or is swapped already)."""
    if isinstance(m, FusedFront):
        return None
    if critic_form(m)[0] is not None:
        mixin, lstm = FusedFrontCritic, m.lstm
    elif actor_form(m) is not None:
        mixin, lstm = FusedFrontActor, m.bilstm
    else:
        return None
    if not isinstance(lstm, FusedLSTM):
        raise ValueError('fuse_front: the LSTM of %s is a plain nn.LSTM; the fused front feeds FusedLSTM.forward_gates (lstm.fuse_lstm '
                         'first, or accelerate_trainer(lstm=True, front=True))' % type(m).__name__)
    width = _linear(m.dense1, wrapped=True).in_features
    if width > MAX_D0 + MAX_D1:
        raise ValueError('fuse_front: dense1 of %s takes %d numbers; the kernels serve up to %d + %d' % (type(m).__name__, width, MAX_D0, MAX_D1))
    return _fused_class(type(m), mixin)


def fuse_front(module):
    """Every critic (``attention.critic_form``) and actor (``actor_form``) inside ``module`` (``module`` itself included) computes its
    front with ``front_projection`` and its recurrence with ``FusedLSTM.forward_gates``, by a swap of ``__class__`` to a run-time
    subclass of its own class: parameters and ``state_dict`` keys stay, ``isinstance`` checks keep holding, ``copy.deepcopy`` keeps the
    swap, and it composes with ``fuse_attention`` / ``fuse_model_attention`` in either order.  The network's LSTM must be a
    ``FusedLSTM`` already (``ValueError`` otherwise).  Returns the number of networks swapped."""
    return _reclass(module, _front_class)


def unfuse_front(module):
    """The reverse of ``fuse_front``: every swapped network gets exactly the class it had without it (a fused-attention class stays
    one).  The ``fused_heads`` mode (``heads.fuse_heads``), which lives in the swapped forwards' last lines, goes with it.  Returns the
    number swapped back."""
    from .heads import unfuse_heads
    unfuse_heads(module)
    return _reclass(module, lambda m: _without(type(m), FusedFront) if isinstance(m, FusedFront) else None)


def fuse_trainer(trainer):
    """``fuse_front`` on ``trainer.actor``, ``trainer.critic`` and on the target networks that are still modules
    (``accelerate_trainer(targets=True)`` has replaced them by wrappers on the no-gradient kernels).  Returns the number swapped."""
    return sum(fuse_front(getattr(trainer, name, None)) for name in ('actor', 'critic', 'target_actor', 'target_critic'))
