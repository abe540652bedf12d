"""The output layers of the learner's networks WITH gradient on the HIP kernels: ``head_projection`` (an autograd function over
``pw_head_train_forward`` / ``pw_head_train_backward``) and ``fuse_heads`` / ``unfuse_heads``.

All three passes with gradient of an update (``critic(s0, a0)``, ``actor(s0)``, ``critic(s0, sample(actor(s0)))``) end with

    A = relu(X) or X  ->  out_k = A W_k^T + b_k      for one to three heads on the same ``X [rows, 64]``

(the actor: the ReLU on the BiLSTM's output, then ``dense2`` or ``dense2_1`` + ``dense2_2``, and ``dense3`` in the model-learning
variant; the critics: ``dense2`` -- and ``dense3`` -- on the pooled context, or the per-step ``dense2.module`` on the LSTM's steps).  On
torch that is a ``relu`` and an ``addmm`` per head forward, and per head two ``mm`` and a column sum backward, the adds that merge the
heads' ``dX`` and ``threshold_backward``.  Here it is ONE launch forward for all heads and TWO backward (one for at most 16 rows): ``X``
is read once, the ReLU'd copy never exists (the backward takes its mask from ``X``), and a head that received no gradient -- the
critic's reward head when the actor's loss reads ``Q`` only -- is handed over as a NULL ``dOut``: no zero-fill, no work.  The parameter
gradients are sums over the rows, across workgroups: every workgroup leaves its partial sums in a scratch tensor and a second kernel
adds them as a balanced tree (the bias gradients as compensated sums) -- no floating-point atomics, and the split is a function of
``rows`` alone, so the same inputs give the same bits on every launch, eager or replayed from a graph.

Served: float32 on the GPU, 64 input features, 1 to 3 heads of 1 to 104 columns each.  ``head_projection`` raises for anything else:
there is no CPU fallback.  Sums run in another order than rocBLAS's, so results differ from the stock expression in the last bits and
a seeded run does not reproduce across the switch -- which is why it is opt-in everywhere (``accelerate_trainer(trainer, heads=True)``).

The switch on a network is a plain instance attribute, ``m.fused_heads = True``, on a network ``dense.fuse_front`` has swapped -- not
another class layer: the swapped forwards find ``_unfused`` on the instance, and a further layer without a ``forward`` of its own would
change what the layers beneath it find.  ``output_layers`` is what those forwards call for their last lines, with the switch and
without.  This module imports only ``_lib`` at load time: ``attention`` and ``dense`` import it.
"""
import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

HIDDEN = 64       # the width of X
MAX_HEADS = 3
MAX_WIDTH = 104   # the widest head (dense3 of the model actor: the observation's width)

# Agent-axis lengths at which a network with the switch still takes the stock output layers: read from profiles/head_train.txt
# (tools/head_train_bench.py: an N at which stock is ahead by more than the spread of its own repeats).  Empty: no such N was measured.
HANDED_BACK = ()

FAMILY = 'the output-layer kernels run on the GPU (no CPU fallback; unfuse_heads restores the stock expression)'


def _shape(x, weights, biases):
    """-> (rows, [n_k]) of arguments that are consistent and served; ``ValueError`` otherwise."""
    if not 1 <= len(weights) <= MAX_HEADS or len(biases) != len(weights):
        raise ValueError('weights and biases: one tensor each for 1 to %d heads (got %d and %d)' % (MAX_HEADS, len(weights), len(biases)))
    if x.dim() != 2 or x.shape[1] != HIDDEN:
        raise ValueError('x must be [rows, %d] (got %r)' % (HIDDEN, tuple(x.shape)))
    if x.shape[0] < 1:
        raise ValueError('x must hold at least one row (got %r)' % (tuple(x.shape),))
    widths = []
    for k, (w, b) in enumerate(zip(weights, biases)):
        if w.dim() != 2 or w.shape[1] != HIDDEN or tuple(b.shape) != (w.shape[0],):
            raise ValueError('head %d: the weight must be [n, %d] and the bias [n] (got %r and %r)' % (k, HIDDEN, tuple(w.shape), tuple(b.shape)))
        if not 1 <= w.shape[0] <= MAX_WIDTH:
            raise ValueError('head %d is %d columns wide: a head holds 1 to %d' % (k, w.shape[0], MAX_WIDTH))
        widths.append(w.shape[0])
    return x.shape[0], widths


def _pointers(tensors):
    """The ABI's array of addresses, one per head (None: a null entry)."""
    arr = (C.c_void_p * MAX_HEADS)()
    for i, t in enumerate(tensors):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def _widths(widths):
    return (C.c_int32 * MAX_HEADS)(*widths)


def _check_all(named, anchor):
    for what, t in named:
        if t is not None:
            _lib.check_f32(t, what, FAMILY, anchor.device if t is not anchor else None, 'x')


# ---- the overridable pieces: the two launches.  A CPU test replaces them with torch stand-ins of the same signature. ------------
def launch_forward(x, weights, biases, relu):
    """x [rows,64] contiguous, the heads' parameters in place -> [out_k [rows,n_k]]: one ``pw_head_train_forward``."""
    rows, widths = _shape(x, weights, biases)
    _check_all([('x', x)] + [('weight', w) for w in weights] + [('bias', b) for b in biases], x)
    outs = [torch.empty((rows, n), dtype=torch.float32, device=x.device) for n in widths]
    _lib.check(_lib.load().pw_head_train_forward(_lib.ptr(x), rows, int(bool(relu)), len(widths), _pointers(weights), _pointers(biases),
                                                 _widths(widths), _pointers(outs), _lib.stream(x.device)))
    return outs


def launch_backward(dOuts, x, weights, relu, want_dx):
    """dOuts: per head ``[rows,n_k]`` contiguous or None (the head received no gradient), the forward's ``x`` and weights ->
    (dx [rows,64] or None, [dW_k or None], [db_k or None]): one ``pw_head_train_backward`` (two kernels; one for at most 16 rows).  A
    head without a ``dOut`` gets no result and costs nothing.  The scratch for the per-workgroup partial sums is a torch tensor: a
    graph capture sees an ordinary allocation."""
    rows, widths = x.shape[0], [w.shape[0] for w in weights]
    if len(dOuts) != len(weights) or all(d is None for d in dOuts):
        raise ValueError('dOuts: one entry per head, at least one of them a tensor')
    _check_all([('x', x)] + [('dOut', d) for d in dOuts] + [('weight', w) for w in weights], x)
    for k, d in enumerate(dOuts):
        if d is not None and tuple(d.shape) != (rows, widths[k]):
            raise ValueError('dOut of head %d must be %r (got %r)' % (k, (rows, widths[k]), tuple(d.shape)))
    lib, dev = _lib.load(), x.device
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
    dW = [None if d is None else new(n, HIDDEN) for d, n in zip(dOuts, widths)]
    db = [None if d is None else new(n) for d, n in zip(dOuts, widths)]
    dx = new(rows, HIDDEN) if want_dx else None
    n = _widths(widths)
    nbytes = lib.pw_head_train_scratch_bytes(rows, len(widths), n)
    scratch = new(nbytes // 4)
    p = _lib.ptr
    _lib.check(lib.pw_head_train_backward(_pointers(dOuts), p(x), rows, int(bool(relu)), len(widths), _pointers(weights), n, p(dx),
                                          _pointers(dW), _pointers(db), p(scratch), nbytes, _lib.stream(dev)))
    return dx, dW, db


class _Heads(torch.autograd.Function):
    """(x, relu, heads, W_0 .. W_{heads-1}, b_0 .. b_{heads-1}) -> (out_0, ..).  ``x`` and the weights are kept only when an argument
    needs a gradient; a gradient that does not arrive stays None (no zeros are materialised for it)."""

    @staticmethod
    def forward(ctx, x, relu, heads, *params):
        weights, biases = list(params[:heads]), list(params[heads:])
        ctx.set_materialize_grads(False)
        outs = launch_forward(x, weights, biases, relu)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, *weights)
            ctx.relu, ctx.heads = relu, heads
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dOuts):
        heads, need = ctx.heads, ctx.needs_input_grad
        if all(d is None for d in dOuts):
            return (None,) * (3 + 2 * heads)
        x, weights = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        # autograd hands over expanded zero-stride gradients (out.sum())
        dx, dW, db = launch_backward([None if d is None else d.contiguous() for d in dOuts], x, weights, ctx.relu, need[0])
        return (dx, None, None) + tuple(g if need[3 + k] else None for k, g in enumerate(dW)) + \
            tuple(g if need[3 + heads + k] else None for k, g in enumerate(db))


def head_projection(x, weights, biases, relu=False):
    """``out_k = (relu(x) if relu else x) W_k^T + b_k`` for every head, as a tuple; differentiable once in every tensor argument.

    ``x``: ``[rows, 64]`` or ``[b, N, 64]`` (the outputs then are ``[b, N, n_k]``); ``weights`` / ``biases``: a tensor each, or
    sequences of one to three (``nn.Linear`` layout, 1 to 104 rows).  One launch forward for all heads; the backward forms ``dx`` only
    when ``x`` needs a gradient, and nothing at all for a head whose output received no gradient (its parameters' gradients stay
    None).  When no argument needs a gradient, or under ``no_grad``, nothing is kept."""
    weights = [weights] if isinstance(weights, torch.Tensor) else list(weights)
    biases = [biases] if isinstance(biases, torch.Tensor) else list(biases)
    lead = tuple(x.shape[:-1])
    if x.dim() not in (2, 3):
        raise ValueError('x must be [rows, %d] or [b, N, %d] (got %r)' % (HIDDEN, HIDDEN, tuple(x.shape)))
    flat = x.reshape(-1, x.shape[-1]).contiguous()
    _shape(flat, weights, biases)
    args = [flat] + weights + biases
    if not torch.is_grad_enabled():   # under no_grad the function still sees requires_grad inputs: detached, it stores nothing
        args = [t.detach() for t in args]
    outs = _Heads.apply(args[0], bool(relu), len(weights), *args[1:])
    return tuple(o.view(lead + (o.shape[-1],)) for o in outs) if len(lead) != 1 else tuple(outs)


# ---- the module surface ---------------------------------------------------------------------------------------------------------
def _lin(m):
    """The Linear of a head: the module itself, or what a TimeDistributed wrapper holds."""
    return m if isinstance(m, nn.Linear) else m.module


def _heads_of(m, kind):
    """The head modules of a swapped network, in the order of its outputs."""
    if kind == 'actor':
        heads = [m.dense2_1, m.dense2_2] if getattr(m, 'dense2', None) is None else [m.dense2]
        return heads + ([m.dense3] if getattr(m, 'dense3', None) is not None else [])
    return [m.dense2, m.dense3] if kind == 'model' else [m.dense2]


def output_layers(m, x, kind):
    """The last lines of a swapped network's forward.  ``kind``: ``'actor'`` (``x``: the BiLSTM's output BEFORE the ReLU; returns the
    policy logits, a list of two for two heads, and ``(policy, next_state)`` with a ``dense3``), ``'attention'`` (``x``: the pooled
    context; ``dense2(x)``), ``'model'`` (``(dense2(x), dense3(x))``) or ``'steps'`` (``x``: the LSTM's steps; the per-step ``dense2``).
    Without ``m.fused_heads`` these are the stock torch calls in the stock order; with it, one ``head_projection``."""
    on = m.__dict__.get('fused_heads', False) and not (x.dim() == 3 and x.shape[1] in HANDED_BACK)
    if on:
        lins = [_lin(h) for h in _heads_of(m, kind)]
        outs = head_projection(x, [lin.weight for lin in lins], [lin.bias for lin in lins], relu=kind == 'actor')
    if kind == 'actor':
        two, third = getattr(m, 'dense2', None) is None, getattr(m, 'dense3', None) is not None
        if on:
            policy = [outs[0], outs[1]] if two else outs[0]
            return (policy, outs[-1]) if third else policy
        hid = F.relu(x)
        policy = [m.dense2_1(hid), m.dense2_2(hid)] if two else m.dense2(hid)
        return (policy, m.dense3(hid)) if third else policy
    if kind == 'model':
        return (outs[0], outs[1]) if on else (m.dense2(x), m.dense3(x))
    return outs[0] if on else m.dense2(x)


def _network_kind(m):
    """``'critic'`` / ``'actor'`` if ``m`` is a network of the two families ``dense.fuse_front`` serves, else None."""
    from .attention import critic_form
    from .dense import actor_form
    return 'critic' if critic_form(m)[0] is not None else 'actor' if actor_form(m) is not None else None


def fuse_heads(module):
    """Every critic and actor inside ``module`` (``module`` itself included) that ``dense.fuse_front`` has swapped computes its output
    layers with ``head_projection``.  The mode is a plain instance attribute (``m.fused_heads``): a deep copy keeps it, ``state_dict``
    does not hold it, ``unfuse_heads`` and ``dense.unfuse_front`` remove it.  A network of the two families that is not swapped is a
    ``ValueError`` naming it; so is a head wider than the kernels serve.  Returns the number of networks switched."""
    from .attention import critic_form
    from .dense import FusedFront
    todo = []
    for m in (module.modules() if isinstance(module, nn.Module) else ()):
        kind = _network_kind(m)
        if kind is None:
            continue
        if not isinstance(m, FusedFront):
            raise ValueError('fuse_heads: %s has not been swapped by dense.fuse_front; the fused output layers are the last lines of the '
                             'swapped forwards (dense.fuse_front first, or accelerate_trainer(front=True, heads=True))' % type(m).__name__)
        heads = _heads_of(m, 'actor' if kind == 'actor' else critic_form(m)[0])
        wide = [_lin(h).out_features for h in heads if _lin(h).out_features > MAX_WIDTH]
        if wide:
            raise ValueError('fuse_heads: a head of %s is %d columns wide; the kernels serve up to %d' % (type(m).__name__, wide[0], MAX_WIDTH))
        if not m.__dict__.get('fused_heads', False):
            todo.append(m)
    for m in todo:
        m.fused_heads = True
    return len(todo)


def unfuse_heads(module):
    """The reverse of ``fuse_heads``: the attribute is removed and the swapped forwards end with the stock calls again.  Returns the
    number of networks switched back."""
    n = 0
    for m in (module.modules() if isinstance(module, nn.Module) else ()):
        if m.__dict__.pop('fused_heads', False):
            n += 1
    return n


def fuse_trainer(trainer, dry=False):
    """``fuse_heads`` on ``trainer.actor``, ``trainer.critic`` and on the target networks that are still modules
    (``accelerate_trainer(targets=True)`` has replaced them by wrappers on the no-gradient kernels).  ``dry``: only the check, nothing
    is switched.  Returns the number switched."""
    from .dense import FusedFront
    nets = [getattr(trainer, name, None) for name in ('actor', 'critic', 'target_actor', 'target_critic')]
    for net in nets[:2]:
        if not isinstance(net, FusedFront):
            raise ValueError('heads=True: %s has not been swapped by dense.fuse_front; the fused output layers need front=True '
                             '(accelerate_trainer(..., lstm=True, front=True, heads=True)) or a network that is swapped already'
                             % type(net).__name__)
    return 0 if dry else sum(fuse_heads(net) for net in nets)
