"""The learner's Gumbel-softmax sample WITH gradient on the HIP kernels: ``gumbel_st`` (an autograd function over
``pw_gumbel_st_forward`` / ``pw_gumbel_st_backward``) and ``GumbelSampler``, which numbers the draws of a learner.

``F.gumbel_softmax(logits, hard=True)`` is a dozen elementwise kernels, a softmax, a max and a scatter forward and a softmax chain
backward, and every update runs it twice: without gradient on the target actor's logits (``ddpg_gumbel_fix.py:150``) and with gradient in
the actor loss (``:178``); twice that for MultiDiscrete.  Here a sample is ONE launch forward and ONE backward.  It is also the one place
where an update draws from torch's global generator; the kernels draw from the library's own source instead -- Philox4x32-10 keyed
(seed; step, row), the draw of the actor heads -- and read the step from a device cell, so the noise of a sample is a pure function of
(seed, update number, call site, row, logit): a captured update replays with new noise, and a graphed run reproduces an eager one bit for
bit (tests/test_gpu_sampling.py).

Served: float32 on the GPU, 1 to ``MAX_LOGITS`` logits on the last axis, ``tau > 0``.  ``gumbel_st`` raises for anything else: there is
no CPU fallback.  The noise stream is not torch's, so a seeded run does not reproduce across the switch -- which is why it is opt-in
everywhere (``accelerate_trainer(trainer, sampling=True)``, the example learner's ``fused_sampling``).

What the launch computes, per row: ``v = (logits - noise) / tau``, ``idx`` = the first maximum of ``v``, ``soft = softmax(v)``, and
``y = (onehot(idx) - soft) + soft`` (``hard``; the value of torch's ``y_hard - y_soft.detach() + y_soft``) or ``y = soft``.  The
gradient is the soft sample's for both: ``dLogits_o = soft_o (dY_o - sum_k dY_k soft_k) / tau``.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib

MAX_LOGITS = 16          # four Philox blocks per row (pw_gumbel_st_forward's bound)
SITES_PER_UPDATE = 16    # the step numbers one update owns: a sampler's cell advances by this much per update
_MASK64 = (1 << 64) - 1

# The learner's default seed is the exploration seed plus this constant (mod 2^64; the 64-bit golden-ratio constant, odd, far from
# any seed a user types).  The exploration actor (``FusedActor(seed=...)``) keys the same noise function by (seed; its own call
# count, row): with another key the learner's stream never coincides with it, whatever the two step counters hold.
LEARNER_STREAM = 0x9E3779B97F4A7C15


def default_seed(exploration_seed=0):
    """The sampler seed that goes with an exploration seed: ``(exploration_seed + LEARNER_STREAM) mod 2^64``."""
    return (int(exploration_seed) + LEARNER_STREAM) & _MASK64


FAMILY = 'the sampling kernels run on the GPU (no CPU fallback; F.gumbel_softmax is the stock expression)'


def _shape(logits):
    if logits.dim() != 2:
        raise ValueError('the launch takes logits [rows, n] (got %r)' % (tuple(logits.shape),))
    rows, n = logits.shape
    if not 1 <= n <= MAX_LOGITS:
        raise ValueError('the last axis must hold 1 to %d logits (got %d): a wider head is not served' % (MAX_LOGITS, n))
    if rows < 1:
        raise ValueError('logits must hold at least one row (got %r)' % (tuple(logits.shape),))
    return rows, n


def _tau(tau):
    tau = float(tau)
    if not 0.0 < tau < float('inf'):
        raise ValueError('tau must be a finite number > 0 (got %r)' % (tau,))
    return tau


# ---- the overridable pieces: the launches.  A CPU test replaces them with torch stand-ins of the same signature. ----------------
def launch_forward(logits, tau, hard, seed, step, cell, keep, want_idx=False, want_noise=False):
    """logits [rows,n] contiguous -> ``(y, soft or None, idx or None, noise or None)``: one ``pw_gumbel_st_forward``.  The noise's step is
    ``step`` plus the content of ``cell`` (an int64 device tensor, or None).  ``soft`` is stored only when ``keep``."""
    _shape(logits)
    _lib.check_f32(logits, 'logits', FAMILY)
    tau = _tau(tau)
    if cell is not None and (cell.dtype != torch.int64 or cell.device != logits.device or cell.numel() < 1):
        raise RuntimeError('the step cell must be an int64 tensor on %s' % logits.device)
    rows, n = logits.shape
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=logits.device)  # noqa: E731
    y = new((rows, n), torch.float32)
    soft = new((rows, n), torch.float32) if keep else None
    idx = new((rows,), torch.int32) if want_idx else None
    noise = new((rows, n), torch.float32) if want_noise else None
    p = _lib.ptr
    _lib.check(_lib.load().pw_gumbel_st_forward(p(logits), rows, n, tau, int(bool(hard)), int(seed) & _MASK64, int(step) & _MASK64, p(cell),
                                                p(y), p(soft), p(idx), p(noise), _lib.stream(logits.device)))
    return y, soft, idx, noise


def launch_backward(dY, soft, tau):
    """dY [rows,n] contiguous, soft as returned by ``launch_forward`` -> dLogits [rows,n]: one ``pw_gumbel_st_backward``."""
    rows, n = _shape(soft)
    _lib.check_f32(soft, 'soft', FAMILY)
    _lib.check_f32(dY, 'dY', FAMILY, soft.device, 'the logits')
    if dY.shape != soft.shape:
        raise ValueError('dY must be %r (got %r)' % (tuple(soft.shape), tuple(dY.shape)))
    dLogits = torch.empty_like(soft)
    p = _lib.ptr
    _lib.check(_lib.load().pw_gumbel_st_backward(p(dY), p(soft), rows, n, _tau(tau), p(dLogits), _lib.stream(soft.device)))
    return dLogits


def launch_advance(cell, delta):
    """``cell += delta`` on the device, in stream order (``pw_counter_add``): inside a captured region every replay advances it."""
    _lib.check(_lib.load().pw_counter_add(_lib.ptr(cell), int(delta), 0, _lib.stream(cell.device)))


class _Sample(torch.autograd.Function):
    """(logits [rows,n], tau, hard, seed, step, cell) -> y.  ``soft`` is kept only when the logits need a gradient."""

    @staticmethod
    def forward(ctx, logits, tau, hard, seed, step, cell):
        need = ctx.needs_input_grad[0]
        y, soft, _, _ = launch_forward(logits.contiguous(), tau, hard, seed, step, cell, need)
        if need:
            ctx.save_for_backward(soft)
            ctx.tau = tau
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dY):
        soft, = ctx.saved_tensors
        return launch_backward(dY.contiguous(), soft, ctx.tau), None, None, None, None, None   # autograd may hand over an expanded dY


def _rows(logits):
    """Any leading shape -> ``[rows, n]`` (a view where the tensor allows it)."""
    if logits.dim() < 1:
        raise ValueError('logits need a last axis of 1 to %d logits (got a scalar)' % MAX_LOGITS)
    n = logits.shape[-1]
    return logits.reshape(logits.numel() // n if n else 0, n)


def gumbel_st(logits, tau=1.0, hard=True, seed=0, step=0, cell=None):
    """``F.gumbel_softmax(logits, tau, hard, dim=-1)`` with the library's noise: ``logits [..., n]`` -> the sample ``[..., n]``.  The noise
    of (row, logit) is keyed ``(seed; step + cell[0], row)``, rows counted over the flattened leading axes.  Differentiable once in
    ``logits``; when they need no gradient (or under ``no_grad``) the launch stores nothing but the sample."""
    if not torch.is_grad_enabled():   # under no_grad the function still sees a requires_grad input: detached, it stores nothing
        logits = logits.detach()
    flat = _rows(logits)
    _shape(flat)
    return _Sample.apply(flat, _tau(tau), bool(hard), int(seed), int(step), cell).reshape(logits.shape)


class GumbelSampler(object):
    """The draws of one learner, numbered: ``seed`` keys the stream, an int64 device cell holds ``SITES_PER_UPDATE`` times the number of
    finished updates, and the ``s``-th sampling call of an update (its call SITE ``s`` = 0, 1, ...) passes ``s`` as the by-value step.  The
    noise of a call is therefore a function of (seed, update number, site, row, logit) and of nothing else: not of torch's generator, not of
    whether the update runs eagerly or as a replay of a captured graph (the by-value steps are what a capture records; the cell is read by
    the kernel).  ``end_update()`` closes an update: the cell advances on the device (``pw_counter_add``, capturable) and the site count
    restarts.  A 17th site in one update is a ``ValueError``: it would draw the first site's noise of the next update.

    ``seed=None``: ``default_seed(exploration_seed)``, see ``LEARNER_STREAM``."""

    def __init__(self, seed=None, device=None, exploration_seed=0):
        self.seed = default_seed(exploration_seed) if seed is None else int(seed) & _MASK64
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.cell = torch.zeros(1, dtype=torch.int64, device=self.device)   # created here, eagerly: never inside a captured region
        self.site = 0        # host ordinal of the next call site within the current update
        self.updates = 0     # end_update() calls issued (a captured one counts when it is recorded, like the optimisers' step)

    def _next_site(self):
        if self.site >= SITES_PER_UPDATE:
            raise ValueError('GumbelSampler: more than %d sampling calls in one update (is end_update() called after each optimize()?)'
                             % SITES_PER_UPDATE)
        self.site += 1
        return self.site - 1

    def _one(self, logits, hard, tau):
        return gumbel_st(logits, tau=tau, hard=hard, seed=self.seed, step=self._next_site(), cell=self.cell)

    def sample(self, logits, hard=True, tau=1.0):
        """``logits [..., n]`` -> the sample ``[..., n]``; a list of heads: one launch (one site) each, concatenated on the last axis, as
        the example learner's ``_sample`` does."""
        if isinstance(logits, (list, tuple)):
            return torch.cat([self._one(x, hard, tau) for x in logits], dim=-1)
        return self._one(logits, hard, tau)

    def gumbel_softmax(self, x, hard=True):
        """The reference Trainer's method (``ddpg_gumbel_fix.py:109-116``): ``x [n, t, A]`` -> ``[n, t, A]``, ``tau = 1``."""
        if x.dim() != 3:
            raise ValueError('gumbel_softmax takes [n, t, A] (got %r)' % (tuple(x.shape),))
        return self._one(x, hard, 1.0)

    @torch.no_grad()
    def sample_index(self, logits, tau=1.0):
        """``logits [..., n]`` -> the sampled class per row, int32 ``[...]`` (one site; no gradient)."""
        flat = _rows(logits.detach()).contiguous()
        idx = launch_forward(flat, tau, True, self.seed, self._next_site(), self.cell, False, want_idx=True)[2]
        return idx.reshape(logits.shape[:-1])

    def end_update(self):
        """Close an update: the cell advances by ``SITES_PER_UPDATE`` in stream order and the next call is site 0 again."""
        launch_advance(self.cell, SITES_PER_UPDATE)
        self.site = 0
        self.updates += 1

    def reset(self, updates=0):
        """Set the update number (eagerly; not inside a captured region): the stream continues as after ``updates`` updates."""
        self.cell.fill_(int(updates) * SITES_PER_UPDATE)
        self.site, self.updates = 0, int(updates)


def install(trainer, seed=None, exploration_seed=0):
    """``accelerate_trainer(sampling=True)``: a ``GumbelSampler`` on the trainer's device becomes ``trainer.gumbel_softmax`` (the
    reference Trainer's method) and / or ``trainer._sample`` (the example learner's), whichever the trainer has, as INSTANCE attributes.
    A trainer that already carries a sampler (the example learner's ``fused_sampling=True``) keeps it.  -> ``(sampler, owned)``: ``owned``
    is False where the trainer closes its updates itself."""
    have = getattr(trainer, 'sampler', None)
    if isinstance(have, GumbelSampler):
        return have, False
    names = [n for n in ('gumbel_softmax', '_sample') if hasattr(trainer, n)]
    if not names:
        raise ValueError('accelerate_trainer(sampling=True): the trainer has neither a gumbel_softmax nor a _sample method to replace')
    device = getattr(trainer, 'device', None)
    if device is None:
        device = next(trainer.actor.parameters()).device
    sampler = GumbelSampler(seed=seed, device=device, exploration_seed=exploration_seed)
    if 'gumbel_softmax' in names:
        trainer.gumbel_softmax = sampler.gumbel_softmax
    if '_sample' in names:
        trainer._sample = sampler.sample
    return sampler, True
