"""The tail of a network's update on the HIP kernels: global-norm clip, Adam step and the Polyak update of the target network as
ONE launch per network (``pw_adam_step``), and the Polyak update alone (``pw_soft_update``).

What ``Trainer.optimize`` does after each backward pass (``ddpg_gumbel_fix.py:172-173,208-213``) is arithmetic on about twenty
small tensors; stock PyTorch spends a launch or several on each of them.  ``FusedAdam`` is a ``torch.optim.Optimizer`` with
torch Adam's state (``step``, ``exp_avg``, ``exp_avg_sq``) and ``param_groups``, so its ``state_dict()`` loads into
``torch.optim.Adam`` and the other way round; ``step()`` is one launch per parameter group.

Differences from the stock sequence, all stated in ``include/pworld.h``: with ``max_norm`` the gradients are scaled in registers
only (``clip_grad_norm_`` writes ``.grad``; here ``.grad`` is left as autograd produced it), and the norm is taken over the
parameters of one group (one launch) -- a learner that clips a whole network keeps that network in one group.  There is no
fallback: parameters that are not contiguous float32 tensors on the GPU raise.
"""
import ctypes as C

import torch

from . import _lib


_REFUSED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay')


def _refuse(group):
    """The switches of torch Adam's ``param_groups`` that the kernel does not implement (``decoupled_weight_decay`` is AdamW's
    form of the decay; ``pw_adam_step`` has the L2 form only)."""
    on = [k for k in _REFUSED if group.get(k)]
    if on:
        raise ValueError('FusedAdam serves none of %s (got %s)' % (', '.join(_REFUSED), ', '.join(on)))


FAMILY = 'the fused optimiser runs on the GPU (no CPU fallback)'


def _check_tensor(t, what, device=None):
    if t.is_sparse:
        raise RuntimeError('%s is sparse: not served' % what)
    _lib.check_f32(t, what, FAMILY, device, 'the group')


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` (no ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``, ``decoupled_weight_decay``) whose ``step()`` is one
    ``pw_adam_step`` launch per parameter group.

    ``max_norm``: clip the group's gradients to this global norm inside the launch (``clip_grad_norm_(params, max_norm)``
    followed by ``step()``, without writing ``.grad``).  ``targets``: the target network's parameters, in the order of
    ``params`` (an iterable of tensors, or a list of such per group); with ``tau`` the Polyak update
    ``t = t * (1 - tau) + p * tau`` rides in the same launch, on the new ``p``.  Parameters whose ``.grad`` is ``None`` take no
    part in the norm or the Adam step and get no state, as in torch; their targets still move, as the stock ``soft_update``
    moves every target: one ``pw_soft_update`` launch for them, before the group's own.  ``last_total_norm``: the gradient norm of the most
    recent launch as a device scalar (never read back here).

    ``graph_steps=True`` (what a captured update needs, ``multiagent_rl_amd.graph``): the step count of every group also lives in an
    int64 device cell; ``step()`` launches ``pw_adam_step_dev``, which forms the bias corrections from that cell in the kernel, and then
    advances the cell with ``pw_counter_add`` -- so a replayed ``step()`` takes step t + 1, not step t again.  The host-side
    ``state[p]['step']`` advances in ``step()`` as always (also while a graph is being captured, when nothing runs on the device);
    ``note_graph_steps(n)`` advances it for ``n`` replays.  ``state_dict()`` is unchanged: it still loads into ``torch.optim.Adam``.  The
    other hyper-parameters travel as kernel arguments: a captured ``step()`` keeps the ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` it
    was captured with."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, targets=None, tau=None,
                 amsgrad=False, maximize=False, graph_steps=False):
        if amsgrad or maximize:
            raise ValueError('FusedAdam serves neither amsgrad nor maximize')
        # the defaults of the installed torch's Adam, key for key: a state_dict of either loads into the other
        probe = torch.optim.Adam([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, dict(probe.defaults))
        if (targets is None) != (tau is None):
            raise ValueError('targets and tau come together')
        if tau is not None and not 0.0 <= float(tau) <= 1.0:
            raise ValueError('tau must be in [0, 1]')
        if max_norm is not None and not float(max_norm) > 0.0:
            raise ValueError('max_norm must be positive (None: no clipping)')
        self.max_norm = None if max_norm is None else float(max_norm)
        self.tau = None if tau is None else float(tau)
        self._targets = None
        if targets is not None:
            targets = list(targets)
            if targets and isinstance(targets[0], torch.Tensor):
                targets = [targets]
            targets = [list(t) for t in targets]
            if [len(t) for t in targets] != [len(g['params']) for g in self.param_groups]:
                raise ValueError('targets must match params, tensor for tensor')
            for tg, g in zip(targets, self.param_groups):
                for t, p in zip(tg, g['params']):
                    if t.shape != p.shape:
                        raise ValueError('target %r against parameter %r' % (tuple(t.shape), tuple(p.shape)))
            self._targets = targets
        self._norms = {}
        self.last_total_norm = None
        self._lib = None
        self.graph_steps = bool(graph_steps)
        self._step_cells = {}    # group index -> int64 device cell: the step the group's NEXT launch takes

    def sync_step_cells(self):
        """Rewrite the device step cells from the host-side ``step`` (after ``load_state_dict``, or after ``step`` was set by hand)."""
        for gi, group in enumerate(self.param_groups):
            cell = self._step_cells.get(gi)
            steps = [float(self.state[p]['step']) for p in group['params'] if len(self.state.get(p, {}))]
            if cell is not None and steps:
                cell.fill_(int(steps[0]) + 1)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self.sync_step_cells()

    def note_graph_steps(self, n=1):
        """Host bookkeeping for ``n`` ``step()`` calls that ran inside a replayed graph (the device cells have advanced there)."""
        for group in self.param_groups:
            for p in group['params']:
                st = self.state.get(p)
                if st is not None and len(st):
                    st['step'] = st['step'] + n

    def __setstate__(self, state):
        super().__setstate__(state)
        for g in self.param_groups:
            _refuse(g)

    @classmethod
    def from_adam(cls, adam, **kw):
        """A ``FusedAdam`` over the parameters of ``adam`` (a ``torch.optim.Adam``) with its hyper-parameters and state."""
        groups = [dict(g) for g in adam.param_groups]
        for g in groups:
            _refuse(g)
        g0 = groups[0]
        opt = cls(groups, lr=g0['lr'], betas=g0['betas'], eps=g0['eps'], weight_decay=g0['weight_decay'],
                  amsgrad=any(g.get('amsgrad') for g in groups), maximize=any(g.get('maximize') for g in groups), **kw)
        opt.load_state_dict(adam.state_dict())
        return opt

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self._lib is None:
            self._lib = _lib.load()
        for gi, group in enumerate(self.param_groups):
            _refuse(group)
            targets = self._targets[gi] if self._targets is not None else None
            rows, steps, device, total, idle = [], [], None, 0, []
            for pi, p in enumerate(group['params']):
                if p.grad is None or p.numel() == 0:
                    if targets is not None and p.numel():
                        idle.append((targets[pi], p.detach()))
                    continue
                if device is None:
                    device = p.device
                _check_tensor(p, 'parameter', device)
                _check_tensor(p.grad, 'gradient', device)
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                _check_tensor(st['exp_avg'], 'exp_avg', device)
                _check_tensor(st['exp_avg_sq'], 'exp_avg_sq', device)
                t = None
                if targets is not None:
                    t = targets[pi]
                    _check_tensor(t, 'target', device)
                steps.append(st)
                total += p.numel()
                rows.append((p.data_ptr(), p.grad.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr(),
                             None if t is None else t.data_ptr(), p.numel()))
            if idle:   # the stock sequence moves every target, whether or not its parameter had a gradient
                soft_update([t for t, _ in idle], [q for _, q in idle], self.tau)
            if not rows:
                continue
            if len(rows) > _lib.PW_OPT_MAX_TENSORS or total > _lib.PW_OPT_MAX_ELEMENTS:
                raise RuntimeError('a parameter group of %d tensors / %d elements: one launch serves at most %d tensors and 2^20 '
                                   'elements (split the group)' % (len(rows), total, _lib.PW_OPT_MAX_TENSORS))
            counts = set(float(st['step']) for st in steps)
            if len(counts) != 1:
                raise RuntimeError('the parameters of one group disagree on `step` (%s): one launch takes one step' % sorted(counts))
            step = int(counts.pop()) + 1
            table = (_lib.PwOptTensor * len(rows))(*rows)
            norm = self._norms.get(gi)
            if norm is None or norm.device != device:
                norm = self._norms[gi] = torch.zeros((), dtype=torch.float32, device=device)
            beta1, beta2 = group['betas']
            hyper = (float(group['lr']), float(beta1), float(beta2), float(group['eps']), float(group['weight_decay']),
                     self.max_norm if self.max_norm is not None else 0.0, self.tau if self.tau is not None else 0.0,
                     _lib.ptr(norm), _lib.stream(device))
            if self.graph_steps:
                cell = self._step_cells.get(gi)
                if cell is None or cell.device != device:
                    if torch.cuda.is_current_stream_capturing():   # a captured fill would reset the cell at every replay
                        raise RuntimeError('FusedAdam(graph_steps=True): take one step() eagerly before capturing (it creates the '
                                           'Adam state and the device step cell; created inside a capture they would be reset by every replay)')
                    cell = self._step_cells[gi] = torch.full((1,), step, dtype=torch.int64, device=device)
                _lib.check(self._lib.pw_adam_step_dev(table, len(rows), _lib.ptr(cell), *hyper))
                _lib.check(self._lib.pw_counter_add(_lib.ptr(cell), 1, 0, _lib.stream(device)))
            else:
                _lib.check(self._lib.pw_adam_step(table, len(rows), step, *hyper))
            for st in steps:
                if isinstance(st['step'], torch.Tensor):
                    st['step'] += 1
                else:
                    st['step'] = st['step'] + 1
            self.last_total_norm = norm
        return loss


def _parameters(net):
    return list(net.parameters()) if hasattr(net, 'parameters') else list(net)


@torch.no_grad()
def soft_update(target, source, tau):
    """``target = target * (1 - tau) + source * tau`` over the parameters of two modules (``ddpg_gumbel_fix.py:36-47``, bit for
    bit) as one ``pw_soft_update`` launch (one per 32 tensors / 2^20 elements).  ``target`` / ``source``: ``nn.Module``s, the
    target wrappers of ``accelerate_trainer(targets=True)``, or iterables of tensors.  ``tau == 1`` is ``hard_update``."""
    lib = _lib.load()
    tps, sps = _parameters(target), _parameters(source)
    if len(tps) != len(sps):
        raise ValueError('target has %d parameters, source %d' % (len(tps), len(sps)))
    if not tps:
        return
    device = tps[0].device
    for t, s in zip(tps, sps):
        _check_tensor(t, 'target', device)
        _check_tensor(s, 'source', device)
        if t.shape != s.shape:
            raise ValueError('target %r against source %r' % (tuple(t.shape), tuple(s.shape)))
    batch, total = [], 0
    pairs = list(zip(tps, sps))

    def launch(batch):
        n = len(batch)
        tp = (C.c_void_p * n)(*[t.data_ptr() for t, _ in batch])
        sp = (C.c_void_p * n)(*[s.data_ptr() for _, s in batch])
        ne = (C.c_int64 * n)(*[t.numel() for t, _ in batch])
        _lib.check(lib.pw_soft_update(tp, sp, ne, n, float(tau), _lib.stream(device)))
    for t, s in pairs:
        if t.numel() == 0:
            continue
        if t.numel() > _lib.PW_OPT_MAX_ELEMENTS:
            raise RuntimeError('a tensor of %d elements: one launch serves at most 2^20' % t.numel())
        if len(batch) == _lib.PW_OPT_MAX_TENSORS or total + t.numel() > _lib.PW_OPT_MAX_ELEMENTS:
            launch(batch)
            batch, total = [], 0
        batch.append((t, s))
        total += t.numel()
    if batch:
        launch(batch)


def fuse_optimizers(trainer, graph_steps=False):
    """``trainer.actor_optimizer`` / ``trainer.critic_optimizer`` -> ``FusedAdam`` with the hyper-parameters and state of the
    optimisers they replace; ``trainer.soft_update`` -> the one-launch ``soft_update``.  The Trainer's own ``clip_grad_norm_``
    calls stay torch's (the Trainer is not modified), so the kernels' clip is off here (``max_norm=None``).  ``graph_steps``:
    ``FusedAdam``'s switch of that name.  Returns the two optimisers."""
    out = []
    for name in ('actor_optimizer', 'critic_optimizer'):
        old = getattr(trainer, name)
        if isinstance(old, FusedAdam):   # the Trainer took the switch itself (the example learner's fused_optimizer)
            old.graph_steps = old.graph_steps or bool(graph_steps)
            out.append(old)
            continue
        if not isinstance(old, torch.optim.Adam):
            raise ValueError('%s is %s: accelerate_trainer(optimizer=True) replaces torch.optim.Adam' % (name, type(old).__name__))
        new = FusedAdam.from_adam(old, graph_steps=graph_steps)
        setattr(trainer, name, new)
        out.append(new)
    trainer.soft_update = soft_update
    return tuple(out)
