"""The learner's update as ONE captured graph: ``GraphedUpdate(trainer)`` stands in for ``trainer.optimize``.

With all four switches of ``accelerate_trainer`` on, what is left of an update's cost is the host issuing its launches.
``torch.cuda.graph`` records them once -- the stock ops and this package's ctypes launches alike, on one stream -- and every later update is
one graph launch.  A replay repeats the recorded launches with the recorded arguments, so everything that changes from update to update
must live in device memory:

* the batch: ``ReplayBuffer(device_index='counter')`` -- ``pw_replay_sample`` numbers the draw and bounds it by the ring's length from two
  device cells (a replayed ``torch.randint(0, len)`` would keep the length of the capture);
* Adam's bias corrections: ``FusedAdam(graph_steps=True)`` -- ``pw_adam_step_dev`` forms them in the kernel from a device step cell (the host
  form would repeat one step number forever);
* the target actor's packed weights: ``FusedActor.refresh(in_place=True)`` inside the captured region (the default ``refresh`` allocates new
  tensors, which a captured forward never reads);
* optionally the sampling noise: ``sampling.GumbelSampler`` -- ``pw_gumbel_st_forward`` adds a device cell to its step, and the cell advances
  inside the captured region (without it the stock ``F.gumbel_softmax`` is captured: torch's generator serves a replay new noise too, but
  not the noise an eager run would draw).

Served: the configuration in which no vendor RNN call and no stock optimiser is captured -- ``targets``, ``optimizer``, ``lstm`` and
``attention`` on (a critic without an attention block, ``BiCNetCritic``, needs the first three), the optimisers in ``graph_steps`` mode, the
memory in ``'counter'`` mode with at least ``batch_size`` transitions.  Anything else is a ``ValueError`` that names what is missing.  The
hyper-parameters ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` travel as kernel arguments: when a group's differ from the captured ones the
update is captured again (``recapture()`` does it on request, e.g. after the batch size changed).

What is captured must not read back, allocate through libpworld or branch on a device value; the example learner's ``optimize_tensors()``
(the body of ``optimize()`` returning the loss tensors) is such a region.  A Trainer without ``optimize_tensors`` has its ``optimize``
captured as it is, and a read-back in it (``float(loss)``) fails the capture loudly.
"""
import torch
import torch.nn as nn

from .optim import FusedAdam

_HYPER = ('lr', 'betas', 'eps', 'weight_decay')


def _plain_lstms(module):
    from .lstm import FusedLSTM
    return [m for m in module.modules() if isinstance(m, nn.LSTM) and not isinstance(m, FusedLSTM)] if isinstance(module, nn.Module) else []


def missing_for_graph(trainer):
    """-> what keeps ``trainer`` from the served configuration, as a list of sentences (empty: it can be captured).  Host-side checks
    only: this runs where there is no GPU."""
    from .attention import _Fused, critic_form
    from .critic import _FusedTarget
    miss = []
    fx = getattr(trainer, '_pw_accel', None)
    fused_targets = isinstance(getattr(trainer, 'target_actor', None), _FusedTarget) and \
        isinstance(getattr(trainer, 'target_critic', None), _FusedTarget) and getattr(fx, 'target_actor', None) is not None
    if not fused_targets:
        miss.append('targets: the target actor and target critic must run on the HIP kernels (accelerate_trainer(..., targets=True))')
    for name in ('actor_optimizer', 'critic_optimizer'):
        opt = getattr(trainer, name, None)
        if not isinstance(opt, FusedAdam):
            miss.append('optimizer: %s is %s, not FusedAdam (accelerate_trainer(..., optimizer=True) / fused_optimizer=True); a stock '
                        'optimiser is not captured' % (name, type(opt).__name__))
        elif not opt.graph_steps:
            miss.append('optimizer: %s is not in graph_steps mode (FusedAdam(..., graph_steps=True)): a replay would repeat one Adam step '
                        'number' % name)
    nets = ['actor', 'critic'] + ([] if fused_targets else ['target_actor', 'target_critic'])
    plain = [name for name in nets if _plain_lstms(getattr(trainer, name, None))]
    if plain:
        miss.append('lstm: %s still run(s) nn.LSTM (accelerate_trainer(..., lstm=True) / fused_lstm=True); a vendor RNN call is not captured'
                    % ', '.join(plain))
    critic = getattr(trainer, 'critic', None)
    if critic_form(critic)[0] in ('attention', 'model') and not isinstance(critic, _Fused):
        miss.append("attention: the critic's attention block is the stock expression (accelerate_trainer(..., attention=True) / "
                    'fused_attention=True)')
    memory = getattr(trainer, 'memory', None)
    if getattr(memory, 'device_index', None) != 'counter':
        miss.append("memory: the replay ring must draw on the device from device cells (ReplayBuffer(..., device_index='counter')); it is %s"
                    % (type(memory).__name__ if not hasattr(memory, 'device_index') else 'in device_index=%r mode' % (memory.device_index,)))
    return miss


class GraphedUpdate(object):
    """A callable that stands in for ``trainer.optimize``.  Calls 1 .. ``warmup`` run eagerly (real updates; they also create the Adam
    state and every lazily allocated buffer); call ``warmup + 1`` captures one update under ``torch.cuda.graph`` and replays it once --
    capture executes nothing on the device but its Python side advances the host counters, so capture plus first replay count as ONE
    update; every later call is one ``replay()`` plus the host bookkeeping (``note_graph_steps(1)`` per optimiser, ``trainer.iter += 1``).
    Returns the two loss tensors (device, overwritten by the next replay); ``losses()`` synchronises and returns floats.  After each
    update the exploration actor's snapshot is refreshed eagerly, as ``accelerate_trainer`` does behind ``optimize``."""

    def __init__(self, trainer, warmup=3):
        miss = missing_for_graph(trainer)
        if miss:
            raise ValueError('GraphedUpdate: this trainer is not in the configuration a captured update serves -- ' + '; '.join(miss))
        if int(warmup) < 1:
            raise ValueError('GraphedUpdate: warmup must be >= 1 (the eager updates create the Adam state and the device step cells; created '
                             'inside the capture they would be reset by every replay)')
        self.trainer, self.warmup = trainer, int(warmup)
        fx = trainer._pw_accel
        self._fx, self._target_actor = fx, fx.target_actor
        self._sampler = getattr(fx, 'owned_sampler', None)
        self._body = getattr(trainer, 'optimize_tensors', None) or fx.inner_optimize
        self.graph, self._out, self._hyper = None, None, None
        self.eager_calls = self.replays = self.captures = 0

    def _optimizers(self):
        return [self.trainer.actor_optimizer, self.trainer.critic_optimizer]

    def _hyper_now(self):
        return [tuple(g[k] if k != 'betas' else tuple(g[k]) for k in _HYPER) for opt in self._optimizers() for g in opt.param_groups]

    def _update(self):
        """One update: the learner's body, then the target actor's packed weights follow the soft update -- in place, in the same region."""
        out = self._body()
        if self._sampler is not None:          # accelerate_trainer(sampling=True): the noise cell advances inside the region, replay by replay
            self._sampler.end_update()
        self._target_actor.refresh(in_place=True)
        return out

    def _check_ring(self):
        need = int(getattr(self.trainer, 'batch_size', 1))
        if len(self.trainer.memory) < need:
            raise ValueError('GraphedUpdate: the ring holds %d transitions, an update draws %d' % (len(self.trainer.memory), need))
        miss = missing_for_graph(self.trainer)
        if miss:
            raise ValueError('GraphedUpdate: the trainer left the served configuration -- ' + '; '.join(miss))

    def recapture(self):
        """Forget the captured graph: the next call captures again (without new warm-up calls)."""
        self.graph, self._out = None, None

    def _capture(self):
        dev = self._target_actor.device
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):     # one side stream; libpworld's launches go to torch's current stream, i.e. into the capture
            out = self._update()
        self._out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        self._hyper = self._hyper_now()
        self._snapshot = self._target_actor.frag.data_ptr()
        self.captures += 1

    def __call__(self):
        self._check_ring()
        # by-value arguments of the captured launches that may have changed: the optimisers' hyper-parameters, and the target actor's
        # packed image if somebody took a default (allocating) refresh() since
        if self.graph is not None and (self._hyper_now() != self._hyper or self._target_actor.frag.data_ptr() != self._snapshot):
            self.recapture()
        if self.graph is None and self.eager_calls < self.warmup:
            self.eager_calls += 1
            out = self._update()
            self._fx.refresh()
            return out
        if self.graph is None:
            self._capture()               # the Python side has advanced step / iter once: the first replay is that update
        else:
            for opt in self._optimizers():
                opt.note_graph_steps(1)
            if hasattr(self.trainer, 'iter'):
                self.trainer.iter += 1
        self.graph.replay()
        self.replays += 1
        self._fx.refresh()
        return self._out

    def losses(self):
        """The most recent replay's losses as floats (synchronises)."""
        if self._out is None:
            raise RuntimeError('GraphedUpdate.losses(): nothing has been replayed yet')
        return tuple(float(t) for t in self._out)
