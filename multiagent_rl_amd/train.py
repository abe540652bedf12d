"""The batched counterpart of the reference's entry path: ``main.py:29-67`` (seed protocol, dims read from the env, the
nets, the call of ``run``) and ``experiments/run.py:11-103`` (rollout -> ``memory.add`` -> learner gate -> report -> history
pickle + ``save_models``), for B environments advanced together on the GPU.

What changes against the B = 1 loop of ``rollout.run`` is only WHERE the work happens:

* rollout: ``BatchedRollout.collect_one_launch`` -- ``chunk`` batched steps of actor + Gumbel sampling + env step + replay
  append + episode statistics as ONE launch (``pw_policy_rollout``), no host synchronisation inside a chunk;
* learner gate (run.py:78-81): ``optimize()`` runs once per ``update_rate`` ENV-steps once more than ``warmup_steps`` have been
  taken -- counted in env-steps exactly as the reference counts ``train_step`` (one per ``env.step`` of one world); a chunk
  advances ``chunk * B`` of them, so the gate opens ``LearnGate.due_between(before, after)`` times after it (bounded by
  ``max_updates_per_chunk``: at B = 4096 a 100-step chunk would otherwise owe 4096 updates; ``stats`` reports ``updates_owed``
  beside ``updates_run`` and the log says so when they differ);
* after the learner ran, the rollout's weight snapshot follows it (``FusedActor.refresh``) and, with several ranks, the
  learner rank's actor goes to every rollout rank as one flat broadcast (``dist.broadcast_actor``);
* multi-GPU: every rank rolls out its shard of the env batch; the transitions of all ranks reach the learner rank's ring
  through ``dist.FullTransitionGather`` (state-only wire blocks for simple_spread).

The Trainer is duck-typed exactly as in ``experiments/run.py:21``: ``Trainer(actor, critic, memory, action_type=...)`` with
``.actor``, ``.optimize()``, ``.save_models(name)`` -- the reference's own ``rls.agent.multiagent.ddpg_gumbel_fix.Trainer`` plugs
in unchanged (its ``process_batch`` reads the device ring through ``make_index`` / ``sample_index``).
"""
import time

import numpy as np
import torch

from . import arglist as _default_arglist
from .rollout import BatchedRollout, LearnGate, write_history


def seed_everything(seed):
    """main.py:41-49: ``np.random.seed``, ``torch.manual_seed``, ``torch.cuda.manual_seed_all`` (the env's own seed is the
    ``seed`` argument of ``make_batched_env``: the batched env draws its resets from Philox keyed by it, not from NumPy)."""
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    return seed


def dims_from_env(env):
    """main.py:51-58: observation length, per-agent action size(s), and 'Discrete' | 'MultiDiscrete'."""
    dim_obs = env.observation_space[0].shape[0]
    space = env.action_space[0]
    if hasattr(space, 'high'):
        return dim_obs, (space.high + 1).tolist(), 'MultiDiscrete'
    return dim_obs, space.n, 'Discrete'


class ChunkLedger(object):
    """Per-episode returns out of a chunk's [T, B] outputs, vectorised: ``reward_episodes`` / ``reward_episodes_by_agents``
    get one entry per FINISHED episode, in the order the B = 1 loop of ``experiments/run.py:55-65`` would have appended them had it
    stepped the B worlds side by side: by END STEP, then by env (``terminal.nonzero()`` order) -- the lists
    ``experiments/reward_plot.py:35-50`` reads.  ``history()`` closes them the way run.py:62-65 leaves its lists: behind the finished
    episodes stands the entry of the episode in progress -- here one per env, in env order (B = 1: the reference's single trailing
    entry); ``open_episodes`` says how many, so a reader that wants finished episodes only drops that many from the end."""

    def __init__(self, num_envs, num_agents, device):
        self.carry = torch.zeros(num_envs, num_agents, dtype=torch.float64, device=device)
        self.totals, self.by_agent = [], [[] for _ in range(num_agents)]

    @torch.no_grad()
    def absorb(self, rew, terminal):
        """rew [T,B,N] float32, terminal [T,B] bool."""
        T, B, N = rew.shape
        term = terminal.bool()
        ends_before = torch.cumsum(term.long(), 0) - term.long()            # episode index of each step inside the chunk
        n_seg = int(ends_before.max().item()) + 1
        sums = torch.zeros(n_seg, B, N, dtype=torch.float64, device=rew.device)
        sums.scatter_add_(0, ends_before[:, :, None].expand(T, B, N), rew.double())
        sums[0] += self.carry
        t_end, e_end = torch.nonzero(term, as_tuple=True)                   # row-major: by end step, then by env
        if t_end.numel():
            per_agent = sums[ends_before[t_end, e_end], e_end].cpu().numpy()  # [finished episodes, N]
            self.totals.extend(per_agent.sum(1).tolist())
            for i in range(N):
                self.by_agent[i].extend(per_agent[:, i].tolist())
        ends = torch.cumsum(term.long(), 0)[-1]                             # finished episodes per env
        last = torch.clamp(ends, max=n_seg - 1)
        open_ = sums[last, torch.arange(B, device=rew.device)]
        self.carry = torch.where((ends < n_seg)[:, None], open_, torch.zeros_like(open_))

    def mean_of_last(self, n):
        """run.py:86: ``np.mean(episode_rewards[-save_rate:])`` over finished episodes."""
        tail = self.totals[-int(n):]
        return float(np.mean(tail)) if tail else float('nan')

    def history(self, include_open=True):
        totals, by_agent, n_open = list(self.totals), [list(x) for x in self.by_agent], 0
        if include_open:
            open_ = self.carry.cpu().numpy()
            n_open = open_.shape[0]
            totals.extend(open_.sum(1).tolist())
            for i in range(open_.shape[1]):
                by_agent[i].extend(open_[:, i].tolist())
        return {'reward_episodes': totals, 'reward_episodes_by_agents': by_agent, 'open_episodes': n_open}


class EpisodeLog(object):
    """The same two lists from a HIP launch (``pw_episode_log_absorb``): one entry per finished episode -- total and per-agent return
    in float64, the batched step at which it ended, its env -- in a log of ``capacity`` entries in device memory, in ``ChunkLedger``'s
    order (end step, then env).  Every sum is one thread's chain in the order of ``experiments/run.py:55-57`` (the total is a sum of
    its own over the agents, not the sum of the shares), so the entries are a function of the planes alone, bit for bit, however the
    steps are cut into chunks.  The log's length, its step count and the returns of the episodes in progress are device cells:
    ``absorb`` reads nothing back.  A drop-in where a ``ChunkLedger`` is used (``absorb`` / ``mean_of_last`` / ``history``)."""

    def __init__(self, num_envs, num_agents, capacity, device):
        from . import _lib
        self.B, self.N, self.capacity = int(num_envs), int(num_agents), int(capacity)
        if self.B < 1 or self.capacity < 1 or not 1 <= self.N <= _lib.PW_EPISODE_LOG_MAX_AGENTS:
            raise ValueError('EpisodeLog: num_envs >= 1, capacity >= 1 and 1 <= num_agents <= %d (got %d, %d, %d)'
                             % (_lib.PW_EPISODE_LOG_MAX_AGENTS, self.B, self.capacity, self.N))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise _lib.PworldError('EpisodeLog lives on the GPU (got %s): there is no CPU fallback; ChunkLedger is the host form' % self.device)
        self._lib, self.lib = _lib, _lib.load()
        dev = self.device
        self.total = torch.zeros(self.capacity, dtype=torch.float64, device=dev)
        self.by_agent = torch.zeros(self.capacity, self.N, dtype=torch.float64, device=dev)
        self.end_step = torch.zeros(self.capacity, dtype=torch.int64, device=dev)
        self.env = torch.zeros(self.capacity, dtype=torch.int32, device=dev)
        self.carry = torch.zeros(self.B, self.N + 1, dtype=torch.float64, device=dev)
        self.cells = torch.zeros(2, dtype=torch.int64, device=dev)      # length, step_base
        self._scratch, self._scratch_T = None, None
        self._c = _lib.PwEpisodeLog()
        c = self._c
        c.struct_size, c.num_envs, c.num_agents, c.capacity = _lib.C.sizeof(_lib.PwEpisodeLog), self.B, self.N, self.capacity
        c.total, c.by_agent, c.end_step, c.env = (t.data_ptr() for t in (self.total, self.by_agent, self.end_step, self.env))
        c.carry, c.length, c.step_base = self.carry.data_ptr(), self.cells.data_ptr(), self.cells.data_ptr() + 8

    def absorb(self, rew, terminal):
        """rew [T,B,N] float32, terminal [T,B] bool or uint8, both contiguous on the log's device: one call of the launch."""
        if rew.dim() != 3 or tuple(rew.shape[1:]) != (self.B, self.N) or rew.shape[0] < 1:
            raise ValueError('EpisodeLog.absorb: rew must be [T, %d, %d] (got %r)' % (self.B, self.N, tuple(rew.shape)))
        T = int(rew.shape[0])
        if tuple(terminal.shape) != (T, self.B):
            raise ValueError('EpisodeLog.absorb: terminal must be [%d, %d] (got %r)' % (T, self.B, tuple(terminal.shape)))
        if rew.dtype != torch.float32 or terminal.dtype not in (torch.bool, torch.uint8):
            raise ValueError('EpisodeLog.absorb: rew float32 and terminal bool / uint8 (got %s, %s)' % (rew.dtype, terminal.dtype))
        if rew.device != self.device or terminal.device != self.device:
            raise ValueError('EpisodeLog.absorb: the planes are on %s / %s, the log on %s' % (rew.device, terminal.device, self.device))
        if not rew.is_contiguous() or not terminal.is_contiguous():
            raise ValueError('EpisodeLog.absorb: rew and terminal must be contiguous')
        if self._scratch_T != T:
            nbytes = self.lib.pw_episode_log_scratch_bytes(T, self.B)
            if nbytes == 0:
                raise ValueError('EpisodeLog.absorb: T * num_envs = %d flags are more than one launch serves' % (T * self.B))
            if self._scratch is None or self._scratch.numel() < nbytes:
                self._scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                self._c.scratch = self._scratch.data_ptr()
            self._scratch_T = T
        p = self._lib.ptr
        self._lib.check(self.lib.pw_episode_log_absorb(self._lib.C.byref(self._c), p(rew), p(terminal), T, self._lib.stream(self.device)))

    def finished(self):
        """Episodes finished so far (one cell read; keeps counting past ``capacity``)."""
        return int(self.cells[0].item())

    __len__ = finished

    def entries(self):
        """One read-back of the filled part -> dict of numpy arrays: total [n], by_agent [n,N], end_step [n], env [n]."""
        n = self.finished()
        if n > self.capacity:
            raise RuntimeError('EpisodeLog overflowed: %d episodes finished, capacity %d (the entries past it were not stored)'
                               % (n, self.capacity))
        return dict(total=self.total[:n].cpu().numpy(), by_agent=self.by_agent[:n].cpu().numpy(),
                    end_step=self.end_step[:n].cpu().numpy(), env=self.env[:n].cpu().numpy())

    def mean_of_last(self, n, finished=None):
        """run.py:86: ``np.mean(episode_rewards[-save_rate:])`` over finished episodes (``finished``: the length, where the caller has
        just read it)."""
        have = self.finished() if finished is None else int(finished)
        if have > self.capacity:
            raise RuntimeError('EpisodeLog overflowed: %d episodes finished, capacity %d' % (have, self.capacity))
        tail = self.total[max(0, have - int(n)):have].cpu().numpy()
        return float(np.mean(tail)) if tail.size else float('nan')

    def history(self, include_open=True):
        """``include_open=True``: the dict ``ChunkLedger.history`` returns (finished episodes in log order, then the episode in
        progress of every env from ``carry``).  ``include_open=False``: finished episodes only, ``open_episodes = 0``, and beside them
        ``episode_end_step`` / ``episode_env``."""
        ent = self.entries()
        totals = ent['total'].tolist()
        by_agent = [ent['by_agent'][:, i].tolist() for i in range(self.N)]
        if not include_open:
            return {'reward_episodes': totals, 'reward_episodes_by_agents': by_agent, 'open_episodes': 0,
                    'episode_end_step': ent['end_step'].tolist(), 'episode_env': ent['env'].tolist()}
        open_ = self.carry.cpu().numpy()
        totals.extend(open_[:, self.N].tolist())
        for i in range(self.N):
            by_agent[i].extend(open_[:, i].tolist())
        return {'reward_episodes': totals, 'reward_episodes_by_agents': by_agent, 'open_episodes': self.B}


def merge_histories_chronological(parts):
    """Per-rank histories of an ``EpisodeLog`` -> one a learning-curve reader can use: the FINISHED episodes of all ranks sorted by
    (``episode_end_step``, rank, env) -- the order one loop stepping all ``world * B`` worlds side by side would have appended them in
    -- with ``episode_rank`` and ``episode_env`` (global env id = rank * B + env) beside them; behind them the open returns of all
    ranks in global env order, ``open_episodes`` their single count (0 where the parts carry none); ``episodes_per_rank`` as
    ``merge_histories`` keeps it.  Every part needs ``episode_end_step`` / ``episode_env`` and ``num_envs``; a part built with
    ``include_open=True`` carries its open entries behind its finished ones and the two lists cover those only."""
    n_agents = len(parts[0]['reward_episodes_by_agents'])
    B = int(parts[0]['num_envs'])
    keys, tails = [], []
    for r, p in enumerate(parts):
        if int(p['num_envs']) != B or len(p['reward_episodes_by_agents']) != n_agents:
            raise ValueError('merge_histories_chronological: rank %d has another shape than rank 0' % r)
        n = len(p['episode_end_step'])
        if len(p['episode_env']) != n or len(p['reward_episodes']) != n + p.get('open_episodes', 0):
            raise ValueError('merge_histories_chronological: rank %d: %d end steps, %d envs, %d entries of which %d open'
                             % (r, n, len(p['episode_env']), len(p['reward_episodes']), p.get('open_episodes', 0)))
        keys.extend((int(p['episode_end_step'][k]), r, int(p['episode_env'][k]), k) for k in range(n))
        tails.append(n)
    keys.sort()
    out = {'reward_episodes': [parts[r]['reward_episodes'][k] for _, r, _, k in keys],
           'reward_episodes_by_agents': [[parts[r]['reward_episodes_by_agents'][i][k] for _, r, _, k in keys] for i in range(n_agents)],
           'episode_end_step': [s for s, _, _, _ in keys], 'episode_rank': [r for _, r, _, _ in keys],
           'episode_env': [r * B + e for _, r, e, _ in keys],
           'open_episodes': sum(p.get('open_episodes', 0) for p in parts), 'episodes_per_rank': list(tails)}
    for p, n in zip(parts, tails):          # rank order = global env order
        out['reward_episodes'].extend(p['reward_episodes'][n:])
        for i in range(n_agents):
            out['reward_episodes_by_agents'][i].extend(p['reward_episodes_by_agents'][i][n:])
    return out


def merge_histories(parts):
    """Per-rank histories -> one, in RANK order (rank r owns global envs [r B, (r + 1) B)): what the learner rank pickles."""
    out = {'reward_episodes': [], 'reward_episodes_by_agents': [[] for _ in parts[0]['reward_episodes_by_agents']],
           'open_episodes': [p.get('open_episodes', 0) for p in parts], 'episodes_per_rank': [len(p['reward_episodes']) for p in parts]}
    for p in parts:
        out['reward_episodes'].extend(p['reward_episodes'])
        for i, lst in enumerate(p['reward_episodes_by_agents']):
            out['reward_episodes_by_agents'][i].extend(lst)
    return out


def train_batched(env, actor, critic, Trainer, scenario_name, action_type='Discrete', cnt=0, arglist=None, memory=None,
                  out_dir='Models', log=print, chunk=100, max_updates_per_chunk=None, policy_seed=None,
                  per_episode_history=True, gather=None, rank=0, world=1, make_rollout=None, ring='rows',
                  per_agent_transition=False, graph_update=False, ledger='host', make_ledger=None):
    """``experiments/run.py:run`` for a ``BatchedParticleEnv`` (auto_reset=True).  Runs until ``arglist.num_episodes`` episodes
    have finished (over all envs of this rank), then pickles the history with the reference's keys and saves the models.
    ``gather`` (a ``dist.FullTransitionGather``) switches to the multi-GPU form: every rank rolls out into the gather's wire
    block, the learner lives on rank 0.  ``make_rollout(env, actor, memory, seed) -> (fused_actor, batched_rollout)`` replaces
    the HIP pair (tests drive the control flow without a GPU).  ``ring='state'`` (single-rank form; simple_spread with the local
    observation, simple_tag): the rollout's ring sink fills a STATE ring -- {vel, pos} + the episode's landmarks per transition, a
    third of the bytes -- and ``sample_index`` rebuilds the rows the learner trains on (bit-identical batches).  Envs only the generic
    one-launch rollout serves (the full observation, L > N, landmark contact on simple_spread, ``policy_form=5``) take ``ring='rows'``:
    their rollout refuses a STATE ring.  ``per_agent_transition=True`` (the BiCNet baseline, ``experiments/run_BIC.py:46,50``): the ring
    holds per-agent ``rew`` / ``done`` planes ([cap, N]) and every chunk is one launch, as with a shared ring (the rollout's sink stores
    every agent's own reward).  The ring built here is the single-rank row ring -- with ``ring='state'`` it raises; a per-agent STATE ring
    (``ReplayBuffer(per_agent=True, state_ring=...)``) comes in through ``memory=`` or, on several ranks, with the gather: ``gather`` must
    then be a per-agent gather (``dist.FullTransitionGather(per_agent=True)``: per-agent wire blocks; its ``memory`` is the learner's ring,
    row or STATE as the gather was built), any other gather raises -- as a per-agent gather does without ``per_agent_transition=True``.  ``graph_update=True``: the ring this
    function creates draws its batches from device cells (``ReplayBuffer(device_index='counter')``) and the learner's ``optimize`` is
    replaced, after construction, by a ``graph.GraphedUpdate`` (a learner that has installed one itself keeps it): a few eager updates,
    then one graph launch per update; the learner must be in the configuration that serves (``accelerate_trainer``'s four switches), or
    the ``ValueError`` says what is missing.  ``ledger='device'``: the per-episode history comes from an ``EpisodeLog`` (one HIP launch per
    chunk, no read-back but the episode count's) in place of the ``ChunkLedger`` of ``ledger='host'``, in single-rank and gather mode alike, with
    ``num_episodes + B (chunk // max_episode_len + 2)`` entries; on several ranks the histories are then merged in time order
    (``merge_histories_chronological``) instead of rank order.  ``make_ledger(num_envs, num_agents, capacity, device)`` replaces the
    ``EpisodeLog`` (tests).  A gather's ring is switched to ``'counter'`` mode here, a ring passed in through ``memory=`` must be in it already; the side-stream
    appends of a gather stay ordered against the replays by ``wait_ingested`` / ``mark_reads_done``.  ``stats`` gains ``graph_replays``.
    Returns the history dict (with ``stats``: env-steps, updates, wall time)."""
    from .replay_buffer import ReplayBuffer
    cfg = _default_arglist if arglist is None else arglist
    if action_type not in ('Discrete', 'MultiDiscrete'):
        raise ValueError('action_type must be Discrete or MultiDiscrete, got %r' % (action_type,))
    gather_per_agent = gather is not None and bool(getattr(gather, 'per_agent', False))
    if per_agent_transition and gather is not None and not gather_per_agent:
        raise ValueError('per_agent_transition=True with gather=: the multi-rank gather carries the shared reward only (per-agent wire '
                         'blocks are not served)')
    if gather_per_agent and not per_agent_transition:
        raise ValueError('gather= is a per-agent gather (FullTransitionGather(per_agent=True): its ring holds rew / done [cap, N]) but '
                         'per_agent_transition is not set: the learner would read the BiCNet tuple as a shared-reward batch')
    if ledger not in ('host', 'device'):
        raise ValueError("ledger must be 'host' or 'device', got %r" % (ledger,))
    if per_agent_transition and ring == 'state':
        raise ValueError("per_agent_transition=True with ring='state': a STATE ring is a shared-reward ring (per-agent rewards are not served)")
    B, N = env.num_envs, env.n
    log('observation shape: ', env.observation_space)
    log('action shape: ', env.action_space)
    learns = rank == 0
    if memory is None and learns:
        if gather is not None:
            memory = gather.memory
            if graph_update and hasattr(memory, 'use_counter_index'):
                memory.use_counter_index()
        else:
            heads = tuple(int(h) for h in (env.action_space[0].high + 1)) if action_type == 'MultiDiscrete' else None
            kw = dict(act_heads=heads) if heads else {}
            if ring == 'state':
                if heads or getattr(env, 'scenario_name', None) not in ('simple_spread', 'simple_tag'):
                    raise ValueError("ring='state' serves simple_spread (local observation) and simple_tag")
                kw = dict(state_ring=dict(scenario=env.scenario_name, num_landmarks=env.num_landmarks,
                                          num_adversaries=env.cfg.num_adversaries if env.scenario_name == 'simple_tag' else 0))
            if per_agent_transition:
                kw['per_agent'] = True
            # the batch's indices drawn on the device (graph_update: by a launch that reads the draw number and the length from device cells)
            memory = ReplayBuffer(int(1e6), N, env.obs_dim, device_index='counter' if graph_update else True, **kw)
    learner = Trainer(actor, critic, memory, action_type=action_type)
    graphed = None
    if graph_update and learns:
        from .graph import GraphedUpdate
        graphed = learner.optimize if isinstance(getattr(learner, 'optimize', None), GraphedUpdate) else None
        if graphed is None:
            fx = getattr(learner, '_pw_accel', None)
            if fx is None:
                raise ValueError('train_batched(graph_update=True): the learner has not been through accelerate_trainer (targets=True, '
                                 'optimizer=True, lstm=True, attention=True): there is no fused target actor to keep in step')
            for opt in (learner.actor_optimizer, learner.critic_optimizer):
                if hasattr(opt, 'graph_steps'):
                    opt.graph_steps = True
            graphed = fx.graphed = GraphedUpdate(learner)
            learner.optimize = graphed
    seed = (cnt + 12345678 if policy_seed is None else policy_seed) + rank
    if make_rollout is None:
        from .policy import FusedActor
        fused = FusedActor(learner.actor, seed=seed)
        ro = BatchedRollout(env, fused, None if gather is not None else memory)
    else:
        fused, ro = make_rollout(env, learner.actor, None if gather is not None else memory, seed)
    gate = LearnGate(cfg)
    # one ledger per rank in EVERY mode: a gather's chunk leaves rew / terminal in its side buffers, a MultiDiscrete chunk has the
    # same [T, B, N] rewards as a Discrete one (run.py:96-100 pickles one entry per episode whatever the action type)
    device_ledger = ledger == 'device' and per_episode_history
    if device_ledger:
        capacity = int(cfg.num_episodes) + B * (int(chunk) // int(cfg.max_episode_len) + 2)
        led = (EpisodeLog if make_ledger is None else make_ledger)(B, N, capacity, ro.obs.device)
    else:
        led = ChunkLedger(B, N, ro.obs.device) if per_episode_history else None
    updates = updates_owed = reports = 0
    t_begin = clock = time.time()
    log('Starting iterations...')
    obs0 = ro.obs
    while int(ro.finished_episodes.item()) < cfg.num_episodes:      # one read-back per chunk
        before = ro.env_steps * world
        if gather is not None:
            out = gather.outputs()
            fused.rollout(env, chunk, out, stats=(ro.episode_return, ro.finished_return_sum, ro.finished_episodes))
            if led is not None:          # before the next launch reuses the side buffers (same stream: ordered)
                led.absorb(out['rew'], out['terminal'])
            gather(obs0)
            obs0 = out['obs'][chunk - 1]
            ro.env_steps += chunk * B
        else:
            ro.collect_one_launch(chunk, chunk=chunk, keep_outputs=led is not None)
            if led is not None:
                led.absorb(ro.last_chunk['rew'], ro.last_chunk['terminal'])
        due = gate.due_between(before, ro.env_steps * world)
        updates_owed += due                 # what run.py:78-81 would have run at one optimize() per update_rate env-steps
        if max_updates_per_chunk is not None:
            due = min(due, int(max_updates_per_chunk))
        if due and learns and len(memory) >= getattr(cfg, 'batch_size', 1):
            if gather is not None:
                gather.wait_ingested()          # the root appends on a side stream: order the learner's reads behind them
            for _ in range(due):
                learner.optimize()
            updates += due
            if gather is not None and hasattr(gather, 'mark_reads_done'):
                gather.mark_reads_done()        # ... and the next appends behind these reads (the ring wraps)
        if due:
            if world > 1:
                from .dist import broadcast_actor
                broadcast_actor(learner.actor, src=0, fused=fused)
            else:
                fused.refresh()
        st_eps = int(ro.finished_episodes.item())
        if st_eps // cfg.save_rate > reports:
            reports = st_eps // cfg.save_rate
            s = ro.stats()
            # run.py:86: the mean over the LAST save_rate episodes (the all-time mean only where no ledger is kept)
            mean = led.mean_of_last(cfg.save_rate) if led is not None else s['mean_episode_reward']
            log('steps: {}, episodes: {}, mean episode reward: {}, time: {}'.format(
                ro.env_steps, s['episodes'], mean, round(time.time() - clock, 3)))
            clock = time.time()
    if gather is not None:
        gather.finish()
    s = ro.stats()
    hist = led.history() if led is not None else {'reward_episodes': [], 'reward_episodes_by_agents': [[] for _ in range(N)],
                                                        'open_episodes': 0}
    if world > 1 and led is not None:    # every rank's episodes to the learner rank, concatenated in rank order
        import torch.distributed as tdist
        parts = [None] * world if learns else None
        if device_ledger:                   # ... or, with the log's end steps, in the order one loop over all worlds would have had
            fin = led.history(include_open=False)
            hist.update(episode_end_step=fin['episode_end_step'], episode_env=fin['episode_env'], num_envs=B)
        tdist.gather_object(hist, parts, dst=0)
        if learns:
            hist = merge_histories_chronological(parts) if device_ledger else merge_histories(parts)
    hist['stats'] = dict(env_steps=ro.env_steps, episodes=s['episodes'], mean_episode_reward=s['mean_episode_reward'],
                         updates=updates, updates_run=updates, updates_owed=updates_owed,
                         updates_skipped=updates_owed - updates if learns else None,
                         graph_replays=graphed.replays if graphed is not None else 0,
                         wall_s=time.time() - t_begin, num_envs=B, chunk=chunk, world=world)
    if learns and updates < updates_owed:
        log('learner: {} of {} owed updates run (max_updates_per_chunk={}, or the ring was still empty)'.format(
            updates, updates_owed, max_updates_per_chunk))
    log('...Finished total of {} episodes.'.format(s['episodes']))
    if learns:
        write_history(hist, out_dir, scenario_name, cnt)
        learner.save_models(scenario_name + '_fin_' + str(cnt))
    return hist


def evaluate_batched(env, actor, critic, Trainer, scenario_name, action_type='Discrete', cnt=0, arglist=None, memory=None,
                     out_dir='Models', log=print, chunk=None, policy_seed=None, model_prefix=None, make_rollout=None,
                     make_ledger=None, rank=0, world=1):
    """``experiments/run.py:run_test`` (run.py:106-200) for a ``BatchedParticleEnv`` (auto_reset=True): the test phase of the
    experiment on the batched engine.  Builds the learner as ``train_batched`` does, loads
    ``<prefix><scenario>_fin_<cnt>`` (``prefix = arglist.appx`` unless ``model_prefix`` is given, as ``rollout.run_test``), and plays
    chunks of ``chunk`` steps (default ``arglist.max_episode_len``) until at least ``arglist.num_episodes`` episodes have finished
    over this rank's envs.  Each chunk is ONE ``FusedActor.rollout`` launch with the statistics sink -- and the ring sink when
    ``memory`` is given: the reference stores the test transitions and pickles the memory, so ``hist['memory'] = memory`` only then --
    whose step outputs are ``rew`` and ``terminal`` alone, then one ``EpisodeLog.absorb``; per chunk the host reads the log's
    length (the loop's end) and the last ten totals (the progress line), nothing else.  ``optimize()`` is NEVER called: the reference's ``run_test`` keeps updating the networks it evaluates because it leaves
    ``is_training`` True; an evaluation here does not, so the models on disk are the models that are measured.  No ``save_models``.
    One progress line per chunk in run.py:182's format with the mean over the last 10 finished episodes.  The history is
    ``EpisodeLog.history(include_open=False)`` -- every finished episode, in (end step, env) order; a reader takes ``[:num_episodes]``
    as ``experiments/reward_test_phase_csv.py`` does -- plus ``stats``; rank 0 writes it as ``test_history_<scenario>_<cnt>.pkl``.  With
    ``world > 1`` every rank plays its own envs (the policy seed is ``cnt + 12345678 + rank``; ``rank`` is added to an explicit
    ``policy_seed`` too, as in ``train_batched``: two ranks never share a noise stream) and rank 0 gathers and merges the histories in time order
    (``merge_histories_chronological``); no transition gather is involved.  ``make_rollout(env, actor, memory, seed) -> (fused_actor,
    batched_rollout)`` and ``make_ledger(num_envs, num_agents, capacity, device)`` replace the HIP pieces (tests)."""
    cfg = _default_arglist if arglist is None else arglist
    if action_type not in ('Discrete', 'MultiDiscrete'):
        raise ValueError('action_type must be Discrete or MultiDiscrete, got %r' % (action_type,))
    B, N = env.num_envs, env.n
    log('observation shape: ', env.observation_space)
    log('action shape: ', env.action_space)
    learner = Trainer(actor, critic, memory, action_type=action_type)
    prefix = getattr(cfg, 'appx', '') if model_prefix is None else model_prefix
    learner.load_models(prefix + scenario_name + '_fin_' + str(cnt))
    seed = (cnt + 12345678 if policy_seed is None else policy_seed) + rank
    if make_rollout is None:
        from .policy import FusedActor
        fused = FusedActor(learner.actor, seed=seed)
        ro = BatchedRollout(env, fused, memory)
    else:
        fused, ro = make_rollout(env, learner.actor, memory, seed)
    T = int(cfg.max_episode_len if chunk is None else chunk)
    dev = ro.obs.device
    # a chunk finishes at most B (T // max_episode_len + 1) episodes, and the loop stops at the first chunk that reaches num_episodes
    capacity = int(cfg.num_episodes) + B * (T // int(cfg.max_episode_len) + 2)
    ledger = (EpisodeLog if make_ledger is None else make_ledger)(B, N, capacity, dev)
    out = {'rew': torch.empty(T, B, N, dtype=torch.float32, device=dev), 'terminal': torch.empty(T, B, dtype=torch.bool, device=dev),
           'act': None}
    stats = (ro.episode_return, ro.finished_return_sum, ro.finished_episodes)
    t_begin = clock = time.time()
    log('Starting iterations...')
    finished = 0
    while finished < cfg.num_episodes:
        fused.rollout(env, T, out, memory=memory, stats=stats)
        ledger.absorb(out['rew'], out['terminal'])
        ro.env_steps += T * B
        finished = len(ledger)                  # one read-back per chunk
        log('steps: {}, episodes: {}, mean episode reward: {}, time: {}'.format(
            ro.env_steps, finished, ledger.mean_of_last(10, finished), round(time.time() - clock, 3)))
        clock = time.time()
    hist = ledger.history(include_open=False)
    s = ro.stats()
    if world > 1:
        import torch.distributed as tdist
        parts = [None] * world if rank == 0 else None
        tdist.gather_object(dict(hist, num_envs=B), parts, dst=0)
        if rank == 0:
            hist = merge_histories_chronological(parts)
    hist['stats'] = dict(env_steps=ro.env_steps, episodes=s['episodes'], mean_episode_reward=s['mean_episode_reward'], updates=0,
                         wall_s=time.time() - t_begin, num_envs=B, chunk=T, world=world)
    if memory is not None:
        hist['memory'] = memory
    log('...Finished total of {} episodes.'.format(finished))
    if rank == 0:
        write_history(hist, out_dir, scenario_name, cnt, evaluate=True)
    return hist
