"""The action producer of the rollout: the reference's actor architecture and its
Gumbel-softmax exploration, batched over [B envs x N agents] and kept on the device.

``ActorNetwork`` has the layer structure AND parameter names of
``rls/model/ac_network_multi_gumbel.py:24-67`` (``dense1.module``, ``bilstm``,
``dense2.module``), so state_dicts saved by the reference's Trainer
(``ddpg_gumbel_fix.py:221-229``) load unchanged.  It stays stock PyTorch-ROCm
(rocBLAS / MIOpen on MFMA) as BASELINE.json's north_star prescribes; the
hand-written HIP work is the environment, not the policy GEMMs.

``GumbelPolicy`` is the batched form of ``Trainer.get_exploration_action`` /
``gumbel_softmax(hard=True)`` (``ddpg_gumbel_fix.py:86-116``): the hard one-hot of
``F.gumbel_softmax`` is ``argmax(logits + g)`` with ``g = -log(Exponential(1))``, drawn here with
the same RNG call, but the result stays an int32 index tensor [B,N] in HBM -- no
``.cpu().numpy()`` round trip per env-step.
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


class TimeDistributed(nn.Module):
    """Applies ``module`` over the last axis of [batch, agents, features]."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x):
        if x.dim() <= 2:
            return self.module(x)
        lead = x.shape[:2]
        return self.module(x.reshape(lead[0] * lead[1], x.shape[2])).reshape(lead[0], lead[1], -1)


class ActorNetwork(nn.Module):
    """Linear(D, 64) -> ReLU -> BiLSTM(64 -> 2x32) over the AGENT axis -> ReLU -> Linear(64, 5).
    ``out_dim`` may be a list of two sizes (MultiDiscrete scenarios, main.py:52-54): then there are two
    heads, ``dense2_1`` / ``dense2_2``, and ``forward`` returns the list of their logits."""

    def __init__(self, input_dim, out_dim):
        super().__init__()
        self.out_dim = out_dim
        self.dense1 = TimeDistributed(nn.Linear(input_dim, 64))
        self.bilstm = nn.LSTM(64, 32, num_layers=1, batch_first=True, bidirectional=True)
        if type(out_dim) is list:
            self.dense2_1 = TimeDistributed(nn.Linear(64, out_dim[0]))
            self.dense2_2 = TimeDistributed(nn.Linear(64, out_dim[1]))
        else:
            self.dense2 = TimeDistributed(nn.Linear(64, out_dim))

    def forward(self, obs):
        hid = F.relu(self.dense1(obs))
        hid, _ = self.bilstm(hid, None)
        hid = F.relu(hid)
        if type(self.out_dim) is list:
            return [self.dense2_1(hid), self.dense2_2(hid)]
        return self.dense2(hid)


class ModelActorNetwork(ActorNetwork):
    """The actor of the model-learning variant (``rls/model/ac_network_model_multi_gumbel.py:23-66``): ``ActorNetwork`` with a third
    head, ``dense3`` = TimeDistributed(Linear(64, input_dim)), that predicts the next observation from the same ReLU'd BiLSTM output.
    ``forward`` returns ``(policy, next_state)``; ``policy`` is what ``ActorNetwork.forward`` returns.  Parameter names as the
    reference's (``dense3.module`` behind the policy head(s)), so its Trainer's ``*_actor.pt`` files load unchanged.  ``FusedActor``
    serves it as it is: the rollout and the target half read the policy head(s) only."""

    def __init__(self, input_dim, out_dim):
        super().__init__(input_dim, out_dim)
        self.dense3 = TimeDistributed(nn.Linear(64, input_dim))

    def forward(self, obs):
        hid = F.relu(self.dense1(obs))
        hid, _ = self.bilstm(hid, None)
        hid = F.relu(hid)
        if type(self.out_dim) is list:
            policy = [self.dense2_1(hid), self.dense2_2(hid)]
        else:
            policy = self.dense2(hid)
        return policy, self.dense3(hid)


class GumbelPolicy(object):
    """obs [B,N,D] (device) -> action index [B,N] int32 (device)."""

    def __init__(self, actor, generator=None):
        self.actor = actor
        self.generator = generator

    @torch.no_grad()
    def logits(self, obs):
        return self.actor(obs)

    def _sample(self, logits):
        gumbels = -torch.empty_like(logits).exponential_(generator=self.generator).log()
        return (logits + gumbels).argmax(dim=-1).to(torch.int32)

    @torch.no_grad()
    def __call__(self, obs):
        logits = self.actor(obs)
        if isinstance(logits, (list, tuple)):  # MultiDiscrete: [B,N,2] = (movement index, communication symbol)
            return torch.stack([self._sample(x) for x in logits], dim=-1)
        return self._sample(logits)


class FusedActor(object):
    """The same ActorNetwork evaluated by libpworld instead of MIOpen's ~45-kernel RNN path.

    Weights are snapshotted from ``actor`` (call ``refresh()`` after the learner updates it).  Default: ONE launch
    (``pw_actor_fused``): dense1 + ReLU and the input projections of both LSTM directions on the matrix cores
    (exact float32 MFMA), the recurrence over the agent axis, the output head and the Gumbel-argmax sampling, with
    every intermediate in registers / LDS.  ``PW_ACTOR_NO_FUSE=1`` selects the same arithmetic as three launches
    (``pw_actor_front``, ``pw_bilstm_forward``, ``pw_actor_head`` -- identical results, also used when N > 96), and
    ``PW_ACTOR_NO_MFMA=1`` additionally replaces the front end by weight-stationary dense1 + a rocBLAS GEMM.

    Observation rows hold up to 104 numbers (simple_spread's local rows up to N = 50) in the one-launch form and in the
    three-launch chain alike; the ``PW_ACTOR_NO_MFMA=1`` front end (``pw_dense``) stops at 64 and raises
    ``NotImplementedError`` beyond.
    """

    def __init__(self, actor, seed=0):
        self.lib = _lib.load()
        self.actor, self.seed, self.calls = actor, int(seed), 0
        self.use_mfma_front = not os.environ.get('PW_ACTOR_NO_MFMA')
        self.use_fused = self.use_mfma_front and not os.environ.get('PW_ACTOR_NO_FUSE')
        self.refresh()
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=self.device)  # Philox step (hipGraph mode)
        self.graph_mode = False
        self.defer_step_advance = False  # graph mode: the caller advances _step_dev (pw_rollout_tail)

    @torch.no_grad()
    def refresh(self, in_place=False):
        """Re-snapshot the actor's weights.  Default: new tensors (``cat`` / ``contiguous`` / a new packed image).  ``in_place=True``:
        the same values written INTO the existing buffers (``copy_`` / ``torch.cat(out=...)`` / the pack launch onto the existing
        image), so every address a captured launch holds stays valid and a captured ``refresh(in_place=True)`` feeds the captured
        forward; shapes are fixed after construction, and a changed one raises."""
        a = self.actor
        lin1, lstm = a.dense1.module, a.bilstm
        two = type(a.out_dim) is list  # MultiDiscrete actor: two heads on the same BiLSTM output
        heads = [a.dense2_1.module, a.dense2_2.module] if two else [a.dense2.module]
        if in_place:
            return self._refresh_in_place(lin1, lstm, heads)
        self.heads = tuple(int(h.out_features) for h in heads)
        assert lstm.hidden_size == 32 and lstm.bidirectional and lstm.num_layers == 1 and sum(self.heads) <= 16
        dev = lin1.weight.device
        assert dev.type == 'cuda', 'FusedActor needs the actor on the GPU (no CPU fallback)'
        f = lambda t: t.detach().to(torch.float32).contiguous()  # noqa: E731
        self.w1, self.b1 = f(lin1.weight), f(lin1.bias)                                          # [64, D]
        self.wih = f(torch.cat([lstm.weight_ih_l0, lstm.weight_ih_l0_reverse], 0))             # [256, 64]
        self.wih_t = f(self.wih.t())                                                            # [64, 256]
        self.bih = f(torch.cat([lstm.bias_ih_l0 + lstm.bias_hh_l0,
                                lstm.bias_ih_l0_reverse + lstm.bias_hh_l0_reverse], 0))         # [256]
        self.whh_f, self.whh_r = f(lstm.weight_hh_l0), f(lstm.weight_hh_l0_reverse)             # [128, 32]
        self.w2 = f(torch.cat([h.weight for h in heads], 0))                                    # [sum(heads), 64]
        self.b2 = f(torch.cat([h.bias for h in heads], 0))
        self.device = dev
        D = self.w1.shape[1]
        self.frag = torch.empty(self.lib.pw_actor_front_pack_floats(D), dtype=torch.float32, device=dev)
        self._pack_front()

    def _refresh_in_place(self, lin1, lstm, heads):
        srcs = dict(w1=lin1.weight, b1=lin1.bias, whh_f=lstm.weight_hh_l0, whh_r=lstm.weight_hh_l0_reverse)
        cats = dict(wih=[lstm.weight_ih_l0, lstm.weight_ih_l0_reverse], w2=[h.weight for h in heads], b2=[h.bias for h in heads])
        want = dict((k, tuple(v.shape)) for k, v in srcs.items())
        want.update((k, (sum(t.shape[0] for t in v),) + tuple(v[0].shape[1:])) for k, v in cats.items())
        for k, shape in want.items():
            have = getattr(self, k)
            if tuple(have.shape) != shape or have.device != lin1.weight.device or tuple(int(h.out_features) for h in heads) != self.heads:
                raise ValueError('FusedActor.refresh(in_place=True): %s is %r on %s, the actor now has %r on %s -- shapes are fixed after '
                                 'construction (build a new FusedActor)' % (k, tuple(have.shape), have.device, shape, lin1.weight.device))
        for k, v in srcs.items():
            getattr(self, k).copy_(v.detach())
        for k, v in cats.items():
            torch.cat([t.detach() for t in v], 0, out=getattr(self, k))
        self.wih_t.copy_(self.wih.t())
        H4 = 4 * lstm.hidden_size   # bih = [b_ih + b_hh | the reverse direction's]: each half summed into its place
        torch.add(lstm.bias_ih_l0.detach(), lstm.bias_hh_l0.detach(), out=self.bih[:H4])
        torch.add(lstm.bias_ih_l0_reverse.detach(), lstm.bias_hh_l0_reverse.detach(), out=self.bih[H4:])
        self._pack_front()

    def _pack_front(self):
        p = _lib.ptr
        _lib.check(self.lib.pw_actor_front_pack(p(self.w1), p(self.wih), self.w1.shape[1], p(self.frag), self._stream()))

    def _stream(self):
        return _lib.stream(self.device)

    @torch.no_grad()
    def _fused(self, obs, want_h=False, want_logits=False, want_act=False):
        """One launch: obs [B,N,D] -> (H [B,N,64], logits [B,N,5], act [B,N] int32), each None unless wanted."""
        B, N, D = obs.shape
        x = obs.reshape(B * N, D).to(torch.float32).contiguous()
        h = torch.empty(B, N, 64, dtype=torch.float32, device=self.device) if want_h else None
        n0, n1 = self.heads[0], (self.heads[1] if len(self.heads) > 1 else 0)
        logits = torch.empty(B, N, n0 + n1, dtype=torch.float32, device=self.device) if want_logits else None
        act = torch.empty((B, N, 2) if n1 else (B, N), dtype=torch.int32, device=self.device) if want_act else None
        p = _lib.ptr
        step_dev = p(self._step_dev) if (self.graph_mode and want_act) else None
        _lib.check(self.lib.pw_actor_fused(p(x), p(self.frag), p(self.b1), p(self.bih), p(self.whh_f),
                                           p(self.whh_r), p(self.w2), p(self.b2), n0, n1, B, N, D, 1,
                                           self.seed, self.calls, step_dev, p(h), p(logits), p(act),
                                           self._stream()))
        if step_dev is not None and not self.defer_step_advance:  # captured: the counter advances on the device
            _lib.check(self.lib.pw_counter_add(p(self._step_dev), 1, 0, self._stream()))
        return h, logits, act

    @torch.no_grad()
    def hidden(self, obs):
        """obs [B,N,D] -> relu(BiLSTM(relu(dense1(obs)))) [B,N,64].  D <= 104 (``PW_ACTOR_NO_MFMA=1``: D <= 64)."""
        B, N, D = obs.shape
        if self.use_fused and N <= 96:
            return self._fused(obs, want_h=True)[0]
        if not self.use_mfma_front and D > 64:
            raise NotImplementedError('PW_ACTOR_NO_MFMA=1: the weight-stationary dense1 (pw_dense) serves rows of at most 64 '
                                      'numbers, got D = %d; unset the switch (PW_ACTOR_NO_FUSE=1 alone keeps the three-launch '
                                      'chain, which serves D <= 104)' % D)
        x = obs.reshape(B * N, D).to(torch.float32).contiguous()
        p = _lib.ptr
        h = torch.empty(B, N, 64, dtype=torch.float32, device=self.device)
        if self.use_mfma_front:
            # dense1 + ReLU + both input projections in ONE launch on the matrix cores (exact f32 MFMA);
            # the hidden activations never leave registers
            g = torch.empty(B * N, 256, dtype=torch.float32, device=self.device)     # [B,N,2,128]
            _lib.check(self.lib.pw_actor_front(p(x), p(self.frag), p(self.b1), p(self.bih), B * N, D, p(g),
                                               self._stream()))
        else:
            # the same in three launches: weight-stationary dense1 + ReLU, then a rocBLAS GEMM
            x1 = torch.empty(B * N, 64, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.pw_dense(p(x), p(self.w1), p(self.b1), B * N, D, 64, 1, p(x1), self._stream()))
            g = torch.addmm(self.bih, x1, self.wih_t)        # [B*N, 256] = [B,N,2,128]
        _lib.check(self.lib.pw_bilstm_forward(p(g), p(self.whh_f), p(self.whh_r), B, N, 1, p(h),
                                              self._stream()))
        return h

    @torch.no_grad()
    def _head(self, h, want_logits, want_act):
        B, N, _ = h.shape
        logits = torch.empty(B, N, 5, dtype=torch.float32, device=self.device) if want_logits else None
        act = torch.empty(B, N, dtype=torch.int32, device=self.device) if want_act else None
        p = _lib.ptr
        step_dev = p(self._step_dev) if (self.graph_mode and want_act) else None
        _lib.check(self.lib.pw_actor_head(p(h), p(self.w2), p(self.b2), B * N, self.seed, self.calls,
                                          step_dev, p(logits), p(act), self._stream()))
        if step_dev is not None and not self.defer_step_advance:  # captured: the counter advances on the device
            _lib.check(self.lib.pw_counter_add(p(self._step_dev), 1, 0, self._stream()))
        return logits, act

    def _one_launch(self, obs):
        if self.use_fused and obs.shape[1] <= 96:
            return True
        if self.heads != (5,):
            raise NotImplementedError('the three-launch chain serves the single 5-logit head only; two-head '
                                      '(MultiDiscrete) actors need the one-launch kernel (N <= 96)')
        return False

    def logits(self, obs):
        """[B,N,5]; two-head actors: the list [logits_move [B,N,n0], logits_comm [B,N,n1]] like ActorNetwork."""
        if self._one_launch(obs):
            lg = self._fused(obs, want_logits=True)[1]
            return lg if len(self.heads) == 1 else [lg[..., :self.heads[0]], lg[..., self.heads[0]:]]
        return self._head(self.hidden(obs), True, False)[0]

    def __call__(self, obs):
        """-> Gumbel-sampled action index [B,N] int32 (one fresh Philox stream per call)."""
        if self._one_launch(obs):
            act = self._fused(obs, want_act=True)[2]
        else:
            act = self._head(self.hidden(obs), False, True)[1]
        self.calls += 1
        return act

    @torch.no_grad()
    def rollout(self, env, num_steps, out=None, memory=None, stats=None):
        """``num_steps`` x (this actor + Gumbel sampling + ``env`` step with auto-reset) as ONE launch
        (``pw_policy_rollout``): observations, actions and world state stay on the CU between steps.  Continues
        from the env's current state.  -> dict of [T, ...] outputs as ``BatchedParticleEnv.rollout`` plus
        ``act`` [T,B,N] int32.  Same results as ``num_steps`` iterations of ``act = self(obs); env.step(act)``.

        ``memory`` (a device ``ReplayBuffer``): the transitions go straight into the ring from the same launch (a ``per_agent`` ring takes
        every agent's own reward, ``out['rew']``, into its [cap, N] planes; a shared ring ``out['rew_shared']``);
        ``stats`` = (episode_return [B], finished_sum, finished_count) tensors: the episode bookkeeping too.  With a
        sink, ``out=False`` skips the step outputs altogether (only the ring / statistics are written), and a caller's ``out`` may
        hold any subset of them (``'act': None`` leaves the sampled actions out; an absent ``'act'`` is allocated here).  What is left
        out changes nothing else.  Without a sink the library refuses a launch that lacks ``act``, ``obs``, ``rew``, ``rew_shared``,
        ``done`` or ``terminal`` (``PworldError``, nothing launched)."""
        T, B, N = int(num_steps), env.num_envs, env.n
        two = len(self.heads) == 2   # MultiDiscrete actor: simple_reference, act [T,B,N,2] = (movement, symbol); the sink is a two-head ring
        if two:
            assert env.scenario_name == 'simple_reference' and self.heads == (5, env.dim_c), \
                'two-head rollouts serve simple_reference (heads 5 | dim_c)'
            assert memory is None or tuple(memory.act_heads or ()) == self.heads, \
                'simple_reference: the ring sink is a ReplayBuffer built with act_heads=(5, dim_c)'
        else:
            assert self.heads == (5,), 'single 5-logit head only' 
        if out is False:
            assert memory is not None or stats is not None
            out = {}
        else:
            out = env.alloc_outputs(T, coll=False) if out is None else out
            if 'act' not in out:
                out['act'] = torch.empty((T, B, N, 2) if two else (T, B, N), dtype=torch.int32, device=self.device)
            # a caller-supplied action buffer of the single-head shape under a two-head actor would be overrun by the kernel
            # (it writes act[2 row], act[2 row + 1]): refuse it here, whoever built the dict.  out['act'] = None: the caller does not
            # want the sampled actions (pw_policy_rollout's act_out = NULL: served with a sink, refused by the library without one)
            want = (T, B, N, 2) if two else (T, B, N)
            if out['act'] is not None and (tuple(out['act'].shape) != want or out['act'].dtype != torch.int32 or not out['act'].is_contiguous()):
                raise ValueError('rollout: out["act"] must be a contiguous int32 tensor of shape %r (%s actor), got %r %s'
                                 % (want, 'two-head' if two else 'one-head', tuple(out['act'].shape), out['act'].dtype))
        io = _lib.step_io(out, ('obs', 'final_obs', 'rew', 'rew_shared', 'done', 'terminal'), lead=(T,))
        p = _lib.ptr
        sink = None
        if memory is not None or stats is not None:
            sink = _lib.PwRolloutSink()
            if memory is not None:
                sink.ring_start = memory.claim(T * B, N, env.obs_dim, self.device)   # refuses on the host, before the launch
                sink.ring = C.addressof(memory._store)
            if stats is not None:
                if getattr(self, '_sink_scratch_key', None) != (B, N):
                    nbytes = self.lib.pw_policy_rollout_scratch_bytes(env._h)
                    self._sink_scratch = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
                    self._sink_scratch_key = (B, N)
                sink.episode_return, sink.finished_sum, sink.finished_count = (t.data_ptr() for t in stats)
                sink.scratch = self._sink_scratch.data_ptr()
        step_dev = p(self._step_dev) if self.graph_mode else None
        _lib.check(self.lib.pw_policy_rollout(env._h, p(self.frag), p(self.b1), p(self.bih), p(self.whh_f),
                                              p(self.whh_r), p(self.w2), p(self.b2), 1, self.seed, self.calls,
                                              step_dev, C.byref(io), p(out.get('act')), T,
                                              None if sink is None else C.byref(sink), self._stream()))
        if memory is not None:
            memory._advance(T * B)
        if step_dev is not None and not self.defer_step_advance:
            _lib.check(self.lib.pw_counter_add(p(self._step_dev), T, 0, self._stream()))
        self.calls += T
        return out

    def begin_graph(self):
        """Switch to the device-side step counter (call before hipGraph capture)."""
        self._step_dev.fill_(self.calls)
        self.graph_mode = True


class FusedExploration(object):
    """``Trainer.get_exploration_action`` (rls/agent/multiagent/ddpg_gumbel_fix.py:86-107) on the one-launch actor:
    list of N observation arrays -> the hard Gumbel-softmax one-hot(s) the reference returns -- ``ndarray [1,N,5]``
    float32 (Discrete) or a list of two such arrays (MultiDiscrete, [1,N,5] and [1,N,dim_c]).  One HIP launch
    instead of MIOpen's ~45-kernel RNN path per environment step; weights are re-snapshotted by ``refresh()``."""

    def __init__(self, actor, action_type='Discrete', seed=0):
        self.action_type = action_type
        self.fused = FusedActor(actor, seed=seed)
        assert (len(self.fused.heads) == 2) == (action_type == 'MultiDiscrete')

    def refresh(self):
        self.fused.refresh()

    @torch.no_grad()
    def get_exploration_action(self, state):
        obs = torch.from_numpy(np.array([np.stack(state)], dtype='float32')).to(self.fused.device)   # process_obs
        idx = self.fused(obs).cpu().numpy()
        eye = [np.eye(n, dtype=np.float32) for n in self.fused.heads]
        if self.action_type == 'Discrete':
            return eye[0][idx]
        return [eye[0][idx[..., 0]], eye[1][idx[..., 1]]]


def accelerate_trainer(trainer, seed=0, targets=False, optimizer=False, lstm=False, attention=False, graph=False, graph_warmup=3,
                       sampling=False, sampling_seed=None, front=False, wgrad=False, heads=False):
    """Patch an instance of the reference's ``Trainer`` in place: ``get_exploration_action`` runs on the one-launch
    HIP actor, and the weight snapshot is refreshed after every ``optimize()`` (and ``load_models``).  Everything
    else of the learner is untouched.  Returns the ``FusedExploration`` object.

    ``targets=True`` additionally hands the no-gradient half of ``optimize()`` to the HIP kernels: ``trainer.target_actor`` and
    ``trainer.target_critic`` become thin wrappers whose ``forward`` / ``__call__`` run on ``FusedActor.logits`` and
    ``critic.FusedCritic`` (one launch each) and which pass everything else -- ``parameters()``, ``state_dict()``,
    ``load_state_dict()``, ``eval()``, ``train()``, ``to()`` -- to the wrapped module, so ``soft_update``, ``hard_update``,
    ``save_models`` and ``load_models`` work on the real networks.  The critic kernel reads the module's parameters in place; the
    target actor's snapshot is refreshed where the exploration actor's is.  The Gumbel sampling of ``a1`` stays the Trainer's.

    ``optimizer=True`` hands the arithmetic after the backward passes to the HIP kernels (``multiagent_rl_amd.optim``):
    ``trainer.actor_optimizer`` / ``trainer.critic_optimizer`` become ``FusedAdam`` objects with the hyper-parameters and state of
    the ``torch.optim.Adam`` they replace (one launch per ``step()``), and ``trainer.soft_update`` becomes the one-launch
    ``optim.soft_update``.  The Trainer's ``clip_grad_norm_`` calls stay torch's.  Works with and without ``targets``; the default
    leaves optimisers and ``soft_update`` exactly as they are.

    ``lstm=True`` runs the recurrent part of every served ``nn.LSTM`` the trainer owns -- actor, critic, and the target networks unless
    ``targets=True`` has already wrapped them -- on the HIP kernels with gradient (``multiagent_rl_amd.lstm.fuse_lstm``: a class swap,
    parameters and ``state_dict`` keys unchanged).  Opt-in like the other two: the kernels' gate activations differ from MIOpen's in
    the last bits, so a seeded run does not reproduce across the switch.

    ``attention=True`` runs the attention block of ``trainer.critic`` -- and of ``trainer.target_critic`` unless ``targets=True`` has
    already wrapped it -- on the HIP kernels with gradient (``multiagent_rl_amd.attention.fuse_attention``: a class swap to a subclass
    of the critic's own class, one launch forward and one backward instead of ``bmm`` / ``softmax`` / ``bmm`` / ``relu``).  The critic
    of the model-learning variant (a ``dense3`` beside ``dense2``) gets the same block without the ReLU (``fuse_model_attention``); a
    critic without that block (the BiCNet critic) is left as it is.  Opt-in for the same reason: the sums run in another order than
    rocBLAS's.

    The model-learning variant's Trainer (``model_ddpg_gumbel_fix.py``) is served by every switch: with ``targets=True`` the target
    actor's wrapper returns ``(logits, None)`` and the target critic's ``(q, r)``, as that Trainer unpacks them.

    ``graph=True`` (with all four switches; a critic without an attention block needs the first three) replaces ``trainer.optimize`` by a
    ``multiagent_rl_amd.graph.GraphedUpdate``: ``graph_warmup`` eager updates, then one captured update replayed as one graph launch per
    call.  The optimisers switch to ``graph_steps`` mode, the target actor's snapshot is refreshed in place inside the captured region,
    the exploration actor's eagerly after each replay; ``trainer.memory`` must be a ``ReplayBuffer(device_index='counter')``.  What is
    missing from that configuration is a ``ValueError`` that names it.  Switches a Trainer has already taken itself (the example
    learner's ``fused_optimizer`` / ``fused_lstm`` / ``fused_attention``) count.

    ``sampling=True`` runs the learner's Gumbel-softmax samples on the HIP kernels with gradient (``multiagent_rl_amd.sampling``): a
    ``GumbelSampler`` becomes ``trainer.gumbel_softmax`` (the reference Trainer's method) and / or ``trainer._sample`` (the example
    learner's), whichever the trainer has -- one launch forward and one backward per sample instead of ``F.gumbel_softmax``'s dozen
    kernels -- and its ``end_update()`` runs behind every ``optimize()``; with ``graph=True`` inside the captured region, so that every
    replay draws new noise.  The noise is the library's own Philox stream keyed by ``sampling_seed`` (default:
    ``sampling.default_seed(seed)``, never the exploration actor's key), a function of (seed, update number, call site, row, logit): not
    torch's generator, which is why this switch is opt-in too, and why a graphed run with it reproduces an eager one bit for bit.  A
    trainer that carries its own sampler (the example learner's ``fused_sampling``) keeps it.

    ``front=True`` runs what every pass with gradient begins with -- dense1, the ReLU and the LSTM's input projection -- on the HIP
    kernels with gradient (``multiagent_rl_amd.dense.fuse_front``: a class swap to a subclass of the network's own class, one launch
    forward and two backward instead of a dozen) for ``trainer.actor``, ``trainer.critic`` and the target networks that are still
    modules.  It needs ``lstm=True`` or LSTMs that are fused already (``ValueError`` otherwise) and composes with ``attention`` in
    either order.  Opt-in because the sums run in another order than rocBLAS's; it is not a precondition of ``graph=True``.

    ``wgrad=True`` takes the two ``W_hh`` gradients of every fused LSTM off torch (``multiagent_rl_amd.lstm.launch_wgrad``: one call of
    two device kernels per LSTM backward instead of two strided copies and a GEMM per direction).  It needs ``lstm=True`` or LSTMs that
    are fused already: ``ValueError`` if no LSTM is or becomes fused.  Opt-in because the sums run in another order than rocBLAS's; it
    is not a precondition of ``graph=True``.

    ``heads=True`` runs what every pass with gradient ends with -- the ReLU on the actor's BiLSTM output and every output layer
    (``dense2``, ``dense2_1`` + ``dense2_2``, ``dense3``) -- on the HIP kernels with gradient (``multiagent_rl_amd.heads.fuse_heads``: a
    plain attribute on the swapped networks, one launch forward for all heads and two backward) for ``trainer.actor``,
    ``trainer.critic`` and the target networks that are still modules.  It needs ``front=True`` or networks that ``dense.fuse_front``
    has swapped already (``ValueError`` otherwise): the fused output layers are the last lines of the swapped forwards.  Opt-in because
    the sums run in another order than rocBLAS's; it is not a precondition of ``graph=True`` and composes with it."""
    if heads and not front:   # refused before anything is patched
        from .heads import fuse_trainer as fuse_heads_trainer
        fuse_heads_trainer(trainer, dry=True)
    if wgrad and not lstm:   # refused before anything is patched
        from .lstm import wgrad_trainer
        wgrad_trainer(trainer, dry=True)
    if graph:   # what this call will not put right is refused before anything is patched (and before the GPU is needed)
        from .graph import missing_for_graph
        mended = [name for name, on in (('targets', targets), ('optimizer', optimizer), ('lstm', lstm), ('attention', attention)) if on]
        miss = [m for m in missing_for_graph(trainer) if m.split(':')[0] not in mended]
        if miss:
            raise ValueError('accelerate_trainer(graph=True): a captured update needs -- ' + '; '.join(miss))
    fx = FusedExploration(trainer.actor, getattr(trainer, 'action_type', 'Discrete'), seed=seed)
    trainer.get_exploration_action = fx.get_exploration_action
    trainer._pw_accel = fx
    target_actor = None
    if targets:
        from .critic import fuse_targets
        target_actor, fx.target_critic = fuse_targets(trainer)
        fx.target_actor = target_actor
    if optimizer:
        from .optim import fuse_optimizers
        fx.optimizers = fuse_optimizers(trainer, graph_steps=graph)
    if lstm:
        from .lstm import fuse_trainer
        fx.fused_lstms = fuse_trainer(trainer)
    if wgrad:
        from .lstm import wgrad_trainer
        fx.wgrad_lstms = wgrad_trainer(trainer)   # ValueError: lstm=True found no LSTM that FusedLSTM serves
    if attention:
        from .attention import fuse_trainer as fuse_attention_trainer
        fx.fused_attentions = fuse_attention_trainer(trainer)
    if front:
        from .dense import fuse_trainer as fuse_front_trainer
        fx.fused_fronts = fuse_front_trainer(trainer)
    if heads:
        from .heads import fuse_trainer as fuse_heads_trainer
        fx.fused_heads = fuse_heads_trainer(trainer)
    sampler = None
    if sampling:
        from .sampling import install
        fx.sampler, owned = install(trainer, seed=sampling_seed, exploration_seed=seed)
        sampler = fx.sampler if owned else None   # a trainer with its own sampler closes its updates itself
        fx.owned_sampler = sampler

    def _wrap(name):
        inner = getattr(trainer, name, None)
        if inner is None:
            return

        def wrapped(*a, **k):
            out = inner(*a, **k)
            if sampler is not None and name == 'optimize':
                sampler.end_update()
            fx.refresh()
            if target_actor is not None:
                target_actor.refresh(in_place=graph)   # a captured update holds the snapshot's addresses
            return out
        setattr(trainer, name, wrapped)
    fx.inner_optimize = getattr(trainer, 'optimize', None)
    if graph:
        from .graph import GraphedUpdate
        fx.graphed = GraphedUpdate(trainer, warmup=graph_warmup)   # ValueError naming what is missing
        trainer.optimize = fx.graphed
    else:
        _wrap('optimize')
    _wrap('load_models')
    return fx


class UniformRandomPolicy(object):
    """i.i.d. uniform action indices (the synthetic-action workload of bench.py).  ``num_actions`` may be a
    list with one entry per agent (simple_speaker_listener: [3, 5])."""

    def __init__(self, num_actions=5, generator=None):
        self.num_actions, self.generator = num_actions, generator

    def __call__(self, obs):
        if isinstance(self.num_actions, (list, tuple)):
            cols = [torch.randint(0, int(n), obs.shape[:1], device=obs.device, dtype=torch.int32, generator=self.generator)
                    for n in self.num_actions]
            return torch.stack(cols, 1)
        return torch.randint(0, self.num_actions, obs.shape[:2], device=obs.device, dtype=torch.int32,
                             generator=self.generator)
