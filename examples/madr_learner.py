"""A minimal stock-PyTorch learner with the Trainer surface ``experiments/run.py:21,37,52,81,102`` consumes, so that
``examples/train_batched.py`` runs where the reference checkout (and its ``rls`` package) is not importable.

NOT part of the product and not the reference's algorithm in detail: the learner is out of scope of this repo (north_star: it
stays stock PyTorch-ROCm); inside a checkout of the reference, pass its own
``rls.agent.multiagent.ddpg_gumbel_fix.Trainer`` / ``rls.model.ac_network_multi_gumbel.CriticNetwork`` instead (``--reference``).
What it keeps: DDPG with hard Gumbel-softmax categorical actions, one shared reward per transition, target networks with
soft updates, Adam, batches drawn through ``memory.make_index`` / ``memory.sample_index``.
``BiCNetTrainer`` is the per-agent variant (the BiCNet baseline's tuple, ``experiments/run_BIC.py:46,50`` and
``BIC_gumbel_fix.py:155-160``): a ``per_agent`` ring, a critic that returns one Q per agent (``multiagent_rl_amd.critic.BiCNetCritic``)
and the TD target formed on ``[b, N]``.
``ModelTrainer`` is the model-learning variant (``model_ddpg_gumbel_fix.py``): networks that return pairs (``ModelActorNetwork`` /
``ModelCriticNetwork``) and an L1 model loss on each of the two losses.
``Trainer(..., fused_optimizer=True)``: each network's clip + Adam step + soft update is one HIP launch
(``multiagent_rl_amd.optim.FusedAdam``); the default is the stock sequence.
``Trainer(..., fused_lstm=True)``: the LSTMs of actor and critic (and of the target networks copied from them) run their recurrence,
forward and backward, on the HIP kernels (``multiagent_rl_amd.lstm.fuse_lstm``); the default is ``nn.LSTM``.
``Trainer(..., fused_attention=True)``: the attention block of an attention critic (and of the target critic copied from it) runs,
forward and backward, on the HIP kernels (``multiagent_rl_amd.attention.fuse_attention``); the default is the stock expression, and a
critic without that block is left as it is.
``Trainer(..., graph_update=True)``: the whole update is captured once and replayed as one graph launch per ``optimize()``
(``multiagent_rl_amd.graph.GraphedUpdate``, installed by ``accelerate_trainer(self, targets=True, ..., graph=True)``); it needs the three
switches above and a ``ReplayBuffer(device_index='counter')``, and says what is missing otherwise.  ``optimize()`` then returns the two
loss TENSORS of the replay (no read-back per update); ``optimize.losses()`` reads them.
``Trainer(..., fused_sampling=True, sampling_seed=None)``: both Gumbel-softmax samples of an update (four with two heads) run on the HIP
kernels, one launch forward and one backward each (``multiagent_rl_amd.sampling.GumbelSampler``), with the library's own noise keyed
(``sampling_seed``; update number, call site, row) instead of torch's generator -- a graphed run then reproduces an eager one bit for bit.
The default is ``F.gumbel_softmax``; the B = 1 ``get_exploration_action`` keeps it either way.
``Trainer(..., fused_front=True)``: dense1, the ReLU and the LSTM's input projection of actor and critic (and of the target networks
copied from them) run, forward and backward, on the HIP kernels (``multiagent_rl_amd.dense.fuse_front``); it needs ``fused_lstm``, and
the default is the stock expression.
``Trainer(..., fused_wgrad=True)``: the two ``W_hh`` gradients of every fused LSTM come from ``multiagent_rl_amd.lstm.launch_wgrad`` (two
device kernels per LSTM backward) instead of two strided copies and a GEMM per direction; it needs ``fused_lstm``, and the default is the
GEMMs (the sums run in another order).
``Trainer(..., fused_heads=True)``: the ReLU on the actor's BiLSTM output and every output layer of actor and critic (and of the target
networks copied from them) run, forward and backward, on the HIP kernels (``multiagent_rl_amd.heads.fuse_heads``: one launch forward
for all heads of a network, two backward); it needs ``fused_front``, and the default is the stock expression.
"""
import copy
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

GAMMA, TAU = 0.95, 1e-2   # rls/agent/multiagent/ddpg_gumbel_fix.py:10, rls/arglist.py:12


class CriticNetwork(nn.Module):
    """Q(obs [b,N,D], action one-hots [b,N,A]) -> [b,1]: per-agent embedding, mean over the agent axis, two dense layers."""

    def __init__(self, input_dim, out_dim=1):
        super().__init__()
        self.embed = nn.Linear(input_dim, 64)
        self.mix = nn.Linear(64, 64)
        self.out = nn.Linear(64, out_dim)

    def forward(self, obs, action):
        h = F.relu(self.embed(torch.cat([obs, action], dim=-1))).mean(dim=1)
        return self.out(F.relu(self.mix(h)))


class Trainer(object):
    per_agent = False   # BiCNetTrainer: per-agent rewards / dones [b,N] and a critic that returns [b,N,1]

    def __init__(self, actor, critic, memory, action_type='Discrete', batch_size=1024, lr=1e-2, device=None, fused_optimizer=False,
                 fused_lstm=False, fused_attention=False, graph_update=False, fused_sampling=False, sampling_seed=None,
                 fused_front=False, fused_wgrad=False, fused_heads=False):
        if fused_heads and not fused_front:
            raise ValueError('fused_heads needs fused_front: the fused output layers are the last lines of the swapped forwards')
        if fused_wgrad and not fused_lstm:
            raise ValueError('fused_wgrad needs fused_lstm: the W_hh gradients of a plain nn.LSTM are MIOpen\'s')
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.actor, self.critic = actor.to(self.device), critic.to(self.device)
        self.sampler = None
        if fused_sampling:   # an INSTANCE attribute: a subclass (or a test) that overrides _sample keeps its own on every other instance
            from multiagent_rl_amd.sampling import GumbelSampler
            self.sampler = GumbelSampler(seed=sampling_seed, device=self.device)
            self._sample = self.sampler.sample
        if fused_attention:   # before the deep copies, like fused_lstm
            self._fuse_attention(self.critic)
        if fused_lstm:   # before the deep copies: a class swap survives them, so the target networks are fused too
            from multiagent_rl_amd.lstm import fuse_lstm
            fuse_lstm(self.actor, wgrad=bool(fused_wgrad))
            fuse_lstm(self.critic, wgrad=bool(fused_wgrad))
        if fused_front:   # before the deep copies too; a ValueError says so where an LSTM is still nn.LSTM
            from multiagent_rl_amd.dense import fuse_front
            fuse_front(self.actor)
            fuse_front(self.critic)
        if fused_heads:   # before the deep copies: the mode is an instance attribute, which they keep
            from multiagent_rl_amd.heads import fuse_heads
            fuse_heads(self.actor)
            fuse_heads(self.critic)
        self.target_actor, self.target_critic = copy.deepcopy(self.actor).eval(), copy.deepcopy(self.critic).eval()
        self.actor_optimizer = torch.optim.Adam(self.actor.parameters(), lr)
        self.critic_optimizer = torch.optim.Adam(self.critic.parameters(), lr)
        self.fused_optimizer = bool(fused_optimizer)
        if self.fused_optimizer:   # clip (0.5) + Adam + soft update of the target: one launch per network
            from multiagent_rl_amd.optim import FusedAdam
            self.actor_optimizer = FusedAdam(self.actor.parameters(), lr, max_norm=0.5, targets=self.target_actor.parameters(), tau=TAU,
                                             graph_steps=bool(graph_update))
            self.critic_optimizer = FusedAdam(self.critic.parameters(), lr, max_norm=0.5, targets=self.target_critic.parameters(), tau=TAU,
                                              graph_steps=bool(graph_update))
        self.memory, self.action_type, self.batch_size = memory, action_type, batch_size
        self.iter = 0
        if graph_update:   # the target networks go to the HIP kernels and optimize() becomes the graphed update (or a ValueError says why not)
            from multiagent_rl_amd.policy import accelerate_trainer
            accelerate_trainer(self, targets=True, graph=True)

    @staticmethod
    def _fuse_attention(critic):
        from multiagent_rl_amd.attention import fuse_attention
        fuse_attention(critic)

    # What ModelTrainer overrides: its networks return pairs, and each loss gains an L1 term on the pair's second value.
    @staticmethod
    def _first(out):
        return out

    @staticmethod
    def _with_reward_loss(loss, out, r):
        return loss

    @staticmethod
    def _with_state_loss(loss, out, s1):
        return loss

    @staticmethod
    def _sample(logits):
        if isinstance(logits, (list, tuple)):       # MultiDiscrete: one one-hot per head, concatenated (run.py:39-41)
            return torch.cat([F.gumbel_softmax(x, hard=True, dim=-1) for x in logits], dim=-1)
        return F.gumbel_softmax(logits, hard=True, dim=-1)

    @torch.no_grad()
    def get_exploration_action(self, state):
        import numpy as np
        obs = torch.from_numpy(np.array([np.stack(state)], dtype='float32')).to(self.device)
        logits = self._first(self.actor(obs))
        if isinstance(logits, (list, tuple)):
            return [F.gumbel_softmax(x, hard=True, dim=-1).cpu().numpy() for x in logits]
        return F.gumbel_softmax(logits, hard=True, dim=-1).cpu().numpy()

    def optimize(self):
        loss_actor, loss_critic = self.optimize_tensors()
        return float(loss_actor), float(loss_critic)

    def optimize_tensors(self):
        """One update; -> (loss_actor, loss_critic) as device tensors: no read-back, so the whole of it can be captured in a graph."""
        s0, a0, r, s1, d = (torch.as_tensor(x, dtype=torch.float32, device=self.device)
                            for x in self.memory.sample_index(self.memory.make_index(self.batch_size)))
        if r.dim() != (2 if self.per_agent else 1):
            raise ValueError('%s needs a ring with %s rewards' % (type(self).__name__, 'per-agent' if self.per_agent else 'shared'))
        with torch.no_grad():   # shared: [b,1]; per agent: [b,N,1] (q_next one per agent, y formed on [b,N])
            q_next = self._first(self.target_critic(s1, self._sample(self._first(self.target_actor(s1)))))
            y = r.unsqueeze(-1) + GAMMA * (1.0 - d.unsqueeze(-1)) * q_next
        out = self.critic(s0, a0)
        loss_critic = self._with_reward_loss(F.smooth_l1_loss(self._first(out), y), out, r)
        self.critic_optimizer.zero_grad()
        loss_critic.backward()
        if not self.fused_optimizer:
            nn.utils.clip_grad_norm_(self.critic.parameters(), 0.5)
        self.critic_optimizer.step()
        out = self.actor(s0)
        loss_actor = self._with_state_loss(-self._first(self.critic(s0, self._sample(self._first(out)))).mean(), out, s1)
        self.actor_optimizer.zero_grad()
        loss_actor.backward()
        if not self.fused_optimizer:
            nn.utils.clip_grad_norm_(self.actor.parameters(), 0.5)
        self.actor_optimizer.step()
        if not self.fused_optimizer:
            with torch.no_grad():
                for tgt, src in ((self.target_actor, self.actor), (self.target_critic, self.critic)):
                    for pt, ps in zip(tgt.parameters(), src.parameters()):
                        pt.mul_(1.0 - TAU).add_(ps, alpha=TAU)
        if self.sampler is not None:   # the next update's noise: the cell advances on the device, inside a captured update too
            self.sampler.end_update()
        self.iter += 1
        return loss_actor.detach(), loss_critic.detach()

    def save_models(self, name, out_dir='Models'):
        """Target nets' state_dicts as ``<name>_actor.pt`` / ``<name>_critic.pt`` (ddpg_gumbel_fix.py:221-229)."""
        os.makedirs(out_dir, exist_ok=True)
        torch.save(self.target_actor.state_dict(), os.path.join(out_dir, name + '_actor.pt'))
        torch.save(self.target_critic.state_dict(), os.path.join(out_dir, name + '_critic.pt'))

    def load_models(self, name, out_dir='Models'):
        self.actor.load_state_dict(torch.load(os.path.join(out_dir, name + '_actor.pt')))
        self.critic.load_state_dict(torch.load(os.path.join(out_dir, name + '_critic.pt')))
        self.target_actor.load_state_dict(self.actor.state_dict())
        self.target_critic.load_state_dict(self.critic.state_dict())


class ModelTrainer(Trainer):
    """The learner of the model-learning variant (``rls/agent/multiagent/model_ddpg_gumbel_fix.py``): ``actor`` returns ``(policy,
    next_state)`` and ``critic`` ``(Q, r)`` (``multiagent_rl_amd.policy.ModelActorNetwork`` / ``multiagent_rl_amd.critic.ModelCriticNetwork``);
    the critic loss gains ``L1(pred_r, r)`` (:171) and the actor loss ``L1(pred_s1, s1)`` (:204).  The no-gradient half keeps the first
    value of each pair (:150, :158).  Same switches as ``Trainer``; ``fused_attention`` is the swap without the ReLU
    (``fuse_model_attention``).  The reference's ``l2_reg`` term stays out, as in ``Trainer``."""

    @staticmethod
    def _fuse_attention(critic):
        from multiagent_rl_amd.attention import fuse_model_attention
        fuse_model_attention(critic)

    @staticmethod
    def _first(out):
        return out[0]

    @staticmethod
    def _with_reward_loss(loss, out, r):
        return loss + F.l1_loss(out[1].squeeze(-1), r)

    @staticmethod
    def _with_state_loss(loss, out, s1):
        return loss + F.l1_loss(out[1], s1)


class BiCNetTrainer(Trainer):
    """The same learner on the BiCNet tuple: ``memory`` is a ``per_agent`` ring (``rew`` / ``done`` [b,N]), ``critic`` returns one Q per
    agent ([b,N,1], e.g. ``multiagent_rl_amd.critic.BiCNetCritic``), y = r + GAMMA * (1 - d) * q_next per agent."""
    per_agent = True
