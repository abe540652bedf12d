"""The learner's critic: the reference's architecture as a host module, and its no-gradient forward as one HIP launch.

``CriticNetwork`` has the layer structure AND parameter names of ``rls/model/ac_network_multi_gumbel.py:70-146``
(``dense1.module``, ``lstm``, ``dense2``), so ``<scenario>_fin_<cnt>_critic.pt`` files saved by the reference's Trainer
(``ddpg_gumbel_fix.py:221-229``) load unchanged.  It is the autograd path: the learner keeps it for ``critic(s0, a0)`` and the
actor loss (the gradient path stays stock PyTorch-ROCm).

``FusedCritic`` evaluates the same module with ``pw_critic_forward`` -- dense1, the LSTM over the agent axis, the attention and
dense2 in ONE launch instead of MIOpen's many-kernel RNN path, two ``bmm``s, a softmax and the glue -- for the half of
``Trainer.optimize`` that needs no gradient: ``q_next = target_critic(s1, a1)`` and ``y = r + GAMMA * q_next * (1 - d)``
(``ddpg_gumbel_fix.py:148-154``).  ``accelerate_trainer(trainer, targets=True)`` hands both target networks of an unmodified
Trainer to the HIP kernels.

``BiCNetCritic`` is the baseline's critic (``rls/model/ac_network_multi_gumbel_BIC.py:69-141``): the same dense1 and LSTM, then
``TimeDistributed(Linear(64, 1))`` on every step's output -- one Q per agent, ``[b, N, 1]``, no attention.  ``FusedCritic`` serves
it with ``pw_critic_forward_steps`` (q and the per-agent TD target of ``BIC_gumbel_fix.py:155-160`` on ``[b, N]``); which of the
two critics it wraps is read off the structure: ``dense2`` is a ``TimeDistributed`` there and a plain ``Linear`` here.

``ModelCriticNetwork`` is the critic of the paper's own method, the model-learning variant
(``rls/model/ac_network_model_multi_gumbel.py:69-143``): the attention critic without the ReLU on the context and with a second head,
``dense3``, that predicts the reward -- ``forward`` returns ``(Q, r)``.  ``FusedCritic`` serves it with ``pw_critic_forward_model``
(``model``: a plain ``dense3 = Linear(64, 1)`` beside a plain ``dense2``): ``q``, ``reward``, ``td_target`` from the launch's own q
(``model_ddpg_gumbel_fix.py:158-163``), and ``forward`` -> the pair.
"""
import torch
import torch.nn as nn

from . import _lib
from .attention import attend, critic_form, lstm_trunk
from .policy import FusedActor, TimeDistributed
from .policy import accelerate_trainer  # noqa: F401  (the one entry point; ``targets=True`` uses the classes below)


class _LstmCritic(nn.Module):
    """The trunk of the three critics: Linear(D + A, 64) -> ReLU -> LSTM(64 -> 64) over the AGENT axis (``attention.lstm_trunk`` runs
    it).  Subclasses add ``dense2`` (then ``dense3``) after it, so submodules register in the reference's order."""

    def __init__(self, input_dim):
        super().__init__()
        self.dense1 = TimeDistributed(nn.Linear(input_dim, 64))
        self.lstm = nn.LSTM(64, 64, num_layers=1, batch_first=True, bidirectional=False)

    def context(self, obs, action, relu):
        """The attention of every step's output against the final hidden state (dot product, softmax over the agents, weighted sum)."""
        steps, h_n = lstm_trunk(self, obs, action)                        # [b,N,64], [1,b,64]
        return attend(steps, h_n[-1], relu)


class CriticNetwork(_LstmCritic):
    """The trunk -> attention -> ReLU -> Linear(64, out_dim).
    ``forward(obs [b,N,D], action [b,N,A] or a list of such)`` -> ``[b, out_dim]``."""

    def __init__(self, input_dim, out_dim=1):
        super().__init__(input_dim)
        self.dense2 = nn.Linear(64, out_dim)

    def forward(self, obs, action):
        return self.dense2(self.context(obs, action, relu=True))


class BiCNetCritic(_LstmCritic):
    """The trunk -> TimeDistributed(Linear(64, out_dim)) on the LSTM's output itself (no ReLU, no attention): one Q per agent.  Layer
    names as the reference's (``dense1.module``, ``lstm``, ``dense2.module``).
    ``forward(obs [b,N,D], action [b,N,A] or a list of such)`` -> ``[b, N, out_dim]``."""

    def __init__(self, input_dim, out_dim=1):
        super().__init__(input_dim)
        self.dense2 = TimeDistributed(nn.Linear(64, out_dim))

    def forward(self, obs, action):
        return self.dense2(lstm_trunk(self, obs, action)[0])


class ModelCriticNetwork(_LstmCritic):
    """The trunk -> the attention of ``CriticNetwork`` -> two heads on the context itself (no ReLU): ``dense2`` = Q, ``dense3`` = the
    predicted reward.  Layer names as the reference's (``dense1.module``, ``lstm``, ``dense2``, ``dense3``).
    ``forward(obs [b,N,D], action [b,N,A] or a list of such)`` -> ``(Q [b, out_dim], r [b, out_dim])``."""

    def __init__(self, input_dim, out_dim=1):
        super().__init__(input_dim)
        self.dense2 = nn.Linear(64, out_dim)
        self.dense3 = nn.Linear(64, out_dim)

    def forward(self, obs, action):
        ctx = self.context(obs, action, relu=False)
        return self.dense2(ctx), self.dense3(ctx)


class FusedCritic(object):
    """``critic`` (a ``CriticNetwork``, a ``BiCNetCritic`` or a ``ModelCriticNetwork`` -- this module's or the reference's -- on the
    GPU) evaluated by ``pw_critic_forward`` / ``pw_critic_forward_steps`` / ``pw_critic_forward_model``.  ``per_step`` says which: True
    where ``critic.dense2`` wraps its Linear in a ``.module`` (the per-step critic: ``q`` / ``td_target`` are ``[b, N]``, ``forward``
    ``[b, N, 1]``, ``rew`` / ``done`` ``[b, N]``).  ``model``: True where the critic has a ``dense3`` (it must be a plain ``Linear(64, 1)``
    beside a plain ``dense2``): no ReLU on the context, ``reward(obs, act)`` is the second head and ``forward`` returns ``(q, r)``.

    The kernel reads the parameters where the module keeps them (``nn.Module`` layout, no packed image), so every call computes
    with the module's CURRENT values: a soft update in place between two calls needs no ``refresh()``.  No gradient flows through
    it: results have ``requires_grad == False``.  ``heads``: the widths of a two-head (MultiDiscrete) joint action, needed only
    for index actions of shape ``[b,N,2]``."""

    def __init__(self, critic, heads=None):
        self.lib = _lib.load()
        self.critic = critic
        self.heads = None if heads is None else tuple(int(h) for h in heads)
        form, widths = critic_form(critic)
        self.per_step, self.model = form == 'steps', form == 'model'
        if form is None or any(w != 1 for w in widths):
            raise ValueError('FusedCritic serves Linear(D + A, 64) -> LSTM(64 -> 64) -> attention -> Linear(64, 1), the per-step '
                             'form Linear(D + A, 64) -> LSTM(64 -> 64) -> TimeDistributed(Linear(64, 1)) and the model-learning form '
                             'LSTM(64 -> 64) -> attention -> Linear(64, 1) twice (dense2, dense3); other heads (a dense3 that is '
                             'not a plain Linear(64, 1), or one beside a per-step dense2) are not served')
        self._params()

    def _dense2(self):
        return self.critic.dense2.module if self.per_step else self.critic.dense2

    def _params(self):
        c = self.critic
        lin1, lstm, lin2 = c.dense1.module, c.lstm, self._dense2()
        ps = (lin1.weight, lin1.bias, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0, lin2.weight, lin2.bias)
        if self.model:
            ps += (c.dense3.weight, c.dense3.bias)
        dev = ps[0].device
        if dev.type != 'cuda':
            raise RuntimeError('FusedCritic needs the critic on the GPU (no CPU fallback)')
        for p in ps:   # read in place: anything else would be a snapshot that an in-place update leaves behind
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError('FusedCritic reads contiguous float32 parameters on one GPU')
        self.device = dev
        return ps

    @torch.no_grad()
    def _run(self, obs, act, rew=None, done=None, gamma=0.0, want_reward=False):
        """-> (q, y or None); the model form: (q, y or None, r_pred or None)."""
        ps = self._params()
        if obs.dim() != 3:
            raise ValueError('obs must be [b, N, D]')
        b, N, D = obs.shape
        A = ps[0].shape[1] - D
        f32 = lambda t: t.detach().to(device=self.device, dtype=torch.float32).contiguous()  # noqa: E731
        x = f32(obs)
        if isinstance(act, (list, tuple)):
            act = torch.cat(list(act), dim=-1)
        idx = vec = None
        if act.dtype.is_floating_point:
            if tuple(act.shape) != (b, N, A):
                raise ValueError('float action must be [b, N, %d], got %r' % (A, tuple(act.shape)))
            vec, n0, n1 = f32(act), A, 0
        else:
            idx = act.detach().to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(idx.shape) == (b, N):
                n0, n1 = A, 0
            elif tuple(idx.shape) == (b, N, 2):
                if self.heads is None or len(self.heads) != 2 or sum(self.heads) != A:
                    raise ValueError('index actions [b, N, 2] need FusedCritic(critic, heads=(n0, n1)) with n0 + n1 = %d' % A)
                n0, n1 = self.heads
            else:
                raise ValueError('index action must be [b, N] or [b, N, 2], got %r' % (tuple(idx.shape),))
        shape = (b, N) if self.per_step else (b,)
        q = torch.empty(shape, dtype=torch.float32, device=self.device)
        y = r = d = None
        if rew is not None:
            if self.per_step:
                if tuple(rew.shape) != shape or tuple(done.shape) != shape:
                    raise ValueError('the per-step critic takes per-agent rew and done of shape [b, N] = %r, got %r and %r' % (
                        shape, tuple(rew.shape), tuple(done.shape)))
                r, d = f32(rew), f32(done)
            else:
                r, d = f32(rew).reshape(-1), f32(done).reshape(-1)
                if r.numel() != b or d.numel() != b:
                    raise ValueError('rew and done must hold one number per batch row')
            y = torch.empty(shape, dtype=torch.float32, device=self.device)
        p, stream = _lib.ptr, _lib.stream(self.device)
        if self.model:   # the second head only where it is asked for: the target critic's launch stores no reward prediction
            rp = torch.empty(shape, dtype=torch.float32, device=self.device) if want_reward else None
            _lib.check(self.lib.pw_critic_forward_model(p(x), p(idx), p(vec), n0, n1, *[p(t) for t in ps], b, N, D, p(r), p(d),
                                                        float(gamma), p(q), p(rp), p(y), stream))
            return q, y, rp
        entry = self.lib.pw_critic_forward_steps if self.per_step else self.lib.pw_critic_forward
        _lib.check(entry(p(x), p(idx), p(vec), n0, n1, *[p(t) for t in ps], b, N, D, p(r), p(d), float(gamma), p(q), p(y), stream))
        return q, y

    def q(self, obs, act):
        """obs [b,N,D]; act int [b,N] / [b,N,2] (indices) or float [b,N,A] -> q [b] ([b,N] for the per-step critic)."""
        return self._run(obs, act)[0]

    def td_target(self, next_obs, act, rew, done, gamma, return_q=False):
        """-> y [b] = rew + gamma * q(next_obs, act) * (1 - done) from one launch (``return_q``: also that launch's q).  The per-step
        critic: rew, done and y are per agent, [b,N]."""
        q, y = self._run(next_obs, act, rew, done, gamma)[:2]
        return (y, q) if return_q else y

    def reward(self, obs, act):
        """The model form's second head: the predicted reward [b] (from a launch that also forms q)."""
        if not self.model:
            raise ValueError('reward() needs a model-learning critic (one with dense3)')
        return self._run(obs, act, want_reward=True)[2]

    def forward(self, obs, action):
        """As the module: ``[b, 1]`` (``[b, N, 1]`` for the per-step critic; the pair ``(q [b, 1], r [b, 1])`` for the model form); a
        list of action tensors is concatenated along the last axis."""
        if self.model:
            q, _, rp = self._run(obs, action, want_reward=True)
            return q.unsqueeze(-1), rp.unsqueeze(-1)
        return self._run(obs, action)[0].unsqueeze(-1)

    __call__ = forward


class _FusedTarget(object):
    """A target network of a Trainer whose ``forward`` / ``__call__`` run on a HIP kernel; every other attribute
    (``parameters``, ``state_dict``, ``load_state_dict``, ``eval``, ``train``, ``to``, ...) is the wrapped module's."""

    def __init__(self, module, forward):
        self.__dict__['module'] = module
        self.__dict__['forward'] = forward

    def __call__(self, *a, **k):
        return self.forward(*a, **k)

    def __getattr__(self, name):
        return getattr(self.__dict__['module'], name)


def fuse_targets(trainer):
    """``trainer.target_actor`` / ``trainer.target_critic`` -> wrappers on ``FusedActor.logits`` / ``FusedCritic``.
    Returns ``(fused_target_actor, fused_target_critic)``; the caller refreshes the actor's snapshot after the target moves.
    The model-learning variant: a target actor with ``dense3`` returns ``(logits, None)`` -- the no-gradient half discards the
    predicted next state (``model_ddpg_gumbel_fix.py:150``), so the launch does not form it -- and a model critic the pair ``(q, r)``."""
    fa = FusedActor(trainer.target_actor, seed=0)
    fc = FusedCritic(trainer.target_critic)
    actor_forward = (lambda obs: (fa.logits(obs), None)) if hasattr(trainer.target_actor, 'dense3') else fa.logits
    trainer.target_actor = _FusedTarget(trainer.target_actor, actor_forward)
    trainer.target_critic = _FusedTarget(trainer.target_critic, fc.forward)
    return fa, fc
