"""One update of the example learner (examples/madr_learner.py: Trainer, BiCNetTrainer, ModelTrainer) restated in plain torch on stock
modules, a recorder that reads what a live learner did in one ``optimize()``, and the check that holds the two together.

Written from ``Trainer.optimize_tensors``' formulas, not from the kernels:

    (A)  a1 = sample(target_actor(s1));  q_next = target_critic(s1, a1);  y = r + GAMMA (1 - d) q_next          (no gradient)
    (B)  loss_critic = smooth_l1(critic(s0, a0), y) [+ L1(r_pred, r)];  backward from zeroed critic gradients
    (C)  clip to 0.5, Adam, Polyak update of the target critic
    (D)  loss_actor = -mean critic(s0, sample(actor(s0))) [+ L1(s1_pred, s1)];  backward from zeroed actor gradients: the critic's
         gradients ACCUMULATE on those of (B)
    (E)  clip, Adam, Polyak update of the target actor

``Restatement`` runs that in any dtype on any device.  Free-running it is the algorithm itself (tests/test_update_ref_host.py holds it
to the learner's three classes in float64).  STAGED on a record (``restate``) it continues from the learner's own value wherever the
map is discontinuous or ill-conditioned, so that a float32 learner can be compared with float64 quantity by quantity:

* noise: ``sampling_ref.noise(seed, SITES_PER_UPDATE * update + site, rows, n)``, one site per head per ``_sample`` call;
* picks: the hard sample is ``(onehot(pick) - soft) + soft`` with the restatement's own ``soft`` and the learner's ``pick``;
* the actor pass runs with the critic at the learner's post-step parameters;
* both optimiser stages take the learner's gradients and pre-step state (float64: ``optim_ref.AdamF64``; float32: the stock
  ``clip_grad_norm_`` + ``torch.optim.Adam(foreach=False)`` + soft update).

One thing differs between the learner's two optimisers and is restated as such (``meta['fused_optimizer']``): ``FusedAdam`` scales the
gradients in registers, so the critic's gradients of (D) accumulate on those of (B) as autograd left them; the stock sequence's
``clip_grad_norm_`` writes ``.grad``, so there they accumulate on the clipped ones.

The pick itself is checked apart (``check_case``): the learner's pick must be the float64 argmax on every row whose float64 top-two
margin of ``logits - noise`` is at least 2 e, e the site's largest |learner logits - float64 logits|.

``Recorder`` is test-side: instance attributes and hooks on one learner, nothing in the package changes.  What it cannot read it says:
``y`` is never handed to anything the recorder can wrap, so the record's ``y`` is the learner's expression on the recorded ``q_next``,
``r`` and ``d`` in the learner's dtype.  With a stock optimiser (the CPU runs) ``clip_grad_norm_`` has already scaled ``.grad`` when
``step()`` runs, so there the gradients are read by post-accumulate hooks and the norm is formed from them; with ``FusedAdam`` they are
read in the ``step()`` wrapper, as autograd left them, and the norm is ``last_total_norm``.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests import optim_ref, sampling_ref

GAMMA, TAU, MAX_NORM, BETAS, EPS = 0.95, 1e-2, 0.5, (0.9, 0.999), 1e-8
SITES_PER_UPDATE = 16
NETS = ('actor', 'critic', 'target_actor', 'target_critic')
BOUND, NORM_REL, SMALL, LEFT_OUT, L1_MARGIN = 4.0, 2e-6, 64, 0.02, 1e-4

MUTATIONS = ('stale target critic', 'stale target actor', 'noise of site + 1', '(1 - d) dropped', 'actor pass on the pre-step critic',
             'critic gradients cleared between the passes', 'accumulated gradients fed to the optimiser', 'clip coefficient omitted',
             'soft update from the pre-step parameters', 'L1 term dropped', 'y from the agent-mean reward')


def make_meta(variant, seed, lr=1e-2):
    """What a record says about its learner: the variant of tests/test_gpu_update_graph.VARIANTS, the sampler's seed, the learning rate."""
    import tests.test_gpu_update_graph as ug
    from multiagent_rl_amd import critic as cr, policy as pol
    cls_name, mk_actor, mk_critic, ring_kw, N, D = ug.VARIANTS[variant]
    actor, critic = mk_actor(pol, cr), mk_critic(pol, cr)
    return dict(variant=variant, cls=cls_name, model=cls_name == 'ModelTrainer', per_agent=cls_name == 'BiCNetTrainer',
                make_actor=lambda: mk_actor(pol, cr), make_critic=lambda: mk_critic(pol, cr), seed=int(seed), lr=float(lr),
                names=dict(actor=[n for n, _ in actor.named_parameters()], critic=[n for n, _ in critic.named_parameters()]))


def flat(out):
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in flat(o)]
    return [out]


def _heads(x):
    return list(x) if isinstance(x, (list, tuple)) else [x]


def _clone(ts):
    return [t.detach().clone() for t in ts]


# ---- the complete state of a learner ------------------------------------------------------------------------------------------------
def learner_state(t):
    """Parameters of the four networks and both optimisers' moments and step (a parameter without state yet: zeros and step 0, what
    Adam starts from)."""
    st = {n: _clone(getattr(t, n).parameters()) for n in NETS}
    for n in ('actor', 'critic'):
        opt, ps = getattr(t, n + '_optimizer'), list(getattr(t, n).parameters())
        have = [opt.state.get(p) or None for p in ps]
        st[n + '_opt'] = dict(exp_avg=[torch.zeros_like(p) if s is None else s['exp_avg'].detach().clone() for p, s in zip(ps, have)],
                              exp_avg_sq=[torch.zeros_like(p) if s is None else s['exp_avg_sq'].detach().clone() for p, s in zip(ps, have)],
                              step=[0.0 if s is None else float(s['step']) for s in have])
    return st


def state_tensors(st):
    out = [t for n in NETS for t in st[n]]
    for n in ('actor_opt', 'critic_opt'):
        out += st[n]['exp_avg'] + st[n]['exp_avg_sq'] + [torch.tensor(st[n]['step'])]
    return out


def same_bits(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32) if a.dtype == torch.float32 else a,
                                                                      b.contiguous().view(torch.int32) if b.dtype == torch.float32 else b)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
class Restatement(object):
    """The learner of ``meta`` in ``dtype`` on ``device``, from ``state`` (cast exactly).  ``update(batch, u)`` runs update number ``u``
    and returns a record of the recorder's form; ``staged``: the learner's record it continues from (see the module's docstring);
    ``mutate``: one of ``MUTATIONS``, the update done wrongly in that one way."""

    def __init__(self, meta, state, dtype, device):
        self.meta, self.dtype, self.device = meta, dtype, torch.device(device)
        self.state = self._cast_state(state)
        self.prev = self.prev_acc = None
        mk = dict(actor=meta['make_actor'], critic=meta['make_critic'], target_actor=meta['make_actor'], target_critic=meta['make_critic'])
        self.nets = {n: mk[n]().to(device=self.device, dtype=dtype) for n in NETS}

    def _cast(self, t):
        return t.detach().to(device=self.device, dtype=self.dtype)

    def _cast_state(self, st):
        out = {n: [self._cast(t) for t in st[n]] for n in NETS}
        for n in ('actor_opt', 'critic_opt'):
            out[n] = dict(exp_avg=[self._cast(t) for t in st[n]['exp_avg']], exp_avg_sq=[self._cast(t) for t in st[n]['exp_avg_sq']],
                          step=list(st[n]['step']))
        return out

    def _load(self, name, values):
        net = self.nets[name]
        with torch.no_grad():
            for p, v in zip(net.parameters(), values):
                p.copy_(v)
        return net

    def _first(self, out):
        return out[0] if self.meta['model'] else out

    def _sample(self, logits, u, sites, picks, shift):
        outs = []
        for x in _heads(logits):
            s, n = len(sites), x.shape[-1]
            nz = sampling_ref.noise(self.meta['seed'], SITES_PER_UPDATE * u + s + shift, x.numel() // n, n)
            nz = nz.to(device=self.device, dtype=self.dtype).view_as(x)
            v = x.detach() - nz                                                    # tau = 1
            soft = torch.softmax(x - nz, dim=-1)
            own = torch.from_numpy(np.argmax(v.cpu().numpy(), axis=-1)).to(self.device)          # the FIRST maximum
            pick = own if picks is None else picks[s].to(self.device).long().view_as(own)
            onehot = F.one_hot(pick, n).to(self.dtype)
            outs.append((onehot - soft.detach()) + soft)                           # the value of (onehot - soft) + soft, soft's gradient
            sites.append(dict(logits=x.detach().clone(), pick=pick, argmax=own, v=v))
        return torch.cat(outs, dim=-1)

    def _step(self, which, fed, mutate):
        """Clip, Adam and the Polyak update of ``which`` from the current state on the gradients ``fed`` -> the step's record."""
        st, lr = self.state, self.meta['lr']
        p0, opt, t0 = st[which], st[which + '_opt'], st['target_' + which]
        max_norm = None if mutate == 'clip coefficient omitted' else MAX_NORM
        stale = mutate == 'soft update from the pre-step parameters'
        if self.dtype == torch.float64:
            npy = lambda ts: [t.detach().cpu().numpy() for t in ts]  # noqa: E731
            ref = optim_ref.AdamF64(npy(p0), lr=lr, betas=BETAS, eps=EPS, max_norm=max_norm, targets=npy(t0), tau=TAU)
            ref.m, ref.v = [a.copy() for a in npy(opt['exp_avg'])], [a.copy() for a in npy(opt['exp_avg_sq'])]
            ref.steps = [int(s) for s in opt['step']]
            ref.step(npy(fed))
            back = lambda arrs: [torch.from_numpy(np.array(a)).to(self.device) for a in arrs]  # noqa: E731
            params, m, v, targets = back(ref.p), back(ref.m), back(ref.v), back(ref.t)
            if stale:
                targets = [optim_ref.soft_update_f64(t, p, TAU) for t, p in zip(t0, p0)]
            norm = torch.tensor(ref.total_norm, dtype=torch.float64)
        else:
            ps = [p.clone().requires_grad_() for p in p0]
            adam = torch.optim.Adam(ps, lr=lr, betas=BETAS, eps=EPS, foreach=False)
            for p, a, b, s, g in zip(ps, opt['exp_avg'], opt['exp_avg_sq'], opt['step'], fed):
                adam.state[p] = dict(step=torch.tensor(float(s)), exp_avg=a.clone(), exp_avg_sq=b.clone())
                p.grad = g.detach().clone()
            if max_norm is None:
                norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in ps]))
            else:
                norm = torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
            adam.step()
            with torch.no_grad():
                targets = [t.clone().mul_(1.0 - TAU).add_(q if stale else p, alpha=TAU) for t, p, q in zip(t0, ps, p0)]
            params = [p.detach() for p in ps]
            m, v = [adam.state[p]['exp_avg'] for p in ps], [adam.state[p]['exp_avg_sq'] for p in ps]
        st[which], st['target_' + which] = params, targets
        st[which + '_opt'] = dict(exp_avg=m, exp_avg_sq=v, step=[s + 1.0 for s in opt['step']])
        return dict(fed=_clone(fed), total_norm=norm.detach().clone(), params=_clone(params), exp_avg=_clone(m), exp_avg_sq=_clone(v),
                    targets=_clone(targets))

    def update(self, batch, u, staged=None, mutate=None):
        meta, st = self.meta, self.state
        pre = self._cast_state(st)
        old = self.prev if self.prev is not None else pre
        s0, a0, r, s1, d = (self._cast(torch.as_tensor(x)) for x in batch)
        picks = None if staged is None else [s['pick'] for s in staged['sites']]
        shift = 1 if mutate == 'noise of site + 1' else 0
        sites = []
        # (A)
        target_actor = self._load('target_actor', (old if mutate == 'stale target actor' else st)['target_actor'])
        target_critic = self._load('target_critic', (old if mutate == 'stale target critic' else st)['target_critic'])
        with torch.no_grad():
            logits_t = _heads(self._first(target_actor(s1)))
            q_next = self._first(target_critic(s1, self._sample(logits_t, u, sites, picks, shift)))
            rew = r.mean(dim=1, keepdim=True).expand_as(r) if mutate == 'y from the agent-mean reward' else r
            keep = 1.0 if mutate == '(1 - d) dropped' else (1.0 - d.unsqueeze(-1))
            y = rew.unsqueeze(-1) + GAMMA * keep * q_next
        # (B)
        actor, critic = self._load('actor', st['actor']), self._load('critic', st['critic'])
        l1 = meta['model'] and mutate != 'L1 term dropped'
        margins = []
        out = critic(s0, a0)
        loss_critic = F.smooth_l1_loss(self._first(out), y)
        if meta['model']:
            margins.append(float((out[1].detach().squeeze(-1) - r).abs().min()))
        if l1:
            loss_critic = loss_critic + F.l1_loss(out[1].squeeze(-1), r)
        for p in critic.parameters():
            p.grad = None
        loss_critic.backward()
        for p in critic.parameters():                                               # (a mutant may leave a head unused)
            p.grad = torch.zeros_like(p) if p.grad is None else p.grad
        critic_grads = [p.grad.detach().clone() for p in critic.parameters()]
        # (C)
        fed = critic_grads if staged is None else [self._cast(g) for g in staged['critic_step']['fed']]
        if mutate == 'accumulated gradients fed to the optimiser' and self.prev_acc is not None:
            fed = critic_grads = [g + a for g, a in zip(critic_grads, self.prev_acc)]   # what a recorder finds at step()
        pre_critic = st['critic']
        critic_step = self._step('critic', fed, mutate)
        if not meta.get('fused_optimizer', True) and mutate != 'clip coefficient omitted':
            with torch.no_grad():                                                   # clip_grad_norm_ has scaled .grad: (D) accumulates on that
                coef = torch.clamp(MAX_NORM / (critic_step['total_norm'].to(self.device) + 1e-6), max=1.0)
                for p in critic.parameters():
                    p.grad.mul_(coef.to(p.grad.dtype))
        # (D)
        if staged is not None:
            at = [self._cast(p) for p in staged['critic_step']['params']]
        else:
            at = pre_critic if mutate == 'actor pass on the pre-step critic' else st['critic']
        self._load('critic', at)
        if mutate == 'critic gradients cleared between the passes':
            for p in critic.parameters():
                p.grad = None
        out_a = actor(s0)
        q_actor = self._first(critic(s0, self._sample(self._first(out_a), u, sites, picks, shift)))
        loss_actor = -q_actor.mean()
        if meta['model']:
            margins.append(float((out_a[1].detach() - s1).abs().min()))
        if l1:
            loss_actor = loss_actor + F.l1_loss(out_a[1], s1)
        for p in actor.parameters():
            p.grad = None
        loss_actor.backward()
        actor_grads = [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in actor.parameters()]
        critic_acc = [torch.zeros_like(p) if p.grad is None else p.grad.detach().clone() for p in critic.parameters()]
        # (E)
        actor_step = self._step('actor', actor_grads if staged is None else [self._cast(g) for g in staged['actor_step']['fed']], mutate)
        self.prev, self.prev_acc = pre, critic_acc
        return dict(meta=dict(meta, update=u), pre=pre, batch=tuple(torch.as_tensor(x).detach().clone() for x in batch), sites=sites,
                    target_logits=[x.detach() for x in logits_t], q_next=q_next.detach(), y=y.detach(),
                    critic_out=[x.detach() for x in flat(out)], loss_critic=loss_critic.detach(), critic_grads=critic_grads,
                    critic_step=critic_step, actor_out=[x.detach() for x in flat(out_a)], q_actor=q_actor.detach(),
                    loss_actor=loss_actor.detach(), actor_grads=actor_grads, critic_acc=critic_acc, actor_step=actor_step,
                    post=self._cast_state(self.state), l1_margin=min(margins) if margins else None)


def restate(record, dtype, device):
    """One update recomputed from ``record`` (pre-update state, batch), staged on it -> a record of the same form."""
    meta = record['meta']
    return Restatement(meta, record['pre'], dtype, device).update(record['batch'], meta['update'], staged=record)


# ---- the named quantities of a record -----------------------------------------------------------------------------------------------
def named(rec):
    """{'<stage>.<quantity>': tensor}: everything the check compares, stages (A) to (E)."""
    names = rec['meta']['names']
    q = {'A.target_logits%d' % h: x for h, x in enumerate(rec['target_logits'])}
    q['A.q_next'], q['A.y'] = rec['q_next'], rec['y']
    q.update({'B.critic_out%d' % i: x for i, x in enumerate(rec['critic_out'])})
    q['B.loss_critic'] = rec['loss_critic']
    q.update({'B.grad.' + n: g for n, g in zip(names['critic'], rec['critic_grads'])})
    q.update({'D.actor_out%d' % i: x for i, x in enumerate(rec['actor_out'])})
    q['D.q'], q['D.loss_actor'] = rec['q_actor'], rec['loss_actor']
    q.update({'D.grad.' + n: g for n, g in zip(names['actor'], rec['actor_grads'])})
    q.update({'D.critic_grad.' + n: g for n, g in zip(names['critic'], rec['critic_acc'])})
    for stage, net in (('C', 'critic'), ('E', 'actor')):
        step = rec[net + '_step']
        q[stage + '.total_norm'] = step['total_norm']
        for kind, key in (('param', 'params'), ('exp_avg', 'exp_avg'), ('exp_avg_sq', 'exp_avg_sq'), ('target', 'targets')):
            q.update({'%s.%s.%s' % (stage, kind, n): t for n, t in zip(names[net], step[key])})
    return q


# ---- the recorder -------------------------------------------------------------------------------------------------------------------
class Recorder(object):
    """Installed on one eager learner: every ``optimize()`` appends a record to ``records``."""

    def __init__(self, trainer, meta):
        self.fused = bool(trainer.fused_optimizer)
        self.t, self.meta, self.records, self.cur = trainer, dict(meta, fused_optimizer=self.fused), [], None
        self._last_grad = {}
        t = trainer
        inner_tensors, inner_sample, inner_index = t.optimize_tensors, t._sample, t.memory.sample_index

        def sample_index(idx):
            out = inner_index(idx)
            self.cur['batch'] = tuple(torch.as_tensor(x).detach().clone() for x in out)
            return out

        def sample(logits):
            y = inner_sample(logits)
            at = 0
            for x in _heads(logits):
                part = y.detach()[..., at:at + x.shape[-1]]
                at += x.shape[-1]
                hot = part > 0.5                                                    # the pick: the entry above 0.5
                self.cur['one_hot'] = self.cur['one_hot'] and bool((hot.sum(-1) == 1).all())
                self.cur['sites'].append(dict(logits=x.detach().clone(), pick=hot.float().argmax(-1)))
            return y

        def optimize_tensors():
            self.cur = dict(meta=dict(self.meta, update=len(self.records)), pre=learner_state(t), sites=[], one_hot=True, q_next=[],
                            critic_calls=[], actor_calls=[])
            loss_actor, loss_critic = inner_tensors()
            self._finish(loss_actor, loss_critic)
            return loss_actor, loss_critic
        t.memory.sample_index, t._sample, t.optimize_tensors = sample_index, sample, optimize_tensors
        keep = lambda name: (lambda out: self.cur[name].append([x.detach().clone() for x in flat(out)]))  # noqa: E731
        target = t.target_critic
        if 'forward' in vars(target):                                               # _FusedTarget keeps its forward in its __dict__
            inner_forward = vars(target)['forward']

            def forward(*a, **k):
                out = inner_forward(*a, **k)
                keep('q_next')(out)
                return out
            vars(target)['forward'] = forward
        else:
            target.register_forward_hook(lambda m, i, out: keep('q_next')(out))
        t.critic.register_forward_hook(lambda m, i, out: keep('critic_calls')(out))
        t.actor.register_forward_hook(lambda m, i, out: keep('actor_calls')(out))
        for net in ('critic', 'actor'):
            self._wrap_step(net)

    def _wrap_step(self, net):
        t = self.t
        opt, ps = getattr(t, net + '_optimizer'), list(getattr(t, net).parameters())
        inner = opt.step
        if not self.fused:
            for p in ps:
                p.register_post_accumulate_grad_hook(lambda p: self._last_grad.__setitem__(p, p.grad.detach().clone()))

        def step(*a, **k):
            if self.fused:
                fed = [p.grad.detach().clone() for p in ps]                         # as autograd left them: FusedAdam does not write .grad
            else:
                fed = [self._last_grad[p] for p in ps]
            out = inner(*a, **k)
            if self.fused:
                norm = opt.last_total_norm.detach().clone()
            else:
                norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in fed]))
            self.cur[net + '_step'] = dict(fed=fed, total_norm=norm, params=_clone(ps),
                                           exp_avg=[opt.state[p]['exp_avg'].detach().clone() for p in ps],
                                           exp_avg_sq=[opt.state[p]['exp_avg_sq'].detach().clone() for p in ps],
                                           targets=_clone(getattr(t, 'target_' + net).parameters()))
            return out
        opt.step = step

    def _finish(self, loss_actor, loss_critic):
        t, c = self.t, self.cur
        first = lambda outs: outs[0]  # noqa: E731  (flat: the first tensor of a pair is the pair's first value)
        heads = len(c['sites']) // 2
        assert len(c['sites']) == 2 * heads and len(c['q_next']) == 1 and len(c['critic_calls']) == 2 and len(c['actor_calls']) == 1
        c['post'] = learner_state(t)
        if not self.fused:                                                          # the stock soft updates run after both steps
            for net in ('critic', 'actor'):
                c[net + '_step']['targets'] = _clone(c['post']['target_' + net])
        q_next = first(c['q_next'][0])
        r, d = (torch.as_tensor(x, dtype=torch.float32, device=q_next.device) for x in (c['batch'][2], c['batch'][4]))
        c['target_logits'] = [s['logits'] for s in c['sites'][:heads]]
        c['q_next'], c['y'] = q_next, r.unsqueeze(-1) + GAMMA * (1.0 - d.unsqueeze(-1)) * q_next
        c['critic_out'], c['q_actor'] = c['critic_calls'][0], first(c['critic_calls'][1])
        c['actor_out'] = c['actor_calls'][0]
        c['loss_critic'], c['loss_actor'] = loss_critic.detach().clone(), loss_actor.detach().clone()
        c['critic_grads'], c['actor_grads'] = c['critic_step']['fed'], c['actor_step']['fed']
        c['critic_acc'] = [p.grad.detach().clone() for p in t.critic.parameters()]
        self.records.append(c)
        self.cur = None


# ---- what the CPU tests put around a learner or a restatement -----------------------------------------------------------------------
class StockSampler(object):
    """A learner's ``_sample`` on the CPU: ``sampling_ref.stock`` (F.gumbel_softmax's own lines) on the noise of ``GumbelSampler``'s
    numbering; ``end_update()`` after every ``optimize()``."""

    def __init__(self, seed):
        self.seed, self.update, self.site = int(seed), 0, 0

    def __call__(self, logits):
        outs = []
        for x in _heads(logits):
            n = x.shape[-1]
            nz = sampling_ref.noise(self.seed, SITES_PER_UPDATE * self.update + self.site, x.numel() // n, n).to(x.dtype).view_as(x)
            outs.append(sampling_ref.stock(x, nz, 1.0, True))
            self.site += 1
        return torch.cat(outs, dim=-1)

    def end_update(self):
        self.update, self.site = self.update + 1, 0


class HostRing(object):
    """A ring of the variant's tuple without a device: every ``sample_index`` returns a fresh batch of float32 tensors (one-hot
    actions, one in ten transitions done)."""
    device_index = True

    def __init__(self, variant, seed=2):
        import tests.test_gpu_update_graph as ug
        _, _, _, kw, self.N, self.D = ug.VARIANTS[variant]
        self.heads, self.per_agent = kw.get('act_heads', (5,)), bool(kw.get('per_agent'))
        self.g = torch.Generator().manual_seed(seed)

    def __len__(self):
        return 200

    def make_index(self, b):
        return torch.arange(b)

    def sample_index(self, idx):
        b, g = len(idx), self.g
        act = torch.cat([torch.eye(h)[torch.randint(0, h, (b, self.N), generator=g)] for h in self.heads], dim=-1)
        rd = (b, self.N) if self.per_agent else (b,)
        return (torch.randn(b, self.N, self.D, generator=g), act, torch.randn(rd, generator=g), torch.randn(b, self.N, self.D, generator=g),
                (torch.rand(rd, generator=g) < 0.1).float())


def initial_state(meta, seed):
    """A learner's state before its first update: fresh networks, targets equal to them, Adam's zeros."""
    torch.manual_seed(seed)
    actor, critic = _clone(meta['make_actor']().parameters()), _clone(meta['make_critic']().parameters())
    zeros = lambda ps: dict(exp_avg=[torch.zeros_like(p) for p in ps], exp_avg_sq=[torch.zeros_like(p) for p in ps], step=[0.0] * len(ps))  # noqa: E731
    return dict(actor=actor, critic=critic, target_actor=_clone(actor), target_critic=_clone(critic), actor_opt=zeros(actor),
                critic_opt=zeros(critic))


# ---- the check ----------------------------------------------------------------------------------------------------------------------
def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def _err(a, b):
    return float((_f64(a) - _f64(b)).abs().max())


def check_picks(rec, ref):
    """-> (failures, rows left out, rows): the learner's pick against the float64 argmax wherever the float64 margin is at least 2 e."""
    fails, left, rows = [], 0, 0
    for s, (got, want) in enumerate(zip(rec['sites'], ref['sites'])):
        e = _err(got['logits'], want['logits'])
        top = torch.topk(_f64(want['v']), min(2, want['v'].shape[-1]), dim=-1).values
        margin = (top[..., 0] - top[..., -1]) if top.shape[-1] == 2 else torch.full(top.shape[:-1], float('inf'), dtype=torch.float64)
        clear = margin >= 2 * e
        pick, arg = got['pick'].cpu().long().view_as(clear), want['argmax'].cpu().long().view_as(clear)
        wrong = int((clear & (pick != arg)).sum())
        out = int((~clear).sum())
        left, rows = left + out, rows + clear.numel()
        if wrong:
            fails.append('pick.site%d: %d of %d clear rows differ from the float64 argmax (e %.3e)' % (s, wrong, int(clear.sum()), e))
        if out > LEFT_OUT * clear.numel():
            fails.append('pick.site%d: %d of %d rows under the margin 2 e = %.3e: the check is vacuous' % (s, out, clear.numel(), 2 * e))
    return fails, left, rows


def check_case(tag, records, device, report=print):
    """Every record of one learner (one variant, one batch size) against ``restate`` in float64 on the CPU and in float32 on
    ``device``.  Bound: |learner - float64| <= 4 x max(|stock float32 - float64|, one float32 rounding of the reference's largest
    entry); for the two losses and tensors under 64 elements the stock error is the largest over the case's updates (one scalar's
    error is a single draw); total_norm within 2e-6 relative.  -> (failures, worst ratio per stage); ``report`` gets one line per
    update and stage."""
    got = [named(rec) for rec in records]
    refs = [restate(rec, torch.float64, 'cpu') for rec in records]
    ref = [named(x) for x in refs]
    stock = [named(restate(rec, torch.float32, device)) for rec in records]
    assert all(set(g) == set(r) == set(s) for g, r, s in zip(got, ref, stock))
    e_stock = [{n: _err(s[n], r[n]) for n in r} for s, r in zip(stock, ref)]
    small = {n for n in ref[0] if ref[0][n].numel() < SMALL or n in ('B.loss_critic', 'D.loss_actor')}
    over_updates = {n: max(e[n] for e in e_stock) for n in small}
    fails, worst_ratio = [], {}
    for u, rec in enumerate(records):
        if not rec.get('one_hot', True):
            fails.append('update %d: a hard sample without exactly one entry above 0.5 in a row' % u)
        if refs[u]['l1_margin'] is not None and refs[u]['l1_margin'] < L1_MARGIN:
            fails.append('update %d: precondition: an L1 term within %.1e of its kink (%.3e)' % (u, L1_MARGIN, refs[u]['l1_margin']))
        pick_fails, left, rows = check_picks(rec, refs[u])
        fails += ['update %d: %s' % (u, f) for f in pick_fails]
        stages = {}
        for n, r in ref[u].items():
            if not bool(torch.isfinite(_f64(got[u][n])).all()):
                fails.append('update %d: %s is not finite' % (u, n))
                continue
            e_k, scale = _err(got[u][n], r), float(_f64(r).abs().max())
            if n.endswith('.total_norm'):
                e_s, ratio = _err(stock[u][n], r), e_k / max(NORM_REL * scale, 1e-300) * BOUND      # on the scale of the bound 4
            else:
                e_s = over_updates[n] if n in small else e_stock[u][n]
                ratio = e_k / max(e_s, 2.0 ** -23 * scale, 1e-300)
            if ratio > BOUND:
                fails.append('update %d: %s: learner %.3e stock %.3e against float64 (largest entry %.3e): ratio %.2f' % (u, n, e_k, e_s, scale, ratio))
            if ratio >= stages.get(n[0], (-1.0,))[0]:
                stages[n[0]] = (ratio, n, e_k, e_s)
        for stage in sorted(stages):
            ratio, n, e_k, e_s = stages[stage]
            worst_ratio[stage] = max(worst_ratio.get(stage, 0.0), ratio)
            report('%-28s update %d stage %s: worst %-38s learner %.3e  stock %.3e  ratio %.2f | pick rows left out %d of %d' % (
                tag, u, stage, n, e_k, e_s, ratio, left, rows))
    if refs[0]['l1_margin'] is not None:
        report('%-28s least |prediction - target| under an L1 term over the updates (float64): %.3e' % (tag, min(x['l1_margin'] for x in refs)))
    return fails, worst_ratio
