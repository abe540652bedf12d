#!/usr/bin/env python3
"""Entry script of the batched engine -- the counterpart of the reference's ``main.py:29-67``.

    python examples/train_batched.py --scenario simple_spread --envs 4096 --episodes 40960
    python examples/train_batched.py --scenario simple_spread --agents 3 --full-observation --envs 256 --episodes 512
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/train_batched.py --envs 4096
    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 examples/train_batched.py --backend gloo   (one GPU)

For every scenario and seed count ``cnt`` it does what main.py does -- build the env (``make_batched_env``: the reference's
``make_env`` contract, B worlds), seed protocol ``seed = cnt + 12345678`` (main.py:41-49), read the dims from the env
(:51-58), build ``ActorNetwork`` / ``CriticNetwork`` (:60-61), hand everything to the rollout-and-learn loop (:65-67) -- with
``multiagent_rl_amd.train.train_batched`` in the place of ``experiments.run.run``.  ``--reference`` takes the Trainer and the
critic from the reference checkout on ``sys.path`` (``rls.agent.multiagent.ddpg_gumbel_fix``); otherwise the small stock-PyTorch
learner of ``examples/madr_learner.py`` stands in (the learner is not part of this repo's scope).  ``--critic attention`` gives
it the reference's critic architecture (``multiagent_rl_amd.critic.CriticNetwork``); ``--critic bicnet`` is the BiCNet baseline: per-agent
transitions (``train_batched(per_agent_transition=True)``), ``multiagent_rl_amd.critic.BiCNetCritic`` and the per-agent stand-in learner
(with ``--reference``: ``BIC_gumbel_fix.Trainer`` and ``ac_network_multi_gumbel_BIC``), any number of ranks -- where the other critics get a
STATE ring (simple_spread with the local observation, simple_tag; not ``--policy-form 5``) a single rank builds the per-agent STATE ring itself
and passes it as ``memory=``, the row ring otherwise or under ``--ring rows`` (the batches are bit-identical); with several ranks the ring is the
gather's (``FullTransitionGather(per_agent=True)``: per-agent wire blocks, the same choice of ring); ``--critic model`` is the
paper's own method, the model-learning variant: ``ModelActorNetwork`` / ``ModelCriticNetwork`` and ``madr_learner.ModelTrainer`` (with
``--reference``: ``model_ddpg_gumbel_fix.Trainer`` and ``ac_network_model_multi_gumbel``) on the shared-reward ring, any number of ranks.  ``--fused-targets`` runs its target networks'
forwards on the HIP kernels (``accelerate_trainer(trainer, targets=True)``), ``--fused-optimizer`` runs each network's clip + Adam +
soft update as one launch (``multiagent_rl_amd.optim``: the learner's own switch, or ``accelerate_trainer(.., optimizer=True)`` with
``--reference``), ``--fused-lstm`` runs the recurrence of the learner's LSTMs with gradient on the HIP kernels
(``multiagent_rl_amd.lstm``: the learner's own ``fused_lstm`` switch, or ``accelerate_trainer(.., lstm=True)`` with ``--reference``),
``--fused-attention`` runs the attention critic's attention block with gradient on the HIP kernels (``multiagent_rl_amd.attention``: the
learner's own ``fused_attention`` switch, or ``accelerate_trainer(.., attention=True)`` with ``--reference``),
``--fused-sampling`` runs the learner's Gumbel-softmax samples with gradient on the HIP kernels, with the library's own noise stream
(``multiagent_rl_amd.sampling``: the learner's own ``fused_sampling`` switch, or ``accelerate_trainer(.., sampling=True)`` with ``--reference``),
``--fused-front`` runs dense1, the ReLU and the LSTM's input projection of the learner's networks with gradient on the HIP kernels
(``multiagent_rl_amd.dense``: the learner's own ``fused_front`` switch, or ``accelerate_trainer(.., front=True)`` with ``--reference``; needs ``--fused-lstm``),
``--fused-wgrad`` takes the ``W_hh`` gradients of the fused LSTMs from the HIP kernels as well (``multiagent_rl_amd.lstm.launch_wgrad``:
the learner's own ``fused_wgrad`` switch, or ``accelerate_trainer(.., wgrad=True)`` with ``--reference``; needs ``--fused-lstm``),
``--fused-heads`` runs the ReLU on the actor's BiLSTM output and every output layer of the learner's networks with gradient on the HIP
kernels (``multiagent_rl_amd.heads``: the learner's own ``fused_heads`` switch, or ``accelerate_trainer(.., heads=True)`` with
``--reference``; needs ``--fused-front``).
``--ledger device`` takes the per-episode history from the HIP episode log (``train.EpisodeLog``: one launch per chunk; several ranks are
merged in time order) instead of the torch pipeline of ``ChunkLedger`` (``--ledger host``, the default).  ``--test-only`` is the
experiment's test phase (``run_test``, run.py:106-200) on the batched engine: ``train.evaluate_batched`` loads the
``<scenario>_fin_<cnt>`` models a training run saved (``Models/`` under the working directory, the default ``--out-dir``), plays ``--episodes`` episodes without updating anything and
writes ``test_history_<scenario>_<cnt>.pkl`` to ``--out-dir``; it needs none of the learner switches.
With several ranks (torchrun) every rank rolls out its shard of the env batch (``env_id_base = rank * envs``) and the
transitions of all ranks reach rank 0's ring through the RCCL full gather; rank 0 learns and broadcasts the actor.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenario', action='append', help='simple_spread | simple_tag | simple_reference (repeatable)')
    ap.add_argument('--envs', type=int, default=4096, help='B per GPU')
    ap.add_argument('--agents', type=int, default=None, help='simple_spread: make_world(num_agents=n), scenarios.py:170')
    ap.add_argument('--full-observation', action='store_true',
                    help="simple_spread: upstream MPE's own observation (make_env(local_observation=False), scenarios.py:124); the rollout "
                         'runs on the generic one-launch kernel and the ring keeps rows')
    ap.add_argument('--policy-form', type=int, default=0,
                    help='pw_dispatch.policy_form of the rollout: 0 automatic, 3 / 4 the simple_spread forms, 5 the generic form')
    ap.add_argument('--ring', default='auto', choices=['auto', 'rows', 'state'],
                    help='the replay ring: state = {vel, pos} + landmarks per transition, rows rebuilt when a batch is sampled (bit-identical '
                         'batches, a third of the bytes; simple_spread with the local observation and simple_tag on the specialised rollout '
                         'forms); rows = the observation rows themselves; auto = state wherever it is served')
    ap.add_argument('--episodes', type=int, default=None, help='arglist.num_episodes (finished episodes over all envs of a rank)')
    ap.add_argument('--seeds', type=int, default=1, help='cnt in range(seeds), main.py:37')
    ap.add_argument('--chunk', type=int, default=100, help='batched env steps per launch')
    ap.add_argument('--max-updates-per-chunk', type=int, default=8)
    ap.add_argument('--save-rate', type=int, default=None)
    ap.add_argument('--out-dir', default='Models')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'],
                    help='process group of a multi-rank run: nccl (= RCCL, one GPU per rank) or gloo (the blocks of the full gather '
                         'travel through pinned host buffers; ranks may share a GPU -- RCCL refuses that)')
    ap.add_argument('--reference', action='store_true', help="use the reference's Trainer / CriticNetwork (rls on sys.path)")
    ap.add_argument('--critic', default='standin', choices=['standin', 'attention', 'bicnet', 'model'],
                    help="standin: madr_learner's mean-pooling critic; attention: multiagent_rl_amd.critic.CriticNetwork, the "
                         "reference's LSTM + attention architecture (its saved *_critic.pt files load into it); bicnet: the BiCNet "
                         'baseline -- one Q per agent (multiagent_rl_amd.critic.BiCNetCritic) and per-agent transitions; model: the '
                         'model-learning variant -- ModelActorNetwork / ModelCriticNetwork (an actor that also predicts the next '
                         'observation, an attention critic that also predicts the reward) and the learner with the two L1 model losses')
    ap.add_argument('--fused-targets', action='store_true',
                    help='target actor and target critic of the learner run on the HIP kernels (accelerate_trainer(.., targets=True); '
                         'needs the attention, the bicnet or the model critic)')
    ap.add_argument('--fused-optimizer', action='store_true',
                    help="each network's gradient clip + Adam step + soft update is one HIP launch (madr_learner's fused_optimizer "
                         'switch; with --reference: accelerate_trainer(.., optimizer=True))')
    ap.add_argument('--fused-lstm', action='store_true',
                    help="the learner's LSTMs run their recurrence, forward and backward, on the HIP kernels (madr_learner's fused_lstm "
                         'switch; with --reference: accelerate_trainer(.., lstm=True)); off by default: losses differ from '
                         "MIOpen's in the last bits")
    ap.add_argument('--fused-attention', action='store_true',
                    help="the attention block of the learner's critic runs, forward and backward, on the HIP kernels (madr_learner's "
                         'fused_attention switch; with --reference: accelerate_trainer(.., attention=True)); needs the attention or '
                         'the model critic; off by default: losses differ from the stock expression in the last bits')
    ap.add_argument('--graph-update', action='store_true',
                    help="the learner's whole update is captured once and replayed as one graph launch per update "
                         '(multiagent_rl_amd.graph.GraphedUpdate); needs --fused-targets --fused-optimizer --fused-lstm --fused-attention '
                         '(--critic bicnet, which has no attention block: the first three); the ring draws its batches from device cells')
    ap.add_argument('--fused-sampling', action='store_true',
                    help="the learner's Gumbel-softmax samples run, forward and backward, on the HIP kernels (madr_learner's "
                         'fused_sampling switch; with --reference: accelerate_trainer(.., sampling=True)); off by default: the noise is '
                         "the library's Philox stream keyed (seed; update, call site, row), not torch's generator")
    ap.add_argument('--fused-front', action='store_true',
                    help="dense1, the ReLU and the LSTM's input projection of the learner's networks run, forward and backward, on the HIP "
                         "kernels (madr_learner's fused_front switch; with --reference: accelerate_trainer(.., front=True)); needs "
                         '--fused-lstm; off by default: the sums run in another order than the stock GEMMs')
    ap.add_argument('--fused-wgrad', action='store_true',
                    help="the W_hh gradients of the learner's fused LSTMs come from the HIP kernels, two per LSTM backward, instead of two "
                         "strided copies and a GEMM per direction (madr_learner's fused_wgrad switch; with --reference: "
                         'accelerate_trainer(.., wgrad=True)); needs --fused-lstm; off by default: the sums run in another order than '
                         'the stock GEMMs')
    ap.add_argument('--fused-heads', action='store_true',
                    help="the ReLU on the actor's BiLSTM output and every output layer of the learner's networks run, forward and "
                         "backward, on the HIP kernels (madr_learner's fused_heads switch; with --reference: "
                         'accelerate_trainer(.., heads=True)); needs --fused-front; off by default: the sums run in another order than '
                         'the stock GEMMs')
    ap.add_argument('--ledger', default='host', choices=['host', 'device'],
                    help='who makes the per-episode history: host = ChunkLedger (a torch pipeline per chunk), device = EpisodeLog (one HIP '
                         'launch per chunk, float64 sums in a fixed order; several ranks merge in time order)')
    ap.add_argument('--test-only', action='store_true',
                    help="the test phase: load the <scenario>_fin_<cnt> models a training run saved (Models/), play --episodes episodes in launches of "
                         'max_episode_len steps without any update and write test_history_<scenario>_<cnt>.pkl there')
    args = ap.parse_args(argv)
    if args.fused_heads and not args.fused_front:
        ap.error('--fused-heads needs --fused-front: the fused output layers are the last lines of the swapped forwards')
    if args.fused_front and not args.fused_lstm:
        ap.error('--fused-front needs --fused-lstm: the fused front feeds the fused recurrence')
    if args.fused_wgrad and not args.fused_lstm:
        ap.error('--fused-wgrad needs --fused-lstm: the W_hh gradients of a plain nn.LSTM are not the kernels\' to form')
    if args.graph_update:
        need = ['--fused-targets', '--fused-optimizer', '--fused-lstm'] + ([] if args.critic == 'bicnet' else ['--fused-attention'])
        lacking = [f for f in need if not getattr(args, f[2:].replace('-', '_'))]
        if lacking:
            ap.error('--graph-update needs %s: a captured update holds no vendor RNN call and no stock optimiser (missing: %s)'
                     % (' '.join(need), ' '.join(lacking)))
    if args.fused_attention and args.critic not in ('attention', 'model') and not args.reference:
        ap.error('--fused-attention needs --critic attention or --critic model (the block exists in the LSTM + attention critics only)')
    if args.fused_targets and args.critic not in ('attention', 'bicnet', 'model') and not args.reference:
        ap.error('--fused-targets needs --critic attention, bicnet or model (the HIP critics are the LSTM architectures)')
    bicnet, model = args.critic == 'bicnet', args.critic == 'model'

    os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')   # dmabuf IPC for multi-process GPU work (read at the first GPU call)
    import torch
    import torch.distributed as dist
    from multiagent_rl_amd import arglist, make_batched_env
    from multiagent_rl_amd.policy import ActorNetwork
    from multiagent_rl_amd.train import dims_from_env, evaluate_batched, seed_everything, train_batched
    if args.reference and model:
        from rls.agent.multiagent.model_ddpg_gumbel_fix import Trainer
        from rls.model.ac_network_model_multi_gumbel import ActorNetwork, CriticNetwork
    elif model:
        from madr_learner import ModelTrainer as Trainer
        from multiagent_rl_amd.critic import ModelCriticNetwork as CriticNetwork
        from multiagent_rl_amd.policy import ModelActorNetwork as ActorNetwork
    elif args.reference and bicnet:
        from rls.agent.multiagent.BIC_gumbel_fix import Trainer
        from rls.model.ac_network_multi_gumbel_BIC import CriticNetwork
    elif args.reference:
        from rls.agent.multiagent.ddpg_gumbel_fix import Trainer
        from rls.model.ac_network_multi_gumbel import CriticNetwork
    elif bicnet:
        from madr_learner import BiCNetTrainer as Trainer
        from multiagent_rl_amd.critic import BiCNetCritic as CriticNetwork
    else:
        from madr_learner import CriticNetwork, Trainer
        if args.critic == 'attention':
            from multiagent_rl_amd.critic import CriticNetwork
    if args.fused_targets or args.fused_optimizer or args.fused_lstm or args.fused_attention or args.fused_sampling or args.fused_front:
        from multiagent_rl_amd.policy import accelerate_trainer
        plain_trainer = Trainer

        def Trainer(*a, **k):   # train_batched builds the learner itself: patch the instance it gets
            if args.fused_optimizer and not args.reference:
                k['fused_optimizer'] = True
            if args.fused_lstm and not args.reference:
                k['fused_lstm'] = True
            if args.fused_attention and not args.reference:
                k['fused_attention'] = True
            if args.fused_sampling and not args.reference:
                k['fused_sampling'] = True
            if args.fused_front and not args.reference:
                k['fused_front'] = True
            if args.fused_wgrad and not args.reference:
                k['fused_wgrad'] = True
            if args.fused_heads and not args.reference:
                k['fused_heads'] = True
            if args.graph_update and not args.reference:
                k['graph_update'] = True     # madr_learner installs the fused targets and the graphed update itself
                return plain_trainer(*a, **k)
            learner = plain_trainer(*a, **k)
            if args.fused_targets or args.reference:
                accelerate_trainer(learner, targets=args.fused_targets, optimizer=args.fused_optimizer and args.reference,
                                   lstm=args.fused_lstm and args.reference, attention=args.fused_attention and args.reference,
                                   graph=args.graph_update, sampling=args.fused_sampling and args.reference,
                                   front=args.fused_front and args.reference, wgrad=args.fused_wgrad and args.reference,
                                   heads=args.fused_heads and args.reference)
            return learner

    rank, world = int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if args.backend == 'gloo':
        local_rank %= max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29541')
        if args.backend == 'gloo':
            dist.init_process_group('gloo', rank=rank, world_size=world)
        else:
            dist.init_process_group('nccl', rank=rank, world_size=world, device_id=dev)

    if args.episodes is not None:
        arglist.num_episodes = args.episodes
    if args.save_rate is not None:
        arglist.save_rate = args.save_rate
    results = []
    for scenario_name in (args.scenario or ['simple_spread']):
        for cnt in range(args.seeds):
            seed = seed_everything(cnt + 12345678)                             # main.py:41-49
            kw = dict(n=args.agents) if scenario_name == 'simple_spread' and args.agents else {}
            if scenario_name == 'simple_tag':
                kw = dict(num_adversaries=3, num_good=1) if args.agents is None else dict(num_adversaries=args.agents - 2, num_good=2)
            if args.full_observation:
                kw['local_observation'] = False
            env = make_batched_env(scenario_name, args.envs, auto_reset=True, max_episode_len=arglist.max_episode_len,
                                   seed=seed, env_id_base=rank * args.envs, **kw)
            if args.policy_form:
                env.set_dispatch(policy_form=args.policy_form)
            # a STATE ring holds {vel, pos} + landmarks: enough for the local observation and simple_tag on the specialised rollout forms only
            state_ok = scenario_name in ('simple_spread', 'simple_tag') and not args.full_observation and args.policy_form != 5
            if args.ring == 'state' and not state_ok:
                ap.error('--ring state serves simple_spread with the local observation and simple_tag on the specialised rollout forms '
                         '(not --full-observation, not --policy-form 5)')
            state_ok = state_ok and args.ring != 'rows'
            memory = None
            if bicnet and state_ok and world == 1:
                # the per-agent STATE ring: train_batched(per_agent_transition=True) builds the row ring only, this one comes in as memory=
                from multiagent_rl_amd.replay_buffer import ReplayBuffer
                memory = ReplayBuffer(int(1e6), env.n, env.obs_dim, per_agent=True, device_index='counter' if args.graph_update else True,
                                      state_ring=dict(scenario=scenario_name, num_landmarks=env.num_landmarks,
                                                      num_adversaries=env.cfg.num_adversaries if scenario_name == 'simple_tag' else 0))
            dim_obs, dim_action, action_type = dims_from_env(env)             # main.py:51-58
            actor = ActorNetwork(input_dim=dim_obs, out_dim=dim_action)       # main.py:60-61
            n_act = sum(dim_action) if isinstance(dim_action, list) else dim_action
            critic = CriticNetwork(input_dim=dim_obs + n_act, out_dim=1)
            if args.test_only:
                # load_models reads <scenario>_fin_<cnt>_actor.pt / _critic.pt where save_models wrote them (Models/ under the working
                # directory, the reference's place): model_prefix='' -- not arglist.appx -- names what the training run above saved
                hist = evaluate_batched(env, actor, critic, Trainer, scenario_name, action_type, cnt=cnt, out_dir=args.out_dir,
                                        model_prefix='', rank=rank, world=world, log=print if rank == 0 else (lambda *a: None))
                results.append((scenario_name, cnt, hist['stats']))
                continue
            gather = None
            if world > 1:
                from multiagent_rl_amd.dist import FullTransitionGather, broadcast_actor
                actor = actor.to(dev)
                broadcast_actor(actor, src=0)                                  # same initial weights on every rank
                # state-only blocks (simple_spread, simple_tag) land in a STATE ring on the learner rank (rows rebuilt when a batch is
                # sampled: a third of the ring writes); simple_reference travels on compact-row blocks into its two-head row ring;
                # --critic bicnet: per-agent wire blocks into the per-agent ring of the same kind
                state_ring = state_ok
                gather = FullTransitionGather(env, args.chunk, rank, world, dev, ring='state' if state_ring else 'rows', per_agent=bicnet)
                gather.prime()
            hist = train_batched(env, actor, critic, Trainer, scenario_name, action_type, cnt=cnt, out_dir=args.out_dir,
                                 chunk=args.chunk, max_updates_per_chunk=args.max_updates_per_chunk, gather=gather,
                                 ring='state' if (gather is None and state_ok and not bicnet) else 'rows', memory=memory,
                                 rank=rank, world=world, log=print if rank == 0 else (lambda *a: None), per_agent_transition=bicnet,
                                 graph_update=args.graph_update, ledger=args.ledger)
            results.append((scenario_name, cnt, hist['stats']))
            if rank == 0:
                s = hist['stats']
                print('%s cnt=%d: %d env-steps, %d episodes, mean episode reward %.3f, %d updates, %.1f s (%.3g env-steps/s)'
                      % (scenario_name, cnt, s['env_steps'], s['episodes'], s['mean_episode_reward'], s['updates'], s['wall_s'],
                         s['env_steps'] * world / s['wall_s']))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return results


if __name__ == '__main__':
    main()
