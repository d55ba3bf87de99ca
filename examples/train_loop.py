#!/usr/bin/env python3
"""The reference's training loop (train_problem.py:82-115) on the device: per episode, a rollout window of T steps into an
on-device `RolloutStorage` (batched softmax-16 policy, one env launch per step), then ONE `SA2CLearner.train` -- the
batched `SA2CAgents.train_NN` (SAC_agents.py:280-357): critic MSE + clip + Adam, baseline from the post-update critic,
actor loss + clip + Adam, for all N agents' networks at once in HIP.

    python examples/train_loop.py [--envs 256] [--agents 5] [--episodes 5] [--learner {sa2c,ppo}] [--epochs 10]
                                  [--lam X] [--window T] [--time-limit {terminal,bootstrap}] [--ent-coef X]
                                  [--normalize-advantage] [--minibatches K] [--shuffle-seed S] [--target-kl X] [--vf-clip X]
                                  [--obs-norm] [--obs-clip X] [--share all] [--grid G] [--reward-norm] [--reward-clip X]
                                  [--shield] [--shield-rate X] [--shield-margin X] [--obstacles N] [--per-env-obstacles]

``--learner ppo`` trains with `PPOLearner` instead -- the batched `SPPOAgents.train` (SAC_agents.py:410-573): the window is
used for ``--epochs`` critic-and-actor steps with the clipped probability ratio (train_problem.py:43, ``M = 10``).

``--lam X`` (off by default) switches either learner to bootstrapped lambda-returns, TD(lambda) / GAE: the envs reset
themselves, so a window cuts the episodes that started inside it, and without a bootstrap from the value of the observation
after the window's last step their returns are truncated.  With it a window may be shorter than an episode (``--window T``).

``--time-limit bootstrap`` (needs ``--lam``) treats an episode that ran into the time limit as truncated, not finished: its
return bootstraps from the critic's value of its terminal observation.  After the loop the share of truncated among the last
window's finished episodes is printed (an untrained policy: nearly all of them).

``--ent-coef X`` adds an entropy bonus to the actor loss (-X x the mean entropy of the policy over the window's rows), and
``--normalize-advantage`` (``--learner ppo``) standardises each agent's advantages over the window before the epochs; with
either, every episode line also shows the mean entropy.

``--minibatches K`` (``--learner ppo``; K must divide window x envs) reshuffles the window's rows on the device every epoch and
takes one critic and one actor step per minibatch: K x ``--epochs`` Adam steps per network per window instead of ``--epochs``.
``--shuffle-seed S`` keys the permutations; the diagnostics shown are then the last epoch's, averaged over its minibatches.

``--target-kl X`` (``--learner ppo``) stops an agent's actor for the rest of the window once its KL estimate to the policy that
collected the window passes X -- decided and obeyed on the device, per agent; the critics keep stepping.  The episode line then
shows the actors' step counts of the window (min / mean / max over the agents), and its means skip the NaN a skipped step
reports.  ``--vf-clip X`` (``--learner ppo``) clips the value loss against the window's pre-update values; the line shows the
share of rows it clipped in the last step.

``--obs-norm`` gives the policy, the critic and the learner an `ObsNormalizer`: running per-(agent, input column) statistics on
the device.  The rollout feeds the networks ``norm(env.z)``, ``train()`` normalises the window with the same table and merges the
window into the statistics as its last work.  One warm-up window of `update` only runs before the first ``train``, so that
window 0 is not trained on the identity map.  Every episode line then shows the largest ``|mean|`` and the range of the
columns' standard deviations.  ``--obs-clip X`` clamps the normalised observation to [-X, X] (default 10).

``--grid G`` sets the side length of the square the goals lie in (default 5, the reference's).  The reward grows with its
square and the return with 200 such terms, which is what ``--reward-norm`` is for: a `RewardNormalizer` (team scope) keeps the
running discounted return of every (env, agent) on the device, ``train()`` merges the window into its statistics and trains on
the rewards times ``1 / std(return)``; ``storage.reward`` and the printed mean reward stay in raw units.  Every episode line then
shows the scale and the returns' standard deviation.  ``--reward-clip X`` clamps the scaled reward to [-X, X] (default 10).
Try ``--grid 28 --reward-norm --obs-norm``.

``--shield`` trains THROUGH an `ActionShield` (rate ``--shield-rate``, margin ``--shield-margin``, box 1): the env integrates
the projected action, the projection counting as part of the environment, while the storage -- and with it the learner -- keeps
the policy's own sample (the discrete actor's action index needs unit vectors).  Every episode line then shows the share of the
window's decisions the shield changed and the mean correction.  ``--obstacles N`` (with ``--shield``) puts N static discs of the
reference's sizes off the goals (`place_obstacles`, an `ObstacleField`): the shield then also projects onto one half-plane per
listed disc, and every episode line shows the share of the window's first episodes in which no agent touched a disc.  Without
``--obstacle-inputs`` the reward and the networks' input do not know the discs: the policy meets them as part of the environment.
``--per-env-obstacles`` gives every env N discs of its own (`place_obstacles_per_env`, ``ObstacleField(per_env=True)``) and redraws
them between windows with ``field.set(*place_obstacles_per_env(..., seed=window))``, as the reference's ``reset()`` redraws its
discs: the networks' obstacle columns and the obstacle cost then describe as many maps as there are envs and windows.

``--obstacle-inputs`` makes the training obstacle-aware: the networks read `ObstacleField.observe` -- the record plus
``(p.x, p.y, r)`` of the two nearest discs in range, 12 inputs at k = 2 -- in the rollout (ahead of ``--obs-norm``) and in the
learner (``obstacles=field``), and the learner takes ``--obstacle-weight W`` times the obstacle cost (the reference's collision term
with a disc in the neighbour's place) off every stored reward; the default W is the env's ``collision_weight x dt``.  With a weight
> 0 the discs need no ``--shield``.  Every episode line then shows the window's mean obstacle cost next to the obstacle-free share.

``--share all`` trains ONE actor and ONE critic for the whole team (parameter sharing): the networks are tied
(`BatchedMLP.tie_weights`) and every update pools the agents' gradients (`dronesim_adam_step_shared`); with ``--target-kl`` the
team stops together, on the mean of the agents' KL estimates.  After the loop the script prints that agent 0's and agent N-1's
weights are identical.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scalable_collision_avoidance_rl_amd import drones
from scalable_collision_avoidance_rl_amd.drone_env import dt
from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
from scalable_collision_avoidance_rl_amd.obstacles import ObstacleField, place_obstacles, place_obstacles_per_env
from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
from scalable_collision_avoidance_rl_amd.shield import ActionShield


def linear_init(gen, n, fan_in, fan_out):
    """torch.nn.Linear's default initialisation, stacked over agents, in the kernels' [in, out] layout."""
    b = 1 / np.sqrt(fan_in)
    return ((torch.rand(n, fan_in, fan_out, generator=gen) * 2 - 1) * b, (torch.rand(n, fan_out, generator=gen) * 2 - 1) * b)


def network(gen, n, sizes):
    out = []
    for fi, fo in zip(sizes[:-1], sizes[1:]):
        out += linear_init(gen, n, fi, fo)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--learner", choices=("sa2c", "ppo"), default="sa2c")
    ap.add_argument("--epochs", type=int, default=10, help="epochs per window (--learner ppo)")
    ap.add_argument("--lam", type=float, default=None, help="bootstrapped lambda-returns with this lambda in [0, 1] (default: off)")
    ap.add_argument("--window", type=int, default=200, help="steps per rollout window (default: one episode, 200)")
    ap.add_argument("--time-limit", choices=("terminal", "bootstrap"), default="terminal",
                    help="bootstrap: a time-limit end bootstraps from the value of its terminal observation (needs --lam)")
    ap.add_argument("--ent-coef", type=float, default=0.0, help="entropy bonus: -X x the mean policy entropy in the actor loss (default: off)")
    ap.add_argument("--normalize-advantage", action="store_true",
                    help="standardise each agent's advantages over the window before the epochs (--learner ppo)")
    ap.add_argument("--minibatches", type=int, default=1, help="shuffled minibatches per epoch (--learner ppo; default 1: whole-window epochs)")
    ap.add_argument("--shuffle-seed", type=int, default=0, help="key of the per-epoch row permutations (--minibatches)")
    ap.add_argument("--target-kl", type=float, default=None, help="per-agent KL early stop of the actors (--learner ppo; default: off)")
    ap.add_argument("--vf-clip", type=float, default=None, help="clipped value loss with this range (--learner ppo; default: off)")
    ap.add_argument("--obs-norm", action="store_true", help="normalise observations with running per-agent statistics on the device")
    ap.add_argument("--obs-clip", type=float, default=10.0, help="clamp of the normalised observation (--obs-norm; default 10)")
    ap.add_argument("--share", choices=("all",), default=None, help="parameter sharing: one actor and one critic for all agents (default: off)")
    ap.add_argument("--grid", type=float, default=5.0, help="side length of the goals' square (default 5)")
    ap.add_argument("--reward-norm", action="store_true", help="scale rewards by the running std of the discounted return, on the device")
    ap.add_argument("--reward-clip", type=float, default=10.0, help="clamp of the scaled reward (--reward-norm; default 10)")
    ap.add_argument("--shield", action="store_true", help="train through an ActionShield: the env integrates the projected action")
    ap.add_argument("--shield-rate", type=float, default=0.25, help="share of a gap an agent may close per step, in (0, 0.5]")
    ap.add_argument("--shield-margin", type=float, default=0.05, help="clearance [m] below which a gap may not shrink at all")
    ap.add_argument("--obstacles", type=int, default=0,
                    help="static discs off the goals, enforced by the shield (needs --shield or an --obstacle-weight > 0)")
    ap.add_argument("--per-env-obstacles", action="store_true",
                    help="every env gets discs of its own (--obstacles N each), redrawn between windows as the reference's reset() does")
    ap.add_argument("--obstacle-inputs", action="store_true",
                    help="obstacle-aware training: the networks read the record plus the nearest discs, the reward pays the obstacle cost")
    ap.add_argument("--obstacle-weight", type=float, default=None,
                    help="weight of the obstacle cost in the reward (--obstacle-inputs; default: the env's collision_weight x dt)")
    args = ap.parse_args()
    if args.obstacle_inputs and not args.obstacles:
        ap.error("--obstacle-inputs needs --obstacles N")
    if args.per_env_obstacles and not args.obstacles:
        ap.error("--per-env-obstacles needs --obstacles N")
    if args.obstacle_weight is not None and not args.obstacle_inputs:
        ap.error("--obstacle-weight needs --obstacle-inputs (a cost the networks cannot see teaches nothing)")
    if args.obstacle_weight is not None and not 0.0 <= args.obstacle_weight < float("inf"):
        ap.error("--obstacle-weight must be finite and >= 0")
    penalised = args.obstacle_inputs and (args.obstacle_weight is None or args.obstacle_weight > 0)
    if args.obstacles and not args.shield and not penalised:
        ap.error("--obstacles needs --shield or --obstacle-inputs with a weight > 0 (nothing else makes the discs matter)")
    if args.minibatches != 1 and args.learner != "ppo":
        ap.error("--minibatches needs --learner ppo (one update per window is what A2C is)")
    if args.normalize_advantage and args.learner != "ppo":
        ap.error("--normalize-advantage needs --learner ppo (SA2CLearner has no advantage standardisation)")
    if (args.target_kl is not None or args.vf_clip is not None) and args.learner != "ppo":
        ap.error("--target-kl and --vf-clip need --learner ppo")
    N, E, T, dev = args.agents, args.envs, args.window, "cuda:0"
    env = drones(N, 0, [args.grid, args.grid], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True,
                 device=dev, seed=1, auto_reset=True)
    field = None
    own_discs = lambda window: place_obstacles_per_env(env.grid, args.obstacles, E, seed=window,
                                                       keep_clear=env.end_points.reshape(N, 2), clearance=0.3)
    if args.per_env_obstacles:                               # a list per env: no policy can memorise one map
        discs, counts = own_discs(0)
        field = ObstacleField(env, discs, m=2, per_env=True, counts=counts)
    elif args.obstacles:
        field = ObstacleField(env, place_obstacles(env.grid, args.obstacles, seed=0, keep_clear=env.end_points.reshape(N, 2),
                                                   clearance=0.3), m=2)
    seen_field = field if args.obstacle_inputs else None     # the field whose columns the networks read
    obstacle_weight = 0.0
    if seen_field is not None:                               # the reference's own collision weight, per step
        obstacle_weight = float(env.collision_weight) * dt if args.obstacle_weight is None else args.obstacle_weight
    d_in = env.local_state_space if seen_field is None else seen_field.obs_width
    gen = torch.Generator().manual_seed(0)
    actor = BatchedMLP(*network(gen, N, [d_in, 300, 300, 16]), 1, 1, device=dev, seed=3)     # DiscreteSoftmaxNN x N
    critic = BatchedMLP(*network(gen, N, [d_in, 200, 200, 1]), 0, 0, device=dev)            # CriticNN x N
    if args.share:            # one network for the team: every agent starts from agent 0's weights
        actor.tie_weights(args.share)
        critic.tie_weights(args.share)
    storage = RolloutStorage(env, T, actions=True)
    shield = ActionShield(env, args.shield_rate, args.shield_margin, u_max=1.0, stats=True, obstacles=field) if args.shield else None
    safe = torch.empty(E, N, 2, device=dev) if shield is not None else None

    def step(t):              # the storage keeps the policy's own sample; with a shield the env integrates its projection
        if shield is None:
            env.step(storage.actions[t], into=(storage, t))
        else:
            env.step(storage.actions[t], into=(storage, t), execute=shield(storage.actions[t], out=safe))
    norm = ObsNormalizer(N, d_in, dev, clip=args.obs_clip) if args.obs_norm else None
    augment = (lambda z: z) if seen_field is None else seen_field.observe
    see = augment if norm is None else (lambda z: norm(augment(z)))            # what the networks read of an observation
    rnorm = RewardNormalizer(N, 0.99, dev, clip=args.reward_clip) if args.reward_norm else None
    # the reference's actor_lr argument is never read by train_NN; here the actor's lr is explicit
    if args.learner == "ppo":
        learner = PPOLearner(actor, critic, gamma=0.99, epochs=args.epochs, clip_eps=0.2, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0,
                             lam=args.lam, time_limit=args.time_limit, ent_coef=args.ent_coef,
                             normalize_advantage=args.normalize_advantage, minibatches=args.minibatches, shuffle_seed=args.shuffle_seed,
                             target_kl=args.target_kl, vf_clip=args.vf_clip, obs_norm=norm, share=args.share, reward_norm=rnorm,
                             obstacles=seen_field, obstacle_weight=obstacle_weight)
    else:
        learner = SA2CLearner(actor, critic, gamma=0.99, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0, lam=args.lam,
                              time_limit=args.time_limit, ent_coef=args.ent_coef, obs_norm=norm, share=args.share, reward_norm=rnorm,
                              obstacles=seen_field, obstacle_weight=obstacle_weight)
    if norm is not None:      # one warm-up window of statistics only: window 0 is not trained on the identity map
        storage.begin()
        for t in range(T):
            actor.sample_action(augment(env.z), env=env, act_out=storage.actions[t])
            step(t)
        norm.update(augment(storage.z_pre))
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for ep in range(args.episodes):
        if args.per_env_obstacles and ep:                    # other discs for every window, uploaded in place (inside a stored
            field.set(*own_discs(ep))                        # window a list does not change: the tables and the cost read one)
        storage.begin()
        if shield is not None:
            shield.reset_totals()
        for t in range(T):
            actor.sample_action(see(env.z), env=env, act_out=storage.actions[t])
            step(t)
        start.record()
        out = learner.train(storage)
        stop.record()
        torch.cuda.synchronize()
        ppo = ""
        mean = torch.nanmean if args.target_kl is not None else torch.mean       # a skipped actor step reports NaN
        if args.target_kl is not None:  # the gate is on: the last step's diagnostics of the agents that still computed it
            last = lambda k: out[k][-1][torch.isfinite(out[k][-1])]
            steps = out["actor_steps"].float()
            ppo = (f"  actor steps {int(steps.min())} / {float(steps.mean()):.1f} / {int(steps.max())}  "
                   f"largest kl {float(out['kl'][torch.isfinite(out['kl'])].max()):.2e}")
            if last("clip_fraction").numel():
                ppo += (f"  clipped {float(last('clip_fraction').mean()):.3f}  ratio [{float(last('ratio_min').min()):.3f}, "
                        f"{float(last('ratio_max').max()):.3f}]")
        elif args.learner == "ppo":       # the last epoch's diagnostics (the first epoch's ratio is exactly 1; --minibatches: to rounding)
            ppo = (f"  clipped {float(out['clip_fraction'][-1].mean()):.3f}  kl {float(out['approx_kl'][-1].mean()):+.2e}  "
                   f"ratio [{float(out['ratio_min'][-1].min()):.3f}, {float(out['ratio_max'][-1].max()):.3f}]")
        if "entropy" in out:            # (PPO: the last epoch's; with the gate: over the computed steps)
            ent = out["entropy"] if args.target_kl is not None or out["entropy"].dim() < 2 else out["entropy"][-1]
            ppo += f"  entropy {float(mean(ent)):.3f}"
        if "vf_clip_fraction" in out:
            ppo += f"  value rows clipped {float(out['vf_clip_fraction'][-1].mean()):.3f}"
        if norm is not None:
            std = norm.var.sqrt()
            ppo += f"  obs |mean| <= {float(norm.mean.abs().max()):.2f}  std [{float(std.min()):.3g}, {float(std.max()):.3g}]"
        if rnorm is not None:
            ppo += f"  reward scale {float(out['reward_scale'][0]):.3g}  return std {float(rnorm.std[0]):.4g}"
        if shield is not None:
            sh = shield.summary()
            ppo += f"  shield changed {sh['intervention_share']:.2%} of the decisions, mean correction {sh['mean_correction']:.4f}"
        if field is not None:
            tab = field.episode_safety(storage)
            ok = tab["ep_len"] > 0
            free = (ok & (tab["ep_obstacle_hit_steps"] == 0)).sum().item() / max(int(ok.sum().item()), 1)
            discs = f"{float(field.counts.mean()):.1f} discs per env, redrawn" if field.per_env else f"{field.M} discs"
            ppo += f"  obstacle-free episodes {free:.2%} ({discs})"
        if "obstacle_cost" in out:
            ppo += f"  obstacle cost {float(out['obstacle_cost'].mean()):.4g} (weight {obstacle_weight:.3g})"
        print(f"episode {ep}: mean reward {float(storage.reward.mean()):+.4f}  critic loss {float(out['critic_loss'].mean()):.3f}  "
              f"actor loss {float(mean(out['actor_loss'])):+.3f}  grad norms {float(out['critic_grad_norm'].mean()):.1f} / "
              f"{float(mean(out['actor_grad_norm'])):.1f}{ppo}  update {start.elapsed_time(stop):.2f} ms")
    # one host read after the loop: the kinds of the last window's episode ends
    _, _, n_trunc = (learner.ends, learner.slot_t, learner.n_trunc) if args.time_limit == "bootstrap" else storage.episode_ends()
    finished = int(storage.done.sum())
    print(f"last window: {finished} finished episodes, {int(n_trunc.sum())} of them truncated by the time limit"
          + (f" ({int(n_trunc.sum()) / finished:.1%})" if finished else ""))
    if args.share:
        same = all(torch.equal(getattr(m, n)[0], getattr(m, n)[N - 1]) for m in (actor, critic) for n in ("w1", "b1", "w2", "b2", "w3", "b3"))
        print(f"share {args.share}: agent 0's and agent {N - 1}'s actor and critic weights are {'identical' if same else 'DIFFERENT'}")


if __name__ == "__main__":
    main()
