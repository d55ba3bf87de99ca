#!/usr/bin/env python3
"""The reference's `benchmark_agent.py` on the MI355X-native stack: roll a trained actor out without learning and report the
per-episode figures, the critic against the simulated return and the collision histogram.

The reference runs 1500 episodes one after the other (benchmark_agent.py:53-118); here E envs run `rounds` fresh episodes
each (E x rounds >= --episodes), every step of every env in one launch, and the tables are reduced on the device.

    python examples/benchmark_agent.py --critics discrete-A2Ccritics.pth --actors discrete-A2Cactors.pth [--models models]
    python examples/benchmark_agent.py --controller proportional            # the commented alternatives of :76-77
    python examples/benchmark_agent.py ... --obs-norm stats.pt             # the observation statistics the networks were trained with
    python examples/benchmark_agent.py ... --safety                        # closest approach, arrival and formation error per episode
    python examples/benchmark_agent.py ... --shield [--shield-rate X --shield-margin X]   # the same episodes again through an ActionShield
    python examples/benchmark_agent.py ... --obstacles 8 [--shield --safety]              # static discs that matter
    python examples/benchmark_agent.py ... --obstacles 8 --per-env-obstacles               # a list of its own for every env

``--obs-norm FILE``: an `ObsNormalizer.state_dict()` saved with ``torch.save``; the actor and the critic then read the normalised
observation (the reference's files carry no statistics, so there is none by default).

``--shield``: after the plain evaluation the same number of episodes runs again with every action projected by an `ActionShield`
(box 1, the clip of the controllers and the norm of the discrete actions) before the step integrates it, and the collision-free
share is printed next to the unshielded one, with the share of decisions the shield changed and what it cost in arrival
(``--safety``).  With ``--controller`` the shielded rounds are three launches per step instead of one fused launch per round.

``--obstacles N``: N discs of the reference's sizes off the goals (`place_obstacles`) in an `ObstacleField`; the evaluation (with
``--safety`` implied) then reports the share of episodes in which no agent touched a disc, and with ``--shield`` the shield also
projects onto one half-plane per listed disc, so the obstacle-free share is printed shielded next to unshielded.  The reward does
not know the discs, and neither do the networks' inputs unless ``--obstacle-inputs`` is given: the saved networks were then trained
obstacle-aware (``train_loop.py --obstacle-inputs``: ``d_in = field.obs_width``) and read ``field.observe(env.z)``, ahead of
``--obs-norm``.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scalable_collision_avoidance_rl_amd.drone_env as drone_env          # was: import drone_env
from scalable_collision_avoidance_rl_amd.evaluate import Evaluator, TrainedAgent    # was: from SAC_agents import *
from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
from scalable_collision_avoidance_rl_amd.obstacles import ObstacleField, place_obstacles, place_obstacles_per_env
from scalable_collision_avoidance_rl_amd.shield import ActionShield


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--critics", default="discrete-A2Ccritics.pth")
    ap.add_argument("--actors", default="discrete-A2Cactors.pth")
    ap.add_argument("--models", default="models")
    ap.add_argument("--controller", choices=["proportional", "gradient"], default=None)
    ap.add_argument("--agents", type=int, default=None, help="default: the number of saved critics (8 with a controller)")
    ap.add_argument("--episodes", type=int, default=1500)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--obs-norm", default=None, help="a torch.save'd ObsNormalizer.state_dict() (network actors only)")
    ap.add_argument("--safety", action="store_true", help="also reduce and print the per-episode safety tables")
    ap.add_argument("--shield", action="store_true", help="run the episodes again through an ActionShield and compare")
    ap.add_argument("--shield-rate", type=float, default=0.25, help="share of a gap an agent may close per step, in (0, 0.5]")
    ap.add_argument("--shield-margin", type=float, default=0.05, help="clearance [m] below which a gap may not shrink at all")
    ap.add_argument("--obstacles", type=int, default=0, help="static discs off the goals, sensed, reported and (--shield) enforced")
    ap.add_argument("--per-env-obstacles", action="store_true", help="every env gets --obstacles N discs of its own")
    ap.add_argument("--obstacle-rate", type=float, default=None, help="share of the gap to a disc an agent may close per step, in (0, 1]")
    ap.add_argument("--obstacle-inputs", action="store_true",
                    help="the saved networks were trained obstacle-aware: they read the record plus the field's obstacle columns")
    a = ap.parse_args()
    if a.obstacle_inputs and (not a.obstacles or a.controller):
        ap.error("--obstacle-inputs needs --obstacles N and saved networks (no --controller)")
    if a.per_env_obstacles and not a.obstacles:
        ap.error("--per-env-obstacles needs --obstacles N")
    a.safety = a.safety or a.obstacles > 0

    if a.controller:
        n_agents, actor, critic = a.agents or 8, a.controller, None
    else:
        agents = TrainedAgent(critics_name=a.critics, actors_name=a.actors, n_agents=a.agents or "auto", models_dir=a.models,
                              precision=a.precision)                                                # benchmark_agent.py:47
        n_agents, actor, critic = agents.n_agents, agents.actor, agents.critic
    deltas = np.ones(n_agents) * 1                                                                  # :29
    env = drone_env.drones(n_agents=n_agents, n_obstacles=0, grid=[5, 5], end_formation="O", deltas=deltas, simplify_zstate=True,
                           n_envs=a.envs, auto_reset=True)                                          # :30
    env.collision_weight = 0.2                                                                      # :31
    rounds = -(-a.episodes // a.envs)
    print("### Running Trained agent (no learning)")                                               # :48-50
    print(f"Episodes = {rounds * a.envs} ({a.envs} envs x {rounds} rounds), max Time iterations = {drone_env.max_time_steps} "
          f"(T = {drone_env.max_time_steps * drone_env.dt}s, dt = {drone_env.dt}s)")
    print(f"N of agents = {env.n_agents}, collision weight b = {env.collision_weight}")

    obs_norm = None
    field = None
    if a.per_env_obstacles:
        discs, counts = place_obstacles_per_env(env.grid, a.obstacles, env.n_envs, seed=0, keep_clear=env.end_points.reshape(n_agents, 2),
                                                clearance=0.3)
        field = ObstacleField(env, discs, m=2, per_env=True, counts=counts)
    elif a.obstacles:
        discs = place_obstacles(env.grid, a.obstacles, seed=0, keep_clear=env.end_points.reshape(n_agents, 2), clearance=0.3)
        field = ObstacleField(env, discs, m=2)
    if a.obs_norm:
        import torch
        width = field.obs_width if a.obstacle_inputs else env.local_state_space
        obs_norm = ObsNormalizer(n_agents, width, env.device).load_state_dict(torch.load(a.obs_norm))
    if field is not None and field.per_env:
        print(f"Obstacles = a list per env: {int(counts.min())} .. {int(counts.max())} discs (of {a.obstacles} drawn per env; the rest "
              f"covered a goal)")
    elif field is not None:
        print(f"Obstacles = {field.M} discs (of {a.obstacles} drawn; the rest covered a goal), radius {discs[:, 2].min():.2f} .. "
              f"{discs[:, 2].max():.2f} m" if field.M else f"Obstacles = 0 (all {a.obstacles} drawn covered a goal)")
    ev = Evaluator(env, actor, critic, gamma=0.99, obs_norm=obs_norm, safety=a.safety, obstacles=field, obstacle_inputs=a.obstacle_inputs)
    ev.run(rounds)
    s = ev.summary()
    print(f"Episodes {s['episodes']} - Average Reward/Collisions/Steps: {s['mean_return']:.1f}/{s['mean_collisions']:.2f}/"
          f"{s['mean_length']:.1f}. True r={s['mean_true_return']:.1f}.")                          # :119-120
    if s["mean_advantage"] is not None:
        print("mean_T [G_t - V(z_t)] per agent: " + " ".join(f"{x:.3f}" for x in s["mean_advantage"]))   # :105, :143
    # the reference's histogram has bins of two collisions starting at the smallest count seen (:150): counts[0], counts[1]
    hist = np.asarray(s["collision_hist"], np.float64)
    lo = int(np.flatnonzero(hist)[0]) if hist.any() else 0
    pair = lambda j: hist[lo + 2 * j:lo + 2 * j + 2].sum() / max(hist.sum(), 1.0)
    print(f"Runs with 0 coll. = {pair(0) * 100:.2f}%. 2 coll. = {pair(1) * 100:.2f}%")             # :151
    print(f"(episodes without any collision: {s['zero_collision_share'] * 100:.2f}%)")
    if a.safety:                                             # (no reference line: the reference logs none of these)
        f = ev.safety_summary()
        fmt = lambda x, spec: "-" if x is None else format(x, spec)
        print(f"Arrived = {f['arrived_share'] * 100:.2f}%. Arrived without a collision = {f['success_share'] * 100:.2f}%. "
              f"Mean step of an agent's arrival = {fmt(f['mean_arrive_step'], '.1f')}")
        print(f"Smallest clearance per episode: mean {f['mean_min_clearance']:.3f} m, minimum {fmt(f['min_clearance'], '.3f')} m. "
              f"Largest final goal distance per episode: mean {f['mean_goal_dist_max']:.3f} m")
        if field is not None:
            print(f"Episodes without an obstacle hit = {f['obstacle_free_share'] * 100:.2f}%. Arrived with no collision and no hit = "
                  f"{f['arrived_clear_share'] * 100:.2f}%. Smallest gap to a disc per episode: mean {f['mean_min_obstacle_gap']:.3f} m, "
                  f"minimum {fmt(f['min_obstacle_gap'], '.3f')} m")
    if a.shield:                                             # (no reference line: the reference has no safety layer)
        shield = ActionShield(env, rate=a.shield_rate, margin=a.shield_margin, u_max=1.0, stats=True, obstacles=field,
                              obstacle_rate=a.obstacle_rate if field is not None else None)
        evs = Evaluator(env, actor, critic, gamma=0.99, obs_norm=obs_norm, safety=a.safety, shield=shield, obstacles=field,
                        obstacle_inputs=a.obstacle_inputs)
        evs.run(rounds)
        t = evs.summary()
        print(f"### Shielded (rate = {shield.rate}, margin = {shield.margin} m, box = {shield.u_max})")
        print(f"Episodes {t['episodes']} - Average Reward/Collisions/Steps: {t['mean_return']:.1f}/{t['mean_collisions']:.2f}/"
              f"{t['mean_length']:.1f}. True r={t['mean_true_return']:.1f}.")
        print(f"(episodes without any collision: shielded {t['zero_collision_share'] * 100:.2f}%, unshielded "
              f"{s['zero_collision_share'] * 100:.2f}%)")
        print(f"The shield changed {t['shield_intervention_share'] * 100:.2f}% of the decisions; mean correction {t['shield_mean_correction']:.4f} m/s "
              f"(over the changed ones {t['shield']['mean_correction_intervened']:.4f}, largest {t['shield']['max_correction']:.4f})")
        if a.safety:
            g = evs.safety_summary()
            print(f"Arrived = {g['arrived_share'] * 100:.2f}% (unshielded {f['arrived_share'] * 100:.2f}%). Smallest clearance per episode: "
                  f"mean {g['mean_min_clearance']:.3f} m, minimum {fmt(g['min_clearance'], '.3f')} m (unshielded "
                  f"{fmt(f['min_clearance'], '.3f')} m)")
            if field is not None:
                print(f"Episodes without an obstacle hit: shielded {g['obstacle_free_share'] * 100:.2f}%, unshielded "
                      f"{f['obstacle_free_share'] * 100:.2f}%. Smallest gap to a disc: shielded {fmt(g['min_obstacle_gap'], '.3f')} m, "
                      f"unshielded {fmt(f['min_obstacle_gap'], '.3f')} m")


if __name__ == "__main__":
    main()
