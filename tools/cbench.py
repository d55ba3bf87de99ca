#!/usr/bin/env python3
"""Developer micro-benchmark of the closed-loop rollout (dronesim_rollout_control: T fused steps with the controller's
action computed in the launch) against the two-launch loop it replaces (`env.control(kind)` then `env.step(act)`), with the
episode layer (records + in-kernel reset) on.  The loop is timed twice: eager from Python (what a caller of the two methods
gets: host-bound) and captured as one hipGraph (the device's share: two dependent launches per step).  All three are timed
ALTERNATELY, `reps` times each, from the same start state; prints median / min / max per step and the number of near pairs per
env (centres closer than dhat + 2 l) along the episode, next to the random walk's.

    python tools/cbench.py [c3 c2 ...] [--T 200] [--reps 7]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scalable_collision_avoidance_rl_amd import drones
from tools.kbench import PRESETS


def near_pairs(pos, reach):
    """Mean number of unordered pairs per env closer than `reach` (centre to centre)."""
    d = torch.cdist(pos, pos)
    n = pos.shape[1]
    return float(((d < reach).sum((1, 2)) - n).double().mean()) / 2


def along(env, advance, n_envs, reach, marks=(0, 50, 100, 150, 199)):
    """[(step, near pairs per env)] of the first `n_envs` envs along one episode (199: ahead of the 200-step limit's reset)."""
    out, at = [], 0
    for s in marks:
        if s > at:
            advance(s - at)
            at = s
        out.append((s, near_pairs(env.pos[:n_envs], reach)))
    return out


def main():
    args = [a for a in sys.argv[1:] if a in PRESETS]
    opt = lambda k, d: int(sys.argv[sys.argv.index(k) + 1]) if k in sys.argv else d
    T, reps = opt("--T", 200), opt("--reps", 7)
    for spec in (args or ["c3", "c2"]):
        N, E, G, delta = PRESETS[spec]
        mk = lambda: drones(N, 0, [G, G], "O", deltas=np.ones(N) * delta, simplify_zstate=True, n_envs=E, batched=True,
                            seed=1, auto_reset=True)
        chunk = max(1, 512 // N)                              # (cdist over all envs at once would be E x N x N floats)
        for kind in ("proportional", "gradient"):
            env = mk()
            reach = float(env.d_safety.max()) + 2 * float(env.drone_radius.max())
            start = env.get_state()
            fused, loop, graphed = [], [], []

            def two_launch_loop():
                for _ in range(T):
                    env.step(env.control(kind))               # (captured: control()'s output lives in the graph's own pool)
            two_launch_loop(); torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                two_launch_loop()
            for rep in range(reps + 1):                       # (the first pass warms both up and is dropped)
                env.load_state(start)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); out = env.rollout_control(kind, T); b.record(); torch.cuda.synchronize()
                fused.append(a.elapsed_time(b) * 1e3 / T)
                del out
                env.load_state(start)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(T):
                    env.step(env.control(kind))
                b.record(); torch.cuda.synchronize()
                loop.append(a.elapsed_time(b) * 1e3 / T)
                env.load_state(start)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(); graph.replay(); b.record(); torch.cuda.synchronize()
                graphed.append(a.elapsed_time(b) * 1e3 / T)
            f, l, g = np.array(fused[1:]), np.array(loop[1:]), np.array(graphed[1:])
            st = lambda v: f"{np.median(v):6.2f} (min {v.min():.2f} max {v.max():.2f})"
            print(f"{spec} {kind:12s} T={T} us/step: fused {st(f)}  control()+step() eager {st(l)}  as one hipGraph {st(g)}  "
                  f"fused is {np.median(l) / np.median(f):.2f}x / {np.median(g) / np.median(f):.2f}x faster", flush=True)
            del graph
            env.load_state(start)
            print(f"{spec} {kind:12s} near pairs per env at step " + "  ".join(
                f"{s}: {n:.1f}" for s, n in along(env, lambda n: env.rollout_control(kind, n), chunk * 8, reach)), flush=True)
        # the random walk the other fused rollouts time, for the "denser distribution" comparison
        env = mk()
        print(f"{spec} random walk  near pairs per env at step " + "  ".join(
            f"{s}: {n:.1f}" for s, n in along(env, env.rollout_random, chunk * 8, reach)), flush=True)


if __name__ == "__main__":
    main()
