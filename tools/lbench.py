#!/usr/bin/env python3
"""Learner micro-benchmark (developer tool; bench.py stays the project's yardstick): one `SA2CLearner.train` per shape --
or, with ``--learner ppo``, one `PPOLearner.train` of ``--epochs M`` epochs --, timed with device events after warm-up.

    python tools/lbench.py [--configs c1,c3,c5] [--reps 3] [--warmup 1] [--learner {sa2c,ppo}] [--epochs M] [--lam X]
                           [--time-limit {terminal,bootstrap}]
    python tools/lbench.py --scans [--configs c3,c5] [--reps 9] [--out profiles/lambda_returns_lbench.jsonl]
    python tools/lbench.py --scans --time-limit bootstrap [--configs c3,c5] [--reps 9] [--out profiles/timelimit_lbench.jsonl]
    python tools/lbench.py --scans --standardize [--configs c3,c5] [--reps 3] [--out profiles/entropy_lbench.jsonl]
    python tools/lbench.py --learner ppo --epochs M --ent-coef 0.01 --normalize-advantage [--out profiles/entropy_lbench.jsonl]
    python tools/lbench.py --learner ppo --epochs M --minibatches K [--out profiles/minibatch_lbench.jsonl]
    python tools/lbench.py --gather [--configs c1,c3,c5] [--reps 5] [--minibatches K] [--out profiles/minibatch_lbench.jsonl]
    python tools/lbench.py --learner ppo --epochs M [--target-kl X] [--vf-clip X] [--out profiles/target_kl_lbench.jsonl]
    python tools/lbench.py --gate-compare [--configs c3,c5] [--reps 3] [--out profiles/target_kl_lbench.jsonl]
    python tools/lbench.py --scans --obsnorm [--configs c3,c5] [--reps 9] [--out profiles/obsnorm_lbench.jsonl]
    python tools/lbench.py [--learner ppo --epochs M] --obs-norm [--out profiles/obsnorm_lbench.jsonl]
    python tools/lbench.py --scans --rewnorm [--configs c3,c5] [--reps 9] [--out profiles/rewnorm_lbench.jsonl]
    python tools/lbench.py [--learner ppo --epochs M] --reward-norm [--out profiles/rewnorm_lbench.jsonl]
    python tools/lbench.py [--learner ppo --epochs M] --share all [--out profiles/share_lbench.jsonl]
    python tools/lbench.py --adam-step [--share all] [--configs c3,c5] [--reps 9] [--calls 20] [--out profiles/share_lbench.jsonl]

``--lam X`` times the learner with bootstrapped lambda-returns (one more ring slot of observations; off by default).
``--time-limit bootstrap`` (with ``--lam``) times it with time-limit ends bootstrapped from their terminal observations: the
window's last step ends every episode with all agents outside the goal disk, so every env has one truncated end (M = 1).
With ``--scans`` it times `dronesim_lambda_returns_ends` (one truncated end per env at a random slot) against
`dronesim_lambda_returns` on the same rewards and values with ``done = ends != 0`` (allowed: the yardstick + 15 %), and
`dronesim_episode_ends` on a window with those ends (microseconds and bytes: it is launch-floor work).
``--scans --standardize`` times `dronesim_standardize` in place on a window's advantages, which is the learner's call (12 bytes
per element: read, then read and write), against `dronesim_returns` on an array of the same size in the same process (8 bytes
per element): expected is the yardstick x 1.5, allowed that + 15 %.  A third line, `dronesim_standardize_out_of_place`, is
the same call with ``y != x`` against the same bound.  ``--ent-coef X`` / ``--normalize-advantage`` time a whole update with the
entropy bonus / the per-agent advantage standardisation (the latter ``--learner ppo`` only).
``--minibatches K`` (``--learner ppo``) times the learner with K shuffled minibatches per epoch (K x epochs Adam steps per
network; per epoch one `dronesim_row_permutation` and one `dronesim_gather_rows`).  ``--gather`` times those two alone, on the
five learner arrays of a window (z_pre, actions, logp_old, adv, G: 4 N (d_in + 5) bytes per row) cut into K blocks (default 4,
``--minibatches 1`` is a single block), every block rounded up to 256 bytes as the learner does, next to a plain device-to-device copy of the same five arrays in the same process: device events around
``--calls`` back-to-back calls, median and minimum over ``--reps``; bytes moved = 2 x the arrays' bytes.
``--target-kl X`` / ``--vf-clip X`` (``--learner ppo``) time a whole update with the per-agent KL early stop / the clipped value
loss; with either, the line also carries ``critic_epoch_ms``, a critic-only epoch (the critic's gradient chain + its Adam step)
timed in the same process.  ``--gate-compare`` answers "does a stopped agent cost no matrix work": in ONE process, alternating
after a warm-up, it times `PPOLearner.train` at 2 and at 6 epochs with ``target_kl = 1e-30`` (every agent stops on its second
step) and without the gate, and the critic-only epoch.  The marginal cost of a later gated epoch, (t_gated(6) - t_gated(2)) / 4,
is allowed the critic-only epoch + 15 %; it is also reported as a share of the ungated marginal epoch.
``--scans --obsnorm`` times the observation normaliser's two entry points on a window's observations x [T E][N d] against
`dronesim_returns` on that shape's [T,E,N] rewards in the same process (8 bytes per [T,E,N] element): `dronesim_obsnorm_update`
reads 4 bytes per x element (expected: the yardstick x d / 2), `dronesim_obsnorm_apply` reads and writes 8 (expected: x d),
allowed = expected + 15 %.  For c3 it then times the captured rollout loop (softmax-16 actor ``precision="f16x2"`` + step) with and
without `norm(env.z)` in front of the policy: required <= 1.05 x the loop without it.  ``--obs-norm`` times a whole update with
an `ObsNormalizer` (normalise first, update last).
``--scans --rewnorm`` times the reward normaliser's two entry points next to `dronesim_returns` on the same [T,E,N] rewards in the
same process: `dronesim_rewnorm_update` reads 4 bytes per element (and the flags) and moves 64 per column (the carry in and out, the triple out and in again), the
yardstick moves 8 per element, `dronesim_rewnorm_apply` 8 per element.  Each line carries its bytes, TB/s and ``us_per_byte_ratio``,
its time per byte over the yardstick's; there is no bound.  ``--reward-norm`` times a whole update with a `RewardNormalizer`
(update, then apply, then the scans on the normalised copy).
``--share all`` times the learner with parameter sharing: both networks tied over all agents (`BatchedMLP.tie_weights`), every
Adam step `dronesim_adam_step_shared`.  ``--adam-step`` times `BatchedAdam.step` alone, actor + critic on fixed gradients
(``refresh=False``; device events around ``--calls`` back-to-back step pairs, median / min / max over ``--reps``), unshared or
with ``--share all``, next to the bytes each form has to move (36 |G| against 8 |G| + 44 per element of a group).
``--scans`` times the learner-side scans alone instead: `dronesim_returns` (the yardstick) and `dronesim_lambda_returns`
with G only and with G + A, on the same buffers in the same process, device events around ``--calls`` back-to-back calls
after a warm-up, median and minimum over ``--reps`` repetitions, one JSON line each (appended to ``--out`` when given).

A PPO epoch's cost is the marginal one, (t_3 - t_1) / 2 from runs at ``--epochs 1`` and ``--epochs 3``; the once-per-window
part (returns, old log-probabilities, baseline, advantage) is t_1 less one epoch.

Shapes (N x E x T, actor + critic of the reference's widths):
    c1   5 x 1 x 200       softmax-16 actor (6 -> 300 -> 300 -> 16) + critic (6 -> 200 -> 200 -> 1)
    c3   64 x 4096 x 200   the same networks
    c5   256 x 512 x 200   Gaussian actor (6 -> 400 -> 200|200 -> 4) + critic          (the C5 shard)
Prints one JSON line per shape: ms per update, FLOP from shapes (2 per multiply-add: forward, the two backward products of
each layer, and the critic's post-update forward for the baseline) and the share of the 157.3 TF float32 matrix peak.
Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -d DIR -o lbench -- python tools/lbench.py
--configs c3 --reps 1 --warmup 0` (one update, nothing else on the GPU but the setup's small kernels):
`python tools/lbench.py --stats DIR/.../lbench_kernel_stats.csv` prints each kernel's total ms and share of the update's."""
import argparse
import json
import math
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TF = 157.3
CONFIGS = {"c1": (5, 1, 200, "softmax"), "c3": (64, 4096, 200, "softmax"), "c5": (256, 512, 200, "gaussian")}


def mlp_flop(rows, d_in, h1, h2, nout, backward=True):
    fwd = 2 * rows * (d_in * h1 + h1 * h2 + h2 * nout)
    if not backward:
        return fwd
    # dW3, dH2, dW2, dH1, dW1 (the bias rows are noise)
    return fwd + 2 * rows * (2 * h2 * nout + 2 * h1 * h2 + d_in * h1)


def scans(args):
    """The scans of a stored window [T][E][N] next to each other: bytes per element 8 (r in, G out), 12 (+ V in), 16 (+ A out)."""
    import ctypes as C
    import statistics

    import torch
    from scalable_collision_avoidance_rl_amd import _native
    lib, dev = _native.lib(), "cuda:0"
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []
    for name in args.configs.split(","):
        N, E, T, _ = CONFIGS[name]
        g = torch.Generator(device=dev).manual_seed(0)
        r = torch.randn(T, E, N, device=dev, generator=g)
        V = torch.randn(T + 1, E, N, device=dev, generator=g)
        done = (torch.rand(T, E, device=dev, generator=g) < 0.01).to(torch.uint8)
        done[-1] = 1
        G, A = torch.empty_like(r), torch.empty_like(r)
        lam = 0.95 if args.lam is None else args.lam
        calls = {"dronesim_returns": (8, lambda: lib.dronesim_returns(r.data_ptr(), done.data_ptr(), 0.99, G.data_ptr(), T, E, N, stream())),
                 "dronesim_lambda_returns G": (12, lambda: lib.dronesim_lambda_returns(r.data_ptr(), done.data_ptr(), V.data_ptr(), 0.99, lam,
                                                                                       G.data_ptr(), None, T, E, N, stream())),
                 "dronesim_lambda_returns G+A": (16, lambda: lib.dronesim_lambda_returns(r.data_ptr(), done.data_ptr(), V.data_ptr(), 0.99, lam,
                                                                                         G.data_ptr(), A.data_ptr(), T, E, N, stream()))}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        base = None
        for what, (bpe, fn) in calls.items():
            for _ in range(max(1, args.warmup) * args.calls):
                _native.check(fn(), what)
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                ev[0].record()
                for _ in range(args.calls):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                us.append(ev[0].elapsed_time(ev[1]) * 1e3 / args.calls)
            med, lo = statistics.median(us), min(us)
            line = dict(what=what, config=name, N=N, E=E, T=T, lam=None if bpe == 8 else lam, us=round(med, 2), us_min=round(lo, 2),
                        bytes_per_element=bpe, tb_s=round(r.numel() * bpe / 1e6 / med, 3), calls=args.calls, reps=args.reps)
            if base is None:
                base = med
            else:       # the byte ratio to the yardstick plus 15 % (the longer dependent chain per step, run-to-run spread)
                line.update(ratio=round(med / base, 3), expected_us=round(base * bpe / 8, 2), allowed_us=round(base * bpe / 8 * 1.15, 2),
                            inside=bool(med <= base * bpe / 8 * 1.15))
            if args.tag:
                line["tag"] = args.tag
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def scans_standardize(args):
    """`dronesim_standardize` next to its yardstick `dronesim_returns` on an array of the same size."""
    import ctypes as C
    import statistics

    import torch
    from scalable_collision_avoidance_rl_amd import _native
    lib, dev = _native.lib(), "cuda:0"
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []
    for name in args.configs.split(","):
        N, E, T, _ = CONFIGS[name]
        g = torch.Generator(device=dev).manual_seed(0)
        r = torch.randn(T, E, N, device=dev, generator=g)
        done = (torch.rand(T, E, device=dev, generator=g) < 0.01).to(torch.uint8)
        done[-1] = 1
        G = torch.empty_like(r)
        adv = torch.randn(T, E, N, device=dev, generator=g) * 0.5 - 500.0
        out, stats = torch.empty_like(adv), torch.empty(2, N, device=dev)
        n = C.c_size_t(0)
        _native.check(lib.dronesim_standardize_workspace(T * E, N, C.byref(n)), "dronesim_standardize_workspace")
        ws = torch.empty(n.value // 8, dtype=torch.float64, device=dev)
        std = lambda y: lib.dronesim_standardize(adv.data_ptr(), y.data_ptr(), stats.data_ptr(), T * E, N, 1e-8, ws.data_ptr(), n.value, stream())
        # in place every call after the first standardises standardised advantages: the same traffic and arithmetic
        calls = {"dronesim_returns": (8, lambda: lib.dronesim_returns(r.data_ptr(), done.data_ptr(), 0.99, G.data_ptr(), T, E, N, stream())),
                 "dronesim_standardize_out_of_place": (12, lambda: std(out)),
                 "dronesim_standardize": (12, lambda: std(adv))}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        base = None
        for what, (bpe, fn) in calls.items():
            for _ in range(max(1, args.warmup) * args.calls):
                _native.check(fn(), what)
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                ev[0].record()
                for _ in range(args.calls):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                us.append(ev[0].elapsed_time(ev[1]) * 1e3 / args.calls)
            med, lo = statistics.median(us), min(us)
            line = dict(what=what, config=name, R=T * E, N=N, us=round(med, 2), us_min=round(lo, 2), bytes_per_element=bpe,
                        tb_s=round(r.numel() * bpe / 1e6 / lo, 3), calls=args.calls, reps=args.reps)
            if base is None:
                base = lo
            else:       # best of the repetitions against best: the byte ratio to the yardstick, plus 15 %
                line.update(ratio=round(lo / base, 3), expected_us=round(base * 1.5, 2), allowed_us=round(base * 1.5 * 1.15, 2),
                            inside=bool(lo <= base * 1.5 * 1.15), workspace_bytes=int(n.value))
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def scans_obsnorm(args):
    """`dronesim_obsnorm_update` / `dronesim_obsnorm_apply` next to their yardstick `dronesim_returns`, and the captured C3
    rollout loop with and without the per-step map."""
    import ctypes as C
    import statistics

    import numpy as np
    import torch
    from scalable_collision_avoidance_rl_amd import _native, drones
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    lib, dev = _native.lib(), "cuda:0"
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lines = []

    def timed(fn, what):
        for _ in range(max(1, args.warmup) * args.calls):
            _native.check(fn(), what)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.reps):
            ev[0].record()
            for _ in range(args.calls):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            us.append(ev[0].elapsed_time(ev[1]) * 1e3 / args.calls)
        return statistics.median(us), min(us)

    for name in args.configs.split(","):
        N, E, T, _ = CONFIGS[name]
        d = 6
        g = torch.Generator(device=dev).manual_seed(0)
        r = torch.randn(T, E, N, device=dev, generator=g)
        done = (torch.rand(T, E, device=dev, generator=g) < 0.01).to(torch.uint8)
        done[-1] = 1
        G = torch.empty_like(r)
        x = torch.randn(T, E, N, d, device=dev, generator=g) * 30 + 100
        y = torch.empty_like(x)
        norm = ObsNormalizer(N, d, dev)
        norm.update(x)
        ws, wsb = norm._workspace(T * E)
        R_, C_ = T * E, N * d
        calls = [("dronesim_returns", 8 * r.numel(), None,
                  lambda: lib.dronesim_returns(r.data_ptr(), done.data_ptr(), 0.99, G.data_ptr(), T, E, N, stream())),
                 ("dronesim_obsnorm_update", 4 * x.numel(), d / 2,
                  lambda: lib.dronesim_obsnorm_update(x.data_ptr(), R_, C_, norm.state.data_ptr(), norm.table.data_ptr(), norm.eps,
                                                      ws.data_ptr(), wsb, stream())),
                 ("dronesim_obsnorm_apply", 8 * x.numel(), float(d),
                  lambda: lib.dronesim_obsnorm_apply(x.data_ptr(), y.data_ptr(), R_, C_, norm.table.data_ptr(), 10.0, stream())),
                 ("dronesim_obsnorm_apply_in_place", 8 * x.numel(), float(d),
                  lambda: lib.dronesim_obsnorm_apply(y.data_ptr(), y.data_ptr(), R_, C_, norm.table.data_ptr(), 10.0, stream()))]
        base = None
        for what, nbytes, factor, fn in calls:
            med, lo = timed(fn, what)
            line = dict(what=what, config=name, R=R_, C=C_, N=N, us=round(med, 2), us_min=round(lo, 2), bytes=nbytes,
                        tb_s=round(nbytes / 1e6 / med, 3), calls=args.calls, reps=args.reps)
            if base is None:
                base = med
            else:
                line.update(ratio=round(med / base, 3), expected_us=round(base * factor, 2), allowed_us=round(base * factor * 1.15, 2),
                            inside=bool(med <= base * factor * 1.15))
            lines.append(line)
            print(json.dumps(line), flush=True)
        del r, G, x, y, norm
        if name != "c3":
            continue
        # the captured rollout loop: policy -> step, with and without the map in front of the policy (same session, alternating)
        from tools.kbench import PRESETS
        Np, Ep, Gp, delta = PRESETS["c3"]
        steps, graphs, keep = 50, {}, []                 # (keep: what a captured graph reads and writes must outlive its replays)
        for with_norm in (False, True):
            env = drones(Np, 0, [Gp, Gp], "O", deltas=np.ones(Np) * delta, simplify_zstate=True, n_envs=Ep, batched=True, seed=1,
                         auto_reset=True)
            gp = torch.Generator().manual_seed(4321)
            rw = lambda *sh: (torch.rand(*sh, generator=gp) * 2 - 1) * 0.2
            actor = BatchedMLP(rw(Np, 6, 300), rw(Np, 300), rw(Np, 300, 300), rw(Np, 300), rw(Np, 300, 16), rw(Np, 16), 1, 1,
                               device=dev, seed=1234, precision="f16x2")
            act = torch.zeros(Ep, Np, 2, device=dev)
            norm = ObsNormalizer(Np, env.local_state_space, dev)
            norm.update(env.z)

            def loop(n, env=env, actor=actor, act=act, norm=norm, with_norm=with_norm):
                for _ in range(n):
                    actor.sample_action(norm(env.z) if with_norm else env.z, env=env, act_out=act)
                    env.step(act)

            loop(3)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                loop(steps)
            graph.replay()
            torch.cuda.synchronize()
            graphs[with_norm] = graph
            keep.append((env, actor, act, norm, loop))
        us = {False: [], True: []}
        for _ in range(args.reps):
            for with_norm, graph in graphs.items():
                ev[0].record(); graph.replay(); ev[1].record()
                torch.cuda.synchronize()
                us[with_norm].append(ev[0].elapsed_time(ev[1]) * 1e3 / steps)
        plain, normed = statistics.median(us[False]), statistics.median(us[True])
        line = dict(what="captured rollout step, softmax-16 f16x2 + step, without / with norm(env.z)", config=name, N=Np, E=Ep,
                    us_without=round(plain, 2), us_with=round(normed, 2), ratio=round(normed / plain, 4), required=1.05,
                    inside=bool(normed <= 1.05 * plain), us_all_without=[round(u, 2) for u in us[False]],
                    us_all_with=[round(u, 2) for u in us[True]], steps=steps, reps=args.reps)
        lines.append(line)
        print(json.dumps(line), flush=True)
        del graphs, keep
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def scans_rewnorm(args):
    """`dronesim_rewnorm_update` / `dronesim_rewnorm_apply` next to `dronesim_returns` on the same [T,E,N] in the same process."""
    import ctypes as C
    import statistics

    import torch
    from scalable_collision_avoidance_rl_amd import _native
    from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
    lib, dev = _native.lib(), "cuda:0"
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    lines = []

    def timed(fn, what):
        for _ in range(max(1, args.warmup) * args.calls):
            _native.check(fn(), what)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.reps):
            ev[0].record()
            for _ in range(args.calls):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            us.append(ev[0].elapsed_time(ev[1]) * 1e3 / args.calls)
        return statistics.median(us), min(us)

    for name in args.configs.split(","):
        N, E, T, _ = CONFIGS[name]
        g = torch.Generator(device=dev).manual_seed(0)
        r = -torch.rand(T, E, N, device=dev, generator=g) * 30
        done = (torch.rand(T, E, device=dev, generator=g) < 0.01).to(torch.uint8)
        done[-1] = 1
        G, y = torch.empty_like(r), torch.empty_like(r)
        for scope in ("team", "agent"):
            norm = RewardNormalizer(N, 0.99, dev, scope=scope)
            norm.update(r, done)
            ws, wsb = norm._workspace(T, E)
            calls = [("dronesim_returns", 8 * r.numel(),
                      lambda: lib.dronesim_returns(r.data_ptr(), done.data_ptr(), 0.99, G.data_ptr(), T, E, N, stream())),
                     ("dronesim_rewnorm_update", 4 * r.numel() + done.numel() + (16 + 24 + 24) * E * N,
                      lambda: lib.dronesim_rewnorm_update(r.data_ptr(), done.data_ptr(), T, E, N, 0.99, norm.group.data_ptr(), norm.n_groups,
                                                          norm.ret.data_ptr(), norm.state.data_ptr(), norm.scale.data_ptr(), norm.eps,
                                                          ws.data_ptr(), wsb, stream())),
                     ("dronesim_rewnorm_apply", 8 * r.numel(),
                      lambda: lib.dronesim_rewnorm_apply(r.data_ptr(), y.data_ptr(), T, E, N, norm.scale.data_ptr(), 10.0, stream())),
                     ("dronesim_rewnorm_apply_in_place", 8 * r.numel(),
                      lambda: lib.dronesim_rewnorm_apply(y.data_ptr(), y.data_ptr(), T, E, N, norm.scale.data_ptr(), 10.0, stream()))]
            base = None
            for what, nbytes, fn in calls:
                if scope == "agent" and what != "dronesim_rewnorm_update":
                    continue                                   # (only the update's last launch depends on the groups)
                med, lo = timed(fn, what)
                line = dict(what=what, config=name, T=T, E=E, N=N, us=round(med, 2), us_min=round(lo, 2), bytes=nbytes,
                            tb_s=round(nbytes / 1e6 / med, 3), calls=args.calls, reps=args.reps)
                if what == "dronesim_returns":
                    base = med / nbytes
                else:
                    line.update(scope=scope)
                    if base is not None:
                        line.update(us_per_byte_ratio=round(med / nbytes / base, 3))
                if args.tag:
                    line["tag"] = args.tag
                lines.append(line)
                print(json.dumps(line), flush=True)
        del r, G, y, norm
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def gather_bench(args):
    """`dronesim_row_permutation` + `dronesim_gather_rows` of the five learner arrays next to a plain copy of the same bytes."""
    import ctypes as C
    import statistics

    import torch
    from scalable_collision_avoidance_rl_amd import _native
    from scalable_collision_avoidance_rl_amd.learner import GatheredRows
    lib, dev = _native.lib(), "cuda:0"
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []
    for name in args.configs.split(","):
        N, E, T, _ = CONFIGS[name]
        d_in, rows = 6, T * E
        K = 4 if args.minibatches is None else args.minibatches
        if rows % K:
            raise SystemExit(f"--minibatches {K} does not divide the {rows} rows of {name}")
        M = rows // K
        g = torch.Generator(device=dev).manual_seed(0)
        srcs = [torch.randn(rows, *s, device=dev, generator=g) for s in ((N, d_in), (N, 2), (N,), (N,), (N,))]
        mb = [GatheredRows(tuple(s.shape[1:]), K, M, dev) for s in srcs]
        plain = [torch.empty_like(s) for s in srcs]
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        perm = torch.empty(rows, dtype=torch.int32, device=dev)
        arr = lambda ty, vals: (ty * 5)(*vals)
        src_p, dst_p = arr(C.c_void_p, [s.data_ptr() for s in srcs]), arr(C.c_void_p, [m.buf.data_ptr() for m in mb])
        rb, bb = arr(C.c_int64, [m.row_bytes for m in mb]), arr(C.c_int64, [m.block_bytes for m in mb])
        permute = lambda: lib.dronesim_row_permutation(rows, 12345, counter.data_ptr(), perm.data_ptr(), stream())
        gather = lambda: lib.dronesim_gather_rows(perm.data_ptr(), rows, M, 5, src_p, dst_p, rb, bb, stream())

        def copy():
            for d, s_ in zip(plain, srcs):
                d.copy_(s_)
            return 0

        def both():
            return permute() or gather()

        nbytes = sum(s.numel() * 4 for s in srcs)
        _native.check(both(), "permutation + gather")
        torch.cuda.synchronize()
        assert all(torch.equal(torch.stack(m.blocks).reshape(s.shape), s[perm.long()]) for m, s in zip(mb, srcs))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        base = None
        for what, fn in (("plain copy of the five arrays", copy), ("dronesim_row_permutation", permute), ("dronesim_gather_rows", gather),
                         ("dronesim_row_permutation + dronesim_gather_rows", both)):
            for _ in range(max(1, args.warmup) * args.calls):
                _native.check(fn(), what)
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                ev[0].record()
                for _ in range(args.calls):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                us.append(ev[0].elapsed_time(ev[1]) * 1e3 / args.calls)
            med, lo = statistics.median(us), min(us)
            line = dict(what=what, config=name, N=N, R=rows, K=K, M=M, row_bytes=[m.row_bytes for m in mb], us=round(med, 2),
                        us_min=round(lo, 2), us_all=[round(u, 2) for u in us], calls=args.calls, reps=args.reps)
            if what != "dronesim_row_permutation":
                line.update(bytes_moved=2 * nbytes, tb_s=round(2 * nbytes / 1e6 / med, 3))
            if base is None:
                base = med
            else:
                line.update(ratio_to_copy=round(med / base, 3))
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def scans_time_limit(args):
    """`dronesim_lambda_returns_ends` next to its yardstick `dronesim_lambda_returns` (done = ends != 0), and `dronesim_episode_ends`."""
    import ctypes as C
    import statistics

    import torch
    from scalable_collision_avoidance_rl_amd import _native
    lib, dev = _native.lib(), "cuda:0"
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []
    for name in args.configs.split(","):
        N, E, T, _ = CONFIGS[name]
        d, M = 6, 1
        g = torch.Generator(device=dev).manual_seed(0)
        r = torch.randn(T, E, N, device=dev, generator=g)
        V = torch.randn(T + 1, E, N, device=dev, generator=g)
        Vend = torch.randn(M, E, N, device=dev, generator=g)
        at = torch.randint(0, T, (E,), device=dev, generator=g)                       # one truncated end per env at a random slot
        ends = (torch.arange(T, device=dev)[:, None] == at[None]).to(torch.uint8) * 2
        done = (ends != 0).to(torch.uint8)
        z_final = torch.ones(T, E, N, d, device=dev)                                  # every agent outside the goal disk
        out = (torch.empty_like(done), torch.empty(M, E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev),
               torch.empty(M, E, N, d, device=dev))
        G = torch.empty_like(r)
        lam = 0.95 if args.lam is None else args.lam
        calls = {"dronesim_lambda_returns G (done = ends != 0)": lambda: lib.dronesim_lambda_returns(
                     r.data_ptr(), done.data_ptr(), V.data_ptr(), 0.99, lam, G.data_ptr(), None, T, E, N, stream()),
                 "dronesim_lambda_returns_ends G": lambda: lib.dronesim_lambda_returns_ends(
                     r.data_ptr(), ends.data_ptr(), V.data_ptr(), Vend.data_ptr(), M, 0.99, lam, G.data_ptr(), None, T, E, N, stream()),
                 "dronesim_episode_ends": lambda: lib.dronesim_episode_ends(
                     done.data_ptr(), z_final.data_ptr(), T, E, N, d, 0.2, *[t.data_ptr() for t in out], M, stream())}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        base = None
        for what, fn in calls.items():
            for _ in range(max(1, args.warmup) * args.calls):
                _native.check(fn(), what)
            torch.cuda.synchronize()
            us = []
            for _ in range(args.reps):
                ev[0].record()
                for _ in range(args.calls):
                    fn()
                ev[1].record()
                torch.cuda.synchronize()
                us.append(ev[0].elapsed_time(ev[1]) * 1e3 / args.calls)
            med, lo = statistics.median(us), min(us)
            line = dict(what=what, config=name, N=N, E=E, T=T, M=M, us=round(med, 2), us_min=round(lo, 2), calls=args.calls, reps=args.reps)
            if what == "dronesim_episode_ends":
                assert torch.equal(out[0], ends) and int(out[2].sum()) == E
                line.update(bytes_read=T * E + E * N * d * 4 + T * E, bytes_written=T * E + M * E * 4 + E * 4 + M * E * N * d * 4)
            else:
                line.update(lam=lam, bytes_per_element=12, tb_s=round(r.numel() * 12 / 1e6 / med, 3))
                if base is None:
                    base = med
                else:       # the same bytes (+ M / T of one V stream): the yardstick plus 15 % (one more select and a counter, spread)
                    line.update(ratio=round(med / base, 3), allowed_us=round(base * 1.15, 2), inside=bool(med <= base * 1.15))
            if args.tag:
                line["tag"] = args.tag
            lines.append(line)
            print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def networks_of(torch, name, dev, g):
    """The seeded networks of one shape, drawn from the generator ``g``: (actor weights, actor kind, critic weights, widths)."""
    N, E, T, kind = CONFIGS[name]
    d_in = 6
    u = lambda *s, fan: (torch.rand(*s, device=dev, generator=g) * 2 - 1) / math.sqrt(fan)
    net = lambda h1, h2, no: [u(N, d_in, h1, fan=d_in), u(N, h1, fan=d_in), u(N, h1, h2, fan=h1), u(N, h2, fan=h1),
                              u(N, h2, no, fan=h2), u(N, no, fan=h2)]
    if kind == "softmax":
        aw, ak, widths = net(300, 300, 16), 1, (300, 300, 16)
    else:
        aw, ak, widths = net(400, 400, 4), 2, (400, 400, 4)
        aw[4][:, :200, 2:] = 0; aw[4][:, 200:, :2] = 0
    return aw, ak, net(200, 200, 1), widths


def window_of(torch, name, dev="cuda:0", lam=None, boot=False):
    """The seeded networks and the storage-like window of one shape: (actor weights, actor kind, critic weights, storage, widths)."""
    N, E, T, kind = CONFIGS[name]
    d_in = 6
    g = torch.Generator(device=dev).manual_seed(0)
    aw, ak, cw, widths = networks_of(torch, name, dev, g)
    ring = (torch.rand(T + (lam is not None), E, N, d_in, device=dev, generator=g) * 2 - 1) * 3
    a = torch.randint(0, 16, (T, E, N), device=dev, generator=g).float() * (2 * math.pi / 16)
    st = SimpleNamespace(z_pre=ring[:T], reward=torch.randn(T, E, N, device=dev, generator=g),
                         done=torch.zeros(T, E, dtype=torch.uint8, device=dev), actions=torch.stack([a.cos(), a.sin()], -1),
                         nbr_pre=torch.stack([torch.arange(N, device=dev).expand(T, E, N)] * 3, -1).int().contiguous())
    st.done[-1] = 1
    if lam is not None:        # the T+1-slot observation ring the bootstrap reads (`RolloutStorage.z_all`)
        st.z_all = ring
    if boot:                        # every episode ends at the window's last step with all agents outside the goal disk
        st.z_final = torch.ones(T, E, N, d_in, device=dev)
    return aw, ak, cw, st, widths


def critic_epoch_ms(torch, learner, st, reps):
    """A critic-only epoch of a whole-window `PPOLearner` that has trained once: its gradient chain + its Adam step (best of reps)."""
    T, E, N = learner._shape
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = []
    for _ in range(reps + 1):
        ev[0].record()
        if learner.vf_clip is not None:
            cg, _, _ = learner._critic_grad.run_vclip(st.z_pre, 1.0 / (T * E), learner.G, learner.V, learner.vf_clip)
        else:
            cg, _ = learner._critic_grad.run(st.z_pre, 1.0 / (T * E), target=learner.G)
        learner.critic_opt.step(cg, refresh=False)
        ev[1].record()
        torch.cuda.synchronize()
        times.append(ev[0].elapsed_time(ev[1]))
    return min(times[1:])


def gate_compare(args):
    """`PPOLearner.train` at 2 and 6 epochs, gated (target_kl = 1e-30: every agent stops on its second step) and not, alternating in
    one process after a warm-up, next to the critic-only epoch."""
    import statistics

    import torch
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    dev = "cuda:0"
    lines = []
    for name in args.configs.split(","):
        N, E, T, kind = CONFIGS[name]
        aw, ak, cw, st, _ = window_of(torch, name)
        runs = {}
        for what, kw in (("gated_2", dict(epochs=2, target_kl=1e-30)), ("gated_6", dict(epochs=6, target_kl=1e-30)),
                         ("plain_2", dict(epochs=2)), ("plain_6", dict(epochs=6))):
            actor = BatchedMLP(*[w.clone() for w in aw], ak, ak, device=dev)
            critic = BatchedMLP(*[w.clone() for w in cw], 0, 0, device=dev)
            runs[what] = PPOLearner(actor, critic, 0.99, **kw)
        for learner in runs.values():
            for _ in range(max(1, args.warmup)):
                learner.train(st)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = {k: [] for k in runs}
        for _ in range(args.reps):
            for what, learner in runs.items():
                ev[0].record(); out = learner.train(st); ev[1].record()
                torch.cuda.synchronize()
                times[what].append(ev[0].elapsed_time(ev[1]))
                if what.startswith("gated"):
                    assert out["actor_steps"].tolist() == [1] * N, out["actor_steps"]
        critic_ms = critic_epoch_ms(torch, runs["plain_2"], st, args.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        gated, plain = (med["gated_6"] - med["gated_2"]) / 4, (med["plain_6"] - med["plain_2"]) / 4
        line = dict(what="marginal epoch with every agent stopped", config=name, N=N, E=E, T=T, actor=kind,
                    ms={k: round(v, 3) for k, v in med.items()}, ms_all={k: [round(t, 3) for t in v] for k, v in times.items()},
                    gated_marginal_epoch_ms=round(gated, 3), plain_marginal_epoch_ms=round(plain, 3),
                    critic_epoch_ms=round(critic_ms, 3), allowed_ms=round(critic_ms * 1.15, 3), inside=bool(gated <= critic_ms * 1.15),
                    share_of_plain_epoch=round(gated / plain, 4), reps=args.reps)
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def adam_step_bench(args):
    """`BatchedAdam.step` alone (no gradient chain, ``refresh=False``): per repetition ``--calls`` back-to-back steps of the actor's
    and the critic's optimiser on fixed random gradients, between two device events.  ``--share all`` ties each network first
    and times the shared step.  The byte counts per element of a group of |G| members: unshared 36 |G| (the norm reads g; Adam
    reads and writes g, m1, m2, p), shared 8 |G| + 44 (every member's g read and p written, one 40-byte leader pass, one
    broadcast read); the line carries both and the bandwidth the measured time amounts to."""
    import statistics

    import torch
    from scalable_collision_avoidance_rl_amd.learner import BatchedAdam
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    dev = "cuda:0"
    lines = []
    for name in args.configs.split(","):
        N, E, T, kind = CONFIGS[name]
        g = torch.Generator(device=dev).manual_seed(0)
        aw, ak, cw, _ = networks_of(torch, name, dev, g)
        nets = [BatchedMLP(*aw, ak, ak, device=dev), BatchedMLP(*cw, 0, 0, device=dev)]
        kw = {}
        if args.share:
            kw["share"] = args.share
            for mlp in nets:
                mlp.tie_weights(args.share)
        opts = [BatchedAdam(mlp, **kw) for mlp in nets]
        grads = [torch.randn(o.numel, device=dev, generator=g) * 1e-3 for o in opts]
        keep = [t.clone() for t in grads]

        def steps(n):
            for _ in range(n):
                for o, t in zip(opts, grads):
                    o.step(t, refresh=False)
        steps(max(1, args.warmup))
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = []
        for _ in range(args.reps):
            for t, k in zip(grads, keep):          # (the step clips in place: every repetition starts from the same gradients)
                t.copy_(k)
            torch.cuda.synchronize()
            ev[0].record(); steps(args.calls); ev[1].record()
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]) / args.calls)
        elements = sum(o.numel for o in opts)        # all agents, both networks
        groups = 1 if args.share == "all" else N
        unshared_bytes, shared_bytes = 36 * elements, 8 * elements + 44 * elements // N * groups
        ms = statistics.median(times)
        moved = shared_bytes if args.share else unshared_bytes
        line = dict(what="BatchedAdam.step, actor + critic", config=name, N=N, actor=kind, share=args.share, elements=elements,
                    ms_per_step=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4),
                    ms_all=[round(t, 4) for t in times], calls=args.calls, unshared_bytes=unshared_bytes,
                    expected_bytes=moved, expected_share_of_unshared=round(moved / unshared_bytes, 4),
                    tb_per_s=round(moved / ms / 1e9, 3))
        if args.tag:
            line["tag"] = args.tag
        lines.append(line)
        print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c1,c3,c5")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--learner", choices=("sa2c", "ppo"), default="sa2c")
    ap.add_argument("--epochs", type=int, default=1, help="epochs per PPOLearner.train (--learner ppo)")
    ap.add_argument("--stats", help="a rocprofv3 kernel_stats.csv to summarise instead of running")
    ap.add_argument("--lam", type=float, default=None, help="bootstrapped lambda-returns with this lambda (default: off)")
    ap.add_argument("--time-limit", choices=("terminal", "bootstrap"), default="terminal",
                    help="bootstrap: time-limit ends bootstrap from their terminal observations (needs --lam; with --scans: the new scan)")
    ap.add_argument("--scans", action="store_true", help="time dronesim_returns / dronesim_lambda_returns instead of a learner")
    ap.add_argument("--standardize", action="store_true", help="with --scans: time dronesim_standardize against dronesim_returns")
    ap.add_argument("--obsnorm", action="store_true", help="with --scans: time dronesim_obsnorm_update / _apply against dronesim_returns")
    ap.add_argument("--rewnorm", action="store_true", help="with --scans: time dronesim_rewnorm_update / _apply next to dronesim_returns")
    ap.add_argument("--reward-norm", action="store_true", help="time the learner with a RewardNormalizer (update, apply, then the scans)")
    ap.add_argument("--obs-norm", action="store_true", help="time the learner with an ObsNormalizer (normalise first, update last)")
    ap.add_argument("--ent-coef", type=float, default=0.0, help="entropy bonus of the timed learner (default: off)")
    ap.add_argument("--normalize-advantage", action="store_true", help="per-agent advantage standardisation (--learner ppo)")
    ap.add_argument("--minibatches", type=int, default=None,
                    help="shuffled minibatches per epoch (--learner ppo; default 1: off); with --gather: the blocks (default 4; 1 = a single block)")
    ap.add_argument("--gather", action="store_true", help="time dronesim_row_permutation + dronesim_gather_rows against a plain copy")
    ap.add_argument("--target-kl", type=float, default=None, help="per-agent KL early stop of the actors (--learner ppo; default: off)")
    ap.add_argument("--vf-clip", type=float, default=None, help="clipped value loss with this range (--learner ppo; default: off)")
    ap.add_argument("--gate-compare", action="store_true",
                    help="gated against ungated PPOLearner.train at 2 and 6 epochs and the critic-only epoch, in one process")
    ap.add_argument("--share", choices=("all",), default=None,
                    help="parameter sharing: all agents train ONE actor and ONE critic (tied weights; default: off)")
    ap.add_argument("--adam-step", action="store_true", help="time BatchedAdam.step alone (actor + critic), unshared or with --share")
    ap.add_argument("--tag", help="a free label copied into the JSON lines (e.g. which build was timed)")
    ap.add_argument("--calls", type=int, default=20, help="back-to-back calls per timed repetition (--scans)")
    ap.add_argument("--out", help="append the JSON lines to this file")
    args = ap.parse_args()
    if args.normalize_advantage and args.learner != "ppo":
        ap.error("--normalize-advantage needs --learner ppo (SA2CLearner has no advantage standardisation)")
    if args.minibatches is not None and args.minibatches < 1:
        ap.error("--minibatches must be >= 1")
    if args.minibatches not in (None, 1) and not (args.gather or args.learner == "ppo"):
        ap.error("--minibatches needs --learner ppo (or --gather)")
    if not args.gather and args.minibatches is None:
        args.minibatches = 1
    if args.stats:
        import csv
        rows = list(csv.DictReader(open(args.stats)))
        tot = sum(float(r["TotalDurationNs"]) for r in rows)
        for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
            print(json.dumps(dict(kernel=r["Name"][:60], calls=int(r["Calls"]), total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3),
                                  share=round(float(r["TotalDurationNs"]) / tot, 4))))
        return
    if (args.target_kl is not None or args.vf_clip is not None) and args.learner != "ppo":
        ap.error("--target-kl and --vf-clip need --learner ppo")
    if args.adam_step:
        return adam_step_bench(args)
    if args.gate_compare:
        return gate_compare(args)
    if args.gather:
        return gather_bench(args)
    if args.scans and args.standardize:
        return scans_standardize(args)
    if args.scans and args.obsnorm:
        return scans_obsnorm(args)
    if args.scans and args.rewnorm:
        return scans_rewnorm(args)
    if args.scans:
        return scans_time_limit(args) if args.time_limit == "bootstrap" else scans(args)
    import torch
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    dev = "cuda:0"
    lines = []
    for name in args.configs.split(","):
        N, E, T, kind = CONFIGS[name]
        d_in = 6
        lam_kw = {} if args.lam is None else dict(lam=args.lam)
        boot = args.time_limit == "bootstrap"
        if boot:
            lam_kw["time_limit"] = "bootstrap"
        aw, ak, cw, st, (h1a, h2a, noa) = window_of(torch, name, dev, args.lam, boot)
        actor, critic = BatchedMLP(*aw, ak, ak, device=dev), BatchedMLP(*cw, 0, 0, device=dev)
        ppo = args.learner == "ppo"
        if args.ent_coef:
            lam_kw["ent_coef"] = args.ent_coef
        if args.normalize_advantage:
            lam_kw["normalize_advantage"] = True
        if args.minibatches > 1:
            lam_kw["minibatches"] = args.minibatches
        if args.target_kl is not None:
            lam_kw["target_kl"] = args.target_kl
        if args.vf_clip is not None:
            lam_kw["vf_clip"] = args.vf_clip
        if args.obs_norm:
            from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
            lam_kw["obs_norm"] = ObsNormalizer(N, d_in, dev)
        if args.reward_norm:
            from scalable_collision_avoidance_rl_amd.reward_norm import RewardNormalizer
            lam_kw["reward_norm"] = RewardNormalizer(N, 0.99, dev)
        if args.share:
            lam_kw["share"] = args.share
            actor.tie_weights(args.share); critic.tie_weights(args.share)
        learner = PPOLearner(actor, critic, 0.99, epochs=args.epochs, **lam_kw) if ppo else SA2CLearner(actor, critic, 0.99, **lam_kw)
        for _ in range(args.warmup):
            learner.train(st)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        times = []
        for _ in range(args.reps):
            ev[0].record(); learner.train(st); ev[1].record()
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]))
        rows = T * E * N
        step = mlp_flop(rows, d_in, 200, 200, 1) + mlp_flop(rows, d_in, h1a, h2a, noa)
        ring_rows = (T + 1) * E * N
        if ppo:     # per window: the old policy's and the critic's forward; per epoch: both gradient chains
            flop = (args.epochs * step + mlp_flop(rows, d_in, h1a, h2a, noa, False) +
                    mlp_flop(rows if args.lam is None else ring_rows, d_in, 200, 200, 1, False))
        else:       # (with --lam: one more critic forward, over the T+1 ring slots)
            flop = step + mlp_flop(rows, d_in, 200, 200, 1, False) + (0 if args.lam is None else mlp_flop(ring_rows, d_in, 200, 200, 1, False))
        ms = min(times)
        tag = dict(learner="ppo", epochs=args.epochs) if ppo else {}
        if args.lam is not None:
            tag["lam"] = args.lam
        if boot:
            tag["time_limit"] = "bootstrap"
        if args.ent_coef:
            tag["ent_coef"] = args.ent_coef
        if args.normalize_advantage:
            tag["normalize_advantage"] = True
        if args.minibatches > 1:
            tag["minibatches"] = args.minibatches
        if args.target_kl is not None:
            tag.update(target_kl=args.target_kl, actor_steps=[int(v) for v in (learner.actor_steps.min(), learner.actor_steps.max())])
        if args.vf_clip is not None:
            tag["vf_clip"] = args.vf_clip
        if args.obs_norm:
            tag["obs_norm"] = True
        if args.reward_norm:
            tag["reward_norm"] = True
        if args.share:
            tag["share"] = args.share
        if (args.target_kl is not None or args.vf_clip is not None) and args.minibatches == 1:
            tag["critic_epoch_ms"] = round(critic_epoch_ms(torch, learner, st, args.reps), 3)
        if args.tag:
            tag["tag"] = args.tag
        lines.append(dict(config=name, **tag, N=N, E=E, T=T, actor=kind, ms_per_update=round(ms, 3),
                          ms_all=[round(t, 3) for t in times], flop=flop, tflops=round(flop / ms / 1e9, 2),
                          peak_share=round(flop / ms / 1e9 / PEAK_TF, 4)))
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
