#!/usr/bin/env python3
"""Developer benchmark of the evaluation layer (csrc/evaluate.hip, evaluate.py), device events around hipGraph replays:

  1. `dronesim_episode_eval` on a stored window (with and without V; G written) next to its yardstick, `dronesim_returns` on
     the same rewards in the same session: the scan moves 16 B per element (12 B without V) against the yardstick's 8 B;
  2. `dronesim_episode_safety` on a stored window of observations next to `dronesim_episode_eval, G = NULL` on the same
     storage: expected = that line scaled by the bytes fetched, counted as whole 64-byte segments touched per record;
  3. one `Evaluator` round (softmax-16 actor + critic, f16x2) next to the bare loop of examples/rollout_loop.py part 2 (b)
     without the evaluation, and the same round with safety=True;
  4. `--shield` (alone: nothing of 1-3 runs): `dronesim_action_shield` on the env's own observation next to the step launch,
     `dronesim_control` and `dronesim_shield_totals` in the same session, and the control -> shield -> step(execute=) chain;
  5. `--obstacles` (alone): for M in {16, 64} discs, m = 2: the sense launch; sense + `dronesim_action_shield_obstacles` next to the
     plain `dronesim_action_shield` on the same observation; `dronesim_episode_obstacle_safety` next to `dronesim_episode_safety`
     on the same window; and the control -> sense -> shield -> step(execute=) chain next to the plain chain;
  6. `--obstacle-obs` (alone): for M in {16, 64} discs, m = 2: `dronesim_obstacle_observe` on one step next to the sense launch and
     on a T-step ring; `dronesim_obstacle_reward` on the window next to `dronesim_episode_obstacle_safety` on it; and
     ``SA2CLearner.train`` with and without ``obstacles=`` on a 16-step window;
  7. `--obstacles --per-env` (alone): per-env obstacle sets (csrc/env_obstacles.hip) next to the shared-list kernels in the same
     session, for M in {16, 64}, m = 2: sense, sense + obstacle shield, observe, reward, the tables and the control -> sense ->
     shield -> step(execute=) chain, each with its per-env : shared ratio; then, at M = 64, the two small-N shapes on either side
     of the staging rule (`dronesim_env_obstacle_plan` picks them): one takes the direct path, one the staged path.

    python tools/ebench.py [--T 200] [--envs 4096] [--agents 64] [--k 2] [--c 2] [--out profiles/ebench.jsonl] [--skip-round] [--tag LABEL]
    python tools/ebench.py --shield [--envs 4096] [--agents 64] [--k 2] [--c 2] [--out profiles/shield_ebench.jsonl]
    python tools/ebench.py --obstacles [--T 200] [--envs 4096] [--agents 64] [--k 2] [--c 2] [--out profiles/obstacles_ebench.jsonl]
    python tools/ebench.py --obstacles --per-env [--T 200] [--envs 4096] [--agents 64] [--out profiles/env_obstacles_ebench.jsonl]
    python tools/ebench.py --obstacle-obs [--T 200] [--envs 4096] [--agents 64] [--k 2] [--c 2] [--out profiles/obstacle_obs_ebench.jsonl]
Prints one JSON line per measurement (appended to --out when given).  DRONESIM_LIB selects the build."""
import argparse
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from scalable_collision_avoidance_rl_amd import _native, drones
from scalable_collision_avoidance_rl_amd.evaluate import Evaluator, episode_eval, episode_safety
from scalable_collision_avoidance_rl_amd.policies import BatchedMLP


def gtime(fn, calls=8, reps=9):
    """Median microseconds per call over `reps` replays of a graph of `calls` calls."""
    fn(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); g.replay(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3 / calls)
    return float(np.median(ts)), float(np.min(ts))


def kernels(T, E, N, emit):
    dev = "cuda:0"
    r, tr, V = (torch.randn(T, E, N, device=dev) for _ in range(3))
    n_coll = torch.randint(0, 3, (T, E), device=dev, dtype=torch.int32)
    done = torch.zeros(T, E, dtype=torch.uint8, device=dev); done[-1] = 1
    done[torch.randint(0, T, (E,), device=dev), torch.arange(E, device=dev)] = 1
    G = torch.empty_like(r)
    lib = _native.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    us_ret, lo_ret = gtime(lambda: _native.check(lib.dronesim_returns(r.data_ptr(), done.data_ptr(), 0.99, G.data_ptr(), T, E, N, stream()), "returns"))
    emit(dict(what="dronesim_returns", T=T, E=E, N=N, us=us_ret, us_min=lo_ret, bytes_per_element=8, tb_s=r.numel() * 8 / 1e6 / us_ret))
    full = episode_eval(r, tr, n_coll, done, V, 0.99)
    for name, v, nbytes in (("dronesim_episode_eval", V, 16), ("dronesim_episode_eval, V = NULL", None, 12)):
        out = {k: x for k, x in full.items() if v is not None or k != "mean_adv"}
        us, lo = gtime(lambda: episode_eval(r, tr, n_coll, done, v, 0.99, out=out))
        emit(dict(what=name, T=T, E=E, N=N, us=us, us_min=lo, bytes_per_element=nbytes, tb_s=r.numel() * nbytes / 1e6 / us,
                  yardstick_us=us_ret, expected_us=us_ret * nbytes / 8, allowed_us=us_ret * nbytes / 8 * 1.25,
                  within_allowance=bool(us <= us_ret * nbytes / 8 * 1.25)))
    tables = {k: x for k, x in full.items() if k != "G"}                              # what Evaluator asks for: G stays in registers
    us, lo = gtime(lambda: episode_eval(r, tr, n_coll, done, V, 0.99, out=tables))
    emit(dict(what="dronesim_episode_eval, G = NULL", T=T, E=E, N=N, us=us, us_min=lo, bytes_per_element=12, tb_s=r.numel() * 12 / 1e6 / us,
              yardstick_us=us_ret))
    return done, us


def segment_bytes(stride, ranges, records=4096):
    """Bytes fetched per record when consecutive records of `stride` bytes are read at the byte `ranges` [(lo, hi), ...] and
    memory moves in whole 64-byte-aligned segments."""
    touched = set()
    for i in range(records):
        for lo, hi in ranges:
            touched.update(range((i * stride + lo) // 64, (i * stride + hi - 1) // 64 + 1))
    return len(touched) * 64 / records


def safety(T, E, N, k, c, done, us_eval, emit):
    """`dronesim_episode_safety` with and without terminal observations; yardstick: `dronesim_episode_eval, G = NULL` (12 B per
    element) measured just before on the same `done`."""
    dev, k1 = "cuda:0", k + 1
    z, zf = (torch.randn(T, E, N, k1 * c, device=dev) * 0.3 for _ in range(2))
    nbr, nf = (torch.randint(-1, N, (T, E, N, k1), device=dev, dtype=torch.int32) for _ in range(2))
    radius, delta = torch.full((N,), 0.1, device=dev), torch.ones(N, device=dev)
    nbytes = segment_bytes(4 * k1 * c, [(0, 8), (4 * c, 4 * c + 8)]) + segment_bytes(4 * k1, [(4, 8)])
    for name, fin in (("dronesim_episode_safety", (None, None)), ("dronesim_episode_safety, z_final", (zf, nf))):
        out = episode_safety(z, nbr, done, radius, delta, *fin)
        us, lo = gtime(lambda: episode_safety(z, nbr, done, radius, delta, *fin, out=out))
        emit(dict(what=name, T=T, E=E, N=N, k=k, c=c, us=us, us_min=lo, bytes_per_element=nbytes, useful_bytes_per_element=20,
                  tb_s=T * E * N * nbytes / 1e6 / us, yardstick_us=us_eval, expected_us=us_eval * nbytes / 12,
                  allowed_us=us_eval * nbytes / 12 * 1.25, within_allowance=bool(us <= us_eval * nbytes / 12 * 1.25)))


def one_round(E, N, emit):
    G = 28.0 if N == 64 else max(6.0, 0.45 * N)
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * 0.2
    wa = [rnd(N, 6, 300), rnd(N, 300), rnd(N, 300, 300), rnd(N, 300), rnd(N, 300, 16), rnd(N, 16)]
    wc = [rnd(N, 6, 200), rnd(N, 200), rnd(N, 200, 200), rnd(N, 200), rnd(N, 200, 1), rnd(N, 1)]
    env = drones(N, 0, [G, G], "O", deltas=np.ones(N), simplify_zstate=True, n_envs=E, seed=0, auto_reset=True)
    actor = BatchedMLP(*wa, 1, 1, device=env.device, seed=1, precision="f16x2")
    critic = BatchedMLP(*wc, 0, 0, device=env.device, precision="f16x2")
    ev = Evaluator(env, actor, critic)
    ev.run(1)
    us_round, lo_round = gtime(lambda: ev.run(1), calls=1, reps=5)
    us_loop, lo_loop = gtime(ev.rollout, calls=1, reps=5)
    s = ev.summary()
    emit(dict(what="Evaluator round (softmax-16 + critic, f16x2)", T=ev.T, E=E, N=N, us=us_round, us_min=lo_round, bare_loop_us=us_loop,
              bare_loop_us_min=lo_loop, evaluation_us=us_round - us_loop, agent_steps_per_s=E * N * ev.T / (us_round * 1e-6),
              mean_return=s["mean_return"], mean_length=s["mean_length"], zero_collision_share=s["zero_collision_share"]))
    env2 = drones(N, 0, [G, G], "O", deltas=np.ones(N), simplify_zstate=True, n_envs=E, seed=0, auto_reset=True)
    ev2 = Evaluator(env2, actor, critic, safety=True)
    ev2.run(1)
    us_safe, lo_safe = gtime(lambda: ev2.run(1), calls=1, reps=5)
    s2 = ev2.safety_summary()
    emit(dict(what="Evaluator round, safety=True (softmax-16 + critic, f16x2)", T=ev2.T, E=E, N=N, us=us_safe, us_min=lo_safe,
              plain_round_us=us_round, safety_us=us_safe - us_round, **{k: v for k, v in s2.items() if k != "world_size"}))


def shield(E, N, k, c, emit):
    """`dronesim_action_shield` (rate 0.25, margin 0.05, box 1) on the observation of an env 20 proportional steps off the
    lattice, with the controller's action as the nominal one and with a random action in 1.5 x the box (most lanes solve);
    the step launch, the controller and the totals launch in the same session; then the three launches of a shielded step."""
    from scalable_collision_avoidance_rl_amd.shield import ActionShield
    G = 28.0 if N == 64 else max(6.0, 0.45 * N)
    env = drones(N, 0, [G, G], "O", k_closest=k, deltas=np.ones(N), simplify_zstate=c == 2, n_envs=E, seed=0, auto_reset=True)
    act, safe = env.control("proportional"), torch.empty(E, N, 2, device=env.device)
    for _ in range(20):
        env.step(env.control("proportional", out=act))
    wild = torch.rand(E, N, 2, device=env.device) * 3 - 1.5
    sh, shs = ActionShield(env, 0.25, 0.05, 1.0), ActionShield(env, 0.25, 0.05, 1.0, stats=True)
    k1 = k + 1
    nbytes = 4 * k1 * c + 4 * k1 + 8 + 8 + 1 + 4
    base = dict(E=E, N=N, k=k, c=c)
    for name, u in (("dronesim_action_shield, controller's action", act), ("dronesim_action_shield, random action in 1.5 x the box", wild)):
        us, lo = gtime(lambda: sh(u, out=safe))
        emit(dict(what=name, us=us, us_min=lo, bytes_per_record=nbytes, tb_s=E * N * nbytes / 1e6 / us,
                  intervention_share=float(sh.intervened.float().mean()), **base))
    us_both, lo_both = gtime(lambda: shs(act, out=safe))
    emit(dict(what="dronesim_action_shield + dronesim_shield_totals", us=us_both, us_min=lo_both, **base))
    us_ctl, lo_ctl = gtime(lambda: env.control("proportional", out=act))
    emit(dict(what="dronesim_control (proportional)", us=us_ctl, us_min=lo_ctl, **base))
    us_step, lo_step = gtime(lambda: env.step(wild))
    emit(dict(what="step launch (env.step, episode layer, auto_reset)", us=us_step, us_min=lo_step, **base))

    def chain():
        env.control("proportional", out=act)
        env.step(act, execute=sh(act, out=safe))
    us, lo = gtime(chain)
    emit(dict(what="control -> shield -> step(execute=)", us=us, us_min=lo, **base))
    us, lo = gtime(lambda: env.step(env.control("proportional", out=act)))
    emit(dict(what="control -> step", us=us, us_min=lo, **base))


def obstacles(T, E, N, k, c, emit, counts=(16, 64), m=2):
    """The obstacle layer on an env 20 proportional steps off the lattice (the shield measurement's state), `place_obstacles`'
    discs off the goals, the controller's action as the nominal one.  Every line carries its yardstick, measured in the same
    session: the plain shield launch, `dronesim_episode_safety` on the same window, the plain chain."""
    from scalable_collision_avoidance_rl_amd.obstacles import ObstacleField, episode_obstacle_safety, place_obstacles
    from scalable_collision_avoidance_rl_amd.shield import ActionShield
    G = 28.0 if N == 64 else max(6.0, 0.45 * N)
    dev, k1 = "cuda:0", k + 1
    env = drones(N, 0, [G, G], "O", k_closest=k, deltas=np.ones(N), simplify_zstate=c == 2, n_envs=E, seed=0, auto_reset=True)
    act, safe = env.control("proportional"), torch.empty(E, N, 2, device=env.device)
    for _ in range(20):
        env.step(env.control("proportional", out=act))
    plain = ActionShield(env, 0.25, 0.05, 1.0)
    us_plain, lo_plain = gtime(lambda: plain(act, out=safe))
    base = dict(E=E, N=N, k=k, c=c, m=m)
    emit(dict(what="dronesim_action_shield (yardstick)", us=us_plain, us_min=lo_plain, **base))

    def plain_chain():
        env.control("proportional", out=act)
        env.step(act, execute=plain(act, out=safe))
    us_chain, lo_chain = gtime(plain_chain)
    emit(dict(what="control -> shield -> step(execute=) (yardstick)", us=us_chain, us_min=lo_chain, **base))
    # the window of the tables: observations around the goals (row 0 = x - xF), every env ends once
    z = torch.randn(T, E, N, k1 * c, device=dev) * 3.0
    nbr = torch.randint(-1, N, (T, E, N, k1), device=dev, dtype=torch.int32)
    done = torch.zeros(T, E, dtype=torch.uint8, device=dev); done[-1] = 1
    radius, delta = env._radius, env._delta
    out_s = episode_safety(z, nbr, done, radius, delta)
    us_safety, lo_safety = gtime(lambda: episode_safety(z, nbr, done, radius, delta, out=out_s), calls=4)
    emit(dict(what="dronesim_episode_safety (yardstick)", T=T, us=us_safety, us_min=lo_safety, **base))
    zbytes = segment_bytes(4 * k1 * c, [(0, 8)])
    for M in counts:
        discs = place_obstacles([G, G], 2 * M, seed=M, keep_clear=env.end_points.reshape(N, 2), clearance=0.3)[:M]
        assert discs.shape[0] == M
        field = ObstacleField(env, discs, m=m)
        rec = dict(base, M=M)
        us, lo = gtime(lambda: field.sense(gap_min=True))
        emit(dict(what="dronesim_obstacle_sense (with gap_min, hit)", us=us, us_min=lo, slots_filled=float((field.oid >= 0).float().mean()),
                  hit_share=float(field.hit.float().mean()), **rec))
        field2 = ObstacleField(env, discs, m=m)
        us, lo = gtime(lambda: field2.sense())
        emit(dict(what="dronesim_obstacle_sense", us=us, us_min=lo, **rec))
        sh = ActionShield(env, 0.25, 0.05, 1.0, obstacles=field2)
        us, lo = gtime(lambda: sh(act, out=safe))
        emit(dict(what="dronesim_obstacle_sense + dronesim_action_shield_obstacles", us=us, us_min=lo, yardstick_us=us_plain,
                  ratio=us / us_plain, intervention_share=float(sh.intervened.float().mean()), **rec))
        out_o = episode_obstacle_safety(z, done, env._xF, radius, field.device_obstacles, c)
        us, lo = gtime(lambda: episode_obstacle_safety(z, done, env._xF, radius, field.device_obstacles, c, out=out_o), calls=4)
        emit(dict(what="dronesim_episode_obstacle_safety", T=T, us=us, us_min=lo, yardstick_us=us_safety, ratio=us / us_safety,
                  z_bytes_per_element=zbytes, z_tb_s=T * E * N * zbytes / 1e6 / us, gap_evaluations=T * E * N * M,
                  gaps_per_ns=T * E * N * M / 1e3 / us, **rec))

        def chain():
            env.control("proportional", out=act)
            env.step(act, execute=sh(act, out=safe))
        us, lo = gtime(chain)
        emit(dict(what="control -> sense -> shield -> step(execute=)", us=us, us_min=lo, yardstick_us=us_chain, ratio=us / us_chain, **rec))


def obstacle_obs(T, E, N, k, c, emit, counts=(16, 64), m=2, train_T=16):
    """Obstacle-aware training's two kernels next to their yardsticks, on `obstacles`' env state and discs: `observe` on one step
    next to `dronesim_obstacle_sense`; `observe` on the T + 1 slots of a ring; `shape_reward` on the T-step window next to
    `dronesim_episode_obstacle_safety` on it; and ``SA2CLearner.train`` on a ``train_T``-step window with and without the option
    (the same hidden sizes; the option's networks read d + 3m inputs)."""
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    from scalable_collision_avoidance_rl_amd.obstacles import ObstacleField, episode_obstacle_safety, place_obstacles
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    G = 28.0 if N == 64 else max(6.0, 0.45 * N)
    dev, k1 = "cuda:0", k + 1
    d = k1 * c
    env = drones(N, 0, [G, G], "O", k_closest=k, deltas=np.ones(N), simplify_zstate=c == 2, n_envs=E, seed=0, auto_reset=True)
    act = env.control("proportional")
    for _ in range(20):
        env.step(env.control("proportional", out=act))
    base = dict(E=E, N=N, k=k, c=c, m=m)
    # the window: the env's own positions jittered per slot, so that the lists are as full as on the env's observation
    ring = env.z.unsqueeze(0).repeat(T + 1, 1, 1, 1)
    ring[..., :2] += torch.randn(T + 1, E, N, 2, device=dev) * 0.3
    done = torch.zeros(T, E, dtype=torch.uint8, device=dev); done[-1] = 1
    reward = -torch.rand(T, E, N, device=dev)
    window = SimpleNamespace(env=env, z=ring[1:], z_final=None, done=done, reward=reward)

    def networks(d_in):
        gp = torch.Generator().manual_seed(0)
        rw = lambda *s: (torch.rand(*s, generator=gp) * 2 - 1) * 0.2
        wa = [rw(N, d_in, 48), rw(N, 48), rw(N, 48, 48), rw(N, 48), rw(N, 48, 16), rw(N, 16)]
        wc = [rw(N, d_in, 32), rw(N, 32), rw(N, 32, 32), rw(N, 32), rw(N, 32, 1), rw(N, 1)]
        return BatchedMLP(*wa, 1, 1, device=dev, seed=7), BatchedMLP(*wc, 0, 0, device=dev)

    st = RolloutStorage(env, train_T, actions=True)
    actor, critic = networks(d)
    st.begin()
    for t in range(train_T):
        actor.sample_action(env.z, env=env, act_out=st.actions[t])
        env.step(st.actions[t], into=(st, t))
    plain = SA2CLearner(actor, critic, 0.99)
    us_train, lo_train = gtime(lambda: plain.train(st), calls=1, reps=5)
    emit(dict(what="SA2CLearner.train (yardstick)", T=train_T, d_in=d, us=us_train, us_min=lo_train, **base))
    for M in counts:
        discs = place_obstacles([G, G], 2 * M, seed=M, keep_clear=env.end_points.reshape(N, 2), clearance=0.3)[:M]
        assert discs.shape[0] == M
        field = ObstacleField(env, discs, m=m)
        rec = dict(base, M=M)
        w = field.obs_width
        us_sense, lo_sense = gtime(lambda: field.sense())
        emit(dict(what="dronesim_obstacle_sense (yardstick)", us=us_sense, us_min=lo_sense, **rec))
        us, lo = gtime(lambda: field.observe())
        emit(dict(what="dronesim_obstacle_observe, one step", us=us, us_min=lo, yardstick_us=us_sense, ratio=us / us_sense,
                  bytes_written=4 * w * E * N, write_tb_s=4 * w * E * N / 1e6 / us, slots_filled=float((field.oid >= 0).float().mean()), **rec))
        us, lo = gtime(lambda: field.observe(cost=0.01))
        emit(dict(what="dronesim_obstacle_observe with cost, one step", us=us, us_min=lo, yardstick_us=us_sense, ratio=us / us_sense, **rec))
        x = torch.empty(T + 1, E, N, w, device=dev)
        us, lo = gtime(lambda: field.observe(ring, out=x), calls=2)
        emit(dict(what="dronesim_obstacle_observe, ring", T=T, us=us, us_min=lo, bytes_written=4 * w * (T + 1) * E * N,
                  write_tb_s=4 * w * (T + 1) * E * N / 1e6 / us, gaps_per_ns=(T + 1) * E * N * M / 1e3 / us, **rec))
        del x
        out_o = episode_obstacle_safety(ring[1:], done, env._xF, env._radius, field.device_obstacles, c)
        us_tab, lo_tab = gtime(lambda: episode_obstacle_safety(ring[1:], done, env._xF, env._radius, field.device_obstacles, c, out=out_o), calls=2)
        emit(dict(what="dronesim_episode_obstacle_safety (yardstick)", T=T, us=us_tab, us_min=lo_tab, **rec))
        shaped, cost = torch.empty_like(reward), torch.empty_like(reward)
        us, lo = gtime(lambda: field.shape_reward(window, 0.01, out=shaped, cost_out=cost), calls=2)
        emit(dict(what="dronesim_obstacle_reward", T=T, us=us, us_min=lo, yardstick_us=us_tab, ratio=us / us_tab,
                  gaps_per_ns=T * E * N * M / 1e3 / us, paying_share=float((cost > 0).float().mean()), **rec))
        actor_o, critic_o = networks(w)
        learner = SA2CLearner(actor_o, critic_o, 0.99, obstacles=field, obstacle_weight=0.01)
        us, lo = gtime(lambda: learner.train(st), calls=1, reps=5)
        emit(dict(what="SA2CLearner.train(obstacles=field)", T=train_T, d_in=w, us=us, us_min=lo, yardstick_us=us_train,
                  ratio=us / us_train, **rec))


def env_obstacles(T, E, N, k, c, emit, counts=(16, 64), m=2):
    """Per-env obstacle sets next to the shared-list kernels, on `obstacles`' env state: for every M the shared rows first (the
    yardstick, the rows of profiles/obstacles_ebench.jsonl), then the per-env rows with ``ratio`` = per-env : shared.  Env e's
    list is `place_obstacles` seeded ``[M, e]``, M discs each.  Then the small-N pair of the staging rule at M = 64."""
    from scalable_collision_avoidance_rl_amd.obstacles import ObstacleField, env_obstacle_plan, place_obstacles
    from scalable_collision_avoidance_rl_amd.shield import ActionShield
    G = 28.0 if N == 64 else max(6.0, 0.45 * N)
    dev, k1 = "cuda:0", k + 1
    env = drones(N, 0, [G, G], "O", k_closest=k, deltas=np.ones(N), simplify_zstate=c == 2, n_envs=E, seed=0, auto_reset=True)
    act, safe = env.control("proportional"), torch.empty(E, N, 2, device=env.device)
    for _ in range(20):
        env.step(env.control("proportional", out=act))
    base = dict(E=E, N=N, k=k, c=c, m=m)
    z = torch.randn(T, E, N, k1 * c, device=dev) * 3.0
    done = torch.zeros(T, E, dtype=torch.uint8, device=dev); done[-1] = 1
    window = SimpleNamespace(env=env, z=z, z_final=None, done=done, reward=-torch.rand(T, E, N, device=dev))
    shaped = torch.empty_like(window.reward)
    goals = env.end_points.reshape(N, 2)

    def rows(field, label, rec, yard):
        """The six rows of one field; `yard`: the shared field's medians by row name (None: this IS the yardstick)."""
        got = {}
        sh = ActionShield(env, 0.25, 0.05, 1.0, obstacles=field)
        tables = field.episode_safety(window)

        def chain():
            env.control("proportional", out=act)
            env.step(act, execute=sh(act, out=safe))
        for name, fn, calls in (("sense", lambda: field.sense(), 8), ("sense + obstacle shield", lambda: sh(act, out=safe), 8),
                                ("observe", lambda: field.observe(), 8),
                                ("reward", lambda: field.shape_reward(window, 0.01, out=shaped), 2),
                                ("tables", lambda: field.episode_safety(window, out=tables), 2),
                                ("control -> sense -> shield -> step(execute=)", chain, 8)):
            us, lo = gtime(fn, calls=calls)
            got[name] = us
            line = dict(what=f"{label}: {name}", us=us, us_min=lo, **rec)
            if name in ("reward", "tables"):
                line["T"] = T
            if yard is not None:
                line.update(yardstick_us=yard[name], ratio=us / yard[name])
            emit(line)
        return got

    for M in counts:
        discs = place_obstacles([G, G], 2 * M, seed=M, keep_clear=goals, clearance=0.3)[:M]
        assert discs.shape[0] == M
        rec = dict(base, M=M)
        yard = rows(ObstacleField(env, discs, m=m), "shared", rec, None)
        def own_list(e):                                       # M discs off the goals, from as many draws as it takes
            n = 2 * M
            while True:
                kept = place_obstacles([G, G], n, seed=[M, e], keep_clear=goals, clearance=0.3)
                if kept.shape[0] >= M:
                    return kept[:M]
                n *= 2
        per = np.stack([own_list(e) for e in range(E)])
        assert per.shape == (E, M, 3)
        plan = env_obstacle_plan(N, M, m)
        rows(ObstacleField(env, per, m=m, per_env=True), "per-env", dict(rec, staged=plan["staged"], list_bytes=12 * M * E), yard)
        del per
    # the staging rule at small N: the largest N the rule sends to the direct path and the next one, which it stages, at the same
    # M and about the same record count, on stand-in records (positions uniform over the discs' square)
    M, records = 64, 1 << 20
    n_direct = max(n for n in range(1, 65) if not env_obstacle_plan(n, M, m)["staged"])
    n_staged = n_direct + 1
    assert env_obstacle_plan(n_staged, M, m)["staged"]
    for n in (n_direct, n_staged):
        Es = records // n
        plan = env_obstacle_plan(n, M, m)
        g = torch.Generator(device=dev).manual_seed(n)
        stand_in = SimpleNamespace(batched=True, n_envs=Es, n_agents=n, k_closest=k, c=2, device=torch.device(dev), z=None,
                                   _xF=torch.zeros(n, 2, device=dev), _radius=torch.full((n,), 0.1, device=dev),
                                   _delta=torch.ones(n, device=dev), obstacles=np.zeros((0, 3)))
        lists = np.random.default_rng(n).uniform(0.0, 1.0, (Es, M, 3)) * np.array([G, G, 0.1 * G])
        field = ObstacleField(stand_in, lists, m=m, per_env=True)
        zs = torch.zeros(Es, n, k1 * 2, device=dev)
        zs[..., :2] = torch.rand(Es, n, 2, device=dev, generator=g) * G
        rec = dict(E=Es, N=n, k=k, c=2, m=m, M=M, staged=plan["staged"], rows_per_block=plan["rows_per_block"], list_bytes=12 * M * Es)
        for name, fn in (("sense", lambda: field.sense(zs)), ("observe", lambda: field.observe(zs)),
                         ("observe with cost", lambda: field.observe(zs, cost=0.01))):
            us, lo = gtime(fn)
            emit(dict(what=f"per-env, small N: {name}", us=us, us_min=lo, ns_per_record=1e3 * us / (Es * n), **rec))
        shared = ObstacleField(stand_in, lists[0], m=m)
        us, lo = gtime(lambda: shared.sense(zs))
        emit(dict(what="shared, small N: sense (yardstick)", us=us, us_min=lo, ns_per_record=1e3 * us / (Es * n), **dict(rec, staged=None)))
        del field, lists


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=200)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--agents", type=int, default=64)
    ap.add_argument("--k", type=int, default=2, help="k_closest of the safety window's records")
    ap.add_argument("--c", type=int, default=2, choices=(2, 5), help="floats per row of the safety window's records")
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-round", action="store_true")
    ap.add_argument("--shield", action="store_true", help="only the action shield next to the step launch")
    ap.add_argument("--obstacles", action="store_true", help="only the obstacle layer next to its yardsticks")
    ap.add_argument("--obstacle-obs", action="store_true", help="only the obstacle columns and the obstacle cost next to their yardsticks")
    ap.add_argument("--per-env", action="store_true", help="with --obstacles: the per-env obstacle sets next to the shared-list kernels")
    ap.add_argument("--tag", help="a free label copied into the JSON lines (e.g. which build was timed)")
    a = ap.parse_args()

    def emit(rec):
        if a.tag:
            rec["tag"] = a.tag
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
    if a.shield:
        shield(a.envs, a.agents, a.k, a.c, emit)
        return
    if a.per_env and not a.obstacles:
        ap.error("--per-env goes with --obstacles")
    if a.obstacles and a.per_env:
        env_obstacles(a.T, a.envs, a.agents, a.k, a.c, emit)
        return
    if a.obstacles:
        obstacles(a.T, a.envs, a.agents, a.k, a.c, emit)
        return
    if a.obstacle_obs:
        obstacle_obs(a.T, a.envs, a.agents, a.k, a.c, emit)
        return
    done, us_eval = kernels(a.T, a.envs, a.agents, emit)
    safety(a.T, a.envs, a.agents, a.k, a.c, done, us_eval, emit)
    if not a.skip_round:
        one_round(a.envs, a.agents, emit)


if __name__ == "__main__":
    main()
