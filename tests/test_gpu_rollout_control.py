"""Closed-loop controller rollouts fused into one launch: `drones.rollout_control` / `dronesim_rollout_control`.

The action of step s is the classical controller's (/root/reference/drone_env.py:609-679) on the positions the env holds
before step s, computed inside the rollout launch.  Checked here, at the smallest shape of every geometry (packed, kSym64,
workgroup-per-env with a ragged wave, N = 256, N > 256), with and without `auto_reset` and the episode accumulator:

1. teacher-forced, step by step: the recorded in-kernel action is `env.control()`'s and the float64 oracle's;
2. one launch of T steps == launches of 1 + 7 + 32 steps == `rollout()` replaying the recorded actions, bit for bit
   (the comparison of tests/test_gpu_fuzz.py between a fused rollout and single steps);
3. the P-controller makes every env ARRIVE: `done` by arrival at the oracle's step index, the in-kernel reset, and the
   next action computed on the re-sampled positions;
4. the interface (compat mode, argument checks, the exported symbol);
5. c = 5: the velocity columns of the observation rows are the actions of THIS launch (they exist in LDS only), and the one
   documented size limit (c = 5 rows that do not fit the LDS tile) is an error that leaves the state untouched;
6. a captured graph replays the launch with its controller and u_max; non-finite coordinates stay inside their env.
tests/test_gpu_rollout_control_fuzz.py runs the comparison of 2. over seeded random shapes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import helpers as H

pytestmark = pytest.mark.gpu

# N, E, G, k, c, Delta kind ("uniform" | "hetero" | "none": the reference's default construction) -- and the code path each row reaches
SHAPES = {
    "packed5": (5, 300, 5.0, 2, 2, "uniform"),             # kPacked, several envs per wave, ragged last wave
    "hetero8": (8, 37, 8.0, 3, 5, "hetero"),               # heterogeneous deltas, k = 3, c = 5 (the FAR variant)
    "sym64": (64, 33, 28.0, 2, 2, "uniform"),              # kSym64
    "block70": (70, 9, 30.0, 2, 2, "uniform"),             # workgroup per env, ragged second wave
    "block256": (256, 4, 64.0, 2, 2, "uniform"),           # kBlock256 / kBlockU256
    "block300": (300, 2, 70.0, 2, 2, "uniform"),           # kBlock1024
    "sym64_c5": (64, 33, 28.0, 2, 5, "uniform"),           # kSym64 FAR: 5-column rows staged per wave, the waves' velocity blocks
    "sym64_default": (64, 33, 28.0, 2, 5, "none"),         # deltas=None, simplify_zstate=False: kSym64 FAR with far agents in the mask
    "block70_c5_hetero": (70, 9, 30.0, 3, 5, "hetero"),    # kBlock256 FAR, ragged wave, k = 3
    "block256_hetero": (256, 4, 64.0, 2, 2, "hetero"),     # kBlock256 proper (not kBlockU256)
    "block300_c5": (300, 2, 70.0, 2, 5, "uniform"),        # kBlock1024 FAR
    "packed5_k1": (5, 300, 5.0, 1, 2, "uniform"),          # the two ends of the k range
    "block70_k8": (70, 9, 30.0, 8, 2, "uniform"),
}
C5_SHAPES = ("hetero8", "sym64_c5", "sym64_default", "block70_c5_hetero", "block300_c5")
EPISODE_CFG = {"plain": {}, "acc": dict(track_episodes=True), "auto": dict(auto_reset=True, keep_final_obs=True)}
OUTPUTS = ("reward", "true_reward", "z", "nbr_idx", "n_coll", "done")
FINAL = ("z_final", "nbr_final", "pos_final")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def host(t):
    return t.detach().cpu().numpy()


def shape_deltas(name):
    N, _, _, _, _, kind = SHAPES[name]
    return {"uniform": np.ones(N), "hetero": np.linspace(0.3, 1.2, N), "none": None}[kind]


def make_env(name, cfg, seed=11):
    from scalable_collision_avoidance_rl_amd import drones
    N, E, G, k, c, _ = SHAPES[name]
    return drones(N, 0, [G, G], "O", k_closest=k, deltas=shape_deltas(name), simplify_zstate=(c == 2), n_envs=E,
                  batched=True, device="cuda:0", seed=seed, **EPISODE_CFG[cfg])


def make_oracle(name):
    N, _, G, k, c, _ = SHAPES[name]
    return Oracle(N, [G, G], k, shape_deltas(name), c == 2)


def box_start(name, seed):
    """Agents drawn uniformly in a box half the grid wide around its centre (float32, as the env stores them)."""
    N, E, G, _, _, _ = SHAPES[name]
    rng = np.random.default_rng(seed)
    return (G / 2 + (rng.random((E, N, 2)) - 0.5) * (G / 2)).astype(np.float32)


def gradient_masks(orc, pos64):
    """(safe [E,N], near count [E,N]): agents whose every d_ij is >= 1e-2 from 0 and from dhat_i, and how many partners
    their repulsion sum has (d_ij <= dhat_i)."""
    N = orc.N
    d = np.linalg.norm(pos64[:, :, None] - pos64[:, None], axis=-1) - orc.radius[None, :, None] - orc.radius[None, None, :]
    d[:, np.arange(N), np.arange(N)] = 1e9
    near = (d <= orc.d_hat[None, :, None]).sum(-1)
    safe = np.minimum(np.abs(d), np.abs(d - orc.d_hat[None, :, None])).min(axis=2) > 1e-2
    return safe, near


def arrival_start(name, seed):
    """Every agent at its goal plus an offset of radius U(0.25, 0.9) and a random angle."""
    N, E, G, _, _, _ = SHAPES[name]
    rng = np.random.default_rng(seed)
    r, ang = rng.uniform(0.25, 0.9, (E, N)), rng.uniform(0, 2 * np.pi, (E, N))
    xF = make_oracle(name).xF.reshape(N, 2)
    return (xF[None] + np.stack([r * np.cos(ang), r * np.sin(ang)], -1)).astype(np.float32)


def oracle_arrival(name, pos0, T):
    """Float64 closed loop (orc.proportional_control + orc.step): per env the first step whose `done` fires (-1: none)
    and whether its largest agent error at that step and at the step before is at least H.MARGIN from 0.2."""
    orc = make_oracle(name)
    N, E = orc.N, pos0.shape[0]
    xF = orc.xF.reshape(N, 2)
    pos = pos0.astype(np.float64).copy(); vel = np.zeros_like(pos); t = np.zeros(E, np.int32)
    err = [np.linalg.norm(pos - xF[None], axis=-1).max(1)]
    first = np.full(E, -1)
    for s in range(T):
        out = orc.step(pos, vel, t, orc.proportional_control(pos))
        err.append(np.linalg.norm(pos - xF[None], axis=-1).max(1))
        first[(out["done"] == 1) & (first < 0)] = s
    err = np.stack(err)                                       # err[s + 1] = after step s
    e = np.arange(E)
    at, before = err[first + 1, e], err[first, e]
    clear = (first >= 0) & (np.abs(at - 0.2) >= H.MARGIN) & (np.abs(before - 0.2) >= H.MARGIN)
    return first, clear


def same(torch, x, y):
    """The comparison of tests/test_gpu_fuzz.py: equal bit for bit, NaN matching NaN."""
    return torch.equal(x, y) or (x.is_floating_point() and torch.equal(torch.nan_to_num(x, nan=7.0), torch.nan_to_num(y, nan=7.0)))


# ---------------------------------------------------------------------------------------------- 1. the action
@pytest.mark.parametrize("cfg", list(EPISODE_CFG))
@pytest.mark.parametrize("kind", ["proportional", "gradient"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_in_kernel_action_is_the_controllers(torch, name, kind, cfg):
    """Teacher-forced (float32 drift and barrier thresholds cannot compound): at every step the action recorded by a
    one-step `rollout_control` is `env.control()`'s on the same state and the oracle's on `env.pos` read just before.
    Gradient: agents whose every d_ij is >= 1e-2 from 0 and from dhat_i, at the tolerance of the `dronesim_control`
    tests; the plain case runs unclipped (u_max = 1e4: the repulsion sum itself), the others clip at 0.7."""
    N, E, G, _, _, _ = SHAPES[name]
    T = 24
    u = 1.0 if kind == "proportional" else (1e4 if cfg == "plain" else 0.7)
    env, orc = make_env(name, cfg), make_oracle(name)
    # with auto_reset half of the envs hit the 200-step limit at step 9 and go on from re-sampled positions
    t0 = np.where(np.arange(E) % 2 == 0, 190, 0).astype(np.int32) if cfg == "auto" else np.zeros(E, np.int32)
    env.set_state(box_start(name, 100 + N), None, t0)
    episode0 = host(env.episode).copy()
    for s in range(T):
        a_ref = host(env.control(kind, u))
        pos64 = host(env.pos).astype(np.float64)
        out = env.rollout_control(kind, 1, u, record_actions=True)
        got = host(out["actions"][0])
        assert got.shape == (E, N, 2)
        if kind == "proportional":
            H.assert_close(got, a_ref, f"{name} {cfg} prop vs control() @{s}")
            H.assert_close(got, orc.proportional_control(pos64), f"{name} {cfg} prop vs oracle @{s}")
        else:
            safe, near = gradient_masks(orc, pos64)
            assert safe.mean() > 0.3 and (near[safe] > 0).mean() >= 0.05, (name, cfg, s, safe.mean(), (near[safe] > 0).mean())
            atol = H.ATOL + 0.1 * 2e-7 / 1e-2 ** 2 + 4 * float(np.spacing(np.float32(max(G, np.abs(pos64).max()))))
            H.assert_close(got[safe], a_ref[safe], f"{name} {cfg} grad vs control() @{s}", atol=atol)
            H.assert_close(got[safe], orc.gradient_control(pos64, u)[safe], f"{name} {cfg} grad vs oracle @{s}", atol=atol)
    if cfg == "auto":                                         # the envs that started at t = 190 were re-sampled in a launch
        assert np.array_equal(host(env.episode) - episode0, (t0 == 190).astype(np.int32))
        assert np.array_equal(host(env.t), np.where(t0 == 190, T - 10, T))
    else:
        assert np.array_equal(host(env.t), t0 + T)


# ---------------------------------------------------------------------------------------------- 2. splits and replay
@pytest.mark.parametrize("cfg", list(EPISODE_CFG))
@pytest.mark.parametrize("kind", ["proportional", "gradient"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_launch_equals_split_launches_equals_pool_replay(torch, name, kind, cfg):
    """(a) one launch of T = 40 steps, (b) launches of 1, 7 and 32 steps, (c) `rollout()` on the actions (a) recorded:
    every output, the final-observation buffers, the final state and the episode records agree bit for bit.  With
    `auto_reset` the envs start at t = 170 ... 195, so T spans a reset of every env."""
    N, E, G, _, _, _ = SHAPES[name]
    T = 40
    u = 1.0 if kind == "proportional" else 0.7
    rng = np.random.default_rng(7 + N)
    t0 = rng.integers(170, 196, E).astype(np.int32) if cfg == "auto" else np.zeros(E, np.int32)
    pos0 = box_start(name, 200 + N)
    envs = [make_env(name, cfg, seed=23) for _ in range(3)]
    for e in envs:
        e.set_state(pos0, None, t0)
    a = envs[0].rollout_control(kind, T, u, record_actions=True, with_pre=True)
    parts = [envs[1].rollout_control(kind, n, u, record_actions=True, with_pre=True) for n in (1, 7, 32)]
    b = {key: torch.cat([p[key] for p in parts], dim=0) for key in a}
    c = envs[2].rollout(a["actions"], with_pre=True)
    keys = OUTPUTS + ("z_pre", "nbr_idx_pre") + (FINAL if cfg == "auto" else ())
    for key in keys:
        assert a[key].shape[0] == T
        assert same(torch, a[key], b[key]), (name, kind, cfg, "split", key)
        assert same(torch, a[key], c[key]), (name, kind, cfg, "replay", key)
    assert same(torch, a["actions"], b["actions"]), (name, kind, cfg, "split actions")
    for other, what in ((envs[1], "split"), (envs[2], "replay")):
        for attr in ("pos", "vel", "t", "episode", "z", "nbr_idx", "reward", "true_reward", "n_coll", "done") + \
                    (("episode_acc",) if cfg != "plain" else ()) + (FINAL if cfg == "auto" else ()):
            assert same(torch, getattr(envs[0], attr), getattr(other, attr)), (name, kind, cfg, what, attr)
    # the live buffers are left as after rollout(): the last step's outputs
    assert same(torch, envs[0].z, a["z"][-1]) and same(torch, envs[0].done, a["done"][-1])
    # the velocity the env holds is the last action applied (drone_env.py:238), except where the last step re-sampled
    keep = host(a["done"][-1]) == 0 if cfg == "auto" else np.ones(E, bool)
    assert np.array_equal(host(envs[0].vel)[keep], host(a["actions"][-1])[keep])
    if cfg == "auto":
        assert int(a["done"].sum(0).min()) >= 1               # T spanned a reset of every env
    else:
        assert np.array_equal(host(envs[0].t), t0 + T)


# ---------------------------------------------------------------------------------------------- 3. arrival
@pytest.mark.parametrize("name", ["packed5", "sym64", "block70", "block256"])
def test_arrival_ends_episodes_at_every_geometry(torch, name):
    """P-controller from goal + U(0.25, 0.9) m offsets (inside 1 m the error shrinks by 0.95 per step: 0.9 m is under
    0.2 m within 30 steps), T = 60 with `auto_reset` and `keep_final_obs`: `done` fires for every env at some s < 40 --
    by arrival, the reduction over the env's agents being TRUE -- at the float64 oracle's step index wherever the oracle's
    largest agent error is H.MARGIN clear of 0.2 at that step and the one before (at most 10 % of the envs are not;
    about 2 % expected), the terminal positions lie within 0.2 of the goals, every `done` advanced the episode counter by
    one, and the action recorded at s + 1 is the controller's on the RE-SAMPLED positions (reconstructed from the goal-error
    row of the observation the reset wrote), not on the old ones.
    (The counter is compared with the env's number of `done` flags: an env re-sampled next to its goals can arrive a
    second time inside the 60 steps, a few of the 300 five-agent envs do.)"""
    N, E, G, k, c, _ = SHAPES[name]
    T = 60
    env, orc = make_env(name, "auto", seed=31), make_oracle(name)
    xF = orc.xF.reshape(N, 2)
    pos0 = arrival_start(name, 300 + N)
    first_ref, clear = oracle_arrival(name, pos0, T)
    assert (first_ref >= 0).all() and first_ref.max() < 40 and (~clear).mean() <= 0.10, (first_ref.max(), (~clear).mean())
    env.set_state(pos0, None, 0)
    episode0 = host(env.episode).copy()
    out = env.rollout_control("proportional", T, 1.0, record_actions=True)
    done = host(out["done"])
    assert done.any(0).all()
    first = done.argmax(0)
    assert first.max() < 40                                                       # well short of the 200-step limit
    assert np.array_equal(first[clear], first_ref[clear]), (name, np.flatnonzero(first != first_ref))
    e = np.arange(E)
    pos_final = host(out["pos_final"])[first, e].astype(np.float64)                # [E, N, 2]
    assert (np.linalg.norm(pos_final - xF[None], axis=-1)[clear] <= 0.2).all()
    assert np.array_equal(host(env.episode) - episode0, done.sum(0).astype(np.int32)) and done.sum(0).min() >= 1
    if N == 64:
        assert (done.sum(0) == 1).all()                       # (spread over a 28 m grid nobody arrives twice)
    # the observation written at step `first` is the new episode's first one: row 0 of z is x - xF
    z_new = host(out["z"])[first, e].reshape(E, N, k + 1, c)[:, :, 0, :2].astype(np.float64)
    pos_new = xF[None] + z_new
    act_next = host(out["actions"])[np.minimum(first + 1, T - 1), e]
    H.assert_close(act_next, orc.proportional_control(pos_new), f"{name}: action after the reset")
    stale = orc.proportional_control(pos_final)
    assert (np.abs(act_next - stale).max(axis=(1, 2)) > 0.1).all()


# ---------------------------------------------------------------------------------------------- 5. c = 5 rows, the limit
Z_VEL = slice(2, 4)     # a c = 5 row is (x, y, vx, vy, l): oracle/drone_oracle.c, `Zi[2] = vel[2 * i]` / `row[2] = vel[2 * j]`


@pytest.mark.parametrize("kind", ["proportional", "gradient"])
@pytest.mark.parametrize("name", C5_SHAPES)
def test_c5_rows_carry_the_actions_of_this_launch(torch, name, kind):
    """c = 5, T = 12 in one launch, no resets: the velocity an agent holds after step s is the action applied at step s
    (drone_env.py:238), so row 0 of agent i carries actions[s, e, i] and every real neighbour row (nbr_idx = j >= 0) carries
    actions[s, e, j] -- bit for bit, whatever geometry staged them.  (Ghost rows: left to the replay comparison.)"""
    N, E, G, k, c, _ = SHAPES[name]
    assert c == 5
    T = 12
    env = make_env(name, "plain")
    env.set_state(box_start(name, 400 + N), None, 0)
    out = env.rollout_control(kind, T, 1.0 if kind == "proportional" else 0.7, record_actions=True)
    z = host(out["z"]).reshape(T, E, N, k + 1, 5)
    nbr, act = host(out["nbr_idx"]).astype(np.int64), host(out["actions"])
    assert np.array_equal(nbr[..., 0], np.broadcast_to(np.arange(N), (T, E, N)))
    assert np.array_equal(z[:, :, :, 0, Z_VEL].view(np.uint32), act.view(np.uint32)), (name, kind, "row 0")
    real = nbr[..., 1:] >= 0                                                     # [T, E, N, k]
    assert real.mean() > 0.2, (name, real.mean())                                # (the box start keeps neighbours in range)
    s_, e_, i_, m_ = np.nonzero(real)
    want = act[s_, e_, nbr[s_, e_, i_, m_ + 1]]
    got = z[s_, e_, i_, m_ + 1][:, Z_VEL]
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    assert bad.size == 0, (name, kind, bad.size, "first (s, e, i, m):", s_[bad[0]], e_[bad[0]], i_[bad[0]], m_[bad[0]] + 1)
    assert len(np.unique(act[1:].reshape(T - 1, -1), axis=0)) == T - 1           # the actions do change from step to step


# csrc/dronesim.hip, launch(), at k = 8 without the episode layer: a wave of 64 agents takes 2 x 512 bytes of positions and
# constants, 4 x 64 x 6 x 9 = 13824 of staged 5-column rows, 1024 of cell tables and 512 of velocities = 16384 bytes, the
# workgroup 8 x 21 + 16 more.  Ten waves therefore fit the 160 KiB tile only while N stays under 640 (8 N bytes of positions
# and 8 N of velocities count by agent): 577 agents take 162528 bytes and run, 640 take 164024 and lose the staged rows, while
# their 2-column tile (89776 bytes) fits by far.
LIMIT_N, FIT_N, LIMIT_K = 640, 577, 8


def limit_env(N, c, E):
    from scalable_collision_avoidance_rl_amd import drones
    G = 0.25 * N + 6.0
    return drones(N, 0, [G, G], "O", k_closest=LIMIT_K, deltas=np.ones(N) * 0.3, simplify_zstate=(c == 2), n_envs=E,
                  batched=True, device="cuda:0", seed=5)


def test_c5_rows_beyond_the_lds_tile_are_refused(torch):
    """N = 640, k = 8: the env constructs at c = 5 and `rollout()` runs it (the rows leave as 4-byte stores), but the closed
    loop needs the partners' actions in LDS: `rollout_control` raises the documented error and leaves the state untouched.
    The same N and k at c = 2 run in closed loop, and so does the largest c = 5 tile of ten waves that still fits (N = 577,
    a ragged last wave): its launch of 3 steps equals the replay of its recorded actions and carries them in its rows."""
    from scalable_collision_avoidance_rl_amd import _native
    env = limit_env(LIMIT_N, 5, 2)
    pos, t = env.pos.clone(), env.t.clone()
    for kind in ("proportional", "gradient"):
        with pytest.raises(_native.DroneSimError) as ei:
            env.rollout_control(kind, 3, 1.0, record_actions=True)
        assert ei.value.code == _native.EUNSUPPORTED and "c = 5 rows" in str(ei.value) and "LDS tile" in str(ei.value)
    torch.cuda.synchronize()
    assert torch.equal(env.pos, pos) and torch.equal(env.t, t)
    out = env.rollout(torch.zeros(3, 2, LIMIT_N, 2, device="cuda:0"))            # the action pool serves this shape
    assert out["z"].shape == (3, 2, LIMIT_N, (LIMIT_K + 1) * 5) and int(env.t.min()) == 3
    env2 = limit_env(LIMIT_N, 2, 2)
    out = env2.rollout_control("gradient", 3, 1.0, record_actions=True)
    assert out["actions"].shape == (3, 2, LIMIT_N, 2) and int(env2.t.min()) == 3
    assert bool(torch.isfinite(out["actions"]).all()) and float(out["actions"].abs().max()) > 0
    a, b = limit_env(FIT_N, 5, 1), limit_env(FIT_N, 5, 1)
    assert torch.equal(a.pos, b.pos)
    out = a.rollout_control("gradient", 3, 1.0, record_actions=True)
    rep = b.rollout(out["actions"])
    for key in OUTPUTS:
        assert same(torch, out[key], rep[key]), key
    assert torch.equal(a.pos, b.pos) and torch.equal(a.vel, b.vel)
    z = out["z"].reshape(3, 1, FIT_N, LIMIT_K + 1, 5)
    assert torch.equal(z[:, :, :, 0, Z_VEL], out["actions"])
    j = out["nbr_idx"][..., 1:].long()                                           # [3, 1, N, k]
    partner = out["actions"][torch.arange(3, device="cuda:0")[:, None, None, None], 0, j.clamp(min=0)]   # [3, 1, N, k, 2]
    real = j >= 0
    assert bool(real.any()) and torch.equal(z[:, :, :, 1:, Z_VEL][real], partner[real])


# ---------------------------------------------------------------------------------------------- 6. graphs, non-finite input
def test_graph_replay_equals_eager(torch):
    """kSym64, gradient, T = 16 with `auto_reset` (every env passes the 200-step limit in the first or in the second
    replay): the launch captured in a graph (one kernel node; u_max and the controller bit travel in its arguments) and
    replayed twice equals, each time, the eager call from the same state -- outputs, recorded actions and the env's state."""
    N, E, G, _, _, _ = SHAPES["sym64"]
    T, u = 16, 0.7
    a, b = make_env("sym64", "auto", seed=41), make_env("sym64", "auto", seed=41)
    t0 = np.where(np.arange(E) % 2 == 0, 190, 176).astype(np.int32)
    pos0 = box_start("sym64", 500)
    for e in (a, b):
        e.set_state(pos0, None, t0)
    start = a.get_state()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.rollout_control("gradient", T, u, record_actions=True)                 # warm-up: what capture may not do happens here
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    a.load_state(start)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = a.rollout_control("gradient", T, u, record_actions=True)
    resets = 0
    for rep in range(2):
        graph.replay()
        ref = b.rollout_control("gradient", T, u, record_actions=True)
        for key in OUTPUTS + FINAL + ("actions",):
            assert same(torch, out[key], ref[key]), (rep, key)
        for attr in ("pos", "vel", "t", "episode", "episode_acc", "z", "nbr_idx", "done"):
            assert same(torch, getattr(a, attr), getattr(b, attr)), (rep, attr)
        resets += int(ref["done"].sum())
        assert float(ref["actions"].abs().max()) == pytest.approx(u)             # the clip is the one asked for
    assert resets == E and np.array_equal(host(b.episode) - host(start["episode"]), np.ones(E, np.int32))


POISON = (np.nan, np.inf, 1e30)


@pytest.mark.parametrize("name", ["sym64", "block70"])
def test_non_finite_coordinates_are_contained(torch, name):
    """The input family of tests/test_gpu_parity.py::test_non_finite_and_huge_coordinates_are_contained, in closed loop
    (gradient, T = 10): one agent of every fourth env starts at NaN, +inf or 1e30 in one coordinate.  The other envs' outputs
    are those of a run that has no such agent, bit for bit, and one launch equals single-step launches on ALL envs (NaN
    matching NaN): the candidate list of a poisoned env is never trusted."""
    N, E, G, _, _, _ = SHAPES[name]
    T, u = 10, 0.7
    pos = box_start(name, 600 + N)
    bad = pos.copy()
    dirty = np.arange(E) % 4 == 0
    for n, e in enumerate(np.flatnonzero(dirty)):
        bad[e, (3 * e + 1) % N, n % 2] = POISON[n % 3]
    clean_env, one, steps = make_env(name, "plain"), make_env(name, "plain"), make_env(name, "plain")
    clean_env.set_state(pos, None, 0); one.set_state(bad, None, 0); steps.set_state(bad, None, 0)
    ref = clean_env.rollout_control("gradient", T, u, record_actions=True)
    got = one.rollout_control("gradient", T, u, record_actions=True)
    parts = [steps.rollout_control("gradient", 1, u, record_actions=True) for _ in range(T)]
    torch.cuda.synchronize()
    keep = torch.as_tensor(np.flatnonzero(~dirty), device="cuda:0")
    for key in OUTPUTS + ("actions",):
        assert torch.equal(got[key].index_select(1, keep), ref[key].index_select(1, keep)), (name, "clean envs", key)
        assert bool(torch.isfinite(ref[key].float()).all()), key
        assert same(torch, got[key], torch.cat([p[key] for p in parts], dim=0)), (name, "single steps", key)
    for attr in ("pos", "vel", "t"):
        assert torch.equal(getattr(one, attr)[keep], getattr(clean_env, attr)[keep]), (name, attr)
        assert same(torch, getattr(one, attr), getattr(steps, attr)), (name, attr)
    nb = host(got["nbr_idx"])
    assert ((nb >= -1) & (nb < N)).all()


# ---------------------------------------------------------------------------------------------- 4. interface
def test_compat_mode_matches_steps(torch):
    """E = 1 (the reference's Python types): the dict comes back, and `env.state` / `internal_t` are left as T calls of
    `step(control())` leave them."""
    from scalable_collision_avoidance_rl_amd import drones
    N, G, T = 5, 5.0, 12
    mk = lambda: drones(N, 0, [G, G], "O", deltas=np.ones(N), simplify_zstate=True, seed=3)
    for kind, u in (("proportional", 1.0), ("gradient", 0.7)):
        a, b = mk(), mk()
        assert not a.batched and np.array_equal(a.state, b.state)
        out = a.rollout_control(kind, T, u, record_actions=True)
        assert out["actions"].shape == (T, 1, N, 2) and out["reward"].shape == (T, 1, N) and out["done"].shape == (T, 1)
        for s in range(T):
            acts = b.control(kind, u)
            H.assert_close(host(out["actions"][s, 0]), np.asarray(acts), f"compat {kind} action @{s}")
            b.step(acts)
        assert a.internal_t == b.internal_t == T
        assert isinstance(a.state, np.ndarray) and a.state.shape == (N, 5)
        H.assert_close(a.state, b.state, f"compat {kind} state")
        H.assert_close(np.asarray(a.z_states), np.asarray(b.z_states), f"compat {kind} z_states")
        assert a.Ni == b.Ni


def test_bad_arguments_raise(torch):
    from scalable_collision_avoidance_rl_amd import _native
    env = make_env("packed5", "plain")
    pos = env.pos.clone()
    with pytest.raises(ValueError):
        env.rollout_control("pid", 3)
    for u in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            env.rollout_control("gradient", 3, u)
    assert torch.equal(env.pos, pos)
    # the C entry point itself
    lib, p = _native.lib(), env._params()
    f32 = dict(dtype=torch.float32, device="cuda:0")
    N, E, K1 = env.n_agents, env.n_envs, env.k_closest + 1
    z, nb = torch.empty(1, E, N, K1 * 2, **f32), torch.empty(1, E, N, K1, dtype=torch.int32, device="cuda:0")
    dn = torch.empty(1, E, dtype=torch.uint8, device="cuda:0")
    call = lambda kind, u: lib.dronesim_rollout_control(
        C.byref(p), None, kind, u, env.pos.data_ptr(), env.vel.data_ptr(), env.t.data_ptr(), None, None, None,
        z.data_ptr(), nb.data_ptr(), None, dn.data_ptr(), E, 1, None)
    assert call(7, 1.0) == _native.EINVAL and call(-1, 1.0) == _native.EINVAL
    assert call(_native.CONTROL_GRADIENT, 0.0) == _native.EINVAL and call(_native.CONTROL_PROPORTIONAL, -2.0) == _native.EINVAL
    assert call(_native.CONTROL_GRADIENT, float("nan")) == _native.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(env.pos, pos) and int(env.t.max()) == 0
    # reward / true_reward / n_coll / act_out / ctl may be NULL: a plain one-step call on the default stream
    assert call(_native.CONTROL_PROPORTIONAL, 1.0) == _native.OK
    torch.cuda.synchronize()
    assert int(env.t.min()) == 1 and not torch.equal(env.pos, pos)


def test_symbol_is_exported(torch):
    from scalable_collision_avoidance_rl_amd import _native
    assert "dronesim_rollout_control" in _native.SYMBOLS
    assert getattr(_native.lib(), "dronesim_rollout_control") is not None
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    assert "dronesim_rollout_control" in [l.split()[-1] for l in out.splitlines() if l.strip()]
    assert "dronesim_rollout_control" in open(_native.HEADER_PATH).read()
