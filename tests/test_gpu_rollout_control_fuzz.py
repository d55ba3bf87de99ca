"""Seeded fuzz of the closed-loop rollouts (`drones.rollout_control` / `dronesim_rollout_control`) over every kernel family:
k = 1..8, every geometry, c = 2 / 5, uniform / heterogeneous / default (`deltas=None`) Delta, the episode layer on and off,
both controllers, slow to teleporting `u_max`, sparse to crowded start boxes -- the shape distribution of
tests/test_gpu_fuzz.py::test_rollout_fuzz_against_step_launches with the action source inside the launch.

1. the fuzz: (a) one launch of T steps == (b) T launches of one step == (c) `rollout()` replaying the actions (a) recorded,
   bit for bit.  A launch of one step computes its action by the pass over ALL partners, so every step of (a) that walked a
   kept candidate list (several steps old, rebuilt in mid-rollout, crowded, ragged wave) is checked against an independent
   evaluation; (c) chains every output but the action to `rollout()`, which the suite holds to step launches and the oracle.
2. the chain of the action to the float64 oracle: teacher-forced over a subset of the same distribution, at the safe mask
   and the tolerance of tests/test_gpu_rollout_control.py::test_in_kernel_action_is_the_controllers.
   tests/test_rollout_control_host.py replays these draws through the oracle's own closed loop (no GPU) and proves that
   the mask leaves enough to compare.

Semantics guarded: the reference's drone_env.py:609-679 (the controllers), :235-238 (the integrator and the velocity)."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import helpers as H
from tests.test_gpu_rollout_control import FINAL, OUTPUTS, gradient_masks, host, same

pytestmark = pytest.mark.gpu

ORDINARY_N = [5, 24, 48, 64, 64, 65, 100, 128, 130, 192, 200, 250, 256, 256, 300]
BIG_N = [257, 300, 384, 512, 1024]
# the slow values keep a candidate list alive for many steps (0.05 m/s x 0.05 s against 0.49 x skin ~ 0.1 m); 1e4 is the
# unclipped repulsion sum: agents teleport, coordinates leave the cell tables, every step rebuilds
U_MAX = [0.05, 0.05, 0.05, 0.3, 0.3, 0.3, 1.0, 3.0, 1e4]
SLOW_U = 0.3
KEPT_STEPS = 5
# seed, iterations, N > 256 (the seeds of the open-loop fuzz; an iteration takes about 10 ms, so three times the 40 / 20 that
# would reach every counter below with hand-picked seeds only)
FUZZ_SEEDS = [(7, 120, False), (9, 120, False), (31, 120, False), (2026, 60, True), (2027, 60, True)]
# the chain to the oracle: start boxes and clips at which the float64 closed loop alone stays inside the compared share
# (tests/test_rollout_control_host.py::test_chain_draws_stay_inside_the_compared_share)
CHAIN_SEEDS = [(3, 12), (5, 12)]
CHAIN_BOX = (0.3, 0.7)
CHAIN_U = [0.3, 0.7, 1.0, 3.0]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def draw(rng, big_n, chain=False):
    """One iteration's shape, in the order the draws are made (the host-side test replays them).  None: the goal ring of
    this N and G leaves no safety distance (as the open-loop fuzz skips it)."""
    from scalable_collision_avoidance_rl_amd import formation_O
    N = int(rng.choice(BIG_N if big_n else ORDINARY_N))
    k = int(rng.integers(1, min(N - 1, 8) + 1))
    c = int(rng.choice([2, 2, 2, 5]))
    G = float(rng.choice([0.25, 0.45, 1.0])) * N + 6.0
    d_hat = formation_O(N, [G, G])[1]
    kind = str(rng.choice(["uniform", "uniform", "hetero", "none"]))
    deltas = (np.ones(N) * float(rng.uniform(0.2, 0.95)) * d_hat.min() if kind == "uniform"
              else rng.uniform(0.1, 1.3, N) * d_hat.min() if kind == "hetero" else None)
    E = int(rng.integers(1, 13)) if N <= 130 else int(rng.integers(1, 7)) if N <= 300 else int(rng.integers(1, 4))
    T = int(rng.integers(12, 31)) if big_n else int(rng.integers(20, 61))
    auto = bool(rng.integers(0, 2))
    track = bool(rng.integers(0, 3) == 0)
    ctrl = str(rng.choice(["gradient", "gradient", "gradient", "proportional"]))
    u_max = float(rng.choice(CHAIN_U if chain else U_MAX))
    box = float(rng.uniform(*(CHAIN_BOX if chain else (0.1, 0.9)))) * G
    pos0 = (G / 2 + (rng.random((E, N, 2)) - 0.5) * box).astype(np.float32)
    t0 = rng.integers(150, 199, E).astype(np.int32) if auto else np.zeros(E, np.int32)
    if d_hat.min() <= 0.05:
        return None
    if chain:                                                 # teacher-forced against the oracle: no in-kernel resets,
        auto, t0 = False, np.zeros(E, np.int32)               # and the oracle's P-controller clips at the reference's 1.0
        u_max = 1.0 if ctrl == "proportional" else u_max
    return dict(N=N, k=k, c=c, G=G, kind=kind, deltas=deltas, E=E, T=T, auto=auto, track=track, ctrl=ctrl, u_max=u_max,
                box=box, pos0=pos0, t0=t0)


def make(d, seed):
    from scalable_collision_avoidance_rl_amd import drones
    kw = dict(auto_reset=True, keep_final_obs=True) if d["auto"] else dict(track_episodes=d["track"])
    return drones(d["N"], 0, [d["G"], d["G"]], "O", k_closest=d["k"], deltas=d["deltas"], simplify_zstate=(d["c"] == 2),
                  n_envs=d["E"], batched=True, device="cuda:0", seed=seed, **kw)


def geometry_class(env):
    """(class, keeps a candidate list between steps) by the rules of csrc/dronesim.hip, launch(): "packed" N < 64, "sym64"
    N == 64 with uniform constants, "block" 65..256, "u256" N == 256 uniform without far agents, "big" N > 256 ("wave64": 64
    agents with per-agent constants, one env per wave of the packed kernel).  The list is kept where no far agent matters:
    c == 2 and max Delta < min d_hat, in the classes sym64, block and u256."""
    p, N = env._params(), env.n_agents
    uniform = p.d_hat_min == p.d_hat_max and p.delta_min == p.delta_max and p.radius_min == p.radius_max
    far = env.c == 5 or not (p.delta_max < p.d_hat_min)
    cls = ("packed" if N < 64 else ("sym64" if uniform else "wave64") if N == 64 else "big" if N > 256
           else "u256" if (N == 256 and uniform and not far) else "block")
    return cls, (not far) and cls in ("sym64", "block", "u256")


def kept_run(pos, skin):
    """Longest run of consecutive steps over which some env's candidate list stays valid, as the kernel keeps it: taken on the
    positions a step leaves (pos[s], s >= 1), kept while every agent of the env is within 0.49 x skin of where it stood then,
    taken anew on the first positions that are not.  pos: [T + 1, E, N, 2] float64."""
    best = 0
    for e in range(pos.shape[1]):
        ref, run = pos[1, e], 0
        for s in range(2, pos.shape[0]):
            if np.linalg.norm(pos[s, e] - ref, axis=-1).max() <= 0.49 * skin:
                run += 1
                best = max(best, run)
            else:
                ref, run = pos[s, e], 0
    return best


def first_step_that_differs(torch, x, y):
    nz = lambda v: torch.nan_to_num(v, nan=7.0) if v.is_floating_point() else v
    return int((nz(x) != nz(y)).reshape(x.shape[0], -1).any(1).nonzero()[0])


@pytest.mark.parametrize("seed,iters,big_n", FUZZ_SEEDS)
def test_closed_loop_fuzz_one_launch_equals_step_launches_equals_replay(torch, seed, iters, big_n):
    from scalable_collision_avoidance_rl_amd import _native
    rng = np.random.default_rng(seed)
    differs = lambda x, y: first_step_that_differs(torch, x, y)
    ran, resets, kept = 0, 0, 0
    classes, ctrls, ks = set(), set(), set()
    c5_outside_packed = none_outside_packed = False
    for it in range(iters):
        d = draw(rng, big_n)
        if d is None:
            continue
        N, k, c, E, T, auto, ctrl, u = d["N"], d["k"], d["c"], d["E"], d["T"], d["auto"], d["ctrl"], d["u_max"]
        tag = (f"seed {seed} it {it}: N {N} k {k} c {c} Delta {d['kind']} E {E} T {T} auto_reset {auto} track {d['track']} "
               f"{ctrl} u_max {u} box {d['box'] / d['G']:.2f} G")
        try:
            envs = [make(d, 100 + it) for _ in range(3)]
        except Exception as ex:                                # the one documented size limit (LDS tile at N ~ 1024, k = 8)
            assert "160 KiB LDS tile" in str(ex) and N > 900, f"{tag} | {ex}"
            continue
        for e in envs:
            e.set_state(d["pos0"], None, d["t0"])
        try:
            a = envs[0].rollout_control(ctrl, T, u, record_actions=True, with_pre=True)
        except _native.DroneSimError as ex:
            # closed loop refused: only for the LDS tile, and only where the action pool is refused too or N > 900
            assert ex.code == _native.EUNSUPPORTED and "LDS tile" in str(ex), f"{tag} | {ex}"
            try:
                envs[2].rollout(torch.zeros(1, E, N, 2, device="cuda:0"))
                pool_refused = False
            except _native.DroneSimError:
                pool_refused = True
            assert pool_refused or N > 900, f"{tag} | {ex}"
            continue
        pos = [envs[1].pos.clone()]
        parts = []
        for s in range(T):
            parts.append(envs[1].rollout_control(ctrl, 1, u, record_actions=True, with_pre=True))
            pos.append(envs[1].pos.clone())
        b = {key: torch.cat([p[key] for p in parts], dim=0) for key in a}
        r = envs[2].rollout(a["actions"], with_pre=True)
        for key in OUTPUTS + ("z_pre", "nbr_idx_pre") + (FINAL if auto else ()):
            assert a[key].shape[0] == T
            for other, what in ((b, "steps"), (r, "replay")):
                assert same(torch, a[key], other[key]), f"{tag} | {what} | {key} | first at step {differs(a[key], other[key])}"
        assert same(torch, a["actions"], b["actions"]), f"{tag} | steps | actions | first at step {differs(a['actions'], b['actions'])}"
        for other, what in ((envs[1], "steps"), (envs[2], "replay")):
            for attr in ("pos", "vel", "t", "episode") + (("episode_acc",) if envs[0].episode_acc is not None else ()):
                assert same(torch, getattr(envs[0], attr), getattr(other, attr)), f"{tag} | {what} | {attr} at the end"
        # ---- what this iteration covered
        cls, keeps = geometry_class(envs[0])
        ran += 1
        resets += int(a["done"].sum()) if auto else 0
        classes.add(cls); ctrls.add(ctrl); ks.add(k)
        c5_outside_packed |= c == 5 and cls != "packed"
        none_outside_packed |= d["kind"] == "none" and cls != "packed"
        if keeps and ctrl == "gradient" and u <= SLOW_U:
            p = envs[0]._params()
            skin = 0.4 * (p.d_hat_max + 2.0 * p.radius_max)
            kept += kept_run(host(torch.stack(pos)).astype(np.float64), skin) >= KEPT_STEPS
    counters = dict(ran=ran, resets=resets, classes=sorted(classes), ctrls=sorted(ctrls), ks=sorted(ks),
                    c5_outside_packed=c5_outside_packed, none_outside_packed=none_outside_packed, kept=kept)
    print("closed-loop fuzz seed", seed, counters)
    assert ran >= iters * 2 // 3 and resets > 0, counters
    assert ctrls == {"gradient", "proportional"} and c5_outside_packed and none_outside_packed, counters
    assert 1 in ks and max(ks) >= 6, counters
    if big_n:
        assert classes == {"big"}, counters
    else:
        assert classes >= {"packed", "sym64", "block", "u256", "big"}, counters
        # a kept list: the gradient controller walked, for >= 5 consecutive steps, a list taken earlier
        assert kept >= 5, counters


@pytest.mark.parametrize("seed,iters", CHAIN_SEEDS)
def test_closed_loop_fuzz_action_against_the_oracle(torch, seed, iters):
    """Teacher-forced, as test_in_kernel_action_is_the_controllers: at every step of single-step launches the recorded action
    is the float64 oracle's on `env.pos` read just before.  Gradient: on that test's safe mask, at its tolerance, under its cap
    on what the mask may leave out."""
    rng = np.random.default_rng(seed)
    ran, ctrls = 0, set()
    for it in range(iters):
        d = draw(rng, False, chain=True)
        if d is None:
            continue
        N, G, ctrl, u = d["N"], d["G"], d["ctrl"], d["u_max"]
        tag = f"seed {seed} it {it}: N {N} k {d['k']} c {d['c']} Delta {d['kind']} E {d['E']} T {d['T']} {ctrl} u_max {u}"
        env = make(d, 100 + it)
        orc = Oracle(N, [G, G], d["k"], d["deltas"], d["c"] == 2)
        env.set_state(d["pos0"], None, d["t0"])
        for s in range(d["T"]):
            pos64 = host(env.pos).astype(np.float64)
            got = host(env.rollout_control(ctrl, 1, u, record_actions=True)["actions"][0])
            if ctrl == "proportional":
                H.assert_close(got, orc.proportional_control(pos64), f"{tag} prop vs oracle @{s}")
            else:
                safe, near = gradient_masks(orc, pos64)
                share, busy = safe.mean(), (near[safe] > 0).mean()
                assert share > 0.3 and busy >= 0.05, f"{tag} @{s}: safe share {share:.3f}, with a repulsion sum {busy:.3f}"
                atol = H.ATOL + 0.1 * 2e-7 / 1e-2 ** 2 + 4 * float(np.spacing(np.float32(max(G, np.abs(pos64).max()))))
                H.assert_close(got[safe], orc.gradient_control(pos64, u)[safe], f"{tag} grad vs oracle @{s}", atol=atol)
        assert np.array_equal(host(env.t), d["t0"] + d["T"])
        ran += 1
        ctrls.add(ctrl)
    assert ran >= iters * 2 // 3 and ctrls == {"gradient", "proportional"}, (ran, ctrls)
