"""GPU tests of the per-env obstacle sets (include/dronesim_env_obstacles.h, csrc/env_obstacles.hip) through
``ObstacleField(per_env=True)``, at the smallest shapes at which each thing can go wrong (tests/env_obstacle_ref.py has the table
and the reasons; tests/test_env_obstacles_host.py asserts them and that the table reaches the staged AND the direct path):
  1. the same list in every env equals the shared field bit for bit (the yardstick is code from before the per-env kernels);
  2. different lists: per env the shared kernels run with that env's list, bit for bit, and the float64 per-env restatement at
     the shared tests' bars (ids, hits, counts exact; rows / gaps / costs within the standing 1e-5; the cost also inside the
     derived bound of tests/obstacle_obs_ref.py);
  3. ragged counts with a hitting disc planted in every row at or beyond an env's count;
  4. rows and wraps: a ring and a block of rows against the one-row call, the shaped reward over a window, bases off alignment;
  5. capture and determinism;
  6. through the stack: the shield's guarantee per env on a real env, the Evaluator's tables, one train() of each learner."""
import types

import numpy as np
import pytest

from tests import env_obstacle_ref as ER
from tests import obstacle_obs_ref as OO
from tests import obstacle_ref as OR
from tests import shield_ref as S
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WEIGHT = 0.01
K, C = 1, 2                                                  # k1 = 2, c = 2: an aligned z takes the 16-byte row-0 load


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def host(t):
    return t.detach().cpu().numpy()


def dev(torch, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def same(torch, a, b):
    """Bit for bit (NaNs and signed zeros included)."""
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return a.shape == b.shape and bool(torch.equal(a, b))


def stand_in_env(torch, cs, E, k=K, c=C):
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)
    return types.SimpleNamespace(batched=True, n_envs=E, n_agents=cs["xF"].shape[0], k_closest=k, c=c, device=torch.device("cuda", 0),
                                 z=None, nbr_idx=None, _radius=t(cs["radius"]), _xF=t(cs["xF"]), _delta=t(cs["sense"]),
                                 obstacles=np.zeros((0, 3)))


def per_env_field(torch, cs, m, k=K, c=C, env=None):
    from scalable_collision_avoidance_rl_amd import ObstacleField
    env = stand_in_env(torch, cs, cs["obstacles"].shape[0], k, c) if env is None else env
    return ObstacleField(env, cs["obstacles"], m=m, per_env=True, counts=cs["counts"])


def shared_field(torch, cs, discs, m, E, k=K, c=C):
    from scalable_collision_avoidance_rl_amd import ObstacleField
    return ObstacleField(stand_in_env(torch, cs, E, k, c), np.asarray(discs, np.float64).reshape(-1, 3), m=m)


def storage_of(torch, field, w):
    t = lambda a: dev(torch, a)
    zbuf = t(w["z_all"])
    T = w["reward"].shape[0]
    return types.SimpleNamespace(env=field.env, zbuf=zbuf, z=zbuf[1:], z_pre=zbuf[:T], z_all=zbuf, z_final=t(w["z_final"]),
                                 done=t(w["done"]), reward=t(w["reward"]))


def outputs(torch, field, z, st=None):
    """Every output of sense (with the planes), observe (with the cost) and -- with a storage -- shape_reward (with cost_out)."""
    field.sense(z, gap_min=True)
    out = [field.orow.clone(), field.oid.clone(), field.gap_min.clone(), field.hit.clone(), field.observe(z, cost=WEIGHT).clone(),
           field.cost.clone()]
    if st is not None:
        cost = torch.empty_like(st.reward)
        out += [field.shape_reward(st, WEIGHT, cost_out=cost).clone(), cost]
    return out


NAMES = ("orow", "oid", "gap_min", "hit", "x", "cost", "shaped reward", "reward cost")
WITH_DISCS = [(s, st) for s, st, _ in ER.SHAPES if s[2] > 0]


# ------------------------------------------------------------------------------------------ 1. the same list in every env
@pytest.mark.parametrize("shape,staged", WITH_DISCS, ids=[str(s) for s, _ in WITH_DISCS])
def test_same_list_in_every_env_is_the_shared_field_bit_for_bit(torch, shape, staged):
    from scalable_collision_avoidance_rl_amd.obstacles import env_obstacle_plan
    E, N, M, m = shape
    assert env_obstacle_plan(N, M, m)["staged"] == staged
    w = ER.reward_window(E, N, M, same_list=True)
    per, sh = per_env_field(torch, w, m), shared_field(torch, w, w["obstacles"][0], m, E)
    z = dev(torch, w["z"])
    got, want = outputs(torch, per, z, storage_of(torch, per, w)), outputs(torch, sh, z, storage_of(torch, sh, w))
    torch.cuda.synchronize()
    for name, a, b in zip(NAMES, got, want):
        assert same(torch, a, b), (shape, name)
    assert int((got[1] >= 0).sum()) > 0 and float(got[5].max()) > 0                # lists and costs are not empty


@pytest.mark.parametrize("window,M", ER.WINDOW_SHAPES, ids=[str(s) for s, _ in ER.WINDOW_SHAPES])
@pytest.mark.parametrize("c", [2, 5])
def test_same_list_tables_are_the_shared_tables_bit_for_bit(torch, window, M, c):
    from scalable_collision_avoidance_rl_amd.obstacles import episode_env_obstacle_safety, episode_obstacle_safety
    T, E, N = window
    w = ER.window_case(T, E, N, M, c=c, same_list=True)
    t = lambda a: dev(torch, a)
    args = (t(w["z"]), t(w["done"]), t(w["xF"]), t(w["radius"]))
    for zf in (t(w["z_final"]), None):
        got = episode_env_obstacle_safety(*args, t(w["obstacles"]), None, c, zf)
        want = episode_obstacle_safety(*args, t(w["obstacles"][0]), c, zf)
        torch.cuda.synchronize()
        for name in OR.TABLES:
            assert same(torch, got[name], want[name]), (window, c, name)
    assert int(want["obstacle_hit_steps"].sum()) > 0


# ------------------------------------------------------------------------------------------ 2. different lists per env
def check_against_restatement(torch, cs, field, m, what):
    """The field's sense / observe outputs of cs["z"] against the per-env restatement, at the shared tests' bars."""
    E, N = cs["z"].shape[:2]
    z = dev(torch, cs["z"])
    orow, oid, gm, hit, x, cost = (host(a) for a in outputs(torch, field, z))
    ref = ER.sense(cs, m)
    assert oid.dtype == np.int32 and np.array_equal(oid, ref["oid"]), what
    assert_close(orow, ref["orow"], what + " orow")
    inf = np.isinf(ref["gap_min"])
    assert np.array_equal(gm[inf], ref["gap_min"][inf].astype(np.float32)), what
    assert_close(gm[~inf], ref["gap_min"][~inf], what + " gap_min")
    assert hit.dtype == np.uint8 and np.array_equal(hit.astype(bool), ref["hit"]), what
    assert (oid < cs["counts"][:, None, None]).all() and (orow[oid < 0] == 0).all(), what
    # the columns are the restatement's bits; the cost within 1e-5 and inside its derived bound
    assert np.array_equal(x.view(np.uint32), ER.columns(cs, m).view(np.uint32)), what
    want, bound = ER.cost(cs, WEIGHT)
    err = np.abs(cost.astype(np.float64) - want)
    print(f"{what}: cost error / bound, largest {np.max(err / np.maximum(bound, 1e-300)):.3f}; {int((want > 0).sum())} of {E * N} pay, "
          f"{int((oid >= 0).any(-1).sum())} list a disc, {int(hit.sum())} hit")
    assert_close(cost, want, what + " cost")
    assert (err <= bound).all(), what
    return orow, oid, gm, hit, x, cost


@pytest.mark.parametrize("shape", [s for s, _, _ in ER.SHAPES], ids=ER.IDS)
def test_different_lists_match_the_restatement(torch, shape):
    E, N, M, m = shape
    cs = ER.case(E, N, M, m)
    orow, oid, gm, hit, x, cost = check_against_restatement(torch, cs, per_env_field(torch, cs, m), m, str(shape))
    if M == 0:
        assert np.isposinf(gm).all() and (oid == -1).all() and not orow.any() and not hit.any() and not cost.any()
    elif E > 1:
        assert len({oid[e].tobytes() + orow[e].tobytes() for e in range(E)}) > 1


@pytest.mark.parametrize("shape", [s for s, _, _ in ER.SHAPES if s[0] <= 40 and s[2] > 0], ids=[i for (s, _, _), i in zip(ER.SHAPES, ER.IDS)
                                                                                              if s[0] <= 40 and s[2] > 0])
def test_each_env_is_the_shared_kernel_run_with_its_list(torch, shape):
    """One shared field, `set` to env e's list in turn: its outputs on env e's records are the per-env outputs, bit for bit."""
    E, N, M, m = shape
    w = ER.reward_window(E, N, M)
    per, sh = per_env_field(torch, w, m), shared_field(torch, w, w["obstacles"][0], m, E)
    z = dev(torch, w["z"])
    got = outputs(torch, per, z, storage_of(torch, per, w))
    st = storage_of(torch, sh, w)
    for e in range(E):
        sh.set(w["obstacles"][e])
        want = outputs(torch, sh, z, st)
        for name, a, b in zip(NAMES, got, want):
            a, b = (a[:, e], b[:, e]) if name.startswith("reward") or name.startswith("shaped") else (a[e], b[e])
            assert same(torch, a, b), (shape, e, name)


@pytest.mark.parametrize("window,M", ER.WINDOW_SHAPES, ids=[str(s) for s, _ in ER.WINDOW_SHAPES])
def test_tables_match_the_restatement_and_the_shared_scan_per_env(torch, window, M):
    from scalable_collision_avoidance_rl_amd.obstacles import episode_env_obstacle_safety, episode_obstacle_safety
    T, E, N = window
    t = lambda a: dev(torch, a)
    for c, counts in ((2, None), (5, ER.ragged_counts(E, M))):
        w = ER.window_case(T, E, N, M, c=c, counts=counts)
        args = (t(w["z"]), t(w["done"]), t(w["xF"]), t(w["radius"]))
        got = episode_env_obstacle_safety(*args, t(w["obstacles"]), t(w["counts"].astype(np.int32)), c, t(w["z_final"]))
        ref = ER.episode_tables(w)
        for name in OR.TABLES:
            a, b = host(got[name]), ref[name]
            if a.dtype == np.int32:
                assert np.array_equal(a, b), (window, c, name)
            else:
                special = ~np.isfinite(b)
                assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[special & ~np.isnan(b)], b[special & ~np.isnan(b)])
                assert_close(a[~special], b[~special], f"{window} c={c} {name}")
        if E <= 15:                                            # per env: the shared scan with that env's (truncated) list
            for e in range(E):
                want = episode_obstacle_safety(*args, t(ER.env_list(w, e).reshape(-1, 3)), c, t(w["z_final"]))
                for name in OR.TABLES:
                    assert same(torch, got[name][e], want[name][e]), (window, c, e, name)
        if counts is not None:                                 # an env without discs: +inf and 0, as M = 0
            empty = np.flatnonzero((w["counts"] == 0) & (ref["ep_len"] > 0))
            assert empty.size and np.isposinf(host(got["min_obstacle_gap"])[empty]).all()
            assert np.isposinf(host(got["ep_min_obstacle_gap"])[empty]).all() and not host(got["obstacle_hit_steps"])[empty].any()


# ------------------------------------------------------------------------------------------ 3. ragged counts
@pytest.mark.parametrize("shape", [s for s, _, _ in ER.SHAPES if s[2] > 0], ids=[i for (s, _, _), i in zip(ER.SHAPES, ER.IDS) if s[2] > 0])
def test_ragged_counts_never_read_the_rows_behind_the_count(torch, shape):
    """Rows at or beyond count[e] hold a disc ON the agents: the outputs are those of the truncated lists -- the restatement's,
    and bit for bit those of the same field with harmless padding."""
    E, N, M, m = shape
    cs = ER.case(E, N, M, m, counts=ER.ragged_counts(E, M))
    planted = ER.plant_on_agents(cs)
    field = per_env_field(torch, planted, m)
    orow, oid, gm, hit, x, cost = check_against_restatement(torch, planted, field, m, f"{shape} ragged")
    empty = cs["counts"] == 0
    assert empty.any() or E < 3
    assert np.isposinf(gm[empty]).all() and (oid[empty] == -1).all() and not orow[empty].any() and not hit[empty].any()
    assert not cost[empty].any() and not x[empty][..., (K + 1) * C:].any()
    z = dev(torch, cs["z"])
    w = ER.reward_window(E, N, M, counts=cs["counts"])
    st = storage_of(torch, field, w)
    got = outputs(torch, field, z, st)
    field.set(cs["obstacles"] * (np.arange(M)[None, :, None] < cs["counts"][:, None, None]), cs["counts"])    # zero padding
    want = outputs(torch, field, z, st)
    for name, a, b in zip(NAMES, got, want):
        assert same(torch, a, b), (shape, name)
    # a count beyond M or below 0 on the device is clamped, never followed past the env's rows
    field._counts.copy_(torch.as_tensor(np.where(np.arange(E) % 2, 10 ** 6, -5).astype(np.int32)))
    clamped = outputs(torch, field, z)
    field.set(field.obstacles, np.where(np.arange(E) % 2, M, 0))
    for name, a, b in zip(NAMES, clamped, outputs(torch, field, z)):
        assert same(torch, a, b), (shape, name, "clamped")


# ------------------------------------------------------------------------------------------ 4. rows and wraps
@pytest.mark.parametrize("shape", [s for s, _, _ in ER.SHAPES], ids=ER.IDS)
def test_rows_of_a_ring_and_a_block_give_the_one_row_result(torch, shape):
    E, N, M, m = shape
    cs = ER.case(E, N, M, m, counts=ER.ragged_counts(E, M) if M else None)
    field = per_env_field(torch, cs, m)
    rows = dev(torch, ER.rows_case(cs, 5))                     # a [T+1,E,N,d] ring with T = 4 (and an [M_t,E,N,d] block alike)
    x = field.observe(rows, cost=WEIGHT)
    cost = field.cost
    assert tuple(x.shape) == (5, E, N, field.obs_width) and tuple(cost.shape) == (5, E, N)
    for j in range(5):
        xj = field.observe(rows[j], cost=WEIGHT)
        assert xj.data_ptr() != x.data_ptr()
        assert same(torch, xj, x[j]) and same(torch, field.cost, cost[j]), (shape, j)
    block = field.observe(rows[1:4], out=torch.empty(3, E, N, field.obs_width, device=DEV))
    assert same(torch, block, x[1:4])
    want = ER.columns(cs, m, z=host(rows))
    assert np.array_equal(host(x).view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError, match="end in E"):
        field.observe(rows.view(5 * E, N, -1)[:E + 1])


@pytest.mark.parametrize("shape", [(7, 5, 8, 2), (300, 1, 64, 4)], ids=["staged", "direct"])
def test_shaped_reward_over_a_window_matches_the_restatement(torch, shape):
    E, N, M, m = shape
    w = ER.reward_window(E, N, M, counts=ER.ragged_counts(E, M))
    assert {tuple(np.flatnonzero(w["done"][:, e])) for e in range(E)} >= {tuple(p) for p in OO.WINDOW_ENDS}
    field = per_env_field(torch, w, m)
    st = storage_of(torch, field, w)
    raw = st.reward.clone()
    cost = torch.empty_like(raw)
    out = field.shape_reward(st, WEIGHT, cost_out=cost)
    torch.cuda.synchronize()
    assert torch.equal(st.reward, raw) and out.data_ptr() != st.reward.data_ptr()          # storage.reward is untouched
    ref = ER.shaped_reward(w, WEIGHT)
    err, cerr = np.abs(host(out) - ref["reward"]), np.abs(host(cost) - ref["cost"])
    assert (err <= ref["bound"]).all() and (cerr <= ref["cost_bound"]).all() and int((ref["cost"] > 0).sum()) > 0
    assert_close(host(cost), ref["cost"], "cost")
    assert torch.equal(out, raw - cost)
    twin = types.SimpleNamespace(**dict(vars(st), reward=raw.clone()))                      # in place
    assert field.shape_reward(twin, WEIGHT, out=twin.reward) is twin.reward and same(torch, twin.reward, out)
    ring_only = types.SimpleNamespace(**dict(vars(st), z_final=None))                       # without z_final the ring is read
    got = field.shape_reward(ring_only, WEIGHT)
    ref_ring = ER.shaped_reward(w, WEIGHT, with_final=False)
    assert (np.abs(host(got) - ref_ring["reward"]) <= ref_ring["bound"]).all() and not torch.equal(got, out)


@pytest.mark.parametrize("shape", [(7, 5, 8, 2), (40, 2, 64, 2)], ids=["staged", "direct"])
def test_bases_off_alignment_give_the_aligned_bits(torch, shape):
    from scalable_collision_avoidance_rl_amd.obstacles import episode_env_obstacle_safety
    E, N, M, m = shape
    cs = ER.case(E, N, M, m, counts=ER.ragged_counts(E, M))
    field = per_env_field(torch, cs, m)
    z = dev(torch, cs["z"])
    d, w = z.shape[-1], field.obs_width
    want = outputs(torch, field, z)
    T = 3
    win = dev(torch, ER.rows_case(cs, T))
    done = torch.zeros(T, E, dtype=torch.uint8, device=DEV)
    done[T - 1] = 1
    tab = lambda zz: episode_env_obstacle_safety(zz, done, field.env._xF, field.env._radius, field.device_obstacles, field._counts, C)
    want_tab = {n: v.clone() for n, v in tab(win).items()}
    assert z.data_ptr() % 16 == 0 and want[4].data_ptr() % 16 == 0
    for off_in, off_out in ((1, 0), (2, 0), (0, 1), (0, 2), (3, 3)):
        zbuf = torch.zeros(z.numel() + 4, device=DEV)
        zo = zbuf[off_in:off_in + z.numel()].view(E, N, d)
        zo.copy_(z)
        xbuf = torch.full((E * N * w + 8,), 7.0, device=DEV)
        xo = xbuf[off_out:off_out + E * N * w].view(E, N, w)
        assert zo.data_ptr() % 16 == 4 * off_in and xo.data_ptr() % 16 == 4 * off_out
        field.sense(zo, gap_min=True)
        got = [field.orow, field.oid, field.gap_min, field.hit, field.observe(zo, out=xo, cost=WEIGHT), field.cost]
        for name, a, b in zip(NAMES, got, want):
            assert same(torch, a, b), (shape, off_in, off_out, name)
        assert bool((xbuf[:off_out] == 7.0).all()) and bool((xbuf[off_out + E * N * w:] == 7.0).all())
        wbuf = torch.zeros(win.numel() + 4, device=DEV)
        wo = wbuf[off_in:off_in + win.numel()].view(T, E, N, d)
        wo.copy_(win)
        for name, v in tab(wo).items():
            assert same(torch, v, want_tab[name]), (shape, off_in, name)


# ------------------------------------------------------------------------------------------ 5. capture and determinism
def test_chain_replays_from_a_graph_follows_set_and_is_deterministic(torch):
    """sense -> shield -> step(execute=) -> observe on a real env, captured after an eager warm-up: a replay equals the eager run
    bit for bit, after `field.set(other discs, other counts)` it equals an eager run that was given those, and two runs agree."""
    from scalable_collision_avoidance_rl_amd import ActionShield, ObstacleField, drones, place_obstacles_per_env
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    N, E, steps = 5, 12, 6

    def setup():
        env = drones(N, 0, [5, 5], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True, device=DEV,
                     seed=9, auto_reset=True)
        obs, cnt = place_obstacles_per_env(env.grid, 8, E, seed=1, keep_clear=env.end_points.reshape(-1, 2), clearance=0.1)
        field = ObstacleField(env, obs, m=2, per_env=True, counts=cnt)
        shield = ActionShield(env, 0.25, 0.05, 1.0, obstacles=field)
        g = torch.Generator(device=DEV).manual_seed(4)
        act = torch.rand(steps, E, N, 2, device=DEV, generator=g) * 2 - 1
        return env, field, shield, act, torch.zeros(E, N, 2, device=DEV), RolloutStorage(env, steps, actions=True)

    def chain(env, field, shield, act, safe, st):
        st.begin()
        for t in range(steps):
            env.step(act[t], into=(st, t), execute=shield(act[t], out=safe))
        return field.observe(env.z, cost=WEIGHT)

    def snap(env, field, shield, act, safe, st, x):
        return [t.clone() for t in (env.z, env.pos, safe, st.zbuf, st.reward, field.orow, field.oid, x, field.cost, shield.intervened)]

    a = setup()
    other = place_obstacles_per_env(a[0].grid, 8, E, seed=2, keep_clear=a[0].end_points.reshape(-1, 2), clearance=0.1)
    assert not np.array_equal(other[0], a[1].obstacles)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        x = chain(*a)                                          # eager warm-up: builds every buffer
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x = chain(*a)
    b, b2 = setup(), setup()
    ref, ref2 = [], []
    for rep in range(4):
        if rep == 2:
            b[1].set(*other), b2[1].set(*other)
        ref.append(snap(*b, chain(*b)))
        ref2.append(snap(*b2, chain(*b2)))
    torch.cuda.synchronize()
    for rep in (1, 2, 3):
        if rep == 2:
            a[1].set(*other)
        graph.replay()
        torch.cuda.synchronize()
        for j, (p, q, q2) in enumerate(zip(snap(*a, x), ref[rep], ref2[rep])):
            assert same(torch, p, q) and same(torch, q, q2), (rep, j)
    assert int((a[1].oid >= 0).sum()) > 0 and int(a[2].intervened.sum()) > 0


# ------------------------------------------------------------------------------------------ 6. through the stack
def test_shield_guarantee_per_env_and_an_empty_list_is_the_plain_shield(torch):
    from scalable_collision_avoidance_rl_amd import ActionShield, ObstacleField, drones, place_obstacles_per_env
    from scalable_collision_avoidance_rl_amd.drone_env import dt
    N, E, M, m, rate, margin, orate = 5, 16, 12, 3, S.RATE, S.MARGIN, OR.OBSTACLE_RATE
    mk = lambda: drones(N, 0, [5, 5], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True, device=DEV,
                        seed=21, auto_reset=True)
    env, twin = mk(), mk()
    obs, cnt = place_obstacles_per_env(env.grid, M, E, seed=5, keep_clear=env.end_points.reshape(-1, 2), clearance=0.1)
    cnt[3] = cnt[7] = 0                                       # two envs without discs
    field = ObstacleField(env, obs, m=m, per_env=True, counts=cnt)
    shield = ActionShield(env, rate, margin, S.U_MAX, obstacles=field, obstacle_rate=orate)
    plain = ActionShield(twin, rate, margin, S.U_MAX)
    g = torch.Generator(device=DEV).manual_seed(8)
    live = 0
    for step in range(25):
        act = torch.rand(E, N, 2, device=DEV, generator=g) * 2 - 1
        z, nbr = env.z.clone(), env.nbr_idx.clone()
        safe = shield(act)
        assert torch.equal(z, twin.z)
        ref = plain(act)
        torch.cuda.synchronize()
        orow, oid, radius = host(field.orow), host(field.oid), host(env._radius)
        assert same(torch, safe[[3, 7]], ref[[3, 7]]) and (oid[[3, 7]] == -1).all()          # an empty list: the plain shield
        assert (oid < cnt[:, None, None]).all()
        for e in range(E):                                     # the guarantee per env, with that env's list
            tol = OR.tolerance(host(act[e]), host(z[e]).reshape(N, -1), 3, 2, radius, rate, orate, margin, S.U_MAX, dt, orow[e])
            rows = np.concatenate([host(z[e]).reshape(N, 3, 2)[:, 1:].reshape(-1, 2), orow[e].reshape(-1, 3)[:, :2]]).astype(np.float64)
            dist = np.sqrt((rows ** 2).sum(1))
            slack = 2 * dt * tol + 4 * S.EPS32 * dist[np.isfinite(dist)].max()
            short, n = OR.guarantee_shortfall(host(safe[e]), orow[e], oid[e], radius, int(cnt[e]), orate, margin, dt)
            live += n
            assert n == 0 or short <= slack, (step, e, short, slack)
        env.step(act, execute=safe)
        twin.step(act, execute=safe)
    assert live > 50


def test_evaluator_reports_the_fields_tables(torch):
    from scalable_collision_avoidance_rl_amd import ObstacleField, drones, place_obstacles_per_env
    from scalable_collision_avoidance_rl_amd.evaluate import Evaluator
    from tests import test_gpu_obstacle_obs as GO
    N, E = GO.N, 6
    env = drones(N, 0, [5, 5], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True, device=DEV, seed=3,
                 auto_reset=True)
    obs, cnt = place_obstacles_per_env(env.grid, 12, E, seed=1, keep_clear=env.end_points.reshape(-1, 2), clearance=0.1)
    field = ObstacleField(env, obs, m=GO.M_SLOTS, per_env=True, counts=cnt)
    actor, critic = GO.wide_networks(torch)
    ev = Evaluator(env, actor, critic, gamma=0.99, n_bins=6, safety=True, obstacles=field, obstacle_inputs=True)
    tab = ev.run(1)
    want = field.episode_safety(ev.storage)
    torch.cuda.synchronize()
    for name in OR.TABLES:
        assert same(torch, tab[name][0], want[name]), name
    w = dict(z=host(ev.storage.z), done=host(ev.storage.done), xF=host(env._xF), radius=host(env._radius),
             obstacles=obs.astype(np.float32), counts=cnt, z_final=host(ev.storage.z_final))
    ref = ER.episode_tables(w)
    assert np.array_equal(host(tab["ep_len"][0]), ref["ep_len"]) and int(ref["ep_len"].min()) > 0
    assert_close(host(tab["ep_min_obstacle_gap"][0]), ref["ep_min_obstacle_gap"], "ep_min_obstacle_gap")


@pytest.mark.parametrize("which", ["sa2c", "ppo"])
def test_learner_equals_a_plain_learner_on_a_storage_made_with_the_per_env_entries(torch, which):
    from scalable_collision_avoidance_rl_amd import ObstacleField, place_obstacles_per_env
    from tests import test_gpu_obsnorm_learner as OL
    from tests import test_gpu_obstacle_obs as GO
    N, E, T, WIDTH = GO.N, GO.E, GO.T, GO.WIDTH
    env, st = OL.real_window(torch, N, 5.0, E, T, [0, 180, 190, 0, 3, 175, 199, 0])
    obs, cnt = place_obstacles_per_env(env.grid, 12, E, seed=1, keep_clear=env.end_points.reshape(-1, 2), clearance=0.1)
    field = ObstacleField(env, obs, m=GO.M_SLOTS, per_env=True, counts=cnt)
    kw = dict(lam=0.95)
    raw_reward = st.reward.clone()
    actor, critic, learner = GO.wide_learner(torch, which, obstacles=field, obstacle_weight=WEIGHT, **kw)
    out = learner.train(st)
    torch.cuda.synchronize()
    assert torch.equal(st.reward, raw_reward)
    cost_mean = out.pop("obstacle_cost")
    run_a = OL.snapshot(actor, critic, learner, out)
    ring = field.observe(st.z_all, out=torch.empty(T + 1, E, N, WIDTH, device=DEV))
    final = field.observe(st.z_final, out=torch.empty(T, E, N, WIDTH, device=DEV))
    cost = torch.empty(T, E, N, device=DEV)
    shaped = field.shape_reward(st, WEIGHT, cost_out=cost)
    stand_in = types.SimpleNamespace(zbuf=ring, z_pre=ring[:T], z_all=ring, z_final=final, reward=shaped, done=st.done,
                                     actions=st.actions, nbr_pre=st.nbr_pre)
    actor, critic, plain = GO.wide_learner(torch, which, **kw)
    out = plain.train(stand_in)
    torch.cuda.synchronize()
    OL.assert_same(torch, run_a, OL.snapshot(actor, critic, plain, out), which)
    assert torch.equal(learner._rs, shaped) and torch.equal(learner._oc, cost) and torch.equal(learner._xo, ring)
    assert torch.equal(cost_mean, cost.view(T * E, N).mean(0)) and float(cost_mean.max()) > 0
    # the envs saw different discs: the same records under env 0's list in every env give another window
    tiled = ObstacleField(env, np.tile(obs[:1], (E, 1, 1)), m=GO.M_SLOTS, per_env=True, counts=np.full(E, cnt[0]))
    assert not torch.equal(tiled.observe(st.z_all, out=torch.empty_like(ring)), ring)
