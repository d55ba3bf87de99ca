"""Obstacles on the device: `dronesim_obstacle_sense`, `dronesim_action_shield_obstacles`, `dronesim_episode_obstacle_safety`
(csrc/obstacles.hip, csrc/shield.hip), `ObstacleField`, `ActionShield(obstacles=)` and `Evaluator(obstacles=)` against the float64
brute-force restatement tests/obstacle_ref.py.

Sense: ids exact, rows / gaps / gap_min within the standing 1e-5 (tests/helpers.py) on records whose decisions are 1e-4 apart
(the generator redraws until they are; tests/test_obstacles_host.py asserts none is left out), plus exact hand-placed records.
Shield: tests/test_gpu_shield.py's bars -- feasible and optimal against the restatement within the derived tolerance
16 eps32 (max(|u|inf, u_max) + max(rate, obstacle_rate) (D + l_max + max(l_max, r_max) + margin) / dt), flags compared outside the
band.  Tables: floats within 1e-5, counts exact.  Closed loop: the per-step guarantee of DESIGN.md on a real env."""
import types

import numpy as np
import pytest

from tests import obstacle_ref as O
from tests import shield_ref as S
from tests.helpers import assert_close
from tests.test_gpu_shield import check_against_ref, dev, host, make_env

pytestmark = pytest.mark.gpu
E = S.E_CASE


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def stand_in_env(torch, E, N, k, c, case):
    """What `ObstacleField` and `ActionShield` read of an env, for record shapes no `drones` env has (N = 1)."""
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32), device="cuda:0")
    return types.SimpleNamespace(batched=True, n_envs=E, n_agents=N, k_closest=k, c=c, device=torch.device("cuda", 0), z=None,
                                 nbr_idx=None, _radius=t(case["radius"]), _xF=t(case["xF"]), _delta=t(case["sense"]),
                                 obstacles=np.asarray(case["obstacles"], np.float64))


def field_of(torch, case, N, k, c, m, E=E, sense=None):
    from scalable_collision_avoidance_rl_amd import ObstacleField
    return ObstacleField(stand_in_env(torch, E, N, k, c, case), m=m, sense=sense)


def close(a, b, what):
    """`assert_close` (1e-5), with infinities compared exactly (the gaps without a disc are +inf)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    inf = np.isinf(b)
    assert np.array_equal(a[inf], b[inf]), what
    assert_close(a[~inf], b[~inf], what)


def check_sense(what, field, case, m, R):
    N = case["radius"].shape[0]
    ref = O.sense(case["z"].reshape(R, -1), case["xF"], case["radius"], case["sense"], case["obstacles"], m)
    oid, orow = host(field.oid).reshape(R, m), host(field.orow).reshape(R, m, 3)
    gm, hit = host(field.gap_min).reshape(R), host(field.hit).reshape(R)
    assert oid.dtype == np.int32 and np.array_equal(oid, ref["oid"]), what
    assert_close(orow, ref["orow"], what + " orow")
    close(gm, ref["gap_min"], what + " gap_min")
    assert np.array_equal(hit.astype(bool), ref["hit"]) and hit.dtype == np.uint8, what
    # the gaps of the listed discs, from the kernel's own rows
    ri = case["radius"].astype(np.float64)[np.arange(R) % N]
    got = np.sqrt((orow[..., :2].astype(np.float64) ** 2).sum(2)) - ri[:, None] - orow[..., 2]
    listed = ref["oid"] >= 0
    want = np.take_along_axis(ref["G"], np.maximum(ref["oid"], 0), 1) if ref["G"].shape[1] else np.zeros_like(got)
    assert_close(got[listed], want[listed], what + " gaps")
    assert (orow[~listed] == 0).all(), what
    return ref


# ---------------------------------------------------------------------------------------------- 1. sense
@pytest.mark.parametrize("Mm", O.SENSE_CASES, ids=lambda c: "M%dm%d" % c)
@pytest.mark.parametrize("shape", S.CASES, ids=lambda c: "N%dk%dc%d" % c)
def test_sense_matches_the_restatement(torch, shape, Mm):
    (N, k, c), (M, m) = shape, Mm
    case = O.sense_case(N, k, c, M, m)
    field = field_of(torch, case, N, k, c, m)
    orow, oid = field.sense(dev(torch, case["z"]), gap_min=True)
    assert tuple(orow.shape) == (E, N, m, 3) and tuple(oid.shape) == (E, N, m) and field.M == M
    ref = check_sense(f"sense {shape} {Mm}", field, case, m, E * N)
    print(f"{shape} M={M} m={m}: slots filled {np.mean(ref['oid'] >= 0):.3f}, hits {ref['hit'].mean():.3f}, discs in range {ref['n_in'].mean():.1f}")


@pytest.mark.parametrize("offset", [4, 8])
def test_sense_reads_z_at_a_base_that_breaks_the_alignment(torch, offset):
    """(2, 1, 2): 16-byte records; a base at 8 (mod 16) takes the 8-byte load, at 4 (mod 8) the dword loads -- same bits."""
    N, k, c = S.CASES[0]
    case = O.sense_case(N, k, c, 16, 4)
    field = field_of(torch, case, N, k, c, 4)
    field.sense(dev(torch, case["z"]), gap_min=True)
    keep = [x.clone() for x in (field.orow, field.oid, field.gap_min, field.hit)]
    field.sense(dev(torch, case["z"], offset), gap_min=True)
    for a, b in zip(keep, (field.orow, field.oid, field.gap_min, field.hit)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_sense_exact_records_ties_touch_nan_and_empty_slots(torch):
    e = O.exact_case()
    for m, (oid, orow, gap_min, hit) in e["want"].items():
        field = field_of(torch, e, 4, 1, 2, m, E=1)
        field.sense(dev(torch, e["z"]), gap_min=True)
        assert np.array_equal(host(field.oid)[0], oid), m                          # mirrored discs: the lower id first
        assert np.array_equal(host(field.orow)[0], orow.astype(np.float32)), m     # dyadic: exact
        assert np.array_equal(host(field.gap_min)[0], gap_min.astype(np.float32), equal_nan=True), m   # gap == 0 exactly; NaN
        assert np.array_equal(host(field.hit)[0], hit), m                          # the touch is a hit, the NaN is none
    # the touch is in range even with a range of 0; nothing else is
    field = field_of(torch, e, 4, 1, 2, 2, E=1, sense=0.0)
    field.sense(dev(torch, e["z"]))
    assert host(field.oid)[0].tolist() == [[-1, -1], [2, -1], [-1, -1], [-1, -1]] and field.gap_min is None


# ---------------------------------------------------------------------------------------------- 2. shield
SHIELD_CASES = [((9, 8, 2), dict(M=64, reach=3.0)), ((1, 1, 2), {}), ((5, 2, 2), {}), ((5, 2, 5), {})]


def run_shield(torch, case, N, k, c, m=4, u=None, out=None, obstacle_rate=O.OBSTACLE_RATE, **kw):
    from scalable_collision_avoidance_rl_amd import ActionShield
    field = field_of(torch, case, N, k, c, m)
    sh = ActionShield(field.env, S.RATE, S.MARGIN, S.U_MAX, obstacles=field, obstacle_rate=obstacle_rate, **kw)
    u = dev(torch, case["u"]) if u is None else u
    res = sh(u, z=dev(torch, case["z"]), nbr=dev(torch, case["nbr"]), out=out)
    return res, sh, field


@pytest.mark.parametrize("shape,kw", SHIELD_CASES, ids=lambda c: "N%dk%dc%d" % c if isinstance(c, tuple) else None)
def test_obstacle_shield_is_feasible_and_optimal_against_the_restatement(torch, shape, kw):
    N, k, c = shape
    case = O.shield_case(N, k, c, **kw)
    out, sh, field = run_shield(torch, case, N, k, c)
    orow, oid = host(field.orow), host(field.oid)
    want_row, want_id = O.case_list(case, 4)
    assert np.array_equal(oid, want_id)                                            # (the list itself: checked in part 1)
    ref = O.shield_reference(case, c, orow, oid)                                   # the kernel's own rows, as the shield read them
    check_against_ref(f"obstacle shield {shape}", host(out), host(sh.intervened), host(sh.correction), case["u"], case["z"], case["nbr"],
                      case["radius"], c, ref=ref)
    on = ref["on"][:, 4 + k:]
    assert on.any()
    if k == 8:
        assert ref["on"].shape[1] == 16 and ref["on"].all(1).any()                 # all 16 constraints of a record listed
    if N == 1:
        assert not ref["on"][:, 4:4 + k].any()                                     # obstacle-only: no neighbour is listed


def test_obstacle_shield_without_a_listed_disc_is_the_plain_shield_bit_for_bit(torch):
    from scalable_collision_avoidance_rl_amd import ActionShield
    N, k, c = 5, 2, 2
    base = O.shield_case(N, k, c)
    far = dict(base, obstacles=(base["obstacles"] + np.float32([100.0, 100.0, 0.0])).astype(np.float32))
    none = dict(base, obstacles=np.zeros((0, 3), np.float32))
    plain = ActionShield(stand_in_env(torch, E, N, k, c, base), S.RATE, S.MARGIN, S.U_MAX)
    want = plain(dev(torch, base["u"]), z=dev(torch, base["z"]), nbr=dev(torch, base["nbr"]))
    for what, case in (("M = 0", none), ("out of range", far)):
        out, sh, field = run_shield(torch, case, N, k, c)
        assert int((field.oid >= 0).sum()) == 0, what
        assert torch.equal(out.view(torch.int32), want.view(torch.int32)), what
        assert torch.equal(sh.intervened, plain.intervened) and torch.equal(sh.correction.view(torch.int32), plain.correction.view(torch.int32)), what
    out, sh, field = run_shield(torch, base, N, k, c)                              # (and with discs listed the answer differs)
    assert not torch.equal(out, want)


def test_obstacle_shield_in_place_and_bit_identical_run_to_run(torch):
    N, k, c = 9, 8, 2
    case = O.shield_case(N, k, c, M=64, reach=3.0)
    a, sh_a, _ = run_shield(torch, case, N, k, c, stats=True)
    u = dev(torch, case["u"])
    b, sh_b, _ = run_shield(torch, case, N, k, c, u=u, out=u, stats=True)
    assert b is u and torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(sh_a.intervened, sh_b.intervened) and torch.equal(sh_a.correction.view(torch.int32), sh_b.correction.view(torch.int32))
    ta, tb = sh_a.totals(), sh_b.totals()
    for n in ("interventions", "nonfinite", "correction_sum", "correction_max"):
        assert torch.equal(ta[n].view(torch.uint8), tb[n].view(torch.uint8)), n
    assert int(ta["interventions"].sum()) == int(sh_a.intervened.sum()) > 0


# ---------------------------------------------------------------------------------------------- 3. episode tables
def run_tables(torch, w, z_final, **kw):
    from scalable_collision_avoidance_rl_amd.obstacles import episode_obstacle_safety
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
    return episode_obstacle_safety(t(w["z"]), t(w["done"]), t(w["xF"]), t(w["radius"]), t(w["obstacles"]), w["c"],
                                   None if z_final is None else t(z_final), **kw)


@pytest.mark.parametrize("with_final", [True, False], ids=["z_final", "no z_final"])
@pytest.mark.parametrize("c", [2, 5])
def test_episode_tables_match_the_restatement(torch, c, with_final):
    from scalable_collision_avoidance_rl_amd.evaluate import episode_safety
    w = O.window(c=c, with_final=with_final)
    got = run_tables(torch, w, w["z_final"])
    ref = O.episode_tables(w["z"], w["done"], w["xF"], w["radius"], w["obstacles"], w["z_final"])
    assert np.array_equal(host(got["ep_len"]), ref["ep_len"]) and sorted(set(ref["ep_len"].tolist())) == [0, 1, 4, 5, 12]
    for name in ("min_obstacle_gap", "ep_min_obstacle_gap"):
        assert host(got[name]).dtype == np.float32
        close(host(got[name]), ref[name], name)
    for name in ("obstacle_hit_steps", "ep_obstacle_hit_steps"):
        assert host(got[name]).dtype == np.int32 and np.array_equal(host(got[name]), ref[name]), name
    assert host(got["obstacle_hit_steps"])[1, 0] == 1 and host(got["min_obstacle_gap"])[1, 0] == 0.0   # the exact touch
    # ep_len is the safety tables' own
    T, En, N, d = w["z"].shape
    t = lambda a: torch.as_tensor(a, device="cuda:0")
    nbr = torch.zeros(T, En, N, d // c, dtype=torch.int32, device="cuda:0")
    fin = dict(z_final=t(w["z_final"]), nbr_final=nbr) if with_final else {}
    safety = episode_safety(t(w["z"]), nbr, t(w["done"]), t(w["radius"]), torch.ones(N, device="cuda:0"), **fin)
    assert torch.equal(got["ep_len"], safety["ep_len"])
    # a subset of the tables, and two runs bit for bit
    part = dict(ep_len=torch.zeros(En, dtype=torch.int32, device="cuda:0"), min_obstacle_gap=torch.zeros(En, N, device="cuda:0"))
    assert run_tables(torch, w, w["z_final"], out=part) is part
    assert torch.equal(part["min_obstacle_gap"].view(torch.int32), got["min_obstacle_gap"].view(torch.int32))
    again = run_tables(torch, w, w["z_final"])
    for name in O.TABLES:
        assert torch.equal(again[name].view(torch.uint8), got[name].view(torch.uint8)), name


def test_episode_tables_of_empty_windows_and_without_discs(torch):
    w = O.window()
    WN = O.WINDOW["N"]
    for cut in (dict(z=w["z"][:0], done=w["done"][:0]), dict(z=w["z"][:, :0], done=w["done"][:, :0])):
        got = run_tables(torch, dict(w, **cut), None)
        En = cut["z"].shape[1]
        assert tuple(got["ep_len"].shape) == (En,) and tuple(got["min_obstacle_gap"].shape) == (En, WN)
        if En:
            assert int(got["ep_len"].abs().sum()) == 0                                                                     # T = 0: no episode anywhere
            assert np.isnan(host(got["min_obstacle_gap"])).all() and int(got["ep_obstacle_hit_steps"].sum()) == 0
    got = run_tables(torch, dict(w, obstacles=np.zeros((0, 3), np.float32)), None)
    valid = host(got["ep_len"]) > 0
    assert np.isposinf(host(got["ep_min_obstacle_gap"])[valid]).all() and np.isnan(host(got["ep_min_obstacle_gap"])[~valid]).all()
    assert int(got["obstacle_hit_steps"].sum()) == 0


# ---------------------------------------------------------------------------------------------- 4. closed loop on a real env
def loop_env(torch, su):
    env = make_env(O.LOOP["N"], O.LOOP["E"], 23, k=O.LOOP["k"])
    assert np.allclose(host(env._xF), su["xF"], atol=1e-6) and np.allclose(host(env._delta), O.LOOP["delta"])
    env.set_state(su["starts"].astype(np.float32))
    return env


def test_closed_loop_keeps_the_guarantee_and_the_plain_shield_hits_where_predicted(torch):
    """60 steps of control("proportional") -> shield -> step(execute=) from the scene of `obstacle_ref.loop_setup`.  With the
    field: after every step, for every LISTED disc, g' >= (1 - obstacle_rate) max(g, 0) + min(g, 0) - slack with g the gap minus
    the margin from the float32 positions in float64 and slack = 2 dt tol + 4 eps32 D (tests/test_gpu_shield_geometry.py's form).
    With the plain shield: obstacle hits in the envs the float64 closed loop predicts.  Arrival is reported."""
    from scalable_collision_avoidance_rl_amd import ActionShield, ObstacleField
    from scalable_collision_avoidance_rl_amd.obstacles import episode_obstacle_safety
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    su = O.loop_setup()
    N, k, m, steps, margin, rate, orate = (O.LOOP[n] for n in ("N", "k", "m", "steps", "margin", "rate", "obstacle_rate"))
    obs = su["obstacles"].astype(np.float32).astype(np.float64)
    rad = su["radius"]
    tables = {}
    for with_obstacles in (True, False):
        env = loop_env(torch, su)
        En = env.n_envs
        field = ObstacleField(env, su["obstacles"], m=m)
        sh = ActionShield(env, rate, margin, S.U_MAX, obstacles=field if with_obstacles else None,
                          obstacle_rate=orate if with_obstacles else None)
        st = RolloutStorage(env, steps, actions=True)
        st.begin()
        worst, listed_n = -np.inf, 0
        for t in range(steps):
            u = env.control("proportional", out=st.actions[t])
            before = host(env.pos).astype(np.float64)
            z_now = host(env.z)
            safe = sh(u)
            env.step(u, into=(st, t), execute=safe)
            if not with_obstacles:
                continue
            oid, orow = host(field.oid).reshape(En * N, m), host(field.orow).reshape(En * N, m, 3)
            after = host(env.pos).astype(np.float64)
            gap = lambda p: (np.linalg.norm(obs[None, None, :, :2] - p[:, :, None, :], axis=3) - rad[None, :, None] - obs[None, None, :, 2]
                             - margin).reshape(En * N, -1)
            g, g_after = gap(before), gap(after)
            on = oid >= 0
            pick = np.maximum(oid, 0)
            g, g_after = np.take_along_axis(g, pick, 1)[on], np.take_along_axis(g_after, pick, 1)[on]
            tol = O.tolerance(host(u).reshape(-1, 2), z_now.reshape(En * N, -1), k + 1, 2, rad, rate, orate, margin, S.U_MAX, S.DT, orow)
            rows = np.concatenate([np.linalg.norm(z_now.reshape(En * N, k + 1, 2)[:, 1:], axis=2).ravel(),
                                   np.linalg.norm(orow[..., :2], axis=2).ravel()])
            slack = 2 * S.DT * tol + 4 * O.EPS32 * rows.max()
            short = (1 - orate) * np.maximum(g, 0) + np.minimum(g, 0) - g_after
            worst, listed_n = max(worst, float((short - slack).max(initial=-np.inf))), listed_n + int(on.sum())
        done = torch.zeros(steps, En, dtype=torch.uint8, device="cuda:0")
        done[steps - 1] = 1                                                        # the window is the episode so far
        tab = episode_obstacle_safety(st.z, done, env._xF, env._radius, field.device_obstacles, 2)
        tables[with_obstacles] = {n: host(x) for n, x in tab.items()}
        arrived = (np.linalg.norm(host(env.pos) - su["xF"][None], axis=2) <= 0.2).all(1)
        if with_obstacles:
            print(f"with the field: listed (step, agent, disc) triples {listed_n}, largest shortfall minus slack {worst:.3e}, smallest gap "
                  f"{tables[True]['ep_min_obstacle_gap'].min():.4f}, hit steps {tables[True]['ep_obstacle_hit_steps'].sum()}, arrived {arrived.mean():.3f}")
            assert listed_n > 0 and worst <= 0.0
        else:
            print(f"plain shield: envs with an obstacle hit {(tables[False]['ep_obstacle_hit_steps'] > 0).sum()} / {En}, deepest "
                  f"{tables[False]['ep_min_obstacle_gap'].min():.3f}, arrived {arrived.mean():.3f}")
    predicted = O.closed_loop(su, False)["min_gap"] < -O.HIT_DEPTH
    assert predicted.any() and (tables[False]["ep_obstacle_hit_steps"][predicted] > 0).all()
    assert (tables[True]["ep_len"] == steps).all()


# ---------------------------------------------------------------------------------------------- 5. plumbing
def test_chain_replays_from_a_graph_bit_for_bit_and_sees_field_set(torch):
    """control -> sense -> shield -> step(execute=) on one stream: the eager chain equals its graph replay, two runs are
    bit-identical, and discs uploaded by `field.set` after the capture are the ones a replay reads."""
    from scalable_collision_avoidance_rl_amd import ActionShield, ObstacleField
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    from scalable_collision_avoidance_rl_amd import place_obstacles
    N, k, T = O.LOOP["N"], O.LOOP["k"], 6
    first = place_obstacles([5, 5], 12, seed=6)
    moved = first + np.array([0.15, -0.1, 0.05])
    sides = []
    for _ in range(2):
        env = make_env(N, 16, 31, k=k)
        field = ObstacleField(env, first, m=2)
        sides.append((env, RolloutStorage(env, T, actions=True), ActionShield(env, S.RATE, S.MARGIN, S.U_MAX, stats=True, obstacles=field),
                      torch.zeros(16, N, 2, device="cuda:0")))

    def steps(env, st, sh, safe):
        env.reset(renew_obstacles=False)
        st.begin()
        for t in range(T):
            env.control("proportional", out=st.actions[t])
            env.step(st.actions[t], into=(st, t), execute=sh(st.actions[t], out=safe))

    for side in sides:                                                             # eager warm-up: buffers exist, counters agree
        steps(*side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        steps(*sides[1])
    for discs in (first, moved, first):
        for side in sides:
            side[2].obstacles.set(discs)
        steps(*sides[0])
        graph.replay()
        torch.cuda.synchronize()
        (ea, sa, ha, fa), (eb, sb, hb, fb) = sides
        for name in ("reward", "true_reward", "n_coll", "done", "zbuf", "nbrbuf", "actions"):
            assert torch.equal(getattr(sa, name), getattr(sb, name)), name
        assert torch.equal(ea.pos, eb.pos) and torch.equal(fa.view(torch.int32), fb.view(torch.int32))
        assert torch.equal(ha.obstacles.oid, hb.obstacles.oid) and torch.equal(ha.obstacles.orow.view(torch.int32), hb.obstacles.orow.view(torch.int32))
        assert torch.equal(ha.intervened, hb.intervened) and torch.equal(ha.correction.view(torch.int32), hb.correction.view(torch.int32))
        # the replay read the discs `set` uploaded: every listed radius is the current list's own (they differ by 0.05)
        oid, radii = host(hb.obstacles.oid), host(hb.obstacles.orow)[..., 2]
        assert (oid >= 0).any() and np.array_equal(radii[oid >= 0], discs.astype(np.float32)[oid[oid >= 0], 2])
    assert int(ha.totals()["interventions"].sum()) > 0


def test_evaluator_reports_the_obstacle_tables(torch):
    from scalable_collision_avoidance_rl_amd import ActionShield, Evaluator, ObstacleField, place_obstacles
    N, En = 5, 12
    figures = {}
    for shielded in (False, True):
        env = make_env(N, En, 17, k=4)
        discs = place_obstacles([5, 5], 8, seed=2, keep_clear=env.end_points.reshape(N, 2), clearance=0.3)
        field = ObstacleField(env, discs, m=2)
        sh = ActionShield(env, 0.25, 0.05, 1.0, obstacles=field if shielded else None)
        ev = Evaluator(env, "proportional", shield=sh, safety=True, obstacles=field)
        tab = ev.run(2)
        s = ev.safety_summary()
        t = {n: host(x) for n, x in tab.items()}
        assert t["ep_obstacle_hit_steps"].shape == (2, En) and t["min_obstacle_gap"].shape == (2, En, N)
        ok = t["ep_len"] > 0
        assert ok.all() and s["episodes"] == 2 * En
        free = t["ep_obstacle_hit_steps"] == 0
        clear = (t["ep_arrived"] != 0) & (t["ep_collisions"] == 0) & free
        assert s["obstacle_free_share"] == free.mean() and s["arrived_clear_share"] == clear.mean()
        assert s["min_obstacle_gap"] == float(t["ep_min_obstacle_gap"].min())
        assert s["mean_min_obstacle_gap"] == pytest.approx(t["ep_min_obstacle_gap"].astype(np.float64).mean(), rel=1e-12)
        assert np.array_equal(t["ep_obstacle_hit_steps"], t["obstacle_hit_steps"].sum(2))
        assert np.array_equal(t["ep_min_obstacle_gap"], t["min_obstacle_gap"].min(2))
        # the tables against the restatement on the stored window of the last round
        st = ev.storage
        ref = O.episode_tables(host(st.z), host(st.done), host(env._xF), host(env._radius), host(field.device_obstacles),
                               None if st.z_final is None else host(st.z_final))
        assert np.array_equal(t["ep_len"][1], ref["ep_len"])
        assert_close(t["min_obstacle_gap"][1], ref["min_obstacle_gap"], "min_obstacle_gap")
        figures[shielded] = s
    print("obstacle-free share: unshielded %.3f, shielded %.3f; smallest gap %.4f / %.4f" % (
        figures[False]["obstacle_free_share"], figures[True]["obstacle_free_share"], figures[False]["min_obstacle_gap"],
        figures[True]["min_obstacle_gap"]))
    plain = Evaluator(make_env(N, En, 17, k=4), "proportional", safety=True)
    plain.run(1)
    assert "obstacle_free_share" not in plain.safety_summary()
