"""Obstacles on the host (no GPU): parameter and shape errors of `obstacles.py` / `ActionShield(obstacles=)` / `Evaluator(obstacles=)`,
`place_obstacles`, the exports with their argtypes, the float64 restatement tests/obstacle_ref.py against hand-computed cases,
and the conditions the shared generators promise to the GPU tests -- asserted under the restatement alone: separation, the scan
path every window shape is there for (`ScanCols` restated), eviction shares, ties, the shares of records in which a list slot of a
converted shield family is active, the `on` rule's slots."""
import ctypes as C
import types

import numpy as np
import pytest

from scalable_collision_avoidance_rl_amd import _native
from scalable_collision_avoidance_rl_amd import obstacles as OB
from scalable_collision_avoidance_rl_amd.shield import ActionShield, check_obstacle_rate
from tests import obstacle_ref as O
from tests import shield_ref as S

BAND_CAP = 0.02                                              # tests/test_gpu_shield.py's cap on the flag band


def fake_env(N=5, obstacles=None):
    return types.SimpleNamespace(batched=True, n_agents=N, n_envs=3, k_closest=2, c=2, device="cpu",
                                 obstacles=np.zeros((0, 3)) if obstacles is None else obstacles)


# ---------------------------------------------------------------------------------------------- parameters and shapes
@pytest.mark.parametrize("bad,match", [
    (np.zeros((3, 2)), r"\[M,3\]"), (np.zeros(3), r"\[M,3\]"), ([[0.0, 0.0, np.nan]], "finite"), ([[np.inf, 0.0, 0.1]], "finite"),
    ([[0.0, 0.0, -0.1]], ">= 0"), (np.zeros((1025, 3)), "at most 1024"), ("discs", r"\[M,3\]")])
def test_field_rejects_bad_obstacles_before_anything_touches_a_device(bad, match):
    with pytest.raises(ValueError, match=match):
        OB.check_obstacles(bad)
    with pytest.raises(ValueError, match=match):
        OB.ObstacleField(fake_env(), bad)
    with pytest.raises(ValueError, match=match):
        OB.ObstacleField(fake_env(obstacles=bad))               # the default: env.obstacles


def test_field_rejects_bad_m_sense_env_and_a_changed_count():
    for m in (0, 5, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="1..4"):
            OB.ObstacleField(fake_env(), np.zeros((2, 3)), m=m)
    for sense in (np.ones(4), np.ones((5, 1)), [np.nan] * 5):
        with pytest.raises(ValueError, match="sense"):
            OB.ObstacleField(fake_env(), np.zeros((2, 3)), sense=sense)
    with pytest.raises(ValueError, match="batched"):
        OB.ObstacleField(types.SimpleNamespace(batched=False), np.zeros((2, 3)))
    assert OB.check_obstacles(np.zeros((0, 3))).shape == (0, 3) and OB.check_obstacles([]).shape == (0, 3)
    assert OB.check_obstacles([[1, 2, 0]]).dtype == np.float64
    with pytest.raises(ValueError, match="fixed at construction"):
        OB.check_obstacles(np.zeros((3, 3)), M=2)
    assert (OB.MAX_OBSTACLES, OB.MAX_SENSE) == (1024, 4)


def test_shield_and_evaluator_reject_a_foreign_field_and_a_bad_obstacle_rate():
    from scalable_collision_avoidance_rl_amd.evaluate import Evaluator
    env = fake_env()
    field = types.SimpleNamespace(env=fake_env())
    with pytest.raises(ValueError, match="ObstacleField of this env"):
        ActionShield(env, obstacles=field)
    with pytest.raises(ValueError, match="needs obstacles"):
        ActionShield(env, obstacle_rate=0.5)
    own = types.SimpleNamespace(env=env)
    for bad in (0.0, 1.5, -0.1, float("nan"), "1", True):
        with pytest.raises(ValueError, match="obstacle_rate"):
            ActionShield(env, obstacles=own, obstacle_rate=bad)
    sh = ActionShield(env, rate=0.3, obstacles=own)
    assert sh.obstacle_rate == 0.3 and ActionShield(env, obstacles=own, obstacle_rate=1.0).obstacle_rate == 1.0
    assert ActionShield(env).obstacles is None and ActionShield(env).obstacle_rate is None
    assert check_obstacle_rate(None, 0.25) == 0.25
    with pytest.raises(ValueError, match="ObstacleField of this env"):
        Evaluator(env, "proportional", safety=True, obstacles=field)
    with pytest.raises(ValueError, match="safety=True"):
        Evaluator(env, "proportional", obstacles=own)


def test_table_function_rejects_shapes_dtypes_and_host_tensors():
    import torch
    T, E, N = 3, 2, 5
    z, done = torch.zeros(T, E, N, 6), torch.zeros(T, E, dtype=torch.uint8)
    xF, radius, obs = torch.zeros(N, 2), torch.zeros(N), torch.zeros(2, 3)
    with pytest.raises(ValueError, match="device tensors only"):
        OB.episode_obstacle_safety(z, done, xF, radius, obs, 2)
    with pytest.raises(ValueError, match=r"\[T,E,N"):
        OB.episode_obstacle_safety(z[0], done, xF, radius, obs, 2)
    with pytest.raises(ValueError, match="tensors"):
        OB.episode_obstacle_safety(z, done.numpy(), xF, radius, obs, 2)


def test_summarize_safety_handles_both_forms():
    import torch
    from scalable_collision_avoidance_rl_amd.evaluate import summarize_safety
    plain = torch.tensor([[4.0, 2, 1, 0.4, 0.05, 1.2, 10, 300], [4.0, 4, 3, 0.8, 0.02, 0.4, 20, 500]], dtype=torch.float64)
    s = summarize_safety(plain)
    assert s["episodes"] == 8 and s["min_clearance"] == 0.02 and "obstacle_free_share" not in s
    both = torch.cat([plain, torch.tensor([[3.0, 1, 0.8, 0.1], [4.0, 3, 1.2, -0.2]], dtype=torch.float64)], 1)
    o = summarize_safety(both)
    assert {k: o[k] for k in s} == s
    assert o["obstacle_free_share"] == 7 / 8 and o["arrived_clear_share"] == 4 / 8
    assert o["min_obstacle_gap"] == -0.2 and o["mean_min_obstacle_gap"] == pytest.approx(2.0 / 8)
    with pytest.raises(ValueError, match="8 figures"):
        summarize_safety(both[:, :10])


# ---------------------------------------------------------------------------------------------- place_obstacles
def test_place_obstacles_draws_the_reference_sizes_and_keeps_points_clear():
    grid = [5.0, 8.0]
    a, b = OB.place_obstacles(grid, 200, seed=4), OB.place_obstacles(grid, 200, seed=4)
    assert a.shape == (200, 3) and a.dtype == np.float64 and np.array_equal(a, b)
    assert not np.array_equal(a, OB.place_obstacles(grid, 200, seed=5))
    assert (a[:, 0] >= 0).all() and (a[:, 0] <= 5).all() and (a[:, 1] <= 8).all() and a[:, 1].max() > 5
    assert a[:, 2].min() >= 0.05 * 0.8 and a[:, 2].max() <= 0.8 and a[:, 2].max() > 0.7      # [0.005, 0.1] max(grid)
    pts = np.array([[1.0, 1.0], [4.0, 6.0], [2.5, 4.0]])
    kept = OB.place_obstacles(grid, 200, seed=4, keep_clear=pts, clearance=0.25)
    d = np.linalg.norm(kept[:, None, :2] - pts[None], axis=2) - kept[:, None, 2]
    assert 0 < kept.shape[0] < 200 and (d > 0.25).all()
    dropped = np.array([row for row in a if not (kept == row).all(1).any()])
    dd = np.linalg.norm(dropped[:, None, :2] - pts[None], axis=2) - dropped[:, None, 2]
    assert (dd.min(1) <= 0.25).all() and kept.shape[0] + dropped.shape[0] == 200
    cen = np.array([[1.0, 2.0], [3.0, 4.0]])
    given = OB.place_obstacles(grid, 2, seed=4, centres=cen)
    assert np.array_equal(given[:, :2], cen) and np.array_equal(given[:, 2], OB.place_obstacles(grid, 2, seed=4)[:, 2])
    assert OB.place_obstacles(grid, 0).shape == (0, 3)
    for kw in (dict(grid=[5.0], n=3), dict(grid=grid, n=-1), dict(grid=grid, n=3, clearance=-1.0), dict(grid=grid, n=3, centres=cen)):
        with pytest.raises(ValueError):
            OB.place_obstacles(**kw)


# ---------------------------------------------------------------------------------------------- exports
def test_library_exports_the_obstacle_entries_with_their_argtypes():
    import scalable_collision_avoidance_rl_amd as pkg
    assert pkg.ObstacleField is OB.ObstacleField and "ObstacleField" in pkg.__all__ and "place_obstacles" in pkg.__all__
    lib = _native.lib()
    header = open(_native.HEADER_PATH).read()
    want = {"dronesim_obstacle_sense": 16, "dronesim_action_shield_obstacles": 21, "dronesim_episode_obstacle_safety": 18}
    for name, n_args in want.items():
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args and fn.argtypes[-1] is C.c_void_p
        decl = header[header.index("int " + name + "("):]
        assert decl[:decl.index(";")].count(",") + 1 == n_args, name
    assert lib.dronesim_action_shield_obstacles.argtypes[-2] is C.c_float
    assert lib.dronesim_version() == 600
    assert "#define DRONESIM_MAX_OBSTACLES 1024" in header and "#define DRONESIM_MAX_SENSE 4" in header


# ---------------------------------------------------------------------------------------------- the restatement, by hand
def test_restatement_matches_the_hand_computed_records():
    e = O.exact_case()
    for m, (oid, orow, gap_min, hit) in e["want"].items():
        r = O.sense(e["z"].reshape(4, 4), e["xF"], e["radius"], e["sense"], e["obstacles"], m)
        assert np.array_equal(r["oid"], oid) and np.array_equal(r["orow"], orow)
        assert np.array_equal(r["gap_min"], gap_min, equal_nan=True) and np.array_equal(r["hit"], hit.astype(bool))
    # M = 0: empty slots, +inf, no hit
    r = O.sense(e["z"].reshape(4, 4), e["xF"], e["radius"], e["sense"], np.zeros((0, 3)), 2)
    assert (r["oid"] == -1).all() and (r["orow"] == 0).all() and np.isposinf(r["gap_min"][[0, 1, 3]]).all() and not r["hit"].any()


def test_restatement_constraints_by_hand():
    """One record: radius 0.125, disc r 0.25 at p = (0.75, 0): d 0.75, g = 0.75 - 0.125 - 0.25 - 0.05 = 0.325, b = 0.5 g / 0.05."""
    orow, oid = np.array([[[0.75, 0.0, 0.25], [0.0, 0.0, 0.0]]]), np.array([[0, -1]])
    A, B, on = O.obstacle_constraints(orow, oid, [0.125], 1, 0.5, 0.05, 0.05)
    assert np.array_equal(on, [[True, False]]) and np.array_equal(A[0, 0], [1.0, 0.0]) and B[0, 0] == pytest.approx(3.25) and np.isinf(B[0, 1])
    z, nbr = np.zeros((1, 4)), np.array([[0, -1]])
    ref = O.shield(np.array([[5.0, 0.5]]), z, nbr, [0.125], 0.25, 0.05, np.inf, 0.05, 2, orow, oid, 1, 0.5)
    assert np.allclose(ref["ustar"], [[3.25, 0.5]]) and ref["intervened"][0] and ref["A"].shape == (1, 4 + 1 + 2, 2)
    # an id outside [0, M), a zero row and a NaN row are skipped; inside the margin b = 0
    for row, o in (([0.75, 0.0, 0.25], 1), ([0.75, 0.0, 0.25], -1), ([0.0, 0.0, 0.25], 0), ([np.nan, 0.0, 0.25], 0)):
        assert not O.obstacle_constraints(np.array([[row]]), np.array([[o]]), [0.125], 1, 0.5, 0.05, 0.05)[2].any()
    assert O.obstacle_constraints(np.array([[[0.3, 0.0, 0.25]]]), np.array([[0]]), [0.125], 1, 0.5, 0.05, 0.05)[1][0, 0] == 0.0


def test_restatement_episode_tables_by_hand():
    """N = 1, one disc at (2, 0) r 0.5, radius 0.25, goal 0: positions x = 0, 1, 1.25, 3 -> gaps 1.25, 0.25, 0, 0.25."""
    z = np.zeros((4, 3, 1, 4))
    z[:, :, 0, 0] = np.array([0.0, 1.0, 1.25, 3.0])[:, None]
    done = np.zeros((4, 3), np.uint8)
    done[2, 1] = done[3, 1] = 1                                                    # env 1: L = 3 (the first end); env 2: L = 1
    done[0, 2] = 1
    zf = np.zeros_like(z)
    zf[:, :, 0, 0] = 1.5                                                           # the end step's observation: gap -0.25
    args = (np.zeros((1, 2)), [0.25], [[2.0, 0.0, 0.5]])
    t = O.episode_tables(z, done, *args)
    assert t["ep_len"].tolist() == [0, 3, 1] and np.isnan(t["min_obstacle_gap"][0, 0]) and t["obstacle_hit_steps"][:, 0].tolist() == [0, 1, 0]
    assert t["min_obstacle_gap"][1:, 0].tolist() == [0.0, 1.25] and t["ep_obstacle_hit_steps"].tolist() == [0, 1, 0]
    t = O.episode_tables(z, done, *args, z_final=zf)
    assert t["min_obstacle_gap"][1:, 0].tolist() == [-0.25, -0.25] and t["obstacle_hit_steps"][:, 0].tolist() == [0, 1, 1]
    assert np.isnan(t["ep_min_obstacle_gap"][0]) and t["ep_min_obstacle_gap"][1:].tolist() == [-0.25, -0.25]
    empty = O.episode_tables(z, done, args[0], args[1], np.zeros((0, 3)))
    assert np.isposinf(empty["min_obstacle_gap"][1:]).all() and empty["ep_obstacle_hit_steps"].sum() == 0


# ---------------------------------------------------------------------------------------------- the generators' conditions
@pytest.mark.parametrize("Mm", O.SENSE_CASES, ids=lambda c: "M%dm%d" % c)
def test_sense_records_are_separated_and_none_is_left_out(Mm):
    M, m = Mm
    for N, k, c in S.CASES:
        case = O.sense_case(N, k, c, M, m)
        E = S.E_CASE
        assert case["z"].shape == (E, N, (k + 1) * c) and case["z"].dtype == np.float32 and case["obstacles"].shape == (M, 3)
        R = E * N
        G = O.gaps(case["z"].reshape(R, -1), case["xF"], case["radius"], case["obstacles"])[1]
        reach = case["sense"].astype(np.float64)[np.arange(R) % N]
        first = np.sort(G, axis=1)[:, :m + 1]
        v = np.sort(np.concatenate([first, reach[:, None], np.zeros((R, 1))], 1), axis=1)
        assert (np.diff(v, axis=1) > 1e-4).all()                                  # every record: none left out
    if M >= 16:                                                                    # (N = 5 case) the list is used: slots filled and empty, hits
        r = O.sense(case["z"].reshape(R, -1), case["xF"], case["radius"], case["sense"], case["obstacles"], m)
        assert (r["oid"] >= 0).any() and r["hit"].any()


def test_shield_cases_bind_obstacle_half_planes_and_stay_under_the_band_cap():
    for (N, k, c), kw in [((9, 8, 2), dict(M=64, reach=3.0)), ((1, 1, 2), {}), ((5, 2, 2), {}), ((5, 2, 5), {})]:
        case = O.shield_case(N, k, c, **kw)
        orow, oid = O.case_list(case, 4)
        ref = O.shield_reference(case, c, orow, oid)
        n_nb = 4 + k
        act = S.active(dict(A=ref["A"], B=ref["B"], on=ref["on"], ustar=ref["ustar"]))
        band = ref["min_slack"] <= ref["tol"]
        print(f"{(N, k, c)}: listed discs per record {ref['on'][:, n_nb:].sum(1).mean():.2f}, an obstacle half-plane active "
              f"{act[:, n_nb:].any(1).mean():.3f}, intervened {ref['intervened'].mean():.3f}, band {band.mean():.4f}, tol {ref['tol']:.2e}")
        assert band.mean() <= BAND_CAP
        assert act[:, n_nb:].any(1).mean() >= 0.05                                 # obstacle half-planes decide answers
        if k == 8:                                                                 # all 16 constraints bound to something
            full = ref["on"].all(1)
            # (`synthetic` makes one neighbour slot in ten a ghost: 0.9^8 = 0.43 of the records list all eight)
            assert ref["on"].shape[1] == 16 and full.mean() >= 0.3
            assert (act[full].sum(1) >= 2).any()


def test_window_has_every_kind_of_env_and_hits():
    for with_final in (True, False):
        w = O.window(with_final=with_final)
        t = O.episode_tables(w["z"], w["done"], w["xF"], w["radius"], w["obstacles"], w["z_final"])
        assert sorted(set(t["ep_len"].tolist())) == [0, 1, 4, 5, 12]
        assert t["obstacle_hit_steps"][1, 0] == 1 and t["min_obstacle_gap"][1, 0] == 0.0       # the exact touch counts
        assert (t["ep_obstacle_hit_steps"] > 0).sum() >= 4 and (t["obstacle_hit_steps"] == 0).sum() >= 10
        flat = w["z"].reshape(-1, w["z"].shape[-1])
        g = O.gaps(flat, w["xF"], w["radius"], w["obstacles"])[1].min(1)
        assert (np.abs(g) > 1e-4).sum() == g.size - 1                              # all but the touch are 1e-4 off gap = 0


def test_closed_loop_restatement_predicts_hits_without_and_none_with_the_obstacle_half_planes():
    su = O.loop_setup()
    assert su["obstacles"].shape[0] >= 3 and su["starts"].shape == (O.LOOP["E"], O.LOOP["N"], 2)
    assert O.LOOP["delta"] > np.sqrt(2) * S.U_MAX * S.DT + O.LOOP["margin"]       # the guarantee's condition on the range
    plain, shielded = O.closed_loop(su, False), O.closed_loop(su, True)
    predicted = plain["min_gap"] < -O.HIT_DEPTH
    print(f"plain shield: envs predicted to hit {predicted.sum()} / {predicted.size}, deepest {plain['min_gap'].min():.3f}; with the discs "
          f"listed: smallest gap {shielded['min_gap'].min():.4f}, largest shortfall of the guarantee {shielded['shortfall']:.2e}")
    assert predicted.sum() >= 1
    assert shielded["hit_steps"].sum() == 0 and shielded["min_gap"].min() >= O.LOOP["margin"] - 1e-9
    assert shielded["shortfall"] <= 1e-9


# ---------------------------------------------------------------------------------------------- episode tables on every scan path
def same_tables(a, b):
    return all(a[n].dtype == b[n].dtype and np.array_equal(a[n], b[n], equal_nan=a[n].dtype.kind == "f") for n in O.TABLES)


@pytest.mark.parametrize("with_final", [True, False], ids=["z_final", "no z_final"])
@pytest.mark.parametrize("c", [2, 5])
def test_vectorised_tables_equal_the_loop_restatement_exactly(c, with_final):
    w = O.window(c=c, with_final=with_final)
    args = (w["z"], w["done"], w["xF"], w["radius"], w["obstacles"], w["z_final"])
    assert same_tables(O.episode_tables(*args), O.episode_tables_fast(*args))
    w = O.window_case(12, 15, 5, c, 3, with_final=with_final)                      # (unequal radii, a NaN record, ends at every step)
    args = (w["z"], w["done"], w["xF"], w["radius"], w["obstacles"], w["z_final"])
    assert same_tables(O.episode_tables(*args), O.episode_tables_fast(*args))
    none = (w["z"], w["done"], w["xF"], w["radius"], np.zeros((0, 3)), w["z_final"])
    assert same_tables(O.episode_tables(*none), O.episode_tables_fast(*none))


@pytest.mark.parametrize("shape,why", O.WINDOW_SHAPES, ids=["T%dE%dN%d" % s for s, _ in O.WINDOW_SHAPES])
def test_window_shapes_take_the_scan_path_they_are_there_for(shape, why):
    """`ScanCols` restated (`obstacle_ref.scan_waves`): a span of at most 7 envs means the cooperative flag fetch.  If someone
    changes a shape, its reason must stay true."""
    T, E, N = shape
    waves = [w for w in O.scan_waves(E, N) if w["active"]]
    stages, rest = divmod(T, O.STAGE_T)
    if shape == (12, 15, 5):
        assert [(w["active"], w["e_first"], w["span"], w["coop"]) for w in waves] == [(64, 0, 12, False), (11, 12, 2, True)]
        assert waves[1]["e_first"] + 8 > E                                         # the fetch of wave 1 asks for envs 15..19: masked
    elif shape == (17, 40, 8):
        assert len(waves) == 5 and all(w["coop"] and w["span"] == 7 and w["active"] == 64 for w in waves)
        assert E * N > 256 and (stages, rest) == (2, 1)
    elif shape == (8, 30, 12):
        assert all(w["coop"] for w in waves) and sum((64 * n) % N != 0 for n in range(len(waves))) >= 3 and (stages, rest) == (1, 0)
    elif shape == (9, 7, 64):
        assert [(w["e_first"], w["span"]) for w in waves] == [(e, 0) for e in range(7)] and (stages, rest) == (1, 1)
    elif shape == (7, 70, 1):
        assert (waves[0]["span"], waves[0]["coop"]) == (63, False) and waves[1]["coop"] and waves[1]["active"] == 6 and stages == 0
    elif shape == (1, 3, 1):
        assert len(waves) == 1 and waves[0]["active"] == 3
    else:
        assert shape == (3, 1, 1024) and O.WINDOW_M[shape] == OB.MAX_OBSTACLES and len(waves) == 16      # 4 workgroups of 4 waves


@pytest.mark.parametrize("shape", [s for s, _ in O.WINDOW_SHAPES], ids=lambda s: "T%dE%dN%d" % s)
def test_window_cases_hold_what_they_promise(shape):
    """Separation (none left out but the touch and the NaN record), unequal radii, distinct goals, the ends of `done_patterns`
    with both sides of every stage seam, and the touch / NaN records in the float64 tables."""
    T, E, N = shape
    M = O.WINDOW_M.get(shape, 3)
    pats = O.done_patterns(T)
    assert [T - 1] in pats and [] in pats and [0] in pats and list(range(T)) in pats
    for s in range(1, T // O.STAGE_T + 1):
        assert [T - O.STAGE_T * s] in pats and (T - 1 - O.STAGE_T * s < 0 or [T - 1 - O.STAGE_T * s] in pats)
    if T >= 2:
        assert any(len(p) == 2 and p[1] == p[0] + 1 for p in pats)
    for c in (2, 5):
        for with_final in (True, False):
            w = O.window_case(T, E, N, c, M, with_final=with_final)
            assert w["z"].shape == (T, E, N, 3 * c) and w["z"].dtype == np.float32 and w["obstacles"].shape == (M, 3)
            assert len(np.unique(w["radius"])) == N and len(np.unique(w["xF"], axis=0)) == N
            for e in range(E):
                assert np.flatnonzero(w["done"][:, e]).tolist() == pats[e % len(pats)]
            for z in [w["z"]] + ([w["z_final"]] if with_final else []):
                g = O.gaps(z.reshape(-1, 3 * c), w["xF"], w["radius"], w["obstacles"])[1].min(1).reshape(T, E, N)
                placed = np.zeros((T, E, N), bool)
                placed[w["touch"]] = True
                if w["nan"] is not None:
                    placed[w["nan"]] = True
                    assert np.isnan(g[w["nan"]])
                assert (np.abs(g) > O.SEPARATION)[~placed].all()                   # none left out but the two placed by hand
            t = O.episode_tables_fast(w["z"], w["done"], w["xF"], w["radius"], w["obstacles"], w["z_final"])
            assert t["ep_len"][0] == T and t["obstacle_hit_steps"][0, 0] >= 1 and (T > 1 or M > 3 or t["min_obstacle_gap"][0, 0] == 0.0)
            zt = (w["z_final"] if with_final and T == 1 else w["z"])[0, 0, 0]
            touch = O.gaps(zt[None], w["xF"][:1], w["radius"][:1], w["obstacles"])[1][0]
            assert touch[0] == 0.0 and (M > 3 or touch.min() == 0.0)               # the touch: exactly 0 (among many discs another may overlap)
            if w["nan"] is not None:
                tn, en, an = w["nan"]
                assert tn < t["ep_len"][en] and np.isnan(t["min_obstacle_gap"][en, an]) and np.isnan(t["ep_min_obstacle_gap"][en])
                other = dict(w, z=np.nan_to_num(w["z"], nan=100.0), z_final=None if not with_final else np.nan_to_num(w["z_final"], nan=100.0))
                far = O.episode_tables_fast(other["z"], w["done"], w["xF"], w["radius"], w["obstacles"], other["z_final"])
                assert t["obstacle_hit_steps"][en, an] == far["obstacle_hit_steps"][en, an]           # the NaN step counts no hit
    if E >= 15:
        assert (t["ep_obstacle_hit_steps"] > 0).sum() >= 3 and (t["ep_len"] == 0).any()


# ---------------------------------------------------------------------------------------------- sense: eviction and ties
@pytest.mark.parametrize("Mm", O.SENSE_CASES_EVICT, ids=lambda c: "M%dm%d" % c)
def test_eviction_cases_have_more_discs_in_range_than_slots(Mm):
    """From the restatement alone: the share of records with more discs in range than list slots.  Measured: 1.000 in every
    case but (9, 8, 2) at (70, 3), 0.994 (ranges from [1.5, 2.5] at M = 70)."""
    M, m = Mm
    for N, k, c in (S.CASES if M == 70 else [S.CASES[1], S.CASES[3]]):
        case = O.sense_case(N, k, c, M, m, reach=O.EVICT_REACH[M])
        R = S.E_CASE * N
        r = O.sense(case["z"].reshape(R, -1), case["xF"], case["radius"], case["sense"], case["obstacles"], m)
        reach = case["sense"].astype(np.float64)[np.arange(R) % N]
        assert O.separated(r["G"], reach, m).all()                                 # every record: none left out
        share = (r["n_in"] > m).mean()
        print(f"M={M} m={m} {(N, k, c)}: more discs in range than slots in {share:.3f} of the records")
        assert share > 0.5


@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_ordered_lists_make_record_0_insert_in_front_every_time_and_never(order):
    N, k, c = S.CASES[1]
    case = O.sense_case(N, k, c, 70, 4, reach=O.EVICT_REACH[70], order=order)
    plain = O.sense_case(N, k, c, 70, 4, reach=O.EVICT_REACH[70])
    assert np.array_equal(case["z"], plain["z"]) and not np.array_equal(case["obstacles"], plain["obstacles"])
    assert np.array_equal(np.sort(case["obstacles"], axis=0), np.sort(plain["obstacles"], axis=0))
    R = S.E_CASE * N
    r = O.sense(case["z"].reshape(R, -1), case["xF"], case["radius"], case["sense"], case["obstacles"], 4)
    step = np.diff(r["G"][0])
    assert (step < 0).all() if order == "descending" else (step > 0).all()
    assert r["n_in"][0] > 4 and (r["n_in"] > 4).mean() > 0.5
    want = [69, 68, 67, 66] if order == "descending" else [0, 1, 2, 3]
    assert r["oid"][0].tolist() == want
    reach = case["sense"].astype(np.float64)[np.arange(R) % N]
    assert O.separated(r["G"], reach, 4).all()


def test_tie_case_by_hand_under_the_restatement():
    t = O.tie_case()
    tied = [o for o in range(18) if o not in (0, 3, 8, 15, 16, 17)]
    z = t["z"].reshape(5, 4)
    G = O.gaps(z, t["xF"], t["radius"], t["obstacles"])[1]
    assert len(tied) == 12 and (G[:4][:, tied] == 0.375).all() and G[0, 15] == 0.25 and G[0, 16] == 0.125    # ties: bit for bit
    p = (t["obstacles"][tied, :2] - np.float32([2.0, 2.0])).astype(np.float32)
    assert (np.float32(p[:, 1] * p[:, 1]) + np.float32(p[:, 0] * p[:, 0]) == np.float32(25 / 64)).all()   # every product and sum exact
    assert t["sense"][1] == 0.375 and t["sense"][2] < 0.375 and np.float32(t["sense"][2]) == t["sense"][2] and np.isposinf(t["sense"][3])
    for m in (1, 2, 3, 4):
        r = O.sense(z, t["xF"], t["radius"], t["sense"], t["obstacles"], m)
        assert np.array_equal(r["oid"], t["want"][m][0]) and np.array_equal(r["orow"], t["want"][m][1]), m
        assert np.array_equal(r["gap_min"], t["gap_min"]) and np.array_equal(r["hit"], t["hit"].astype(bool))
    assert r["n_in"].tolist() == [15, 14, 2, 18, 1]
    assert t["want"][4][0].tolist() == [[16, 15, 1, 2], [16, 15, 1, 2], [16, 15, -1, -1], [16, 15, 1, 2], [0, -1, -1, -1]]


# ---------------------------------------------------------------------------------------------- shield: every m, families, the on rule
def test_sweep_cases_evict_bind_list_slots_and_stay_under_the_band_cap():
    """From the restatement alone.  Measured: every record has more discs in range than m; a list slot is active at u* in
    0.065 .. 0.156 of the records (0.076 at (5, 2, 2) m = 1, 0.135 at (9, 8, 2) m = 1); the flag band is empty."""
    for shape, m, orate, pset in O.SHIELD_SWEEP:
        N, k, c = shape
        case = O.sweep_case(shape, pset)
        ref, orow, oid = O.sweep_reference(case, shape, m, orate, pset)
        s = O.sense(case["z"].reshape(S.E_CASE * N, -1), case["xF"], case["radius"], case["sense"], case["obstacles"], m)
        act = S.active(dict(A=ref["A"], B=ref["B"], on=ref["on"], ustar=ref["ustar"]))[:, 4 + k:].any(1).mean()
        band = (ref["min_slack"] <= ref["tol"]).mean()
        print(f"{shape} m={m} obstacle_rate={orate} {pset}: more in range than m {(s['n_in'] > m).mean():.3f}, a list slot active {act:.3f}, band {band:.4f}")
        assert (s["n_in"] > m).mean() > 0.5 and act >= 0.05 and band <= BAND_CAP and ref["on"][:, 4 + k:].all()
        if pset == "free":
            assert len(np.unique(case["radius"])) == N and np.isinf(ref["B"][:, :4]).all()


@pytest.fixture(scope="module")
def fams():
    return S.families()


# the smallest share of records whose float64 answer has a LIST slot active, per converted family
LIST_ACTIVE_FLOOR = {"duplicates": 0.1, "antipodal": 0.25, "crowd": 0.7, "near_parallel rate 0.25 box one": 0.35,
                     "near_parallel rate 0.25 box both": 0.9, "near_parallel rate 0.25 no box one": 0.35,
                     "near_parallel rate 0.25 no box both": 0.9, "wedge": 0.95, "axes": 0.2, "crowd permuted": 0.7,
                     "antipodal own radius": 0.2, "crowd own radius": 0.6}


@pytest.mark.parametrize("name", O.LIST_FAMILY_NAMES)
def test_converted_families_keep_the_feasible_set_and_bind_list_slots(fams, name):
    """A family with lines moved into the list (obstacle_rate = rate, r_o the neighbour's radius) has the family's own answer
    (within 1e-12; measured: 0, the candidates are the same); per family, the share of records with a list slot active at u*
    (`S.active` on the appended columns) and the flag band.  Measured shares: duplicates 0.160, antipodal 0.341, crowd 0.817,
    near_parallel box one 0.458 / both 0.961, no box one 0.455 / both 1.000, wedge 0.992, axes 0.297, crowd permuted 0.828,
    antipodal own radius 0.296, crowd own radius 0.726."""
    conv, orate = O.list_family(fams, name)
    own = name.endswith(" own radius")
    base = fams[O.LIST_FAMILIES[name[:-len(" own radius")] if own else name][0]]
    E, N, k1 = conv["nbr"].shape
    m = conv["oid"].shape[2]
    assert np.array_equal(conv["z"], base["z"]) and conv["orow"].dtype == np.float32 and conv["oid"].dtype == np.int32
    assert conv["oid"].max() < O.LIST_M and (orate == 1.0) == own
    act, band = [], []
    for label, e0, e1 in conv["blocks"]:
        ref = O.list_block_reference(conv, e0, e1, orate)
        assert ref["A"].shape[1] == 4 + (k1 - 1) + m
        if not own:
            orig = S.block_reference(base, e0, e1)
            assert np.abs(ref["ustar"] - orig["ustar"]).max() <= 1e-12 and np.array_equal(ref["intervened"], orig["intervened"])
            assert np.array_equal(np.sort(ref["B"], axis=1)[:, :orig["B"].shape[1]], np.sort(orig["B"], axis=1))   # the same lines
        act.append(S.active(dict(A=ref["A"], B=ref["B"], on=ref["on"], ustar=ref["ustar"]))[:, 4 + k1 - 1:].any(1))
        band.append(ref["min_slack"] <= ref["tol"])
    act, band = np.concatenate(act), np.concatenate(band)
    print(f"{name}: a list slot active in {act.mean():.3f} of {act.size} records, flag band {band.mean():.4f}")
    assert act.mean() >= LIST_ACTIVE_FLOOR[name] and band.mean() <= BAND_CAP
    if name.startswith("crowd"):                                                   # 4 + 8 + 4: the whole capacity of the solve
        assert ref["A"].shape[1] == 16 and (conv["oid"] >= 0).all(2).mean() >= 0.2
        point = conv["point"]
        assert (act & point).sum() >= 100                                          # where 0 is the only feasible action too
    if own:
        neighbour = base["radius"][np.maximum(base["nbr"].reshape(E * N, k1), 0)[np.arange(E * N)[:, None], conv["moved"]]]
        live = conv["oid"].reshape(E * N, m)[:, :conv["moved"].shape[1]] >= 0
        assert (conv["orow"].reshape(E * N, m, 3)[:, :conv["moved"].shape[1], 2] != neighbour)[live].all()


def test_off_lists_are_off_and_the_mixed_ones_keep_three_live_slots():
    case = O.shield_case(5, 2, 2)
    M = case["obstacles"].shape[0]
    for live in (0, 3):
        orow, oid = O.off_lists(case, 4, live)
        on = O.obstacle_constraints(orow.reshape(-1, 4, 3), oid.reshape(-1, 4), case["radius"], M, 0.5, S.MARGIN, S.DT)[2]
        assert (on.sum(1) == live).all()
        flat_id, flat_row = oid.reshape(-1), orow.reshape(-1, 3)
        off = ~on.reshape(-1)
        kinds = [(flat_id == -1) & (flat_row[:, :2] != 0).any(1), flat_id == M, flat_id == O.INT32_MIN,
                 (flat_id >= 0) & (flat_id < M) & (flat_row[:, :2] == 0).all(1), np.isinf(flat_row[:, :2]).any(1), np.isnan(flat_row[:, :2]).any(1)]
        assert all((kind & off).sum() >= 20 for kind in kinds) and (np.logical_or.reduce(kinds) == off).all()
    ref = O.shield_reference(case, 2, orow, oid)
    act = S.active(dict(A=ref["A"], B=ref["B"], on=ref["on"], ustar=ref["ustar"]))[:, 6:].any(1).mean()
    print(f"mixed lists: a list slot active {act:.3f}, band {(ref['min_slack'] <= ref['tol']).mean():.4f}, tol {ref['tol']:.2e}")
    assert act >= 0.05 and (ref["min_slack"] <= ref["tol"]).mean() <= BAND_CAP and np.isfinite(ref["tol"])
