"""Obstacles on the host (no GPU): parameter and shape errors of `obstacles.py` / `ActionShield(obstacles=)` / `Evaluator(obstacles=)`,
`place_obstacles`, the exports with their argtypes, the float64 restatement tests/obstacle_ref.py against hand-computed cases,
and the conditions the shared generators promise to the GPU tests -- asserted under the restatement alone."""
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
