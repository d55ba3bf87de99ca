"""Per-env obstacle sets on the host (no GPU needed; nothing here reaches a launch): every parameter error of
`check_env_obstacles` / ``ObstacleField(per_env=True)`` / `set` / `observe`'s leading dims, raised before a device is touched;
`place_obstacles_per_env` against `place_obstacles`; the header of its own (include/dronesim_env_obstacles.h) parsed and bound;
`dronesim_env_obstacle_plan` against a restatement of the launch geometry, with the reasons of the GPU tests' shape table; and the
separation the generated cases promise, under the float64 restatement alone."""
import ctypes as C
import types

import numpy as np
import pytest

from scalable_collision_avoidance_rl_amd import _native
from scalable_collision_avoidance_rl_amd import obstacles as OB
from tests import env_obstacle_ref as ER
from tests import obstacle_ref as OR


class NoDevice:
    """An env whose device must never be looked at."""
    batched, n_envs, n_agents, k_closest, c = True, 4, 3, 2, 2
    obstacles = np.zeros((0, 3))

    @property
    def device(self):
        raise AssertionError("a device was touched before the arguments were checked")


def good(E=4, M=5):
    obs = np.zeros((E, M, 3))
    obs[..., 2] = 0.1
    return obs


# ---------------------------------------------------------------------------------------------- parameter errors
@pytest.mark.parametrize("what,obstacles,counts,match", [
    ("rank 2", np.zeros((5, 3)), None, r"\[E,M,3\]"),
    ("rank 4", np.zeros((4, 5, 3, 1)), None, r"\[E,M,3\]"),
    ("last dim", np.zeros((4, 5, 2)), None, r"\[E,M,3\]"),
    ("not an array", object(), None, r"\[E,M,3\]"),
    ("E mismatch", good(E=3), None, "E = 4"),
    ("M > 64", good(M=65), None, "at most 64"),
    ("nan", np.full((4, 5, 3), np.nan), None, "finite"),
    ("negative radius", -good(), None, ">= 0"),
    ("counts shape", good(), [1, 2, 3], r"counts must be \[E\]"),
    ("counts float", good(), [1.0, 2.0, 3.0, 4.0], "integers"),
    ("counts bool", good(), [True, False, True, False], "integers"),
    ("counts above M", good(), [0, 1, 5, 6], "0..M"),
    ("counts below 0", good(), [0, -1, 5, 2], "0..M"),
])
def test_field_refuses_bad_lists_before_a_device_is_touched(what, obstacles, counts, match):
    with pytest.raises(ValueError, match=match):
        OB.ObstacleField(NoDevice(), obstacles, per_env=True, counts=counts)
    if what != "E mismatch":
        with pytest.raises(ValueError, match=match):
            OB.check_env_obstacles(obstacles, counts)


def test_padding_rows_are_checked_too_and_the_shared_field_still_refuses_three_dims():
    obs = good()
    obs[2, 4, 0] = np.inf                                      # a row behind the env's count: uploaded all the same
    with pytest.raises(ValueError, match="finite"):
        OB.check_env_obstacles(obs, [1, 1, 1, 1])
    with pytest.raises(ValueError, match=r"\[M,3\]"):
        OB.ObstacleField(NoDevice(), good())                   # without per_env
    with pytest.raises(ValueError, match="per_env"):
        OB.ObstacleField(NoDevice(), np.zeros((0, 3)), counts=[0, 0, 0, 0])
    with pytest.raises(ValueError, match="per_env=True needs obstacles"):
        OB.ObstacleField(NoDevice(), per_env=True)
    obs, cnt = OB.check_env_obstacles(good(), None)
    assert obs.dtype == np.float64 and cnt.dtype == np.int64 and cnt.tolist() == [5] * 4
    assert OB.check_env_obstacles(np.zeros((4, 0, 3)))[1].tolist() == [0] * 4


def bare_field(E=4, M=5, N=3):
    """A per-env field as `__init__` leaves it, without a device: what `set` and `observe` check before they reach one."""
    f = OB.ObstacleField.__new__(OB.ObstacleField)
    f.env, f.per_env, f.M, f.m = NoDevice(), True, M, 2
    return f


def test_set_refuses_a_changed_M_another_E_and_bad_counts():
    f = bare_field()
    for obstacles, counts, match in ((good(M=4), None, "fixed at construction"), (good(M=6), None, "fixed at construction"),
                                     (good(E=5), None, "E = 4"), (good(), [0, 0, 0, 9], "0..M"), (good() * np.nan, None, "finite")):
        with pytest.raises(ValueError, match=match):
            f.set(obstacles, counts)
    shared = OB.ObstacleField.__new__(OB.ObstacleField)
    shared.env, shared.per_env, shared.M = NoDevice(), False, 0
    with pytest.raises(ValueError, match="per_env"):
        shared.set(np.zeros((0, 3)), counts=[0])


def test_observe_refuses_leading_dims_that_do_not_end_in_E():
    import torch
    f = bare_field()
    f.env = types.SimpleNamespace(batched=True, n_envs=4, n_agents=3, k_closest=2, c=2, device="cpu", z=None)
    for shape in ((3, 6), (5, 3, 6), (4, 2, 3, 6)):
        with pytest.raises(ValueError, match="end in E = 4"):
            f.observe(torch.zeros(shape))


# ---------------------------------------------------------------------------------------------- placement
def test_place_obstacles_per_env_is_place_obstacles_per_env_and_reproducible():
    grid, n, E = [5.0, 4.0], 8, 6
    pts = np.array([[1.0, 1.0], [4.0, 3.0], [2.5, 2.0]])
    obs, cnt = OB.place_obstacles_per_env(grid, n, E, seed=3, keep_clear=pts, clearance=0.2)
    assert obs.shape == (E, n, 3) and obs.dtype == np.float64 and cnt.shape == (E,) and cnt.dtype == np.int64
    for e in range(E):
        want = OB.place_obstacles(grid, n, seed=[3, e], keep_clear=pts, clearance=0.2)
        assert cnt[e] == want.shape[0] and np.array_equal(obs[e, :cnt[e]], want) and not obs[e, cnt[e]:].any()
    assert len({obs[e].tobytes() for e in range(E)}) == E and cnt.min() < n    # the envs differ, and some list is padded
    again = OB.place_obstacles_per_env(grid, n, E, seed=3, keep_clear=pts, clearance=0.2)
    assert np.array_equal(again[0], obs) and np.array_equal(again[1], cnt)
    assert not np.array_equal(OB.place_obstacles_per_env(grid, n, E, seed=4)[0], OB.place_obstacles_per_env(grid, n, E, seed=3)[0])
    OB.check_env_obstacles(obs, cnt, E=E, M=n)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            OB.place_obstacles_per_env(grid, n, bad)
    import scalable_collision_avoidance_rl_amd as pkg
    assert pkg.place_obstacles_per_env is OB.place_obstacles_per_env and "place_obstacles_per_env" in pkg.__all__


# ---------------------------------------------------------------------------------------------- the header
NAMES = ("dronesim_env_obstacle_plan", "dronesim_env_obstacle_sense", "dronesim_env_obstacle_observe", "dronesim_env_obstacle_reward",
         "dronesim_episode_env_obstacle_safety")


def test_the_header_parses_and_its_names_are_bound_on_the_library():
    constants, signatures = _native.parse_header(open(_native.ENV_OBSTACLES_HEADER_PATH).read())
    assert tuple(signatures) == NAMES == _native.ENV_OBSTACLE_SYMBOLS
    assert constants == {"MAX_ENV_OBSTACLES": 64} and _native.MAX_ENV_OBSTACLES == 64 == OB.MAX_ENV_OBSTACLES
    assert not set(NAMES) & set(_native.SYMBOLS) and not set(NAMES) & set(_native.SIGNATURES)
    assert "MAX_ENV_OBSTACLES" not in open(_native.HEADER_PATH).read()
    lib = _native.lib()
    for name in NAMES:
        fn, sig = getattr(lib, name), _native.ENV_OBSTACLE_SIGNATURES[name]
        assert fn.argtypes == sig.argtypes and fn.restype is C.c_int and _native.signature(name) is sig
        assert sig.stream == (name != "dronesim_env_obstacle_plan")
    assert _native.ENV_OBSTACLE_SIGNATURES[NAMES[0]].argtypes[-1] is _native._MIRRORS["size_t"]
    assert _native.signature("dronesim_obstacle_sense") is _native.SIGNATURES["dronesim_obstacle_sense"]
    with pytest.raises(KeyError, match="dronesim_no_such"):
        _native.signature("dronesim_no_such")


def test_a_missing_header_is_an_import_error_naming_the_path(tmp_path):
    with pytest.raises(ImportError, match="dronesim_env_obstacles.h"):
        _native._read_header(str(tmp_path / "dronesim_env_obstacles.h"))


def test_entries_refuse_bad_arguments_under_their_own_name():
    lib, p = _native.lib(), 4096                               # (a fake non-NULL address: no case reaches a launch)
    calls = {
        "dronesim_env_obstacle_sense": lambda M, obs: lib.dronesim_env_obstacle_sense(p, p, p, p, obs, None, 2, 3, 3, 2, M, 2, p, p, None, None, None),
        "dronesim_env_obstacle_observe": lambda M, obs: lib.dronesim_env_obstacle_observe(p, p, p, p, obs, None, 4, 2, 3, 3, 2, M, 2, p, None, 0.0, None),
        "dronesim_env_obstacle_reward": lambda M, obs: lib.dronesim_env_obstacle_reward(p, None, p, p, p, p, p, obs, None, 2, 2, 3, 3, 2, M, 0.0, p, None, None),
        "dronesim_episode_env_obstacle_safety": lambda M, obs: lib.dronesim_episode_env_obstacle_safety(p, None, p, p, p, obs, None, 2, 2, 3, 3, 2, M, p, None, None, None, None, None),
    }
    for name, fn in calls.items():
        for M, obs in ((65, p), (-1, p), (3, None)):
            assert fn(M, obs) == _native.EINVAL
            assert lib.dronesim_last_error().decode().startswith(name + ": M outside 0..64")
    # observe: R must be a multiple of E; an empty batch enqueues nothing and is fine
    assert lib.dronesim_env_obstacle_observe(p, p, p, p, p, None, 5, 2, 3, 3, 2, 4, 2, p, None, 0.0, None) == _native.EINVAL
    assert "multiple of E" in lib.dronesim_last_error().decode()
    assert lib.dronesim_env_obstacle_observe(p, p, p, p, p, None, 3, 0, 3, 3, 2, 4, 2, p, None, 0.0, None) == _native.EINVAL
    assert lib.dronesim_env_obstacle_observe(p, p, p, p, p, None, 0, 2, 3, 3, 2, 4, 2, p, None, 0.0, None) == _native.OK
    assert lib.dronesim_env_obstacle_sense(p, p, p, p, p, None, 0, 3, 3, 2, 4, 2, p, p, None, None, None) == _native.OK
    assert lib.dronesim_env_obstacle_reward(p, None, p, p, p, p, p, p, None, 0, 2, 3, 3, 2, 4, 0.0, p, None, None) == _native.OK
    assert lib.dronesim_episode_env_obstacle_safety(None, None, None, None, None, None, None, 2, 0, 3, 3, 2, 0, None, None, None, None, None, None) == _native.OK


# ---------------------------------------------------------------------------------------------- the plan
def test_plan_matches_the_restated_geometry_and_fits_the_workgroup():
    staged_seen = set()
    for N in (1, 2, 3, 5, 8, 64, 70, 127, 128, 254, 255, 256, 1024):
        for M in (0, 1, 3, 8, 16, 33, 64):
            for m in (1, 4):
                plan = OB.env_obstacle_plan(N, M, m)
                assert plan["rows_per_block"] == ER.rows_per_block(N) == 254 // N + 2
                # no workgroup of a launch over N-record rows touches more rows than the plan says; the bound is that of a workgroup
                # that starts on the last record of a row, which a launch reaches or misses by one row
                most = max(n for _, n in ER.block_rows(N, 256 * N * 4))
                assert plan["rows_per_block"] - 1 <= most <= plan["rows_per_block"]
                parked = 256 * 12 * m                           # the observe kernel's output lists
                assert parked <= plan["lds_bytes"] <= 64 * 1024
                if plan["staged"]:                              # every slot holds a whole list
                    assert plan["lds_bytes"] - parked >= plan["rows_per_block"] * 12 * M > 0
                else:
                    assert plan["lds_bytes"] == parked
                staged_seen.add(plan["staged"])
    assert staged_seen == {True, False}
    for bad in ((0, 8, 2), (1025, 8, 2), (5, -1, 2), (5, 65, 2), (5, 8, 0), (5, 8, 5)):
        with pytest.raises(_native.DroneSimError, match="dronesim_env_obstacle_plan"):
            OB.env_obstacle_plan(*bad)
    rows = C.c_int(0)                                           # any of the three outputs may be NULL
    _native.call("dronesim_env_obstacle_plan", 5, 8, 2, None, C.byref(rows), None)
    assert rows.value == 52


def test_the_shape_table_reaches_both_paths_and_its_reasons_hold():
    paths = {}
    for (E, N, M, m), staged, why in ER.SHAPES:
        plan = OB.env_obstacle_plan(N, M, m)
        if staged is not None:
            assert plan["staged"] == staged, (E, N, M, m, why)
        paths[(E, N, M, m)] = plan["staged"]
    assert set(paths.values()) == {True, False}
    # (7, 5, 8, 2): a wave spans 13 rows, more than E; workgroup 0 of a ring of 8 rows-of-E wraps several times
    assert max(ER.wave_rows(5, 7 * 5)) == 7 and max(ER.wave_rows(5, 8 * 7 * 5)) >= 13 > 7
    assert ER.block_wraps(7, 5, 8 * 7)[0] >= 3 and ER.block_rows(5, 8 * 7 * 5)[0][1] == 52
    # (3, 64, 64, 4): one env per wave; an even 3 M = 192 floats would put every env's disc o into one bank
    assert set(ER.wave_rows(64, 3 * 64)) == {1} and (3 * 64) % 32 == 0
    # (5, 70, 16, 3): waves with an env boundary inside; the last workgroup is ragged
    assert 2 in ER.wave_rows(70, 5 * 70) and (5 * 70) % 256 != 0
    # (300, 1, ...): 256 rows in a workgroup, two workgroups, the second ragged
    assert ER.block_rows(1, 300) == [(0, 256), (256, 44)] and ER.rows_per_block(1) == 256
    assert paths[(300, 1, 64, 4)] is False and paths[(300, 1, 8, 1)] is True and paths[(40, 2, 64, 2)] is False
    # the tables' windows keep E > 1 and hold both a wide and a narrow list
    assert all(E > 1 for (T, E, N), M in ER.WINDOW_SHAPES) and {M for _, M in ER.WINDOW_SHAPES} == {3, 64}
    assert len(ER.WINDOW_SHAPES) == len(OR.WINDOW_SHAPES) - 1


# ---------------------------------------------------------------------------------------------- the generators
@pytest.mark.parametrize("shape", [s for s, _, _ in ER.SHAPES if s[0] <= 40], ids=[str(s) for s, _, _ in ER.SHAPES if s[0] <= 40])
def test_generated_cases_keep_the_separation_under_the_restatement(shape):
    E, N, M, m = shape
    for counts in (None, ER.ragged_counts(E, M)):
        cs = ER.case(E, N, M, m, counts=counts)
        assert ER.separated_everywhere(cs, m)
        planted = ER.plant_on_agents(cs)
        assert np.array_equal(planted["z"], cs["z"]) and ER.separated_everywhere(planted, m)
        for e in range(E):                                     # the planted rows would hit if they were read
            if cs["counts"][e] < M:
                full = OR.sense(cs["z"][e], cs["xF"], cs["radius"], cs["sense"], planted["obstacles"][e], m)
                assert full["hit"].any() and (full["oid"] >= cs["counts"][e]).any()
    if M:
        counts = ER.ragged_counts(E, M)
        assert {0, 1, M} <= set(counts.tolist()) or E < 3


def test_window_cases_keep_every_gap_off_zero_under_their_own_lists():
    (T, E, N), M = ER.WINDOW_SHAPES[0]
    w = ER.window_case(T, E, N, M, counts=ER.ragged_counts(E, M))
    for e in range(1, E):
        for z in (w["z"], w["z_final"]):
            if w["counts"][e]:
                g = OR.gaps(z[:, e].reshape(T * N, -1), w["xF"], w["radius"], ER.env_list(w, e))[1].min(1)
                assert not (np.abs(g) <= OR.SEPARATION).any()
    tables = ER.episode_tables(w)
    assert tables["ep_len"].shape == (E,) and tables["min_obstacle_gap"].shape == (E, N)
    empty = np.flatnonzero((w["counts"] == 0) & (tables["ep_len"] > 0))
    assert empty.size and np.isposinf(tables["min_obstacle_gap"][empty]).all() and not tables["obstacle_hit_steps"][empty].any()
