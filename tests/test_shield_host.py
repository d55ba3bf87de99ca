"""Action shield, the parts that need no GPU: the float64 restatement's own properties, the closed loop that shows the GPU test's
shapes are meaningful, `ActionShield`'s and `step(execute=)`'s argument checks, the header against the binding."""
import ctypes as C
import types

import numpy as np
import pytest

from scalable_collision_avoidance_rl_amd import _native
from tests import shield_ref as S

NEW_SYMBOLS = ("dronesim_action_shield", "dronesim_shield_totals")


@pytest.fixture(scope="module")
def refs():
    return {case: S.case_reference(*case) for case in S.CASES}


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "N%dk%dc%d" % c)
def test_zero_is_feasible_and_the_projection_is_feasible_and_idempotent(refs, case):
    r = refs[case]
    assert (r["B"] >= 0).all()                                                     # 0 satisfies every constraint
    R = r["ustar"].shape[0]
    zero = S.project(np.zeros((R, 2)), r["A"], r["B"], r["on"])
    assert np.array_equal(zero, np.zeros((R, 2)))
    slack = (r["A"] * r["ustar"][:, None, :]).sum(2) - r["B"]
    assert slack.max() <= 1e-11
    again = S.project(r["ustar"], r["A"], r["B"], r["on"])
    assert np.abs(again - r["ustar"]).max() <= 1e-11
    assert r["intervened"].any() and not r["intervened"].all()                     # both branches are drawn
    # never farther from u than 0 is (0 is feasible), and where nothing is violated u itself
    u = r["u"].reshape(R, 2).astype(np.float64)
    assert (np.linalg.norm(r["ustar"] - u, axis=1) <= np.linalg.norm(u, axis=1) + 1e-12).all()
    assert np.array_equal(r["ustar"][~r["intervened"]], u[~r["intervened"]])


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "N%dk%dc%d" % c)
def test_the_projection_is_one_lipschitz_in_u(refs, case):
    r = refs[case]
    R = r["ustar"].shape[0]
    rng = np.random.default_rng(5)
    u = r["u"].reshape(R, 2).astype(np.float64)
    for scale in (1e-3, 0.3, 2.0):
        v = u + rng.normal(0.0, scale, (R, 2))
        pv = S.project(v, r["A"], r["B"], r["on"])
        assert (np.linalg.norm(pv - r["ustar"], axis=1) <= np.linalg.norm(v - u, axis=1) + 1e-11).all()


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: "N%dk%dc%d" % c)
def test_the_draw_keeps_the_flag_band_under_two_percent(refs, case):
    """Records whose smallest slack |a.u - b| is inside the derived tolerance are left out of the GPU test's flag comparison;
    the draw must keep them under 2 % of a case by itself."""
    r = refs[case]
    assert 0.0 < r["tol"] < 1e-5
    assert (r["min_slack"] <= r["tol"]).mean() <= 0.02
    if case[0] > 1:                                                                # neighbour constraints, negative gaps included
        nb = r["on"][:, S.M_BOX:]
        assert nb.any() and (r["B"][:, S.M_BOX:][nb] == 0).any() and (r["B"][:, S.M_BOX:][nb] > 0).any()
    else:
        assert not r["on"][:, S.M_BOX:].any()


def test_closed_loop_in_float64_unshielded_collides_shielded_does_not():
    """N = 5, k = 4, Delta = 1, rate 0.25, margin 0.05, box 1, 64 lattice starts, 200 steps of proportional control."""
    free, arrived_free = S.closed_loop(5, 4, 64, shielded=False)
    safe, arrived_safe = S.closed_loop(5, 4, 64, shielded=True)
    print("unshielded: envs with a collision", int((free < 0).sum()), "min clearance", free.min(), "arrived", int(arrived_free.sum()))
    print("shielded:   envs with a collision", int((safe < 0).sum()), "min clearance", safe.min(), "arrived", int(arrived_safe.sum()))
    assert (free < 0).sum() >= 1
    assert (safe < 0).sum() == 0 and safe.min() >= 0.02 - 1e-9


def test_ghosts_self_zero_distance_and_nan_rows_are_skipped_and_a_nan_action_goes_through():
    N, k1, c = 3, 4, 2
    z = np.zeros((N, k1, c))
    z[:, 1] = [0.3, 0.0]                                                           # slot 1: a neighbour 0.3 to the right, gap 0.05
    z[:, 2] = [0.0, 0.0]                                                           # slot 2: d = 0
    z[:, 3] = [np.nan, 0.1]                                                        # slot 3: a NaN row
    nbr = np.array([[0, 1, 2, 2], [1, 1, 0, 2], [2, 7, 0, 0]])                     # agent 1 lists itself, agent 2 the id 7
    u = np.array([[1.0, 0.0], [1.0, 0.0], [np.nan, 0.0]])
    out, iv, corr, _ = S.shield(u, z.reshape(N, -1), nbr, np.full(N, 0.1), 0.25, 0.05, 1.0, 0.05, c)
    assert iv.tolist() == [True, False, False]
    assert np.allclose(out[0], [0.25 * 0.05 / 0.05, 0.0]) and np.array_equal(out[1], u[1])
    assert np.isnan(out[2, 0]) and out[2, 1] == 0.0 and np.isnan(corr[2]) and corr[1] == 0.0 and np.isclose(corr[0], 0.75)


# ---- argument checks ------------------------------------------------------------------------------------------------------------
def fake_env(E=3, N=5, k=2, c=2, batched=True):
    import torch
    return types.SimpleNamespace(batched=batched, n_envs=E, n_agents=N, k_closest=k, c=c, device=torch.device("cuda", 0),
                                 z=None, nbr_idx=None, _radius=torch.zeros(N))


@pytest.mark.parametrize("kw", [dict(rate=0.0), dict(rate=0.51), dict(rate=float("nan")), dict(rate="0.25"), dict(rate=True),
                                dict(margin=-1e-9), dict(margin=float("inf")), dict(margin=float("nan")),
                                dict(u_max=0.0), dict(u_max=-1.0), dict(u_max=float("nan"))])
def test_action_shield_refuses_bad_parameters(kw):
    from scalable_collision_avoidance_rl_amd.shield import ActionShield
    with pytest.raises(ValueError):
        ActionShield(fake_env(), **kw)


def test_action_shield_parameters_and_the_batched_requirement():
    from scalable_collision_avoidance_rl_amd import ActionShield
    s = ActionShield(fake_env(), 0.5, 0.0)
    assert (s.rate, s.margin, s.u_max, s.stats) == (0.5, 0.0, float("inf"), False)
    assert s.intervened is None and s.correction is None                           # nothing is allocated before the first call
    with pytest.raises(ValueError, match="batched"):
        ActionShield(fake_env(batched=False))
    with pytest.raises(RuntimeError, match="stats=True"):
        s.totals()


def test_action_shield_checks_shapes_dtypes_and_devices_before_touching_a_device():
    """CPU tensors throughout: every refusal below is raised by the checks, none by a launch."""
    import torch
    from scalable_collision_avoidance_rl_amd.shield import ActionShield, _shield_shapes
    env = fake_env()
    E, N, k1, c = 3, 5, 3, 2
    s = ActionShield(env, 0.25, 0.05, 1.0)
    good = dict(actions=torch.zeros(E, N, 2), z=torch.zeros(E, N, k1 * c), nbr=torch.zeros(E, N, k1, dtype=torch.int32), out=None)
    cpu = torch.device("cpu")
    _shield_shapes(radius=env._radius, E=E, N=N, k1=k1, c=c, device=cpu, **good)   # (the checks pass on a matching device)
    with pytest.raises(ValueError, match="device"):
        s.shield(**good)                                                           # the env lives on cuda:0, these do not
    for name, bad in (("actions", torch.zeros(E, N, 3)), ("actions", torch.zeros(E, N, 2, dtype=torch.float64)),
                      ("actions", np.zeros((E, N, 2), np.float32)), ("z", torch.zeros(E, N, k1 * c + 1)),
                      ("z", torch.zeros(E, N, 2 * k1 * c)[:, :, ::2]), ("nbr", torch.zeros(E, N, k1, dtype=torch.int64)),
                      ("nbr", torch.zeros(E, N, k1 + 1, dtype=torch.int32)), ("out", torch.zeros(E, N)),
                      ("out", torch.zeros(E, N, 2, dtype=torch.float16))):
        with pytest.raises(ValueError, match=name):
            _shield_shapes(radius=env._radius, E=E, N=N, k1=k1, c=c, device=cpu, **dict(good, **{name: bad}))
    with pytest.raises(ValueError, match="c in"):
        _shield_shapes(radius=env._radius, E=E, N=N, k1=k1, c=3, device=cpu, **good)
    assert s.intervened is None and s.calls == 0


def test_step_execute_is_validated_without_a_gpu():
    import torch
    from scalable_collision_avoidance_rl_amd.drone_env import check_execute
    shape, cpu = (3, 5, 2), torch.device("cpu")
    ok = torch.zeros(shape)
    assert check_execute(ok, shape, cpu) is ok
    for bad in (torch.zeros(3, 5, 3), torch.zeros(shape, dtype=torch.float64), np.zeros(shape, np.float32), [[0.0, 0.0]],
                torch.zeros(3, 5, 4)[:, :, ::2]):
        with pytest.raises(ValueError, match="execute"):
            check_execute(bad, shape, cpu)
    with pytest.raises(ValueError, match="device"):
        check_execute(ok, shape, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="batched"):
        check_execute(ok, shape, cpu, batched=False)


def test_evaluator_refuses_a_shield_of_another_env():
    from scalable_collision_avoidance_rl_amd import ActionShield, Evaluator
    env, other = fake_env(), fake_env()
    with pytest.raises(ValueError, match="shield"):
        Evaluator(env, "proportional", shield=ActionShield(other))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_shield_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    want = dict(dronesim_action_shield=[vp, vp, vp, vp, f32, f32, f32, f32, i32, i32, i32, i32, vp, vp, vp, vp],
                dronesim_shield_totals=[vp, vp, i32, i32, vp, vp, vp, vp, vp])
    assert set(want) == set(NEW_SYMBOLS)
    header = open(_native.HEADER_PATH).read()
    kinds = {"const float *": vp, "const int32_t *": vp, "const uint8_t *": vp, "float *": vp, "uint8_t *": vp, "int64_t *": vp,
             "double *": vp, "void *": vp, "float": f32, "int": i32}
    for name, args in want.items():
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert list(fn.argtypes) == args and fn.restype is C.c_int, name
        assert f"int {name}(" in header, name
        params = header.split(f"int {name}(")[1].split(");")[0].replace("\n", " ").split(",")
        declared = []
        for p in params:
            p = " ".join(p.split())
            t = p[:p.rindex("*") + 1] if "*" in p else p.rsplit(" ", 1)[0]
            declared.append(kinds[t])
        assert declared == args, name
    assert lib.dronesim_version() == 600


A_OK = dict(z=4096, nbr=4096, act=4096, radius=4096, rate=0.25, margin=0.05, u_max=1.0, dt=0.05, E=0, N=5, k1=3, c=2, act_out=4096,
            intervened=None, correction=None)


@pytest.mark.parametrize("bad", [dict(z=None), dict(nbr=None), dict(act=None), dict(radius=None), dict(act_out=None),
                                 dict(rate=0.0), dict(rate=0.5001), dict(rate=float("nan")), dict(margin=-0.1), dict(margin=float("nan")),
                                 dict(u_max=0.0), dict(u_max=float("nan")), dict(dt=0.0), dict(dt=-1.0), dict(c=3), dict(k1=1),
                                 dict(k1=_native.MAX_K + 2), dict(N=0), dict(N=_native.MAX_AGENTS + 1), dict(E=-1)],
                         ids=lambda d: "%s=%s" % next(iter(d.items())))
def test_action_shield_entry_point_refuses_bad_arguments(bad):
    """E = 0 enqueues nothing, so the refusals (and the one accepted call) run without a device."""
    lib = _native.lib()
    call = lambda **kw: lib.dronesim_action_shield(*[dict(A_OK, **kw)[n] for n in A_OK], None)
    assert call() == _native.OK
    assert call(u_max=float("inf")) == _native.OK                                  # no box
    assert call(**bad) == _native.EINVAL
    assert b"dronesim_action_shield" in lib.dronesim_last_error()


def test_shield_totals_entry_point_refuses_bad_arguments():
    lib = _native.lib()
    ok = dict(intervened=4096, correction=4096, E=0, N=5, interventions=4096, nonfinite=4096, correction_sum=4096, correction_max=4096)
    call = lambda **kw: lib.dronesim_shield_totals(*[dict(ok, **kw)[n] for n in ok], None)
    assert call() == _native.OK
    for bad in [dict(intervened=None), dict(correction=None), dict(interventions=None), dict(nonfinite=None), dict(correction_sum=None),
                dict(correction_max=None), dict(E=-1), dict(N=0), dict(N=_native.MAX_AGENTS + 1)]:
        assert call(**bad) == _native.EINVAL, bad
        assert b"dronesim_shield_totals" in lib.dronesim_last_error()
