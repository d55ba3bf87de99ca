"""Host-side tests of the observation normaliser: the float64 restatement (tests/obsnorm_ref.py) against itself -- the windowed
merge against the two-pass moments of the concatenation --, the inputs of the GPU tests (the column a float32 accumulator
fails), the entry points' declarations, the workspace query, every EINVAL, and the host logic of `ObsNormalizer`, the learners'
and the `Evaluator`'s keyword (no GPU needed)."""
import ctypes as C

import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from tests import obsnorm_ref as OR
from tests import test_ppo_host as PH

NEW_SYMBOLS = ("dronesim_obsnorm_workspace", "dronesim_obsnorm_update", "dronesim_obsnorm_apply")


@pytest.mark.parametrize("shape", OR.SHAPES[:2] + [(70, 15)], ids=lambda s: f"N{s[0]}d{s[1]}")
def test_windowed_merge_equals_the_two_pass_moments_of_the_concatenation(shape):
    ws = OR.windows(*shape)
    state = torch.zeros(3, shape[0] * shape[1], dtype=torch.float64)
    for k, w in enumerate(ws):
        before = state.clone()
        state = OR.merge(state, OR.moments(w))
        ref = OR.moments(torch.cat(ws[:k + 1]))
        assert torch.equal(state[0], ref[0])
        assert torch.all((state[1] - ref[1]).abs() <= 1e-12 * OR.column_max(ws[:k + 1]))
        assert torch.allclose(state[2], ref[2], rtol=1e-11, atol=0)
        if k == OR.NAN_WINDOW:
            assert torch.equal(state[:, OR.NAN_COLUMN], before[:, OR.NAN_COLUMN])
    assert float(state[2, OR.CONSTANT]) == 0.0 and float(state[1, OR.CONSTANT]) == OR.CONSTANT_VALUE
    # the inputs are what the GPU tests say they are
    allx = torch.cat(ws)
    assert 0.005 < float(torch.isnan(allx).float().mean()) < 0.02 and not torch.isnan(allx[:, OR.CONSTANT]).any()
    assert int(torch.isinf(allx).sum()) == len(ws) and torch.isnan(ws[OR.NAN_WINDOW][:, OR.NAN_COLUMN]).all()
    assert abs(float(state[1, OR.WIDE]) - 256) < 10 and 40 < float((state[2, OR.WIDE] / state[0, OR.WIDE]).sqrt()) < 70
    assert float((state[2, OR.SMALL] / state[0, OR.SMALL]).sqrt()) < 2e-3


def test_table_and_map_of_the_restatement():
    ws = OR.windows(5, 6)
    state = OR.moments(torch.cat(ws))
    tab = OR.table(state, 1e-8)
    assert torch.equal(tab[0], state[1]) and torch.allclose(tab[1], 1 / torch.sqrt(state[2] / state[0] + 1e-8), rtol=1e-15)
    fresh = OR.table(torch.zeros(3, 30, dtype=torch.float64), 1e-8)
    assert torch.equal(fresh[0], torch.zeros(30, dtype=torch.float64)) and torch.equal(fresh[1], torch.ones(30, dtype=torch.float64))
    x = ws[0]
    y = OR.apply(x, tab, 10.0)
    assert torch.equal(torch.isnan(y), torch.isnan(x)) and float(y[0, OR.INF_COLUMN]) == 10.0
    assert float(OR.apply(x, tab)[0, OR.INF_COLUMN]) == float("inf")
    assert torch.all(y[:, OR.CONSTANT] == 0)
    fin = torch.isfinite(x)
    allx = torch.cat(ws)
    z = OR.apply(allx, tab)[:, OR.HARD]
    z = z[torch.isfinite(z)]
    assert abs(float(z.std(unbiased=False)) - 1) < 1e-6 and abs(float(z.mean())) < 1e-9   # (over everything the state has seen)
    assert torch.equal(OR.apply(x, fresh)[fin], x.double()[fin])


def test_the_hard_column_fails_a_float32_accumulator():
    """The -500 +- 0.5 column does its job: float32 running sums of x and x^2 miss the GPU test's bar on m2 (rtol 1e-10) by many
    orders, so a kernel that passes accumulates wider and shifts before it squares."""
    x = OR.windows(5, 6)[0]
    ref, wrong = OR.moments(x), OR.moments_float32(x)
    assert abs(float(ref[1, OR.HARD]) + 500) < 0.1 and abs(float((ref[2] / ref[0])[OR.HARD]) - 1 / 12) < 0.01
    assert abs(float(wrong[2, OR.HARD] - ref[2, OR.HARD])) > 0.5 * float(ref[2, OR.HARD])


def test_library_exports_the_new_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    want = ("dronesim_obsnorm_workspace", "dronesim_obsnorm_update", "dronesim_obsnorm_apply")
    assert set(want) == set(NEW_SYMBOLS)
    header = open(_native.HEADER_PATH).read()
    for name in want:
        assert name in _native.SYMBOLS and "f64" not in name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert f"int {name}(" in header, name


def test_workspace_query_is_a_pure_function_of_the_shape():
    lib = _native.lib()
    for N, d in OR.SHAPES:
        for R in OR.WINDOW_ROWS + (200 * 4096, 200 * 512):
            a, b = C.c_size_t(0), C.c_size_t(0)
            assert lib.dronesim_obsnorm_workspace(R, N * d, C.byref(a)) == lib.dronesim_obsnorm_workspace(R, N * d, C.byref(b)) == _native.OK
            # [S][3][C] doubles: whole slabs, at least one, and no more than one per row
            assert a.value == b.value and a.value % (24 * N * d) == 0 and 1 <= a.value // (24 * N * d) <= R
    n = C.c_size_t(0)
    for bad in ((0, 5), (-1, 5), (5, 0), (5, -3)):
        assert lib.dronesim_obsnorm_workspace(*bad, C.byref(n)) == _native.EINVAL
        assert lib.dronesim_last_error().startswith(b"dronesim_obsnorm_workspace")
    assert lib.dronesim_obsnorm_workspace(5, 5, None) == _native.EINVAL


UPDATE_OK = dict(x=4096, R=64, C=30, state=8192, table=16384, eps=1e-8, ws=4096, wsb=1 << 20)
APPLY_OK = dict(x=4096, y=8192, R=64, C=30, table=16384, clip=10.0)


def test_entry_points_reject_bad_arguments_on_the_host():
    """Every EINVAL is decided before anything is enqueued (the pointers are never dereferenced: this runs without a GPU)."""
    lib = _native.lib()
    update = lambda **kw: lib.dronesim_obsnorm_update(*{**UPDATE_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(state=None), dict(table=None), dict(ws=None), dict(R=0), dict(R=-2), dict(C=0), dict(C=-1),
                dict(eps=-1e-8), dict(eps=float("nan")), dict(wsb=8), dict(wsb=0), dict(ws=4100)):
        assert update(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_obsnorm_update"), bad
    apply = lambda **kw: lib.dronesim_obsnorm_apply(*{**APPLY_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(y=None), dict(table=None), dict(R=0), dict(R=-2), dict(C=0), dict(C=-1)):
        assert apply(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_obsnorm_apply"), bad


def test_state_dict_round_trip_on_cpu_tensors():
    import scalable_collision_avoidance_rl_amd as pkg
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    assert pkg.ObsNormalizer is ObsNormalizer and "ObsNormalizer" in pkg.__all__
    a = ObsNormalizer(5, 6, "cpu", clip=4.0, eps=1e-6)
    assert torch.equal(a.table[0], torch.zeros(5, 6, dtype=torch.float64)) and torch.equal(a.table[1], torch.ones(5, 6, dtype=torch.float64))
    assert float(a.count.sum()) == 0 and float(a.var.sum()) == 0 and tuple(a.mean.shape) == (5, 6)
    ref = OR.moments(torch.cat(OR.windows(5, 6)))
    ref[:, 7] = 0                                                             # one column that has seen nothing
    a.state.copy_(ref.view(3, 5, 6))
    sd = a.state_dict()
    assert sd["state"].dtype == torch.float64 and sd["state"].device.type == "cpu" and sd["state"].data_ptr() != a.state.data_ptr()
    assert (sd["clip"], sd["eps"], sd["n_agents"], sd["d_in"]) == (4.0, 1e-6, 5, 6)
    b = ObsNormalizer(5, 6, "cpu")
    b.load_state_dict(sd)
    assert torch.equal(b.state, a.state) and (b.clip, b.eps) == (4.0, 1e-6)
    assert torch.equal(b.table.view(2, 30), OR.table(ref, 1e-6))                # rebuilt from the state
    assert float(b.table[0].view(-1)[7]) == 0.0 and float(b.table[1].view(-1)[7]) == 1.0
    assert torch.allclose(b.var.view(-1)[:4], (ref[2] / ref[0])[:4], rtol=1e-15)
    none = ObsNormalizer(5, 6, "cpu", clip=None)
    assert ObsNormalizer(5, 6, "cpu").load_state_dict(none.state_dict()).clip is None
    for other in (ObsNormalizer(6, 5, "cpu"), ObsNormalizer(5, 15, "cpu")):
        with pytest.raises(ValueError, match="agents"):
            other.load_state_dict(sd)
    b.reset()
    assert float(b.state.abs().sum()) == 0 and torch.equal(b.table, ObsNormalizer(5, 6, "cpu").table)


def test_normaliser_checks_its_arguments():
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    for bad in (0.0, -1.0, float("nan"), float("inf"), "10", True):
        with pytest.raises(ValueError, match="clip"):
            ObsNormalizer(5, 6, "cpu", clip=bad)
    for bad in (-1e-8, float("nan"), "1e-8"):
        with pytest.raises(ValueError, match="eps"):
            ObsNormalizer(5, 6, "cpu", eps=bad)
    with pytest.raises(ValueError):
        ObsNormalizer(0, 6, "cpu")
    n = ObsNormalizer(5, 6, "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # host tensors: there is no other backend
        n.update(torch.zeros(4, 5, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        n.norm(torch.zeros(4, 5, 6))
    for bad in (torch.zeros(4, 5, 6, dtype=torch.float64), torch.zeros(4, 6, 5).transpose(1, 2), torch.zeros(0, 5, 6)):
        with pytest.raises(ValueError, match="contiguous float32"):
            n.update(bad)


def test_learners_and_evaluator_check_the_normaliser():
    from scalable_collision_avoidance_rl_amd.evaluate import Evaluator
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    actor, critic = PH.host_mlp(1, 16), PH.host_mlp(0, 1)                      # 3 agents x 6 inputs
    good = ObsNormalizer(3, 6, "cpu")
    for cls in (PPOLearner, SA2CLearner):
        plain = cls(actor, critic, 0.99)
        assert plain.obs_norm is None and plain.update_obs_norm is True
        on = cls(actor, critic, 0.99, obs_norm=good, update_obs_norm=False)
        assert on.obs_norm is good and on.update_obs_norm is False
        for bad in (ObsNormalizer(5, 6, "cpu"), ObsNormalizer(3, 15, "cpu")):
            with pytest.raises(ValueError, match="normaliser"):
                cls(actor, critic, 0.99, obs_norm=bad)
    env = type("Env", (), dict(batched=True, n_agents=3, local_state_space=6))()
    with pytest.raises(ValueError, match="obs_norm"):
        Evaluator(env, "proportional", obs_norm=good)
    sampler = PH.host_mlp(1, 16)
    sampler.sample_kind = 1
    assert Evaluator(env, sampler, obs_norm=good).obs_norm is good and Evaluator(env, sampler).obs_norm is None
    with pytest.raises(ValueError, match="normaliser"):
        Evaluator(env, sampler, obs_norm=ObsNormalizer(5, 6, "cpu"))
