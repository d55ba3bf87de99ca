"""Host-side tests of the entropy bonus and the per-agent advantage standardisation: the float64 restatement
(tests/entropy_ref.py) against torch autograd and torch's own mean / std, the inputs of the GPU tests (the column a float32
accumulator fails; the rows near a zero advantage), the new entry points' declarations and argument validation, and the
learners' host logic (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from tests import entropy_ref as ER
from tests import learner_ref as R
from tests import ppo_ref as P
from tests import test_gpu_learner as TG
from tests import test_learner_host as TH
from tests import test_ppo_host as PH

NAMES = R.NAMES
NEW_SYMBOLS = ("dronesim_standardize_workspace", "dronesim_standardize", "dronesim_mlp_grad_ent_workspace", "dronesim_mlp_grad_ent",
               "dronesim_mlp_grad_ppo_ent_workspace", "dronesim_mlp_grad_ppo_ent")


@pytest.mark.parametrize("kind", [1, 2])
def test_closed_form_entropy_gradient_equals_autograd(kind):
    """dH/dO as the heads add it (entropy_ref.entropy_dO) against autograd through the entropy's definition, to 1e-12; the
    softmax rows include one with a logit 120 above the rest (p = 0 for the others in float32, tiny in float64)."""
    gen = torch.Generator().manual_seed(7 + kind)
    nout = 16 if kind == 1 else 4
    O = (torch.randn(3, 50, nout, generator=gen, dtype=torch.float64) * 2).requires_grad_(True)
    H = ER.row_entropy(kind, O)
    g, = torch.autograd.grad(H.sum(), O)
    closed = ER.entropy_dO(kind, O.detach())
    assert torch.all((g - closed).abs() <= 1e-12 * (1 + closed.abs())), float((g - closed).abs().max())
    if kind == 1:
        p = torch.softmax(O.detach(), -1)
        assert torch.allclose(H.detach(), -(p * torch.log(p)).sum(-1), rtol=1e-12, atol=0)
        assert float(H.detach().max()) <= np.log(nout) + 1e-12 and float(H.detach().min()) >= 0
        sat = torch.zeros(1, 1, nout, dtype=torch.float64)
        sat[..., 3] = 120.0
        assert 0 <= float(ER.row_entropy(1, sat)) < 1e-6 and torch.isfinite(ER.entropy_dO(1, sat)).all()
    else:
        var = torch.sigmoid(O.detach()[..., 2:])
        ref = torch.distributions.Normal(torch.zeros_like(var), var.sqrt()).entropy().sum(-1)       # (scale = sqrt(variance))
        assert torch.allclose(H.detach(), ref, rtol=1e-12, atol=1e-12)
        assert torch.all(closed[..., :2] == 0)


@pytest.mark.parametrize("kind", [1, 2])
def test_restated_gradients_with_the_entropy_term_equal_autograd_on_the_whole_objective(kind):
    """entropy_ref.actor_grads / a2c_grads (the siblings' gradients plus the entropy's) against autograd on the objective
    written out in one piece."""
    N, rows, d_in, nout, eps, es = 3, 60, 6, (16 if kind == 1 else 4), 0.2, 0.01 / 60
    gen = torch.Generator().manual_seed(50 + kind)
    W = TG.random_net(torch, gen, N, d_in, 24, 20, nout)
    if kind == 2:
        W[4] = W[4] * R.structural_mask(2, W)
    x, _, act, adv = TG.random_rows(torch, gen, rows, 1, N, d_in, nout, kind)
    x, act, adv = x.reshape(rows, N, d_in), act.reshape(rows, N, 2), adv.reshape(rows, N).double()
    old = P.draw_logp_old(P.logp(kind, W, x, act), adv, eps, gen)[0].double()
    got = ER.actor_grads(kind, W, x, act, old, adv, eps, es)
    Wd = [w.double().clone().requires_grad_(True) for w in W]
    r = torch.exp(P.logp(kind, Wd, x, act) - old)
    H = ER.row_entropy(kind, R.forward(Wd, x.double())[2]).transpose(0, 1)
    loss = -torch.minimum(r * adv, torch.clamp(r, 1 - eps, 1 + eps) * adv).mean(0) - es * H.sum(0)
    g = list(torch.autograd.grad(loss.sum(), Wd))
    g[4] = g[4] * R.structural_mask(kind, Wd)
    assert torch.allclose(got["loss"], loss.detach(), rtol=1e-12, atol=0)
    assert torch.allclose(got["entropy"], H.detach().mean(0), rtol=1e-12, atol=0)
    for name, a, b, m in zip(NAMES, got["grad"], g, got["mag"]):
        assert torch.all((a - b).abs() <= 1e-12 * m + 1e-300), name
    a2c = ER.a2c_grads(kind, W, x, 0.5, act, adv, es)
    Wd = [w.double().clone().requires_grad_(True) for w in W]
    H = ER.row_entropy(kind, R.forward(Wd, x.double())[2]).transpose(0, 1)
    loss = -0.5 * (adv * P.logp(kind, Wd, x, act)).sum(0) - es * H.sum(0)
    g = list(torch.autograd.grad(loss.sum(), Wd))
    g[4] = g[4] * R.structural_mask(kind, Wd)
    assert torch.allclose(a2c["loss"], loss.detach(), rtol=1e-12, atol=0)
    for name, a, b, m in zip(NAMES, a2c["grad"], g, a2c["mag"]):
        assert torch.all((a - b).abs() <= 1e-12 * m + 1e-300), name
    # ent_scale = 0 is the sibling's restatement
    zero = ER.actor_grads(kind, W, x, act, old, adv, eps, 0.0)
    plain = P.actor_grads(kind, W, x, act, old, adv, eps)
    assert all(torch.equal(a, b) for a, b in zip(zero["grad"], plain["grad"])) and torch.equal(zero["loss"], plain["loss"])


@pytest.mark.parametrize("shape", ER.STANDARDIZE_SHAPES, ids=[f"R{r}N{n}" for r, n in ER.STANDARDIZE_SHAPES])
def test_standardize_restatement_equals_torch_mean_and_std(shape):
    x = ER.standardize_case(*shape).double()
    y, mean, std = ER.standardize(x, 1e-8)
    assert torch.allclose(y, (x - x.mean(0)) / (x.std(0, unbiased=False) + 1e-8), rtol=1e-12, atol=1e-12)
    assert torch.allclose(mean, x.mean(0), rtol=1e-14, atol=0) and torch.allclose(std, x.std(0, unbiased=False), rtol=1e-12, atol=1e-14)
    assert torch.all(y[:, ER.CONSTANT_COLUMN] == 0) and float(std[ER.CONSTANT_COLUMN]) == 0.0
    if shape[0] == 1:
        assert torch.all(y == 0)
    # a window's leading axes are flattened
    y3, _, _ = ER.standardize(x.reshape(1, *shape), 1e-8)
    assert torch.equal(y3.reshape(shape), y)


@pytest.mark.parametrize("shape", [(600, 5), (8193, 64), (4099, 3)])
def test_the_hard_column_fails_a_float32_accumulator(shape):
    """The GPU test's -500 +- 0.5 column does its job: float32 running sums of x and x^2 (the plausible wrong kernel) miss the
    bar |a - b| <= 1e-5 + 1e-5 |ref| on it, so a kernel that passes accumulates wider."""
    x = ER.standardize_case(*shape)
    assert abs(float(x[:, ER.HARD_COLUMN].double().mean()) + 500) < 0.1
    assert abs(float(x[:, ER.HARD_COLUMN].double().std()) - 0.5) < 0.05
    ref, _, _ = ER.standardize(x)
    wrong = ER.standardize_float32(x).double()
    miss = (wrong - ref).abs() > 1e-5 + 1e-5 * ref.abs()
    assert miss[:, ER.HARD_COLUMN].float().mean() > 0.5, float(miss[:, ER.HARD_COLUMN].float().mean())


def synthetic_window(seed=3, T=12, E=32, N=16, d_in=6):
    """A window of the GPU learner test's shape with seeded data (the GPU test's own window comes from a rollout)."""
    gen = torch.Generator().manual_seed(seed)
    Wa, Wc = TG.random_net(torch, gen, N, d_in, 48, 48, 16), TG.random_net(torch, gen, N, d_in, 32, 32, 1)
    x, _, act, _ = TG.random_rows(torch, gen, T, E, N, d_in, 16, 1)
    reward = -torch.rand(T, E, N, generator=gen) * 3
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[6] = 1
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                       torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
    return Wa, Wc, x, reward, done, act, nbr


def test_ppo_restatement_with_both_options():
    """entropy_ref.ppo_train: the standardised advantage has mean 0 and std 1 per agent, the defaults reproduce
    ppo_ref.ppo_train, epoch 1 has ratio 1, and the rows within ZERO_MARGIN of a zero advantage -- which may fall on either
    side of the clip test in float32 -- stay within the GPU test's cap of 1 % of the window."""
    Wa, Wc, *data = synthetic_window()
    plain = P.ppo_train(1, Wa, Wc, *data, 0.99, epochs=2)
    same = ER.ppo_train(1, Wa, Wc, *data, 0.99, epochs=2)
    assert torch.equal(plain["adv"], same["adv"]) and not same["near_zero"].any()
    for k in ("actor_loss", "actor_norm", "critic_loss"):
        assert all(torch.equal(a, b) for a, b in zip(plain[k], same[k])), k
    out = ER.ppo_train(1, Wa, Wc, *data, 0.99, epochs=2, ent_coef=0.01, normalize_advantage=True)
    adv = out["adv"].reshape(-1, out["adv"].shape[-1])
    assert torch.allclose(adv.mean(0), torch.zeros(adv.shape[1], dtype=torch.float64), atol=1e-12)
    assert torch.allclose(adv.std(0, unbiased=False), torch.ones(adv.shape[1], dtype=torch.float64), atol=1e-6)
    assert torch.allclose(out["adv_mean"], plain["adv"].reshape(adv.shape).mean(0), rtol=1e-12)
    assert float(out["near_zero"].double().mean()) <= 0.01
    a0 = out["actor"][0]
    assert float(a0["r"].min()) == float(a0["r"].max()) == 1.0 and not a0["clipped"].any()
    assert torch.allclose(out["actor_loss"][0], a0["surrogate_loss"] - 0.01 * out["entropy"][0], rtol=1e-12, atol=1e-15)
    assert float(out["entropy"][0].min()) > 0 and float(out["entropy"][0].max()) <= np.log(16) + 1e-12


def test_sa2c_restatement_with_the_entropy_term():
    Wa, Wc, *data = synthetic_window(seed=4, T=9, E=4, N=5)
    plain = R.sa2c_train(1, Wa, Wc, *data, 0.99)
    zero = ER.sa2c_train(1, Wa, Wc, *data, 0.99, ent_coef=0.0)
    for a, b in zip(plain["actor_post"], zero["actor_post"]):
        assert torch.equal(a, b)
    out = ER.sa2c_train(1, Wa, Wc, *data, 0.99, ent_coef=0.01)
    assert torch.allclose(out["actor_loss"], plain["actor_loss"] - 0.01 * out["entropy"], rtol=1e-12, atol=1e-15)
    assert any(not torch.equal(a, b) for a, b in zip(plain["actor_post"], out["actor_post"]))
    for a, b in zip(plain["critic_post"], out["critic_post"]):
        assert torch.equal(a, b)


def test_library_exports_the_new_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    want = ("dronesim_standardize_workspace", "dronesim_standardize", "dronesim_mlp_grad_ent_workspace", "dronesim_mlp_grad_ent", "dronesim_mlp_grad_ppo_ent_workspace", "dronesim_mlp_grad_ppo_ent")
    assert set(want) == set(NEW_SYMBOLS)
    header = open(_native.HEADER_PATH).read()
    for name in want:
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert f"int {name}(" in header, name


def test_workspace_queries():
    lib = _native.lib()
    n, g, p = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    m = PH.actor_struct(h1=300, h2=300)
    assert lib.dronesim_mlp_grad_workspace(C.byref(m), 128, C.byref(g)) == _native.OK
    assert lib.dronesim_mlp_grad_ppo_workspace(C.byref(m), 128, C.byref(p)) == _native.OK
    assert lib.dronesim_mlp_grad_ent_workspace(C.byref(m), 128, C.byref(n)) == _native.OK
    assert n.value == g.value + 4 * 5 * 128
    assert lib.dronesim_mlp_grad_ppo_ent_workspace(C.byref(m), 128, C.byref(n)) == _native.OK
    assert n.value == p.value + 4 * 5 * 128
    for fn in (lib.dronesim_mlp_grad_ent_workspace, lib.dronesim_mlp_grad_ppo_ent_workspace):
        for rows in (0, 100, -64):
            assert fn(C.byref(m), rows, C.byref(n)) == _native.EINVAL
        assert fn(C.byref(m), 64, None) == _native.EINVAL
        assert fn(C.byref(TH.fake_struct()), 64, C.byref(n)) == _native.EINVAL                      # a critic
    # the slab rule depends on (R, N) only: the same query twice, a multiple of 16 N bytes, and enough for one slab
    for R_, N_ in ER.STANDARDIZE_SHAPES + [(819200, 64), (102400, 256)]:
        a, b = C.c_size_t(0), C.c_size_t(0)
        assert lib.dronesim_standardize_workspace(R_, N_, C.byref(a)) == lib.dronesim_standardize_workspace(R_, N_, C.byref(b)) == _native.OK
        assert a.value == b.value and a.value >= 16 * N_ and a.value % (16 * N_) == 0
    for bad in ((0, 5), (-1, 5), (5, 0)):
        assert lib.dronesim_standardize_workspace(*bad, C.byref(n)) == _native.EINVAL
    assert lib.dronesim_standardize_workspace(5, 5, None) == _native.EINVAL


STD_OK = dict(x=4096, y=8192, stats=None, R=64, N=5, eps=1e-8, ws=4096, wsb=1 << 20)
ENT_OK = dict(x=4096, R=64, scale=1.0, act=4096, weight=4096, es=0.01, grad=4096, loss=4096, entropy=4096, rc=64, ws=4096, wsb=1 << 30)
PPO_ENT_OK = dict(x=4096, R=64, scale=1.0, act=4096, logp_old=4096, adv=4096, eps=0.2, es=0.01, grad=4096, loss=4096, stats=4096,
                  rc=64, ws=4096, wsb=1 << 30)


def test_new_entry_points_reject_null_buffers_and_bad_sizes():
    """Every EINVAL case is decided on the host, before anything is enqueued (the pointers are never dereferenced)."""
    lib = _native.lib()
    std = lambda **kw: lib.dronesim_standardize(*{**STD_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(y=None), dict(ws=None), dict(R=0), dict(R=-2), dict(N=0), dict(eps=-1e-8), dict(eps=float("nan")),
                dict(wsb=8), dict(ws=4100)):
        assert std(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_standardize"), bad
    m = C.byref(PH.actor_struct())
    plain = 4 * 5 * 64 * (200 + 200 + 16 + 1)
    ent = lambda **kw: lib.dronesim_mlp_grad_ent(m, *{**ENT_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(act=None), dict(weight=None), dict(grad=None), dict(loss=None), dict(entropy=None), dict(ws=None),
                dict(R=0), dict(rc=96), dict(wsb=plain), dict(es=-0.1), dict(es=float("nan")), dict(es=float("inf"))):
        assert ent(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_mlp_grad_ent"), bad
    ppo = lambda **kw: lib.dronesim_mlp_grad_ppo_ent(m, *{**PPO_ENT_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(act=None), dict(logp_old=None), dict(adv=None), dict(grad=None), dict(loss=None), dict(stats=None),
                dict(ws=None), dict(R=0), dict(rc=-64), dict(wsb=plain + 4 * 5 * 64 * 3), dict(eps=0.0), dict(eps=1.0),
                dict(es=-0.1), dict(es=float("nan"))):
        assert ppo(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_mlp_grad_ppo_ent"), bad
    mc = C.byref(TH.fake_struct())                                                                   # a critic
    assert lib.dronesim_mlp_grad_ent(mc, *ENT_OK.values(), None) == _native.EINVAL and b"actor" in lib.dronesim_last_error()
    assert lib.dronesim_mlp_grad_ppo_ent(mc, *PPO_ENT_OK.values(), None) == _native.EINVAL and b"actor" in lib.dronesim_last_error()


def test_learners_check_the_new_arguments():
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    actor, critic = PH.host_mlp(1, 16), PH.host_mlp(0, 1)
    ppo = PPOLearner(actor, critic, 0.99)
    assert (ppo.ent_coef, ppo.normalize_advantage, ppo.adv_eps) == (0.0, False, 1e-8)
    sa = SA2CLearner(actor, critic, 0.99)
    assert sa.ent_coef == 0.0 and "standardis" in SA2CLearner.__doc__
    on = PPOLearner(actor, critic, 0.99, ent_coef=0.01, normalize_advantage=True, adv_eps=1e-6)
    assert (on.ent_coef, on.normalize_advantage, on.adv_eps) == (0.01, True, 1e-6)
    assert SA2CLearner(actor, critic, 0.99, ent_coef=0.02).ent_coef == 0.02
    for cls in (PPOLearner, SA2CLearner):
        for bad in (-0.01, float("nan"), float("inf"), -float("inf"), "0.01", None, True):
            with pytest.raises(ValueError, match="ent_coef"):
                cls(actor, critic, 0.99, ent_coef=bad)
    for bad in (-1e-8, float("nan")):
        with pytest.raises(ValueError, match="adv_eps"):
            PPOLearner(actor, critic, 0.99, adv_eps=bad)
    with pytest.raises(TypeError):
        SA2CLearner(actor, critic, 0.99, normalize_advantage=True)


def test_standardize_wrapper_refuses_host_tensors():
    from scalable_collision_avoidance_rl_amd.rollout_buffer import standardize
    with pytest.raises(RuntimeError, match="device"):
        standardize(torch.zeros(4, 5))
