"""Host-side tests of the PPO learner's two guards (per-agent KL early stop, clipped value loss): the new entry points'
declarations and argument validation, `PPOLearner`'s argument checks, and the float64 restatement (tests/ppo_guard_ref.py)
against torch autograd, the KL definition and a hand-written gate table (no GPU needed)."""
import ctypes as C
import math

import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from tests import learner_ref as R
from tests import ppo_guard_ref as GR
from tests import ppo_ref as P
from tests import test_entropy_host as EH
from tests import test_gpu_learner as TG
from tests import test_learner_host as TH
from tests import test_ppo_host as PH

NAMES = R.NAMES
NEW_SYMBOLS = ("dronesim_mlp_grad_ppo_gated_workspace", "dronesim_mlp_grad_ppo_gated", "dronesim_kl_gate", "dronesim_adam_step_gated",
               "dronesim_mlp_grad_vclip_workspace", "dronesim_mlp_grad_vclip")
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_new_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    want = ("dronesim_mlp_grad_ppo_gated_workspace", "dronesim_mlp_grad_ppo_gated", "dronesim_kl_gate", "dronesim_adam_step_gated", "dronesim_mlp_grad_vclip_workspace", "dronesim_mlp_grad_vclip")
    assert set(want) == set(NEW_SYMBOLS)
    header = open(_native.HEADER_PATH).read()
    for name in want:
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
        assert f"int {name}(" in header, name
    assert lib.dronesim_version() == 600


def test_workspace_queries():
    lib = _native.lib()
    n, g, p = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    m = PH.actor_struct(h1=300, h2=300)
    assert lib.dronesim_mlp_grad_ppo_ent_workspace(C.byref(m), 128, C.byref(p)) == _native.OK
    assert lib.dronesim_mlp_grad_ppo_gated_workspace(C.byref(m), 128, C.byref(n)) == _native.OK
    assert n.value == p.value + 4 * 5 * 128 + 8 * 5                     # the k plane and the float64 running sums
    mc = TH.fake_struct()
    assert lib.dronesim_mlp_grad_workspace(C.byref(mc), 128, C.byref(g)) == _native.OK
    assert lib.dronesim_mlp_grad_vclip_workspace(C.byref(mc), 128, C.byref(n)) == _native.OK
    assert n.value == g.value + 4 * mc.N * 128
    for fn, ok, wrong in ((lib.dronesim_mlp_grad_ppo_gated_workspace, m, mc), (lib.dronesim_mlp_grad_vclip_workspace, mc, m)):
        for rows in (0, 100, -64):
            assert fn(C.byref(ok), rows, C.byref(n)) == _native.EINVAL
        assert fn(C.byref(ok), 64, None) == _native.EINVAL
        assert fn(C.byref(wrong), 64, C.byref(n)) == _native.EINVAL     # a critic to the gated call, an actor to vclip


GATED_OK = dict(x=4096, R=64, scale=1.0, act=4096, logp_old=4096, adv=4096, eps=0.2, es=0.01, active=4096, grad=4096, loss=4096,
                stats=4096, rc=64, ws=4096, wsb=1 << 30)
GATE_OK = dict(kl=4096, tau=0.02, active=4096, taken=4096, N=5, reset=0)
ADAM_OK = dict(grad=4096, m1=4096, m2=4096, step=4096, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, max_norm=10.0, norm=4096, active=4096)
VCLIP_OK = dict(x=4096, R=64, scale=1.0, target=4096, v_old=4096, vf=0.2, grad=4096, loss=4096, clip=4096, rc=64, ws=4096, wsb=1 << 30)


def test_new_entry_points_reject_bad_arguments_without_a_device():
    """Every EINVAL case is decided on the host, before anything is enqueued (the pointers are never dereferenced)."""
    lib = _native.lib()
    m, mc = C.byref(PH.actor_struct()), C.byref(TH.fake_struct())
    ent = 4 * 5 * 64 * (200 + 200 + 16 + 1 + 3 + 1)                      # dronesim_mlp_grad_ppo_ent's workspace at this shape
    gated = lambda **kw: lib.dronesim_mlp_grad_ppo_gated(m, *{**GATED_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(act=None), dict(logp_old=None), dict(adv=None), dict(grad=None), dict(loss=None), dict(stats=None),
                dict(ws=None), dict(R=0), dict(rc=-64), dict(rc=96), dict(wsb=ent), dict(wsb=ent + 4 * 5 * 64), dict(ws=4100),
                dict(eps=0.0), dict(eps=1.0), dict(es=-0.1), dict(es=NAN), dict(es=INF)):
        assert gated(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_mlp_grad_ppo_gated"), bad
    assert lib.dronesim_mlp_grad_ppo_gated(mc, *GATED_OK.values(), None) == _native.EINVAL and b"actor" in lib.dronesim_last_error()

    gate = lambda **kw: lib.dronesim_kl_gate(*{**GATE_OK, **kw}.values(), None)
    for bad in (dict(kl=None), dict(active=None), dict(taken=None), dict(N=0), dict(N=-3), dict(tau=0.0), dict(tau=-0.01), dict(tau=NAN),
                dict(tau=INF), dict(reset=1, tau=0.0), dict(reset=1, tau=NAN), dict(reset=1, active=None), dict(reset=1, taken=None)):
        assert gate(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_kl_gate"), bad

    adam = lambda **kw: lib.dronesim_adam_step_gated(m, *{**ADAM_OK, **kw}.values(), None)
    for bad in (dict(grad=None), dict(m1=None), dict(m2=None), dict(step=None), dict(norm=None), dict(active=None), dict(lr=-1.0),
                dict(b1=1.0), dict(b2=-0.1), dict(eps=0.0), dict(max_norm=0.0), dict(lr=NAN)):
        assert adam(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_adam_step_gated"), bad
    assert lib.dronesim_adam_step_gated(None, *ADAM_OK.values(), None) == _native.EINVAL

    fake = TH.fake_struct()
    plain = 4 * fake.N * 64 * (fake.h1 + fake.h2 + fake.nout + 1)
    vclip = lambda **kw: lib.dronesim_mlp_grad_vclip(mc, *{**VCLIP_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(target=None), dict(v_old=None), dict(grad=None), dict(loss=None), dict(clip=None), dict(ws=None),
                dict(R=0), dict(rc=0), dict(rc=100), dict(wsb=plain), dict(vf=0.0), dict(vf=-0.2), dict(vf=NAN), dict(vf=-INF)):
        assert vclip(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_mlp_grad_vclip"), bad
    assert lib.dronesim_mlp_grad_vclip(m, *VCLIP_OK.values(), None) == _native.EINVAL and b"critic" in lib.dronesim_last_error()


def test_ppo_learner_checks_the_new_arguments():
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    actor, critic = PH.host_mlp(1, 16), PH.host_mlp(0, 1)
    off = PPOLearner(actor, critic, 0.99)
    assert off.target_kl is None and off.vf_clip is None and off._ent is False and off._stat_rows == 4
    on = PPOLearner(actor, critic, 0.99, target_kl=0.02, vf_clip=0.2, minibatches=4)
    assert (on.target_kl, on.vf_clip) == (0.02, 0.2) and on._ent is True and on._stat_rows == 6
    assert PPOLearner(actor, critic, 0.99, vf_clip=1)._stat_rows == 4 and PPOLearner(actor, critic, 0.99, ent_coef=0.01)._stat_rows == 5
    for name in ("target_kl", "vf_clip"):
        for bad in (0, 0.0, -0.02, NAN, INF, -INF, "0.02", True, False):
            with pytest.raises(ValueError, match=name):
                PPOLearner(actor, critic, 0.99, **{name: bad})
        with pytest.raises(TypeError):
            SA2CLearner(actor, critic, 0.99, **{name: 0.02})
    doc = PPOLearner.__doc__
    assert "target_kl" in doc and "vf_clip" in doc and "NaN" in doc and "actor_steps" in doc


# the restatement checks itself ----------------------------------------------------------------------------------------
def critic_rows(seed=11, N=3, rows=80, d_in=6):
    gen = torch.Generator().manual_seed(seed)
    W = TG.random_net(torch, gen, N, d_in, 24, 20, 1)
    x, target, _, _ = TG.random_rows(torch, gen, rows, 1, N, d_in, 1, 0)
    return W, x.reshape(rows, N, d_in), target.reshape(rows, N).double() * 0.1, gen


def test_restated_vclip_gradient_equals_autograd_of_torch_maximum():
    W, x, G, gen = critic_rows()
    eps = 0.2
    Wd = [w.double().clone().requires_grad_(True) for w in W]
    V = R.forward(Wd, x.double())[2][..., 0].transpose(0, 1)
    v_old = (V.detach() - (torch.rand(V.shape, generator=gen, dtype=torch.float64) * 2 - 1) * 2 * eps)
    got = GR.vclip_grads(W, x, 1.0 / x.shape[0], G, v_old, eps)
    assert not got["near"].any()
    Vc = v_old + torch.clamp(V - v_old, -eps, eps)
    loss = torch.maximum((V - G) ** 2, (Vc - G) ** 2).mean(0)
    g = torch.autograd.grad(loss.sum(), Wd)
    assert torch.allclose(got["loss"], loss.detach(), rtol=1e-13, atol=0)
    for name, a, b, mg in zip(NAMES, got["grad"], g, got["mag"]):
        assert torch.all((a - b).abs() <= 1e-12 * mg + 1e-300), name
    # both branches are exercised; a zero-gradient row is a clamped row; the share is the mean of the flags
    share = got["zero"].double().mean()
    assert 0.1 < float(share) < 0.45 and 0.3 < float(got["clamped"].double().mean()) < 0.7
    assert not (got["zero"] & ~got["clamped"]).any()
    assert torch.equal(got["clip_fraction"], got["zero"].double().mean(0))
    # vf_clip = inf, and a v_old within eps / 2 everywhere: the plain squared error
    plain_g, plain_l = R.grads(0, W, x, 1.0 / x.shape[0], target=G)
    for v, e in ((v_old, INF), (V.detach() + 0.5 * eps * (torch.rand(V.shape, generator=gen, dtype=torch.float64) * 2 - 1), eps)):
        same = GR.vclip_grads(W, x, 1.0 / x.shape[0], G, v, e)
        assert not same["zero"].any() and torch.allclose(same["loss"], plain_l, rtol=1e-14, atol=0)
        assert all(torch.allclose(a, b, rtol=1e-12, atol=1e-300) for a, b in zip(same["grad"], plain_g))


def test_restated_kl_is_schulmans_estimator():
    gen = torch.Generator().manual_seed(5)
    lp = torch.randn(500, 4, generator=gen, dtype=torch.float64) - 2
    old = lp - (torch.rand(500, 4, generator=gen, dtype=torch.float64) * 2 - 1) * math.log(2.0)
    r = torch.exp(lp - old)
    kl = GR.kl_estimate(lp, old)
    assert torch.allclose(kl, (r - 1 - torch.log(r)).mean(0), rtol=1e-12, atol=0)
    assert float(GR.kl_rows(lp, old).min()) >= 0 and float(kl.min()) > 0
    assert torch.equal(GR.kl_estimate(lp, lp), torch.zeros(4, dtype=torch.float64))
    # (r - 1) - log r in float32 cancels where expm1 does not: a shift of 1e-4 has k = 5e-9, below float32's rounding of r - 1
    small = torch.full((1, 1), 1e-4, dtype=torch.float64)
    k = float(GR.kl_rows(small, torch.zeros(1, 1)))
    assert abs(k - 5e-9) < 1e-12


def test_gate_rule_on_a_hand_written_table():
    tau = 0.02
    active, taken = GR.gate([0, 0, 1, 0, 1, 0, 1], [3, 1, 4, 1, 5, 9, 2], None, tau, reset=True)
    assert active == [1] * 7 and taken == [0] * 7
    #            below  equal  above  NaN   zero  inf   just above
    kl1 = [0.01, tau, 0.03, NAN, 0.0, INF, math.nextafter(tau, 1.0)]
    active, taken = GR.gate(active, taken, kl1, tau)
    assert active == [1, 1, 0, 0, 1, 0, 0] and taken == [1, 1, 0, 0, 1, 0, 0]
    # a stop is sticky whatever the next estimate says (a skipped step reports NaN); the others count on
    kl2 = [0.019, 0.021, 0.0, NAN, tau, 0.0, 0.0]
    active, taken = GR.gate(active, taken, kl2, tau)
    assert active == [1, 0, 0, 0, 1, 0, 0] and taken == [2, 1, 0, 0, 2, 0, 0]
    active, taken = GR.gate(active, taken, None, tau, reset=True)
    assert active == [1] * 7 and taken == [0] * 7
    table = torch.tensor([[0.0, 0.0, 0.0], [0.01, 0.03, 0.001], [0.05, 0.001, 0.002], [0.0, 0.0, 0.003]], dtype=torch.float64)
    assert GR.stops_of(table, tau) == [2, 1, 4]


def test_restated_train_with_the_guards_off_is_the_existing_restatement_and_the_gate_freezes_agents():
    Wa, Wc, *data = EH.synthetic_window(seed=6, T=9, E=8, N=5)
    plain = P.ppo_train(1, Wa, Wc, *data, 0.99, epochs=3, lr_actor=3e-3)
    same = GR.ppo_train(1, Wa, Wc, *data, 0.99, epochs=3, lr_actor=3e-3)
    for a, b in zip(plain["actor_post"] + plain["critic_post"], same["actor_post"] + same["critic_post"]):
        assert torch.equal(a, b)
    assert same["actor_steps"].tolist() == [3] * 5 and float(same["kl"][0].abs().max()) == 0.0 and float(same["kl"][1].min()) > 0
    table = torch.stack(same["kl"])
    tau = math.sqrt(float(table[1].min()) * float(table[1].sort().values[1]))      # between the two smallest second-step values
    gated = GR.ppo_train(1, Wa, Wc, *data, 0.99, epochs=3, lr_actor=3e-3, target_kl=tau)
    assert gated["actor_steps"].tolist() == GR.stops_of(table, tau)
    for i, s in enumerate(gated["actor_steps"].tolist()):
        ref = P.ppo_train(1, Wa, Wc, *data, 0.99, epochs=s, lr_actor=3e-3)["actor_post"] if s else [w.double() for w in Wa]
        assert all(torch.equal(a[i], b[i]) for a, b in zip(gated["actor_post"], ref)), i
    for a, b in zip(plain["critic_post"], gated["critic_post"]):                    # the critic is never gated
        assert torch.equal(a, b)
    # vf_clip = inf is the plain critic; a finite one clips nothing in the first step (V == v_old) and something later
    inf = GR.ppo_train(1, Wa, Wc, *data, 0.99, epochs=3, lr_critic=3e-2, vf_clip=INF)
    ref = P.ppo_train(1, Wa, Wc, *data, 0.99, epochs=3, lr_critic=3e-2)
    assert all(torch.allclose(a, b, rtol=1e-12, atol=1e-14) for a, b in zip(inf["critic_post"], ref["critic_post"]))
    fin = GR.ppo_train(1, Wa, Wc, *data, 0.99, epochs=3, lr_critic=3e-2, vf_clip=0.02)
    assert float(fin["critic"][0]["clip_fraction"].max()) == 0.0 and float(fin["critic"][2]["clip_fraction"].max()) > 0
