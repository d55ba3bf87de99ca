"""Host-side tests of the PPO learner (SAC_agents.py:410-573, `SPPOAgents.train`): the float64 restatement of the contract
(tests/ppo_ref.py) against what the reference's own `probability_of_ai` returned (tests/golden/ppo_n5.npz) and against torch
autograd on a literal transcription of the loss lines; the new entry points' argument validation and `PPOLearner`'s host
logic (no GPU needed)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from scalable_collision_avoidance_rl_amd import _native
from tests import helpers as H
from tests import learner_ref as R
from tests import ppo_ref as P
from tests import test_gpu_learner as TG
from tests import test_learner_host as TH

NAMES = R.NAMES
ACTOR_CASES = [c for c in TG.FUZZ if c[6] != 0]
PPO_SYMBOLS = ("dronesim_neighbour_advantage", "dronesim_mlp_grad_ppo_workspace", "dronesim_mlp_logp", "dronesim_mlp_grad_ppo")


def test_float64_restatement_reproduces_the_reference_probabilities_returns_and_neighbour_sum():
    """exp(logp_old), G and Q of tests/ppo_ref.py against the reference's `probability_of_ai` (float64 modules) and the
    generator's own loops of :476-481 and :498-501, at the 1e-11 relative bar of test_oracle_golden.py."""
    fx, ep = dict(H.load("ppo_n5.npz")), dict(H.load("episode_n5.npz"))
    actor, _ = R.reference_weights("gaussian", 5, 6, int(fx["seed_gauss"]))
    for name, w in zip(NAMES, actor):
        np.testing.assert_allclose(w.double().reshape(5, -1).sum(1).numpy(), fx[f"init_sum_{name}"], rtol=1e-12, atol=1e-9)
    T = ep["act"].shape[0]
    x = torch.cat([torch.as_tensor(ep["z0"])[None], torch.as_tensor(ep["z"])[:-1]]).reshape(T, 5, 6).double()
    act = torch.as_tensor(ep["act"]).reshape(T, 5, 2).double()
    p = torch.exp(P.logp(2, actor, x, act))
    np.testing.assert_allclose(p.numpy(), fx["p_old"], rtol=1e-11, atol=0)
    reward = torch.as_tensor(ep["reward"]).reshape(T, 1, 5).double()
    done = torch.as_tensor(ep["done"]).reshape(T, 1).to(torch.uint8)
    G = R.returns(reward, done, float(fx["gamma"]))
    np.testing.assert_allclose(G[:, 0].numpy(), fx["G"], rtol=1e-11, atol=0)
    nbr = torch.as_tensor(ep["nbr_idx_pre"]).reshape(T, 1, 5, -1)
    Q = P.neighbour_sum(G, nbr)
    np.testing.assert_allclose(Q[:, 0].numpy(), fx["Q"], rtol=1e-11, atol=0)
    # the two baselines differ by (|N_i| - 1) V
    V = torch.randn(T, 1, 5, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    cnt = (nbr >= 0).double().sum(-1)
    assert torch.allclose(P.advantage(G, V, nbr, "once") - P.advantage(G, V, nbr, "per_neighbour"), (cnt - 1) * V, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", [1, 2])
def test_restated_actor_gradient_equals_autograd_on_the_literal_loss_lines(kind):
    """One epoch's actor gradient of tests/ppo_ref.py (the constant-weight identity) against torch autograd applied to the
    three loss lines as the reference writes them (:545-549): r = pi / pi_old, left = r Adv, right = clamp(r) Adv,
    loss = -mean(min(left, right)).  Ratios spread over [0.5, 2], advantages of both signs."""
    N, rows, d_in, nout, eps = 3, 60, 6, (16 if kind == 1 else 4), 0.2
    gen = torch.Generator().manual_seed(40 + kind)
    W = TG.random_net(torch, gen, N, d_in, 24, 20, nout)
    if kind == 2:
        W[4] = W[4] * R.structural_mask(2, W)
    x, _, act, adv = TG.random_rows(torch, gen, rows, 1, N, d_in, nout, kind)
    x, act, adv = x.reshape(rows, N, d_in), act.reshape(rows, N, 2), adv.reshape(rows, N).double()
    old, _ = P.draw_logp_old(P.logp(kind, W, x, act), adv, eps, gen)
    old = old.double()
    got = P.actor_grads(kind, W, x, act, old, adv, eps)
    assert 0 < int(got["clipped"].sum()) < got["clipped"].numel()           # both branches are exercised
    Wd = [w.double().clone().requires_grad_(True) for w in W]
    r_theta = torch.exp(P.logp(kind, Wd, x, act)) / torch.exp(old)
    left_min = r_theta * adv
    right_min = torch.clamp(r_theta, 1 - eps, 1 + eps) * adv
    loss = -torch.mean(torch.min(left_min, right_min), dim=0)
    g = list(torch.autograd.grad(loss.sum(), Wd))
    g[4] = g[4] * R.structural_mask(kind, Wd)
    assert torch.allclose(got["loss"], loss.detach(), rtol=1e-12, atol=0)
    for name, a, b, m in zip(NAMES, got["grad"], g, got["mag"]):
        assert torch.all((a - b).abs() <= 1e-12 * m + 1e-300), (name, float(((a - b).abs() - 1e-12 * m).max()))


@pytest.mark.parametrize("case", ACTOR_CASES, ids=[f"N{c[0]}E{c[1]}T{c[2]}k{c[6]}" for c in ACTOR_CASES])
def test_head_cases_redraw_at_most_one_percent_of_rows(case):
    """The draw of the GPU head test (tests/test_gpu_ppo.py) keeps the rows near a clip edge, whose offsets are redrawn,
    within 1 % per case, spreads the ratio over roughly [0.5, 2] and has advantages of both signs on both branches."""
    c = P.head_case(case)
    assert c["redrawn"] <= 0.01, c["redrawn"]
    N, E, T = case[:3]
    rows = lambda t: t.reshape(T * E, N, *t.shape[3:])
    lp = P.logp(c["kind"], c["W"], rows(c["x"]), rows(c["act"]))
    r, clipped, near = P.ratio_terms(lp, rows(c["logp_old"]), rows(c["adv"]), 0.2)
    assert not near.any()
    assert 0.49 < float(r.min()) and float(r.max()) < 2.01
    if r.numel() >= 1000:
        assert float(r.min()) < 0.6 and float(r.max()) > 1.8 and 0.05 < float(clipped.double().mean()) < 0.6
        assert bool((rows(c["adv"]) > 0).any()) and bool((rows(c["adv"]) < 0).any())


def test_library_exports_the_ppo_entry_points_with_the_declared_argtypes():
    lib = _native.lib()
    want = ("dronesim_neighbour_advantage", "dronesim_mlp_grad_ppo_workspace", "dronesim_mlp_logp", "dronesim_mlp_grad_ppo")
    assert set(want) == set(PPO_SYMBOLS)
    for name in want:
        assert name in _native.SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int, name
    header = open(_native.HEADER_PATH).read()
    for name in PPO_SYMBOLS:
        assert f"int {name}(" in header, name
    assert lib.dronesim_version() == 600


def actor_struct(**kw):
    return TH.fake_struct(**{**dict(out_kind=1, nout=16), **kw})


def test_ppo_workspace_query():
    lib = _native.lib()
    n, g = C.c_size_t(0), C.c_size_t(0)
    m = actor_struct(h1=300, h2=300)
    assert lib.dronesim_mlp_grad_ppo_workspace(C.byref(m), 128, C.byref(n)) == _native.OK
    assert lib.dronesim_mlp_grad_workspace(C.byref(m), 128, C.byref(g)) == _native.OK
    assert n.value == g.value + 4 * 5 * 128 * 3 == 4 * 5 * 128 * (300 + 300 + 16 + 1 + 3)
    for rows in (0, 100, -64):
        assert lib.dronesim_mlp_grad_ppo_workspace(C.byref(m), rows, C.byref(n)) == _native.EINVAL
    assert lib.dronesim_mlp_grad_ppo_workspace(C.byref(m), 64, None) == _native.EINVAL
    assert lib.dronesim_mlp_grad_ppo_workspace(C.byref(TH.fake_struct()), 64, C.byref(n)) == _native.EINVAL     # a critic


LOGP_OK = dict(x=4096, R=64, act=4096, logp=4096, rc=64, ws=4096, wsb=1 << 30)
PPO_OK = dict(x=4096, R=64, scale=1.0, act=4096, logp_old=4096, adv=4096, eps=0.2, grad=4096, loss=4096, stats=4096, rc=64,
              ws=4096, wsb=1 << 30)


def test_ppo_entry_points_reject_null_buffers_and_bad_sizes():
    """Every EINVAL case is decided on the host, before anything is enqueued (the pointers are never dereferenced)."""
    lib = _native.lib()
    m = C.byref(actor_struct())
    logp = lambda **kw: lib.dronesim_mlp_logp(m, *{**LOGP_OK, **kw}.values(), None)
    for bad in (dict(x=None), dict(act=None), dict(logp=None), dict(ws=None), dict(R=0), dict(R=-3), dict(rc=96), dict(rc=0),
                dict(wsb=1000)):
        assert logp(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_mlp_logp"), bad
    ppo = lambda **kw: lib.dronesim_mlp_grad_ppo(m, *{**PPO_OK, **kw}.values(), None)
    short = 4 * 5 * 64 * (200 + 200 + 16 + 1)                  # the plain gradient workspace: three per-row floats short
    for bad in (dict(x=None), dict(act=None), dict(logp_old=None), dict(adv=None), dict(grad=None), dict(loss=None),
                dict(stats=None), dict(ws=None), dict(R=0), dict(rc=96), dict(rc=-64), dict(wsb=short), dict(eps=0.0),
                dict(eps=1.0), dict(eps=-0.2), dict(eps=1.5), dict(eps=float("nan"))):
        assert ppo(**bad) == _native.EINVAL, bad
        assert lib.dronesim_last_error().startswith(b"dronesim_mlp_grad_ppo"), bad
    # a critic passed to an actor entry
    mc = C.byref(TH.fake_struct())
    assert lib.dronesim_mlp_logp(mc, *LOGP_OK.values(), None) == _native.EINVAL
    assert b"actor" in lib.dronesim_last_error()
    assert lib.dronesim_mlp_grad_ppo(mc, *PPO_OK.values(), None) == _native.EINVAL
    assert b"actor" in lib.dronesim_last_error()
    adv = lambda *p, per=0, dims=(4, 2, 5, 3): lib.dronesim_neighbour_advantage(*p[:3], per, p[3], *dims, None)
    for bad in ((None, 4096, 4096, 4096), (4096, None, 4096, 4096), (4096, 4096, None, 4096), (4096, 4096, 4096, None)):
        assert adv(*bad) == _native.EINVAL, bad
    ok = (4096, 4096, 4096, 4096)
    assert adv(*ok, per=2) == _native.EINVAL and adv(*ok, per=-1) == _native.EINVAL
    for dims in ((-1, 2, 5, 3), (4, -1, 5, 3), (4, 2, 0, 3), (4, 2, 5, 0)):
        assert adv(*ok, dims=dims) == _native.EINVAL, dims
    assert adv(*ok, dims=(0, 2, 5, 3)) == _native.OK                     # an empty window enqueues nothing


@pytest.mark.parametrize("bad", [dict(w2_layout=1), dict(d_in=65), dict(nout=1), dict(out_kind=2, nout=4, h2=201), dict(out_kind=3),
                                 dict(w3=None), dict(N=0)])
def test_ppo_entry_points_reject_bad_networks(bad):
    lib = _native.lib()
    m = C.byref(actor_struct(**bad))
    n = C.c_size_t(0)
    assert lib.dronesim_mlp_grad_ppo_workspace(m, 64, C.byref(n)) == _native.EINVAL
    assert lib.dronesim_mlp_logp(m, *LOGP_OK.values(), None) == _native.EINVAL
    assert lib.dronesim_mlp_grad_ppo(m, *PPO_OK.values(), None) == _native.EINVAL


def host_mlp(kind, nout, n=3, d_in=6, h1=8, h2=8):
    """What `PPOLearner`'s constructor reads of a `BatchedMLP`, in host memory."""
    shapes = ((n, d_in, h1), (n, h1), (n, h1, h2), (n, h2), (n, h2, nout), (n, nout))
    return SimpleNamespace(n_agents=n, d_in=d_in, h1=h1, h2=h2, nout=nout, out_kind=kind, device="cpu",
                           **{name: torch.zeros(*s) for name, s in zip(NAMES, shapes)})


def test_ppo_learner_rejects_bad_arguments():
    import scalable_collision_avoidance_rl_amd as pkg
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    assert pkg.PPOLearner is PPOLearner and "PPOLearner" in pkg.__all__
    actor, critic = host_mlp(1, 16), host_mlp(0, 1)
    learner = PPOLearner(actor, critic, 0.99)
    assert (learner.epochs, learner.clip_eps, learner.baseline) == (10, 0.2, "once")
    assert PPOLearner(host_mlp(2, 4), critic, 0.99, epochs=1, baseline="per_neighbour").baseline == "per_neighbour"
    for a, c in ((critic, critic), (actor, actor), (host_mlp(1, 16, n=4), critic), (host_mlp(1, 16, d_in=15), critic)):
        with pytest.raises(ValueError):
            PPOLearner(a, c, 0.99)
    for kw in (dict(epochs=0), dict(epochs=-1), dict(epochs=1.5), dict(clip_eps=0.0), dict(clip_eps=1.0), dict(clip_eps=-0.1),
               dict(baseline="twice"), dict(baseline=None)):
        with pytest.raises(ValueError):
            PPOLearner(actor, critic, 0.99, **kw)
    z = torch.zeros(4, 2, 3, 6)
    with pytest.raises(ValueError, match="actions"):
        learner.train(SimpleNamespace(z_pre=z, reward=torch.zeros(4, 2, 3), done=torch.zeros(4, 2, dtype=torch.uint8), actions=None,
                                      nbr_pre=torch.zeros(4, 2, 3, 3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="match"):
        learner.train(SimpleNamespace(z_pre=torch.zeros(4, 2, 5, 6), reward=torch.zeros(4, 2, 5), done=torch.zeros(4, 2, dtype=torch.uint8),
                                      actions=torch.zeros(4, 2, 5, 2), nbr_pre=torch.zeros(4, 2, 5, 3, dtype=torch.int32)))
