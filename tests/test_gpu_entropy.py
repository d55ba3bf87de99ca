"""GPU tests of the learners' entropy bonus and per-agent advantage standardisation (csrc/standardize.hip: the standardisation
kernels; csrc/learner.hip: the entropy heads; `rollout_buffer.standardize`, `learner.GradientRunner.run_ent / run_ppo_ent`, the ``ent_coef`` and
``normalize_advantage`` options of `PPOLearner` / `SA2CLearner`) against the float64 restatement tests/entropy_ref.py."""
import numpy as np
import pytest

from tests import entropy_ref as ER
from tests import helpers as H
from tests import learner_ref as R
from tests import ppo_ref as P
from tests import test_gpu_learner as TG

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV
ACTOR_CASES = [c for c in TG.FUZZ if c[6] != 0]
CASE_IDS = [f"N{c[0]}E{c[1]}T{c[2]}d{c[3]}h{c[4]}x{c[5]}k{c[6]}" for c in ACTOR_CASES]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def weights_of(mlp):
    return [getattr(mlp, n).detach().cpu().clone() for n in NAMES]


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ER.STANDARDIZE_SHAPES, ids=[f"R{r}N{n}" for r, n in ER.STANDARDIZE_SHAPES])
def test_standardize_matches_float64(torch, shape):
    """`dronesim_standardize` against float64: y at the plain bar |a - b| <= 1e-5 + 1e-5 |ref|, stats at
    rtol 1e-6 -- the column at -500 +- 0.5 included, which float32 sums of x and x^2 miss (tests/test_entropy_host.py) --,
    the constant column exactly 0, everything 0 at R = 1, in place == out of place, two calls equal bit for bit."""
    from scalable_collision_avoidance_rl_amd.rollout_buffer import standardize
    rows, n = shape
    x = ER.standardize_case(rows, n)
    ref, mean, std = ER.standardize(x, 1e-8)
    xd = x.to(DEV)
    y, stats = standardize(xd, eps=1e-8, return_stats=True)
    y2 = standardize(xd.clone(), eps=1e-8)
    inplace = xd.clone()
    assert standardize(inplace, eps=1e-8, out=inplace) is inplace
    shaped = standardize(xd.reshape(1, rows, n), eps=1e-8)                 # a window's leading axes are flattened
    unaligned = torch.empty(rows * n + 1, device=DEV)[1:].view(rows, n)    # 4-byte aligned only: same lanes, scalar accesses
    unaligned.copy_(xd)
    y_un = torch.empty(rows * n + 1, device=DEV)[1:].view(rows, n)
    assert unaligned.is_contiguous() and unaligned.data_ptr() % 16 == 4
    y_un = standardize(unaligned, eps=1e-8, out=y_un)
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), x)                                        # the input is untouched out of place
    got = y.double().cpu()
    err = (got - ref).abs()
    bar = 1e-5 + 1e-5 * ref.abs()
    print(shape, "worst y error / bar", float((err / bar).max()), "hard column", float((err / bar)[:, ER.HARD_COLUMN].max()))
    assert torch.isfinite(got).all() and torch.all(err <= bar), float((err / bar).max())
    np.testing.assert_allclose(stats[0].cpu().numpy(), mean.numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(stats[1].cpu().numpy(), std.numpy(), rtol=1e-6, atol=0)
    assert torch.all(y[:, ER.CONSTANT_COLUMN] == 0) and float(stats[1, ER.CONSTANT_COLUMN]) == 0.0
    if rows == 1:
        assert torch.all(y == 0)
    assert torch.equal(y, y2) and torch.equal(y, inplace) and torch.equal(y, shaped.view(rows, n)) and torch.equal(y, y_un)


# 2 --------------------------------------------------------------------------------------------------------------------
def head_inputs(torch, case):
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c = P.head_case(case)
    assert c["redrawn"] <= 0.01, c["redrawn"]
    d = lambda t: t.to(DEV).contiguous()
    rows = T * E
    r2 = lambda t: d(t).reshape(rows, N, *t.shape[3:])
    return c, d, r2, rows


@pytest.mark.parametrize("case", ACTOR_CASES, ids=CASE_IDS)
def test_ppo_entropy_head_matches_float64_autograd(torch, case):
    """`dronesim_mlp_grad_ppo_ent` with ent_scale = 0.01 / rows on the inputs of test_gpu_ppo's head test (supplied logp_old
    with ratios over [0.5, 2], advantages of both signs, ragged R, several chunks): gradients at 1e-5 x the reference's
    magnitudes, the loss (the whole objective) at that test's bar, the entropy at
    rtol 1e-5 / atol 1e-6, stats[0..3] as that test checks them."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c, d, r2, rows = head_inputs(torch, case)
    es = 0.01 / rows
    mlp = TG.make_mlp(c["W"], kind)
    runner = GradientRunner(mlp, rows, rc)
    g, loss, stats = runner.run_ppo_ent(d(c["x"]), 1.0 / rows, d(c["act"]), d(c["logp_old"]), d(c["adv"]), 0.2, es)
    torch.cuda.synchronize()
    assert stats.shape == (5, N)
    ref = ER.actor_grads(kind, [d(w) for w in c["W"]], r2(c["x"]), r2(c["act"]), r2(c["logp_old"]), r2(c["adv"]), 0.2, es)
    assert not ref["near"].any()
    print(case, "entropy", float(ref["entropy"].min()), float(ref["entropy"].max()), "entropy share of the loss",
          float((ref["entropy_loss"].abs() / ref["loss"].abs()).max()))
    TG.assert_grads(TG.split(torch, g, mlp), ref["grad"], ref["mag"], str(case))
    count = torch.round(stats[0].double() * rows).long()
    assert torch.equal(count, ref["clipped"].sum(0)), (count, ref["clipped"].sum(0))
    A = r2(c["adv"]).double()
    lmag = (ref["r"] * A).abs().sum(0) / rows
    assert torch.all((loss.double() - ref["loss"]).abs() <= 1e-5 * lmag + 1e-30), (loss, ref["loss"])
    klmag = (r2(c["logp_old"]).double().abs() + ref["logp"].abs()).mean(0)
    assert torch.all((stats[1].double() - ref["approx_kl"]).abs() <= 1e-5 * klmag), (stats[1], ref["approx_kl"])
    rtol = 1e-5 * (1 + float(ref["logp"].abs().max()))
    np.testing.assert_allclose(stats[2].cpu().numpy(), ref["ratio_min"].cpu().numpy(), rtol=rtol)
    np.testing.assert_allclose(stats[3].cpu().numpy(), ref["ratio_max"].cpu().numpy(), rtol=rtol)
    np.testing.assert_allclose(stats[4].cpu().numpy(), ref["entropy"].cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", ACTOR_CASES, ids=CASE_IDS)
def test_a2c_entropy_head_matches_float64_autograd(torch, case):
    """`dronesim_mlp_grad_ent` with the ``weight`` input (here the case's advantage), row_scale 1 / E as the learner passes."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c, d, r2, rows = head_inputs(torch, case)
    es = 0.01 / rows
    mlp = TG.make_mlp(c["W"], kind)
    runner = GradientRunner(mlp, rows, rc)
    g, loss, ent = runner.run_ent(d(c["x"]), 1.0 / E, d(c["act"]), d(c["adv"]), es)
    torch.cuda.synchronize()
    Wd = [d(w) for w in c["W"]]
    ref = ER.a2c_grads(kind, Wd, r2(c["x"]), 1.0 / E, r2(c["act"]), r2(c["adv"]), es)
    TG.assert_grads(TG.split(torch, g, mlp), ref["grad"], ref["mag"], str(case))
    lmag = (1.0 / E) * R.row_losses(kind, R.forward([w.double() for w in Wd], r2(c["x"]).double())[2], act=r2(c["act"]).double(),
                                    weight=r2(c["adv"]).double()).abs().sum(1)
    assert torch.all((loss.double() - ref["loss"]).abs() <= 1e-5 * lmag + 1e-30), (loss, ref["loss"])
    np.testing.assert_allclose(ent.cpu().numpy(), ref["entropy"].cpu().numpy(), rtol=1e-5, atol=1e-6)


# 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [ACTOR_CASES[0], ACTOR_CASES[1]], ids=CASE_IDS[:2])
def test_zero_entropy_scale_keeps_the_siblings_bits(torch, case):
    """Both new entry points at ent_scale = 0 against `dronesim_mlp_grad_ppo` / `dronesim_mlp_grad`: torch.equal gradient
    buffers, losses and stats[0..3] (a softmax case of 5 chunks with a ragged last one, a Gaussian case of 4)."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c, d, r2, rows = head_inputs(torch, case)
    assert rows % rc != 0 and rows > 3 * rc
    mlp = TG.make_mlp(c["W"], kind)
    x, act, old, adv = d(c["x"]), d(c["act"]), d(c["logp_old"]), d(c["adv"])
    a, b = GradientRunner(mlp, rows, rc), GradientRunner(mlp, rows, rc)
    g0, l0, s0 = (t.clone() for t in a.run_ppo(x, 1.0 / rows, act, old, adv, 0.2))
    g1, l1, s1 = b.run_ppo_ent(x, 1.0 / rows, act, old, adv, 0.2, 0.0)
    assert torch.equal(g0, g1) and torch.equal(l0, l1) and torch.equal(s0, s1[:4])
    assert torch.isfinite(s1[4]).all() and float(s1[4].min()) != 0.0
    g0, l0 = (t.clone() for t in a.run(x, 1.0 / E, act=act, weight=adv))
    g1, l1, e1 = b.run_ent(x, 1.0 / E, act, adv, 0.0)
    assert torch.equal(g0, g1) and torch.equal(l0, l1) and torch.allclose(e1, s1[4], rtol=1e-6, atol=0)
    # and the log-probability is the forward-only pass's: ratio exactly 1 with a non-zero entropy scale
    lp = a.logp(x, act, torch.empty(T, E, N, device=DEV))
    _, _, s2 = b.run_ppo_ent(x, 1.0 / rows, act, lp, adv, 0.2, 0.01 / rows)
    one = torch.ones(N, device=DEV)
    assert torch.equal(s2[2], one) and torch.equal(s2[3], one) and torch.equal(s2[0], 0 * one) and torch.equal(s2[1], 0 * one)


# 4 --------------------------------------------------------------------------------------------------------------------
def test_saturated_softmax_row_stays_finite(torch):
    """One agent's b3 puts one logit 120 above the rest: p = 0 for the others in float32.  The entropy comes from
    lq = o - lse, not log(p): every gradient element, the loss and the entropy are finite, that agent's entropy below 1e-6."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    case = ACTOR_CASES[0]
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c, d, r2, rows = head_inputs(torch, case)
    W = [w.clone() for w in c["W"]]
    W[5][2] = 0.0
    W[5][2, 7] = 250.0
    O = R.forward([w.double() for w in W], c["x"].reshape(rows, N, d_in).double())[2][2]
    gap = O[:, 7] - torch.cat([O[:, :7], O[:, 8:]], 1).max(1).values
    assert float(gap.min()) >= 120.0, float(gap.min())
    mlp = TG.make_mlp(W, kind)
    runner = GradientRunner(mlp, rows, rc)
    for run in (lambda: runner.run_ppo_ent(d(c["x"]), 1.0 / rows, d(c["act"]), d(c["logp_old"]), d(c["adv"]), 0.2, 0.01 / rows),
                lambda: runner.run_ent(d(c["x"]), 1.0 / E, d(c["act"]), d(c["adv"]), 0.01 / rows)):
        g, loss, last = (t.clone() for t in run())
        ent = last[4] if last.dim() == 2 else last
        assert torch.isfinite(g).all() and torch.isfinite(loss).all() and torch.isfinite(last).all()
        assert 0 <= float(ent[2]) < 1e-6, float(ent[2])
        assert float(ent[[0, 1, 3, 4]].min()) > 0.1


# 5 --------------------------------------------------------------------------------------------------------------------
N_RS, G_RS, E_RS, T_RS = TG.N_RS, TG.G_RS, TG.E_RS, TG.T_RS


def storage_setup(torch, kind=1, seed_env=5, **kw):
    """`test_gpu_ppo.storage_setup` with either actor kind: a batched env whose episodes end inside the first window, a
    softmax-16 or Gaussian actor, a critic, a real RolloutStorage, a PPOLearner with the given options."""
    from scalable_collision_avoidance_rl_amd import drones
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    from scalable_collision_avoidance_rl_amd.policies import BatchedMLP
    from scalable_collision_avoidance_rl_amd.rollout_buffer import RolloutStorage
    N, G, E, T = N_RS, G_RS, E_RS, T_RS
    gp = torch.Generator().manual_seed(0)
    rw = lambda *s: (torch.rand(*s, generator=gp) * 2 - 1) * 0.2
    nout = 16 if kind == 1 else 4
    wa = [rw(N, 6, 48), rw(N, 48), rw(N, 48, 48), rw(N, 48), rw(N, 48, nout), rw(N, nout)]
    wc = [rw(N, 6, 32), rw(N, 32), rw(N, 32, 32), rw(N, 32), rw(N, 32, 1), rw(N, 1)]
    if kind == 2:
        wa[4] = wa[4] * R.structural_mask(2, wa)
    env = drones(N, 0, [G, G], "O", k_closest=2, deltas=np.ones(N), simplify_zstate=True, n_envs=E, batched=True,
                 device=DEV, seed=seed_env, auto_reset=True)
    env.t.fill_(193)                                       # the time limit fires inside the first window
    actor, critic = BatchedMLP(*wa, kind, kind, device=DEV, seed=7), BatchedMLP(*wc, 0, 0, device=DEV)
    st = RolloutStorage(env, T, actions=True)
    return env, actor, critic, st, PPOLearner(actor, critic, 0.99, **kw)


@pytest.mark.parametrize("kind", [1, 2], ids=["softmax", "gaussian"])
@pytest.mark.parametrize("baseline", ["once", "per_neighbour"])
def test_four_epochs_with_both_options_match_float64(torch, baseline, kind):
    """One rollout window with an episode end inside it, then `PPOLearner(ent_coef=0.01, normalize_advantage=True).train` of
    four epochs against entropy_ref.ppo_train, at the tolerances of test_gpu_ppo's four-epoch test.  A row whose standardised
    advantage is within 1e-4 of 0 may take either side of the clip test: the clipped COUNT is compared up to the number of
    such rows (plus those near a clip edge, as that test allows), and they are at most 1 % of the window."""
    epochs = 4
    env, actor, critic, st, learner = storage_setup(torch, kind, epochs=epochs, baseline=baseline, ent_coef=0.01,
                                                    normalize_advantage=True)
    T, E, N = T_RS, E_RS, N_RS
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    Wa, Wc = weights_of(actor), weights_of(critic)
    data = [t.cpu().clone() for t in (st.z_pre, st.reward, st.done, st.actions, st.nbr_pre)]
    assert int(data[2].sum()) == E
    out = learner.train(st)
    torch.cuda.synchronize()
    assert set(out) >= {"entropy", "adv_mean", "adv_std"} and out["entropy"].shape == (epochs, N) and out["adv_mean"].shape == (N,)
    assert learner.adv_stats.shape == (2, N) and torch.equal(learner.adv_stats[0], out["adv_mean"])
    ref = ER.ppo_train(kind, Wa, Wc, *data, 0.99, epochs=epochs, baseline=baseline, ent_coef=0.01, normalize_advantage=True)
    amax = lambda t: float(t.abs().max())
    rows = T * E
    near0 = ref["near_zero"].sum(0)
    print(baseline, kind, "rows within 1e-4 of a zero advantage", near0.tolist(), "raw adv mean", ref["adv_mean"].tolist()[:4],
          "std", ref["adv_std"].tolist()[:4])
    assert int(near0.sum()) <= 0.01 * rows * N
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
    # the raw advantage's float32 rounding (test_gpu_ppo: 1e-5 of its largest value) divided by the std, like the advantage
    atol = float((1e-5 * amax(ref["adv_raw"]) / ref["adv_std"]).max())
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-4, atol=atol)
    np.testing.assert_allclose(out["adv_mean"].cpu().numpy(), ref["adv_mean"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["adv_raw"]))
    np.testing.assert_allclose(out["adv_std"].cpu().numpy(), ref["adv_std"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["adv_raw"]))
    for ep in range(epochs):
        a = ref["actor"][ep]
        slack = a["near"].sum(0) + near0
        count = torch.round(out["clip_fraction"][ep].double().cpu() * rows).long()
        print(baseline, kind, "epoch", ep, "clipped", count.tolist(), "ref", a["clipped"].sum(0).tolist(), "slack", slack.tolist(),
              "entropy", float(out["entropy"][ep].mean()))
        assert torch.all((count - a["clipped"].sum(0)).abs() <= slack), (ep, count, a["clipped"].sum(0), slack)
        np.testing.assert_allclose(out["critic_loss"][ep].cpu().numpy(), ref["critic_loss"][ep].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["critic_grad_norm"][ep].cpu().numpy(), ref["critic_norm"][ep].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["actor_grad_norm"][ep].cpu().numpy(), ref["actor_norm"][ep].numpy(), rtol=1e-5)
        aref = a["loss"].numpy()
        np.testing.assert_allclose(out["actor_loss"][ep].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
        np.testing.assert_allclose(out["entropy"][ep].cpu().numpy(), ref["entropy"][ep].numpy(), rtol=1e-5, atol=1e-6)
    one = torch.ones(N, device=DEV)
    assert torch.equal(out["ratio_min"][0], one) and torch.equal(out["ratio_max"][0], one)
    assert torch.equal(out["clip_fraction"][0], 0 * one) and torch.equal(out["approx_kl"][0], 0 * one)


# 6 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["softmax", "gaussian"])
def test_sa2c_with_entropy_on_the_episode_matches_float64(torch, kind):
    """One `SA2CLearner(ent_coef=0.01).train` on the N = 5 episode of the learner fixture's inputs against
    entropy_ref.sa2c_train, at the existing learner tests' tolerances; the critic step is the plain learner's, bit for bit."""
    from scalable_collision_avoidance_rl_amd.learner import SA2CLearner
    fx = dict(H.load("learner_n5.npz"))
    x, reward, done, act, nbr = TG.episode(torch)
    actor_w, critic_w = TG.initial(fx, kind)
    k = 1 if kind == "softmax" else 2
    actor, critic = TG.make_mlp(actor_w, k), TG.make_mlp(critic_w, 0)
    learner = SA2CLearner(actor, critic, 0.99, ent_coef=0.01)
    out = learner.train(TG.storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    ref = ER.sa2c_train(k, actor_w, critic_w, x.cpu(), reward.cpu(), done.cpu(), act.cpu(), nbr.cpu(), 0.99, ent_coef=0.01)
    assert out["entropy"].shape == (5,)
    np.testing.assert_allclose(out["entropy"].cpu().numpy(), ref["entropy"].numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["critic_loss"].cpu().numpy(), ref["critic_loss"].numpy(), rtol=1e-5)
    np.testing.assert_allclose(out["critic_grad_norm"].cpu().numpy(), ref["critic_norm"].numpy(), rtol=2e-5)
    np.testing.assert_allclose(out["actor_grad_norm"].cpu().numpy(), ref["actor_norm"].numpy(), rtol=2e-5)
    aref = ref["actor_loss"].numpy()
    np.testing.assert_allclose(out["actor_loss"].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    np.testing.assert_allclose(learner.w.cpu().numpy(), ref["w"].numpy(), rtol=1e-5, atol=1e-5 * float(ref["w"].abs().max()))
    # the gradient buffer holds the CLIPPED gradient after the Adam step: scale the reference alike
    coef = torch.clamp(10.0 / (ref["actor_norm"] + 1e-6), max=1.0)
    sc = lambda t: t * coef.view(-1, *([1] * (t.dim() - 1)))
    TG.assert_grads(TG.split(torch, learner._actor_grad.grad, actor), [sc(g) for g in ref["actor_grad"]],
                    [sc(m) for m in ref["actor_mag"]], kind)
    for name, p in zip(NAMES, ref["actor_post"]):
        assert torch.all((getattr(actor, name).double().cpu() - p).abs() <= 1e-3 * 0.02 + 1e-6), name
    actor2, critic2 = TG.make_mlp(actor_w, k), TG.make_mlp(critic_w, 0)
    out2 = SA2CLearner(actor2, critic2, 0.99).train(TG.storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    assert "entropy" not in out2 and torch.equal(out["critic_loss"], out2["critic_loss"])
    for n in NAMES:
        assert torch.equal(getattr(critic, n), getattr(critic2, n)), n
    assert any(not torch.equal(getattr(actor, n), getattr(actor2, n)) for n in NAMES)


# 7 --------------------------------------------------------------------------------------------------------------------
def test_defaults_are_the_old_path(torch):
    """Learners built with ``ent_coef=0.0, normalize_advantage=False`` and learners built without the keywords: torch.equal
    weights, moments, G, adv and every returned tensor after two windows, the same keys, and no buffer of the new paths."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    N, E, T, d_in = 6, 9, 41, 6
    gen = torch.Generator().manual_seed(19)
    Wa, Wc = TG.random_net(torch, gen, N, d_in, 72, 40, 16), TG.random_net(torch, gen, N, d_in, 40, 33, 1)
    d = lambda t: t.to(DEV).contiguous()
    windows = []
    for _ in range(2):
        x, _, act, _ = TG.random_rows(torch, gen, T, E, N, d_in, 16, 1)
        reward = torch.randn(T, E, N, generator=gen)
        done = torch.zeros(T, E, dtype=torch.uint8)
        done[20, ::2] = 1
        nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                           torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
        windows.append(TG.storage_of(d(x), d(reward), d(done), d(act), d(nbr)))
    for cls, kws, extra in ((PPOLearner, dict(ent_coef=0.0, normalize_advantage=False), dict(epochs=3, rows_per_chunk=128)),
                            (SA2CLearner, dict(ent_coef=0.0), dict(rows_per_chunk=128))):
        runs = []
        for kw in ({}, kws):
            actor, critic = TG.make_mlp(Wa, 1), TG.make_mlp(Wc, 0)
            learner = cls(actor, critic, 0.97, **extra, **kw)
            snap = []
            for st in windows:
                out = learner.train(st)
                torch.cuda.synchronize()
                snap += [out[k].clone() for k in sorted(out)] + [learner.G.clone()]
                snap += [learner.adv.clone()] if cls is PPOLearner else [learner.w.clone()]
            assert sorted(out) == sorted(["critic_loss", "actor_loss", "critic_grad_norm", "actor_grad_norm"] +
                                         (["clip_fraction", "approx_kl", "ratio_min", "ratio_max"] if cls is PPOLearner else []))
            assert not hasattr(learner, "adv_stats") and not hasattr(learner._actor_grad, "stats5")
            assert not hasattr(learner._actor_grad, "entropy")
            if cls is PPOLearner:
                assert learner._stats.shape == (3, 4, N)
            runs.append(snap + [getattr(m, n).clone() for m in (actor, critic) for n in NAMES] +
                        [learner.actor_opt.m1, learner.actor_opt.m2, learner.critic_opt.m1, learner.critic_opt.m2])
        for j, (a, b) in enumerate(zip(*runs)):
            assert torch.equal(a, b), (cls.__name__, j)


# 8 --------------------------------------------------------------------------------------------------------------------
def test_rollout_window_and_train_with_both_options_in_one_graph(torch):
    """A storage window (policy -> step, T steps) and `PPOLearner(ent_coef=0.01, normalize_advantage=True).train` (3 epochs)
    captured in ONE graph: three replays equal the same sequence run eagerly by a second learner on the same data, bit for
    bit (so two learners on the same data are bit-identical, too)."""
    epochs = 3
    kw = dict(epochs=epochs, ent_coef=0.01, normalize_advantage=True)
    env, actor, critic, st, learner = storage_setup(torch, **kw)

    def window(env, actor, st, learner):
        TG.rollout_window(env, actor, st)
        return learner.train(st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = window(env, actor, st, learner)              # window 1 eagerly: builds the slots and the learner's buffers
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = window(env, actor, st, learner)
    env2, actor2, critic2, st2, learner2 = storage_setup(torch, **kw)
    keys = sorted(out)
    assert "entropy" in keys and "adv_std" in keys
    snap = lambda a, c, l, s_, o: [t.clone() for t in [getattr(m, n) for m in (a, c) for n in NAMES] +
                                   [l.actor_opt.m1, l.actor_opt.m2, l.critic_opt.m1, l.critic_opt.m2, s_.z_pre, l.logp_old, l.adv,
                                    l.adv_stats] + [o[k] for k in keys]]
    ref = []
    for _ in range(4):
        o2 = window(env2, actor2, st2, learner2)
        ref.append(snap(actor2, critic2, learner2, st2, o2))
    torch.cuda.synchronize()
    for rep in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        got = snap(actor, critic, learner, st, out)
        for j, (a, b) in enumerate(zip(got, ref[rep])):
            assert torch.equal(a, b), (rep, j)
        assert int(learner.actor_opt.steps.min()) == int(learner.critic_opt.steps.max()) == epochs * (rep + 1)
    assert all(torch.isfinite(t).all() for t in got)
    assert float(out["entropy"].min()) > 0 and float((learner.adv.mean((0, 1))).abs().max()) < 1e-4
