"""GPU tests of the learner's loss heads at SATURATED policies (csrc/learner.hip: a2c_head_kernel, ppo_head_kernel) through the
public runners, against the float64 cancellation-free restatement and its sharp error scale (tests/saturation_ref.py): softmax
actors whose dominant logit is 0 .. 120 above the rest (one with every logit offset by 250), Gaussian actors whose mean sits
at tanh pre-activations of 0 .. 20 with variance pre-activations of -10, 0 and 10, one agent per regime, on a window of five
chunks with a tail of 3 rows.  The bar is |got - ref| <= 1e-5 x sharp scale + 1e-30 in every regime and form."""
import functools

import numpy as np
import pytest

from tests import entropy_ref as ER
from tests import learner_ref as R
from tests import ppo_ref as P
from tests import saturation_ref as S
from tests import test_gpu_learner as TG

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV
SENTINEL = -7.25
CASES = [(kind, actions) for kind in (1, 2) for actions in S.ACTIONS]
CASE_IDS = [f"{'softmax' if k == 1 else 'gaussian'}-{a}" for k, a in CASES]
BAR, FLOOR = S.BAR, S.FLOOR


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def reference(kind, actions, form):
    """The float64 truth of one form, computed once and shared (``gated`` is the entropy PPO form plus the kl row)."""
    return S.form_reference(S.case(kind, actions), "ppo_ent" if form == "gated" else form)


def device_inputs(c):
    d = lambda t: t.to(DEV).contiguous()
    return d(c["x"]), d(c["act"]), d(c["adv"]), d(c["logp_old"])


def run_form(torch, runner, c, form, logp_old=None, active=None, es=None):
    """One form of S.FORMS through its public runner, as the learners call it.  Returns (grad, loss, extra): extra is the
    entropy [N], the stats [4 | 5 | 6, N] or, for ``logp``, the log-probabilities [rows, N] (grad and loss None)."""
    x, act, adv, old = device_inputs(c)
    old = old if logp_old is None else logp_old
    es = S.ENT_SCALE if es is None else es
    if form == "logp":
        return None, None, runner.logp(x, act, torch.empty(S.T, S.E, len(c["regimes"]), device=DEV)).reshape(S.ROWS, -1)
    if form == "a2c":
        return (*runner.run(x, 1.0 / S.E, act=act, weight=adv), None)
    if form == "a2c_ent":
        return runner.run_ent(x, 1.0 / S.E, act, adv, es)
    if form == "ppo":
        return runner.run_ppo(x, 1.0 / S.ROWS, act, old, adv, S.CLIP_EPS)
    if form == "ppo_ent":
        return runner.run_ppo_ent(x, 1.0 / S.ROWS, act, old, adv, S.CLIP_EPS, es)
    return runner.run_ppo_gated(x, 1.0 / S.ROWS, act, old, adv, S.CLIP_EPS, es, active=active)


def extreme_bar(r, r_scale, smallest):
    """The bar of min_r / max_r over the rows [R, N] -> [N]: 1e-5 x the largest scale among the rows that may be the extreme
    one, i.e. whose ratio is within its own bar of the extreme row's."""
    bar = BAR * r_scale
    if smallest:
        edge = (r + bar).min(0).values
        cand = r - bar <= edge
    else:
        edge = (r - bar).max(0).values
        cand = r + bar >= edge
    return (bar * cand.double()).max(0).values


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_form_meets_the_sharp_bar_in_every_regime(torch, case):
    """`GradientRunner.run`, `run_ent`, `run_ppo`, `run_ppo_ent`, `run_ppo_gated`, `logp` and `mlp_gradients` on one actor kind and
    action set: all six gradient tensors, the per-agent loss, the mean entropy, the log-probabilities, the clipped count (exact),
    mean logp_old - logp, min and max ratio and the KL estimate against the float64 cancellation-free restatement at
    1e-5 x the sharp scale; everything finite, the gap of 120 and the offset of 250 included.  Prints the worst error / bar
    ratio per regime and form."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner, mlp_gradients
    kind, actions = case
    c = S.case(kind, actions)
    assert c["redrawn"] <= 0.01, c["redrawn"]
    names = [S.regime_name(kind, r) for r in c["regimes"]]
    N = len(names)
    mlp = TG.make_mlp(c["W"], kind)
    runner = GradientRunner(mlp, S.ROWS, S.ROWS_PER_CHUNK)
    failures = []

    def check(form, what, ratio):
        ratio = ratio.reshape(N, -1).max(1).values if ratio.dim() > 1 else ratio
        print(f"{CASE_IDS[CASES.index(case)]:20s} {form:8s} {what:10s} worst error / bar per regime:",
              {n: f"{float(v):.2g}" for n, v in zip(names, ratio)})
        assert bool(torch.isfinite(ratio).all()), (form, what)
        if float(ratio.max()) > 1.0:
            failures.append((form, what, names[int(ratio.argmax())], float(ratio.max())))

    for form in S.FORMS:
        ref = reference(kind, actions, form)
        g, loss, extra = (None if t is None else t.clone() for t in run_form(torch, runner, c, form))
        torch.cuda.synchronize()
        if form == "logp":
            assert bool(torch.isfinite(extra).all())
            check(form, "lp", S.ratios(extra, ref["lp"], ref["lp_scale"]).transpose(0, 1))
            continue
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss).all()) and (extra is None or bool(torch.isfinite(extra).all()))
        check(form, "gradients", S.worst_per_agent(TG.split(torch, g, mlp), ref["grad"], ref["mag"]))
        check(form, "loss", S.ratios(loss, ref["loss"], ref["loss_scale"]))
        if form == "a2c":
            g2, l2 = mlp_gradients(mlp, c["x"], act=c["act"], weight=c["adv"], rows_per_chunk=S.ROWS_PER_CHUNK)
            assert torch.equal(g2, g) and torch.equal(l2, loss)
        if form == "a2c_ent":
            check(form, "entropy", S.ratios(extra, ref["entropy"], ref["entropy_scale"]))
        if form in ("ppo", "ppo_ent", "gated"):
            stats = extra.double().cpu()
            assert stats.shape == ({"ppo": 4, "ppo_ent": 5, "gated": 6}[form], N)
            count = torch.round(stats[0] * S.ROWS).long()
            assert torch.equal(count, ref["clipped"].sum(0)), (form, count, ref["clipped"].sum(0))
            check(form, "approx_kl", S.ratios(stats[1], ref["approx_kl"], ref["dl_scale"].mean(0)))
            for row, key, smallest in ((2, "ratio_min", True), (3, "ratio_max", False)):
                bar = extreme_bar(ref["r"], ref["r_scale"], smallest)
                check(form, key, (stats[row] - ref[key]).abs() / (bar + FLOOR))
            if form != "ppo":
                check(form, "entropy", S.ratios(stats[4], ref["entropy"], ref["entropy_scale"]))
            if form == "gated":
                assert bool((stats[5] >= 0).all())
                check(form, "kl", S.ratios(stats[5], ref["kl"], ref["k_scale"].mean(0)))
    assert not failures, failures


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_heads_promises_hold_in_saturation(torch, case):
    """What the heads promise at outputs of order 1, at saturated ones: an entropy scale of 0 gives the plain head's bits (both
    families); the forward-only `logp` pass fed back as logp_old gives r == 1 exactly (clipped share 0, mean difference 0, kl 0)
    with a non-zero entropy scale; a gated agent's loss and stats are NaN and its gradient slices untouched while the others keep
    the ungated bits; a second runner reproduces every form bit for bit."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    kind, actions = case
    c = S.case(kind, actions)
    N = len(c["regimes"])
    mlp = TG.make_mlp(c["W"], kind)
    a, b = GradientRunner(mlp, S.ROWS, S.ROWS_PER_CHUNK), GradientRunner(mlp, S.ROWS, S.ROWS_PER_CHUNK)
    keep = lambda out: tuple(None if t is None else t.clone() for t in out)
    first = {form: keep(run_form(torch, a, c, form)) for form in S.FORMS}
    for form in S.FORMS:                                   # two runs, bit for bit
        for s, t in zip(first[form], run_form(torch, b, c, form)):
            assert (s is None and t is None) or torch.equal(s, t), form
    # es = 0 is the sibling
    g, l, e = run_form(torch, b, c, "a2c_ent", es=0.0)
    assert torch.equal(g, first["a2c"][0]) and torch.equal(l, first["a2c"][1]) and bool(torch.isfinite(e).all())
    g, l, s = run_form(torch, b, c, "ppo_ent", es=0.0)
    assert torch.equal(g, first["ppo"][0]) and torch.equal(l, first["ppo"][1]) and torch.equal(s[:4], first["ppo"][2])
    assert torch.equal(first["ppo_ent"][2][:4], first["ppo"][2]) and torch.equal(first["gated"][2][:5], first["ppo_ent"][2])
    assert torch.equal(first["gated"][0], first["ppo_ent"][0]) and torch.equal(first["gated"][1], first["ppo_ent"][1])
    # the forward-only pass gives ratio exactly 1
    lp = first["logp"][2].reshape(S.T, S.E, N)
    one, zero = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    for form in ("ppo", "ppo_ent", "gated"):
        g, l, s = run_form(torch, b, c, form, logp_old=lp)
        assert torch.equal(s[2], one) and torch.equal(s[3], one) and torch.equal(s[0], zero) and torch.equal(s[1], zero), form
        assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(l).all())
        if form == "gated":
            assert torch.equal(s[5], zero)
    # the gate
    active = torch.zeros(N, dtype=torch.int32)
    active[::2] = 1
    on, off = active.bool().nonzero().flatten().to(DEV), (active == 0).nonzero().flatten().to(DEV)
    b.grad.fill_(SENTINEL)
    g, l, s = run_form(torch, b, c, "gated", active=active.to(DEV))
    torch.cuda.synchronize()
    for name, got, want in zip(NAMES, TG.split(torch, g, mlp), TG.split(torch, first["gated"][0], mlp)):
        assert torch.equal(got[on], want[on]) and bool((got[off] == SENTINEL).all()), name
    assert torch.equal(l[on], first["gated"][1][on]) and torch.equal(s[:, on], first["gated"][2][:, on])
    assert bool(torch.isnan(l[off]).all()) and bool(torch.isnan(s[:, off]).all())


# 3 --------------------------------------------------------------------------------------------------------------------
def test_three_ppo_epochs_and_one_sa2c_train_on_a_collapsed_window_match_float64(torch):
    """The collapsed softmax window through `PPOLearner.train` (3 epochs) and `SA2CLearner.train` (ent_coef 0.01) against
    `ppo_ref.ppo_train` / `entropy_ref.sa2c_train` fed the cancellation-free heads, at the tolerances of test_gpu_ppo's epoch
    test (the 1e-30 floor added to the actor norms: the gap-120 agent's true gradient is 1e-50).  The softmax kind is the one
    end-to-end case: one Adam step of a Gaussian actor whose variance is 4.5e-5 moves its ratios to 1e-10 .. 9, where those
    tolerances, set for ratios near 1, have no derivation."""
    kind = 1
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner, SA2CLearner
    c = S.case(kind, "collapsed")
    T, E, N, rows, epochs = S.T, S.E, len(c["regimes"]), S.ROWS, 3
    gen = torch.Generator().manual_seed(31 + kind)
    Wa, Wc = c["W"], TG.random_net(torch, gen, N, S.D_IN, 40, 33, 1)
    x, act = c["x"], c["act"]
    reward = torch.randn(T, E, N, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8)
    done[20, ::2] = 1
    nbr = torch.stack([torch.arange(N)[None, None, :].expand(T, E, N), torch.randint(-1, N, (T, E, N), generator=gen),
                       torch.randint(0, N, (T, E, N), generator=gen)], -1).int()
    d = lambda t: t.to(DEV).contiguous()
    storage = TG.storage_of(d(x), d(reward), d(done), d(act), d(nbr))
    amax = lambda t: float(t.abs().max())
    offset_agent = [i for i, r in enumerate(c["regimes"]) if r[1] != 0]
    assert offset_agent == [N - 1]
    weights_of = lambda mlp: [getattr(mlp, n).double().cpu() for n in NAMES]

    actor, critic = TG.make_mlp(Wa, kind), TG.make_mlp(Wc, 0)
    learner = PPOLearner(actor, critic, 0.97, epochs=epochs, rows_per_chunk=S.ROWS_PER_CHUNK)
    out = learner.train(storage)
    torch.cuda.synchronize()
    ref = P.ppo_train(kind, Wa, Wc, x, reward, done, act, nbr, 0.97, epochs=epochs, actor_grads=S.actor_grads, logp=S.logp)
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["adv"]))
    assert float(S.ratios(learner.logp_old.reshape(rows, N), ref["actor"][0]["lp"], ref["actor"][0]["lp_scale"]).max()) <= 1.0
    for ep in range(epochs):
        a = ref["actor"][ep]
        near = a["near"].sum(0)
        count = torch.round(out["clip_fraction"][ep].double().cpu() * rows).long()
        print(kind, "epoch", ep, "clipped", count.tolist(), "ref", a["clipped"].sum(0).tolist(), "near an edge", near.tolist(),
              "actor norm", [f"{v:.3g}" for v in ref["actor_norm"][ep].tolist()])
        assert torch.all((count - a["clipped"].sum(0)).abs() <= near), (ep, count, a["clipped"].sum(0), near)
        np.testing.assert_allclose(out["critic_loss"][ep].cpu().numpy(), ref["critic_loss"][ep].numpy(), rtol=1e-5)
        np.testing.assert_allclose(out["critic_grad_norm"][ep].cpu().numpy(), ref["critic_norm"][ep].numpy(), rtol=1e-5)
        # the agent whose logits sit at 250: a float32 near 250 is rounded to ulp(250) / 2 = 2^-17.  The forward GEMM rounds every
        # output o_j = acc + b3_j so, and z_j = o_j - max carries two of those; once Adam has moved b3 the STORED biases are
        # rounded so as well (the float32 weights are another network than the float64 trainer's): two more.  Every p_j, so the
        # gradient norm, moves by that much of itself: 2 x 2^-17 in epoch 0, 4 x 2^-17 = 3.1e-5 after.  Measured: 7.6e-7, 1.1e-5,
        # 2.8e-5.  Every other agent at rtol 1e-5.
        rtol = np.full(N, 1e-5)
        rtol[offset_agent] += (2 if ep == 0 else 4) * 2.0 ** -17
        got, want = out["actor_grad_norm"][ep].double().cpu().numpy(), ref["actor_norm"][ep].numpy()
        print(kind, "epoch", ep, "actor norm, relative error", np.abs(got - want) / np.maximum(want, 1e-300))
        assert np.all(np.abs(got - want) <= rtol * np.abs(want) + FLOOR), (ep, got, want)
        aref = a["loss"].numpy()
        np.testing.assert_allclose(out["actor_loss"][ep].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    one = torch.ones(N, device=DEV)
    assert torch.equal(out["ratio_min"][0], one) and torch.equal(out["ratio_max"][0], one)
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    for opt, mlp, post, m2 in ((learner.critic_opt, critic, ref["critic_post"], ref["state"]["cm2"]),
                               (learner.actor_opt, actor, ref["actor_post"], ref["state"]["am2"])):
        assert int(opt.steps.min()) == int(opt.steps.max()) == epochs
        for name, got, p, v in zip(NAMES, weights_of(mlp), post, m2):
            sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
            tol = epochs * torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * opt.lr), torch.full_like(p, 2 * opt.lr))
            assert torch.all((got - p).abs() <= tol), (name, float(((got - p).abs() - tol).max()))

    actor, critic = TG.make_mlp(Wa, kind), TG.make_mlp(Wc, 0)
    learner = SA2CLearner(actor, critic, 0.97, ent_coef=0.01, rows_per_chunk=S.ROWS_PER_CHUNK)
    out = learner.train(storage)
    torch.cuda.synchronize()
    ref = ER.sa2c_train(kind, Wa, Wc, x, reward, done, act, nbr, 0.97, ent_coef=0.01, a2c_grads=S.a2c_grads)
    print(kind, "sa2c actor norm", [f"{v:.3g}" for v in ref["actor_norm"].tolist()])
    np.testing.assert_allclose(learner.w.cpu().numpy(), ref["w"].numpy(), rtol=1e-4, atol=1e-5 * amax(ref["w"]))
    np.testing.assert_allclose(out["critic_loss"].cpu().numpy(), ref["critic_loss"].numpy(), rtol=1e-5)
    np.testing.assert_allclose(out["critic_grad_norm"].cpu().numpy(), ref["critic_norm"].numpy(), rtol=1e-5)
    np.testing.assert_allclose(out["actor_grad_norm"].cpu().numpy(), ref["actor_norm"].numpy(), rtol=1e-5, atol=FLOOR)
    aref = ref["actor_loss"].numpy()
    np.testing.assert_allclose(out["actor_loss"].cpu().numpy(), aref, rtol=1e-4, atol=1e-4 * np.abs(aref).max())
    np.testing.assert_allclose(out["entropy"].cpu().numpy(), ref["entropy"].numpy(), rtol=1e-5, atol=1e-6)
    coef = torch.clamp(10.0 / (ref["actor_norm"] + 1e-6), max=1.0)
    sc = lambda t: t * coef.view(-1, *([1] * (t.dim() - 1)))
    TG.assert_grads(TG.split(torch, learner._actor_grad.grad, actor), [sc(g) for g in ref["actor_grad"]],
                    [sc(m) for m in ref["actor_mag"]], f"sa2c {kind}")
    for mlp, post in ((critic, ref["critic_post"]), (actor, ref["actor_post"])):
        for name, got, p in zip(NAMES, weights_of(mlp), post):
            assert torch.all((got - p).abs() <= 1e-3 * 0.02 + 1e-6), name
