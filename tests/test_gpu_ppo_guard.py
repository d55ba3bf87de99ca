"""GPU tests of the PPO learner's two guards (csrc/learner.hip: the per-agent gate through the chain, `dronesim_kl_gate`,
`dronesim_adam_step_gated`, the clipped value head; `learner.PPOLearner(target_kl=, vf_clip=)`) against the siblings bit for bit
and against the float64 restatement (tests/ppo_guard_ref.py)."""
import ctypes as C
import math
import time

import numpy as np
import pytest

from tests import learner_ref as R
from tests import ppo_guard_ref as GR
from tests import ppo_ref as P
from tests import test_gpu_learner as TG
from tests import test_gpu_minibatch as TM
from tests import test_gpu_ppo as TP

pytestmark = pytest.mark.gpu
NAMES = R.NAMES
DEV = TG.DEV
ACTOR_CASES = TP.ACTOR_CASES
CRITIC_CASES = [c for c in TG.FUZZ if c[6] == 0]
CASE_ID = lambda c: f"N{c[0]}E{c[1]}T{c[2]}d{c[3]}h{c[4]}x{c[5]}k{c[6]}"
SENTINEL = -12345.5
EPOCHS = 6                                                              # of the learner tests on the synthetic Gaussian window
KW = dict(epochs=EPOCHS, rows_per_chunk=128, lr_actor=3e-3)
ACTOR_KEYS = ("actor_loss", "clip_fraction", "approx_kl", "ratio_min", "ratio_max", "entropy", "kl")


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def same_bits(torch, a, b):
    """`torch.equal` that also holds NaN against NaN: the bits of the two tensors."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == torch.float32:
        a, b = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return torch.equal(a, b)


def patterns(torch, N):
    """all ones, all zeros, only agent 0, only agent N - 1, alternating"""
    one, zero = torch.ones(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int32)
    first, last, alt = zero.clone(), zero.clone(), zero.clone()
    first[0], last[N - 1] = 1, 1
    alt[::2] = 1
    return dict(ones=one, zeros=zero, first=first, last=last, alternating=alt)


def agent_slices(torch, flat, mlp):
    return TG.split(torch, flat, mlp)


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACTOR_CASES, ids=[CASE_ID(c) for c in ACTOR_CASES])
def test_gated_head_equals_the_entropy_head_on_active_agents_and_skips_the_others(torch, case):
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c = P.head_case(case)
    rows = T * E
    mlp = TG.make_mlp(c["W"], kind)
    d = lambda t: t.to(DEV).contiguous()
    args = (d(c["x"]), 1.0 / rows, d(c["act"]), d(c["logp_old"]), d(c["adv"]), 0.2, 0.01 / rows)
    plain = GradientRunner(mlp, rows, rc)
    g0, l0, s0 = plain.run_ppo_ent(*args)
    g0, l0, s0 = agent_slices(torch, g0.clone(), mlp), l0.clone(), s0.clone()
    runner = GradientRunner(mlp, rows, rc)
    nan_of = lambda t: bool(torch.isnan(t).all())
    for name, active in [("none", None)] + list(patterns(torch, N).items()):
        on = torch.ones(N, dtype=torch.bool) if active is None else active.bool()
        runner.grad.fill_(SENTINEL)
        g, loss, stats = runner.run_ppo_gated(*args, active=None if active is None else active.to(DEV))
        torch.cuda.synchronize()
        assert stats.shape == (6, N)
        idx, off = on.nonzero().flatten().to(DEV), (~on).nonzero().flatten().to(DEV)
        for tn, a, b in zip(NAMES, agent_slices(torch, g, mlp), g0):
            assert torch.equal(a[idx], b[idx]), (name, tn)
            assert bool((a[off] == SENTINEL).all()), (name, tn)
        assert torch.equal(loss[idx], l0[idx]) and torch.equal(stats[:5, idx], s0[:, idx]), name
        assert bool(torch.isfinite(stats[5, idx]).all()) and bool((stats[5, idx] >= 0).all()), name
        if len(off):
            assert nan_of(loss[off]) and nan_of(stats[:, off]), name
        if name == "none":
            kl_all = stats[5].clone()
        else:
            assert torch.equal(stats[5, idx], kl_all[idx]), name          # an agent's KL does not depend on who else is gated


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ACTOR_CASES, ids=[CASE_ID(c) for c in ACTOR_CASES])
def test_kl_estimate_matches_float64_and_is_exactly_zero_at_ratio_one(torch, case):
    """stats[5] at the bar test_gpu_ppo puts on approx_kl, 1e-5 x mean(|logp_old| + |logp|): |dk / d dl| = |r - 1| <= 1 on
    `head_case`'s ratios in [0.5, 2]."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    c = P.head_case(case)
    rows = T * E
    mlp = TG.make_mlp(c["W"], kind)
    d = lambda t: t.to(DEV).contiguous()
    runner = GradientRunner(mlp, rows, rc)
    _, _, stats = runner.run_ppo_gated(d(c["x"]), 1.0 / rows, d(c["act"]), d(c["logp_old"]), d(c["adv"]), 0.2, 0.0)
    torch.cuda.synchronize()
    r2 = lambda t: d(t).reshape(rows, N, *t.shape[3:])
    lp = P.logp(kind, [d(w) for w in c["W"]], r2(c["x"]), r2(c["act"]))
    old = r2(c["logp_old"]).double()
    ref = GR.kl_estimate(lp, old)
    bar = 1e-5 * (old.abs() + lp.abs()).mean(0)
    print(case, "kl", stats[5].tolist()[:4], "ref", ref.tolist()[:4], "worst / bar", float(((stats[5].double() - ref).abs() / bar).max()))
    assert torch.all((stats[5].double() - ref).abs() <= bar), (stats[5], ref)
    assert float(ref.min()) > 0 and float(stats[5].min()) > 0
    own = runner.logp(d(c["x"]), d(c["act"]), torch.empty(T, E, N, device=DEV))
    _, _, stats = runner.run_ppo_gated(d(c["x"]), 1.0 / rows, d(c["act"]), own, d(c["adv"]), 0.2, 0.0)
    assert torch.equal(stats[5], torch.zeros(N, device=DEV))


# 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 5, 257])
def test_kl_gate_kernel_follows_the_host_rule(torch, N):
    from scalable_collision_avoidance_rl_amd import _native
    lib, tau = _native.lib(), 0.02
    tau32 = float(np.float32(tau))
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = torch.Generator().manual_seed(N)
    active = torch.randint(0, 2, (N,), generator=gen).int().to(DEV)
    taken = torch.randint(0, 9, (N,), generator=gen).int().to(DEV)
    _native.check(lib.dronesim_kl_gate(None, tau, active.data_ptr(), taken.data_ptr(), N, 1, stream()), "dronesim_kl_gate")
    assert torch.equal(active.cpu(), torch.ones(N, dtype=torch.int32)) and torch.equal(taken.cpu(), torch.zeros(N, dtype=torch.int32))
    ha, ht = [1] * N, [0] * N
    special = [tau32, float(np.nextafter(np.float32(tau), np.float32(1))), float(np.nextafter(np.float32(tau), np.float32(0))),
               float("nan"), 0.0, float("inf"), 0.03]
    for step in range(6):
        kl = (torch.rand(N, generator=gen) * 0.0225).float()           # about nine in ten below the threshold
        for j, v in enumerate(special):
            if (j + step) % 3 == 0 and j < N:
                kl[(j * 37 + step) % N] = v
        kl_dev = kl.to(DEV)
        _native.check(lib.dronesim_kl_gate(kl_dev.data_ptr(), tau, active.data_ptr(), taken.data_ptr(), N, 0, stream()),
                      "dronesim_kl_gate")
        ha, ht = GR.gate(ha, ht, kl.tolist(), tau32)
        assert active.cpu().tolist() == ha and taken.cpu().tolist() == ht, step
    if N == 257:
        assert 0 in ha and 1 in ha and max(ht) == 6 and min(ht) == 0     # some stopped (and stayed stopped), some never did
    _native.check(lib.dronesim_kl_gate(None, tau, active.data_ptr(), taken.data_ptr(), N, 1, stream()), "dronesim_kl_gate")
    assert int(active.sum()) == N and int(taken.sum()) == 0


# 4 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 2])
def test_gated_adam_step_is_the_plain_step_on_active_agents_and_nothing_on_the_others(torch, kind):
    """The shapes of `test_clip_and_adam_match_torch_over_five_steps`, five steps, a pattern that changes per step; every step is
    compared with `dronesim_adam_step` on a twin built from the copied state."""
    from scalable_collision_avoidance_rl_amd.learner import BatchedAdam
    N, d_in, h1, h2, nout = 6, 6, 40, 32, (1 if kind == 0 else 4)
    gen = torch.Generator().manual_seed(9)
    W = TG.random_net(torch, gen, N, d_in, h1, h2, nout)
    mask = R.structural_mask(kind, W)
    W[4] = W[4] * mask
    mlp = TG.make_mlp(W, kind)
    opt = BatchedAdam(mlp, lr=2e-3, max_norm=10.0)
    scales = torch.tensor([0.01, 0.3, 1.0, 5.0, 30.0, 100.0])
    pats = [[1, 0, 1, 1, 0, 1], [0, 1, 1, 0, 1, 1], [1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 0, 0], [0, 1, 0, 1, 1, 0]]
    for step, pat in enumerate(pats):
        g = [torch.randn(*w.shape, generator=gen) * scales.view(-1, *([1] * (w.dim() - 1))) / 30 for w in W]
        g[4] = g[4] * mask
        flat = torch.cat([t.reshape(-1) for t in g]).to(DEV)
        before = [getattr(mlp, n).clone() for n in NAMES]
        twin = TG.make_mlp([w.cpu() for w in before], kind)
        topt = BatchedAdam(twin, lr=2e-3, max_norm=10.0)
        topt.m1.copy_(opt.m1); topt.m2.copy_(opt.m2); topt.steps.copy_(opt.steps)
        m1b, m2b, sb = opt.m1.clone(), opt.m2.clone(), opt.steps.clone()
        tflat = flat.clone()
        tnorm = topt.step(tflat).clone()
        active = torch.tensor(pat, dtype=torch.int32, device=DEV)
        gflat = flat.clone()
        norm = opt.step(gflat, active=active).clone()
        torch.cuda.synchronize()
        on, off = active.bool().nonzero().flatten(), (active == 0).nonzero().flatten()
        assert torch.equal(norm[on], tnorm[on]) and bool(torch.isnan(norm[off]).all()), step
        assert torch.equal(opt.steps[on], topt.steps[on]) and torch.equal(opt.steps[off], sb[off]), step
        for j, name in enumerate(NAMES):
            assert torch.equal(getattr(mlp, name)[on], getattr(twin, name)[on]), (step, name)
            assert torch.equal(getattr(mlp, name)[off], before[j][off]), (step, name)
        for what, got, want_on, want_off in (("m1", opt.m1, topt.m1, m1b), ("m2", opt.m2, topt.m2, m2b), ("grad", gflat, tflat, flat)):
            for a, b, c_ in zip(agent_slices(torch, got, mlp), agent_slices(torch, want_on, mlp), agent_slices(torch, want_off, mlp)):
                assert torch.equal(a[on], b[on]) and torch.equal(a[off], c_[off]), (step, what)
    assert opt.steps.cpu().tolist() == [sum(p[i] for p in pats) for i in range(N)]


# 5 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CRITIC_CASES, ids=[CASE_ID(c) for c in CRITIC_CASES])
def test_clipped_value_head_matches_float64_and_is_the_plain_head_where_nothing_is_clamped(torch, case):
    """v_old = V_ref - u, u ~ U[-2 eps, 2 eps], eps = 0.2: about half the rows clamped, a quarter on the zero-gradient branch; rows
    near an edge were redrawn by `ppo_guard_ref.vclip_case`, at most 1 %."""
    from scalable_collision_avoidance_rl_amd.learner import GradientRunner
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    eps = 0.2
    c = GR.vclip_case(case, eps)
    assert c["redrawn"] <= 0.01, c["redrawn"]
    rows = T * E
    mlp = TG.make_mlp(c["W"], 0)
    d = lambda t: t.to(DEV).contiguous()
    r2 = lambda t: d(t).reshape(rows, N, *t.shape[3:])
    x, G, v_old = d(c["x"]), d(c["target"]), d(c["v_old"])
    runner = GradientRunner(mlp, rows, rc)
    g, loss, clip = runner.run_vclip(x, 1.0 / rows, G, v_old, eps)
    torch.cuda.synchronize()
    ref = GR.vclip_grads([d(w) for w in c["W"]], r2(c["x"]), 1.0 / rows, r2(c["target"]), r2(c["v_old"]), eps)
    assert not ref["near"].any()
    print(case, "redrawn", c["redrawn"], "zero-gradient share", float(ref["zero"].double().mean()), "clamped share",
          float(ref["clamped"].double().mean()))
    TG.assert_grads(TG.split(torch, g, mlp), ref["grad"], ref["mag"], str(case))
    lmag = ref["rows"].abs().sum(0) / rows
    assert torch.all((loss.double() - ref["loss"]).abs() <= 1e-5 * lmag + 1e-30), (loss, ref["loss"])
    count = torch.round(clip.double() * rows).long()
    assert torch.equal(count, ref["zero"].sum(0)), (count, ref["zero"].sum(0))
    if rows > 1:
        assert 0.15 < float(ref["zero"].double().mean()) < 0.35 and 0.4 < float(ref["clamped"].double().mean()) < 0.6
    # nothing clamped: the plain head's bits
    g1, l1 = [t.clone() for t in GradientRunner(mlp, rows, rc).run(x, 1.0 / rows, target=G)]
    V = R.forward([w.double() for w in c["W"]], c["x"].reshape(rows, N, d_in).double())[2][..., 0].transpose(0, 1)
    inside = (V - (V - c["v_old"].reshape(rows, N).double()) / 4).float().reshape(T, E, N)      # within eps / 2 of V
    for v, e in ((v_old, float("inf")), (d(inside), eps)):
        g2, l2, clip2 = GradientRunner(mlp, rows, rc).run_vclip(x, 1.0 / rows, G, v, e)
        assert torch.equal(g2, g1) and torch.equal(l2, l1) and torch.equal(clip2, torch.zeros(N, device=DEV)), e


# the learner on the synthetic Gaussian window ----------------------------------------------------------------------------
_CACHE = {}


def window(torch):
    """The data of `test_two_learners_on_the_same_data_are_bit_identical`, its float64 restatement WITHOUT the gate (the kl table of
    every agent and epoch: an agent's actor depends on no other agent and not on the critic after step 2) and the threshold
    `ppo_guard_ref.pick_tau` takes from it; computed once."""
    if not _CACHE:
        _, _, Wa, Wc, data = TM.gaussian_setup(torch)
        ref = GR.ppo_train(2, Wa, Wc, *data, 0.97, epochs=EPOCHS, lr_actor=3e-3)
        table, bar = torch.stack(ref["kl"]), 1e-5 * torch.stack(ref["klmag"])
        _CACHE.update(Wa=Wa, Wc=Wc, data=data, ref=ref, table=table, bar=bar, pick=GR.pick_tau(table, bar))
    return _CACHE


def run_learner(torch, w, windows=1, **kw):
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    actor, critic = TG.make_mlp(w["Wa"], 2), TG.make_mlp(w["Wc"], 0)
    learner = PPOLearner(actor, critic, 0.97, **{**KW, **kw})
    st = TG.storage_of(*[t.to(DEV).contiguous() for t in w["data"]])
    outs = []
    for _ in range(windows):
        out = learner.train(st)
        torch.cuda.synchronize()
        outs.append({k: v.clone() for k, v in out.items()})
    return actor, critic, learner, outs[0] if windows == 1 else outs


def moments(torch, learner, mlp):
    return agent_slices(torch, learner.actor_opt.m1, mlp) + agent_slices(torch, learner.actor_opt.m2, mlp)


# 6 --------------------------------------------------------------------------------------------------------------------
def test_stop_epochs_match_the_float64_restatement(torch):
    w = window(torch)
    assert w["pick"] is not None, "no threshold with a wide enough gap: change the inputs, never the margin"
    tau, stops, gap = w["pick"]
    print("tau", tau, "stops", stops, "smallest gap", gap, "bars")
    assert len(set(stops)) >= 3 and EPOCHS in stops and any(0 < s < EPOCHS for s in stops), stops
    actor, critic, learner, out = run_learner(torch, w, target_kl=tau)
    assert out["actor_steps"].dtype == torch.int32 and out["actor_steps"].cpu().tolist() == stops
    assert torch.equal(learner.actor_opt.steps, out["actor_steps"])
    assert learner.critic_opt.steps.cpu().tolist() == [EPOCHS] * 6        # the critic is never gated
    kl = out["kl"].double().cpu()
    for i, s in enumerate(stops):
        for ep in range(EPOCHS):
            computed, crossing = ep <= s, ep == s
            for k in ACTOR_KEYS:
                assert bool(torch.isfinite(out[k][ep, i])) == computed, (k, ep, i)
            assert bool(torch.isfinite(out["actor_grad_norm"][ep, i])) == (computed and not crossing), (ep, i)
            if computed:
                err, bar = abs(float(kl[ep, i] - w["table"][ep, i])), float(w["bar"][ep, i])
                print("agent", i, "epoch", ep, "kl", float(kl[ep, i]), "ref", float(w["table"][ep, i]), "err / bar", err / bar)
                assert err <= bar, (ep, i, err, bar)
    for k in ("critic_loss", "critic_grad_norm"):
        assert bool(torch.isfinite(out[k]).all()), k
    assert float(out["kl"][0].abs().max()) == 0.0


# 7 --------------------------------------------------------------------------------------------------------------------
def test_a_stopped_agent_is_bitwise_the_ungated_learner_with_that_many_epochs(torch):
    w = window(torch)
    tau, stops, _ = w["pick"]
    actor, critic, learner, out = run_learner(torch, w, target_kl=tau)
    steps = out["actor_steps"].cpu().tolist()
    mom = moments(torch, learner, actor)
    for s in sorted(set(steps)):
        who = torch.tensor([i for i, v in enumerate(steps) if v == s], device=DEV)
        if s == 0:
            for n, w0 in zip(NAMES, w["Wa"]):
                assert torch.equal(getattr(actor, n)[who], w0.to(DEV)[who]), n
            continue
        actor2, critic2, learner2, _ = run_learner(torch, w, epochs=s)
        for n in NAMES:
            assert torch.equal(getattr(actor, n)[who], getattr(actor2, n)[who]), (s, n)
        for j, (a, b) in enumerate(zip(mom, moments(torch, learner2, actor2))):
            assert torch.equal(a[who], b[who]), (s, j)


# 8 --------------------------------------------------------------------------------------------------------------------
def test_a_threshold_nobody_reaches_is_the_plain_learner(torch):
    w = window(torch)
    a1, c1, l1, o1 = run_learner(torch, w, target_kl=1e30)
    a2, c2, l2, o2 = run_learner(torch, w)
    assert o1["actor_steps"].cpu().tolist() == [EPOCHS] * 6
    for n in NAMES:
        assert torch.equal(getattr(a1, n), getattr(a2, n)) and torch.equal(getattr(c1, n), getattr(c2, n)), n
    for x1, x2 in ((l1.actor_opt, l2.actor_opt), (l1.critic_opt, l2.critic_opt)):
        assert torch.equal(x1.m1, x2.m1) and torch.equal(x1.m2, x2.m2) and torch.equal(x1.steps, x2.steps)
    assert set(o2) <= set(o1) and set(o1) - set(o2) == {"kl", "entropy", "actor_steps"}
    for k in o2:
        assert torch.equal(o1[k], o2[k]), k
    assert bool(torch.isfinite(o1["kl"]).all()) and bool((o1["kl"] >= 0).all())


# 9 --------------------------------------------------------------------------------------------------------------------
def test_a_threshold_everybody_passes_stops_after_one_step(torch):
    w = window(torch)
    actor, critic, learner, out = run_learner(torch, w, target_kl=1e-30)
    assert out["actor_steps"].cpu().tolist() == [1] * 6 and learner.actor_opt.steps.cpu().tolist() == [1] * 6
    assert float(out["kl"][0].abs().max()) == 0.0 and float(out["kl"][1].min()) > 0
    assert bool(torch.isnan(out["kl"][2:]).all()) and bool(torch.isnan(out["actor_grad_norm"][1:]).all())
    assert bool(torch.isfinite(out["actor_loss"][:2]).all()) and bool(torch.isnan(out["actor_loss"][2:]).all())
    _, _, l1, _ = run_learner(torch, w, epochs=1)
    a1 = l1.actor
    for n in NAMES:
        assert torch.equal(getattr(actor, n), getattr(a1, n)), n
    assert learner.critic_opt.steps.cpu().tolist() == [EPOCHS] * 6


# 10 -------------------------------------------------------------------------------------------------------------------
def test_the_gate_resets_for_the_next_window(torch):
    w = window(torch)
    tau, stops, _ = w["pick"]
    actor, critic, learner, (o1, o2) = run_learner(torch, w, windows=2, target_kl=tau)
    s1, s2 = o1["actor_steps"].cpu(), o2["actor_steps"].cpu()
    print("window 1", s1.tolist(), "window 2", s2.tolist())
    assert s1.tolist() == stops and min(stops) < EPOCHS
    assert int(s2.min()) >= 1                                           # every agent trains again: the first step's KL is exactly 0
    assert float(o2["kl"][0].abs().max()) == 0.0
    assert torch.equal(learner.actor_opt.steps.cpu(), s1 + s2)
    assert learner.critic_opt.steps.cpu().tolist() == [2 * EPOCHS] * 6
    assert bool(torch.isfinite(o2["kl"][1]).all())


# 11 -------------------------------------------------------------------------------------------------------------------
def compare_guarded_steps(torch, out, ref, epochs, K, M, what, skip_actor_loss=()):
    """The per-step part of `compare_guarded_with_float64`: `test_gpu_minibatch.compare_with_float64`'s assertions and bars on the
    steps the restatement computed; the steps it skipped are NaN.  ``out`` entries ``[epochs, K, N]``.  ``skip_actor_loss``: the steps
    (``ep K + b``) whose ``actor_loss`` the caller compares itself."""
    for ep in range(epochs):
        for b in range(K):
            j = ep * K + b
            a, (computed, stepped) = ref["actor"][j], ref["active"][j]
            on = computed.nonzero().flatten()
            count = torch.round(out["clip_fraction"][ep, b].double().cpu() * M).long()
            near = a["near"].sum(0)
            print(what, "step", j, "computed", computed.int().tolist(), "clipped", count.tolist(), "ref", a["clipped"].sum(0).tolist(),
                  "near", near.tolist())
            assert torch.all(((count - a["clipped"].sum(0)).abs() <= near)[on]), (j, count, a["clipped"].sum(0), near)
            cl, cn = out["critic_loss"][ep, b].cpu().numpy(), out["critic_grad_norm"][ep, b].cpu().numpy()
            np.testing.assert_allclose(cl, ref["critic_loss"][j].numpy(), rtol=1e-5)
            np.testing.assert_allclose(cn, ref["critic_norm"][j].numpy(), rtol=1e-5)
            got = out["actor_grad_norm"][ep, b].cpu()
            s = stepped.nonzero().flatten()
            np.testing.assert_allclose(got[s].numpy(), ref["actor_norm"][j][s].numpy(), rtol=1e-5)
            assert bool(torch.isnan(got[~stepped]).all()), j
            if j not in skip_actor_loss:
                aref = a["loss"].numpy()
                al = out["actor_loss"][ep, b].cpu()
                np.testing.assert_allclose(al[on].numpy(), aref[on.numpy()], rtol=1e-4, atol=1e-4 * np.abs(aref).max())
            for k in ACTOR_KEYS:
                if k in out:
                    assert bool(torch.isfinite(out[k][ep, b].cpu()[on]).all()) and bool(torch.isnan(out[k][ep, b].cpu()[~computed]).all()), (k, j)
            if "kl" in out:
                err = (out["kl"][ep, b].double().cpu() - ref["kl"][j]).abs()[on]
                assert torch.all(err <= 1e-5 * ref["klmag"][j][on]), (j, err)
            if "vf_clip_fraction" in out:
                c = ref["critic"][j]
                vcount = torch.round(out["vf_clip_fraction"][ep, b].double().cpu() * M).long()
                print(what, "step", j, "value rows clipped", vcount.tolist(), "ref", c["zero"].sum(0).tolist(), "near", c["near"].sum(0).tolist())
                assert torch.all((vcount - c["zero"].sum(0)).abs() <= c["near"].sum(0)), (j, vcount, c["zero"].sum(0))


def compare_guarded_weights(torch, mlp, lr, post, m2, n_steps, what=""):
    """The weight part of `compare_guarded_with_float64`: the sharp / loose split on sqrt(m2), times the steps ``n_steps`` [N] each
    agent took."""
    for name, p, v in zip(NAMES, post, m2):
        got = getattr(mlp, name).double().cpu()
        sharp = v.sqrt() > 1e-3 * float(v.sqrt().max())
        tol = torch.where(sharp, torch.full_like(p, 1e-6 + 1e-3 * lr), torch.full_like(p, 2 * lr))
        tol = tol * n_steps.double().view(-1, *([1] * (v.dim() - 1)))
        assert torch.all((got - p).abs() <= tol), (what, name, float(((got - p).abs() - tol).max()))


def compare_guarded_with_float64(torch, learner, actor, critic, out, ref, epochs, K, M, what):
    """One call from fresh optimisers: `compare_guarded_steps`, the two step counters, `compare_guarded_weights`."""
    N = actor.n_agents
    steps = epochs * K
    taken = ref["actor_steps"]
    compare_guarded_steps(torch, out, ref, epochs, K, M, what)
    assert learner.critic_opt.steps.cpu().tolist() == [steps] * N and learner.actor_opt.steps.cpu().tolist() == taken.tolist()
    compare_guarded_weights(torch, critic, learner.critic_opt.lr, ref["critic_post"], ref["cm2"], torch.full((N,), steps))
    compare_guarded_weights(torch, actor, learner.actor_opt.lr, ref["actor_post"], ref["am2"], taken)


def test_minibatches_with_both_guards_and_the_other_options_match_float64(torch):
    """`test_gpu_ppo.storage_setup` (T E = 384 rows, N = 16, softmax-16): K = 4, M = 96, two epochs, with target_kl, vf_clip,
    ent_coef, normalize_advantage and lam.  The threshold comes from the restatement's ungated per-minibatch table."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    epochs, K, seed, vf = 2, 4, 2 ** 40 + 3, 0.01
    env, actor, critic, st, _ = TP.storage_setup(torch)
    T, E, N = TP.T_RS, TP.E_RS, TP.N_RS
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    Wa, Wc = TM.weights_of(actor), TM.weights_of(critic)
    z_all, reward, done, act, nbr = [t.cpu().clone() for t in (st.z_all, st.reward, st.done, st.actions, st.nbr_pre)]
    kw = dict(epochs=epochs, minibatches=K, shuffle_seed=seed, lr_actor=3e-3, ent_coef=0.01, normalize_advantage=True, lam=0.95, vf_clip=vf)
    rkw = dict(kw, x_all=z_all)
    free = GR.ppo_train(1, Wa, Wc, None, reward, done, act, nbr, 0.99, **rkw)
    table, bar = torch.stack(free["kl"]), 1e-5 * torch.stack(free["klmag"])
    pick = GR.pick_tau(table, bar)
    assert pick is not None
    tau, stops, gap = pick
    print("tau", tau, "stops", stops, "gap", gap)
    assert len(set(stops)) >= 2 and min(stops) < epochs * K
    ref = GR.ppo_train(1, Wa, Wc, None, reward, done, act, nbr, 0.99, target_kl=tau, **rkw)
    assert ref["actor_steps"].tolist() == stops
    learner = PPOLearner(actor, critic, 0.99, target_kl=tau, **kw)
    out = learner.train(st)
    torch.cuda.synchronize()
    assert np.array_equal(learner.perm.cpu().numpy(), ref["perms"][-1])
    assert len(learner._mb) == 6 and torch.equal(torch.stack(learner._mb[5].blocks).reshape(T * E, N),
                                                 learner.V.reshape(T * E, N)[learner.perm.long()])
    for k in ACTOR_KEYS + ("critic_loss", "critic_grad_norm", "actor_grad_norm", "vf_clip_fraction"):
        assert out[k].shape == (epochs, K, N), k
    assert out["actor_steps"].cpu().tolist() == stops
    assert float(out["vf_clip_fraction"][0, 0].abs().max()) == 0.0       # the first step sees V == v_old
    amax = lambda t: float(t.abs().max())
    np.testing.assert_allclose(learner.G.cpu().numpy(), ref["G"].numpy(), rtol=1e-5, atol=1e-5 * amax(ref["G"]))
    np.testing.assert_allclose(learner.adv.cpu().numpy(), ref["adv"].numpy(), rtol=1e-4, atol=1e-4 * amax(ref["adv"]))
    compare_guarded_with_float64(torch, learner, actor, critic, out, ref, epochs, K, T * E // K, "guards")


# 12 -------------------------------------------------------------------------------------------------------------------
def test_whole_window_epochs_with_the_clipped_value_loss_match_float64(torch):
    """`test_four_epochs_on_a_rollout_storage_match_float64`'s set-up and bars with ``vf_clip`` alone; eps is taken from the
    restatement so that its last epoch has 5-50 % of the rows on the zero-gradient branch."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    epochs = 4
    env, actor, critic, st, _ = TP.storage_setup(torch)
    T, E, N = TP.T_RS, TP.E_RS, TP.N_RS
    rows = T * E
    TG.rollout_window(env, actor, st)
    torch.cuda.synchronize()
    Wa, Wc = TM.weights_of(actor), TM.weights_of(critic)
    data = [t.cpu().clone() for t in (st.z_pre, st.reward, st.done, st.actions, st.nbr_pre)]
    plain = GR.ppo_train(1, Wa, Wc, *data, 0.99, epochs=epochs - 1)
    from tests import lambda_ref as LR
    xr = data[0].reshape(rows, N, -1)
    moved = (LR.critic_values(plain["critic_post"], xr) - LR.critic_values(Wc, xr)).abs().flatten()
    ref = None
    for q in (0.7, 0.5, 0.8, 0.3, 0.9):
        eps = float(torch.quantile(moved, q))
        cand = GR.ppo_train(1, Wa, Wc, *data, 0.99, epochs=epochs, vf_clip=eps)
        share = float(cand["critic"][-1]["zero"].double().mean())
        print("quantile", q, "eps", eps, "last epoch's zero-gradient share", share)
        if 0.05 <= share <= 0.5:
            ref = cand
            break
    assert ref is not None, "no eps with 5-50 % of the last epoch's rows clipped"
    learner = PPOLearner(actor, critic, 0.99, epochs=epochs, vf_clip=eps)
    out = learner.train(st)
    torch.cuda.synchronize()
    assert set(out) == {"critic_loss", "actor_loss", "critic_grad_norm", "actor_grad_norm", "clip_fraction", "approx_kl", "ratio_min",
                        "ratio_max", "vf_clip_fraction"}
    assert float(out["vf_clip_fraction"][0].abs().max()) == 0.0
    view = {k: v.view(epochs, 1, N) for k, v in out.items()}
    compare_guarded_with_float64(torch, learner, actor, critic, view, ref, epochs, 1, rows, "vf_clip")


# 13 -------------------------------------------------------------------------------------------------------------------
def test_rollout_window_and_guarded_train_in_one_graph(torch):
    """A storage window and `PPOLearner(target_kl, vf_clip).train` captured in ONE graph: three replays equal the eager sequence
    bit for bit, `actor_steps`, the NaN positions and the counters included."""
    epochs = 3
    probe = TP.storage_setup(torch, epochs=epochs, target_kl=1e30, lr_actor=3e-3)
    TG.rollout_window(probe[0], probe[1], probe[3])
    second = probe[4].train(probe[3])["kl"][1]
    torch.cuda.synchronize()
    tau = float(second.median())                                         # about half the agents cross on their second step
    kw = dict(epochs=epochs, target_kl=tau, vf_clip=0.01, lr_actor=3e-3)
    env, actor, critic, st, learner = TP.storage_setup(torch, **kw)

    def window_(env, actor, st, learner):
        TG.rollout_window(env, actor, st)
        return learner.train(st)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = window_(env, actor, st, learner)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    first_steps = out["actor_steps"].clone()
    assert int(first_steps.min()) < epochs and int(first_steps.max()) >= 2, first_steps
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = window_(env, actor, st, learner)
    env2, actor2, critic2, st2, learner2 = TP.storage_setup(torch, **kw)
    keys = sorted(out)
    snap = lambda a, c, l, s_, o: [t.clone() for t in [getattr(m, n) for m in (a, c) for n in NAMES] +
                                   [l.actor_opt.m1, l.actor_opt.m2, l.critic_opt.m1, l.critic_opt.m2, l.actor_opt.steps,
                                    l.critic_opt.steps, l.active, s_.z_pre, l.logp_old, l.adv] + [o[k] for k in keys]]
    ref = []
    for _ in range(4):
        o2 = window_(env2, actor2, st2, learner2)
        ref.append(snap(actor2, critic2, learner2, st2, o2))
    torch.cuda.synchronize()
    assert torch.equal(ref[0][keys.index("actor_steps") - len(keys)], first_steps)
    for rep in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        got = snap(actor, critic, learner, st, out)
        for j, (a, b) in enumerate(zip(got, ref[rep])):
            assert same_bits(torch, a, b), (rep, j)
        assert int(learner.critic_opt.steps.min()) == int(learner.critic_opt.steps.max()) == epochs * (rep + 1)
    nan = sum(int(torch.isnan(o[keys.index("actor_grad_norm") - len(keys)]).sum()) for o in ref)
    assert nan > 0                                                      # the replays did meet gated steps


# 14 -------------------------------------------------------------------------------------------------------------------
def test_one_guarded_train_at_c3_size(torch):
    """`test_gpu_ppo.test_one_train_at_c3_size` with both guards on, under its time limit; everything not skipped is finite."""
    from scalable_collision_avoidance_rl_amd.learner import PPOLearner
    N, E, T, d_in, epochs = 64, 4096, 200, 6, 2
    limit = 2 * (epochs + 1) * TP.SA2C_SECONDS
    gen = torch.Generator(device=DEV).manual_seed(1)
    cpu = torch.Generator().manual_seed(1)
    actor = TG.make_mlp(TG.random_net(torch, cpu, N, d_in, 300, 300, 16), 1)
    critic = TG.make_mlp(TG.random_net(torch, cpu, N, d_in, 200, 200, 1), 0)
    x = (torch.rand(T, E, N, d_in, device=DEV, generator=gen) * 2 - 1) * 3
    reward = torch.randn(T, E, N, device=DEV, generator=gen)
    done = torch.zeros(T, E, dtype=torch.uint8, device=DEV)
    done[-1] = 1; done[99, ::3] = 1
    a = torch.randint(0, 16, (T, E, N), device=DEV, generator=gen).float() * (2 * math.pi / 16)
    act = torch.stack([a.cos(), a.sin()], -1)
    nbr = torch.stack([torch.arange(N, device=DEV).expand(T, E, N), torch.randint(0, N, (T, E, N), device=DEV, generator=gen),
                       torch.randint(-1, N, (T, E, N), device=DEV, generator=gen)], -1).int()
    learner = PPOLearner(actor, critic, 0.99, epochs=epochs, target_kl=0.02, vf_clip=0.2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = learner.train(TG.storage_of(x, reward, done, act, nbr))
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    print(f"C3 PPO train with both guards, {epochs} epochs: {seconds:.2f} s (limit {limit:.2f} s); actor steps "
          f"{int(out['actor_steps'].min())}..{int(out['actor_steps'].max())}")
    assert seconds <= limit, (seconds, limit)
    steps = out["actor_steps"]
    assert int(steps.min()) >= 1 and int(steps.max()) <= epochs
    for k, v in out.items():
        if k == "actor_steps":
            continue
        assert v.shape == (epochs, N), k
        if k == "actor_grad_norm":                                     # the crossing step discards its gradient: NaN there only
            assert torch.isfinite(v[0]).all() and torch.equal(torch.isfinite(v[1]), steps == 2), k
        else:
            assert torch.isfinite(v).all(), k                          # two epochs: a crossing step is computed, nothing is skipped
    assert float(out["kl"][0].abs().max()) == 0.0 and float(out["kl"][1].min()) > 0
    assert float(out["vf_clip_fraction"][0].max()) == 0.0 and 0.0 <= float(out["vf_clip_fraction"][1].min())
    for mlp in (actor, critic):
        assert all(torch.isfinite(getattr(mlp, n)).all() for n in NAMES)
