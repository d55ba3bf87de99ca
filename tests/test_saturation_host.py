"""Host checks of tests/saturation_ref.py (no GPU): the regimes are what they claim, the float64 cancellation-free restatement
of the heads agrees with 50-digit mpmath and -- where autograd can be trusted -- with the existing references, and the sharp
bar has the power the GPU tests rely on: a float32 restatement of the heads as csrc/learner.hip stood before (lse = max +
log(sum), onehot - p, 1 - mu mu) FAILS it at saturated policies, the repaired expressions pass it in every regime."""

import pytest
import torch

from tests import entropy_ref as ER
from tests import learner_ref as R
from tests import ppo_ref as P
from tests import saturation_ref as S

KINDS = [1, 2]
KIND_IDS = ["softmax", "gaussian"]


def agents(c, idx):
    """The case's inputs as rows, restricted to the agents `idx`: (W, x, act, adv, logp_old)."""
    x, act, adv, old = S.rows_of(c)
    return [w[idx] for w in c["W"]], x[:, idx], act[:, idx], adv[:, idx], old[:, idx]


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_the_regimes_are_what_they_claim(kind):
    """From the float64 forward: every agent's realised gap / centres are the regime's up to the spread of the small net's own
    outputs; the window is five chunks with a tail of 3; both action sets keep `draw_logp_old`'s redrawn share within 1 %; the
    collapsed set takes the dominant action on every row, the mixed set another one on about 10 % of them."""
    assert S.ROWS == 259 and S.ROWS // S.ROWS_PER_CHUNK == 4 and S.ROWS % S.ROWS_PER_CHUNK == 3
    c = S.case(kind, "collapsed")
    N = len(c["regimes"])
    x, act, adv, old = S.rows_of(c)
    O = R.forward([w.double() for w in c["W"]], x.double())[2]
    small = c["small"]
    spread = (small.max(-1).values - small.min(-1).values).amax(1)            # [N]
    assert float(spread.max()) < 4.0
    for i, regime in enumerate(c["regimes"]):
        name = S.regime_name(kind, regime)
        if kind == 1:
            a = S.dominant(i)
            rest = torch.cat([O[i, :, :a], O[i, :, a + 1:]], -1)
            gap = O[i, :, a] - rest.max(-1).values
            print(name, "realised gap", float(gap.min()), float(gap.max()), "offset", float(rest.mean()))
            assert float((gap - regime[0]).abs().max()) <= float(spread[i]) + 1e-4, name
            assert float((rest - regime[1]).abs().max()) <= float(small[i].abs().max()) + 1e-4, name
            if regime[0] >= 12:
                assert float(torch.softmax(O[i], -1)[:, a].min()) > 0.999, name
            assert torch.all(R.action_index(act[:, i], 16) == a), name
        else:
            sign = torch.tensor(S.MU_SIGNS[i % 4], dtype=torch.float64)
            centre, vc = O[i, :, :2] * sign, O[i, :, 2:]
            print(name, "realised tanh centre", float(centre.min()), float(centre.max()), "variance centre", float(vc.min()), float(vc.max()))
            bound = float(small[i].abs().max()) + 1e-4
            assert float((centre - regime[0]).abs().max()) <= bound and float((vc - regime[1]).abs().max()) <= bound, name
    assert {s for s in S.MU_SIGNS} == {(1.0, -1.0), (-1.0, 1.0), (1.0, 1.0), (-1.0, -1.0)}
    assert float(adv.min()) < -1 and float(adv.max()) > 1
    for actions in S.ACTIONS:
        c = S.case(kind, actions)
        ref = S.form_reference(c, "ppo")
        print(kind, actions, "redrawn", c["redrawn"], "largest margin", float(c["margin"].max()), "clipped share",
              float(ref["clipped"].double().mean()), "r in", float(ref["r"].min()), float(ref["r"].max()))
        assert c["redrawn"] <= 0.01, (actions, c["redrawn"])
        assert not P.ratio_terms(ref["lp"], S.rows_of(c)[3], S.rows_of(c)[2], S.CLIP_EPS, c["margin"])[2].any()
        assert 0.1 < float(ref["clipped"].double().mean()) < 0.5
        share = float(c["other"].double().mean())
        assert (share == 0.0) if actions == "collapsed" else (0.07 < share < 0.13)
    if kind == 1:
        c = S.case(1, "mixed")
        idx = R.action_index(S.rows_of(c)[1], 16)
        dom = torch.tensor([S.dominant(i) for i in range(N)])
        assert torch.equal(idx != dom, c["other"])


# 2 --------------------------------------------------------------------------------------------------------------------
def mp_head(kind, o, a_idx, a, A, old, scale, es, clip_eps):
    """One row of the entropy PPO head and the A2C entropy head (weight = A) straight from the definitions -- log of the sum,
    onehot - p, 1 - mu^2, 1 - var --, good to 50 digits: the working precision is 50 digits more than the worst cancellation of
    these regimes loses (1 - p_a at a gap of 120 is 1e-52).  Returns dict(lp, H, r, k, ppo_dO, ppo_loss, a2c_dO, a2c_loss)."""
    import mpmath as mp
    mp.mp.dps = 50 + 60
    o = [mp.mpf(float(v)) for v in o]
    if kind == 1:
        lse = mp.log(mp.fsum(mp.exp(v) for v in o))
        lq = [v - lse for v in o]
        p = [mp.exp(v) for v in lq]
        lp = lq[a_idx]
        H = -mp.fsum(pj * lj for pj, lj in zip(p, lq))
        dlp = [(1 if j == a_idx else 0) - p[j] for j in range(len(o))]
        dH = [-p[j] * (lq[j] + H) for j in range(len(o))]
    else:
        mu = [mp.tanh(o[d]) for d in range(2)]
        var = [1 / (1 + mp.exp(-o[2 + d])) for d in range(2)]
        diff = [mp.mpf(float(a[d])) - mu[d] for d in range(2)]
        lp = mp.fsum(-mp.log(2 * mp.pi * var[d]) / 2 - diff[d] ** 2 / (2 * var[d]) for d in range(2))
        H = mp.fsum(mp.log(2 * mp.pi * mp.e * var[d]) / 2 for d in range(2))
        dlp = [diff[d] / var[d] * (1 - mu[d] ** 2) for d in range(2)] + \
              [(-mp.mpf(1) / 2 + diff[d] ** 2 / (2 * var[d])) * (1 - var[d]) for d in range(2)]
        dH = [mp.mpf(0), mp.mpf(0)] + [(1 - var[d]) / 2 for d in range(2)]
    A, old, es = mp.mpf(float(A)), mp.mpf(float(old)), mp.mpf(es)
    dl = lp - old
    r = mp.exp(dl)
    lo, hi = 1 - mp.mpf(clip_eps), 1 + mp.mpf(clip_eps)
    clipped = (A > 0 and r > hi) or (A < 0 and r < lo)
    c = 0 if clipped else -mp.mpf(scale["ppo"]) * A * r
    ppo_loss = -mp.mpf(scale["ppo"]) * min(r * A, min(max(r, lo), hi) * A) - es * H
    c2 = -mp.mpf(scale["a2c"]) * A
    return dict(lp=lp, H=H, r=r, k=mp.expm1(dl) - dl, ppo_dO=[c * g - es * e for g, e in zip(dlp, dH)], ppo_loss=ppo_loss,
                a2c_dO=[c2 * g - es * e for g, e in zip(dlp, dH)], a2c_loss=c2 * lp - es * H, clipped=clipped)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_float64_restatement_against_mpmath(kind):
    """Four rows per regime (two that took the dominant action, two that took another) of the mixed set: dO, the per-row loss,
    lp, H, r and k of the entropy forms of both heads against the definitions evaluated at 50 digits, to 1e-12 of the sharp
    scale (i.e. 1e-7 of the bar)."""
    import mpmath
    c = S.case(kind, "mixed")
    x, act, adv, old = S.rows_of(c)
    ppo, a2c = S.form_reference(c, "ppo_ent"), S.form_reference(c, "a2c_ent")
    O = ppo["O"]
    idx = R.action_index(act, O.shape[-1])
    worst = 0.0
    for i, regime in enumerate(c["regimes"]):
        other = c["other"][:, i].nonzero().flatten().tolist()
        same = (~c["other"][:, i]).nonzero().flatten().tolist()
        for m in same[:1] + same[-1:] + other[:1] + other[-1:]:
            mp = mp_head(kind, O[i, m].tolist(), int(idx[m, i]), act[m, i].tolist(), float(adv[m, i]), float(old[m, i]),
                         dict(ppo=1.0 / S.ROWS, a2c=1.0 / S.E), S.ENT_SCALE, S.CLIP_EPS)
            assert bool(ppo["clipped"][m, i]) == mp["clipped"]
            pairs = [(ppo["lp"][m, i], mp["lp"], ppo["lp_scale"][m, i]), (ppo["H"][m, i], mp["H"], ppo["H_scale"][m, i]),
                     (ppo["r"][m, i], mp["r"], ppo["r_scale"][m, i]), (ppo["k"][m, i], mp["k"], ppo["k_scale"][m, i]),
                     (ppo["loss_rows"][m, i], mp["ppo_loss"], ppo["loss_rows_scale"][m, i]),
                     (a2c["loss_rows"][m, i], mp["a2c_loss"], a2c["loss_rows_scale"][m, i])]
            pairs += [(ppo["dO"][i, m, j], mp["ppo_dO"][j], ppo["dOa"][i, m, j]) for j in range(O.shape[-1])]
            pairs += [(a2c["dO"][i, m, j], mp["a2c_dO"][j], a2c["dOa"][i, m, j]) for j in range(O.shape[-1])]
            for n, (got, want, scale) in enumerate(pairs):
                err = abs(mpmath.mpf(float(got)) - want)
                bar = mpmath.mpf(1e-12) * mpmath.mpf(float(scale)) + mpmath.mpf(1e-300)
                worst = max(worst, float(err / bar))
                assert err <= bar, (S.regime_name(kind, regime), m, n, float(got), float(want), float(scale))
    print(kind, "worst error / (1e-12 x sharp scale)", worst)


# 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("actions", S.ACTIONS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_moderate_regimes_match_the_autograd_references(kind, actions):
    """Gap <= 8 and tanh centre <= 3: float64 autograd is trustworthy there, and `learner_ref.grads`, `entropy_ref.a2c_grads`,
    `ppo_ref.actor_grads` and `entropy_ref.actor_grads` agree with the restatement at the existing bar, 1e-5 x `magnitude_grads`
    (between two float64 computations the difference is far below it)."""
    c = S.case(kind, actions)
    idx = [i for i, r in enumerate(c["regimes"]) if (r[0] <= 8 and r[1] == 0 if kind == 1 else r[0] <= 3)]
    assert len(idx) == (2 if kind == 1 else 6)
    W, x, act, adv, old = agents(c, idx)
    es = S.ENT_SCALE
    g, l = R.grads(kind, W, x, 1.0 / S.E, act=act, weight=adv)
    mag = R.magnitude_grads(kind, W, x, 1.0 / S.E, act=act, weight=adv)
    ours = S.reference(kind, W, x, act, "a2c", 1.0 / S.E, weight=adv)
    e = ER.a2c_grads(kind, W, x, 1.0 / S.E, act, adv, es)
    ours_e = S.a2c_grads(kind, W, x, 1.0 / S.E, act, adv, es)
    p = P.actor_grads(kind, W, x, act, old, adv, S.CLIP_EPS)
    ours_p = S.actor_grads(kind, W, x, act, old, adv, S.CLIP_EPS)
    pe = ER.actor_grads(kind, W, x, act, old, adv, S.CLIP_EPS, es)
    ours_pe = S.actor_grads(kind, W, x, act, old, adv, S.CLIP_EPS, es)
    for what, got, want, m in (("a2c", ours["grad"], g, mag), ("a2c_ent", ours_e["grad"], e["grad"], e["mag"]),
                               ("ppo", ours_p["grad"], p["grad"], p["mag"]), ("ppo_ent", ours_pe["grad"], pe["grad"], pe["mag"])):
        w = float(S.worst_per_agent(got, want, m).max())
        print(kind, actions, what, "worst / existing bar", w)
        assert w <= 1.0, what
    close = lambda a, b: torch.allclose(a, b, rtol=1e-10, atol=1e-12)
    assert close(ours["loss"], l) and close(ours_e["loss"], e["loss"]) and close(ours_e["entropy"], e["entropy"])
    assert close(ours_e["likelihood_loss"], e["likelihood_loss"]) and close(ours_e["entropy_loss"], e["entropy_loss"])
    for k in ("loss", "r", "clip_fraction", "approx_kl", "ratio_min", "ratio_max"):
        assert close(ours_p[k], p[k]), k
    assert torch.equal(ours_p["clipped"], p["clipped"]) and close(ours_p["logp"], p["logp"])
    assert close(ours_pe["loss"], pe["loss"]) and close(ours_pe["entropy"], pe["entropy"])
    assert close(S.logp(kind, W, x, act), P.logp(kind, W, x, act))
    sharp = S.sharp_magnitude_grads(kind, W, x, 1.0 / S.E, act, adv)
    assert all(torch.equal(s, m) for s, m in zip(sharp, ours["mag"]))


# 4 --------------------------------------------------------------------------------------------------------------------
def float32_ratios(c, form, variant):
    """Worst error / bar per agent of a float32 restatement of one form: dict(grad, loss, entropy, lp[, r])."""
    x, act, adv, old = S.rows_of(c)
    ref = S.form_reference(c, form)
    base = "a2c" if form.startswith("a2c") else "ppo"
    es = S.ENT_SCALE if form.endswith("ent") else 0.0
    kw = dict(weight=adv) if base == "a2c" else dict(logp_old=old, adv=adv)
    g, h = S.float32_grads(c["kind"], c["W"], x, act, base, 1.0 / S.E if base == "a2c" else 1.0 / S.ROWS, variant, es=es, **kw)
    out = dict(grad=S.worst_per_agent(g, ref["grad"], ref["mag"]), loss=S.ratios(h["loss"].sum(1), ref["loss"], ref["loss_scale"]),
               entropy=S.ratios(h["H"].mean(1), ref["entropy"], ref["entropy_scale"]),
               lp=S.ratios(h["lp"].transpose(0, 1), ref["lp"], ref["lp_scale"]).amax(0))
    if base == "ppo":
        assert torch.equal(h["clipped"].transpose(0, 1), ref["clipped"]), (form, variant)
        out["r"] = S.ratios(h["r"].transpose(0, 1), ref["r"], ref["r_scale"]).amax(0)
    assert all(bool(torch.isfinite(v).all()) for v in out.values()), (form, variant)
    return out


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_the_sharp_bar_fails_the_old_expressions_and_passes_the_repaired_ones(kind):
    """On the collapsed set the float32 restatement of the heads' OLD expressions misses 1e-5 x the sharp scale at softmax gaps
    16, 20 and 30 and at tanh centres >= 7 with variance centres 0 and 10, and meets it at gap 0 and centre 0; the repaired
    expressions meet it in every regime, form and action set -- gradients, per-agent loss, mean entropy, lp and ratio."""
    c = S.case(kind, "collapsed")
    names = [S.regime_name(kind, r) for r in c["regimes"]]
    old = float32_ratios(c, "a2c", "parent")
    new = float32_ratios(c, "a2c", "free")
    for i, (name, regime) in enumerate(zip(names, c["regimes"])):
        print(f"{name:12s} a2c gradients, worst error / bar: old expressions {float(old['grad'][i]):9.3g}   repaired {float(new['grad'][i]):9.3g}"
              f"   loss: old {float(old['loss'][i]):9.3g}   repaired {float(new['loss'][i]):9.3g}")
        must_fail = (regime[0] in (16, 20, 30)) if kind == 1 else (regime[0] >= 7 and regime[1] in (0, 10))
        if must_fail:
            assert float(old["grad"][i]) > 1.0, name
        if regime[0] == 0:
            assert float(old["grad"][i]) <= 1.0 and float(old["loss"][i]) <= 1.0, name
    for actions in S.ACTIONS:
        c = S.case(kind, actions)
        for form in ("a2c", "a2c_ent", "ppo", "ppo_ent"):
            parent, got = float32_ratios(c, form, "parent"), float32_ratios(c, form, "free")
            print(actions, form, "repaired, worst per regime:", {n: f"{float(v):.2g}" for n, v in zip(names, got["grad"])})
            print(actions, form, "old expressions:          ", {n: f"{float(v):.2g}" for n, v in zip(names, parent["grad"])})
            for what, v in got.items():
                assert float(v.max()) <= 1.0, (actions, form, what, names[int(v.argmax())], float(v.max()))
