"""The learner's loss heads at SATURATED policies: seeded regimes, a float64 restatement of the heads written without
cancellation, the sharp error scale that goes with it, and two float32 restatements of the head expressions (test
infrastructure of tests/test_saturation_host.py and tests/test_gpu_saturation.py; CPU or GPU tensors).  Built on
tests/learner_ref.py, tests/ppo_ref.py and tests/entropy_ref.py, same layouts: weights stacked [N, ...], rows x [R, N, d_in].

Why another restatement.  A softmax actor that has trained for a while has p_max = 0.999..., a Gaussian actor's mean sits
against tanh's +-1, and there the heads' gradients are small: `learner_ref.magnitude_grads` scales the softmax head by
onehot + p and the Gaussian mean column by 1 + mu^2, i.e. it takes the cancellations in (j == a) - p and 1 - mu mu as
inherent.  They are not:

  1 - p_a        is the sum of the other probabilities
  log p_j        is (o_j - max) - log1p(sum of the non-max exponentials): nothing of the size of the maximum is added back
  1 - tanh^2(o)  is 4 t / (1 + t)^2 with t = exp(-2 |o|)
  1 - sigmoid(s) is sigmoid(-s)

`head` states the heads with these forms (``variant="free"``), in the arithmetic of the outputs it is given: float64 is the
truth (checked against 50-digit mpmath in the host tests; float64 autograd is NOT the truth here, at a logit gap of 60
float64's own 1 - p_a is 0), float32 is the "repaired" restatement of csrc/learner.hip.  ``variant="parent"`` is the head as
csrc/learner.hip stood before these tests: lse = max + log(sum), p = exp(o - lse), onehot - p, 1 - mu mu, e / (1 + e).

The sharp scale.  `reference` returns, next to every value, the error scale a float32 head cannot be expected to beat: the
TRUE magnitudes of the head's terms (not onehot + p), each times cond = 1 + the magnitudes of the pre-activation outputs
that enter it -- the forward GEMM rounds an output o by eps x (its magnitude chain |H2| |W3| + |b3|), which moves exp(o_j - max) by
that much of itself.  In detail, with Oa the magnitude chain of the outputs:

  softmax    cond_j = 1 + Oa_j + Oa_max for a logit that is not the row's maximum; the maximum's own probability 1 / (1 + s)
             depends on the others only through s, cond_max = 1 + sum_{k != max} p_k cond_k.
             dlogp/dO:  p_j cond_j off the chosen logit, sum_{j != a} p_j cond_j on it;  entropy: p_j (|lq_j| + H) cond_j.
  Gaussian   cond_d = 1 + Oa_mu_d + Oa_s_d;  mean column (d / var)(1 - mu^2) cond with d = |a| + |mu| kept (a - mu on a
             float32 mu is inherent), variance column (0.5 + d^2 / (2 var)) omv cond; entropy 0.5 omv cond.
  log pi     softmax |lq_a| + (cond_a - 1) + the scale of log1p(s); Gaussian the terms' magnitudes, the logarithm's argument
             rounding (0.5 per dimension) and a - mu's rounding |a - mu| d / var.
  PPO        r = exp(lp - logp_old) carries the rounding of both log-probabilities: every factor r is scaled by
             rel = 1 + scale(lp) + |lp| + |logp_old|.

The bar of every comparison is the project's: |got - ref| <= 1e-5 x scale + 1e-30."""
import functools
import math

import torch

from tests import entropy_ref as ER
from tests import learner_ref as R
from tests import ppo_ref as P

D_IN, H1, H2 = 6, 48, 40
T, E, ROWS_PER_CHUNK = 37, 7, 64            # 259 rows: four whole chunks and a tail of 3
ROWS = T * E
CLIP_EPS = 0.2
ENT_SCALE = 0.01 / ROWS
OTHER_SHARE = 0.1                           # "mixed" actions: this share of the rows takes another action
BAR, FLOOR = 1e-5, 1e-30
EPS32 = 2.0 ** -24

# one agent per regime
SOFTMAX_REGIMES = [(gap, 0.0) for gap in (0, 8, 12, 16, 20, 30, 60, 120)] + [(16, 250.0)]     # (gap of the dominant logit, offset)
GAUSSIAN_REGIMES = [(m, v) for m in (0, 3, 5, 7, 9, 12, 20) for v in (-10, 0, 10)]            # (tanh centre, variance centre)
MU_SIGNS = ((1.0, -1.0), (-1.0, 1.0), (1.0, 1.0), (-1.0, -1.0))
ACTIONS = ("collapsed", "mixed")
FORMS = ("a2c", "a2c_ent", "ppo", "ppo_ent", "gated", "logp")


def regimes_of(kind):
    return SOFTMAX_REGIMES if kind == 1 else GAUSSIAN_REGIMES


def regime_name(kind, regime):
    return (f"gap{regime[0]}" + (f"+{regime[1]:g}" if regime[1] else "")) if kind == 1 else f"mu{regime[0]}var{regime[1]}"


def dominant(i, nout=16):
    return (3 * i + 1) % nout


# ----------------------------------------------------------------------------------------------------------------------
# the heads
def head(kind, O, act, form, scale, weight=None, logp_old=None, adv=None, es=0.0, clip_eps=CLIP_EPS, variant="free"):
    """The head of csrc/learner.hip on pre-activation outputs O [N, R, nout], in O's dtype.  act [R, N, 2]; weight (forms
    ``a2c``) or logp_old and adv (``ppo``) [R, N]; ``logp`` needs neither.  ``es`` is the entropy scale (0: the plain head's
    values).  Returns a dict of [N, R(, nout)] tensors: lp, H, and for the gradient forms dO, loss (per row), and for ``ppo``
    r, dl, clipped, k = expm1(dl) - dl; ``parts`` holds the intermediates `reference` builds the scale from."""
    assert form in ("a2c", "ppo", "logp") and variant in ("free", "parent")
    dt = O.dtype
    tr = lambda t: t.to(dt).transpose(0, 1)
    a = act.transpose(0, 1)
    if kind == 1:
        idx = R.action_index(a, O.shape[-1])[..., None]
        onehot = torch.zeros_like(O).scatter_(-1, idx, 1.0)
        mx, imax = O.max(-1, keepdim=True)
        notmax = torch.ones_like(O).scatter_(-1, imax, 0.0)
        if variant == "parent":
            lq = O - (mx + torch.log(torch.exp(O - mx).sum(-1, keepdim=True)))
            p = torch.exp(lq)
            dlp = onehot - p
        else:
            z = O - mx
            lq = z - torch.log1p((torch.exp(z) * notmax).sum(-1, keepdim=True))
            p = torch.exp(lq)
            dlp = onehot * (p * (1 - onehot)).sum(-1, keepdim=True) - (1 - onehot) * p
        lp = lq.gather(-1, idx)[..., 0]
        H = -(p * lq).sum(-1)
        dH = -p * (lq + H[..., None])
        parts = dict(onehot=onehot, notmax=notmax, imax=imax, p=p, lq=lq)
    else:
        om, s = O[..., :2], O[..., 2:]
        mu = torch.tanh(om)
        e = torch.exp(-s)
        var = 1 / (1 + e)
        if variant == "parent":
            omv, omm = e / (1 + e), 1 - mu * mu
        else:
            t = torch.exp(-2 * om.abs())
            omv, omm = 1 / (1 + torch.exp(s)), 4 * t / ((1 + t) * (1 + t))
        diff = a.to(dt) - mu
        lp = (-0.5 * torch.log(2 * math.pi * var) - diff * diff / (2 * var)).sum(-1)
        H = (0.5 * torch.log(2 * math.pi * math.e * var)).sum(-1)
        dlp = torch.cat([(diff / var) * omm, (-0.5 + diff * diff / (2 * var)) * omv], -1)
        dH = torch.cat([torch.zeros_like(omv), 0.5 * omv], -1)
        parts = dict(mu=mu, var=var, omv=omv, omm=omm, diff=diff, a=a.to(dt))
    out = dict(lp=lp, H=H, parts=parts, dlp=dlp, dH=dH)
    if form == "logp":
        return out
    if form == "a2c":
        c = -scale * tr(weight)
        loss = c * lp
    else:
        dl = lp - tr(logp_old)
        r, A = torch.exp(dl), tr(adv)
        one, ce = torch.ones((), dtype=dt), torch.tensor(clip_eps, dtype=dt)
        lo, hi = one - ce, one + ce
        clipped = ((A > 0) & (r > hi)) | ((A < 0) & (r < lo))
        c = torch.where(clipped, torch.zeros_like(r), -scale * A * r)
        loss = -scale * torch.minimum(r * A, torch.minimum(torch.maximum(r, lo), hi) * A)
        out.update(r=r, dl=dl, clipped=clipped, k=torch.clamp(torch.expm1(dl) - dl, min=0))
    out.update(dO=c[..., None] * dlp - es * dH, loss=loss - es * H, c=c)
    return out


def forward_parts(W, x):
    """float64 forward and its magnitude chain: (W, H1, H2, O, Oa) with Oa = |H2|' |W3| + |b3| as `magnitude_grads` forms it."""
    W = [w.double() for w in W]
    x = x.double()
    H1, H2, O = R.forward(W, x)
    A = [w.abs() for w in W]
    xa = x.abs().transpose(0, 1)
    H1a = (H1 > 0).double() * (xa @ A[0] + A[1][:, None])
    H2a = (H2 > 0).double() * (H1a @ A[2] + A[3][:, None])
    return W, H1, H2, O, H2a @ A[4] + A[5][:, None]


def chain(kind, W, x, dO):
    """dO [N, R, nout] -> the six gradient tensors, float64 matmuls (the kernel's backward chain)."""
    W = [w.double() for w in W]
    x = x.double()
    H1, H2, _ = R.forward(W, x)
    dO = dO.double()
    dH2 = (H2 > 0).double() * (dO @ W[4].transpose(1, 2))
    dH1 = (H1 > 0).double() * (dH2 @ W[2].transpose(1, 2))
    xt = x.transpose(0, 1)
    out = [xt.transpose(1, 2) @ dH1, dH1.sum(1), H1.transpose(1, 2) @ dH2, dH2.sum(1), H2.transpose(1, 2) @ dO, dO.sum(1)]
    out[4] = out[4] * R.structural_mask(kind, W)
    return out


def head_scales(kind, h, Oa):
    """From the float64 head `h` and the outputs' magnitudes Oa: (|dlogp/dO| scale, |dH/dO| scale [N,R,nout], lp scale, H scale [N,R])."""
    q = h["parts"]
    if kind == 1:
        p, lq, onehot, notmax = q["p"], q["lq"], q["onehot"], q["notmax"]
        cond = (1 + Oa + Oa.gather(-1, q["imax"])) * notmax
        dls = (p * cond).sum(-1, keepdim=True)                     # the scale of log1p(s): every exponential by its own cond
        cond = cond + (1 - notmax) * (1 + dls)
        pmag = p * cond
        dlp = onehot * (pmag * (1 - onehot)).sum(-1, keepdim=True) + (1 - onehot) * pmag
        Hrow = h["H"][..., None]
        dH = p * (lq.abs() + Hrow) * cond
        lqmag = lq.abs() + (cond - 1) + dls
        return dlp, dH, lqmag.gather(-1, onehot.argmax(-1, keepdim=True))[..., 0], (p * ((1 + lq.abs()) * lqmag + lq.abs())).sum(-1)
    mu, var, omv, omm, diff = q["mu"], q["var"], q["omv"], q["omm"], q["diff"]
    Om, Os = Oa[..., :2], Oa[..., 2:]
    cond = 1 + Om + Os
    d = q["a"].abs() + mu.abs()
    dlp = torch.cat([(d / var) * omm * cond, (0.5 + d * d / (2 * var)) * omv * cond], -1)
    dH = torch.cat([torch.zeros_like(omv), 0.5 * omv * cond], -1)
    sq = diff * diff / (2 * var)
    lps = (0.5 * (torch.log(2 * math.pi * var).abs() + 1 + omv * Os) + sq * (1 + omv * Os) + diff.abs() * d / var
           + (diff.abs() / var) * omm * Om).sum(-1)
    Hs = (0.5 * (torch.log(2 * math.pi * math.e * var).abs() + 1 + omv * Os)).sum(-1)
    return dlp, dH, lps, Hs


def reference(kind, W, x, act, form, scale, weight=None, logp_old=None, adv=None, es=0.0, clip_eps=CLIP_EPS):
    """The float64 cancellation-free truth of one gradient call and its sharp scales.  W six float32 / float64 tensors, x
    [R, N, d], act [R, N, 2], per-row inputs [R, N].  Returns a dict: grad / mag (six [N, ...]), loss / loss_scale [N], entropy /
    entropy_scale [N] (the mean row entropy), lp / lp_scale [R, N], H [R, N]; for ``ppo`` also r / r_scale, dl / dl_scale, k /
    k_scale, clipped [R, N], clip_fraction, approx_kl, ratio_min, ratio_max, kl [N]; ``rel`` [R, N] is the relative scale of r."""
    Wd, H1, H2, O, Oa = forward_parts(W, x)
    f = lambda t: None if t is None else t.double()
    h = head(kind, O, act.double(), form, scale, f(weight), f(logp_old), f(adv), es, clip_eps)
    dlp_s, dH_s, lp_s, H_s = head_scales(kind, h, Oa)
    tr = lambda t: t.transpose(0, 1)
    out = dict(lp=tr(h["lp"]), lp_scale=tr(lp_s), H=tr(h["H"]), entropy=h["H"].mean(1), entropy_scale=H_s.mean(1), O=O, Oa=Oa)
    if form == "logp":
        return out
    if form == "a2c":
        cmag = abs(scale) * tr(f(weight)).abs()
        loss_s = cmag * lp_s
    else:
        r = h["r"]
        rel = 1 + lp_s + h["lp"].abs() + tr(f(logp_old)).abs()
        cmag = abs(scale) * tr(f(adv)).abs() * r * rel
        loss_s = cmag
        cmag = cmag * (~h["clipped"]).double()
        dl_s = rel - 1
        out.update(r=tr(r), r_scale=tr(r * rel), rel=tr(rel), dl=tr(h["dl"]), dl_scale=tr(dl_s), k=tr(h["k"]),
                   k_scale=tr((r - 1).abs() * dl_s + torch.expm1(h["dl"]).abs() + h["dl"].abs()), clipped=tr(h["clipped"]),
                   clip_fraction=h["clipped"].double().mean(1), approx_kl=-h["dl"].mean(1), ratio_min=r.min(1).values,
                   ratio_max=r.max(1).values, kl=h["k"].mean(1))
    dOa = cmag[..., None] * dlp_s + abs(es) * dH_s
    loss_s = loss_s + abs(es) * H_s
    out.update(grad=chain(kind, Wd, x, h["dO"]), mag=ER._magnitude_chain(kind, Wd, x, dOa), loss=h["loss"].sum(1),
               loss_scale=loss_s.sum(1), dO=h["dO"], dOa=dOa, loss_rows=tr(h["loss"]), loss_rows_scale=tr(loss_s), H_scale=tr(H_s))
    return out


def sharp_magnitude_grads(kind, W, x, row_scale, act, weight, ent_scale=0.0):
    """`learner_ref.magnitude_grads` of an actor with the head's true term magnitudes (the module docstring)."""
    return reference(kind, W, x, act, "a2c", row_scale, weight=weight, es=ent_scale)["mag"]


def float32_grads(kind, W, x, act, form, scale, variant, **kw):
    """One of the two float32 restatements ("parent" / "free" = repaired) of the head on the float32 forward of W, x; its dO is
    chained to the six gradients in float64, so that the head's own error is what the comparison sees.  Returns (grads, head dict)."""
    W32 = [w.float() for w in W]
    O = R.forward(W32, x.float())[2]
    g = lambda t: None if t is None else t.float()
    h = head(kind, O, act.float(), form, scale, g(kw.get("weight")), g(kw.get("logp_old")), g(kw.get("adv")), kw.get("es", 0.0),
             variant=variant)
    return chain(kind, W, x, h["dO"]), h


def ratios(got, ref, scale):
    """|got - ref| / (1e-5 scale + 1e-30), elementwise, float64 CPU."""
    c = lambda t: torch.as_tensor(t).detach().double().cpu()
    return (c(got) - c(ref)).abs() / (BAR * c(scale) + FLOOR)


def worst_per_agent(got, ref, mag):
    """[N]: the worst error / bar ratio over the six gradient tensors of each agent."""
    n = ref[0].shape[0]
    return torch.stack([ratios(g, r, m).reshape(n, -1).max(1).values for g, r, m in zip(got, ref, mag)]).max(0).values


# ----------------------------------------------------------------------------------------------------------------------
# the trainers' hooks: `ppo_ref.ppo_train(actor_grads=, logp=)`, `entropy_ref.sa2c_train(a2c_grads=)`
def logp(kind, W, x, act):
    return reference(kind, W, x, act, "logp", 1.0)["lp"]


def actor_grads(kind, W, x, act, logp_old, adv, clip_eps, ent_scale=0.0):
    """`ppo_ref.actor_grads` (the same keys) from the cancellation-free head, ``mag`` the sharp scale."""
    ref = reference(kind, W, x, act, "ppo", 1.0 / x.shape[0], logp_old=logp_old, adv=adv, es=ent_scale, clip_eps=clip_eps)
    _, _, near = P.ratio_terms(ref["lp"], logp_old, adv, clip_eps)
    ref.update(near=near, logp=ref["lp"])
    return ref


def a2c_grads(kind, W, x, row_scale, act, weight, ent_scale=0.0):
    """`entropy_ref.a2c_grads` (the same keys) from the cancellation-free head, ``mag`` the sharp scale."""
    ref = reference(kind, W, x, act, "a2c", row_scale, weight=weight, es=ent_scale)
    plain = reference(kind, W, x, act, "a2c", row_scale, weight=weight)["loss"]
    ref.update(likelihood_loss=plain, entropy_loss=ref["loss"] - plain)
    return ref


# ----------------------------------------------------------------------------------------------------------------------
# the regimes
@functools.lru_cache(maxsize=None)
def case(kind, actions):
    """The seeded inputs of one actor kind (1 softmax-16, 2 Gaussian) and action set: one agent per regime, whose b3 moves
    the outputs of a small random net (`test_gpu_learner.random_net`, rows through `learner_ref.clean_rows`) to the regime's
    centre.  CPU tensors; a dict with W, x [T,E,N,d], act [T,E,N,2], adv (also the A2C weight; both signs), logp_old
    [T,E,N] float32, ``redrawn`` (the share of rows `ppo_ref.draw_logp_old` redrew), ``margin`` [R, N] (its per-row margin),
    ``small`` (the small net's own outputs [N, R, nout] float64) and ``other`` [R, N] (the rows that take another action).
    The same network and rows serve both action sets."""
    from tests import test_gpu_learner as TG
    assert kind in (1, 2) and actions in ACTIONS
    regimes = regimes_of(kind)
    N, nout = len(regimes), 16 if kind == 1 else 4
    gen = torch.Generator().manual_seed(7100 + kind)
    W = TG.random_net(torch, gen, N, D_IN, H1, H2, nout)
    if kind == 2:
        W[4] = W[4] * R.structural_mask(2, W)
    x, _, _, adv = TG.random_rows(torch, gen, T, E, N, D_IN, nout, kind)
    x = R.clean_rows(W, x, gen)
    xr = x.reshape(ROWS, N, D_IN)
    small = R.forward([w.double() for w in W], xr.double())[2]
    for i, regime in enumerate(regimes):
        if kind == 1:
            W[5][i] += regime[1]
            W[5][i, dominant(i)] += regime[0]
        else:
            W[5][i, :2] += torch.tensor(MU_SIGNS[i % 4]) * regime[0]
            W[5][i, 2:] += regime[1]
    gen = torch.Generator().manual_seed(7200 + 10 * kind + ACTIONS.index(actions))
    other = torch.zeros(ROWS, N, dtype=torch.bool)
    if actions == "mixed":
        other = torch.rand(ROWS, N, generator=gen) < OTHER_SHARE
    O = R.forward([w.double() for w in W], xr.double())[2]
    if kind == 1:
        dom = torch.tensor([dominant(i) for i in range(N)])
        idx = torch.where(other, (dom + torch.randint(1, nout, (ROWS, N), generator=gen)) % nout, dom.expand(ROWS, N))
        ang = idx.double() * 2 * math.pi / nout
        act = torch.stack([ang.cos(), ang.sin()], -1).float()
    else:
        mu, var = torch.tanh(O[..., :2]).transpose(0, 1), torch.sigmoid(O[..., 2:]).transpose(0, 1)
        act = (mu + var.sqrt() * torch.randn(ROWS, N, 2, generator=gen, dtype=torch.float64)).float()
        far = torch.randn(ROWS, N, 2, generator=gen) * 0.7
        act = torch.where(other[..., None], far, act)
    advr = adv.reshape(ROWS, N).double()
    ref = reference(kind, W, xr, act, "logp", 1.0)
    # logp_old is given, so a float32 ratio is off by its own lp's error, a few eps x the scale of lp, relatively (a far action
    # under a variance of 4.5e-5 has lp ~ -1e5): a row that close to a clip edge may take the other branch, whatever the head's form
    margin = torch.clamp(2 * EPS32 * ref["lp_scale"], min=P.EDGE_MARGIN)
    old, share = P.draw_logp_old(ref["lp"], advr, CLIP_EPS, gen, margin=margin)
    return dict(kind=kind, actions=actions, regimes=regimes, W=W, x=x, act=act.reshape(T, E, N, 2), adv=adv,
                logp_old=old.reshape(T, E, N), redrawn=share, margin=margin, small=small, other=other)


def rows_of(c):
    """(x, act, adv, logp_old) of a `case` as rows [R, N, ...]."""
    N = len(c["regimes"])
    return tuple(c[k].reshape(ROWS, N, *c[k].shape[3:]) for k in ("x", "act", "adv", "logp_old"))


def form_reference(c, form):
    """`reference` of a case for one of FORMS, as the GPU tests call the runners: a2c with row_scale 1 / E, ppo with 1 / rows;
    the ``_ent`` forms and ``gated`` with ENT_SCALE."""
    x, act, adv, old = rows_of(c)
    es = ENT_SCALE if form in ("a2c_ent", "ppo_ent", "gated") else 0.0
    if form == "logp":
        return reference(c["kind"], c["W"], x, act, "logp", 1.0)
    if form.startswith("a2c"):
        return reference(c["kind"], c["W"], x, act, "a2c", 1.0 / E, weight=adv, es=es)
    return reference(c["kind"], c["W"], x, act, "ppo", 1.0 / ROWS, logp_old=old, adv=adv, es=es)
