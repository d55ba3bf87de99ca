"""Float64 torch restatement of the PPO learner's two guards -- the per-agent KL early stop (``target_kl``) and the clipped value
loss (``vf_clip``) -- written from the text of include/dronesim.h: the checker of tests/test_ppo_guard_host.py and
tests/test_gpu_ppo_guard.py (test infrastructure; CPU or GPU tensors, float64).  Built on tests/learner_ref.py, tests/ppo_ref.py,
tests/entropy_ref.py, tests/lambda_ref.py and tests/minibatch_ref.py, same layouts: weights stacked [N, ...], rows x [R, N, d_in].

  kl            per agent the mean over the rows of k = expm1(dl) - dl, dl = logp - logp_old   (Schulman's (r - 1) - log r)
  gate          active &= kl <= target_kl (NaN stops, equality continues, a stop is sticky); taken += active
  value loss    Vc = v_old + clamp(V - v_old, +-vf_clip),  l = max((V - G)^2, (Vc - G)^2);  the gradient of a row is 2 (V - G)
                unless the clipped term is the STRICT maximum, where V is clamped and the gradient is 0"""
import math

import numpy as np
import torch

from tests import entropy_ref as EN
from tests import lambda_ref as LR
from tests import learner_ref as R
from tests import minibatch_ref as MB
from tests import ppo_ref as P

VCLIP_MARGIN = 1e-4         # rows this close (relative) to a clamp edge, or to a tie of the two squared errors, may go either way in float32


def kl_rows(lp, logp_old):
    """k [R, N] float64 = expm1(dl) - dl >= 0."""
    dl = lp.double() - logp_old.double()
    return torch.expm1(dl) - dl


def kl_estimate(lp, logp_old):
    return kl_rows(lp, logp_old).mean(0)


def gate(active, taken, kl, target_kl, reset=False):
    """The host rule of `dronesim_kl_gate` on Python lists; returns the new (active, taken)."""
    if reset:
        return [1] * len(active), [0] * len(active)
    a2, t2 = [], []
    for a, t, k in zip(active, taken, kl):
        if a and not (k <= target_kl):
            a = 0
        a2.append(1 if a else 0)
        t2.append(t + 1 if a else t)
    return a2, t2


def stops_of(table, tau):
    """The steps each actor takes, from an UNGATED kl table [S, N] (an agent's actor depends on nobody else's): the index of
    the first step whose kl is not <= tau (that step is computed and discarded), S if there is none."""
    S, N = table.shape
    out = []
    for i in range(N):
        s = S
        for j in range(S):
            if not (float(table[j, i]) <= tau):
                s = j
                break
        out.append(s)
    return out


def pick_tau(table, bar, factor=4.0):
    """Among the geometric midpoints of adjacent sorted positive table values, the candidate with the most distinct stop steps
    whose gap is wide enough: every entry an agent reaches (its crossing step included) is at least ``factor`` x its bar away.
    table, bar [S, N] float64.  Returns (tau, stops, smallest gap in bars) or None."""
    vals = sorted({float(v) for v in table.flatten().tolist() if v > 0})
    best = None
    for lo, hi in zip(vals[:-1], vals[1:]):
        tau = math.sqrt(lo * hi)
        stops = stops_of(table, tau)
        gap = math.inf
        for i, s in enumerate(stops):
            for j in range(min(s + 1, table.shape[0])):
                gap = min(gap, abs(float(table[j, i]) - tau) / float(bar[j, i]))
        if gap < factor:
            continue
        key = (len(set(stops)), gap)
        if best is None or key > best[0]:
            best = (key, tau, stops, gap)
    return None if best is None else best[1:]


def vclip_terms(V, v_old, G, vf_clip):
    """(l, zero, clamped, near) [R, N]: the per-row clipped loss, the rows whose gradient is zero (the clipped term is the strict
    maximum), the clamped rows, and the rows near an edge: ||V - v_old| / vf_clip - 1| <= VCLIP_MARGIN, or clamped with the two
    squared errors within VCLIP_MARGIN (relative) of each other."""
    V, v_old, G = V.double(), v_old.double(), G.double()
    dv = V - v_old
    clamped = dv.abs() > vf_clip
    # (V itself where it is not clamped: v_old + (V - v_old) rounds, and a rounding must not make the clipped term a strict maximum)
    Vc = torch.where(clamped, v_old + torch.clamp(dv, -vf_clip, vf_clip), V)
    l1, l2 = (V - G) ** 2, (Vc - G) ** 2
    zero = l2 > l1
    near = torch.zeros_like(zero)
    if math.isfinite(vf_clip):
        near = ((dv.abs() / vf_clip - 1).abs() <= VCLIP_MARGIN) | (clamped & ((l1 - l2).abs() <= VCLIP_MARGIN * torch.maximum(l1, l2)))
    return torch.maximum(l1, l2), zero, clamped, near


def vclip_grads(W, x, row_scale, target, v_old, vf_clip):
    """The clipped value loss L_i = row_scale sum_r max((V - G)^2, (Vc - G)^2) of a critic over the R rows of x.  Returns a dict:
    grad (six [N, ...]), mag (`learner_ref.magnitude_grads`'s chain behind |dO| = 2 s (|V|' + |G|) on the rows with a gradient),
    loss [N], zero / clamped / near [R, N], clip_fraction [N]."""
    Wd = [w.detach().double().clone().requires_grad_(True) for w in W]
    _, _, O = R.forward(Wd, x.double())
    V = O[..., 0].transpose(0, 1)                                       # [R, N]
    l, zero, clamped, near = vclip_terms(V.detach(), v_old, target, vf_clip)
    # a zero-gradient row is a constant of the loss (V is clamped there); every other row is the plain squared error
    rows = torch.where(zero, l, (V - target.double()) ** 2)
    loss = row_scale * rows.sum(0)
    g = list(torch.autograd.grad(loss.sum(), Wd))
    with torch.no_grad():
        Wn = [w.detach() for w in Wd]
        H1, H2, _ = R.forward(Wn, x.double())
        A = [w.abs() for w in Wn]
        xa = x.double().abs().transpose(0, 1)
        H1a = (H1 > 0).double() * (xa @ A[0] + A[1][:, None])
        H2a = (H2 > 0).double() * (H1a @ A[2] + A[3][:, None])
        Oa = H2a @ A[4] + A[5][:, None]
        dOa = 2 * abs(row_scale) * (Oa + target.double().transpose(0, 1).abs()[..., None]) * (~zero).double().transpose(0, 1)[..., None]
        mag = EN._magnitude_chain(0, Wn, x, dOa)
    return dict(grad=[t.detach() for t in g], mag=mag, loss=loss.detach(), zero=zero, clamped=clamped, near=near,
                clip_fraction=zero.double().mean(0), rows=rows.detach())


def vclip_case(case, vf_clip=0.2):
    """The inputs of the clipped-value-head test for one critic row of `test_gpu_learner.FUZZ`: the fuzz test's seeded network, rows
    and target G, and ``v_old = V_ref - u`` with u uniform in [-2 vf_clip, 2 vf_clip]; the offsets of rows near an edge are redrawn
    (as `ppo_ref.draw_logp_old` redraws).  CPU tensors; returns a dict with W, x [T,E,N,d], target, v_old [T,E,N] float32, ``redrawn``."""
    from tests import test_gpu_learner as TG
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    assert kind == 0
    gen = torch.Generator().manual_seed(sum((j + 1) * (c or 0) for j, c in enumerate(case)))
    W = TG.random_net(torch, gen, N, d_in, h1, h2, nout)
    x, target, _, _ = TG.random_rows(torch, gen, T, E, N, d_in, nout, kind)
    x = R.clean_rows(W, x, gen)
    rows = T * E
    V = LR.critic_values(W, x.reshape(rows, N, d_in))
    G = target.reshape(rows, N).double()
    draw = lambda n: (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * 2 * vf_clip
    u = draw(V.numel()).view_as(V)
    redrawn = torch.zeros_like(V, dtype=torch.bool)
    for _ in range(20):
        old = (V - u).float()
        _, _, _, near = vclip_terms(V, old, G, vf_clip)
        if not near.any():
            return dict(W=W, x=x, target=target, v_old=old.reshape(T, E, N), redrawn=float(redrawn.double().mean()), rows_per_chunk=rc)
        redrawn |= near
        u[near] = draw(int(near.sum()))
    raise RuntimeError("could not draw old values away from the clamp edges")


def ppo_train(kind, Wa, Wc, x, reward, done, act, nbr, gamma, epochs=10, minibatches=1, shuffle_seed=0, clip_eps=0.2, lr_actor=1e-3,
              lr_critic=1e-3, max_norm=10.0, baseline="once", ent_coef=0.0, normalize_advantage=False, adv_eps=1e-8, lam=None,
              x_all=None, target_kl=None, vf_clip=None):
    """One `PPOLearner.train` from fresh optimisers with the two guards, whole-window (``minibatches = 1``: every epoch is one step
    over the rows in window order) or in shuffled minibatches (`minibatch_ref.ppo_train_minibatch`'s loop).  With ``lam`` the
    once-per-window critic forward runs over the ring ``x_all`` [T+1,E,N,d] (`lambda_ref.ppo_train`).

    ``target_kl``: per actor step, all agents' gradients are formed, then the gate, then Adam for the agents still active (an
    active agent has taken every earlier step of the call, so one step count serves them all).  ``vf_clip``: the critic steps use
    `vclip_grads` with v_old = the pre-update V.  Returns a dict; the per-step entries are flat lists over the
    ``epochs x minibatches`` steps: critic_loss, critic_norm, critic (the `vclip_grads` dict, with vf_clip), actor_loss,
    actor_norm, actor (the `entropy_ref.actor_grads` dict), kl, klmag (the error scale mean(|logp_old| + |logp|) of kl),
    active (the agents that took the step); and actor_steps, perms, the post-update weights and the Adam moments."""
    T, E, N = reward.shape
    rows, K = T * E, int(minibatches)
    assert rows % K == 0
    M = rows // K
    Wa, Wc = [w.double() for w in Wa], [w.double() for w in Wc]
    if lam is None:
        xr = x.reshape(rows, N, -1).double()
        G = R.returns(reward, done, gamma)
        V = LR.critic_values(Wc, xr).reshape(T, E, N)
    else:
        xa = x_all.reshape((T + 1) * E, N, -1).double()
        xr = xa[:rows]
        V_all = LR.critic_values(Wc, xa).reshape(T + 1, E, N)
        G, _ = LR.lambda_returns(reward, V_all, done, gamma, lam)
        V = V_all[:T]
    actr = act.reshape(rows, N, 2).double()
    zeros = lambda W: [torch.zeros_like(w) for w in W]
    cm1, cm2, am1, am2 = zeros(Wc), zeros(Wc), zeros(Wa), zeros(Wa)
    logp_old = P.logp(kind, Wa, xr, actr).detach()
    adv = P.advantage(G, V, nbr, baseline)
    out = dict(G=G, V=V, adv_raw=adv, logp_old=logp_old.reshape(T, E, N), perms=[])
    if normalize_advantage:
        adv, mean, std = EN.standardize(adv, adv_eps)
        out.update(adv_mean=mean, adv_std=std)
    out["adv"] = adv
    Gr, advr, Vr = G.reshape(rows, N), adv.reshape(rows, N), V.reshape(rows, N)
    keys = ("critic_loss", "critic_norm", "critic", "actor_loss", "actor_norm", "actor", "kl", "klmag", "active")
    out.update({k: [] for k in keys})
    active = torch.ones(N, dtype=torch.bool)
    taken = torch.zeros(N, dtype=torch.long)
    step = 0
    sel = lambda mask, new, old: [torch.where(mask.view(-1, *([1] * (n.dim() - 1))), n, o) for n, o in zip(new, old)]
    for ep in range(epochs):
        if K > 1:
            perm = MB.row_permutation(rows, shuffle_seed, step)
            assert np.array_equal(np.sort(perm), np.arange(rows))
            out["perms"].append(perm)
        for b in range(K):
            idx = torch.arange(rows) if K == 1 else torch.as_tensor(perm[b * M:(b + 1) * M])
            step += 1
            if vf_clip is None:
                gc, lc = R.grads(0, Wc, xr[idx], 1.0 / M, target=Gr[idx])
                c = None
            else:
                c = vclip_grads(Wc, xr[idx], 1.0 / M, Gr[idx], Vr[idx], vf_clip)
                gc, lc = c["grad"], c["loss"]
            Wc, cm1, cm2, nc = R.clip_adam(Wc, gc, cm1, cm2, step, lr_critic, max_norm)
            a = EN.actor_grads(kind, Wa, xr[idx], actr[idx], logp_old[idx], advr[idx], clip_eps, ent_coef / M)
            if normalize_advantage:           # a standardised advantage this close to 0 may fall on either side of the clip test
                a["near"] = a["near"] | (advr[idx].abs() <= EN.ZERO_MARGIN)
            kl = kl_estimate(a["logp"], logp_old[idx])
            klmag = (logp_old[idx].abs() + a["logp"].abs()).mean(0)
            computed = active.clone()
            if target_kl is not None:
                active = active & (kl <= target_kl)
            taken = taken + active.long()
            Wn, n1, n2, na = R.clip_adam(Wa, a["grad"], am1, am2, step, lr_actor, max_norm)
            Wa, am1, am2 = sel(active, Wn, Wa), sel(active, n1, am1), sel(active, n2, am2)
            for k, v in zip(keys, (lc, nc, c, a["loss"], na, a, kl, klmag, (computed, active.clone()))):
                out[k].append(v)
    out.update(critic_post=Wc, actor_post=Wa, actor_steps=taken, cm2=cm2, am1=am1, am2=am2, steps=step)
    return out
