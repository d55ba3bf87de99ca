"""Float64 torch restatement of the PPO learner's contract (SAC_agents.py:410-573, `SPPOAgents.train`, generalised to a
window of E envs x T steps): the checker of the PPO tests (test infrastructure; CPU or GPU tensors, float64).  Built on the
helpers of tests/learner_ref.py, same layouts: weights stacked [N, ...], rows x [R, N, d_in].

The reference class cannot be executed as written (its actors are built without the required ``lr``, ``Qjsum`` is read one
line before it is assigned, and ``Adv`` keeps the critic's autograd graph across epochs), so this file states the algorithm
of those lines with exactly these three repairs; the one part of the class that does run, ``probability_of_ai``, is
recorded in tests/golden/ppo_n5.npz and checked against `logp` here (tests/test_ppo_host.py)."""
import math

import torch

from tests import learner_ref as R

EDGE_MARGIN = 1e-4          # rows whose ratio is this close (relative) to 1 +- clip_eps may take the other branch in float32


def logp(kind, W, x, act):
    """log pi_i(act | x) [R, N] float64 (differentiable in W): kind 1 the log softmax at the stored action's index, kind 2
    the log of the product of two normal densities with VARIANCE sigma (:558-573)."""
    _, _, O = R.forward([w.double() for w in W], x.double())
    ones = torch.ones(x.shape[0], x.shape[1], dtype=torch.float64, device=x.device)
    return -R.row_losses(kind, O, act=act.double(), weight=ones).transpose(0, 1)


def neighbour_sum(G, nbr):
    """Q[t,e,i] = sum_{j in nbr[t,e,i]} G[t,e,j] (:498-501), -1 slots skipped."""
    T, E, N = G.shape
    nb = nbr.long()
    Gj = torch.gather(G.double()[:, :, None, :].expand(T, E, N, N), 3, nb.clamp(min=0))
    return (Gj * (nb >= 0).double()).sum(-1)


def advantage(G, V, nbr, baseline="once"):
    """Adv = Q - V (``once``: one baseline against the neighbour sum, :513) or Q - |N_i| V (``per_neighbour``)."""
    c = 1.0 if baseline == "once" else (nbr >= 0).double().sum(-1)
    assert baseline in ("once", "per_neighbour")
    return neighbour_sum(G, nbr) - c * V.double()


def ratio_terms(lp, logp_old, adv, clip_eps, margin=EDGE_MARGIN):
    """(r, clipped, near): the ratio, the rows where the clipped branch is the strict minimum, and the rows within
    ``margin`` (relative; a number or a tensor [R, N], default EDGE_MARGIN) of a clip edge; all [R, N]."""
    r = torch.exp(lp.double() - logp_old.double())
    adv = adv.double()
    clipped = ((adv > 0) & (r > 1 + clip_eps)) | ((adv < 0) & (r < 1 - clip_eps))
    near = ((r / (1 + clip_eps) - 1).abs() <= margin) | ((r / (1 - clip_eps) - 1).abs() <= margin)
    return r, clipped, near


def actor_grads(kind, W, x, act, logp_old, adv, clip_eps):
    """The PPO actor step's gradients over the R rows of x: L_i = -(1/R) sum_rows min(r Adv, clamp(r, 1 - eps, 1 + eps) Adv).
    A row's gradient is -(1/R) Adv r dlogp/dtheta unless the clipped branch is the strict minimum, i.e. the A2C-style
    gradient `learner_ref.grads` with the CONSTANT weight Adv r [unclipped].  Returns a dict: grad (six [N, ...]), mag (its
    error scale, `magnitude_grads` with the same weight), loss [N], r, clipped, near [R, N], clip_fraction, approx_kl,
    ratio_min, ratio_max [N]."""
    rows = x.shape[0]
    with torch.no_grad():
        lp = logp(kind, W, x, act)
        r, clipped, near = ratio_terms(lp, logp_old, adv, clip_eps)
        A = adv.double()
        weight = A * r * (~clipped).double()
        loss = -torch.minimum(r * A, torch.clamp(r, 1 - clip_eps, 1 + clip_eps) * A).sum(0) / rows
    grad, _ = R.grads(kind, W, x, 1.0 / rows, act=act, weight=weight)
    mag = R.magnitude_grads(kind, W, x, 1.0 / rows, act=act, weight=weight)
    return dict(grad=grad, mag=mag, loss=loss, r=r, clipped=clipped, near=near, logp=lp, weight=weight,
                clip_fraction=clipped.double().mean(0), approx_kl=(logp_old.double() - lp).mean(0),
                ratio_min=r.min(0).values, ratio_max=r.max(0).values)


def draw_logp_old(lp, adv, clip_eps, gen, spread=math.log(2.0), margin=EDGE_MARGIN):
    """``logp_old = lp - u`` with a continuous offset u uniform in [-spread, spread] (r = exp(u) spreads over [0.5, 2] at the
    default), offsets of rows within ``margin`` of a clip edge redrawn (as `learner_ref.clean_rows` does for relu kinks).
    lp, adv CPU float64 [R, N].  Returns (logp_old float32 -- what the kernel is given --, share of rows redrawn)."""
    draw = lambda n: (torch.rand(n, generator=gen, dtype=torch.float64) * 2 - 1) * spread
    u = draw(lp.numel()).view_as(lp)
    redrawn = torch.zeros_like(lp, dtype=torch.bool)
    for _ in range(20):
        old = (lp - u).float()                        # the float32 value the kernel reads decides the float64 ratio
        _, _, near = ratio_terms(lp, old, adv, clip_eps, margin)
        if not near.any():
            return old, float(redrawn.double().mean())
        redrawn |= near
        u[near] = draw(int(near.sum()))
    raise RuntimeError("could not draw ratios away from the clip edges")


def ppo_train(kind, Wa, Wc, x, reward, done, act, nbr, gamma, epochs=10, clip_eps=0.2, lr_actor=1e-3, lr_critic=1e-3,
              max_norm=10.0, baseline="once", state=None, actor_grads=None, logp=None):
    """One `SPPOAgents.train` over a window: x [T,E,N,d], reward [T,E,N], done [T,E], act [T,E,N,2], nbr [T,E,N,k+1].
    ``state``: the Adam state of earlier calls (None = fresh optimisers).  ``actor_grads`` / ``logp``: other statements of
    this module's functions of those names (tests/saturation_ref.py: the heads written without cancellation).
    Returns a dict: G, Q, V (pre-update critic), adv, logp_old [T,E,N]; per epoch lists ``critic_loss, critic_norm, critic_grad, actor_loss, actor_norm, actor`` (the
    `actor_grads` dict); the post-update weights and the new Adam ``state``."""
    T, E, N = reward.shape
    rows = T * E
    xr = x.reshape(rows, N, -1).double()
    actr = act.reshape(rows, N, 2).double()
    G = R.returns(reward, done, gamma)
    Wa, Wc = [w.double() for w in Wa], [w.double() for w in Wc]
    zeros = lambda W: [torch.zeros_like(w) for w in W]
    if state is None:
        state = dict(cm1=zeros(Wc), cm2=zeros(Wc), am1=zeros(Wa), am2=zeros(Wa), step=0)
    actor_grads, logp = actor_grads or globals()["actor_grads"], logp or globals()["logp"]
    logp_old = logp(kind, Wa, xr, actr).detach()
    V = R.forward(Wc, xr)[2][..., 0].transpose(0, 1).reshape(T, E, N)
    adv = advantage(G, V, nbr, baseline)
    out = dict(G=G, Q=neighbour_sum(G, nbr), V=V, adv=adv, logp_old=logp_old.reshape(T, E, N), critic_loss=[], critic_norm=[],
               critic_grad=[], actor_loss=[], actor_norm=[], actor=[])
    cm1, cm2, am1, am2, step = state["cm1"], state["cm2"], state["am1"], state["am2"], state["step"]
    for _ in range(epochs):
        step += 1
        gc, lc = R.grads(0, Wc, xr, 1.0 / rows, target=G.reshape(rows, N))
        Wc, cm1, cm2, nc = R.clip_adam(Wc, gc, cm1, cm2, step, lr_critic, max_norm)
        a = actor_grads(kind, Wa, xr, actr, logp_old, adv.reshape(rows, N), clip_eps)
        Wa, am1, am2, na = R.clip_adam(Wa, a["grad"], am1, am2, step, lr_actor, max_norm)
        out["critic_loss"].append(lc); out["critic_norm"].append(nc); out["critic_grad"].append(gc)
        out["actor_loss"].append(a["loss"]); out["actor_norm"].append(na); out["actor"].append(a)
    out.update(critic_post=Wc, actor_post=Wa, state=dict(cm1=cm1, cm2=cm2, am1=am1, am2=am2, step=step))
    return out


def head_case(case, clip_eps=0.2):
    """The inputs of the head tests for one actor row of `test_gpu_learner.FUZZ`: seeded random networks and rows (relu
    kinks cleaned), an advantage of both signs and a `logp_old` drawn by `draw_logp_old`.  CPU tensors; returns a dict with
    W, x [T,E,N,d], act [T,E,N,2], adv, logp_old [T,E,N] float32, and ``redrawn``, the share of rows whose offset was redrawn."""
    from tests import test_gpu_learner as TG
    N, E, T, d_in, h1, h2, kind, nout, rc = case
    gen = torch.Generator().manual_seed(1000 + sum((j + 1) * (c or 0) for j, c in enumerate(case)))
    W = TG.random_net(torch, gen, N, d_in, h1, h2, nout)
    if kind == 2:
        W[4] = W[4] * R.structural_mask(2, W)
    x, _, act, adv = TG.random_rows(torch, gen, T, E, N, d_in, nout, kind)
    x = R.clean_rows(W, x, gen)
    lp = logp(kind, W, x.reshape(T * E, N, d_in), act.reshape(T * E, N, 2))
    old, share = draw_logp_old(lp, adv.reshape(T * E, N).double(), clip_eps, gen)
    return dict(W=W, x=x, act=act, adv=adv, logp_old=old.reshape(T, E, N), redrawn=share, kind=kind, rows_per_chunk=rc)
