"""Float64 torch restatement of the learners' entropy bonus and per-agent advantage standardisation: the checker of
tests/test_entropy_host.py and tests/test_gpu_entropy.py (test infrastructure; CPU or GPU tensors, float64).  Built on
tests/learner_ref.py and tests/ppo_ref.py, same layouts: weights stacked [N, ...], rows x [R, N, d_in].

The reference has neither term (SAC_agents.py:327-357, :522-555); the definitions are the usual ones:

  standardise   per agent over the window's R rows: (x - mean) / (std + eps), std the population form (divide by R)
  entropy       softmax: H = -sum_j p_j log p_j;  Gaussian with var = sigmoid(o): H = sum_d 0.5 log(2 pi e var_d)
  loss          L_i - ent_scale sum_r H_i(x_r)   (the learners pass ent_scale = ent_coef / rows: -ent_coef x the mean entropy)"""
import math

import torch

from tests import learner_ref as R
from tests import ppo_ref as P

ZERO_MARGIN = 1e-4          # rows whose standardised advantage is this close to 0 may take either side of the clip test in float32

# (R, N) of the standardisation tests: one row, less than a wave, several slabs, a ragged last slab, column tiles, N % 4 != 0,
# and 257 lane groups of four (the tile is capped at 256: a second column tile with one live group)
STANDARDIZE_SHAPES = [(1, 5), (63, 5), (600, 5), (8193, 64), (1000, 70), (257, 256), (4099, 3), (257, 1028)]
HARD_COLUMN, CONSTANT_COLUMN = 0, 1


def standardize(x, eps=1e-8):
    """x [..., N] -> (y, mean [N], std [N]) float64 over all leading axes, population std."""
    xd = x.double()
    flat = xd.reshape(-1, xd.shape[-1])
    mean = flat.mean(0)
    std = torch.sqrt(((flat - mean) ** 2).mean(0))
    return (xd - mean) / (std + eps), mean, std


def standardize_case(rows, n, seed=0):
    """The input of the standardisation tests, float32 [rows, n]: seeded normal data with a per-agent offset and scale;
    column HARD_COLUMN sits at -500 +- 0.5 (a near-converged critic's advantages: a float32 sum of squares loses its
    variance), column CONSTANT_COLUMN is one value."""
    gen = torch.Generator().manual_seed(100 + seed)
    offset = torch.randn(n, generator=gen, dtype=torch.float64) * 10
    scale = torch.exp(torch.randn(n, generator=gen, dtype=torch.float64))
    offset[HARD_COLUMN], scale[HARD_COLUMN] = -500.0, 0.5
    x = (torch.randn(rows, n, generator=gen, dtype=torch.float64) * scale + offset).float()
    x[:, CONSTANT_COLUMN] = -3.7
    return x


def standardize_float32(x, eps=1e-8):
    """The plausible wrong kernel: sum x and sum x^2 accumulated in float32, var = E[x^2] - mean^2."""
    import numpy as np
    a = x.numpy().astype(np.float32)
    s1 = np.cumsum(a, axis=0, dtype=np.float32)[-1]
    s2 = np.cumsum(a * a, axis=0, dtype=np.float32)[-1]
    n = np.float32(a.shape[0])
    mean = s1 / n
    var = np.maximum(s2 / n - mean * mean, np.float32(0))
    return torch.from_numpy((a - mean) / (np.sqrt(var) + np.float32(eps)))


def row_entropy(kind, O):
    """H [N, R] float64 from the pre-activation outputs O [N, R, nout] (differentiable)."""
    if kind == 1:
        lq = torch.log_softmax(O, -1)
        return -(torch.exp(lq) * lq).sum(-1)
    var = torch.sigmoid(O[..., 2:])
    return (0.5 * torch.log(2 * math.pi * math.e * var)).sum(-1)


def entropy_dO(kind, O):
    """dH / dO [N, R, nout] in closed form -- what the heads add, times -ent_scale:
    softmax -p_j (log p_j + H); Gaussian 0 for the mu outputs and 0.5 (1 - var_d) for the variance outputs."""
    if kind == 1:
        lq = torch.log_softmax(O, -1)
        p = torch.exp(lq)
        H = -(p * lq).sum(-1, keepdim=True)
        return -p * (lq + H)
    var = torch.sigmoid(O[..., 2:])
    return torch.cat([torch.zeros_like(var), 0.5 * (1 - var)], -1)


def _magnitude_chain(kind, W, x, dOa):
    """`learner_ref.magnitude_grads`'s backward chain (every operand by its absolute value) behind a given |dO| [N,R,nout]."""
    W = [w.double() for w in W]
    x = x.double()
    H1, H2, _ = R.forward(W, x)
    m1, m2 = (H1 > 0).double(), (H2 > 0).double()
    A = [w.abs() for w in W]
    xa = x.abs().transpose(0, 1)
    H1a = m1 * (xa @ A[0] + A[1][:, None])
    H2a = m2 * (H1a @ A[2] + A[3][:, None])
    dH2a = m2 * (dOa @ A[4].transpose(1, 2))
    dH1a = m1 * (dH2a @ A[2].transpose(1, 2))
    out = [xa.transpose(1, 2) @ dH1a, dH1a.sum(1), H1a.transpose(1, 2) @ dH2a, dH2a.sum(1), H2a.transpose(1, 2) @ dOa, dOa.sum(1)]
    out[4] = out[4] * R.structural_mask(kind, W)
    return out


def entropy_grads(kind, W, x, ent_scale):
    """The entropy term -ent_scale sum_r H_i(x_r) of agent i over the R rows of x, by float64 autograd.  Returns a dict:
    grad (six [N, ...]), mag (its error scale: the closed-form dO with every operand by its absolute value -- log p = o - lse
    counts |o| + |lse| --, then `magnitude_grads`'s chain), loss [N], H [R, N], entropy [N] (the mean row entropy)."""
    Wd = [w.detach().double().clone().requires_grad_(True) for w in W]
    _, _, O = R.forward(Wd, x.double())
    H = row_entropy(kind, O)
    loss = -ent_scale * H.sum(1)
    g = list(torch.autograd.grad(loss.sum(), Wd))
    g[4] = g[4] * R.structural_mask(kind, Wd)
    with torch.no_grad():
        O = O.detach()
        A = [w.detach().abs() for w in Wd]
        H1, H2, _ = R.forward([w.detach() for w in Wd], x.double())
        xa = x.double().abs().transpose(0, 1)
        H1a = (H1 > 0).double() * (xa @ A[0] + A[1][:, None])
        H2a = (H2 > 0).double() * (H1a @ A[2] + A[3][:, None])
        Oa = H2a @ A[4] + A[5][:, None]
        if kind == 1:
            p = torch.softmax(O, -1)
            la = O.abs() + torch.logsumexp(O, -1, keepdim=True).abs()
            dOa = abs(ent_scale) * p * (la + (p * la).sum(-1, keepdim=True))
        else:
            var = torch.sigmoid(O[..., 2:])
            cond = 1 + Oa[..., :2] + Oa[..., 2:]          # (as magnitude_grads: an output's own rounding error moves var)
            dOa = torch.cat([torch.zeros_like(var), abs(ent_scale) * 0.5 * (1 - var) * cond], -1)
        mag = _magnitude_chain(kind, [w.detach() for w in Wd], x, dOa)
    Hd = H.detach().transpose(0, 1)
    return dict(grad=[t.detach() for t in g], mag=mag, loss=loss.detach(), H=Hd, entropy=Hd.mean(0))


def _add(a, b):
    return [s + t for s, t in zip(a, b)]


def actor_grads(kind, W, x, act, logp_old, adv, clip_eps, ent_scale=0.0):
    """`ppo_ref.actor_grads` plus the entropy term: L_i = -(1/R) sum_rows min(r Adv, clamp(r) Adv) - ent_scale sum_rows H.
    The entropy gradient is on every row, the clipped ones included.  The dict of `ppo_ref.actor_grads` with grad, mag and
    loss of the whole objective, plus ``surrogate_loss``, ``H`` [R, N] and ``entropy`` [N]."""
    a = P.actor_grads(kind, W, x, act, logp_old, adv, clip_eps)
    e = entropy_grads(kind, W, x, ent_scale)
    a.update(surrogate_loss=a["loss"], grad=_add(a["grad"], e["grad"]), mag=_add(a["mag"], e["mag"]), loss=a["loss"] + e["loss"],
             H=e["H"], entropy=e["entropy"], entropy_loss=e["loss"])
    return a


def a2c_grads(kind, W, x, row_scale, act, weight, ent_scale=0.0):
    """`learner_ref.grads` of an actor plus the entropy term: L_i = -row_scale sum_r w log pi - ent_scale sum_r H.
    Returns a dict: grad, mag, loss [N] (the whole objective), likelihood_loss, H [R, N], entropy [N]."""
    g, l = R.grads(kind, W, x, row_scale, act=act, weight=weight)
    mag = R.magnitude_grads(kind, W, x, row_scale, act=act, weight=weight)
    e = entropy_grads(kind, W, x, ent_scale)
    return dict(grad=_add(g, e["grad"]), mag=_add(mag, e["mag"]), loss=l + e["loss"], likelihood_loss=l, H=e["H"],
                entropy=e["entropy"], entropy_loss=e["loss"])


def ppo_train(kind, Wa, Wc, x, reward, done, act, nbr, gamma, epochs=10, clip_eps=0.2, lr_actor=1e-3, lr_critic=1e-3,
              max_norm=10.0, baseline="once", state=None, ent_coef=0.0, normalize_advantage=False, adv_eps=1e-8):
    """`ppo_ref.ppo_train` with the two options: ``normalize_advantage`` standardises agent i's advantages over the T E rows
    once per window (``adv_raw``, ``adv_mean``, ``adv_std`` keep what came before); ``ent_coef`` adds -ent_coef x the mean row
    entropy to every epoch's actor loss.  ``near_zero`` [rows, N] marks the rows whose advantage is within ZERO_MARGIN of 0
    after the standardisation (none without it)."""
    T, E, N = reward.shape
    rows = T * E
    xr = x.reshape(rows, N, -1).double()
    actr = act.reshape(rows, N, 2).double()
    G = R.returns(reward, done, gamma)
    Wa, Wc = [w.double() for w in Wa], [w.double() for w in Wc]
    zeros = lambda W: [torch.zeros_like(w) for w in W]
    if state is None:
        state = dict(cm1=zeros(Wc), cm2=zeros(Wc), am1=zeros(Wa), am2=zeros(Wa), step=0)
    logp_old = P.logp(kind, Wa, xr, actr).detach()
    V = R.forward(Wc, xr)[2][..., 0].transpose(0, 1).reshape(T, E, N)
    adv_raw = P.advantage(G, V, nbr, baseline)
    adv, near_zero = adv_raw, torch.zeros(rows, N, dtype=torch.bool)
    out = dict(G=G, Q=P.neighbour_sum(G, nbr), V=V, adv_raw=adv_raw, logp_old=logp_old.reshape(T, E, N), critic_loss=[],
               critic_norm=[], critic_grad=[], actor_loss=[], actor_norm=[], actor=[], entropy=[])
    if normalize_advantage:
        adv, mean, std = standardize(adv_raw, adv_eps)
        near_zero = adv.reshape(rows, N).abs() <= ZERO_MARGIN
        out.update(adv_mean=mean, adv_std=std)
    out.update(adv=adv, near_zero=near_zero)
    cm1, cm2, am1, am2, step = state["cm1"], state["cm2"], state["am1"], state["am2"], state["step"]
    for _ in range(epochs):
        step += 1
        gc, lc = R.grads(0, Wc, xr, 1.0 / rows, target=G.reshape(rows, N))
        Wc, cm1, cm2, nc = R.clip_adam(Wc, gc, cm1, cm2, step, lr_critic, max_norm)
        a = actor_grads(kind, Wa, xr, actr, logp_old, adv.reshape(rows, N), clip_eps, ent_coef / rows)
        Wa, am1, am2, na = R.clip_adam(Wa, a["grad"], am1, am2, step, lr_actor, max_norm)
        out["critic_loss"].append(lc); out["critic_norm"].append(nc); out["critic_grad"].append(gc)
        out["actor_loss"].append(a["loss"]); out["actor_norm"].append(na); out["actor"].append(a); out["entropy"].append(a["entropy"])
    out.update(critic_post=Wc, actor_post=Wa, state=dict(cm1=cm1, cm2=cm2, am1=am1, am2=am2, step=step))
    return out


def sa2c_train(kind, Wa, Wc, x, reward, done, act, nbr, gamma, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0, state=None,
               ent_coef=0.0, a2c_grads=None):
    """`learner_ref.sa2c_train` whose actor loss carries -ent_coef x the mean row entropy (the likelihood term keeps its
    1 / E).  Adds ``entropy`` [N] and ``actor_mag`` to the returned dict.  ``a2c_grads``: another statement of this module's
    function of that name (tests/saturation_ref.py: the heads written without cancellation)."""
    T, E, N = reward.shape
    rows = T * E
    out = R.sa2c_train(kind, Wa, Wc, x, reward, done, act, nbr, gamma, lr_actor, lr_critic, max_norm, state)
    if state is None:
        zeros = lambda W: [torch.zeros_like(w, dtype=torch.float64) for w in W]
        state = dict(am1=zeros(Wa), am2=zeros(Wa), step=0)
    xr = x.reshape(rows, N, -1).double()
    a = (a2c_grads or globals()["a2c_grads"])(kind, Wa, xr, 1.0 / E, act.reshape(rows, N, 2), out["w"].reshape(rows, N), ent_coef / rows)
    Wa2, am1, am2, na = R.clip_adam(Wa, a["grad"], state["am1"], state["am2"], state["step"] + 1, lr_actor, max_norm)
    out["state"].update(am1=am1, am2=am2)
    out.update(actor_grad=a["grad"], actor_mag=a["mag"], actor_loss=a["loss"], actor_norm=na, actor_post=Wa2, entropy=a["entropy"])
    return out
