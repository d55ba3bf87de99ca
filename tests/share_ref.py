"""Float64 torch restatement of parameter sharing across agent groups (include/dronesim.h: dronesim_adam_step_shared,
dronesim_kl_gate_shared): the checker of tests/test_share_host.py and tests/test_gpu_share.py (test infrastructure; CPU tensors).
Built on tests/learner_ref.py and tests/ppo_ref.py (with the KL estimate of tests/ppo_guard_ref.py and the row permutation of
tests/minibatch_ref.py), same layouts: weights stacked [N, ...], rows x [R, N, d_in].

  sharing map    every agent has a group; a group's members hold ONE network, its LEADER is the lowest-numbered member
  gradient       the mean of the members' per-agent gradients (= one network on the pooled rows, row scale 1 / (|G| rows))
  update         `learner_ref.clip_adam` ONCE PER GROUP on that mean: one norm, one Adam state; every member gets the result
  gate           a group stops when the mean of its members' kl is not <= target_kl; all its members together"""
import numpy as np
import torch

from tests import learner_ref as R
from tests import minibatch_ref as MB
from tests import ppo_guard_ref as GR
from tests import ppo_ref as P


def groups_of(share, n):
    """``(group_of [N], groups)`` of a map, written from the rules of include/dronesim.h independently of
    `learner.agent_groups`: groups are lists of ascending members, ordered by their first (lowest) member."""
    ids = [0] * n if isinstance(share, str) else list(range(n)) if share is None else [int(v) for v in share]
    groups = []
    for v in sorted(set(ids), key=ids.index):
        groups.append([i for i in range(n) if ids[i] == v])
    group_of = [next(g for g, mem in enumerate(groups) if i in mem) for i in range(n)]
    return group_of, groups


def leaders(groups):
    return torch.tensor([g[0] for g in groups])


def group_mean_f32(g, groups):
    """The kernel's prescription on one float32 tensor g [N, ...]: per group float64 partial sums in ascending member order
    starting from the first member's value, divided by |G|, rounded ONCE to float32.  Returns [n_groups, ...] float32."""
    out = []
    for mem in groups:
        s = g[mem[0]].double().clone()
        for i in mem[1:]:
            s += g[i].double()
        out.append((s / float(len(mem))).float())
    return torch.stack(out)


def group_mean(g, groups):
    """The float64 mean of the members' per-agent gradients, [n_groups, ...]."""
    return torch.stack([g[mem].double().mean(0) for mem in groups])


def clip_adam(group_of, groups, W, g, m1, m2, step, lr, max_norm=10.0, **kw):
    """`learner_ref.clip_adam` once per group on the mean gradient.  W, g [N, ...] (the members of a group hold equal W); the
    moments m1, m2 [n_groups, ...], one per group.  Returns (new W [N, ...], m1, m2, norms [N]: the group's in every slot)."""
    lead, of = leaders(groups), torch.tensor(group_of)
    Wg, M1, M2, norm = R.clip_adam([w[lead] for w in W], [group_mean(t, groups) for t in g], m1, m2, step, lr, max_norm, **kw)
    return [w[of] for w in Wg], M1, M2, norm[of]


def zeros(W, groups):
    return [torch.zeros(len(groups), *w.shape[1:], dtype=torch.float64) for w in W]


def sa2c_train(share, kind, Wa, Wc, x, reward, done, act, nbr, gamma, lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0):
    """`learner_ref.sa2c_train` from fresh optimisers with both networks under the map ``share``."""
    T, E, N = reward.shape
    group_of, groups = groups_of(share, N)
    xr = x.reshape(T * E, N, -1).double()
    G = R.returns(reward, done, gamma)
    gc, lc = R.grads(0, Wc, xr, 1.0 / (T * E), target=G.reshape(T * E, N))
    Wc2, cm1, cm2, nc = clip_adam(group_of, groups, Wc, gc, zeros(Wc, groups), zeros(Wc, groups), 1, lr_critic, max_norm)
    V = R.forward(Wc2, xr)[2][..., 0].transpose(0, 1).reshape(T, E, N)
    w = R.advantage(G, V, nbr, done, gamma)
    ga, la = R.grads(kind, Wa, xr, 1.0 / E, act=act.reshape(T * E, N, 2), weight=w.reshape(T * E, N))
    Wa2, am1, am2, na = clip_adam(group_of, groups, Wa, ga, zeros(Wa, groups), zeros(Wa, groups), 1, lr_actor, max_norm)
    of = torch.tensor(group_of)
    return dict(critic_loss=lc, critic_norm=nc, critic_post=Wc2, actor_loss=la, actor_norm=na, actor_post=Wa2, G=G, w=w,
                cm2=[t[of] for t in cm2], am2=[t[of] for t in am2])


def ppo_train(share, kind, Wa, Wc, x, reward, done, act, nbr, gamma, epochs=10, minibatches=1, shuffle_seed=0, clip_eps=0.2,
              lr_actor=1e-3, lr_critic=1e-3, max_norm=10.0, baseline="once", target_kl=None):
    """`ppo_ref.ppo_train` from fresh optimisers under the map ``share``, whole-window or in shuffled minibatches (the loop of
    `ppo_guard_ref.ppo_train`), with the GROUP gate: per actor step all agents' gradients and kl are formed, a group still
    active stops when the mean of its members' kl is not <= target_kl, and Adam runs for the groups still active.

    Returns a dict; per-step lists over the ``epochs x minibatches`` steps: critic_loss, critic_norm, actor_loss, actor_norm,
    actor (the `ppo_ref.actor_grads` dict), kl [N] (each agent's own), group_kl [n_groups], active ((computed, stepped) [N]);
    and actor_steps [N], the post-update weights and second moments expanded to [N, ...]."""
    T, E, N = reward.shape
    rows, K = T * E, int(minibatches)
    assert rows % K == 0
    M = rows // K
    group_of, groups = groups_of(share, N)
    of = torch.tensor(group_of)
    Wa, Wc = [w.double() for w in Wa], [w.double() for w in Wc]
    xr = x.reshape(rows, N, -1).double()
    actr = act.reshape(rows, N, 2).double()
    G = R.returns(reward, done, gamma)
    V = R.forward(Wc, xr)[2][..., 0].transpose(0, 1).reshape(T, E, N)
    logp_old = P.logp(kind, Wa, xr, actr).detach()
    adv = P.advantage(G, V, nbr, baseline)
    Gr, advr = G.reshape(rows, N), adv.reshape(rows, N)
    cm1, cm2, am1, am2 = (zeros(W, groups) for W in (Wc, Wc, Wa, Wa))
    keys = ("critic_loss", "critic_norm", "actor_loss", "actor_norm", "actor", "kl", "group_kl", "active")
    out = dict(G=G, V=V, adv=adv, logp_old=logp_old.reshape(T, E, N), perms=[], **{k: [] for k in keys})
    active = torch.ones(len(groups), dtype=torch.bool)
    taken = torch.zeros(len(groups), dtype=torch.long)
    sel = lambda mask, new, old: [torch.where(mask.view(-1, *([1] * (n.dim() - 1))), n, o) for n, o in zip(new, old)]
    step = 0
    for ep in range(epochs):
        if K > 1:
            perm = MB.row_permutation(rows, shuffle_seed, step)
            assert np.array_equal(np.sort(perm), np.arange(rows))
            out["perms"].append(perm)
        for b in range(K):
            idx = torch.arange(rows) if K == 1 else torch.as_tensor(perm[b * M:(b + 1) * M])
            step += 1
            gc, lc = R.grads(0, Wc, xr[idx], 1.0 / M, target=Gr[idx])
            Wc, cm1, cm2, nc = clip_adam(group_of, groups, Wc, gc, cm1, cm2, step, lr_critic, max_norm)
            a = P.actor_grads(kind, Wa, xr[idx], actr[idx], logp_old[idx], advr[idx], clip_eps)
            kl = GR.kl_estimate(a["logp"], logp_old[idx])
            group_kl = torch.stack([kl[mem].mean() for mem in groups])
            computed = active.clone()
            if target_kl is not None:
                active = active & (group_kl <= target_kl)
            taken = taken + active.long()
            # (an active group has taken every earlier step of the call, so one step count serves them all)
            Wn, n1, n2, na = clip_adam(group_of, groups, Wa, a["grad"], am1, am2, step, lr_actor, max_norm)
            Wa, am1, am2 = sel(active[of], Wn, Wa), sel(active, n1, am1), sel(active, n2, am2)
            for k, v in zip(keys, (lc, nc, a["loss"], na, a, kl, group_kl, (computed[of], active[of].clone()))):
                out[k].append(v)
    out.update(critic_post=Wc, actor_post=Wa, actor_steps=taken[of], cm2=[t[of] for t in cm2], am2=[t[of] for t in am2], steps=step)
    return out
