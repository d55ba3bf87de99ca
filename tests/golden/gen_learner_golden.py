#!/usr/bin/env python3
"""Generate tests/golden/learner_n5.npz from the REFERENCE's own `SA2CAgents.train_NN` (SAC_agents.py:280-357).

Runs only where the reference is available (like gen_golden.py, with the same import-time shims); the .npz it writes is
committed and is what the learner tests read.  Data only: the reference's gradients, norms, losses and updated weights.

The experience buffer is rebuilt from the committed episode fixture episode_n5.npz (config C1: N = 5, E = 1, one
episode): z_state[t] = z0 for t = 0 and z[t-1] after, Ni from nbr_idx_pre, the stored actions, rewards and done flags.
Two updates of seeded networks, each ONE train_NN call:
  run "s": SA2CAgents(5, 6, 2, 0.99, 10) after torch.manual_seed(SEED_AGENTS)  (DiscreteSoftmaxNN(16) actors + CriticNN)
  run "g": the same agents rebuilt, actors replaced by NormalActorNN(6, 1e-3, 2) built after torch.manual_seed(SEED_GAUSS)
           (the alternative at SAC_agents.py:144)
The initial weights are reproducible without the reference (tests/learner_ref.py: reference_weights); their per-agent sums
are stored to check that.  Gradients are captured by wrapping torch.nn.utils.clip_grad_norm_ (pre-clip) together with the
norm it returns.  Stored, in the kernel's stacked layout (w [in, out]):
  c_* critic, s_* softmax actor, g_* Gaussian actor:
    {p}_grad_{w1..b3}    pre-clip gradient of agent REC            {p}_post_{w1,b1,b2,w3,b3}  post-update weights of agent REC
    {p}_post_w2_sub      post-update w2 of agent REC, flat elements 0, 7, 14, ...
    {p}_loss, {p}_norm   [5] losses and pre-clip norms of every agent
    {p}_init_sum_{name}  [5] float64 sums of every agent's initial tensors
  w                      [T, 5] actor-loss weights gamma^t / N sum_j (G_j - V_i) with the POST-update critic
"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_golden  # noqa: E402,F401  (the reference's import-time shims; puts the reference on sys.path)
import torch  # noqa: E402

from scalable_collision_avoidance_rl_amd.policies import stack_reference_modules  # noqa: E402

SEED_AGENTS, SEED_GAUSS, REC, W2_STRIDE = 11, 12, 2, 7
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


class GradNS:
    """A module-shaped view of a module's gradients (stack_reference_modules reads .weight / .bias by attribute name)."""
    def __init__(self, module):
        for name, child in module.named_children():
            if isinstance(child, torch.nn.Linear):
                setattr(self, name, type("L", (), {"weight": child.weight.grad.clone(), "bias": child.bias.grad.clone()})())


def stacked(modules, kind):
    return [t.double().numpy() for t in stack_reference_modules(modules, kind)[:6]]


def buffers_from_episode(fx, N):
    from utils import ExperienceBuffers
    buf = ExperienceBuffers(N)
    T = fx["act"].shape[0]
    for t in range(T):
        z = fx["z0"] if t == 0 else fx["z"][t - 1]
        Ni = [[int(j) for j in fx["nbr_idx_pre"][t, i] if j >= 0] for i in range(N)]
        buf.append([z[i] for i in range(N)], [fx["act"][t, i] for i in range(N)], fx["reward"][t],
                   [fx["z"][t][i] for i in range(N)], Ni, bool(fx["done"][t]))
    return buf


def run(fx, gaussian):
    from SAC_agents import SA2CAgents
    from utils import NormalActorNN
    N = int(fx["N"])
    torch.manual_seed(SEED_AGENTS)
    agents = SA2CAgents(N, 6, 2, 0.99, 10)
    if gaussian:
        torch.manual_seed(SEED_GAUSS)
        agents.actors = [NormalActorNN(6, lr=1e-3, dim_action=2) for _ in range(N)]
    akind = "normal_actor" if gaussian else "discrete_softmax"
    init_c, init_a = stacked(agents.criticsNN, "critic"), stacked(agents.actors, akind)
    critics0 = copy.deepcopy(agents.criticsNN)
    actors0 = copy.deepcopy(agents.actors)
    buf = buffers_from_episode(fx, N)

    captured = []
    orig = torch.nn.utils.clip_grad_norm_

    def wrapped(params, *a, **kw):
        params = list(params)
        grads = [p.grad.clone() for p in params]
        norm = orig(params, *a, **kw)
        captured.append((grads, float(norm)))
        return norm

    torch.nn.utils.clip_grad_norm_ = wrapped
    try:
        agents.train_NN(buf)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig
    assert len(captured) == 2 * N

    # gradients of agent REC in the stacked layout: load them as .grad of the modules and stack
    def grads_of(module, grads):
        m = copy.deepcopy(module)
        for p, g in zip(m.parameters(), grads):
            p.grad = g
        return GradNS(m)

    T = fx["act"].shape[0]
    rewards = fx["reward"]
    Gts = []
    for i in range(N):
        G = np.zeros(T); G[-1] = rewards[-1, i]
        for t in range(T - 2, -1, -1):
            G[t] = G[t + 1] * agents.discount + rewards[t, i]
        Gts.append(G)
    states = [torch.tensor(np.array([buf.buffers[i][t].z_state for t in range(T)]), dtype=torch.float32) for i in range(N)]
    closs = [float(torch.nn.functional.mse_loss(critics0[i](states[i]).squeeze(), torch.tensor(Gts[i], dtype=torch.float32)).detach())
             for i in range(N)]
    # actor-loss weights with the POST-update critic (SAC_agents.py:340-351), and the actor losses of the initial actors
    w = np.zeros((T, N))
    aloss = []
    for i in range(N):
        V = agents.criticsNN[i](states[i]).detach().numpy()[:, 0]
        tot = 0.0
        for t in range(T):
            adv = sum(Gts[j][t] - V[t] for j in buf.buffers[i][t].Ni)
            w[t, i] = 1 / N * agents.discount ** t * adv
            lp = actors0[i].log_p_of_a(buf.buffers[i][t].z_state, buf.buffers[i][t].action)
            tot += float(-lp.detach().squeeze() * w[t, i])
        aloss.append(tot)

    out = {}
    for p, kind, mods, mods0, init, losses, off in (("c", "critic", agents.criticsNN, critics0, init_c, closs, 0),
                                                    ("a", akind, agents.actors, actors0, init_a, aloss, N)):
        g = stacked([grads_of(mods0[REC], captured[off + REC][0])], kind)
        post = stacked([mods[REC]], kind)
        for name, gg, pp, ii in zip(NAMES, g, post, init):
            out[f"{p}_grad_{name}"] = gg[0].astype(np.float32)
            if name == "w2":
                out[f"{p}_post_w2_sub"] = pp[0].reshape(-1)[::W2_STRIDE].astype(np.float32)
            else:
                out[f"{p}_post_{name}"] = pp[0].astype(np.float32)
            out[f"{p}_init_sum_{name}"] = ii.reshape(N, -1).sum(1)
        out[f"{p}_loss"] = np.array(losses)
        out[f"{p}_norm"] = np.array([captured[off + i][1] for i in range(N)])
    out["w"] = w
    return out


def main():
    fx = dict(np.load(os.path.join(HERE, "episode_n5.npz")))
    s, g = run(fx, False), run(fx, True)
    for k in s:
        if k.startswith("c_"):
            assert np.array_equal(s[k], g[k]), k            # the critic update does not depend on the actor
    data = {k: v for k, v in s.items() if k.startswith("c_")}
    data.update({"s_" + k[2:]: v for k, v in s.items() if k.startswith("a_")})
    data.update({"g_" + k[2:]: v for k, v in g.items() if k.startswith("a_")})
    assert np.array_equal(s["w"], g["w"])
    data.update(w=s["w"], rec=REC, w2_stride=W2_STRIDE, seed_agents=SEED_AGENTS, seed_gauss=SEED_GAUSS,
                **{f"meta_{a}": b for a, b in gen_golden.META.items()})
    path = os.path.join(HERE, "learner_n5.npz")
    np.savez_compressed(path, **data)
    print(f"learner_n5: {os.path.getsize(path) / 1e6:.2f} MB; critic norms {data['c_norm']}, softmax {data['s_norm']}, "
          f"Gaussian {data['g_norm']}")


if __name__ == "__main__":
    main()
