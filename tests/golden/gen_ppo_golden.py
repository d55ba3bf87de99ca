#!/usr/bin/env python3
"""Generate tests/golden/ppo_n5.npz from the part of the REFERENCE's `SPPOAgents` (SAC_agents.py:410-573) that runs.

Runs only where the reference is available (like gen_learner_golden.py, with the same import-time shims); the .npz it
writes is committed and is what the PPO tests read.  Data only.

`SPPOAgents.__init__` raises (it builds `NormalActorNN` without the required ``lr``) and `train` reads ``Qjsum`` before it
is assigned, so no whole update can be recorded.  What does run is ``probability_of_ai``: a bare instance
(``SPPOAgents.__new__``, attributes set by hand) gets ``actorsNN`` = N x ``NormalActorNN(6, 1e-3, 2)`` built after
``torch.manual_seed(SEED_GAUSS)`` -- the networks of gen_learner_golden.py's run "g", reproducible without the reference
(tests/learner_ref.py: reference_weights) -- converted to float64, and ITS method is called on the states and actions of the
committed episode fixture episode_n5.npz (z_state[t] = z0 for t = 0 and z[t-1] after).  Stored:
  p_old      [T, 5] float64   probability_of_ai(states_i, actions_i, i)            (:494, :558-573)
  G          [T, 5] float64   the returns of :476-481, by this file's own loop
  Q          [T, 5] float64   the neighbour sum of :498-501 over nbr_idx_pre (-1 slots skipped), by this file's own loop
  init_sum_{w1..b3}  [5]      float64 sums of every actor's initial tensors (kernel layout)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_golden  # noqa: E402,F401  (the reference's import-time shims; puts the reference on sys.path)
import torch  # noqa: E402

from scalable_collision_avoidance_rl_amd.policies import stack_reference_modules  # noqa: E402

SEED_GAUSS, GAMMA = 12, 0.99
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def main():
    from SAC_agents import SPPOAgents
    from utils import NormalActorNN
    fx = dict(np.load(os.path.join(HERE, "episode_n5.npz")))
    N, T = int(fx["N"]), fx["act"].shape[0]
    agents = SPPOAgents.__new__(SPPOAgents)
    agents.n_agents, agents.dim_local_state, agents.dim_local_action = N, 6, 2
    agents.discount, agents.epochs, agents.epsilon = GAMMA, 10, 0.2
    torch.manual_seed(SEED_GAUSS)
    agents.actorsNN = [NormalActorNN(6, 1e-3, 2) for _ in range(N)]
    init = [t.double().numpy() for t in stack_reference_modules(agents.actorsNN, "normal_actor")[:6]]
    for a in agents.actorsNN:
        a.double()

    states = np.concatenate([fx["z0"][None], fx["z"][:-1]]).reshape(T, N, 6)
    p_old = np.zeros((T, N))
    for i in range(N):
        s = torch.tensor(states[:, i], dtype=torch.float64)
        a = torch.tensor(fx["act"][:, i], dtype=torch.float64)
        p_old[:, i] = agents.probability_of_ai(s, a, i).detach().numpy()

    G = np.zeros((T, N))
    G[-1] = fx["reward"][-1]
    for t in range(T - 2, -1, -1):
        G[t] = G[t + 1] * GAMMA + fx["reward"][t]
    Q = np.zeros((T, N))
    for i in range(N):
        for t in range(T):
            for j in fx["nbr_idx_pre"][t, i]:
                if j >= 0:
                    Q[t, i] += G[t, int(j)]

    data = dict(p_old=p_old, G=G, Q=Q, gamma=GAMMA, seed_gauss=SEED_GAUSS,
                **{f"init_sum_{n}": w.reshape(N, -1).sum(1) for n, w in zip(NAMES, init)},
                **{f"meta_{a}": b for a, b in gen_golden.META.items()})
    path = os.path.join(HERE, "ppo_n5.npz")
    np.savez_compressed(path, **data)
    print(f"ppo_n5: {os.path.getsize(path) / 1e3:.1f} kB; p_old in [{p_old.min():.3e}, {p_old.max():.3e}], "
          f"|Q| max {np.abs(Q).max():.3f}")


if __name__ == "__main__":
    main()
