#!/usr/bin/env python3
"""Generate tests/golden/safety_n5.npz from the REFERENCE's own `drones`: three N = 5 episodes with, for every step, what the
reference stores (``new_z``, ``Ni``, ``finished``, ``n_collisions``) and its own clipped distance matrix ``d_ij``
(`distance_data`), plus the per-episode safety tables derived from ``d_ij`` and ``state`` -- NOT from z.

Runs only where the reference is available (like gen_eval_golden.py, with gen_golden.py's import-time shims).  The .npz it writes
is committed and is what the safety tests read.  Data only.  Episodes (prefix of their arrays):
  p_   `proportional_control`, c = 2, deltas = 1.0: ends by arrival, the agents enter their goal disks at different steps
  r_   seeded random actions, c = 2, deltas = 1.0, run to the time limit; the seed is one whose episode has a collision
  s_   short c = 5 episode (simplify_zstate=False), deltas = 0.25, small random actions, started 12 steps before the time limit
Per episode: new_z [T,5,(k+1)c], Ni [T,5,k+1] (-1 = no neighbour), finished [T], n_coll [T], d_ij [T,5,5], pos [T,5,2] (after the
step), deltas, radius, xF, and the expected tables
  min_clearance [5]    min over steps of min(min_{j != i} d_ij[i,j], deltas[i])     goal_dist_final [5]   |xF_i - x_i| at the end
  arrive_step [5]      smallest t + 1 with |xF_i - x_i| <= 0.2 after step t, -1     ep_len, ep_arrived, ep_collisions
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden  # noqa: E402  (the reference's import-time shims; puts the reference on sys.path)

N, K, DONE_RADIUS, MARGIN = 5, 2, 0.2, 1e-5
SEEDS = dict(p=21, r=None, s=5)        # r: the first seed from 1 up whose random episode has a collision (recorded in the file)


def record(env, policy, rng):
    import drone_env
    rec = {kk: [] for kk in ("new_z", "Ni", "finished", "n_coll", "d_ij", "pos")}
    xF = env.end_points.reshape(N, 2)
    finished = False
    while not finished:
        actions = drone_env.proportional_control(env.state, env) if policy == "proportional" else \
            [a for a in rng.uniform(-1, 1, (N, 2)) * (1.0 if policy == "random" else 0.1)]
        state, new_z, _, n_collisions, finished, _ = env.step(actions)
        d_ij, _, _, _ = env.distance_data(state, env.deltas, env.d_safety)
        rec["new_z"].append(np.stack([np.asarray(z, np.float64).flatten() for z in new_z]))
        rec["Ni"].append(gen_golden.pack_ni(env.Ni, K + 1))
        rec["finished"].append(bool(finished)); rec["n_coll"].append(int(n_collisions))
        rec["d_ij"].append(d_ij.copy()); rec["pos"].append(state[:, 0:2].copy())
    out = {kk: np.stack(v) for kk, v in rec.items()}
    T = len(out["finished"])
    off = ~np.eye(N, dtype=bool)
    assert not (out["d_ij"][:, off] == 0).any() and not (out["d_ij"][:, off] == -1e-6).any()      # (drone_env.py:319-320 never fired)
    nearest = np.where(off[None], out["d_ij"], np.inf).min(2)                                     # [T,N]
    err = np.linalg.norm(xF[None] - out["pos"], axis=2)                                           # [T,N], drone_env.py:249
    assert np.abs(err - DONE_RADIUS).min() > MARGIN, "a goal distance within 1e-5 of the disk's radius: change the seed"
    inside = err <= DONE_RADIUS
    out.update(deltas=np.asarray(env.deltas, np.float64), radius=np.asarray(env.drone_radius, np.float64), xF=xF,
               min_clearance=np.minimum(nearest, env.deltas[None]).min(0), goal_dist_final=err[-1],
               arrive_step=np.where(inside.any(0), inside.argmax(0) + 1, -1).astype(np.int32), ep_len=np.int32(T),
               ep_arrived=np.bool_(inside[-1].all()), ep_collisions=np.int64(out["n_coll"].sum()))
    return out


def episode(policy, seed, simplify, deltas, start_t=0):
    random.seed(seed); np.random.seed(seed)
    env = gen_golden.quiet_env(n_agents=N, n_obstacles=0, grid=[5, 5], end_formation="O", k_closest=K, deltas=np.ones(N) * deltas,
                               simplify_zstate=simplify)
    env.internal_t = start_t
    return record(env, policy, np.random.default_rng(seed))


def main():
    import drone_env
    p = episode("proportional", SEEDS["p"], True, 1.0)
    seed_r = next(s for s in range(1, 400) if episode("random", s, True, 1.0)["ep_collisions"] > 0)
    r = episode("random", seed_r, True, 1.0)
    s = episode("small", SEEDS["s"], False, 0.25, start_t=drone_env.max_time_steps - 12)
    eps = dict(p=p, r=r, s=s)
    # what the recorded episodes must contain between them (if a seed does not give these, change the seed, not the assertion)
    assert p["ep_arrived"] and p["ep_len"] < drone_env.max_time_steps, "an arrival end"
    assert r["ep_len"] == drone_env.max_time_steps and not r["ep_arrived"], "a time-limit end"
    assert s["ep_len"] == 12 and s["new_z"].shape[2] == 5 * (K + 1)
    assert any((e["n_coll"] > 0).any() for e in eps.values()), "a step with a collision"
    assert any((e["Ni"][:, :, 1] < 0).all(0).any() for e in eps.values()), "an agent whose slot 1 is a ghost for a whole episode"
    assert any(((e["arrive_step"] > 0) & (e["arrive_step"] < e["ep_len"])).any() for e in eps.values()), "an early arrival"
    for e in eps.values():                                   # a collision is a negative clearance, and the other way round
        assert (e["ep_collisions"] > 0) == (e["min_clearance"].min() <= 0)
    data = {f"{a}_{kk}": v for a, e in eps.items() for kk, v in e.items()}
    data.update(seed_p=SEEDS["p"], seed_r=seed_r, seed_s=SEEDS["s"], N=N, k=K, done_radius=DONE_RADIUS,
                **{f"meta_{a}": b for a, b in gen_golden.META.items()})
    path = os.path.join(HERE, "safety_n5.npz")
    np.savez_compressed(path, **data)
    print(f"safety_n5: {os.path.getsize(path) / 1e3:.1f} kB; lengths {[int(e['ep_len']) for e in eps.values()]}, random seed {seed_r}, "
          f"collisions {[int(e['ep_collisions']) for e in eps.values()]}, arrive {p['arrive_step'].tolist()}, "
          f"min clearance {[round(float(e['min_clearance'].min()), 4) for e in eps.values()]}")


if __name__ == "__main__":
    main()
