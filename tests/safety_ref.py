"""NumPy / float64 restatement of `dronesim_episode_safety`'s contract (include/dronesim.h), as plain loops over (e, i, t) --
test infrastructure, no GPU needed.  tests/test_safety_host.py checks it against the reference's own distance matrices
(tests/golden/safety_n5.npz) and against a second, vectorised formulation."""
import numpy as np

TABLES = ("ep_len", "min_clearance", "goal_dist_final", "arrive_step", "ep_min_clearance", "ep_goal_dist_max", "ep_arrived")


def episode_safety(z, nbr, done, radius, delta, done_radius, z_final=None, nbr_final=None):
    """The first episode of every env of a window: z [T,E,N,k1 c], nbr [T,E,N,k1], done [T,E], radius, delta [N]; z_final /
    nbr_final: the terminal observations (both or neither).  Returns the tables of `TABLES` plus ``near [E,N]``: the (env,
    agent) entries with a goal distance within 4 float32 ulps of ``done_radius`` at some step of the episode -- there a float32
    evaluation may land on the other side of the test."""
    z, nbr = np.asarray(z, np.float64), np.asarray(nbr, np.int64)
    T, E, N, k1 = nbr.shape
    c = z.shape[3] // k1
    assert z.shape == (T, E, N, k1 * c) and c in (2, 5) and k1 >= 2 and (z_final is None) == (nbr_final is None)
    done = np.asarray(done).reshape(T, E) != 0
    radius, delta = np.asarray(radius, np.float64), np.asarray(delta, np.float64)
    done_radius = float(done_radius)
    band = 4.0 * float(np.spacing(np.float32(done_radius)))
    nan = float("nan")
    out = dict(ep_len=np.zeros(E, np.int32), min_clearance=np.full((E, N), nan), goal_dist_final=np.full((E, N), nan),
               arrive_step=np.full((E, N), -1, np.int32), ep_min_clearance=np.full(E, nan), ep_goal_dist_max=np.full(E, nan),
               ep_arrived=np.zeros(E, np.uint8), near=np.zeros((E, N), bool))
    for e in range(E):
        L = 0
        for t in range(T):
            if done[t, e]:
                L = t + 1
                break
        out["ep_len"][e] = L
        if L == 0:
            continue
        for i in range(N):
            m, goal, arrive = nan, nan, -1
            for t in range(L):
                final = t == L - 1 and z_final is not None
                rec = np.asarray(z_final[t, e, i], np.float64) if final else z[t, e, i]
                j = int(nbr_final[t, e, i, 1]) if final else int(nbr[t, e, i, 1])
                goal = np.sqrt(rec[1] * rec[1] + rec[0] * rec[0])
                if 0 <= j < N:
                    clr = np.minimum(np.sqrt(rec[c + 1] * rec[c + 1] + rec[c] * rec[c]) - radius[i] - radius[j], delta[i])
                else:
                    clr = delta[i]
                m = clr if t == 0 else np.minimum(m, clr)                    # (a NaN stays)
                if arrive < 0 and goal <= done_radius:
                    arrive = t + 1
                if abs(goal - done_radius) <= band:
                    out["near"][e, i] = True
            out["min_clearance"][e, i], out["goal_dist_final"][e, i], out["arrive_step"][e, i] = m, goal, arrive
        lo, hi, outside = out["min_clearance"][e, 0], out["goal_dist_final"][e, 0], False
        for i in range(N):
            lo, hi = np.minimum(lo, out["min_clearance"][e, i]), np.maximum(hi, out["goal_dist_final"][e, i])
            outside = outside or not out["goal_dist_final"][e, i] <= done_radius
        out["ep_min_clearance"][e], out["ep_goal_dist_max"][e], out["ep_arrived"][e] = lo, hi, 0 if outside else 1
    return out


def golden_window(fx, a, pad=3, dtype=np.float64):
    """Episode `a` of the fixture as a window of E = 1 with `pad` steps behind its end (they must not count)."""
    rng = np.random.default_rng(7)
    z, nbr = fx[f"{a}_new_z"], fx[f"{a}_Ni"]
    z = np.concatenate([z, rng.standard_normal((pad,) + z.shape[1:]) * 0.01])[:, None].astype(dtype)
    nbr = np.concatenate([nbr, np.zeros((pad,) + nbr.shape[1:], nbr.dtype)])[:, None].astype(np.int32)
    done = np.concatenate([fx[f"{a}_finished"], [False, True, False][:pad]]).astype(np.uint8)[:, None]
    return z, nbr, done


SLOT1 = ("valid", "ghost", "N", "large", "negative")


def synthetic_window(T, E, N, k1, c, seed, with_final=True):
    """A seeded float32 window with everything the kernel has to get right.  `done` cycles over the envs as in
    eval_ref.synthetic_window (none, at t = 0, only at T - 1, several, one random).  Row 0 straddles the goal disk (0.2; every third env ends inside it), row 1
    the contact distance; slot 1 is a valid id, -1, N, a large value or a negative one other than -1; radius and delta differ
    per agent; the terminal record of one episode has a NaN in row 0, the first record of another one a NaN in row 1."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((T, E, N, k1 * c)) * 0.3).astype(np.float32)
    z[..., 0:2] *= rng.choice([0.3, 1.0], (T, E, N, 1)).astype(np.float32)
    z[:, ::3, :, 0:2] *= np.float32(0.25)                    # every third env: (almost) everybody inside its goal disk
    nbr = rng.integers(0, N, (T, E, N, k1)).astype(np.int32)
    kind = rng.choice(len(SLOT1), (T, E, N), p=[0.6, 0.25, 0.05, 0.05, 0.05])
    nbr[..., 1] = np.select([kind == 1, kind == 2, kind == 3, kind == 4], [-1, N, 2 ** 30 + 5, -7], nbr[..., 1])
    done = np.zeros((T, E), np.uint8)
    for e in range(E):
        pat = (e + seed) % 5
        if pat == 1:
            done[0, e] = 1
        elif pat == 2:
            done[T - 1, e] = 1
        elif pat == 3:
            done[rng.integers(0, T, 3), e] = 1
            done[T - 1, e] = 1
        elif pat == 4:
            done[rng.integers(0, T), e] = 1
    w = dict(z=z, nbr=nbr, done=done, radius=rng.uniform(0.05, 0.15, N).astype(np.float32),
             delta=rng.uniform(0.3, 1.0, N).astype(np.float32), z_final=None, nbr_final=None)
    if with_final:
        w["z_final"] = (rng.standard_normal(z.shape) * 0.3).astype(np.float32)
        w["z_final"][:, ::3, :, 0:2] *= np.float32(0.25)
        w["nbr_final"] = np.where(rng.random(nbr.shape) < 0.3, -1, rng.integers(0, N, nbr.shape)).astype(np.int32)
    has = np.flatnonzero(done.any(0))
    for n, e in enumerate(has[:2]):                          # NaN offsets: row 0 of an env's terminal record, row 1 of another
        last = int(done[:, e].argmax())
        t = last if n == 0 else 0
        final = with_final and t == last
        (w["z_final"] if final else z)[t, e, N - 1, 0 if n == 0 else c] = np.nan
        if n == 1:                                           # (with a valid slot 1: the NaN counts)
            (w["nbr_final"] if final else nbr)[t, e, N - 1, 1] = 0
    return w
