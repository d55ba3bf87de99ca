"""Restatement of the obstacle columns and the obstacle cost (include/dronesim.h: the obstacle observe and reward entries) by plain
loops -- test infrastructure, no GPU needed.  The gap is the rule's ONE float32 expression restated in numpy float32, every
operation correctly rounded (the fused multiply-add by an exact float64 product, a float64 sum and its TwoSum error term, so the
one rounding to float32 is the right one): its bits are the kernels' bits, and so are the decisions taken on it (in range, hit,
order).  The logarithm and the sum of the cost are in float64.  The seeded generator the test files share is here as well; the
conditions it promises are asserted in tests/test_obstacle_obs_host.py on this restatement alone."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)                      # 2^-23: one ulp of a float32 in [1, 2)
HIT_COST = 9.99e3                                            # the reference's collision cost (drone_env.py:268-334)
F32 = np.float32


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a b + c) of float32 arrays with ONE rounding: the product of two float32 is exact in float64; the float64 sum s is
    off the exact sum by TwoSum's e; rounding s to float32 differs from rounding the exact sum only where s is exactly the
    midpoint of two neighbouring float32 -- there e decides."""
    a, b, c = (np.asarray(x, F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)
        f = s.astype(F32)
        other = np.nextafter(f, np.where(s > f.astype(np.float64), F32(np.inf), F32(-np.inf)).astype(F32))
        mid = (f.astype(np.float64) + other.astype(np.float64)) / 2 == s
        fix = mid & np.isfinite(s) & (e != 0) & (np.sign(e) == np.sign(other.astype(np.float64) - f.astype(np.float64)))
    return np.where(fix, other, f).astype(F32)


def gaps32(z, xF, radius, obstacles):
    """P [R,M,2] = o.xy - position and G [R,M] = (d - radius[i]) - o.r in float32, agent i = r % N: the kernels' bits."""
    z, xF, radius = np.asarray(z, F32), np.asarray(xF, F32), np.asarray(radius, F32)
    obs = np.asarray(obstacles, F32).reshape(-1, 3)
    R, N = z.shape[0], xF.shape[0]
    i = np.arange(R) % N
    with np.errstate(invalid="ignore", over="ignore"):
        pos = (z[:, :2] + xF[i]).astype(F32)
        P = (obs[None, :, :2] - pos[:, None, :]).astype(F32)
        d = np.sqrt(fma32(P[..., 1], P[..., 1], (P[..., 0] * P[..., 0]).astype(F32))).astype(F32)
        G = ((d - radius[i][:, None]).astype(F32) - obs[None, :, 2]).astype(F32)
    return P, G


def columns(z, xF, radius, sense, obstacles, m):
    """dict(x [R, d + 3m] float32, oid [R,m], n_in [R], G [R,M] float32): every record with its obstacle columns -- the discs
    with gap <= sense[i] (a NaN gap is not in range), the m smallest gaps, ties to the lower id; empty slots (0, 0, 0)."""
    z = np.asarray(z, F32)
    obs = np.asarray(obstacles, F32).reshape(-1, 3)
    P, G = gaps32(z, xF, radius, obs)
    R, d = z.shape
    N = len(radius)
    x = np.zeros((R, d + 3 * m), F32)
    x[:, :d] = z
    oid, n_in = np.full((R, m), -1, np.int64), np.zeros(R, np.int64)
    for r in range(R):
        s = F32(sense[r % N])
        listed = []
        for o in range(obs.shape[0]):
            if G[r, o] <= s:                                                       # (False for a NaN on either side)
                listed.append((G[r, o], o))
        listed.sort()                                                              # gap ascending, then id ascending
        n_in[r] = len(listed)
        for slot, (_, o) in enumerate(listed[:m]):
            x[r, d + 3 * slot:d + 3 * slot + 3] = (P[r, o, 0], P[r, o, 1], obs[o, 2])
            oid[r, slot] = o
    return dict(x=x, oid=oid, n_in=n_in, G=G)


def cost_terms(G, sense_r):
    """terms [R,M] float64 of the float32 gaps G [R,M] and the ranges sense_r [R]: 9.99e3 where gap <= 0, log(s / gap) where
    0 < gap <= s, 0 otherwise (NaN gap, NaN range, s <= 0 with a positive gap)."""
    R, M = G.shape
    terms = np.zeros((R, M))
    for r in range(R):
        s = float(sense_r[r])
        for o in range(M):
            g = float(G[r, o])
            if g <= 0:
                terms[r, o] = HIT_COST
            elif g <= s:
                terms[r, o] = np.log(s / g)
    return terms


def cost(z, xF, radius, sense, obstacles, weight):
    """dict(cost [R] float64 = weight sum of the terms, bound [R], terms [R,M], G): `bound` is the derived distance a float32
    evaluation may lie from `cost` -- per log term eps32 (|term| + 1) (one ulp of logf, plus the quotient's half ulp through a
    logarithm of unit relative slope; a hit term is exact), n eps32 sum|term| for the n additions of non-zero terms, all times
    the weight, plus the product's own rounding."""
    G = gaps32(z, xF, radius, obstacles)[1]
    R = G.shape[0]
    sense_r = np.asarray(sense, F32)[np.arange(R) % len(radius)]
    terms = cost_terms(G, sense_r)
    total = terms.sum(1)
    logs = (terms != 0) & (terms != HIT_COST)
    per_term = (EPS32 * (np.abs(terms) + 1.0) * logs).sum(1)
    n = (terms != 0).sum(1)
    bound = weight * (per_term + n * EPS32 * np.abs(terms).sum(1))
    bound = bound + EPS32 * (np.abs(weight * total) + bound)
    return dict(cost=weight * total, bound=bound, terms=terms, G=G)


def pair_term(d_i, d_ij, b):
    """The reference's pair term with a second agent in the disc's place: b log(d_i / d_ij) inside the Delta-neighbourhood
    (drone_env.py:268-334) -- `cost_terms` at gap = d_ij and range = d_i, times b."""
    return b * cost_terms(np.array([[d_ij]], F32), np.array([d_i], F32))[0, 0]


def shaped_reward(reward, z_post, z_final, done, xF, radius, sense, obstacles, weight):
    """dict(reward [T,E,N] float64, cost, bound): reward[t] - cost(observation after step t), that observation being z_final[t]
    where done[t] and z_final is given, z_post[t] otherwise."""
    z_post = np.asarray(z_post, F32)
    T, E, N, d = z_post.shape
    seen = z_post.copy()
    if z_final is not None:
        for t in range(T):
            for e in range(E):
                if done[t, e]:
                    seen[t, e] = np.asarray(z_final, F32)[t, e]
    c = cost(seen.reshape(T * E * N, d), xF, radius, sense, obstacles, weight)
    reward = np.asarray(reward, np.float64)
    value = reward - c["cost"].reshape(T, E, N)
    bound = c["bound"].reshape(T, E, N) + EPS32 * (np.abs(value) + c["bound"].reshape(T, E, N))
    return dict(reward=value, cost=c["cost"].reshape(T, E, N), bound=bound, cost_bound=c["bound"].reshape(T, E, N), seen=seen)


# ---- the generator ----------------------------------------------------------------------------------------------------------------
# (E, N, k, c, M, m) of tests/test_gpu_obstacle_obs.py with the path each one is there for
SHAPES = [
    ((3, 5, 2, 2, 7, 2), "the smallest: one ragged wave, d + 3m = 12 (16-byte stores with a scalar tail: 180 floats)"),
    ((70, 64, 2, 2, 16, 2), "18 workgroups, a ragged last wave (4480 records = 17 x 256 + 128)"),
    ((9, 6, 2, 5, 7, 2), "c = 5, k1 = 3: dword loads of row 0, d + 3m = 21 (records straddle the 16-byte stores)"),
    ((5, 7, 2, 2, 7, 1), "m = 1: d + 3m = 9"),
    ((5, 7, 3, 2, 7, 3), "m = 3, k1 = 4 (16-byte row-0 loads): d + 3m = 17"),
    ((5, 7, 2, 2, 7, 4), "m = 4: d + 3m = 18"),
    ((4, 5, 2, 2, 0, 2), "M = 0: empty lists, cost 0"),
    ((2, 37, 1, 2, 1024, 4), "M = 1024: the full 12 KB list"),
]
SPECIAL = dict(touch=0, at_range=1, above_range=2, no_range=3, nan=4)              # env 0's agents (N >= 5 and M >= 1)


def case(E, N, k, c, M, m, seed=0, like=None):
    """Seeded float32 inputs: dict(z [E,N,(k+1)c], xF, radius, sense, obstacles [M,3]); `like`: an earlier case whose goals, radii,
    ranges and discs these records share.  The discs lie in [0, 3]^2 (radii 0.05 ..
    0.3), two records in three stand in that square ("crowded": with M >= 7 several discs are in range, at gaps of both signs),
    the third in [6, 9]^2 (nothing in range); ranges in [0.8, 1.6].  Where N >= 5 and M >= 1 the first five agents have dyadic
    goals, radius 0.125 and disc 0 = (1.5, 1.5, 0.375), and env 0 holds the hand-placed records of SPECIAL:
      touch        (1.5, 1.0): d = 0.5, gap 0 bit for bit -- a hit, listed
      at_range     (1.5, 0.0), range 1: d = 1.5, gap = 1 = the range bit for bit -- listed, log(1) = 0
      above_range  the same place, range the float32 below 1: the gap is one float32 above the range -- not listed, 0
      no_range     (1.5, 1.75), range 0: d = 0.25, gap -0.25 <= 0 -- a hit (and listed: gap <= range); every positive gap gives 0
      nan          x = NaN: empty slots, cost 0"""
    rng = np.random.default_rng(52361 + 7919 * seed + 131 * E + 17 * N + 5 * k + c + 3 * M + m)
    k1 = k + 1
    d = k1 * c
    xF = rng.uniform(0.0, 5.0, (N, 2)).astype(F32)
    radius = rng.uniform(0.05, 0.2, N).astype(F32)
    sense = rng.uniform(0.8, 1.6, N).astype(F32)
    obs = np.concatenate([rng.uniform(0.0, 3.0, (M, 2)), rng.uniform(0.05, 0.3, (M, 1))], 1).astype(F32)
    special = N >= 5 and M >= 1
    if like is not None:                                     # other records of the same scene
        xF, radius, sense, obs = like["xF"], like["radius"], like["sense"], like["obstacles"]
    elif special:
        xF[:5] = [[0.5, 0.5], [3.0, 1.0], [2.0, 2.5], [1.0, 3.0], [4.0, 4.0]]
        radius[:5] = 0.125
        obs[0] = (1.5, 1.5, 0.375)
        sense[SPECIAL["at_range"]] = 1.0
        sense[SPECIAL["above_range"]] = np.nextafter(F32(1.0), F32(0.0))
        sense[SPECIAL["no_range"]] = 0.0
    z = (rng.standard_normal((E, N, d)) * 0.3).astype(F32)
    far = rng.random((E, N)) < 1.0 / 3.0
    pos = np.where(far[..., None], rng.uniform(6.0, 9.0, (E, N, 2)), rng.uniform(0.0, 3.0, (E, N, 2))).astype(F32)
    z[..., :2] = pos - xF[None]
    if special:
        for name, p in (("touch", (1.5, 1.0)), ("at_range", (1.5, 0.0)), ("above_range", (1.5, 0.0)), ("no_range", (1.5, 1.75)),
                        ("nan", (np.nan, 2.0))):
            i = SPECIAL[name]
            z[0, i, :2] = np.array(p, F32) - xF[i]
    return dict(z=z, xF=xF, radius=radius, sense=sense, obstacles=obs, special=special)


WINDOW = dict(T=6, E=7, N=5, k=2, c=2, M=7)
# the ends of env e: none | the first slot | the last slot | two adjacent | every slot | one in the middle | first and last
WINDOW_ENDS = [[], [0], [5], [2, 3], [0, 1, 2, 3, 4, 5], [3], [0, 5]]


def window(seed=0):
    """A stored window for the reward entry: the ring z_all [T+1,E,N,d] and z_final [T,E,N,d] are `case` records (other
    positions in z_final), done [T,E] per env as WINDOW_ENDS, reward [T,E,N] in [-3, 0].  The hand-placed records of `case` sit
    in ring slot 1 of env 0 (the observation after step 0) and in z_final[0] of env 1 (an end at the first slot)."""
    T, E, N, k, c, M = (WINDOW[n] for n in ("T", "E", "N", "k", "c", "M"))
    ring = case((T + 1) * E, N, k, c, M, 2, seed=seed)
    fin = case(T * E, N, k, c, M, 2, seed=seed + 1, like=ring)
    d = (k + 1) * c
    z_all = ring["z"].reshape(T + 1, E, N, d).copy()
    z_all[[0, 1], 0] = z_all[[1, 0], 0]                                            # `case` planted env 0 of its first row
    z_final = fin["z"].reshape(T, E, N, d).copy()
    z_final[0, [0, 1]] = z_final[0, [1, 0]]
    done = np.zeros((T, E), np.uint8)
    for e, ends in enumerate(WINDOW_ENDS):
        done[ends, e] = 1
    rng = np.random.default_rng(977 + seed)
    reward = rng.uniform(-3.0, 0.0, (T, E, N)).astype(F32)
    return dict(ring, z_all=z_all, z_final=z_final, done=done, reward=reward)
