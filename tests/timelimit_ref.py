"""Numpy restatement of the time-limit handling of the bootstrapped lambda-returns ("Time-limit ends"): the
classification of a stored window's episode ends, the ranking of the truncated ones, the demotion beyond M, the zero fill of
the gathered terminal observations, and the scan (float64).  The checker of the time-limit tests (test infrastructure)."""
import numpy as np


def outside(z_final, done_radius):
    """[T,E,N] bool: !(sqrt(zx^2 + zy^2) <= done_radius) with the agent's own offset (zx, zy) = the first two floats of its
    row, in float32 like the step kernel's test -- a non-finite offset is outside.  (The kernel forms the sum of squares as
    fma(zy, zy, zx zx); the plain float32 sum here can differ from it by an ulp, so the two verdicts may differ only for an
    agent within an ulp of the radius.)"""
    z = np.asarray(z_final, dtype=np.float32)
    zx, zy = z[..., 0], z[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        return ~(np.sqrt(zx * zx + zy * zy) <= np.float32(done_radius))


def episode_ends(done, z_final, done_radius, M):
    """done [T,E], z_final [T,E,N,d] -> (ends [T,E] u8, slot_t [M,E] i32, n_trunc [E] i32, z_trunc [M,E,N,d] f32)."""
    done, z = np.asarray(done), np.asarray(z_final, dtype=np.float32)
    T, E, N, d = z.shape
    assert done.shape == (T, E) and M >= 1
    some_outside = outside(z, done_radius).any(axis=2)
    ends = np.where(done != 0, np.where(some_outside, 2, 1), 0).astype(np.uint8)
    slot_t = np.full((M, E), -1, np.int32)
    n_trunc = np.zeros(E, np.int32)
    z_trunc = np.zeros((M, E, N, d), np.float32)
    for e in range(E):
        k = 0
        for t in range(T - 1, -1, -1):                      # ranked from the back of the window
            if ends[t, e] == 2:
                if k < M:
                    slot_t[k, e] = t
                    z_trunc[k, e] = z[t, e]
                else:
                    ends[t, e] = 1                          # demoted: nothing beyond the capacity is read or written
                k += 1
        n_trunc[e] = k                                      # (the count before the demotion)
    return ends, slot_t, n_trunc, z_trunc


def lambda_returns_ends(reward, V, ends, Vend, gamma, lam):
    """reward [T,E,N], V [T+1,E,N], ends [T,E] in {0, 1, 2}, Vend [M,E,N]; float64.  Backwards from Gn = V[T], k[e] = 0:
        ends = 0           G[t] = r[t] + gamma ((1 - lam) V[t+1] + lam Gn)
        ends = 1           G[t] = r[t]
        ends = 2, k < M    G[t] = r[t] + gamma Vend[k, e],  k += 1;      k >= M: as ends = 1
    Returns (G, A = G - V[:T])."""
    r, V, Vend = (np.asarray(a, dtype=np.float64) for a in (reward, V, Vend))
    ends = np.asarray(ends)
    T, E, N = r.shape
    M = Vend.shape[0]
    G = np.zeros_like(r)
    Gn = V[T].copy()
    k = np.zeros(E, np.int64)
    cols = np.arange(E)
    for t in range(T - 1, -1, -1):
        boot = r[t] + gamma * ((1 - lam) * V[t + 1] + lam * Gn)
        trunc = (ends[t] == 2) & (k < M)
        vend = Vend[np.minimum(k, M - 1), cols]              # [E,N]; only read where trunc
        g = np.where((ends[t] != 0)[:, None], r[t], boot)
        g = np.where(trunc[:, None], r[t] + gamma * vend, g)
        k = k + trunc
        G[t] = Gn = g
    return G, G - V[:T]
