"""Float64 restatement of the action shield (include/dronesim.h: dronesim_action_shield) by BRUTE FORCE, sharing nothing with the
kernel's incremental solve: the projection of u onto an intersection of half-planes is u itself, or its projection onto one
of the lines, or a vertex of two lines -- list all of them, keep the feasible ones, take the closest.  Also the rule's closed
loop in float64 (single integrator, proportional control, lattice starts) that shows the shapes of the GPU tests are meaningful,
and the seeded record generator both test files share."""
import numpy as np

M_BOX = 4
BOX = np.array([[1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])
EPS32 = 2.0 ** -24


def constraints(z, nbr, radius, rate, margin, u_max, dt, c):
    """The half-planes of every record, in the rule's order.  z [R, k1 c] (any float), nbr [R, k1] int, agent ids i = r % N with
    N = len(radius).  Returns A [R, 4 + k, 2], B [R, 4 + k] float64 and on [R, 4 + k] bool (skipped slots: A = 0, B = +inf)."""
    z, radius = np.asarray(z, np.float64), np.asarray(radius, np.float64)
    nbr = np.asarray(nbr, np.int64)
    R, k1 = nbr.shape
    N = radius.shape[0]
    i = np.arange(R) % N
    rows = z.reshape(R, k1, c)
    A = np.zeros((R, M_BOX + k1 - 1, 2))
    B = np.full((R, M_BOX + k1 - 1), np.inf)
    on = np.zeros((R, M_BOX + k1 - 1), bool)
    A[:, :M_BOX], B[:, :M_BOX], on[:, :M_BOX] = BOX, float(u_max), True
    for s in range(1, k1):
        j, p = nbr[:, s], rows[:, s, :2]
        with np.errstate(invalid="ignore", over="ignore"):
            d = np.sqrt((p * p).sum(1))
        ok = (j >= 0) & (j < N) & (j != i) & np.isfinite(d) & (d > 0)
        dd = np.where(ok, d, 1.0)
        g = dd - radius[i] - radius[np.where(ok, j, 0)] - margin
        A[:, M_BOX + s - 1] = np.where(ok[:, None], np.where(ok[:, None], p, 0.0) / dd[:, None], 0.0)
        B[:, M_BOX + s - 1] = np.where(ok, rate * np.maximum(g, 0.0) / dt, np.inf)
        on[:, M_BOX + s - 1] = ok
    return A, B, on


def project(u, A, B, on, feas_tol=1e-12):
    """u* [R, 2] float64: the feasible candidate closest to u among u, its projection onto every line and every pairwise vertex.
    Rows with a non-finite u come back unchanged."""
    u = np.asarray(u, np.float64)
    R, M = B.shape
    fin = np.isfinite(u).all(1)
    u0 = np.where(fin[:, None], u, 0.0)
    Bf = np.where(np.isfinite(B), B, 0.0)
    line_ok = on & np.isfinite(B)
    cands, valid = [u0[:, None, :]], [np.ones((R, 1), bool)]
    # projection onto line m: u - (a.u - b) a   (|a| = 1)
    r = (A * u0[:, None, :]).sum(2) - Bf
    cands.append(u0[:, None, :] - r[:, :, None] * A)
    valid.append(line_ok)
    ii, jj = np.triu_indices(M, 1)
    a1, a2, b1, b2 = A[:, ii], A[:, jj], Bf[:, ii], Bf[:, jj]
    det = a1[..., 0] * a2[..., 1] - a1[..., 1] * a2[..., 0]
    okv = line_ok[:, ii] & line_ok[:, jj] & (np.abs(det) > 1e-9)
    sd = np.where(okv, det, 1.0)
    vx = (b1 * a2[..., 1] - b2 * a1[..., 1]) / sd
    vy = (a1[..., 0] * b2 - a2[..., 0] * b1) / sd
    cands.append(np.stack([vx, vy], 2))
    valid.append(okv)
    X = np.concatenate(cands, 1)                                                   # [R, 1 + M + M (M - 1) / 2, 2]
    V = np.concatenate(valid, 1)
    scale = 1.0 + np.abs(u0).max(1) + np.where(np.isfinite(B), np.abs(B), 0.0).max(1)
    slack = (X[:, :, None, :] * A[:, None, :, :]).sum(3) - B[:, None, :]           # [R, cand, M]
    feas = V & (slack <= feas_tol * scale[:, None, None]).all(2)
    dist = np.where(feas, np.sqrt(((X - u0[:, None, :]) ** 2).sum(2)), np.inf)
    best = dist.argmin(1)
    assert np.isfinite(dist[np.arange(R), best]).all(), "no feasible candidate: the set contains 0, so a vertex or u must serve"
    out = X[np.arange(R), best]
    return np.where(fin[:, None], out, u)


def shield(u, z, nbr, radius, rate, margin, u_max, dt, c):
    """(u*, intervened, correction, min_slack) of the rule in float64.  min_slack [R]: the smallest |a.u - b| over the listed
    constraints -- the distance of the intervened flag's decision from its threshold."""
    A, B, on = constraints(z, nbr, radius, rate, margin, u_max, dt, c)
    u = np.asarray(u, np.float64)
    fin = np.isfinite(u).all(1)
    u0 = np.where(fin[:, None], u, 0.0)
    resid = (A * u0[:, None, :]).sum(2) - B
    intervened = fin & (resid > 0).any(1)
    with np.errstate(invalid="ignore"):
        min_slack = np.where(on & np.isfinite(B), np.abs(resid), np.inf).min(1)
    ustar = project(u, A, B, on)
    ustar = np.where(intervened[:, None], ustar, u)
    corr = np.where(fin, np.where(intervened, np.sqrt(((np.where(fin[:, None], ustar, 0.0) - u0) ** 2).sum(1)), 0.0), np.nan)
    return ustar, intervened, corr, min_slack


def tolerance(u, z, k1, c, radius, rate, margin, u_max, dt):
    """The derived bar of the GPU test, per case: 16 eps32 (max(|u|inf, u_max) + rate (D + 2 l_max + margin) / dt), D the largest
    finite |p| of the case, |u|inf over the finite actions, u_max counted only where it is finite."""
    rows = np.asarray(z, np.float64).reshape(-1, k1, c)[:, 1:, :2]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.sqrt((rows * rows).sum(2))
    D = float(d[np.isfinite(d)].max()) if np.isfinite(d).any() else 0.0
    u = np.asarray(u, np.float64)
    umag = float(np.abs(u[np.isfinite(u)]).max()) if np.isfinite(u).any() else 0.0
    if np.isfinite(u_max):
        umag = max(umag, float(u_max))
    return 16.0 * EPS32 * (umag + rate * (D + 2.0 * float(np.max(radius)) + margin) / dt)


# (N, k, c): the record shapes of the GPU test -- 16-byte path, 24-byte records (8-byte path), 60-byte records (dword path), all
# 12 constraints, box only (every id a ghost: N = 1 has no other agent)
CASES = [(2, 1, 2), (5, 2, 2), (5, 2, 5), (9, 8, 2), (1, 1, 2)]
E_CASE = 37                                                                        # a ragged last wave: 37 N is no multiple of 64
RATE, MARGIN, U_MAX, DT, L = 0.25, 0.05, 1.0, 0.05, 0.1


def synthetic(N, k, c, E=E_CASE, seed=0):
    """Seeded records of one case, float32 as the kernel reads them: gaps log-uniform in [1e-3, 0.5] (one in eight negative),
    directions uniform, ids a random other agent (ghosts -1 here and there; all ghosts at N = 1), u uniform in 1.5 x the box --
    neighbour constraints, box faces and vertices all bind.  Returns dict(z, nbr, u, radius)."""
    rng = np.random.default_rng(1000 * N + 10 * k + c + 7919 * seed)
    R, k1 = E * N, k + 1
    z = rng.uniform(-2.0, 2.0, (R, k1, c))
    gap = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (R, k)))
    gap = np.where(rng.random((R, k)) < 0.125, -rng.uniform(0.0, 0.15, (R, k)), gap)
    d = gap + 2 * L + MARGIN
    ang = rng.uniform(0.0, 2 * np.pi, (R, k))
    z[:, 1:, 0], z[:, 1:, 1] = d * np.cos(ang), d * np.sin(ang)
    i = np.arange(R) % N
    nbr = np.full((R, k1), -1, np.int32)
    nbr[:, 0] = i
    if N > 1:
        other = (i[:, None] + 1 + rng.integers(0, N - 1, (R, k))) % N
        nbr[:, 1:] = np.where(rng.random((R, k)) < 0.1, -1, other)
    u = rng.uniform(-1.5 * U_MAX, 1.5 * U_MAX, (R, 2))
    return dict(z=z.reshape(E, N, k1 * c).astype(np.float32), nbr=nbr.reshape(E, N, k1), u=u.reshape(E, N, 2).astype(np.float32),
                radius=np.full(N, L, np.float32))


def case_reference(N, k, c, seed=0):
    """A case's records with the restatement's answer and the derived tolerance (computed once per case by the test modules)."""
    case = synthetic(N, k, c, seed=seed)
    R, k1 = E_CASE * N, k + 1
    z, nbr, u = case["z"].reshape(R, k1 * c), case["nbr"].reshape(R, k1), case["u"].reshape(R, 2)
    ustar, iv, corr, slack = shield(u, z, nbr, case["radius"], RATE, MARGIN, U_MAX, DT, c)
    A, B, on = constraints(z, nbr, case["radius"], RATE, MARGIN, U_MAX, DT, c)
    tol = tolerance(u, z, k1, c, case["radius"], RATE, MARGIN, U_MAX, DT)
    return dict(case, ustar=ustar, intervened=iv, correction=corr, min_slack=slack, A=A, B=B, on=on, tol=tol)


# ---- the closed loop in float64 ---------------------------------------------------------------------------------------------------
def goal_ring(N, G):
    ang = np.arange(N) * (2 * np.pi / N)
    return np.stack([np.cos(ang) * 0.9 * G / 2 + G / 2, np.sin(ang) * 0.9 * G / 2 + G / 2], 1)


def lattice_starts(E, N, G, rng):
    """E x N distinct nodes of the reference's start lattice (pitch 2 x 1.1 x radius, drone_env.py:193-205)."""
    pitch = 2 * 1.1 * L
    div = int(np.floor(G / pitch))
    pos = np.empty((E, N, 2))
    for e in range(E):
        nodes = rng.choice(div * div, N, replace=False)
        pos[e, :, 0], pos[e, :, 1] = (nodes // div) * pitch, (nodes % div) * pitch
    return pos


def observe(pos, k, delta):
    """The shield's inputs from positions [E, N, 2]: rows 1..k = x_j - x_i of the k closest agents with gap <= delta (closest
    first, ties to the lower id), ghost rows (id -1, zeros) behind them.  Returns z [E N, (k+1) 2], nbr [E N, k+1]."""
    E, N, _ = pos.shape
    diff = pos[:, None, :, :] - pos[:, :, None, :]                                 # [e, i, j] = x_j - x_i
    gap = np.sqrt((diff ** 2).sum(3)) - 2 * L
    gap[:, np.arange(N), np.arange(N)] = np.inf
    order = np.argsort(gap, axis=2, kind="stable")[:, :, :k]
    g = np.take_along_axis(gap, order, 2)
    inside = g <= delta
    rows = np.take_along_axis(diff, order[..., None], 2) * inside[..., None]
    z = np.zeros((E, N, k + 1, 2))
    z[:, :, 1:] = rows
    nbr = np.full((E, N, k + 1), -1, np.int64)
    nbr[:, :, 0] = np.arange(N)
    nbr[:, :, 1:] = np.where(inside, order, -1)
    return z.reshape(E * N, (k + 1) * 2), nbr.reshape(E * N, k + 1)


def closed_loop(N, k, E, G=5.0, delta=1.0, shielded=True, rate=RATE, margin=MARGIN, u_max=U_MAX, steps=200, seed=0):
    """`proportional_control` (drone_env.py:655-679, norm cap 1) on lattice starts, single integrator x' = x + dt u, with or
    without the shield.  Returns (min_clearance [E] over all pairs and all states, arrived [E])."""
    rng = np.random.default_rng(seed)
    pos, xF = lattice_starts(E, N, G, rng), goal_ring(N, G)
    radius = np.full(N, L)
    iu = np.triu_indices(N, 1)

    def clearance(p):
        d = np.sqrt(((p[:, :, None, :] - p[:, None, :, :]) ** 2).sum(3)) - 2 * L
        return d[:, iu[0], iu[1]].min(1)

    clr = clearance(pos)
    for _ in range(steps):
        u = xF[None] - pos
        n = np.sqrt((u ** 2).sum(2, keepdims=True))
        u = np.where(n > 1.0, u / np.maximum(n, 1e-300), u)
        if shielded:
            z, nbr = observe(pos, k, delta)
            u = shield(u.reshape(E * N, 2), z, nbr, radius, rate, margin, u_max, DT, 2)[0].reshape(E, N, 2)
        pos = pos + DT * u
        clr = np.minimum(clr, clearance(pos))
    arrived = (np.sqrt(((pos - xF[None]) ** 2).sum(2)) <= 0.2).all(1)
    return clr, arrived
