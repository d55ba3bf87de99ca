"""Float64 restatement of the action shield (include/dronesim.h: dronesim_action_shield) by BRUTE FORCE, sharing nothing with the
kernel's incremental solve: the projection of u onto an intersection of half-planes is u itself, or its projection onto one
of the lines, or a vertex of two lines -- list all of them, keep the feasible ones, take the closest.  Also the rule's closed
loop in float64 (single integrator, proportional control, lattice starts) that shows the shapes of the GPU tests are meaningful,
and the seeded record generators the test files share: `synthetic` (generic records of a shape), `families` (the geometry the
incremental solve is about: axis-aligned, duplicate, antipodal and near-parallel lines, crowds inside the margin, wedges, huge
actions, permuted slots) and `mutual` (everyone lists everyone, for the guarantee itself)."""
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


def synthetic(N, k, c, E=E_CASE, seed=0, radius=None, margin=MARGIN, u_max=U_MAX):
    """Seeded records of one case, float32 as the kernel reads them: gaps log-uniform in [1e-3, 0.5] (one in eight negative),
    directions uniform, ids a random other agent (ghosts -1 here and there; all ghosts at N = 1), u uniform in 1.5 x the box --
    neighbour constraints, box faces and vertices all bind.  `radius` [N]: per-agent radii (the distance of slot s is then gap +
    radius[i] + radius[j] + margin, at least 0.02); `margin`, `u_max` (+inf: u as for a box of 1): the parameters the case is
    drawn for.  The defaults give the arrays of the recorded cases bit for bit.  Returns dict(z, nbr, u, radius)."""
    rng = np.random.default_rng(1000 * N + 10 * k + c + 7919 * seed)
    R, k1 = E * N, k + 1
    z = rng.uniform(-2.0, 2.0, (R, k1, c))
    gap = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (R, k)))
    gap = np.where(rng.random((R, k)) < 0.125, -rng.uniform(0.0, 0.15, (R, k)), gap)
    ang = rng.uniform(0.0, 2 * np.pi, (R, k))
    i = np.arange(R) % N
    nbr = np.full((R, k1), -1, np.int32)
    nbr[:, 0] = i
    if N > 1:
        other = (i[:, None] + 1 + rng.integers(0, N - 1, (R, k))) % N
        nbr[:, 1:] = np.where(rng.random((R, k)) < 0.1, -1, other)
    box = u_max if np.isfinite(u_max) else U_MAX
    u = rng.uniform(-1.5 * box, 1.5 * box, (R, 2))
    if radius is None:
        d = gap + 2 * L + margin
        radius = np.full(N, L, np.float32)
    else:
        radius = np.asarray(radius, np.float32)
        rad = radius.astype(np.float64)
        d = np.maximum(gap + (rad[i][:, None] + rad[np.where(nbr[:, 1:] >= 0, nbr[:, 1:], i[:, None])]) + margin, 0.02)
    z[:, 1:, 0], z[:, 1:, 1] = d * np.cos(ang), d * np.sin(ang)
    return dict(z=z.reshape(E, N, k1 * c).astype(np.float32), nbr=nbr.reshape(E, N, k1), u=u.reshape(E, N, 2).astype(np.float32),
                radius=radius)


def reference(case, c=2, rate=RATE, margin=MARGIN, u_max=U_MAX, dt=DT):
    """Records dict(z [E, N, k1 c], nbr [E, N, k1], u [E, N, 2], radius [N]) with the restatement's answer, its constraints and
    the derived tolerance at these parameters."""
    E, N, k1 = case["nbr"].shape
    R = E * N
    z, nbr, u = case["z"].reshape(R, k1 * c), case["nbr"].reshape(R, k1), case["u"].reshape(R, 2)
    ustar, iv, corr, slack = shield(u, z, nbr, case["radius"], rate, margin, u_max, dt, c)
    A, B, on = constraints(z, nbr, case["radius"], rate, margin, u_max, dt, c)
    tol = tolerance(u, z, k1, c, case["radius"], rate, margin, u_max, dt)
    return dict(case, ustar=ustar, intervened=iv, correction=corr, min_slack=slack, A=A, B=B, on=on, tol=tol)


def case_reference(N, k, c, seed=0):
    """A case's records with the restatement's answer and the derived tolerance (computed once per case by the test modules)."""
    return reference(synthetic(N, k, c, seed=seed), c)


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


# ---- record sets for the geometry the solve is about ------------------------------------------------------------------------------
# The shapes (N, k, c) that take every load path with more than one load (k + 1 even, c = 2: rows 2h - 1 and 2h out of one 16-byte
# load), the odd k + 1 in between and c = 5 at its extremes; all drawn with unequal radii.  (1024, 3, 2) runs at E = 2.
GEOMETRY_SHAPES = [(4, 3, 2), (6, 5, 2), (8, 7, 2), (5, 4, 2), (7, 6, 2), (6, 5, 5), (3, 8, 5), (3, 1, 5)]
WIDE_SHAPE, WIDE_E = (1024, 3, 2), 2
# (rate, margin, u_max): the edge of the guarantee without a margin, a small rate in a small box, no box, a box beyond 1
PARAMETER_SETS = [(0.5, 0.0, 1.0), (0.01, 0.3, 0.25), (0.25, 0.0, np.inf), (0.5, 0.05, 3.0)]
PARAMETER_SHAPES = [(4, 3, 2), (5, 4, 2)]                                          # k + 1 even, k + 1 odd
WEDGE_DEGREES = (1, 5, 30, 90, 150, 179)
MAGNITUDES = (10, 20, 40, 60, 66, 100)                                             # |u| = 2^m
NEAR_PARALLEL_E = tuple(range(12, 27))
NEAR_PARALLEL_DB = (0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-4, -1e-4, 0.05)


def radii(N, seed=0):
    """Unequal radii: N draws from [0.05, 0.2], float32."""
    return np.random.default_rng(104729 * (seed + 1) + N).uniform(0.05, 0.2, N).astype(np.float32)


def _unit(ang):
    return np.stack([np.cos(ang), np.sin(ang)], -1)


def _blank(N, E, k, rng):
    """Agent ids, empty rows (row 0: the agent's own, arbitrary), ghost ids and the radii of E N records."""
    R = E * N
    i = np.arange(R) % N
    z = np.zeros((R, k + 1, 2))
    z[:, 0] = rng.uniform(-2.0, 2.0, (R, 2))
    nbr = np.full((R, k + 1), -1, np.int64)
    nbr[:, 0] = i
    return i, z, nbr, radii(N, int(rng.integers(1 << 20))).astype(np.float64)


def _others(i, N, m, rng):
    """m distinct other agents per record, [R, m]."""
    off = np.argsort(rng.random((i.shape[0], N - 1)), axis=1)[:, :m]
    return (i[:, None] + 1 + off) % N


def _gaps(rng, shape, lo=1e-3, hi=0.5, negative=0.125):
    """Gaps (clearance minus margin): log-uniform in [lo, hi], a share `negative` uniform in [-0.1, -1e-3]."""
    gap = np.exp(rng.uniform(np.log(lo), np.log(hi), shape))
    return np.where(rng.random(shape) < negative, -rng.uniform(1e-3, 0.1, shape), gap)


def _put(z, nbr, rows, slot, j, direction, gap, rad, i, margin):
    """Into `slot` of the records `rows` (bool [R]): neighbour j [R] in `direction` [R, 2] at gap `gap` [R]."""
    d = gap + rad[i] + rad[j] + margin
    assert (d[rows] > 0).all()
    z[rows, slot] = (d[:, None] * direction)[rows]
    nbr[rows, slot] = j[rows]


def _pack(E, N, z, nbr, u, rad, rate=RATE, margin=MARGIN, u_max=U_MAX, blocks=None, **meta):
    """A record set as the kernel reads it (c = 2) with its parameters; `blocks`: (label, first env, end env) -- the runs of envs
    that are checked with a tolerance of their own; `meta`: per-record arrays [E N] the tests select by."""
    k1 = nbr.shape[1]
    z32 = z if z.dtype == np.float32 else z.astype(np.float32)
    return dict(z=z32.reshape(E, N, k1 * 2), nbr=nbr.astype(np.int32).reshape(E, N, k1), u=np.asarray(u, np.float32).reshape(E, N, 2),
                radius=rad.astype(np.float32), rate=rate, margin=margin, u_max=u_max, dt=DT, c=2,
                blocks=blocks or [("", 0, E)], **meta)


def _box_u(rng, R, u_max=U_MAX):
    return rng.uniform(-1.5 * u_max, 1.5 * u_max, (R, 2))


def _axes(rng, N=5, E=512, k=4):
    """Neighbour directions exactly (+-1, 0), (0, +-1), one per slot in a random order; b = 5 gap from 0.005 to 2.5 around the
    box's 1; one slot in four a ghost (its row stays)."""
    i, z, nbr, rad = _blank(N, E, k, rng)
    R = E * N
    order = np.argsort(rng.random((R, 4)), axis=1)
    j = _others(i, N, k, rng)
    gap = _gaps(rng, (R, k))
    for s in range(k):
        _put(z, nbr, np.ones(R, bool), s + 1, j[:, s], BOX[order[:, s]], gap[:, s], rad, i, MARGIN)
    nbr[:, 1:] = np.where(rng.random((R, k)) < 0.25, -1, nbr[:, 1:])
    return _pack(E, N, z, nbr, _box_u(rng, R), rad)


def _duplicates(rng, N=5, E=512, k=3):
    """Slots 1 and 2 (and 3 in every other record) hold the same direction bit for bit: p, 2^m p, 2^m' p in float32; ids differ,
    so the radii and b differ.  The other slot 3 is a generic neighbour."""
    i, z, nbr, rad = _blank(N, E, k, rng)
    R = E * N
    j = _others(i, N, k, rng)
    every = np.ones(R, bool)
    _put(z, nbr, every, 1, j[:, 0], _unit(rng.uniform(0, 2 * np.pi, R)), _gaps(rng, R, 0.02, 0.4, 0.0), rad, i, MARGIN)
    _put(z, nbr, every, 3, j[:, 2], _unit(rng.uniform(0, 2 * np.pi, R)), _gaps(rng, R), rad, i, MARGIN)
    z = z.astype(np.float32)
    m2 = rng.choice([-1, 1, 2], R)
    z[:, 2] = z[:, 1] * np.exp2(m2).astype(np.float32)[:, None]
    nbr[:, 2] = j[:, 1]
    triple = rng.random(R) < 0.5
    m3 = np.where(m2 == 1, 2, 1)
    z[triple, 3] = (z[:, 1] * np.exp2(m3).astype(np.float32)[:, None])[triple]
    return _pack(E, N, z, nbr, _box_u(rng, R), rad, triple=triple)


def _antipodal(rng, N=4, E=640, k=3):
    """Slots 1 and 2: p and -2^m p in float32 (m in -1..2), gaps of both signs, so both b > 0, one b = 0 and both b = 0 (the
    feasible set a line through 0) all occur; slot 3 a generic neighbour or a ghost."""
    i, z, nbr, rad = _blank(N, E, k, rng)
    R = E * N
    j = _others(i, N, k, rng)
    every = np.ones(R, bool)
    _put(z, nbr, every, 1, j[:, 0], _unit(rng.uniform(0, 2 * np.pi, R)), _gaps(rng, R, 0.01, 0.4, 0.5), rad, i, MARGIN)
    _put(z, nbr, rng.random(R) < 0.5, 3, j[:, 2], _unit(rng.uniform(0, 2 * np.pi, R)), _gaps(rng, R), rad, i, MARGIN)
    z = z.astype(np.float32)
    z[:, 2] = -z[:, 1] * np.exp2(rng.integers(-1, 3, R)).astype(np.float32)[:, None]
    nbr[:, 2] = j[:, 1]
    return _pack(E, N, z, nbr, _box_u(rng, R), rad)


def _crowd(rng, N=9, E=288, k=8):
    """Neighbours inside the margin (g < 0, b = 0).  `point` records: three to eight of them, adjacent directions less than pi
    apart all the way round, so 0 is the only feasible action.  The others: two of them 0.2 to 2.9 apart -- a cone.  The
    remaining slots are ghosts or neighbours with a gap."""
    i, z, nbr, rad = _blank(N, E, k, rng)
    R = E * N
    j = _others(i, N, k, rng)
    point = rng.random(R) < 0.6
    m = np.where(point, rng.integers(3, 9, R), 2)
    base = rng.uniform(0, 2 * np.pi, R)
    for s in range(k):
        round_about = base + 2 * np.pi * (s + rng.uniform(-0.2, 0.2, R)) / m
        cone = base + s * rng.uniform(0.2, 2.9, R)
        inside = s < m
        _put(z, nbr, inside, s + 1, j[:, s], _unit(np.where(point, round_about, cone)), -rng.uniform(1e-3, 0.1, R), rad, i, MARGIN)
        far = ~inside & (rng.random(R) < 0.5)
        _put(z, nbr, far, s + 1, j[:, s], _unit(rng.uniform(0, 2 * np.pi, R)), _gaps(rng, R, 0.02, 0.5, 0.0), rad, i, MARGIN)
    return _pack(E, N, z, nbr, _box_u(rng, R), rad, point=point)


def _vertex(a1, b1, a2, b2):
    det = a1[:, 0] * a2[:, 1] - a1[:, 1] * a2[:, 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([(b1 * a2[:, 1] - b2 * a1[:, 1]) / det, (a1[:, 0] * b2 - a2[:, 0] * b1) / det], 1)


def _near_parallel(rng, rate, u_max, N=4, E=160, k=3):
    """Slots 1 and 2 at an angle 2^-e (0.5 .. 1), e = 12 .. 26 -- both sides of the kernel's parallel threshold 2^-21 --, gaps
    >= 0.02, b2 - b1 from NEAR_PARALLEL_DB; u lies beyond both lines, above their vertex where that is within 2 of the foot and
    above a point of the lower line otherwise.  Every other record has a third neighbour across the pair's direction, on the far
    side of u: it clips the pair's lines and u satisfies it."""
    i, z, nbr, rad = _blank(N, E, k, rng)
    R = E * N
    j = _others(i, N, k, rng)
    e = np.resize(np.array(NEAR_PARALLEL_E), R)
    db = np.resize(np.repeat(np.array(NEAR_PARALLEL_DB), len(NEAR_PARALLEL_E)), R)
    theta = np.exp2(-e.astype(np.float64)) * rng.uniform(0.5, 1.0, R) * rng.choice([-1.0, 1.0], R)
    phi = rng.uniform(0, 2 * np.pi, R)
    a1, a2 = _unit(phi), _unit(phi + theta)
    scale = rate / DT
    g_hi = min(0.4, 0.9 * u_max / scale) if np.isfinite(u_max) else 0.4             # (with a box: b below it, so the pair binds)
    g1 = rng.uniform(0.03, g_hi, R) + np.maximum(-db, 0.0) / scale
    g2 = g1 + db / scale
    assert min(g1.min(), g2.min()) >= 0.02
    every = np.ones(R, bool)
    _put(z, nbr, every, 1, j[:, 0], a1, g1, rad, i, MARGIN)
    _put(z, nbr, every, 2, j[:, 1], a2, g2, rad, i, MARGIN)
    b1, b2 = scale * g1, scale * g2
    t = np.stack([-a1[:, 1], a1[:, 0]], 1)
    v = _vertex(a1, b1, a2, b2)
    foot = np.where((b1 <= b2)[:, None], b1[:, None] * a1, b2[:, None] * a2)
    near = np.isfinite(v).all(1) & (np.linalg.norm(v - foot, axis=1) <= 2.0)
    tau = rng.uniform(-1.0, 1.0, R)
    base = np.where(near[:, None], v, foot + tau[:, None] * t)
    u = base + rng.uniform(0.05, 0.5, R)[:, None] * _unit(phi + 0.5 * theta)
    third = rng.random(R) < 0.5
    side = np.where((u * t).sum(1) >= 0, -1.0, 1.0)                                # a3 points away from u along the pair's lines
    a3 = _unit(np.arctan2(side * t[:, 1], side * t[:, 0]) + rng.uniform(-0.3, 0.3, R))
    _put(z, nbr, third, 3, j[:, 2], a3, rng.uniform(0.02, 0.5, R), rad, i, MARGIN)
    return _pack(E, N, z, nbr, u, rad, rate=rate, u_max=u_max, e=e, db=db, third=third)


def _wedge(rng, N=4, E_each=96, k=3):
    """Slots 1 and 2: two lines whose normals are 1, 5, 30, 90, 150, 179 degrees apart (one block of envs each), gaps 0.02 to
    0.1; u = vertex + a positive combination of the two normals, so the vertex is the answer.  No box.  Every other record
    lists a third neighbour behind the wedge, which never binds."""
    E = E_each * len(WEDGE_DEGREES)
    i, z, nbr, rad = _blank(N, E, k, rng)
    R = E * N
    j = _others(i, N, k, rng)
    deg = np.repeat(np.array(WEDGE_DEGREES, np.float64), E_each * N)
    alpha = np.deg2rad(deg) * rng.choice([-1.0, 1.0], R)
    phi = rng.uniform(0, 2 * np.pi, R)
    a1, a2 = _unit(phi), _unit(phi + alpha)
    g1, g2 = rng.uniform(0.02, 0.1, R), rng.uniform(0.02, 0.1, R)
    every = np.ones(R, bool)
    _put(z, nbr, every, 1, j[:, 0], a1, g1, rad, i, MARGIN)
    _put(z, nbr, every, 2, j[:, 1], a2, g2, rad, i, MARGIN)
    v = _vertex(a1, RATE / DT * g1, a2, RATE / DT * g2)
    u = v + rng.uniform(0.05, 0.5, R)[:, None] * a1 + rng.uniform(0.05, 0.5, R)[:, None] * a2
    behind = _unit(phi + 0.5 * alpha + np.pi + rng.uniform(-0.5, 0.5, R))
    _put(z, nbr, rng.random(R) < 0.5, 3, j[:, 2], behind, rng.uniform(0.02, 0.5, R), rad, i, MARGIN)
    blocks = [("%d deg" % d, q * E_each, (q + 1) * E_each) for q, d in enumerate(WEDGE_DEGREES)]
    return _pack(E, N, z, nbr, u, rad, u_max=np.inf, blocks=blocks, deg=deg)


def _magnitude(rng, u_max, N=5, E_each=48, k=2):
    """Generic neighbours (`synthetic`, unequal radii), |u| = 2^m for m in MAGNITUDES (one block of envs each) times a unit
    vector."""
    E = E_each * len(MAGNITUDES)
    case = synthetic(N, k, 2, E=E, seed=int(rng.integers(1 << 20)), radius=radii(N, int(rng.integers(1 << 20))), u_max=u_max)
    m = np.repeat(np.array(MAGNITUDES, np.float64), E_each * N)
    u = np.exp2(m)[:, None] * _unit(rng.uniform(0, 2 * np.pi, E * N))
    blocks = [("2^%d" % p, q * E_each, (q + 1) * E_each) for q, p in enumerate(MAGNITUDES)]
    return dict(case, u=u.astype(np.float32).reshape(E, N, 2), rate=RATE, margin=MARGIN, u_max=u_max, dt=DT, c=2, blocks=blocks)


def _permuted(base, copies, rng):
    """`base`'s envs `copies` + 1 times over: first as they are, then with slots 1..k of every record permuted (ids with rows)."""
    E, N, k1 = base["nbr"].shape
    z, nbr = base["z"].reshape(E, N, k1, 2), base["nbr"]
    zs, ns = [z], [nbr]
    for _ in range(copies):
        perm = 1 + np.argsort(rng.random((E, N, k1 - 1)), axis=2)
        zs.append(np.take_along_axis(z[:, :, 1:], (perm - 1)[..., None], 2))
        zs[-1] = np.concatenate([z[:, :, :1], zs[-1]], 2)
        ns.append(np.concatenate([nbr[:, :, :1], np.take_along_axis(nbr, perm, 2)], 2))
    rep = copies + 1
    out = {n: v for n, v in base.items() if not isinstance(v, np.ndarray) or n == "radius"}
    out.update(z=np.concatenate(zs).reshape(rep * E, N, k1 * 2), nbr=np.concatenate(ns), u=np.concatenate([base["u"]] * rep))
    for n, v in base.items():
        if isinstance(v, np.ndarray) and v.shape == (E * N,):
            out[n] = np.concatenate([v] * rep)
    out["blocks"] = [("%s copy %d" % (label, q), q * E + e0, q * E + e1) for q in range(rep) for label, e0, e1 in base["blocks"]]
    out["copies"], out["E0"] = rep, E
    return out


def families(seed=0):
    """Named record sets, each dict(z, nbr, u, radius, rate, margin, u_max, dt, c, blocks, ...): the geometry the solve is about,
    drawn so that the constraint a family is named after binds (tests/test_shield_host.py holds the shares).  Unequal radii
    from [0.05, 0.2], N >= 3, c = 2, two to four thousand records per family."""
    rng = np.random.default_rng(31337 + seed)
    out = {"axes": _axes(rng), "duplicates": _duplicates(rng), "antipodal": _antipodal(rng), "crowd": _crowd(rng)}
    for rate in (0.01, 0.25, 0.5):
        for u_max in (U_MAX, np.inf):
            out["near_parallel rate %g %s" % (rate, "box" if np.isfinite(u_max) else "no box")] = _near_parallel(rng, rate, u_max)
    out["wedge"] = _wedge(rng)
    out["magnitude box"], out["magnitude no box"] = _magnitude(rng, U_MAX), _magnitude(rng, np.inf)
    out["order wedge"] = _permuted(out["wedge"], 1, rng)
    out["order crowd"] = _permuted(out["crowd"], 1, rng)
    return out


FAMILY_NAMES = (["axes", "duplicates", "antipodal", "crowd"]
                + ["near_parallel rate %g %s" % (rate, box) for rate in (0.01, 0.25, 0.5) for box in ("box", "no box")]
                + ["wedge", "magnitude box", "magnitude no box", "order wedge", "order crowd"])
ILL_CONDITIONED = ("near_parallel", "wedge", "order wedge")                         # families checked with the backward-stable bar


def lowered(ref, tol):
    """u* of the problem with every finite b lowered by tol: C(B - tol) of the backward-stable optimality bar."""
    R = ref["ustar"].shape[0]
    B = np.where(np.isfinite(ref["B"]), ref["B"] - tol, ref["B"])
    return project(ref["u"].reshape(R, 2), ref["A"], B, ref["on"])


def block_reference(fam, e0, e1):
    """`reference` of the envs e0 .. e1 of a record set at its own parameters."""
    part = dict(z=fam["z"][e0:e1], nbr=fam["nbr"][e0:e1], u=fam["u"][e0:e1], radius=fam["radius"])
    return reference(part, fam["c"], fam["rate"], fam["margin"], fam["u_max"], fam["dt"])


def active(ref, rel=1e-9):
    """[R, 4 + k] bool: the listed constraints that hold with equality at the restatement's u*."""
    r = (ref["A"] * ref["ustar"][:, None, :]).sum(2) - np.where(np.isfinite(ref["B"]), ref["B"], np.inf)
    scale = 1.0 + np.abs(ref["ustar"]).max(1)
    return ref["on"] & np.isfinite(ref["B"]) & (np.abs(r) <= rel * scale[:, None])


def mutual(N, E, seed=0, margin=MARGIN, u_max=U_MAX):
    """Everyone lists everyone (k = N - 1): float32 positions [E, N, 2] grown as a cluster (each agent placed next to an earlier
    one at a clearance log-uniform from 0.2 margin to 0.5, no pair closer than that), unequal radii, rows p = float32(x_j - x_i)
    in ascending j, nominal actions that aim at the nearest neighbour with 1.5 u_max plus noise.
    Returns dict(pos, z, nbr, u, radius)."""
    rng = np.random.default_rng(577 * N + seed)
    rad = radii(N, seed + 17).astype(np.float64)
    lo = 0.2 * margin if margin > 0 else 0.01
    pos = np.zeros((E, N, 2))
    for e in range(E):
        pos[e, 0] = rng.uniform(-1.0, 1.0, 2)
        n = 1
        while n < N:
            m = rng.integers(n)
            c = np.exp(rng.uniform(np.log(lo), np.log(0.5)))
            x = pos[e, m] + (c + rad[m] + rad[n]) * _unit(rng.uniform(0, 2 * np.pi))
            if (np.linalg.norm(pos[e, :n] - x, axis=1) - rad[:n] - rad[n] >= 0.999 * lo).all():
                pos[e, n] = x
                n += 1
    pos = pos.astype(np.float32)
    p64 = pos.astype(np.float64)
    diff = p64[:, None, :, :] - p64[:, :, None, :]                                 # [e, i, j] = x_j - x_i
    ids = np.array([[j for j in range(N) if j != i] for i in range(N)])            # [N, N - 1]
    rows = diff[:, np.arange(N)[:, None], ids]                                     # [E, N, N - 1, 2]
    z = np.zeros((E, N, N, 2), np.float32)
    z[:, :, 1:] = rows.astype(np.float32)
    nbr = np.concatenate([np.broadcast_to(np.arange(N)[None, :, None], (E, N, 1)), np.broadcast_to(ids[None], (E, N, N - 1))], 2)
    clear = np.linalg.norm(rows, axis=3) - rad[None, :, None] - rad[ids][None]
    nearest = np.take_along_axis(rows, clear.argmin(2)[..., None, None], 2)[:, :, 0]
    u = 1.5 * u_max * nearest / np.linalg.norm(nearest, axis=2, keepdims=True) + rng.normal(0.0, 0.2 * u_max, (E, N, 2))
    return dict(pos=pos, z=z.reshape(E, N, N * 2), nbr=nbr.astype(np.int32), u=u.astype(np.float32), radius=rad.astype(np.float32))
