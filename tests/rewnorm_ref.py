"""Float64 restatement of the reward normaliser (csrc/rewnorm.hip, include/dronesim.h: dronesim_rewnorm_update /
dronesim_rewnorm_apply) in NumPy on the CPU -- the running discounted return with its carry, the finite rule, the two-pass
moments of everything counted so far, Chan's merge, the scale and the map -- and the inputs of the GPU tests: per shape four
successive windows of seeded rewards over a few orders of magnitude, with every `done` pattern the scan has to survive."""
import numpy as np

GAMMA = 0.99
N_WINDOWS = 4
# (T, E, N) -- chosen for where the scan can go wrong (tests/test_gpu_rewnorm.py says which shape takes which path)
SHAPES = [(7, 3, 5), (33, 9, 4), (17, 8, 64), (40, 130, 5)]

# the special columns (env, agent) and envs; every shape has E >= 3 and N >= 4
ENV_NO_END, ENV_ALWAYS, ENV_PATTERN = 0, 1, 2       # never done | done on every step | done at t = 0, 2, 3 and T - 1 exactly
ZERO_COL = (ENV_NO_END, 2)                          # constant zero reward
NAN_COL, NAN_WINDOW, NAN_STEPS = (ENV_PATTERN, 0), 1, (1, 2)     # NaN at t = 1, 2; done at t = 2 ends the poison: 2 uncounted
INF_COL, INF_WINDOW, INF_STEP = (ENV_PATTERN, 1), 2, 4           # +inf at t = 4; done at T - 1: T - 4 uncounted


def uncounted(T):
    """What the rule takes out of the counts: {window: {column: steps}}."""
    return {NAN_WINDOW: {NAN_COL: len(NAN_STEPS)}, INF_WINDOW: {INF_COL: T - INF_STEP}}


def windows(T, E, N, n=N_WINDOWS, seed=0):
    """``n`` successive windows ``(reward [T,E,N] float32, done [T,E] uint8)``.  Rewards are negative (as the env's are), a
    column's magnitude is 10^U(-1, 2) and every entry varies by a factor in [0.5, 1.5)."""
    rng = np.random.default_rng(1000 * T + 10 * E + N + seed)
    mag = 10.0 ** rng.uniform(-1.0, 2.0, size=(E, N))
    out = []
    for k in range(n):
        r = -(mag[None] * rng.uniform(0.5, 1.5, size=(T, E, N))).astype(np.float32)
        d = (rng.uniform(size=(T, E)) < 0.06).astype(np.uint8)
        d[:, ENV_NO_END] = 0
        d[:, ENV_ALWAYS] = 1
        d[:, ENV_PATTERN] = 0
        d[[0, 2, 3, T - 1], ENV_PATTERN] = 1
        r[:, ZERO_COL[0], ZERO_COL[1]] = 0.0
        if k == NAN_WINDOW:
            r[list(NAN_STEPS), NAN_COL[0], NAN_COL[1]] = np.nan
        if k == INF_WINDOW:
            r[INF_STEP, INF_COL[0], INF_COL[1]] = np.inf
        out.append((r, d))
    return out


def groups(scope, N):
    """``(group_of [N], n_groups)``: "team", "agent" or a list of group ids numbered in the order of first appearance."""
    if scope == "team":
        return np.zeros(N, dtype=np.int64), 1
    if scope == "agent":
        return np.arange(N), N
    number = {}
    g = np.array([number.setdefault(int(v), len(number)) for v in scope])
    return g, len(number)


def two_group_map(N):
    """A sharing map with two tied groups, labels that are not contiguous and a leader order that is not the label order."""
    return [7 if i % 3 == 1 else 2 for i in range(N)]


def scan(reward, done, gamma, ret):
    """The recurrence over one window from the carry ``ret [E,N]``: ``(R [T,E,N], the new carry)``, float64.  R[t] is the
    value BEFORE the reset behind done[t]; non-finite values stay (the carry is not repaired)."""
    T = reward.shape[0]
    R = np.array(ret, dtype=np.float64)
    vals = np.empty(reward.shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            R = gamma * R + reward[t].astype(np.float64)
            vals[t] = R
            R = np.where(done[t][:, None] != 0, 0.0, R)
    return vals, R


def moments(values, group_of, n_groups):
    """Two-pass ``[3, G]`` = (count, mean, m2) over the FINITE entries of ``values [..., N]`` (or a list of such arrays)."""
    vs = values if isinstance(values, (list, tuple)) else [values]
    out = np.zeros((3, n_groups))
    for g in range(n_groups):
        v = np.concatenate([a[..., group_of == g].ravel() for a in vs])
        v = v[np.isfinite(v)]
        if v.size:
            mean = v.sum() / v.size
            out[:, g] = v.size, mean, ((v - mean) ** 2).sum()
    return out


def merge(a, b):
    """Chan's merge of two ``[3, G]`` states; an empty side changes nothing."""
    out = np.array(a, dtype=np.float64)
    for g in range(a.shape[1]):
        na, ma, qa = a[:, g]
        nb, mb, qb = b[:, g]
        if nb == 0:
            continue
        if na == 0:
            out[:, g] = nb, mb, qb
            continue
        n, d = na + nb, mb - ma
        out[:, g] = n, ma + d * nb / n, qa + qb + d * d * na * nb / n
    return out


def scale(state, eps):
    """``[G]``: 1 / sqrt(m2 / count + eps); 1 where the count is 0 and 1 where the denominator is 0."""
    n, m2 = state[0], state[2]
    var = np.where(n > 0, m2 / np.maximum(n, 1.0) + eps, 0.0)
    return np.where(var > 0, 1.0 / np.sqrt(np.where(var > 0, var, 1.0)), 1.0)


def apply(reward, agent_scale, clip=None):
    """``(float32)((double) r * scale[i])``, clamped by comparisons: NaN stays NaN."""
    with np.errstate(invalid="ignore", over="ignore"):
        y = (reward.astype(np.float64) * agent_scale).astype(np.float32)
        if clip is not None:
            y = np.where(y > clip, np.float32(clip), np.where(y < -clip, np.float32(-clip), y))
    return y


_RUNS = {}


def run(shape, scope="team", gamma=GAMMA):
    """The whole history of a shape under a scope, computed once and shared (do not modify): per window k the returns ``R[k]``,
    the carry after it ``ret[k]``, the streaming state ``stream[k]`` (Chan merges of the windows' own two-pass moments), the
    two-pass state over everything seen so far ``twopass[k]`` and ``maxabs[k]`` ``[G]``, the largest finite |R| so far."""
    key = (tuple(shape), scope if isinstance(scope, str) else tuple(scope), gamma)
    if key in _RUNS:
        return _RUNS[key]
    T, E, N = shape
    group_of, G = groups(scope, N)
    ws = windows(T, E, N)
    ret = np.zeros((E, N))
    state = np.zeros((3, G))
    res = dict(windows=ws, group_of=group_of, n_groups=G, R=[], ret=[], stream=[], twopass=[], maxabs=[])
    for r, d in ws:
        vals, ret = scan(r, d, gamma, ret)
        res["R"].append(vals)
        res["ret"].append(ret)
        state = merge(state, moments(vals, group_of, G))
        res["stream"].append(state)
        res["twopass"].append(moments(res["R"], group_of, G))
        fin = [np.where(np.isfinite(v), np.abs(v), 0.0) for v in res["R"]]
        res["maxabs"].append(np.array([max(f[..., group_of == g].max() for f in fin) for g in range(G)]))
    _RUNS[key] = res
    return res
