"""Per-env restatement of the obstacle rule (include/dronesim_env_obstacles.h) -- test infrastructure, no GPU needed: the float64
functions of tests/obstacle_ref.py and the float32-exact ones of tests/obstacle_obs_ref.py, LOOPED OVER ENVS with env e's first
``counts[e]`` discs as the list.  Nothing of the rule is restated here.  Also: the launch geometry of csrc/env_obstacles.hip restated
(rows per workgroup, envs per wave, wraps), the shape table of tests/test_gpu_env_obstacles.py with the reason each shape is there
(tests/test_env_obstacles_host.py asserts the reasons), and the seeded generators both test files share."""
import numpy as np

from tests import obstacle_obs_ref as OO
from tests import obstacle_ref as OR
from tests import shield_ref as S

BLOCK = 256
# (E, N, M, m) with the reason each shape is there; `staged`: the path dronesim_env_obstacle_plan must send it to
SHAPES = [
    ((7, 5, 8, 2), True, "a wave spans 13 rows, more than E, so a block wraps several times; staged"),
    ((3, 64, 64, 4), True, "one env per wave at the full M; staged, bank stride"),
    ((5, 70, 16, 3), True, "env boundary inside a wave; ragged last block"),
    ((300, 1, 64, 4), False, "256 rows per block, direct path, two blocks"),
    ((300, 1, 8, 1), True, "256 slots staged"),
    ((40, 2, 64, 2), False, "direct path"),
    ((1, 5, 3, 2), True, "E = 1"),
    ((7, 5, 0, 2), None, "M = 0: no discs"),
]
IDS = [str(s) for s, _, _ in SHAPES]
# (T, E, N) of the tables: obstacle_ref.WINDOW_SHAPES with E > 1 (they reach every scan path); M = 64 where the shared tests run
# a wide list, 3 otherwise
WINDOW_SHAPES = [(shape, 64 if shape in OR.WINDOW_M else 3) for shape, _ in OR.WINDOW_SHAPES if shape[1] > 1]


# ---- the launch geometry ----------------------------------------------------------------------------------------------------------
def rows_per_block(N):
    """The most rows (a row = N records of one env) a 256-record workgroup touches."""
    return 254 // N + 2


def block_rows(N, records):
    """Per workgroup (first row, rows touched) of a launch over `records` records."""
    out = []
    for rb in range(0, records, BLOCK):
        last = min(rb + BLOCK - 1, records - 1)
        out.append((rb // N, last // N - rb // N + 1))
    return out


def block_wraps(E, N, rows):
    """Per workgroup of a launch over `rows` rows of N records: how often its rows pass from env E - 1 to env 0."""
    return [sum(1 for q in range(lo + 1, lo + n) if q % E == 0) for lo, n in block_rows(N, rows * N)]


def wave_rows(N, records):
    """Per wave of a launch: the rows its active lanes touch."""
    return [min(w + 63, records - 1) // N - w // N + 1 for w in range(0, records, 64)]


# ---- the rule, per env ------------------------------------------------------------------------------------------------------------
def env_list(cs, e):
    return np.asarray(cs["obstacles"])[e, :int(cs["counts"][e])]


def sense(cs, m):
    """`obstacle_ref.sense` per env: dict(orow [E,N,m,3], oid [E,N,m], gap_min [E,N], hit [E,N]) in float64."""
    parts = [OR.sense(cs["z"][e], cs["xF"], cs["radius"], cs["sense"], env_list(cs, e), m) for e in range(cs["z"].shape[0])]
    return {name: np.stack([p[name] for p in parts]) for name in ("orow", "oid", "gap_min", "hit")}


def columns(cs, m, z=None):
    """`obstacle_obs_ref.columns` per env (the kernels' bits): x [..., E, N, d + 3m] float32 of z [..., E, N, d]."""
    z = np.asarray(cs["z"] if z is None else z, np.float32)
    E, N, d = z.shape[-3:]
    rows = z.reshape(-1, E, N, d)
    x = np.zeros(rows.shape[:3] + (d + 3 * m,), np.float32)
    for e in range(E):
        got = OO.columns(rows[:, e].reshape(-1, d), cs["xF"], cs["radius"], cs["sense"], env_list(cs, e), m)["x"]
        x[:, e] = got.reshape(-1, N, d + 3 * m)
    return x.reshape(z.shape[:-1] + (d + 3 * m,))


def cost(cs, weight, z=None):
    """`obstacle_obs_ref.cost` per env: (cost, bound) float64 [..., E, N]."""
    z = np.asarray(cs["z"] if z is None else z, np.float32)
    E, N, d = z.shape[-3:]
    rows = z.reshape(-1, E, N, d)
    c, b = np.zeros(rows.shape[:3]), np.zeros(rows.shape[:3])
    for e in range(E):
        got = OO.cost(rows[:, e].reshape(-1, d), cs["xF"], cs["radius"], cs["sense"], env_list(cs, e), weight)
        c[:, e], b[:, e] = got["cost"].reshape(-1, N), got["bound"].reshape(-1, N)
    return c.reshape(z.shape[:-1]), b.reshape(z.shape[:-1])


def shaped_reward(w, weight, with_final=True):
    """`obstacle_obs_ref.shaped_reward` per env on a window of `reward_window`: dict(reward, cost, bound, cost_bound) [T,E,N]."""
    T, E, N = w["reward"].shape
    out = {name: np.zeros((T, E, N)) for name in ("reward", "cost", "bound", "cost_bound")}
    for e in range(E):
        zf = w["z_final"][:, e:e + 1] if with_final else None
        got = OO.shaped_reward(w["reward"][:, e:e + 1], w["z_all"][1:, e:e + 1], zf, w["done"][:, e:e + 1], w["xF"], w["radius"],
                               w["sense"], env_list(w, e), weight)
        for name in out:
            out[name][:, e] = got[name][:, 0]
    return out


def episode_tables(w):
    """`obstacle_ref.episode_tables_fast` per env on a window of `window_case`."""
    E = w["z"].shape[1]
    parts = [OR.episode_tables_fast(w["z"][:, e:e + 1], w["done"][:, e:e + 1], w["xF"], w["radius"], env_list(w, e),
                                    None if w["z_final"] is None else w["z_final"][:, e:e + 1]) for e in range(E)]
    return {name: np.concatenate([p[name] for p in parts]) for name in OR.TABLES}


# ---- generators -------------------------------------------------------------------------------------------------------------------
def lists(E, M, seed=0):
    """[E,M,3] float32: env e's list is `obstacle_ref.discs(M, seed', lo=0, hi=5)` with a seed of its own."""
    return np.stack([OR.discs(M, 1000 * (seed + 1) + e, lo=0.0, hi=5.0) for e in range(E)]).reshape(E, M, 3)


def ragged_counts(E, M):
    """Counts 0, 1, M and values between, cycling over the envs."""
    cycle = [0, 1, M, M // 2, max(M - 1, 0), M // 3]
    return np.array([min(cycle[e % len(cycle)], M) for e in range(E)], np.int64)


def case(E, N, M, m, k=1, c=2, seed=0, counts=None, same_list=False):
    """Seeded float32 inputs for the sense / observe entries: dict(z [E,N,(k+1)c], xF, radius, sense, obstacles [E,M,3], counts [E]).
    Positions uniform in the 5 x 5 square the discs lie in; ranges in [0.5, 1.5]; the rest of a record is noise.  A record is
    REDRAWN until the decisions taken on it under ITS env's list (the first counts[e] rows) are obstacle_ref.SEPARATION apart
    (`obstacle_ref.separated`).  `same_list`: every env holds env 0's list."""
    rng = np.random.default_rng(88001 + 7919 * seed + 131 * E + 17 * N + 3 * M + m + 5 * k + c)
    d = (k + 1) * c
    xF, radius = OR.goals(N, seed), S.radii(N, seed)
    reach = rng.uniform(0.5, 1.5, N).astype(np.float32)
    obs = lists(E, M, seed)
    if same_list:
        obs = np.tile(obs[:1], (E, 1, 1))
    counts = np.full(E, M, np.int64) if counts is None else np.asarray(counts, np.int64)
    z = (rng.standard_normal((E, N, d)) * 0.3).astype(np.float32)
    z[..., :2] = rng.uniform(0.0, 5.0, (E, N, 2)).astype(np.float32) - xF[None]
    for e in range(E):
        for _ in range(200):
            G = OR.gaps(z[e], xF, radius, obs[e, :counts[e]])[1]
            bad = ~OR.separated(G, reach.astype(np.float64), m)
            if not bad.any():
                break
            z[e, bad, :2] = rng.uniform(0.0, 5.0, (int(bad.sum()), 2)).astype(np.float32) - xF[bad]
        else:
            raise AssertionError("case: records left that are not separated")
    return dict(z=z, xF=xF, radius=radius, sense=reach, obstacles=obs, counts=counts)


def plant_on_agents(cs):
    """The case with every row at or beyond counts[e] holding a disc of radius 0.5 centred ON an agent of env e (agent j % N for
    row j): read, it would hit and be listed.  The records, and so their separation, are unchanged."""
    obs = cs["obstacles"].copy()
    E, M = obs.shape[:2]
    N = cs["xF"].shape[0]
    for e in range(E):
        for j in range(int(cs["counts"][e]), M):
            i = j % N
            obs[e, j] = (cs["z"][e, i, 0] + cs["xF"][i, 0], cs["z"][e, i, 1] + cs["xF"][i, 1], 0.5)
    return dict(cs, obstacles=obs)


def separated_everywhere(cs, m):
    """Every record of the case keeps SEPARATION between its decisions under its env's list (float64)."""
    reach = np.asarray(cs["sense"], np.float64)
    return all(OR.separated(OR.gaps(cs["z"][e], cs["xF"], cs["radius"], env_list(cs, e))[1], reach, m).all()
               for e in range(cs["z"].shape[0]))


def rows_case(cs, L, seed=0):
    """z [L, E, N, d]: L rows of records of the case's scene, row 0 the case's own, the others drawn like it (not separated: the
    rows are compared with one-row calls of the same kernel, bit for bit)."""
    E, N, d = cs["z"].shape
    rng = np.random.default_rng(3301 + seed + L + E + N)
    z = (rng.standard_normal((L, E, N, d)) * 0.3).astype(np.float32)
    z[..., :2] = rng.uniform(0.0, 5.0, (L, E, N, 2)).astype(np.float32) - cs["xF"][None, None]
    z[0] = cs["z"]
    return z


def reward_window(E, N, M, T=6, k=1, seed=0, counts=None, same_list=False):
    """A stored window for the reward entry at the case's scene: ring z_all [T+1,E,N,d], z_final [T,E,N,d] (other positions),
    done [T,E] cycling through obstacle_obs_ref.WINDOW_ENDS, reward [T,E,N] in [-3, 0]."""
    cs = case(E, N, M, 2, k=k, seed=seed, counts=counts, same_list=same_list)
    rng = np.random.default_rng(4409 + seed + E + N)
    d = cs["z"].shape[-1]

    def draw(L):
        z = (rng.standard_normal((L, E, N, d)) * 0.3).astype(np.float32)
        z[..., :2] = rng.uniform(0.0, 5.0, (L, E, N, 2)).astype(np.float32) - cs["xF"][None, None]
        return z

    done = np.zeros((T, E), np.uint8)
    for e in range(E):
        ends = [t for t in OO.WINDOW_ENDS[e % len(OO.WINDOW_ENDS)] if t < T]
        done[ends, e] = 1
    return dict(cs, z_all=draw(T + 1), z_final=draw(T), done=done, reward=rng.uniform(-3.0, 0.0, (T, E, N)).astype(np.float32))


def window_case(T, E, N, M, c=2, seed=0, counts=None, same_list=False):
    """`obstacle_ref.window_case` with a list per env: env 0 keeps its list (and the exact-touch record), env e > 0 holds
    `lists(E, M)[e]`, and its records are redrawn until the smallest gap under ITS list (the first counts[e] rows) is SEPARATION
    off 0.  The NaN record stays.  dict(z, done, xF, radius, obstacles [E,M,3], counts, c, z_final)."""
    w = OR.window_case(T, E, N, c, M, seed=seed)
    rng = np.random.default_rng(9157 + seed + 101 * T + 11 * E + N + M)
    obs = lists(E, M, seed)
    obs[0] = w["obstacles"]
    if same_list:
        obs = np.tile(obs[:1], (E, 1, 1))
    counts = np.full(E, M, np.int64) if counts is None else np.asarray(counts, np.int64)
    d = w["z"].shape[-1]
    i = np.tile(np.arange(N), T)
    for name in ("z", "z_final"):
        for e in range(0 if (counts[0] != M) else 1, E):
            if same_list and counts[e] == M:
                continue
            flat = np.ascontiguousarray(w[name][:, e]).reshape(T * N, d)
            for _ in range(200):
                if counts[e] == 0:
                    break
                g = OR.gaps(flat, w["xF"], w["radius"], obs[e, :counts[e]])[1].min(1)
                bad = np.abs(g) <= OR.SEPARATION
                if not bad.any():
                    break
                flat[bad, :2] = rng.uniform(0.0, 5.0, (int(bad.sum()), 2)).astype(np.float32) - w["xF"][i[bad]]
            else:
                raise AssertionError("window_case: records left within SEPARATION of gap = 0")
            w[name][:, e] = flat.reshape(T, N, d)
    return dict(w, obstacles=obs, counts=counts)
