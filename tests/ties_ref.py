"""Neighbour-list ties with the self entry: fixtures and a tie-aware NumPy float64 restatement (test infrastructure).

Written from the reference's drone_env.py:309-346 and SURVEY's rule for its argsort (stable, the lowest index first), not from
the kernels.  Row i of the clipped gap matrix holds the agent's own entry d_ii = min(-2 l_i, dhat_i); a partner sorts at or
ahead of it when it is exactly coincident with an agent of the same radius (an exact tie, the lower index wins) or when it is a
larger agent whose disk contains the smaller agent's centre (strictly ahead, whatever the index).  tests/test_ties_host.py pins
the oracle to this file, tests/test_gpu_ties.py the kernels to the oracle.

An EXACT tie is a pair of bitwise-equal float64 gaps.  The fixtures copy positions bitwise and use radii that float32 holds
exactly, so the float32 kernels see the same exact ties and both sides resolve them by index; `tie_margin` therefore leaves
them out and measures every other discrete decision."""
import functools

import numpy as np

from oracle.oracle import Oracle
from tests import helpers as H

E = 48
RADII = (0.0625, 0.125, 0.375)                # exact in float32
NEST_OFFSET = (0.0625, 0.03125)               # pattern (d): the smallest agent's centre inside the largest agent's disk
CLUSTER = 24                                  # pattern (c): more than the bucket filter's 10 candidates per agent
TIE_PATTERNS = "abcde"

# name: (N, G, k, c, heterogeneous radii, Delta given, geometry class, ASC list form)
CONFIGS = {
    "sym64-k1": (64, 28.0, 1, 2, False, True, "sym64", True),
    "sym64-k2": (64, 28.0, 2, 2, False, True, "sym64", True),
    "sym64-k8": (64, 28.0, 8, 2, False, True, "sym64", True),
    "block": (130, 60.0, 3, 2, False, True, "block", True),
    "block-hetero": (130, 60.0, 3, 2, True, True, "block", True),
    "u256": (256, 70.0, 2, 2, False, True, "u256", True),
    "big": (300, 81.0, 5, 2, False, True, "big", True),
    "big-hetero": (300, 140.0, 2, 2, True, True, "big", True),
    "big600-hetero": (600, 300.0, 2, 2, True, True, "big", True),
    "packed": (48, 24.0, 2, 2, False, True, "packed", False),
    "wave64-hetero": (64, 28.0, 2, 2, True, True, "wave64", False),
    "far-c5": (64, 28.0, 2, 5, False, True, "sym64", False),
    "far-none": (130, 60.0, 2, 2, False, False, "block", False),
}
ASC_CONFIGS = [n for n, cfg in CONFIGS.items() if cfg[7]]


def gaps(pos, radius, d_hat):
    """One env: the clipped gap matrix d_ij with the self entry on the diagonal (drone_env.py:309-325), and the unclipped
    off-diagonal gaps (diagonal: +inf)."""
    pos = np.asarray(pos, np.float64)
    radius, d_hat = np.asarray(radius, np.float64), np.asarray(d_hat, np.float64)
    N = pos.shape[0]
    dx = pos[:, None, 0] - pos[None, :, 0]
    dy = pos[:, None, 1] - pos[None, :, 1]
    raw = np.sqrt(dx * dx + dy * dy) - radius[:, None] - radius[None, :]
    d = np.minimum(raw, d_hat[:, None])
    d[d == 0] = -1e-6
    eye = np.eye(N, dtype=bool)
    d[eye] = np.minimum(-radius - radius, d_hat)
    raw[eye] = np.inf
    return d, raw


def lists(pos, radius, d_hat, k, delta=None):
    """nbr_idx [E, N, k+1] int32 and n_coll [E] as the oracle packs them: slot 0 is the agent, slot kth = 1..k is entry kth of
    the STABLE argsort of row i -- the agent itself where a partner precedes it -- or -1 beyond the agent's in-range count
    (drone_env.py:346, 362: entries with d_ij <= Delta_j, minus itself; with Delta < dhat those are unclipped entries).
    delta=None is the reference's default Delta = dhat (:85-89)."""
    pos = np.asarray(pos, np.float64)
    pos = pos.reshape((-1,) + pos.shape[-2:])
    delta = np.asarray(d_hat if delta is None else delta, np.float64)
    nE, N = pos.shape[:2]
    nbr = np.full((nE, N, k + 1), -1, np.int32)
    n_coll = np.zeros(nE, np.int32)
    off = ~np.eye(N, dtype=bool)
    for e in range(nE):
        d, _ = gaps(pos[e], radius, d_hat)
        order = np.argsort(d, axis=1, kind="stable")[:, :k + 1]
        in_range = (d <= delta[None, :]).sum(1) - 1
        valid = np.arange(k + 1)[None, :] <= in_range[:, None]
        nbr[e] = np.where(valid, order, -1)
        nbr[e, :, 0] = np.arange(N)
        n_coll[e] = int(((d < 0) & off).sum())        # dhat_i / d_ij <= 0 (:327), d == 0 having become -1e-6
    return nbr, n_coll


def preceded(pos, radius, d_hat):
    """[E] bool: some agent's row has a partner ahead of or tied with the self entry."""
    pos = np.asarray(pos, np.float64)
    out = np.zeros(pos.shape[0], bool)
    for e in range(pos.shape[0]):
        d, _ = gaps(pos[e], radius, d_hat)
        off = ~np.eye(d.shape[0], dtype=bool)
        out[e] = bool(((d <= np.diag(d)[:, None]) & off).any())
    return out


def tie_margin(pos, radius, d_hat, delta, k):
    """[E]: the distance of every discrete decision from its threshold, exact ties left out: the collision test |gap|, the clip
    |gap - dhat_i|, the Delta mask |min(gap, dhat_i) - Delta_j|, and the differences of adjacent entries among the first k+3 of
    each sorted row that are neither exactly 0 nor between two clipped entries."""
    pos = np.asarray(pos, np.float64)
    d_hat, delta = np.asarray(d_hat, np.float64), np.asarray(delta, np.float64)
    out = np.empty(pos.shape[0])
    for e in range(pos.shape[0]):
        d, raw = gaps(pos[e], radius, d_hat)
        N = d.shape[0]
        off = ~np.eye(N, dtype=bool)
        m = np.abs(d[off]).min()
        m = min(m, np.abs(raw - d_hat[:, None])[off].min())
        mask = np.abs(d - delta[None, :])[off]          # Delta = dhat (the default): a clipped entry meets it exactly
        m = min(m, mask[mask != 0].min())
        s = np.sort(d, axis=1)[:, :k + 3]
        diff = np.diff(s, axis=1)
        clipped = s >= d_hat[:, None]
        count = (diff != 0) & ~(clipped[:, :-1] & clipped[:, 1:])
        if count.any():
            m = min(m, diff[count].min())
        out[e] = m
    return out


def row_tie_free(pos, radius, d_hat, k):
    """[E, N] bool, as tests/golden/gen_golden.py defines it: no two adjacent clipped entries among the first k+2 of the sorted
    row, i.e. the agent a ghost row borrows v and l from (c = 5) does not depend on the tie order."""
    pos = np.asarray(pos, np.float64)
    d_hat = np.asarray(d_hat, np.float64)
    out = np.ones(pos.shape[:2], bool)
    for e in range(pos.shape[0]):
        d, _ = gaps(pos[e], radius, d_hat)
        clipped = np.sort(d, axis=1)[:, :k + 2] >= d_hat[:, None]
        out[e] = ~(clipped[:, :-1] & clipped[:, 1:]).any(1)
    return out


def patterns(N, G, n_envs, rng, radius=None, reach=None):
    """float32 positions [E, N, 2] = G/2 + U(-0.3 G, 0.3 G) with one tie pattern written into each env, repeated over the env
    axis; the pattern letters [E]; and per env the groups of agents that have to move together for the pattern to persist.
      a  one coincident pair far apart in index: N-3 onto 1
      b  a coincident triple: 5, 9, N-1
      c  a coincident pair inside a cluster of 24 agents within +-1.2 reach of one point
      d  (heterogeneous radii) the smallest agent NEST_OFFSET off the centre of the largest: nested, not coincident
      e  (heterogeneous radii) the smallest agent exactly on the largest, the larger agent having the higher index
      f  no tie
    Positions are copied bitwise, so a tie is exact in float32 and in float64."""
    letters = "abcdef" if radius is not None else "abcf"
    pos = (G / 2 + rng.uniform(-0.3 * G, 0.3 * G, (n_envs, N, 2))).astype(np.float32)
    pat = np.array([letters[e % len(letters)] for e in range(n_envs)])
    cluster = np.arange(CLUSTER) * (N // CLUSTER)
    groups = []
    if radius is not None:
        small = int(np.argmin(radius))
        large = int(N - 1 - np.argmax(np.asarray(radius)[::-1]))
        assert radius[small] < radius[large] and small < large
    for e in range(n_envs):
        if pat[e] == "a":
            pos[e, N - 3] = pos[e, 1]
            groups.append([[1, N - 3]])
        elif pat[e] == "b":
            pos[e, 9] = pos[e, 5]
            pos[e, N - 1] = pos[e, 5]
            groups.append([[5, 9, N - 1]])
        elif pat[e] == "c":
            centre = (G / 2 + rng.uniform(-0.2 * G, 0.2 * G, 2))
            pos[e, cluster] = (centre + rng.uniform(-1.2 * reach, 1.2 * reach, (CLUSTER, 2))).astype(np.float32)
            pos[e, cluster[20]] = pos[e, cluster[3]]
            groups.append([[int(cluster[3]), int(cluster[20])]])
        elif pat[e] == "d":
            pos[e, small] = pos[e, large] + np.asarray(NEST_OFFSET, np.float32)
            groups.append([[small, large]])
        elif pat[e] == "e":
            pos[e, small] = pos[e, large]
            groups.append([[small, large]])
        else:
            groups.append([])
    return pos, pat, groups


class Fixture:
    """One configuration of CONFIGS: positions, constants, the oracle and what it gives on the positions (computed once)."""

    def __init__(self, name):
        self.name = name
        self.N, self.G, self.k, self.c, self.hetero, given, self.cls, self.asc = CONFIGS[name]
        N, G, k = self.N, self.G, self.k
        rng = np.random.default_rng(N + k)
        self.radius = rng.choice(RADII, N) if self.hetero else None
        d_hat = Oracle(N, [G, G], k, None, self.c == 2, radius=self.radius).d_hat
        self.delta = np.ones(N) * 0.47 * d_hat.min() if given else None
        self.orc = Oracle(N, [G, G], k, self.delta, self.c == 2, radius=self.radius, threads=4)
        self.d_hat = self.orc.d_hat
        self.l = self.orc.radius
        self.pos, self.pat, self.groups = patterns(N, G, E, rng, self.radius, reach=float(d_hat.max() + 2 * self.l.max()))
        self.pos64 = self.pos.astype(np.float64)
        self.margin = tie_margin(self.pos64, self.l, self.d_hat, self.orc.delta, k)
        self.kept = self.margin > H.MARGIN
        self.ref = self.orc.observe(self.pos64)
        self.row_tie_free = row_tie_free(self.pos64, self.l, self.d_hat, k) if self.c == 5 else None

    def kept_after(self, pos64):
        return tie_margin(pos64, self.l, self.d_hat, self.orc.delta, self.k) > H.MARGIN


@functools.lru_cache(maxsize=None)
def fixture(name):
    return Fixture(name)
