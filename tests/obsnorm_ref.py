"""Float64 restatement of the observation normaliser (csrc/obsnorm.hip, include/dronesim.h: dronesim_obsnorm_update /
dronesim_obsnorm_apply): the two-pass moments over the finite values, Chan's merge, the table and the map -- and the inputs of
the GPU tests, made here once so that the host tier can check that they do their job."""
import torch

SHAPES = [(5, 6), (6, 6), (64, 6), (70, 15), (256, 6), (257, 4)]      # (N, d): C = 30, 36, 384, 1050, 1536, 1028
WINDOW_ROWS = (4099, 64, 1, 777)
HARD, CONSTANT, SMALL, WIDE, INF_COLUMN, NAN_COLUMN = 0, 1, 2, 3, 4, 5
CONSTANT_VALUE = 3.25
NAN_WINDOW = 1                                               # the window in which NAN_COLUMN is entirely NaN


def windows(N, d, seed=0):
    """Four successive float32 windows ``[R, N d]``, R = 4099, 64, 1, 777.  Column HARD drifts, -500 + 0.3 k +- 0.5 in window k;
    CONSTANT is one value; SMALL is scaled by 1e-3; WIDE is 256 +- 100; the rest are normal with a scale per column.  About 1 %
    NaN are scattered (none in CONSTANT), every window has one +inf (row 0 of INF_COLUMN), and in window NAN_WINDOW the column
    NAN_COLUMN is entirely NaN."""
    C = N * d
    gen = torch.Generator().manual_seed(1000 * N + d + seed)
    scale = torch.exp(torch.randn(C, generator=gen, dtype=torch.float64))
    shift = torch.randn(C, generator=gen, dtype=torch.float64) * 10
    out = []
    for k, R in enumerate(WINDOW_ROWS):
        x = torch.randn(R, C, generator=gen, dtype=torch.float64) * scale + shift
        u = torch.rand(R, 3, generator=gen, dtype=torch.float64)
        x[:, HARD] = -500 + 0.3 * k + (u[:, 0] - 0.5)
        x[:, CONSTANT] = CONSTANT_VALUE
        x[:, SMALL] = torch.randn(R, generator=gen, dtype=torch.float64) * 1e-3
        x[:, WIDE] = 256 + 200 * (u[:, 1] - 0.5)
        x = x.float()
        nan = torch.rand(R, C, generator=gen) < 0.01
        nan[:, CONSTANT] = False
        x[nan] = float("nan")
        x[0, INF_COLUMN] = float("inf")
        if k == NAN_WINDOW:
            x[:, NAN_COLUMN] = float("nan")
        out.append(x)
    return out


def moments(x):
    """``(n, mean, m2)`` per column of ``x [R, C]`` over its FINITE values, two passes in float64 (0, 0, 0 where there is none)."""
    x = x.double().reshape(-1, x.shape[-1])
    fin = torch.isfinite(x)
    n = fin.sum(0).double()
    xz = torch.where(fin, x, torch.zeros_like(x))
    mean = xz.sum(0) / n.clamp(min=1.0)
    dev = torch.where(fin, x - mean, torch.zeros_like(x))
    return torch.stack([n, torch.where(n > 0, mean, torch.zeros_like(mean)), (dev * dev).sum(0)])


def merge(state, batch):
    """Chan's rule on ``[3, C]`` triples; a column with ``n_b = 0`` keeps its state."""
    n, mean, m2 = state
    nb, mb, qb = batch
    tot = n + nb
    safe = tot.clamp(min=1.0)
    d = mb - mean
    new = torch.stack([tot, mean + d * nb / safe, m2 + qb + d * d * n * nb / safe])
    return torch.where((nb > 0)[None], new, state)


def table(state, eps):
    """``[2, C]``: ``(mean, 1 / sqrt(m2 / count + eps))``; 0 where that denominator is 0; ``(0, 1)`` where the count is 0."""
    n, mean, m2 = state
    seen = n > 0
    var = torch.where(seen, m2 / n.clamp(min=1.0) + eps, torch.ones_like(n))
    inv = torch.where(var > 0, 1.0 / torch.sqrt(var), torch.zeros_like(var))
    return torch.stack([torch.where(seen, mean, torch.zeros_like(mean)), torch.where(seen, inv, torch.ones_like(inv))])


def apply(x, tab, clip=None):
    """The map in float64 (before the rounding to float32): ``(x - mean) inv`` clamped to ``[-clip, clip]``; NaN stays NaN."""
    y = (x.double().reshape(-1, tab.shape[-1]) - tab[0]) * tab[1]
    if clip is not None:
        y = torch.where(y > clip, torch.full_like(y, clip), torch.where(y < -clip, torch.full_like(y, -clip), y))
    return y.reshape(x.shape)


def moments_float32(x):
    """The plausible wrong kernel: float32 running sums of x and x^2 over the finite values, m2 = sum x^2 - (sum x)^2 / n."""
    x = x.reshape(-1, x.shape[-1]).float()
    fin = torch.isfinite(x)
    s = torch.zeros(x.shape[1], dtype=torch.float32)
    s2 = torch.zeros(x.shape[1], dtype=torch.float32)
    for r in range(x.shape[0]):
        v = torch.where(fin[r], x[r], torch.zeros_like(x[r]))
        s = s + v
        s2 = s2 + v * v
    n = fin.sum(0).float()
    return torch.stack([n, s / n.clamp(min=1.0), s2 - s * s / n.clamp(min=1.0)]).double()


def column_max(ws):
    """max |x| per column over the finite values of the windows ``ws``."""
    x = torch.cat(ws).double()
    return torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).max(0).values

