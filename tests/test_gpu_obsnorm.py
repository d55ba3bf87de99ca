"""GPU tests of the observation normaliser's kernels (csrc/obsnorm.hip) through `ObsNormalizer`: the running statistics against
the float64 restatement (tests/obsnorm_ref.py) over four successive windows, the exact cases, determinism (run to run, and
16-byte against 4-byte aligned inputs) and the map.  Shapes: C = N d = 30 (4-byte path), 36 (C % 4 == 0 but not % 64), 384
(% 64), 1050 (two column tiles, odd), 1536 and 1028 (257 lane groups of four: the tile capped at 256, a second tile with one live
group); windows of 4099, 64, 1 and 777 rows."""
import pytest

from tests import obsnorm_ref as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"N{n}d{d}" for n, d in OR.SHAPES]
_WINDOWS = {}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


def windows(shape):
    """The four windows of a shape on the host and on the device, made once."""
    if shape not in _WINDOWS:
        host = OR.windows(*shape)
        _WINDOWS[shape] = (host, [w.to(DEV) for w in host])
    return _WINDOWS[shape]


def make(shape, **kw):
    from scalable_collision_avoidance_rl_amd.obs_norm import ObsNormalizer
    return ObsNormalizer(shape[0], shape[1], DEV, **kw)


def fitted(shape, **kw):
    norm = make(shape, **kw)
    for w in windows(shape)[1]:
        norm.update(w)
    return norm


def offset_view(torch, x):
    """The same values in memory that is 4-byte but not 16-byte aligned."""
    buf = torch.empty(x.numel() + 1, device=x.device)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and x.data_ptr() % 16 == 0 and v.is_contiguous()
    return v


# 1 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OR.SHAPES, ids=IDS)
def test_update_matches_the_two_pass_moments_of_the_concatenated_windows(torch, shape):
    """After every window: count exact, mean within 1e-10 max|x| of the column, m2 within rtol 1e-10 of the two-pass float64
    moments over the finite values of everything seen so far (float64 sums of <= 4099 terms are good to about 5e-13); the table
    within rtol 1e-9 of its definition on the state; the all-NaN column's state bit-unchanged by its window."""
    host, dev = windows(shape)
    C = shape[0] * shape[1]
    norm = make(shape)
    worst_mean = worst_m2 = 0.0
    for k, w in enumerate(dev):
        before = norm.state.clone()
        norm.update(w.view(w.shape[0], shape[0], shape[1]))                  # [R,N,d]: leading dims are rows
        torch.cuda.synchronize()
        state, tab = norm.state.view(3, C).cpu(), norm.table.view(2, C).cpu()
        ref = OR.moments(torch.cat(host[:k + 1]))
        scale = OR.column_max(host[:k + 1])
        assert torch.equal(state[0], ref[0]), f"window {k}: count"
        err_mean = ((state[1] - ref[1]).abs() / scale.clamp(min=1e-300)).max()
        rel_m2 = ((state[2] - ref[2]).abs() / ref[2].clamp(min=1e-300))[ref[2] > 0].max()
        worst_mean, worst_m2 = max(worst_mean, float(err_mean)), max(worst_m2, float(rel_m2))
        assert torch.all((state[1] - ref[1]).abs() <= 1e-10 * scale), f"window {k}: mean, worst {float(err_mean):.3e} max|x|"
        assert torch.all((state[2] - ref[2]).abs() <= 1e-10 * ref[2].abs()), f"window {k}: m2, worst relative {float(rel_m2):.3e}"
        want = OR.table(state, norm.eps)
        assert torch.allclose(tab, want, rtol=1e-9, atol=0), f"window {k}: table"
        if k == OR.NAN_WINDOW:
            assert torch.equal(norm.state.view(3, C)[:, OR.NAN_COLUMN], before.view(3, C)[:, OR.NAN_COLUMN])
            assert not torch.equal(norm.state.view(3, C)[:, OR.HARD], before.view(3, C)[:, OR.HARD])
        assert torch.equal(norm.count.view(C).cpu(), ref[0]) and torch.equal(norm.mean.view(C).cpu(), state[1])
        assert torch.allclose(norm.var.view(C).cpu(), state[2] / state[0].clamp(min=1.0), rtol=1e-15, atol=0)
    print(f"{shape}: worst |mean - ref| / max|x| {worst_mean:.3e}, worst relative m2 error {worst_m2:.3e}")


# 2 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OR.SHAPES, ids=IDS)
def test_exact_cases(torch, shape):
    host, dev = windows(shape)
    C = shape[0] * shape[1]
    norm = fitted(shape)
    assert float(norm.state.view(3, C)[2, OR.CONSTANT]) == 0.0
    assert float(norm.state.view(3, C)[1, OR.CONSTANT]) == OR.CONSTANT_VALUE
    for w in dev:
        assert torch.all(norm(w)[:, OR.CONSTANT] == 0.0)
    # a fresh normaliser without a clamp is the identity on finite values (and keeps NaN and inf what they are)
    fresh = make(shape, clip=None)
    for h, w in zip(host, dev):
        y = fresh.norm(w)
        fin = torch.isfinite(w)
        assert torch.equal(y[fin], w[fin]) and torch.equal(torch.isnan(y), torch.isnan(w)) and torch.equal(torch.isinf(y), torch.isinf(w))
    x = torch.randn(257, C, device=DEV)
    assert torch.equal(fresh.norm(x), x)
    # reset: back to the identity
    norm.reset()
    assert float(norm.state.abs().sum()) == 0 and torch.equal(norm.table, fresh.table)


# 3 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OR.SHAPES, ids=IDS)
def test_bits_do_not_depend_on_the_run_or_the_alignment(torch, shape):
    _, dev = windows(shape)
    a, b, c = fitted(shape), fitted(shape), make(shape)
    for w in dev:
        c.update(offset_view(torch, w))
    torch.cuda.synchronize()
    assert torch.equal(a.state, b.state) and torch.equal(a.table, b.table)
    assert torch.equal(a.state, c.state) and torch.equal(a.table, c.table)
    nan_eq = lambda p, q: torch.equal(torch.nan_to_num(p, nan=12345.0), torch.nan_to_num(q, nan=12345.0))
    for w in dev:
        y = a.norm(w).clone()
        v = offset_view(torch, w)
        out = offset_view(torch, torch.zeros_like(w))
        assert nan_eq(a.norm(v, out=out), y)                                  # both 4-byte aligned
        assert nan_eq(a.norm(v), y) and nan_eq(a.norm(w, out=out), y)         # one of the two
        assert nan_eq(b.norm(w), y)


# 4 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", OR.SHAPES, ids=IDS)
def test_apply_matches_the_restatement(torch, shape):
    """R = 4099, 64 and 1 rows (the first three windows) x clip 10, 0.5 and none, at the project's plain bar
    |a - b| <= 1e-5 + 1e-5 |ref| against the float64 map with the device's own table.  NaN exactly where the input has it; +inf
    gives clip, or +inf without a clamp; in place equals out of place bit for bit."""
    host, dev = windows(shape)
    C = shape[0] * shape[1]
    stats = fitted(shape)
    tab = stats.table.view(2, C).cpu()
    assert [w.shape[0] for w in host[:3]] == [4099, 64, 1]
    for clip in (10.0, 0.5, None):
        norm = fitted(shape, clip=clip)
        assert torch.equal(norm.table, stats.table)
        for h, w in zip(host[:3], dev[:3]):
            y = norm.norm(w.view(-1, shape[0], shape[1])).view(-1, C)
            ref = OR.apply(h, tab, clip)
            got = y.double().cpu()
            assert torch.equal(torch.isnan(got), torch.isnan(h)), (clip, h.shape[0])
            assert float(got[0, OR.INF_COLUMN]) == (float("inf") if clip is None else clip)
            ok = torch.isfinite(ref)
            assert torch.equal(ok, torch.isfinite(got))
            err = (got[ok] - ref[ok]).abs() - (1e-5 + 1e-5 * ref[ok].abs())
            assert float(err.max()) <= 0, (clip, h.shape[0], float(err.max()))
            if clip is not None:
                assert float(got[ok].abs().max()) <= clip
                assert bool((got[ok].abs() == clip).any())                               # the clamp is exercised
            inplace = w.clone()
            assert norm.norm(inplace, out=inplace) is inplace
            assert torch.equal(torch.nan_to_num(inplace, nan=777.0), torch.nan_to_num(y, nan=777.0))
    # the owned output buffer is reused per input shape
    assert norm.norm(dev[0]).data_ptr() == norm.norm(dev[0]).data_ptr() != norm.norm(dev[1]).data_ptr()


def test_wrapper_rejects_what_is_not_a_row_matrix_of_its_columns(torch):
    norm = make((5, 6))
    for bad in (torch.zeros(7, 5, 5, device=DEV), torch.zeros(31, device=DEV), torch.zeros(4, 6, 6, device=DEV)):
        with pytest.raises(ValueError, match="flatten"):
            norm.update(bad)
    with pytest.raises(ValueError, match="out must be"):
        norm.norm(torch.zeros(4, 5, 6, device=DEV), out=torch.zeros(4, 30, device=DEV))
    x = torch.randn(3, 2, 5, 3, 2, device=DEV)                                # [T,E,N,k+1,c]
    norm.update(x)
    assert float(norm.count.min()) == float(norm.count.max()) == 6.0
    assert tuple(norm.norm(x).shape) == tuple(x.shape)
