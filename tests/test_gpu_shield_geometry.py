"""Action shield on the device, where tests/test_gpu_shield.py does not look: every record shape and load path with unequal
radii, the parameter edges, the geometry the incremental solve is about (tests/shield_ref.families), huge finite actions, and
the guarantee of DESIGN.md on the kernel's own output.

The reference is the float64 brute force of tests/shield_ref.py and the bar its derived `tolerance`, both unchanged: per record
FEASIBLE (a.u* - b <= tol) and OPTIMAL.  Optimality is |u* - u| <= |u_ref - u| + tol, except in the families whose answer is a
vertex of two lines at a small angle theta (`near_parallel`, `wedge` and the permuted copies of `wedge`): a vertex moves by
eps / sin(theta) under rounding of its lines, so no bar on its position follows from the number format.  There the bar is the
backward-stable one, |u* - u| <= dist(u, C(B - tol)) + tol with C(B - tol) the restatement's answer after every finite b was
lowered by tol: with feasibility, the kernel's answer lies between the exact answers of two problems tol apart."""
import ctypes as C

import numpy as np
import pytest

from tests import shield_ref as S
from tests.test_gpu_shield import BAND_CAP, dev, host, stand_in_env

pytestmark = pytest.mark.gpu
EPS32 = S.EPS32


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fams():
    return S.families()


@pytest.fixture(scope="module")
def refs():
    """References computed once per module and shared: name -> `S.reference` (shapes) or a list per block (families)."""
    return {}


def family_refs(refs, fams, name):
    if name not in refs:
        refs[name] = [(label, e0, e1, S.block_reference(fams[name], e0, e1)) for label, e0, e1 in fams[name]["blocks"]]
    return refs[name]


def launch(torch, recs, c, rate, margin, u_max, offset=0, stats=False):
    """One `ActionShield` call on the records; z at `offset` bytes past a 16-byte boundary.  Host arrays (u*, intervened,
    correction), the shield and the address of z."""
    from scalable_collision_avoidance_rl_amd import ActionShield
    E, N, k1 = recs["nbr"].shape
    sh = ActionShield(stand_in_env(torch, E, N, k1 - 1, c, recs["radius"]), rate, margin, None if np.isinf(u_max) else u_max, stats=stats)
    z = dev(torch, recs["z"], offset)
    out = sh(dev(torch, recs["u"]), z=z, nbr=dev(torch, recs["nbr"]))
    return (host(out), host(sh.intervened), host(sh.correction)), sh, z.data_ptr()


def check(what, got, ref, lowered=False):
    """The bars of tests/test_gpu_shield.check_against_ref on (u*, intervened, correction) against a `S.reference` -- or any `ref`
    with the same entries over MORE constraint columns (`obstacle_ref.shield_reference`: the obstacle slots appended; nothing here
    or in `S.lowered` depends on the count); `lowered`: the backward-stable optimality bar of the module docstring.  Returns the per-record residuals (feasibility, optimality
    excess) and tol."""
    o, iv, corr = got
    A, B, tol, ustar, riv, slack = (ref[n] for n in ("A", "B", "tol", "ustar", "intervened", "min_slack"))
    R = B.shape[0]
    u2 = ref["u"].reshape(R, 2)
    o, iv, corr = o.reshape(R, 2), iv.reshape(R).astype(bool), corr.reshape(R)
    fin = np.isfinite(u2).all(1)
    o64, u64 = o.astype(np.float64), u2.astype(np.float64)
    with np.errstate(invalid="ignore"):
        feas_r = np.where(fin, ((A * o64[:, None, :]).sum(2) - B).max(1), -np.inf)
        target = S.lowered(ref, tol) if lowered else ustar
        d_got, d_ref = np.linalg.norm(o64 - u64, axis=1), np.linalg.norm(target - u64, axis=1)
    opt_r = np.where(fin, d_got - d_ref, -np.inf)
    feas, opt, band = feas_r.max(), opt_r.max(), slack <= tol
    print(f"{what}: tol {tol:.3e}; feasibility residual {feas:.3e} ({feas / tol:.3f} tol); optimality excess "
          f"({'lowered' if lowered else 'plain'}) {opt:.3e} ({opt / tol:.3f} tol); intervened {iv.mean():.3f}; flag band {band.mean():.4f}")
    assert np.isfinite(o[fin]).all(), what
    assert feas <= tol, (what, feas, tol)
    assert opt <= tol, (what, opt, tol)
    assert band.mean() <= BAND_CAP, (what, band.mean())
    assert np.array_equal(iv[~band], riv[~band]), what
    # pass-through: u's own bits, correction 0; a non-finite u: copied through, flag 0, correction NaN
    assert np.array_equal(o[~iv].view(np.uint32), u2[~iv].view(np.uint32)), what
    assert (corr[~iv & fin] == 0).all() and np.isnan(corr[~fin]).all() and not iv[~fin].any(), what
    assert np.abs(corr[iv].astype(np.float64) - d_got[iv]).max(initial=0.0) <= tol, what
    return feas_r, opt_r, tol


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- (a) record shapes and load paths
def shape_records(shape):
    N, k, c = shape
    return S.synthetic(N, k, c, E=S.WIDE_E if shape == S.WIDE_SHAPE else S.E_CASE, radius=S.radii(N))


@pytest.mark.parametrize("shape", S.GEOMETRY_SHAPES + [S.WIDE_SHAPE], ids=lambda s: "N%dk%dc%d" % s)
def test_every_record_shape_and_load_path_with_unequal_radii(torch, shape):
    """c = 2 with k + 1 even at a 16-byte base: (k + 1) / 2 16-byte loads, rows 2h - 1 and 2h out of one load for h > 0.  The same
    records with z at +8 (8-byte loads) and +4 (dword loads): the same bits."""
    N, k, c = shape
    ref = S.reference(shape_records(shape), c)
    assert len(np.unique(ref["radius"])) >= min(N, 8)
    got, _, ptr = launch(torch, ref, c, S.RATE, S.MARGIN, S.U_MAX)
    assert ptr % 16 == 0
    if c == 2 and k in (3, 5, 7):
        assert (k + 1) % 2 == 0 and (k + 1) // 2 > 1                               # the 16-byte path with more than one load
    check(f"shape {shape}", got, ref)
    if c == 2:
        for offset in (8, 4):
            shifted, _, ptr = launch(torch, ref, c, S.RATE, S.MARGIN, S.U_MAX, offset=offset)
            assert ptr % 16 == offset
            assert same_bits(got, shifted), (shape, offset)


# ---------------------------------------------------------------------------------------------- (b) parameter sets
@pytest.mark.parametrize("shape", S.PARAMETER_SHAPES, ids=lambda s: "N%dk%dc%d" % s)
@pytest.mark.parametrize("params", S.PARAMETER_SETS, ids=lambda p: "rate%g-margin%g-box%g" % p)
def test_parameter_sets(torch, params, shape):
    N, k, c = shape
    rate, margin, u_max = params
    ref = S.reference(S.synthetic(N, k, c, radius=S.radii(N), margin=margin, u_max=u_max), c, rate, margin, u_max)
    got, _, _ = launch(torch, ref, c, rate, margin, u_max)
    check(f"shape {shape} rate {rate} margin {margin} u_max {u_max}", got, ref)


def test_entry_point_at_another_dt(torch):
    """`ActionShield` passes the env's dt = 0.05; the entry point itself at dt = 0.02 against the restatement at that dt."""
    from scalable_collision_avoidance_rl_amd import _native
    N, k, c = shape = (4, 3, 2)
    dt = 0.02
    ref = S.reference(shape_records(shape), c, dt=dt)
    u, z, nbr, radius = dev(torch, ref["u"]), dev(torch, ref["z"]), dev(torch, ref["nbr"]), dev(torch, ref["radius"])
    out = torch.empty_like(u)
    iv = torch.zeros(S.E_CASE, N, dtype=torch.uint8, device="cuda:0")
    corr = torch.zeros(S.E_CASE, N, dtype=torch.float32, device="cuda:0")
    rc = _native.lib().dronesim_action_shield(z.data_ptr(), nbr.data_ptr(), u.data_ptr(), radius.data_ptr(), S.RATE, S.MARGIN, S.U_MAX, dt,
                                              S.E_CASE, N, k + 1, c, out.data_ptr(), iv.data_ptr(), corr.data_ptr(),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    check("dt = 0.02", (host(out), host(iv), host(corr)), ref)


# ---------------------------------------------------------------------------------------------- (c) families
def per_bucket(what, key, feas_r, opt_r, tol):
    for v in np.unique(key):
        print(f"  {what} {v}: feasibility {feas_r[key == v].max() / tol:.3f} tol, optimality {opt_r[key == v].max() / tol:.3f} tol")


@pytest.mark.parametrize("name", [n for n in S.FAMILY_NAMES if not n.startswith("magnitude")])
def test_family_is_feasible_and_optimal(torch, fams, refs, name):
    fam = fams[name]
    E, N, k1 = fam["nbr"].shape
    (o, iv, corr), _, _ = launch(torch, fam, fam["c"], fam["rate"], fam["margin"], fam["u_max"])
    lowered = name.startswith(S.ILL_CONDITIONED)
    for label, e0, e1, ref in family_refs(refs, fams, name):
        feas_r, opt_r, tol = check(f"{name} {label}", (o[e0:e1], iv[e0:e1], corr[e0:e1]), ref, lowered=lowered)
        if name.startswith("near_parallel"):
            per_bucket("e =", fam["e"][e0 * N:e1 * N], feas_r, opt_r, tol)
        if "crowd" in name:                                                        # 0 is the only feasible action
            point = fam["point"][e0 * N:e1 * N]
            worst = np.abs(o[e0:e1].reshape(-1, 2)[point]).max()
            print(f"  {name} {label}: |u*| where the set is {{0}}: {worst:.3e} ({worst / tol:.3f} tol), {point.sum()} records")
            assert point.sum() >= 100 and worst <= tol
    if name.startswith("order"):
        # every copy met the bars above; a record's flag does not depend on the order of its slots, and where it passes through,
        # neither do the bits
        q, E0 = fam["copies"], fam["E0"]
        assert q * E0 == E
        for copy in range(1, q):
            lo = copy * E0
            assert np.array_equal(iv[:E0], iv[lo:lo + E0]), name
            still = iv[:E0] == 0
            assert np.array_equal(o[:E0][still].view(np.uint32), o[lo:lo + E0][still].view(np.uint32)), name
            assert np.array_equal(corr[:E0][still].view(np.uint32), corr[lo:lo + E0][still].view(np.uint32)), name


# ---------------------------------------------------------------------------------------------- (d) magnitude
@pytest.mark.parametrize("name", [n for n in S.FAMILY_NAMES if n.startswith("magnitude")])
def test_huge_finite_actions(torch, fams, refs, name):
    """|u| = 2^10 .. 2^100: u* finite and inside the bars (tol scales with |u| by its own formula); the correction finite and within
    4 eps32 of |u* - u| relative (u* - u rounded once, a product, an fma, a root: 2.5 eps32) -- every |u* - u| here is
    representable in float32; the running sum of one call finite and the float64 sum of the plane."""
    fam = fams[name]
    E, N, _ = fam["nbr"].shape
    (o, iv, corr), sh, _ = launch(torch, fam, fam["c"], fam["rate"], fam["margin"], fam["u_max"], stats=True)
    assert np.isfinite(o).all() and np.isfinite(corr).all()
    for label, e0, e1, ref in family_refs(refs, fams, name):
        check(f"{name} {label}", (o[e0:e1], iv[e0:e1], corr[e0:e1]), ref)
        d = np.linalg.norm(o[e0:e1].astype(np.float64) - fam["u"][e0:e1].astype(np.float64), axis=2)
        assert d.max() < 2.0 ** 127 and iv[e0:e1].mean() >= 0.5
        rel = (np.abs(corr[e0:e1].astype(np.float64) - d) / np.maximum(d, 1e-300))[iv[e0:e1] != 0].max()
        print(f"  {name} {label}: correction off by {rel / EPS32:.2f} eps32 relative at most")
        assert rel <= 4 * EPS32, (name, label, rel)
    t = sh.totals()
    total, want = host(t["correction_sum"]), corr.astype(np.float64).sum(0)
    assert np.isfinite(total).all() and (np.abs(total - want) <= 1e-6 * want).all()
    assert np.array_equal(host(t["correction_max"]), corr.max(0)) and int(host(t["nonfinite"]).sum()) == 0


# ---------------------------------------------------------------------------------------------- (e) the guarantee
@pytest.mark.parametrize("rate", [0.25, 0.5])
@pytest.mark.parametrize("N,E", [(2, 512), (4, 256), (9, 112)])
def test_the_guarantee_holds_on_the_kernels_output(torch, N, E, rate):
    """Everyone lists everyone, unequal radii, float32 positions, rows p = float32(x_j - x_i).  After x' = x + dt u* in float64
    every pair keeps g' >= (1 - 2 rate) max(g, 0) + min(g, 0) - slack, slack = 2 dt tol + 4 eps32 D: two agents' feasibility
    residuals times dt and the rounding of the float32 differences.  No reference: DESIGN.md's statement."""
    w = S.mutual(N, E)
    rad = w["radius"].astype(np.float64)
    assert len(np.unique(rad)) == N
    (o, iv, _), _, ptr = launch(torch, w, 2, rate, S.MARGIN, S.U_MAX)
    if N == 4:
        assert ptr % 16 == 0                                                       # k + 1 = 4: the two-load 16-byte path
    tol = S.tolerance(w["u"], w["z"], N, 2, rad, rate, S.MARGIN, S.U_MAX, S.DT)
    x = w["pos"].astype(np.float64)
    after = x + S.DT * o.astype(np.float64)
    iu, ju = np.triu_indices(N, 1)
    gap = lambda p: np.linalg.norm(p[:, iu] - p[:, ju], axis=2) - rad[iu] - rad[ju] - S.MARGIN
    g, g_after = gap(x), gap(after)
    D = np.linalg.norm(x[:, iu] - x[:, ju], axis=2).max()
    slack = 2 * S.DT * tol + 4 * EPS32 * D
    short = (1 - 2 * rate) * np.maximum(g, 0) + np.minimum(g, 0) - g_after
    print(f"N={N} rate={rate}: gaps {g.min():.3f} .. {g.max():.3f}, below the margin {np.mean(g < 0):.3f}; intervened {iv.mean():.3f}; "
          f"largest shortfall {short.max():.3e} (slack {slack:.3e}); pairs within 1e-3 of the bound {np.mean(short > -1e-3):.3f}")
    assert (g < 0).mean() >= 0.05 and g.max() > 0.3 and iv.mean() >= 0.5           # the draw: both regimes, mostly intervening
    assert (short > -1e-3).mean() >= 0.05                                          # the bound is attained, not merely respected
    assert short.max() <= slack, (N, rate, short.max(), slack)
