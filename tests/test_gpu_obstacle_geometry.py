"""The obstacle shield (`dronesim_action_shield_obstacles`, csrc/shield.hip) where tests/test_gpu_obstacles.py does not look: every
list width m with more discs in range than slots, `obstacle_rate` at the shield's rate, 0.5 and 1, margin 0 without a box, the
load paths of z with a field, the geometry families of `shield_ref.families` with their lines moved INTO the list (the list
slots are the last lines of the incremental solve, where `slack` relaxes every earlier neighbour and obstacle line), the `on`
rule of a list slot, and the per-step guarantee of DESIGN.md on the kernel's own output.

The reference is the float64 brute force (tests/obstacle_ref.py on tests/shield_ref.py), the bar `obstacle_ref.tolerance`, the
checks `test_gpu_shield.check_against_ref` and `test_gpu_shield_geometry.check` unchanged (the backward-stable `lowered` bar for the
ILL_CONDITIONED families).  The families go through the C entry with hand-made lists: a list made by `sense` is one list of discs
for all envs, so per-record geometry cannot be placed through the field without large coordinates."""
import ctypes as C

import numpy as np
import pytest

from tests import obstacle_ref as O
from tests import shield_ref as S
from tests.test_gpu_obstacles import field_of
from tests.test_gpu_shield import check_against_ref, dev, host
from tests.test_gpu_shield_geometry import check, same_bits

pytestmark = pytest.mark.gpu
E = S.E_CASE
EPS32 = S.EPS32


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def fams():
    return S.families()


def entry(torch, recs, c, rate, margin, u_max, dt, orow=None, oid=None, M=0, obstacle_rate=None):
    """One call of the C entry on host records (`dronesim_action_shield` without a list): host (u*, intervened, correction)."""
    from scalable_collision_avoidance_rl_amd import _native
    En, N, k1 = recs["nbr"].shape
    u, z, nbr, radius = dev(torch, recs["u"]), dev(torch, recs["z"]), dev(torch, recs["nbr"]), dev(torch, recs["radius"])
    out = torch.empty_like(u)
    iv = torch.zeros(En, N, dtype=torch.uint8, device="cuda:0")
    corr = torch.zeros(En, N, dtype=torch.float32, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (z.data_ptr(), nbr.data_ptr(), u.data_ptr(), radius.data_ptr(), rate, margin, u_max, dt, En, N, k1, c, out.data_ptr(),
            iv.data_ptr(), corr.data_ptr())
    if oid is None:
        rc = _native.lib().dronesim_action_shield(*head, stream)
    else:
        m = oid.shape[-1]
        d_row, d_id = dev(torch, np.ascontiguousarray(orow, np.float32)), dev(torch, np.ascontiguousarray(oid, np.int32))
        assert tuple(d_row.shape) == (En, N, m, 3) and tuple(d_id.shape) == (En, N, m)
        rc = _native.lib().dronesim_action_shield_obstacles(*head, d_row.data_ptr(), d_id.data_ptr(), m, M, obstacle_rate, stream)
    assert rc == 0
    return host(out), host(iv), host(corr)


def guarantee(what, ustar, orow, oid, z, k1, c, radius, M, obstacle_rate, margin, dt, tol):
    """DESIGN.md's statement on the kernel's own answer: for every live list slot, with g from the float32 row in float64,
    |p - dt u*| - l_i - r_o - margin >= (1 - obstacle_rate) max(g, 0) + min(g, 0) - slack, slack = 2 dt tol + 4 eps32 D (the
    feasibility residual times dt and the rounding of the float32 rows; D the largest finite |p| of the neighbour and list rows)."""
    rows = np.asarray(z, np.float64).reshape(-1, k1, c)[:, 1:, :2]
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.concatenate([np.sqrt((rows ** 2).sum(2)).ravel(), np.sqrt((np.asarray(orow, np.float64)[..., :2] ** 2).sum(-1)).ravel()])
    slack = 2 * dt * tol + 4 * EPS32 * d[np.isfinite(d)].max()
    short, n = O.guarantee_shortfall(ustar, orow, oid, radius, M, obstacle_rate, margin, dt)
    print(f"  {what}: {n} live list slots, largest shortfall of the guarantee {short:.3e} (slack {slack:.3e})")
    assert n > 0 and short <= slack, (what, short, slack)


# ---------------------------------------------------------------------------------------------- every m, rate, parameter set
def through_the_field(torch, case, shape, m, obstacle_rate, pset, offset=0):
    from scalable_collision_avoidance_rl_amd import ActionShield
    N, k, c = shape
    rate, margin, u_max = O.SWEEP_PARAMETERS[pset]
    field = field_of(torch, case, N, k, c, m)
    sh = ActionShield(field.env, rate, margin, None if np.isinf(u_max) else u_max, obstacles=field, obstacle_rate=obstacle_rate)
    out = sh(dev(torch, case["u"]), z=dev(torch, case["z"], offset), nbr=dev(torch, case["nbr"]))
    return (host(out), host(sh.intervened), host(sh.correction)), host(field.orow), host(field.oid), sh


@pytest.mark.parametrize("shape,m,obstacle_rate,pset", O.SHIELD_SWEEP,
                         ids=["N%dk%dc%d-m%d-orate%s-%s" % (s + (m, r, p)) for s, m, r, p in O.SHIELD_SWEEP])
def test_obstacle_shield_at_every_list_width_rate_and_parameter_set(torch, shape, m, obstacle_rate, pset):
    """More discs in range than m in every record (tests/test_obstacles_host.py), so the strides 3 m and m of the list decide
    which rows a record reads."""
    N, k, c = shape
    rate, margin, u_max = O.SWEEP_PARAMETERS[pset]
    case = O.sweep_case(shape, pset)
    (out, iv, corr), orow, oid, sh = through_the_field(torch, case, shape, m, obstacle_rate, pset)
    assert sh.obstacle_rate == (rate if obstacle_rate is None else obstacle_rate) and oid.shape == (E, N, m)
    assert np.array_equal(oid, O.case_list(case, m)[1]) and (oid >= 0).all()       # (the list itself: test_gpu_obstacle_paths.py)
    ref, _, _ = O.sweep_reference(case, shape, m, obstacle_rate, pset, orow, oid)  # the kernel's own rows, as the shield read them
    what = f"obstacle shield {shape} m={m} obstacle_rate={obstacle_rate} {pset}"
    check_against_ref(what, out, iv, corr, case["u"], case["z"], case["nbr"], case["radius"], c, ref=ref)
    guarantee(what, out, orow, oid, case["z"], k + 1, c, case["radius"], case["obstacles"].shape[0], sh.obstacle_rate, margin, S.DT, ref["tol"])


@pytest.mark.parametrize("offset", [4, 8])
def test_obstacle_shield_reads_z_at_a_base_that_breaks_the_alignment(torch, offset):
    """(4, 3, 2): 32-byte records, two 16-byte loads at an aligned base; at +8 the 8-byte loads, at +4 the dword loads, in the
    sense launch and in the shield launch -- the same bits."""
    shape = (4, 3, 2)
    case = O.sweep_case(shape, "standard")
    aligned, orow, oid, _ = through_the_field(torch, case, shape, 3, O.OBSTACLE_RATE, "standard")
    shifted, orow2, oid2, _ = through_the_field(torch, case, shape, 3, O.OBSTACLE_RATE, "standard", offset=offset)
    assert same_bits(aligned, shifted) and same_bits((orow, oid), (orow2, oid2)) and (oid >= 0).any()
    assert aligned[1].any() and not same_bits(aligned[:1], (case["u"],))


# ---------------------------------------------------------------------------------------------- families through the C entry
@pytest.mark.parametrize("name", O.LIST_FAMILY_NAMES)
def test_family_with_lines_in_the_list_is_feasible_and_optimal(torch, fams, name):
    conv, orate = O.list_family(fams, name)
    En, N, k1 = conv["nbr"].shape
    o, iv, corr = entry(torch, conv, conv["c"], conv["rate"], conv["margin"], conv["u_max"], conv["dt"], conv["orow"], conv["oid"],
                        O.LIST_M, orate)
    lowered = name.startswith(S.ILL_CONDITIONED)
    for label, e0, e1 in conv["blocks"]:
        ref = O.list_block_reference(conv, e0, e1, orate)
        what = f"{name} {label}"
        feas_r, opt_r, tol = check(what, (o[e0:e1], iv[e0:e1], corr[e0:e1]), ref, lowered=lowered)
        if name in ("crowd", "crowd permuted"):                                    # 0 is the only feasible action (the family's own radii)
            point = conv["point"][e0 * N:e1 * N]
            worst = np.abs(o[e0:e1].reshape(-1, 2)[point]).max()
            print(f"  {what}: |u*| where the set is {{0}}: {worst:.3e} ({worst / tol:.3f} tol), {point.sum()} records")
            assert point.sum() >= 100 and worst <= tol
        if name.startswith(("crowd", "antipodal")):
            guarantee(what, o[e0:e1], conv["orow"][e0:e1], conv["oid"][e0:e1], conv["z"][e0:e1], k1, 2, conv["radius"], O.LIST_M, orate,
                      conv["margin"], conv["dt"], tol)


# ---------------------------------------------------------------------------------------------- the on rule of a list slot
def test_a_list_of_slots_that_must_be_off_is_the_plain_shield_bit_for_bit(torch):
    """Every slot of every record is one of `obstacle_ref.OFF_SLOTS`: id -1 with a non-zero row, id M, id INT32_MIN, a valid id
    with a zero row, with an inf and with a NaN coordinate.  Output, flags and corrections are the plain entry's bits."""
    N, k, c = 5, 2, 2
    case = O.shield_case(N, k, c)
    M = case["obstacles"].shape[0]
    plain = entry(torch, case, c, S.RATE, S.MARGIN, S.U_MAX, S.DT)
    for m in (4, 2):
        orow, oid = O.off_lists(case, 4, 0)
        got = entry(torch, case, c, S.RATE, S.MARGIN, S.U_MAX, S.DT, orow[:, :, :m], oid[:, :, :m], M, O.OBSTACLE_RATE)
        assert same_bits(plain, got), m
    live = O.case_list(case, 4)
    assert not same_bits(plain, entry(torch, case, c, S.RATE, S.MARGIN, S.U_MAX, S.DT, live[0], live[1], M, O.OBSTACLE_RATE))


def test_one_off_slot_among_three_live_ones_leaves_the_answer_of_the_three(torch):
    N, k, c = 5, 2, 2
    case = O.shield_case(N, k, c)
    M = case["obstacles"].shape[0]
    orow, oid = O.off_lists(case, 4, 3)
    out, iv, corr = entry(torch, case, c, S.RATE, S.MARGIN, S.U_MAX, S.DT, orow, oid, M, O.OBSTACLE_RATE)
    ref = O.shield_reference(case, c, orow, oid)
    assert (ref["on"][:, 4 + k:].sum(1) == 3).all()
    check_against_ref("one off slot among three live", out, iv, corr, case["u"], case["z"], case["nbr"], case["radius"], c, ref=ref)
    guarantee("one off slot among three live", out, orow, oid, case["z"], k + 1, c, case["radius"], M, O.OBSTACLE_RATE, S.MARGIN, S.DT, ref["tol"])
