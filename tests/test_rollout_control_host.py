"""Closed-loop controller rollouts (`dronesim_rollout_control`), the part that needs no GPU: the kRolloutCtrl instances of
the BUILT library, and the oracle-side conditions tests/test_gpu_rollout_control.py relies on for the start states it commits."""
import os
import shutil

import numpy as np
import pytest

import scalable_collision_avoidance_rl_amd as pkg
from tests import helpers as H
from tests import test_gpu_rollout_control as R
from tests import test_gpu_rollout_control_fuzz as F

LIB = os.path.join(os.path.dirname(os.path.abspath(pkg.__file__)), "libdronesim.so")
MODE_CTRL = 5


def _need_readelf():
    from tools import kernel_resources as KR
    if not os.path.exists(KR.READELF) and not shutil.which(KR.READELF):
        pytest.skip("llvm-readelf not available")
    return KR


def test_every_geometry_has_its_controller_instances():
    """One kRolloutCtrl kernel per k x geometry x FAR x episode layer (kBlockU256 has no FAR form): 8 x (4 x 2 + 1) x 2."""
    KR = _need_readelf()
    rows = [r[1] for r in KR.resources(LIB) if r[1] is not None and r[1]["mode"] == MODE_CTRL]
    have = {(r["k"], r["far"], r["geo"], r["epi"]) for r in rows}
    want = {(k, far, geo, epi) for k in range(1, 9) for geo in range(5) for far in (0, 1) for epi in (0, 1) if not (geo == 4 and far)}
    assert have == want and len(rows) == 144


def test_controller_rollouts_do_not_spill_on_their_hot_path():
    """What tests/test_host_logic.py::test_no_rollout_kernel_spills_on_its_hot_path asks of the pool / in-kernel action
    sources, of the controller source: k = 2 without far agents at every BASELINE geometry -- kPacked, kSym64, kBlockU256 with
    and without the episode layer, kBlock256 plain -- has NO scratch instruction inside the per-step loop."""
    KR = _need_readelf()
    from tools import spill_sites as SS
    for geo in (0, 1, 2, 4):
        for epi in ((0,) if geo == 2 else (0, 1)):
            r = SS.hot_loop_scratch(LIB, 2, 0, MODE_CTRL, geo, epi)
            assert r is not None, (geo, epi)
            n_ins, loop, hot, total = r
            assert loop is not None and loop[1] - loop[0] > 500, (geo, epi, loop)
            assert hot == 0, f"GEO={geo} EPI={epi}: {hot} scratch instructions inside the per-step loop {loop}"
            if geo == 1:
                assert total == 0, (geo, epi, total)


@pytest.mark.parametrize("name", list(R.SHAPES))
def test_gradient_start_states_exercise_the_repulsion_sum(name):
    """The box start of the teacher-forced test, driven by the ORACLE's gradient controller for its 24 steps (unclipped and
    clipped at 0.7), and the lattice states an in-kernel reset draws: the compared share stays above 0.3 and at least 5 %
    of the compared agents have a non-empty repulsion sum."""
    N, E = R.SHAPES[name][:2]
    orc = R.make_oracle(name)
    for u in (1e4, 0.7):
        pos = R.box_start(name, 100 + N).astype(np.float64); vel = np.zeros_like(pos); t = np.zeros(E, np.int32)
        for s in range(24):
            safe, near = R.gradient_masks(orc, pos)
            assert safe.mean() > 0.3 and (near[safe] > 0).mean() >= 0.05, (name, u, s)
            orc.step(pos, vel, t, orc.gradient_control(pos, u))
    lattice = orc.reset(E, 11)[0]
    safe, near = R.gradient_masks(orc, lattice)
    assert safe.mean() > 0.3 and (near[safe] > 0).mean() >= 0.05


@pytest.mark.parametrize("seed,iters", F.CHAIN_SEEDS)
def test_chain_draws_stay_inside_the_compared_share(seed, iters):
    """The seeded draws of tests/test_gpu_rollout_control_fuzz.py::test_closed_loop_fuzz_action_against_the_oracle, driven by the
    ORACLE's own closed loop in float64: at every step of every gradient iteration the GPU test will compare, the safe share stays
    above 0.3 and at least 5 % of the compared agents have a non-empty repulsion sum -- the start boxes (F.CHAIN_BOX) and clips
    (F.CHAIN_U) of that test are the range at which this holds."""
    from oracle.oracle import Oracle
    rng = np.random.default_rng(seed)
    kinds, worst = set(), (1.0, 1.0)
    for it in range(iters):
        d = F.draw(rng, False, chain=True)
        if d is None:
            continue
        kinds.add(d["ctrl"])
        if d["ctrl"] != "gradient":
            continue
        orc = Oracle(d["N"], [d["G"], d["G"]], d["k"], d["deltas"], d["c"] == 2)
        pos = d["pos0"].astype(np.float64); vel = np.zeros_like(pos); t = np.zeros(d["E"], np.int32)
        for s in range(d["T"]):
            safe, near = R.gradient_masks(orc, pos)
            share, busy = safe.mean(), (near[safe] > 0).mean()
            worst = (min(worst[0], share), min(worst[1], busy))
            assert share > 0.3 and busy >= 0.05, (seed, it, d["N"], d["G"], d["u_max"], d["box"], s, share, busy)
            orc.step(pos, vel, t, orc.gradient_control(pos, d["u_max"]))
    print("chain draws, seed", seed, "smallest safe share %.3f, smallest share with a repulsion sum %.3f" % worst)
    assert kinds == {"gradient", "proportional"}


@pytest.mark.parametrize("name", ["packed5", "sym64", "block70", "block256"])
def test_arrival_start_states_are_clear_of_the_threshold(name):
    """Float64 closed loop from the arrival test's start states: every env arrives at some s < 40, and at most 10 % of the
    envs (about 2 % expected: the error moves 0.01 per step near 0.2, the band is 2 x H.MARGIN wide) have their largest
    agent error within H.MARGIN of 0.2 at that step or the one before."""
    N = R.SHAPES[name][0]
    first, clear = R.oracle_arrival(name, R.arrival_start(name, 300 + N), 60)
    assert (first >= 0).all() and first.max() < 40 and (~clear).mean() <= 0.10
