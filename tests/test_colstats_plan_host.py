"""The column-statistics plan (csrc/colstats_common.hpp: col_plan) as the C ABI shows it -- the slab count S, through the two
workspace queries: `dronesim_standardize_workspace` returns 16 S N bytes, `dronesim_obsnorm_workspace` 24 S C -- against the
sizes the library returned when `standardize.hip` and `obsnorm.hip` each carried a copy of the plan (no GPU needed: the queries
make no HIP call).  tests/golden/colstats_plan.npz was recorded from the parent commit of that change with
tests/golden/gen_colstats_plan.py."""
import ctypes as C
import os

import numpy as np

from scalable_collision_avoidance_rl_amd import _native

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "colstats_plan.npz")
# rows: around every q = 1024 / tw of the columns below, the learner's windows, and the largest int
ROWS = (1, 2, 3, 4, 63, 64, 65, 203, 204, 205, 255, 256, 257, 1023, 1024, 1025, 4096, 4099, 16383, 16384, 16385, 102400, 819200,
        2 ** 31 - 1)
# columns: one per thread and lane groups of four, whole-row tiles and tiles of 64, the tile cap at 1024 columns and past it
COLS = (1, 2, 3, 4, 5, 8, 30, 36, 60, 64, 68, 70, 128, 252, 256, 260, 384, 1020, 1024, 1028, 1050, 1536, 4096, 4100)


def workspaces(lib):
    """``[2, len(ROWS), len(COLS)]`` int64: the standardize and the obsnorm workspace bytes over the grid."""
    out = np.zeros((2, len(ROWS), len(COLS)), dtype=np.int64)
    n = C.c_size_t(0)
    for k, fn in enumerate((lib.dronesim_standardize_workspace, lib.dronesim_obsnorm_workspace)):
        fn.argtypes, fn.restype = [C.c_int, C.c_int, C.POINTER(C.c_size_t)], C.c_int
        for i, r in enumerate(ROWS):
            for j, c in enumerate(COLS):
                assert fn(r, c, C.byref(n)) == 0, (fn.__name__, r, c)
                out[k, i, j] = n.value
    return out


def test_workspace_sizes_equal_the_recorded_ones():
    gold = np.load(GOLDEN)
    assert tuple(gold["rows"].tolist()) == ROWS and tuple(gold["cols"].tolist()) == COLS, "the grid is not the recorded one"
    got = workspaces(_native.lib())
    bad = np.argwhere(got != gold["bytes"])
    msg = "\n".join(f"{('standardize', 'obsnorm')[k]} R = {ROWS[i]} C = {COLS[j]}: recorded {gold['bytes'][k, i, j]}, now {got[k, i, j]}"
                    for k, i, j in bad[:10])
    assert len(bad) == 0, f"{len(bad)} of {got.size} workspace sizes differ:\n{msg}"


def test_both_features_size_their_workspace_from_one_plan():
    """16 S N against 24 S C at the same (R, C): 3 x the one is 2 x the other exactly when both count the same slabs."""
    std, obs = workspaces(_native.lib())
    assert np.array_equal(3 * std, 2 * obs)
    slabs = std // (16 * np.array(COLS, dtype=np.int64)[None, :])
    assert np.array_equal(slabs * 16 * np.array(COLS, dtype=np.int64)[None, :], std)
    assert slabs.min() == 1 and (slabs <= np.array(ROWS, dtype=np.int64)[:, None]).all()
    assert slabs.max() <= 256                                                # the plan aims at 256 workgroups, tiles included
