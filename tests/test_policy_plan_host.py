"""The policy kernels' launch plan (csrc/policy_common.hpp: plan_policy_launch -- the refusals, the variant, grid, LDS, opt-in, stream
length and division magic of every family) against the plan the library made while every entry point added its own LDS sizes up and
chose its own variant (no GPU needed: the plan makes no HIP call).

tests/golden/policy_plan.npz was recorded from the parent commit of that change: a scratch copy of it with the same hook,
`dronesim_debug_policy_plan`, calling the real entry points with launch_policy recording what it was handed instead of launching,
built with csrc/Makefile's flags, and

    python tests/test_policy_plan_host.py --record <that build's libdronesim.so>

run from the repository root.  `plan` holds the ten values of PLAN per row of sweep() (one row of the array per value: it packs
smaller), `rows_sha` the sweep's digest."""
import ctypes as C
import hashlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from scalable_collision_avoidance_rl_amd import _native

GOLDEN = os.path.join(ROOT, "tests", "golden", "policy_plan.npz")
PLAN = ("rc", "family", "variant", "grid", "threads", "lds", "opt_in", "stream", "rb_magic", "why")
ROW = ("config", "N", "d_in", "h1", "h2", "nout", "layout", "reserved_off", "arrays", "misaligned", "E")
# tests/helpers.py: POLICY_CONFIGS -> (entry point of the hook, DroneMlp.w2_layout); "f32" is the row-tile stream (the host class
# falls back to the fragments for d_in > 14, where the library refuses w2_layout = 2)
CONFIGS = ("f32", "f32-fragments", "f32-w2-unpacked", "bf16x3", "f16x2", "f16x2-split", "bf16")
ENTRY = {"f32": (0, 2), "f32-fragments": (0, 1), "f32-w2-unpacked": (0, 0), "bf16x3": (2, 0), "f16x2": (1, 0), "f16x2-split": (3, 0), "bf16": (4, 0)}
RT, RT16, STAGED, SPLIT, BF16 = range(5)                          # enum PolicyFamily
VARIANTS = {RT: 2, RT16: 2, STAGED: 5, SPLIT: 2, BF16: 16}
ROWS_PER_BLOCK = {RT: 128, RT16: 128, STAGED: 32, SPLIT: 64, BF16: 64}
OPT_IN_ABOVE = {RT: 0, RT16: 0, STAGED: 0, SPLIT: 48 * 1024, BF16: 48 * 1024}
# substrings of dronesim_last_error() of every refusal an entry point makes between its NULL m / x check and the launch
# (`why` = index; the hook passes out_kind = sample_kind = 0, so check_mlp's two texts about them are out of its reach)
REFUSALS = ("need d_in<=64", "E < 0", "NULL weight array", "w2_layout = 2 needs d_in <= 14", "(w2_layout = 2) must be 16-byte aligned",
            "w2_layout must be 0, 1 or 2", "(w2_layout = 1) must be 16-byte aligned", "f16x2_rt: d_in <= 16", "rt16_blocks",
            "the stream must be 16-byte aligned", "bf16x3 path: d_in <= 16", "f16x2 path: d_in <= 16", "bf16 path: d_in <= 16",
            "bf16x3_stages", "hidden layer too wide for the LDS tile")
D_IN = (1, 6, 14, 15, 16, 17, 64, 65)
HIDDEN = (1, 31, 32, 33, 224, 225, 256, 257, 352, 353, 512, 513)
NOUT = (1, 4, 5, 16, 17, 32, 33)
ES = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4096, 6_000_000, -1)     # one row block +- 1 of every family; 6e6: div_magic gives 0
STREAM = 0x7F0000001000


def sweep():
    rows = []
    for c in range(len(CONFIGS)):
        layout = ENTRY[CONFIGS[c]][1]
        for d_in, h1, h2, nout in itertools.product(D_IN, HIDDEN, HIDDEN, NOUT):
            rows.append((c, 3, d_in, h1, h2, nout, layout, 0, 1, 0, 4096))
        for h1 in range(32, 513, 32):                             # every chunk count of h1: mlp3_bf16_kernel<NC1>
            rows.append((c, 3, 6, h1, 64, 4, layout, 0, 1, 0, 4096))
        for d_in, h1, h2, nout in itertools.product((6, 16), (31, 256, 352), (31, 256, 352), (4, 16)):
            for N, E in itertools.product((1, 3, 64), ES):
                rows.append((c, N, d_in, h1, h2, nout, layout, 0, 1, 0, E))
            for E in (0, 4096):                                   # (E = 0 comes ahead of some refusals and behind others)
                rows.append((c, 3, d_in, h1, h2, nout, layout, 4, 1, 0, E))       # a wrong DroneMlpBf16.reserved
                rows.append((c, 3, d_in, h1, h2, nout, layout, 0, 1, 1, E))       # a misaligned stream
                rows.append((c, 3, d_in, h1, h2, nout, layout, 0, 0, 0, E))       # NULL arrays
                rows.append((c, 3, 17, h1, h2, nout, layout, 0, 0, 1, E))         # ... with d_in over the cap: which refusal comes first
                if ENTRY[CONFIGS[c]][0] == 0:
                    rows.append((c, 3, d_in, h1, h2, nout, 3, 0, 1, 0, E))        # no such w2_layout
    return np.array(rows, dtype=np.int32)


def digest(rows):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(rows).tobytes()).digest(), dtype=np.uint8)


def recorded():
    gold = np.load(GOLDEN)
    return gold["plan"].astype(np.int64).T, gold["rows_sha"]


def plans(lib, rows):
    fn = lib.dronesim_debug_policy_plan
    fn.argtypes = [C.c_int] * 9 + [C.c_uint64, C.c_int, C.POINTER(C.c_int64)]
    fn.restype = None
    err = lib.dronesim_last_error
    err.restype = C.c_char_p
    for name in ("dronesim_mlp_rt16_blocks", "dronesim_mlp_bf16x3_stages"):
        getattr(lib, name).restype = C.c_int
    out = np.zeros((len(rows), len(PLAN)), dtype=np.int64)
    buf = (C.c_int64 * 9)()
    for i, (c, N, d_in, h1, h2, nout, layout, reserved_off, arrays, misaligned, E) in enumerate(rows.tolist()):
        entry = ENTRY[CONFIGS[c]][0]
        reserved = (lib.dronesim_mlp_rt16_blocks(h1, h2, nout) if entry == 1 else lib.dronesim_mlp_bf16x3_stages(h1, h2) if entry in (2, 3) else 0)
        fn(entry, N, d_in, h1, h2, nout, layout, reserved + reserved_off, arrays, STREAM + 8 * misaligned, E, buf)
        out[i, :9] = buf[:]
        why = [j for j, text in enumerate(REFUSALS) if text.encode() in err()] if buf[0] else [-1]
        assert len(why) == 1, (rows[i].tolist(), err())
        out[i, 9] = why[0]
    return out


def test_plan_equals_the_recorded_plan_of_every_swept_launch():
    want, sha = recorded()
    rows = sweep()
    assert np.array_equal(digest(rows), sha), "the sweep is not the recorded one"
    got = plans(_native.lib(), rows)
    bad = np.nonzero((want != got).any(axis=1))[0]
    msg = "\n".join(f"{dict(zip(ROW, rows[i].tolist()))}\n  recorded {dict(zip(PLAN, want[i].tolist()))}\n  now      {dict(zip(PLAN, got[i].tolist()))}"
                    for i in bad[:10])
    assert bad.size == 0, f"{bad.size} of {len(rows)} plans differ:\n{msg}"


def test_sweep_covers_every_variant_and_refusal_and_lds_stays_in_the_tile():
    plan, rows = recorded()[0], sweep()
    col, inp = {n: plan[:, i] for i, n in enumerate(PLAN)}, {n: rows[:, i] for i, n in enumerate(ROW)}
    ok = (col["rc"] == _native.OK) & (inp["E"] != 0)
    assert (plan[~ok, 1:9] == 0).all()                                           # a refused launch and E = 0 report the code only
    for c, name in enumerate(CONFIGS):                                           # every configuration launches, every family is reached
        assert (ok & (inp["config"] == c)).any(), name
    for family, n in VARIANTS.items():
        assert set(col["variant"][ok & (col["family"] == family)].tolist()) == set(range(n)), family
    assert set(col["rc"].tolist()) == {_native.OK, _native.EINVAL, _native.EUNSUPPORTED}
    # every refusal but one is reached.  "hidden layer too wide for the LDS tile" (the LDS-staged f32 kernel and bf16) is reached by no
    # swept shape, and by none that check_mlp lets through: at its caps (d_in = 64, h1 = 512) the staged kernel's tile is 92800 bytes,
    # bf16's (h1 = h2 = 512) 73856
    assert set(col["why"][col["rc"] != 0].tolist()) == set(range(len(REFUSALS))) - {REFUSALS.index("hidden layer too wide for the LDS tile")}
    assert col["lds"][ok & (col["family"] == STAGED)].max() == 92800 and col["lds"][ok & (col["family"] == BF16)].max() == 73856
    assert col["lds"][ok].max() <= 160 * 1024 and col["lds"][ok].min() > 0 and (col["lds"][ok] % 16 == 0).all()
    for family, above in OPT_IN_ABOVE.items():
        f = ok & (col["family"] == family)
        assert np.array_equal(col["opt_in"][f] == 1, col["lds"][f] > above), family
        assert np.array_equal(col["grid"][f], (inp["E"][f] + ROWS_PER_BLOCK[family] - 1) // ROWS_PER_BLOCK[family] * inp["N"][f]), family
    assert (ok & (col["opt_in"] == 0)).any() and (col["rb_magic"][ok & (inp["E"] == 6_000_000) & (inp["N"] > 1)] == 0).all()
    assert (col["rb_magic"][ok & np.isin(col["family"], (RT, RT16, STAGED)) & (inp["E"] == 4096)] != 0).all()


# Which kernel serves which shape -- the table at the top of csrc/policy_common.hpp and in DESIGN.md section 4, restated:
# (configuration, d_in range, nout range) -> (family, variant; None: mlp3_bf16_kernel<NC1>, variant = ceil(h1 / 32) - 1).
# BatchedMLP's "f32" takes the f32-fragments rows when d_in > 14.
TABLE = (("f32", (1, 14), (1, 4), RT, 1), ("f32", (1, 14), (5, 32), RT, 0),
         ("f32-fragments", (1, 6), (1, 16), STAGED, 4), ("f32-fragments", (7, 64), (1, 16), STAGED, 3), ("f32-fragments", (1, 64), (17, 32), STAGED, 2),
         ("f32-w2-unpacked", (1, 64), (1, 16), STAGED, 1), ("f32-w2-unpacked", (1, 64), (17, 32), STAGED, 0),
         ("f16x2", (1, 16), (1, 4), RT16, 1), ("f16x2", (1, 16), (5, 32), RT16, 0),
         ("f16x2-split", (1, 16), (1, 32), SPLIT, 1), ("bf16x3", (1, 16), (1, 32), SPLIT, 0), ("bf16", (1, 16), (1, 32), BF16, None))


def test_the_table_of_kernels_per_shape_is_the_plans():
    plan, rows = recorded()[0], sweep()
    plain = (rows[:, 7] == 0) & (rows[:, 8] == 1) & (rows[:, 9] == 0) & (rows[:, 10] > 0) & (rows[:, 6] != 3)     # a well-formed call
    hidden_ok = (rows[:, 3] <= 512) & (rows[:, 4] <= 512)
    served = np.zeros(len(rows), bool)
    for config, (d_lo, d_hi), (o_lo, o_hi), family, variant in TABLE:
        f = plain & hidden_ok & (rows[:, 0] == CONFIGS.index(config)) & (rows[:, 2] >= d_lo) & (rows[:, 2] <= d_hi) & (rows[:, 5] >= o_lo) & (rows[:, 5] <= o_hi)
        assert f.any() and not (f & served).any(), config
        want = (rows[f, 3] + 31) // 32 - 1 if variant is None else variant
        assert (plan[f, 0] == _native.OK).all() and (plan[f, 1] == family).all() and (plan[f, 2] == want).all(), (config, d_lo, o_lo)
        served |= f
    assert (plan[plain & ~served, 0] != _native.OK).all()                        # ... and nothing else is served


def extreme_shapes():
    """Per configuration, the accepted swept shapes (d_in, h1, h2, nout) with the largest and the smallest LDS of the recorded plan
    (the first of equals in sweep order): tests/test_gpu_policy_extremes.py runs them."""
    plan, rows = recorded()[0], sweep()
    out = {}
    for c, name in enumerate(CONFIGS):
        f = np.nonzero((plan[:, 0] == 0) & (rows[:, 0] == c) & (rows[:, 10] == 4096))[0]
        lds = plan[f, 5]
        out[name] = [tuple(rows[f[j], 2:6].tolist()) for j in (int(np.argmax(lds)), int(np.argmin(lds)))]
    return out


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    import torch  # noqa: F401  (the library binds to the HIP runtime torch ships, as in _native.lib())
    rows = sweep()
    plan = plans(C.CDLL(os.path.abspath(sys.argv[2])), rows)
    np.savez_compressed(GOLDEN, rows_sha=digest(rows), plan=np.ascontiguousarray(plan.T))
    print(f"{GOLDEN}: {len(rows)} plans, {os.path.getsize(GOLDEN)} bytes")
