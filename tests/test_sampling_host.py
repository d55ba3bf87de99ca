"""CPU tests of tests/sampling_ref.py, the host restatement tests/test_gpu_sampling.py holds every policy kernel family to."""
import numpy as np

from tests import sampling_ref as R


def test_numpy_philox_equals_the_oracles():
    """The second Philox4x32-10 against the oracle's (C, pinned on the Random123 known answers by tests/test_host_logic.py): the three
    known-answer vectors and 1000 random counters and keys."""
    from oracle import oracle as O
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for c, k, want in kat:
        assert O.philox(c, k) == want
        assert [int(w) for w in R.philox4x32_10(*c, *k)] == want
    rng = np.random.default_rng(1)
    ck = rng.integers(0, 2 ** 32, (1000, 6), dtype=np.uint64).astype(np.uint32)
    got = np.stack(R.philox4x32_10(*[ck[:, i] for i in range(6)]), axis=-1)
    assert got.dtype == np.uint32 and got.shape == (1000, 4)
    want = np.array([O.philox(row[:4], row[4:]) for row in ck], dtype=np.uint32)
    assert np.array_equal(got, want)


def test_draw_words_counter_layout_and_wrap_rules():
    """ctr = (agent, env_base + e, counter.lo + t[e], counter.hi + episode[e]), key = (seed.lo, seed.hi); every word wraps on its own."""
    from oracle import oracle as O
    seed = (0x1234 << 32) | 0xABCD0001
    w = R.draw_words(seed, (7 << 32) | 9, 100, 3, 2, t=[0, 5, 199], episode=[0, 2, 3])
    assert w.shape == (3, 2, 4) and w.dtype == np.uint32
    for e, (t, ep) in enumerate([(0, 0), (5, 2), (199, 3)]):
        for a in range(2):
            assert list(w[e, a]) == O.philox([a, 100 + e, 9 + t, 7 + ep], [0xABCD0001, 0x1234])
    # counter = 2^32 - 1 with t = 3: the low word wraps to 2 and nothing is carried into the high word
    w = R.draw_words(5, 2 ** 32 - 1, 0, 2, 1, t=[3, 3])
    assert list(w[1, 0]) == O.philox([0, 1, 2, 0], [5, 0])
    # counter = 2^32 + 5: low word 5, high word 1 (plus the episode)
    w = R.draw_words(5, 2 ** 32 + 5, 0, 1, 1, episode=[4])
    assert list(w[0, 0]) == O.philox([0, 0, 5, 5], [5, 0])
    # env_base + e and counter.hi + episode wrap modulo 2^32 too
    w = R.draw_words(5, (2 ** 32 - 1) << 32, 2 ** 32 - 1, 2, 1, episode=[0, 2])
    assert list(w[1, 0]) == O.philox([0, 0, 0, 1], [5, 0])


def test_categorical_pick_states_the_rule():
    p = np.array([[0.25, 0.0, 0.5, 0.25]], np.float32)
    word = lambda u: np.array([[int(u * 2 ** 24) << 8, 0, 0, 0]], np.uint32)
    for u, want in [(0.0, 0), (0.2, 0), (0.25, 2), (0.3, 2), (0.74, 2), (0.75, 3), (0.999, 3)]:   # first j with u < cdf_j: never the p = 0 output
        pick, amb, uu = R.categorical_pick(p, word(u))
        assert int(pick[0]) == want and uu[0] == int(u * 2 ** 24) / 2 ** 24
        assert bool(amb[0]) == (u in (0.25, 0.75))
    pick, amb, _ = R.categorical_pick(np.array([[0.5, 0.25]], np.float32), word(0.9))              # beyond the total: clamped
    assert int(pick[0]) == 1 and not amb[0]
    assert np.allclose(R.unit_action([0, 1, 2], 4), [[1, 0], [0, 1], [-1, 0]], atol=1e-15)


def test_band_stays_under_the_cap_on_the_gpu_tests_own_cases():
    """For every (weight class, nout) of the GPU file, on its own networks, inputs and E x N: the share of draws within delta of a cdf value
    (float64 softmax rounded to float32) stays at or below 1e-3 per case -- expected 2 delta (nout - 1) or less, 2.4e-4 at nout = 32.
    Also: the peaked class does reach probabilities that are exactly 0 in float32, the ordinary class does not."""
    shares = {}
    for (d, h2) in ((6, 65), (15, 65), (6, 129)):
        for cls in R.CLASSES:
            for (nout, N, E) in R.grid_cases():
                c = R.softmax_case(cls, nout, N, E, d=d, h2=h2)
                p64 = R.host_softmax(c["w"], c["x"])
                words = R.draw_words(c["seed"], c["counter"], c["env_base"], E, N)
                pick, amb, u = R.categorical_pick(p64.astype(np.float32), words)
                assert amb.mean() <= R.CAP, (c["tag"], int(amb.sum()), amb.size)
                assert np.all(np.take_along_axis(p64, pick[..., None], -1)[~amb] > 0), c["tag"]
                s = shares.setdefault((cls, nout), [0, 0, 0.0, 1.0])
                s[0] += int(amb.sum()); s[1] += amb.size
                s[2] = max(s[2], float((p64 < 2.0 ** -150).mean())); s[3] = min(s[3], float(p64.min()))
    for (cls, nout), (a, n, zeros, pmin) in sorted(shares.items()):
        print(f"band share {cls:9s} nout={nout:2d}: {a} / {n} = {a / n:.2e}   (bound {2 * nout * 2.0 ** -23 * nout:.2e}; "
              f"largest share of p < 2^-150: {zeros:.2f}, smallest p {pmin:.1e})")
        assert a / n <= R.CAP
        if cls == "peaked" and nout >= 2:
            assert zeros > 0.0, (cls, nout, zeros)
        if cls == "ordinary":
            assert pmin > 1e-30, (cls, nout, pmin)
        if cls == "uniform":
            assert zeros == 0.0 and pmin == 1.0 / nout


def test_gaussian_restatement_has_normal_moments():
    """mu = 0, var = 1 over 1e6 draws of the stream (both components): mean 0, variance 1, fourth moment 3 within three standard errors
    (sigma of the sample mean 1 / sqrt n, of the variance sqrt(2 / n), of the fourth moment sqrt(96 / n))."""
    E, N = 1000, 500
    words = R.draw_words(11, 3, 0, E, N)
    act, r = R.gaussian_action(np.zeros((E, N, 2)), np.ones((E, N, 2)), words)
    assert np.all(r >= 0) and r.max() <= np.sqrt(2 * 24 * np.log(2.0)) + 1e-12
    z = act.ravel()
    n = z.size
    assert n == 10 ** 6
    assert abs(z.mean()) <= 3 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 3 * np.sqrt(2.0 / n)
    assert abs((z ** 4).mean() - 3.0) <= 3 * np.sqrt(96.0 / n)
    # the two components use disjoint word pairs: uncorrelated
    assert abs(np.mean(act[..., 0] * act[..., 1])) <= 3 / np.sqrt(E * N)
    # mu and sqrt(var) enter linearly
    act2, _ = R.gaussian_action(np.full((E, N, 2), 0.5), np.full((E, N, 2), 0.25), words)
    assert np.allclose(act2, 0.5 + 0.5 * act, atol=1e-14)
