"""The tie fixtures of tests/ties_ref.py on the CPU: the oracle's neighbour lists and collision counts are the stable-argsort
restatement's on every configuration tests/test_gpu_ties.py launches (heterogeneous radii included, for which no golden
exists), the margin mask leaves enough of every pattern to compare, and every kept tie env really is degenerate.

Semantics guarded: the reference's drone_env.py:309-346 with SURVEY's rule for its argsort (stable: the lowest index first)."""
import numpy as np
import pytest

from tests import ties_ref as R


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_oracle_lists_are_the_stable_argsort_restatement(name):
    fx = R.fixture(name)
    nbr, n_coll = R.lists(fx.pos64, fx.l, fx.d_hat, fx.k, fx.orc.delta)
    assert fx.kept.any()
    np.testing.assert_array_equal(fx.ref["nbr_idx"][fx.kept], nbr[fx.kept])
    np.testing.assert_array_equal(fx.ref["n_coll"][fx.kept], n_coll[fx.kept])


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_margin_mask_keeps_at_least_half_of_every_pattern(name):
    fx = R.fixture(name)
    assert set(fx.pat) == set("abcdef" if fx.hetero else "abcf")
    for letter in sorted(set(fx.pat)):
        of, kept = fx.pat == letter, fx.kept[fx.pat == letter]
        print(name, letter, f"keeps {int(kept.sum())} of {int(of.sum())}, margins {np.sort(fx.margin[of])[:3]}")
        assert kept.sum() >= 1 and 2 * kept.sum() >= of.sum(), (name, letter, int(kept.sum()), int(of.sum()))


@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_kept_tie_envs_are_degenerate(name):
    """In every kept tie env some agent's restated row has a partner ahead of or tied with the self entry -- and the list shows
    it: some agent is listed a second time among its own neighbours.  With uniform radii the control envs have none (with
    heterogeneous radii a random draw can nest a small agent in a large one)."""
    fx = R.fixture(name)
    deg = R.preceded(fx.pos64, fx.l, fx.d_hat)
    tie = fx.pat != "f"
    nbr, _ = R.lists(fx.pos64, fx.l, fx.d_hat, fx.k, fx.orc.delta)
    own = np.arange(fx.N)[None, :, None]
    listed_twice = (nbr[:, :, 1:] == own).any((1, 2))
    assert (tie & fx.kept).any() and deg[tie & fx.kept].all() and listed_twice[tie & fx.kept].all()
    if not fx.hetero:
        assert not deg[~tie].any() and not listed_twice[~tie].any()
    # pattern (e): the larger agent has the higher index and still precedes the smaller one (strictly ahead, not by index)
    if fx.hetero:
        for e in np.flatnonzero((fx.pat == "e") & fx.kept):
            small, large = fx.groups[e][0]
            assert small < large and nbr[e, small, 1] == small and nbr[e, large, 1] == small
