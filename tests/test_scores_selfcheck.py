"""The tolerance of the per-token log-probability test (tests/_scores_ref.py: tol) cannot hide a defect: on the crafted rows the GPU test also
runs, every way of getting the sum or the pick wrong moves the reference's own logprob by more than 10x that tolerance — dropping any entry
that carries mass, counting one twice, taking the pick one index off — and, where the row lets them apply, changes top2 / margin as well."""
import numpy as np
import pytest

import _scores_ref as R


def _moves(ref, got):
    return abs(got - ref) > 10 * R.tol(ref)


@pytest.mark.parametrize("kind", ["two", "slices", "flat"])
def test_mutations_move_logprob_past_ten_tolerances(kind):
    x, at = R.crafted(kind)
    n = x.shape[0]
    t1, t2 = R.top2_row(x)
    for pick in (t1, at[-1]):
        ref = R.logprob_row(x, pick)
        assert np.isfinite(ref) and abs(ref) < 32
        for i in at:                               # every entry that carries mass: one dropped, one counted twice
            assert _moves(ref, R.logprob_row(x, pick, drop=i)), (kind, pick, i)
            assert _moves(ref, R.logprob_row(x, pick, twice=i)), (kind, pick, i)
        if kind != "flat":                         # (a flat row gives every pick the same logprob: the mutation does not apply)
            for off in (-1, 1):
                if 0 <= pick + off < n:
                    assert _moves(ref, R.logprob_row(x, pick + off)), (kind, pick, off)


@pytest.mark.parametrize("kind", ["two", "slices", "flat"])
def test_mutations_change_top2_and_margin(kind):
    x, at = R.crafted(kind)
    t1, t2 = R.top2_row(x)
    m = R.margin_row(x, t1, t2)
    assert m >= 0
    for skip in (t1, t2):                          # the search loses the largest / the runner-up
        u1, u2 = R.top2_row(x, skip=skip)
        assert (u1, u2) != (t1, t2)
        if kind != "flat":                         # (flat: every margin is 0)
            assert R.margin_row(x, u1, u2) != m


def test_the_mass_sits_where_the_mutations_reach():
    """the entries outside `at` carry no mass the contract's fixed point can see: dropping ALL of them moves the float64 logprob by less than
    a hundredth of the tolerance, so "any one entry" above covers every entry whose loss could matter"""
    for kind in ("two", "slices"):
        x, at = R.crafted(kind)
        ref = R.logprob_row(x, at[0])
        only = np.full_like(x, -np.inf)
        only[at] = x[at]
        assert abs(R.logprob_row(only, at[0]) - ref) < R.tol(ref) / 100
        assert float(np.exp(np.float32(R.LOW))) * 2.0 ** 40 < 1.0
    # the slices row: one entry in every slice of the kernel
    x, at = R.crafted("slices")
    b = R.slice_bounds(x.shape[0])
    assert len(at) == len(b) == 16 and all(lo <= i < hi for i, (lo, hi) in zip(at, b))


def test_reference_ties_and_picks():
    x = np.array([1.0, 3.0, 3.0, -2.0, 3.0], np.float32)
    assert R.top2_row(x) == (1, 2) and R.margin_row(x, 1, 2) == 0
    assert R.top2_row(np.array([2.0, 2.0], np.float32)) == (0, 1)
    assert R.top2_row(np.array([-5.0, -1.0, -3.0], np.float32)) == (1, 2)
    assert np.isnan(R.logprob_row(x, -1)) and np.isnan(R.logprob_row(x, 5))
    lp = [R.logprob_row(x, i) for i in range(5)]
    assert abs(sum(np.exp(lp)) - 1) < 1e-12
