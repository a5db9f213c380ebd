"""Inputs and reference sums shared by tests/test_oracle.py (CPU) and tests/test_gpu_libdistance_device.py (GPU).
TEST INFRASTRUCTURE, not product code.

``special_rows`` is the zero-laden / non-finite recipe: where randn data never goes.  Values come from
{0, 0, 0, 1, 2, -0.0}, so most feature pairs are 0 against 0 (canberra's `sdenom > 0` guard, hamming on -0.0 == 0.0) and
many rows tie; two rows are all zero (braycurtis and jaccard give 0/0 = NaN between them); one row holds a NaN, one +inf,
one -inf (every comparison of assign's strict `<` against DBL_MAX sees NaN and inf).  ``special_centres`` takes the
centres from those five rows first and duplicates one centre.
"""
import math

import numpy as np

VALUES = np.array([0.0, 0.0, 0.0, 1.0, 2.0, -0.0])


def special_rows(n, m, dtype, seed=0):
    """[n, m] rows of the recipe and the indices (zero, zero, NaN, +inf, -inf) of the five special rows; n >= 5."""
    rs = np.random.RandomState(seed)
    X = VALUES[rs.randint(0, len(VALUES), size=(n, m))].astype(dtype)
    rows = rs.choice(n, 5, replace=False)
    X[rows[0]] = 0.0
    X[rows[1]] = 0.0
    X[rows[2], rs.randint(m)] = np.nan
    X[rows[3], rs.randint(m)] = np.inf
    X[rows[4], rs.randint(m)] = -np.inf
    return X, rows


def special_centres(X, rows, k, seed=0):
    """k >= 7 centres: the five special rows, ordinary rows, and the last one a copy of the first ordinary one."""
    assert k >= 7
    rs = np.random.RandomState(seed + 1)
    Y = np.concatenate([X[rows], X[rs.randint(0, X.shape[0], size=k - 5)]])
    Y[k - 1] = Y[5]
    return np.ascontiguousarray(Y)


def ref_sum(terms):
    """The correctly rounded sum of non-negative float64 terms (math.fsum), NaN if one of them is NaN, inf if one is
    inf or the exact sum is beyond the float64 range."""
    t = np.asarray(terms, dtype=np.float64)
    if np.isnan(t).any():
        return float("nan")
    if np.isinf(t).any():
        return float("inf")
    try:
        return math.fsum(t)
    except OverflowError:
        return float("inf")


def sum_matches(got, terms, depth):
    """`got` is a float64 sum, in whatever order, of the non-negative `terms`, none of which passed through more than
    `depth` additions.  Each addition of non-negative numbers multiplies what it carries by (1 + e), |e| <= 2^-53, so
    the result lies within depth * 2^-53 of the exact sum, relatively.  `depth` counts a thread's first addition, which
    is onto a zero accumulator and exact: that spare unit covers the rounding of math.fsum itself and the second-order
    terms of (1 + 2^-53)^depth.  Non-finite sums must agree in kind."""
    ref = ref_sum(terms)
    if math.isnan(ref):
        return math.isnan(got)
    if math.isinf(ref):
        return got == ref
    return abs(got - ref) <= depth * 2.0 ** -53 * ref
