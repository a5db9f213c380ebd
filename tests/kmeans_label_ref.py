"""Exact reference and acceptance rule for k-means labelling (plain numpy, float64; shares nothing with the kernels).

The label kernels minimise the GEMM form ``s_j = fl(cn_j - 2 fl(x.c_j))`` (``cn_j``: the float64 sum of squares rounded once
to the rows' type) instead of the squared distance itself, so on a near-tie they may pick another centre than an exact
argmin.  How near is "near" is derived, not tuned:

    d[i, j]     = sum_f (x_if - c_jf)^2                    float64, by direct difference (never the GEMM form)
    ref[i]      = the lowest index among the exact minima of d[i, :]
    bound_i(j)  = 1.01 u ( ||c_j||^2 + | ||c_j||^2 - 2 x.c_j | + 2 m sum_f |x_if c_jf| )

``bound_i(j)`` is the forward error of ``s_j``: one rounding of ``cn_j`` (``u ||c_j||^2``), one of the final subtraction
(``u |s_j|``) and ``m`` roundings inside the dot product, doubled (``2 m u sum |x c|``).  ``u`` is one ulp, 2^-23 for
float32 rows and 2^-52 for float64 rows -- not half an ulp, so it holds whatever rounding the matrix pipe uses inside an
accumulation and for any summation order; 1.01 covers the second-order terms.  A kernel label ``l != ref[i]`` is accepted
only if

    d[i, l] - d[i, ref[i]] <= bound_i(l) + bound_i(ref[i])

and never when centre ``l`` is a bit-for-bit copy of centre ``ref[i]``: the two scores are then bit-identical and the
lowest index must win.  Every row is checked; no number of rows may be wrong.

The inertia is ``sum_i d[i, label_i]`` of the kernel's own labels.  The float32 kernels take the difference in float32
(relative error 2^-24), square it and add in float64: ``INERTIA_RTOL_F32 = 3 * 2^-24`` (twice 2^-24 for the square, the
rest for the float64 sum of positive terms).  Float64 rows: 1e-12.
"""
import numpy as np

U_F32 = 2.0 ** -23
U_F64 = 2.0 ** -52
INERTIA_RTOL_F32 = 3 * 2.0 ** -24
INERTIA_RTOL_F64 = 1e-12

_DIRECT_ELEMS = 1 << 22     # rows x centres x features of one direct-difference block
_GEMM_ELEMS = 1 << 23       # rows x centres of one GEMM block
_SHORTLIST = 4


def unit_roundoff(dtype):
    return U_F64 if np.dtype(dtype) == np.float64 else U_F32


def inertia_rtol(dtype):
    return INERTIA_RTOL_F64 if np.dtype(dtype) == np.float64 else INERTIA_RTOL_F32


def pair_sqdist(X, C, rows, cols):
    """d[rows[k], cols[k]] in float64 by direct difference."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    out = np.empty(len(rows))
    step = max(1, _DIRECT_ELEMS // max(1, X.shape[1]))
    for a in range(0, len(rows), step):
        r, c = rows[a:a + step], cols[a:a + step]
        diff = X[r].astype(np.float64) - C[c].astype(np.float64)
        out[a:a + step] = (diff * diff).sum(axis=1)
    return out


def pair_bound(X, C, rows, cols, u):
    """bound_i(j) for the pairs (rows[k], cols[k])."""
    rows = np.asarray(rows, dtype=np.int64)
    cols = np.asarray(cols, dtype=np.int64)
    m = X.shape[1]
    out = np.empty(len(rows))
    step = max(1, _DIRECT_ELEMS // max(1, m))
    for a in range(0, len(rows), step):
        x = X[rows[a:a + step]].astype(np.float64)
        c = C[cols[a:a + step]].astype(np.float64)
        cn = (c * c).sum(axis=1)
        prod = x * c
        out[a:a + step] = 1.01 * u * (cn + np.abs(cn - 2.0 * prod.sum(axis=1)) + 2.0 * m * np.abs(prod).sum(axis=1))
    return out


def _direct_block(Xb, C64):
    d = np.empty((Xb.shape[0], C64.shape[0]))
    step = max(1, _DIRECT_ELEMS // max(1, Xb.shape[0] * Xb.shape[1]))
    for a in range(0, C64.shape[0], step):
        diff = Xb[:, None, :] - C64[None, a:a + step, :]
        d[:, a:a + step] = (diff * diff).sum(axis=2)
    return d


def _two_lowest(d):
    """(index, value) of the lowest entry of each row of d (lowest index among equals) and of the lowest of the rest."""
    r = np.arange(d.shape[0])
    j1 = d.argmin(axis=1)
    d1 = d[r, j1]
    if d.shape[1] == 1:
        return j1, d1, np.full(len(r), -1), np.full(len(r), np.inf)
    e = d.copy()
    e[r, j1] = np.inf
    j2 = e.argmin(axis=1)
    return j1, d1, j2, e[r, j2]


def exact_argmin(X, C):
    """ref, d_ref, second, d_second: the exact nearest centre of every row (lowest index among exact minima), the
    nearest of the remaining centres, and both squared distances (float64, direct difference).  Rows must be finite.
    Small blocks are computed by difference outright; large ones shortlist the best few centres per row with a
    float64 GEMM and recompute only those by difference (a row whose shortlist is not clearly separated from the
    rest -- many-fold ties -- is computed against every centre)."""
    n, m = X.shape
    K = C.shape[0]
    C64 = C.astype(np.float64)
    ref = np.empty(n, dtype=np.int64)
    sec = np.empty(n, dtype=np.int64)
    dref = np.empty(n)
    dsec = np.empty(n)
    t = _SHORTLIST
    if K <= 2 * t or K * m <= 4096:
        step = max(1, _DIRECT_ELEMS // (K * m))
        for a in range(0, n, step):
            ref[a:a + step], dref[a:a + step], sec[a:a + step], dsec[a:a + step] = \
                _two_lowest(_direct_block(X[a:a + step].astype(np.float64), C64))
        return ref, dref, sec, dsec
    cn = (C64 * C64).sum(axis=1)
    step = max(1, _GEMM_ELEMS // K)
    for a in range(0, n, step):
        Xb = X[a:a + step].astype(np.float64)
        nb = Xb.shape[0]
        g = Xb @ C64.T
        g *= -2.0
        g += cn[None, :]
        part = np.argpartition(g, t, axis=1)[:, :t + 1]            # the t lowest and the lowest of the rest
        r = np.arange(nb)
        gp = g[r[:, None], part]
        order = np.argsort(gp, axis=1)
        gp = np.take_along_axis(gp, order, axis=1)
        cand = np.take_along_axis(part, order, axis=1)[:, :t]
        xn = (Xb * Xb).sum(axis=1)
        # the GEMM form is good to ~m 2^-52 (||x||^2 + ||c||^2): a shortlist whose runner-up lies 1e-9 of that above
        # the best certainly holds the exact best two
        clear = gp[:, t] - gp[:, 0] > 1e-9 * (xn + cn.max())
        diff = Xb[:, None, :] - C64[cand]
        d = (diff * diff).sum(axis=2)
        # equal distances: the lowest INDEX wins, so order the shortlist by index before the argmin
        o2 = np.argsort(cand, axis=1)
        cand = np.take_along_axis(cand, o2, axis=1)
        d = np.take_along_axis(d, o2, axis=1)
        k1, d1, k2, d2 = _two_lowest(d)
        ref[a:a + nb], dref[a:a + nb], sec[a:a + nb], dsec[a:a + nb] = cand[r, k1], d1, cand[r, k2], d2
        for i in np.nonzero(~clear)[0]:
            j1, d1, j2, d2 = _two_lowest(_direct_block(Xb[i:i + 1], C64))
            ref[a + i], dref[a + i], sec[a + i], dsec[a + i] = j1[0], d1[0], j2[0], d2[0]
    return ref, dref, sec, dsec


def near_tie_share(X, C, u=None):
    """Share of rows that the rule cannot decide: exact best and second best no further apart than their two bounds."""
    u = unit_roundoff(X.dtype) if u is None else u
    if C.shape[0] < 2:
        return 0.0
    ref, dref, sec, dsec = exact_argmin(X, C)
    rows = np.arange(X.shape[0])
    return float(np.mean(dsec - dref <= pair_bound(X, C, rows, ref, u) + pair_bound(X, C, rows, sec, u)))


def check_labels(labels, X, C, ref, dref, u=None, skip=None):
    """Hold kernel labels to the rule of the module docstring against (ref, dref) = exact_argmin(X, C)[:2].  Rows listed
    in ``skip`` (rows with a NaN: no distance to compare) are left out.  Returns the number of accepted near-ties."""
    u = unit_roundoff(X.dtype) if u is None else u
    labels = np.asarray(labels)
    assert labels.shape == ref.shape
    differ = labels != ref
    if skip is not None:
        differ[np.asarray(skip, dtype=np.int64)] = False
    bad = np.nonzero(differ)[0]
    if len(bad) == 0:
        return 0
    lab = labels[bad].astype(np.int64)
    assert lab.min() >= 0 and lab.max() < C.shape[0], ("label out of range", bad[:5], lab[:5])
    gap = pair_sqdist(X, C, bad, lab) - dref[bad]
    tol = pair_bound(X, C, bad, lab, u) + pair_bound(X, C, bad, ref[bad], u)
    copies = (C[lab] == C[ref[bad]]).all(axis=1)      # bit-identical scores: the lowest index must have won
    wrong = (gap > tol) | copies
    if wrong.any():
        k = np.nonzero(wrong)[0][:5]
        raise AssertionError("%d of %d rows mislabelled; first (row, label, exact, gap, allowed, copy-of-exact): %s" % (
            int(wrong.sum()), len(labels),
            [(int(bad[q]), int(lab[q]), int(ref[bad[q]]), float(gap[q]), float(tol[q]), bool(copies[q])) for q in k]))
    return len(bad)


def exact_inertia(X, C, labels):
    """sum_i d[i, labels[i]] in float64 by direct difference."""
    return float(pair_sqdist(X, C, np.arange(X.shape[0]), labels).sum())


# ---------------------------------------------------------------------------------------------------------------------
# input generators (seeded; shared by the GPU tests and the host test of the rule's decidability)
# ---------------------------------------------------------------------------------------------------------------------
OFFSET_SHIFT = 3.0    # see tests/test_kmeans_label_rule.py::test_offset_shift_is_the_largest_that_stays_decidable


def gen_unstructured(n, m, K, dtype=np.float32, seed=0):
    """X = randn(n, m), C = randn(K, m): no cluster structure, so near-ties are ordinary."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, m).astype(dtype)
    C = rs.randn(K, m).astype(dtype)
    return X, C


def gen_offset(n, m, K, dtype=np.float32, seed=0, shift=OFFSET_SHIFT):
    """The unstructured data moved away from the origin, where ||c||^2 - 2 x.c cancels."""
    X, C = gen_unstructured(n, m, K, dtype, seed)
    s = np.asarray(shift, dtype=dtype)
    return (X + s).astype(dtype), (C + s).astype(dtype)


def gen_lattice(n, m, K, dtype=np.float32, seed=0):
    """Small integers: every product and sum of the GEMM form is exact in float32 in any order (|x.c| <= 9 m < 2^24), so
    the kernel's scores ARE the distances (minus ||x||^2) and its label must equal the exact one on every row -- and with
    seven values per coordinate exact ties between different centres are common."""
    rs = np.random.RandomState(seed)
    X = rs.randint(-3, 4, (n, m)).astype(dtype)
    C = rs.randint(-3, 4, (K, m)).astype(dtype)
    return X, C


GENERATORS = {"unstructured": gen_unstructured, "offset": gen_offset, "lattice": gen_lattice}
