"""oracle/mle_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Two independent checkers of the reversible maximum-likelihood transition matrix (msm_transmat_mle):

* ``ref_mle``         -> oracle/_ref/libref_mle.so, the reference's own solver (msm/src/transmat_mle_prinz.c:
                         Prinz's element-wise quadratic updates, stopped on the log-likelihood) compiled by
                         oracle/Makefile from where it lies.  A different algorithm from the device's fixed point.
* ``mle_longdouble``  -> the fixed point x = g(x) on the simplex in numpy.longdouble (80-bit on x86-64, eps 1.08e-19),
                         Anderson-mixed, stopped at max|g - x| / max g < 1e-18: the converged estimate to well beyond
                         float64, against which a float64 solver's distance is a measurement and not a comment.

``kkt_longdouble`` is the stationarity residual and ``t_from_pi`` the closed form T_ij = Cs_ij / (c_i + c_j pi_i / pi_j)
of the estimator in its populations; both work in the precision of the ``pi`` they are given.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_MLE_SO = os.path.join(_HERE, "_ref", "libref_mle.so")
LD = np.longdouble
_f64p = ctypes.POINTER(ctypes.c_double)
_ref = None


def have_extended_precision():
    return bool(np.finfo(LD).eps < 1e-18)


def _ref_lib():
    global _ref
    if _ref is None and os.path.exists(REF_MLE_SO):
        lib = ctypes.CDLL(REF_MLE_SO)
        lib.transmat_mle_prinz.restype = ctypes.c_int
        lib.transmat_mle_prinz.argtypes = [_f64p, ctypes.c_int, ctypes.c_double, _f64p, _f64p]
        _ref = lib
    return _ref


def ref_mle(C, tol=1e-10):
    """The reference's solver on the counts C: (n_iter, T, pi), or None when the library has not been built.
    n_iter < 0 is the reference's error code (-1 row sums, -2 domain, -3 not converged after its 10,000 sweeps)
    and is returned, not raised."""
    lib = _ref_lib()
    if lib is None:
        return None
    C = np.ascontiguousarray(C, dtype=np.float64)
    n = C.shape[0]
    assert C.shape == (n, n)
    T = np.zeros((n, n))
    pi = np.zeros(n)
    n_iter = lib.transmat_mle_prinz(C.ctypes.data_as(_f64p), n, float(tol), T.ctypes.data_as(_f64p),
                                    pi.ctypes.data_as(_f64p))
    return int(n_iter), T, pi


class _Pattern:
    """Cs = C + C^T on its nonzero pattern, row-sorted, so g costs O(nnz) and not O(K^2)."""

    def __init__(self, C, dtype):
        C = np.asarray(C, dtype=np.float64)
        Cs = C + C.T
        self.rows, self.cols = np.nonzero(Cs)
        # in long double Cs and c are exact sums of the float64 counts: a Cs rounded in float64 beside an exact c leaves
        # g(x) = lambda x with lambda - 1 ~ 1e-17, a floor the residual then cannot pass
        self.vals = C[self.rows, self.cols].astype(dtype) + C[self.cols, self.rows].astype(dtype)
        self.c = C.astype(dtype).sum(1) if dtype is LD else C.sum(1)
        self.K = C.shape[0]
        self.start = np.searchsorted(self.rows, np.arange(self.K))
        if len(np.unique(self.rows)) != self.K or np.any(self.c <= 0):
            raise ValueError("every row of C and of C + C^T needs a positive sum")

    def g(self, x):
        d = self.c / x
        return np.add.reduceat(self.vals / (d[self.rows] + d[self.cols]), self.start)


def _solve_small(M, r):
    """Gaussian elimination with partial pivoting in the dtype of M; None if singular or non-finite."""
    n = len(r)
    a = np.concatenate([M, r[:, None]], axis=1)
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if not np.abs(a[p, k]) > 0:
            return None
        if p != k:
            a[[k, p]] = a[[p, k]]
        a[k + 1:] -= (a[k + 1:, k] / a[k, k])[:, None] * a[k]
    gam = np.zeros(n, dtype=M.dtype)
    for i in range(n - 1, -1, -1):
        gam[i] = (a[i, n] - a[i, i + 1:n] @ gam[i + 1:]) / a[i, i]
    return gam if np.all(np.isfinite(gam)) else None


def mle_longdouble(C, tol=1e-18, m=6, max_iter=200000):
    """(T, pi, iterations) of the reversible MLE of C in numpy.longdouble: x = g(x) on the simplex, Anderson mixing over
    m iterates, plain step whenever the mixed one is not positive; stops at max|g(x) - x| / max g(x) < tol.  T is the
    closed form in the converged populations.  Raises if it does not converge."""
    return mle_fixed_point(C, LD, tol, m, max_iter)


def mle_fixed_point(C, dtype=np.float64, tol=1e-14, m=6, max_iter=200000):
    """The same solve in `dtype` over the pattern only (O(nnz) per iteration): with float64 and 1e-14 it is the float64
    yardstick at sizes where the dense mle_numpy of the golden script is too slow."""
    P = _Pattern(C, dtype)
    x = np.add.reduceat(P.vals, P.start)
    x = x / x.sum()
    dF, dG, Fp, Gp = [], [], None, None
    for it in range(max_iter + 1):
        g = P.g(x)
        res = np.abs(g - x).max() / g.max()
        if res < tol:
            break
        if it == max_iter:
            raise ValueError("mle_fixed_point: not converged after %d iterations" % max_iter)
        G = g / g.sum()
        F = G - x
        if Fp is not None:
            dF.append(F - Fp)
            dG.append(G - Gp)
            if len(dF) > m:
                dF.pop(0)
                dG.pop(0)
        Fp, Gp = F, G
        x = G
        if dF:
            A = np.array(dF)
            gam = _solve_small(A @ A.T, A @ F)
            if gam is not None:
                xn = G - gam @ np.array(dG)
                if np.all(xn > 0) and np.all(np.isfinite(xn)):
                    x = xn / xn.sum()
    pi = g / g.sum()
    return t_from_pi(C, pi), pi, it


def kkt_longdouble(C, pi, dtype=LD):
    """max|g(pi) - pi| / max pi evaluated in numpy.longdouble (or `dtype`), over the pattern only."""
    P = _Pattern(C, dtype)
    pi = np.asarray(pi, dtype=dtype)
    return float(np.abs(P.g(pi) - pi).max() / pi.max())


def t_from_pi(C, pi):
    """The estimator's transition matrix as a function of its populations, T_ij = Cs_ij / (c_i + c_j pi_i / pi_j), in the
    dtype of pi (dense K x K; zero off the pattern of C + C^T)."""
    pi = np.asarray(pi)
    P = _Pattern(C, LD if pi.dtype == LD else np.float64)
    T = np.zeros((P.K, P.K), dtype=pi.dtype)
    T[P.rows, P.cols] = P.vals / (P.c[P.rows] + P.c[P.cols] * (pi[P.rows] / pi[P.cols]))
    return T
