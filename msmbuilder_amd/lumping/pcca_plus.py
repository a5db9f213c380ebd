"""Robust Perron cluster analysis on MI355X: drop-in for ``msmbuilder.lumping.PCCAPlus`` (reference:
msmbuilder/lumping/pcca_plus.py; Deuflhard and Weber, Linear Algebra Appl. 398, 161 (2005); Kube and Weber, J. Chem. Phys.
126, 024103 (2007)).

PCCA+ looks for the m x m transformation A of the first m right eigenvectors V whose memberships ``chi = V A`` give the
best lumping under one of three objectives.  scipy's ``basinhopping`` and ``fmin`` evaluate that objective 10^3 to 10^5
times, and in the reference every evaluation multiplies the dense n x n transition matrix with chi.  Here T, pi and V are
uploaded once into a handle (csrc/pcca.hip) and every evaluation is one queued call:

* ``metastability`` needs T once, not once per evaluation: ``chi_i^T diag(pi) T chi_i = (A^T G A)_ii`` with the m x m
  ``G = V^T diag(pi) T V`` computed at set-up;
* ``crisp_metastability`` (the default) depends on the argmax mapping only: a new mapping costs one read of T with a label
  predicate, and a mapping equal to the previous evaluation's costs none;
* ``crispness`` never needed T.

The search itself (``basinhopping``, ``fmin``) runs on the host as in the reference, with the same calls.

Differences to the reference, both deliberate:

* ``random_state`` (default ``None``) is handed to ``basinhopping`` as its ``rng``; the reference leaves the search unseeded.
* what ``PCCA`` lists: ``from_msm`` keeps the device eigensystem and takes constructor keywords, too few eigenvectors raise
  ``ValueError``.

The module functions have the reference's names and signatures and run in numpy on the host.
"""
import ctypes as C

import numpy as np
import scipy.optimize

from .. import _lib
from .._lib import check
from .pcca import PCCA

__all__ = ['PCCAPlus', 'PccaHandle', 'pcca_plan', 'metastability', 'crisp_metastability', 'crispness', 'get_maps', 'to_flat',
           'to_square', 'has_constraint_violation', 'index_search', 'fill_A', 'calculate_fuzzy_chi']

KINDS = {'crispness': 0, 'metastability': 1, 'crisp_metastability': 2}


# ---- the reference's module functions, numpy on the host -------------------------------------------------------------------
def get_maps(A):
    """(flat_map [(N-1)^2, 2], square_map [N, N]): flat index k <-> the entry (i, j) of ``A[1:, 1:]``, row-major."""
    N = A.shape[0]
    i, j = np.divmod(np.arange((N - 1) ** 2), N - 1) if N > 1 else (np.zeros(0, int), np.zeros(0, int))
    flat_map = np.stack([i + 1, j + 1], axis=1).astype(int).reshape(-1, 2)
    square_map = np.zeros(A.shape, 'int')
    square_map[flat_map[:, 0], flat_map[:, 1]] = np.arange(len(flat_map))
    return flat_map, square_map


def to_flat(A, flat_map):
    return A[flat_map[:, 0], flat_map[:, 1]]


def to_square(alpha, square_map):
    return alpha[square_map]


def has_constraint_violation(A, right_eigenvectors, epsilon=1E-8):
    lhs = 1 - A[0, 1:].sum()
    rhs = -1 * np.dot(right_eigenvectors[:, 1:], A[1:, 0]).min()
    return bool(abs(lhs - rhs) > epsilon)


def index_search(right_eigenvectors):
    """The rows of the eigenvectors that span the simplex, found by Gram-Schmidt; vectorised over the rows."""
    V = np.asarray(right_eigenvectors)
    num_eigen = V.shape[1]
    index = np.zeros(num_eigen, 'int')
    index[0] = np.argmax(np.sqrt((V * V).sum(axis=1)))
    ortho = V - V[index[0]]
    for j in range(1, num_eigen):
        temp = ortho[index[j - 1]].copy()
        ortho = ortho - np.outer(ortho.dot(temp), temp)
        dist = np.sqrt((ortho * ortho).sum(axis=1))
        index[j] = np.argmax(dist)
        ortho = ortho / dist.max()
    return index


def fill_A(A, right_eigenvectors):
    """A made feasible: the first column by the row-sum condition, the first row by the maximum condition, then scaled."""
    A = np.array(A, dtype=float)
    with np.errstate(all='ignore'):   # (an all-zero alpha fills to NaN, which the objectives answer with -inf)
        A[1:, 0] = -1 * A[1:, 1:].sum(1)
        A[0] = -1 * np.dot(np.real(right_eigenvectors[:, 1:]), A[1:]).min(0)
        A /= A[0].sum()
    return A


def calculate_fuzzy_chi(alpha, square_map, right_eigenvectors):
    A = fill_A(to_square(alpha, square_map), right_eigenvectors)
    chi_fuzzy = np.dot(right_eigenvectors, A)
    return A, chi_fuzzy, np.argmax(chi_fuzzy, 1)


def _infeasible(A, mapping, right_eigenvectors):
    return len(np.unique(mapping)) != right_eigenvectors.shape[1] or has_constraint_violation(A, right_eigenvectors)


def _lumped_trace(T, chi, pi):
    moved = np.asarray(T.dot(chi))
    return float(np.sum(np.einsum('ai,ai->i', moved, pi[:, None] * chi) / chi.T.dot(pi)))


def metastability(alpha, T, right_eigenvectors, square_map, pi):
    with np.errstate(all='ignore'):
        A, chi, mapping = calculate_fuzzy_chi(alpha, square_map, right_eigenvectors)
        if _infeasible(A, mapping, right_eigenvectors):
            return -1.0 * np.inf
        return _lumped_trace(T, chi, np.asarray(pi))


def crisp_metastability(alpha, T, right_eigenvectors, square_map, pi):
    with np.errstate(all='ignore'):
        A, chi_fuzzy, mapping = calculate_fuzzy_chi(alpha, square_map, right_eigenvectors)
        if _infeasible(A, mapping, right_eigenvectors):
            return -1.0 * np.inf
        chi = np.zeros_like(chi_fuzzy)
        chi[np.arange(len(mapping)), mapping] = 1.
        return _lumped_trace(T, chi, np.asarray(pi))


def crispness(alpha, T, right_eigenvectors, square_map, pi):
    with np.errstate(all='ignore'):
        A, chi, mapping = calculate_fuzzy_chi(alpha, square_map, right_eigenvectors)
        if _infeasible(A, mapping, right_eigenvectors):
            return -1.0 * np.inf
        return float(np.trace(np.dot(np.diag(1. / A[0]), np.dot(A.transpose(), A))))


# ---- the device handle -----------------------------------------------------------------------------------------------------
def pcca_plan():
    """``msm_pcca_plan`` as a dict: rows of T per workgroup, columns per pass, threads per workgroup, largest n and m."""
    out = (C.c_int64 * 5)()
    check(_lib.lib().msm_pcca_plan(out))
    return dict(zip(('rows', 'cols', 'threads', 'max_n', 'max_m'), (int(v) for v in out)))


class PccaHandle(object):
    """T (n x n), pi (n) and the first m right eigenvectors V (n x m) on the device (``msm_pcca_create``).  The three arrays
    are numpy arrays or all torch CUDA tensors.  Use as a context manager, or ``close()`` it."""

    def __init__(self, T, pi, V):
        arrs = [_lib.Arr(x, np.float64) for x in (T, pi, V)]
        if len(set(a.on_device for a in arrs)) != 1:
            raise ValueError('T, pi and V must all be host arrays or all device tensors')
        aT, api, aV = arrs
        if len(aV.shape) != 2 or aT.shape != (aV.shape[0], aV.shape[0]) or api.shape != (aV.shape[0],):
            raise ValueError('T must be n x n, pi n and V n x m')
        self.n, self.m = int(aV.shape[0]), int(aV.shape[1])
        self._h = C.c_void_p(None)
        _lib.ensure_device()
        check(_lib.lib().msm_pcca_create(aT.vp, api.vp, aV.vp, self.n, self.m, aT.on_device, C.byref(self._h)))
        self._value = C.c_double(0.0)
        self._info = np.zeros(4, dtype=np.int32)
        self.evaluations = self.passes = self.reused = 0

    def close(self):
        if self._h:
            check(_lib.lib().msm_pcca_destroy(self._h))
            self._h = C.c_void_p(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def moments(self):
        """(G [m, m], w [m]) of the set-up."""
        G, w = np.empty((self.m, self.m)), np.empty(self.m)
        check(_lib.lib().msm_pcca_moments(self._h, G.ctypes.data, w.ctypes.data))
        return G, w

    def chi(self, A, want_chi=True):
        """(fill_A(A), chi = V fill_A(A) or None, the argmax mapping [int32])."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        if A.shape != (self.m, self.m):
            raise ValueError('A must be %d x %d' % (self.m, self.m))
        out, mapping = np.empty((self.m, self.m)), np.empty(self.n, dtype=np.int32)
        chi = np.empty((self.n, self.m)) if want_chi else None
        check(_lib.lib().msm_pcca_chi(self._h, A.ctypes.data, out.ctypes.data, chi.ctypes.data if want_chi else None,
                                      mapping.ctypes.data))
        return out, chi, mapping

    def objective(self, kind, alpha):
        """(value, info) of ``msm_pcca_objective``; ``kind`` is a name or 0, 1, 2."""
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        if alpha.size != (self.m - 1) ** 2:
            raise ValueError('alpha must have %d entries' % (self.m - 1) ** 2)
        check(_lib.lib().msm_pcca_objective(self._h, KINDS.get(kind, kind), alpha.ctypes.data, C.byref(self._value),
                                            self._info.ctypes.data))
        self.evaluations += 1
        self.passes += int(self._info[3])
        self.reused += int(self._info[2])
        return self._value.value, self._info.copy()

    def crisp(self, mapping):
        """(num [m], den [m]): the block sums of any mapping."""
        mapping = np.ascontiguousarray(mapping, dtype=np.int32)
        if mapping.shape != (self.n,):
            raise ValueError('the mapping must have one entry per state')
        num, den = np.empty(self.m), np.empty(self.m)
        check(_lib.lib().msm_pcca_crisp(self._h, mapping.ctypes.data, num.ctypes.data, den.ctypes.data))
        return num, den


class PCCAPlus(PCCA):
    """Perron cluster cluster analysis plus (PCCA+) for coarse-graining (lumping) microstates into macrostates.

    Parameters
    ----------
    n_macrostates : int
        The number of macrostates in the lumped model, 2 to 64.
    do_minimization : bool, default=True
        False: keep the initial transformation found by ``index_search``.
    objective_function : {'crisp_metastability', 'metastability', 'crispness'}
        What the search maximises; ``None`` is the default.  Anything else raises ``AttributeError``.
    random_state : None, int or numpy Generator / RandomState
        The ``rng`` of ``basinhopping``.
    **kwargs
        ``pcca_tolerance`` (unused by PCCA+, kept) and the keywords of :class:`MarkovStateModel`.

    Attributes
    ----------
    A_ : [m, m] the transformation;  chi_ : [n_states_, m] the memberships;  microstate_mapping_ : int array, [n_states_]
    optimize_info_ : dict with the search's ``evaluations``, ``passes`` over T and evaluations that ``reused`` the mapping.
    """

    def __init__(self, n_macrostates, do_minimization=True, objective_function='crisp_metastability', **kwargs):
        self.random_state = kwargs.pop('random_state', None)
        super(PCCAPlus, self).__init__(n_macrostates, **kwargs)
        if objective_function is None:
            objective_function = 'crisp_metastability'
        if objective_function not in KINDS:
            raise AttributeError("Objective function must be one of %s" % sorted(KINDS))
        self.objective_function = objective_function
        self.do_minimization = do_minimization

    @classmethod
    def _get_param_names(cls):
        return sorted(['do_minimization', 'random_state'] + PCCA._get_param_names())

    def _do_lumping(self):
        vectors = self._lumping_eigenvectors()
        m = vectors.shape[1]
        if m < 2:
            raise ValueError('PCCAPlus needs at least 2 macrostates, got %d' % m)
        A = fill_A(np.linalg.inv(vectors[index_search(vectors), :]), vectors)
        T = self.transmat_ if _lib.is_device_array(self.transmat_) else np.asarray(self.transmat_, dtype=np.float64)
        if _lib.is_device_array(T):
            import torch
            pi, V = torch.as_tensor(np.asarray(self.populations_, dtype=np.float64), device=T.device), torch.as_tensor(vectors, device=T.device)
        else:
            pi, V = np.asarray(self.populations_, dtype=np.float64), vectors
        with PccaHandle(T, pi, V) as handle:
            if self.do_minimization:
                A = self._optimize_A(A, handle)
            self.optimize_info_ = {'evaluations': handle.evaluations, 'passes': handle.passes, 'reused': handle.reused}
            self.A_, self.chi_, mapping = handle.chi(A)
        self.microstate_mapping_ = mapping.astype(int)

    def _optimize_A(self, A, handle):
        flat_map, square_map = get_maps(A)
        alpha = to_flat(1.0 * A, flat_map)
        kind = KINDS[self.objective_function]

        def obj(x):
            return -1 * handle.objective(kind, x)[0]

        alpha = scipy.optimize.basinhopping(obj, alpha, niter_success=1000, rng=self.random_state)['x']
        alpha = scipy.optimize.fmin(obj, alpha, full_output=True, xtol=1E-4, ftol=1E-4, maxfun=5000, maxiter=100000, disp=False)[0]
        if np.isneginf(handle.objective(kind, alpha)[0]):
            raise ValueError("Error: minimization has not located a feasible point.")
        return to_square(alpha, square_map)
