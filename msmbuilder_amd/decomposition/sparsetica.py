"""SparseTICA: tICA with sparse pseudo-eigenvectors (``decomposition/sparsetica.py`` of msmbuilder).

The accumulators, ``fit`` / ``partial_fit`` / ``fit_sharded``, pickling, ``transform`` and the mappings are tICA's; only the
solve differs: each component is a sparse approximate generalized eigenpair of ``(offset_correlation_, covariance_)`` from
the persistent launch of ``csrc/speigh_dev.h``, followed by a Schur complement deflation of the lagged
matrix, which stays on the device between components.  ``covariance_`` is decomposed once per solve.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib
from .._lib import check
from . import _moments
from .speigh import _run, STATUS
from .tica import tICA

__all__ = ['SparseTICA']


class _DeviceDoubles:
    """A block of float64 in HBM for the duration of one solve."""

    def __init__(self, count):
        self.ptr = C.c_void_p(0)
        self.count = int(count)
        check(_lib.lib().msm_malloc(C.byref(self.ptr), self.count * 8))

    def put(self, host):
        host = np.ascontiguousarray(host, dtype=np.float64)
        assert host.size == self.count
        check(_lib.lib().msm_memcpy_h2d(self.ptr, host.ctypes.data, host.nbytes))
        return self

    def get(self, shape):
        out = np.empty(shape)
        assert out.size == self.count
        check(_lib.lib().msm_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            _lib.lib().msm_free(self.ptr)
            self.ptr = C.c_void_p(0)


class SparseTICA(tICA):
    """Sparse time-structure Independent Component Analysis (tICA).

    Finds sparse linear combinations of the input features which decorrelate most slowly; these serve feature
    selection as well as dimensionality reduction.  Unlike dense tICA the solver is not guaranteed to find the global
    solution, and the components are not necessarily found from slowest to fastest: they are sorted by eigenvalue after
    the solve, so a larger ``n_components`` may turn up further slow processes.

    Parameters
    ----------
    n_components : int
        Number of sparse tICs to find.
    lag_time : int
        Delay between the two frames of a correlated pair.
    rho : positive float
        Regularisation strength: larger values give sparser tICs.  ``rho <= 0`` is standard tICA.
    shrinkage : float, default=None
        Covariance shrinkage intensity (0-1); ``None`` estimates it (Rao-Blackwellized Ledoit-Wolf).
    kinetic_mapping, commute_mapping : bool
        As for ``tICA``.
    epsilon : positive float, default=1e-6
        Sharpness of the approximation to the L0 penalty.
    tolerance : positive float
        Convergence criterion of the sparse eigensolver.
    maxiter : int
        Iteration limit of the sparse eigensolver (outer steps, and ADMM iterations per step).
    verbose : bool, default=False
        Print the counters of every component's solve.

    Attributes
    ----------
    As ``tICA``; ``eigenvalues_`` are pseudo-eigenvalues in decreasing order, ``eigenvectors_`` the sparse
    pseudo-eigenvectors.  ``solve_info_`` lists, per component in the order found, the counters of its solve.
    """

    def __init__(self, n_components=None, lag_time=1, rho=0.01,
                 kinetic_mapping=False, commute_mapping=False, epsilon=1e-6, shrinkage=None,
                 tolerance=1e-6, maxiter=10000, verbose=False):
        super(SparseTICA, self).__init__(n_components, lag_time=lag_time,
                                         kinetic_mapping=kinetic_mapping, commute_mapping=commute_mapping)
        self.rho = rho
        self.epsilon = epsilon
        self.shrinkage = shrinkage
        self.tolerance = tolerance
        self.maxiter = maxiter
        self.verbose = verbose
        self.solve_info_ = None

    def _solve(self):
        if not self._is_dirty:
            if self._eigenvalues_ is not None and len(self._eigenvalues_) >= self.n_components:
                return

        if self.rho <= 0:
            # if no sparse regularization, it's just regular tICA
            return super(SparseTICA, self)._solve()

        if not self.n_observations_:
            raise RuntimeError('The model must be fit() before use.')

        A = self.offset_correlation_
        B = self.covariance_
        if not _moments.is_symmetric(A):
            raise RuntimeError('offset correlation matrix is not symmetric')
        if not _moments.is_symmetric(B):
            raise RuntimeError('correlation matrix is not symmetric')
        F, k = int(self.n_features), int(self.n_components)
        if not (self.epsilon > 0 and self.tolerance > 0 and int(self.maxiter) >= 1):
            raise ValueError('SparseTICA needs epsilon > 0, tolerance > 0 and maxiter >= 1')

        L = _lib.lib()
        vals = np.zeros(k)
        vecs = np.zeros((F, k))
        infos = []
        bufs = []
        try:
            dA = _DeviceDoubles(F * F).put(A)
            bufs.append(dA)
            dB = _DeviceDoubles(F * F).put(B)
            bufs.append(dB)
            d_ev, d_E, d_v = _DeviceDoubles(F), _DeviceDoubles(F * F), _DeviceDoubles(F)
            bufs += [d_ev, d_E, d_v]
            # B never changes between components: one decomposition per solve
            _run(L.msm_syev_top(dB.ptr, F, F, d_ev.ptr, d_E.ptr, 1))
            u = C.c_double(0.0)
            info = np.zeros(8)
            for i in range(k):
                _run(L.msm_speigh(dA.ptr, dB.ptr, F, float(self.rho), float(self.epsilon), float(self.tolerance), int(self.maxiter),
                                  None, d_ev.ptr, d_E.ptr, C.byref(u), d_v.ptr, None, info.ctypes.data_as(C.POINTER(C.c_double)), 1))
                vals[i] = u.value
                vecs[:, i] = d_v.get((F,))
                infos.append({'outer': int(info[0]), 'admm': int(info[1]), 'launches': int(info[2]), 'objective': float(info[3]),
                              'nnz': int(info[4]), 'status': STATUS[int(info[5])], 'workgroups': int(info[6])})
                if self.verbose:
                    print("SparseTICA component %d: %s" % (i, infos[-1]))
                if i + 1 < k:
                    check(L.msm_scdeflate(dA.ptr, d_v.ptr, F, dA.ptr, 1))
        finally:
            for b in bufs:
                b.free()

        # sort in order of decreasing value
        ind = np.argsort(vals)[::-1]
        self._eigenvalues_ = vals[ind]
        self._eigenvectors_ = vecs[:, ind]
        self.solve_info_ = infos
        self._is_dirty = False

    def summarize(self):
        """Some summary information."""
        nonzeros = np.sum(np.abs(self.eigenvectors_) > 0, axis=0)
        active = '[%s]' % ', '.join(['%d/%d' % (n, self.n_features) for n in nonzeros[:5]])

        return """Sparse time-structure based Independent Components Analysis (tICA)
------------------------------------------------------------------
n_components        : {n_components}
shrinkage           : {shrinkage}
lag_time            : {lag_time}
kinetic_mapping     : {kinetic_mapping}
commute_mapping     : {commute_mapping}
rho                 : {rho}
n_features          : {n_features}

Top 5 timescales :
{timescales}

Top 5 eigenvalues :
{eigenvalues}

Number of active degrees of freedom:
{active}
""".format(n_components=self.n_components, lag_time=self.lag_time,
           rho=self.rho, shrinkage=self.shrinkage_,
           kinetic_mapping=self.kinetic_mapping,
           commute_mapping=self.commute_mapping,
           timescales=self.timescales_[:5], eigenvalues=self.eigenvalues_[:5],
           n_features=self.n_features, active=active)
