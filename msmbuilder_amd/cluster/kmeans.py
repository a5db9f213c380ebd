"""Full-batch k-means (Lloyd) on MI355X: drop-in for ``msmbuilder.cluster.KMeans``.

In the reference this class is scikit-learn's ``KMeans`` behind ``MultiSequenceClusterMixin``
(msmbuilder/cluster/__init__.py:63).  This module restates scikit-learn 1.7's ``KMeans.fit`` /
``_kmeans_single_lloyd`` (sklearn/cluster/_kmeans.py) with the same constructor arguments and the
same host-side ``RandomState`` call sequence for the seeding; every pass over the rows runs on the
GPU (msmbuilder_amd/csrc/kmeans.hip, ``msm_lloyd_run``): the column statistics behind ``tol``, the
mean centring, k-means++, and the iterations themselves -- label on the matrix pipes, then a centre
update that sorts the row numbers by label and sums every cluster's rows in float64 in a fixed
order, then the stop rules, with nothing returning to the host between iterations.

What differs from scikit-learn, on purpose: the centre update sums in float64 whatever the rows'
type and rounds once (scikit-learn accumulates float32 rows in float32), and its order is fixed, so
two fits of the same input give bit-identical centres.  ``algorithm='elkan'`` is accepted and runs
Lloyd: the triangle-inequality bookkeeping saves distance evaluations a GPU does not miss, and the
fixed point is the same.  ``sample_weight``, sparse input and multi-GPU fits are not supported.
"""
import ctypes as C

import numpy as np
from sklearn.base import ClusterMixin, TransformerMixin
from sklearn.utils import check_random_state

from .. import _lib
from .._lib import Arr, check, is_device_array
from ..base import BaseEstimator
from .base import MultiSequenceClusterMixin
from .minibatchkmeans import _work_dtype, kmeans_plusplus, label_inertia

__all__ = ['KMeans', 'lloyd_plan', 'lloyd_run']

LLOYD_MAXITER, LLOYD_STRICT, LLOYD_TOL = 0, 1, 2
_PLAN_FIELDS = ("hist_span", "hist_groups", "piece", "pieces_max", "feature_tiles", "tile_features", "vec16", "scratch_bytes")


def lloyd_plan(n, m, K, dtype=np.float32, aligned=True):
    """What the centre update of one iteration launches for ``n`` rows of ``m`` features and ``K`` clusters
    (``msm_lloyd_plan``; a pure host function, no device needed): a dict of rows per histogram wave, histogram waves,
    members per piece of the segmented sum, the upper bound on pieces, feature tiles, features per tile, whether rows
    are read with 16-byte loads, and scratch bytes."""
    out = (C.c_int64 * 8)()
    check(_lib.lib().msm_lloyd_plan(int(n), int(m), int(K), int(np.dtype(dtype) == np.float64), int(bool(aligned)), out))
    return dict(zip(_PLAN_FIELDS, (int(v) for v in out)))


def lloyd_run(X, centers, max_iter=300, tol_abs=0.0):
    """Lloyd iterations from ``centers`` on the rows ``X`` (numpy or torch CUDA; float32 stays float32, everything else is
    float64) exactly as given -- no centring, ``tol_abs`` is the absolute bound on the summed squared centre shift.
    Returns (centers, labels, inertia, n_iter, status): ``labels`` int32 placed like ``X``, ``status`` one of
    ``LLOYD_MAXITER`` / ``LLOYD_STRICT`` / ``LLOYD_TOL``."""
    ax = X if isinstance(X, Arr) else Arr(X, _work_dtype(X))
    centers = np.ascontiguousarray(centers, dtype=ax.dtype)
    if len(ax.shape) != 2 or centers.ndim != 2 or centers.shape[1] != ax.shape[1]:
        raise ValueError("lloyd_run: X must be [n, F] and centers [K, F]")
    L = _lib.lib()
    labels = _lib.empty_like_placement(ax, (ax.shape[0],), np.int32)
    al = Arr(labels, np.int32)
    h = C.c_void_p()
    create = L.msm_lloyd_create_f64 if ax.dtype == np.float64 else L.msm_lloyd_create
    check(create(C.byref(h), centers.shape[0], centers.shape[1]))
    try:
        check(L.msm_lloyd_set_centers(h, centers.ctypes.data))
        inertia, n_iter, status = C.c_double(0.0), C.c_int64(0), C.c_int(0)
        check(L.msm_lloyd_run(h, ax.vp, ax.shape[0], int(max_iter), float(tol_abs), al.vp, ax.on_device,
                              C.byref(inertia), C.byref(n_iter), C.byref(status)))
        out = np.empty_like(centers)
        check(L.msm_lloyd_get_centers(h, out.ctypes.data))
    finally:
        L.msm_lloyd_destroy(h)
    return out, labels, float(inertia.value), int(n_iter.value), int(status.value)


def _colstats(xd):
    """(mean, variance) per column of a device tensor, float64 (``msm_colstats``)."""
    ax = Arr(xd)
    F = ax.shape[1]
    out = np.empty((5, F))
    has_inf = C.c_int(0)
    ptrs = (C.c_void_p * 1)(ax.ptr)
    rows = (C.c_int64 * 1)(ax.shape[0])
    check(_lib.lib().msm_colstats(ptrs, rows, 1, ax.dtype.itemsize, F, F, 1, out.ctypes.data, C.byref(has_inf)))
    if has_inf.value or np.any(out[0] != ax.shape[0]):
        raise ValueError("Input X contains NaN or infinity.")
    return out[1], out[2] / out[0]


def _shift_rows(xd, shift, mode):
    """In place on a device tensor: mode 0 ``x - shift``, mode 1 ``x + shift`` (``msm_scale_apply``, the scalers' kernel)."""
    ax = Arr(xd)
    sh = np.ascontiguousarray(shift, dtype=np.float64)
    check(_lib.lib().msm_scale_apply(ax.ptr, ax.dtype.itemsize, ax.shape[0], ax.shape[1], ax.shape[1], sh.ctypes.data, None,
                                     mode, ax.ptr, ax.shape[1], 1))


class _KMeans(ClusterMixin, TransformerMixin):
    """Single-array k-means with scikit-learn 1.7's constructor."""

    def __init__(self, n_clusters=8, init='k-means++', n_init='auto', max_iter=300, tol=1e-4, verbose=0,
                 random_state=None, copy_x=True, algorithm='lloyd'):
        self.n_clusters = n_clusters
        self.init = init
        self.n_init = n_init
        self.max_iter = max_iter
        self.tol = tol
        self.verbose = verbose
        self.random_state = random_state
        self.copy_x = copy_x
        self.algorithm = algorithm

    def _check_params_vs_input(self, n_samples):
        if self.algorithm not in ("lloyd", "elkan"):
            raise ValueError("The 'algorithm' parameter of KMeans must be a str among {'lloyd', 'elkan'}. Got %r instead."
                             % (self.algorithm,))
        if n_samples < self.n_clusters:
            raise ValueError("n_samples=%d should be >= n_clusters=%d." % (n_samples, self.n_clusters))
        n_init = self.n_init
        if isinstance(n_init, str):
            if n_init != "auto":
                raise ValueError("The 'n_init' parameter of KMeans must be a str among {'auto'} or an int in the range "
                                 "[1, inf). Got %r instead." % (n_init,))
            n_init = 10 if isinstance(self.init, str) and self.init == "random" else 1
            if callable(self.init):
                n_init = 10
        elif isinstance(n_init, bool) or not isinstance(n_init, (int, np.integer)) or n_init < 1:
            raise ValueError("The 'n_init' parameter of KMeans must be a str among {'auto'} or an int in the range "
                             "[1, inf). Got %r instead." % (n_init,))
        if isinstance(self.init, str) and self.init not in ("k-means++", "random"):
            raise ValueError("The 'init' parameter of KMeans must be a str among {'k-means++', 'random'}, a callable or "
                             "an array-like. Got %r instead." % (self.init,))
        self._n_init = int(n_init)
        if (hasattr(self.init, "__array__") or is_device_array(self.init)) and self._n_init != 1:
            import warnings
            warnings.warn("Explicit initial center position passed: performing only one init in KMeans instead of "
                          "n_init=%d." % self._n_init, RuntimeWarning)
            self._n_init = 1

    def _init_centroids(self, xd, host_input, mean_t, random_state):
        """_kmeans.py ``_init_centroids`` on the centred rows ``xd`` (device); returns host centres of the rows' type."""
        K, F = self.n_clusters, xd.shape[1]
        dtype = mean_t.dtype
        init = self.init
        if isinstance(init, str) and init == "k-means++":
            centers = kmeans_plusplus(xd, K, random_state)   # on the device (csrc/kpp.hip), scikit-learn's draws
        elif isinstance(init, str) and init == "random":
            n = xd.shape[0]
            w = np.ones(n, dtype=dtype)
            seeds = random_state.choice(n, size=K, replace=False, p=w / w.sum())
            import torch
            centers = xd[torch.as_tensor(np.ascontiguousarray(seeds, dtype=np.int64), device=xd.device)].cpu().numpy()
        elif callable(init):
            centers = np.asarray(init(xd.cpu().numpy() if host_input else xd, K, random_state=random_state))
            if is_device_array(centers):
                centers = centers.detach().cpu().numpy()
        else:
            if is_device_array(init):
                init = init.detach().cpu().numpy()
            centers = np.array(init, dtype=dtype, copy=True, order="C")
            if centers.ndim == 2 and centers.shape == (K, F):
                centers -= mean_t
        centers = np.ascontiguousarray(centers, dtype=dtype)
        if centers.ndim != 2 or centers.shape[0] != K:
            raise ValueError("The shape of the initial centers %s does not match the number of clusters %d."
                             % (centers.shape, K))
        if centers.shape[1] != F:
            raise ValueError("The shape of the initial centers %s does not match the number of features of the data %d."
                             % (centers.shape, F))
        return centers

    def fit(self, X, y=None):
        import torch
        dtype = _work_dtype(X)
        if len(X.shape) != 2:
            raise ValueError("Expected 2D array")
        n_samples, n_features = int(X.shape[0]), int(X.shape[1])
        self._check_params_vs_input(n_samples)
        random_state = check_random_state(self.random_state)
        host_input = not is_device_array(X)
        tdt = torch.float64 if dtype == np.float64 else torch.float32
        if host_input:   # the upload is the copy: the caller's array is never written
            _lib.ensure_device()
            xd = torch.from_numpy(np.ascontiguousarray(X, dtype=dtype)).cuda()
            in_place = False
        else:
            src = X if (X.dtype == tdt and X.is_contiguous()) else X.to(tdt).contiguous()
            in_place = (not self.copy_x) and src is X
            xd = src if (in_place or src is not X) else src.clone()
        self.n_features_in_ = n_features

        mean, var = _colstats(xd)
        tol_abs = float(np.mean(var)) * self.tol
        mean_t = mean.astype(dtype)
        _shift_rows(xd, mean_t, 0)
        try:
            best = None
            for _ in range(self._n_init):
                centers0 = self._init_centroids(xd, host_input, mean_t, random_state)
                centers, labels, inertia, n_iter, status = lloyd_run(xd, centers0, self.max_iter, tol_abs)
                if self.verbose:
                    print("KMeans: %d iterations, inertia %s (%s)" % (n_iter, inertia, ("max_iter reached", "strict convergence",
                                                                                         "centre shift within tolerance")[status]))
                if best is None or inertia < best[2]:
                    best = (centers, labels, inertia, n_iter)
        finally:
            if in_place:
                _shift_rows(xd, mean_t, 1)
        centers, labels, inertia, n_iter = best
        centers += mean_t
        self.cluster_centers_ = centers
        self.labels_ = labels.cpu().numpy() if host_input else labels
        self.inertia_ = inertia
        self.n_iter_ = n_iter
        return self

    def _like_centers(self, X):
        return Arr(X, self.cluster_centers_.dtype)

    def predict(self, X):
        """Index of the closest centre (squared euclidean, GEMM form, in the centres' element type) for each row of X."""
        labels, _ = label_inertia(self._like_centers(X), self.cluster_centers_)
        return labels

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def score(self, X, y=None):
        """Opposite of the k-means objective on X."""
        _, inertia = label_inertia(self._like_centers(X), self.cluster_centers_)
        return -inertia


class KMeans(MultiSequenceClusterMixin, _KMeans, BaseEstimator):
    __doc__ = """K-Means clustering of a list of sequences (see module docstring).

    Parameters are scikit-learn 1.7's ``KMeans`` parameters (``algorithm='elkan'`` is accepted and runs Lloyd);
    ``labels_`` is a list of int32 arrays, one per input sequence (msmbuilder/cluster/base.py:50-51).
    """

    def fit_predict(self, sequences, y=None):
        self.fit(sequences)
        return self.labels_

    def summarize(self):
        return """KMeans clustering
-----------------
n_clusters : {n_clusters}
n_iter     : {n_iter}

Inertia    : {inertia}
""".format(n_clusters=self.n_clusters, n_iter=getattr(self, "n_iter_", None), inertia=getattr(self, "inertia_", None))
