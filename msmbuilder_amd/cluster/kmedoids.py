"""K-medoids clustering on MI355X: drop-in for ``msmbuilder.cluster.KMedoids``
(reference: msmbuilder/cluster/kmedoids.py:22-173 over _kmedoids.pyx and src/kmedoids.cc).

The reference computes the condensed distance matrix with ``libdistance.pdist`` and runs the k-medoids loop of the C
clustering library over it on one CPU thread.  Here both are ONE call, ``msm_kmedoids_fit_*``: the matrix is written by
the pdist kernel into device memory and stays there, and every iteration of the loop -- the summed distance of every
element to the other members of its cluster, the medoid of every cluster, the new assignment, the total -- runs over it
on the GPU.  Every sum is added in the reference's order, so ``labels_``, ``cluster_ids_`` and ``inertia_`` are the
reference's bit for bit.  The random initial assignments, which the reference draws from the ``RandomState`` inside
its C loop, are drawn here up front with the same calls in the same order: they do not depend on the data, and the
generator ends in the state the reference leaves it in.
"""
import ctypes as C

import numpy as np
from sklearn.base import ClusterMixin, TransformerMixin
from sklearn.utils import check_random_state

from .. import _lib, libdistance
from .._lib import Arr, check, is_device_array
from ..base import BaseEstimator
from .base import MultiSequenceClusterMixin
from .minibatchkmeans import _rows_to_host

__all__ = ['KMedoids']


def random_assignments(random_state, n_elements, n_clusters, n_passes):
    """The ``n_passes`` initial assignments of kmedoids.cc:314-383 (randomassign), one row each: cluster sizes from
    successive binomial draws with one element reserved per cluster, then a shuffle -- the calls the reference makes
    on the generator from C, in its order."""
    out = np.empty((n_passes, n_elements), dtype=np.intp)
    for p in range(n_passes):
        n_free, k = n_elements - n_clusters, 0
        for i in range(n_clusters - 1):
            j = int(random_state.binomial(float(n_free), 1.0 / (n_clusters - i)))
            n_free -= j
            out[p, k:k + j + 1] = i
            k += j + 1
        out[p, k:] = n_clusters - 1
        random_state.shuffle(out[p])
    return out


def contigify_ids(ids):
    """Medoid ids renumbered 0, 1, ... in order of first appearance (kmedoids.cc:386-400): (labels, the ids in that
    order)."""
    ids = np.asarray(ids)
    uniq, first, inv = np.unique(ids, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')
    rank = np.empty(len(uniq), dtype=np.intp)
    rank[order] = np.arange(len(uniq))
    return rank[inv.reshape(-1)].astype(np.intp), uniq[order]


def vector_metric(metric):
    metric = metric.decode() if isinstance(metric, bytes) else metric
    if metric not in libdistance.VECTOR_METRICS:
        raise ValueError('metric must be one of %s' % ', '.join("'%s'" % s for s in libdistance.VECTOR_METRICS))
    return metric


def working_array(X):
    """The reference's dtype rule (kmedoids.py:88-90): float32 and float64 rows are used as given, anything else is
    computed in float64."""
    if isinstance(X, np.ndarray):
        if X.dtype not in (np.float32, np.float64):
            X = np.asarray(X, dtype=np.float64)
    elif is_device_array(X):
        import torch
        if X.dtype not in (torch.float32, torch.float64):
            X = X.to(torch.float64)
    else:
        raise TypeError('X must be a numpy array or a torch CUDA tensor')
    ax = Arr(X)
    if len(ax.shape) != 2:
        raise ValueError("X must be 2-dimensional")
    return ax


def kmedoids_fit(ax, metric, n_clusters, n_pass, init, X_indices=None):
    """``msm_kmedoids_fit_*`` on the rows (or the indexed rows) of ``ax``: (medoid id per element, error, ifound)."""
    kind = "f64" if ax.dtype == np.float64 else "f32"
    idx, n = None, ax.shape[0]
    if X_indices is not None and not ax.on_device:
        # host rows: only the indexed rows travel (a mini-batch is 108 rows of possibly millions); the distances of the
        # gathered rows are those of the indexed ones bit for bit
        ax = Arr(np.ascontiguousarray(ax.keep[np.asarray(X_indices, dtype=np.int64)]))
        n = ax.shape[0]
    elif X_indices is not None:
        import torch
        idx = Arr(torch.as_tensor(np.ascontiguousarray(X_indices, dtype=np.int64), device=ax.keep.device), np.int64)
        n = idx.shape[0]
    init = np.ascontiguousarray(init, dtype=np.int64).reshape(max(n_pass, 1), n)
    ids = np.zeros(n, dtype=np.int64)
    error, ifound = C.c_double(0.0), C.c_int64(0)
    check(getattr(_lib.lib(), "msm_kmedoids_fit_" + kind)(
        ax.vp, ax.shape[0], ax.shape[1], metric.encode(), idx.vp if idx is not None else None, n, int(n_clusters),
        int(n_pass), init.ctypes.data, ids.ctypes.data, C.byref(error), C.byref(ifound), ax.on_device))
    return ids.astype(np.intp), error.value, int(ifound.value)


def rmsd_input(est, X):
    """Prepared frames when the estimator's metric is rmsd and X is a set of conformations, else None."""
    if libdistance.is_rmsd(est.metric) and libdistance.conformations(X) is not None:
        return X if isinstance(X, libdistance.RmsdFrames) else libdistance.RmsdFrames(X)
    return None


def kmedoids_fit_rmsd(frames, n_clusters, n_pass, init, X_indices=None):
    """``kmedoids_fit`` for conformations: ``msm_rmsd_pdist`` of the (indexed) frames into device memory, then the
    existing loop ``msm_kmedoids`` over that matrix where it lies."""
    dmat = libdistance.rmsd_pdist(frames, X_indices, device=True)
    n = len(frames) if X_indices is None else len(X_indices)
    init = np.ascontiguousarray(init, dtype=np.int64).reshape(max(n_pass, 1), n)
    ids = np.zeros(n, dtype=np.int64)
    error, ifound = C.c_double(0.0), C.c_int64(0)
    check(_lib.lib().msm_kmedoids(Arr(dmat, np.float64).vp, n, int(n_clusters), int(n_pass), init.ctypes.data, ids.ctypes.data,
                                  C.byref(error), C.byref(ifound), 1))
    return ids.astype(np.intp), error.value, int(ifound.value)


def nearest_centre(est, X):
    """``predict`` of both k-medoids estimators: the exact ``assign_nearest`` kernel against the fitted centres, on rows
    cast by the fit's dtype rule."""
    if rmsd_input(est, X) is not None:
        return libdistance.assign_nearest(X, est.cluster_centers_, metric="rmsd")[0]
    ax = working_array(X)
    return libdistance.assign_nearest(ax.keep, est.cluster_centers_, metric=vector_metric(est.metric))[0]


def last_stats():
    """{passes, iterations, small, snapshots} of this process's last k-medoids call (``msm_kmedoids_last_stats``)."""
    out = (C.c_int64 * 4)()
    check(_lib.lib().msm_kmedoids_last_stats(out))
    return dict(zip(("passes", "iterations", "small", "snapshots"), (int(v) for v in out)))


class _KMedoids(ClusterMixin, TransformerMixin):
    """K-Medoids clustering of ONE array (the sequence-list estimator is :class:`KMedoids`).

    Finds cluster centres that are themselves data points, lowering the summed distance from the data points to their
    centres.  The full distance matrix between all pairs of data points is computed, O(N^2) memory -- on the device.
    The method is that of the C clustering library (de Hoon et al., Bioinformatics 20 (2004) 1453).

    Parameters
    ----------
    n_clusters : int, optional, default: 8
        The number of clusters to be found.
    n_passes : int, default=1
        The number of times clustering is performed, each time starting from a different (random) initial
        assignment; the pass with the lowest summed distance is kept.
    metric : str (default "euclidean")
        One of libdistance's vector metrics: euclidean, sqeuclidean, cityblock, chebyshev, canberra, braycurtis,
        hamming, jaccard -- or "rmsd" for conformations: float32 (n_frames, n_atoms, 3) arrays, torch CUDA tensors or
        objects with such an ``.xyz``; ``cluster_centers_`` is then a host (n_clusters, n_atoms, 3) array.
    random_state : integer or numpy.RandomState, optional
        The generator of the initial assignments.  An integer fixes the seed; the default is numpy's global one.

    Rows are numpy arrays or torch CUDA tensors; float32 and float64 rows are used as given, any other dtype is cast
    to float64.  A NaN or infinite distance raises ``ValueError``: the loop is not defined for them.

    The result depends on all pairs of rows, so there is no row-sharded form: a fit inside an initialised
    ``torch.distributed`` clusters exactly the rows the calling process was given, on its own GPU, with no collective.

    Attributes
    ----------
    cluster_ids_ : array, [n_clusters]
        Index of the data point that each cluster label corresponds to.
    cluster_centers_ : (n_clusters, n_features) host array of X's dtype, the rows themselves
    labels_ : array, [n_samples,]
        The label of each point is an integer in [0, n_clusters).
    inertia_ : float
        Sum of distances of samples to their closest cluster center (``DBL_MAX`` when the single pass ended with every
        label equal to its medoid's index, as in the reference).
    """

    def __init__(self, n_clusters=8, n_passes=1, metric='euclidean', random_state=None):
        self.n_clusters = n_clusters
        self.n_passes = n_passes
        self.metric = metric
        self.random_state = random_state

    def fit(self, X, y=None):
        if self.n_passes < 1:
            raise ValueError('n_passes must be greater than 0. got %s' % self.n_passes)
        if self.n_clusters < 1:
            raise ValueError('n_passes must be greater than 0. got %s' % self.n_clusters)
        frames = rmsd_input(self, X)
        if frames is None:
            metric = vector_metric(self.metric)
            ax = working_array(X)
        n = len(frames) if frames is not None else ax.shape[0]
        if self.n_clusters > n:
            raise ValueError('Number of clusters requested (%d) greater than number of elements (%d)'
                             % (self.n_clusters, n))
        init = random_assignments(check_random_state(self.random_state), n, self.n_clusters, self.n_passes)
        if frames is not None:
            # conformations: the condensed rmsd matrix on the device, then the same loop; the centres are the medoids'
            # original coordinates, host (n_clusters, n_atoms, 3)
            ids, self.inertia_, _ = kmedoids_fit_rmsd(frames, self.n_clusters, self.n_passes, init)
            self.labels_, self.cluster_ids_ = contigify_ids(ids)
            self.cluster_centers_ = frames.frames(self.cluster_ids_)
            return self
        ids, self.inertia_, _ = kmedoids_fit(ax, metric, self.n_clusters, self.n_passes, init)
        self.labels_, self.cluster_ids_ = contigify_ids(ids)
        # cluster_centers_ (kmedoids.py:98: X[cluster_ids_]) is a HOST array like the other clusterers': predict needs it there
        self.cluster_centers_ = _rows_to_host(ax, self.cluster_ids_)
        return self

    def predict(self, X):
        """Index of the closest cluster centre for each sample in X (kmedoids.py:102-124 -> libdistance.assign_nearest)."""
        return nearest_centre(self, X)

    def fit_predict(self, X, y=None):
        return self.fit(X, y).labels_


class KMedoids(MultiSequenceClusterMixin, _KMedoids, BaseEstimator):
    __doc__ = _KMedoids.__doc__[: _KMedoids.__doc__.find('Attributes')] + \
        '''Attributes
    ----------
    cluster_ids_ : (n_clusters, 2) int array, one (trajectory index, frame index) pair per centre
    cluster_centers_ : (n_clusters, n_features)
    labels_ : list of arrays, one per sequence, each label in [0, n_clusters)
    inertia_ : float
    '''
    _takes_rmsd = True

    def fit(self, sequences, y=None):
        """Fit the clustering on a list of [sequence_length, n_features] arrays."""
        MultiSequenceClusterMixin.fit(self, sequences)
        self.cluster_ids_ = self._split_indices(self.cluster_ids_)
        return self

    def summarize(self):
        return """KMedoids clustering
-------------------
n_clusters : {n_clusters}
n_passes   : {n_passes}
metric     : {metric}

Inertia    : {inertia_}
""".format(**self.__dict__)
