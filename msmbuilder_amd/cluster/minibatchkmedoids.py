"""Mini-batch k-medoids clustering on MI355X: drop-in for ``msmbuilder.cluster.MiniBatchKMedoids``
(reference: msmbuilder/cluster/minibatchkmedoids.py:22-200).

The reference's loop with the same ``randint`` calls in the same order: initial ``cluster_ids_``, initial
``labels_``, then one batch per iteration.  Each step clusters the current centres plus the batch, starting from the
labels the batch's rows have: ONE ``msm_kmedoids_fit_*`` call that computes the condensed matrix of those rows on the
device and runs the k-medoids pass over it there (with the default sizes, 8 + 100 rows, in a single launch on one
workgroup).  The bookkeeping between the steps is the reference's numpy.  The final ``labels_`` and ``inertia_`` are
the exact ``assign_nearest`` kernel's, the inertia added over its distances in row order as the reference's assign.hpp
adds it (the kernel's own inertia is a tree sum).
"""
import ctypes as C

import numpy as np
from sklearn.base import ClusterMixin, TransformerMixin
from sklearn.utils import check_random_state

from .. import _lib, libdistance
from .._lib import Arr, check, empty_like_placement
from ..base import BaseEstimator
from .base import MultiSequenceClusterMixin
from .kmedoids import (contigify_ids, kmedoids_fit, kmedoids_fit_rmsd, nearest_centre, rmsd_input, vector_metric,
                       working_array)
from .minibatchkmeans import _rows_to_host

__all__ = ['MiniBatchKMedoids']


def assign_ordered(ax, centers, metric):
    """``libdistance.assign_nearest(X, centers)`` with the reference's inertia bits: labels (placed like X) and the sum
    of the minimum distances in row order (assign.hpp:30: ``inertia += min_d`` row after row).  The distances of
    device rows come to the host for that sum, 8 bytes per row."""
    n, kind = ax.shape[0], "f64" if ax.dtype == np.float64 else "f32"
    ay = np.ascontiguousarray(centers, dtype=ax.dtype)
    labels = empty_like_placement(ax, (n,), np.intp)
    dist = empty_like_placement(ax, (n,), np.float64)
    if n == 0:
        return labels, 0.0
    al, ad = Arr(labels, np.int64), Arr(dist, np.float64)
    inertia = C.c_double(0.0)
    check(getattr(_lib.lib(), "msm_assign_nearest_" + kind)(
        ax.vp, C.c_void_p(ay.ctypes.data), metric.encode(), None, n, ay.shape[0], ax.shape[1], n, al.vp, ad.vp,
        C.byref(inertia), ax.on_device))
    d = dist.cpu().numpy() if ax.on_device else dist
    return labels, float(np.add.accumulate(d)[-1])


class _MiniBatchKMedoids(ClusterMixin, TransformerMixin):
    """Mini-Batch K-Medoids clustering of ONE array (the sequence-list estimator is :class:`MiniBatchKMedoids`).

    Finds cluster centres that are themselves data points using only mini-batches of the data: each batch is
    augmented with the current centres and clustered by k-medoids, so the memory scales with the square of
    ``batch_size`` instead of the square of the data's size.

    Parameters
    ----------
    n_clusters : int, optional, default: 8
        The number of clusters to form.
    max_iter : int, optional, default=5
        Maximum number of iterations over the complete dataset.
    batch_size : int, optional, default: 100
        Size of the mini batches.
    metric : str (default "euclidean")
        One of libdistance's vector metrics: euclidean, sqeuclidean, cityblock, chebyshev, canberra, braycurtis,
        hamming, jaccard -- or "rmsd" for conformations: float32 (n_frames, n_atoms, 3) arrays, torch CUDA tensors or
        objects with such an ``.xyz``; ``cluster_centers_`` is then a host (n_clusters, n_atoms, 3) array.
    max_no_improvement : int, default: 10
        Stop after this many consecutive mini batches that change no assignment.
    random_state : integer or numpy.RandomState, optional
        The generator of the initial centres, labels and the batches.

    Rows are numpy arrays or torch CUDA tensors; float32 and float64 rows are used as given, any other dtype is cast
    to float64.  A NaN or infinite distance inside a batch raises ``ValueError``.

    The batches index all rows, so there is no row-sharded form: a fit inside an initialised ``torch.distributed``
    clusters exactly the rows the calling process was given, on its own GPU, with no collective.

    Attributes
    ----------
    cluster_ids_ : array, [n_clusters]
        Index of the data point that each cluster label corresponds to.
    cluster_centers_ : (n_clusters, n_features) host array of X's dtype, the rows themselves
    labels_ : array, [n_samples,]
        The label of each point is an integer in [0, n_clusters).
    inertia_ : float
        Sum of distances of samples to their closest cluster center.
    """

    def __init__(self, n_clusters=8, max_iter=5, batch_size=100, metric='euclidean', max_no_improvement=10,
                 random_state=None):
        self.n_clusters = n_clusters
        self.batch_size = batch_size
        self.max_iter = max_iter
        self.max_no_improvement = max_no_improvement
        self.metric = metric
        self.random_state = random_state

    def fit(self, X, y=None):
        frames = rmsd_input(self, X)   # conformations: prepared once, every batch gathers from the same image
        if frames is None:
            metric = vector_metric(self.metric)
            ax = working_array(X)
        n, K, B = len(frames) if frames is not None else ax.shape[0], self.n_clusters, self.batch_size
        rs = check_random_state(self.random_state)
        # the generator is used exactly as the reference uses it (minibatchkmedoids.py:89-98): K centre rows, one label
        # per row, then B row indices per step
        centres = rs.randint(0, n, size=K)
        labels = rs.randint(0, K, size=n)
        own = np.arange(K)
        budget = int(self.max_iter * int(np.ceil(float(n) / B)))
        quiet, self.n_steps_ = 0, 0
        for _ in range(budget):
            rows = np.concatenate([centres, rs.randint(0, n, B)]).astype(np.intp)
            # positions 0 .. K-1 are the centres, each starting in its own cluster; a batch row starts where it is now
            start = np.concatenate([own, labels[rows[K:]]])
            if frames is not None:
                medoids, _, _ = kmedoids_fit_rmsd(frames, K, 0, start, X_indices=rows)
            else:
                medoids, _, _ = kmedoids_fit(ax, metric, K, 0, start, X_indices=rows)
            self.n_steps_ += 1
            new_labels, positions = contigify_ids(medoids)   # clusters renumbered by first appearance over the positions
            centres = rows[positions]
            if np.array_equal(labels[rows], new_labels):
                quiet += 1
            else:
                labels[rows] = new_labels   # (a row drawn twice keeps the label of its last position, as numpy assigns)
                quiet = 0
            if quiet >= self.max_no_improvement:   # tested after the step: at least one step runs
                break

        self.cluster_ids_ = centres
        if frames is not None:
            self.cluster_centers_ = frames.frames(centres)
            self.labels_, dist, _ = libdistance.rmsd_assign(frames, libdistance.RmsdFrames(self.cluster_centers_))
            dist = dist.cpu().numpy() if frames.on_device else dist
            self.inertia_ = float(np.add.accumulate(dist)[-1]) if n else 0.0   # in row order, as below
            return self
        self.cluster_centers_ = _rows_to_host(ax, centres)
        self.labels_, self.inertia_ = assign_ordered(ax, self.cluster_centers_, metric)
        return self

    def predict(self, X):
        """Index of the closest cluster centre for each sample in X
        (minibatchkmedoids.py:131-153 -> libdistance.assign_nearest)."""
        return nearest_centre(self, X)

    def fit_predict(self, X, y=None):
        return self.fit(X, y).labels_


class MiniBatchKMedoids(MultiSequenceClusterMixin, _MiniBatchKMedoids, BaseEstimator):
    __doc__ = _MiniBatchKMedoids.__doc__[: _MiniBatchKMedoids.__doc__.find('Attributes')] + \
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
        return """MiniBatchKMedoids clustering
----------------------------
n_clusters : {n_clusters}
metric     : {metric}

Inertia    : {inertia_}
""".format(**self.__dict__)
