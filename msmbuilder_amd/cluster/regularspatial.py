"""Regular spatial clustering on MI355X: drop-in for ``msmbuilder.cluster.RegularSpatial``
(reference: msmbuilder/cluster/regularspatial.py:25-140).

The reference walks the rows in Python, one ``libdistance.dist(X, X[i], X_indices=centres)`` call per row on one
thread (regularspatial.py:69-81).  Here the whole loop is ``msm_regspatial_fit_*`` in libmsmhip: the rows are taken in
blocks; a block is screened against the centres known so far on the whole GPU, the rows that no centre covers are
compacted and resolved in row order by one workgroup, and the host synchronises once per block.  Every distance is the
exact libdistance one and every decision is the reference's ``d > d_min``, so the chosen rows are the reference's:
the same ids in the same order, for float32 and float64 rows and every vector metric.  ``predict`` is the exact
``assign_nearest`` kernel.
"""
import ctypes as C

import numpy as np
from sklearn.base import ClusterMixin, TransformerMixin

from .. import _lib, libdistance
from .._lib import Arr, check, is_device_array
from ..base import BaseEstimator
from .base import MultiSequenceClusterMixin

__all__ = ['RegularSpatial']


class _RegularSpatial(ClusterMixin, TransformerMixin):
    """Leader clustering of ONE array (the sequence-list estimator is :class:`RegularSpatial`).

    The first row is a centre; going through the rows in order, a row becomes a centre when it is farther than
    ``d_min`` from every centre chosen before it (Senne et al., J. Chem. Theory Comput. 8 (2012) 2223).  The centres
    are data points, roughly evenly spaced in the metric; their number follows from ``d_min``.

    Parameters
    ----------
    d_min : float
        Minimum distance between centres.  A row at exactly ``d_min`` from a centre, or at a NaN distance, is not a
        centre; ``d_min < 0`` makes every row one.
    metric : str (default "euclidean")
        One of libdistance's vector metrics: euclidean, sqeuclidean, cityblock, chebyshev, canberra, braycurtis,
        hamming, jaccard.  (The reference's "rmsd" needs mdtraj trajectories and is out of scope.)

    Rows are float32 or float64 numpy arrays or torch CUDA tensors and are used as given: there is no dtype
    conversion (the reference has none; ``libdistance.dist`` accepts these two types).

    The result depends on the order of the rows, so there is no row-sharded form: a fit inside an initialised
    ``torch.distributed`` clusters exactly the rows the calling process was given, on its own GPU, with no collective.

    Attributes
    ----------
    cluster_center_indices_ : list of n_clusters_ row indices, ascending (the order they were chosen in)
    cluster_centers_ : (n_clusters_, n_features) host array of X's dtype, the rows themselves
    n_clusters_ : int
    """

    _block_rows = 0   # test hook: rows per block of the device loop, 0 = the library's rule

    def __init__(self, d_min, metric='euclidean'):
        self.d_min = d_min
        self.metric = metric

    def _metric(self):
        metric = self.metric.decode() if isinstance(self.metric, bytes) else self.metric
        if metric not in libdistance.VECTOR_METRICS:
            raise ValueError('metric must be one of %s' %
                             ', '.join("'%s'" % s for s in libdistance.VECTOR_METRICS))
        return metric

    def fit(self, X, y=None):
        metric = self._metric()
        if not (isinstance(X, np.ndarray) or is_device_array(X)):
            raise TypeError('X must be a numpy array or a torch CUDA tensor')
        ax = Arr(X)
        if len(ax.shape) != 2:
            raise ValueError("X must be 2-dimensional")
        if ax.dtype not in (np.float32, np.float64):
            raise TypeError('X and y must be both float32 or float64')
        kind = "f64" if ax.dtype == np.float64 else "f32"
        L = _lib.lib()
        k = C.c_int64(0)
        check(getattr(L, "msm_regspatial_fit_" + kind)(ax.vp, ax.shape[0], ax.shape[1], metric.encode(),
                                                       float(self.d_min), int(self._block_rows), ax.on_device, C.byref(k)))
        # cluster_centers_ (regularspatial.py:79: X[ids]) comes back as a HOST array like KCenters': predict needs it there
        ids = np.empty(k.value, dtype=np.int64)
        centers = np.empty((k.value, ax.shape[1]), dtype=ax.dtype)
        check(getattr(L, "msm_regspatial_result_" + kind)(ids.ctypes.data, centers.ctypes.data))
        self.cluster_center_indices_ = ids.tolist()
        self.cluster_centers_ = centers
        self.n_clusters_ = int(k.value)
        return self

    def predict(self, X):
        """Index of the closest cluster centre for each sample in X
        (regularspatial.py:83-102 -> libdistance.assign_nearest)."""
        labels, inertia = libdistance.assign_nearest(X, self.cluster_centers_, metric=self._metric())
        return labels

    def fit_predict(self, X, y=None):
        return self.fit(X, y=y).predict(X)


def last_stats():
    """{blocks, survivors, rounds, growths} of this process's last fit (``msm_regspatial_last_stats``)."""
    out = (C.c_int64 * 4)()
    check(_lib.lib().msm_regspatial_last_stats(out))
    return dict(zip(("blocks", "survivors", "rounds", "growths"), (int(v) for v in out)))


class RegularSpatial(MultiSequenceClusterMixin, _RegularSpatial, BaseEstimator):
    __doc__ = _RegularSpatial.__doc__[: _RegularSpatial.__doc__.find('Attributes')] + \
        '''Attributes
    ----------
    cluster_center_indices_ : (n_clusters_, 2) int array, one (trajectory index, frame index) pair per centre
    cluster_centers_ : (n_clusters_, n_features)
    n_clusters_ : int
    '''

    def fit(self, sequences, y=None):
        """Fit the clustering on a list of [sequence_length, n_features] arrays."""
        MultiSequenceClusterMixin.fit(self, sequences)
        self.cluster_center_indices_ = self._split_indices(self.cluster_center_indices_)
        return self

    def fit_predict(self, sequences, y=None):
        return self.fit(sequences).predict(sequences)

    def summarize(self):
        return """
RegularSpatial clustering
-------------------------
d_min      : {d_min}
metric     : {metric}

n_clusters : {n_clusters}
""".format(d_min=self.d_min, metric=self.metric,
           n_clusters=self.n_clusters_)
