"""Landmark agglomerative clustering on MI355X: drop-in for ``msmbuilder.cluster.LandmarkAgglomerative``
(reference: msmbuilder/cluster/agglomerative.py:77-289).

The reference computes the condensed distance matrix of the landmarks with ``libdistance.pdist``, hands it to
fastcluster's linkage on one CPU thread, walks all L(L-1)/2 pairs in a Python loop for the within-cluster sums, and in
``predict`` forms the N x L ``cdist`` matrix on the host and pools it cluster by cluster in numpy.  Here the matrix is
written by the pdist kernel into device memory and stays there: ``msm_linkage_fit_*`` runs the agglomeration over it (plain
global-minimum merging with cached nearest neighbours, three small launches per merge, all queued before the host reads
the (L-1) x 4 linkage matrix), ``msm_landmark_within`` adds the squared distances per cluster in a fixed order, and
``msm_landmark_predict_*`` is one fused kernel that computes each distance with libdistance's exact arithmetic, pools per
cluster and keeps the running minimum, so the N x L matrix is never formed.  Only ``fcluster`` on the small linkage
matrix, ``bincount`` and the L x F means of ``cluster_centers_`` run on the host.

Besides libdistance's vector metrics the three symmetric divergences of ``utils.divergence`` (``js_metric``,
``js_divergence``, ``sym_kl_divergence``, by name or as their ``*_array`` functions) are metrics here: the fit queues the
divergence tile kernel's condensed matrix in the vector pdist's place, and predict computes the divergences of blocks of
rows to the landmarks into a bounded scratch buffer and pools each block with the same pooling code
(``msm_landmark_predict_dmat``'s kernel).  That is what ``lumping.MVCA`` is assembled from.

Ties: the pair of lowest distance is merged; among equal distances the lowest row slot, then the lowest column slot,
where a merged cluster lives on in the higher of its two slots.  ``average`` and ``ward`` pooled values are sums of one
term per landmark in ascending landmark order within the cluster (numpy's ``mean`` / ``sum`` add pairwise): they agree
with the reference's to a few units in the last place, and so do the labels wherever the best and the second-best
cluster are further apart than that.
"""
import ctypes as C
import warnings

import numpy as np
from sklearn.base import ClusterMixin, TransformerMixin
from sklearn.utils import check_random_state

from .. import _lib, libdistance
from .._lib import Arr, check
from ..base import BaseEstimator
from ..utils import divergence
from .base import MultiSequenceClusterMixin
from .kmedoids import working_array
from .minibatchkmeans import _rows_to_host

__all__ = ['LandmarkAgglomerative']

LINKAGES = ('single', 'complete', 'average', 'ward')


def landmark_metric(metric):
    """One of libdistance's vector metrics, or one of the three symmetric divergences of ``utils.divergence`` by name or
    as its ``*_array`` function (recognised by identity); any other callable, ``kl_divergence`` (not symmetric) and
    'rmsd' (the reference's mdtraj path) raise ValueError."""
    metric = metric.decode() if isinstance(metric, bytes) else metric
    names = ', '.join("'%s'" % s for s in libdistance.VECTOR_METRICS[:8] + tuple(divergence.SYMMETRIC_KINDS))
    if callable(metric):
        kind = divergence.ARRAY_FUNCTION_KINDS.get(metric)
        if kind is None:
            raise ValueError('a callable metric is not supported, except the sym_kl_divergence_array, js_divergence_array '
                             'and js_metric_array of msmbuilder_amd.utils.divergence: metric must be one of %s' % names)
        metric = kind
    if metric == 'kl_divergence':
        raise ValueError("metric 'kl_divergence' is not symmetric: use sym_kl_divergence, js_divergence or js_metric")
    if metric in divergence.SYMMETRIC_KINDS:
        return metric
    if metric == 'rmsd':
        raise ValueError("metric 'rmsd' needs mdtraj trajectories and is not supported")
    if metric not in libdistance.VECTOR_METRICS:
        raise ValueError('metric must be one of %s' % names)
    return metric


def linkage_method(linkage):
    if linkage not in LINKAGES:
        raise ValueError('Invalid method: {0}'.format(linkage))   # (fastcluster's message)
    return linkage


def pooling_rule(linkage, ward_predictor):
    """The pooling function's name (agglomerative.py:249-254): ``ward_predictor`` after a ward fit, else the linkage."""
    name = ward_predictor if linkage == 'ward' else linkage
    if name not in LINKAGES:
        raise ValueError("linkage {} is not supported".format(name))
    return name


def effective_n_landmarks(n_clusters, n_landmarks, max_landmarks):
    """agglomerative.py:178-180: ``max_landmarks`` replaces ``n_landmarks`` when there are more clusters than landmarks."""
    if max_landmarks is not None:
        if n_clusters > n_landmarks:
            return max_landmarks
    return n_landmarks


def landmark_indices(n, n_landmarks, landmark_strategy='stride', random_state=None):
    """The rows that become landmarks (agglomerative.py:201-206); ``random`` may draw a row twice."""
    if landmark_strategy == 'random':
        return check_random_state(random_state).randint(n, size=n_landmarks)
    return np.arange(n)[::(n // n_landmarks)][:n_landmarks]


def permute_by_cluster(labels, n_clusters):
    """(perm, offsets): the landmarks in stable order of their label, cluster c's at offsets[c] .. offsets[c+1]-1."""
    labels = np.asarray(labels, dtype=np.int64)
    perm = np.argsort(labels, kind='stable')
    counts = np.bincount(labels, minlength=n_clusters)[:n_clusters] if len(labels) else np.zeros(n_clusters, np.int64)
    return perm, np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def linkage(dmat, n, method):
    """``msm_linkage``: the (n-1) x 4 linkage matrix (scipy's convention) of a condensed float64 matrix on the host or,
    as a torch CUDA tensor, on the device."""
    ad = Arr(dmat, np.float64)
    Z = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
    check(_lib.lib().msm_linkage(ad.vp, int(n), method.encode(), Z.ctypes.data, ad.on_device))
    return Z


def linkage_fit(ax, metric, method, X_indices=None):
    """``msm_linkage_fit_*`` on the rows (or the indexed rows) of ``ax``: the linkage matrix; the condensed matrix stays
    in the library for :func:`within_cluster`."""
    kind = "f64" if ax.dtype == np.float64 else "f32"
    idx, n = None, ax.shape[0]
    if X_indices is not None and not ax.on_device:
        ax = Arr(np.ascontiguousarray(ax.keep[np.asarray(X_indices, dtype=np.int64)]))   # only the landmarks travel
        n = ax.shape[0]
    elif X_indices is not None:
        import torch
        idx = Arr(torch.as_tensor(np.ascontiguousarray(X_indices, dtype=np.int64), device=ax.keep.device), np.int64)
        n = idx.shape[0]
    Z = np.zeros((max(n - 1, 0), 4), dtype=np.float64)
    check(getattr(_lib.lib(), "msm_linkage_fit_" + kind)(
        ax.vp, ax.shape[0], ax.shape[1], metric.encode(), idx.vp if idx is not None else None, n, method.encode(),
        Z.ctypes.data, ax.on_device))
    return Z


def within_cluster(dmat, n, labels, n_clusters):
    """``msm_landmark_within``: per cluster the sum of d^2 over its pairs.  ``dmat`` None: the matrix of the last
    :func:`linkage_fit`."""
    labels = np.ascontiguousarray(labels, dtype=np.int64)
    out = np.zeros(n_clusters, dtype=np.float64)
    ad = Arr(dmat, np.float64) if dmat is not None else None
    check(_lib.lib().msm_landmark_within(ad.vp if ad is not None else None, int(n), labels.ctypes.data, int(n_clusters),
                                         out.ctypes.data, ad.on_device if ad is not None else 0))
    return out


def pooled_predict_dmat(D, offsets, intra, pooling, want_pooled=False):
    """``msm_landmark_predict_dmat``: (labels, winning pooled values or None, negative flag) from an n x L float64 distance
    matrix whose columns are the landmarks permuted by cluster.  ``D`` is a numpy array or a torch CUDA tensor; rows may
    be strided (a view of a wider matrix), anything else is copied."""
    if len(D.shape) != 2:
        raise ValueError('D must be 2-dimensional')
    on_device = int(_lib.is_device_array(D))
    if on_device:
        import torch
        D = D.to(torch.float64)
        if D.stride(1) != 1 or D.stride(0) < D.shape[1]:
            D = D.contiguous()
        ld, ptr = D.stride(0), D.data_ptr()
        ref = Arr(D.new_empty(1))   # (selects the device and the stream)
    else:
        D = np.asarray(D, dtype=np.float64)
        if D.strides[1] != 8 or D.strides[0] % 8 or D.strides[0] < 8 * D.shape[1]:
            D = np.ascontiguousarray(D)
        ld, ptr = D.strides[0] // 8, D.ctypes.data
        ref = Arr(np.empty(1))
    n, L = D.shape
    ld = max(int(ld), L)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    K = len(offsets) - 1
    intra = None if intra is None else np.ascontiguousarray(intra, dtype=np.float64)
    if intra is not None and len(intra) != K:
        raise ValueError('intra must have one entry per cluster')
    labels = _lib.empty_like_placement(ref, (n,), np.int64)
    pooled = _lib.empty_like_placement(ref, (n,), np.float64) if want_pooled else None
    neg = C.c_int(0)
    al = Arr(labels, np.int64) if n else None
    ap = Arr(pooled, np.float64) if (want_pooled and n) else None
    check(_lib.lib().msm_landmark_predict_dmat(
        C.c_void_p(ptr) if n else None, n, L, ld, offsets.ctypes.data, K, intra.ctypes.data if intra is not None else None,
        pooling.encode(), al.vp if al is not None else None, ap.vp if ap is not None else None, C.byref(neg), on_device))
    return labels, pooled, bool(neg.value)


def pooled_predict_condensed(dmat, n, perm, offsets, intra, pooling, want_pooled=False):
    """``msm_landmark_predict_condensed``: every one of the n rows pooled against all of them from their own condensed
    float64 matrix (numpy, or a torch CUDA tensor as :func:`msmbuilder_amd.utils.divergence.divergence_pdist` leaves it);
    ``perm`` lists the rows by cluster.  (labels, winning pooled values or None, negative flag), placed like ``dmat``."""
    ad = Arr(dmat, np.float64)
    if ad.shape != (n * (n - 1) // 2,):
        raise ValueError('dmat must be the condensed matrix of %d rows' % n)
    perm = np.ascontiguousarray(perm, dtype=np.int64)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    K = len(offsets) - 1
    if perm.shape != (n,):
        raise ValueError('perm must have one entry per row')
    intra = None if intra is None else np.ascontiguousarray(intra, dtype=np.float64)
    if intra is not None and len(intra) != K:
        raise ValueError('intra must have one entry per cluster')
    labels = _lib.empty_like_placement(ad, (n,), np.int64)
    pooled = _lib.empty_like_placement(ad, (n,), np.float64) if want_pooled else None
    neg = C.c_int(0)
    al = Arr(labels, np.int64)
    ap = Arr(pooled, np.float64) if want_pooled else None
    check(_lib.lib().msm_landmark_predict_condensed(
        ad.vp, n, perm.ctypes.data, offsets.ctypes.data, K, intra.ctypes.data if intra is not None else None, pooling.encode(),
        al.vp, ap.vp if ap is not None else None, C.byref(neg), ad.on_device))
    return labels, pooled, bool(neg.value)


def pooled_predict(X, landmarks, offsets, intra, metric, pooling, want_pooled=False):
    """``msm_landmark_predict_*``: (labels, winning pooled values or None, negative flag).  ``landmarks`` are already
    permuted by cluster; labels and values live where X lives."""
    ax = X if isinstance(X, Arr) else Arr(X)
    kind = "f64" if ax.dtype == np.float64 else "f32"
    lm = np.ascontiguousarray(landmarks, dtype=ax.dtype)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    K = len(offsets) - 1
    intra = None if intra is None else np.ascontiguousarray(intra, dtype=np.float64)
    if intra is not None and len(intra) != K:
        raise ValueError('intra must have one entry per cluster')
    if lm.ndim != 2 or lm.shape[1] != ax.shape[1]:
        raise ValueError('X and the landmarks must have the same number of columns')
    n = ax.shape[0]
    labels = _lib.empty_like_placement(ax, (n,), np.int64)
    pooled = _lib.empty_like_placement(ax, (n,), np.float64) if want_pooled else None
    neg = C.c_int(0)
    al = Arr(labels, np.int64) if n else None
    ap = Arr(pooled, np.float64) if (want_pooled and n) else None
    check(getattr(_lib.lib(), "msm_landmark_predict_" + kind)(
        ax.vp if n else None, n, ax.shape[1], lm.ctypes.data, lm.shape[0], offsets.ctypes.data, K,
        intra.ctypes.data if intra is not None else None, metric.encode(), pooling.encode(),
        al.vp if al is not None else None, ap.vp if ap is not None else None, C.byref(neg), ax.on_device))
    return labels, pooled, bool(neg.value)


class _LandmarkAgglomerative(ClusterMixin, TransformerMixin):
    """Landmark-based agglomerative hierarchical clustering of ONE array (the sequence-list estimator is
    :class:`LandmarkAgglomerative`).

    A scalable form of hierarchical clustering that never needs the distances between all pairs of data points:
    ``n_landmarks`` rows are picked, only those are clustered, and every other point gets the label of the cluster
    whose landmarks are nearest to it in the sense of the linkage.

    Parameters
    ----------
    n_clusters : int
        The number of clusters to find.
    n_landmarks : int, optional
        The number of landmarks, picked by ``landmark_strategy``.  ``None`` makes every row a landmark (O(N^2) device
        memory).
    linkage : {'single', 'complete', 'average', 'ward'}, default='average'
        The distance between two sets of observations that the merging minimises: the mean, the largest or the smallest
        distance between their members, or Ward's variance criterion.  ``predict`` pools a point's distances to each
        cluster's landmarks with the same rule (``ward_predictor`` after a ward fit) and picks the lowest.
    metric : str, default="euclidean"
        One of libdistance's vector metrics: euclidean, sqeuclidean, cityblock, chebyshev, canberra, braycurtis,
        hamming, jaccard; or one of the symmetric divergences between non-negative rows, 'js_metric', 'js_divergence',
        'sym_kl_divergence', by name or as the ``js_metric_array``, ``js_divergence_array``, ``sym_kl_divergence_array``
        function of ``msmbuilder_amd.utils.divergence``.  (Any other callable, ``kl_divergence`` and "rmsd" are out of
        scope: ``ValueError``.)
    landmark_strategy : {'stride', 'random'}, default='stride'
        "stride" takes every (n // n_landmarks)-th row, "random" draws rows uniformly with replacement.
    random_state : integer or numpy.RandomState, optional
        The generator of the random landmarks.
    max_landmarks : int, optional
        When given and ``n_clusters > n_landmarks``, it replaces ``n_landmarks`` (for hyperparameter searches).
    ward_predictor : {'single', 'complete', 'average', 'ward'}, default='ward'
        The pooling rule of ``predict`` after a fit with ward linkage.

    Rows are numpy arrays or torch CUDA tensors; float32 and float64 rows are used as given, any other dtype is cast
    to float64, in ``fit`` and in ``predict`` alike; after that, the rows given to ``predict`` must have the landmarks'
    type (``TypeError``, as from the reference's ``cdist``).  A NaN or infinite distance between landmarks raises
    ``ValueError``.

    The linkage depends on all pairs of landmarks, so there is no row-sharded form: a fit inside an initialised
    ``torch.distributed`` clusters exactly the rows the calling process was given, on its own GPU, with no collective.

    Attributes
    ----------
    landmark_labels_ : array, [n_landmarks]
    landmarks_ : (n_landmarks, n_features) host array of X's dtype
    cluster_centers_ : (n_clusters, n_features), the mean of each cluster's landmarks
    cardinality_ : array, landmarks per cluster (``np.bincount(landmark_labels_)``)
    squared_distances_within_cluster_ : (n_clusters,) float64, per cluster the sum of squared distances over its pairs
    """

    def __init__(self, n_clusters, n_landmarks=None, linkage='average', metric='euclidean', landmark_strategy='stride',
                 random_state=None, max_landmarks=None, ward_predictor='ward'):
        self.n_clusters = n_clusters
        self.n_landmarks = n_landmarks
        self.metric = metric
        self.landmark_strategy = landmark_strategy
        self.random_state = random_state
        self.linkage = linkage
        self.max_landmarks = max_landmarks
        self.ward_predictor = ward_predictor

        self.landmark_labels_ = None
        self.landmarks_ = None
        self.cluster_centers_ = None

    def fit(self, X, y=None):
        from scipy.cluster.hierarchy import fcluster
        metric = landmark_metric(self.metric)
        method = linkage_method(self.linkage)
        self.n_landmarks = effective_n_landmarks(self.n_clusters, self.n_landmarks, self.max_landmarks)
        ax = working_array(X)
        n = ax.shape[0]
        land_indices = None
        if self.n_landmarks is not None:
            land_indices = landmark_indices(n, self.n_landmarks, self.landmark_strategy, self.random_state)
        n_land = n if land_indices is None else len(land_indices)
        tree = linkage_fit(ax, metric, method, land_indices)
        self.landmark_labels_ = fcluster(tree, criterion='maxclust', t=self.n_clusters) - 1
        self.cardinality_ = np.bincount(self.landmark_labels_)
        self.squared_distances_within_cluster_ = within_cluster(None, n_land, self.landmark_labels_, self.n_clusters)
        # landmarks_ is a HOST array like the other clusterers' centres: predict needs it there
        if land_indices is None:
            self.landmarks_ = ax.keep.detach().cpu().numpy() if ax.on_device else ax.keep
        else:
            self.landmarks_ = _rows_to_host(ax, land_indices)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)   # (a cluster id without a landmark: a row of NaN, as in the reference)
            self.cluster_centers_ = np.array([list(np.mean(self.landmarks_[self.landmark_labels_ == i], axis=0))
                                              for i in range(self.n_clusters)])
        return self

    def predict(self, X):
        """The cluster whose landmarks, pooled by the linkage rule, are nearest to each sample (a host int array)."""
        pooling = pooling_rule(self.linkage, self.ward_predictor)
        metric = landmark_metric(self.metric)
        ax = working_array(X)
        if ax.dtype != self.landmarks_.dtype:
            raise TypeError('XA and XB must be identically float32 or float64')
        perm, offsets = permute_by_cluster(self.landmark_labels_, self.n_clusters)
        labels, _, negative = pooled_predict(ax, self.landmarks_[perm], offsets,
                                             self.squared_distances_within_cluster_ if pooling == 'ward' else None,
                                             metric, pooling)
        if negative:
            warnings.warn("Distance shouldn't be negative.")
        for i in np.flatnonzero(np.diff(offsets) == 0):
            print("No data points were assigned to cluster {}".format(i))
        labels = labels.cpu().numpy() if ax.on_device else labels
        return labels.astype(int, copy=False)

    def fit_predict(self, X, y=None):
        self.fit(X)
        return self.predict(X)


class LandmarkAgglomerative(MultiSequenceClusterMixin, _LandmarkAgglomerative, BaseEstimator):
    __doc__ = _LandmarkAgglomerative.__doc__
