"""Minimum variance cluster analysis on MI355X: drop-in for ``msmbuilder.lumping.MVCA`` (reference:
msmbuilder/lumping/mvca.py; Husic, McKiernan, Wayment-Steele, Sultan and Pande, J. Chem. Theory Comput. 14, 1071 (2018)).

MVCA lumps the microstates of a Markov state model into macrostates by Ward-linking the rows of the transition matrix
under the Jensen-Shannon metric and then giving every row the label of the cluster whose members are nearest to it in
Ward's pooled sense.  The reference evaluates the metric in nested Python loops, n^2 * n logarithms for the linkage and
as many again for the labels.  Here the transition matrix is uploaded once and stays on the device: the divergence tile
kernel (csrc/divergence.hip) writes the condensed matrix in device memory, the linkage runs on it there, and the labels
are pooled on the device -- with landmarks from the divergences of every row to the landmarks, computed in blocks of rows
(``msm_landmark_predict_*``); without, from the condensed matrix itself (``msm_landmark_predict_condensed``), so that no
divergence is computed twice.

``n_landmarks < n_states`` works.  (The reference raises ``IndexError`` there: its ``cdist`` hands a callable metric the
index of a row of the data, which it then looks up among the landmarks.)

The MSM attributes of an ``MVCA`` object describe the MICROSTATE model, as in the reference; fit a new
``MarkovStateModel`` on ``transform``'s output for the macrostate model.
"""
import numpy as np

from ..cluster import agglomerative as A
from ..cluster.agglomerative import LandmarkAgglomerative
from ..msm import MarkovStateModel
from ..utils import divergence
from ..utils.divergence import js_metric_array

__all__ = ['MVCA']


def _device_rows(transmat):
    """The transition matrix as a float64 torch CUDA tensor (one upload), or the host array where torch is missing."""
    T = np.ascontiguousarray(transmat, dtype=np.float64)
    try:
        import torch
    except ImportError:
        return T
    from .. import _lib
    _lib.ensure_device()
    return torch.as_tensor(T, device='cuda')


class MVCA(MarkovStateModel):
    """Minimum variance cluster analysis (MVCA) for coarse-graining (lumping) microstates into macrostates.

    Parameters
    ----------
    n_macrostates : int or None
        The number of macrostates in the lumped model.  ``None`` is accepted by ``from_msm`` only (for its linkage
        outputs); ``fit`` raises ``RuntimeError`` after fitting the MSM.
    metric : {'js_metric', 'js_divergence', 'sym_kl_divergence'} or the matching ``*_array`` function of
        ``msmbuilder_amd.utils.divergence``, default=js_metric_array
        The distance between two rows of the transition matrix.  Any other callable and ``kl_divergence`` (not
        symmetric) raise ``ValueError``.
    fit_only : bool, default=False
        True: ``microstate_mapping_`` is the landmarks' labels from the linkage.  False: the predicted label of every row.
        In general these differ.
    n_landmarks : int, optional
        Link only this many rows, picked by ``landmark_strategy``, and label the rest by their distances to them.
        ``None`` makes every row a landmark.
    landmark_strategy : {'stride', 'random'}, default='stride'
    random_state : integer or numpy.RandomState, optional
        The generator of the random landmarks.
    **kwargs
        Passed to :class:`MarkovStateModel`.  (``get_params`` and ``clone`` keep them, which the reference's do not.)

    Attributes
    ----------
    microstate_mapping_ : int array, [n_states_]
    """

    def __init__(self, n_macrostates, metric=js_metric_array, fit_only=False, n_landmarks=None, landmark_strategy='stride',
                 random_state=None, **kwargs):
        self.n_macrostates = n_macrostates
        self.metric = metric
        self.fit_only = fit_only
        self.n_landmarks = n_landmarks
        self.landmark_strategy = landmark_strategy
        self.random_state = random_state
        super(MVCA, self).__init__(**kwargs)

    @classmethod
    def _get_param_names(cls):
        own = ['n_macrostates', 'metric', 'fit_only', 'n_landmarks', 'landmark_strategy', 'random_state']
        return sorted(own + MarkovStateModel._get_param_names())

    def fit(self, sequences, y=None):
        """Fit the microstate MSM on sequences of cluster assignments, then lump it."""
        super(MVCA, self).fit(sequences, y=y)
        if self.n_macrostates is None:
            raise RuntimeError('n_macrostates must not be None to fit')
        self._do_lumping()
        return self

    def _do_lumping(self, keep_linkage=False):
        kind = A.landmark_metric(self.metric)
        if self.n_landmarks is None and kind in divergence.KINDS:
            self._lump_every_row(kind, keep_linkage)
            return
        model = LandmarkAgglomerative(linkage='ward', n_clusters=self.n_macrostates, metric=self.metric,
                                      n_landmarks=self.n_landmarks, landmark_strategy=self.landmark_strategy,
                                      random_state=self.random_state)
        rows = _device_rows(self.transmat_)
        model.fit([rows])
        if self.fit_only:
            self.microstate_mapping_ = model.landmark_labels_
        else:
            self.microstate_mapping_ = np.asarray(model.transform([rows])[0])

    def _lump_every_row(self, kind, keep_linkage):
        """Every row is a landmark: the condensed matrix is computed once and stays on the device for the linkage, the
        within-cluster sums and the labels (its square form, expanded in blocks, is what ``predict``'s cdist of the rows
        against themselves would compute a second time: d(i, j) = d(j, i) bit for bit and d(i, i) = 0).  The same labels
        as the LandmarkAgglomerative route, bit for bit."""
        import warnings
        from scipy.cluster.hierarchy import fcluster
        rows = _device_rows(self.transmat_)
        n, K = int(rows.shape[0]), self.n_macrostates
        dists = divergence.divergence_pdist(rows, kind)
        tree = A.linkage(dists, n, 'ward')
        labels = fcluster(tree, criterion='maxclust', t=K) - 1
        if keep_linkage:
            self._linkage_cache = (kind, dists, tree)
        if self.fit_only:
            self.microstate_mapping_ = labels
            return
        within = A.within_cluster(dists, n, labels, K)
        perm, offsets = A.permute_by_cluster(labels, K)
        mapping, _, negative = A.pooled_predict_condensed(dists, n, perm, offsets, within, 'ward')
        if negative:
            warnings.warn("Distance shouldn't be negative.")
        for i in np.flatnonzero(np.diff(offsets) == 0):
            print("No data points were assigned to cluster {}".format(i))
        mapping = mapping if isinstance(mapping, np.ndarray) else mapping.cpu().numpy()
        self.microstate_mapping_ = mapping.astype(int, copy=False)

    def partial_transform(self, sequence, mode='clip'):
        """One sequence of microstate labels to macrostate labels: ``'clip'`` -> the list of mapped runs, ``'fill'`` ->
        one array with NaN where a label is not in the model."""
        if self.n_macrostates is None:
            raise RuntimeError('n_macrostates must not be None to transform')
        if mode not in ('clip', 'fill'):
            raise ValueError('mode must be one of ["clip", "fill"]: %s' % mode)
        trimmed = super(MVCA, self).partial_transform(sequence, mode)
        if mode == 'clip':
            return [self.microstate_mapping_[seq] for seq in trimmed]
        trimmed = np.asarray(trimmed, dtype=float)
        known = np.isfinite(trimmed)
        if np.all(known):
            return np.asarray(self.microstate_mapping_[trimmed.astype(int)])
        out = np.full(len(trimmed), np.nan)
        out[known] = self.microstate_mapping_[trimmed[known].astype(int)]
        return out

    @classmethod
    def from_msm(cls, msm, n_macrostates, metric=js_metric_array, n_landmarks=None, landmark_strategy='stride',
                 random_state=None, get_linkage=False, fit_only=False):
        """A lumped model from a fitted MSM.

        With ``get_linkage`` the result also carries ``pairwise_dists`` (the condensed matrix of ALL n_states rows, a
        host array), ``linkage`` (the ward linkage of it, scipy's layout) and ``elbow_data = linkage[:, 2][::-1]``, the
        merge heights indexed by ``n_macrostates - 1``; all three are ``None`` otherwise."""
        params = msm.get_params()
        for own in ('n_macrostates', 'metric', 'fit_only', 'n_landmarks', 'landmark_strategy', 'random_state'):
            params.pop(own, None)   # (msm may itself be an MVCA)
        lumper = cls(n_macrostates, metric=metric, fit_only=fit_only, n_landmarks=n_landmarks,
                     landmark_strategy=landmark_strategy, random_state=random_state, **params)
        lumper.transmat_ = msm.transmat_
        lumper.populations_ = msm.populations_
        lumper.mapping_ = msm.mapping_
        lumper.countsmat_ = msm.countsmat_
        lumper.n_states_ = msm.n_states_
        if n_macrostates is not None:
            lumper._do_lumping(keep_linkage=get_linkage)
        if get_linkage:
            kind = A.landmark_metric(metric)
            if kind not in divergence.KINDS:
                raise ValueError('get_linkage needs one of the divergence metrics')
            cached = lumper.__dict__.pop('_linkage_cache', None)   # (the lumping of every row has linked this matrix already)
            if cached is not None and cached[0] == kind:
                dists, lumper.linkage = cached[1], cached[2]
            else:
                dists = divergence.divergence_pdist(_device_rows(msm.transmat_), kind)
                lumper.linkage = A.linkage(dists, len(msm.transmat_), 'ward')   # on the matrix where the kernel wrote it
            lumper.pairwise_dists = dists if isinstance(dists, np.ndarray) else dists.cpu().numpy()
            lumper.elbow_data = lumper.linkage[:, 2][::-1]
        else:
            lumper.pairwise_dists = None
            lumper.linkage = None
            lumper.elbow_data = None
        return lumper
