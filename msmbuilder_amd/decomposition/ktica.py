"""Kernel tICA on MI355X: drop-in for ``msmbuilder.decomposition.KernelTICA``
(msmbuilder/decomposition/ktica.py:22-211): tICA on the Nystroem features of the frames.

The reference maps every frame on the host (scikit-learn's ``pairwise_kernels`` and a dot product, an N x L host array) and
hands the result to tICA.  Here ``fit`` / ``partial_fit`` produce the features on the device (``msm_kernel_map_*``) and hand
them to ``tICA``'s device path -- nothing N-sized goes to the host --, and ``transform`` never forms the features at all:

    (K(X, landmarks) . M^T - mu) . V^T  =  K(X, landmarks) . (M^T V^T)  -  mu V^T

with M = ``normalization_``, mu the tICA mean and V the k x L projection matrix (kinetic mapping folded in), is the same
fused kernel with an L x k right-hand matrix.
"""
from __future__ import print_function, division, absolute_import

import numpy as np

from .._lib import is_device_array
from ..utils import check_iter_of_sequences
from .kernel_approximation import LandmarkNystroem, kernel_map_sequences
from .tica import tICA

__all__ = ['KernelTICA']

_FEATURE_BYTES = 1 << 30   # the features of at most this many bytes are held on the device at a time


class KernelTICA(tICA):
    """Time-structure Independent Component Analysis (tICA) using the kernel trick, through a landmark Nystroem
    approximation of the kernel's feature map.

    Parameters
    ----------
    n_components, lag_time, shrinkage, kinetic_mapping : as ``tICA``
    kernel : 'rbf' (default), 'linear', 'poly', 'sigmoid', 'laplacian' or 'cosine'
        A callable is refused with a ValueError (there is no host path).
    degree, gamma, coef0 : kernel parameters (defaults 3, None -> 1 / n_features, 1.)
    stride : int
        When no landmarks are given, every ``stride``-th pair of frames (x_t, x_{t + lag_time}) of the training data
        becomes a landmark.
    landmarks : ndarray (n_landmarks, n_features) or None
    random_state, kernel_params : as in the reference (``kernel_params`` is the keyword dictionary of the
        ``LandmarkNystroem`` map; by default it is built from the arguments above).

    Attributes are ``tICA``'s, over the ``n_landmarks`` Nystroem features.
    """

    def __init__(self, n_components=None, lag_time=1, shrinkage=None,
                 kinetic_mapping=False, kernel='rbf', degree=3, gamma=None,
                 coef0=1., stride=1, landmarks=None, random_state=None,
                 kernel_params=None):
        self.kernel = kernel
        self.degree = degree
        self.gamma = gamma
        self.coef0 = coef0
        self.stride = stride
        self.landmarks = landmarks
        self.random_state = random_state
        self.kernel_params = kernel_params
        if kernel_params is None:
            self.kernel_params = {
                                  'kernel': self.kernel,
                                  'degree': self.degree,
                                  'gamma': self.gamma,
                                  'coef0': self.coef0,
                                  'random_state': self.random_state
                                  }
        self._nystroem = None
        super(KernelTICA, self).__init__(n_components=n_components,
                                         lag_time=lag_time,
                                         shrinkage=shrinkage,
                                         kinetic_mapping=kinetic_mapping)

    def _gen_landmarks(self, sequences):
        """The frames of every ``stride``-th lagged pair, as one host array (ktica.py:136-144); device trajectories are
        indexed on the device and only the chosen frames are copied."""
        X = []
        for seq in sequences:
            u = np.arange(seq.shape[0])[self.lag_time::self.stride]
            v = np.arange(seq.shape[0])[::self.stride][:u.shape[0]]
            idx = np.unique((u, v))
            if is_device_array(seq):
                import torch
                X.append(seq.index_select(0, torch.as_tensor(idx, device=seq.device)).cpu().numpy())
            else:
                X.append(np.asarray(seq)[idx])
        return np.concatenate(X, axis=0)

    def _ensure_map(self, sequences):
        if self.landmarks is None:
            self.landmarks = self._gen_landmarks(sequences)
        if self._nystroem is None:
            self._nystroem = LandmarkNystroem(landmarks=self.landmarks, **self.kernel_params)
            self._nystroem.fit(sequences)

    def _to_device(self, X):
        if is_device_array(X):
            return X
        import torch
        from .. import _lib
        X = np.ascontiguousarray(X, dtype=None if np.asarray(X).dtype in (np.float32, np.float64) else np.float64)
        _lib.ensure_device()
        return torch.from_numpy(X).to(torch.device("cuda", int(_lib._initialized_device or 0)))

    def _row_bytes(self, X):
        """Device bytes one frame costs while it is accumulated: its F values (uploaded, for a host trajectory) and its L
        features."""
        comps = self._nystroem.components_
        name = str(X.dtype)
        f32 = name.endswith("float32") and comps.dtype == np.float32   # (the dtype rule of kernel_map)
        row = 4 if name.endswith("float32") else 8                     # (anything but float32 / float64 is widened to float64)
        return int(X.shape[1]) * row + int(comps.shape[0]) * (4 if f32 else 8)

    def _accumulate_group(self, group):
        """Whole trajectories that together fit the budget: uploaded where they are host arrays, mapped as ONE list (one
        launch, ``kernel_map_sequences``) and accumulated as one list (``tICA._fit_many``: one launch over the features,
        which lie back to back)."""
        if group:
            feats = self._nystroem.transform([self._to_device(X) for X in group])
            self._fit_many(feats)

    def _accumulate_pieces(self, X):
        """A trajectory beyond the budget: pieces that overlap by ``lag_time`` frames (``partial_fit_segments``), so that no
        lagged pair is lost at a cut; a host trajectory is uploaded piece by piece."""
        n, lag = int(X.shape[0]), int(self.lag_time)
        rows_max = max(2 * lag + 2, _FEATURE_BYTES // self._row_bytes(X))
        step = rows_max - lag
        for ob in range(0, n, step):
            oe = min(ob + step, n)
            end = min(oe + lag, n)
            feats = self._nystroem.partial_transform(self._to_device(X[ob:end]))
            self.partial_fit_segments([(feats, n, ob, ob, oe)])
            del feats

    def _accumulate(self, sequences):
        """Features on the device, into tICA's accumulators, at most ``_FEATURE_BYTES`` of rows and features at a time:
        consecutive trajectories of one dtype and placement are grouped up to that budget, a longer one goes in pieces."""
        group, group_bytes, key = [], 0, None
        for X in sequences:
            nbytes = int(X.shape[0]) * self._row_bytes(X)
            k = (is_device_array(X), str(X.dtype))
            if group and (k != key or group_bytes + nbytes > _FEATURE_BYTES):
                self._accumulate_group(group)
                group, group_bytes = [], 0
            key = k
            if nbytes > _FEATURE_BYTES and int(X.shape[0]) > 2 * int(self.lag_time) + 2:
                self._accumulate_pieces(X)
                continue
            group.append(X)
            group_bytes += nbytes
        self._accumulate_group(group)

    def fit(self, sequences, y=None):
        if not isinstance(sequences, (list, tuple)):
            sequences = list(sequences)
        check_iter_of_sequences(sequences)
        if self.landmarks is None:
            self.landmarks = self._gen_landmarks(sequences)
        self._nystroem = LandmarkNystroem(landmarks=self.landmarks, **self.kernel_params)
        self._nystroem.fit(sequences)
        self._initialized = False
        self.n_sequences_ = 0
        self._accumulate(sequences)
        if not self.n_sequences_:
            raise ValueError('All sequences were shorter than '
                             'the lag time, %d' % self.lag_time)
        return self

    def partial_fit(self, X):
        self._ensure_map([X])
        self._accumulate([X])
        return self

    def _folded(self):
        """(B, c) of the folded transform: B = M^T V^T (L x k), c = mu V^T, in float64 on the host."""
        mean, comps = self._projection()
        B = np.ascontiguousarray(np.dot(self._nystroem.normalization_.T, comps.T))
        return B, np.ascontiguousarray(np.dot(mean, comps.T))

    def transform(self, sequences):
        """One (n_i, n_components) float64 array per trajectory, on the device when the input is: the kernel map with the
        projection folded into its right-hand matrix, one call per list."""
        B, c = self._folded()
        ny = self._nystroem
        return kernel_map_sequences(sequences, ny.components_, B, c, out_f64=True, **ny._kernel_kw())

    def partial_transform(self, features):
        return self.transform([features])[0]

    def fit_transform(self, sequences, y=None):
        self.fit(sequences)
        return self.transform(sequences)

    def score(self, sequences, y=None):
        """Generalized matrix Rayleigh quotient of this model's slow directions on other data (ktica.py:146-186): a second
        model with the same landmarks and kernel is fitted to ``sequences`` and its moments are read in this model's
        eigenvector basis."""
        assert self._initialized
        V = self.eigenvectors_

        m2 = self.__class__(shrinkage=self.shrinkage, n_components=self.n_components, lag_time=self.lag_time,
                            landmarks=self.landmarks, kernel_params=self.kernel_params)
        m2.fit(sequences)
        numerator = V.T.dot(m2.offset_correlation_).dot(V)
        denominator = V.T.dot(m2.covariance_).dot(V)

        try:
            trace = np.trace(numerator.dot(np.linalg.inv(denominator)))
        except np.linalg.LinAlgError:
            trace = np.nan
        return trace
