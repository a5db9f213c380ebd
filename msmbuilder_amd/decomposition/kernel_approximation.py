"""Nystroem kernel feature maps on MI355X: drop-ins for ``msmbuilder.decomposition.Nystroem`` and ``LandmarkNystroem``
(msmbuilder/decomposition/kernel_approximation.py:20-105, which are scikit-learn's ``Nystroem`` behind the
multi-sequence mixin).

What the reference does per frame -- ``pairwise_kernels(X, components_)`` followed by ``np.dot(embedded,
normalization_.T)``, both in scikit-learn on the host -- is one fused launch of libmsmhip (``msm_kernel_map_*``,
msmbuilder_amd/csrc/nystroem.hip): the n x L kernel values stay in LDS between the two products.  What it does once per
fit at L^3 cost -- the SVD of the L x L basis kernel and ``normalization_ = U / sqrt(S) . V`` -- stays scipy on the host,
so that it shares the reference's definition; the basis kernel itself comes from the same device kernel (B = I).

Kernels: 'linear', 'poly', 'sigmoid', 'cosine', 'rbf', 'laplacian'.  A callable or 'precomputed' kernel is refused with a
ValueError: there is no host path in this package.  Inputs may be numpy arrays (staged over PCIe in groups) or 2-D torch
CUDA tensors (read in place; the features come back as CUDA tensors that ``tICA.fit`` reads in place).
"""
from __future__ import print_function, division, absolute_import

import ctypes as C
import warnings

import numpy as np
import scipy.linalg
from sklearn.base import TransformerMixin
from sklearn.utils import check_random_state

from .. import _lib
from .._lib import check, is_device_array
from ..base import BaseEstimator
from ..utils import check_iter_of_sequences

__all__ = ['Nystroem', 'LandmarkNystroem', 'kernel_map', 'kernel_map_plan', 'resolve_kernel', 'KERNEL_IDS']

KERNEL_IDS = {'linear': 0, 'poly': 1, 'sigmoid': 2, 'cosine': 3, 'rbf': 4, 'laplacian': 5}   # enum msm_kernel
_HOST_GROUP_BYTES = 256 << 20   # small host trajectories are joined into groups of about this size, one call each


def resolve_kernel(kernel, gamma, coef0, degree, n_features):
    """(kernel id, gamma, coef0, degree) as floats, with scikit-learn's defaults filled in: gamma None -> 1 / n_features,
    coef0 None -> 1, degree None -> 3 (sklearn.metrics.pairwise: polynomial_kernel, sigmoid_kernel, rbf_kernel,
    laplacian_kernel)."""
    if callable(kernel) or kernel == 'precomputed':
        raise ValueError("kernel %r is not supported: msmbuilder_amd evaluates kernels on the device and has no host path "
                         "(use one of %s)" % (kernel, sorted(KERNEL_IDS)))
    if kernel not in KERNEL_IDS:
        raise ValueError("Unknown kernel %r (valid kernels: %s)" % (kernel, sorted(KERNEL_IDS)))
    return (KERNEL_IDS[kernel], 1.0 / n_features if gamma is None else float(gamma), 1.0 if coef0 is None else float(coef0),
            3.0 if degree is None else float(degree))


def kernel_map_plan(L, P, n_features, itemsize):
    """``msm_kernel_map_plan`` as a dict: route ('fused' / 'scratch'), rows per workgroup R, the tile sizes, the padded L,
    the block's pitch, its LDS bytes and the default rows of a scratch chunk."""
    out = (C.c_int64 * 9)()
    check(_lib.lib().msm_kernel_map_plan(int(L), int(P), int(n_features), int(itemsize), out))
    keys = ("fused", "R", "landmark_tile", "depth", "column_tile", "L_padded", "pitch", "lds_bytes", "chunk_rows")
    d = dict(zip(keys, [int(v) for v in out]))
    d["route"] = "fused" if d["fused"] else "scratch"
    return d


def _work_rows(X, landmarks):
    """Rows in the dtype the kernel reads: float32 when rows AND landmarks are float32, float64 otherwise (scikit-learn's
    check_pairwise_arrays rule).  Rows whose elements are unit-stride keep their row pitch; nothing is copied then."""
    lm32 = np.asarray(landmarks).dtype == np.float32
    if is_device_array(X):
        import torch
        want = torch.float32 if (X.dtype == torch.float32 and lm32) else torch.float64
        if X.dtype != want:
            X = X.to(want)
        if X.dim() != 2:
            raise ValueError("rows must be 2-dimensional")
        if X.shape[0] > 1 and (X.stride(1) != 1 or X.stride(0) < X.shape[1]) or X.shape[0] <= 1 and not X.is_contiguous():
            X = X.contiguous()
        return X, (X.stride(0) if X.shape[0] > 1 else X.shape[1])
    X = np.asarray(X)
    want = np.float32 if (X.dtype == np.float32 and lm32) else np.float64
    if X.dtype != want:
        X = X.astype(want)
    if X.ndim != 2:
        raise ValueError("rows must be 2-dimensional")
    item = X.itemsize
    if X.shape[0] > 1 and X.shape[1] > 0 and X.strides[1] == item and X.strides[0] % item == 0 and X.strides[0] >= X.shape[1] * item:
        return X, X.strides[0] // item
    X = np.ascontiguousarray(X)
    return X, X.shape[1]


def kernel_map(X, landmarks, B, c=None, kernel='rbf', gamma=None, coef0=None, degree=None, out_f64=False, scratch_rows=0):
    """``k(X, landmarks) . B - c`` for one 2-D array of rows (numpy, or a torch CUDA tensor: the result is then a CUDA
    tensor): (n, P) in the rows' dtype, or float64 with ``out_f64``."""
    landmarks = np.asarray(landmarks)
    X, ld = _work_rows(X, landmarks)
    n, F = int(X.shape[0]), int(X.shape[1])
    if landmarks.ndim != 2 or landmarks.shape[1] != F:
        raise ValueError("Incompatible dimension for X and Y matrices: X.shape[1] == %d while Y.shape[1] == %d"
                         % (F, landmarks.shape[1] if landmarks.ndim == 2 else -1))
    kid, gamma, coef0, degree = resolve_kernel(kernel, gamma, coef0, degree, F)
    on_device = is_device_array(X)
    f32 = str(X.dtype).endswith("float32")
    landmarks = np.ascontiguousarray(landmarks, dtype=np.float32 if f32 else np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    if B.ndim != 2 or B.shape[0] != landmarks.shape[0]:
        raise ValueError("B must have one row per landmark")
    L, P = int(B.shape[0]), int(B.shape[1])
    if L < 1 or P < 1:
        raise ValueError("the kernel map needs at least one landmark and one column of B, got B of shape %r" % (B.shape,))
    if c is not None:
        c = np.ascontiguousarray(c, dtype=np.float64)
        if c.shape != (P,):
            raise ValueError("c must have one entry per column of B")
    odt = np.float64 if (out_f64 or not f32) else np.float32
    if on_device:
        import torch
        _lib.ensure_device(X.device.index)
        _lib.set_stream(torch.cuda.current_stream(X.device).cuda_stream)
        out = torch.empty((n, P), dtype=torch.float64 if odt == np.float64 else torch.float32, device=X.device)
        xp, op = X.data_ptr(), out.data_ptr()
    else:
        _lib.ensure_device()
        out = np.empty((n, P), dtype=odt)
        xp, op = X.ctypes.data, out.ctypes.data
    if n == 0:
        return out
    fn = _lib.lib().msm_kernel_map_f32 if f32 else _lib.lib().msm_kernel_map_f64
    check(fn(C.c_void_p(xp), n, F, int(ld), landmarks.ctypes.data, L, B.ctypes.data, P, None if c is None else c.ctypes.data,
             kid, gamma, coef0, degree, C.c_void_p(op), int(bool(out_f64)), int(on_device), int(scratch_rows)))
    return out


def kernel_map_sequences(sequences, landmarks, B, c=None, **kw):
    """``kernel_map`` of every trajectory of a list, with ``tICA.transform``'s conventions: trajectories that lie back to
    back in one allocation are one launch over the joined view; separately allocated device tensors are joined on the
    device (F values per frame against the P written) and mapped in one launch; host arrays are joined into groups of about
    256 MiB, each of which the library stages through the device."""
    if not isinstance(sequences, (list, tuple)):
        sequences = list(sequences)
    check_iter_of_sequences(sequences)
    if not sequences:
        return []
    lens = [int(X.shape[0]) for X in sequences]
    joined = _lib.adjacent_view(sequences)
    if joined is not None:
        return _lib.cut_rows(kernel_map(joined, landmarks, B, c, **kw), lens)
    if len(sequences) > 1 and all(is_device_array(X) for X in sequences) \
            and len(set((X.dtype, X.device, X.shape[1]) for X in sequences)) == 1:
        import torch
        return _lib.cut_rows(kernel_map(torch.cat(list(sequences), dim=0), landmarks, B, c, **kw), lens)
    out, group, group_bytes = [], [], 0

    def flush():
        if len(group) == 1:
            out.append(kernel_map(group[0], landmarks, B, c, **kw))
        elif group:
            out.extend(_lib.cut_rows(kernel_map(np.concatenate(group, axis=0), landmarks, B, c, **kw), [g.shape[0] for g in group]))
        del group[:]

    for X in sequences:
        if is_device_array(X) or (group and (X.dtype != group[0].dtype or X.shape[1] != group[0].shape[1])):
            flush()
            group_bytes = 0
        if is_device_array(X):
            out.append(kernel_map(X, landmarks, B, c, **kw))
            continue
        X = np.asarray(X)
        group.append(X)
        group_bytes += X.nbytes
        if group_bytes >= _HOST_GROUP_BYTES:
            flush()
            group_bytes = 0
    flush()
    return out


def _gather_rows(sequences, indices):
    """Rows ``indices`` of the concatenated sequences as one host array; device sequences are indexed on the device and only
    the gathered rows cross to the host."""
    lens = np.array([int(X.shape[0]) for X in sequences], dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum(lens)))
    which = np.searchsorted(starts, indices, side='right') - 1
    rows = [None] * len(indices)
    for s in np.unique(which):
        sel = np.nonzero(which == s)[0]
        local = indices[sel] - starts[s]
        X = sequences[s]
        if is_device_array(X):
            import torch
            got = X.index_select(0, torch.as_tensor(local, device=X.device)).cpu().numpy()
        else:
            got = np.asarray(X)[local]
        for j, g in zip(sel, got):
            rows[j] = g
    return np.stack(rows, axis=0)


class Nystroem(BaseEstimator, TransformerMixin):
    """Approximate a kernel map using a random subset of the training frames as basis (scikit-learn's ``Nystroem`` over a
    list of trajectories, as in the reference).

    Parameters
    ----------
    kernel : 'rbf' (default), 'linear', 'poly', 'sigmoid', 'cosine' or 'laplacian'
    gamma, coef0, degree : float or None
        Kernel parameters; ``None`` leaves scikit-learn's defaults (1 / n_features, 1, 3).
    kernel_params : ignored for the named kernels (scikit-learn passes it to callables only)
    n_components : int
        How many frames form the basis (at most the number of frames).
    random_state : int, RandomState or None
        The basis is ``check_random_state(random_state).permutation(n_samples)[:n_components]`` over the concatenated
        trajectories -- scikit-learn's stream, so the same frames are picked.

    Attributes
    ----------
    components_ : (n_components, n_features) host array     the basis frames
    component_indices_ : (n_components,)                     their indices in the concatenated training set
    normalization_ : (n_components, n_components) float64    K(basis, basis)^(-1/2) by SVD, as the reference forms it
    """

    def __init__(self, kernel='rbf', gamma=None, coef0=None, degree=None, kernel_params=None, n_components=100,
                 random_state=None):
        self.kernel = kernel
        self.gamma = gamma
        self.coef0 = coef0
        self.degree = degree
        self.kernel_params = kernel_params
        self.n_components = n_components
        self.random_state = random_state

    def _kernel_kw(self):
        return dict(kernel=self.kernel, gamma=self.gamma, coef0=self.coef0, degree=self.degree)

    def _fit_basis(self, basis):
        basis = np.asarray(basis)
        if basis.dtype not in (np.float32, np.float64):
            basis = basis.astype(np.float64)
        basis = np.ascontiguousarray(basis)
        L = basis.shape[0]
        resolve_kernel(self.kernel, self.gamma, self.coef0, self.degree, basis.shape[1])   # refuse before any work
        basis_kernel = kernel_map(basis, basis, np.eye(L), None, out_f64=True, **self._kernel_kw())
        # sqrt of kernel matrix on basis vectors (kernel_approximation.py:97-99)
        U, S, V = scipy.linalg.svd(basis_kernel)
        S = np.maximum(S, 1e-12)
        self.normalization_ = np.dot(U / np.sqrt(S), V)
        self.components_ = basis
        return self

    def fit(self, sequences, y=None):
        if not isinstance(sequences, (list, tuple)):
            sequences = list(sequences)
        check_iter_of_sequences(sequences)
        rnd = check_random_state(self.random_state)
        n_samples = int(sum(int(X.shape[0]) for X in sequences))
        n_components = self.n_components
        if n_components > n_samples:
            n_components = n_samples
            warnings.warn("n_components > n_samples. This is not possible.\nn_components was set to n_samples, which results"
                          " in inefficient evaluation of the full kernel.")
        inds = rnd.permutation(n_samples)
        basis_inds = inds[:n_components]
        self._fit_basis(_gather_rows(sequences, basis_inds))
        self.component_indices_ = basis_inds
        return self

    def partial_fit(self, X):
        """The basis from ONE trajectory (the model is refitted, not updated: a Nystroem basis has no online form)."""
        return self.fit([X])

    def transform(self, sequences):
        """One (n_i, n_components) array of the rows' dtype per trajectory, on the device when the input is."""
        return kernel_map_sequences(sequences, self.components_, np.ascontiguousarray(self.normalization_.T), None,
                                    **self._kernel_kw())

    def partial_transform(self, sequence):
        return self.transform([sequence])[0]

    def fit_transform(self, sequences, y=None):
        self.fit(sequences)
        return self.transform(sequences)


class LandmarkNystroem(Nystroem):
    """Nystroem map over given landmark frames (kernel_approximation.py:24-105).

    ``landmarks`` : ndarray of shape (n_landmarks, n_features) -- the basis, used as given (``components_`` is the array,
    ``component_indices_`` is None); ``None`` -- a random basis of ``n_components`` frames, as ``Nystroem``.  Anything but an
    ndarray, an int or None raises the reference's ValueError.  AN EXTENSION, not the reference's behaviour: an ``int``, which
    passes the reference's type check and then fails inside scikit-learn's ``pairwise_kernels`` there, is read here as
    that many random components (``Nystroem`` with ``n_components = landmarks``).  The remaining parameters and the
    attributes are ``Nystroem``'s.
    """

    def __init__(self, landmarks=None, kernel='rbf', gamma=None, coef0=None, degree=None, kernel_params=None, n_components=100,
                 random_state=None):
        if (landmarks is not None and
                not isinstance(landmarks, (int, np.ndarray))):
            raise ValueError('landmarks should be an int, ndarray, or None.')
        self.landmarks = landmarks
        super(LandmarkNystroem, self).__init__(kernel=kernel, gamma=gamma, coef0=coef0, degree=degree,
                                               kernel_params=kernel_params, n_components=n_components,
                                               random_state=random_state)

    def fit(self, sequences, y=None):
        if isinstance(self.landmarks, np.ndarray):
            self._fit_basis(self.landmarks)
            self.component_indices_ = None
            return self
        if self.landmarks is not None:
            saved = self.n_components
            self.n_components = int(self.landmarks)
            try:
                return super(LandmarkNystroem, self).fit(sequences, y=y)
            finally:
                self.n_components = saved
        return super(LandmarkNystroem, self).fit(sequences, y=y)
