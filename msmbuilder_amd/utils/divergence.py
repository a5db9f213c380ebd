"""Kullback-Leibler, symmetrised KL and Jensen-Shannon divergences on MI355X: drop-in for ``msmbuilder.utils.divergence``
(reference: msmbuilder/utils/divergence.py).

The reference evaluates every divergence in nested Python loops over rows and columns.  Here the rows go to
``msm_divergence_*`` (csrc/divergence.hip), which keeps the reference's definition -- float64, terms added in ascending
column order, a term skipped where the float64 product ``P_k * Q_k`` is zero, ``max(sum, 0)`` with a NaN kept -- and its
summation order, so the only differences to the host loop are the device's ``log`` and division.

``kl_divergence(manual=False)`` stays ``scipy.stats.entropy`` on the host, as in the reference.  The ``*_msm`` variants
and ``fnorm`` are not provided.

Inputs are numpy arrays or torch CUDA tensors; results are placed like the (first) input.
"""
import numpy as np

from .. import _lib
from .._lib import Arr, check, is_device_array

__all__ = ['kl_divergence', 'sym_kl_divergence', 'js_divergence', 'js_metric', 'kl_divergence_array',
           'sym_kl_divergence_array', 'js_divergence_array', 'js_metric_array', 'divergence_cdist', 'divergence_pdist',
           'scipy_kl_divergence', 'manual_kl_divergence', 'KINDS', 'SYMMETRIC_KINDS']

KINDS = ('kl_divergence', 'sym_kl_divergence', 'js_divergence', 'js_metric')
SYMMETRIC_KINDS = KINDS[1:]


def _kind(kind):
    kind = kind.decode() if isinstance(kind, bytes) else kind
    if kind not in KINDS:
        raise ValueError('kind must be one of %s' % ', '.join("'%s'" % s for s in KINDS))
    return kind


def _rows(X, dtype=None):
    """A 2-D float32 / float64 ``Arr`` of X (anything else is computed in float64)."""
    if is_device_array(X):
        import torch
        if dtype is not None:
            X = X.to({np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}[np.dtype(dtype)])
        elif X.dtype not in (torch.float32, torch.float64):
            X = X.to(torch.float64)
    else:
        X = np.asarray(X)
        if dtype is not None:
            X = np.asarray(X, dtype=dtype)
        elif X.dtype not in (np.float32, np.float64):
            X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError('the rows must form a 2-dimensional array')
    if X.shape[1] < 1:
        raise ValueError('the rows must have at least one column')
    return Arr(X)


def _sfx(a):
    return "f64" if a.dtype == np.float64 else "f32"


def divergence_cdist(XA, XB, kind):
    """``out[i, j] = kind(XA[i], XB[j])``, float64, placed like XA.  XB takes XA's element type."""
    kind = _kind(kind)
    a = _rows(XA)
    if is_device_array(XB) != bool(a.on_device):
        raise ValueError('XA and XB must both be numpy arrays or both be torch CUDA tensors')
    b = _rows(XB, a.dtype)
    if a.shape[1] != b.shape[1]:
        raise ValueError('XA and XB must have the same number of columns')
    out = _lib.empty_like_placement(a, (a.shape[0], b.shape[0]), np.float64)
    if a.shape[0] and b.shape[0]:
        ao = Arr(out, np.float64)
        check(getattr(_lib.lib(), "msm_divergence_cdist_" + _sfx(a))(
            a.vp, a.shape[0], b.vp, b.shape[0], a.shape[1], kind.encode(), ao.vp, a.on_device))
    return out


def divergence_pdist(X, kind, X_indices=None, device=False):
    """The condensed matrix (``i < j``, scipy's order) of ``kind`` between the rows of X, or between the rows that
    ``X_indices`` names (a row may repeat).  float64, placed like X; ``device=True`` leaves the result of a numpy X on
    the device as a torch CUDA tensor (for :func:`msmbuilder_amd.cluster.agglomerative.linkage`)."""
    kind = _kind(kind)
    a = _rows(X)
    n = a.shape[0]
    idx = None
    if X_indices is not None:
        X_indices = np.ascontiguousarray(X_indices.cpu().numpy() if is_device_array(X_indices) else X_indices, dtype=np.int64)
        if X_indices.ndim != 1:
            raise ValueError('X_indices must be 1-dimensional')
        if len(X_indices) and (X_indices.min() < 0 or X_indices.max() >= n):
            raise ValueError('X_indices must lie in [0, %d)' % n)
    if device and not a.on_device:
        import torch
        _lib.ensure_device()
        a = Arr(torch.as_tensor(a.keep, device='cuda'))
    if X_indices is not None:
        if a.on_device:
            import torch
            idx = Arr(torch.as_tensor(X_indices, device=a.keep.device), np.int64)
        else:
            idx = Arr(X_indices, np.int64)
    nn = n if idx is None else idx.shape[0]
    out = _lib.empty_like_placement(a, (nn * (nn - 1) // 2 if nn > 1 else 0,), np.float64)
    if nn > 1:
        ao = Arr(out, np.float64)
        check(getattr(_lib.lib(), "msm_divergence_pdist_" + _sfx(a))(
            a.vp, n, a.shape[1], idx.vp if idx is not None else None, nn, kind.encode(), ao.vp, a.on_device))
    return out


def _pair_rows(P, Q, kind):
    """``out[r] = kind(P[r], Q[r])`` as a host float64 array (the paired-rows kernel); P and Q are 2-D."""
    if is_device_array(P):
        P = P.cpu().numpy()
    if is_device_array(Q):
        Q = Q.cpu().numpy()
    a = _rows(P)
    b = _rows(Q, a.dtype)
    if a.shape != b.shape:
        raise ValueError('P and Q must have the same shape')
    out = np.zeros(a.shape[0], dtype=np.float64)
    if a.shape[0]:
        check(getattr(_lib.lib(), "msm_divergence_rows_" + _sfx(a))(
            a.vp, b.vp, a.shape[0], a.shape[1], _kind(kind).encode(), out.ctypes.data))
    return out


def _two_d(P, Q):
    on_device = is_device_array(P)
    P = P if is_device_array(P) else np.asarray(P)
    Q = Q if is_device_array(Q) else np.asarray(Q)
    if P.ndim == 1:
        P, Q = P[None, :], Q[None, :]
    if P.ndim != 2 or tuple(P.shape) != tuple(Q.shape):
        raise ValueError('P and Q must be 1-D or 2-D arrays of the same shape')
    return P, Q, on_device


def _placed(values, on_device, like):
    if on_device:
        import torch
        return torch.as_tensor(values, device=like.device)
    return values


def _pair(P, Q, kind, scalar):
    """The reference's pair functions: per-row values (``scalar=False``) or, for ``scalar=True``, what the reference's
    sums over the rows give.  For the compound kinds those sums are taken per KL part, as the reference takes them."""
    first = P
    P, Q, on_device = _two_d(P, Q)
    if not scalar:
        return _placed(_pair_rows(P, Q, kind), on_device, first)
    if P.shape[0] == 1 or kind == 'kl_divergence':
        value = np.sum(_pair_rows(P, Q, kind))
    elif kind == 'sym_kl_divergence':
        value = np.sum(_pair_rows(P, Q, 'kl_divergence')) + np.sum(_pair_rows(Q, P, 'kl_divergence'))
    else:
        Ph, Qh = _rows(P.cpu().numpy() if on_device else P).keep, _rows(Q.cpu().numpy() if on_device else Q).keep
        M = (Ph.astype(np.float64) + Qh.astype(np.float64)) / 2
        value = (0.5 * np.sum(_pair_rows(Ph.astype(np.float64), M, 'kl_divergence'))
                 + 0.5 * np.sum(_pair_rows(Qh.astype(np.float64), M, 'kl_divergence')))
        if kind == 'js_metric':
            value = np.sqrt(value)
    return value


def scipy_kl_divergence(P, Q, scalar=True):
    from scipy.stats import entropy
    P = P.cpu().numpy() if is_device_array(P) else np.asarray(P)
    Q = Q.cpu().numpy() if is_device_array(Q) else np.asarray(Q)
    result = entropy(P.T, Q.T)
    return np.sum(result) if scalar else result


def manual_kl_divergence(P, Q, scalar=True):
    return _pair(P, Q, 'kl_divergence', scalar)


def kl_divergence(P, Q, manual=True, scalar=True):
    """``sum_k P_k log(P_k / Q_k)`` over the columns where ``P_k * Q_k != 0``, clamped at 0; 1-D or 2-D input
    (row by row).  ``manual=False``: ``scipy.stats.entropy`` on the host."""
    if manual:
        return manual_kl_divergence(P, Q, scalar=scalar)
    return scipy_kl_divergence(P, Q, scalar=scalar)


def sym_kl_divergence(P, Q, scalar=True):
    """``kl(P, Q) + kl(Q, P)``."""
    return _pair(P, Q, 'sym_kl_divergence', scalar)


def js_divergence(P, Q, scalar=True):
    """``0.5 kl(P, M) + 0.5 kl(Q, M)`` with ``M = (P + Q) / 2``."""
    return _pair(P, Q, 'js_divergence', scalar)


def js_metric(P, Q, scalar=True):
    """The square root of the Jensen-Shannon divergence."""
    return _pair(P, Q, 'js_metric', scalar)


def _array(ref, target, i, kind):
    a = _rows(ref)
    i = int(i)
    if not -a.shape[0] <= i < a.shape[0]:
        raise IndexError('index %d is out of bounds for %d rows' % (i, a.shape[0]))
    return divergence_cdist(a.keep[i:i + 1] if i >= 0 else a.keep[i:][:1], target, kind)[0]


def kl_divergence_array(ref, target, i):
    """``kl_divergence(ref[i], t)`` for every row t of ``target``."""
    return _array(ref, target, i, 'kl_divergence')


def sym_kl_divergence_array(ref, target, i):
    return _array(ref, target, i, 'sym_kl_divergence')


def js_divergence_array(ref, target, i):
    return _array(ref, target, i, 'js_divergence')


def js_metric_array(ref, target, i):
    return _array(ref, target, i, 'js_metric')


# The callables that LandmarkAgglomerative and MVCA accept as ``metric``, by identity.
ARRAY_FUNCTION_KINDS = {kl_divergence_array: 'kl_divergence', sym_kl_divergence_array: 'sym_kl_divergence',
                        js_divergence_array: 'js_divergence', js_metric_array: 'js_metric'}
