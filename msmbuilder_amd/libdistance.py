"""Drop-in for ``msmbuilder.libdistance`` on MI355X.

Same python-level signatures, dtype rules and error types as
/root/reference/msmbuilder/libdistance/libdistance.pyx:82-270 (``assign_nearest``,
``cdist``, ``dist``, ``pdist``, ``sumdist``); the arithmetic runs in libmsmhip's exact HIP kernels
(msmbuilder_amd/csrc/distance.hip) and is bit-identical to the reference's
scalar loops.  Extension: X / X_indices may be torch CUDA tensors, in which case
the per-row outputs come back as CUDA tensors too (nothing crosses PCIe).

The ninth metric, ``"rmsd"`` (minimal RMSD after optimal superposition), is accepted for conformations only: a
C-contiguous float32 array or torch CUDA tensor of shape (n_frames, n_atoms, 3), any object with an ``.xyz`` attribute of
that shape (an ``md.Trajectory``; mdtraj itself is never imported), or prepared :class:`RmsdFrames`.  With 2-D arrays it
raises the same ``ValueError`` as any unknown metric.  The arithmetic is libmsmhip's own (csrc/rmsd.hip):
every function returns the same float64 bits for the same pair, where the reference rounds some of them through a C
``float`` (libdistance.pyx:325, 350) and not others (:438-440); inputs are never centred in place.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import Arr, check, empty_like_placement, is_device_array

__all__ = ['assign_nearest', 'cdist', 'dist', 'pdist', 'sumdist', 'RmsdFrames']

VECTOR_METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev",
                  "canberra", "braycurtis", "hamming", "jaccard",
                  "cityblock")


def _is_array(x):
    return isinstance(x, np.ndarray) or is_device_array(x)


def _dtype_of(x):
    return np.dtype(str(x.dtype).replace("torch.", ""))


def _metric(metric):
    if isinstance(metric, bytes):
        metric = metric.decode()
    if metric not in VECTOR_METRICS:
        raise ValueError('metric must be one of %s' %
                         ', '.join("'%s'" % s for s in VECTOR_METRICS))
    return metric.encode()


def _pair_kind(X, Y, what):
    dx, dy = _dtype_of(X), _dtype_of(Y)
    if dx == np.float64 and dy == np.float64:
        return "f64", np.float64
    if dx == np.float32 and dy == np.float32:
        return "f32", np.float32
    raise TypeError(what)


def _host(y, dt):
    """per-centre arrays are host memory in the C ABI"""
    if is_device_array(y):
        y = y.detach().cpu().numpy()
    return np.ascontiguousarray(y, dtype=dt)


def _require_c_contiguous(*arrays):
    # the reference's typed memoryviews (float[:, ::1]) raise ValueError otherwise
    for a in arrays:
        if isinstance(a, np.ndarray) and not a.flags.c_contiguous:
            raise ValueError("ndarray is not C-contiguous")
        if is_device_array(a) and not a.is_contiguous():
            raise ValueError("tensor is not contiguous")


# --------------------------------------------------------------------------
# the rmsd metric: conformations, prepared once
# --------------------------------------------------------------------------
def is_rmsd(metric):
    if isinstance(metric, bytes):
        metric = metric.decode()
    return metric == "rmsd"


def conformations(x):
    """``x`` as a set of conformations -- prepared frames, or the 3-D array behind it -- or None when it is none."""
    if isinstance(x, RmsdFrames):
        return x
    if not _is_array(x) and hasattr(x, 'xyz'):
        x = x.xyz
    if _is_array(x) and x.ndim == 3:
        return x
    return None


class RmsdFrames(object):
    """Conformations prepared for the rmsd metric (``msm_rmsd_prepare``): every frame centred (centroid and difference in
    float64, rounded once to float32) and laid out atom-major, frame-fastest in device memory, with the float64 sum of
    squares of each frame.  Every libdistance function takes it in place of the raw coordinates, so a caller that
    measures against the same frames many times (a clusterer's ``fit``) prepares them once.

    ``xyz``: C-contiguous float32 (n_frames, n_atoms, 3), numpy or torch CUDA, or an object with such an ``.xyz``.  It is
    never modified and stays reachable as ``.xyz``; per-frame results come back on its side (host or device).
    """

    def __init__(self, xyz):
        if isinstance(xyz, RmsdFrames):
            raise TypeError('these frames are prepared already')
        if not _is_array(xyz) and hasattr(xyz, 'xyz'):
            xyz = xyz.xyz
        if not _is_array(xyz):
            raise TypeError('conformations must be a numpy array, a torch CUDA tensor or have an .xyz attribute')
        if xyz.ndim != 3:
            raise ValueError("Buffer has wrong number of dimensions (expected 3, got %d)" % xyz.ndim)
        if _dtype_of(xyz) != np.float32:   # the reference's float[:, :, ::1] view
            raise ValueError("Buffer dtype mismatch, expected 'float' but got '%s'" % _dtype_of(xyz).name)
        if xyz.shape[2] != 3:
            raise ValueError("conformations must have shape (n_frames, n_atoms, 3), got %s" % (tuple(xyz.shape),))
        _require_c_contiguous(xyz)
        self.xyz = xyz
        self.n_frames, self.n_atoms = int(xyz.shape[0]), int(xyz.shape[1])
        self._arr = Arr(xyz, np.float32)
        self._handle = None
        if self.n_frames and self.n_atoms:
            h = C.c_void_p()
            check(_lib.lib().msm_rmsd_prepare(C.byref(h), self._arr.vp, self.n_frames, self.n_atoms, self._arr.on_device))
            self._handle = h

    on_device = property(lambda self: self._arr.on_device)
    shape = property(lambda self: (self.n_frames, self.n_atoms, 3))

    def __len__(self):
        return self.n_frames

    @property
    def handle(self):
        if self._handle is None:
            raise ValueError("conformations need at least one frame and one atom")
        return self._handle

    def frames(self, ids):
        """The original coordinates of the listed frames: a host (len(ids), n_atoms, 3) float32 array."""
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        if self.on_device:
            import torch
            return self.xyz[torch.as_tensor(ids, device=self.xyz.device)].detach().cpu().numpy()
        return np.ascontiguousarray(self.xyz[ids])

    def close(self):
        h, self._handle = self._handle, None
        if h is not None:
            _lib.lib().msm_rmsd_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _frames(x):
    return x if isinstance(x, RmsdFrames) else RmsdFrames(x)


def _rmsd_indices(fx, X_indices):
    idx = Arr(X_indices, np.int64)
    if len(idx.shape) != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % len(idx.shape))
    if idx.on_device != fx.on_device:
        raise ValueError("X and X_indices must live on the same side (host or device)")
    return idx


def rmsd_assign(fx, fy, X_indices=None):
    """(labels, minimum distances, ordered inertia) of ``msm_rmsd_assign_nearest``, placed like the frames."""
    if fx.n_atoms != fy.n_atoms:
        raise ValueError("Input trajectories must have same number of atoms. found %d and %d." % (fx.n_atoms, fy.n_atoms))
    idx = _rmsd_indices(fx, X_indices) if X_indices is not None else None
    n = idx.shape[0] if idx is not None else fx.n_frames
    labels = empty_like_placement(fx._arr, (n,), np.intp)
    mind = empty_like_placement(fx._arr, (n,), np.float64)
    if n == 0:
        return labels, mind, 0.0
    al, am = Arr(labels, np.int64), Arr(mind, np.float64)
    inertia = C.c_double(0.0)
    check(_lib.lib().msm_rmsd_assign_nearest(fx.handle, fy.handle, idx.vp if idx is not None else None, n, al.vp, am.vp,
                                             C.byref(inertia), fx.on_device))
    return labels, mind, float(inertia.value)


def _rmsd_cdist(XA, XB):
    fa, fb = _frames(XA), _frames(XB)
    if fa.n_atoms != fb.n_atoms:
        raise ValueError('XA and XB must have the same number of atoms')
    out = empty_like_placement(fa._arr, (fa.n_frames, fb.n_frames), np.float64)
    if fa.n_frames == 0 or fb.n_frames == 0:
        return out
    check(_lib.lib().msm_rmsd_cdist(fa.handle, fb.handle, Arr(out, np.float64).vp, fa.on_device))
    return out


def _rmsd_dist(X, y, X_indices):
    fx = _frames(X)
    if not isinstance(y, RmsdFrames):
        if not _is_array(y) and hasattr(y, 'xyz'):
            y = y.xyz
        if _is_array(y) and y.ndim == 2:   # one conformation, (n_atoms, 3)
            y = y.reshape((1,) + tuple(y.shape))
        y = RmsdFrames(y)
    if y.n_frames != 1:
        raise ValueError("y must be a single conformation, got %d frames" % y.n_frames)
    if fx.n_atoms != y.n_atoms:
        raise ValueError("Input trajectories must have same number of atoms. found %d and %d." % (fx.n_atoms, y.n_atoms))
    idx = _rmsd_indices(fx, X_indices) if X_indices is not None else None
    n = idx.shape[0] if idx is not None else fx.n_frames
    out = empty_like_placement(fx._arr, (n,), np.float64)
    if n == 0:
        return out
    check(_lib.lib().msm_rmsd_dist(fx.handle, y.handle, 0, idx.vp if idx is not None else None, n, Arr(out, np.float64).vp,
                                   fx.on_device))
    return out


def rmsd_pdist(fx, X_indices=None, device=False):
    """Condensed rmsd matrix of the (indexed) frames.  ``device=True``: always a torch CUDA tensor (host frames and host
    indices included), for the callers that run the k-medoids loop over it where it lies."""
    fx = _frames(fx)
    if device:
        import torch
        dev = fx.xyz.device if fx.on_device else torch.device("cuda", _lib.ensure_device())
        idx = None
        n = fx.n_frames
        if X_indices is not None:
            if not is_device_array(X_indices):
                X_indices = torch.as_tensor(np.ascontiguousarray(X_indices, dtype=np.int64), device=dev)
            idx = Arr(X_indices, np.int64)
            n = idx.shape[0]
        out = torch.empty((n * (n - 1) // 2,), dtype=torch.float64, device=dev)
        on_device = 1
    else:
        idx = _rmsd_indices(fx, X_indices) if X_indices is not None else None
        n = idx.shape[0] if idx is not None else fx.n_frames
        out = empty_like_placement(fx._arr, (n * (n - 1) // 2,), np.float64)
        on_device = fx.on_device
    if n < 2:
        return out
    check(_lib.lib().msm_rmsd_pdist(fx.handle, idx.vp if idx is not None else None, n, Arr(out, np.float64).vp, on_device))
    return out


def _rmsd_sumdist(X, pair_indices):
    fx = _frames(X)
    pairs = Arr(pair_indices, np.int64)
    if len(pairs.shape) != 2 or pairs.shape[1] != 2:
        raise ValueError('pair_indices must be of shape = (n_pairs, 2)')
    if pairs.on_device != fx.on_device:
        raise ValueError("X and pair_indices must live on the same side (host or device)")
    s = C.c_double(0.0)
    if pairs.shape[0] == 0:
        return 0.0
    check(_lib.lib().msm_rmsd_sumdist(fx.handle, pairs.vp, pairs.shape[0], C.byref(s), fx.on_device))
    return float(s.value)


def assign_nearest(X, Y, metric, X_indices=None):
    """For each point in X (or X[X_indices]) the index of the nearest row of Y, and the
    summed distance.  libdistance.pyx:82-131 -> assign.hpp:6-91."""
    if is_rmsd(metric) and conformations(X) is not None and conformations(Y) is not None:
        labels, _, inertia = rmsd_assign(_frames(X), _frames(Y), X_indices)
        return labels, inertia
    if not _is_array(X) and _is_array(Y):
        raise TypeError()
    m = _metric(metric)
    kind, dt = _pair_kind(X, Y, 'X and y must be both float32 or float64')
    _require_c_contiguous(X, Y)
    if X.ndim != 2 or Y.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2)")
    assert X.shape[1] == Y.shape[1]
    ax = Arr(X, dt)
    ay = _host(Y, dt)
    idx = None
    n = ax.shape[0]
    if X_indices is not None:
        idx = Arr(X_indices, np.int64)
        if idx.on_device != ax.on_device:
            raise ValueError("X and X_indices must live on the same side (host or device)")
        n = idx.shape[0]
    out = empty_like_placement(ax, (n,), np.intp)
    if n == 0:
        return out, 0.0   # nothing to assign (assign.hpp's loop does not run; an empty device tensor has no address)
    aout = Arr(out, np.int64)
    inertia = C.c_double(0.0)
    fn = getattr(_lib.lib(), "msm_assign_nearest_" + kind)
    check(fn(ax.vp, C.c_void_p(ay.ctypes.data), m, idx.vp if idx is not None else None,
             ax.shape[0], ay.shape[0], ax.shape[1], n, aout.vp, None, C.byref(inertia), ax.on_device))
    return out, float(inertia.value)


def cdist(XA, XB, metric):
    """Distance between each pair of the two collections: libdistance.pyx:134-179 ->
    cdist.hpp:4-49.  float64 [na, nb]."""
    if is_rmsd(metric) and conformations(XA) is not None and conformations(XB) is not None:
        return _rmsd_cdist(XA, XB)
    if not (_is_array(XA) and _is_array(XB)):
        raise TypeError('XA and XB must be numpy arrays')
    m = _metric(metric)
    kind, dt = _pair_kind(XA, XB, 'XA and XB must be identically float32 or float64')
    _require_c_contiguous(XA, XB)
    if XA.shape[1] != XB.shape[1]:
        raise ValueError('XA and XB must have the same number of columns')
    ax = Arr(XA, dt)
    ab = _host(XB, dt)
    out = empty_like_placement(ax, (ax.shape[0], ab.shape[0]), np.float64)
    if ax.shape[0] == 0 or ab.shape[0] == 0:
        return out   # no pair (cdist.hpp's loops do not run; an empty device tensor has no address)
    aout = Arr(out, np.float64)
    fn = getattr(_lib.lib(), "msm_cdist_" + kind)
    check(fn(ax.vp, C.c_void_p(ab.ctypes.data), m, ax.shape[0], ab.shape[0], ax.shape[1], aout.vp,
             ax.on_device))
    return out


def dist(X, y, metric, X_indices=None):
    """Distance from one point to many: libdistance.pyx:229-270 -> dist.hpp:4-80."""
    if is_rmsd(metric) and conformations(X) is not None:
        return _rmsd_dist(X, y, X_indices)
    if not _is_array(X) and _is_array(y):
        raise TypeError()
    m = _metric(metric)
    kind, dt = _pair_kind(X, y, 'X and y must be both float32 or float64')
    _require_c_contiguous(X, y)
    if y.ndim != 1:
        raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % y.ndim)
    assert X.shape[1] == y.shape[0]
    ax = Arr(X, dt)
    ay = _host(y, dt)
    idx = None
    n = ax.shape[0]
    if X_indices is not None:
        idx = Arr(X_indices, np.int64)
        if idx.on_device != ax.on_device:
            raise ValueError("X and X_indices must live on the same side (host or device)")
        n = idx.shape[0]
    out = empty_like_placement(ax, (n,), np.float64)
    if n == 0:
        return out   # no row (an empty device tensor has no address, and a null X_indices would mean "every row")
    aout = Arr(out, np.float64)
    fn = getattr(_lib.lib(), "msm_dist_" + kind)
    check(fn(ax.vp, C.c_void_p(ay.ctypes.data), m, ax.shape[0], ax.shape[1],
             idx.vp if idx is not None else None, n, aout.vp, ax.on_device))
    return out


def pdist(X, metric, X_indices=None):
    """Condensed pairwise distances between the rows of X (or X[X_indices]):
    libdistance.pyx:182-226 -> pdist.hpp:4-88.  float64 [n(n-1)/2]."""
    if is_rmsd(metric) and conformations(X) is not None:
        return rmsd_pdist(X, X_indices)
    if not _is_array(X):
        raise TypeError()
    m = _metric(metric)
    dx = _dtype_of(X)
    if dx == np.float64:
        kind, dt = "f64", np.float64
    elif dx == np.float32:
        kind, dt = "f32", np.float32
    else:
        raise TypeError('X must be float32 or float64')
    _require_c_contiguous(X)
    ax = Arr(X, dt)
    idx = None
    n = ax.shape[0]
    if X_indices is not None:
        idx = Arr(X_indices, np.int64)
        if idx.on_device != ax.on_device:
            raise ValueError("X and X_indices must live on the same side (host or device)")
        n = idx.shape[0]
    out = empty_like_placement(ax, (n * (n - 1) // 2,), np.float64)
    if n < 2:
        return out   # no pair (an empty device tensor has no address)
    aout = Arr(out, np.float64)
    fn = getattr(_lib.lib(), "msm_pdist_" + kind)
    check(fn(ax.vp, m, ax.shape[0], ax.shape[1], idx.vp if idx is not None else None, n, aout.vp, ax.on_device))
    return out


def sumdist(X, metric, pair_indices):
    """Sum of the distances between the listed pairs of rows: libdistance.pyx:273-310 ->
    sumdist.hpp:4-44 (the reference adds sequentially; here an fp64 tree sum)."""
    if is_rmsd(metric) and conformations(X) is not None:
        return _rmsd_sumdist(X, pair_indices)
    m = _metric(metric)
    dx = _dtype_of(X)
    if dx == np.float64:
        kind, dt = "f64", np.float64
    elif dx == np.float32:
        kind, dt = "f32", np.float32
    else:
        raise TypeError('X must be both float32 or float64')
    _require_c_contiguous(X)
    ax = Arr(X, dt)
    pairs = Arr(pair_indices, np.int64)
    if len(pairs.shape) != 2 or pairs.shape[1] != 2:
        raise ValueError('pair_indices must be of shape = (n_pairs, 2)')
    if pairs.on_device != ax.on_device:
        raise ValueError("X and pair_indices must live on the same side (host or device)")
    s = C.c_double(0.0)
    fn = getattr(_lib.lib(), "msm_sumdist_" + kind)
    check(fn(ax.vp, m, ax.shape[0], ax.shape[1], pairs.vp, pairs.shape[0], C.byref(s), ax.on_device))
    return float(s.value)
