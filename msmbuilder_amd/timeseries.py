"""Time-series smoothers in front of tICA, computed on the GPU.

Drop-ins for ``msmbuilder.preprocessing.timeseries``'s ``Butterworth``, ``EWMA`` and ``DoubleEWMA``: the reference's
constructor arguments, ``fit`` (a no-op) / ``transform(sequences)`` / ``partial_transform(X)`` / ``fit_transform``.  Inputs
are numpy arrays or ``torch`` CUDA tensors (contiguous or pitched rows); every output lies where its input does.

All three are ONE linear recurrence along the time axis (scipy's ``lfilter`` in transposed direct form II; an EWMA's
numerator is its order-1 case), which ``msm_ts_filter`` runs parallel in time over every (trajectory, segment, column) of
a list in three launches per direction: a local pass per segment, a stitch per trajectory, a final pass.  The filter's
design -- ``butter`` and ``lfilter_zi`` -- is scipy's, on the host, as in the reference; the arithmetic over the frames is
float64 whatever the rows' type, rounded once at the store.

The segment length is read off the decay of the filter's state matrix (``segment_length``: the slowest pole's memory and
the transient in front of it): stitching across segments shorter than that cancels large numbers (DESIGN 3.15 has the
measurements).  ``MSM_TS_SEGMENT=<frames>`` overrides it (0: one segment per trajectory, the recurrence serial in time).
"""
import ctypes as C
import os

import numpy as np
import sklearn.base

from . import _lib
from ._lib import check, is_device_array
from .base import BaseEstimator
from .utils.validation import check_iter_of_sequences

__all__ = ['Butterworth', 'EWMA', 'DoubleEWMA', 'segment_length', 'ts_filter']

TS_BUTTERWORTH, TS_EWMA, TS_DOUBLE_EWMA = 0, 1, 2
MAX_ORDER = 8
SEGMENT_DECAY = 2.0 ** -10   # a segment is long enough for the state's memory to fall to this: max |A^S| <= SEGMENT_DECAY
SEGMENT_MIN = 256            # frames, at least
SEGMENT_MAX = 1 << 20


def _state_power(a, S):
    """A^S in long double; A is the recurrence's state matrix, A[k][0] = -a[k+1], A[k][k+1] = 1."""
    p = len(a) - 1
    A = np.zeros((p, p), dtype=np.longdouble)
    A[:, 0] = -np.asarray(a[1:], dtype=np.longdouble)
    for k in range(p - 1):
        A[k, k + 1] = 1
    R = np.eye(p, dtype=np.longdouble)
    while S > 0:
        if S & 1:
            R = R.dot(A)
        S >>= 1
        if S:
            A = A.dot(A)
    return R


def segment_length(a):
    """Frames per segment for the denominator ``a`` (a[0] = 1): the shortest of 256, 384, 512, 768, 1024, ... at which the
    state's memory has decayed, max |A^S| <= SEGMENT_DECAY -- the slowest pole's time constant times the logarithm of the
    transient the bunched poles of a high order put in front of it (|A^S| passes 1e5 before it falls).  0, one segment per
    trajectory, when no length up to SEGMENT_MAX gets there: the float64 coefficients of a wide high-order design have
    poles ON or outside the unit circle, and nothing is gained by cutting what does not forget."""
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    if len(a) < 2:
        return SEGMENT_MIN
    S, step = SEGMENT_MIN, 0
    with np.errstate(all="ignore"):
        while S <= SEGMENT_MAX:
            if all(float(np.max(np.abs(_state_power(a, s)))) <= SEGMENT_DECAY for s in (S, 2 * S)):
                return S
            S = S * 3 // 2 if step % 2 == 0 else S * 4 // 3
            step += 1
    return 0


def _segment_for(a, longest):
    """The segment handed to the library: the switch if set, else the rule -- and one segment per trajectory where the
    rule would leave the longest trajectory fewer than two whole segments."""
    env = os.environ.get("MSM_TS_SEGMENT")
    if env is not None and env != "":
        s = int(env)
        if s < 0:
            raise ValueError("MSM_TS_SEGMENT must be a number of frames (0: one segment per trajectory)")
        return s
    s = segment_length(a)
    return s if s and longest >= 2 * s else 0


def _rows(X):
    """A 2-D float32 / float64 array the library can read in place: numpy C-contiguous, or a CUDA tensor whose rows are
    contiguous (unit column stride; the row stride may exceed the width)."""
    if is_device_array(X):
        import torch
        if X.dim() != 2:
            raise ValueError("a trajectory is a 2-D array (n_frames, n_features)")
        if X.dtype not in (torch.float32, torch.float64):
            X = X.to(torch.float64)
        if X.shape[0] > 1 and (X.stride(1) != 1 or X.stride(0) < X.shape[1]) or X.shape[0] <= 1 and not X.is_contiguous():
            X = X.contiguous()
        return X
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError("a trajectory is a 2-D array (n_frames, n_features)")
    if X.dtype not in (np.float32, np.float64):
        X = X.astype(np.float64)
    return np.ascontiguousarray(X)


def _joined(sequences):
    """(rows, F, itemsize) of a list of CUDA tensors that are contiguous float views of one tensor lying back to back --
    what ``X.view(n, T, F).unbind(0)`` or ``split`` give, and what this module returns -- or None.  Spares a thousand
    trajectories the per-tensor checks and pointer reads, which cost more than the kernels."""
    head = sequences[0]
    if len(sequences) < 2 or not is_device_array(head):
        return None
    import torch
    if head.dtype not in (torch.float32, torch.float64) or not all(map(is_device_array, sequences)):
        return None
    rows = _lib.adjacent_rows(sequences)
    if rows is None or not (rows > 0).all():
        return None
    return rows, int(head.shape[1]), head.element_size()


def ts_filter(sequences, kind, order=1, b=None, a=None, zi=None, width=0, alpha=0.0, adjust=True, min_periods=0,
              segment=0):
    """``msm_ts_filter`` over a list of trajectories: one call per (placement, dtype, row stride, device) class.  Returns
    the list of outputs, each placed like its input (float64 for the EWMA kinds, the input's dtype for Butterworth).
    ``segment``: frames per segment, or a function of the longest trajectory's frames that returns them."""
    sequences = list(sequences)
    if not sequences:
        return []
    coef = [None if v is None else np.ascontiguousarray(v, dtype=np.float64) for v in (b, a, zi)]
    cp = [None if v is None else v.ctypes.data for v in coef]
    L = _lib.lib()

    def run(xp, op, rows, n, nbytes, F, ld, dev, longest):
        seg = segment(longest) if callable(segment) else segment
        check(L.msm_ts_filter(xp, op, rows, n, nbytes, F, ld, F, int(dev), int(kind), int(order), cp[0], cp[1], cp[2],
                              int(width), float(alpha), int(bool(adjust)), int(min_periods), int(seg)))

    joined = _joined(sequences)
    if joined is not None:
        import torch
        rows, F, nbytes = joined
        head = sequences[0]
        _lib.ensure_device(head.device.index)
        _lib.set_stream(torch.cuda.current_stream(head.device).cuda_stream)
        out_f64 = kind != TS_BUTTERWORTH or nbytes == 8
        block = torch.empty((int(rows.sum()), F), dtype=torch.float64 if out_f64 else torch.float32, device=head.device)
        first = np.concatenate(([0], np.cumsum(rows[:-1])))
        xptr = (head.data_ptr() + first * (F * nbytes)).astype(np.uint64)
        optr = (block.data_ptr() + first * (F * block.element_size())).astype(np.uint64)
        run(xptr.ctypes.data_as(C.POINTER(C.c_void_p)), optr.ctypes.data_as(C.POINTER(C.c_void_p)),
            rows.ctypes.data_as(C.POINTER(C.c_int64)), len(rows), nbytes, F, F, True, int(rows.max()))
        return list(block.split(rows.tolist()))

    arrs = [_rows(X) for X in sequences]
    F = arrs[0].shape[1]
    for x in arrs:
        if x.shape[1] != F:
            raise ValueError("X has %d features, but %d were expected" % (x.shape[1], F))
    if F < 1:
        raise ValueError("a trajectory needs at least one feature")
    longest = max(x.shape[0] for x in arrs)
    outs = [None] * len(arrs)
    classes = {}
    for i, x in enumerate(arrs):
        dev = is_device_array(x)
        nbytes = 8 if str(x.dtype).endswith("64") else 4
        ld = int(x.stride(0)) if dev and x.shape[0] > 1 else F
        classes.setdefault((dev, nbytes, ld, x.device.index if dev else -1), []).append(i)
    for (dev, nbytes, ld, _), idx in classes.items():
        n = len(idx)
        out_f64 = kind != TS_BUTTERWORTH or nbytes == 8
        if dev:
            import torch
            head = arrs[idx[0]]     # device / stream binding once; raw pointers for the rest (pitched rows are read in place)
            _lib.ensure_device(head.device.index)
            _lib.set_stream(torch.cuda.current_stream(head.device).cuda_stream)
            # one allocation for the class, cut into per-trajectory views: a thousand small allocations cost more than
            # the kernels, and outputs that lie back to back go through the next stage's joined-rows path as one array
            block = torch.empty((sum(arrs[i].shape[0] for i in idx), F), dtype=torch.float64 if out_f64 else torch.float32,
                                device=head.device)
            for i, piece in zip(idx, block.split([arrs[i].shape[0] for i in idx])):
                outs[i] = piece
            xp = (C.c_void_p * n)(*[arrs[i].data_ptr() for i in idx])
            op = (C.c_void_p * n)(*[outs[i].data_ptr() for i in idx])
        else:
            _lib.ensure_device()
            for i in idx:
                outs[i] = np.empty(arrs[i].shape, dtype=np.float64 if out_f64 else np.float32)
            xp = (C.c_void_p * n)(*[arrs[i].ctypes.data for i in idx])
            op = (C.c_void_p * n)(*[outs[i].ctypes.data for i in idx])
        rows = (C.c_int64 * n)(*[arrs[i].shape[0] for i in idx])
        run(xp, op, rows, n, nbytes, F, ld, dev, longest)
    return outs


class _TimeSeriesSmoother(BaseEstimator, sklearn.base.TransformerMixin):
    """fit (nothing to learn) / transform over lists of sequences (preprocessing/base.py's multi-sequence mixin)."""

    def fit(self, sequences, y=None):
        return self

    def partial_fit(self, sequence, y=None):
        return self

    def transform(self, sequences):
        """All trajectories in one library call: the work is parallel over trajectories x segments x columns."""
        check_iter_of_sequences(sequences)
        return self._smooth(list(sequences))

    def partial_transform(self, sequence):
        return self._smooth([sequence])[0]

    def fit_transform(self, sequences, y=None):
        return self.transform(sequences)


class Butterworth(_TimeSeriesSmoother):
    """Smooth time-series data using a low-pass, zero-delay Butterworth filter.

    Parameters
    ----------
    width : int, optional, default=5
        Like the window of a moving average: the cut-off frequency is two over this width.  An integer greater than one;
        the nearest odd integer upwards is used.
    order : int, optional, default=3
        The order of the filter, 1 to 8.  Higher orders cut off more sharply and are worse conditioned: the (b, a) form
        bunches its poles near 1 at large widths, and what scipy computes there this computes no better.
    analog : bool
        Kept for the reference's signature; unused there as well.

    Per column: reflect-pad by ``width - 1`` rows (``x[w-1:0:-1], x, x[-1:-w:-1]``), apply ``scipy.signal.filtfilt``'s
    defaults to that signal, crop the padding.  The result has the input's dtype.  A trajectory shorter than ``width``
    raises ``ValueError``; a column holding a NaN or an infinity comes out all NaN.
    """

    def __init__(self, width=5, order=3, analog=True):
        from scipy.signal import butter, lfilter_zi
        if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or width < 2:
            raise ValueError('width must be an integer greater than 1.')
        if isinstance(order, bool) or not isinstance(order, (int, np.integer)):
            raise ValueError('order must be an integer')
        if not 1 <= order <= MAX_ORDER:
            raise ValueError('order must lie in 1 .. %d' % MAX_ORDER)
        self.width = int(np.ceil((width + 1) / 2) * 2 - 1)   # nearest odd integer upwards
        self.order = int(order)
        self.analog = analog
        self._num, self._denom = butter(self.order, 2.0 / self.width)
        self._zi = lfilter_zi(self._num, self._denom)

    def _smooth(self, sequences):
        pad = 2 * (self.width - 1) + 6 * (self.order + 1)   # a pass runs over the padded signal
        return ts_filter(sequences, TS_BUTTERWORTH, order=self.order, b=self._num, a=self._denom, zi=self._zi, width=self.width,
                         segment=lambda longest: _segment_for(self._denom, longest + pad))


class EWMA(_TimeSeriesSmoother):
    """Smooth time-series data using an exponentially-weighted moving average: ``DataFrame.ewm(...).mean()``.

    Parameters
    ----------
    com, span, halflife : float, optional
        Exactly one: the decay as centre of mass (alpha = 1 / (1 + com), com >= 0), span (alpha = 2 / (span + 1),
        span >= 1) or half-life (alpha = 1 - exp(log(0.5) / halflife), halflife > 0).
    min_periods : int, default 0
        The first ``min_periods - 1`` rows are NaN.
    freq : None
        The pandas the reference was written for took a frequency here; current pandas does not, so anything but None
        raises.
    adjust : bool, default True
        True: ``sum_i (1-alpha)^i x_{t-i} / sum_i (1-alpha)^i``.  False: ``y_0 = x_0``, ``y_t = (1-alpha) y_{t-1} + alpha x_t``.

    The output is float64 whatever the input, as pandas returns it.  Non-finite input raises ``ValueError`` (pandas'
    missing-value weighting is not implemented).
    """
    _kind = TS_EWMA

    def __init__(self, com=None, span=None, halflife=None, min_periods=0, freq=None, adjust=True):
        self.com = com
        self.span = span
        self.halflife = halflife
        self.min_periods = min_periods
        self.freq = freq
        self.adjust = adjust

    def _alpha(self):
        if self.freq is not None:
            raise ValueError("freq is not supported: DataFrame.ewm takes no such argument any more")
        given = [v for v in (self.com, self.span, self.halflife) if v is not None]
        if len(given) > 1:
            raise ValueError("comass, span and halflife are mutually exclusive")
        if not given:
            raise ValueError("Must pass one of comass, span or halflife")
        if self.com is not None:
            if not self.com >= 0:
                raise ValueError("comass must satisfy: comass >= 0")
            com = float(self.com)
        elif self.span is not None:
            if not self.span >= 1:
                raise ValueError("span must satisfy: span >= 1")
            com = (float(self.span) - 1) / 2.0
        else:
            if not self.halflife > 0:
                raise ValueError("halflife must satisfy: halflife > 0")
            decay = 1 - np.exp(np.log(0.5) / float(self.halflife))
            com = 1 / decay - 1
        mp = self.min_periods
        if isinstance(mp, bool) or not isinstance(mp, (int, np.integer)) or mp < 0:
            raise ValueError("min_periods must be an integer >= 0")
        return 1.0 / (1.0 + com)

    def _smooth(self, sequences):
        alpha = self._alpha()
        return ts_filter(sequences, self._kind, alpha=alpha, adjust=self.adjust, min_periods=int(self.min_periods),
                         segment=lambda longest: _segment_for([1.0, -(1.0 - alpha)], longest))


class DoubleEWMA(EWMA):
    """Smooth time-series data using forward and backward exponentially-weighted moving averages: ``(fwd + bwd) / 2``.

    The parameters are EWMA's.  As in the reference, ``bwd`` is the EWMA of the time-reversed trajectory and is NOT
    reversed back before the two are averaged: row t of the result is the mean of the forward average at frame t and the
    backward average at frame n - 1 - t.  This is a drop-in, so that is reproduced, not corrected.
    """
    _kind = TS_DOUBLE_EWMA
