"""A numpy restatement of the time-series smoothers (Butterworth, EWMA, DoubleEWMA), written from their formulas.

Two uses of one recurrence, scipy's ``lfilter`` in transposed direct form II with state z in R^p:

    y    = z[0] + b[0] x
    z[k] = (z[k+1] + b[k+1] x) - a[k+1] y          (z[p] = 0)

* ``dtype=np.longdouble`` (the default): the sequential loop in extended precision -- the reference every other
  implementation (scipy, pandas, the device) is measured against;
* ``butterworth_segmented`` / ``ewma_segmented`` in float64: the DEVICE's order of operations -- a local pass per segment
  from ``zi * u[segment start]``, a stitch with the float64 image of the long-double ``A^S``, a final pass.  numpy rounds
  every product and sum on its own, as the device unit does (it is built without contraction).

Also here: the seeded inputs shared by the golden generator and the tests, and the tolerances with their derivations.
"""
import numpy as np

LD = np.longdouble
EPS64 = float(np.finfo(np.float64).eps)
EPS32 = float(np.finfo(np.float32).eps)

# ---- tolerances -----------------------------------------------------------------------------------------------------------
# Butterworth.  The yardstick is scipy's own error against the long-double loop on the same input, e_scipy (relative to
# the output's scale max|y|): the (b, a) form is ill-conditioned at large widths and no float64 evaluation does better than
# that by more than a constant.  The device may use MARGIN times that -- the reassociation at the seams; the margin was
# set from the float64 emulation of the device's order (profiles/timeseries_bounds.txt records the measured ratios, at most
# MARGIN_MEASURED_MAX; the issue caps the margin at 4) -- plus ULPS units in the last place of the output's type at the
# output's scale: the final store's rounding (half an ulp), and a floor for inputs on which scipy happens to be exact.
MARGIN = 2.0
ULPS = 4.0


def butterworth_bound(e_scipy, scale, out_dtype):
    """Absolute tolerance of a device Butterworth output whose scale is ``scale``, given scipy's relative error."""
    eps = EPS32 if np.dtype(out_dtype) == np.float32 else EPS64
    return (MARGIN * e_scipy + ULPS * eps) * scale


# EWMA.  One pole q = 1 - alpha in [0, 1), positive weights: no cancellation.  With u = eps / 2 the unit roundoff and
# X = max|x| of the column:
#   numerator  n_t = q n_{t-1} + x_t: a product and a sum, each within u of a value bounded by X d_t (d_t = sum_i q^i <= 1 /
#              alpha), so the error obeys e_t <= q e_{t-1} + 2 u X d_t  =>  e_t <= 2 u X d_t^2;
#   denominator the same recurrence on ones: relative error <= 2 u d_t;  the quotient adds u.
#   => |y_t - exact| <= (4 d_t + 1) u X <= (2 / alpha + 1) eps X     sequentially (adjust=False: the same recurrence on y);
#   a seam     adds q^S (rounded from long double: u), a product and a sum on the numerator's scale: <= 3 u X d_t, which
#              later frames damp by q per frame; after the division <= 3 u X per seam in front of the frame, undamped at worst.
#   => |y_t - exact| <= ((2 / alpha + 1) + 2 n_seams) eps X.
# DoubleEWMA is the mean of two such values: the same bound.
def ewma_bound(alpha, n_seams, xmax):
    return ((2.0 / alpha + 1.0) + 2.0 * n_seams) * EPS64 * xmax


# ---- inputs (regenerated from seeds wherever they are needed) -----------------------------------------------------------------
def walk(n, F, seed, offset=0.0, dtype=np.float64):
    """A random walk per column, standardised to unit spread, then shifted by ``offset`` (|mean| / std = offset)."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, F).cumsum(0)
    X = (X - X.mean(0)) / np.maximum(X.std(0), 1e-12) + 0.1 * rs.randn(n, F)
    return np.ascontiguousarray((X + offset).astype(dtype))


def butter_design(width, order):
    """(odd width, b, a, zi) as the reference's constructor forms them (scipy on the host)."""
    from scipy.signal import butter, lfilter_zi
    w = int(np.ceil((width + 1) / 2) * 2 - 1)
    b, a = butter(order, 2.0 / w)
    return w, b, a, lfilter_zi(b, a)


def ewm_alpha(com=None, span=None, halflife=None):
    if com is not None:
        c = float(com)
    elif span is not None:
        c = (float(span) - 1) / 2.0
    else:
        c = 1 / (1 - np.exp(np.log(0.5) / float(halflife))) - 1
    return 1.0 / (1.0 + c)


def relerr(y, ref):
    """max |y - ref| over max |ref|, in long double."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.max(np.abs(np.asarray(y, dtype=LD) - ref)) / np.max(np.abs(ref)))


def scipy_butterworth(X, width, order):
    """What the reference computes per column, in float64: filtfilt over the reflect-padded signal, cropped."""
    from scipy.signal import filtfilt
    w, b, a, _ = butter_design(width, order)
    X = np.asarray(X, dtype=np.float64)
    return np.stack([filtfilt(b, a, reflect_pad(X[:, c], w))[w - 1:-(w - 1)] for c in range(X.shape[1])], 1)


# The Butterworth test inputs, shared by the CPU and the GPU tests: (name, width, order, frames, segment) -- segment None:
# the library's rule.  Three un-centred columns (|mean| / std = 100) each.  Every input has scipy's own error below 1e-9
# of scale (test_timeseries_ref.py asserts it): the domain in which scipy computes the filter at all.  The forced segment of
# 64 is far below the rule's for width 101, so it is held only at the orders whose stitch stays well conditioned there
# (orders 1 and 3; order 5 at 64 frames is 300 x scipy's error in the emulation, which is what the rule is for).
BW_CASES = [
    ("w2_o1_s64", 2, 1, 193, 64), ("w2_o3_s64", 2, 3, 193, 64), ("w2_o8_s64", 2, 8, 193, 64),
    ("w5_o1_s64", 5, 1, 193, 64), ("w5_o3_s64", 5, 3, 193, 64), ("w5_o8_s64", 5, 8, 193, 64),
    ("w101_o1_s64", 101, 1, 257, 64), ("w101_o3_s64", 101, 3, 257, 64),
    ("w5_o3_long", 5, 3, 20000, None), ("w101_o3_long", 101, 3, 20000, None), ("w101_o5_long", 101, 5, 20000, None),
    ("w1001_o3_long", 1001, 3, 20000, None), ("w1001_o3_single", 1001, 3, 5000, None),
]
# EWMA: (name, decay, adjust, min_periods, frames, segment)
EW_CASES = [
    ("com0.5_adj_s64", dict(com=0.5), True, 0, 193, 64), ("com0.5_rec_s64", dict(com=0.5), False, 1, 193, 64),
    ("span20_adj_s64", dict(span=20), True, 5, 193, 64), ("span20_rec_s64", dict(span=20), False, 5, 193, 64),
    ("hl7.5_adj_s64", dict(halflife=7.5), True, 300, 193, 64), ("hl7.5_rec_s64", dict(halflife=7.5), False, 0, 193, 64),
    ("com0_adj_s64", dict(com=0), True, 0, 65, 64),
    ("com100_adj_long", dict(com=100), True, 0, 20000, None), ("com100_rec_long", dict(com=100), False, 0, 20000, None),
]


# the goldens (tests/golden/make_golden_timeseries.py): outputs of the reference / of pandas on golden_input
GOLDEN_BUTTERWORTH = [(2, 1), (2, 3), (5, 1), (5, 3), (5, 8), (101, 3)]
GOLDEN_EWMA = [("com0.5_adj", dict(com=0.5), True, 0), ("com0.5_rec", dict(com=0.5), False, 0),
               ("span20_adj_mp5", dict(span=20), True, 5), ("span20_rec_mp5", dict(span=20), False, 5),
               ("hl7.5_adj", dict(halflife=7.5), True, 1), ("hl7.5_rec", dict(halflife=7.5), False, 1)]


def golden_input(dtype):
    return walk(300, 3, seed=2024, offset=100.0, dtype=dtype)


def case_input(name, n, F=3, dtype=np.float64):
    seed = sum(ord(c) * (i + 1) for i, c in enumerate("%s/%d" % (name, n))) % (2 ** 31)
    return walk(n, F, seed, offset=100.0, dtype=dtype)


LENGTHS = (63, 64, 65, 129, 193)   # around one, two and three segments of 64 frames


def bw_case_lengths(case):
    """Frames of the trajectories a Butterworth case runs: at a forced segment the shortest the filter takes (the width, or
    what brings the padded length above padlen) and the lengths around the seams (none shorter), else the one long
    trajectory."""
    name, width, order, n_max, seg = case
    w = int(np.ceil((width + 1) / 2) * 2 - 1)
    lo = max(w, 3 * (order + 1) - 2 * (w - 1) + 1)
    return sorted({max(n, lo) for n in (lo,) + LENGTHS + (n_max,)}) if seg else [n_max]


# ---- the recurrence ---------------------------------------------------------------------------------------------------------
def tdf2(b, a, u, z, dtype=LD):
    """Run u (n, C) through the recurrence from state z (p, C); returns (y, end state).  Sequential in time."""
    b = np.asarray(b, dtype=dtype)
    a = np.asarray(a, dtype=dtype)
    u = np.asarray(u, dtype=dtype)
    z = np.array(z, dtype=dtype, copy=True)
    p = len(a) - 1
    y = np.empty(u.shape, dtype=dtype)
    for t in range(u.shape[0]):
        x = u[t]
        yt = z[0] + b[0] * x
        for k in range(p - 1):
            z[k] = (z[k + 1] + b[k + 1] * x) - a[k + 1] * yt
        z[p - 1] = b[p] * x - a[p] * yt
        y[t] = yt
    return y, z


def state_power(a, S):
    """A^S in long double (A[k][0] = -a[k+1], A[k][k+1] = 1), rounded to float64."""
    p = len(a) - 1
    A = np.zeros((p, p), dtype=LD)
    A[:, 0] = -np.asarray(a[1:], dtype=LD)
    for k in range(p - 1):
        A[k, k + 1] = 1
    R = np.eye(p, dtype=LD)
    e = int(S)
    while e > 0:
        if e & 1:
            R = R.dot(A)
        e >>= 1
        if e:
            A = A.dot(A)
    return R.astype(np.float64)


def tdf2_segmented(b, a, u, z0, zi, S):
    """The device's order in float64: u (n, C); z0, zi (p,) multiply u[0] / u[segment start].  Returns y."""
    u = np.asarray(u, dtype=np.float64)
    n = u.shape[0]
    p = len(a) - 1
    z0 = np.asarray(z0, dtype=np.float64)[:, None]
    zi = np.asarray(zi, dtype=np.float64)[:, None]
    if not S or S >= n:
        return tdf2(b, a, u, z0 * u[0], np.float64)[0]
    nseg = -(-n // S)
    AS = state_power(a, S)
    local = lambda j: (z0 if j == 0 else zi) * u[j * S]
    ends = [tdf2(b, a, u[j * S:(j + 1) * S], local(j), np.float64)[1] for j in range(nseg - 1)]
    starts = [local(0)]
    for j in range(nseg - 1):
        d = starts[j] - local(j)
        zn = np.empty_like(d)
        for k in range(p):
            acc = ends[j][k]
            for m in range(p):
                acc = acc + AS[k, m] * d[m]
            zn[k] = acc
        starts.append(zn)
    return np.concatenate([tdf2(b, a, u[j * S:(j + 1) * S], starts[j], np.float64)[0] for j in range(nseg)])


# ---- Butterworth ------------------------------------------------------------------------------------------------------------
def reflect_pad(X, w):
    """x[w-1:0:-1], x, x[-1:-w:-1] along time."""
    return np.concatenate([X[w - 1:0:-1], X, X[-1:-w:-1]])


def odd_extend(P, pl):
    """2 p[0] - p[pl:0:-1], p, 2 p[-1] - p[-2:-(pl+2):-1]."""
    return np.concatenate([2 * P[0] - P[pl:0:-1], P, 2 * P[-1] - P[-2:-(pl + 2):-1]])


def _butterworth(X, w, b, a, zi, run):
    X = np.asarray(X)
    if X.shape[0] < w:
        raise ValueError("a trajectory of %d frames is shorter than the filter's width %d" % (X.shape[0], w))
    order = len(a) - 1
    pl = 3 * (order + 1)
    P = reflect_pad(X, w)
    if P.shape[0] <= pl:
        raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % pl)
    ext = odd_extend(P, pl)
    yf = run(ext)
    yb = run(yf[::-1])[::-1]
    out = yb[pl + w - 1:pl + w - 1 + X.shape[0]]
    bad = ~np.isfinite(np.asarray(X, dtype=np.float64)).all(0)
    out[:, bad] = np.nan
    return out


def butterworth(X, width, order, dtype=LD):
    """The long-double reference: (n, F) in, (n, F) long double out."""
    w, b, a, zi = butter_design(width, order)
    zi_ = np.asarray(zi, dtype=dtype)[:, None]
    return _butterworth(np.asarray(X, dtype=dtype), w, b, a, zi, lambda u: tdf2(b, a, u, zi_ * u[0], dtype)[0])


def butterworth_segmented(X, width, order, S):
    """The device's order of operations in float64 with segments of S elements of the padded signal (0: one segment)."""
    w, b, a, zi = butter_design(width, order)
    return _butterworth(np.asarray(X, dtype=np.float64), w, b, a, zi, lambda u: tdf2_segmented(b, a, u, zi, zi, S))


# ---- EWMA -------------------------------------------------------------------------------------------------------------------
def _check_finite(X):
    if not np.isfinite(np.asarray(X, dtype=np.float64)).all():
        raise ValueError("Input contains NaN, infinity or a value too large")


def _min_periods(y, min_periods):
    y[:max(int(min_periods) - 1, 0)] = np.nan
    return y


def ewma(X, alpha, adjust=True, min_periods=0, dtype=LD):
    """sum_i q^i x_{t-i} / sum_i q^i (adjust) or y_0 = x_0, y_t = q y_{t-1} + alpha x_t; q = 1 - alpha (rounded in float64
    first, as every float64 implementation has it); the first min_periods - 1 rows NaN."""
    _check_finite(X)
    X = np.asarray(X, dtype=dtype)
    q = dtype(1.0 - alpha)
    y = np.empty(X.shape, dtype=dtype)
    if adjust:
        num = np.zeros(X.shape[1], dtype=dtype)
        den = dtype(0)
        for t in range(X.shape[0]):
            num = q * num + X[t]
            den = q * den + 1
            y[t] = num / den
    else:
        al = dtype(alpha)
        for t in range(X.shape[0]):
            y[t] = X[t] if t == 0 else q * y[t - 1] + al * X[t]
    return _min_periods(y, min_periods)


def ewma_segmented(X, alpha, adjust=True, min_periods=0, S=0):
    """The device's order in float64."""
    _check_finite(X)
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[0]
    q = 1.0 - alpha
    a = np.array([1.0, -q])
    if not adjust:
        return _min_periods(tdf2_segmented([alpha, 0.0], a, X, [q], [q], S), min_periods)
    num = tdf2_segmented([1.0, 0.0], a, X, [0.0], [0.0], S)
    S = S if S and S < n else n
    den = np.empty(n)
    for j in range(-(-n // S)):
        d = float((1 - LD(q) ** (j * S)) / LD(alpha))
        for t in range(j * S, min((j + 1) * S, n)):
            d = q * d + 1.0
            den[t] = d
    return _min_periods(num / den[:, None], min_periods)


def double_ewma(X, alpha, adjust=True, min_periods=0, dtype=LD, S=None):
    """(fwd + bwd) / 2 with bwd the EWMA of the reversed rows, not reversed back (the reference's recipe)."""
    X = np.asarray(X)
    if S is None:
        f, bk = ewma(X, alpha, adjust, min_periods, dtype), ewma(X[::-1], alpha, adjust, min_periods, dtype)
    else:
        f, bk = ewma_segmented(X, alpha, adjust, min_periods, S), ewma_segmented(X[::-1], alpha, adjust, min_periods, S)
    return (f + bk) / 2
