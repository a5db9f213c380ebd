"""tests/nystroem_ref.py -- numpy restatement of the kernel feature map and the bound every GPU comparison uses.

THE MAP.  ``kernel_values`` and ``kernel_map`` are written from the formulas, not from scikit-learn's code:

    linear x.l | poly (g x.l + c0)^d | sigmoid tanh(g x.l + c0) | cosine x.l / (|x| |l|), a zero vector left as it is
    rbf exp(-g |x - l|_2^2) | laplacian exp(-g |x - l|_1)            out[i, :] = k(x_i, landmarks) . B - c

``rbf`` and ``laplacian`` take DIRECT differences (no |x|^2 + |l|^2 - 2 x.l), every sum runs in ``np.longdouble``
(64-bit mantissa, unit roundoff 2^-64) and the result is rounded to float64 once.  tests/test_nystroem_ref.py holds this
file to scikit-learn's ``pairwise_kernels`` and ``Nystroem`` on float64.

THE BOUND (``bound``), per element, derived here rather than fitted.  The device evaluates the map in float64 for both row
dtypes (float32 rows are widened exactly), u = 2^-53, and rounds the result once to the output dtype, u_out
(2^-24 for float32 output, 0 extra for float64 output: that rounding is one of the u's counted below).  Standard model
fl(a op b) = (a op b)(1 + d), |d| <= u; a sum of m products in ANY order has error <= m u sum |terms| to first order
(Higham, Accuracy and Stability, 3.1 and 3.5) -- the MFMA's association in groups of four is covered.

  1. The kernel's argument.  s = x.l over F products: |ds| <= F u S, S = sum_f |x_f l_f|.
       linear     k = s                       |dk| <= F u S
       poly       z = g s + c0 (2 more ops)   |dz| <= (F + 2) u Z, Z = g S + |c0|;  k = z^d: |dk| <= |d| |z|^(d-1) |dz| + 2 u |k|
       sigmoid    same z;  |dk| <= (1 - k^2) |dz| + 2 u |k|           (pow, tanh, exp: correctly rounded to within 2 u)
       cosine     |x|, |l| from F squares and a sqrt each: relative error (F + 2) u / 2 each;  the normalised product:
                  |dk| <= F u S / (|x| |l|) + (F + 5) u |k|
       rbf        the device forms |x|^2 + |l|^2 - 2 x.l: three sums of F products and two additions, error
                  <= (F + 2) u (|x|^2 + |l|^2 + 2 S) <= (F + 2) u (|x| + |l|)^2 -- the magnitude BEFORE the cancellation;
                  times g, one more op, then exp:  |dk| <= k [(F + 3) u g (|x| + |l|)^2 + 2 u]
       laplacian  F differences and F additions: |dk| <= k [(F + 2) u g |x - l|_1 + 2 u]
     All six are covered by   |dk_il| <= (F + 8) u a_il   with the "argument magnitude" a_il >= |k_il|:
       linear S | poly |d| |z|^(d-1) Z + |k| | sigmoid (1 - k^2) Z + |k| | cosine S / (|x| |l|) + |k|
       rbf k (g (|x| + |l|)^2 + 1) | laplacian k (g |x - l|_1 + 1)
     (a_il = gA_il |k_il| in the notation "gA = magnitude of the argument before cancellation"; for linear and cosine
     gA_il = S / |x.l|, which is 1 only when no product cancels -- so the per-element a_il is kept instead of a per-row gA.)
  2. The second product.  L products with the computed k, then - c_j: <= (L + 2) u sum_l |k_il| |B_lj| + u |c_j|.
  3. The final rounding: u_out |ref_ij|.
  A factor 4 absorbs the second-order terms, the longdouble reference's own 2^-64-class error and the float64 rounding of
  the reference:

     |out_ij - ref_ij| <= 4 u [ sum_l ((F + 8) a_il + (L + 2) |k_il|) |B_lj| + |c_j| ] + u_out |ref_ij|

THE NORMALISATION (``normalization_tolerance``).  M = K^(-1/2) of a symmetric positive definite basis kernel.  The Frechet
derivative of K -> K^(-1/2) is bounded in the 2-norm by 1 / (2 s_min^(3/2)); both sides (device basis kernel + LAPACK SVD
here, scikit-learn + LAPACK SVD in the golden) carry the SVD's backward error, taken as L u s_max each, and the device's
basis kernel the element errors of step 1 in Frobenius norm:

     max |M_dev - M_gold| <= (4 (F + 8) u |a|_F + 2 L u s_max) / (2 s_min^(3/2))
"""
import numpy as np

KERNELS = ("linear", "poly", "sigmoid", "cosine", "rbf", "laplacian")
U64 = 2.0 ** -53
U32 = 2.0 ** -24
LD = np.longdouble


def resolve(kernel, gamma, coef0, degree, F):
    return (1.0 / F if gamma is None else float(gamma), 1.0 if coef0 is None else float(coef0),
            3.0 if degree is None else float(degree))


def _parts(X, Lm):
    """longdouble x.l, S = sum |x_f l_f|, |x|, |l|, |x - l|_2^2, |x - l|_1."""
    X = np.asarray(X, dtype=LD)
    Lm = np.asarray(Lm, dtype=LD)
    dot = X @ Lm.T
    S = np.abs(X) @ np.abs(Lm).T
    nx = np.sqrt((X * X).sum(1))
    nl = np.sqrt((Lm * Lm).sum(1))
    d2 = np.empty((X.shape[0], Lm.shape[0]), dtype=LD)
    d1 = np.empty_like(d2)
    for j in range(Lm.shape[0]):
        diff = X - Lm[j]
        d2[:, j] = (diff * diff).sum(1)
        d1[:, j] = np.abs(diff).sum(1)
    return dot, S, nx, nl, d2, d1


def kernel_values(X, Lm, kernel, gamma=None, coef0=None, degree=None, with_magnitude=False):
    """K[i, l] in longdouble (and a_il of the bound)."""
    F = np.shape(X)[1]
    g, c0, d = resolve(kernel, gamma, coef0, degree, F)
    dot, S, nx, nl, d2, d1 = _parts(X, Lm)
    with np.errstate(all="ignore"):
        if kernel == "linear":
            K, a = dot, S
        elif kernel == "poly":
            z = g * dot + c0
            K = z ** LD(d)
            a = abs(d) * np.abs(z) ** LD(d - 1) * (g * S + abs(c0)) + np.abs(K)
        elif kernel == "sigmoid":
            z = g * dot + c0
            K = np.tanh(z)
            a = (1 - K * K) * (g * S + abs(c0)) + np.abs(K)
        elif kernel == "cosine":
            den = np.where(nx == 0, 1, nx)[:, None] * np.where(nl == 0, 1, nl)[None, :]
            K = dot / den
            a = S / den + np.abs(K)
        elif kernel == "rbf":
            K = np.exp(-g * d2)
            a = K * (g * (nx[:, None] + nl[None, :]) ** 2 + 1)
        elif kernel == "laplacian":
            K = np.exp(-g * d1)
            a = K * (g * d1 + 1)
        else:
            raise ValueError(kernel)
    return (K, a) if with_magnitude else K


def kernel_map(X, Lm, B, c=None, kernel="rbf", gamma=None, coef0=None, degree=None):
    """(ref float64 [n, P], bound terms) -- see ``bound``."""
    K, a = kernel_values(X, Lm, kernel, gamma, coef0, degree, with_magnitude=True)
    Bl = np.asarray(B, dtype=LD)
    out = K @ Bl
    cabs = 0.0
    if c is not None:
        out = out - np.asarray(c, dtype=LD)
        cabs = np.abs(np.asarray(c, dtype=np.float64))
    F, L = np.shape(X)[1], np.shape(Lm)[0]
    core = ((F + 8) * a + (L + 2) * np.abs(K)) @ np.abs(Bl)
    return np.asarray(out, dtype=np.float64), (np.asarray(core, dtype=np.float64), cabs)


def bound(ref, terms, out_dtype, extra=0.0):
    """Per-element bound of the module docstring; ``extra`` adds a derived term (e.g. a perturbed B)."""
    core, cabs = terms
    u_out = U32 if np.dtype(out_dtype) == np.float32 else 0.0
    return 4 * U64 * (core + cabs) + u_out * np.abs(ref) + extra


def check(out, ref, terms, out_dtype, what="", extra=0.0):
    """Assert the bound; prints the worst ratio first."""
    out = np.asarray(out, dtype=np.float64)
    b = bound(ref, terms, out_dtype, extra)
    err = np.abs(out - ref)
    ok = (err <= b) | (np.isnan(out) & np.isnan(ref))
    with np.errstate(all="ignore"):
        ratio = np.nanmax(np.where(b > 0, err / b, np.where(err > 0, np.inf, 0.0))) if err.size else 0.0
    print("%s: max error / bound = %.3g, max |error| = %.3g" % (what, ratio, np.nanmax(err) if err.size else 0.0))
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    assert ok.all(), "%s: %d of %d elements outside the bound (worst ratio %.3g)" % (what, (~ok).sum(), ok.size, ratio)
    return ratio


def normalization(K):
    """The reference's normalization_ (kernel_approximation.py:97-99) of a basis kernel."""
    import scipy.linalg
    U, S, V = scipy.linalg.svd(np.asarray(K, dtype=np.float64))
    S = np.maximum(S, 1e-12)
    return np.dot(U / np.sqrt(S), V)


def condition(K):
    s = np.linalg.svd(np.asarray(K, dtype=np.float64), compute_uv=False)
    return s[-1] / s[0], s


def normalization_tolerance(Lm, kernel, gamma=None, coef0=None, degree=None):
    K, a = kernel_values(Lm, Lm, kernel, gamma, coef0, degree, with_magnitude=True)
    F, L = np.shape(Lm)[1], np.shape(Lm)[0]
    _, s = condition(K)
    aF = float(np.sqrt((np.asarray(a, dtype=np.float64) ** 2).sum()))
    return (4 * (F + 8) * U64 * aF + 2 * L * U64 * s[0]) / (2 * s[-1] ** 1.5)


# ---- case lists (shared by the CPU and the GPU tier) -------------------------------------------------------------------
def data(seed, n, F, L, dtype=np.float64, shift=0.0):
    """Standard-normal rows and landmarks (+ shift), rounded to dtype."""
    rs = np.random.RandomState(seed)
    X = (rs.randn(n, F) + shift).astype(dtype)
    Lm = (rs.randn(L, F) + shift).astype(dtype)
    return X, Lm


def params(kernel):
    """Kernel parameters of the conformance cases: scikit-learn's defaults (gamma = 1 / F, coef0 = 1, degree = 3)."""
    return dict(kernel=kernel, gamma=None, coef0=None, degree=None)


def est_seed(kernel, F, L):
    return 1000 * KERNELS.index(kernel) + 10 * F + L


def nystroem_sequences():
    """Three trajectories (40, 1 and 25 rows of 5 features) for the random-basis case."""
    rs = np.random.RandomState(11)
    return [rs.randn(n, 5) for n in (40, 1, 25)]


MAP_F = (1, 3, 4, 5, 17)        # crosses the MFMA depth step of 4
MAP_L = (1, 15, 16, 17, 33)     # crosses the 16-landmark tile
# (F, L) of the estimator conformance cases: well-conditioned basis kernels (sigma_min / sigma_max > 1e-6 is asserted where
# each is built); linear and cosine have rank <= F, so theirs keep L <= F
EST_CASES = {"rbf": ((3, 16), (7, 33), (16, 64)), "laplacian": ((3, 16), (7, 33)), "poly": ((16, 8),), "sigmoid": ((7, 5),),
             "linear": ((16, 8), (40, 33)), "cosine": ((16, 8), (40, 33))}


def double_well(seed, n, n_features=3):
    """Brownian dynamics in the 1-D double well V(x) = (x^2 - 1)^2 at kT = 1 (Euler-Maruyama, D dt = 0.01: the pure-numpy
    recipe of the reference's brownian1d example with a quartic well), observed through n_features noisy nonlinear channels:
    one slow mode, the hop between the wells, which a linear tICA of the even channels cannot see."""
    rs = np.random.RandomState(seed)
    x = np.empty(n)
    x[0] = -1.0
    Ddt = 0.01
    noise = rs.randn(n) * np.sqrt(2 * Ddt)
    for t in range(1, n):
        xp = x[t - 1]
        x[t] = xp - Ddt * 4 * xp * (xp * xp - 1) + noise[t]
    cols = [x, x * x - 1, np.cos(2 * x)][:n_features]
    return np.stack(cols, axis=1) + 0.05 * rs.randn(n, len(cols))


def ktica_sequences():
    """Three trajectories (400, 250 and 150 frames) of the double well and 24 landmarks drawn from them."""
    lens = (400, 250, 150)
    seqs = [double_well(100 + i, n) for i, n in enumerate(lens)]
    allrows = np.concatenate(seqs)
    idx = np.random.RandomState(7).permutation(len(allrows))[:24]
    return seqs, np.ascontiguousarray(allrows[np.sort(idx)])


KTICA_KW = dict(n_components=4, lag_time=3, kernel="rbf", gamma=2.0)
