"""tests/divergence_ref.py -- TEST INFRASTRUCTURE: the KL-family divergences and MVCA restated in numpy.

Written from the definition, not from the reference's text.

DEFINITION (all arithmetic float64 in the reference; here longdouble for the values, float64 for the tests on products):
    kl(P, Q)  = max(sum_k [fl64(P_k * Q_k) != 0] P_k log(P_k / Q_k), 0)      a NaN sum stays NaN
    sym_kl    = kl(P, Q) + kl(Q, P)
    js        = 0.5 kl(P, M) + 0.5 kl(Q, M),   M_k = (P_k + Q_k) / 2  (rounded to float64 for the product test)
    js_metric = sqrt(js)

``pairs`` is the longdouble restatement over paired rows, with the bound; ``emulate64`` is the float64 evaluation in the
device's order (sequential sums in ascending column, numpy's log and division); ``cdist`` / ``pdist`` arrange either over
all pairs.

THE BOUND, per element.  u = 2^-53.  One included term t = p log(p / q) is computed as fl(p * LOG(fl(p / q))):
  * the division rounds the ratio by at most u relative (js: the ratio's denominator M carries another u), which moves
    the logarithm by at most c u absolutely, c = 1 (kl, sym_kl) or 2 (js): c u |p| on the term;
  * the device's log is within E units in the last place of the true value, an ulp being at most 2 u |log|: 2 E u |t|;
  * the product rounds by u |t|; a subnormal product, or one whose ratio was a subnormal (rounded far more coarsely
    than u, under a p that is itself tiny), is off by at most two subnormal spacings 2^-1074 instead.
The sum runs in the reference's order, so against exact arithmetic its n_inc - 1 additions add at most
(n_inc - 1) u sum|t| (Higham, lemma 3.1, first order).  Hence
    b_kl = u (c sum_inc |p| + (2 E + n_inc) sum_inc |t|) + 2 n_inc 2^-1074,
through the clamp unchanged (max(., 0) is 1-Lipschitz), b_sym = b(P,Q) + b(Q,P) + u |sym|,
b_js = (b(P,M) + b(Q,M)) / 2 + 2 u |js|, and through the square root |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(a),
sqrt|a - b|):  b_metric = min(b_js / sqrt(js), sqrt(b_js)) + 2 u |metric|.  A factor 1 + 2^-20 covers the second-order
terms.  E is LOG_ULP: the error of the device's log measured on the card by scripts/divergence_probe.py
(profiles/divergence_bounds.txt), times 2 for the arguments that probe did not sample.

A float64 ratio that overflows to inf or underflows to zero is part of the definition (the reference's arithmetic is
float64): the restatement keeps it, so the term is +-inf there as in the reference and on the device.
"""
import numpy as np

U = 2.0 ** -53
TINY = 2.0 ** -1074
KINDS = ("kl_divergence", "sym_kl_divergence", "js_divergence", "js_metric")
SYMMETRIC = KINDS[1:]
LOG_ULP_MEASURED = 0.6377   # profiles/divergence_bounds.txt: LOG_ULP_MEASURED
LOG_ULP = 2.0 * LOG_ULP_MEASURED
LD = np.longdouble


# ---- the generator of transition-like matrices with planted blocks ------------------------------------------------------
def gen(n, blocks, seed, sparse=0.5):
    r = np.random.RandomState(seed); C = r.rand(n, n) * 0.02
    C[r.rand(n, n) < sparse] = 0.0; b = n // blocks
    for k in range(blocks): C[k*b:(k+1)*b, k*b:(k+1)*b] += r.rand(b, b)
    C = C + C.T + np.eye(n) * 1e-3; return C / C.sum(1, keepdims=True)


GEN_CASES = ((33, 3, 0), (65, 4, 1), (130, 5, 2), (257, 6, 3))
GOLDEN_GEN = {"gen33": (33, 3, 0), "gen65": (65, 4, 1)}     # the systems of tests/golden/mvca_golden.npz


def four_state_labels(seed=0, n=250):
    """A label sequence over four microstates with two obvious macrostates: stretches of n frames that hop at random
    between states 0 and 1 alternate with stretches that hop between 2 and 3."""
    r = np.random.RandomState(seed)
    return np.concatenate([base + r.randint(2, size=n) for base in (0, 2, 0, 2)])


def golden_pair_rows():
    """The rows the stored outputs of the reference's pair functions were computed on."""
    A = np.concatenate([rows(5, 7, 100), special_rows(7)[[0, 2, 4]]])
    B = np.concatenate([rows(5, 7, 101), special_rows(7)[[1, 2, 5]]])
    return A, B


def rows(n, m, seed, dt=np.float64, zeros=0.4, normalise=True):
    """n non-negative rows of m columns with many exact zeros."""
    r = np.random.RandomState(seed)
    X = r.rand(n, m)
    X[r.rand(n, m) < zeros] = 0.0
    if normalise:
        s = X.sum(1, keepdims=True)
        X = X / np.where(s == 0, 1.0, s)
    else:
        X = X * r.uniform(0.1, 50.0, size=(n, 1))
    return np.ascontiguousarray(X.astype(dt))


def special_rows(m, dt=np.float64):
    """Rows that meet the definition's corners: all zeros, one entry, underflowing products (1e-200 against 1e-200),
    the smallest subnormal against 1 (the ratio is exact) and an un-normalised row.  Subnormals exist only in float64."""
    X = np.zeros((6, m), dtype=np.float64)
    X[1, 0] = 1.0
    X[2, :] = 1e-200 if dt == np.float64 else 1e-30
    X[3, :] = 1.0
    X[3, m // 2] = 5e-324 if dt == np.float64 else 1e-45
    X[4, :] = np.arange(1, m + 1)
    X[5, ::2] = 0.25
    return np.ascontiguousarray(X.astype(dt))


# ---- longdouble restatement with the bound -----------------------------------------------------------------------------
def _kl_part(P, Q, c):
    """(sum in longdouble, bound of the float64 sum in device order) of kl's sum over paired rows, before the clamp.
    P, Q: float64 (r, m); the product test is float64's."""
    with np.errstate(all="ignore"):
        inc = (P * Q) != 0
        Pl, Ql = P.astype(LD), Q.astype(LD)
        r64 = np.where(inc, P / Q, 1.0)
        normal = np.isfinite(r64) & (r64 != 0)          # a float64 ratio that overflows or underflows to zero is kept:
        ratio = np.where(normal, Pl / Ql, r64.astype(LD))   # log gives +-inf there, in the reference and on the device
        t = np.where(inc, Pl * np.log(np.where(inc, ratio, LD(1))), LD(0))
        s = t.sum(axis=1)
        n_inc = inc.sum(axis=1)
        at = np.abs(t).sum(axis=1).astype(np.float64)
        ap = np.where(inc, np.abs(P), 0.0).sum(axis=1)
        b = U * (c * ap + (2.0 * LOG_ULP + n_inc) * at) + 2.0 * n_inc * TINY
    return s, b


def _clamp(s):
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(s), s, np.maximum(s, LD(0)))


def pairs(P, Q, kind):
    """(values float64, bounds float64) of kind(P[r], Q[r]) over paired rows."""
    assert kind in KINDS
    P = np.atleast_2d(np.asarray(P)).astype(np.float64)
    Q = np.atleast_2d(np.asarray(Q)).astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == "kl_divergence":
            s, b = _kl_part(P, Q, 1.0)
            v = _clamp(s)
        elif kind == "sym_kl_divergence":
            s1, b1 = _kl_part(P, Q, 1.0)
            s2, b2 = _kl_part(Q, P, 1.0)
            v = _clamp(s1) + _clamp(s2)
            b = b1 + b2 + U * np.abs(v.astype(np.float64))
        else:
            M = (P + Q) / 2.0
            s1, b1 = _kl_part(P, M, 2.0)
            s2, b2 = _kl_part(Q, M, 2.0)
            v = LD(0.5) * _clamp(s1) + LD(0.5) * _clamp(s2)
            b = 0.5 * (b1 + b2) + 2.0 * U * np.abs(v.astype(np.float64))
            if kind == "js_metric":
                js = v.astype(np.float64)
                v = np.sqrt(v)
                b = np.minimum(np.where(js > 0, b / np.sqrt(np.where(js > 0, js, 1.0)), np.inf), np.sqrt(b)) \
                    + 2.0 * U * np.abs(v.astype(np.float64))
        return v.astype(np.float64), b * (1.0 + 2.0 ** -20)


def emulate64(P, Q, kind):
    """The float64 evaluation in the device's order: sequential sums in ascending column (np.add.accumulate), numpy's log
    and division in place of the device's."""
    P = np.atleast_2d(np.asarray(P)).astype(np.float64)
    Q = np.atleast_2d(np.asarray(Q)).astype(np.float64)

    def part(A, B):
        with np.errstate(all="ignore"):
            inc = (A * B) != 0
            t = np.where(inc, A * np.log(np.where(inc, A / B, 1.0)), 0.0)
            s = np.add.accumulate(t, axis=1)[:, -1]
            return np.where(np.isnan(s), s, np.maximum(s, 0.0))

    with np.errstate(all="ignore"):
        if kind == "kl_divergence":
            return part(P, Q)
        if kind == "sym_kl_divergence":
            return part(P, Q) + part(Q, P)
        M = (P + Q) / 2.0
        js = 0.5 * part(P, M) + 0.5 * part(Q, M)
        return js if kind == "js_divergence" else np.sqrt(js)


def cdist(XA, XB, kind, fn=pairs):
    XA, XB = np.asarray(XA), np.asarray(XB)
    i, j = np.meshgrid(np.arange(len(XA)), np.arange(len(XB)), indexing="ij")
    r = fn(XA[i.ravel()], XB[j.ravel()], kind)
    if isinstance(r, tuple):
        return tuple(x.reshape(len(XA), len(XB)) for x in r)
    return r.reshape(len(XA), len(XB))


def pdist(X, kind, fn=pairs):
    X = np.asarray(X)
    i, j = np.triu_indices(len(X), 1)
    return fn(X[i], X[j], kind)


def assert_within(got, want, bound, what=""):
    """|got - want| <= bound elementwise; NaN where want is NaN; equal where want is infinite."""
    got, want, bound = np.asarray(got, dtype=np.float64), np.asarray(want), np.asarray(bound)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN pattern differs" % what
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), "%s: infinite values differ" % what
    ok = ~(nan | inf)
    with np.errstate(invalid="ignore"):
        err = np.abs(got[ok] - want[ok])
        bad = err > bound[ok]
    if np.any(bad):
        k = int(np.argmax(err - bound[ok]))
        raise AssertionError("%s: %d of %d outside the bound; worst error %.3e against bound %.3e (value %.6e)"
                             % (what, int(bad.sum()), int(ok.sum()), err[k], bound[ok][k], want[ok][k]))
    return float(np.max(err / np.maximum(bound[ok], TINY))) if np.any(ok) else 0.0


# ---- MVCA from the pieces ----------------------------------------------------------------------------------------------
def squareform(D, n):
    S = np.zeros((n, n), dtype=np.float64)
    iu = np.triu_indices(n, 1)
    S[iu] = D
    S.T[iu] = D
    return S


def landmark_indices(n, n_landmarks, strategy="stride", random_state=None):
    if n_landmarks is None:
        return np.arange(n)
    if strategy == "random":
        return np.random.RandomState(random_state).randint(n, size=n_landmarks)
    return np.arange(n)[::n // n_landmarks][:n_landmarks]


LINKAGES = ("single", "complete", "average", "ward")


def mvca(T, n_macrostates, kind="js_metric", n_landmarks=None, strategy="stride", random_state=None, fn=pairs,
         linkage_name="ward"):
    """The restated MVCA (``linkage_name='ward'``) or, with another linkage, the restated LandmarkAgglomerative under a
    divergence metric.  Distances: ``fn`` (pairs -> longdouble values rounded to float64, with bounds; emulate64 ->
    float64 in device order).  Linkage: scipy's on the condensed landmark matrix; labels: fcluster maxclust; prediction:
    the linkage's pooling rule over each cluster's landmarks in ascending index (sequential sums), strict < over ascending
    cluster id.  ``eps``: how far another float64 evaluation, from distances within their bounds of these, may lie from
    ``values`` -- the distances' bounds carried through the rule, plus the rounding of the sums as in
    landmark_ref.pooled_eps."""
    from scipy.cluster.hierarchy import fcluster, linkage
    T = np.asarray(T, dtype=np.float64)
    idx = landmark_indices(len(T), n_landmarks, strategy, random_state)
    Lm = T[idx]
    r = pdist(Lm, kind, fn)
    D, DB = r if isinstance(r, tuple) else (r, np.zeros_like(r))
    Z = linkage(D, linkage_name)
    lab = fcluster(Z, t=n_macrostates, criterion="maxclust") - 1
    L = len(idx)
    i, j = np.triu_indices(L, 1)
    within = np.zeros(n_macrostates)
    within_b = np.zeros(n_macrostates)
    for c in range(n_macrostates):
        sel = (lab[i] == c) & (lab[j] == c)
        d = D[sel]
        if len(d):
            within[c] = np.add.accumulate(d * d)[-1]
            within_b[c] = (2.0 * d * DB[sel] + DB[sel] ** 2).sum()
    r = cdist(T, Lm, kind, fn)
    X, XB = (r if isinstance(r, tuple) else (r, np.zeros_like(r)))
    vals = np.full((len(T), n_macrostates), np.nan)
    eps = np.zeros((len(T), n_macrostates))
    present = np.zeros(n_macrostates, dtype=bool)
    for c in range(n_macrostates):
        cols = np.flatnonzero(lab == c)
        if not len(cols):
            continue
        present[c] = True
        m = float(len(cols))
        x, xb = X[:, cols], XB[:, cols]
        if linkage_name == "single":
            vals[:, c], eps[:, c] = x.min(axis=1), xb.max(axis=1)
        elif linkage_name == "complete":
            vals[:, c], eps[:, c] = x.max(axis=1), xb.max(axis=1)
        elif linkage_name == "average":
            vals[:, c] = np.add.accumulate(x, axis=1)[:, -1] / m
            eps[:, c] = xb.sum(axis=1) / m + 2.0 * m * U * np.abs(vals[:, c])
        else:
            q = np.add.accumulate(x * x, axis=1)[:, -1]
            norm = m * (m + 1.0) / 2.0
            vals[:, c] = (m * q - within[c]) / norm
            dq = (2.0 * x * xb + xb * xb).sum(axis=1)
            p = m * (m - 1.0) / 2.0
            eps[:, c] = (m * dq + within_b[c]) / norm \
                + U * (2.0 * (m + 2.0) * m * q + 2.0 * (p + 1.0) * within[c] + 4.0 * np.abs(vals[:, c]) * norm) / norm
    best = np.full(len(T), np.inf)
    pred = np.zeros(len(T), dtype=np.int64)
    for c in np.flatnonzero(present):
        mask = vals[:, c] < best
        best[mask] = vals[mask, c]
        pred[mask] = c
    return {"Z": Z, "D": D, "DB": DB, "landmark_labels": lab, "predict": pred, "values": vals, "eps": eps, "present": present,
            "within": within, "indices": idx}


def height_tolerance(D, DB, n):
    """Relative tolerance between the merge heights of two linkages of matrices that differ by at most DB: the largest
    relative bound of a distance, plus landmark_ref.height_bound's 8 n u for the chain of float64 updates."""
    with np.errstate(all="ignore"):
        rel = np.where(D > 0, DB / np.where(D > 0, D, 1.0), 0.0)
    return 8.0 * n * U + 2.0 * float(np.max(rel)) if len(D) else 0.0


def decided_rows(values, present, eps, slack=0.0):
    """Rows whose label every evaluation within eps must agree on (the best beats every other cluster by more than the
    two bounds)."""
    v = np.where(present[None, :], values, np.inf)
    e = np.where(present[None, :], eps, 0.0)
    best = np.argmin(v, axis=1)
    r = np.arange(len(v))
    gap = v - v[r, best][:, None] - (e + e[r, best][:, None]) - slack
    gap[r, best] = np.inf
    return np.all(gap > 0, axis=1)


def relative_gap(heights):
    h = np.sort(np.asarray(heights, dtype=np.float64))
    return float(np.min(np.diff(h) / h[1:]))
