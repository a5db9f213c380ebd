"""tests/landmark_ref.py -- TEST INFRASTRUCTURE: landmark agglomerative clustering restated in numpy.

Written from the description of the algorithm, not from the reference's text.

LINKAGE.  Plain global-minimum agglomeration of n observations on a square float64 copy of the condensed matrix D
(entry (i, j), i < j, at ``n*i - i(i+1)/2 + j - 1 - i``).  Every observation starts as an active slot of size 1.  Each of
the n - 1 steps picks the active pair (i < j) of lowest distance -- at a tie the lowest row slot, then the lowest column
slot: ``np.argmin`` over the row-major upper triangle --, writes Z's row (id_a < id_b, height, size; observations are
0 .. n-1 and the cluster made at step s is n + s: scipy's convention), retires slot i, lets the merged cluster live on in
slot j, and gives every other active slot k, with a = D[i,k], b = D[j,k] and sizes as float64,
    single    min(a, b)              complete   max(a, b)              average   (ni*a + nj*b)/(ni + nj)
    ward      t = 1.0/(ni + nj + nk);   sqrt((ni + nk)*t*a*a + (nj + nk)*t*b*b - nk*t*dij*dij)
every product and sum left to right as written.  The updates are vectorised over k: elementwise numpy operations round
like the scalar ones.

WITHIN-CLUSTER SUMS.  Per cluster the float64 sum of d*d over the condensed entries whose two ends carry its label,
added in condensed order (``np.add.accumulate``: sequential by definition).

POOLED PREDICT.  From the exact N x L distances (the project's C oracle of libdistance): per cluster, over its landmarks
in ascending landmark index, min / max (numpy's: a NaN stays), the sequential sum of d divided by the count, or
``(m * sequential sum of d*d - intra) / (m*(m+1)/2)``; then a running strict ``<`` over the clusters in ascending id from
(+inf, label 0), clusters without a landmark skipped.

BOUNDS.  u = 2^-53.  Each is derived in the docstring of its function below.
"""
import functools

import numpy as np

U = 2.0 ** -53
METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "canberra", "braycurtis", "hamming", "jaccard")
LINKAGES = ("single", "complete", "average", "ward")
DT = {"f32": np.float32, "f64": np.float64}


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.libdistance_oracle import Oracle
    return Oracle()


# ---- inputs shared by the golden generator and the tests, regenerated from seeds ---------------------------------------
def cloud(n, m, seed, dt=np.float64, metric="euclidean"):
    X = np.random.RandomState(seed).randn(n, m)
    if metric in ("hamming", "jaccard"):
        X = np.rint(X)
    return np.ascontiguousarray(X.astype(dt))


def walk(n=3000, m=5, seed=3, dt=np.float32):
    """The golden input: a random walk, converted to the rows' type."""
    return np.ascontiguousarray(np.cumsum(np.random.RandomState(seed).randn(n, m), axis=0).astype(dt))


def golden_sequences(dt=np.float32):
    """The golden walk cut into four ragged trajectories (separate allocations)."""
    X = walk(dt=dt)
    cuts = [0, 700, 1900, 1903, 3000]
    return [np.array(X[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]


GOLDEN_K = 7
GOLDEN_LANDMARKS = 120
# (name, linkage, dtype, landmark_strategy, n_landmarks, rows used, ward_predictor); the random seed is found by the generator
GOLDEN_CASES = tuple(
    [("stride_%s_%s" % (lk, dn), lk, dn, "stride", GOLDEN_LANDMARKS, 3000, "ward") for lk in LINKAGES for dn in ("f32", "f64")]
    + [("random_%s_%s" % (lk, dn), lk, dn, "random", GOLDEN_LANDMARKS, 3000, "ward")
       for lk, dn in (("single", "f64"), ("complete", "f32"), ("average", "f32"), ("ward", "f64"))]
    + [("all_%s_%s" % (lk, dn), lk, dn, "stride", None, 300, "ward")
       for lk, dn in (("single", "f32"), ("complete", "f64"), ("average", "f64"), ("ward", "f32"))]
    + [("wardavg_ward_f32", "ward", "f32", "stride", GOLDEN_LANDMARKS, 3000, "average")])


def random_seed_without_duplicate(n=3000, n_landmarks=GOLDEN_LANDMARKS):
    """The lowest seed whose ``randint(n, size=n_landmarks)`` draws no row twice (most seeds do at these sizes)."""
    seed = 0
    while len(np.unique(np.random.RandomState(seed).randint(n, size=n_landmarks))) != n_landmarks:
        seed += 1
    return seed


# ---- condensed matrices ------------------------------------------------------------------------------------------------
def condensed_index(i, j, n):
    i, j = (int(i), int(j)) if i < j else (int(j), int(i))
    return n * i - i * (i + 1) // 2 + j - 1 - i


def squareform(D, n):
    S = np.zeros((n, n), dtype=np.float64)
    iu = np.triu_indices(n, 1)
    S[iu] = np.asarray(D, dtype=np.float64)
    S.T[iu] = S[iu]
    return S


def n_of(D):
    n = int(round((1 + np.sqrt(8 * len(D) + 1)) / 2.0))
    assert n * (n - 1) // 2 == len(D)
    return n


# ---- linkage -----------------------------------------------------------------------------------------------------------
def linkage(D, method):
    """Z ((n-1) x 4 float64) of the condensed matrix D; see the module docstring."""
    assert method in LINKAGES
    D = np.asarray(D, dtype=np.float64)
    n = n_of(D)
    assert n >= 2 and np.all(np.isfinite(D))
    S = squareform(D, n)
    W = np.full((n, n), np.inf)            # the candidates: upper triangle of the active slots
    iu = np.triu_indices(n, 1)
    W[iu] = S[iu]
    active = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.float64)
    ids = np.arange(n)
    Z = np.empty((n - 1, 4), dtype=np.float64)
    with np.errstate(all="ignore"):
        for s in range(n - 1):
            i, j = divmod(int(np.argmin(W)), n)   # first minimum in row-major order: lowest row, then lowest column
            dij = W[i, j]
            assert i < j and active[i] and active[j] and dij < np.inf
            ni, nj = size[i], size[j]
            Z[s] = (min(ids[i], ids[j]), max(ids[i], ids[j]), dij, ni + nj)
            active[i] = False
            W[i, :] = np.inf
            W[:, i] = np.inf
            k = np.flatnonzero(active)
            k = k[k != j]
            a, b, nk = S[i, k], S[j, k], size[k]
            if method == "single":
                v = np.minimum(a, b)
            elif method == "complete":
                v = np.maximum(a, b)
            elif method == "average":
                v = (ni * a + nj * b) / (ni + nj)
            else:
                t = 1.0 / (ni + nj + nk)
                v = np.sqrt((ni + nk) * t * a * a + (nj + nk) * t * b * b - nk * t * dij * dij)
            assert np.all(np.isfinite(v)), "a merged distance is not finite"
            S[j, k] = v
            S[k, j] = v
            lo, hi = k[k < j], k[k > j]
            W[lo, j] = v[k < j]
            W[j, hi] = v[k > j]
            size[j] = ni + nj
            ids[j] = n + s
    return Z


def height_bound(n):
    """Relative bound 8 n u between the heights of two correct float64 implementations of the average update.

    A height is the result of at most n - 2 nested updates.  One average update (ni*a + nj*b)/(ni + nj) is a convex
    combination of non-negative numbers -- no cancellation -- computed with two products, one sum and one division
    (ni + nj is exact): its result carries at most 4u relative on top of its operands' relative error, to first order.
    Along a chain of n - 2 updates that is 4(n - 2)u for one implementation, whatever equivalent form it uses (scipy
    divides once by the sum too), and 8(n - 2)u < 8 n u between two.  For ward the update subtracts, so no such
    argument bounds it; 8 n u is used all the same, and the test only accepts it together with the check that the
    reference's heights are further apart than twice the bound (so equal topology cannot be an accident).  single and
    complete select one of the inputs: their heights are compared bit for bit."""
    return 8.0 * n * U


def relative_gap(heights):
    """The smallest relative gap between two consecutive sorted heights."""
    h = np.sort(np.asarray(heights, dtype=np.float64))
    return float(np.min(np.diff(h) / h[1:]))


def labels_from_linkage(Z, n_clusters):
    from scipy.cluster.hierarchy import fcluster
    return fcluster(Z, t=n_clusters, criterion="maxclust") - 1


# ---- within-cluster sums -----------------------------------------------------------------------------------------------
def within(D, labels, n_clusters):
    """out[c] = sequential float64 sum, in condensed order, of d*d over the pairs inside cluster c."""
    D = np.asarray(D, dtype=np.float64)
    labels = np.asarray(labels)
    n = len(labels)
    assert len(D) == n * (n - 1) // 2
    i, j = np.triu_indices(n, 1)            # condensed order
    out = np.zeros(n_clusters, dtype=np.float64)
    for c in range(n_clusters):
        d = D[(labels[i] == c) & (labels[j] == c)]
        if len(d):
            out[c] = np.add.accumulate(d * d)[-1]
    return out


def pairs_within(labels, n_clusters):
    m = np.bincount(np.asarray(labels), minlength=n_clusters)[:n_clusters].astype(np.int64)
    return m * (m - 1) // 2


def within_bound(p):
    """Relative bound between two float64 sums of the same p squares added in ANY two orders.

    Each square is rounded once (relative u) and goes through at most p - 1 additions of non-negative numbers, so a
    computed sum is S(1 + theta) with |theta| <= g = p u / (1 - p u) (Higham, Accuracy and Stability, lemma 3.1) for
    the exact sum S, in any order.  Two such sums differ by at most 2 g S, and S <= |either| / (1 - g):
    |x - y| <= 2 g / (1 - g) |y|.  That is the issue's 2 p u up to a factor 1 + O(p u); p = 0 and p = 1 give 0 and
    one rounded product: bit-identical."""
    p = np.asarray(p, dtype=np.float64)
    g = p * U / (1.0 - p * U)
    return np.where(p <= 1, 0.0, 2.0 * g / (1.0 - g))


# ---- pooled predict ----------------------------------------------------------------------------------------------------
def exact_cdist(X, landmarks, metric):
    """N x L float64, libdistance's arithmetic (the C oracle)."""
    with np.errstate(all="ignore"):
        return _oracle().cdist(np.ascontiguousarray(X), np.ascontiguousarray(landmarks), metric)


def pooled_values(dists, landmark_labels, n_clusters, rule, intra=None):
    """N x K float64: cluster c's pooled value per row, NaN-filled columns for clusters without a landmark (see
    ``present``); sums are sequential in ascending landmark index."""
    assert rule in LINKAGES
    landmark_labels = np.asarray(landmark_labels)
    out = np.full((dists.shape[0], n_clusters), np.nan)
    present = np.zeros(n_clusters, dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(n_clusters):
            cols = np.flatnonzero(landmark_labels == c)
            if not len(cols):
                continue
            present[c] = True
            x = dists[:, cols]
            m = len(cols)
            if rule == "single":
                v = np.min(x, axis=1)
            elif rule == "complete":
                v = np.max(x, axis=1)
            elif rule == "average":
                v = np.add.accumulate(x, axis=1)[:, -1] / float(m)
            else:
                v = (float(m) * np.add.accumulate(x * x, axis=1)[:, -1] - intra[c]) / (float(m) * (float(m) + 1.0) / 2.0)
            out[:, c] = v
    return out, present


def argmin_strict(values, present):
    """(labels int64, winning values): running strict < in ascending cluster id from (+inf, 0)."""
    n = values.shape[0]
    best = np.full(n, np.inf)
    labels = np.zeros(n, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for c in np.flatnonzero(present):
            mask = values[:, c] < best
            best[mask] = values[mask, c]
            labels[mask] = c
    return labels, best


def pooled_predict(dists, landmark_labels, n_clusters, rule, intra=None):
    """(labels, winning pooled value, whether some ward value is negative)."""
    v, present = pooled_values(dists, landmark_labels, n_clusters, rule, intra)
    labels, best = argmin_strict(v, present)
    with np.errstate(invalid="ignore"):
        negative = bool(rule == "ward" and np.any(v[:, present] < 0))
    return labels, best, negative


def reference_pooled(dists, landmark_labels, n_clusters, rule, cardinality, intra):
    """The pooled values as the reference's numpy expressions give them (``np.mean`` / ``.sum`` add pairwise), with the
    intermediate quantities the bounds need: (values N x K, present, sums of squares N x K or None)."""
    landmark_labels = np.asarray(landmark_labels)
    out = np.full((dists.shape[0], n_clusters), np.nan)
    sq = np.full((dists.shape[0], n_clusters), np.nan) if rule == "ward" else None
    present = np.zeros(n_clusters, dtype=bool)
    for c in range(n_clusters):
        sel = landmark_labels == c
        if not np.any(sel):
            continue
        present[c] = True
        x = dists[:, sel]
        if rule == "single":
            out[:, c] = np.min(x, axis=1)
        elif rule == "complete":
            out[:, c] = np.max(x, axis=1)
        elif rule == "average":
            out[:, c] = np.mean(x, axis=1)
        else:
            m = cardinality[c]
            sq[:, c] = (x ** 2).sum(axis=1)
            out[:, c] = (m * sq[:, c] - intra[c]) / (m * (m + 1) / 2)
    return out, present, sq


def pooled_eps(values, present, rule, cardinality, intra=None, sq=None):
    """N x K: how far another correct float64 evaluation of the same pooled value may lie from ``values``.

    single / complete select one of the (bit-identical) distances: 0.

    average: the m distances are non-negative, so a float64 sum of them in any order is S(1 + theta), |theta| <=
    (m - 1)u to first order, and the division by m adds u: each evaluation is within m u of the exact value, two
    evaluations within 2 m u of each other:  eps = 2 m u value.

    ward: value = (m Q - I) / norm with Q the sum of m squares, I the within-cluster sum over p = m(m-1)/2 pairs and
    norm = m(m+1)/2 (exact).  Q computed: one rounding per square and at most m - 1 additions of non-negative terms,
    then the product by m: relative (m + 1)u, absolute (m + 1) u m Q.  I computed: relative p u in any order
    (within_bound), absolute p u I.  The subtraction and the division each add u of the result: 2 u |value|.  One
    evaluation is therefore within u ((m + 1) m Q + p I)/norm + 2 u |value| of the exact value and two are within
    twice that of each other; the issue's form rounds the two counts up by one, which covers the second-order terms:
        eps = u (2 (m + 2) m Q + 2 (p + 1) I + 4 |value| norm) / norm."""
    eps = np.zeros_like(values)
    for c in np.flatnonzero(present):
        m = float(cardinality[c])
        if rule == "average":
            eps[:, c] = 2.0 * m * U * np.abs(values[:, c])
        elif rule == "ward":
            p, norm = m * (m - 1.0) / 2.0, m * (m + 1.0) / 2.0
            eps[:, c] = U * (2.0 * (m + 2.0) * m * sq[:, c] + 2.0 * (p + 1.0) * intra[c] + 4.0 * np.abs(values[:, c]) * norm) / norm
    return eps


def decided_rows(values, present, eps):
    """Rows whose label every correct evaluation must agree on: the best value v1 (first at the minimum) satisfies
    v_c - v1 > eps_1 + eps_c for EVERY other cluster c -- in particular for the second best, the issue's criterion."""
    v = np.where(present[None, :], values, np.inf)
    e = np.where(present[None, :], eps, 0.0)
    best = np.argmin(v, axis=1)
    rows = np.arange(len(v))
    gap = v - v[rows, best][:, None] - (e + e[rows, best][:, None])
    gap[rows, best] = np.inf
    return np.all(gap > 0, axis=1)


# ---- the estimator's host logic ----------------------------------------------------------------------------------------
def landmark_indices(n, n_landmarks, strategy="stride", random_state=None):
    if n_landmarks is None:
        return np.arange(n)
    if strategy == "random":
        rs = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
        return rs.randint(n, size=n_landmarks)
    return np.arange(n)[::n // n_landmarks][:n_landmarks]


def estimator(X, n_clusters, n_landmarks=None, linkage_name="average", metric="euclidean", strategy="stride",
              random_state=None, ward_predictor="ward", predict=True):
    """fit (and predict on X) of the estimator, from the pieces above."""
    idx = landmark_indices(len(X), n_landmarks, strategy, random_state)
    landmarks = np.ascontiguousarray(X[idx])
    with np.errstate(all="ignore"):
        D = _oracle().pdist(landmarks, metric)
    Z = linkage(D, linkage_name)
    labels = labels_from_linkage(Z, n_clusters)
    r = {"Z": Z, "landmark_labels": labels, "landmarks": landmarks, "cardinality": np.bincount(labels),
         "within": within(D, labels, n_clusters),
         "centers": np.array([list(np.mean(landmarks[labels == i], axis=0)) for i in range(n_clusters)])}
    if predict:
        rule = ward_predictor if linkage_name == "ward" else linkage_name
        r["predict"], r["pooled"], r["negative"] = pooled_predict(exact_cdist(X, landmarks, metric), labels, n_clusters,
                                                                  rule, r["within"])
    return r
