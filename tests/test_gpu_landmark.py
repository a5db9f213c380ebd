"""GPU tier of landmark agglomerative clustering: msm_linkage / msm_linkage_fit_* / msm_landmark_within /
msm_landmark_predict_* / LandmarkAgglomerative against the numpy restatement (tests/landmark_ref.py, itself held to scipy
and to the reference's goldens by tests/test_landmark_ref.py) and against the golden file.

Z, predicted labels and winning pooled values are compared BIT FOR BIT with the restatement; the within-cluster sums
within 2 p u (two float64 sums of the same p squares in different orders), and two runs of them bit for bit; the estimator
against the goldens by the CPU tier's criteria.

Sizes are the smallest that reach each seam of the device code: the 256-thread workgroups of the linkage kernels (255,
256, 257), the 4 rows one workgroup of the refresh launch covers (3, 4, 5), the 64 lanes of a row scan (63, 64, 65), about
1,000 observations; for predict the 256 rows of a workgroup (the grid is one workgroup per 256 rows whatever N: there is
no second seam), the landmarks of one LDS tile (512 for narrow rows, 23 for 171 float64 columns), rows held in registers
or not (more than 32 float32 / 16 float64 columns), and rows wider than the tile (chunked features)."""
import ctypes as C
import functools
import os
import pickle
import warnings

import numpy as np
import pytest

import landmark_ref as R
from test_landmark_ref import check_fit_against_golden, check_predict_against_golden

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark_golden.npz")
SIZES = (2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1001)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def A():
    from msmbuilder_amd.cluster import agglomerative
    return agglomerative


def dev(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda")


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


@functools.lru_cache(maxsize=None)
def matrix(n, seed=0, metric="euclidean", integer=False):
    """(rows, condensed matrix by the C oracle): computed once, shared, never written to."""
    X = R.cloud(n, 3, seed)
    if integer:
        X = np.ascontiguousarray(np.random.RandomState(seed).randint(0, 4, (n, 2)).astype(np.float64))
    D = R._oracle().pdist(X, metric)
    X.setflags(write=False)
    D.setflags(write=False)
    return X, D


@functools.lru_cache(maxsize=None)
def ref_linkage(n, method, seed=0, metric="euclidean", integer=False):
    Z = R.linkage(matrix(n, seed, metric, integer)[1], method)
    Z.setflags(write=False)
    return Z


def lib_linkage(D, n, method, on_device=False, fill=-7.0):
    from msmbuilder_amd import _lib
    L = _lib.lib()
    _lib.ensure_device(0)
    Z = np.full((max(n - 1, 1), 4), fill)
    keep = dev(D) if on_device else np.ascontiguousarray(D)
    ptr = keep.data_ptr() if on_device else keep.ctypes.data
    rc = L.msm_linkage(C.c_void_p(ptr), n, method if isinstance(method, bytes) or method is None else method.encode(),
                       Z.ctypes.data, int(on_device))
    return rc, Z[:max(n - 1, 0)] if rc == 0 else Z


# ---- msm_linkage -------------------------------------------------------------------------------------------------------
def test_plans(gpu):
    out = (C.c_int64 * 2)()
    assert gpu.lib().msm_linkage_plan(out) == 0
    assert list(out) == [256, 4]   # the seams SIZES is built around


@pytest.mark.parametrize("method", R.LINKAGES)
@pytest.mark.parametrize("n", SIZES)
def test_linkage_sizes(gpu, n, method):
    X, D = matrix(n)
    Zr = ref_linkage(n, method)
    for on_device in (False, True):
        rc, Z = lib_linkage(D, n, method, on_device)
        assert rc == 0
        assert np.array_equal(bits(Z), bits(Zr)), "n=%d %s device=%d" % (n, method, on_device)


# (ward's update is only defined for Euclidean distances)
@pytest.mark.parametrize("metric,method", [("cityblock", lk) for lk in R.LINKAGES[:3]] + [("euclidean", lk) for lk in R.LINKAGES])
def test_linkage_exact_ties(gpu, metric, method):
    n = 70   # integer rows on a 4 x 4 grid: every distance is tied many times over, duplicate rows give zero heights
    X, D = matrix(n, 1, metric, True)
    Zr = ref_linkage(n, method, 1, metric, True)
    assert np.sum(Zr[:, 2] == 0.0) >= 10 and len(np.unique(Zr[:, 2])) < n // 2
    for on_device in (False, True):
        rc, Z = lib_linkage(D, n, method, on_device)
        assert rc == 0 and np.array_equal(bits(Z), bits(Zr))


def test_linkage_errors(gpu):
    from msmbuilder_amd import _lib
    X, D = matrix(65)
    for bad in (np.nan, np.inf, -np.inf):
        for pos in (0, 1000, len(D) - 1):
            Db = np.array(D)
            Db[pos] = bad
            for on_device in (False, True):
                rc, Z = lib_linkage(Db, 65, "average", on_device)
                assert rc == _lib.MSM_ERR_NONFINITE and np.all(Z == -7.0)
    rc, Z = lib_linkage(D, 1, "single")
    assert rc == _lib.MSM_ERR_INVALID and np.all(Z == -7.0)
    rc, Z = lib_linkage(D, 0, "single")
    assert rc == _lib.MSM_ERR_INVALID
    for method in ("centroid", "", None):
        rc, Z = lib_linkage(D, 65, method)
        assert rc == _lib.MSM_ERR_INVALID and np.all(Z == -7.0)
    with pytest.raises(ValueError):
        A().linkage(np.array([1.0, np.nan, 2.0]), 3, "single")
    # and the library still works afterwards
    rc, Z = lib_linkage(D, 65, "ward")
    assert rc == 0 and np.array_equal(bits(Z), bits(ref_linkage(65, "ward")))


@pytest.mark.parametrize("dn", ("f32", "f64"))
def test_linkage_fit_equals_linkage_of_pdist(gpu, dn):
    from msmbuilder_amd import libdistance
    from msmbuilder_amd._lib import Arr
    X = R.cloud(300, 4, 5, R.DT[dn])
    idx = np.random.RandomState(6).permutation(300)[:97]
    for metric, method in (("euclidean", "ward"), ("cityblock", "average"), ("chebyshev", "single"), ("canberra", "complete")):
        for indices in (None, idx):
            D = libdistance.pdist(X, metric, X_indices=indices)
            n = 300 if indices is None else len(indices)
            want = A().linkage(D, n, method)
            for on_device in (False, True):
                ax = Arr(dev(X) if on_device else X)
                Z = A().linkage_fit(ax, metric, method, indices)
                assert np.array_equal(bits(Z), bits(want)), (metric, method, indices is None, on_device)


# ---- within-cluster sums -----------------------------------------------------------------------------------------------
def within_ratio(got, ref, labels, K):
    bound = R.within_bound(R.pairs_within(labels, K)) * np.abs(ref)
    err = np.abs(got - ref)
    assert np.all(err <= bound), (err, bound)
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))


@pytest.mark.parametrize("n", (2, 65, 257, 700))
def test_within_cluster_sums(gpu, n):
    X, D = matrix(n, 2)
    rs = np.random.RandomState(n)
    worst = 0.0
    for K, labels in ((1, np.zeros(n, dtype=np.int64)), (n, rs.permutation(n)), (5, rs.randint(0, 5, n)),
                      (9, np.concatenate(([7], rs.randint(0, 7, n - 1))))):   # cluster 7: one landmark; cluster 8: none
        ref = R.within(D, labels, K)
        runs = [A().within_cluster(dev(D) if on_device else D, n, labels, K) for on_device in (False, True, False)]
        assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.array_equal(bits(runs[0]), bits(runs[2]))
        worst = max(worst, within_ratio(runs[0], ref, labels, K))
        if K == n:
            assert np.all(runs[0] == 0.0) and not np.any(np.signbit(runs[0]))
        if K == 9:
            assert runs[0][7] == 0.0 and runs[0][8] == 0.0
    print("within-cluster sums n=%d: worst error / bound = %.3g" % (n, worst))


def test_within_after_fit_and_errors(gpu):
    from msmbuilder_amd import libdistance
    from msmbuilder_amd._lib import Arr
    X = R.cloud(130, 3, 8, np.float32)
    labels = np.random.RandomState(1).randint(0, 4, 130)
    A().linkage_fit(Arr(X), "euclidean", "average")
    got = A().within_cluster(None, 130, labels, 4)          # the matrix the fit left in the library
    want = A().within_cluster(libdistance.pdist(X, "euclidean"), 130, labels, 4)
    assert np.array_equal(bits(got), bits(want))
    with pytest.raises(Exception):
        A().within_cluster(None, 131, np.zeros(131, dtype=np.int64), 4)   # no matrix of that size
    with pytest.raises(ValueError):
        A().within_cluster(None, 130, labels, 3)                           # a label outside [0, K)


# ---- msm_landmark_predict_* --------------------------------------------------------------------------------------------
def plan(m, dt):
    from msmbuilder_amd import _lib
    out = (C.c_int64 * 4)()
    assert _lib.lib().msm_landmark_predict_plan(m, np.dtype(dt).itemsize, out) == 0
    return dict(zip(("rows", "tile", "chunk", "regs"), list(out)))


def offsets_for(L, K, seed, empty=()):
    """K + 1 offsets from 0 to L: random cluster sizes >= 1, the ids in ``empty`` without a landmark."""
    full = [c for c in range(K) if c not in empty]
    assert len(full) <= L
    cuts = np.sort(np.random.RandomState(seed).permutation(L - 1)[:len(full) - 1] + 1) if len(full) > 1 else np.array([], int)
    sizes = np.zeros(K, dtype=np.int64)
    sizes[full] = np.diff(np.concatenate(([0], cuts, [L])))
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def check_predict(X, landmarks, offsets, metric, rule, intra=None, devices=(False, True)):
    """The library on host and device rows against the restatement: labels, winning values, the negative flag."""
    K = len(offsets) - 1
    ll = np.repeat(np.arange(K), np.diff(offsets))
    if rule == "ward" and intra is None:
        with np.errstate(all="ignore"):
            intra = R.within(R._oracle().pdist(np.ascontiguousarray(landmarks), metric), ll, K)
    d = R.exact_cdist(X, landmarks, metric)
    want, best, negative = R.pooled_predict(d, ll, K, rule, intra)
    for on_device in devices:
        labels, pooled, neg = A().pooled_predict(dev(X) if on_device else X, landmarks, offsets, intra, metric, rule, True)
        what = "%s %s %s N=%d L=%d m=%d K=%d device=%d" % (metric, rule, X.dtype, len(X), len(landmarks), X.shape[1], K, on_device)
        assert host(labels).dtype == np.int64 and np.array_equal(host(labels), want), what
        assert np.array_equal(bits(host(pooled)), bits(best)), what
        assert neg == negative, what
        labels2, none, _ = A().pooled_predict(dev(X) if on_device else X, landmarks, offsets, intra, metric, rule)
        assert none is None and np.array_equal(host(labels2), want), what
    return want, best, negative


@pytest.mark.parametrize("dn", ("f32", "f64"))
@pytest.mark.parametrize("metric", R.METRICS)
def test_predict_metrics_single(gpu, metric, dn):
    X = R.cloud(300, 5, 11, R.DT[dn], metric)
    lm = R.cloud(40, 5, 12, R.DT[dn], metric)
    check_predict(X, lm, offsets_for(40, 6, 1), metric, "single")


@pytest.mark.parametrize("dn", ("f32", "f64"))
@pytest.mark.parametrize("rule", ("complete", "average", "ward"))
@pytest.mark.parametrize("metric", ("euclidean", "sqeuclidean", "cityblock"))
def test_predict_rules(gpu, metric, rule, dn):
    X = R.cloud(300, 5, 13, R.DT[dn])
    lm = R.cloud(40, 5, 14, R.DT[dn])
    check_predict(X, lm, offsets_for(40, 6, 2), metric, rule)


@pytest.mark.parametrize("dn", ("f32", "f64"))
@pytest.mark.parametrize("m", (1, 3, 5, 17, 171))
def test_predict_widths(gpu, m, dn):
    p = plan(m, R.DT[dn])
    assert p["chunk"] == m and p["regs"] == (m <= (32 if dn == "f32" else 16))
    X = R.cloud(257, m, 15, R.DT[dn])
    lm = R.cloud(50, m, 16, R.DT[dn])
    for rule in R.LINKAGES:
        check_predict(X, lm, offsets_for(50, 7, m), "euclidean", rule)


@pytest.mark.parametrize("N", (1, 255, 256, 257, 513))
def test_predict_rows_around_a_workgroup(gpu, N):
    assert plan(5, np.float32)["rows"] == 256
    lm = R.cloud(20, 5, 18, np.float32)
    for rule in ("single", "ward"):
        check_predict(R.cloud(N, 5, 17, np.float32), lm, offsets_for(20, 4, 3), "euclidean", rule)


@pytest.mark.parametrize("m,dn,tile", ((5, "f32", 512), (171, "f64", 23)))
def test_predict_landmarks_around_a_tile(gpu, m, dn, tile):
    assert plan(m, R.DT[dn])["tile"] == tile
    X = R.cloud(70, m, 19, R.DT[dn])
    for L in (tile - 1, tile, tile + 1, 2 * tile + 1):
        lm = R.cloud(L, m, 20 + L, R.DT[dn])
        # three clusters: with L > tile one of them straddles every tile edge
        off = np.array([0, L // 3, L - L // 4, L], dtype=np.int64)
        assert L <= tile or any(off[c] < e < off[c + 1] for c in range(3) for e in range(tile, L, tile))
        for rule in R.LINKAGES:
            check_predict(X, lm, off, "euclidean", rule, devices=(False,))
        check_predict(X, lm, off, "cityblock", "average", devices=(True,))


@pytest.mark.parametrize("m,dn", ((8200, "f32"), (4100, "f64")))
def test_predict_rows_wider_than_the_tile(gpu, m, dn):
    p = plan(m, R.DT[dn])
    assert p["tile"] == 1 and p["chunk"] < m
    X = R.cloud(70, m, 21, R.DT[dn])
    lm = R.cloud(5, m, 22, R.DT[dn])
    for metric, rule in (("euclidean", "average"), ("braycurtis", "single"), ("cityblock", "ward")):
        check_predict(X, lm, np.array([0, 2, 2, 5], dtype=np.int64), metric, rule, devices=(False,))


@pytest.mark.parametrize("rule", R.LINKAGES)
def test_predict_cluster_counts(gpu, rule):
    X = R.cloud(130, 3, 23, np.float64)
    lm = R.cloud(33, 3, 24, np.float64)
    check_predict(X, lm, np.array([0, 33], dtype=np.int64), "euclidean", rule)                 # K = 1
    check_predict(X, lm, np.arange(34, dtype=np.int64), "euclidean", rule)                     # K = L
    for empty in ((0,), (5,), (0, 1, 4, 5), (2, 3)):                                            # ids without a landmark
        want, _, _ = check_predict(X, lm, offsets_for(33, 6, 4, empty), "euclidean", rule)
        assert not np.any(np.isin(want, empty))


@pytest.mark.parametrize("rule", R.LINKAGES)
def test_predict_exact_ties_go_to_the_lower_id(gpu, rule):
    # clusters 1 and 3 hold the same landmarks (so does their within-cluster sum): wherever they win they tie exactly
    base = R.cloud(6, 4, 25, np.float32)
    lm = np.ascontiguousarray(np.concatenate([base[:2] + 50, base[2:5], base[5:] - 50, base[2:5]]))
    off = np.array([0, 2, 5, 6, 9], dtype=np.int64)
    X = np.ascontiguousarray(np.concatenate([base[2:5] + 0.25, R.cloud(200, 4, 26, np.float32)]))
    want, _, _ = check_predict(X, lm, off, "euclidean", rule)
    assert np.sum(want == 1) >= 3 and not np.any(want == 3)


@pytest.mark.parametrize("dn", ("f32", "f64"))
@pytest.mark.parametrize("metric", ("euclidean", "sqeuclidean", "cityblock"))
def test_predict_nan_and_inf_rows(gpu, metric, dn):
    X = R.cloud(80, 3, 27, R.DT[dn])
    X[3, 1] = np.nan
    X[7] = np.nan
    X[11, 0] = np.inf
    X[12, 2] = -np.inf
    X[13] = np.inf
    lm = R.cloud(12, 3, 28, R.DT[dn])
    lm[4, 0] = np.inf      # inf - inf = NaN against row 11, inside cluster 1 only
    lm[9, 2] = np.nan      # a NaN landmark: cluster 3 is NaN for every row under min / max / the sums
    off = np.array([0, 3, 6, 8, 12], dtype=np.int64)
    intra = np.array([1.0, 2.0, 0.5, 3.0])
    for rule in R.LINKAGES:
        want, best, _ = check_predict(X, lm, off, metric, rule, intra=intra)
        assert want[7] == 0 and best[7] == np.inf and not np.any(np.isnan(best)) and not np.any(want == 3)


def test_predict_negative_ward_value(gpu):
    X = R.cloud(60, 3, 29, np.float64)
    lm = R.cloud(10, 3, 30, np.float64)
    off = np.array([0, 4, 10], dtype=np.int64)
    _, best, negative = check_predict(X, lm, off, "euclidean", "ward", intra=np.array([1e6, 0.0]))
    assert negative and np.all(best < 0)
    _, _, negative = check_predict(X, lm, off, "euclidean", "ward", intra=np.array([0.0, 0.0]))
    assert not negative
    for rule in ("single", "average"):   # the flag belongs to ward
        _, _, negative = check_predict(X, lm, off, "euclidean", rule, intra=np.array([1e6, 0.0]))
        assert not negative


def test_predict_argument_errors(gpu):
    X = R.cloud(10, 3, 31, np.float64)
    lm = R.cloud(4, 3, 32, np.float64)
    with pytest.raises(ValueError, match="linkage median is not supported"):
        A().pooled_predict(X, lm, np.array([0, 4]), None, "euclidean", "median")
    with pytest.raises(ValueError):
        A().pooled_predict(X, lm, np.array([0, 3]), None, "euclidean", "single")      # offsets do not end at L
    with pytest.raises(ValueError):
        A().pooled_predict(X, lm, np.array([0, 3, 2, 4]), None, "euclidean", "single")  # decreasing
    with pytest.raises(ValueError):
        A().pooled_predict(X, lm, np.array([0, 4]), None, "euclidean", "ward")        # ward without the sums
    with pytest.raises(ValueError):
        A().pooled_predict(X, lm, np.array([0, 4]), None, "mahalanobis", "single")
    labels, _, _ = A().pooled_predict(X[:0], lm, np.array([0, 4]), None, "euclidean", "single")
    assert labels.shape == (0,)


# ---- the estimator -----------------------------------------------------------------------------------------------------
def fitted(m):
    return {"landmark_labels": m.landmark_labels_, "cardinality": m.cardinality_, "centers": m.cluster_centers_,
            "within": m.squared_distances_within_cluster_}


@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=lambda c: c[0])
def test_estimator_against_golden(gpu, golden, case):
    from msmbuilder_amd.cluster import LandmarkAgglomerative
    name, lk, dn, strategy, n_landmarks, rows, ward_predictor = case
    X = R.walk(dt=R.DT[dn])[:rows]
    seed = int(golden["random_seed"])
    if strategy == "random":
        idx = R.landmark_indices(len(X), n_landmarks, "random", seed)
        assert len(np.unique(idx)) == len(idx)   # this seed draws no row twice
    m = LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=n_landmarks, linkage=lk, landmark_strategy=strategy,
                              random_state=seed, ward_predictor=ward_predictor).fit([X])
    assert m.landmarks_.dtype == X.dtype and isinstance(m.landmarks_, np.ndarray)
    assert np.array_equal(m.landmarks_, X[R.landmark_indices(len(X), n_landmarks, strategy, seed)])
    check_fit_against_golden(fitted(m), golden, name + "_")
    labels = m.predict([X])[0]
    assert isinstance(labels, np.ndarray) and labels.dtype == np.dtype(int)
    rule = ward_predictor if lk == "ward" else lk
    check_predict_against_golden(labels, X, m.landmarks_, golden, name + "_", rule)
    # and exactly what the restatement gives on the same input (pooled with the library's own within-cluster sums)
    r = R.estimator(X, R.GOLDEN_K, n_landmarks, lk, "euclidean", strategy, seed, ward_predictor, predict=False)
    assert np.array_equal(m.landmark_labels_, r["landmark_labels"])
    want, _, _ = R.pooled_predict(R.exact_cdist(X, m.landmarks_, "euclidean"), m.landmark_labels_, R.GOLDEN_K, rule,
                                  m.squared_distances_within_cluster_)
    assert np.array_equal(labels, want)


@pytest.mark.parametrize("lk", R.LINKAGES)
def test_estimator_duplicate_landmarks(gpu, lk):
    from msmbuilder_amd.cluster import LandmarkAgglomerative
    X = R.walk(dt=np.float64)[:400]
    idx = R.landmark_indices(400, 90, "random", 0)
    assert len(np.unique(idx)) < len(idx)   # rows drawn twice: zero distances, exact ties
    m = LandmarkAgglomerative(n_clusters=6, n_landmarks=90, linkage=lk, landmark_strategy="random", random_state=0).fit([X])
    r = R.estimator(X, 6, 90, lk, "euclidean", "random", 0)
    assert np.array_equal(m.landmarks_, r["landmarks"]) and np.array_equal(m.landmark_labels_, r["landmark_labels"])
    assert np.array_equal(m.cardinality_, r["cardinality"]) and np.array_equal(bits(m.cluster_centers_), bits(r["centers"]))
    within_ratio(m.squared_distances_within_cluster_, r["within"], r["landmark_labels"], 6)
    # (the pooled values use each side's own within-cluster sums: compare through the library's)
    d = R.exact_cdist(X, m.landmarks_, "euclidean")
    want, _, _ = R.pooled_predict(d, m.landmark_labels_, 6, lk, m.squared_distances_within_cluster_)
    assert np.array_equal(m.predict([X])[0], want)


def test_estimator_sequences_fit_predict_pickle_and_device_input(gpu, golden):
    import torch
    from msmbuilder_amd.cluster import LandmarkAgglomerative
    seqs = R.golden_sequences()
    X = np.concatenate(seqs)
    m = LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=R.GOLDEN_LANDMARKS, linkage="average").fit(seqs)
    check_fit_against_golden(fitted(m), golden, "seq_")
    labels = m.predict(seqs)
    assert [len(a) for a in labels] == [len(s) for s in seqs]
    check_predict_against_golden(np.concatenate(labels), X, m.landmarks_, golden, "seq_", "average")
    assert np.array_equal(m.partial_predict(seqs[1]), labels[1]) and np.array_equal(m.partial_transform(seqs[2]), labels[2])
    assert all(np.array_equal(a, b) for a, b in zip(m.transform(seqs), labels))

    # fit_predict (ward) against the reference's
    w = LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=R.GOLDEN_LANDMARKS, linkage="ward")
    fp = w.fit_predict(seqs)
    assert [len(a) for a in fp] == [len(s) for s in seqs]
    ref = golden["seq_fit_predict"].astype(np.int64)
    d = R.exact_cdist(X, w.landmarks_, "euclidean")
    v, present, sq = R.reference_pooled(d, w.landmark_labels_, R.GOLDEN_K, "ward", w.cardinality_, w.squared_distances_within_cluster_)
    decided = R.decided_rows(v, present, R.pooled_eps(v, present, "ward", w.cardinality_, w.squared_distances_within_cluster_, sq))
    assert np.sum(~decided) <= 0.01 * len(ref) and np.array_equal(np.concatenate(fp)[decided], ref[decided])
    assert all(np.array_equal(a, b) for a, b in zip(w.fit_transform(seqs), fp))

    # a pickle round trip predicts the same
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.get_params() == m.get_params()
    assert all(np.array_equal(a, b) for a, b in zip(m2.predict(seqs), labels))

    # torch CUDA rows give what numpy rows give: attributes on the host, labels host int arrays
    for lk in R.LINKAGES:
        mh = LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=R.GOLDEN_LANDMARKS, linkage=lk).fit(seqs)
        md = LandmarkAgglomerative(n_clusters=R.GOLDEN_K, n_landmarks=R.GOLDEN_LANDMARKS, linkage=lk).fit([dev(s) for s in seqs])
        for a, b in zip(fitted(mh).values(), fitted(md).values()):
            assert isinstance(b, np.ndarray) and np.array_equal(bits(a), bits(b))
        assert isinstance(md.landmarks_, np.ndarray) and np.array_equal(bits(mh.landmarks_), bits(md.landmarks_))
        ld = md.predict([dev(s) for s in seqs])
        assert all(isinstance(a, np.ndarray) for a in ld)
        assert all(np.array_equal(a, b) for a, b in zip(ld, mh.predict(seqs)))
    # every row a landmark, on the device, and an integer input (computed in float64)
    Xi = np.rint(X[:300] * 4).astype(np.int32)
    mi = LandmarkAgglomerative(n_clusters=5, linkage="complete").fit([Xi])
    mf = LandmarkAgglomerative(n_clusters=5, linkage="complete").fit([torch.as_tensor(Xi.astype(np.float64), device="cuda")])
    assert mi.landmarks_.dtype == np.float64 and np.array_equal(mi.landmarks_, mf.landmarks_)
    assert np.array_equal(mi.landmark_labels_, mf.landmark_labels_)
    assert np.array_equal(mi.predict([Xi])[0], mf.predict([Xi.astype(np.float64)])[0])
    with pytest.raises(TypeError):
        mi.predict([Xi.astype(np.float32)])


def test_estimator_warns_on_negative_ward_value(gpu):
    from msmbuilder_amd.cluster import LandmarkAgglomerative
    X = R.walk(dt=np.float32)[:500]
    m = LandmarkAgglomerative(n_clusters=4, n_landmarks=50, linkage="ward").fit([X])
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        m.predict([X])
    assert not any("negative" in str(w.message) for w in seen)
    m.squared_distances_within_cluster_ = m.squared_distances_within_cluster_ + 1e12
    with pytest.warns(UserWarning, match="Distance shouldn't be negative."):
        m.predict([X])
