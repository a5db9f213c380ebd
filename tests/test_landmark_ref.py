"""CPU tier of landmark agglomerative clustering: the numpy restatement (tests/landmark_ref.py) held to scipy's linkage on
tie-free inputs and to the golden file written by the reference's own estimator (tests/golden/make_golden_landmark.py;
the linkage under it is scipy's, standing in for fastcluster), and the estimator's surface that needs no device.

Bounds (u = 2^-53, derived in landmark_ref.py): heights of average / ward within 8 n u relative, after checking that the
reference's heights are further apart than twice that; within-cluster sums within 2 p u relative for p pairs; predicted
labels of average / ward equal wherever the reference's best value is further from every other cluster's than the two
evaluation errors together, with at most 1 % of the rows undecided."""
import os

import numpy as np
import pytest

import landmark_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "landmark_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the restatement's linkage against scipy ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", (40, 150))
@pytest.mark.parametrize("method", R.LINKAGES)
def test_linkage_against_scipy(method, n):
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import pdist
    D = pdist(np.random.RandomState(0).randn(n, 3))
    Zs = linkage(D, method=method)
    Z = R.linkage(D, method)
    assert np.array_equal(Z[:, :2], Zs[:, :2]) and np.array_equal(Z[:, 3], Zs[:, 3])
    if method in ("single", "complete"):
        assert np.array_equal(bits(Z[:, 2]), bits(Zs[:, 2]))
        return
    bound = R.height_bound(n)
    gap = R.relative_gap(Zs[:, 2])
    err = float(np.max(np.abs(Z[:, 2] - Zs[:, 2]) / Zs[:, 2]))
    print("%s n=%d: height error %.3g, bound %.3g (ratio %.3g), smallest gap %.3g" % (method, n, err, bound, err / bound, gap))
    assert gap > 2 * bound   # the topology cannot agree by accident
    assert err <= bound


def test_linkage_tie_rule_and_hand_case():
    # four points on a line at 0, 1, 2, 4: d(0,1) = d(1,2) = 1 tie -> the lowest row slot (0, 1) goes first, into slot 1
    X = np.array([0.0, 1.0, 2.0, 4.0])
    D = np.array([abs(X[i] - X[j]) for i in range(4) for j in range(i + 1, 4)])
    Z = R.linkage(D, "single")
    assert Z.tolist() == [[0, 1, 1, 2], [2, 4, 1, 3], [3, 5, 2, 4]]
    Z = R.linkage(D, "complete")
    # then d({0,1}, 2) = d(2, 3) = 2 tie: the row of slot 1 (the merged cluster) is lower than row 2
    assert Z.tolist() == [[0, 1, 1, 2], [2, 4, 2, 3], [3, 5, 4, 4]]
    Z = R.linkage(D, "average")
    assert Z.tolist() == [[0, 1, 1, 2], [2, 4, 1.5, 3], [3, 5, 3, 4]]
    # equal columns in one row: the lowest column
    D = np.array([1.0, 1.0, 1.0])
    assert R.linkage(D, "single")[0].tolist() == [0, 1, 1, 2]


# ---- the restatement against the goldens -------------------------------------------------------------------------------
def check_fit_against_golden(r, golden, p, n_clusters=R.GOLDEN_K):
    """The issue's criteria for a fitted result (dict of landmark_ref.estimator / attributes of the estimator)."""
    assert np.array_equal(r["landmark_labels"], golden[p + "landmark_labels"])
    assert np.array_equal(r["cardinality"], golden[p + "cardinality"])
    assert r["centers"].dtype == golden[p + "centers"].dtype
    assert np.array_equal(bits(r["centers"]), bits(golden[p + "centers"]))
    ref = golden[p + "within"]
    bound = R.within_bound(R.pairs_within(r["landmark_labels"], n_clusters))
    err = np.abs(np.asarray(r["within"]) - ref)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound * np.abs(ref), 1.0), np.where(err > 0, np.inf, 0.0))))
    print("%s within-cluster sums: worst error / bound = %.3g" % (p, ratio))
    assert np.all(err <= bound * np.abs(ref))
    return ratio


def check_predict_against_golden(labels, X, landmarks, golden, p, rule, metric="euclidean", n_clusters=R.GOLDEN_K):
    """Predicted labels against the reference's: equal for single / complete; for average / ward equal on every decided row
    (landmark_ref.decided_rows on the reference's own pooled values), at most 1 % of the rows undecided."""
    ref = golden[p + "predict"].astype(np.int64)
    labels = np.asarray(labels)
    if rule in ("single", "complete"):
        assert np.array_equal(labels, ref)
        return 0
    ll = golden[p + "landmark_labels"].astype(np.int64)
    d = R.exact_cdist(X, landmarks, metric)
    v, present, sq = R.reference_pooled(d, ll, n_clusters, rule, golden[p + "cardinality"], golden[p + "within"])
    assert np.array_equal(R.argmin_strict(v, present)[0], ref)   # these ARE the reference's values
    eps = R.pooled_eps(v, present, rule, golden[p + "cardinality"], golden[p + "within"], sq)
    decided = R.decided_rows(v, present, eps)
    undecided = int(np.sum(~decided))
    print("%s %s: %d of %d rows undecided" % (p, rule, undecided, len(ref)))
    assert undecided <= 0.01 * len(ref)
    assert np.array_equal(labels[decided], ref[decided])
    return undecided


@pytest.mark.parametrize("case", R.GOLDEN_CASES, ids=lambda c: c[0])
def test_restatement_against_golden(golden, case):
    name, lk, dn, strategy, n_landmarks, rows, ward_predictor = case
    X = R.walk(dt=R.DT[dn])[:rows]
    seed = int(golden["random_seed"])
    if strategy == "random":
        idx = R.landmark_indices(len(X), n_landmarks, "random", seed)
        assert len(np.unique(idx)) == len(idx)   # this seed draws no row twice
    r = R.estimator(X, R.GOLDEN_K, n_landmarks, lk, "euclidean", strategy, seed, ward_predictor)
    check_fit_against_golden(r, golden, name + "_")
    rule = ward_predictor if lk == "ward" else lk
    check_predict_against_golden(r["predict"], X, r["landmarks"], golden, name + "_", rule)


def test_sequence_list_against_golden(golden):
    X = np.concatenate(R.golden_sequences())
    r = R.estimator(X, R.GOLDEN_K, R.GOLDEN_LANDMARKS, "average")
    check_fit_against_golden(r, golden, "seq_")
    check_predict_against_golden(r["predict"], X, r["landmarks"], golden, "seq_", "average")


def test_pooled_predict_corners():
    # two clusters at exactly the same pooled value -> the lower id; a cluster id without a landmark is skipped;
    # NaN never wins, a row of NaN / +inf only gets label 0; a negative ward value is reported
    d = np.array([[1.0, 3.0, 2.0, 2.0], [np.nan, 1.0, 5.0, 5.0], [np.nan, np.nan, np.nan, np.nan], [np.inf, np.inf, np.inf, np.inf]])
    ll = np.array([0, 0, 3, 3])
    for rule, want in (("average", [0, 3, 0, 0]), ("single", [0, 3, 0, 0]), ("complete", [3, 3, 0, 0])):
        labels, best, neg = R.pooled_predict(d, ll, 5, rule)
        assert labels.tolist() == want and not neg, rule
    labels, best, neg = R.pooled_predict(np.array([[0.5, 0.5]]), np.array([1, 1]), 2, "ward", intra=np.array([0.0, 4.0]))
    assert labels.tolist() == [1] and neg and best[0] == (2 * 0.5 - 4.0) / 3.0


# ---- the estimator's surface without a device --------------------------------------------------------------------------
def test_estimator_surface_without_device():
    import msmbuilder_amd
    import msmbuilder_amd.cluster
    from msmbuilder_amd.cluster import LandmarkAgglomerative
    from msmbuilder_amd.cluster import agglomerative as A
    assert msmbuilder_amd.LandmarkAgglomerative is LandmarkAgglomerative
    assert "LandmarkAgglomerative" in msmbuilder_amd.cluster.__all__
    m = LandmarkAgglomerative(n_clusters=4)
    assert m.get_params() == dict(n_clusters=4, n_landmarks=None, linkage="average", metric="euclidean",
                                  landmark_strategy="stride", random_state=None, max_landmarks=None, ward_predictor="ward")
    assert m.landmark_labels_ is None and m.landmarks_ is None and m.cluster_centers_ is None
    m.set_params(n_landmarks=50, linkage="ward", ward_predictor="single", random_state=3)
    p = m.get_params()
    assert (p["n_landmarks"], p["linkage"], p["ward_predictor"], p["random_state"]) == (50, "ward", "single", 3)
    m2 = LandmarkAgglomerative(**p)
    assert m2.get_params() == p
    for name in ("fit", "predict", "partial_predict", "fit_predict", "transform", "partial_transform", "fit_transform"):
        assert callable(getattr(m, name))

    X = [np.random.RandomState(0).randn(30, 2)]
    with pytest.raises(ValueError):
        LandmarkAgglomerative(n_clusters=2, metric=lambda a, b, i: None).fit(X)
    with pytest.raises(ValueError):
        LandmarkAgglomerative(n_clusters=2, metric="rmsd").fit(X)
    with pytest.raises(ValueError):
        LandmarkAgglomerative(n_clusters=2, linkage="centroid").fit(X)
    with pytest.raises(ValueError, match="linkage median is not supported"):
        A.pooling_rule("ward", "median")
    assert A.pooling_rule("ward", "single") == "single" and A.pooling_rule("average", "median") == "average"
    bad = LandmarkAgglomerative(n_clusters=2, linkage="ward", ward_predictor="median")
    bad.landmarks_ = np.zeros((2, 2))
    with pytest.raises(ValueError, match="linkage median is not supported"):
        bad.predict(X)

    # max_landmarks replaces n_landmarks only when there are more clusters than landmarks
    assert A.effective_n_landmarks(10, 5, 40) == 40
    assert A.effective_n_landmarks(5, 10, 40) == 10
    assert A.effective_n_landmarks(10, 5, None) == 5 and A.effective_n_landmarks(3, None, None) is None
    # stride: every (n // n_landmarks)-th row, cut to n_landmarks; random: randint with replacement
    assert A.landmark_indices(10, 3).tolist() == [0, 3, 6]
    assert A.landmark_indices(11, 5).tolist() == [0, 2, 4, 6, 8]
    assert A.landmark_indices(3000, 120).tolist() == list(range(0, 3000, 25))
    assert np.array_equal(A.landmark_indices(100, 30, "random", 7), np.random.RandomState(7).randint(100, size=30))
    assert len(np.unique(A.landmark_indices(20, 200, "random", 1))) <= 20   # duplicates are possible
    for n, L, st, rs in ((3000, 120, "stride", None), (977, 13, "stride", None), (500, 40, "random", 5)):
        assert np.array_equal(A.landmark_indices(n, L, st, rs), R.landmark_indices(n, L, st, rs))
    # the landmarks of one cluster are contiguous after the stable permutation; an id without a landmark is an empty range
    perm, off = A.permute_by_cluster(np.array([2, 0, 2, 0, 4]), 5)
    assert perm.tolist() == [1, 3, 0, 2, 4] and off.tolist() == [0, 2, 2, 4, 4, 5]


def test_c_abi_argument_errors_need_no_device():
    import ctypes as C
    from msmbuilder_amd import _lib
    L = _lib.lib()
    Z = np.full((3, 4), -7.0)
    D = np.ones(6)
    assert L.msm_linkage(D.ctypes.data, 1, b"single", Z.ctypes.data, 0) == _lib.MSM_ERR_INVALID
    assert L.msm_linkage(D.ctypes.data, 4, b"centroid", Z.ctypes.data, 0) == _lib.MSM_ERR_INVALID
    assert L.msm_linkage(D.ctypes.data, 4, None, Z.ctypes.data, 0) == _lib.MSM_ERR_INVALID
    assert np.all(Z == -7.0)
    plan = (C.c_int64 * 4)()
    assert L.msm_landmark_predict_plan(5, 4, plan) == 0 and list(plan) == [256, 512, 5, 1]
    assert L.msm_landmark_predict_plan(171, 8, plan) == 0 and list(plan) == [256, 4096 // 171, 171, 0]
    assert L.msm_landmark_predict_plan(5000, 8, plan) == 0 and list(plan) == [256, 1, 4096, 0]
