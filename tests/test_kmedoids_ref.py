"""CPU tier: the numpy reference loop of k-medoids (tests/kmedoids_ref.py) held to EQUALITY with the golden file written
by the reference's own extension and estimators (tests/golden/make_golden_kmedoids.py), hand cases of the loop's
corners, the exported 64-bit condensed index, and the C ABI's argument errors (none of which needs a device)."""
import ctypes as C
import os

import numpy as np
import pytest

import kmedoids_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmedoids_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("case", R.GOLDEN_LOOP, ids=lambda c: "n%d-K%d-p%d-%s" % (c[0], c[1], c[2], c[4]))
def test_loop_against_golden(golden, case):
    n, K, npass, seed, metric = case
    D, start, rs = R.loop_case(*case)
    inits = R.random_assignments(rs, n, K, npass)
    ids, error, ifound, _ = R.kmedoids(K, D, npass, start, inits)
    p = "loop_%d_%d_%d_%d_" % (n, K, npass, seed)
    assert np.array_equal(ids, golden[p + "ids"])
    assert np.float64(error).tobytes() == golden[p + "error"].tobytes()
    assert ifound == int(golden[p + "ifound"])
    assert rs.random_sample() == float(golden[p + "next"])   # the generator is left where the reference leaves it


@pytest.mark.parametrize("case", R.GOLDEN_KMEDOIDS, ids=lambda c: "%s-%s" % (c[0], c[1]))
def test_kmedoids_estimator_against_golden(golden, case):
    metric, dn, n, m, seed, K, npasses = case
    X = R.cloud(n, m, seed, R.DT[dn], metric)
    rs = np.random.RandomState(seed)
    r = R.kmedoids_estimator(X, K, npasses, metric, rs)
    p = "km_%s_%s_" % (metric, dn)
    assert np.array_equal(r["labels"], golden[p + "labels"])
    assert np.array_equal(r["cluster_ids"], golden[p + "cluster_ids"])
    assert r["centers"].dtype == golden[p + "centers"].dtype and np.array_equal(bits(r["centers"]), bits(golden[p + "centers"]))
    assert np.float64(r["inertia"]).tobytes() == golden[p + "inertia"].tobytes()
    assert rs.random_sample() == float(golden[p + "next"])


@pytest.mark.parametrize("case", R.GOLDEN_MINIBATCH, ids=lambda c: "%s-%s" % (c[0], c[1]))
def test_minibatch_estimator_against_golden(golden, case):
    metric, dn, n, m, seed, kw = case
    X = R.cloud(n, m, seed, R.DT[dn], metric)
    rs = np.random.RandomState(seed)
    r = R.minibatch_estimator(X, metric=metric, random_state=rs, **kw)
    p = "mb_%s_%s_" % (metric, dn)
    assert np.array_equal(r["labels"], golden[p + "labels"])
    assert np.array_equal(r["cluster_ids"], golden[p + "cluster_ids"])
    assert np.array_equal(bits(r["centers"]), bits(golden[p + "centers"]))
    assert np.float64(r["inertia"]).tobytes() == golden[p + "inertia"].tobytes()
    assert rs.random_sample() == float(golden[p + "next"])


def test_sequence_list_against_golden(golden):
    seqs = R.golden_sequences()
    X = np.concatenate(seqs)
    lengths = [len(s) for s in seqs]
    r = R.kmedoids_estimator(X, 5, 2, "euclidean", 3)
    assert np.array_equal(R.split_indices(lengths, r["cluster_ids"]), golden["seq_km_pairs"])
    assert np.array_equal(r["labels"], golden["seq_km_labels"])
    assert np.float64(r["inertia"]).tobytes() == golden["seq_km_inertia"].tobytes()
    r = R.minibatch_estimator(X, n_clusters=5, batch_size=40, random_state=3)
    assert np.array_equal(R.split_indices(lengths, r["cluster_ids"]), golden["seq_mb_pairs"])
    assert np.array_equal(r["labels"], golden["seq_mb_labels"])
    assert np.float64(r["inertia"]).tobytes() == golden["seq_mb_inertia"].tobytes()


# ---- hand cases ------------------------------------------------------------------------------------------------------
def test_one_element_is_the_dbl_max_corner():
    ids, error, ifound, info = R.kmedoids(1, np.zeros(0), 1, None, np.zeros((1, 1), dtype=np.intp))
    assert ids.tolist() == [0] and error == R.DBL_MAX and ifound == 0 and info["iterations"] == 1


def test_two_elements():
    D = np.array([3.0])
    # one cluster: both costs are 3, the lower index is the medoid; labels [0, 0] equal the medoid ids [0, 0]: nothing copied
    ids, error, ifound, _ = R.kmedoids(1, D, 0, np.array([0, 0]))
    assert ids.tolist() == [0, 0] and error == R.DBL_MAX and ifound == 0
    # two clusters, labels swapped: medoids [1, 0], ids differ from the labels [0, 1] -> copied
    ids, error, ifound, _ = R.kmedoids(2, D, 0, np.array([1, 0]))
    assert ids.tolist() == [0, 1] and error == 0.0 and ifound == 1
    ids, error, ifound, _ = R.kmedoids(2, D, 0, np.array([0, 1]))
    assert ids.tolist() == [0, 1] and error == R.DBL_MAX and ifound == 0   # the identity: every label is its medoid's index


def test_k_equals_n_from_the_identity():
    n = 6
    D = np.arange(1.0, n * (n - 1) // 2 + 1)
    ids, error, ifound, _ = R.kmedoids(n, D, 0, np.arange(n))
    assert ids.tolist() == list(range(n)) and error == R.DBL_MAX and ifound == 0
    ids, error, ifound, _ = R.kmedoids(n, D, 0, np.arange(n)[::-1].copy())
    assert ids.tolist() == list(range(n)) and error == 0.0 and ifound == 1


def test_all_ties_matrix():
    n, K = 7, 3
    D = np.full(n * (n - 1) // 2, 0.5)
    start = np.array([2, 2, 1, 0, 1, 0, 2])
    ids, error, ifound, info = R.kmedoids(K, D, 0, start)
    # medoids: the lowest index of each cluster (all costs tie within a cluster): c0 -> 3, c1 -> 2, c2 -> 0; every
    # non-medoid then goes to cluster 0 (first at the minimum): total 4 * 0.5; second iteration: cluster 0 = {1,3,4,5,6}
    # -> medoid 1, the total stays 2.0 and the loop stops
    assert ids.tolist() == [0, 1, 2, 1, 1, 1, 1] and error == 2.0 and ifound == 1 and info["iterations"] == 2


def test_multi_pass_keeps_the_best_and_counts_repeats():
    X = R.cloud(40, 3, 5)
    D = R._oracle().pdist(X, "euclidean")
    rs = np.random.RandomState(0)
    init = R.random_assignments(rs, 40, 4, 1)
    ids1, e1, f1, _ = R.kmedoids(4, D, 1, None, init)
    ids3, e3, f3, _ = R.kmedoids(4, D, 3, None, np.repeat(init, 3, axis=0))
    assert np.array_equal(ids1, ids3) and e1 == e3 and f1 == 1 and f3 == 3


def test_random_assignment_shapes():
    rs = np.random.RandomState(3)
    a = R.random_assignments(rs, 50, 7, 4)
    assert a.shape == (4, 50) and all(sorted(set(r.tolist())) == list(range(7)) for r in a)
    assert sorted(R.random_assignments(np.random.RandomState(3), 5, 5, 1)[0].tolist()) == list(range(5))


# ---- the library without a device ------------------------------------------------------------------------------------
def test_condensed_index_64bit():
    from msmbuilder_amd import _lib
    f = _lib.lib().msm_kmedoids_condensed_index
    n = 3_000_000
    pairs = [(0, 1), (1, 0), (0, n - 1), (1, 2), (715, 716), (716, 0), (1431, 1432), (n - 2, n - 1), (n - 1, n - 2),
             (1_500_000, 2_999_999), (2_000_000, 17), (123_456, 2_345_678)]
    got = [f(i, j, n) for i, j in pairs]
    want = [R.condensed_index(i, j, n) for i, j in pairs]
    assert got == want
    assert any(2 ** 31 < w < 2 ** 32 for w in want) and any(w > 2 ** 32 for w in want)
    assert want[7] == n * (n - 1) // 2 - 1
    for nn in (2, 3, 10):
        assert [f(i, j, nn) for i in range(nn) for j in range(i + 1, nn)] == list(range(nn * (nn - 1) // 2))


def _call(n, K, npass, init, dmat=None):
    from msmbuilder_amd import _lib
    L = _lib.lib()
    init = np.ascontiguousarray(init, dtype=np.int64)
    dmat = np.ones(max(n * (n - 1) // 2, 1)) if dmat is None else dmat
    ids = np.full(n, -7, dtype=np.int64)
    err, found = C.c_double(-7.0), C.c_int64(-7)
    rc = L.msm_kmedoids(dmat.ctypes.data, n, K, npass, init.ctypes.data, ids.ctypes.data, C.byref(err), C.byref(found), 0)
    assert np.all(ids == -7) and err.value == -7.0 and found.value == -7   # an error writes nothing
    return rc, _lib.last_error()


def test_abi_errors_need_no_device():
    from msmbuilder_amd import _lib
    n = 6
    ok = np.array([0, 1, 2, 0, 1, 2])
    assert _call(n, 0, 0, ok)[0] == _lib.MSM_ERR_INVALID
    assert _call(n, 7, 0, ok)[0] == _lib.MSM_ERR_INVALID
    assert _call(n, 3, -1, ok)[0] == _lib.MSM_ERR_INVALID
    rc, msg = _call(n, 3, 0, np.array([0, 1, 3, 0, 1, 2]))
    assert rc == _lib.MSM_ERR_INVALID and "outside" in msg
    assert _call(n, 3, 0, np.array([0, 1, -1, 0, 1, 2]))[0] == _lib.MSM_ERR_INVALID
    rc, msg = _call(n, 3, 0, np.array([0, 1, 1, 0, 1, 0]))
    assert rc == _lib.MSM_ERR_INVALID and "empty" in msg
    # the second pass's assignment is checked too
    assert _call(n, 3, 2, np.array([[0, 1, 2, 0, 1, 2], [0, 1, 1, 0, 1, 0]]))[0] == _lib.MSM_ERR_INVALID
    L = _lib.lib()
    X = np.zeros((n, 2))
    ids = np.full(n, -7, dtype=np.int64)
    err, found = C.c_double(-7.0), C.c_int64(-7)
    init = np.ascontiguousarray(ok, dtype=np.int64)
    rc = L.msm_kmedoids_fit_f64(X.ctypes.data, n, 2, b"rmsd", None, 0, 3, 0, init.ctypes.data, ids.ctypes.data,
                                C.byref(err), C.byref(found), 0)
    assert rc == _lib.MSM_ERR_METRIC and np.all(ids == -7)
    rc = L.msm_kmedoids_fit_f32(X.astype(np.float32).ctypes.data, n, 2, b"euclidean", None, 0, 9, 0, init.ctypes.data,
                                ids.ctypes.data, C.byref(err), C.byref(found), 0)
    assert rc == _lib.MSM_ERR_INVALID and np.all(ids == -7)


def test_estimator_argument_errors_need_no_device():
    from msmbuilder_amd import KMedoids, MiniBatchKMedoids
    from msmbuilder_amd.cluster.kmedoids import _KMedoids
    X = np.zeros((5, 2))
    with pytest.raises(ValueError, match="n_passes must be greater than 0. got 0"):
        _KMedoids(n_passes=0).fit(X)
    with pytest.raises(ValueError, match="n_passes must be greater than 0. got 0"):   # (the reference's message names n_passes)
        _KMedoids(n_clusters=0).fit(X)
    with pytest.raises(ValueError, match="metric must be one of"):
        _KMedoids(metric="rmsd").fit(X)
    with pytest.raises(ValueError, match="metric must be one of"):
        MiniBatchKMedoids(metric="rmsd").fit([X])
    assert "n_passes" in KMedoids().get_params() and "max_no_improvement" in MiniBatchKMedoids().get_params()


def test_host_helpers_match_the_reference_loop():
    from msmbuilder_amd.cluster import kmedoids as K
    a = K.random_assignments(np.random.RandomState(11), 37, 5, 3)
    b = R.random_assignments(np.random.RandomState(11), 37, 5, 3)
    assert np.array_equal(a, b)
    ids = np.array([9, 2, 9, 4, 2, 0, 4])
    la, ia = K.contigify_ids(ids)
    lb, ib = R.contigify_ids(ids)
    assert np.array_equal(la, lb) and np.array_equal(ia, ib) and ia.tolist() == [9, 2, 4, 0]
