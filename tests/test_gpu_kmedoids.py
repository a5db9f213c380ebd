"""GPU tier: msm_kmedoids / msm_kmedoids_fit_* / KMedoids / MiniBatchKMedoids held to EQUALITY with the numpy reference
loop (tests/kmedoids_ref.py, itself held to the reference's own extension by tests/test_kmedoids_ref.py) and with the
golden file: clusterid, the bits of error, ifound, and the iteration and snapshot counts of the last pass.  No tolerance
anywhere: every decision of the loop compares float64 sums that the library adds in the reference's order.

Sizes are the smallest that reach each seam of the device code: the cost kernel's 64 x 64 tile (63, 64, 65, 129), the
256-thread workgroups (255, 256, 257, 513), the one-workgroup path's capacity of 180 elements (179, 180 on both paths,
181, 361), more clusters than a workgroup has threads (1025 at n = 2049), and the issue's list.  The largest matrix is
16 MB."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import kmedoids_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmedoids_golden.npz")
SMALL_MAXN = 180   # KM_SMALL_MAXN of kmedoids_dev.h
SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 179, 180, 181, 255, 256, 257, 361, 513, 1025, 2049)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(autouse=True)
def _default_path(monkeypatch):
    monkeypatch.delenv("MSM_KMEDOIDS_SMALL", raising=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def stats():
    from msmbuilder_amd.cluster.kmedoids import last_stats
    return last_stats()


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


@functools.lru_cache(maxsize=None)
def matrix(n, seed=0, metric="euclidean"):
    """(rows, condensed matrix by the C oracle): computed once, shared, never written to."""
    X = R.cloud(n, 3, seed, np.float64, metric)
    D = R._oracle().pdist(X, metric)
    X.setflags(write=False)
    D.setflags(write=False)
    return X, D


def starts(n, K, npass, seed):
    """The max(npass, 1) x n initial assignments: the reference's random ones, or (npass = 0) any without an empty cluster."""
    rs = np.random.RandomState(seed)
    if npass >= 1:
        return R.random_assignments(rs, n, K, npass)
    t = np.concatenate([np.arange(K), rs.randint(0, K, n - K)]).astype(np.intp)
    rs.shuffle(t)
    return t[None, :]


def lib_kmedoids(D, n, K, npass, init, on_device=False):
    from msmbuilder_amd import _lib
    L = _lib.lib()
    _lib.ensure_device(0)
    init = np.ascontiguousarray(init, dtype=np.int64)
    ids = np.full(n, -7, dtype=np.int64)
    err, found = C.c_double(-7.0), C.c_int64(-7)
    keep = D
    if on_device:
        import torch
        keep = torch.as_tensor(np.array(D), device="cuda")
        ptr = keep.data_ptr() if len(D) else None
    else:
        ptr = np.ascontiguousarray(D).ctypes.data if len(D) else None
    rc = L.msm_kmedoids(C.c_void_p(ptr), n, K, npass, init.ctypes.data, ids.ctypes.data, C.byref(err), C.byref(found),
                        int(on_device))
    return rc, ids, err.value, found.value


def check_loop(D, n, K, npass, init, monkeypatch, paths=None, on_device=False):
    """The library on every path that can run against the reference loop; returns the reference's info."""
    ids_r, err_r, found_r, info = R.kmedoids(K, D, npass, init[0] if npass == 0 else None, init)
    for small in (paths if paths is not None else ((1, 0) if n <= SMALL_MAXN else (0,))):
        monkeypatch.setenv("MSM_KMEDOIDS_SMALL", str(small))
        rc, ids, err, found = lib_kmedoids(D, n, K, npass, init, on_device)
        assert rc == 0
        st = stats()
        what = "n=%d K=%d npass=%d small=%d" % (n, K, npass, small)
        assert np.array_equal(ids, ids_r), what
        assert np.float64(err).tobytes() == np.float64(err_r).tobytes(), what
        assert found == found_r, what
        assert st["small"] == small and st["passes"] == max(npass, 1), what
        assert st["iterations"] == info["iterations"] and st["snapshots"] == info["snapshots"], what
    return info


def cluster_counts(n):
    ks = [k for k in (1, 2, 7, 64, 65) if k <= n] + [n]
    if n == 2049:
        ks.append(1025)   # more clusters than one workgroup has threads
    return sorted(set(ks))


@pytest.mark.parametrize("n,ki,K", [(n, ki, K) for n in SIZES for ki, K in enumerate(cluster_counts(n))])
def test_sizes_cluster_counts_passes_paths(gpu, monkeypatch, n, ki, K):
    X, D = matrix(n)
    # every npass at the small sizes; at the large ones the three values go round the cluster counts
    for npass in ((0, 1, 3) if n <= 257 else ((0, 1, 3)[ki % 3],)):
        check_loop(D, n, K, npass, starts(n, K, npass, 100 + n + K), monkeypatch)


LONG = [(150, 8, 7, 11, 1), (180, 9, 15, 21, 2), (300, 12, 5, 21, 2), (600, 24, 3, 41, 3)]


@pytest.mark.parametrize("n,K,seed,min_iter,snaps", LONG)
def test_long_runs_reach_the_later_snapshots(gpu, monkeypatch, n, K, seed, min_iter, snaps):
    """1-D random walks: seeds picked by the reference loop so that the runs take >= 11 (150, both paths), >= 21 (the
    second snapshot is taken at the 21st iteration: 180 on both paths, 300) and >= 41 iterations (the third: 600)."""
    X = R.walk1d(n, seed)
    D = R._oracle().pdist(X, "euclidean")
    init = R.random_assignments(np.random.RandomState(seed), n, K, 1)
    info = check_loop(D, n, K, 1, init, monkeypatch)
    assert info["iterations"] >= min_iter and info["iterations"] >= 11 and info["snapshots"] == snaps
    assert info["distinct"] == K
    if n == 600:
        assert info["iterations"] >= 31


def test_general_case_stands_for_something(gpu, monkeypatch):
    """A general-path case must run >= 3 iterations with K distinct medoids."""
    X, D = matrix(513)
    info = check_loop(D, 513, 7, 1, starts(513, 7, 1, 5), monkeypatch)
    assert info["iterations"] >= 3 and info["distinct"] == 7 and stats()["small"] == 0


def test_device_matrix(gpu, monkeypatch):
    for n in (100, 300):
        X, D = matrix(n)
        check_loop(D, n, 5, 3, starts(n, 5, 3, 1), monkeypatch, on_device=True)


# ---- ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (150, 230))
def test_constant_matrix(gpu, monkeypatch, n):
    D = np.full(n * (n - 1) // 2, 0.25)
    check_loop(D, n, 6, 0, starts(n, 6, 0, 2), monkeypatch)
    check_loop(D, n, 6, 3, starts(n, 6, 3, 2), monkeypatch)


@pytest.mark.parametrize("n", (160, 260))
def test_duplicate_rows(gpu, monkeypatch, n):
    X = np.repeat(R.cloud(n // 4, 2, 9), 4, axis=0)[np.random.RandomState(1).permutation(n)]   # every row four times: distance 0
    D = R._oracle().pdist(np.ascontiguousarray(X), "euclidean")
    assert np.count_nonzero(D == 0.0) >= n
    for K, npass in ((3, 1), (n // 4 + 5, 0), (n // 4 + 5, 2)):   # more clusters than distinct rows: medoids at distance 0
        check_loop(D, n, K, npass, starts(n, K, npass, 3), monkeypatch)


# ---- the fit: pdist on the device, then the loop -------------------------------------------------------------------------
def lib_fit(X, metric, K, npass, init, X_indices=None, device=False):
    from msmbuilder_amd._lib import Arr
    from msmbuilder_amd.cluster.kmedoids import kmedoids_fit
    if device:
        import torch
        X = torch.as_tensor(X, device="cuda")
    return kmedoids_fit(Arr(X), metric, K, npass, init, X_indices=X_indices)


@pytest.mark.parametrize("dn", ("f32", "f64"))
@pytest.mark.parametrize("metric", R.METRICS)
def test_metrics_and_dtypes(gpu, monkeypatch, metric, dn):
    """All eight metrics x both dtypes at a mid size on the general path, host and device rows (hamming / jaccard: rounded
    rows, many exact ties), and the same through the one-workgroup path at n = 120."""
    for n, K in ((230, 6), (120, 4)):
        X = R.cloud(n, 4, 17, R.DT[dn], metric)
        D = R._oracle().pdist(X, metric)
        init = starts(n, K, 2, 8)
        ids_r, err_r, found_r, info = R.kmedoids(K, D, 2, None, init)
        for device in (False, True):
            ids, err, found = lib_fit(X, metric, K, 2, init, device=device)
            assert np.array_equal(ids, ids_r) and np.float64(err).tobytes() == np.float64(err_r).tobytes() and found == found_r
            assert stats()["small"] == (n <= SMALL_MAXN) and stats()["iterations"] == info["iterations"]


@pytest.mark.parametrize("device", (False, True))
def test_x_indices_with_repeats(gpu, monkeypatch, device):
    X = R.cloud(500, 5, 21, np.float32)
    rs = np.random.RandomState(4)
    for nn, K in ((108, 8), (300, 8)):
        idx = rs.randint(0, 500, nn).astype(np.int64)
        idx[5:9] = idx[0]   # repeats: rows at distance 0
        D = R._oracle().pdist(X, "euclidean", X_indices=idx)
        init = starts(nn, K, 0, 6)
        ids_r, err_r, found_r, info = R.kmedoids(K, D, 0, init[0])
        for small in ((1, 0) if nn <= SMALL_MAXN else (0,)):
            monkeypatch.setenv("MSM_KMEDOIDS_SMALL", str(small))
            ids, err, found = lib_fit(X, "euclidean", K, 0, init, X_indices=idx, device=device)
            assert np.array_equal(ids, ids_r) and np.float64(err).tobytes() == np.float64(err_r).tobytes() and found == found_r
            assert stats()["small"] == small and stats()["iterations"] == info["iterations"]
            if not device:   # the estimators gather host rows themselves: the library's own host X_indices route, directly
                from msmbuilder_amd import _lib
                out = np.full(nn, -7, dtype=np.int64)
                e, f = C.c_double(-7.0), C.c_int64(-7)
                i64 = np.ascontiguousarray(init, dtype=np.int64)
                rc = _lib.lib().msm_kmedoids_fit_f32(X.ctypes.data, 500, 5, b"euclidean", idx.ctypes.data, nn, K, 0,
                                                     i64.ctypes.data, out.ctypes.data, C.byref(e), C.byref(f), 0)
                assert rc == 0 and np.array_equal(out, ids_r) and e.value == err_r and f.value == found_r


# ---- errors and quirks -----------------------------------------------------------------------------------------------
def test_bad_initial_assignments(gpu):
    from msmbuilder_amd import _lib
    X, D = matrix(65)
    ok = starts(65, 4, 0, 1)[0]
    empty = np.where(ok == 2, 3, ok)
    high = ok.copy()
    high[7] = 4
    for bad in (empty, high):
        rc, ids, err, found = lib_kmedoids(D, 65, 4, 0, bad[None, :])
        assert rc == _lib.MSM_ERR_INVALID and np.all(ids == -7) and err == -7.0 and found == -7


def test_hand_cases_through_the_library(gpu, monkeypatch):
    """The literal expectations of tests/test_kmedoids_ref.py's hand cases, bound to the library on both paths."""
    def run(D, n, K, start, want_ids, want_err, want_found, want_iter=None):
        for small in (1, 0):
            monkeypatch.setenv("MSM_KMEDOIDS_SMALL", str(small))
            rc, ids, err, found = lib_kmedoids(np.asarray(D, dtype=np.float64), n, K, 0, np.asarray(start)[None, :])
            assert rc == 0 and ids.tolist() == want_ids and err == want_err and found == want_found, (n, K, small)
            assert stats()["small"] == small and (want_iter is None or stats()["iterations"] == want_iter)
    run([3.0], 2, 1, [0, 0], [0, 0], R.DBL_MAX, 0)
    run([3.0], 2, 2, [1, 0], [0, 1], 0.0, 1)          # labels swapped: medoids [1, 0] differ from the labels -> copied
    run([3.0], 2, 2, [0, 1], [0, 1], R.DBL_MAX, 0)    # the identity: every label is its medoid's index
    n = 6
    D = np.arange(1.0, n * (n - 1) // 2 + 1)
    run(D, n, n, list(range(n)), list(range(n)), R.DBL_MAX, 0)
    run(D, n, n, list(range(n))[::-1], list(range(n)), 0.0, 1)
    run(np.full(21, 0.5), 7, 3, [2, 2, 1, 0, 1, 0, 2], [0, 1, 2, 1, 1, 1, 1], 2.0, 1, want_iter=2)   # all ties


@pytest.mark.parametrize("n", (100, 300))
def test_negative_distances_are_refused(gpu, monkeypatch, n):
    """Distances are >= 0 (the general path orders summed costs by their bit patterns): a negative entry of a caller's
    matrix is MSM_ERR_INVALID on both paths, host and device matrix, nothing written; -0.0 is a zero."""
    from msmbuilder_amd import _lib
    X, D = matrix(n)
    bad = np.array(D)
    bad[len(bad) // 3] = -1e-300
    zero = np.array(D)
    zero[len(zero) // 3] = -0.0
    init = starts(n, 4, 1, 0)
    for small in ((1, 0) if n <= SMALL_MAXN else (0,)):
        monkeypatch.setenv("MSM_KMEDOIDS_SMALL", str(small))
        for on_device in (False, True):
            rc, ids, err, found = lib_kmedoids(bad, n, 4, 1, init, on_device)
            assert rc == _lib.MSM_ERR_INVALID and "negative" in _lib.last_error()
            assert np.all(ids == -7) and err == -7.0 and found == -7
    check_loop(zero, n, 4, 1, init, monkeypatch)


@pytest.mark.parametrize("n", (100, 300))
@pytest.mark.parametrize("what", ("nan", "inf"))
def test_nonfinite_distances_are_refused(gpu, monkeypatch, n, what):
    """A NaN row and an inf row: MSM_ERR_NONFINITE on both paths, nothing written; ValueError from the estimators."""
    from msmbuilder_amd import _lib
    from msmbuilder_amd.cluster.kmedoids import _KMedoids
    from msmbuilder_amd.cluster.minibatchkmedoids import _MiniBatchKMedoids
    X = R.cloud(n, 3, 2).copy()
    X[n // 2, 1] = np.nan if what == "nan" else np.inf
    init = np.ascontiguousarray(starts(n, 3, 1, 0), dtype=np.int64)
    L = _lib.lib()
    for small in ((1, 0) if n <= SMALL_MAXN else (0,)):
        monkeypatch.setenv("MSM_KMEDOIDS_SMALL", str(small))
        ids = np.full(n, -7, dtype=np.int64)
        err, found = C.c_double(-7.0), C.c_int64(-7)
        rc = L.msm_kmedoids_fit_f64(X.ctypes.data, n, 3, b"euclidean", None, 0, 3, 1, init.ctypes.data, ids.ctypes.data,
                                    C.byref(err), C.byref(found), 0)
        assert rc == _lib.MSM_ERR_NONFINITE and np.all(ids == -7) and err.value == -7.0 and found.value == -7
    with pytest.raises(ValueError, match="NaN or infinite"):
        _KMedoids(n_clusters=3, random_state=0).fit(X)
    with pytest.raises(ValueError, match="NaN or infinite"):
        _MiniBatchKMedoids(n_clusters=3, batch_size=n, random_state=0).fit(X)


def test_dbl_max_corner_and_argument_errors_through_the_estimator(gpu):
    from msmbuilder_amd import KMedoids
    one = KMedoids(n_clusters=1, random_state=0).fit([np.ones((1, 3), dtype=np.float32)])
    assert one.inertia_ == R.DBL_MAX and one.labels_[0].tolist() == [0] and one.cluster_ids_.tolist() == [[0, 0]]
    two = KMedoids(n_clusters=1, random_state=0).fit([np.array([[0.0], [2.0]])])   # labels [0, 0] = medoid ids [0, 0]
    assert two.inertia_ == R.DBL_MAX and two.labels_[0].tolist() == [0, 0]
    with pytest.raises(ValueError, match=r"Number of clusters requested \(9\) greater than number of elements \(4\)"):
        KMedoids(n_clusters=9).fit([np.zeros((4, 2))])


# ---- the estimators --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GOLDEN_KMEDOIDS, ids=lambda c: "%s-%s" % (c[0], c[1]))
def test_kmedoids_estimator(gpu, golden, case):
    """Against the golden file AND the reference loop (n = 90 ... 195: both paths), host and device rows; the generator
    is left where the reference leaves it."""
    from msmbuilder_amd.cluster.kmedoids import _KMedoids
    metric, dn, n, m, seed, K, npasses = case
    X = R.cloud(n, m, seed, R.DT[dn], metric)
    r = R.kmedoids_estimator(X, K, npasses, metric, seed)
    p = "km_%s_%s_" % (metric, dn)
    for device in (False, True):
        Xin = X
        if device:
            import torch
            Xin = torch.as_tensor(X, device="cuda")
        rs = np.random.RandomState(seed)
        est = _KMedoids(n_clusters=K, n_passes=npasses, metric=metric, random_state=rs).fit(Xin)
        assert np.array_equal(est.labels_, golden[p + "labels"]) and np.array_equal(est.labels_, r["labels"])
        assert np.array_equal(est.cluster_ids_, golden[p + "cluster_ids"])
        assert isinstance(est.cluster_centers_, np.ndarray) and est.cluster_centers_.dtype == X.dtype
        assert np.array_equal(bits(est.cluster_centers_), bits(golden[p + "centers"]))
        assert np.float64(est.inertia_).tobytes() == golden[p + "inertia"].tobytes() == np.float64(r["inertia"]).tobytes()
        assert np.array_equal(host(est.predict(Xin.flip(0).contiguous() if device else X[::-1].copy())), golden[p + "predict"])
        assert rs.random_sample() == float(golden[p + "next"])
        assert stats()["small"] == (n <= SMALL_MAXN)


def test_kmedoids_casts_other_dtypes_to_float64(gpu):
    from msmbuilder_amd.cluster.kmedoids import _KMedoids
    X = np.rint(R.cloud(70, 3, 3) * 4).astype(np.int32)
    est = _KMedoids(n_clusters=4, random_state=1).fit(X)
    r = R.kmedoids_estimator(X, 4, 1, "euclidean", 1)
    assert np.array_equal(est.labels_, r["labels"]) and est.inertia_ == r["inertia"]
    assert est.cluster_centers_.dtype == np.float64 and np.array_equal(est.cluster_centers_, r["centers"])
    assert np.array_equal(est.predict(X), est.predict(X.astype(np.float64)))


@pytest.mark.parametrize("device", (False, True))
def test_sequence_lists(gpu, golden, device):
    """A ragged list of four trajectories, host and device-resident: (trajectory, frame) pairs, labels per trajectory."""
    from msmbuilder_amd import KMedoids, MiniBatchKMedoids
    seqs = R.golden_sequences()
    lengths = [len(s) for s in seqs]
    given = seqs
    if device:
        import torch
        given = [torch.as_tensor(s, device="cuda") for s in seqs]
    est = KMedoids(n_clusters=5, n_passes=2, random_state=3).fit(given)
    assert np.array_equal(est.cluster_ids_, golden["seq_km_pairs"])
    assert [len(l) for l in est.labels_] == lengths
    assert np.array_equal(np.concatenate([host(l) for l in est.labels_]), golden["seq_km_labels"])
    assert np.array_equal(bits(est.cluster_centers_), bits(golden["seq_km_centers"]))
    assert np.float64(est.inertia_).tobytes() == golden["seq_km_inertia"].tobytes()
    assert np.array_equal(np.concatenate([host(l) for l in est.predict(given)]), golden["seq_km_predict"])
    assert est.summarize() == str(golden["seq_km_summarize"])
    again = KMedoids(n_clusters=5, n_passes=2, random_state=3).fit_predict(given)
    assert np.array_equal(np.concatenate([host(l) for l in again]), golden["seq_km_labels"])
    mb = MiniBatchKMedoids(n_clusters=5, batch_size=40, random_state=3).fit(given)
    assert np.array_equal(mb.cluster_ids_, golden["seq_mb_pairs"])
    assert np.array_equal(np.concatenate([host(l) for l in mb.labels_]), golden["seq_mb_labels"])
    assert np.array_equal(bits(mb.cluster_centers_), bits(golden["seq_mb_centers"]))
    assert np.float64(mb.inertia_).tobytes() == golden["seq_mb_inertia"].tobytes()
    assert mb.summarize() == str(golden["seq_mb_summarize"])


@pytest.mark.parametrize("case", R.GOLDEN_MINIBATCH, ids=lambda c: "%s-%s" % (c[0], c[1]))
def test_minibatch_estimator(gpu, golden, monkeypatch, case):
    """Against the golden file and the reference loop; these three run out max_iter (24, 15 and 2 steps), the last with
    batch_size (300) > n_samples (250).  Both paths of the step."""
    from msmbuilder_amd.cluster.minibatchkmedoids import _MiniBatchKMedoids
    metric, dn, n, m, seed, kw = case
    X = R.cloud(n, m, seed, R.DT[dn], metric)
    r = R.minibatch_estimator(X, metric=metric, random_state=seed, **kw)
    assert r["steps"] == int(kw["max_iter"] * int(np.ceil(n / kw["batch_size"])))
    p = "mb_%s_%s_" % (metric, dn)
    for small in ((1, 0) if kw["n_clusters"] + kw["batch_size"] <= SMALL_MAXN else (0,)):
        monkeypatch.setenv("MSM_KMEDOIDS_SMALL", str(small))
        rs = np.random.RandomState(seed)
        est = _MiniBatchKMedoids(metric=metric, random_state=rs, **kw).fit(X)
        assert est.n_steps_ == r["steps"] and stats()["small"] == small
        assert np.array_equal(est.labels_, golden[p + "labels"]) and np.array_equal(est.labels_, r["labels"])
        assert np.array_equal(est.cluster_ids_, golden[p + "cluster_ids"])
        assert np.array_equal(bits(est.cluster_centers_), bits(golden[p + "centers"]))
        assert np.float64(est.inertia_).tobytes() == golden[p + "inertia"].tobytes()
        assert np.array_equal(est.predict(X), est.labels_)
        assert rs.random_sample() == float(golden[p + "next"])


def test_minibatch_stops_on_max_no_improvement(gpu):
    from msmbuilder_amd.cluster.minibatchkmedoids import _MiniBatchKMedoids
    import torch
    kw = dict(n_clusters=2, max_iter=40, batch_size=30, max_no_improvement=2)
    X = R.cloud(60, 2, 0)
    r = R.minibatch_estimator(X, random_state=0, **kw)
    assert r["steps"] == 11 < 80   # by the reference loop: stopped long before max_iter * n_batches
    for Xin in (X, torch.as_tensor(X, device="cuda")):
        rs = np.random.RandomState(0)
        est = _MiniBatchKMedoids(random_state=rs, **kw).fit(Xin)
        assert est.n_steps_ == 11
        assert np.array_equal(host(est.labels_), r["labels"]) and np.array_equal(est.cluster_ids_, r["cluster_ids"])
        assert np.array_equal(bits(est.cluster_centers_), bits(r["centers"]))
        assert np.float64(est.inertia_).tobytes() == np.float64(r["inertia"]).tobytes()
    # the generator afterwards: the same next draw as after the reference loop
    a, b = np.random.RandomState(0), np.random.RandomState(0)
    R.minibatch_estimator(X, random_state=a, **kw)
    _MiniBatchKMedoids(random_state=b, **kw).fit(X)
    assert a.random_sample() == b.random_sample()
