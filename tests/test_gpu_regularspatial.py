"""GPU tier: RegularSpatial / msm_regspatial_fit_* held to EQUALITY with the sequential reference loop
(tests/regularspatial_ref.py: one oracle `dist` call per row) and with the golden file written by the reference's own
regularspatial.py -- centre ids and n_clusters_ equal, cluster_centers_ bit-equal to X[ids], predict equal to
assign_nearest on those centres.  No tolerance anywhere: the algorithm is deterministic and every decision is a
comparison of a distance the library reproduces bit for bit.

Shapes are the smallest that reach each seam of the device loop: the block seams (forced with the `block_rows`
override), the register / row-tile screen paths, the LDS centre tile, the centre list's initial capacity (4,096).
Block-seam cases: the stats must show ceil(n / block_rows) blocks -- more than one whenever n > block_rows (n = B - 1
and n = B are one block by construction) -- and, wherever a block exists that chose two centres (rounds > blocks), a
block whose survivors were resolved in more than one round."""
import ctypes as C
import functools
import os
import pickle

import numpy as np
import pytest

import regularspatial_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regularspatial_golden.npz")
DT = {"f32": np.float32, "f64": np.float64}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def general_case(name, metric, which, dn):
    """(X, d_min, reference ids): computed once, shared, never written to."""
    X = np.ascontiguousarray(R.general_input(name, metric).astype(DT[dn]))
    X.setflags(write=False)
    d_min = R.GENERAL_DMIN[(name, metric)][which]
    return X, d_min, R.ref_fit(X, d_min, metric)


def fit(X, d_min, metric="euclidean", block_rows=0):
    from msmbuilder_amd.cluster.regularspatial import _RegularSpatial, last_stats
    est = _RegularSpatial(d_min=d_min, metric=metric)
    est._block_rows = block_rows
    est.fit(X)
    return est, last_stats()


def check(est, X, ref_ids, metric, predict=True):
    """The issue's equalities.  X: the host rows."""
    from oracle.libdistance_oracle import Oracle
    assert est.n_clusters_ == len(ref_ids)
    assert est.cluster_center_indices_ == list(ref_ids)
    assert est.cluster_centers_.dtype == X.dtype
    assert np.array_equal(bits(est.cluster_centers_), bits(X[np.asarray(ref_ids)]))
    if predict:
        with np.errstate(all="ignore"):
            want, _ = Oracle().assign_nearest(X, np.ascontiguousarray(X[np.asarray(ref_ids)]), metric)
        assert np.array_equal(np.asarray(est.predict(X)), want)


GENERAL = [(name, metric, which) for (name, metric), ds in sorted(R.GENERAL_DMIN.items()) for which in range(len(ds))]


# ---- 1. general ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("name,metric,which", GENERAL)
def test_general(gpu, name, metric, which, dn):
    X, d_min, ref = general_case(name, metric, which, dn)
    assert 32 <= len(ref) <= len(X) // 4, "a trivial case cannot stand for a real one (reference K = %d)" % len(ref)
    if (name, metric) == ("cloud", "euclidean"):
        assert len(ref) == (250, 747)[which]      # the numpy calibration of the case table
    est, st = fit(X, d_min, metric)
    print("general", name, metric, dn, "d_min", d_min, "K", est.n_clusters_, "reference", len(ref), st)
    check(est, X, ref, metric)
    assert st["rounds"] == len(ref) and st["blocks"] >= 2


# ---- 2. block seams --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_case(n, dn):
    X = np.ascontiguousarray(R.walk(5 * 4096 + 17, 10, seed=5)[:n].astype(DT[dn]))
    X.setflags(write=False)
    return X, R.ref_fit(X, 1.0, "euclidean")


@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("B", [64, 256, 4096])
@pytest.mark.parametrize("shape", ["B-1", "B", "B+1", "2B+1", "5B+17"])
def test_block_seams(gpu, B, shape, dn):
    n = {"B-1": B - 1, "B": B, "B+1": B + 1, "2B+1": 2 * B + 1, "5B+17": 5 * B + 17}[shape]
    X, ref = seam_case(n, dn)
    forced, st = fit(X, 1.0, block_rows=B)
    free, _ = fit(X, 1.0)
    print("seam B", B, "n", n, dn, "K", forced.n_clusters_, "reference", len(ref), st)
    check(forced, X, ref, "euclidean", predict=False)
    assert free.cluster_center_indices_ == forced.cluster_center_indices_
    assert np.array_equal(bits(free.cluster_centers_), bits(forced.cluster_centers_))
    assert st["blocks"] == -(-n // B)
    if n > B:
        assert st["blocks"] > 1
    assert st["rounds"] == len(ref)
    assert len(ref) >= 2 * st["blocks"], "the case must put several centres into a block"
    assert st["rounds"] > st["blocks"]        # pigeonhole: some block's survivors took more than one round


# ---- 3. widths -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def width_case(m, metric, dn):
    from oracle.libdistance_oracle import Oracle
    X = np.ascontiguousarray(R.walk(4096, m, seed=7).astype(DT[dn]))
    X.setflags(write=False)
    with np.errstate(all="ignore"):
        d_min = 0.25 * float(np.median(Oracle().dist(X, X[0], metric)))   # from the data's own scale, not from the code under test
    return X, d_min, R.ref_fit(X, d_min, metric)


@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("place", ["host", "device_offset_by_one_element"])
@pytest.mark.parametrize("metric", ["euclidean", "canberra"])
@pytest.mark.parametrize("m", [1, 3, 16, 17, 32, 33, 171, 512])
def test_widths(gpu, m, metric, place, dn):
    import torch
    X, d_min, ref = width_case(m, metric, dn)
    assert len(ref) >= 8
    rows = X
    if place != "host":
        # a sliced tensor: the rows start one ELEMENT into the allocation, so no row is 16-byte aligned
        flat = torch.empty(X.size + 1, dtype=torch.float32 if dn == "f32" else torch.float64, device="cuda")
        flat[1:] = torch.from_numpy(X.reshape(-1).copy()).cuda()
        rows = flat[1:].view(X.shape)
        assert rows.data_ptr() % 16 != 0
    est, st = fit(rows, d_min, metric, block_rows=1024)
    print("width", m, metric, place, dn, "K", est.n_clusters_, "reference", len(ref), st)
    check(est, X, ref, metric, predict=(place == "host"))
    assert st["blocks"] == 4


# ---- 4. centre list --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "f64"])
def test_k_crosses_an_lds_centre_tile(gpu, dn):
    # the register-path screen stages 16 KiB of centres: 1,024 float32 / 512 float64 centres of 3 (padded to 4) features
    X = np.ascontiguousarray(R.cloud(6000, 3, seed=8).astype(DT[dn]))
    ref = R.ref_fit(X, 0.25)
    assert len(ref) > 1024 + 64
    est, st = fit(X, 0.25)
    print("lds tile", dn, "K", est.n_clusters_, st)
    check(est, X, ref, "euclidean")


@pytest.mark.parametrize("dn", ["f32", "f64"])
def test_k_crosses_the_lists_initial_capacity(gpu, dn):
    X = np.ascontiguousarray((R.cloud(8000, 3, seed=9) * 10.0).astype(DT[dn]))
    ref = R.ref_fit(X, 0.5)
    assert 4096 < len(ref) < len(X)
    for B in (0, 256):
        est, st = fit(X, 0.5, block_rows=B)
        print("capacity", dn, "B", B, "K", est.n_clusters_, st)
        check(est, X, ref, "euclidean", predict=False)
        assert st["growths"] >= 1


@functools.lru_cache(maxsize=None)
def duplicate_rows(dn):
    rs = np.random.RandomState(10)
    base = rs.randn(3000, 4)
    X = np.concatenate([base, base[rs.randint(0, 3000, 500)]])
    X = np.ascontiguousarray(X[rs.permutation(len(X))].astype(DT[dn]))
    assert len(np.unique(X, axis=0)) == 3000
    return X


@pytest.mark.parametrize("dn", ["f32", "f64"])
def test_d_min_zero_skips_exact_duplicates(gpu, dn):
    X = duplicate_rows(dn)
    _, first = np.unique(X, axis=0, return_index=True)
    est, st = fit(X, 0.0)
    assert est.n_clusters_ == 3000
    assert est.cluster_center_indices_ == sorted(first.tolist())     # the first occurrence of every distinct row
    assert len(np.unique(est.cluster_centers_, axis=0)) == 3000
    check(est, X, R.ref_fit(X, 0.0), "euclidean", predict=False)


@pytest.mark.parametrize("dn", ["f32", "f64"])
def test_negative_d_min_takes_every_row(gpu, dn):
    X = duplicate_rows(dn)
    est, st = fit(X, -1.0)
    assert est.cluster_center_indices_ == list(range(len(X)))
    assert np.array_equal(bits(est.cluster_centers_), bits(X))
    assert st["rounds"] == len(X)


@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("d_min", [np.inf, 1e300])
def test_huge_d_min_keeps_row_zero_only(gpu, d_min, dn):
    X = duplicate_rows(dn)
    est, st = fit(X, d_min)
    assert est.cluster_center_indices_ == [0] and est.n_clusters_ == 1
    assert np.array_equal(bits(est.cluster_centers_), bits(X[:1]))


# ---- 5. exact ties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("metric,d_min", [("cityblock", 2.0), ("cityblock", 3.0), ("hamming", 0.5), ("hamming", 0.25),
                                          ("chebyshev", 2.0), ("chebyshev", 1.0)])
def test_exact_ties(gpu, metric, d_min, dn):
    from oracle.libdistance_oracle import Oracle
    X = np.ascontiguousarray(R.lattice().astype(DT[dn]))
    ref = R.ref_fit(X, d_min, metric)
    D = Oracle().cdist(X, np.ascontiguousarray(X[ref]), metric)
    assert (D == d_min).sum() > 1000, "d == d_min must occur constantly"
    for B in (0, 256):
        est, st = fit(X, d_min, metric, block_rows=B)
        print("ties", metric, d_min, dn, "B", B, "K", est.n_clusters_, "reference", len(ref), st)
        check(est, X, ref, metric, predict=(B == 0))


# ---- 6. NaN / inf rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("metric", ["euclidean", "cityblock", "chebyshev", "canberra", "braycurtis"])
def test_nan_and_inf_rows(gpu, metric, dn):
    X = np.array(R.walk(3000, 5, seed=11).astype(DT[dn]))
    d_min = {"euclidean": 0.8, "cityblock": 1.5, "chebyshev": 0.5, "canberra": 1.5, "braycurtis": 0.2}[metric]
    rs = np.random.RandomState(12)
    nan_rows = np.sort(rs.choice(np.arange(1, 3000), 40, replace=False))
    Y = X.copy()
    Y[nan_rows, rs.randint(0, 5, 40)] = np.nan
    ref = R.ref_fit(Y, d_min, metric)
    assert len(ref) > 20
    # chebyshev's running maximum and canberra's `denominator > 0` test both SKIP a NaN coordinate (the reference's
    # arithmetic, reproduced by the oracle), so only for the other metrics is a NaN row's every distance NaN
    propagates = metric not in ("chebyshev", "canberra")
    if propagates:
        assert not set(ref) & set(nan_rows.tolist())                 # never centres ...
        keep = np.setdiff1d(np.arange(3000), nan_rows)
        assert ref == [int(keep[i]) for i in R.ref_fit(np.ascontiguousarray(Y[keep]), d_min, metric)]   # ... and they block no one
    for B in (0, 64):
        est, _ = fit(Y, d_min, metric, block_rows=B)
        check(est, Y, ref, metric, predict=False)
    # NaN in row 0: every distance is NaN (where NaN propagates), nothing else is ever a centre
    Z = X.copy()
    Z[0, 2] = np.nan
    ref0 = R.ref_fit(Z, d_min, metric)
    if propagates:
        assert ref0 == [0]
    est, _ = fit(Z, d_min, metric)
    check(est, Z, ref0, metric, predict=False)
    # +-inf coordinates (inf - inf = NaN, inf - finite = inf): whatever the reference loop decides
    W = X.copy()
    inf_rows = rs.choice(np.arange(1, 3000), 30, replace=False)
    W[inf_rows, rs.randint(0, 5, 30)] = np.where(rs.rand(30) < 0.5, np.inf, -np.inf)
    ref = R.ref_fit(W, d_min, metric)
    for B in (0, 64):
        est, _ = fit(W, d_min, metric, block_rows=B)
        check(est, W, ref, metric, predict=False)


# ---- 7. placement and interface --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


def golden_input(metric, dn):
    X = R.walk(3000, 5, seed=1)
    if metric in ("hamming", "jaccard"):
        X = np.rint(X)
    return np.ascontiguousarray(X.astype(DT[dn]))


@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("metric", R.METRICS)
def test_golden_of_the_references_own_file(gpu, golden, metric, dn):
    X = golden_input(metric, dn)
    p = "%s_%s_" % (metric, dn)
    est, _ = fit(X, float(golden[p + "d_min"]), metric, block_rows=512)
    assert est.cluster_center_indices_ == golden[p + "ids"].tolist()
    assert np.array_equal(bits(est.cluster_centers_), bits(golden[p + "centers"]))
    assert np.array_equal(np.asarray(est.predict(X)), golden[p + "predict"])


@pytest.mark.parametrize("dn", ["f32", "f64"])
def test_host_rows_and_device_rows_agree(gpu, dn):
    import torch
    X, d_min, ref = general_case("walk", "euclidean", 0, dn)
    Xd = torch.from_numpy(np.array(X)).cuda()
    a, _ = fit(X, d_min)
    b, _ = fit(Xd, d_min)
    check(b, X, ref, "euclidean", predict=False)
    assert a.cluster_center_indices_ == b.cluster_center_indices_
    assert isinstance(b.cluster_centers_, np.ndarray) and np.array_equal(bits(a.cluster_centers_), bits(b.cluster_centers_))
    lab = b.predict(Xd)
    assert lab.is_cuda and np.array_equal(lab.cpu().numpy(), np.asarray(a.predict(X)))


def test_ragged_list_of_sequences_gives_the_golden_pairs(gpu, golden):
    import torch
    from msmbuilder_amd import RegularSpatial
    seqs = R.golden_sequences()
    for place in ("host", "device"):
        given = seqs if place == "host" else [torch.from_numpy(s).cuda() for s in seqs]
        est = RegularSpatial(d_min=float(golden["seq_d_min"])).fit(given)
        assert est.cluster_center_indices_.shape == (int(golden["seq_n_clusters"]), 2)
        assert np.array_equal(est.cluster_center_indices_, golden["seq_pairs"])
        assert est.n_clusters_ == int(golden["seq_n_clusters"])
        assert np.array_equal(bits(est.cluster_centers_), bits(golden["seq_centers"]))
        labels = est.predict(given)
        assert len(labels) == len(seqs)
        got = np.concatenate([np.asarray(l.cpu() if hasattr(l, "cpu") else l) for l in labels])
        assert np.array_equal(got, golden["seq_predict"])
        assert est.summarize() == str(golden["seq_summarize"])
        again = RegularSpatial(d_min=float(golden["seq_d_min"])).fit_predict(given)
        assert all(np.array_equal(np.asarray(a.cpu() if hasattr(a, "cpu") else a), np.asarray(b.cpu() if hasattr(b, "cpu") else b))
                   for a, b in zip(again, labels))
        assert np.array_equal(np.concatenate([np.asarray(t.cpu() if hasattr(t, "cpu") else t) for t in est.transform(given)]), got)


def test_single_sequence_one_row_pickle_bytes_metric(gpu, golden):
    from msmbuilder_amd import RegularSpatial
    from msmbuilder_amd.cluster import RegularSpatial as FromCluster
    from msmbuilder_amd.cluster.regularspatial import _RegularSpatial
    assert FromCluster is RegularSpatial
    X = np.concatenate(R.golden_sequences())
    d_min = float(golden["seq_d_min"])
    ref = R.ref_fit(X, d_min)
    one = RegularSpatial(d_min=d_min).fit([X])
    assert np.array_equal(one.cluster_center_indices_, np.stack([np.zeros(len(ref), int), np.array(ref)], axis=1))
    assert "n_clusters : %d" % len(ref) in one.summarize() and "d_min      : %s" % d_min in one.summarize()
    # one row: it is the only centre
    row = RegularSpatial(d_min=d_min).fit([X[:1]])
    assert row.n_clusters_ == 1 and row.cluster_center_indices_.tolist() == [[0, 0]]
    assert np.asarray(row.predict([X[:7]])[0]).tolist() == [0] * 7
    # pickle round trip, then predict
    back = pickle.loads(pickle.dumps(one))
    assert np.array_equal(back.cluster_center_indices_, one.cluster_center_indices_)
    assert np.array_equal(np.asarray(back.predict([X])[0]), np.asarray(one.predict([X])[0]))
    assert back.get_params() == {"d_min": d_min, "metric": "euclidean"}
    # metric given as bytes
    est = _RegularSpatial(d_min=1.5, metric=b"cityblock").fit(X)
    assert est.cluster_center_indices_ == R.ref_fit(X, 1.5, "cityblock")
    assert np.array_equal(np.asarray(est.predict(X)), np.asarray(_RegularSpatial(1.5, "cityblock").fit(X).predict(X)))
    # fit_predict is fit().predict()
    assert np.array_equal(np.asarray(_RegularSpatial(d_min).fit_predict(X)), np.asarray(_RegularSpatial(d_min).fit(X).predict(X)))


def test_unknown_metric_and_wrong_input(gpu):
    from msmbuilder_amd import KCenters, RegularSpatial
    X = R.cloud(100, 3)
    with pytest.raises(ValueError) as e1:
        RegularSpatial(d_min=1.0, metric="rmsd").fit([X])
    with pytest.raises(ValueError) as e2:
        KCenters(n_clusters=2, metric="rmsd").fit([X])
    assert str(e1.value) == str(e2.value)
    with pytest.raises(TypeError):
        RegularSpatial(d_min=1.0).fit([X.astype(np.int64)])


# ---- 8. C ABI --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [None, b"minkowski", b""])
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_c_abi_rejects_a_null_or_unknown_metric(gpu, kind, metric):
    L = gpu.lib()
    X = np.ascontiguousarray(R.cloud(500, 3).astype(DT[kind]))
    # a finished fit first, so that "outputs untouched" covers the library-owned result as well
    k0 = C.c_int64(-7)
    assert getattr(L, "msm_regspatial_fit_" + kind)(X.ctypes.data, 500, 3, b"euclidean", 0.8, 0, 0, C.byref(k0)) == 0
    ids0 = np.full(k0.value, -1, dtype=np.int64)
    cen0 = np.zeros((k0.value, 3), dtype=X.dtype)
    assert getattr(L, "msm_regspatial_result_" + kind)(ids0.ctypes.data, cen0.ctypes.data) == 0
    assert ids0.tolist() == R.ref_fit(X, 0.8)
    stats0 = (C.c_int64 * 4)()
    assert L.msm_regspatial_last_stats(stats0) == 0
    k = C.c_int64(-7)
    rc = getattr(L, "msm_regspatial_fit_" + kind)(X.ctypes.data, 500, 3, metric, 0.8, 0, 0, C.byref(k))
    assert rc == gpu.MSM_ERR_METRIC
    assert k.value == -7
    assert "unknown metric" in gpu.last_error()
    ids1 = np.full(k0.value, -1, dtype=np.int64)
    cen1 = np.zeros((k0.value, 3), dtype=X.dtype)
    assert getattr(L, "msm_regspatial_result_" + kind)(ids1.ctypes.data, cen1.ctypes.data) == 0
    assert np.array_equal(ids1, ids0) and np.array_equal(cen1, cen0)
    stats1 = (C.c_int64 * 4)()
    assert L.msm_regspatial_last_stats(stats1) == 0 and list(stats1) == list(stats0)
    assert L.msm_regspatial_last_stats(None) == gpu.MSM_ERR_INVALID
