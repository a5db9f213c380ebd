"""GPU tests of the divergence tile kernel, the paired-rows kernel and msm_landmark_predict_dmat against the longdouble
restatement of tests/divergence_ref.py, within its per-element bound, and of the bit-identities the kernels promise."""
import ctypes as C

import numpy as np
import pytest

import divergence_ref as R

pytestmark = pytest.mark.gpu

DTS = {"f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def plan(gpu):
    out = np.zeros(4, dtype=np.int64)
    gpu.check(gpu.lib().msm_divergence_plan(out.ctypes.data_as(C.POINTER(C.c_int64))))
    TI, TJ, CH, T = (int(x) for x in out)
    assert TI >= 2 and TJ >= 2 and CH >= 2 and T % 64 == 0
    return TI, TJ, CH


@pytest.fixture(scope="module")
def D(gpu):
    from msmbuilder_amd.utils import divergence
    return divergence


def seams(t):
    return [1, 2, t - 1, t, t + 1, 2 * t + 1]


def col_seams(ch):
    return [1, 2, ch - 1, ch, ch + 1, 3 * ch + 1]


def mixed_rows(n, m, seed, dt):
    """Normalised rows with many zeros, then the special rows, then un-normalised ones; n rows in all."""
    X = np.concatenate([R.rows(n, m, seed, dt), R.special_rows(m, dt), R.rows(3, m, seed + 1, dt, normalise=False)])
    return np.ascontiguousarray(X[np.random.RandomState(seed).permutation(len(X))[:n]])


# ---- values against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_cdist_seams_of_the_tile(D, plan, kind, dn):
    """nA over the seams of the tile rows against nB over the seams of the tile columns (nA != nB in most pairs), m
    straddling one chunk."""
    TI, TJ, CH = plan
    m = CH + 1
    worst = 0.0
    for k, nA in enumerate(seams(TI)):
        nB = seams(TJ)[::-1][k]
        XA, XB = mixed_rows(nA, m, 10 + k, DTS[dn]), mixed_rows(nB, m, 20 + k, DTS[dn])
        got = D.divergence_cdist(XA, XB, kind)
        want, bound = R.cdist(XA, XB, kind)
        assert got.dtype == np.float64 and got.shape == (nA, nB)
        worst = max(worst, R.assert_within(got, want, bound, "%s %s nA=%d nB=%d" % (kind, dn, nA, nB)))
    print("largest error / bound: %.3f" % worst)


@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_pdist_seams_of_the_tile(D, plan, kind, dn):
    TI, TJ, CH = plan
    for k, n in enumerate(seams(TI)):
        X = mixed_rows(n, CH - 1, 30 + k, DTS[dn])
        got = D.divergence_pdist(X, kind)
        want, bound = R.pdist(X, kind)
        assert got.shape == (n * (n - 1) // 2,)
        R.assert_within(got, want, bound, "%s %s n=%d" % (kind, dn, n))


@pytest.mark.parametrize("kind", R.KINDS)
def test_column_chunk_seams(D, plan, kind):
    TI, TJ, CH = plan
    for k, m in enumerate(col_seams(CH)):
        for dn in ("f32", "f64"):
            XA, XB = mixed_rows(TI + 1, m, 40 + k, DTS[dn]), mixed_rows(TJ - 1, m, 50 + k, DTS[dn])
            want, bound = R.cdist(XA, XB, kind)
            R.assert_within(D.divergence_cdist(XA, XB, kind), want, bound, "%s %s m=%d cdist" % (kind, dn, m))
            want, bound = R.pdist(XA, kind)
            R.assert_within(D.divergence_pdist(XA, kind), want, bound, "%s %s m=%d pdist" % (kind, dn, m))


@pytest.mark.parametrize("kind", R.KINDS)
def test_device_pitched_and_indexed_inputs(D, plan, kind):
    """Device tensors give the host call's bits and stay on the device; a pitched (non-contiguous) view is copied;
    X_indices may repeat a row and run out of order."""
    import torch
    TI, TJ, CH = plan
    X = mixed_rows(2 * TI + 1, CH + 3, 60, np.float64)
    host = D.divergence_pdist(X, kind)
    Xd = torch.as_tensor(X, device="cuda")
    dev = D.divergence_pdist(Xd, kind)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host, equal_nan=True)
    kept = D.divergence_pdist(X, kind, device=True)
    assert kept.is_cuda and np.array_equal(kept.cpu().numpy(), host, equal_nan=True)
    wide = np.zeros((len(X), 2 * X.shape[1]))
    wide[:, ::2] = X
    assert np.array_equal(D.divergence_pdist(wide[:, ::2], kind), host, equal_nan=True)
    wd = torch.as_tensor(wide, device="cuda")[:, ::2]
    assert not wd.is_contiguous()
    assert np.array_equal(D.divergence_pdist(wd, kind).cpu().numpy(), host, equal_nan=True)
    cd = D.divergence_cdist(Xd, Xd[:TJ + 1], kind)
    assert cd.is_cuda and np.array_equal(cd.cpu().numpy(), D.divergence_cdist(X, X[:TJ + 1], kind), equal_nan=True)
    idx = np.array([5, 0, TI + 2, 5, 2 * TI, 1, 0])
    want = D.divergence_pdist(np.ascontiguousarray(X[idx]), kind)
    assert np.array_equal(D.divergence_pdist(X, kind, X_indices=idx), want, equal_nan=True)
    assert np.array_equal(D.divergence_pdist(Xd, kind, X_indices=idx).cpu().numpy(), want, equal_nan=True)
    ref, bound = R.pdist(X[idx], kind)
    R.assert_within(want, ref, bound, kind + " indexed")


@pytest.mark.parametrize("kind", R.KINDS)
def test_nan_row_and_negative_entry(D, kind):
    X = R.rows(9, 7, 70)
    X[2, 3] = np.nan
    X[5, 1] = -0.25
    got = D.divergence_cdist(X, X, kind)
    want, bound = R.cdist(X, X, kind)
    R.assert_within(got, want, bound, kind)
    off = ~np.eye(9, dtype=bool)
    assert np.all(np.isnan(got[2][off[2]])) and np.all(np.isnan(got[:, 2][off[:, 2]]))
    P = np.array([[-0.5, 1.5]])
    Q = np.array([[0.5, 0.5]])
    assert np.isnan(D.kl_divergence(P, Q, scalar=False)[0])


@pytest.mark.parametrize("kind", ["js_metric", "kl_divergence"])
def test_larger_case_on_sampled_pairs(D, kind):
    n = m = 1100
    X = R.gen(n, 5, 4)
    got = R.squareform(D.divergence_pdist(X, kind), n) if kind != "kl_divergence" else D.divergence_cdist(X, X, kind)
    r = np.random.RandomState(5)
    i, j = r.randint(n, size=2000), r.randint(n, size=2000)
    keep = i != j
    i, j = i[keep], j[keep]
    if kind != "kl_divergence":
        i, j = np.minimum(i, j), np.maximum(i, j)
    want, bound = R.pairs(X[i], X[j], kind)
    R.assert_within(got[i, j], want, bound, kind + " n=m=1100")


# ---- bit-identities ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("kind", R.KINDS)
def test_bit_identity_between_the_forms(D, plan, kind, dn):
    TI, TJ, CH = plan
    n = 2 * TI + 1
    X = mixed_rows(n, CH + 1, 80, DTS[dn])
    sq = D.divergence_cdist(X, X, kind)
    again = D.divergence_cdist(X, X, kind)
    assert np.array_equal(sq, again, equal_nan=True)                      # run to run
    iu = np.triu_indices(n, 1)
    pd = D.divergence_pdist(X, kind)
    assert np.array_equal(pd, sq[iu], equal_nan=True)                    # pdist == upper triangle of cdist
    assert np.array_equal(pd, D.divergence_pdist(X, kind), equal_nan=True)
    fn = getattr(D, kind + "_array")
    for i in (0, 1, TI, n - 1):
        assert np.array_equal(fn(X, X, i), sq[i], equal_nan=True)        # one row against all
    pair_fn = getattr(D, kind)
    assert np.array_equal(pair_fn(X[iu[0]], X[iu[1]], scalar=False), pd, equal_nan=True)   # paired rows
    assert pair_fn(X[3], X[7]) == sq[3, 7]                               # the 1-D form
    finite = ~np.isnan(sq)
    if kind != "kl_divergence":
        assert np.array_equal(sq, sq.T, equal_nan=True)                  # d(i, j) == d(j, i)
    assert np.all(np.diag(sq)[np.diag(finite)] == 0.0)                   # d(i, i) == 0


def test_hand_cases_on_the_device(D):
    P = np.array([0.5, 0.5, 0.0, 0.0])
    Q = np.array([0.0, 0.0, 0.5, 0.5])
    assert D.js_divergence(P, P) == 0.0 and D.js_metric(P, P) == 0.0 and D.kl_divergence(P, P) == 0.0
    assert abs(D.js_divergence(P, Q) - np.log(2.0)) <= (2 * R.LOG_ULP + 3) * R.U * np.log(2.0)   # log, two products, one sum
    assert D.kl_divergence(P, Q) == 0.0                                   # q = 0 under p > 0: nothing, not infinity
    assert D.kl_divergence(np.array([1e-200, 1.0]), np.array([1e-200, 1.0])) == 0.0
    tiny = np.array([5e-324, 1.0])
    assert D.kl_divergence(tiny, np.array([1.0, 1.0])) == 0.0            # a tiny negative sum: clamped
    for kind in R.KINDS:
        for X, Y in ((P, Q), (tiny, np.array([1.0, 1.0])), (np.array([3.0, 1.0, 0.0]), np.array([1.0, 2.0, 5.0]))):
            want, bound = R.pairs(X, Y, kind)
            R.assert_within([getattr(D, kind)(X, Y)], want, bound, kind)
    # 2-D scalar form: the sums over the rows, per KL part
    A, B = R.rows(6, 5, 90), R.rows(6, 5, 91)
    kl = D.kl_divergence(A, B, scalar=False)
    assert D.kl_divergence(A, B) == np.sum(kl)
    assert D.sym_kl_divergence(A, B) == np.sum(kl) + np.sum(D.kl_divergence(B, A, scalar=False))
    M = (A + B) / 2
    js = 0.5 * np.sum(D.kl_divergence(A, M, scalar=False)) + 0.5 * np.sum(D.kl_divergence(B, M, scalar=False))
    assert D.js_divergence(A, B) == js and D.js_metric(A, B) == np.sqrt(js)
    from scipy.stats import entropy
    assert np.array_equal(D.kl_divergence(A, B, manual=False, scalar=False), entropy(A.T, B.T))


# ---- msm_landmark_predict_dmat -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pooling", ["single", "complete", "average", "ward"])
def test_predict_dmat_equals_the_fused_predict(gpu, pooling):
    """Fed the float64 cdist of a vector metric, the matrix form returns the fused kernel's labels and pooled values:
    K = 1, K = L, and a cluster id without a landmark; host, device and row-strided matrices."""
    import torch
    from msmbuilder_amd import libdistance
    from msmbuilder_amd.cluster import agglomerative as A
    rs = np.random.RandomState(7)
    X = rs.randn(700, 5)
    for L, K, labels in ((37, 1, np.zeros(37, int)), (19, 19, rs.permutation(19)), (50, 6, rs.choice([0, 1, 3, 5], 50))):
        lm = X[rs.choice(len(X), L, replace=False)]
        perm, offsets = A.permute_by_cluster(labels, K)
        lmp = np.ascontiguousarray(lm[perm])
        intra = A.within_cluster(libdistance.pdist(lm, "euclidean"), L, labels, K) if pooling == "ward" else None
        want_l, want_p, want_n = A.pooled_predict(X, lmp, offsets, intra, "euclidean", pooling, want_pooled=True)
        Dm = libdistance.cdist(X, lmp, "euclidean")
        got_l, got_p, got_n = A.pooled_predict_dmat(Dm, offsets, intra, pooling, want_pooled=True)
        assert np.array_equal(got_l, want_l) and np.array_equal(got_p, want_p) and got_n == want_n
        wide = np.full((len(X), L + 3), np.nan)
        wide[:, :L] = Dm
        got_l, got_p, _ = A.pooled_predict_dmat(wide[:, :L], offsets, intra, pooling, want_pooled=True)
        assert np.array_equal(got_l, want_l) and np.array_equal(got_p, want_p)
        for Dd in (torch.as_tensor(Dm, device="cuda"), torch.as_tensor(wide, device="cuda")[:, :L]):
            got_l, got_p, _ = A.pooled_predict_dmat(Dd, offsets, intra, pooling, want_pooled=True)
            assert got_l.is_cuda and np.array_equal(got_l.cpu().numpy(), want_l) and np.array_equal(got_p.cpu().numpy(), want_p)


# ---- refusals through the C ABI ----------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(gpu):
    L = gpu.lib()
    X = R.rows(5, 4, 1)
    out = np.zeros(25)
    p, o = X.ctypes.data, out.ctypes.data
    bad = gpu.MSM_ERR_INVALID
    assert L.msm_divergence_cdist_f64(p, 5, p, 5, 4, b"hellinger", o, 0) == gpu.MSM_ERR_METRIC
    assert L.msm_divergence_cdist_f64(p, 5, p, 5, 4, None, o, 0) == gpu.MSM_ERR_METRIC
    assert L.msm_divergence_cdist_f64(None, 5, p, 5, 4, b"js_metric", o, 0) == bad
    assert L.msm_divergence_cdist_f64(p, 5, p, 5, 4, b"js_metric", None, 0) == bad
    assert L.msm_divergence_cdist_f64(p, 5, p, 5, 0, b"js_metric", o, 0) == bad
    assert L.msm_divergence_cdist_f64(p, -1, p, 5, 4, b"js_metric", o, 0) == bad
    assert L.msm_divergence_pdist_f64(p, 5, 4, None, 0, b"nope", o, 0) == gpu.MSM_ERR_METRIC
    assert L.msm_divergence_pdist_f64(None, 5, 4, None, 0, b"js_metric", o, 0) == bad
    assert L.msm_divergence_pdist_f64(p, 5, 4, None, 0, b"js_metric", None, 0) == bad
    assert L.msm_divergence_pdist_f64(p, 5, 0, None, 0, b"js_metric", o, 0) == bad
    assert L.msm_divergence_pdist_f64(p, -2, 4, None, 0, b"js_metric", o, 0) == bad
    idx = np.array([0, 9], dtype=np.int64)
    assert L.msm_divergence_pdist_f64(p, 5, 4, idx.ctypes.data, 2, b"js_metric", o, 0) == bad
    assert L.msm_divergence_pdist_f64(p, 5, 4, idx.ctypes.data, -1, b"js_metric", o, 0) == bad
    assert L.msm_divergence_rows_f64(p, p, 5, 4, b"nope", o) == gpu.MSM_ERR_METRIC
    assert L.msm_divergence_rows_f64(p, None, 5, 4, b"js_metric", o) == bad
    assert L.msm_divergence_rows_f64(p, p, 5, 0, b"js_metric", o) == bad
    assert L.msm_divergence_rows_f64(p, p, -1, 4, b"js_metric", o) == bad
    assert L.msm_divergence_plan(None) == bad
    # the linkage and the predict: kl_divergence is refused, the symmetric kinds are taken
    Z = np.zeros((4, 4))
    for sfx in ("f32", "f64"):
        Xs = X.astype(DTS[sfx])
        fit = getattr(L, "msm_linkage_fit_" + sfx)
        assert fit(Xs.ctypes.data, 5, 4, b"kl_divergence", None, 0, b"ward", Z.ctypes.data, 0) == gpu.MSM_ERR_METRIC
        assert b"not symmetric" in L.msm_last_error()
        assert fit(Xs.ctypes.data, 5, 4, b"js_metric", None, 0, b"ward", Z.ctypes.data, 0) == gpu.MSM_OK
        off = np.array([0, 5], dtype=np.int64)
        lab = np.zeros(5, dtype=np.int64)
        neg = C.c_int(0)
        pred = getattr(L, "msm_landmark_predict_" + sfx)
        args = (Xs.ctypes.data, 5, 4, Xs.ctypes.data, 5, off.ctypes.data, 1, None)
        assert pred(*args, b"kl_divergence", b"average", lab.ctypes.data, None, C.byref(neg), 0) == gpu.MSM_ERR_METRIC
        assert pred(*args, b"sym_kl_divergence", b"average", lab.ctypes.data, None, C.byref(neg), 0) == gpu.MSM_OK
    Dm = np.zeros((5, 5))
    off = np.array([0, 5], dtype=np.int64)
    lab = np.zeros(5, dtype=np.int64)
    neg = C.c_int(0)
    dm = L.msm_landmark_predict_dmat
    assert dm(Dm.ctypes.data, 5, 5, 5, off.ctypes.data, 1, None, b"median", lab.ctypes.data, None, C.byref(neg), 0) == bad
    assert dm(None, 5, 5, 5, off.ctypes.data, 1, None, b"average", lab.ctypes.data, None, C.byref(neg), 0) == bad
    assert dm(Dm.ctypes.data, 5, 5, 5, None, 1, None, b"average", lab.ctypes.data, None, C.byref(neg), 0) == bad
    assert dm(Dm.ctypes.data, 5, 5, 4, off.ctypes.data, 1, None, b"average", lab.ctypes.data, None, C.byref(neg), 0) == bad
    assert dm(Dm.ctypes.data, -1, 5, 5, off.ctypes.data, 1, None, b"average", lab.ctypes.data, None, C.byref(neg), 0) == bad
    assert dm(Dm.ctypes.data, 5, 5, 5, off.ctypes.data, 1, None, b"ward", lab.ctypes.data, None, C.byref(neg), 0) == bad
    off[1] = 4
    assert dm(Dm.ctypes.data, 5, 5, 5, off.ctypes.data, 1, None, b"average", lab.ctypes.data, None, C.byref(neg), 0) == bad
