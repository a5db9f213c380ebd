"""GPU tier of the Nystroem kernel map: msm_kernel_map_{f32,f64} / Nystroem / LandmarkNystroem / KernelTICA against the
longdouble restatement under its per-element bound (tests/nystroem_ref.py; held to scikit-learn by
tests/test_nystroem_ref.py) and against the reference's goldens.

Sizes are the smallest that reach each seam of the device code, read from msm_kernel_map_plan: the MFMA's feature depth of 4
(F = 1, 3, 4, 5, 17), the 16-landmark tile (L = 1, 15, 16, 17, 33), the R rows of a workgroup (n = 1, R - 1, R, R + 1,
3 R + 1), the 16-column tile of B (P = 1, 4, L), the largest L whose block still fits in LDS and the first that does not, and
a scratch route cut into several chunks.  Each (F, L) computes ONE reference, for 3 R + 1 rows and L columns; fewer rows and
columns are slices of it (the map is row by row and column by column)."""
import ctypes as C
import functools
import os
import pickle
import warnings

import numpy as np
import pytest

import nystroem_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nystroem_golden.npz")
DTYPES = (np.float32, np.float64)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def KA():
    from msmbuilder_amd.decomposition import kernel_approximation
    return kernel_approximation


def dev(a):
    import torch
    return torch.as_tensor(np.array(a), device="cuda")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint8)


def place(X, how):
    """The rows on the device, on the host, or pitched (a column slice of a wider array) on either."""
    if how == "device":
        return dev(X)
    if how == "host":
        return X
    wide = np.zeros((X.shape[0], X.shape[1] + 3), dtype=X.dtype)
    wide[:, :X.shape[1]] = X
    wide[:, X.shape[1]:] = np.nan   # never read
    return dev(wide)[:, :X.shape[1]] if how == "device_pitched" else wide[:, :X.shape[1]]


PLACES = ("device", "host", "device_pitched", "host_pitched")


@functools.lru_cache(maxsize=None)
def grid_case(kernel, dtype, F, L, n):
    X, Lm = R.data(F * 100 + L, n, F, L, dtype=dtype)
    rs = np.random.RandomState(F + L)
    B, c = rs.randn(L, L), rs.randn(L)
    ref, (core, _) = R.kernel_map(X, Lm, B, None, **R.params(kernel))
    for a in (X, Lm, B, c, ref, core):
        a.setflags(write=False)
    return X, Lm, B, c, ref, core


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
@pytest.mark.parametrize("kernel", R.KERNELS)
def test_every_kernel_at_every_tile_seam(gpu, kernel, dtype):
    ka = KA()
    worst, calls = 0.0, 0
    for F in R.MAP_F:
        for L in R.MAP_L:
            Rw = ka.kernel_map_plan(L, L, F, np.dtype(dtype).itemsize)["R"]
            X, Lm, B, c, ref, core = grid_case(kernel, dtype, F, L, 3 * Rw + 1)
            for n in (1, Rw - 1, Rw, Rw + 1, 3 * Rw + 1):
                for P in sorted({1, 4, L}):
                    Pc = min(P, L)   # (B has L columns: P = 4 beside L = 1 is its one column)
                    how = PLACES[calls % len(PLACES)]
                    with_c = (calls // len(PLACES)) % 2 == 0   # (every placement with and without c)
                    calls += 1
                    out = ka.kernel_map(place(X[:n], how), Lm, B[:, :Pc], c[:Pc] if with_c else None, **R.params(kernel))
                    assert str(out.dtype).endswith(np.dtype(dtype).name) and tuple(out.shape) == (n, Pc)
                    assert hasattr(out, "is_cuda") == how.startswith("device")
                    r = ref[:n, :Pc] - (c[:Pc] if with_c else 0.0)
                    terms = (core[:n, :Pc], np.abs(c[:Pc]) if with_c else 0.0)
                    b = R.bound(r, terms, dtype)
                    err = np.abs(host(out).astype(np.float64) - r)
                    assert (err <= b).all(), (kernel, F, L, n, Pc, how, float((err / b).max()))
                    worst = max(worst, float((err / b).max()))
    print("%s %s: %d calls, worst error / bound %.3g" % (kernel, np.dtype(dtype).name, calls, worst))


def largest_fused_L(ka, itemsize):
    lo, hi = 1, 1 << 16   # fused at lo, not at hi
    assert ka.kernel_map_plan(lo, 1, 1, itemsize)["fused"] and not ka.kernel_map_plan(hi, 1, 1, itemsize)["fused"]
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ka.kernel_map_plan(mid, 1, 1, itemsize)["fused"]:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_route_seam_is_bit_identical(gpu, dtype, monkeypatch):
    """Default route against MSM_NYSTROEM_FUSED=0 at the largest fused L, at L + 1 (scratch either way: one chunk against
    several) and with the scratch cut into 64-row chunks: bit for bit, and inside the bound."""
    ka = KA()
    item = np.dtype(dtype).itemsize
    Lf = largest_fused_L(ka, item)
    n, F, P = 130, 3, 5
    for L, kernel in ((Lf, "rbf"), (Lf + 1, "rbf"), (Lf, "laplacian"), (33, "poly")):
        X, Lm = R.data(L, n, F, L, dtype=dtype)
        rs = np.random.RandomState(L)
        B, c = rs.randn(L, P), rs.randn(P)
        monkeypatch.delenv("MSM_NYSTROEM_FUSED", raising=False)
        plan = ka.kernel_map_plan(L, P, F, item)
        assert plan["fused"] == (L <= Lf) and plan["lds_bytes"] == (16 * plan["pitch"] * 8 * plan["R"] // 16 if plan["fused"] else 0)
        a = ka.kernel_map(dev(X), Lm, B, c, **R.params(kernel))
        monkeypatch.setenv("MSM_NYSTROEM_FUSED", "0")
        assert not ka.kernel_map_plan(L, P, F, item)["fused"]
        b1 = ka.kernel_map(dev(X), Lm, B, c, **R.params(kernel))
        b3 = ka.kernel_map(dev(X), Lm, B, c, scratch_rows=64, **R.params(kernel))   # 130 rows: three chunks
        bh = ka.kernel_map(X, Lm, B, c, scratch_rows=64, **R.params(kernel))
        monkeypatch.delenv("MSM_NYSTROEM_FUSED")
        assert np.array_equal(bits(a), bits(b1)) and np.array_equal(bits(a), bits(b3)) and np.array_equal(bits(a), bits(bh))
        ref, terms = R.kernel_map(X, Lm, B, c, **R.params(kernel))
        R.check(host(a), ref, terms, dtype, "%s L=%d %s" % (kernel, L, plan["route"]))


def test_uncentred_float32_rbf_stays_inside_the_bound(gpu):
    """|mean| / std = 100: the difference of near neighbours must survive |x|^2 + |l|^2 - 2 x.l."""
    ka = KA()
    X, Lm = R.data(5, 200, 16, 33, dtype=np.float32, shift=100.0)
    X[:33] = Lm + np.float32(0.01) * np.random.RandomState(1).randn(33, 16).astype(np.float32)   # near neighbours
    B = np.random.RandomState(0).randn(33, 4)
    ref, terms = R.kernel_map(X, Lm, B, None, **R.params("rbf"))
    K = np.asarray(R.kernel_values(X, Lm, **R.params("rbf")), dtype=np.float64)
    assert K[:33].max() > 0.99 and K[33:].max() > 1e-3
    out = ka.kernel_map(dev(X), Lm, B, None, **R.params("rbf"))
    R.check(host(out), ref, terms, np.float32, "rbf float32 |mean|/std = 100")
    # and the kernel values themselves (B = I, float64 output): relative to the argument before the cancellation
    refK, termsK = R.kernel_map(X, Lm, np.eye(33), None, **R.params("rbf"))
    R.check(host(ka.kernel_map(dev(X), Lm, np.eye(33), None, out_f64=True, **R.params("rbf"))), refK, termsK, np.float64, "rbf values")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f64"))
def test_exact_corners(gpu, dtype):
    ka = KA()
    X, Lm = R.data(3, 70, 5, 17, dtype=dtype, shift=3.0)
    X[::4] = Lm[:18][(np.arange(0, 70, 4) % 17)]
    eye = np.eye(17)
    K = host(ka.kernel_map(dev(X), Lm, eye, None, kernel="rbf", out_f64=True))
    rows = np.arange(0, 70, 4)
    assert (K[rows, rows % 17] == 1.0).all()          # a row equal to a landmark: exactly 1
    assert (K <= 1.0).all() and (K >= 0.0).all()
    Z = X.copy()
    Z[3] = 0
    Kc = host(ka.kernel_map(dev(Z), np.vstack([Lm[:16], np.zeros((1, 5), dtype)]), eye, None, kernel="cosine", out_f64=True))
    assert (Kc[3] == 0.0).all() and (Kc[:, 16] == 0.0).all() and np.isfinite(Kc).all()   # scikit-learn's normalize: zero stays zero
    # gamma=None is 1 / F
    a = ka.kernel_map(dev(X), Lm, eye, None, kernel="rbf", gamma=None)
    b = ka.kernel_map(dev(X), Lm, eye, None, kernel="rbf", gamma=1.0 / 5)
    assert np.array_equal(bits(a), bits(b))
    # a non-integer degree: positive bases inside the bound, negative bases NaN as in numpy
    ref, terms = R.kernel_map(X, Lm, eye, None, kernel="poly", degree=2.5, gamma=0.1, coef0=0.5)
    out = host(ka.kernel_map(dev(X), Lm, eye, None, kernel="poly", degree=2.5, gamma=0.1, coef0=0.5, out_f64=True))
    assert np.isfinite(ref).all()
    R.check(out, ref, terms, np.float64, "poly degree 2.5")
    neg = host(ka.kernel_map(dev(-X), Lm, eye, None, kernel="poly", degree=2.5, gamma=1.0, coef0=0.0, out_f64=True))
    assert np.isnan(neg).all()


@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
@pytest.mark.parametrize("where", ("device", "host"))
def test_non_finite_rows_raise(gpu, bad, where):
    ka = KA()
    for dtype in DTYPES:
        X, Lm = R.data(1, 150, 5, 17, dtype=dtype)
        X[149, 4] = bad
        for kernel in ("rbf", "laplacian", "linear"):
            with pytest.raises(ValueError, match="Input contains NaN, infinity or a value too large"):
                ka.kernel_map(place(X, where), Lm, np.eye(17), None, kernel=kernel)
        ok = ka.kernel_map(place(X[:149], where), Lm, np.eye(17), None, kernel="rbf")   # the call after the error is clean
        assert np.isfinite(host(ok)).all()
    Lb = Lm.copy()
    Lb[3, 0] = bad
    with pytest.raises(ValueError, match="Input contains NaN"):
        ka.kernel_map(place(X[:149], where), Lb, np.eye(17), None, kernel="rbf")


def test_callable_and_precomputed_kernels_are_refused(gpu):
    from msmbuilder_amd import KernelTICA, LandmarkNystroem, Nystroem
    X, Lm = R.data(1, 20, 3, 4)
    for kernel in ((lambda a, b: 1.0), "precomputed"):
        with pytest.raises(ValueError, match="no host path"):
            KA().kernel_map(X, Lm, np.eye(4), None, kernel=kernel)
        with pytest.raises(ValueError, match="no host path"):
            Nystroem(kernel=kernel, n_components=4).fit([X])
        with pytest.raises(ValueError, match="no host path"):
            LandmarkNystroem(landmarks=Lm, kernel=kernel).fit([X])
        with pytest.raises(ValueError, match="no host path"):
            KernelTICA(landmarks=Lm, kernel=kernel).fit([X])
    with pytest.raises(ValueError, match="at least one landmark"):        # no landmark: refused, not an unwritten result
        KA().kernel_map(X, Lm[:0], np.zeros((0, 3)), np.zeros(3))
    with pytest.raises(ValueError, match="Unknown kernel"):
        KA().kernel_map(X, Lm, np.eye(4), None, kernel="chi2")
    with pytest.raises(ValueError, match="landmarks should be an int, ndarray, or None."):
        LandmarkNystroem(landmarks=[[1.0, 2.0]])


def test_c_abi(gpu):
    L = gpu.lib()
    X, Lm = R.data(2, 40, 3, 5)
    B = np.ascontiguousarray(np.random.RandomState(0).randn(5, 2))
    out = np.full((40, 2), 7.0)

    def call(n, kid, c=None, fn=L.msm_kernel_map_f64, Xp=X.ctypes.data, op=out.ctypes.data):
        return fn(Xp, n, 3, 3, Lm.ctypes.data, 5, B.ctypes.data, 2, c, kid, 1.0 / 3, 1.0, 3.0, op, 0, 0, 0)

    assert call(40, 4) == 0                                   # null c
    ref, terms = R.kernel_map(X, Lm, B, None, **R.params("rbf"))
    R.check(out, ref, terms, np.float64, "C ABI, null c")
    out[:] = 7.0
    assert call(0, 4) == 0 and (out == 7.0).all()             # n = 0: nothing written
    assert call(0, 4, Xp=None, op=None) == 0
    for kid in (-1, 6, 99):
        assert call(40, kid) == gpu.MSM_ERR_INVALID             # a refused kernel id
        assert "no host path" in gpu.last_error()
    assert call(40, 4, Xp=None) == gpu.MSM_ERR_INVALID
    plan = (C.c_int64 * 9)()
    assert L.msm_kernel_map_plan(0, 1, 1, 8, plan) == gpu.MSM_ERR_INVALID
    assert L.msm_kernel_map_plan(5, 2, 3, 2, plan) == gpu.MSM_ERR_INVALID
    assert L.msm_kernel_map_plan(5, 2, 3, 8, plan) == 0 and plan[1] % 16 == 0 and plan[5] == 16


# ---- estimators against the goldens ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", sorted(R.EST_CASES))
def test_landmark_nystroem_against_golden(gpu, golden, kernel):
    from msmbuilder_amd import LandmarkNystroem
    for F, L in R.EST_CASES[kernel]:
        for dtype in DTYPES:
            X, Lm = R.data(R.est_seed(kernel, F, L), 50, F, L)
            p = "%s_%d_%d_" % (kernel, F, L)
            if dtype == np.float32:   # float32 rows against float32 landmarks: the golden's normalisation no longer applies
                X, Lm = X.astype(np.float32), Lm.astype(np.float32)
                Mg = R.normalization(np.asarray(R.kernel_values(Lm, Lm, **R.params(kernel)), dtype=np.float64))
            else:
                Mg = golden[p + "normalization"]
            m = LandmarkNystroem(landmarks=Lm, **R.params(kernel)).fit([X])
            assert m.component_indices_ is None and np.array_equal(m.components_, Lm)
            tol = R.normalization_tolerance(Lm, **R.params(kernel))
            dM = np.abs(m.normalization_ - Mg).max()
            print(p, np.dtype(dtype).name, "normalization tolerance %.3g, difference %.3g" % (tol, dM))
            assert dM <= tol
            ref, terms = R.kernel_map(X, Lm, Mg.T, None, **R.params(kernel))
            Kabs = np.abs(np.asarray(R.kernel_values(X, Lm, **R.params(kernel)), dtype=np.float64)).sum(1, keepdims=True)
            for seqs in ([dev(X)], [X]):
                out = m.transform(seqs)[0]
                assert str(out.dtype).endswith(np.dtype(dtype).name)
                R.check(host(out), ref, terms, dtype, p + "transform", extra=Kabs * tol)
            if dtype == np.float64:
                R.check(host(m.fit_transform([dev(X)])[0]), golden[p + "features"], terms, dtype, p + "golden features",
                        extra=Kabs * tol + R.bound(ref, terms, dtype))


def test_nystroem_random_basis_and_sequence_conventions(gpu, golden):
    from msmbuilder_amd import Nystroem
    seqs = R.nystroem_sequences()
    allrows = np.concatenate(seqs)
    ref, terms = R.kernel_map(allrows, golden["nys_components"], golden["nys_normalization"].T, None, **R.params("rbf"))
    tol = R.normalization_tolerance(golden["nys_components"], **R.params("rbf"))
    Kabs = np.abs(np.asarray(R.kernel_values(allrows, golden["nys_components"], **R.params("rbf")), dtype=np.float64)).sum(1, keepdims=True)
    lens = [len(s) for s in seqs]
    joined = dev(allrows)
    forms = {
        "host list": list(seqs),
        "device, back to back": list(joined.split(lens)),
        "device, separate": [dev(s) for s in seqs],
        "host views of one array": list(np.split(allrows, np.cumsum(lens)[:-1])),
    }
    first = None
    for name, form in forms.items():
        m = Nystroem(n_components=20, random_state=3, **R.params("rbf")).fit(form)
        assert np.array_equal(m.component_indices_, golden["nys_indices"]), name
        assert np.array_equal(m.components_, golden["nys_components"]), name
        assert np.abs(m.normalization_ - golden["nys_normalization"]).max() <= tol
        out = m.transform(form)
        assert [tuple(o.shape) for o in out] == [(n, 20) for n in lens], name
        assert all(hasattr(o, "is_cuda") == name.startswith("device") for o in out), name
        got = np.concatenate([host(o) for o in out])
        R.check(got, ref, terms, np.float64, "Nystroem, " + name, extra=Kabs * tol)
        first = got if first is None else first
        assert np.array_equal(bits(got), bits(first)), name       # every form runs the same arithmetic
        # an empty trajectory in the middle and a one-row trajectory at the end
        empty = form[0][:0]
        out2 = m.transform([form[0], empty, form[2], form[1]])
        assert [tuple(o.shape) for o in out2] == [(lens[0], 20), (0, 20), (lens[2], 20), (1, 20)], name
        assert np.array_equal(bits(np.concatenate([host(out2[0]), host(out2[3]), host(out2[2])])), bits(first)), name
        assert np.array_equal(bits(m.partial_transform(form[1])), bits(out[1]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert Nystroem(n_components=500, random_state=0).fit(seqs).components_.shape == (66, 5)


@functools.lru_cache(maxsize=None)
def ktica_fit(dtype, where, kinetic=False):
    from msmbuilder_amd import KernelTICA
    seqs, lm = R.ktica_sequences()
    seqs = [s.astype(dtype) for s in seqs]
    m = KernelTICA(landmarks=lm.astype(dtype), kinetic_mapping=kinetic, **R.KTICA_KW)
    m.fit([dev(s) for s in seqs] if where == "device" else seqs)
    return m, seqs


@pytest.mark.parametrize("where", ("device", "host"))
@pytest.mark.parametrize("dtype,rtol", ((np.float32, 1e-5), (np.float64, 1e-10)), ids=("f32", "f64"))
def test_kernel_tica_eigenvalues(gpu, golden, dtype, rtol, where):
    m, seqs = ktica_fit(dtype, where)
    print(np.dtype(dtype).name, where, "relative eigenvalue differences", np.abs(m.eigenvalues_ - golden["kt_eigenvalues"]) / golden["kt_eigenvalues"])
    np.testing.assert_allclose(m.eigenvalues_, golden["kt_eigenvalues"], rtol=rtol, atol=0)
    assert m.n_features == 24 and m.n_sequences_ == 3 and m.n_observations_ == 800
    assert m.components_.shape == (4, 24)


def folded_reference(m, X):
    """Exact reference and bound terms of the folded transform for THIS model's B and c, plus the derived allowance for the
    unfused composition: its features carry the map's bound with B = M^T, its projection (L + 2) u per product, and the
    folded B = fl(M^T V^T) differs from the exact product by L u |M^T| |V^T|."""
    ny = m._nystroem
    mean, comps = m._projection()
    B, c = m._folded()
    ref, terms = R.kernel_map(X, ny.components_, B, c, **ny._kernel_kw())
    feat, fterms = R.kernel_map(X, ny.components_, ny.normalization_.T, None, **ny._kernel_kw())
    L = comps.shape[1]
    K = np.abs(np.asarray(R.kernel_values(X, ny.components_, **ny._kernel_kw()), dtype=np.float64))
    extra = (R.bound(feat, fterms, np.float64) @ np.abs(comps.T)
             + 4 * R.U64 * (L + 2) * ((np.abs(feat) + np.abs(mean)) @ np.abs(comps.T))
             + 4 * R.U64 * L * (K @ (np.abs(ny.normalization_.T) @ np.abs(comps.T))))
    return ref, terms, extra


@pytest.mark.parametrize("kinetic", (False, True), ids=("plain", "kinetic"))
def test_kernel_tica_transform(gpu, golden, kinetic):
    from msmbuilder_amd import tICA
    m, seqs = ktica_fit(np.float64, "device", kinetic)
    X = np.concatenate(seqs)
    lens = [len(s) for s in seqs]
    ref, terms, extra = folded_reference(m, X)
    folded = m.transform([dev(s) for s in seqs])
    assert [tuple(y.shape) for y in folded] == [(n, 4) for n in lens] and all(y.is_cuda for y in folded)
    Y = np.concatenate([host(y) for y in folded])
    R.check(Y, ref, terms, np.float64, "folded transform")
    assert np.array_equal(bits(Y), bits(np.concatenate(m.transform(seqs))))          # host list: the same arithmetic
    assert np.array_equal(bits(Y[:lens[0]]), bits(m.partial_transform(seqs[0])))
    unfused = host(tICA.transform(m, m._nystroem.transform([dev(X)]))[0])    # (ONE tensor: tICA's own per-trajectory path)
    R.check(unfused, ref, terms, np.float64, "unfused composition", extra=extra)
    # against the golden: the eigenvectors are defined up to sign, and move by (eigenvalue-level perturbation) / gap --
    # the standing eigenvalue tolerance 1e-10 over the smallest gap between the kept eigenvalues, relative to the column
    gold = golden["kt_transform_kinetic" if kinetic else "kt_transform"]
    sign = np.sign((Y * gold).sum(0))
    gap = np.abs(np.diff(golden["kt_eigenvalues"])).min()
    tol = 1e-10 / gap * np.abs(gold).max(0) * 4       # (4 kept eigenvectors may each turn towards the other three and the rest)
    print("golden: max difference per column", np.abs(Y * sign - gold).max(0), "tolerance", tol)
    assert (np.abs(Y * sign - gold) <= tol).all()
    # float32 rows: float64 output, inside the bound of ITS model
    m32, seqs32 = ktica_fit(np.float32, "device", kinetic)
    X32 = np.concatenate(seqs32)
    ref32, terms32, _ = folded_reference(m32, X32)
    Y32 = m32.transform([dev(X32)])[0]
    assert str(Y32.dtype) == "torch.float64"
    R.check(host(Y32), ref32, terms32, np.float64, "folded transform, float32 rows")


def test_kernel_tica_partial_fit_score_and_pickle(gpu, golden):
    from msmbuilder_amd import KernelTICA
    m, seqs = ktica_fit(np.float64, "host")
    _, lm = R.ktica_sequences()
    p = KernelTICA(landmarks=lm, **R.KTICA_KW)
    for s in seqs:
        p.partial_fit(dev(s))
    np.testing.assert_allclose(p.eigenvalues_, m.eigenvalues_, rtol=1e-10, atol=0)
    assert p.n_observations_ == m.n_observations_ and p.n_sequences_ == 3
    # pieces cut with a lag-wide overlap (a trajectory whose features exceed the device budget)
    from msmbuilder_amd.decomposition import ktica
    q = KernelTICA(landmarks=lm, **R.KTICA_KW)
    old = ktica._FEATURE_BYTES
    ktica._FEATURE_BYTES = (24 + 3) * 8 * 100   # 100 rows (3 values, 24 features each) at a time
    try:
        q.fit(seqs)
    finally:
        ktica._FEATURE_BYTES = old
    np.testing.assert_allclose(q.eigenvalues_, m.eigenvalues_, rtol=1e-10, atol=0)
    assert q.n_observations_ == m.n_observations_ and q.n_sequences_ == 3
    # score: a trace of k Rayleigh quotients, as sensitive as the eigenvalues (1e-10) times the conditioning of the projected covariance
    test = R.double_well(999, 300)
    V = m.eigenvectors_
    s = m.score([test])
    m2 = KernelTICA(landmarks=lm, **R.KTICA_KW).fit([test])
    cond = np.linalg.cond(V.T @ m2.covariance_ @ V)
    print("score", s, "golden", float(golden["kt_score"]), "cond", cond)
    assert abs(s - golden["kt_score"]) <= 1e-10 * cond * 4 * abs(golden["kt_score"])
    r = pickle.loads(pickle.dumps(m))
    np.testing.assert_array_equal(r.eigenvalues_, m.eigenvalues_)
    assert np.array_equal(bits(np.concatenate(r.transform(seqs))), bits(np.concatenate(m.transform(seqs))))
    r.partial_fit(seqs[0])          # the unpickled model goes on accumulating
    assert r.n_sequences_ == 4
    with pytest.raises(ValueError, match="shorter than the lag time"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            KernelTICA(landmarks=lm, **R.KTICA_KW).fit([seqs[0][:2]])
    # landmarks from the data: every stride-th lagged pair (host and device trajectories pick the same frames)
    a = KernelTICA(stride=40, **R.KTICA_KW).fit(seqs)
    b = KernelTICA(stride=40, **R.KTICA_KW).fit([dev(s) for s in seqs])
    assert np.array_equal(a.landmarks, b.landmarks) and a.landmarks.shape[1] == 3 and len(a.landmarks) < 60
    np.testing.assert_allclose(a.eigenvalues_, b.eigenvalues_, rtol=1e-10)
