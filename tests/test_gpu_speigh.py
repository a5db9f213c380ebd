"""The sparse generalized eigenpair solver on the device (csrc/speigh_dev.h) against the reference's goldens
(tests/golden/speigh_golden.npz, made by make_golden_speigh.py) and the numpy restatement (tests/speigh_ref.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.linalg

import speigh_ref as R

pytestmark = pytest.mark.gpu

EPSM = np.finfo(np.float64).eps
SIZES = (1, 2, 3, 12, 33, 63, 64, 65, 127, 128, 129, 200, 255, 256, 257, 513)
RHOS = (1e-4, 1e-3, 1e-2, 1e-1)
STORED = (12, 33, 65, 129, 200)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speigh_golden.npz"))


@functools.lru_cache(maxsize=None)
def matrices(F):
    A, B = R.matrices(F, F)
    A.setflags(write=False)
    B.setflags(write=False)
    return A, B


def solver_settings():
    eps, tol, maxiter = golden()["eps_tol_maxiter"]
    return float(eps), float(tol), int(maxiter)


def run(F, rho, **kw):
    from msmbuilder_amd.decomposition.speigh import speigh
    A, B = matrices(F)
    eps, tol, maxiter = solver_settings()
    kw.setdefault("maxiter", maxiter)
    return speigh(A, B, rho, eps=eps, tol=tol, return_info=True, **kw)


# ---- project ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", STORED)
def test_project_against_goldens_and_longdouble(gpu, F):
    from msmbuilder_amd.decomposition.speigh import project
    G = golden()
    w, V, a = G["eig_F%d_w" % F], G["eig_F%d_V" % F], G["eig_F%d_proj_a" % F]
    got = project(a, w, V)
    want = np.asarray(R.project(a, w, V, np.longdouble), np.float64)
    bound = max(4 * float(G["eig_F%d_dist_project" % F]), F * EPSM * np.abs(want).max())
    err = np.abs(got - want).max()
    print("project F=%d: error %.3e, bound %.3e, ratio %.3f" % (F, err, bound, err / bound))
    assert err <= bound
    # the stored reference output lies as close (its own distance plus ours)
    assert np.abs(got - G["eig_F%d_proj_ref" % F]).max() <= bound + float(G["eig_F%d_dist_project" % F])
    # on the boundary: x^T B x = 1
    Bm = (V * w).dot(V.T)
    assert abs(got.dot(Bm).dot(got) - 1.0) < 1e-9
    # inside the ellipsoid the input comes back bit for bit
    small = a * (0.5 / np.sqrt(a.dot(Bm).dot(a)))
    assert np.array_equal(project(small, w, V), small)
    out = np.empty(F)
    assert project(small, w, V, out) is out and np.array_equal(out, small)


@pytest.mark.parametrize("F", (5, 129))
def test_project_identity_and_tiny_eigenvalue(gpu, F):
    from msmbuilder_amd.decomposition.speigh import project
    rs = np.random.RandomState(F)
    a = rs.randn(F) * 3
    got = project(a, np.ones(F), np.eye(F))
    np.testing.assert_allclose(got, a / np.linalg.norm(a), rtol=0, atol=F * EPSM)
    # one direction almost unconstrained
    w = rs.uniform(0.5, 2.0, F)
    w[0] = 1e-12
    V = scipy.linalg.qr(rs.randn(F, F))[0]
    got = project(a, w, V)
    want = np.asarray(R.project(a, w, V, np.longdouble), np.float64)
    host = R.project(a, w, V)
    bound = max(4 * np.abs(host - want).max(), F * EPSM * np.abs(want).max())
    assert np.abs(got - want).max() <= bound


def test_project_on_device_arrays(gpu):
    import torch
    from msmbuilder_amd.decomposition.speigh import project
    G = golden()
    w, V, a = G["eig_F33_w"], G["eig_F33_V"], G["eig_F33_proj_a"]
    dev = project(torch.as_tensor(a).cuda(), torch.as_tensor(w).cuda(), torch.as_tensor(V).cuda())
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), project(a, w, V))


# ---- solve_admm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", STORED)
@pytest.mark.parametrize("case", (0, 1, 2))
def test_admm_against_goldens_and_longdouble(gpu, F, case):
    from msmbuilder_amd.decomposition.speigh import solve_admm
    G = golden()
    eps, tol, maxiter = solver_settings()
    key = "eig_F%d_admm%d_" % (F, case)
    w, V = G["eig_F%d_w" % F], G["eig_F%d_V" % F]
    b, ww, x0, x_ref = G[key + "b"], G[key + "w"], G[key + "x0"], G[key + "x_ref"]
    x = x0.copy()
    fun, info = solve_admm(b, ww, w, V, x, tol=tol, maxiter=maxiter, return_info=True)
    assert info["status"] == "converged"
    assert np.array_equal(x != 0, x_ref != 0)
    fine = np.asarray(R.solve_admm(b, ww, w, V, x0, tol / 1000, maxiter, np.longdouble)[0], np.float64)
    err, bound = np.abs(x - fine).max(), 4 * float(G[key + "dist_admm"])
    print("admm F=%d case %d: %d iterations (restatement %d), error %.3e, bound %.3e" % (
        F, case, info["iterations"], int(G[key + "iterations"]), err, bound))
    assert err <= bound
    want_fun = 0.5 * x.dot(x) - x.dot(b) + 0.5 * b.dot(b) + np.abs(ww * x).sum()
    assert abs(fun - want_fun) <= 1e-12 * max(1.0, abs(want_fun))


def test_admm_cases_adapt_the_penalty_both_ways():
    G = golden()
    doubled = sum(int(G["eig_F%d_admm%d_doubled" % (F, c)]) for F in STORED for c in (0, 1, 2))
    halved = sum(int(G["eig_F%d_admm%d_halved" % (F, c)]) for F in STORED for c in (0, 1, 2))
    assert doubled > 0 and halved > 0


def test_admm_penalty_doubling_case_follows_the_restatement(gpu):
    """F = 12, b scaled by 10: the restated run doubles and halves the penalty; the device run takes the same number of
    iterations and ends at the same penalty."""
    from msmbuilder_amd.decomposition.speigh import solve_admm
    G = golden()
    eps, tol, maxiter = solver_settings()
    key = "eig_F12_admm2_"
    assert int(G[key + "doubled"]) > 0 and int(G[key + "halved"]) > 0
    w, V = G["eig_F12_w"], G["eig_F12_V"]
    x = G[key + "x0"].copy()
    _, info = solve_admm(G[key + "b"], G[key + "w"], w, V, x, tol=tol, maxiter=maxiter, return_info=True)
    _, host = R.solve_admm(G[key + "b"], G[key + "w"], w, V, G[key + "x0"], tol, maxiter)
    assert info["iterations"] == host["iterations"] and info["rho"] == host["rho"]


# ---- speigh ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", SIZES)
@pytest.mark.parametrize("ri", range(4))
def test_speigh_against_the_reference(gpu, F, ri):
    G = golden()
    assert [F, ri] in G["qualified"].tolist()
    key = "pair_F%d_r%d_" % (F, ri)
    A, B = matrices(F)
    u, v, info = run(F, RHOS[ri])
    mask = np.abs(v) > 0
    print("F=%d rho=%g: %d outer, %d admm, %d launches, %d workgroups" % (F, RHOS[ri], info["outer"], info["admm"], info["launches"],
                                                                         info["workgroups"]))
    assert info["status"] == "converged"
    assert np.array_equal(mask, G[key + "mask"])
    assert np.array_equal(np.asarray(info["x"]) != 0, mask) and info["nnz"] == mask.sum()
    assert info["outer"] == int(G[key + "outer"])
    np.testing.assert_allclose(u, float(G[key + "u"]), rtol=1e-10)
    v_ref = G[key + "v"]
    if mask.sum() > 1:
        sub = np.ix_(mask, mask)
        ev = scipy.linalg.eigh(A[sub], B[sub], eigvals_only=True)
        gap = min(ev[-1] - ev[-2], 1.0)
    else:
        gap = 1.0
    np.testing.assert_allclose(v, v_ref, rtol=0, atol=1e-8 * np.abs(v_ref).max() / gap)
    assert abs(v.dot(B).dot(v) - 1.0) < 1e-9
    assert not np.signbit(v[v == 0]).any() and v.sum() >= 0
    assert (info["workgroups"] == 0) == (F <= 128)


def test_speigh_start_sign_does_not_matter(gpu):
    A, B = matrices(33)
    x0 = R.top_pair(A, B)[1]
    u1, v1, i1 = run(33, 1e-3, x0=x0)
    u2, v2, i2 = run(33, 1e-3, x0=-x0)
    assert np.array_equal(np.abs(i1["x"]), np.abs(i2["x"])) and np.array_equal(i1["x"], -i2["x"])
    assert u1 == u2 and np.array_equal(v1, v2) and i1["outer"] == i2["outer"] and i1["admm"] == i2["admm"]
    assert np.array_equal(np.abs(v1) > 0, golden()["pair_F33_r1_mask"])


def test_speigh_supplied_decomposition_of_B(gpu):
    A, B = matrices(65)
    u, v, info = run(65, 1e-2, eigh_B=scipy.linalg.eigh(B))
    assert np.array_equal(np.abs(v) > 0, golden()["pair_F65_r2_mask"]) and info["outer"] == int(golden()["pair_F65_r2_outer"])


# ---- determinism -----------------------------------------------------------------------------------------------------
def bits(result):
    u, v, info = result
    return (np.float64(u).tobytes(), np.asarray(v).tobytes(), np.asarray(info["x"]).tobytes(), info["outer"], info["admm"],
            info["objective"])


@pytest.mark.parametrize("F", (65, 200))
def test_speigh_is_bit_identical_across_runs_grids_and_budgets(gpu, monkeypatch, F):
    monkeypatch.delenv("MSM_SPEIGH_GRID", raising=False)
    monkeypatch.delenv("MSM_SPEIGH_BUDGET", raising=False)
    base = run(F, 1e-2)
    want = bits(base)
    assert bits(run(F, 1e-2)) == want
    assert base[2]["launches"] == 1
    grids = {}
    for grid in ("1", "7", "64"):
        monkeypatch.setenv("MSM_SPEIGH_GRID", grid)
        res = run(F, 1e-2)
        grids[grid] = res[2]["workgroups"]
        assert bits(res) == want, "MSM_SPEIGH_GRID=%s" % grid
    assert grids["7"] == 7 and grids["64"] == (33 if F == 65 else 50)   # 65 rows in twos, 200 rows in fours: no workgroup without a row
    assert grids["1"] == (0 if F <= 128 else 1)
    monkeypatch.delenv("MSM_SPEIGH_GRID")
    total = base[2]["admm"]
    for budget in (1, 7, 1000):
        monkeypatch.setenv("MSM_SPEIGH_BUDGET", str(budget))
        res = run(F, 1e-2)
        assert bits(res) == want, "MSM_SPEIGH_BUDGET=%d" % budget
        # a launch ends when its budget is spent at the head of an iteration: the last one may only have had the stop test left
        assert res[2]["launches"] in (-(-total // budget), total // budget + 1)
        monkeypatch.setenv("MSM_SPEIGH_GRID", "7")
        assert bits(run(F, 1e-2)) == want
        monkeypatch.delenv("MSM_SPEIGH_GRID")


# ---- corners ---------------------------------------------------------------------------------------------------------
def test_speigh_empty_mask_and_single_entry(gpu):
    from msmbuilder_amd.decomposition.speigh import speigh
    A, B = matrices(12)
    u, v, info = speigh(A, B, 1e4, eps=1e-6, tol=1e-6, maxiter=10000, return_info=True)
    hu, hv, hi = R.speigh(A, B, 1e4, 1e-6, 1e-6, 10000)
    assert hi["mask"].sum() == 0 and info["nnz"] == 0 and u == 0.0 and not v.any()
    # rank one plus a small diagonal: the fourth entry is thresholded away, then the third, ... a mask of exactly one
    d = np.array([3.0, 0.2, 0.1, 0.05])
    A1, B1 = np.diag(d), np.eye(4)
    hu, hv, hi = R.speigh(A1, B1, 1.0, 1e-6, 1e-6, 10000)
    u, v, info = speigh(A1, B1, 1.0, eps=1e-6, tol=1e-6, maxiter=10000, return_info=True)
    assert hi["mask"].sum() == 1 and np.array_equal(np.abs(v) > 0, hi["mask"])
    assert u == 3.0 and np.array_equal(v, [1.0, 0.0, 0.0, 0.0])


@pytest.mark.parametrize("maxiter", (1, 3))
def test_speigh_maxiter_is_exact(gpu, maxiter):
    u, v, info = run(33, 1e-2, maxiter=maxiter)
    A, B = matrices(33)
    eps, tol, _ = solver_settings()
    hu, hv, hi = R.speigh(A, B, 1e-2, eps, tol, maxiter)
    assert hi["status"] == "maxiter" and info["status"] == "maxiter"
    assert info["outer"] == hi["outer"] == maxiter and info["admm"] == hi["admm"] == maxiter * maxiter
    assert np.array_equal(np.asarray(info["x"]) != 0, hi["mask"])


def test_speigh_indefinite_deflated_and_diagonal(gpu):
    from msmbuilder_amd.decomposition.speigh import speigh, scdeflate
    A, B = matrices(33)
    eps, tol, maxiter = solver_settings()
    # lambda_min < 0: tau grows by it
    Aneg = A - 0.5 * B
    lmin = scipy.linalg.eigvalsh(Aneg).min()
    assert lmin < 0
    u, v, info = speigh(Aneg, B, 1e-2, eps=eps, tol=tol, maxiter=maxiter, return_info=True)
    hu, hv, hi = R.speigh(Aneg, B, 1e-2, eps, tol, maxiter)
    assert abs(info["tau"] - (0.1 - lmin)) < 1e-12
    assert np.array_equal(np.abs(v) > 0, hi["mask"]) and info["outer"] == hi["outer"]
    np.testing.assert_allclose(u, hu, rtol=1e-10)
    # A deflated twice (no longer symmetric to rounding), device and host pointers
    import torch
    Ad, Ah = torch.as_tensor(A).cuda(), A
    Bd = torch.as_tensor(B).cuda()
    for _ in range(2):
        uh, vh, ih = speigh(Ah, B, 1e-2, eps=eps, tol=tol, maxiter=maxiter, return_info=True)
        ud, vd, idv = speigh(Ad, Bd, 1e-2, eps=eps, tol=tol, maxiter=maxiter, return_info=True)
        assert vd.is_cuda and ud == uh and np.array_equal(vd.cpu().numpy(), vh)
        hu, hv, hi = R.speigh(Ah, B, 1e-2, eps, tol, maxiter)
        assert np.array_equal(np.abs(vh) > 0, hi["mask"])
        want = R.scdeflate(Ah, vh, np.longdouble)
        Ah_new = scdeflate(Ah, vh)
        Ad = scdeflate(Ad, vd)
        assert np.array_equal(Ad.cpu().numpy(), Ah_new)
        assert np.abs(Ah_new - np.asarray(want, np.float64)).max() <= 8 * EPSM * np.linalg.norm(Ah, 2)
        Ah = Ah_new
    # B diagonal
    Bdiag = np.diag(np.diag(B))
    u, v, info = speigh(A, Bdiag, 1e-2, eps=eps, tol=tol, maxiter=maxiter, return_info=True)
    hu, hv, hi = R.speigh(A, Bdiag, 1e-2, eps, tol, maxiter)
    assert np.array_equal(np.abs(v) > 0, hi["mask"]) and info["outer"] == hi["outer"]
    np.testing.assert_allclose(u, hu, rtol=1e-10)


@pytest.mark.parametrize("n", (1, 7, 130, 300))
def test_scdeflate_against_the_formula(gpu, n):
    from msmbuilder_amd.decomposition.speigh import scdeflate
    rs = np.random.RandomState(n)
    A = rs.randn(n, n)            # not symmetric: the two products differ
    x = rs.randn(n)
    got = scdeflate(A, x)
    want = np.asarray(R.scdeflate(A, x, np.longdouble), np.float64)
    scale = np.abs(np.outer(A.dot(x), x.dot(A)) / x.dot(A).dot(x)).max() + np.linalg.norm(A, 2)
    assert np.abs(got - want).max() <= 8 * EPSM * scale * max(1, np.sqrt(n))


def test_refusals_with_a_device(gpu):
    from msmbuilder_amd.decomposition.speigh import speigh, project, solve_admm
    A, B = matrices(12)
    bad = A.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError, match="infs or NaNs"):
        speigh(bad, B, 1e-2)
    bad = B.copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="infs or NaNs"):
        speigh(A, bad, 1e-2)
    with pytest.raises(np.linalg.LinAlgError, match="positive definite"):
        speigh(A, -B, 1e-2)
    with pytest.raises(ValueError, match="method=2"):
        speigh(A, B, 1e-2, method=2)
    for kw in ({"eps": 0.0}, {"tol": 0.0}, {"maxiter": 0}, {"eps": -1.0}):
        with pytest.raises(ValueError):
            speigh(A, B, 1e-2, **kw)
    with pytest.raises(ValueError):
        speigh(A, B, -1.0)
    with pytest.raises(ValueError):
        speigh(A, B[:5, :5], 1e-2)
    with pytest.raises(ValueError):
        speigh(A[:, :5], B, 1e-2)
    with pytest.raises(ValueError):
        project(np.zeros(3), np.ones(4), np.eye(4))
    with pytest.raises(ValueError):
        solve_admm(np.zeros(4), np.ones(4), np.ones(4), np.eye(4), np.zeros(3))
    L = gpu.lib()
    wide = np.zeros(2049)
    assert L.msm_speigh_project(wide.ctypes.data, wide.ctypes.data, wide.ctypes.data, 2049, wide.ctypes.data, 0) == gpu.MSM_ERR_INVALID
