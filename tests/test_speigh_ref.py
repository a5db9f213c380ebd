"""CPU tier of the sparse eigenpair solver: the numpy restatement (tests/speigh_ref.py) against the reference's goldens and
its own unit cases restated, the projection's optimality conditions, the C ABI's argument refusals (which need no
device), the new exports and switches."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.linalg

import speigh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RHOS = (1e-4, 1e-3, 1e-2, 1e-1)


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "speigh_golden.npz"))


def test_every_case_of_the_family_qualified():
    G = golden()
    assert len(G["qualified"]) == len(G["sizes"]) * len(G["rhos"]) == 64
    assert np.array_equal(G["rhos"], RHOS)


@pytest.mark.parametrize("F", (1, 2, 3, 12, 33, 65, 129))
def test_restatement_against_the_reference(F):
    G = golden()
    eps, tol, maxiter = G["eps_tol_maxiter"]
    A, B = R.matrices(F, F)
    for ri, rho in enumerate(RHOS):
        key = "pair_F%d_r%d_" % (F, ri)
        u, v, info = R.speigh(A, B, rho, eps, tol, int(maxiter))
        assert np.array_equal(info["mask"], G[key + "mask"])
        assert info["outer"] == int(G[key + "outer"]) and info["admm"] == int(G[key + "admm"])
        np.testing.assert_allclose(u, float(G[key + "u"]), rtol=1e-10)
        np.testing.assert_allclose(v, G[key + "v"], rtol=0, atol=1e-9 * np.abs(v).max())


@pytest.mark.parametrize("F", (12, 33, 65))
def test_restated_project_and_admm_against_the_reference(F):
    G = golden()
    eps, tol, maxiter = G["eps_tol_maxiter"]
    w, V = G["eig_F%d_w" % F], G["eig_F%d_V" % F]
    got = R.project(G["eig_F%d_proj_a" % F], w, V)
    assert np.abs(got - G["eig_F%d_proj_ref" % F]).max() <= max(4 * float(G["eig_F%d_dist_project" % F]), F * 2.3e-16 * np.abs(got).max())
    for case in range(3):
        key = "eig_F%d_admm%d_" % (F, case)
        x, info = R.solve_admm(G[key + "b"], G[key + "w"], w, V, G[key + "x0"], tol, int(maxiter))
        assert np.array_equal(x != 0, G[key + "x_ref"] != 0)
        assert info["iterations"] == int(G[key + "iterations"])
        assert (info["doubled"], info["halved"]) == (int(G[key + "doubled"]), int(G[key + "halved"]))
        np.testing.assert_allclose(x, G[key + "x_ref"], rtol=0, atol=1e-9)


# ---- the reference's own unit cases ------------------------------------------------------------------------------------
def rand_pos_semidef(n, seed=0):
    M = np.random.RandomState(seed).rand(n, n)
    return M.dot(M.T)


def rand_sym(n, seed=0):
    M = np.random.RandomState(seed).randn(n, n)
    return M + M.T


def sorted_eigh(A, B=None):
    w, V = scipy.linalg.eigh(A, b=B)
    order = np.argsort(-w)
    return w[order], V[:, order]


@pytest.mark.parametrize("A,B", [
    (rand_sym(4), np.eye(4)),
    (rand_sym(4), rand_pos_semidef(4)),
    (rand_pos_semidef(4), np.diag(np.random.RandomState(3).randn(4) ** 2)),
    (rand_pos_semidef(4), rand_pos_semidef(4) + np.eye(4)),
], ids=["identity", "general", "diagonal", "shifted"])
def test_rho_zero_is_the_plain_top_pair(A, B):
    u, v, _ = R.speigh(A, B, 0.0)
    w, V = sorted_eigh(A, B)
    np.testing.assert_allclose(u, w[0], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(v ** 2, V[:, 0] ** 2, atol=1e-6)


def test_rank_one_case_loses_its_last_entry():
    x = np.array([1.0, 2.0, 3.0, 1e-4])
    x /= np.linalg.norm(x)
    u, v, info = R.speigh(np.outer(x, x), np.eye(4), 0.01)
    want = np.array([1.0, 2.0, 3.0, 0.0])
    np.testing.assert_allclose(v, want / np.linalg.norm(want), atol=1e-6)
    assert v[3] == 0.0 and not np.signbit(v[3])


@pytest.mark.parametrize("with_B", (False, True))
def test_scdeflate_leaves_one_zero_eigenvalue(with_B):
    A = rand_sym(4)
    B = rand_pos_semidef(4) if with_B else None
    w1, V1 = sorted_eigh(A, B)
    w2, V2 = sorted_eigh(R.scdeflate(A, V1[:, 0]), B)
    zero = np.abs(w2) < 1e-10
    assert zero.sum() == 1
    np.testing.assert_allclose(w1[1:], w2[~zero], atol=1e-6)


# ---- the projection's optimality conditions ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (np.float64, np.longdouble))
def test_project_meets_the_kkt_conditions(dtype):
    rs = np.random.RandomState(5)
    B = rand_pos_semidef(7, 2) + 0.1 * np.eye(7)
    w, V = scipy.linalg.eigh(B)
    a = rs.randn(7) * 3
    x = np.asarray(R.project(a, w, V, dtype), np.float64)
    assert abs(x.dot(B).dot(x) - 1) < 1e-10                           # on the boundary
    g = a - x                                                         # a - x = mu B x with mu > 0
    mu = g.dot(B.dot(x)) / np.linalg.norm(B.dot(x)) ** 2
    assert mu > 0 and np.abs(g - mu * B.dot(x)).max() < 1e-9
    inside = a * 0.5 / np.sqrt(a.dot(B).dot(a))
    assert np.array_equal(R.project(inside, w, V, dtype), inside.astype(dtype))


# ---- the C ABI refuses bad arguments before any device work ------------------------------------------------------------
def test_abi_refuses_bad_arguments_without_a_device():
    from msmbuilder_amd import _lib
    L = _lib.lib()
    n = 4
    A, B = np.eye(n), np.eye(n)
    x, v = np.ones(n), np.zeros(n)
    u = C.c_double(0)
    info = np.zeros(8)
    ip = info.ctypes.data_as(C.POINTER(C.c_double))
    p = lambda a: a.ctypes.data   # noqa: E731

    def pair(A_=p(A), B_=p(B), n_=n, rho=0.01, eps=1e-6, tol=1e-6, maxiter=10, u_=C.byref(u), v_=p(v), info_=ip, ev=None, E=None):
        return L.msm_speigh(A_, B_, n_, rho, eps, tol, maxiter, None, ev, E, u_, v_, None, info_, 0)

    bad = [pair(A_=None), pair(B_=None), pair(v_=None), pair(u_=None), pair(info_=None), pair(n_=0), pair(n_=2049),
           pair(eps=0.0), pair(eps=-1.0), pair(tol=0.0), pair(maxiter=0), pair(rho=-1e-3), pair(rho=float("nan")),
           pair(ev=p(x)), pair(E=p(A))]
    assert bad == [_lib.MSM_ERR_INVALID] * len(bad)
    assert "msm_speigh" in _lib.last_error()
    assert L.msm_speigh_project(None, p(x), p(A), n, p(v), 0) == _lib.MSM_ERR_INVALID
    assert L.msm_speigh_project(p(x), p(x), p(A), 0, p(v), 0) == _lib.MSM_ERR_INVALID
    assert L.msm_speigh_admm(p(x), p(x), p(x), p(A), None, n, 1e-6, 10, ip, 0) == _lib.MSM_ERR_INVALID
    assert L.msm_speigh_admm(p(x), p(x), p(x), p(A), p(v), n, 0.0, 10, ip, 0) == _lib.MSM_ERR_INVALID
    assert L.msm_speigh_admm(p(x), p(x), p(x), p(A), p(v), n, 1e-6, 0, ip, 0) == _lib.MSM_ERR_INVALID
    assert L.msm_scdeflate(None, p(x), n, p(A), 0) == _lib.MSM_ERR_INVALID
    assert L.msm_scdeflate(p(A), p(x), 0, p(B), 0) == _lib.MSM_ERR_INVALID


def test_python_refuses_before_touching_the_device():
    from msmbuilder_amd.decomposition.speigh import speigh
    A = np.eye(3)
    with pytest.raises(ValueError, match="method=2"):
        speigh(A, A, 0.01, method=2)
    for kw in ({"eps": 0.0}, {"tol": 0.0}, {"maxiter": 0}):
        with pytest.raises(ValueError, match="speigh needs"):
            speigh(A, A, 0.01, **kw)
    with pytest.raises(ValueError, match="speigh needs"):
        speigh(A, A, -0.01)


def test_exports_and_switches():
    import inspect
    import msmbuilder_amd
    from msmbuilder_amd import SparseTICA, decomposition, tICA
    from msmbuilder_amd.decomposition import speigh as S
    assert decomposition.SparseTICA is SparseTICA and issubclass(SparseTICA, tICA) and "SparseTICA" in decomposition.__all__
    assert msmbuilder_amd.SparseTICA is SparseTICA
    assert S.__all__ == ['speigh', 'scdeflate', 'project', 'solve_admm']
    sig = inspect.signature(S.speigh).parameters
    assert (sig["eps"].default, sig["tol"].default, sig["maxiter"].default, sig["method"].default) == (1e-6, 1e-8, 100, 1)
    init = inspect.signature(SparseTICA.__init__).parameters
    assert [k for k in init][1:] == ["n_components", "lag_time", "rho", "kinetic_mapping", "commute_mapping", "epsilon", "shrinkage",
                                     "tolerance", "maxiter", "verbose"]
    assert (init["rho"].default, init["epsilon"].default, init["tolerance"].default, init["maxiter"].default) == (0.01, 1e-6, 1e-6, 10000)
    m = SparseTICA(n_components=2, rho=0.5)
    assert (m.rho, m.n_components, m.shrinkage) == (0.5, 2, None)
    readme = open(os.path.join(ROOT, "README.md")).read()
    source = open(os.path.join(ROOT, "msmbuilder_amd", "csrc", "speigh.hip")).read()
    for switch in ("MSM_SPEIGH_BUDGET", "MSM_SPEIGH_GRID"):
        assert switch in readme and 'spg_env("%s")' % switch in source
