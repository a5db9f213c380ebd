"""tests/tica_solve_ref.py on the CPU: the designed eigenpairs and reduced matrix are what float64 LAPACK finds in the stored
moments, the finalisation identities are exact, and every named spectrum has the structure its name claims."""
import numpy as np
import pytest
import scipy.linalg

import tica_solve_ref as R

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("n", [33, 129])
@pytest.mark.parametrize("kappa", [1e2, 1e5, 1e8])
def test_designed_pairs_are_what_lapack_finds(n, kappa):
    """Forward error of the Cholesky reduction: ~ n eps cond(S) on eigenvalues of order 1; the vectors V = R^-1 W have
    entries up to sqrt(kappa) and inherit the same relative error over the gap (0.45 / 9 here)."""
    k = 10
    lam, k, _ = R.spectrum("gap", n, k)
    d = R.design(n, lam, kappa=kappa, seed=n, k=k)
    y = R.host_yardstick(d, k)
    bound = n * kappa * EPS
    assert y["eig"] <= bound, (y["eig"], bound)
    assert y["Cr"] <= bound, (y["Cr"], bound)
    assert y["back"] <= bound * np.abs(d["V"]).max()
    # the designed vectors solve the stored pencil and are S-orthonormal
    V, S, OC = d["V"], d["S"], d["OC"]
    np.testing.assert_allclose(V.T.dot(S).dot(V), np.eye(n), rtol=0, atol=bound)
    for j in d["top"]:
        res, sv = R.pencil_residual(OC, S, V[:, j], lam[j])
        assert res <= bound * sv, (j, res, sv)
    # LAPACK's vectors are the designed ones up to sign (gap 0.05)
    Vh = y["vecs"]
    for c, j in enumerate(d["top"]):
        sg = np.sign(Vh[:, c].dot(S).dot(V[:, j]))
        np.testing.assert_allclose(Vh[:, c] * sg, V[:, j], rtol=0, atol=bound / 0.05 * np.abs(V[:, j]).max())
    # R is THE Cholesky factor: upper triangular, positive diagonal
    assert np.array_equal(d["R"], np.triu(d["R"])) and (np.diag(d["R"]) > 0).all()
    np.testing.assert_allclose(scipy.linalg.cholesky(S), d["R"], rtol=0, atol=bound)
    s = np.linalg.eigvalsh(S)
    np.testing.assert_allclose(s[-1] / s[0], kappa, rtol=1e-6 * kappa / 1e2)


def test_finalisation_identities_are_exact():
    lam, k, _ = R.spectrum("gap", 33, 5)
    d = R.design(33, lam, seed=3, k=k)
    assert np.array_equal(d["OCf"], d["OC"]) and np.array_equal(d["Sf"], d["S"])
    assert np.array_equal(d["OC"], d["OC"].T) and np.array_equal(d["S"], d["S"].T)
    st = d["state"]
    assert st["n_observations_"] - st["lag_time"] * st["n_sequences_"] == 2 ** 20
    assert np.array_equal(st["_outer_0_to_TminusTau"], 2.0 ** 20 * d["S"])
    assert np.array_equal(st["_outer_offset_to_T"], 2.0 ** 20 * d["S"])
    # a nonzero mean is folded into all four accumulators and comes back exactly; the moments to rounding of mean^2
    mean = np.random.RandomState(0).standard_normal(33)
    dm = R.design(33, lam, seed=3, k=k, mean=mean)
    stm = dm["state"]
    assert np.array_equal((stm["_sum_0_to_TminusTau"] + stm["_sum_tau_to_T"]) / 2.0 ** 21, mean)
    assert np.array_equal(dm["OC"], d["OC"]) and np.array_equal(dm["V"], d["V"])
    tol = 4 * EPS * np.abs(mean).max() ** 2
    np.testing.assert_allclose(dm["OCf"], d["OC"], rtol=0, atol=tol)
    np.testing.assert_allclose(dm["Sf"], d["S"], rtol=0, atol=tol)
    assert not d["S"].flags.writeable and not st["_outer_0_to_T_lagged"].flags.writeable


@pytest.mark.parametrize("n,k", [(129, 10), (257, 16), (129, 1)])
def test_spectra_have_the_structure_their_names_claim(n, k):
    sp = R.spectra(n, k)
    assert set(sp) == set(R.SPECTRA) - ({"double"} if k % 2 else set())
    for name, (lam, kk, exempt) in sp.items():
        assert lam.shape == (n,) and (np.diff(lam) <= 0).all(), name
        assert kk == (16 if name == "wide_cluster" else k)
        assert R.exempt_count(lam, kk) == exempt, name
    lam = sp["gap"][0]
    assert 0.5 <= lam[k - 1] and lam[0] <= 0.95 and np.abs(lam[k:]).max() <= 0.08 and lam[k - 1] - lam[k] >= 0.42
    if k > 1:
        assert np.diff(lam[:k]).max() < -R.GAP_MIN
    if "double" in sp:
        lam = sp["double"][0]
        assert np.array_equal(lam[0:k:2], lam[1:k:2]) and (np.diff(lam[0:k:2]) < -R.GAP_MIN).all() and lam[k - 1] - lam[k] > 0.4
        assert sp["double"][2] == k
    lam = sp["edge_tie"][0]
    assert lam[k - 1] == lam[k] and lam[k] - lam[k + 1] > 0.4 and sp["edge_tie"][2] == 1
    lam = sp["negative"][0]
    assert lam.max() < 0 and -0.3 <= lam[k - 1] and lam[0] <= -0.05 and lam[k:].max() <= -0.6 and lam.min() >= -0.9
    lam = sp["neg_outlier"][0]
    assert lam[-1] == -0.97 and np.array_equal(lam[:-1], sp["gap"][0][:-1])
    lam = sp["near_one"][0]
    assert lam[0] == 1.0 - 1e-9 and np.array_equal(lam[1:], sp["gap"][0][1:])
    lam, kk, exempt = sp["wide_cluster"]
    assert ((lam >= 0.90) & (lam <= 0.91)).sum() == 40 and lam[40] <= 0.08 and exempt == 0
    assert np.allclose(-np.diff(lam[:40]), 0.01 / 39, rtol=1e-9, atol=0) and 0.01 / 39 > R.GAP_MIN and 40 > 32 > kk
    lam = sp["outside"][0]
    assert lam[0] == 1.7 and lam[-1] == -1.5 and np.array_equal(lam[1:-1], sp["gap"][0][1:-1])
    with pytest.raises(ValueError):
        R.spectrum("double", n, 3)
    with pytest.raises(ValueError):
        R.spectrum("nope", n, 2)


def test_not_positive_definite_state_names_the_minor():
    lam, k, _ = R.spectrum("gap", 33, 5)
    d = R.design(33, lam, seed=4, k=k)
    for p in (0, 7, 32):
        _, S = R.finalise(R.not_positive_definite(d, p))
        with pytest.raises(np.linalg.LinAlgError, match=r"%d-th leading minor" % (p + 1)):
            scipy.linalg.cholesky(S)
    assert np.array_equal(R.finalise(d["state"])[1], d["S"])          # the shared design is left alone


def test_case_is_shared_and_helpers_measure_what_they_say():
    a = R.case(129, "edge_tie", 10)
    assert R.case(129, "edge_tie", 10) is a
    d, y, k, exempt = a
    assert (k, exempt) == (10, 1) and y["eig"] <= 129 * 1e2 * EPS
    V, S = d["V"], d["S"]
    top = d["top"]
    assert R.s_projector_defect(V[:, top], S, V[:, top]) <= 1e-12
    assert R.s_projector_defect(V[:, top[:3]], S, V[:, top[1:4]]) > 0.5       # a different subspace is seen
    # the tied pair: any rotation inside it keeps the subspace of the first k + 1
    c, s_ = np.cos(0.3), np.sin(0.3)
    rot = V[:, [top[-1], k]].dot(np.array([[c, -s_], [s_, c]]))
    mixed = np.column_stack([V[:, top[:-1]], rot])
    assert R.s_projector_defect(mixed, S, V[:, :k + 1]) <= 1e-12
    res, sv = R.pencil_residual(d["OC"], S, rot[:, 0], d["lam"][k])
    assert res <= 129 * 1e2 * EPS * sv


@pytest.mark.parametrize("name", R.SPECTRA)
def test_gpu_module_checks_accept_lapack_and_reject_wrong_answers(name):
    """The assertions tests/test_gpu_tica_solve_designed.py applies to the device, applied here to float64 LAPACK's answer
    (accepted) and to answers that are wrong in the ways a top-k solver can be wrong (each rejected)."""
    import test_gpu_tica_solve_designed as T
    n = 129
    d, yard, k, exempt = R.case(n, name, 10)
    lam, V = d["lam"], d["V"]
    vals, vecs = yard["vals"].copy(), yard["vecs"].copy()
    T._check_designed(d, yard, k, exempt, name, vals, vecs, name)

    def rejected(v, X):
        with pytest.raises(AssertionError):
            T._check_designed(d, yard, k, exempt, name, v, X, name)

    # a true eigenpair that is not among the k largest (what a residual check alone cannot see)
    X = vecs.copy()
    X[:, k - 1] = V[:, k + 1]
    v = vals.copy()
    v[k - 1] = lam[k + 1]
    if lam[k + 1] != lam[k - 1]:
        rejected(v, X)
    # an eigenvalue off by 1e-10; a vector scaled by 1 + 1e-8
    v = vals.copy()
    v[0] += 1e-10
    rejected(v, vecs)
    X = vecs.copy()
    X[:, 0] *= 1.0 + 1e-8
    rejected(vals, X)
    # a wanted vector tilted by 1e-5 towards a direction outside the wanted set (the bulk)
    X = vecs.copy()
    X[:, 0] = np.cos(1e-5) * vecs[:, 0] + np.sin(1e-5) * V[:, n - 2]
    rejected(vals, X)
    # a vector tilted by 1e-5 towards a wanted neighbour that is NOT tied with it
    a, b = (0, 2) if name == "double" else (0, 1)
    X = vecs.copy()
    X[:, a], X[:, b] = (np.cos(1e-5) * vecs[:, a] + np.sin(1e-5) * vecs[:, b], np.cos(1e-5) * vecs[:, b] - np.sin(1e-5) * vecs[:, a])
    rejected(vals, X)
    # while a rotation INSIDE an exact pair is an equally good answer
    if name == "double":
        X = vecs.copy()
        X[:, 0], X[:, 1] = 0.6 * vecs[:, 0] + 0.8 * vecs[:, 1], 0.6 * vecs[:, 1] - 0.8 * vecs[:, 0]
        T._check_designed(d, yard, k, exempt, name, vals, X, name)
