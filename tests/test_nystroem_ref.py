"""CPU tier of the Nystroem kernel map: tests/nystroem_ref.py (the restatement every GPU comparison uses, and its bound) is
held to scikit-learn's ``pairwise_kernels`` and ``Nystroem`` on float64 and to the reference's goldens, and scikit-learn's
own float64 result is shown to stay inside the bound on every case list the GPU tier uses -- a case that did not would be
removed from the list, not given a wider bound."""
import os

import numpy as np
import pytest
from sklearn.kernel_approximation import Nystroem as SkNystroem
from sklearn.metrics.pairwise import pairwise_kernels

import nystroem_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nystroem_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def sk_params(kernel):
    return {k: v for k, v in R.params(kernel).items() if k != "kernel" and v is not None}


def sk_map(X, Lm, B, c, kernel):
    out = pairwise_kernels(X, Lm, metric=kernel, filter_params=True, **sk_params(kernel)) @ B
    return out if c is None else out - c


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_restatement_matches_pairwise_kernels(kernel):
    for F in R.MAP_F:
        for L in R.MAP_L:
            X, Lm = R.data(F * 100 + L, 37, F, L)
            K = np.asarray(R.kernel_values(X, Lm, **R.params(kernel)), dtype=np.float64)
            Ks = pairwise_kernels(X, Lm, metric=kernel, filter_params=True, **sk_params(kernel))
            np.testing.assert_allclose(K, Ks, rtol=0, atol=3e-13 * max(1.0, np.abs(Ks).max()), err_msg="%s F=%d L=%d" % (kernel, F, L))


@pytest.mark.parametrize("kernel", R.KERNELS)
def test_sklearn_float64_is_inside_the_bound_on_the_map_cases(kernel):
    for F in R.MAP_F:
        for L in R.MAP_L:
            for P in sorted({1, 4, L}):
                X, Lm = R.data(F * 100 + L, 37, F, L)
                rs = np.random.RandomState(P)
                B, c = rs.randn(L, P), rs.randn(P)
                ref, terms = R.kernel_map(X, Lm, B, c, **R.params(kernel))
                R.check(sk_map(X, Lm, B, c, kernel), ref, terms, np.float64, "%s F=%d L=%d P=%d" % (kernel, F, L, P))


def test_sklearn_float64_is_inside_the_bound_on_uncentred_rows():
    X, Lm = R.data(5, 64, 16, 33, shift=100.0)
    B = np.random.RandomState(0).randn(33, 4)
    ref, terms = R.kernel_map(X, Lm, B, None, **R.params("rbf"))
    assert np.abs(ref).max() > 1e-3   # neighbours at distance ~ sqrt(2 F): the kernel values are not all underflow
    R.check(sk_map(X, Lm, B, None, "rbf"), ref, terms, np.float64, "rbf |mean|/std = 100")


@pytest.mark.parametrize("kernel", sorted(R.EST_CASES))
def test_estimator_cases_against_sklearn_and_golden(kernel, golden):
    for F, L in R.EST_CASES[kernel]:
        X, Lm = R.data(R.est_seed(kernel, F, L), 50, F, L)
        K = np.asarray(R.kernel_values(Lm, Lm, **R.params(kernel)), dtype=np.float64)
        ratio, _ = R.condition(K)
        assert ratio > 1e-6, (kernel, F, L, ratio)
        M = R.normalization(K)
        p = "%s_%d_%d_" % (kernel, F, L)
        tol = R.normalization_tolerance(Lm, **R.params(kernel))
        print(p, "normalization tolerance %.3g, difference %.3g" % (tol, np.abs(M - golden[p + "normalization"]).max()))
        assert np.abs(M - golden[p + "normalization"]).max() <= tol
        # scikit-learn's own Nystroem with the landmarks as its basis: the same definition
        sk = SkNystroem(kernel=kernel, n_components=L, **sk_params(kernel))
        sk.components_, sk.normalization_ = Lm, golden[p + "normalization"]
        ref, terms = R.kernel_map(X, Lm, golden[p + "normalization"].T, None, **R.params(kernel))
        R.check(sk.transform(X), ref, terms, np.float64, p + "sklearn transform")
        R.check(golden[p + "features"], ref, terms, np.float64, p + "golden features")


def test_random_basis_golden(golden):
    seqs = R.nystroem_sequences()
    allrows = np.concatenate(seqs)
    idx = np.random.RandomState(3).permutation(len(allrows))[:20]   # scikit-learn's stream
    assert np.array_equal(idx, golden["nys_indices"])
    assert np.array_equal(allrows[idx], golden["nys_components"])
    ref, terms = R.kernel_map(allrows, allrows[idx], golden["nys_normalization"].T, None, **R.params("rbf"))
    R.check(golden["nys_features"], ref, terms, np.float64, "Nystroem golden features")


def test_ktica_golden_is_decidable(golden):
    ev = golden["kt_eigenvalues"]
    assert ev.shape == (4,) and (np.diff(ev) < 0).all() and ev[0] > 0.95   # a slow hop, separated eigenvalues
    assert (np.abs(golden["kt_eigenvalues_f32_input"] - ev) < 1e-5 * np.abs(ev)).all()
    seqs, lm = R.ktica_sequences()
    ratio, _ = R.condition(R.kernel_values(lm, lm, R.KTICA_KW["kernel"], R.KTICA_KW["gamma"]))
    assert ratio > 1e-6
    assert golden["kt_transform"].shape == (sum(len(s) for s in seqs), 4)


def test_bound_scales_with_the_argument_before_cancellation():
    """The rbf bound of rows shifted by 100 is about (|x| + |l|)^2 / |x - l|^2 times the centred one: the term the device's
    product form pays for."""
    Xc, Lc = R.data(1, 8, 16, 8)
    B = np.eye(8)
    _, (core_c, _) = R.kernel_map(Xc, Lc, B, None, **R.params("rbf"))
    _, (core_s, _) = R.kernel_map(Xc + 100.0, Lc + 100.0, B, None, **R.params("rbf"))
    assert (core_s > 1e3 * core_c).all()
