"""SparseTICA on the device against the reference's goldens (tests/golden/speigh_golden.npz) and the numpy restatement."""
import functools
import os
import pickle
import re

import numpy as np
import pytest

import speigh_ref as R

pytestmark = pytest.mark.gpu

NUMBER = re.compile(r"[-+]?(?:\d+\.\d*|\.\d+|\d+)(?:[eE][-+]?\d+)?")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "speigh_golden.npz"))


@functools.lru_cache(maxsize=None)
def data(F):
    X = R.rows(F, F)
    X.setflags(write=False)
    held = R.rows(F, F + 1000)[:200]
    held.setflags(write=False)
    return (X[:len(X) // 2], X[len(X) // 2:]), held


def same_text(got, want, rtol=1e-8):
    """Equal apart from the last digits of the printed numbers (the shrinkage is printed with 17 digits)."""
    assert NUMBER.sub("#", got) == NUMBER.sub("#", want)
    a = np.array([float(t) for t in NUMBER.findall(got)])
    b = np.array([float(t) for t in NUMBER.findall(want)])
    np.testing.assert_allclose(a, b, rtol=rtol)


CASES = [(F, k, ri, s) for F in (12, 33) for k in (1, 3) for ri in (0, 1) for s in (0, None)]


@pytest.mark.parametrize("F,k,ri,shrink", CASES)
def test_sparsetica_against_the_reference(gpu, F, k, ri, shrink):
    from msmbuilder_amd import SparseTICA
    G = golden()
    key = "stica_F%d_k%d_r%d_s%s_" % (F, k, ri, "none" if shrink is None else "0")
    assert key in G["stica_cases"].tolist()
    kinetic = bool(G[key + "kinetic"])
    seqs, held = data(F)
    if (k + ri) % 2:          # numpy and device-resident input in turn
        import torch
        seqs = [torch.as_tensor(s).cuda() for s in seqs]
    m = SparseTICA(n_components=k, lag_time=R.LAG, rho=(1e-3, 1e-2)[ri], shrinkage=shrink, kinetic_mapping=kinetic).fit(seqs)
    comp = G[key + "components"]
    assert m.components_.shape == comp.shape
    assert np.array_equal(np.abs(m.components_) > 0, np.abs(comp) > 0)
    np.testing.assert_allclose(m.eigenvalues_, G[key + "eigenvalues"], rtol=1e-10)
    np.testing.assert_allclose(m.timescales_, G[key + "timescales"], rtol=1e-9)
    # the vectors: 1e-8 max|v| / gap as for the device pair solve; the slow processes of this family stand at least 1e-2
    # apart from the rest of the masked spectrum
    np.testing.assert_allclose(m.components_, comp, rtol=0, atol=1e-6 * np.abs(comp).max())
    Y, Yr = np.asarray(m.transform([held])[0]), G[key + "transform"]
    assert Y.shape == Yr.shape
    np.testing.assert_allclose(Y, Yr, rtol=0, atol=1e-6 * np.abs(Yr).max())
    same_text(m.summarize(), str(G[key + "summary"]))
    assert len(m.solve_info_) == k and all(i["status"] == "converged" for i in m.solve_info_)


def test_two_well_process_is_found_alone(gpu):
    """The reference's double-well statement: one slow coordinate and nine white-noise features -- every entry of the
    component but the first is zero."""
    from msmbuilder_amd import SparseTICA
    X = R.two_well_rows(0)
    m = SparseTICA(n_components=1).fit([X[:10000], X[10000:]])
    c = m.components_[0]
    assert c[0] != 0 and not c[1:].any()
    u, v, info = R.speigh(m.offset_correlation_, m.covariance_, m.rho, m.epsilon, m.tolerance, m.maxiter)
    np.testing.assert_allclose(m.eigenvalues_[0], u, rtol=1e-10)
    np.testing.assert_allclose(c, v, rtol=1e-9)


def test_rho_zero_is_plain_tica(gpu):
    from msmbuilder_amd import SparseTICA, tICA
    seqs, held = data(12)
    a = SparseTICA(n_components=3, lag_time=R.LAG, rho=0).fit(seqs)
    b = tICA(n_components=3, lag_time=R.LAG).fit(seqs)
    assert np.array_equal(a.eigenvalues_, b.eigenvalues_) and np.array_equal(a.components_, b.components_)
    assert np.array_equal(a.transform([held])[0], b.transform([held])[0])


def test_raising_n_components_solves_again(gpu):
    from msmbuilder_amd import SparseTICA
    seqs, _ = data(12)
    m = SparseTICA(n_components=2, lag_time=R.LAG, rho=1e-3).fit(seqs)
    first = m.eigenvalues_.copy()
    info = m.solve_info_
    m.n_components = 1
    assert np.array_equal(m.eigenvalues_, first[:1]) and m.solve_info_ is info      # no new solve
    m.n_components = 3
    assert m.eigenvalues_.shape == (3,) and m.solve_info_ is not info and len(m.solve_info_) == 3
    fresh = SparseTICA(n_components=3, lag_time=R.LAG, rho=1e-3).fit(seqs)
    assert np.array_equal(m.eigenvalues_, fresh.eigenvalues_) and np.array_equal(m.components_, fresh.components_)


def test_pickle_then_partial_fit(gpu):
    from msmbuilder_amd import SparseTICA
    seqs, held = data(12)
    m = SparseTICA(n_components=2, lag_time=R.LAG, rho=1e-3).fit(seqs[:1])
    ev = m.eigenvalues_.copy()
    back = pickle.loads(pickle.dumps(m))
    assert back.rho == 1e-3 and np.array_equal(back.eigenvalues_, ev) and np.array_equal(back.components_, m.components_)
    back.partial_fit(seqs[1])
    whole = SparseTICA(n_components=2, lag_time=R.LAG, rho=1e-3).fit(seqs)
    np.testing.assert_allclose(back.eigenvalues_, whole.eigenvalues_, rtol=1e-10)
    assert np.array_equal(np.abs(back.components_) > 0, np.abs(whole.components_) > 0)


def test_float32_rows_compose_with_the_restatement(gpu):
    """float32 rows take the fp32 accumulation, whose moments differ from the reference's: the estimator is held to the
    restatement applied to its OWN moments (mask exact)."""
    from msmbuilder_amd import SparseTICA
    seqs, _ = data(33)
    m = SparseTICA(n_components=2, lag_time=R.LAG, rho=1e-2).fit([s.astype(np.float32) for s in seqs])
    A, B = m.offset_correlation_, m.covariance_
    vals, vecs = [], []
    for _ in range(2):
        u, v, info = R.speigh(A, B, m.rho, m.epsilon, m.tolerance, m.maxiter)
        vals.append(u)
        vecs.append(v)
        A = R.scdeflate(A, v)
    order = np.argsort(vals)[::-1]
    want = np.array(vecs)[order]
    assert np.array_equal(np.abs(m.components_) > 0, np.abs(want) > 0)
    np.testing.assert_allclose(m.eigenvalues_, np.array(vals)[order], rtol=1e-9)
    np.testing.assert_allclose(m.components_, want, rtol=0, atol=1e-6 * np.abs(want).max())


def test_refusals(gpu):
    from msmbuilder_amd import SparseTICA
    seqs, _ = data(12)
    for kw in ({"epsilon": 0.0}, {"tolerance": -1.0}, {"maxiter": 0}):
        m = SparseTICA(n_components=1, lag_time=R.LAG, **kw).fit(seqs)
        with pytest.raises(ValueError):
            m.eigenvalues_
    with pytest.raises(ValueError):
        SparseTICA(kinetic_mapping=True, commute_mapping=True)
