"""MarkovStateModel on the GPU against the reference's semantics (tests/golden/msm_golden.npz, written by
tests/golden/make_golden_msm.py from the reference's msm.py / core.py), plus certificates of the device MLE."""
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import make_golden_msm as G  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = G.cases()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "msm_golden.npz"), allow_pickle=False)


def _fit(seqs, params):
    import warnings
    from msmbuilder_amd import MarkovStateModel
    p = dict(params)
    p['verbose'] = False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return MarkovStateModel(**p).fit(seqs)


def _cols_close(a, b, tol):
    assert a.shape == b.shape
    for i in range(a.shape[1]):
        s = 1.0 if np.dot(a[:, i], b[:, i]) >= 0 else -1.0
        np.testing.assert_allclose(s * a[:, i], b[:, i], rtol=tol, atol=tol * np.abs(b[:, i]).max())


def _loglik(C, T):
    nz = C > 0
    return float((C[nz] * np.log(T[nz])).sum())


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_parity(gpu, golden, name):
    seqs, params, score_seqs = CASES[name]
    m = _fit(seqs, params)
    g = {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + "_") and
         k[len(name) + 1:] in ("countsmat", "keys", "vals", "n_states", "percent", "transmat", "populations",
                               "eigenvalues", "lv", "rv", "timescales", "score_", "summary", "score", "eig_error")}
    assert np.array_equal(m.countsmat_, g["countsmat"])
    assert m.n_states_ == int(g["n_states"])
    keys = list(m.mapping_.keys())
    assert np.array_equal(np.array(keys), g["keys"])
    assert np.array_equal(np.array([m.mapping_[k] for k in keys], dtype=np.int64), g["vals"])
    assert float(m.percent_retained_) == float(g["percent"])
    np.testing.assert_allclose(m.transmat_, g["transmat"], rtol=1e-9, atol=0)
    # both solvers stop at a fixed-point residual of 1e-14; the error in pi is that residual over the spectral gap
    # (~1e-5 on the 299-state metastable chain), so its rarest states agree to ~1e-9 only
    np.testing.assert_allclose(m.populations_, g["populations"], rtol=1e-8 if name == "meta299" else 1e-9, atol=0)
    if "eig_error" in g:   # the reference fits and then refuses the eigensystem (non-finite matrix): so does this
        for attr in ("eigenvalues_", "left_eigenvectors_", "right_eigenvectors_", "timescales_"):
            with pytest.raises(ValueError) as e:
                getattr(m, attr)
            assert str(e.value) == str(g["eig_error"])
        return
    np.testing.assert_allclose(np.real(m.eigenvalues_), g["eigenvalues"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(np.real(m.timescales_), g["timescales"], rtol=1e-8)
    if params.get('reversible_type', 'mle') is not None:
        _cols_close(m.left_eigenvectors_, g["lv"], 1e-7)
        _cols_close(m.right_eigenvectors_, g["rv"], 1e-7)
    else:   # non-reversible: the columns of real eigenvalues (a complex pair's columns have an arbitrary phase)
        real = np.imag(m.eigenvalues_) == 0
        assert real.sum() >= 2
        _cols_close(np.real(m.left_eigenvectors_)[:, real], g["lv"][:, real], 1e-7)
        _cols_close(np.real(m.right_eigenvectors_)[:, real], g["rv"][:, real], 1e-7)
    np.testing.assert_allclose(np.real(m.score_), float(g["score_"]), rtol=1e-12)
    assert m.summarize() == str(g["summary"])
    if "score" in g:
        np.testing.assert_allclose(m.score(score_seqs), float(g["score"]), rtol=1e-9)


@pytest.mark.parametrize("name", ["ala", "meta299", "nan", "cut_num4"])
def test_mle_certificates(gpu, golden, name):
    seqs, params, _ = CASES[name]
    m = _fit(seqs, params)
    T, pi, C = m.transmat_, m.populations_, m.countsmat_
    flux = pi[:, None] * T
    assert np.abs(flux - flux.T).max() <= 1e-13 * flux.max()
    np.testing.assert_allclose(T.sum(1), 1.0, rtol=0, atol=1e-13)
    assert G.kkt_residual(C, pi) <= 1e-12
    assert m.mle_info_[1] == 1.0 and m.mle_info_[3] <= 1e-12
    ll, ll_gold = _loglik(C, T), _loglik(C, golden[name + "_transmat"])
    assert ll >= ll_gold - 1e-9 * abs(ll_gold)


@pytest.mark.parametrize("prior", [0.0, 0.5])
def test_sparse_dense_ab(gpu, monkeypatch, prior):
    """prior > 0 is added by the library and solved in the dense form; the same counts with the prior added by the
    caller (prior argument 0) go through the sparse form over a full pattern.  prior = 0: MSM_MLE_DENSE=1 forces dense."""
    from msmbuilder_amd.msm.msm import _transmat_mle
    seqs, params, _ = CASES["meta299"]
    C = _fit(seqs, params).countsmat_
    T1, pi1, S1, info1 = _transmat_mle(C + prior)
    if prior == 0.0:
        monkeypatch.setenv("MSM_MLE_DENSE", "1")
    T2, pi2, S2, info2 = _transmat_mle(C, prior=prior)
    assert info1[1] == info2[1] == 1.0
    np.testing.assert_allclose(T2, T1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(pi2, pi1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(S2, S1, rtol=1e-12, atol=0)
    assert np.array_equal(S1, S1.T) and np.array_equal(S2, S2.T)
    if prior:
        assert G.kkt_residual(C + prior, pi2) <= 1e-12 and (T2 > 0).all()


def test_prior_fit_uses_the_library_prior(gpu, golden):
    """MarkovStateModel(prior_counts=0.5) hands the prior to the library (dense form) and matches the golden."""
    seqs, params, _ = CASES["ala_lag5_prior"]
    m = _fit(seqs, params)
    from msmbuilder_amd.msm.msm import _transmat_mle
    T, pi, _, _ = _transmat_mle(m.countsmat_, prior=0.5, want_s=False)
    assert np.array_equal(m.transmat_, T) and np.array_equal(m.populations_, pi)
    np.testing.assert_allclose(m.transmat_, golden["ala_lag5_prior_transmat"], rtol=1e-9, atol=0)


def test_states_past_the_lds_copy(gpu):
    """K = 7,000 > 6,144: the solve keeps d in global memory instead of LDS."""
    from msmbuilder_amd.msm.msm import _transmat_mle
    K = 7000
    rs = np.random.RandomState(5)
    C = np.zeros((K, K))
    idx = np.arange(K)
    for off in (-2, -1, 0, 1, 2):
        C[idx, (idx + off) % K] += rs.poisson(40, K)
    for _ in range(4):                                   # long-range links: a well-mixed chain
        C[idx, rs.randint(0, K, K)] += rs.poisson(3, K)
    T, pi, _, info = _transmat_mle(C, want_s=False)
    assert info[1] == 1.0 and info[3] <= 1e-12
    assert G.kkt_residual(C, pi) <= 1e-12
    flux = pi[:, None] * T
    assert np.abs(flux - flux.T).max() <= 1e-13 * flux.max()
    np.testing.assert_allclose(T.sum(1), 1.0, rtol=0, atol=1e-13)


def test_device_labels(gpu):
    import torch
    seqs, params, _ = CASES["ala"]
    host = _fit(seqs, params)
    dev = _fit([torch.as_tensor(y).cuda() for y in seqs], params)
    assert dev.mapping_ == host.mapping_
    assert np.array_equal(dev.countsmat_, host.countsmat_)
    assert np.array_equal(dev.transmat_, host.transmat_)
    assert np.array_equal(dev.timescales_, host.timescales_)


def test_kcenters_labels_straight_in(gpu):
    import torch
    from msmbuilder_amd import KCenters
    rs = np.random.RandomState(3)
    Y = [torch.as_tensor((rs.randn(4000, 3).cumsum(0) * 0.05).astype(np.float32)).cuda() for _ in range(3)]
    kc = KCenters(n_clusters=12, random_state=0).fit(Y)
    assert all(torch.is_tensor(y) and y.is_cuda for y in kc.labels_)
    dev = _fit(kc.labels_, dict(lag_time=2, n_timescales=4))
    host = _fit([y.cpu().numpy() for y in kc.labels_], dict(lag_time=2, n_timescales=4))
    assert np.array_equal(dev.countsmat_, host.countsmat_) and dev.mapping_ == host.mapping_
    assert np.array_equal(dev.transmat_, host.transmat_)
    np.testing.assert_array_equal(dev.eigenvalues_, host.eigenvalues_)


def test_small_state_counts(gpu):
    m0 = _fit([np.array([0, 1, 2])], {})
    assert m0.n_states_ == 0 and m0.transmat_.shape == (0, 0) and m0.mapping_ == {}
    m1 = _fit([np.array([3, 3, 3, 3, 5])], {})
    assert m1.n_states_ == 1 and m1.transmat_.tolist() == [[1.0]] and m1.populations_.tolist() == [1.0]
    assert m1.eigenvalues_.tolist() == [1.0] and m1.timescales_.shape == (0,)
    m2 = _fit([np.array([0, 0, 1, 1, 1, 0, 0, 1, 0])], {})
    assert m2.n_states_ == 2
    T = m2.transmat_
    np.testing.assert_allclose(T.sum(1), 1.0, atol=1e-15)
    np.testing.assert_allclose(m2.populations_ @ T, m2.populations_, atol=1e-15)


def test_errors(gpu):
    from msmbuilder_amd import MarkovStateModel
    y = np.array([0, 1, 0, 1, 1, 0, 2])   # state 2 only as the last frame: no outgoing counts
    with pytest.warns(UserWarning):
        with pytest.raises(ValueError, match=r"^Row-sums of C must be positive\."):
            MarkovStateModel(ergodic_cutoff='off', verbose=False).fit([y])
    with pytest.raises(ValueError, match="reversible_type must be one of"):
        MarkovStateModel(reversible_type='bogus', verbose=False).fit([y])
    with pytest.raises(ValueError, match="Invalid lag_time"):
        MarkovStateModel(lag_time=0, verbose=False).fit([y])
    from msmbuilder_amd.msm.msm import _transmat_mle
    with pytest.raises(ValueError, match=r"^Domain error\. C must be positive\. Error code=-2$"):
        _transmat_mle(np.array([[1.0, -0.5], [1.0, 1.0]]))
    with pytest.raises(ValueError, match=r"^Row-sums of C must be positive\. Error code=-1$"):
        _transmat_mle(np.array([[0.0, 0.0], [1.0, 1.0]]))
    with pytest.raises(ValueError, match=r"^Row-sums of C must be positive\.Domain error\. C must be positive\. Error code=-1$"):
        _transmat_mle(np.array([[1.0, -1.0], [1.0, 1.0]]))


def test_pickle_and_params(gpu):
    seqs, params, _ = CASES["ala"]
    m = _fit(seqs, params)
    ts = m.timescales_
    m2 = pickle.loads(pickle.dumps(m))
    assert m2.get_params() == m.get_params()
    assert np.array_equal(m2.transmat_, m.transmat_) and np.array_equal(m2.timescales_, ts)
    assert m2.mapping_ == m.mapping_


def test_transform_roundtrip(gpu):
    seqs, params, _ = CASES["cut_on"]
    m = _fit(seqs, params)
    y = seqs[0]
    clipped = m.transform([y])                    # states 20..22 were trimmed: the tail is clipped
    assert len(clipped) == 1 and len(clipped[0]) == len(y) - 3
    filled = m.transform([y], mode='fill')[0]
    assert np.isnan(filled[-3:]).all() and np.array_equal(filled[:-3], clipped[0])
    back = m.inverse_transform(clipped)[0]
    assert np.array_equal(back, y[:-3])
    ev = m.eigtransform([y], mode='fill')[0]
    assert ev.shape == (len(y), m.n_states_ - 1) and np.isnan(ev[-3:]).all()
    assert m.state_labels_ == sorted(m.mapping_, key=m.mapping_.get)


def test_converges_where_the_reference_gives_up(gpu):
    """A 1,000-state metastable matrix: converges well inside max_iter with the KKT certificate."""
    from msmbuilder_amd.msm.msm import _transmat_mle, MAX_ITER
    C = G.well_counts(1000, 7)
    T, pi, S, info = _transmat_mle(C)
    assert info[1] == 1.0 and 0 < info[0] < MAX_ITER
    assert G.kkt_residual(C, pi) <= 1e-12
    flux = pi[:, None] * T
    assert np.abs(flux - flux.T).max() <= 1e-13 * flux.max()
