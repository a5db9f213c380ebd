"""GPU tests of LandmarkAgglomerative under the divergence metrics and of MVCA, against the restatement of
tests/divergence_ref.py (scipy's linkage on the restated matrix, the restated pooling) and the reference's stored outputs
(tests/golden/mvca_golden.npz)."""
import os
import pickle

import numpy as np
import pytest

import divergence_ref as R

pytestmark = pytest.mark.gpu

MAX_LEFT_OUT = 0.02   # at most 2 % of the rows of a case may be too close to call


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "mvca_golden.npz")))


@pytest.fixture(scope="module")
def D(gpu):
    from msmbuilder_amd.utils import divergence
    return divergence


def fitted_msm(T):
    """A MarkovStateModel that carries the transition matrix T, as after a fit."""
    from msmbuilder_amd import MarkovStateModel
    n = len(T)
    msm = MarkovStateModel(verbose=False, lag_time=3)
    msm.transmat_, msm.populations_, msm.countsmat_ = T, np.full(n, 1.0 / n), np.ones((n, n))
    msm.mapping_, msm.n_states_ = dict(zip(range(n), range(n))), n
    return msm


def by_first_occurrence(labels):
    """The labels renamed 0, 1, ... in order of first appearance: equal for two numberings of one partition."""
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    return np.argsort(np.argsort(first))[inverse]


def assert_labels(got, ref, what, renamed=False):
    """Equal to the restated labels wherever the restated pooling decides by more than the bound; few rows may not.
    ``renamed``: the same partition under another numbering passes (landmarks drawn twice are at distance exactly 0 of
    each other, and the order of merges at height 0 -- hence fcluster's numbering -- is free)."""
    decided = R.decided_rows(ref["values"], ref["present"], ref["eps"])
    left_out = 1.0 - decided.mean()
    assert left_out <= MAX_LEFT_OUT, "%s: %.1f %% of the rows are closer than the bound" % (what, 100 * left_out)
    got, want = np.asarray(got)[decided], ref["predict"][decided]
    if renamed:
        got, want = by_first_occurrence(got), by_first_occurrence(want)
    assert np.array_equal(got, want), what
    return left_out


def assert_linkage(Z, ref, n, what):
    tol = R.height_tolerance(ref["D"], ref["DB"], n)
    assert R.relative_gap(ref["Z"][:, 2]) > 2 * tol, what + ": two merge heights are closer than the bound"
    assert np.array_equal(Z[:, [0, 1, 3]], ref["Z"][:, [0, 1, 3]]), what
    np.testing.assert_allclose(Z[:, 2], ref["Z"][:, 2], rtol=tol, err_msg=what)


# ---- LandmarkAgglomerative under a divergence --------------------------------------------------------------------------------
@pytest.mark.parametrize("linkage", R.LINKAGES)
@pytest.mark.parametrize("metric", ["js_metric", "js_metric_array", "sym_kl_divergence", "js_divergence_array"])
def test_landmark_agglomerative(gpu, D, metric, linkage):
    from msmbuilder_amd import LandmarkAgglomerative
    from msmbuilder_amd._lib import Arr
    from msmbuilder_amd.cluster import agglomerative as A
    n, blocks, seed = R.GEN_CASES[1]
    T = R.gen(n, blocks, seed, sparse=0.0 if metric.startswith("sym_kl") else 0.5)
    kind = metric[:-6] if metric.endswith("_array") else metric
    ref = R.mvca(T, blocks, kind=kind, linkage_name=linkage)
    assert_linkage(A.linkage_fit(Arr(T), kind, linkage), ref, n, "%s %s" % (kind, linkage))
    model = LandmarkAgglomerative(n_clusters=blocks, linkage=linkage, metric=getattr(D, metric) if metric.endswith("_array") else metric)
    labels = model.fit_predict([T])[0]
    assert np.array_equal(model.landmark_labels_, ref["landmark_labels"])
    assert_labels(labels, ref, "%s %s" % (kind, linkage))
    bound_w = 4 * R.U * len(ref["D"]) + 2 * float(np.max(ref["DB"] / np.maximum(ref["D"], R.TINY)))
    np.testing.assert_allclose(model.squared_distances_within_cluster_, ref["within"], rtol=bound_w)


def test_landmark_agglomerative_device_rows_and_landmarks(gpu):
    import torch
    from msmbuilder_amd import LandmarkAgglomerative
    n, blocks, seed = R.GEN_CASES[2]
    T = R.gen(n, blocks, seed)
    host = LandmarkAgglomerative(n_clusters=blocks, linkage="ward", metric="js_metric", n_landmarks=40)
    dev = LandmarkAgglomerative(n_clusters=blocks, linkage="ward", metric="js_metric", n_landmarks=40)
    lh = host.fit_predict([T])[0]
    ld = dev.fit_predict([torch.as_tensor(T, device="cuda")])[0]
    assert np.array_equal(lh, np.asarray(ld)) and np.array_equal(host.landmark_labels_, dev.landmark_labels_)
    assert_labels(lh, R.mvca(T, blocks, n_landmarks=40), "130 rows, 40 landmarks")
    f32 = LandmarkAgglomerative(n_clusters=blocks, linkage="ward", metric="js_metric").fit_predict([T.astype(np.float32)])[0]
    assert_labels(f32, R.mvca(T.astype(np.float32), blocks), "float32 rows")


def test_refusals_through_python(gpu, D):
    from msmbuilder_amd import MVCA, LandmarkAgglomerative
    T = R.gen(33, 3, 0)
    for bad in (D.kl_divergence_array, "kl_divergence", lambda a, b, i: np.zeros(len(b)), D.js_metric):
        with pytest.raises(ValueError):
            LandmarkAgglomerative(n_clusters=3, metric=bad).fit([T])
        with pytest.raises(ValueError):
            MVCA.from_msm(fitted_msm(T), 3, metric=bad)
    for entry in (np.nan, -0.5):
        X = T.copy()
        X[4, 2] = entry
        with pytest.raises(ValueError):
            LandmarkAgglomerative(n_clusters=3, linkage="ward", metric="js_metric").fit([X])
    with pytest.raises(ValueError):
        D.divergence_cdist(T, T[:, :5], "js_metric")
    with pytest.raises(ValueError):
        D.divergence_pdist(T, "js_metric", X_indices=[0, 40])
    with pytest.raises(ValueError):
        D.js_metric(T[0], T[1, :5])
    m = MVCA(None, verbose=False)
    with pytest.raises(RuntimeError, match="n_macrostates must not be None to fit"):
        m.fit([R.four_state_labels()])
    assert m.transmat_ is not None                   # raised after the MSM fit, as in the reference


# ---- MVCA --------------------------------------------------------------------------------------------------------------
def test_four_state_system_from_numpy_and_device_labels(gpu, golden):
    import torch
    from msmbuilder_amd import MVCA
    y = R.four_state_labels()
    first = None
    for seqs in ([y], [torch.as_tensor(y, device="cuda")], [y[:300], y[299:]]):   # (cut inside a stretch, the shared frame keeps every transition)
        m = MVCA(n_macrostates=2, verbose=False).fit(seqs)
        first = first if seqs[0] is not y else m
        assert np.array_equal(m.microstate_mapping_, golden["four_mapping"])
        f = MVCA(n_macrostates=2, fit_only=True, verbose=False).fit(seqs)
        assert np.array_equal(f.microstate_mapping_, golden["four_mapping_fit_only"])
    np.testing.assert_allclose(first.transmat_, golden["four_transmat"], atol=1e-7)
    macro = m.transform([y])
    truth = np.repeat([0, 1, 0, 1], 250)
    assert len(macro) == 1 and (np.array_equal(macro[0], truth) or np.array_equal(macro[0], 1 - truth))
    # labels outside the mapping: clip cuts the sequence there, fill marks them
    seq = np.array([0, 1, 7, 2, 3, 9, 9, 1])
    clip = m.partial_transform(seq)
    assert isinstance(clip, list) and [c.tolist() for c in clip] == [m.microstate_mapping_[[0, 1]].tolist(),
                                                                    m.microstate_mapping_[[2, 3]].tolist(),
                                                                    m.microstate_mapping_[[1]].tolist()]
    fill = m.partial_transform(seq, mode="fill")
    want = np.array([np.nan if s > 3 else m.microstate_mapping_[s] for s in seq], dtype=float)
    assert isinstance(fill, np.ndarray) and np.array_equal(fill, want, equal_nan=True)
    assert np.array_equal(m.partial_transform(torch.as_tensor(seq[:2], device="cuda"), mode="fill"), m.microstate_mapping_[[0, 1]])
    with pytest.raises(ValueError):
        m.partial_transform(seq, mode="wrap")


@pytest.mark.parametrize("name", ["four", "gen33", "gen65"])
def test_from_msm_against_the_reference(gpu, D, golden, name):
    from msmbuilder_amd import MVCA
    T = golden["four_transmat"] if name == "four" else R.gen(*R.GOLDEN_GEN[name])
    K = 2 if name == "four" else R.GOLDEN_GEN[name][1]
    n = len(T)
    msm = fitted_msm(T)
    ref = R.mvca(T, K)
    plain = MVCA.from_msm(msm, K)
    assert plain.pairwise_dists is None and plain.linkage is None and plain.elbow_data is None
    assert np.array_equal(plain.microstate_mapping_, golden[name + "_mapping"])
    assert_labels(plain.microstate_mapping_, ref, name)
    assert plain.transmat_ is msm.transmat_ and plain.populations_ is msm.populations_ and plain.mapping_ is msm.mapping_
    assert plain.countsmat_ is msm.countsmat_ and plain.n_states_ == n and plain.lag_time == 3
    assert np.array_equal(MVCA.from_msm(msm, K, fit_only=True).microstate_mapping_, golden[name + "_mapping_fit_only"])
    linked = MVCA.from_msm(msm, K, get_linkage=True)
    assert isinstance(linked.pairwise_dists, np.ndarray) and linked.pairwise_dists.shape == (n * (n - 1) // 2,)
    R.assert_within(linked.pairwise_dists, ref["D"], ref["DB"], name + " pairwise_dists")
    assert np.array_equal(linked.pairwise_dists, D.divergence_pdist(T, "js_metric"))
    np.testing.assert_allclose(linked.pairwise_dists, golden[name + "_pairwise"], rtol=0, atol=2 * float(np.max(ref["DB"])))
    assert_linkage(linked.linkage, ref, n, name)
    tol = R.height_tolerance(ref["D"], ref["DB"], n)
    assert np.array_equal(linked.linkage[:, [0, 1, 3]], golden[name + "_linkage"][:, [0, 1, 3]])
    np.testing.assert_allclose(linked.linkage[:, 2], golden[name + "_linkage"][:, 2], rtol=tol)
    assert np.array_equal(linked.elbow_data, linked.linkage[:, 2][::-1])
    only = MVCA.from_msm(msm, None, get_linkage=True)             # linkage outputs without a lumping
    assert np.array_equal(only.linkage, linked.linkage) and not hasattr(only, "microstate_mapping_")
    named = MVCA.from_msm(msm, K, metric="js_metric")
    assert np.array_equal(named.microstate_mapping_, plain.microstate_mapping_)


@pytest.mark.parametrize("strategy", ["stride", "random"])
@pytest.mark.parametrize("case", [0, 1])
def test_landmarks(gpu, case, strategy):
    """n_landmarks at None, n, n // 2 and a value that does not divide n (the reference raises IndexError below n)."""
    from msmbuilder_amd import MVCA
    from msmbuilder_amd.cluster.agglomerative import landmark_indices
    n, blocks, seed = R.GEN_CASES[case]
    T = R.gen(n, blocks, seed)
    msm = fitted_msm(T)
    for n_landmarks in (None, n, n // 2, n // 2 - 3):
        assert n_landmarks != n // 2 - 3 or n % n_landmarks
        ref = R.mvca(T, blocks, n_landmarks=n_landmarks, strategy=strategy, random_state=11)
        if n_landmarks is not None:
            assert np.array_equal(ref["indices"], landmark_indices(n, n_landmarks, strategy, 11))
        what = "n=%d landmarks=%s %s" % (n, n_landmarks, strategy)
        m = MVCA.from_msm(msm, blocks, n_landmarks=n_landmarks, landmark_strategy=strategy, random_state=11)
        assert m.microstate_mapping_.shape == (n,)
        renamed = strategy == "random" and n_landmarks is not None
        assert_labels(m.microstate_mapping_, ref, what, renamed)
        f = MVCA.from_msm(msm, blocks, n_landmarks=n_landmarks, landmark_strategy=strategy, random_state=11, fit_only=True)
        if renamed:
            assert np.array_equal(by_first_occurrence(f.microstate_mapping_), by_first_occurrence(ref["landmark_labels"])), what
        else:
            assert np.array_equal(f.microstate_mapping_, ref["landmark_labels"]), what


def test_params_clone_and_pickle(gpu):
    from sklearn.base import clone
    from msmbuilder_amd import MVCA
    from msmbuilder_amd.utils.divergence import js_divergence_array
    y = R.four_state_labels(1)
    m = MVCA(n_macrostates=2, metric=js_divergence_array, n_landmarks=3, landmark_strategy="random", random_state=5,
             lag_time=2, prior_counts=0.1, verbose=False)
    params = m.get_params()
    assert params["metric"] is js_divergence_array and params["lag_time"] == 2 and params["n_landmarks"] == 3
    c = clone(m)
    assert c.get_params() == params
    m.fit([y])
    c.fit([y])
    assert np.array_equal(m.microstate_mapping_, c.microstate_mapping_)
    again = pickle.loads(pickle.dumps(m))
    assert again.metric is js_divergence_array and np.array_equal(again.microstate_mapping_, m.microstate_mapping_)
    assert [x.tolist() for x in again.transform([y[:50]])] == [x.tolist() for x in m.transform([y[:50]])]
    m.set_params(n_macrostates=3, lag_time=1)
    assert m.n_macrostates == 3 and m.lag_time == 1


def test_condensed_route_equals_the_cdist_route(gpu, D):
    """With every row a landmark MVCA pools the condensed matrix it has; that is the cdist of the rows against the
    landmarks bit for bit: labels, pooled values, and host against device matrices."""
    import torch
    from msmbuilder_amd import MVCA, LandmarkAgglomerative
    from msmbuilder_amd.cluster import agglomerative as A
    n, blocks, seed = R.GEN_CASES[3]            # 257 rows: more than one workgroup of rows
    T = R.gen(n, blocks, seed)
    model = LandmarkAgglomerative(n_clusters=blocks, linkage="ward", metric="js_metric")
    via_cdist = model.fit_predict([T])[0]
    lumped = MVCA.from_msm(fitted_msm(T), blocks)
    assert np.array_equal(lumped.microstate_mapping_, via_cdist)
    assert_labels(via_cdist, R.mvca(T, blocks), "257 rows")
    perm, offsets = A.permute_by_cluster(model.landmark_labels_, blocks)
    intra = model.squared_distances_within_cluster_
    for pooling in R.LINKAGES:
        want = A.pooled_predict(T, T[perm], offsets, intra, "js_metric", pooling, want_pooled=True)
        cond = D.divergence_pdist(T, "js_metric")
        for dm in (cond, torch.as_tensor(cond, device="cuda")):
            got = A.pooled_predict_condensed(dm, n, perm, offsets, intra, pooling, want_pooled=True)
            lab, val = (x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in got[:2])
            assert np.array_equal(lab, want[0]) and np.array_equal(val, want[1]) and got[2] == want[2]
    L = gpu.lib()
    lab = np.zeros(n, dtype=np.int64)
    import ctypes as C
    neg = C.c_int(0)
    bad_perm = perm.copy()
    bad_perm[3] = n
    args = (offsets.ctypes.data, blocks, intra.ctypes.data, b"ward", lab.ctypes.data, None, C.byref(neg), 0)
    assert L.msm_landmark_predict_condensed(cond.ctypes.data, n, bad_perm.ctypes.data, *args) == gpu.MSM_ERR_INVALID
    assert L.msm_landmark_predict_condensed(None, n, perm.ctypes.data, *args) == gpu.MSM_ERR_INVALID
    assert L.msm_landmark_predict_condensed(cond.ctypes.data, 1, perm.ctypes.data, *args) == gpu.MSM_ERR_INVALID
