"""CPU tier of the KMeans tests: the reference Lloyd loop (tests/kmeans_lloyd_ref.py) is held against scikit-learn, live and
as captured in tests/golden/kmeans_golden.npz; every input of tests/test_gpu_kmeans_lloyd.py is shown to be decidable at every
iteration (no row whose best and second-best centre lie within the label rule's two bounds), which is what forces the
device's label sequence; and msm_lloyd_plan is checked against a restatement at its seams (it needs no device).

What the inputs are FOR is asserted here too, on the reference, so that an input that drifts fails loudly: the iterations at
which the ``late_*`` inputs relocate (odd, even, twice, last permitted iteration); which rows leave which donor in the
``donor_*`` inputs, their status and final sizes; that the K > 2048 inputs (label chunk of the histogram and scatter waves)
run at least three iterations with labels changing on both sides of cluster 2048 after the first; the empty clusters on both
sides of the base kernel's 256-cluster chunk; the plan of the unaligned-rows inputs; and that the estimator's default init
(k-means++) leaves scikit-learn's trajectory no choice."""
import os

import numpy as np
import pytest

import kmeans_label_ref as R
import kmeans_lloyd_ref as LR
from msmbuilder_amd.cluster.kmeans import lloyd_plan

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "kmeans_golden.npz")


def _plan(n, m, K, dtype):
    return lloyd_plan(n, m, K, dtype, True)


CASES = LR.trajectory_cases(_plan)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_gpu_input_is_decidable_at_every_iteration(name):
    X, init, max_iter, tol_abs = CASES[name]
    u = R.U_F32 if X.dtype == np.float32 else R.U_F64
    ref = LR.lloyd(X, init, max_iter, tol_abs, u=u, trace=name in LR.LABEL_CHUNK)
    assert ref["undecided"] and max(ref["undecided"]) == 0, ref["undecided"]
    schedule = [i for i, r in enumerate(ref["relocated"]) if r]
    if name.startswith("stop_"):
        assert ref["status"] == name[len("stop_"):]
        if name == "stop_tol":
            assert 3 < ref["n_iter"] < 300    # neither the first iterations nor the cap
    if name.startswith("reloc_"):
        want = LR.RELOC_AT_0[name]
        assert len(ref["relocated"][0]) == want
    if name.startswith("reloc_tie"):
        assert ref["relocated"][0] == [3] and np.array_equal(X[3], X[11])
    if name in LR.RELOC_TARGETS:    # the clusters that are empty at iteration 0 (either side of a chunk boundary), then none
        assert schedule == [0] and ref["status"] == LR.STRICT and ref["n_iter"] >= 3
        first = LR.lloyd(X, init, 1, 0.0, count_undecided=False)
        assert sorted(first["summed"][first["relocated"][0]]) == LR.RELOC_TARGETS[name] and ref["counts"].min() >= 1
    if name in LR.LABEL_CHUNK:
        # after the first iteration labels still change, in clusters below 2048 and in clusters from 2048 on
        assert ref["n_iter"] >= 3 and X.shape[0] > _plan(*X.shape, init.shape[0], X.dtype)["hist_span"]
        touched = np.concatenate([np.concatenate([a[a != b], b[a != b]]) for a, b in zip(ref["trace"], ref["trace"][1:])])
        print(name, "n_iter", ref["n_iter"], "clusters touched after the first iteration", len(np.unique(touched)))
        assert (touched < 2048).any(), touched
        assert (touched >= 2048).any() or init.shape[0] == 2048, touched    # (K = 2048 fills one chunk: no second side)
    if name in LR.LATE:
        dtype, seed, cap, want = LR.LATE[name]
        assert X.dtype == dtype and max_iter == cap and schedule == want, (seed, schedule)
        if "_last_" in name:    # the relocation is the last thing the run does; the labels are then taken once more
            assert ref["n_iter"] == max_iter == want[-1] + 1 and ref["status"] == LR.MAXITER
            assert len(ref["undecided"]) == max_iter + 1
        else:
            assert ref["n_iter"] < max_iter and ref["status"] == LR.STRICT
    if name == "late_odd_f64":
        assert len(ref["relocated"][1]) == 2
    if name in LR.DONOR:
        rows, n_iter, status, sizes = LR.DONOR[name]
        assert [list(map(int, r)) for r in ref["relocated"]] == rows
        assert (ref["n_iter"], ref["status"], ref["counts"].tolist()) == (n_iter, status, sizes)
        assert np.array_equal(X, np.round(X)) and np.abs(X).max() <= 100    # small integers: every sum is exact
    if name.startswith("donor_two"):      # both rows leave cluster 0, from two different points equally far from it
        first = LR.lloyd(X, init, 1, 0.0, trace=True)
        assert first["trace"][0][[3, 11]].tolist() == [0, 0] and not np.array_equal(X[3], X[11])
        assert np.array_equal(first["centers"], ref["centers"])    # the second iteration moves no centre: tol fires at 0 <= 0
    if name.startswith("donor_single"):   # cluster 1 is left without members and keeps its centre for an iteration
        first = LR.lloyd(X, init, 1, 0.0, trace=True)
        assert first["trace"][0][30] == 1 and np.sum(first["trace"][0] == 1) == 1
        assert first["counts"].tolist()[1:] == [0, 1] and np.array_equal(first["centers"][1], init[1])


def test_new_cases_cover_what_they_are_for():
    """The parities and repetitions the ``late_*`` cases were searched for, whatever the seeds."""
    by = {}
    for name, (dtype, seed, cap, want) in LR.LATE.items():
        by.setdefault(np.dtype(dtype).name, []).append((want, cap))
    for dt in ("float32", "float64"):
        assert any(w[-1] % 2 == 1 for w, _ in by[dt]) and any(w[-1] % 2 == 0 and w[-1] >= 2 for w, _ in by[dt])
    assert sum(len(w) == 2 for w, _ in by["float64"]) == 2
    assert any(cap == w[-1] + 1 for w, cap in by["float64"] + by["float32"])
    for name in LR.UNALIGNED:    # the plan of rows that are a whole number of 16-byte units long but start off the grid
        X, init = CASES[name][:2]
        assert (X.shape[1] * X.dtype.itemsize) % 16 == 0
        assert lloyd_plan(*X.shape, init.shape[0], X.dtype, True)["vec16"] == 1
        assert lloyd_plan(*X.shape, init.shape[0], X.dtype, False)["vec16"] == 0
    X, init = CASES["offset_f32_m512"][:2]
    assert lloyd_plan(*X.shape, init.shape[0], X.dtype, False)["feature_tiles"] == 4


def test_at_size_input_is_decidable():
    X, init, max_iter, tol_abs = LR.at_size_case()
    ref = LR.lloyd(X, init, max_iter, tol_abs)
    assert max(ref["undecided"]) == 0 and ref["n_iter"] <= max_iter
    # the GPU test's cheaper labeller gives exact_argmin's trajectory on this input
    fast = LR.lloyd(X, init, max_iter, tol_abs, count_undecided=False, argmin=LR.clear_argmin)
    assert fast["n_iter"] == ref["n_iter"] and fast["status"] == ref["status"]
    assert np.array_equal(fast["labels"], ref["labels"]) and np.array_equal(fast["summed"], ref["summed"])
    assert fast["centers"].tobytes() == ref["centers"].tobytes()


def _compare_with_sklearn_result(X, kw, centers, labels, n_iter):
    init = kw["init"]
    if isinstance(init, str):    # 'random': scikit-learn's draw, restated
        w = np.ones(X.shape[0])
        seeds = np.random.RandomState(kw["random_state"]).choice(X.shape[0], size=kw["n_clusters"], replace=False, p=w / w.sum())
        init = X[seeds]
    tol_abs = kw["tol"] * float(np.mean(np.var(X, axis=0)))
    ref = LR.lloyd(X, init, kw["max_iter"], tol_abs)
    assert max(ref["undecided"]) == 0
    assert ref["n_iter"] == int(n_iter)
    assert np.array_equal(ref["labels"], labels)
    assert np.all(np.abs(centers - ref["centers"]) <= LR.center_bound(X, ref["labels"], ref["centers"]))


@pytest.mark.parametrize("name", LR.GOLDEN_NAMES)
def test_reference_loop_against_the_scikit_learn_golden(name):
    z = np.load(GOLDEN)
    X, kw = LR.golden_inputs(name)
    _compare_with_sklearn_result(X, kw, z[name + "_centers"], z[name + "_labels"], z[name + "_n_iter"])


@pytest.mark.parametrize("name", LR.GOLDEN_NAMES)
def test_reference_loop_against_scikit_learn_live(name):
    cluster = pytest.importorskip("sklearn.cluster")
    X, kw = LR.golden_inputs(name)
    km = cluster.KMeans(algorithm="lloyd", **kw).fit(X)
    _compare_with_sklearn_result(X, kw, km.cluster_centers_, km.labels_, km.n_iter_)


@pytest.mark.parametrize("name", LR.GOLDEN_NAMES)
def test_default_init_against_scikit_learn_live_is_forced(name):
    """KMeans(n_clusters=K, n_init=1, random_state=3): scikit-learn's k-means++ draw on the centred rows, restated, then the
    reference loop.  Decidable at every iteration, and scikit-learn's own n_iter and labels: an estimator that makes the
    same draws has no choice (tests/test_gpu_kmeans_lloyd.py::test_default_init_equals_scikit_learn_live)."""
    cluster = pytest.importorskip("sklearn.cluster")
    X, kw = LR.default_init_inputs(name)
    km = cluster.KMeans(algorithm="lloyd", **kw).fit(X)
    mean = X.mean(axis=0)
    Xc = X - mean
    init, _ = cluster.kmeans_plusplus(Xc, kw["n_clusters"], random_state=np.random.RandomState(kw["random_state"]))
    ref = LR.lloyd(Xc, init, km.max_iter, km.tol * float(np.mean(np.var(X, axis=0))))
    print(name, "n_iter", ref["n_iter"], km.n_iter_, ref["status"])
    assert max(ref["undecided"]) == 0
    assert ref["n_iter"] == km.n_iter_ and ref["n_iter"] >= 3
    assert np.array_equal(ref["labels"], km.labels_)
    assert np.all(np.abs(km.cluster_centers_ - (ref["centers"] + mean)) <= LR.center_bound(X, ref["labels"], km.cluster_centers_))


def _plan_restated(n, m, K, dtype, aligned):
    """The update's launch plan, written out again: waves of 4096 rows, pieces of 256 members, tiles of at most 128 load units
    (16 bytes when the row pitch and the bases allow, else one element), a power of two."""
    esz = np.dtype(dtype).itemsize
    vec = bool(aligned) and (m * esz) % 16 == 0
    per = 16 // esz if vec else 1
    units = m // per
    tu = 1
    while tu < 128 and tu < units:
        tu *= 2
    return dict(hist_span=4096, hist_groups=-(-n // 4096), piece=256, pieces_max=-(-n // 256) + K, feature_tiles=-(-units // tu),
                tile_features=tu * per, vec16=int(vec))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lloyd_plan_at_its_seams(dtype):
    for n in (1, 255, 256, 257, 4095, 4096, 4097, 8192, 10 ** 7):
        for m in (1, 3, 4, 10, 127, 128, 129, 131, 256, 257, 512, 516, 2048):
            for K in (1, 127, 1000):
                for aligned in (0, 1):
                    got = lloyd_plan(n, m, K, dtype, aligned)
                    want = _plan_restated(n, m, K, dtype, aligned)
                    assert {k: got[k] for k in want} == want, (n, m, K, aligned)
                    assert got["scratch_bytes"] >= 3 * n * 4 + got["pieces_max"] * m * 8 + K * got["hist_groups"] * 4
