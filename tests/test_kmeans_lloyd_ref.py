"""CPU tier of the KMeans tests: the reference Lloyd loop (tests/kmeans_lloyd_ref.py) is held against scikit-learn, live and
as captured in tests/golden/kmeans_golden.npz; every input of tests/test_gpu_kmeans_lloyd.py is shown to be decidable at every
iteration (no row whose best and second-best centre lie within the label rule's two bounds), which is what forces the
device's label sequence; and msm_lloyd_plan is checked against a restatement at its seams (it needs no device)."""
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
    ref = LR.lloyd(X, init, max_iter, tol_abs, u=u)
    assert ref["undecided"] and max(ref["undecided"]) == 0, ref["undecided"]
    if name.startswith("stop_"):
        assert ref["status"] == name[len("stop_"):]
        if name == "stop_tol":
            assert 3 < ref["n_iter"] < 300    # neither the first iterations nor the cap
    if name.startswith("reloc_"):
        want = {"reloc_one": 1, "reloc_three": 3, "reloc_one_f32": 1, "reloc_tie_f64": 1, "reloc_tie_f32": 1}[name]
        assert len(ref["relocated"][0]) == want
    if name.startswith("reloc_tie"):
        assert ref["relocated"][0] == [3] and np.array_equal(X[3], X[11])


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
