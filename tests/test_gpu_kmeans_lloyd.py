"""KMeans (full-batch Lloyd, msm_lloyd_run) on the GPU against the reference loop of tests/kmeans_lloyd_ref.py started from
the same init array.  Every input is decidable at every iteration (tests/test_kmeans_lloyd_ref.py), so the device has no
choice of labels and each iteration's centres are a function of its labels alone:

    n_iter, the stop rule that fired and the label of every row   equal
    centres   |c - c_ref| <= n_j 2^-53 max|x_member| + u_T |c_ref|   (a float64 sum in another order, one rounding to T)
    inertia   against the float64 sum at the device's own centres and labels in the inertia kernel's arithmetic
              (difference in T, square and sum in float64), n 2^-53 relative

Seam sizes (piece length, rows per histogram wave, features per tile) come from msm_lloyd_plan.  Beyond those, the cases of
``trajectory_cases`` hold: the label chunk of the histogram and scatter waves (K = 2048, 2049, 4097: one, two and three
chunks, with empty clusters in two of them); the base kernel's chunk of 256 clusters (K = 255, 256, 257, empty clusters on
both sides of cluster 256); a relocation at an odd and at an even iteration after the first, twice in one run, and in the last
permitted iteration (``late_*``); a donor that loses two rows in one update and a donor that loses its only row, keeps its
centre and is empty again (``donor_*``, small integers: the centres must come out exact).  A donor's device sum holds the
rows that left it, so its centre bound counts them (``center_bound``'s ``taken``, from the reference's own relocation).
test_rows_one_element_into_their_allocation runs the update on rows that are not 16-byte aligned (the per-element loads of
the segmented sum); test_default_init_equals_scikit_learn_live holds the estimator's default init to scikit-learn itself.
"""
import os

import numpy as np
import pytest

import kmeans_label_ref as R
import kmeans_lloyd_ref as LR
from msmbuilder_amd import KMeans
from msmbuilder_amd.cluster.kmeans import lloyd_plan, lloyd_run

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "kmeans_golden.npz")


def _plan(n, m, K, dtype):
    return lloyd_plan(n, m, K, dtype, True)


CASES = LR.trajectory_cases(_plan)
_REF = {}


def _reference(name, X, init, max_iter, tol_abs, argmin=None):
    if name not in _REF:
        _REF[name] = LR.lloyd(X, init, max_iter, tol_abs, count_undecided=False, argmin=argmin)
    return _REF[name]


def _check_against_reference(name, X, init, max_iter, tol_abs, argmin=None, rows=None):
    """``rows``: what is handed to lloyd_run in place of the host array X (a device tensor with X's values)."""
    ref = _reference(name, X, init, max_iter, tol_abs, argmin)
    centers, labels, inertia, n_iter, status = lloyd_run(X if rows is None else rows, init, max_iter, tol_abs)
    if rows is not None:
        labels = labels.cpu().numpy()
    print(name, "n_iter", n_iter, ref["n_iter"], "status", LR.STATUS_OF[status], ref["status"], "inertia", inertia)
    assert n_iter == ref["n_iter"]
    assert LR.STATUS_OF[status] == ref["status"]
    assert labels.dtype == np.int32 and np.array_equal(labels, ref["labels"])
    assert centers.dtype == X.dtype
    err = np.abs(centers.astype(np.float64) - ref["centers"].astype(np.float64))
    # (the members the last update summed, and the rows its relocation took out of a donor's sum again)
    bound = LR.center_bound(X, ref["summed"], ref["centers"], taken=ref["taken"])
    print(name, "max centre error / bound", float(np.max(err / np.maximum(bound, 1e-300))))
    assert np.all(err <= bound)
    want = LR.kernel_inertia(X, centers, labels)
    print(name, "inertia", inertia, "restated", want)
    assert abs(inertia - want) <= X.shape[0] * 2.0 ** -53 * want
    return centers, labels, ref


@pytest.mark.parametrize("name", sorted(CASES))
def test_trajectory_equals_the_reference_loop(name):
    X, init, max_iter, tol_abs = CASES[name]
    centers, labels, ref = _check_against_reference(name, X, init, max_iter, tol_abs)
    if name.startswith("stop_"):
        assert ref["status"] == name[len("stop_"):]          # which rule fired
        if name != "stop_strict":                            # the returned labels belong to the FINAL centres
            assert np.array_equal(labels, R.exact_argmin(X, centers)[0])
    if name.startswith("reloc_"):
        assert len(ref["relocated"][0]) >= 1
        assert np.bincount(labels, minlength=init.shape[0]).min() >= 1
    if name in LR.LATE:
        assert [i for i, r in enumerate(ref["relocated"]) if r] == LR.LATE[name][3]
        if "_last_" in name:                                 # the relocation closes the run: labels against the FINAL centres
            assert ref["status"] == LR.MAXITER and np.array_equal(labels, R.exact_argmin(X, centers)[0])
    if name in LR.DONOR:                                     # small integers: every sum is exact, so is every centre
        assert (ref["n_iter"], ref["status"]) == LR.DONOR[name][1:3]
        assert np.array_equal(centers, ref["centers"])
    if name.startswith("donor_single_cut"):                  # the donor that lost its only row keeps its centre
        assert ref["counts"][1] == 0 and np.array_equal(centers[1], init[1])


@pytest.mark.parametrize("name", LR.UNALIGNED)
def test_rows_one_element_into_their_allocation(name):
    """Contiguous device rows that are a whole number of 16-byte units long but start one element into their allocation:
    the update must read them by the element (``lloyd_segsum_kernel<T, false>``, units = m), and the run is held to the same
    reference as the aligned run of the same input.  (Not to the aligned run's bits: the lane partition of the sum differs.)"""
    import torch
    X, init, max_iter, tol_abs = CASES[name]
    n, m = X.shape
    buf = torch.empty(n * m + 1, dtype=torch.from_numpy(X).dtype, device="cuda")
    view = buf[1:].view(n, m)
    view.copy_(torch.from_numpy(X))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 != 0 and view.is_contiguous()
    assert (m * X.dtype.itemsize) % 16 == 0
    assert lloyd_plan(n, m, init.shape[0], X.dtype, aligned=True)["vec16"] == 1
    plan = lloyd_plan(n, m, init.shape[0], X.dtype, aligned=False)
    assert plan["vec16"] == 0 and plan["tile_features"] * plan["feature_tiles"] >= m
    if name == "offset_f32_m512":
        assert plan["feature_tiles"] == 4
    _check_against_reference(name, X, init, max_iter, tol_abs, rows=view)
    assert torch.equal(view.cpu(), torch.from_numpy(X))    # the rows are read, never written


def test_at_size_2m_rows():
    X, init, max_iter, tol_abs = LR.at_size_case()
    # (clear_argmin: exact_argmin's labels on this input -- tests/test_kmeans_lloyd_ref.py -- in seconds)
    _check_against_reference("at_size", X, init, max_iter, tol_abs, argmin=LR.clear_argmin)


def test_two_fits_give_the_same_bits(monkeypatch):
    rs = np.random.RandomState(80)
    X = rs.randn(200000, 10).astype(np.float32)
    init = X[rs.choice(len(X), 200, replace=False)].copy()
    a = lloyd_run(X, init, 6, 0.0)
    b = lloyd_run(X, init, 6, 0.0)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3] == 6
    monkeypatch.setenv("MSM_LABEL_XCD", "0")
    c = lloyd_run(X, init, 6, 0.0)
    assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[1], c[1])
    # wide rows, where MSM_LABEL_XCD selects another label kernel
    Xw, initw = LR.blobs(70000, 64, 300, np.float32, 81)
    d = lloyd_run(Xw, initw, 4, 0.0)
    monkeypatch.delenv("MSM_LABEL_XCD")
    e = lloyd_run(Xw, initw, 4, 0.0)
    assert d[0].tobytes() == e[0].tobytes() and np.array_equal(d[1], e[1])


# ---------------------------------------------------------------------------------------------------------------------
# the estimator
# ---------------------------------------------------------------------------------------------------------------------
def _seqs(X, cuts):
    return [X[a:b].copy() for a, b in zip([0] + cuts, cuts + [len(X)])]


def test_ragged_sequences_torch_equals_numpy_and_predict():
    import torch
    X, init = LR.blobs(3001, 10, 6, np.float32, 90, spread=0.5)
    seqs = _seqs(X, [17, 900, 901, 2500])
    km = KMeans(n_clusters=6, init=init, n_init=1, tol=0.0).fit(seqs)
    assert [len(l) for l in km.labels_] == [len(s) for s in seqs]
    assert km.cluster_centers_.dtype == np.float32 and km.n_features_in_ == 10
    ref = LR.lloyd(X, init)
    assert np.array_equal(np.concatenate(km.labels_), ref["labels"]) and km.n_iter_ == ref["n_iter"]
    pred = km.predict(seqs)
    assert all(np.array_equal(p, l) for p, l in zip(pred, km.labels_))
    assert km.score(seqs[:1]) <= 0.0 and "KMeans" in km.summarize()
    dev = [torch.from_numpy(s).cuda() for s in seqs]
    kd = KMeans(n_clusters=6, init=init, n_init=1, tol=0.0).fit(dev)
    assert kd.cluster_centers_.tobytes() == km.cluster_centers_.tobytes()
    assert kd.inertia_ == km.inertia_ and kd.n_iter_ == km.n_iter_
    assert all(l.is_cuda and np.array_equal(l.cpu().numpy(), h) for l, h in zip(kd.labels_, km.labels_))
    assert all(torch.equal(d, torch.from_numpy(s).cuda()) for d, s in zip(dev, seqs))    # copy_x=True: rows untouched


def test_n_init_keeps_the_lowest_inertia():
    X, _ = LR.drift(4000, 5, 8, np.float64, 91)
    km = KMeans(n_clusters=8, init="random", n_init=3, random_state=5, max_iter=50).fit([X])
    rs = np.random.RandomState(5)
    w = np.ones(len(X))
    runs = []
    for _ in range(3):
        seeds = rs.choice(len(X), size=8, replace=False, p=w / w.sum())
        runs.append(KMeans(n_clusters=8, init=X[seeds], n_init=1, max_iter=50).fit([X]))
    best = min(runs, key=lambda r: r.inertia_)
    print("inertias", [r.inertia_ for r in runs], "kept", km.inertia_)
    assert km.inertia_ == best.inertia_ and km.cluster_centers_.tobytes() == best.cluster_centers_.tobytes()
    k = KMeans(init="random")
    k._check_params_vs_input(100)
    assert k._n_init == 10
    k = KMeans()
    k._check_params_vs_input(100)
    assert k._n_init == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_copy_x_false_restores_the_rows_within_one_rounding(dtype):
    import torch
    X, init = LR.blobs(2000, 10, 4, dtype, 92, spread=0.5)
    xd = torch.from_numpy(X).cuda()
    km = KMeans(n_clusters=4, init=init, n_init=1, copy_x=False).fit([xd])
    back = xd.cpu().numpy()
    u = 2.0 ** -53 if dtype == np.float64 else 2.0 ** -24
    m = np.abs(X.astype(np.float64).mean(axis=0))
    # fl(fl(x - m) + m): half an ulp of |x - m| <= |x| + |m|, then half an ulp of the sum
    assert np.all(np.abs(back.astype(np.float64) - X) <= 1.01 * u * (2 * np.abs(X.astype(np.float64)) + m))
    ref = KMeans(n_clusters=4, init=init, n_init=1).fit([X])
    assert ref.cluster_centers_.tobytes() == km.cluster_centers_.tobytes()


@pytest.mark.parametrize("name", LR.GOLDEN_NAMES)
def test_scikit_learn_golden(name):
    z = np.load(GOLDEN)
    X, kw = LR.golden_inputs(name)
    km = KMeans(**kw).fit([X])
    print(name, "n_iter", km.n_iter_, int(z[name + "_n_iter"]), "inertia", km.inertia_, float(z[name + "_inertia"]))
    assert km.n_iter_ == int(z[name + "_n_iter"])
    assert np.array_equal(km.labels_[0], z[name + "_labels"])
    want = z[name + "_centers"]
    assert np.all(np.abs(km.cluster_centers_ - want) <= LR.center_bound(X, z[name + "_labels"], want))


@pytest.mark.parametrize("name", LR.GOLDEN_NAMES)
def test_default_init_equals_scikit_learn_live(name):
    """The estimator's default, k-means++ on the centred rows on the device, against scikit-learn with the same arguments.
    tests/test_kmeans_lloyd_ref.py shows the trajectory forced once the draws are scikit-learn's."""
    import torch
    cluster = pytest.importorskip("sklearn.cluster")
    X, kw = LR.default_init_inputs(name)
    sk = cluster.KMeans(algorithm="lloyd", **kw).fit(X)
    bound = LR.center_bound(X, sk.labels_, sk.cluster_centers_)
    for rows in (X, torch.from_numpy(X).cuda()):
        km = KMeans(**kw).fit([rows])
        labels = km.labels_[0] if rows is X else km.labels_[0].cpu().numpy()
        err = np.abs(km.cluster_centers_ - sk.cluster_centers_)
        print(name, type(rows).__name__, "n_iter", km.n_iter_, sk.n_iter_, "max centre error / bound", float(np.max(err / bound)))
        assert km.n_iter_ == sk.n_iter_
        assert np.array_equal(labels, sk.labels_)
        assert np.all(err <= bound)


def test_error_cases():
    X = np.random.RandomState(0).randn(20, 3)
    with pytest.raises(ValueError, match="n_samples=20 should be >= n_clusters=21"):
        KMeans(n_clusters=21).fit([X])
    with pytest.raises(ValueError, match="does not match the number of clusters"):
        KMeans(n_clusters=4, init=np.zeros((3, 3))).fit([X])
    with pytest.raises(ValueError, match="does not match the number of features"):
        KMeans(n_clusters=4, init=np.zeros((4, 2))).fit([X])
    for bad in (0, -1, "many", 1.5):
        with pytest.raises(ValueError, match="n_init"):
            KMeans(n_clusters=4, n_init=bad).fit([X])
    assert KMeans(n_clusters=2, algorithm="elkan", random_state=0).fit([X]).cluster_centers_.shape == (2, 3)
    cb = KMeans(n_clusters=2, init=lambda Xc, k, random_state: Xc[:k], n_init=1).fit([X])
    assert cb.cluster_centers_.shape == (2, 3)
