"""The rmsd metric on the card: libdistance's five functions, KCenters, KMedoids and MiniBatchKMedoids on conformations,
against the restatement in tests/rmsd_ref.py (values within its derived bound, decisions on the rows whose margin
exceeds twice the bound) and against each other (one definition: the same bits for the same pair on every path).

Seams of the kernels: a wave's MFMA tile is 32 x 32, a tile-kernel workgroup holds 4 tiles = 128 frames, a row-kernel
workgroup 256 frames; neither kernel loops over a fixed grid (the grid covers the frames), so "one grid round + 1" is
several workgroups + 1 here: 1025.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import kmedoids_ref as KR
import rmsd_ref as R

pytestmark = pytest.mark.gpu

FRAME_COUNTS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025)
CENTRE_COUNTS = (1, 2, 31, 32, 33, 65)
ATOMS = (1, 2, 3, 4, 5, 33, 257)
_worst = {"ratio": 0.0}


def ld():
    from msmbuilder_amd import libdistance
    return libdistance


def host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def gauss_ref(n, K, A, seed, offset=0.0):
    """(X, Y, D, B), computed once and shared read-only; a prefix of X / Y has the matching block of D / B."""
    X, Y = R.gaussian_frames(n, A, seed, offset=offset), R.gaussian_frames(K, A, seed + 1000, offset=offset)
    D, B = R.cdist(R.Frames(X), R.Frames(Y))
    return freeze(X, Y, D, B)


@functools.lru_cache(maxsize=None)
def self_ref(n, A, seed):
    """(X, D, B) of the frames against themselves."""
    X = R.gaussian_frames(n, A, seed)
    f = R.Frames(X)
    D, B = R.cdist(f, f)
    return freeze(X, D, B)


def within(got, D, B, what):
    got = host(got)
    assert got.shape == D.shape and got.dtype == np.float64, what
    both_nan = np.isnan(got) & np.isnan(D)
    err = np.abs(got - D)
    ok = (err <= B) | both_nan
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.nanmax(np.where(B > 0, err / B, 0.0)) if got.size else 0.0
    _worst["ratio"] = max(_worst["ratio"], float(ratio))
    print("%s: largest error / bound %.3g (largest so far %.3g)" % (what, ratio, _worst["ratio"]))
    assert ok.all(), (what, float(np.nanmax(err - B)))


def same_bits(a, b, what):
    a, b = host(a), host(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8) if a.dtype != np.float64 else a.view(np.uint64),
                          b.view(np.uint8) if b.dtype != np.float64 else b.view(np.uint64)), what


def check_assign(X, Y, D, B, what, X_indices=None):
    L = ld()
    fx, fy = L.RmsdFrames(X), L.RmsdFrames(Y)
    labels, mind, inertia = L.rmsd_assign(fx, fy, X_indices)
    cd = host(L.cdist(fx, fy, "rmsd"))
    if X_indices is not None:
        sel = host(X_indices)
        cd, D, B = cd[sel], D[sel], B[sel]
    own_labels, own_min, own_inertia, _ = R.assign_loop(cd)   # first strict minimum below FLT_MAX
    assert np.array_equal(host(labels), own_labels), what             # the tie rule on the card's own distances, every row
    same_bits(mind, own_min, what + " min_dist")                       # one definition: the tile kernel's two epilogues
    assert abs(inertia - own_inertia) <= len(own_min) * R.U64 * np.abs(own_min).sum(), what
    ref_labels, _, _, margin = R.assign_loop(D)
    decided = margin > 2 * np.max(np.where(np.isnan(B), np.inf, B), axis=1)   # (a row with a NaN pair is not decided)
    assert np.array_equal(host(labels)[decided], ref_labels[decided]), what
    public = L.assign_nearest(X, Y, "rmsd", X_indices=X_indices)
    assert np.array_equal(host(public[0]), host(labels)) and public[1] == inertia
    return decided


# ---- values and the one definition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FRAME_COUNTS)
def test_frame_counts(gpu, n):
    L = ld()
    X, Y, D, B = gauss_ref(1025, 33, 5, 11)
    X, D, B = X[:n], D[:n], B[:n]
    cd = L.cdist(X, Y, "rmsd")
    within(cd, D, B, "cdist n=%d" % n)
    for j in (0, 32):
        same_bits(L.dist(X, Y[j], "rmsd"), cd[:, j], "dist against cdist's column %d" % j)   # row kernel against tile kernel
    check_assign(X, Y, D, B, "assign n=%d" % n)
    if n <= 129:
        Xs, Ds, Bs = self_ref(129, 5, 12)
        pd = L.pdist(Xs[:n], "rmsd")
        within(pd, R.condensed(Ds[:n, :n]), R.condensed(Bs[:n, :n]), "pdist n=%d" % n)
        same_bits(pd, R.condensed(host(L.cdist(Xs[:n], Xs[:n], "rmsd"))), "pdist against cdist")


@pytest.mark.parametrize("K", CENTRE_COUNTS)
def test_centre_counts(gpu, K):
    L = ld()
    X, Y, D, B = gauss_ref(65, 65, 4, 21)
    Y, D, B = Y[:K], D[:, :K], B[:, :K]
    cd = L.cdist(X, Y, "rmsd")
    within(cd, D, B, "cdist K=%d" % K)
    same_bits(L.dist(X, Y[K - 1:K], "rmsd"), cd[:, K - 1], "dist against cdist's last column")
    decided = check_assign(X, Y, D, B, "assign K=%d" % K)
    assert decided.mean() >= 0.9   # (Gaussian conformations: nearly every row is decided)


@pytest.mark.parametrize("A", ATOMS)
def test_atom_counts(gpu, A):
    L = ld()
    X, Y, D, B = gauss_ref(65, 33, A, 30 + A)
    cd = L.cdist(X, Y, "rmsd")
    within(cd, D, B, "cdist A=%d" % A)
    same_bits(L.dist(X, Y[7], "rmsd"), cd[:, 7], "dist against cdist (odd and even atom counts share the k-step rule)")
    check_assign(X, Y, D, B, "assign A=%d" % A)
    Xs, Ds, Bs = self_ref(65, A, 60 + A)
    pd = L.pdist(Xs, "rmsd")   # 65 frames: three tile rows, the diagonal tiles masked, the tiles below skipped
    within(pd, R.condensed(Ds), R.condensed(Bs), "pdist A=%d" % A)
    pairs = np.array([[0, 1], [1, 0], [5, 5], [64, 3], [64, 3], [31, 32], [0, 64]], dtype=np.int64)   # repeated and self pairs
    full = host(L.cdist(Xs, Xs, "rmsd"))
    want = full[pairs[:, 0], pairs[:, 1]]
    got = L.sumdist(Xs, "rmsd", pairs)
    assert abs(got - want.sum()) <= len(want) * R.U64 * np.abs(want).sum()
    assert abs(got - Ds[pairs[:, 0], pairs[:, 1]].sum()) <= Bs[pairs[:, 0], pairs[:, 1]].sum() + 1e-15


class Duck(object):
    def __init__(self, xyz):
        self.xyz = xyz


def test_host_device_and_duck_inputs_agree(gpu):
    import torch
    L = ld()
    X, Y, D, B = gauss_ref(65, 33, 33, 63)
    pairs = np.array([[0, 1], [2, 2], [64, 0]], dtype=np.int64)
    before = X.copy()
    base = (L.cdist(X, Y, "rmsd"), L.dist(X, Y[3], "rmsd"), L.pdist(X, "rmsd"), L.assign_nearest(X, Y, "rmsd"),
            L.sumdist(X, "rmsd", pairs))
    assert all(isinstance(b, np.ndarray) for b in base[:3]) and isinstance(base[3][0], np.ndarray)
    Xd, Yd = cuda(X), cuda(Y)
    forms = {"device": (Xd, Yd, cuda(pairs)), "duck": (Duck(X), Duck(Y), pairs), "device duck": (Duck(Xd), Duck(Yd), cuda(pairs)),
             "prepared": (L.RmsdFrames(X), L.RmsdFrames(Y), pairs)}
    for name, (x, y, p) in forms.items():
        y3 = y.xyz[3] if isinstance(y, Duck) else (Y[3] if isinstance(y, L.RmsdFrames) else y[3])
        got = (L.cdist(x, y, "rmsd"), L.dist(x, y3, "rmsd"), L.pdist(x, "rmsd"), L.assign_nearest(x, y, "rmsd"),
               L.sumdist(x, "rmsd", p))
        if "device" in name:
            assert all(torch.is_tensor(g) and g.is_cuda for g in got[:3]) and got[3][0].is_cuda
        for g, b in zip(got[:3], base[:3]):
            same_bits(g, b, name)
        assert np.array_equal(host(got[3][0]), base[3][0]) and got[3][1] == base[3][1] and got[4] == base[4], name
    assert np.array_equal(X, before) and np.array_equal(host(Xd), before)   # inputs are never centred in place
    fx = L.RmsdFrames(Xd)
    assert fx.xyz is Xd and fx.shape == (65, 33, 3) and len(fx) == 65
    assert np.array_equal(fx.frames([4, 0, 4]), X[[4, 0, 4]])


@pytest.mark.parametrize("where", ["host", "device"])
def test_x_indices(gpu, where):
    L = ld()
    X, Y, D, B = gauss_ref(65, 33, 5, 71)
    idx = np.array([64, 5, 5, 0, 33, 32, 31, 5, 64, 1] + list(range(40, 8, -1)), dtype=np.int64)   # repeats, out of order
    x, ix = (X, idx) if where == "host" else (cuda(X), cuda(idx))
    fx = L.RmsdFrames(x)
    same_bits(L.dist(fx, Y[2], "rmsd", X_indices=ix), host(L.dist(fx, Y[2], "rmsd"))[idx], "dist")
    check_assign(x, Y, D, B, "assign with X_indices", X_indices=ix)
    full = host(L.cdist(fx, fx, "rmsd"))
    same_bits(L.pdist(fx, "rmsd", X_indices=ix), R.condensed(full[np.ix_(idx, idx)]), "pdist")
    assert len(host(L.dist(fx, Y[2], "rmsd", X_indices=ix[:0]))) == 0
    assert len(host(L.pdist(fx, "rmsd", X_indices=ix[:1]))) == 0
    if where == "device":
        with pytest.raises(ValueError):
            L.dist(fx, Y[2], "rmsd", X_indices=idx)   # indices on the other side


def test_degenerate_frames(gpu):
    L = ld()
    for name, (x, y, want) in R.degenerate_frames().items():
        D, B = R.cdist(R.Frames(x), R.Frames(y))
        got = L.dist(x, y[0], "rmsd")
        within(got, D[:, 0], B[:, 0], name)
        same_bits(L.cdist(x, y, "rmsd").reshape(-1), got, name)
        same_bits(L.pdist(np.concatenate([x, y]), "rmsd"), got, name)
        if want == 'positive':
            assert got[0] > 0.1


def test_uncentred_input(gpu):
    L = ld()
    X, Y, D, B = gauss_ref(65, 7, 33, 81, offset=1e3)
    within(L.cdist(X, Y, "rmsd"), D, B, "offset 1e3, spread 1")
    check_assign(X, Y, D, B, "assign, offset 1e3")


def test_one_definition_and_two_runs(gpu):
    """dist, cdist's column, pdist's entries, assign_nearest's minimum and KCenters.distances_ carry the same bits; a second
    run repeats every bit, the inertias included."""
    from msmbuilder_amd.cluster.kcenters import _KCenters
    L = ld()
    X, D, B = self_ref(129, 33, 91)
    fx = L.RmsdFrames(X)
    cd = host(L.cdist(fx, fx, "rmsd"))
    for j in (0, 64, 128):
        col = host(L.dist(fx, X[j], "rmsd"))
        same_bits(col, cd[:, j], "dist / cdist")
    same_bits(L.pdist(fx, "rmsd"), R.condensed(cd), "pdist / cdist")
    runs = []
    for _ in range(2):
        kc = _KCenters(n_clusters=9, metric="rmsd", random_state=3).fit(X)
        sub = L.RmsdFrames(X[kc.cluster_ids_])
        labels, mind, inertia = L.rmsd_assign(fx, sub)
        runs.append((kc.cluster_ids_, host(kc.labels_), host(kc.distances_), kc.inertia_, host(labels), host(mind), inertia))
    ids, klabels, kdist, kinertia, labels, mind, inertia = runs[0]
    same_bits(kdist, cd[:, ids].min(axis=1), "KCenters.distances_ / cdist")
    same_bits(mind, kdist, "assign_nearest's minimum / KCenters.distances_")
    assert np.array_equal(klabels, labels) and kinertia == inertia
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
    # the loop itself, exactly, on the card's own distances: strict updates in centre order, first maximum
    own = R.kcenters_loop(lambda i: (cd[:, i], np.zeros(len(cd))), len(cd), 9, ids[0])
    assert own['ids'] == ids and np.array_equal(own['labels'], klabels)
    same_bits(own['distances'], kdist, "k-centers loop on the card's distances")


# ---- decisions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K,A,seed", R.DECISION_CASES)
def test_decisions_on_planted_conformations(gpu, n, K, A, seed):
    from msmbuilder_amd.cluster.kcenters import _KCenters
    frames, shapes, which = R.planted(n, K, A, seed)
    fx = R.Frames(frames)
    D, B = R.cdist(fx, R.Frames(shapes))
    decided = check_assign(frames, shapes, D, B, "planted assign")
    assert (~decided).sum() <= 0.02 * n
    assert np.array_equal(host(ld().assign_nearest(frames, shapes, "rmsd")[0])[decided], which[decided])
    # k-centers: walk the restated loop beside the library's choices
    kc = _KCenters(n_clusters=K, metric="rmsd", random_state=seed).fit(frames)
    from sklearn.utils import check_random_state
    assert kc.cluster_ids_[0] == check_random_state(seed).randint(0, n)

    def column(i):
        d, b = R.cdist(fx, R.Frames(frames[i:i + 1]))
        return d[:, 0], b[:, 0]
    ref = R.kcenters_loop(column, n, K, kc.cluster_ids_[0], follow=kc.cluster_ids_)
    running = np.full(n, np.inf)
    for k in range(K - 1):
        running = np.minimum(running, ref['D'][:, k])
        own, top, gap, bound = ref['steps'][k]
        chosen = kc.cluster_ids_[k + 1]
        if gap > 2 * bound:
            assert chosen == own, (k, chosen, own)
        else:
            assert running[chosen] >= top - 2 * bound, (k, chosen, own)   # within the bound of the maximum: a legitimate argmax
    within(kc.distances_, ref['distances'], np.nanmax(ref['B'], axis=1), "KCenters.distances_")
    _, _, _, margin = R.assign_loop(ref['D'])
    decided = margin > 2 * np.nanmax(ref['B'], axis=1)
    assert (~decided).sum() <= 0.02 * n
    assert np.array_equal(host(kc.labels_)[decided], ref['labels'][decided])
    assert len(set(which[kc.cluster_ids_].tolist())) == K


def test_exact_ties(gpu):
    from msmbuilder_amd.cluster.kcenters import _KCenters
    L = ld()
    frames, shapes, which = R.planted(120, 3, 33, 5)
    centres = np.concatenate([shapes, shapes[::-1], shapes])   # every centre three times: the lowest index wins
    assert np.array_equal(host(L.assign_nearest(frames, centres, "rmsd")[0]), which)
    many = np.concatenate([shapes[2:3]] * 40 + [shapes[:1]])    # forty copies: across the wave's two halves and a tile boundary
    lab_many = host(L.assign_nearest(frames, many, "rmsd")[0])
    assert set(lab_many[which == 2].tolist()) == {0} and set(lab_many[which == 0].tolist()) == {40}
    # duplicate frames at the k-centers argmax: the first row is chosen
    near = frames[which == 0][:30]
    assert len(near) == 30
    far = (shapes[1] * 4.0).astype(np.float32)
    X = np.concatenate([near[:7], far[None], near[7:19], far[None], near[19:]])   # the outlier at rows 7 and 20
    from sklearn.utils import check_random_state
    seed = next(s for s in range(10) if check_random_state(s).randint(0, len(X)) not in (7, 20))   # the first centre is drawn
    kc = _KCenters(n_clusters=3, metric="rmsd", random_state=seed).fit(X)
    assert kc.cluster_ids_[0] not in (7, 20) and kc.cluster_ids_[1] == 7
    d, lab = host(kc.distances_), host(kc.labels_)
    assert d[7] == d[20] and lab[7] == 1 and lab[20] == 1


def test_one_nan_frame(gpu):
    from msmbuilder_amd.cluster.kcenters import _KCenters
    L = ld()
    X, Y, D, B = gauss_ref(65, 33, 5, 71)
    X = X.copy()
    X[41, 2, 1] = np.nan
    fx = L.RmsdFrames(X)
    cd = host(L.cdist(fx, L.RmsdFrames(Y), "rmsd"))
    assert np.isnan(cd[41]).all() and np.isfinite(np.delete(cd, 41, axis=0)).all()
    labels, mind, inertia = L.rmsd_assign(fx, L.RmsdFrames(Y))
    own_labels, own_min, own_inertia, _ = R.assign_loop(cd)
    assert np.array_equal(host(labels), own_labels) and host(labels)[41] == 0
    same_bits(mind, own_min, "min_dist")
    assert host(mind)[41] == R.FLT_MAX
    assert abs(inertia - own_inertia) <= 65 * R.U64 * own_inertia and inertia >= R.FLT_MAX
    # as a centre it has NaN distances to everything: no row updates; the restated loops say the same
    Yn = Y.copy()
    Yn[0, 0, 0] = np.inf
    Dn, Bn = R.cdist(R.Frames(X), R.Frames(Yn))
    check_assign(X, Yn, Dn, Bn, "assign with NaN frame and NaN centre")
    # k-centers (kcenters.py:79-102 literally): the NaN frame keeps its +inf, is the first maximum, becomes a centre that
    # updates nothing, and is chosen again
    full = host(L.cdist(fx, fx, "rmsd"))
    kc = _KCenters(n_clusters=4, metric="rmsd", random_state=2).fit(X)
    own = R.kcenters_loop(lambda i: (full[:, i], np.zeros(65)), 65, 4, kc.cluster_ids_[0])
    assert own['ids'] == kc.cluster_ids_ and kc.cluster_ids_[0] != 41 and kc.cluster_ids_[1:] == [41, 41, 41]
    assert np.array_equal(own['labels'], host(kc.labels_))
    same_bits(own['distances'], kc.distances_, "distances_ with a NaN frame")
    assert np.isinf(host(kc.distances_)[41]) and np.isinf(kc.inertia_)


# ---- estimators ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_kcenters_on_ragged_trajectories(gpu, where):
    from msmbuilder_amd import KCenters
    L = ld()
    frames, shapes, which = R.planted(129, 5, 33, 17)
    lengths = [40, 1, 70, 18]
    cuts = np.cumsum([0] + lengths)
    trajs = [frames[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    given = trajs if where == "host" else [cuda(t) for t in trajs]
    if where == "host":
        given = [Duck(given[0])] + given[1:]   # an object with .xyz among the arrays
    kc = KCenters(n_clusters=5, metric="rmsd", random_state=4).fit(given)
    assert [len(l) for l in kc.labels_] == lengths and [len(d) for d in kc.distances_] == lengths
    labels, dist = np.concatenate([host(l) for l in kc.labels_]), np.concatenate([host(d) for d in kc.distances_])
    if where == "device":
        assert all(l.is_cuda for l in kc.labels_) and all(d.is_cuda for d in kc.distances_)
    assert isinstance(kc.cluster_centers_, np.ndarray) and kc.cluster_centers_.shape == (5, 33, 3)
    assert kc.cluster_centers_.dtype == np.float32 and np.array_equal(kc.cluster_centers_, frames[kc.cluster_ids_])
    full = host(L.cdist(frames, frames, "rmsd"))
    own = R.kcenters_loop(lambda i: (full[:, i], np.zeros(129)), 129, 5, kc.cluster_ids_[0])
    assert own['ids'] == kc.cluster_ids_ and np.array_equal(own['labels'], labels)
    same_bits(own['distances'], dist, "distances_")
    assert len(set(which[kc.cluster_ids_].tolist())) == 5
    # against the restatement on decided rows
    fx = R.Frames(frames)
    D, B = R.cdist(fx, R.Frames(frames[kc.cluster_ids_]))
    ref_labels, _, _, margin = R.assign_loop(D)
    decided = margin > 2 * B.max(axis=1)
    assert (~decided).sum() <= 0.02 * 129 and np.array_equal(labels[decided], ref_labels[decided])
    predicted = kc.predict(given)
    assert [len(p) for p in predicted] == lengths
    assert np.array_equal(np.concatenate([host(p) for p in predicted])[decided], labels[decided])
    assert np.array_equal(host(kc.partial_predict(given[2])), host(kc.labels_[2]))
    assert np.array_equal(host(kc.transform(given)[2]), host(predicted[2]))
    again = KCenters(n_clusters=5, metric="rmsd", random_state=4).fit_predict(given)
    assert all(np.array_equal(host(a), host(b)) for a, b in zip(again, kc.labels_))
    text = kc.summarize()
    assert "KCenters" in text and "rmsd" in text and ("%s" % kc.inertia_) in text
    assert abs(kc.inertia_ - dist.sum()) <= 129 * R.U64 * dist.sum()


def _kmedoids_inputs():
    frames, shapes, which = R.planted(90, 4, 5, 23)
    return frames


@pytest.mark.parametrize("where", ["host", "device"])
def test_kmedoids(gpu, where):
    from sklearn.utils import check_random_state
    from msmbuilder_amd import KMedoids
    from msmbuilder_amd.cluster.kmedoids import _KMedoids
    L = ld()
    frames = _kmedoids_inputs()
    x = frames if where == "host" else cuda(frames)
    Dm = host(L.pdist(x, "rmsd"))
    f = R.Frames(frames)
    Dr, Br = R.cdist(f, f)
    within(Dm, R.condensed(Dr), R.condensed(Br), "the matrix k-medoids runs on")
    est = _KMedoids(n_clusters=4, n_passes=3, metric="rmsd", random_state=8).fit(x)
    inits = KR.random_assignments(check_random_state(8), 90, 4, 3)
    ids, error, _, _ = KR.kmedoids(4, Dm, 3, None, inits)
    want_labels, want_ids = KR.contigify_ids(ids)
    assert np.array_equal(est.labels_, want_labels) and np.array_equal(est.cluster_ids_, want_ids) and est.inertia_ == error
    assert est.cluster_centers_.shape == (4, 5, 3) and np.array_equal(est.cluster_centers_, frames[want_ids])
    again = _KMedoids(n_clusters=4, n_passes=3, metric="rmsd", random_state=8).fit(x)
    assert np.array_equal(again.labels_, est.labels_) and np.array_equal(again.cluster_ids_, est.cluster_ids_)
    assert again.inertia_ == est.inertia_
    own_labels = R.assign_loop(host(L.cdist(x, est.cluster_centers_, "rmsd")))[0]
    assert np.array_equal(host(est.predict(x)), own_labels)
    # the list estimator: (trajectory, frame) ids
    pieces = [x[:50], x[50:]]
    lst = KMedoids(n_clusters=4, n_passes=3, metric="rmsd", random_state=8).fit(pieces)
    assert np.array_equal(np.concatenate(lst.labels_), want_labels)
    assert np.array_equal(lst.cluster_ids_, KR.split_indices([50, 40], want_ids))


@pytest.mark.parametrize("where", ["host", "device"])
def test_minibatch_kmedoids(gpu, where):
    from sklearn.utils import check_random_state
    from msmbuilder_amd.cluster.minibatchkmedoids import _MiniBatchKMedoids
    L = ld()
    frames = _kmedoids_inputs()
    x = frames if where == "host" else cuda(frames)
    fx = L.RmsdFrames(x)
    n, K, batch = 90, 4, 20
    est = _MiniBatchKMedoids(n_clusters=K, max_iter=2, batch_size=batch, metric="rmsd", random_state=6).fit(x)
    # the estimator's host logic (tests/kmedoids_ref.py: minibatch_estimator) over the card's own rmsd pdist
    rs = check_random_state(6)
    cluster_ids = rs.randint(0, n, size=K)
    labels = rs.randint(0, K, size=n)
    quiet = steps = 0
    for _ in range(int(2 * int(np.ceil(float(n) / batch)))):
        idx = np.concatenate([cluster_ids, rs.randint(0, n, batch)]).astype(np.int64)
        Dm = host(L.pdist(fx, "rmsd", X_indices=idx if where == "host" else cuda(idx)))
        start = np.concatenate([np.arange(K), labels[idx[K:]]])
        ids, _, _, _ = KR.kmedoids(K, Dm, 0, start)
        mb_labels, mb_ids = KR.contigify_ids(ids)
        steps += 1
        cluster_ids = idx[mb_ids]
        if np.sum(labels[idx] != mb_labels) == 0:
            quiet += 1
        else:
            labels[idx] = mb_labels
            quiet = 0
        if quiet >= 10:
            break
    assert est.n_steps_ == steps and np.array_equal(est.cluster_ids_, cluster_ids)
    cd = host(L.cdist(fx, frames[cluster_ids], "rmsd"))
    want_labels, want_min, want_inertia, _ = R.assign_loop(cd)
    assert np.array_equal(host(est.labels_), want_labels) and est.inertia_ == want_inertia
    assert np.array_equal(est.cluster_centers_, frames[cluster_ids])
    again = _MiniBatchKMedoids(n_clusters=K, max_iter=2, batch_size=batch, metric="rmsd", random_state=6).fit(x)
    assert np.array_equal(again.cluster_ids_, est.cluster_ids_) and np.array_equal(host(again.labels_), host(est.labels_))
    assert again.inertia_ == est.inertia_
    assert np.array_equal(host(est.predict(x)), want_labels)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_device(gpu):
    from msmbuilder_amd import KCenters, KMedoids, MiniBatchKMedoids
    L = ld()
    X5, X4 = R.gaussian_frames(6, 5, 1), R.gaussian_frames(3, 4, 2)
    msg = "Input trajectories must have same number of atoms. found 5 and 4."
    with pytest.raises(ValueError) as e:
        L.assign_nearest(X5, X4, "rmsd")
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        L.dist(X5, X4[0], "rmsd")
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        L.cdist(X5, X4, "rmsd")
    assert str(e.value) == 'XA and XB must have the same number of atoms'
    with pytest.raises(ValueError):
        L.dist(X5, X5[:2], "rmsd")   # y is one conformation
    with pytest.raises(ValueError):
        L.sumdist(X5, "rmsd", np.zeros((2, 3), dtype=np.int64))
    for bad in (np.array([0, 6]), np.array([-1])):   # an index outside the frames never reaches a kernel
        with pytest.raises(ValueError):
            L.dist(X5, X5[0], "rmsd", X_indices=bad)
        with pytest.raises(ValueError):
            L.pdist(cuda(X5), "rmsd", X_indices=cuda(np.concatenate([bad, [1]])))
        with pytest.raises(ValueError):
            L.sumdist(X5, "rmsd", np.stack([bad, bad], axis=1))
    # 2-D arrays: the vector metrics' message, unchanged; float64 and a wrong last axis: refused
    vector = 'metric must be one of %s' % ', '.join("'%s'" % s for s in L.VECTOR_METRICS)
    for est in (KCenters(n_clusters=2, metric="rmsd"), KMedoids(n_clusters=2, metric="rmsd"),
                MiniBatchKMedoids(n_clusters=2, metric="rmsd")):
        with pytest.raises(ValueError) as e:
            est.fit([X5.reshape(6, 15)])
        assert str(e.value) == vector
        with pytest.raises(ValueError):
            est.fit([cuda(X5.astype(np.float64))])
        with pytest.raises(ValueError):
            est.fit([cuda(X5[:, :, :2])])
    with pytest.raises(ValueError):
        KMedoids(n_clusters=7, metric="rmsd").fit([X5])   # more clusters than frames
    # empty inputs return as the vector paths do
    assert host(L.cdist(X5[:0], X5, "rmsd")).shape == (0, 6) and host(L.pdist(X5[:1], "rmsd")).shape == (0,)
    lab, inertia = L.assign_nearest(X5[:0], X5, "rmsd")
    assert len(lab) == 0 and inertia == 0.0 and len(L.dist(X5[:0], X5[0], "rmsd")) == 0


def test_c_abi_refusals(gpu):
    lib = gpu.lib()
    X5, X4 = R.gaussian_frames(6, 5, 1), R.gaussian_frames(3, 4, 2)
    h5, h4, h0 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert lib.msm_rmsd_prepare(C.byref(h5), X5.ctypes.data, 6, 5, 0) == gpu.MSM_OK
    assert lib.msm_rmsd_prepare(C.byref(h4), X4.ctypes.data, 3, 4, 0) == gpu.MSM_OK
    n, a, pad = C.c_int64(), C.c_int64(), C.c_int64()
    assert lib.msm_rmsd_shape(h5, C.byref(n), C.byref(a), C.byref(pad)) == gpu.MSM_OK
    assert (n.value, a.value, pad.value) == (6, 5, 64)
    for frames, atoms in ((0, 5), (6, 0), (-1, 5)):
        assert lib.msm_rmsd_prepare(C.byref(h0), X5.ctypes.data, frames, atoms, 0) == gpu.MSM_ERR_INVALID and not h0.value
    assert lib.msm_rmsd_prepare(C.byref(h0), None, 6, 5, 0) == gpu.MSM_ERR_INVALID
    out = np.zeros(64)
    lab = np.zeros(8, dtype=np.int64)
    inertia = C.c_double()
    assert lib.msm_rmsd_cdist(h5, h4, out.ctypes.data, 0) == gpu.MSM_ERR_INVALID
    assert lib.msm_rmsd_dist(h5, h4, 0, None, 0, out.ctypes.data, 0) == gpu.MSM_ERR_INVALID
    assert lib.msm_rmsd_dist(h5, h5, 6, None, 0, out.ctypes.data, 0) == gpu.MSM_ERR_INVALID
    assert lib.msm_rmsd_assign_nearest(h5, h4, None, 0, lab.ctypes.data, None, C.byref(inertia), 0) == gpu.MSM_ERR_INVALID
    bad = np.array([0, 6], dtype=np.int64)
    assert lib.msm_rmsd_dist(h5, h5, 0, bad.ctypes.data, 2, out.ctypes.data, 0) == gpu.MSM_ERR_INVALID
    assert lib.msm_rmsd_pdist(h5, bad.ctypes.data, 2, out.ctypes.data, 0) == gpu.MSM_ERR_INVALID
    assert lib.msm_rmsd_sumdist(h5, bad.ctypes.data, 1, C.byref(inertia), 0) == gpu.MSM_ERR_INVALID
    ids = np.zeros(2, dtype=np.int64)
    for K, seed in ((0, 0), (2, 6), (2, -1)):
        assert lib.msm_rmsd_kcenters_fit(h5, K, seed, ids.ctypes.data, lab.ctypes.data, out.ctypes.data, C.byref(inertia),
                                         0) == gpu.MSM_ERR_INVALID
    assert lib.msm_rmsd_cdist(None, h4, out.ctypes.data, 0) == gpu.MSM_ERR_INVALID
    assert np.all(out == 0.0)   # nothing was written
    # min_dist through the C ABI: the distances to the nearest centre, bit for bit cdist's
    mind = np.zeros(6)
    assert lib.msm_rmsd_assign_nearest(h5, h5, None, 0, lab.ctypes.data, mind.ctypes.data, C.byref(inertia), 0) == gpu.MSM_OK
    sq = np.zeros((6, 6))
    assert lib.msm_rmsd_cdist(h5, h5, sq.ctypes.data, 0) == gpu.MSM_OK
    assert np.array_equal(mind, sq.min(axis=1)) and np.array_equal(lab[:6], np.argmin(sq, axis=1))
    # the vector entry points still refuse the name
    assert lib.msm_cdist_f32(X5.ctypes.data, X5.ctypes.data, b"rmsd", 6, 6, 15, sq.ctypes.data, 0) == gpu.MSM_ERR_METRIC
    assert lib.msm_rmsd_destroy(h5) == gpu.MSM_OK and lib.msm_rmsd_destroy(h4) == gpu.MSM_OK and lib.msm_rmsd_destroy(None) == gpu.MSM_OK


def test_zz_report_largest_ratio(gpu):
    """Last in the file: what the value tests measured, for profiles/rmsd_bounds.txt."""
    print("largest |card - restatement| / bound over this file's value checks: %.4g" % _worst["ratio"])
    assert _worst["ratio"] <= 1.0
