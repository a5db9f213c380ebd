"""The rmsd restatement (tests/rmsd_ref.py) against scipy and hand cases, the emulated device order against the derived
bound, the planted decision inputs against the 2 % cap, and the Python surface's refusals that need no device."""
import numpy as np
import pytest

import rmsd_ref as R

ATOMS = (1, 2, 3, 4, 5, 33, 257)


def _value_cases():
    """(name, X, Y): Gaussian conformations far apart and near pairs (1e-2 noise under a rotation and a translation)."""
    for A in ATOMS:
        yield "far_A%d" % A, R.gaussian_frames(12, A, 10 + A), R.gaussian_frames(7, A, 500 + A)
        frames, shapes, _ = R.planted(12, 5, A, 900 + A)
        yield "near_A%d" % A, frames, shapes
    yield "offset_A33", R.gaussian_frames(12, 33, 3, offset=1e3), R.gaussian_frames(7, 33, 4, offset=1e3)


VALUE_CASES = list(_value_cases())


def test_restatement_against_scipy_on_proper_rotations():
    from scipy.spatial.transform import Rotation
    for name, X, Y in VALUE_CASES:
        fx, fy = R.Frames(X), R.Frames(Y)
        if fx.A < 3:
            continue   # align_vectors needs a determined rotation
        D = R.cdist(fx, fy, with_bound=False)
        for i in range(0, fx.n, 3):
            for j in range(fy.n):
                _, rssd = Rotation.align_vectors(fx.c[i].astype(np.float64), fy.c[j].astype(np.float64))
                # both are backward-stable eigen / singular value sums of the same float64 data: a few hundred roundings of
                # the scale G_x + G_y, compared as mean squares (a distance near 0 magnifies them by its square root)
                tol = 256 * R.U64 * float(fx.G[i] + fy.G[j]) / fx.A
                assert abs(rssd ** 2 / fx.A - D[i, j] ** 2) <= tol, (name, i, j)


def test_restatement_on_hand_cases():
    for name, (x, y, want) in R.degenerate_frames().items():
        D, B = R.cdist(R.Frames(x), R.Frames(y))
        assert np.isfinite(D[0, 0]) and np.isfinite(B[0, 0]), name
        if want == 'zero':
            assert D[0, 0] <= B[0, 0], (name, D[0, 0], B[0, 0])
        else:
            assert D[0, 0] > B[0, 0] and D[0, 0] > 0.1, (name, D[0, 0], B[0, 0])
    x = R.degenerate_frames()['identical'][0]
    assert R.cdist(R.Frames(x), R.Frames(x), with_bound=False)[0, 0] == 0.0
    # a rigid motion changes nothing beyond the input rounding; a mirror image cannot be superposed
    assert R.degenerate_frames()['mirror'][2] == 'positive'


def test_nan_frame_gives_nan():
    X = R.gaussian_frames(4, 5, 1)
    X[2, 1, 0] = np.nan
    X[3, 0, 2] = np.inf
    D, B = R.cdist(R.Frames(X), R.Frames(R.gaussian_frames(3, 5, 2)))
    assert np.isnan(D[2:]).all() and np.isfinite(D[:2]).all()


def test_emulated_device_order_stays_within_the_bound():
    worst, most = 0.0, 0
    cases = VALUE_CASES + [(k, v[0], v[1]) for k, v in R.degenerate_frames().items()]
    for name, X, Y in cases:
        fx, fy = R.Frames(X), R.Frames(Y)
        D, B = R.cdist(fx, fy)
        E, its = R.device_order(fx, fy)
        most = max(most, its)
        assert np.all(np.abs(E - D) <= B), (name, np.max(np.abs(E - D) - B))
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio = np.where(B > 0, np.abs(E - D) / B, 0.0)
        worst = max(worst, float(ratio.max()))
    print("largest error / bound of the emulation: %.3g; most Newton steps: %d" % (worst, most))
    assert most <= R.NEWTON_MAX


def test_bound_terms_are_what_the_derivation_says():
    # a simple root far from the others: the chain term dominates and equals 2 gamma_A sqrt(Gx Gy)
    A, Gx, Gy = 100, 300.0, 280.0
    eig = np.array([[-250.0, -10.0, 5.0, 255.0]])
    d = np.sqrt((Gx + Gy - 2 * 255.0) / A)
    gamma = A * R.U32 / (1 - A * R.U32)
    e_lam = 2 * gamma * np.sqrt(Gx * Gy)
    got = R.pair_bound(A, np.array([Gx]), np.array([Gy]), eig, np.array([d]))[0]
    # (the fifty-step term adds (3/4)^50 * 35 = 2e-5 to e_chain = 3.5e-3: under one per cent)
    assert 2 * e_lam / A / d <= got <= 1.01 * 2 * e_lam / A / d
    # a double largest root: the floor term is a square root and the branch term adds the gap
    eig2 = np.array([[-255.0, -255.0, 255.0, 255.0]])
    got2 = R.pair_bound(A, np.array([Gx]), np.array([Gy]), eig2, np.array([d]))[0]
    assert got2 > got
    # the floor solver: e prod(e + g) = rhs
    e = R.solve_floor(np.array([1e-20, 1e-20]), np.array([[1.0, 2.0, 3.0], [0.0, 2.0, 3.0]]))
    assert abs(e[0] - 1e-20 / 6.0) <= 1e-26 and abs(e[1] - np.sqrt(1e-20 / 6.0)) <= 1e-14


@pytest.mark.parametrize("n,K,A,seed", R.DECISION_CASES)
def test_planted_inputs_stay_within_the_cap(n, K, A, seed):
    """The decision tests leave out rows whose margin is at most twice the bound: no more than 2 % of them."""
    frames, shapes, which = R.planted(n, K, A, seed)
    fx = R.Frames(frames)
    D, B = R.cdist(fx, R.Frames(shapes))
    labels, mind, inertia, margin = R.assign_loop(D)
    left_out = np.sum(~(margin > 2 * B.max(axis=1)))
    assert left_out <= 0.02 * n, (left_out, n)
    assert np.array_equal(labels, which)   # the planted conformation is the nearest centre
    # k-centers on the same frames: rows whose label is not decided
    def column(i):
        d, b = R.cdist(fx, R.Frames(frames[i:i + 1]))
        return d[:, 0], b[:, 0]
    kc = R.kcenters_loop(column, n, K, seed % n)
    _, _, _, kmargin = R.assign_loop(kc['D'])
    left_out = np.sum(~(kmargin > 2 * kc['B'].max(axis=1)))
    assert left_out <= 0.02 * n, (left_out, n)
    assert len(set(which[kc['ids']].tolist())) == K   # farthest-point picks one frame of every conformation


def test_loops_follow_the_reference_rules():
    D = np.array([[1.0, 1.0, 0.5], [np.nan, 2.0, 2.0], [np.nan, np.nan, np.nan], [3.0, np.nan, 1.0]])
    labels, mind, inertia, margin = R.assign_loop(D)
    assert labels.tolist() == [2, 1, 0, 2] and mind.tolist() == [0.5, 2.0, R.FLT_MAX, 1.0]
    assert inertia == float(np.add.accumulate(mind)[-1]) and margin.tolist() == [0.5, 0.0, 0.0, 2.0]
    # k-centers on points of a line: strict updates, first maximum
    pts = np.array([0.0, 4.0, 1.0, 4.0, 2.0])
    kc = R.kcenters_loop(lambda i: (np.abs(pts - pts[i]), np.zeros(5)), 5, 3, 0)
    assert kc['ids'] == [0, 1, 4] and kc['labels'].tolist() == [0, 1, 0, 1, 2]


# ---- the Python surface, without a device ---------------------------------------------------------------------------------
def _vector_message():
    from msmbuilder_amd import libdistance
    return 'metric must be one of %s' % ', '.join("'%s'" % s for s in libdistance.VECTOR_METRICS)


def test_vector_metrics_unchanged():
    from msmbuilder_amd import libdistance
    assert libdistance.VECTOR_METRICS == ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "canberra", "braycurtis",
                                          "hamming", "jaccard", "cityblock")
    assert 'RmsdFrames' in libdistance.__all__


def test_rmsd_on_2d_arrays_raises_the_same_message():
    from msmbuilder_amd import KCenters, KMedoids, MiniBatchKMedoids, libdistance
    X = np.zeros((6, 3), dtype=np.float32)
    calls = [lambda: libdistance.assign_nearest(X, X[:2], "rmsd"), lambda: libdistance.cdist(X, X, "rmsd"),
             lambda: libdistance.dist(X, X[0], "rmsd"), lambda: libdistance.pdist(X, "rmsd"),
             lambda: libdistance.sumdist(X, "rmsd", np.zeros((1, 2), dtype=np.int64)),
             lambda: libdistance.dist(X, X[0], b"rmsd"),
             lambda: KCenters(n_clusters=2, metric="rmsd").fit([X]),
             lambda: KMedoids(n_clusters=2, metric="rmsd").fit([X]),
             lambda: MiniBatchKMedoids(n_clusters=2, metric="rmsd").fit([X])]
    for call in calls:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == _vector_message()


class _Duck(object):
    def __init__(self, xyz):
        self.xyz = xyz


@pytest.mark.parametrize("bad", [np.zeros((4, 5, 3), dtype=np.float64), np.zeros((4, 5, 3), dtype=np.int32),
                                 np.zeros((4, 5, 2), dtype=np.float32), np.zeros((4, 3, 5), dtype=np.float32).transpose(0, 2, 1)],
                         ids=["float64", "int32", "last_axis_2", "not_contiguous"])
def test_refused_conformations(bad):
    from msmbuilder_amd import KCenters, KMedoids, MiniBatchKMedoids, libdistance
    before = bad.copy()
    pairs = np.zeros((1, 2), dtype=np.int64)
    calls = [lambda x: libdistance.RmsdFrames(x), lambda x: libdistance.assign_nearest(x, x, "rmsd"),
             lambda x: libdistance.cdist(x, x, "rmsd"), lambda x: libdistance.dist(x, x, "rmsd"),
             lambda x: libdistance.pdist(x, "rmsd"), lambda x: libdistance.sumdist(x, "rmsd", pairs),
             lambda x: KCenters(n_clusters=2, metric="rmsd").fit([x]),
             lambda x: KMedoids(n_clusters=2, metric="rmsd").fit([x]),
             lambda x: MiniBatchKMedoids(n_clusters=2, metric="rmsd").fit([x])]
    if not bad.flags.c_contiguous:
        calls = calls[:6]   # the list adaptor joins trajectories into one contiguous array, as it does for 2-D ones
    for call in calls:
        for x in (bad, _Duck(bad)):
            with pytest.raises(ValueError):
                call(x)
    assert np.array_equal(bad, before)


def test_estimators_that_still_refuse_rmsd():
    from msmbuilder_amd import KCenters, LandmarkAgglomerative, RegularSpatial
    X3 = np.zeros((8, 5, 3), dtype=np.float32)
    X2 = np.zeros((8, 3), dtype=np.float32)
    for X in (X3, X2):
        with pytest.raises(ValueError):
            RegularSpatial(d_min=1.0, metric="rmsd").fit([X])
        with pytest.raises(ValueError):
            LandmarkAgglomerative(n_clusters=2, metric="rmsd").fit([X])
    # the sharded k-centers loop does not take conformations

    class Sharded(KCenters):
        _force_sharded = True
    with pytest.raises(NotImplementedError):
        Sharded(n_clusters=2, metric="rmsd").fit([X3])
