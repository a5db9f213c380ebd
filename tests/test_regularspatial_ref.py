"""CPU tier: the reference loop of regular spatial clustering (tests/regularspatial_ref.py) checked against the
definition at its edges, against the reference's own compiled distances where oracle/_ref is built, and against the
golden file written by the reference's own regularspatial.py.  No GPU."""
import os

import numpy as np
import pytest

import regularspatial_ref as R
from oracle.libdistance_oracle import Ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regularspatial_golden.npz")


def small_input(metric, dt):
    X = R.walk(3000, 5, seed=1)
    if metric in ("hamming", "jaccard"):
        X = np.rint(X)
    return np.ascontiguousarray(X.astype(dt))


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN, allow_pickle=False)


@pytest.mark.parametrize("dn", ["f32", "f64"])
@pytest.mark.parametrize("metric", R.METRICS)
def test_loop_reproduces_the_reference_files_ids(golden, metric, dn):
    X = small_input(metric, np.float32 if dn == "f32" else np.float64)
    p = "%s_%s_" % (metric, dn)
    ids = R.ref_fit(X, float(golden[p + "d_min"]), metric)
    assert ids == golden[p + "ids"].tolist()
    assert np.array_equal(X[ids], golden[p + "centers"])
    assert len(ids) >= 6


@pytest.mark.skipif(not Ref.available(), reason="oracle/_ref (the reference's compiled headers) is not built here")
@pytest.mark.parametrize("metric", R.METRICS)
def test_loop_on_oracle_equals_loop_on_reference_distances(metric):
    ref = Ref()
    for dt in (np.float32, np.float64):
        X = small_input(metric, dt)[:1200]
        with np.errstate(all="ignore"):
            d_min = 0.7 if metric in ("hamming", "jaccard") else 0.2 * float(np.median(ref.dist(X, X[0], metric)))
        a = R.ref_fit(X, d_min, metric)
        b = R.ref_fit(X, d_min, metric, dist=ref.dist)
        assert a == b and len(a) >= 6


def test_distance_equal_to_d_min_makes_no_centre():
    X = np.array([[0.0], [2.0], [1.0], [4.0], [4.5], [6.0 + 1e-9]])
    # row 1 is at exactly 2 from row 0, row 3 at exactly 2 from ... nothing chosen but row 0 -> 4 > 2 is a centre
    assert R.ref_fit(X, 2.0, "cityblock") == [0, 3, 5]
    assert R.ref_fit(X, np.nextafter(2.0, 0.0), "cityblock") == [0, 1, 3, 5]
    L = R.lattice(600, 4)
    for d in (2.0, 3.0):
        ids = R.ref_fit(L, d, "cityblock")
        D = np.abs(L[ids][:, None, :] - L[ids][None, :, :]).sum(-1)
        assert (D[np.triu_indices(len(ids), 1)] > d).all()          # centres are pairwise FARTHER than d_min
        rest = np.setdiff1d(np.arange(len(L)), ids)
        assert (np.abs(L[rest][:, None, :] - L[ids][None, :, :]).sum(-1).min(1) <= d).all()
        assert (np.abs(L[rest][:, None, :] - L[ids][None, :, :]).sum(-1) == d).any()   # and ties do occur


def test_nan_rows():
    X = R.cloud(400, 3, seed=4)
    clean = R.ref_fit(X, 0.8)
    Y = X.copy()
    bad = [5, 77, 78, 300]
    Y[bad, 1] = np.nan
    ids = R.ref_fit(Y, 0.8)
    assert not set(ids) & set(bad)                                   # a NaN row is never a centre ...
    keep = np.setdiff1d(np.arange(400), bad)
    assert ids == [int(keep[i]) for i in R.ref_fit(Y[keep], 0.8)]    # ... and does not change what the others do
    assert len(clean) > 10
    Y = X.copy()
    Y[0, 0] = np.nan
    assert R.ref_fit(Y, 0.8) == [0]                                  # NaN in row 0: every distance is NaN
    assert R.ref_fit(Y, -1.0) == [0]


def test_negative_d_min_takes_every_row():
    X = R.cloud(50, 2, seed=2)
    X[7] = X[3]
    assert R.ref_fit(X, -1.0) == list(range(50))
    assert R.ref_fit(X, 0.0) == [i for i in range(50) if i != 7]
    assert R.ref_fit(X, np.inf) == [0] and R.ref_fit(X, 1e300) == [0]


def test_split_indices_on_ragged_lengths():
    from msmbuilder_amd.cluster.base import MultiSequenceClusterMixin
    lengths = [5, 1, 0, 7, 2]
    pos = [0, 4, 5, 6, 12, 13, 14]
    want = [(0, 0), (0, 4), (1, 0), (3, 0), (3, 6), (4, 0), (4, 1)]
    assert R.split_indices(lengths, pos).tolist() == [list(w) for w in want]
    mix = MultiSequenceClusterMixin()
    mix._seq_lengths = lengths
    assert np.array_equal(mix._split_indices(pos), R.split_indices(lengths, pos))
    assert mix._split_indices([]).shape == (0, 2)


def test_golden_ragged_pairs_are_the_loops(golden):
    seqs = R.golden_sequences()
    ids = R.ref_fit(np.concatenate(seqs), float(golden["seq_d_min"]))
    assert np.array_equal(R.split_indices([len(s) for s in seqs], ids), golden["seq_pairs"])
    assert int(golden["seq_n_clusters"]) == len(ids)
