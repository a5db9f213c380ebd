"""tests/regularspatial_ref.py -- TEST INFRASTRUCTURE: the reference loop of regular spatial clustering.

The definition, stated once (the reference's cluster/regularspatial.py:69-81): row 0 is a centre; row i > 0 is a centre
iff ``np.all(d > d_min)`` with ``d[j] = metric(X[c_j], X[i])`` over the centres chosen so far -- one
``Oracle().dist(X, X[i], metric, X_indices=ids)`` per row, the project's own C oracle of libdistance (it travels to the
GPU machine; ``Ref().dist``, the reference's compiled headers, can be passed instead where it is built).

Also the inputs the golden generator and the GPU tests share, regenerated from seeds.
"""
import functools

import numpy as np

METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "canberra", "braycurtis", "hamming", "jaccard")


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.libdistance_oracle import Oracle
    return Oracle()


def ref_fit(X, d_min, metric="euclidean", dist=None):
    """Centre ids (ascending list of ints) of the sequential loop."""
    dist = dist or _oracle().dist
    X = np.ascontiguousarray(X)
    ids = [0]
    idx = np.zeros(64, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(1, len(X)):
            d = dist(X, X[i], metric, X_indices=idx[:len(ids)])
            if np.all(d > d_min):
                if len(ids) == len(idx):
                    idx = np.concatenate([idx, np.zeros_like(idx)])
                idx[len(ids)] = i
                ids.append(i)
    return ids


def split_indices(lengths, positions):
    """(trajectory, frame) pairs of positions in the joined array, as the reference's mapping table
    (cluster/base.py:79-88) gives them."""
    out = []
    bounds = np.concatenate(([0], np.cumsum(lengths)))
    for p in positions:
        t = 0
        while not (bounds[t] <= p < bounds[t + 1]):
            t += 1
        out.append((t, p - bounds[t]))
    return np.array(out, dtype=int).reshape(-1, 2)


# ---- shared inputs ---------------------------------------------------------------------------------------------------
def cloud(n=20000, m=3, seed=0):
    """White noise: centres turn up all through the array."""
    return np.random.RandomState(seed).randn(n, m)


def walk(n=20000, m=10, seed=0):
    """A time-ordered random walk: neighbouring rows are close, so whole waves are covered together."""
    return np.cumsum(0.1 * np.random.RandomState(seed).randn(n, m), axis=0)


def lattice(n=5000, m=4, seed=0, hi=6):
    """Integer lattice: exact ties d == d_min everywhere."""
    return np.random.RandomState(seed).randint(0, hi, (n, m)).astype(np.float64)


def general_input(name, metric):
    """The 20,000-row inputs of the general cases.  hamming and jaccard only see whether coordinates are equal / zero, so
    they get the same two shapes rounded to a coarse integer grid (with zeros)."""
    X = cloud() if name == "cloud" else walk()
    if metric in ("hamming", "jaccard"):
        X = np.rint(X * (2.0 if name == "cloud" else 1.0))
    return X


# (input, metric) -> d_min values.  euclidean: calibrated with a numpy loop (K = 250, 747 on the cloud; 462, 1732 on the
# walk with the oracle's distances); the others picked with ref_fit on the CPU so that 32 <= K <= n / 4 (the tests assert it on the reference's K).
GENERAL_DMIN = {
    ("cloud", "euclidean"): (0.8, 0.5),
    ("walk", "euclidean"): (2.0, 1.0),
    ("cloud", "sqeuclidean"): (0.5,), ("walk", "sqeuclidean"): (3.0,),      # K = 343, 612
    ("cloud", "cityblock"): (1.0,), ("walk", "cityblock"): (5.0,),          # K = 391, 509
    ("cloud", "chebyshev"): (0.5,), ("walk", "chebyshev"): (1.0,),          # K = 493, 704
    ("cloud", "canberra"): (1.0,), ("walk", "canberra"): (2.0,),            # K = 388, 338
    ("cloud", "braycurtis"): (0.2,), ("walk", "braycurtis"): (0.15,),       # K = 381, 99
    ("cloud", "hamming"): (0.5,), ("walk", "hamming"): (0.75,),             # K = 114, 103
    ("cloud", "jaccard"): (0.5,), ("walk", "jaccard"): (0.75,),             # K = 124, 129
}


def golden_sequences():
    """Ragged list of the golden file: four trajectories of one walk, float64, 7 features."""
    X = walk(1500, 7, seed=3)
    cuts = (0, 401, 402, 1000, 1500)
    return [np.ascontiguousarray(X[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
