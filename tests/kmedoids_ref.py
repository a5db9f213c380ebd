"""tests/kmedoids_ref.py -- TEST INFRASTRUCTURE: the reference loop of k-medoids clustering in numpy.

Written from the description of the algorithm (cluster/src/kmedoids.cc of the reference, reached through
_kmedoids.pyx), not from its text:

One pass on a condensed matrix D of n elements (entry (i, j), i < j, at ``n*i - i(i+1)/2 + j - 1 - i``), from an
assignment t with values in [0, K): total = DBL_MAX, counter = 0, period = 10; repeat { previous = total; if
counter % period == 0: saved = t, period *= 2; counter += 1; MEDOIDS: element i's cost is the float64 sum, in ascending
k, of D(i, k) over the k != i with t[k] == t[i], and cluster j's medoid is its lowest-index member of strictly lowest
cost; ASSIGN: a medoid of cluster c gets label c and distance 0, every other element the first c, in cluster order,
at the strict minimum of D(i, medoid[c]); TOTAL: the float64 sum of those distances in ascending i; stop when
total >= previous or t == saved }.

Every ordered sum is ``np.add.accumulate`` (sequential by definition) over ``where(same, D, 0.0)`` -- never ``np.sum``,
which adds pairwise; adding +0.0 for non-members leaves every partial sum's bits alone.

Also here: the replay of the random initial assignments on a ``RandomState``, both estimators' host logic over
``oracle.libdistance_oracle.Oracle().pdist`` (the project's own C oracle of libdistance; it travels to the GPU machine),
and the inputs the golden generator and the tests share, regenerated from seeds.
"""
import functools

import numpy as np

DBL_MAX = np.finfo(np.float64).max
METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "canberra", "braycurtis", "hamming", "jaccard")


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.libdistance_oracle import Oracle
    return Oracle()


def condensed_index(i, j, n):
    """Python integers: no width to overflow."""
    i, j = (int(i), int(j)) if i < j else (int(j), int(i))
    return n * i - i * (i + 1) // 2 + j - 1 - i


def squareform(D, n):
    """The symmetric n x n matrix of a condensed one, zeros (+0.0) on the diagonal."""
    S = np.zeros((n, n), dtype=np.float64)
    iu = np.triu_indices(n, 1)
    S[iu] = np.asarray(D, dtype=np.float64)
    S.T[iu] = S[iu]
    return S


def one_pass(S, K, t):
    """One pass on the square matrix S from the assignment t (not modified).
    Returns (t, medoids, total, iterations, snapshots)."""
    n = len(S)
    t = np.array(t, dtype=np.intp)
    total, counter, period, snapshots = DBL_MAX, 0, 10, 0
    saved = None
    rows = np.arange(n)
    while True:
        previous = total
        if counter % period == 0:
            saved = t.copy()
            period *= 2
            snapshots += 1
        counter += 1
        same = t[:, None] == t[None, :]
        cost = np.add.accumulate(np.where(same, S, 0.0), axis=1)[:, -1]   # (the diagonal of S is +0.0)
        med = np.empty(K, dtype=np.intp)
        for c in range(K):
            members = np.flatnonzero(t == c)
            assert len(members), "cluster %d is empty: the reference reads an unset medoid here" % c
            assert np.all(cost[members] < DBL_MAX), "the loop is only defined for finite sums"
            med[c] = members[np.argmin(cost[members])]   # first occurrence of the minimum = strictly below every earlier one
        M = S[:, med]
        assert np.all(M < DBL_MAX)
        t = np.argmin(M, axis=1).astype(np.intp)   # first cluster at the strict minimum
        dist = M[rows, t]
        t[med] = np.arange(K)     # a medoid keeps its own cluster whatever lies at distance 0 from it ...
        dist[med] = 0.0           # ... at distance 0
        total = np.add.accumulate(dist)[-1]
        if total >= previous or np.array_equal(t, saved):
            return t, med, total, counter, snapshots


def kmedoids(K, D, npass, clusterid=None, inits=None):
    """The reference's kmedoids(K, D, npass, clusterid) with the random assignments handed in (``inits``: npass x n).
    Returns (clusterid, error, ifound, info) -- info: iterations and snapshots of the last pass."""
    D = np.asarray(D, dtype=np.float64)
    n = int(1 + np.sqrt(8 * len(D) + 1) / 2.0)
    assert len(D) == n * (n - 1) // 2 and 1 <= K <= n and npass >= 0
    S = squareform(D, n)
    clusterid = np.zeros(n, dtype=np.intp) if clusterid is None else np.array(clusterid, dtype=np.intp)
    error, ifound = DBL_MAX, -1
    info = {}
    for p in range(max(npass, 1)):
        start = clusterid if npass == 0 else np.asarray(inits[p], dtype=np.intp)
        t, med, total, iters, snaps = one_pass(S, K, start)
        if npass <= 1:
            clusterid = t   # the pass works in place on clusterid: labels are compared with medoid ids below
        new = med[t]
        if not np.array_equal(new, clusterid):
            if total < error:
                clusterid, error, ifound = new.copy(), total, 1
        else:
            ifound += 1
        info = dict(iterations=iters, snapshots=snaps, distinct=len(set(med.tolist())))
    return clusterid, error, ifound, info


def random_assignments(random_state, n, K, npass):
    """The draws the reference makes from C on the caller's RandomState, per pass: sizes by binomial with one element
    reserved per cluster, then a shuffle of the intp array."""
    out = np.empty((npass, n), dtype=np.intp)
    for p in range(npass):
        n_free, k = n - K, 0
        for i in range(K - 1):
            j = int(random_state.binomial(float(n_free), 1.0 / (K - i)))
            n_free -= j
            out[p, k:k + j + 1] = i
            k += j + 1
        out[p, k:] = K - 1
        random_state.shuffle(out[p])
    return out


def contigify_ids(ids):
    """(labels, medoid ids in order of first appearance)."""
    mapping = {}
    labels = np.empty(len(ids), dtype=np.intp)
    for i, v in enumerate(ids):
        labels[i] = mapping.setdefault(int(v), len(mapping))
    return labels, np.array(sorted(mapping, key=mapping.get), dtype=np.intp)


def working(X):
    X = np.asarray(X)
    return X if X.dtype in (np.float32, np.float64) else X.astype(np.float64)


def kmedoids_estimator(X, n_clusters=8, n_passes=1, metric="euclidean", random_state=None):
    """_KMedoids.fit's host logic: dict(labels, cluster_ids, centers, inertia, info)."""
    from sklearn.utils import check_random_state
    X = np.ascontiguousarray(working(X))
    D = _oracle().pdist(X, metric)
    inits = random_assignments(check_random_state(random_state), len(X), n_clusters, n_passes)
    ids, error, ifound, info = kmedoids(n_clusters, D, n_passes, None, inits)
    labels, cluster_ids = contigify_ids(ids)
    return dict(labels=labels, cluster_ids=cluster_ids, centers=X[cluster_ids], inertia=error, info=info)


def minibatch_estimator(X, n_clusters=8, max_iter=5, batch_size=100, metric="euclidean", max_no_improvement=10,
                        random_state=None):
    """_MiniBatchKMedoids.fit's host logic: dict(labels, cluster_ids, centers, inertia, steps)."""
    from sklearn.utils import check_random_state
    X = np.ascontiguousarray(working(X))
    o = _oracle()
    n = len(X)
    n_iter = int(max_iter * int(np.ceil(float(n) / batch_size)))
    rs = check_random_state(random_state)
    cluster_ids = rs.randint(0, n, size=n_clusters)
    labels = rs.randint(0, n_clusters, size=n)
    quiet = steps = 0
    for _ in range(n_iter):
        idx = np.concatenate([cluster_ids, rs.randint(0, n, batch_size)]).astype(np.int64)
        D = o.pdist(X, metric, X_indices=idx)
        start = np.concatenate([np.arange(n_clusters), labels[idx[n_clusters:]]])
        ids, _, _, _ = kmedoids(n_clusters, D, 0, start)
        mb_labels, mb_ids = contigify_ids(ids)
        steps += 1
        cluster_ids = idx[mb_ids]
        if np.sum(labels[idx] != mb_labels) == 0:
            quiet += 1
        else:
            labels[idx] = mb_labels
            quiet = 0
        if quiet >= max_no_improvement:
            break
    centers = X[cluster_ids]
    lab, inertia = o.assign_nearest(X, centers, metric)
    return dict(labels=lab, cluster_ids=cluster_ids, centers=centers, inertia=inertia, steps=steps)


def split_indices(lengths, positions):
    """(trajectory, frame) pairs of positions in the joined array."""
    bounds = np.concatenate(([0], np.cumsum(lengths)))
    out = []
    for p in positions:
        t = int(np.searchsorted(bounds, p, side="right") - 1)
        out.append((t, p - bounds[t]))
    return np.array(out, dtype=int).reshape(-1, 2)


# ---- shared inputs, from seeds ---------------------------------------------------------------------------------------
def cloud(n, m, seed, dtype=np.float64, metric="euclidean"):
    """Rows around a few hubs; rounded to integers for the two metrics that compare for equality (many exact ties)."""
    rs = np.random.RandomState(seed)
    hubs = rs.randn(6, m) * 3.0
    X = hubs[rs.randint(0, 6, n)] + rs.randn(n, m)
    if metric in ("hamming", "jaccard"):
        X = np.rint(X)
    return np.ascontiguousarray(X.astype(dtype))


def walk1d(n, seed):
    """A 1-D random walk: the k-medoids loop moves its boundaries slowly along it and runs for tens of iterations."""
    return np.ascontiguousarray(np.random.RandomState(seed).randn(n, 1).cumsum(0))


def golden_sequences(dtype=np.float32):
    rs = np.random.RandomState(7)
    return [np.ascontiguousarray((rs.randn(n, 3).cumsum(0) * 0.3).astype(dtype)) for n in (61, 5, 130, 44)]


# (name, n, m, seed, K, n_passes or mini-batch settings): the cases of tests/golden/kmedoids_golden.npz
GOLDEN_KMEDOIDS = [(metric, dn, 90 + 7 * i, 4, 20 + i, 2 + i % 5, 1 + i % 3)
                   for i, (metric, dn) in enumerate((m, d) for m in METRICS for d in ("f32", "f64"))]
GOLDEN_MINIBATCH = [("euclidean", "f32", 400, 3, 31, dict(n_clusters=6, max_iter=3, batch_size=50, max_no_improvement=4)),
                    ("cityblock", "f64", 300, 5, 32, dict(n_clusters=8, max_iter=5, batch_size=100, max_no_improvement=10)),
                    ("hamming", "f64", 250, 6, 33, dict(n_clusters=4, max_iter=2, batch_size=300, max_no_improvement=3))]
# raw loop cases: (n, K, npass, seed, metric)
GOLDEN_LOOP = [(n, K, npass, 40 + i, metric)
               for i, (n, K, npass, metric) in enumerate([(5, 1, 0, "euclidean"), (5, 5, 0, "euclidean"), (17, 3, 1, "hamming"),
                                                          (40, 7, 3, "hamming"), (64, 12, 2, "euclidean"), (120, 9, 3, "euclidean"),
                                                          (33, 2, 0, "hamming"), (2, 2, 1, "euclidean"), (2, 1, 1, "euclidean")])]
DT = {"f32": np.float32, "f64": np.float64}


def loop_case(n, K, npass, seed, metric):
    """(condensed matrix, npass==0 start or None, RandomState to draw from): inputs of one raw-loop golden case."""
    X = cloud(n, 4, seed, np.float64, metric)
    D = _oracle().pdist(X, metric)
    rs = np.random.RandomState(seed)
    start = None
    if npass == 0:
        start = np.concatenate([np.arange(K), rs.randint(0, K, n - K)]).astype(np.intp)   # no cluster empty
        rs.shuffle(start)
    return D, start, rs
