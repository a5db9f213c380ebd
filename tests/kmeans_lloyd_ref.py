"""Reference Lloyd loop for KMeans (plain numpy, float64; shares nothing with the product) and the seeded inputs of the
KMeans tests.

The loop is scikit-learn 1.7's ``_kmeans_single_lloyd`` with the rules the device follows:

    labels    exact nearest centre, lowest index among equals (``kmeans_label_ref.exact_argmin``)
    update    centre = float64 mean of the members, rounded once to the rows' type; a cluster without members keeps its centre
    empty     the n_empty rows farthest from their own OLD centre (squared distance, float64), lowest row first among equals,
              leave their clusters and become the empty clusters, in ascending cluster order
    stop      labels equal to the previous iteration's -> "strict"; else sum ||c_new - c_old||^2 <= tol_abs -> "tol";
              else after max_iter iterations -> "maxiter".  Unless strict, the rows are labelled once more.

At every iteration the loop counts the rows that ``kmeans_label_ref``'s rule cannot decide (best and second best no further
apart than their two bounds at the rows' unit roundoff).  While that count is 0 the label kernels have no choice, and since
an iteration's centres are a function of its labels alone, no error carries from one iteration to the next.
"""
import numpy as np

import kmeans_label_ref as R

STRICT, TOL, MAXITER = "strict", "tol", "maxiter"
STATUS_OF = {0: MAXITER, 1: STRICT, 2: TOL}    # msm_lloyd_run's *status


def _undecided(X, C, ref, dref, sec, dsec, u):
    if C.shape[0] < 2:
        return 0
    rows = np.arange(X.shape[0])
    return int(np.sum(dsec - dref <= R.pair_bound(X, C, rows, ref, u) + R.pair_bound(X, C, rows, sec, u)))


def relocate(X64, labels, dref, sums, counts):
    """In place on (sums, counts): scikit-learn's _relocate_empty_clusters_dense with the lowest-row tie rule."""
    empty = np.nonzero(counts == 0)[0]
    if len(empty) == 0:
        return []
    order = np.lexsort((np.arange(len(dref)), -dref))[:len(empty)]    # farthest first, lowest row among equals
    for row, new in zip(order, empty):
        old = labels[row]
        sums[old] -= X64[row]
        counts[old] -= 1
        sums[new] = X64[row]
        counts[new] = 1
    return list(order)


def lloyd(X, init, max_iter=300, tol_abs=0.0, u=None, count_undecided=True, argmin=None, trace=False):
    """Returns dict(centers (rows' type), labels, n_iter, status, undecided (per labelling pass), counts (last update),
    relocated (rows per iteration), summed (the cluster each row was summed into by the last update), taken (rows, donors:
    the rows the last update took out of a cluster's sum again, and the clusters they left), trace (the labels of every
    iteration, before relocation, when asked for)).
    ``count_undecided=False`` leaves the count out (the GPU tests: the host test has established it).  ``argmin``: a
    stand-in for ``exact_argmin`` (``clear_argmin`` for the 2M-row input, shown equal to it by the host test)."""
    argmin = R.exact_argmin if argmin is None else argmin
    dtype = X.dtype
    u = R.unit_roundoff(dtype) if u is None else u
    X64 = X.astype(np.float64)
    C = np.array(init, dtype=dtype, copy=True)
    K = C.shape[0]
    prev = np.full(X.shape[0], -1, dtype=np.int64)
    undecided, relocated, history = [], [], []
    status, n_iter, counts, summed, taken = MAXITER, 0, None, None, None
    labels = prev
    for it in range(max_iter):
        labels, dref, sec, dsec = argmin(X, C)
        if count_undecided:
            undecided.append(_undecided(X, C, labels, dref, sec, dsec, u))
        if trace:
            history.append(labels.astype(np.int32))
        counts = np.bincount(labels, minlength=K).astype(np.int64)
        sums = np.stack([np.bincount(labels, weights=X64[:, f], minlength=K) for f in range(X.shape[1])], axis=1)
        relocated.append(relocate(X64, labels, dref, sums, counts))
        summed = labels.copy()                       # membership as the update summed it: relocated rows in their new clusters
        summed[relocated[-1]] = np.nonzero(np.bincount(labels, minlength=K) == 0)[0][:len(relocated[-1])]
        taken = (np.array(relocated[-1], dtype=np.int64), labels[relocated[-1]].astype(np.int64))
        Cn = C.copy()
        live = counts > 0
        Cn[live] = (sums[live] / counts[live, None]).astype(dtype)
        shift = float(((Cn.astype(np.float64) - C.astype(np.float64)) ** 2).sum())
        C = Cn
        n_iter = it + 1
        if np.array_equal(labels, prev):
            status = STRICT
            break
        if shift <= tol_abs:
            status = TOL
            break
        prev = labels
    if status != STRICT:
        labels, dref, sec, dsec = argmin(X, C)
        if count_undecided:
            undecided.append(_undecided(X, C, labels, dref, sec, dsec, u))
    return dict(centers=C, labels=labels.astype(np.int32), n_iter=n_iter, status=status, undecided=undecided, counts=counts,
                relocated=relocated, summed=summed, taken=taken, trace=history)


def clear_argmin(X, C):
    """``exact_argmin`` for inputs whose rows are far from a tie, at a fraction of its cost on millions of rows: the best
    centre by the float64 GEMM form, accepted where the runner-up's score lies 1e-9 (||x||^2 + max ||c||^2) above it (the
    form is good to ~m 2^-52 of that, so the exact best is then the same centre); the other rows go through
    ``exact_argmin``.  The distance is recomputed by direct difference.  No second best is returned (None)."""
    n = X.shape[0]
    C64 = C.astype(np.float64)
    cn = (C64 * C64).sum(axis=1)
    ref = np.empty(n, dtype=np.int64)
    dref = np.empty(n)
    step = max(1, (1 << 23) // C.shape[0])
    for a in range(0, n, step):
        Xb = X[a:a + step].astype(np.float64)
        r = np.arange(Xb.shape[0])
        g = Xb @ C64.T
        g *= -2.0
        g += cn[None, :]
        j1 = g.argmin(axis=1)
        g1 = g[r, j1]
        g[r, j1] = np.inf
        unclear = ~(g.min(axis=1) - g1 > 1e-9 * ((Xb * Xb).sum(axis=1) + cn.max()))
        if unclear.any():
            j1[unclear] = R.exact_argmin(X[a:a + step][unclear], C)[0]
        diff = Xb - C64[j1]
        ref[a:a + step] = j1
        dref[a:a + step] = (diff * diff).sum(axis=1)
    return ref, dref, None, None


def center_bound(X, labels, c_ref, taken=None):
    """|c - c_ref| allowed per cluster: n_j 2^-53 max|x_member| for a float64 sum in another order, one rounding to the
    rows' type (half an ulp: 2^-24 / 2^-53 relative).

    ``taken`` = (rows, donors), from the reference's own relocation (``lloyd``'s "taken"): rows that the update summed
    into cluster donors[q] and then subtracted again.  The device's sum for a donor has those terms in it, so a donor is
    allowed (n_j + t_j) 2^-53 max|x| over its members AND the t_j rows taken out, plus the same one rounding.  A donor left
    without members (n_j = 0) keeps its centre and gets no such room: its sum is never divided.  Sums of small integers
    are exact whatever this bound says: the integer cases are held to an error of 0 by their tests."""
    u_t = 2.0 ** -53 if X.dtype == np.float64 else 2.0 ** -24
    K = c_ref.shape[0]
    out = np.empty_like(c_ref, dtype=np.float64)
    ax = np.abs(X).max(axis=1).astype(np.float64)
    rows, donors = (np.zeros(0, dtype=np.int64),) * 2 if taken is None else taken
    for j in range(K):
        mem = labels == j
        nj = int(mem.sum())
        out_j = rows[donors == j]
        big = max(ax[mem].max() if nj else 0.0, ax[out_j].max() if len(out_j) and nj else 0.0)
        out[j] = (nj + (len(out_j) if nj else 0)) * 2.0 ** -53 * big + u_t * np.abs(c_ref[j].astype(np.float64))
    return out


def kernel_inertia(X, C, labels):
    """The inertia kernel's arithmetic restated: difference in the rows' type, square and sum in float64."""
    d = (X - C[labels]).astype(X.dtype)
    return float((d.astype(np.float64) ** 2).sum())


# ---------------------------------------------------------------------------------------------------------------------
# seeded inputs (shared by the GPU tests and the host test that every one of them is decidable at every iteration)
# ---------------------------------------------------------------------------------------------------------------------
def blobs(n, m, K, dtype, seed, spread=0.05, sizes=None):
    """K blobs (centres 10 * randn, members spread * randn around them) in shuffled row order, and an init near one member
    row of each blob.  ``sizes``: members per blob (else near-equal)."""
    rs = np.random.RandomState(seed)
    true = rs.randn(K, m) * 10.0
    if sizes is None:
        sizes = np.full(K, n // K)
        sizes[:n - sizes.sum()] += 1
    sizes = np.asarray(sizes)
    assert sizes.sum() == n and len(sizes) == K
    which = np.repeat(np.arange(K), sizes)
    X = true[which] + spread * rs.randn(n, m)
    perm = rs.permutation(n)
    X, which = X[perm], which[perm]
    first = np.array([np.nonzero(which == j)[0][0] for j in range(K)])
    init = X[first] + 0.3 * spread * rs.randn(K, m)
    return np.ascontiguousarray(X.astype(dtype)), np.ascontiguousarray(init.astype(dtype))


def drift(n, m, K, dtype, seed):
    """Overlapping data from a poor init: many iterations before the labels settle (for the tol and max_iter rules)."""
    rs = np.random.RandomState(seed)
    X = rs.randn(n, m)
    init = X[rs.choice(n, K, replace=False)] * 0.1
    return np.ascontiguousarray(X.astype(dtype)), np.ascontiguousarray(init.astype(dtype))


def far_init(X, init, which):
    """``init`` with the centres ``which`` moved where no row is nearest: those clusters come out empty."""
    init = init.copy()
    for q, j in enumerate(which):
        init[j] = 1000.0 + 10.0 * q
    return init


def tie_case(dtype):
    """Small integers (every sum exact): two blobs and a centre no row is nearest to.  Rows 3 and 11 are the same point,
    the farthest from its centre: row 3 must be the one that moves."""
    rs = np.random.RandomState(5)
    A = rs.randint(-2, 3, (20, 3)).astype(np.float64)
    B = rs.randint(-2, 3, (20, 3)).astype(np.float64) + 40.0
    far = np.array([9.0, 9.0, -9.0])
    A[3] = far
    A[11] = far
    X = np.concatenate([A, B]).astype(dtype)
    init = np.array([[0, 0, 0], [40, 40, 40], [500, 500, 500]], dtype=dtype)
    return np.ascontiguousarray(X), init


def clumps(seed, dtype, n=300, m=2, K=40):
    """Six clumps of mixed width (members 0.05 or 1.0 wide) and an init of K perturbed member rows: many more centres
    than clumps, so that clusters run empty some iterations INTO the run.  Which iteration depends on the seed: the seeds
    in use and the iterations at which the reference relocates are listed in ``LATE`` (found by search, asserted by the
    host test)."""
    rs = np.random.RandomState(seed)
    clump = 5 * rs.randn(6, m)
    X = clump[rs.randint(0, 6, n)] + rs.randn(n, m) * rs.choice([0.05, 1.0], n)[:, None]
    init = X[rs.choice(n, K, replace=False)] + 0.01 * rs.randn(K, m)
    return np.ascontiguousarray(X.astype(dtype)), np.ascontiguousarray(init.astype(dtype))


def two_from_one_donor_case(dtype):
    """``tie_case``'s blobs with rows 3 and 11 at two different points equally far from centre 0, and TWO centres no row is
    nearest to: both rows leave cluster 0 in the same update (small integers: every sum exact)."""
    X, _ = tie_case(dtype)
    X[3] = [9, 9, -9]
    X[11] = [9, -9, 9]
    init = np.array([[0, 0, 0], [40, 40, 40], [500, 500, 500], [600, 600, 600]], dtype=dtype)
    return np.ascontiguousarray(X), init


def singleton_donor_case(dtype):
    """Small integers: 30 rows in [-3, 3]^2 and the row [100, 0], which is the only member of cluster 1 (centre [90, 0])
    and the farthest row from its centre, so it is the one that moves to the empty cluster 2.  Cluster 1 is left without
    members, keeps [90, 0], is empty again one iteration later and receives a second row."""
    rs = np.random.RandomState(SINGLETON_SEED)
    X = np.concatenate([rs.randint(-3, 4, (30, 2)).astype(np.float64), [[100.0, 0.0]]]).astype(dtype)
    init = np.array([[0, 0], [90, 0], [500, 500]], dtype=dtype)
    return np.ascontiguousarray(X), init


SINGLETON_SEED = 7    # (found by search: the second row to move is row 18, 7 iterations, final sizes [15, 15, 1])

# name -> (dtype, seed of ``clumps``, max_iter, the iterations at which the reference relocates).  max_iter = 60 is
# never reached; the "last" cases stop the run with the relocating iteration.
LATE = {
    "late_odd_f64": (np.float64, 53, 60, [1]),           # two rows move
    "late_even_f64": (np.float64, 31, 60, [2]),
    "late_odd_f32": (np.float32, 375, 60, [1]),
    "late_even_f32": (np.float32, 994, 60, [2]),
    "late_twice_01_f64": (np.float64, 277, 60, [0, 1]),
    "late_twice_02_f64": (np.float64, 1381, 60, [0, 2]),
    "late_last_even_f64": (np.float64, 31, 3, [2]),
    "late_last_odd_f32": (np.float32, 375, 2, [1]),
}

# name -> the rows the reference relocates per iteration, n_iter, status, sizes after the last update: asserted in full by
# the host test
DONOR = {
    "donor_two_f64": ([[3, 11], []], 2, TOL, [18, 20, 1, 1]),
    "donor_two_f32": ([[3, 11], []], 2, TOL, [18, 20, 1, 1]),
    "donor_single_f64": ([[30], [18], [], [], [], [], []], 7, STRICT, [15, 15, 1]),
    "donor_single_f32": ([[30], [18], [], [], [], [], []], 7, STRICT, [15, 15, 1]),
    # the same run cut after its first update: the emptied donor's kept centre is part of the result (a later iteration
    # would overwrite it with the row the cluster receives)
    "donor_single_cut_f64": ([[30]], 1, MAXITER, [30, 0, 1]),
    "donor_single_cut_f32": ([[30]], 1, MAXITER, [30, 0, 1]),
}

# far_init cases: name -> rows relocated at iteration 0 (and at no later iteration)
RELOC_AT_0 = {"reloc_one": 1, "reloc_three": 3, "reloc_one_f32": 1, "reloc_tie_f64": 1, "reloc_tie_f32": 1,
              "reloc_K2049_f32": 3, "reloc_K300_f32": 4, "reloc_K300_first_f32": 2}
RELOC_TARGETS = {"reloc_K2049_f32": [0, 2047, 2048], "reloc_K300_f32": [0, 255, 256, 299], "reloc_K300_first_f32": [5, 255]}

# K > LH_KCH = 2048 cases: the reference runs at least 3 iterations and labels change on both sides of cluster 2048 after
# the first one (asserted by the host test)
LABEL_CHUNK = ("K2048_f32", "K2049_f32", "K4097_f64")

# inputs of the unaligned-rows test (also run aligned, as trajectory cases)
UNALIGNED = ("offset_f32_m4", "offset_f32_m512", "offset_f64_m2")


def golden_inputs(name):
    """Inputs of tests/golden/kmeans_golden.npz, regenerated from seeds: (X float64, kwargs of KMeans)."""
    if name == "array":
        X, init = drift(2000, 5, 6, np.float64, 11)
        return X, dict(n_clusters=6, init=init, n_init=1, tol=1e-4, max_iter=300)
    if name == "random":
        X, _ = blobs(1500, 4, 5, np.float64, 12, spread=2.0)
        return X, dict(n_clusters=5, init="random", n_init=1, tol=1e-4, max_iter=300, random_state=7)
    raise KeyError(name)


GOLDEN_NAMES = ("array", "random")


def default_init_inputs(name):
    """The golden inputs with the estimator's default init (k-means++): (X float64, kwargs of KMeans)."""
    X, kw = golden_inputs(name)
    return X, dict(n_clusters=kw["n_clusters"], n_init=1, random_state=3)


def trajectory_cases(plan):
    """name -> (X, init, max_iter, tol_abs) of every reference-compared GPU case.  ``plan(n, m, K, dtype)``: the update's
    launch plan (msm_lloyd_plan), from which the seam sizes are taken.

    Seams held: piece length, rows per histogram wave, feature tiles, K = 1 and K around 128 (label kernel tiles), the stop
    rules, empty clusters at iteration 0 (``reloc_*``); the label chunk of the histogram and scatter waves (K = 2048, 2049,
    4097, empty clusters in both chunks); the base kernel's chunk of 256 clusters (K = 255 / 256 / 257, empties on both
    sides of cluster 256); the relocating iteration's parity, two relocations in one run and a relocation in the last
    permitted iteration (``late_*``); a donor that loses two rows and one that loses its only row (``donor_*``);
    ``offset_*`` are the inputs that tests/test_gpu_kmeans_lloyd.py runs again from rows that are not 16-byte aligned.
    Not held: K > 4097, more than one relocation AFTER iteration 0 in one run, relocation with several feature tiles."""
    f32, f64 = np.float32, np.float64
    p = plan(1000, 10, 4, f64)
    piece, span = p["piece"], p["hist_span"]
    cases = {}

    def add(name, X, init, max_iter=300, tol_abs=0.0):
        cases[name] = (X, init, max_iter, tol_abs)
    sizes = [piece, piece + 1, 3 * piece + 7, 1]
    add("pieces_f64", *blobs(sum(sizes), 10, 4, f64, 1, sizes=sizes))
    add("pieces_f32", *blobs(sum(sizes), 10, 4, f32, 2, sizes=sizes))
    add("k1_f32", *blobs(1000, 3, 1, f32, 3))
    for n in (span - 1, span, span + 1):
        add("span_%d_f32" % n, *blobs(n, 3, 5, f32, 4))
    wide32 = plan(600, 131, 3, f32)
    assert wide32["feature_tiles"] > 1 and plan(600, 512, 3, f64)["feature_tiles"] > 1
    add("tiles_f32_131", *blobs(600, 131, 3, f32, 5))
    add("tiles_f64_512", *blobs(600, 512, 3, f64, 6))
    for dt, tag in ((f32, "f32"), (f64, "f64")):
        for F in (3, 10):
            add("F%d_%s" % (F, tag), *blobs(2000, F, 7, dt, 7 + F))
    add("F512_f32", *blobs(2000, 512, 7, f32, 20))
    for K in (127, 128, 129):
        add("K%d_f32" % K, *blobs(3000, 10, K, f32, 30 + K))
    add("K1000_100k_f64", *blobs(100000, 10, 1000, f64, 40))
    # stop rules
    add("stop_strict", *blobs(1500, 4, 5, f64, 50, spread=2.0))
    X, init = drift(3000, 4, 6, f64, 51)
    add("stop_tol", X, init, 300, 1e-3)
    add("stop_maxiter", X, init, 3, 0.0)
    # relocation
    X, init = blobs(1200, 4, 5, f64, 60, spread=1.0)
    add("reloc_one", X, far_init(X, init, [2]))
    add("reloc_three", X, far_init(X, init, [0, 2, 3]))
    X, init = blobs(1200, 4, 5, f32, 61, spread=1.0)
    add("reloc_one_f32", X, far_init(X, init, [4]))
    add("reloc_tie_f64", *tie_case(f64))
    add("reloc_tie_f32", *tie_case(f32))
    # label chunks of the histogram / scatter waves (2048 labels per pass; more than one wave: n > span)
    assert 8000 > span
    add("K2048_f32", *blobs(8000, 10, 2048, f32, 301, spread=3.0))    # (spread=4.0 leaves two rows undecidable)
    X, init = blobs(8000, 10, 2049, f32, 300, spread=4.0)
    add("K2049_f32", X, init)
    add("K4097_f64", *blobs(9000, 10, 4097, f64, 302, spread=4.0))
    X, init = blobs(8000, 10, 2049, f32, 300, spread=2.0)
    add("reloc_K2049_f32", X, far_init(X, init, RELOC_TARGETS["reloc_K2049_f32"]))    # both ends of chunk 0, and chunk 1
    # chunks of the base kernel (256 clusters per trip), empty clusters on both sides of the chunk boundary
    for K in (255, 256, 257):
        add("K%d_f32" % K, *blobs(3000, 10, K, f32, 30 + K, spread=2.0))
    X, init = blobs(3000, 10, 300, f32, 330, spread=1.0)
    add("reloc_K300_f32", X, far_init(X, init, RELOC_TARGETS["reloc_K300_f32"]))
    # (empty clusters in the FIRST chunk only: the count of empties has to be carried into the last chunk's trip)
    add("reloc_K300_first_f32", X, far_init(X, init, RELOC_TARGETS["reloc_K300_first_f32"]))
    # relocations after iteration 0: odd / even iteration, twice in a run, in the last permitted iteration
    for name, (dt, seed, max_iter, _) in LATE.items():
        add(name, *clumps(seed, dt), max_iter=max_iter)
    # donors that give more than they keep (small integers)
    for dt, tag in ((f32, "f32"), (f64, "f64")):
        add("donor_two_" + tag, *two_from_one_donor_case(dt))
        add("donor_single_" + tag, *singleton_donor_case(dt))
        add("donor_single_cut_" + tag, *singleton_donor_case(dt), max_iter=1)
    # the inputs of the unaligned-rows test (there the rows start one element into their allocation)
    assert plan(1500, 512, 5, f32)["feature_tiles"] == 1    # (aligned: 128 units of 16 bytes; unaligned: 4 tiles)
    add("offset_f32_m4", *blobs(5000, 4, 6, f32, 400, spread=5.0))    # (16 iterations)
    add("offset_f32_m512", *blobs(1500, 512, 5, f32, 401, spread=1.0))
    add("offset_f64_m2", *blobs(5000, 2, 6, f64, 402, spread=1.0))
    assert set(UNALIGNED) | set(LABEL_CHUNK) | set(DONOR) | set(RELOC_AT_0) <= set(cases)
    return cases


def at_size_case():
    """2M x 10 float64, K = 200, five iterations at the most."""
    X, init = blobs(2000000, 10, 200, np.float64, 70)
    return X, init, 5, 0.0
