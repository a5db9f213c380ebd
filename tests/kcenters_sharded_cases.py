"""Inputs of the two-rank k-centers cases of test_gpu_kcenters_sharded.py: plain numpy, shared by the worker processes
(every rank must build the same array) and by the test that starts them.

Every case is (name, dtype, features, metric, K, rows, cut, random_state, loop): rank 0 fits rows [0, cut), rank 1 the rest.
`loop` is what msm_kcenters_last_stats must show on a rank that has rows: "plain" (fused loop, K plain passes), "batched"
(two plain passes, then fewer rounds than centres) or "generic" (the stats are left as they were)."""
import numpy as np

N = 7013


def seed_state(n, want):
    """The lowest random_state whose first draw, check_random_state(s).randint(0, n) as KCenters makes it, is `want`."""
    for s in range(100_000):
        if np.random.RandomState(s).randint(0, n) == want:
            return s
    raise AssertionError((n, want))


TWO_RANK_CASES = [
    ("f32-fused", np.float32, 10, "euclidean", 25, N, 2000, 4, "plain"),
    ("f32-fused-rank0-empty", np.float32, 10, "euclidean", 25, N, 0, 4, "plain"),
    ("f64-cityblock", np.float64, 10, "cityblock", 25, N, 2600, 5, "plain"),
    ("f64-chebyshev", np.float64, 10, "chebyshev", 25, N, 4100, 6, "plain"),
    ("f64-generic-wide", np.float64, 20, "euclidean", 12, N, 2300, 7, "generic"),
    ("f64-generic-narrow", np.float64, 17, "euclidean", 12, N, 3900, 8, "generic"),
    ("f32-generic-canberra", np.float32, 40, "canberra", 9, N, 3100, 9, "generic"),
    # a one-row shard in the batched loop: its row is the later twin of the farthest row (it ties and loses) ...
    ("f64-batched-one-row", np.float64, 3, "euclidean", 9, 300, 299, 10, "batched"),
    # ... and the same rows with the seed on it
    ("f64-batched-one-row-seed", np.float64, 3, "euclidean", 9, 300, 299, seed_state(300, 299), "batched"),
]


def two_rank_rows(index):
    """Rows around 12 hubs.  Row 3 is the farthest row from the bulk and has a twin in the first rows of rank 1's block, so
    the two ranks offer the same distance and the lower global row must win; four more far rows lie on alternating sides
    of the cut.  The 300-row cases (K = 9 in the batched loop, which needs rows of nearly equal distance to take more
    than one centre in a round): a tight bulk, the twins rows 5 and 299 at twice the distance of six rows on the axes."""
    name, dtype, m, metric, k, n, cut, state, loop = TWO_RANK_CASES[index]
    rs = np.random.RandomState(100 + index)
    hubs = rs.randn(12, m) * 2.0
    X = hubs[rs.randint(0, 12, size=n)] + rs.randn(n, m)
    if n == 300:
        X *= 0.05
        X[5] = X[299] = np.array([100.0, 0.0, 0.0])
        for j, r in enumerate((20, 70, 120, 170, 220, 270)):
            X[r] = 0.0
            X[r, j // 2] = (50.0 + 0.01 * j) * (1 - 2 * (j % 2))
        return np.ascontiguousarray(X.astype(dtype))
    first, twin = 3, cut + 1
    X[first] = 9.0 + rs.rand(m)
    X[twin] = X[first]
    if cut > 1:
        for j, r in enumerate((cut - 1, cut + 2, cut // 2, cut + 4)):
            X[r] = rs.randn(m) * (7.0 + j)
    return np.ascontiguousarray(X.astype(dtype))


def batch_rows(n, m, seed):
    """float64 rows for the batched loop at K = 9 and 10.  A round takes a second centre only where another listed row
    is still farther than the round's threshold from the centre just taken, and the threshold (3 % under the last
    centre's distance, 9 % lower after a round that listed nothing) trails a distance that halves; rows around hubs give
    one centre per round for the first ten centres or so.  So: such rows (the bulk, within about 8 of the origin), row 3
    (the seed of the tests) at the origin, and 16 single rows on the first axis at +-160, +-80, +-40 and +-120, +-20 ...
    +-140 (each off by up to 0.1 %): the farthest-point order on a line, whose levels hold 2, 2, 4 and 8 rows of nearly
    equal distance that are far from each other."""
    rs = np.random.RandomState(seed)
    hubs = rs.randn(12, m) * 2.0
    X = hubs[rs.randint(0, 12, size=n)] + rs.randn(n, m)
    X[3] = 0.0
    rows = rs.choice(np.arange(4, n), size=16, replace=False)
    for j, p in enumerate((8, 4, 2, 6, 1, 3, 5, 7)):
        for sign, r in zip((1.0, -1.0), rows[2 * j:2 * j + 2]):
            X[r] = 0.0
            X[r, 0] = sign * p * 20.0 * (1.0 + 1e-3 * rs.rand())
    return X


def tie_rows(m, dtype):
    """1,000 rows around 12 hubs; rows 40 / 950 and 300 / 600 are two pairs of equal far rows, the first pair the farther
    one; eight more pairs of equal rows lie at distance 30 from the origin in random directions (far from each other and
    nearly equally far from the bulk: the batched loop takes several of them in a round, each against its twin)."""
    rs = np.random.RandomState(91)
    hubs = rs.randn(12, m) * 2.0
    X = hubs[rs.randint(0, 12, size=1000)] + rs.randn(1000, m)
    X[40] = X[950] = 80.0
    X[300] = X[600] = -45.0
    later = []
    for j in range(8):
        a, b = 100 + 37 * j, 999 - 13 * j
        u = rs.randn(m)
        X[a] = X[b] = u / np.linalg.norm(u) * 30.0 * (1.0 + 1e-3 * j)
        later.append(b)
    return np.ascontiguousarray(X.astype(dtype)), later
