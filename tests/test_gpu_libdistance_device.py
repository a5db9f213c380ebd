"""GPU tier: msmbuilder_amd.libdistance where tests/test_gpu_libdistance.py does not go -- device-resident inputs on every
kernel family (aligned and offset base pointers), the grid-stride loops past their block caps, the zero-padded copy of
odd rows, zero-laden / non-finite rows through every family, and empty results and errors on the device.

Reference throughout: oracle.libdistance_oracle.Oracle (plain C, one fp64 accumulator per pair, features in order) on host
copies of the same arrays.  Labels and distances are compared with np.array_equal(..., equal_nan=True): bit for bit, NaN
positions included.  Sums (inertia, sumdist) are compared with math.fsum of the oracle's bit-exact per-row / per-pair
distances to a bound derived from the depth of the summation (libdistance_cases.sum_matches, _assign_depth,
_sumdist_depth below) -- not to a measured tolerance.

Which kernel a call lands on (csrc/distance.hip: row_vecw, wide_ok, launch_pair):
  rows of at most 32 float32 / 16 float64 features, no X_indices, base aligned to the element
      -> register-resident kernels (vector width 16 / 8 / element by base % 16 and row bytes)
  longer rows of whole 16-byte groups, base % 16 == 0, no X_indices  -> wide streaming kernel
  everything else (X_indices, odd long rows, long rows at an offset base)  -> LDS pair kernel

The inputs are small wherever the seam allows it, and the oracle's results are computed once per (shape, dtype, metric)
and shared by the layouts.
"""
import functools
import math

import numpy as np
import pytest

from libdistance_cases import special_centres, special_rows, sum_matches

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev", "canberra", "braycurtis", "hamming", "jaccard")
NORM_METRICS = ("euclidean", "sqeuclidean", "cityblock", "chebyshev")
SEAM_METRICS = ("euclidean", "canberra", "jaccard")
DTYPES = (np.float32, np.float64)

SMALL = [(300, 9, 3), (300, 9, 6), (300, 9, 8), (300, 1, 16)]     # register-resident
LDS = [(777, 20, 45)]                                             # LDS pair kernel
WIDE = [(777, 20, 44), (513, 17, 18), (600, 5, 260)]              # wide kernel (the last: 8-centre groups)

# (layout name, element offset of the view into its buffer, dtypes it applies to)
LAYOUTS = [("contiguous", 0, DTYPES), ("offset1", 1, DTYPES), ("offset2", 2, (np.float32,))]
LAYOUT_CASES = [pytest.param(o, dt, id="%s-%s" % (name, np.dtype(dt).name))
                for name, o, dts in LAYOUTS for dt in dts]


@pytest.fixture(scope="module")
def oracle():
    from oracle.libdistance_oracle import Oracle
    return Oracle()


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _family(m, dtype, offset=0, indexed=False):
    """The kernel family assign_nearest lands on (launch_pair in csrc/distance.hip), for rows that are not padded."""
    size = np.dtype(dtype).itemsize
    if indexed:
        return "lds"
    if m <= 128 // size:               # FeatChunk: 32 float32 / 16 float64 features
        return "small"
    return "wide" if m % (16 // size) == 0 and offset == 0 else "lds"


def _assign_depth(n, family):
    """Additions a row's distance passes through, at most, on its way into assign_nearest's inertia: a thread adds its
    rows sequentially, the workgroup's 256 sums meet in an 8-level tree in LDS, the host adds the g block partials
    sequentially (sum_partials_host).  Per family, with nt = ceil(n / 256):
      "lds"    pair_kernel: g = min(nt, 2048) workgroups, one row per thread and 256-row tile: ceil(nt / g) rows;
      "small"  assign_small2 / assign_small3 / assign_screen: the same g, but two rows per thread and 512-row tile:
               2 * ceil(ceil(n / 512) / g) rows (for n <= 2048 * 512 half of the workgroups add nothing);
      "wide"   wide_kernel: g = min(nt, 2 * CUs) (wide_grid), two rows per 256-row tile in half of the lanes:
               2 * ceil(nt / g) rows."""
    nt = -(-n // 256)
    if family == "lds":
        g = max(1, min(nt, 2048))
        rows = -(-nt // g)
    elif family == "small":
        g = max(1, min(nt, 2048))
        rows = 2 * -(-(-(-n // 512)) // g)
    else:
        assert family == "wide"
        g = max(1, min(nt, 2 * _cus()))
        rows = 2 * -(-nt // g)
    return rows + 8 + g


def _sumdist_depth(p):
    """sumdist_kernel: g = min(ceil(p / 256), 1024) workgroups; a thread adds ceil(p / (256 g)) pairs sequentially, then
    the 8-level tree, then the host's sequential sum of the g partials."""
    g = max(1, min(-(-p // 256), 1024))
    return -(-p // (256 * g)) + 8 + g


def _to_device(a, offset=0):
    """A CUDA copy of a host array: contiguous, or (offset > 0) a view `offset` elements into a larger buffer, so that
    its base pointer is 4 or 8 bytes past a 16-byte boundary."""
    t = torch.from_numpy(np.array(a, order="C"))      # (a copy: the shared references are read-only arrays)
    if offset == 0:
        d = t.cuda()
    else:
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
        d = buf[offset:].view(*t.shape)
        d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 16 == (offset * t.element_size()) % 16
    return d


def _np(x):
    return x.cpu().numpy() if torch.is_tensor(x) else x


def _random_case(n, k, m, dtype, metric):
    """The host test's recipe: randn rows (rounded for the two counting metrics), exact hits, a duplicated centre."""
    rs = np.random.RandomState(n + k + m)
    X = rs.randn(n, m).astype(dtype)
    Y = rs.randn(k, m).astype(dtype)
    if metric in ("hamming", "jaccard"):
        X, Y = np.round(X).astype(dtype), np.round(Y).astype(dtype)
    Y[: min(k, 3)] = X[: min(k, 3)]          # exact hits / duplicate-distance ties
    if k > 4:
        Y[4] = Y[1]                           # identical centres: lowest index must win
    return X, Y


def _special_case(n, k, m, dtype):
    X, rows = special_rows(n, m, dtype, seed=n + m)
    return X, special_centres(X, rows, k, seed=n + m), rows


def _pair_distances(oracle, X, metric, pairs, cond=None):
    """The oracle's distance of every listed pair, bit for bit: out of its condensed pdist (every metric is symmetric in
    its two rows bit for bit: differences under fabs, sums commutative), pairs of a row with itself one by one."""
    n = X.shape[0]
    if cond is None:
        cond = oracle.pdist(X, metric)
    lo, hi = pairs.min(axis=1), pairs.max(axis=1)
    d = np.empty(len(pairs))
    ne = lo < hi
    d[ne] = cond[lo[ne] * n - lo[ne] * (lo[ne] + 1) // 2 + (hi[ne] - lo[ne] - 1)]
    for q in np.flatnonzero(~ne):
        d[q] = oracle.sumdist(X, metric, pairs[q:q + 1])
    return d


@functools.lru_cache(maxsize=None)
def _reference(kind, n, k, m, dtn, metric):
    """Host inputs and the oracle's results for one (recipe, shape, dtype, metric): computed once, shared by the
    placements / layouts that run it, never modified (the arrays are read-only)."""
    from oracle.libdistance_oracle import Oracle
    oracle = Oracle()
    dtype = np.dtype(dtn).type
    if kind == "random":
        X, Y = _random_case(n, k, m, dtype, metric)
        extra = np.zeros(0, dtype=np.int64)
    else:
        X, Y, extra = _special_case(n, k, m, dtype)
    rs = np.random.RandomState(n + k + m + 1)
    idx = rs.randint(0, n, size=41).astype(np.int64)      # unsorted, with duplicates
    idx[:len(extra)] = extra
    idx[40] = idx[7]
    fin = np.flatnonzero(np.isfinite(X).all(axis=1))
    R = dict(X=X, Y=Y, idx=idx, Xfin=np.ascontiguousarray(X[fin]), idx_fin=np.ascontiguousarray(fin[::-1][:101]))
    with np.errstate(all="ignore"):
        R["lab"], _, R["mind"] = oracle.assign_nearest(X, Y, metric, return_distances=True)
        R["lab_i"], _, R["mind_i"] = oracle.assign_nearest(X, Y, metric, idx, return_distances=True)
        # the finite rows on their own, as rows and as an index list: with the NaN / inf rows in, their DBL_MAX terms
        # make most metrics' inertia just inf
        R["lab_f"], _, R["mind_f"] = oracle.assign_nearest(R["Xfin"], Y, metric, return_distances=True)
        R["lab_fi"], _, R["mind_fi"] = oracle.assign_nearest(X, Y, metric, R["idx_fin"], return_distances=True)
        assert np.isfinite(R["mind_f"]).all() and np.isfinite(R["mind_fi"]).all()
        R["cdist"] = oracle.cdist(X, Y, metric)
        R["dist"] = oracle.dist(X, Y[0], metric)
        R["dist_i"] = oracle.dist(X, Y[0], metric, idx)
        if n <= 300:
            R["pdist"] = oracle.pdist(X, metric)
            R["pdist_i"] = oracle.pdist(X, metric, idx)
            pairs = rs.randint(0, n, size=(300, 2)).astype(np.int64)
            pairs[:len(extra), 0] = extra
            pairs[5] = pairs[6, ::-1]
            pairs[7, 1] = pairs[7, 0]                     # a row with itself
            R["pairs"] = pairs
            R["pair_d"] = _pair_distances(oracle, X, metric, pairs, R["pdist"])
            # the pairs of finite rows on their own: with a NaN or inf row in the list most metrics' sum is just NaN
            R["pairs_fin"] = np.ascontiguousarray(pairs[np.isfinite(X[pairs]).all(axis=(1, 2))])
            R["pair_d_fin"] = _pair_distances(oracle, X, metric, R["pairs_fin"], R["pdist"])
    for v in R.values():
        v.setflags(write=False)
    return R


def _run_case(R, metric, offset, device):
    """Every libdistance call of one case against the oracle's results R; `device`: X, Y, X_indices and the pair list
    are CUDA tensors (X `offset` elements into its buffer), and what comes back must be placed as documented."""
    from msmbuilder_amd import libdistance as ld
    n, m = R["X"].shape
    k = R["Y"].shape[0]
    if device:
        X, Y, idx = _to_device(R["X"], offset), _to_device(R["Y"]), _to_device(R["idx"])
    else:
        X, Y, idx = R["X"], R["Y"], R["idx"]

    def placed(out, shape, dt):
        if device:
            assert torch.is_tensor(out) and out.is_cuda and out.dtype == dt and tuple(out.shape) == shape
        else:
            assert isinstance(out, np.ndarray) and out.shape == shape
        return _np(out)

    lab, inertia = ld.assign_nearest(X, Y, metric)
    assert type(inertia) is float
    assert np.array_equal(placed(lab, (n,), torch.int64), R["lab"])
    family = _family(m, R["X"].dtype, offset)
    assert sum_matches(inertia, R["mind"], _assign_depth(n, family)), (inertia, R["mind"].sum())
    lab, inertia = ld.assign_nearest(X, Y, metric, idx)
    assert type(inertia) is float
    assert np.array_equal(placed(lab, (41,), torch.int64), R["lab_i"])
    assert sum_matches(inertia, R["mind_i"], _assign_depth(41, "lds")), (inertia, R["mind_i"].sum())
    nf, ni = R["Xfin"].shape[0], len(R["idx_fin"])
    lab, inertia = ld.assign_nearest(_to_device(R["Xfin"], offset) if device else R["Xfin"], Y, metric)
    assert np.array_equal(placed(lab, (nf,), torch.int64), R["lab_f"])
    assert sum_matches(inertia, R["mind_f"], _assign_depth(nf, family)), (inertia, R["mind_f"].sum())
    lab, inertia = ld.assign_nearest(X, Y, metric, _to_device(R["idx_fin"]) if device else R["idx_fin"])
    assert np.array_equal(placed(lab, (ni,), torch.int64), R["lab_fi"])
    assert sum_matches(inertia, R["mind_fi"], _assign_depth(ni, "lds")), (inertia, R["mind_fi"].sum())
    assert _same(placed(ld.cdist(X, Y, metric), (n, k), torch.float64), R["cdist"])
    assert _same(placed(ld.dist(X, Y[0], metric), (n,), torch.float64), R["dist"])
    assert _same(placed(ld.dist(X, Y[0], metric, idx), (41,), torch.float64), R["dist_i"])
    if "pdist" in R:
        assert _same(placed(ld.pdist(X, metric), (n * (n - 1) // 2,), torch.float64), R["pdist"])
        assert _same(placed(ld.pdist(X, metric, idx), (41 * 40 // 2,), torch.float64), R["pdist_i"])
        for pk, dk in (("pairs", "pair_d"), ("pairs_fin", "pair_d_fin")):
            s = ld.sumdist(X, metric, _to_device(R[pk]) if device else R[pk])
            assert type(s) is float
            assert sum_matches(s, R[dk], _sumdist_depth(len(R[pk]))), (pk, s, R[dk].sum())


# ------------------------------------------------------------------ B1: device inputs on every kernel family
@pytest.mark.parametrize("offset,dtype", LAYOUT_CASES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,k,m", SMALL + LDS + WIDE)
def test_device_inputs_every_family(gpu, n, k, m, metric, offset, dtype):
    """Base % 16 is 0 (contiguous), 4 / 8 (offset 1: float32 / float64) or 8 (offset 2, float32: 8-byte vector loads
    when the row bytes divide by 8).  At an offset base the wide shapes run on the LDS pair kernel."""
    _run_case(_reference("random", n, k, m, np.dtype(dtype).name, metric), metric, offset, True)


# ------------------------------------------------------------------ B3: special rows through every family
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,k,m", [(300, 9, 8), (777, 20, 45), (777, 20, 44), (513, 17, 18), (300, 9, 33)])
def test_special_rows_every_family(gpu, n, k, m, metric, dtype, device):
    """Zero-laden and non-finite rows (libdistance_cases.special_rows) on the register-resident, LDS and wide kernels,
    and at (300, 33) for pdist / sumdist (the 300-row cases run them): labels, distances, NaN and inf positions as the
    oracle's, sums NaN / inf where the oracle's terms make them so."""
    _run_case(_reference("special", n, k, m, np.dtype(dtype).name, metric), metric, 0, device)


# ------------------------------------------------------------------ B2: grid seams
N_PAIR = 524288 + 300      # 2048 workgroups x 256 rows, and a partial tile past them
N_PAIR2 = 2048 * 512 + 300   # the same for the kernels that take 512 rows per tile


def _seam_rows(n, m, dtype, metric, seed, no_zero_rows=False):
    rs = np.random.RandomState(seed)
    X = rs.randn(n, m).astype(dtype)
    if metric in ("hamming", "jaccard"):
        X = np.round(X).astype(dtype)            # (at m = 3 one rounded row in 18 is all zero: jaccard 0/0 between two)
        if no_zero_rows:
            X[~X.any(axis=1), 0] = 1.0
    return X


def _seam_centres(X, k):
    n = X.shape[0]
    Y = X[np.linspace(0, n - 1, k).astype(np.int64)].copy()      # exact hits in the first and the last tile
    if k > 4:
        Y[4] = Y[1]
    return Y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", SEAM_METRICS)
def test_pair_kernels_past_2048_blocks_cdist_dist(gpu, oracle, metric, dtype):
    from msmbuilder_amd import libdistance as ld
    X = _seam_rows(N_PAIR, 5, dtype, metric, 1)
    Y = _seam_centres(X, 3)
    Xd = _to_device(X)
    with np.errstate(all="ignore"):
        assert _same(_np(ld.cdist(Xd, Y, metric)), oracle.cdist(X, Y, metric))
        assert _same(_np(ld.dist(Xd, Y[2], metric)), oracle.dist(X, Y[2], metric))


@pytest.mark.parametrize("dtype,metric,screen", [(np.float32, "euclidean", None), (np.float64, "euclidean", "1"),
                                                 (np.float64, "euclidean", "0"), (np.float32, "sqeuclidean", None),
                                                 (np.float64, "sqeuclidean", None), (np.float32, "cityblock", None),
                                                 (np.float64, "cityblock", None)])
@pytest.mark.parametrize("n", [N_PAIR, N_PAIR2])
def test_pair_kernels_past_2048_blocks_assign(gpu, oracle, monkeypatch, dtype, metric, screen, n):
    """assign_small3 (euclidean family; float64 euclidean: the screened kernel, and assign_small3 with the screen off)
    and assign_small2 (cityblock).  These take two rows per lane, 512 per tile, on a grid of min(ceil(n / 256), 2048)
    workgroups: at 524,588 rows that is 1,025 tiles on 2,048 workgroups (half of them idle, every partial still
    summed), and only at 2048 * 512 + 300 rows does workgroup 0 stride to a second tile."""
    from msmbuilder_amd import libdistance as ld
    if screen is not None:
        monkeypatch.setenv("MSM_ASSIGN_SCREEN", screen)
    X = _seam_rows(n, 5, dtype, metric, 2)
    Y = _seam_centres(X, 9)
    lab, inertia = ld.assign_nearest(_to_device(X), Y, metric)
    lab_o, _, mind = oracle.assign_nearest(X, Y, metric, return_distances=True)
    assert np.array_equal(_np(lab), lab_o)
    assert sum_matches(inertia, mind, _assign_depth(n, "small")), (inertia, mind.sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", SEAM_METRICS)
def test_lds_pair_kernel_past_2048_blocks(gpu, oracle, metric, dtype):
    """X_indices sends every shape to the LDS pair kernel, and the row count is the index count: 524,588 indices into
    1,000 rows."""
    from msmbuilder_amd import libdistance as ld
    X = _seam_rows(1000, 5, dtype, metric, 3)
    Y = _seam_centres(X, 9)
    idx = np.random.RandomState(4).randint(0, 1000, size=N_PAIR).astype(np.int64)
    Xd, idxd = _to_device(X), _to_device(idx)
    with np.errstate(all="ignore"):
        lab, inertia = ld.assign_nearest(Xd, Y, metric, idxd)
        lab_o, _, mind = oracle.assign_nearest(X, Y, metric, idx, return_distances=True)
        assert tuple(lab.shape) == (N_PAIR,) and np.array_equal(_np(lab), lab_o)
        assert sum_matches(inertia, mind, _assign_depth(N_PAIR, "lds")), (inertia, mind.sum())
        assert _same(_np(ld.dist(Xd, Y[3], metric, idxd)), oracle.dist(X, Y[3], metric, idx))


@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", SEAM_METRICS)
def test_wide_kernel_past_its_grid(gpu, oracle, metric, dtype, k):
    """The wide kernel's grid is one resident round, 2 x CUs workgroups of 256 rows: 77 rows more than that, so
    workgroup 0 takes a second (partial) tile.  K = 3: 8-centre groups; K = 20: a full and a partial 16-centre group."""
    from msmbuilder_amd import libdistance as ld
    n, m = 2 * _cus() * 256 + 77, (36 if dtype == np.float32 else 18)
    X = _seam_rows(n, m, dtype, metric, 5)
    Y = _seam_centres(X, k)
    Xd = _to_device(X)
    with np.errstate(all="ignore"):
        lab, inertia = ld.assign_nearest(Xd, Y, metric)
        lab_o, _, mind = oracle.assign_nearest(X, Y, metric, return_distances=True)
        assert np.array_equal(_np(lab), lab_o)
        assert sum_matches(inertia, mind, _assign_depth(n, "wide")), (inertia, mind.sum())
        assert _same(_np(ld.cdist(Xd, Y, metric)), oracle.cdist(X, Y, metric))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("metric", NORM_METRICS)
@pytest.mark.parametrize("dtype,n,m", [(np.float32, 6200, 171), (np.float64, 61700, 17)])
def test_padded_copy_of_odd_rows(gpu, oracle, dtype, n, m, metric, device):
    """Norm metrics, long rows that are no whole number of 16-byte groups, n m >= 2^20: assign_nearest runs the wide
    kernel on a zero-padded copy (pad_rows_pays).  cdist takes no such copy; its first 2,000 rows stay on the LDS kernel."""
    from msmbuilder_amd import libdistance as ld
    assert n * m >= 1 << 20 and (n - 100) * m < 1 << 20       # just past the threshold
    X = _seam_rows(n, m, dtype, metric, 6)
    Y = _seam_centres(X, 9)
    Xa = _to_device(X) if device else X
    lab, inertia = ld.assign_nearest(Xa, Y, metric)
    lab_o, _, mind = oracle.assign_nearest(X, Y, metric, return_distances=True)
    assert np.array_equal(_np(lab), lab_o)
    assert sum_matches(inertia, mind, _assign_depth(n, "wide")), (inertia, mind.sum())
    assert _same(_np(ld.cdist(Xa[:2000], Y, metric)), oracle.cdist(X[:2000], Y, metric))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", SEAM_METRICS)
def test_pdist_past_4096_blocks(gpu, oracle, metric, dtype):
    """pdist_kernel: one workgroup per first row, at most 4096: 4,200 rows, and 4,200 indices into 500 rows."""
    from msmbuilder_amd import libdistance as ld
    X = _seam_rows(4200, 3, dtype, metric, 7)
    X[4100] = X[3]                                              # a zero distance in a strided row
    with np.errstate(all="ignore"):
        got = ld.pdist(_to_device(X), metric)
        assert tuple(got.shape) == (4200 * 4199 // 2,)
        assert _same(_np(got), oracle.pdist(X, metric))
        del got
        idx = np.random.RandomState(8).randint(0, 500, size=4200).astype(np.int64)
        Xs = np.ascontiguousarray(X[:500])
        assert _same(_np(ld.pdist(_to_device(Xs), metric, _to_device(idx))), oracle.pdist(Xs, metric, idx))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", SEAM_METRICS)
def test_pdist_lds_feature_sweeps_on_device(gpu, oracle, metric, dtype):
    """Rows of 1,100 features: two sweeps of the 1,024-feature LDS stage of row i."""
    from msmbuilder_amd import libdistance as ld
    X = _seam_rows(64, 1100, dtype, metric, 9)
    idx = np.random.RandomState(10).randint(0, 64, size=11).astype(np.int64)
    Xd = _to_device(X)
    with np.errstate(all="ignore"):
        assert _same(_np(ld.pdist(Xd, metric)), oracle.pdist(X, metric))
        assert _same(_np(ld.pdist(Xd, metric, _to_device(idx))), oracle.pdist(X, metric, idx))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("metric", SEAM_METRICS)
def test_sumdist_past_1024_blocks(gpu, oracle, metric, dtype, device):
    """sumdist_kernel: 256 pairs per workgroup, at most 1024 workgroups; 513 pairs more, so the first three workgroups
    take a second round.  Every distance is finite, so that the sum says something for every metric."""
    from msmbuilder_amd import libdistance as ld
    p = 262144 + 513
    X = _seam_rows(4200, 3, dtype, metric, 11, no_zero_rows=True)
    pairs = np.random.RandomState(12).randint(0, 4200, size=(p, 2)).astype(np.int64)
    pairs[p - 1] = (4199, 0)
    with np.errstate(all="ignore"):
        d = _pair_distances(oracle, X, metric, pairs)
        s = ld.sumdist(_to_device(X), metric, _to_device(pairs)) if device else ld.sumdist(X, metric, pairs)
    assert type(s) is float
    assert np.isfinite(d).all() and d.sum() > 0
    assert sum_matches(s, d, _sumdist_depth(p)), (s, d.sum())


# ------------------------------------------------------------------ B4: empty results and errors on the device
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_results_on_device(gpu, dtype):
    from msmbuilder_amd import libdistance as ld
    X = torch.zeros(4, 3, dtype=dtype, device="cuda")
    Y = torch.ones(2, 3, dtype=dtype, device="cuda")
    none = torch.zeros(0, dtype=torch.int64, device="cuda")
    for metric in ("euclidean", "jaccard"):
        out = ld.pdist(X[:1], metric)
        assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (0,)
        out = ld.pdist(X, metric, none)
        assert out.is_cuda and tuple(out.shape) == (0,)
        out = ld.dist(X, Y[0], metric, none)
        assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (0,)
        out = ld.cdist(X[:0], Y, metric)
        assert out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (0, 2)
        out = ld.cdist(X, Y[:0], metric)
        assert out.is_cuda and tuple(out.shape) == (4, 0)
        lab, inertia = ld.assign_nearest(X, Y, metric, none)
        assert lab.is_cuda and lab.dtype == torch.int64 and tuple(lab.shape) == (0,) and inertia == 0.0
        assert ld.sumdist(X, metric, torch.zeros(0, 2, dtype=torch.int64, device="cuda")) == 0.0
    # the same calls on host arrays
    Xh, Yh, noneh = X.cpu().numpy(), Y.cpu().numpy(), np.zeros(0, dtype=np.int64)
    assert ld.pdist(Xh[:1], "euclidean").shape == (0,) and ld.dist(Xh, Yh[0], "euclidean", noneh).shape == (0,)
    assert ld.cdist(Xh[:0], Yh, "euclidean").shape == (0, 2)


def test_error_contract_on_device(gpu):
    from msmbuilder_amd import libdistance as ld
    X = torch.zeros(6, 4, dtype=torch.float32, device="cuda")
    Y = torch.zeros(2, 4, dtype=torch.float32, device="cuda")
    idx_h, idx_d = np.arange(3, dtype=np.int64), torch.arange(3, device="cuda")
    pairs_h = np.zeros((2, 2), dtype=np.int64)
    # X and X_indices / pairs on different sides
    for call in (lambda: ld.assign_nearest(X, Y, "euclidean", idx_h), lambda: ld.dist(X, Y[0], "euclidean", idx_h),
                 lambda: ld.pdist(X, "euclidean", idx_h), lambda: ld.sumdist(X, "euclidean", pairs_h),
                 lambda: ld.assign_nearest(X.cpu().numpy(), Y.cpu().numpy(), "euclidean", idx_d),
                 lambda: ld.dist(X.cpu().numpy(), Y[0].cpu().numpy(), "euclidean", idx_d),
                 lambda: ld.pdist(X.cpu().numpy(), "euclidean", idx_d),
                 lambda: ld.sumdist(X.cpu().numpy(), "euclidean", torch.from_numpy(pairs_h).cuda())):
        with pytest.raises(ValueError):
            call()
    # not contiguous
    for call in (lambda: ld.assign_nearest(X[:, ::2], Y[:, ::2], "euclidean"), lambda: ld.cdist(X.t(), Y.t(), "euclidean"),
                 lambda: ld.dist(X[:, ::2], Y[0, ::2], "euclidean"), lambda: ld.pdist(X[::2, 1:], "euclidean"),
                 lambda: ld.sumdist(X.t(), "euclidean", torch.from_numpy(pairs_h).cuda())):
        with pytest.raises(ValueError):
            call()
    # mismatched dtypes, float16
    for call in (lambda: ld.assign_nearest(X, Y.double(), "euclidean"), lambda: ld.cdist(X.double(), Y, "euclidean"),
                 lambda: ld.dist(X, Y[0].double(), "euclidean"), lambda: ld.assign_nearest(X.half(), Y.half(), "euclidean"),
                 lambda: ld.cdist(X.half(), Y.half(), "euclidean"), lambda: ld.dist(X.half(), Y[0].half(), "euclidean"),
                 lambda: ld.pdist(X.half(), "euclidean"),
                 lambda: ld.sumdist(X.half(), "euclidean", torch.from_numpy(pairs_h).cuda())):
        with pytest.raises(TypeError):
            call()
    with pytest.raises(ValueError):
        ld.cdist(X, Y, "minkowski")
