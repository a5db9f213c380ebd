"""The tICA projection restated in numpy alone: an exact reference, the error bound a correct float64 evaluation must meet,
the kernel dispatch, the batch entry's tile table and the host list's grouping -- and the inputs and shapes that
tests/test_tica_project_ref.py (CPU) and tests/test_gpu_tica_project_paths.py (GPU) share.

Rows are held as the kernels see them: float64, float32, or bfloat16 as RAW 16-bit words (numpy uint16).  `DTYPES` names
the three; `store` rounds float64 values into one of them and `widen` gives the stored values back exactly."""
import numpy as np

DTYPES = ("bf16", "f32", "f64")
NBYTES = {"bf16": 2, "f32": 4, "f64": 8}
PJ_MFMA, PJ_ROWS = 0, 1          # MSM_PJ_MFMA / MSM_PJ_ROWS of include/msmhip.h
TILE_ROWS = 256                  # rows of one tile of msm_tica_project_batch
U = 2.0 ** -53                   # unit roundoff of float64


# ------------------------------------------------------------------ element types
def store(x, dt):
    """float64 values rounded (to nearest, ties to even) into the element type: uint16 words for "bf16"."""
    x = np.asarray(x, dtype=np.float64)
    if dt == "f64":
        return x.copy()
    x32 = x.astype(np.float32)
    if dt == "f32":
        return x32
    bits = np.ascontiguousarray(x32).view(np.uint32)
    return ((bits + np.uint32(0x7fff) + ((bits >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def widen(X):
    """The stored values as float64, exactly: bfloat16 words become the upper half of a float32."""
    X = np.asarray(X)
    if X.dtype == np.uint16:
        return (X.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    return X.astype(np.float64)


def poison_like(shape, dt):
    """An array of the element type in which every other element is NaN, alternating with +Inf and -Inf."""
    n = int(np.prod(shape))
    idx = np.arange(n)
    if dt == "bf16":
        words = np.array([0x7fc0, 0x7f80, 0x7fc0, 0xff80], dtype=np.uint16)
        return words[idx % 4].reshape(shape)
    vals = np.array([np.nan, np.inf, np.nan, -np.inf])
    return vals[idx % 4].astype(np.float32 if dt == "f32" else np.float64).reshape(shape)


# ------------------------------------------------------------------ the operation
def project_ref(X, mean, V):
    """(X - mean) . V^T in np.longdouble from the stored values (64 bits of mantissa on x86: 2^11 times finer than the
    arithmetic under test)."""
    Xl = widen(X).astype(np.longdouble)
    return (Xl - np.asarray(mean, dtype=np.float64).astype(np.longdouble)).dot(np.asarray(V, dtype=np.float64).astype(np.longdouble).T)


def project_bound(X, mean, V):
    """Per output element, the largest error of a correct float64 evaluation of X . V^T - mean . V^T:

        (F + 8) * 2^-53 * (|X| . |V|^T + |mean| . |V|^T).

    With u = 2^-53 and gamma_F = F u / (1 - F u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1):
      * a chain of F fused multiply-adds, or of F rounded products and F - 1 rounded additions, computes s = sum x_f v_f
        with |s^ - s| <= gamma_F sum |x_f v_f|, in ANY order of the terms and any grouping -- the MFMA kernel's groups of
        four features and its permutation of them, and the zero terms it pads a partial chunk with (an exact zero adds
        no error), are covered;
      * the host's plain sum m^ of mean . V^T has the same form: |m^ - m| <= gamma_F sum |mean_f v_f|;
      * the final subtraction rounds once: |fl(s^ - m^) - (s^ - m^)| <= u |s^ - m^| <= u (1 + gamma_F) (sum |x v| + sum |mean v|).
    Together: (gamma_F + u (1 + gamma_F)) (sum |x v| + sum |mean v|) = ((F + 1) u + O(F^2 u^2)) (...).  The coefficient F + 8
    leaves 7 u of slack for the second-order terms (F^2 u < 7 for every F < 2^26) and for the rounding of this bound's own
    evaluation in float64.  Nothing in it comes from what the kernels return."""
    F = np.shape(V)[1]
    aV = np.abs(np.asarray(V, dtype=np.float64)).T
    mag = np.abs(widen(X)).dot(aV) + np.abs(np.asarray(mean, dtype=np.float64)).dot(aV)[None, :]
    return (F + 8) * U * mag


def within(got, X, mean, V):
    """(ok, worst error / bound) of `got` against the reference: every element finite and inside the bound."""
    got = np.asarray(got)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.longdouble) - project_ref(X, mean, V))
    bound = project_bound(X, mean, V)
    ok = bool(np.all(np.isfinite(got)) and np.all(err <= bound))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).astype(np.float64)
    ratio[np.isnan(ratio)] = np.inf
    return ok, float(ratio.max()) if got.size else 0.0


def project_f64(X, mean, V):
    """The plain float64 evaluation the bound is derived for: X . V^T - mean . V^T."""
    V = np.asarray(V, dtype=np.float64)
    return widen(X).dot(V.T) - np.asarray(mean, dtype=np.float64).dot(V.T)[None, :]


# ------------------------------------------------------------------ dispatch, tiles, groups
def plan_ref(dtype_bytes, F, ld, aligned16):
    """(kernel, vec) as the comment on msm_tica_project_plan states it: cw = 16 / dtype_bytes elements make a 16-byte vector;
    rows are read with vector loads when the base is 16-byte aligned and F and ld are multiples of cw; vector rows take the
    fp64-MFMA kernel while a 256-row tile spans less than 2^32 bytes, every other row the lane-per-row kernel."""
    cw = 16 // dtype_bytes
    vec = bool(aligned16) and F % cw == 0 and ld % cw == 0
    if vec and 256 * ld * dtype_bytes < 2 ** 32:
        return PJ_MFMA, 1
    return PJ_ROWS, int(vec)


def stride_limit(dtype_bytes):
    """The first row stride (in elements) that no longer takes the fp64-MFMA kernel: rows of 16 MiB."""
    return 2 ** 32 // (256 * dtype_bytes)


def tiles_ref(lens):
    """The tile table of msm_tica_project_batch: per non-empty trajectory, in order, one tile per 256 rows --
    (trajectory, first row, rows of the trajectory from there on)."""
    return [(s, r, n - r) for s, n in enumerate(lens) for r in range(0, n, TILE_ROWS)]


def groups_ref(lens, row_bytes, budget):
    """The groups of msm_tica_project_host_list as [begin, end) over the trajectories: whole trajectories in order; a new
    group begins where the next trajectory would take a group that already holds rows past `budget` bytes (so a
    trajectory larger than the budget is a group of its own, and an empty one after it begins the next group).  No
    groups when there is no row at all."""
    if sum(lens) == 0:
        return []
    ends, held = [], 0
    for s, n in enumerate(lens):
        b = n * row_bytes
        if held > 0 and held + b > budget:
            ends.append(s)
            held = 0
        held += b
    ends.append(len(lens))
    return list(zip([0] + ends[:-1], ends))


# ------------------------------------------------------------------ data families
FAMILIES = ("plain", "offset", "sparseV")


def make_case(family, n, F, k, dt, seed=0):
    """(X stored as `dt`, mean, V) of one data family.
      plain    3 randn + 1 against a random mean and matrix: nothing cancels (the data of tests/test_gpu_tica.py).
      offset   every column sits at an offset of 10^3 .. 10^4 times its spread and the mean within a spread of the offsets
               -- distances, angles --: X . V^T and mean . V^T agree in their leading three digits and the result is 10^3
               times smaller than its terms.  (bfloat16 keeps 8 bits of a value: its stored columns are nearly constant.)
      sparseV  plain rows against a matrix whose first, last and every fifth column are exactly zero (the last alone of two
               columns, none of one: something is left to project)."""
    rs = np.random.RandomState(1000003 * seed + 7919 * n + 31 * F + k)
    V = rs.randn(k, F)
    if family == "offset":
        spread = np.exp(rs.uniform(-2.0, 2.0, F))
        off = spread * 10.0 ** rs.uniform(3.0, 4.0, F) * rs.choice([-1.0, 1.0], F)
        X = off + spread * rs.randn(n, F)
        mean = off + 0.5 * spread * rs.randn(F)
    else:
        X = rs.randn(n, F) * 3 + 1
        mean = rs.randn(F)
        if family == "sparseV" and F > 1:
            V[:, 5::5] = 0.0
            V[:, F - 1] = 0.0
            if F > 2:
                V[:, 0] = 0.0
    return store(X, dt), mean, np.ascontiguousarray(V)


# ------------------------------------------------------------------ the shapes of the GPU module (n, F, k)
CW = {dt: 16 // NBYTES[dt] for dt in DTYPES}
# fp64-MFMA kernel: 128-byte chunks -- 1, 2, 3 and 4 of them, with and without a partial last one
MFMA_F = {"f32": (4, 36, 96, 100), "f64": (2, 18, 48, 50), "bf16": (8, 72, 192, 200)}
MFMA_N = (1, 63, 64, 65, 255, 256, 257)
MFMA_K = (1, 16, 17, 33)
# lane-per-row kernel: the NPW (components per wave) and KT (components per pass) seams
ROWS_F = (1, 63, 64, 65, 130)
ROWS_N = (1, 64, 65, 127, 128, 129)
ROWS_K = (1, 4, 5, 32, 33)


def cover(*axes):
    """Tuples that take every value of every axis at least twice in different company, without the full product: two
    diagonals through the axes' grid."""
    m = max(len(a) for a in axes)
    out = []
    for i in range(m):
        out.append(tuple(a[i % len(a)] for a in axes))
    for i in range(m):
        out.append(tuple(a[(i + 1 + j) % len(a)] for j, a in enumerate(axes)))
    return sorted(set(out))


def mfma_shapes(dt):
    return [(n, F, k) for n, F, k in cover(MFMA_N, MFMA_F[dt], MFMA_K)]


def rows_shapes():
    return [(n, F, k) for n, F, k in cover(ROWS_N, ROWS_F, ROWS_K)]


BATCH_LENS = (0, 1, 255, 256, 257, 512, 513)
BATCH_F = {"f32": 36, "f64": 18, "bf16": 72}          # two chunks, the second partial
GROUP_LENS = (300, 0, 0, 1, 700, 0, 257, 5, 0)
GROUP_BUDGET_ROWS = 300
GROUP_F = {"f32": (36, 35), "f64": (18, 17)}          # a width on each kernel
CONTAIN_N = 300                                       # rows 0, 255, 256 and n - 1: both sides of a 256-row tile
WIDE_F = {"f32": 72, "f64": 72, "bf16": 136}          # 16 MiB rows: the 64-feature chunk of the row kernel is partial


MISALIGNED_SHAPE = {dt: (129, MFMA_F[dt][1], 5) for dt in DTYPES}     # whole vectors one element off the 16-byte grid
HOST_STRIDED_N, HOST_STRIDED_K = 257, 17                              # host rows at ld > F, widths BATCH_F and BATCH_F - 1
CANCEL_SHAPES = {dt: ((257, MFMA_F[dt][3], 17), (257, 65, 17)) for dt in DTYPES}   # the `offset` family on each kernel


def all_shapes(dt):
    """Every (n, F, k) the GPU module draws from make_case for this element type (lists are cut from one draw)."""
    s = set(mfma_shapes(dt)) | set(rows_shapes())
    s |= {(sum(BATCH_LENS), BATCH_F[dt], k) for k in MFMA_K} | {(sum(BATCH_LENS), BATCH_F[dt] - 1, 17)}   # cut into BATCH_LENS
    s |= {(3, WIDE_F[dt], 17), (256, WIDE_F[dt], 17)}
    s |= {(CONTAIN_N, BATCH_F[dt], 5), (CONTAIN_N, BATCH_F[dt] - 1, 5)}
    s |= {MISALIGNED_SHAPE[dt]} | set(CANCEL_SHAPES[dt])
    s |= {(HOST_STRIDED_N, BATCH_F[dt], HOST_STRIDED_K), (HOST_STRIDED_N, BATCH_F[dt] - 1, HOST_STRIDED_K)}
    if dt in GROUP_F:
        s |= {(sum(GROUP_LENS), F, 5) for F in GROUP_F[dt]} | {(700, F, 5) for F in GROUP_F[dt]}
    return sorted(s)
