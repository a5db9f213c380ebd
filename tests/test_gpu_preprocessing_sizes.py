"""The column kernels of preprocess.hip at the sizes they were tuned for: several chunks per workgroup, more than
one column round, the 16-byte load path at the bench width and with mixed alignment, device rows with a pitch, the
row grid-stride of the transform, the LDS digit pass with many tiles / one part, and two host staging groups.

Every case is compared with a plain restatement of the operation written here: numpy in long double where the
data fit on the host, a two-pass float64 computation in torch on the device where they do not (anchored once
against the long-double one, `test_torch_reference_is_anchored`), `np.sort` / `torch.sort` for order statistics.

Constants the arithmetic in the comments uses (preprocess.hip): PNT = 256 threads, PNB = 1024 scan workgroups at
most, SCAN_ROWS = 1024 rows per chunk, CW = 16 / sizeof(T) columns per group (4 float32, 2 float64), cpb = column
groups per workgroup = the power of two >= ngroups, at most 256; rl = 256 / cpb row lanes; DCOLS = 16 columns per
tile and 4096 rows per chunk in the digit passes; 8 * 2048 = 16,384 workgroups at most in msm_scale_apply with
4 * rl rows each; host staging groups of 2^30 bytes.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PNB, SCAN_ROWS, DIGIT_ROWS, DCOLS, APPLY_GRID = 1024, 1024, 4096, 16, 8 * 2048

# 1,310,003 rows in sequences of uneven length: sum(ceil(n_i / 1024)) = 1 + 1 + 2 + 5 + 293 + 2 + 979 = 1283 chunks
# > PNB = 1024 >= gridDim of colstats_kernel (gridDim = min(nchunks, min(PNB, occupancy * CUs))), so workgroups
# 0..258 take two chunks each (grid-stride loop, K = run.mean of the chunks before) whatever the CU count is; the
# last chunk holds 1,001,950 - 978 * 1024 = 478 rows (ragged tail).
BIG_LENGTHS = (1, 1023, 1025, 4097, 300000, 1907, 1001950)
BIG_F = 24


def _nchunks(lengths, rows=SCAN_ROWS):
    return sum(-(-n // rows) for n in lengths)


def _torch_dtype(dtype):
    import torch
    return torch.float32 if np.dtype(dtype) == np.float32 else torch.float64


# ---------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------
def _ref_longdouble(X):
    """[5, F] block (n, mean, M2, min, max) of a host array: two passes in long double, NaN = missing value."""
    X = np.asarray(X)
    ok = ~np.isnan(X)
    n = ok.sum(0)
    Xl = np.where(ok, X, 0).astype(np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = Xl.sum(0) / n
        m2 = (np.where(ok, Xl - mean, 0) ** 2).sum(0)
    lo = np.where(ok, X, np.inf).min(0)
    hi = np.where(ok, X, -np.inf).max(0)
    return np.stack([n.astype(np.float64), mean.astype(np.float64), m2.astype(np.float64),
                     lo.astype(np.float64), hi.astype(np.float64)])


def _ref_torch(seqs):
    """The same block for a list of torch tensors (any device): two passes in float64,
    mean = sum_i x_i.double().nansum(0) / n, M2 = sum_i nansum((x_i.double() - mean)^2)."""
    import torch
    F = seqs[0].shape[1]
    dev = seqs[0].device
    n = torch.zeros(F, dtype=torch.float64, device=dev)
    s = torch.zeros(F, dtype=torch.float64, device=dev)
    lo = torch.full((F,), float("inf"), dtype=torch.float64, device=dev)
    hi = torch.full((F,), float("-inf"), dtype=torch.float64, device=dev)
    for x in seqs:
        if x.shape[0] == 0:
            continue
        bad = torch.isnan(x)
        n += (~bad).sum(0).double()
        s += x.double().nansum(0)
        lo = torch.minimum(lo, torch.where(bad, float("inf"), x).amin(0).double())
        hi = torch.maximum(hi, torch.where(bad, float("-inf"), x).amax(0).double())
    mean = s / n
    m2 = torch.zeros(F, dtype=torch.float64, device=dev)
    for x in seqs:
        if x.shape[0]:
            m2 += ((x.double() - mean) ** 2).nansum(0)
    return torch.stack([n, mean, m2, lo, hi]).cpu().numpy()


def _block(st):
    return np.stack([st["n"], st["mean"], st["m2"], st["min"], st["max"]])


def _assert_block(got, ref, what=""):
    """The tolerances of tests/test_gpu_preprocessing.py: n exact, min / max bit-equal, mean rtol 1e-12 with
    atol 1e-12 x the column's scale (its standard deviation), M2 and var rtol 1e-10."""
    live = ref[0] > 0
    rel = np.abs(got[2][live] - ref[2][live]) / np.maximum(ref[2][live], np.finfo(float).tiny)
    print("%s: max |dmean| / (|mean| + std) = %.3g, max rel dM2 = %.3g" % (
        what, np.max(np.abs(got[1][live] - ref[1][live]) /
                     (np.abs(ref[1][live]) + np.sqrt(ref[2][live] / ref[0][live]) + np.finfo(float).tiny), initial=0.0),
        np.max(rel, initial=0.0)))
    np.testing.assert_array_equal(got[0], ref[0], err_msg=what + " n")
    np.testing.assert_array_equal(got[3][live], ref[3][live], err_msg=what + " min")
    np.testing.assert_array_equal(got[4][live], ref[4][live], err_msg=what + " max")
    std = np.sqrt(ref[2][live] / ref[0][live])
    err = np.abs(got[1][live] - ref[1][live])
    bound = 1e-12 * np.abs(ref[1][live]) + 1e-12 * std
    assert np.all(err <= bound), "%s mean: worst excess %g at column %d" % (
        what, np.max(err - bound), int(np.argmax(err - bound)))
    np.testing.assert_allclose(got[2][live], ref[2][live], rtol=1e-10, err_msg=what + " M2")
    np.testing.assert_allclose(got[2][live] / got[0][live], ref[2][live] / ref[0][live], rtol=1e-10, err_msg=what + " var")


def _randn_rows(n, F, dtype, seed, max_ratio=100.0, device="cuda"):
    """n x F device rows, column c ~ N(shift_c, scale_c^2) with |shift_c| / scale_c up to max_ratio."""
    import torch
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    scale = torch.rand(F, generator=g, device=device, dtype=torch.float64) * 29.99 + 0.01
    ratio = (torch.rand(F, generator=g, device=device, dtype=torch.float64) * 2 - 1) * max_ratio
    X = torch.randn(n, F, generator=g, device=device, dtype=_torch_dtype(dtype))
    X.mul_(scale.to(X.dtype)).add_((scale * ratio).to(X.dtype))
    return X


def _colstats_abi(gpu, blocks, F, ld, nbytes, on_device=1):
    """msm_colstats through the C ABI on (pointer, rows) pairs."""
    import torch
    torch.cuda.synchronize()
    L = gpu.lib()
    n = len(blocks)
    ptrs = (C.c_void_p * n)(*[p for p, _ in blocks])
    rows = (C.c_int64 * n)(*[r for _, r in blocks])
    out = np.empty((5, F))
    has_inf = C.c_int(0)
    gpu.check(L.msm_colstats(ptrs, rows, n, nbytes, F, ld, on_device, out.ctypes.data, C.byref(has_inf)))
    return out, has_inf.value


# ---------------------------------------------------------------------------------------------------------------
# 1. msm_colstats / StandardScaler
# ---------------------------------------------------------------------------------------------------------------
def test_torch_reference_is_anchored(gpu):
    """The device two-pass float64 reference against the long-double one, to 1e-13, on offsets up to 1e6 std and NaNs."""
    import torch
    for dtype, ratio in ((np.float64, 1e6), (np.float32, 1e4)):
        X = _randn_rows(6000, 24, dtype, 11, max_ratio=ratio)
        X[::97, 3] = float("nan")
        X[0, 5] = float("nan")
        a, b = _ref_torch([X[:1], X[1:2500], X[2500:]]), _ref_longdouble(X.cpu().numpy())
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])
        np.testing.assert_allclose(a[1], b[1], rtol=1e-13, atol=1e-13 * np.sqrt(b[2] / b[0]).min())
        np.testing.assert_allclose(a[2], b[2], rtol=1e-13)


def _big(dtype, seed=1):
    X = _randn_rows(sum(BIG_LENGTHS), BIG_F, dtype, seed)
    return X, list(X.split(list(BIG_LENGTHS)))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_colstats_many_chunks_per_workgroup(gpu, dtype):
    """nchunks = 1283 > PNB = 1024 >= gridDim (see BIG_LENGTHS): the grid-stride loop over chunks and the sums shifted
    by the running mean.  Column 1 has a NaN in row 0 of the call, column 2 a NaN in row 0 of every sequence,
    column 3 is NaN over the whole of chunk 9 (rows 0..1023 of the 300,000-row sequence; its workgroup then takes a
    finite chunk with run.n still 0), column 4 has a NaN every 32nd row (F = 24: rl = 32 float32, 16 float64, so the
    same row lanes miss every time)."""
    from msmbuilder_amd.preprocessing import column_statistics, StandardScaler
    assert _nchunks(BIG_LENGTHS) == 1283 and _nchunks(BIG_LENGTHS) > PNB
    X, seqs = _big(dtype)
    X[0, 1] = float("nan")
    for s in seqs:
        s[0, 2] = float("nan")
    seqs[4][:1024, 3] = float("nan")
    X[::32, 4] = float("nan")
    ref = _ref_torch(seqs)
    got = _block(column_statistics(seqs))
    _assert_block(got, ref, "1.3M x 24 %s" % np.dtype(dtype).name)
    m = StandardScaler().fit(seqs)
    np.testing.assert_array_equal(m.n_samples_seen_, ref[0].astype(np.int64))
    np.testing.assert_allclose(m.var_, ref[2] / ref[0], rtol=1e-10)
    np.testing.assert_allclose(m.scale_, np.sqrt(ref[2] / ref[0]), rtol=1e-10)


@pytest.mark.parametrize("dtype,F", [(np.float32, 512), (np.float64, 256)])
def test_colstats_bench_width_vector_path(gpu, dtype, F):
    """F % CW == 0, ld == F and a 256-byte aligned allocation whose rows are 2048 bytes: vec = al = 1 for every chunk
    (load16_global), ngroups = 128 = cpb, rl = 2; 300,001 rows = 1 + 99,999 + 200,001 -> 1 + 98 + 196 chunks."""
    from msmbuilder_amd.preprocessing import column_statistics
    assert F % (16 // np.dtype(dtype).itemsize) == 0
    X = _randn_rows(300001, F, dtype, 2)
    seqs = list(X.split([1, 99999, 200001]))
    assert all(s.data_ptr() % 16 == 0 for s in seqs)
    _assert_block(_block(column_statistics(seqs)), _ref_torch(seqs), "300k x %d" % F)


@pytest.mark.parametrize("dtype,F", [(np.float32, 1100), (np.float64, 600), (np.float32, 1101), (np.float64, 601)])
def test_colstats_second_column_round(gpu, dtype, F):
    """ngroups = ceil(F / CW) = 275 / 300 / 276 / 301 > 256 = the cap of cpb: the g0 loop runs a second round (its own
    __syncthreads pair, `run` re-initialised); 1100 and 600 are multiples of CW (vector path), 1101 and 601 are not."""
    import torch
    from msmbuilder_amd.preprocessing import column_statistics
    CW = 16 // np.dtype(dtype).itemsize
    assert -(-F // CW) > 256
    X = _randn_rows(3001, F, dtype, 3)
    X[0, F - 1] = float("nan")            # a second-round column whose thread starts on a NaN
    X[5::7, 256 * CW + 3] = float("nan")  # group 256 (+ 1): second round as well
    seqs = list(X.split([1, 1500, 1500]))
    ref = _ref_longdouble(X.cpu().numpy())
    _assert_block(_block(column_statistics(seqs)), ref, "3001 x %d" % F)
    _assert_block(_ref_torch(seqs), ref, "torch reference")


def test_colstats_device_pitch_and_alignment(gpu):
    """on_device = 1 with ld = 48 > F = 36 (float32, CW = 4: vec = (36 % 4 == 0 && 48 % 4 == 0) = 1).  The window
    [:, 4:40] starts 16 bytes into a 256-byte aligned allocation with 192-byte rows: al = 1 for all its chunks; the
    window [:, 3:39] starts 12 bytes in: al = 0; the third call holds one sequence of each kind."""
    A = _randn_rows(2500, 48, np.float32, 4)
    B = _randn_rows(1300, 48, np.float32, 5)
    A[0, 4] = float("nan")
    wa, wb = A[:, 4:40], B[:, 3:39]
    assert wa.data_ptr() % 16 == 0 and wb.data_ptr() % 16 == 12
    ha, hb = wa.cpu().numpy(), wb.cpu().numpy()
    for name, blocks, host in (("aligned", [(wa.data_ptr(), 2500)], ha), ("12 bytes off", [(wb.data_ptr(), 1300)], hb),
                               ("mixed", [(wb.data_ptr(), 1300), (wa.data_ptr(), 2500)], np.concatenate([hb, ha]))):
        out, inf = _colstats_abi(gpu, blocks, 36, 48, 4)
        assert inf == 0
        _assert_block(out, _ref_longdouble(host), name)


PLACEMENTS = ("none", "row0_call", "row0_every_seq", "first_row_of_later_chunk", "whole_chunk_then_finite", "every_rl_th_row")
GRID_LENGTHS = (1500, 1, 2600)
GRID_F = 96     # float64: ngroups 48, cpb 64, rl 4 (a thread sums 256 rows of a chunk); float32: ngroups 24, cpb 32, rl 8


def _grid_rows(dtype, ratio, placement):
    """Host rows (std 1, mean = ratio in every column but the first, which keeps mean 0) and the sequence cuts."""
    rs = np.random.RandomState(int(np.log10(ratio)) * 10 + PLACEMENTS.index(placement))
    X = rs.randn(sum(GRID_LENGTHS), GRID_F)
    X[:, 1:] += ratio * np.where(np.arange(1, GRID_F) % 2, 1.0, -1.0)
    X = X.astype(dtype)
    rl = 256 // (1 << int(np.ceil(np.log2(GRID_F * np.dtype(dtype).itemsize / 16))))
    starts = np.concatenate([[0], np.cumsum(GRID_LENGTHS)[:-1]])
    if placement == "row0_call":
        X[0, :] = np.nan
    elif placement == "row0_every_seq":
        X[starts[0], :] = np.nan
        X[starts[2], :] = np.nan
        X[starts[1], ::2] = np.nan        # (the one-row sequence keeps its odd columns)
    elif placement == "first_row_of_later_chunk":
        X[starts[2] + 1024, :] = np.nan
        X[starts[2] + 2048 + 1, 5] = np.nan
    elif placement == "whole_chunk_then_finite":
        X[starts[2]:starts[2] + 1024, 7] = np.nan
        X[starts[0]:starts[0] + 1024, 8] = np.nan
    elif placement == "every_rl_th_row":
        X[::rl, :] = np.nan               # lane 0 of every chunk that starts on a multiple of rl sees nothing
        X[starts[2]::rl, :] = np.nan
    return X, rl


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("dtype,ratio", [(np.float64, 1.0), (np.float64, 1e3), (np.float64, 1e4), (np.float64, 1e6),
                                         (np.float32, 1.0), (np.float32, 1e3), (np.float32, 1e4)])
def test_colstats_offset_times_nan(gpu, dtype, ratio, placement):
    """|mean| / std x where the NaNs sit.  A thread shifts its sums by the first finite value it loads; one whose first
    value was NaN used to shift by 0.0 and lost ratio^2 * eps of M2.  Worst relative error of M2 on the MI355X with
    the NaN in row 0 of the call / of every sequence / of a later chunk, before that was fixed: float64 ratio 1e3
    1.7e-10 / 2.5e-10 / 1.3e-10, ratio 1e4 2.2e-8 / 2.4e-8 / 2.2e-8, ratio 1e6 1.3e-4 / 2.1e-4 / 2.2e-4; float32 ratio
    1e3 1.0e-10 (every sequence), ratio 1e4 6.4e-9 / 1.2e-8 / 6.3e-9.  After: at most 7.7e-12 (ratio 1e6), 1.3e-13 below."""
    import torch
    from msmbuilder_amd.preprocessing import column_statistics
    X, rl = _grid_rows(dtype, ratio, placement)
    assert rl == (4 if dtype == np.float64 else 8)
    cuts = np.cumsum(GRID_LENGTHS)[:-1]
    seqs = [torch.from_numpy(a).cuda() for a in np.split(X, cuts)]
    ref = _ref_longdouble(X)
    _assert_block(_block(column_statistics(seqs)), ref, "%s ratio %g %s" % (np.dtype(dtype).name, ratio, placement))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_standard_scaler_all_nan_column_matches_sklearn(gpu, dtype):
    """A column that is NaN throughout: n_samples_seen_ 0 and NaN mean_ / var_ / scale_ there (mean_ used to be 0.0)."""
    import torch
    from sklearn.preprocessing import StandardScaler as Ref
    from msmbuilder_amd.preprocessing import StandardScaler
    X, _ = _grid_rows(dtype, 1e3, "row0_call")
    X[:, 9] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = Ref().fit(X)
    cuts = np.cumsum(GRID_LENGTHS)[:-1]
    m = StandardScaler().fit([torch.from_numpy(a).cuda() for a in np.split(X, cuts)])
    assert np.isnan(ref.mean_[9]) and ref.n_samples_seen_[9] == 0
    np.testing.assert_array_equal(m.n_samples_seen_, ref.n_samples_seen_)
    for name, rtol in (("mean_", 1e-12), ("var_", 1e-10), ("scale_", 1e-10)):
        a, b = getattr(m, name), getattr(ref, name)
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        np.testing.assert_allclose(a, b, rtol=rtol, atol=1e-12 if name == "mean_" else 0, equal_nan=True, err_msg=name)


@pytest.mark.parametrize("where", ["last_row_of_last_chunk", "second_column_round"])
@pytest.mark.parametrize("value", [float("inf"), float("-inf")])
def test_standard_scaler_inf_flag_at_size(gpu, value, where):
    """One infinity in the last row of the last of 1283 chunks (not its workgroup's first), and one in column 1050 of
    F = 1100 float32 (group 262 >= 256: second g0 round): fit raises scikit-learn's ValueError either way."""
    from msmbuilder_amd.preprocessing import StandardScaler
    if where == "last_row_of_last_chunk":
        X, seqs = _big(np.float32, seed=6)
        StandardScaler().fit(seqs)                       # finite: no error
        seqs[-1][-1, 17] = value
    else:
        X = _randn_rows(3001, 1100, np.float32, 7)
        seqs = list(X.split([1, 1500, 1500]))
        StandardScaler().fit(seqs)
        assert 1050 // 4 >= 256
        seqs[2][777, 1050] = value
    with pytest.raises(ValueError, match="infinity"):
        StandardScaler().fit(seqs)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_colstats_deterministic_and_online(gpu, dtype):
    """Fixed merge order, no atomics: two scans of the same 1.3M rows give the same bits; one fit of all sequences and
    the merge of per-sequence partial_fits agree to the tolerances of the scan."""
    from msmbuilder_amd.preprocessing import column_statistics, StandardScaler
    X, seqs = _big(dtype, seed=8)
    a, b = _block(column_statistics(seqs)), _block(column_statistics(seqs))
    assert a.tobytes() == b.tobytes()
    mo = StandardScaler()
    for s in seqs:
        mo.partial_fit(s)
    ref = _ref_torch(seqs)
    _assert_block(a, ref, "one call")
    _assert_block(mo._stats, ref, "partial_fit per sequence")
    _assert_block(mo._stats, a, "partial_fit against one call")


def test_colstats_two_host_staging_groups(gpu):
    """Host float32 arrays of 700 MiB, 500 MiB and 64 KiB (F = 64, 256-byte rows): the first group takes the 700 MiB
    array alone (700 + 500 MiB > 2^30 bytes), the second the other two, and the host Chan merge joins them."""
    import torch
    from msmbuilder_amd.preprocessing import column_statistics
    F = 64
    rows = (700 * 2 ** 20 // (4 * F), 500 * 2 ** 20 // (4 * F), 256)
    assert rows[0] * 4 * F <= 2 ** 30 < (rows[0] + rows[1]) * 4 * F and (rows[1] + rows[2]) * 4 * F <= 2 ** 30
    rng = np.random.default_rng(12)
    offs = (rng.uniform(-50, 50, F)).astype(np.float32)
    host = []
    for n in rows:
        a = rng.random((n, F), dtype=np.float32)
        a += offs
        host.append(a)
    dev = [torch.from_numpy(a).cuda() for a in host]
    got_host = _block(column_statistics(host))
    got_dev = _block(column_statistics(dev))
    ref = _ref_torch(dev)
    _assert_block(got_dev, ref, "device, one group")
    _assert_block(got_host, ref, "host, two staging groups")
    _assert_block(got_host, got_dev, "host against device")


# ---------------------------------------------------------------------------------------------------------------
# 2. msm_scale_apply
# ---------------------------------------------------------------------------------------------------------------
def _apply_ref(x, shift, scale, mode):
    """Each step computed in float64 and rounded to the array dtype (numpy's in-place `X -= mean; X /= scale`)."""
    y = x
    if mode == 0:
        if shift is not None:
            y = (y.double() - shift).to(x.dtype)
        if scale is not None:
            y = (y.double() / scale).to(x.dtype)
    else:
        if scale is not None:
            y = (y.double() * scale).to(x.dtype)
        if shift is not None:
            y = (y.double() + shift).to(x.dtype)
    return y


def _apply_abi(gpu, x_ptr, nbytes, n, F, ld, shift, scale, mode, out_ptr, ldo):
    import torch
    torch.cuda.synchronize()
    gpu.check(gpu.lib().msm_scale_apply(C.c_void_p(x_ptr), nbytes, n, F, ld,
                                        None if shift is None else C.c_void_p(shift.ctypes.data),
                                        None if scale is None else C.c_void_p(scale.ctypes.data), mode,
                                        C.c_void_p(out_ptr), ldo, 1))


# rows per workgroup = 4 * rl; grid = min(ceil(n / (4 * rl)), 16,384)
#   70,001 x 1100 float32: ngroups 275 -> cpb 256, rl 1: ceil(70,001 / 4) = 17,501 > 16,384 (row grid-stride) and two g0 rounds
#   1,100,003 x 37 float32: ngroups 10 -> cpb 16, rl 16: ceil(1,100,003 / 64) = 17,188 > 16,384, scalar path (37 % 4 != 0)
#   3,001 x 1101 float32: ngroups 276 > 256, scalar path;  3,001 x 600 float64: ngroups 300 > 256, vector path
APPLY_SHAPES = [(np.float32, 70001, 1100), (np.float32, 1100003, 37), (np.float32, 3001, 1101), (np.float64, 3001, 600)]
APPLY_VARIANTS = [(0, True, True), (1, True, True), (0, False, True), (0, True, False), (1, False, True), (1, True, False)]


@pytest.mark.parametrize("mode,with_shift,with_scale", APPLY_VARIANTS)
@pytest.mark.parametrize("dtype,n,F", APPLY_SHAPES)
def test_scale_apply_at_size(gpu, dtype, n, F, mode, with_shift, with_scale):
    import torch
    CW = 16 // np.dtype(dtype).itemsize
    ngroups = -(-F // CW)
    cpb = min(256, 1 << int(np.ceil(np.log2(ngroups))))
    assert (-(-n // (4 * (256 // cpb))) > APPLY_GRID) or ngroups > 256
    x = _randn_rows(n, F, dtype, 20)
    rs = np.random.RandomState(21)
    shift = rs.uniform(-40, 40, F) if with_shift else None
    scale = rs.uniform(0.05, 30, F) if with_scale else None
    out = torch.full_like(x, -7.0)
    _apply_abi(gpu, x.data_ptr(), np.dtype(dtype).itemsize, n, F, F, shift, scale, mode, out.data_ptr(), F)
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    want = _apply_ref(x, dev(shift), dev(scale), mode)
    assert torch.equal(out, want), "%d elements differ" % int((out != want).sum())
    if n <= 4000:                                        # the numpy statement itself, where the case is small
        h = x.cpu().numpy().copy()
        if mode == 0:
            if with_shift:
                h -= shift
            if with_scale:
                h /= scale
        else:
            if with_scale:
                h *= scale
            if with_shift:
                h += shift
        assert h.dtype == dtype and np.array_equal(out.cpu().numpy(), h)


@pytest.mark.parametrize("F,lo,ldo", [(36, 4, 40), (37, 3, 41), (36, 3, 40)])
def test_scale_apply_device_pitch(gpu, F, lo, ldo):
    """Device rows with ld = 48 > F in and ld_out > F out, 70,001 rows: (36, window from column 4, ld_out 40) is the
    vector path (both bases 16-byte aligned, all three of F, ld, ld_out multiples of 4); the other two are scalar
    (F = 37; base 12 bytes off).  The padding columns of the output keep their fill."""
    import torch
    n = 70001
    base = _randn_rows(n, 48, np.float32, 22)
    x = base[:, lo:lo + F]
    rs = np.random.RandomState(23)
    shift, scale = rs.uniform(-40, 40, F), rs.uniform(0.05, 30, F)
    out = torch.full((n, ldo), -7.0, dtype=torch.float32, device="cuda")
    _apply_abi(gpu, x.data_ptr(), 4, n, F, 48, shift, scale, 0, out.data_ptr(), ldo)
    want = _apply_ref(x, torch.from_numpy(shift).cuda(), torch.from_numpy(scale).cuda(), 0)
    assert torch.equal(out[:, :F], want)
    assert bool((out[:, F:] == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------
# 3. order statistics / RobustScaler
# ---------------------------------------------------------------------------------------------------------------
def _key_columns(n, F, dtype, seed):
    """Host rows whose columns carry the key distributions the select has to get right (the rest: scaled normals)."""
    rs = np.random.RandomState(seed)
    X = (rs.randn(n, F) * rs.uniform(1e-3, 1e3, F) - 2).astype(dtype)
    bits = np.uint32 if dtype == np.float32 else np.uint64
    for c in (0, 1, 2):                                   # shared high digits: every later pass counts almost every row
        X[:, c] = 1.0 + 0.001 * rs.rand(n)
    for c, run in ((3, 5000), (4, 977), (5, 20000)):      # piecewise constant, long runs
        X[:, c] = np.repeat(rs.randn(n // run + 1) * 5, run)[:n]
    X[:, 6] = np.where(rs.rand(n) < 0.3, -1.5, 2.25)      # two distinct values
    sub = rs.randint(0, 1 << 20, n).astype(bits)          # denormals of both signs ...
    sub |= (rs.randint(0, 2, n).astype(bits) << bits(8 * np.dtype(dtype).itemsize - 1))
    X[:, 7] = sub.view(dtype)
    X[:, 8] = sub[::-1].view(dtype)
    z = rs.randint(0, 4, n)
    X[z == 0, 8] = 0.0                                    # ... with +0.0 and -0.0 mixed in
    X[z == 1, 8] = -0.0
    X[rs.randint(0, n, 50), 9] = np.inf                   # infinities are ordinary keys here
    X[rs.randint(0, n, 50), 9] = -np.inf
    X[rs.randint(0, n, 500), 10] = np.copysign(np.nan, -1)   # NaNs with the sign bit set are still missing values
    X[rs.randint(0, n, 500), 10] = np.nan
    X[rs.randint(0, n, 30), 11] = np.copysign(np.nan, -1)
    return X


def _rank_sets(n_valid, rs):
    F = len(n_valid)
    q = lambda t: np.minimum((n_valid * t).astype(np.int64), n_valid - 1)
    return {
        "one": np.stack([n_valid // 2]),
        "eight_spread": np.stack([q(t) for t in (0.01, 0.13, 0.25, 0.5, 0.5000001, 0.75, 0.9, 0.999)]),
        "per_column": np.stack([(rs.rand(F) * n_valid).astype(np.int64) for _ in range(5)]),   # distinct prefixes vary by column
        "ends_and_negative": np.stack([np.zeros(F, np.int64), n_valid - 1, np.full(F, -1), np.full(F, -5)]),
    }


@pytest.mark.parametrize("ranks", ["one", "eight_spread", "per_column", "ends_and_negative"])
@pytest.mark.parametrize("dtype,F", [(np.float64, 21), (np.float64, 33), (np.float32, 21)])
def test_order_statistics_key_distributions(gpu, dtype, F, ranks):
    """200,003 rows (49 chunks of 4096) x 21 / 33 columns: ntile = 2 / 3 with a last tile of 5 / 1 columns."""
    import torch
    from msmbuilder_amd.preprocessing import column_order_statistics
    n = 200003
    assert F % DCOLS in (5, 1)
    X = _key_columns(n, F, dtype, 30)
    srt = np.sort(X, axis=0)                              # NaN (either sign) sorts last
    n_valid = (~np.isnan(X)).sum(0)
    rk = _rank_sets(n_valid, np.random.RandomState(31))[ranks]
    Xd = torch.from_numpy(X).cuda()
    got = column_order_statistics(list(Xd.split([1, 4095, 4097, n - 8193])), rk)
    assert got.dtype == dtype and got.shape == rk.shape
    for r in range(len(rk)):
        if rk[r][0] < 0:
            assert np.isnan(got[r]).all()
        else:
            want = srt[rk[r], np.arange(F)]
            assert not np.isnan(want).any()
            assert np.array_equal(got[r], want), (r, np.nonzero(got[r] != want)[0])


def test_order_statistics_32_tiles_several_chunks_per_part(gpu):
    """300,001 x 512 float32: ntile = 512 / 16 = 32, 74 chunks of 4096 rows, nparts = min(74, 2 * CUs / 32) = 16 on 256 CUs
    (nparts < 74 for any CU count below 1184): every part loops over 4 or 5 chunks."""
    import torch
    from msmbuilder_amd.preprocessing import column_order_statistics
    n, F = 300001, 512
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert F // DCOLS >= 32 and max(1, min(_nchunks([n], DIGIT_ROWS), 2 * cus // (F // DCOLS))) < _nchunks([n], DIGIT_ROWS)
    X = _randn_rows(n, F, np.float32, 32)
    g = torch.Generator(device="cuda")
    g.manual_seed(33)
    X[:, :8] = 1.0 + 0.001 * torch.rand(n, 8, generator=g, device="cuda")
    X[:, 8:12] = torch.randn(n // 3000 + 1, 4, generator=g, device="cuda").repeat_interleave(3000, 0)[:n]
    X[::1001, 12] = float("nan")
    n_valid = (~torch.isnan(X)).sum(0).cpu().numpy()
    rk = _rank_sets(n_valid, np.random.RandomState(34))
    rk = np.concatenate([rk["eight_spread"], rk["ends_and_negative"][:2]])
    got = column_order_statistics(list(X.split([100000, 1, 200000])), rk)
    srt = torch.sort(X, dim=0).values                     # NaN sorts last
    want = srt.gather(0, torch.from_numpy(rk).cuda()).cpu().numpy()
    assert not np.isnan(want).any() and np.array_equal(got, want)


def test_order_statistics_one_part(gpu):
    """nparts = max(1, min(nchunks, 2 * CUs / ntile)) = 1 needs ntile > 2 * CUs: F = 16 * (2 * CUs + 1) = 8208 columns on
    256 CUs, computed from the device here.  9,001 rows = 3 chunks, all taken by part 0 (`c += nparts` with nparts = 1);
    col_digit_kernel then runs ceil(2052 / 256) = 9 column rounds."""
    import torch
    from msmbuilder_amd.preprocessing import column_order_statistics
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    F = DCOLS * (2 * cus + 1)
    assert (2 * cus) // (F // DCOLS) < 1 and F // 4 > 256
    n = 9001
    X = _randn_rows(n, F, np.float32, 35)
    X[::7, F - 1] = float("nan")
    n_valid = (~torch.isnan(X)).sum(0).cpu().numpy()
    rk = np.stack([n_valid // 2, np.minimum(n_valid - 1, (np.arange(F) * 37) % n)])
    got = column_order_statistics([X[:5000], X[5000:]], rk)
    want = torch.sort(X, dim=0).values.gather(0, torch.from_numpy(rk).cuda()).cpu().numpy()
    assert not np.isnan(want).any() and np.array_equal(got, want)


def test_robust_scaler_device_rows_match_sklearn(gpu):
    import torch
    from sklearn.preprocessing import RobustScaler as Ref
    from msmbuilder_amd.preprocessing import RobustScaler
    X = _randn_rows(300000, 64, np.float32, 36)
    X[::5003, 3] = float("nan")
    m = RobustScaler().fit(list(X.split([1, 99999, 200000])))
    ref = Ref().fit(X.cpu().numpy())
    assert m.center_.dtype == ref.center_.dtype and np.array_equal(m.center_, ref.center_)
    assert m.scale_.dtype == ref.scale_.dtype and np.array_equal(m.scale_, ref.scale_)
