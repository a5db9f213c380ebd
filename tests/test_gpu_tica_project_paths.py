"""Every path of the tICA projection against an exact reference: the two kernels of csrc/tica_project_dev.h
(tica_project_mfma_kernel on the fp64 matrix pipe, tica_project_kernel with a lane per row, with and without vector loads),
the three C entry points (msm_tica_project, msm_tica_project_batch, msm_tica_project_host_list) and the dispatch of
tICA.transform.  Each result is compared with (X - mean) . V^T in np.longdouble and must lie inside the DERIVED bound of
tests/tica_project_ref.py (project_bound: (F + 8) 2^-53 (|X| |V|^T + |mean| |V|^T); tests/test_tica_project_ref.py shows
that a plain float64 evaluation meets it on these inputs and that three wrong ones do not).  Each test asks
msm_tica_project_plan which kernel its rows take and asserts that it is the one the test names.

Out of scope: a FINITE input whose projection overflows.  The two kernels differ on it by design -- the fp64-MFMA kernel
applies the finite check to its outputs and reports the overflow, the lane-per-row kernel checks its inputs and does not."""
import ctypes as C
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tica_project_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 1.2345678e300                       # what every output buffer holds before a call, two guard rows behind it included
SENT_BITS = np.float64(SENT).view(np.int64)
GUARD = 2


# ------------------------------------------------------------------ helpers
@pytest.fixture()
def L(gpu):
    import torch
    gpu.set_stream(torch.cuda.current_stream().cuda_stream)
    return gpu.lib()


def to_dev(X):
    """The stored rows on the device (bfloat16 from its raw words), contiguous."""
    import torch
    X = np.ascontiguousarray(X)
    if X.dtype == np.uint16:
        return torch.from_numpy(X.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(X).cuda()


def plan(L, nbytes, F, ld, ptr):
    kernel, vec = C.c_int(-1), C.c_int(-1)
    assert L.msm_tica_project_plan(nbytes, F, ld, int(ptr % 16 == 0), C.byref(kernel), C.byref(vec)) == 0
    return kernel.value, vec.value


def last_stats(L):
    out = (C.c_int64 * 2)()
    assert L.msm_tica_project_last_stats(out) == 0
    return int(out[0]), int(out[1])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def fresh_out(n, k):
    import torch
    return torch.full((n + GUARD, k), SENT, dtype=torch.float64, device="cuda")


def read_out(out, n):
    """The n result rows of a device output buffer; its guard rows must still hold the sentinel."""
    got = out.cpu().numpy()
    assert np.all(bits(got[n:]) == SENT_BITS), "rows behind the output were written"
    return got[:n]


def project(L, ptr, nbytes, n, F, ld, mean, V, check_finite=1):
    """msm_tica_project on device rows at `ptr`: (rc, result rows)."""
    k = V.shape[0]
    out = fresh_out(n, k)
    rc = L.msm_tica_project(C.c_void_p(ptr), nbytes, n, F, ld, mean.ctypes.data, V.ctypes.data, k, C.c_void_p(out.data_ptr()), 1,
                            check_finite)
    return rc, read_out(out, n)


def assert_within(got, X, mean, V, what):
    ok, worst = R.within(got, X, mean, V)
    assert ok, "%s: error / bound = %.3g" % (what, worst)
    return worst


def poisoned_view(X, ld, dt):
    """(device tensor, pointer of the view's first row): X inside a larger tensor whose padding columns F .. ld - 1, whole
    row before the view and whole row after it alternate NaN with +-Inf."""
    n, F = X.shape
    big = R.poison_like((n + 2, ld), dt)
    big[1:n + 1, :F] = X
    t = to_dev(big)
    return t, t.data_ptr() + ld * R.NBYTES[dt]


def strided_against_contiguous(L, dt, shapes, pad, kernel, family="plain"):
    nb = R.NBYTES[dt]
    worst = 0.0
    for n, F, k in shapes:
        X, mean, V = R.make_case(family, n, F, k, dt)
        ld = F + pad
        keep, ptr = poisoned_view(X, ld, dt)
        assert plan(L, nb, F, ld, ptr)[0] == kernel, (n, F, k)
        rc, got = project(L, ptr, nb, n, F, ld, mean, V)
        assert rc == 0, (n, F, k, ld)
        worst = max(worst, assert_within(got, X, mean, V, "strided rows %r ld %d" % ((n, F, k), ld)))
        Xc = to_dev(X)
        rc, gotc = project(L, Xc.data_ptr(), nb, n, F, F, mean, V)
        assert rc == 0
        assert_within(gotc, X, mean, V, "contiguous rows %r" % ((n, F, k),))
        if plan(L, nb, F, F, Xc.data_ptr())[0] == kernel:
            assert np.array_equal(bits(got), bits(gotc)), "stride changes the result %r" % ((n, F, k),)
    print("%s kernel %d: worst error / bound %.3f over %d shapes" % (dt, kernel, worst, len(shapes)))


# ------------------------------------------------------------------ row strides on the device
@pytest.mark.parametrize("dt", R.DTYPES)
def test_mfma_kernel_poisoned_stride(L, dt):
    """ld = F + one vector: 1 .. 4 chunks of 128 bytes with and without a partial last one, rows on both sides of the wave
    (64) and tile (256) seams, components on both sides of the 16-wide panels.  The clamped padding lanes, the re-read
    last 16 bytes of a partial chunk and the 32-bit offsets must never reach a padding column or a neighbouring row."""
    strided_against_contiguous(L, dt, R.mfma_shapes(dt), R.CW[dt], R.PJ_MFMA)


@pytest.mark.parametrize("dt", R.DTYPES)
def test_row_kernel_poisoned_stride(L, dt):
    """ld = F + 1 (never whole vectors): the lane-per-row kernel element by element, at the 64-feature chunk, 128-row
    workgroup and NPW / KT component seams."""
    strided_against_contiguous(L, dt, R.rows_shapes(), 1, R.PJ_ROWS)


@pytest.mark.parametrize("dt", R.DTYPES)
def test_misaligned_base_takes_the_row_kernel(L, dt):
    """Whole-vector rows (F % cw == 0) that start one element past a 16-byte boundary."""
    nb = R.NBYTES[dt]
    n, F, k = R.MISALIGNED_SHAPE[dt]
    assert F % R.CW[dt] == 0
    X, mean, V = R.make_case("plain", n, F, k, dt)
    flat = R.poison_like((n * F + 2 * R.CW[dt],), dt)
    flat[1:1 + n * F] = X.reshape(-1)
    t = to_dev(flat)
    ptr = t.data_ptr() + nb
    assert t.data_ptr() % 16 == 0 and plan(L, nb, F, F, ptr) == (R.PJ_ROWS, 0)
    rc, got = project(L, ptr, nb, n, F, F, mean, V)
    assert rc == 0
    assert_within(got, X, mean, V, "misaligned rows")


@pytest.mark.parametrize("dt", R.DTYPES)
def test_host_rows_with_a_stride(L, dt):
    """Host rows at ld > F take the 2-D copy into a contiguous staging buffer: poisoned padding must stay behind, at a width
    for each kernel."""
    nb = R.NBYTES[dt]
    n, k = R.HOST_STRIDED_N, R.HOST_STRIDED_K
    for F, kernel in ((R.BATCH_F[dt], R.PJ_MFMA), (R.BATCH_F[dt] - 1, R.PJ_ROWS)):
        assert plan(L, nb, F, F, 0)[0] == kernel           # the staging buffer is aligned and contiguous
        X, mean, V = R.make_case("plain", n, F, k, dt)
        for ld in (F + 1, F + R.CW[dt]):
            big = R.poison_like((n + 2, ld), dt)
            big[1:n + 1, :F] = X
            out = np.full((n + GUARD, k), SENT)
            rc = L.msm_tica_project(C.c_void_p(big.ctypes.data + ld * nb), nb, n, F, ld, mean.ctypes.data, V.ctypes.data, k,
                                    C.c_void_p(out.ctypes.data), 0, 1)
            assert rc == 0, (F, ld)
            assert np.all(bits(out[n:]) == SENT_BITS)
            assert_within(out[:n], X, mean, V, "host rows F %d ld %d" % (F, ld))
            outc = np.full((n, k), SENT)
            Xc = np.ascontiguousarray(X)
            assert L.msm_tica_project(C.c_void_p(Xc.ctypes.data), nb, n, F, F, mean.ctypes.data, V.ctypes.data, k,
                                      C.c_void_p(outc.ctypes.data), 0, 1) == 0
            assert np.array_equal(bits(out[:n]), bits(outc))


# ------------------------------------------------------------------ the 2^32-byte tile limit
def _wide_rows(X, n, ld, dt):
    """n rows at stride ld on the device, only the F used columns written."""
    import torch
    tdt = {"bf16": torch.bfloat16, "f32": torch.float32, "f64": torch.float64}[dt]
    t = torch.empty((n, ld), dtype=tdt, device="cuda")
    t[:, :X.shape[1]] = to_dev(X)
    return t


@pytest.mark.parametrize("dt", R.DTYPES)
def test_rows_of_16_mib_take_the_row_kernel_with_vector_loads(L, dt):
    """From 256 * ld * dtype_bytes = 2^32 on the fp64-MFMA kernel's 32-bit offsets would wrap: three rows at exactly that
    stride run the `vec` branch of the lane-per-row kernel (a partial 64-feature chunk)."""
    nb = R.NBYTES[dt]
    n, F, k = 3, R.WIDE_F[dt], 17
    ld = R.stride_limit(nb)
    X, mean, V = R.make_case("plain", n, F, k, dt)
    t = _wide_rows(X, n, ld, dt)
    assert plan(L, nb, F, ld, t.data_ptr()) == (R.PJ_ROWS, 1)
    rc, got = project(L, t.data_ptr(), nb, n, F, ld, mean, V)
    assert rc == 0
    assert_within(got, X, mean, V, "16 MiB rows")
    Xc = to_dev(X)
    rc, gotc = project(L, Xc.data_ptr(), nb, n, F, F, mean, V)            # (fp64-MFMA kernel: another order of the sum)
    assert rc == 0
    assert_within(gotc, X, mean, V, "the same rows, contiguous")


def test_largest_row_offset_of_the_mfma_kernel(L):
    """One vector below the limit with a full tile of 256 rows: the last row's byte offset, 255 * (16 MiB - 16), is the
    largest the fp64-MFMA kernel forms.  About 4 GiB of address space, of which only the used columns are written."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 16 << 30:
        pytest.skip("needs 4 GiB of device address space; %.1f GiB free is under the 16 GiB this test asks for" % (free / 2.0 ** 30))
    dt, nb = "f32", 4
    n, F, k = 256, R.WIDE_F[dt], 17
    ld = R.stride_limit(nb) - R.CW[dt]
    X, mean, V = R.make_case("plain", n, F, k, dt)
    t = _wide_rows(X, n, ld, dt)
    try:
        assert plan(L, nb, F, ld, t.data_ptr()) == (R.PJ_MFMA, 1)
        rc, got = project(L, t.data_ptr(), nb, n, F, ld, mean, V)
        assert rc == 0
        assert_within(got, X, mean, V, "rows one vector below the limit")
        Xc = to_dev(X)
        rc, gotc = project(L, Xc.data_ptr(), nb, n, F, F, mean, V)
        assert rc == 0 and np.array_equal(bits(got), bits(gotc))
    finally:
        del t
        torch.cuda.empty_cache()


# ------------------------------------------------------------------ the tile table
def _batch(L, tensors, lens, nb, F, mean, V, ptrs=None, check_finite=1):
    """msm_tica_project_batch on separately allocated trajectories: (rc, [result rows per trajectory]); every output
    has its guard rows and starts as sentinel."""
    k, n = V.shape[0], len(lens)
    outs = [fresh_out(m, k) for m in lens]
    if ptrs is None:
        ptrs = [t.data_ptr() if m else None for t, m in zip(tensors, lens)]
    xp = (C.c_void_p * n)(*ptrs)
    op = (C.c_void_p * n)(*[o.data_ptr() for o in outs])
    rows = (C.c_int64 * n)(*lens)
    rc = L.msm_tica_project_batch(xp, op, rows, n, nb, F, mean.ctypes.data, V.ctypes.data, k, check_finite)
    return rc, [read_out(o, m) for o, m in zip(outs, lens)]


def _cut(X, lens):
    ends = np.cumsum(lens)
    return [np.ascontiguousarray(X[e - m:e]) for e, m in zip(ends, lens)]


@pytest.mark.parametrize("dt", R.DTYPES)
def test_tile_table_direct(L, dt):
    """Tiles at r * k for every block of 16 components (ktot / kbase), every output row written once and nothing else."""
    nb, F, lens = R.NBYTES[dt], R.BATCH_F[dt], list(R.BATCH_LENS)
    for k in R.MFMA_K:
        X, mean, V = R.make_case("plain", sum(lens), F, k, dt)
        parts = _cut(X, lens)
        tensors = [to_dev(p) for p in parts]
        assert all(t.data_ptr() % 16 == 0 for t in tensors)
        rc, gots = _batch(L, tensors, lens, nb, F, mean, V)
        assert rc == 0
        assert last_stats(L)[1] == len(R.tiles_ref(lens)) == 10
        for s, (p, g) in enumerate(zip(parts, gots)):
            if len(p):
                assert_within(g, p, mean, V, "trajectory %d of the batch, k = %d" % (s, k))
        rc1, one = project(L, tensors[-1].data_ptr(), nb, lens[-1], F, F, mean, V)      # the same kernel, called alone
        assert rc1 == 0 and np.array_equal(bits(one), bits(gots[-1]))


@pytest.mark.parametrize("dt", R.DTYPES)
def test_batch_refusals_write_nothing(L, dt):
    """A misaligned pointer (the LAST trajectory's) and rows that are not whole vectors: MSM_ERR_INVALID before any launch."""
    import torch
    from msmbuilder_amd import _lib
    nb, F, lens, k = R.NBYTES[dt], R.BATCH_F[dt], list(R.BATCH_LENS), 17
    X, mean, V = R.make_case("plain", sum(lens), F, k, dt)
    parts = _cut(X, lens)
    tensors = [to_dev(p) for p in parts]
    shifted = to_dev(np.concatenate([parts[-1].reshape(-1)[:1], parts[-1].reshape(-1)]))
    ptrs = [t.data_ptr() if m else None for t, m in zip(tensors, lens)]
    ptrs[-1] = shifted.data_ptr() + nb
    rc, gots = _batch(L, tensors, lens, nb, F, mean, V, ptrs=ptrs)
    assert rc == _lib.MSM_ERR_INVALID and last_stats(L)[1] == 0
    assert all(np.all(bits(g) == SENT_BITS) for g in gots)
    Xn, meann, Vn = R.make_case("plain", sum(lens), F - 1, k, dt)
    tensors = [to_dev(p) for p in _cut(Xn, lens)]
    rc, gots = _batch(L, tensors, lens, nb, F - 1, meann, Vn)
    assert rc == _lib.MSM_ERR_INVALID and last_stats(L)[1] == 0
    assert all(np.all(bits(g) == SENT_BITS) for g in gots)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the host list's groups
def _host_list(L, parts, nb, F, mean, V, check_finite=1):
    k, n = V.shape[0], len(parts)
    lens = [len(p) for p in parts]
    out = np.full((sum(lens) + GUARD, k), SENT)
    xp = (C.c_void_p * n)(*[p.ctypes.data if len(p) else None for p in parts])
    rows = (C.c_int64 * n)(*lens)
    rc = L.msm_tica_project_host_list(xp, rows, n, nb, F, mean.ctypes.data, V.ctypes.data, k, C.c_void_p(out.ctypes.data),
                                      check_finite)
    assert np.all(bits(out[sum(lens):]) == SENT_BITS)
    return rc, out[:sum(lens)]


@pytest.mark.parametrize("dt,which", [("f32", 0), ("f32", 1), ("f64", 0), ("f64", 1)])
def test_host_list_group_seams(L, monkeypatch, dt, which):
    """MSM_TICA_PROJ_GROUP_BYTES at 300 rows cuts the ragged list into four groups -- both halves of the staging buffer used
    twice, the event wait from the third group on, a trajectory larger than the budget, empties on both sides of a
    boundary and behind the last rows -- and the result is the one group's, row for row."""
    from msmbuilder_amd import _lib
    nb, F, k = R.NBYTES[dt], R.GROUP_F[dt][which], 5
    lens = list(R.GROUP_LENS)
    assert plan(L, nb, F, F, 0)[0] == (R.PJ_MFMA, R.PJ_ROWS)[which]
    X, mean, V = R.make_case("plain", sum(lens), F, k, dt)
    parts = _cut(X, lens)
    budget = R.GROUP_BUDGET_ROWS * F * nb
    want_groups = R.groups_ref(lens, F * nb, budget)
    assert len(want_groups) >= 4 and (4, 5) in want_groups

    monkeypatch.delenv("MSM_TICA_PROJ_GROUP_BYTES", raising=False)
    rc, whole = _host_list(L, parts, nb, F, mean, V)
    assert rc == 0 and last_stats(L)[0] == 1
    assert_within(whole, X, mean, V, "one group")
    monkeypatch.setenv("MSM_TICA_PROJ_GROUP_BYTES", "-%d" % budget)        # not positive: the default
    rc, again = _host_list(L, parts, nb, F, mean, V)
    assert rc == 0 and last_stats(L)[0] == 1 and np.array_equal(bits(again), bits(whole))

    monkeypatch.setenv("MSM_TICA_PROJ_GROUP_BYTES", str(budget))
    rc, got = _host_list(L, parts, nb, F, mean, V)
    assert rc == 0 and last_stats(L)[0] == len(want_groups)
    assert_within(got, X, mean, V, "four groups")
    assert np.array_equal(bits(got), bits(whole))

    tail = [parts[4], parts[5]]                                            # [700, 0]: the last group holds no row
    assert R.groups_ref([700, 0], F * nb, budget) == [(0, 1), (1, 2)]
    rc, got2 = _host_list(L, tail, nb, F, mean, V)
    assert rc == 0 and last_stats(L)[0] == 2
    assert np.array_equal(bits(got2), bits(whole[301:1001]))

    for s in (7, 0):                                                       # an Inf in the last group, in the first
        bad = [p.copy() for p in parts]
        bad[s][len(bad[s]) // 2, F - 1] = np.inf
        rc, _ = _host_list(L, bad, nb, F, mean, V)
        assert rc == _lib.MSM_ERR_NONFINITE, s
        rc, clean = _host_list(L, parts, nb, F, mean, V)
        assert rc == 0 and np.array_equal(bits(clean), bits(whole))


# ------------------------------------------------------------------ non-finite values
@pytest.mark.parametrize("dt", R.DTYPES)
def test_nonfinite_value_stays_in_its_row(L, dt):
    """check_finite = 0: a NaN / Inf in one row -- first or last feature; row 0, the rows on both sides of a 256-row tile,
    the last row, which the fp64-MFMA kernel's padding lanes re-read -- changes that row only.  check_finite = 1 reports it
    from both kernels, also where the matrix's column of that feature is zero (`sparseV`)."""
    from msmbuilder_amd import _lib
    nb, n, k = R.NBYTES[dt], R.CONTAIN_N, 5
    bad_values = [0x7f80, 0xff80, 0x7fc0] if dt == "bf16" else [np.nan, np.inf, -np.inf]
    for F, kernel in ((R.BATCH_F[dt], R.PJ_MFMA), (R.BATCH_F[dt] - 1, R.PJ_ROWS)):
        for family in ("sparseV", "plain"):
            X, mean, V = R.make_case(family, n, F, k, dt)
            if family == "sparseV":
                assert not V[:, 0].any() and not V[:, F - 1].any()
            t = to_dev(X)
            assert plan(L, nb, F, F, t.data_ptr())[0] == kernel
            rc, clean = project(L, t.data_ptr(), nb, n, F, F, mean, V, check_finite=0)
            assert rc == 0
            assert_within(clean, X, mean, V, "clean rows")
            i = 0
            for row in (0, 255, 256, n - 1):
                for col in (0, F - 1):
                    Xb = X.copy()
                    Xb[row, col] = bad_values[i % 3]
                    i += 1
                    tb = to_dev(Xb)
                    rc, got = project(L, tb.data_ptr(), nb, n, F, F, mean, V, check_finite=0)
                    assert rc == 0, (F, family, row, col)
                    others = np.arange(n) != row
                    assert np.array_equal(bits(got[others]), bits(clean[others])), (F, family, row, col)
                    assert not np.isfinite(got[row]).any(), (F, family, row, col)
                    rc, _ = project(L, tb.data_ptr(), nb, n, F, F, mean, V, check_finite=1)
                    assert rc == _lib.MSM_ERR_NONFINITE, (F, family, row, col)
            rc, after = project(L, t.data_ptr(), nb, n, F, F, mean, V, check_finite=1)
            assert rc == 0 and np.array_equal(bits(after), bits(clean))


# ------------------------------------------------------------------ cancellation
@pytest.mark.parametrize("dt", R.DTYPES)
def test_offset_family_through_both_kernels_and_the_batch(L, dt):
    """X . V^T - mean . V^T where the two agree in their leading digits: the bound scales with the TERMS, so the kernels may
    not lose more than a float64 evaluation does."""
    nb = R.NBYTES[dt]
    for (n, F, k), kernel in zip(R.CANCEL_SHAPES[dt], (R.PJ_MFMA, R.PJ_ROWS)):
        X, mean, V = R.make_case("offset", n, F, k, dt)
        t = to_dev(X)
        assert plan(L, nb, F, F, t.data_ptr())[0] == kernel
        rc, got = project(L, t.data_ptr(), nb, n, F, F, mean, V)
        assert rc == 0
        w = assert_within(got, X, mean, V, "offset rows %r" % ((n, F, k),))
        print("%s offset %r: error / bound %.3f" % (dt, (n, F, k), w))
    F, lens, k = R.BATCH_F[dt], list(R.BATCH_LENS), 17
    X, mean, V = R.make_case("offset", sum(lens), F, k, dt)
    parts = _cut(X, lens)
    rc, gots = _batch(L, [to_dev(p) for p in parts], lens, nb, F, mean, V)
    assert rc == 0
    for p, g in zip(parts, gots):
        if len(p):
            assert_within(g, p, mean, V, "offset rows through the batch")


# ------------------------------------------------------------------ the narrowest rows through the tile table
def test_batch_two_component_blocks_at_four_features(L):
    """The batch entry at the smallest width that is whole 16-byte vectors (4 float32 features) with k = 17, two blocks of
    components, on trajectories of 1, 255 and 257 rows: the tile table uploads no k x F components, and its flag sits right
    behind the k means."""
    nb, F, k, lens = 4, 4, 17, [1, 255, 257]
    X, mean, V = R.make_case("plain", sum(lens), F, k, "f32")
    parts = _cut(X, lens)
    tensors = [to_dev(p) for p in parts]
    rc, gots = _batch(L, tensors, lens, nb, F, mean, V)
    assert rc == 0 and last_stats(L)[1] == len(R.tiles_ref(lens)) == 4
    for s, (p, t, g) in enumerate(zip(parts, tensors, gots)):
        assert_within(g, p, mean, V, "trajectory %d of %r rows, 4 features" % (s, lens))
        rc1, one = project(L, t.data_ptr(), nb, len(p), F, F, mean, V)
        assert rc1 == 0 and np.array_equal(bits(one), bits(g))
    bad = parts[2].copy()
    bad[256, 3] = np.inf
    rc, _ = _batch(L, tensors[:2] + [to_dev(bad)], lens, nb, F, mean, V)
    from msmbuilder_amd import _lib
    assert rc == _lib.MSM_ERR_NONFINITE
    rc, again = _batch(L, tensors, lens, nb, F, mean, V)
    assert rc == 0 and all(np.array_equal(bits(a), bits(g)) for a, g in zip(again, gots))


# ------------------------------------------------------------------ argument checks
def test_entries_refuse_bad_arguments_with_their_own_messages(L):
    """The argument checks of the three entries: MSM_ERR_INVALID before any device work, each entry named in its null-pointer
    message, bfloat16 rows (dtype_bytes 2) refused by the host list alone, and no rows at all is not an error."""
    from msmbuilder_amd import _lib
    F, k, n = 4, 2, 3
    X = np.zeros((n, F), np.float32)
    mean, V, out = np.zeros(F), np.zeros((k, F)), np.full((n, k), SENT)
    xp, op, rows = (C.c_void_p * 1)(X.ctypes.data), (C.c_void_p * 1)(out.ctypes.data), (C.c_int64 * 1)(n)
    m, v, o = mean.ctypes.data, V.ctypes.data, C.c_void_p(out.ctypes.data)
    x = C.c_void_p(X.ctypes.data)

    def refused(rc, message):
        assert rc == _lib.MSM_ERR_INVALID and _lib.last_error() == message, (rc, _lib.last_error())

    refused(L.msm_tica_project(None, 4, n, F, F, m, v, k, o, 0, 1), "msm_tica_project: null pointer")
    refused(L.msm_tica_project(x, 4, n, F, F, m, None, k, o, 0, 1), "msm_tica_project: null pointer")
    refused(L.msm_tica_project(x, 3, n, F, F, m, v, k, o, 0, 1), "dtype_bytes must be 2 (bfloat16), 4 or 8")
    for shape in ((-1, F, F, k), (n, 0, F, k), (n, F, F - 1, k), (n, F, F, 0)):
        refused(L.msm_tica_project(x, 4, shape[0], shape[1], shape[2], m, v, shape[3], o, 0, 1), "bad shape")
    assert L.msm_tica_project(x, 4, 0, F, F, m, v, k, o, 0, 1) == 0

    refused(L.msm_tica_project_host_list(None, rows, 1, 4, F, m, v, k, o, 1), "msm_tica_project_host_list: null pointer")
    refused(L.msm_tica_project_host_list(xp, rows, 1, 4, F, m, v, k, None, 1), "msm_tica_project_host_list: null pointer")
    refused(L.msm_tica_project_host_list(xp, rows, 1, 2, F, m, v, k, o, 1), "dtype_bytes must be 4 or 8")
    for shape in ((-1, F, k), (1, 0, k), (1, F, 0)):
        refused(L.msm_tica_project_host_list(xp, rows, shape[0], 4, shape[1], m, v, shape[2], o, 1), "bad shape")
    assert L.msm_tica_project_host_list(xp, rows, 0, 4, F, m, v, k, o, 1) == 0

    refused(L.msm_tica_project_batch(xp, None, rows, 1, 4, F, m, v, k, 1), "msm_tica_project_batch: null pointer")
    refused(L.msm_tica_project_batch(xp, op, rows, 1, 4, F, None, v, k, 1), "msm_tica_project_batch: null pointer")
    refused(L.msm_tica_project_batch(xp, op, rows, 1, 16, F, m, v, k, 1), "dtype_bytes must be 2 (bfloat16), 4 or 8")
    for shape in ((-1, F, k), (1, 0, k), (1, F, 0)):
        refused(L.msm_tica_project_batch(xp, op, rows, shape[0], 4, shape[1], m, v, shape[2], 1), "bad shape")
    assert L.msm_tica_project_batch(xp, op, rows, 0, 4, F, m, v, k, 1) == 0
    assert np.all(bits(out) == SENT_BITS)


# ------------------------------------------------------------------ tICA.transform
def test_transform_routes(L):
    """The dispatch of tICA.transform: lists that must fall back to a call per trajectory (mixed dtypes, a misaligned device
    view, a non-contiguous numpy trajectory), the joined view of back-to-back trajectories, and the two list entries --
    rows inside the bound and the input's container type from every route."""
    import torch
    from msmbuilder_amd import _lib, tICA
    F, k = 36, 3
    rs = np.random.RandomState(11)
    fit_rows = (rs.randn(600, F).cumsum(0) * 0.05 + rs.randn(600, F)).astype(np.float32)
    model = tICA(n_components=k, lag_time=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.fit([fit_rows])
    mean, V = model._projection()
    assert V.shape == (k, F)

    def rows(n, dt, seed):
        return R.make_case("plain", n, F, k, dt, seed=seed)[0]

    def check(outs, stored, device):
        assert isinstance(outs, list) and len(outs) == len(stored)
        for o, X in zip(outs, stored):
            if device:
                assert isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.float64
                o = o.cpu().numpy()
            else:
                assert isinstance(o, np.ndarray) and o.dtype == np.float64
            assert o.shape == (len(X), k)
            assert_within(o, X, mean, V, "transform")

    def falls_back(seqs):
        return (_lib.adjacent_view(seqs) is None and model._transform_device_list(seqs) is None
                and model._transform_host_list(seqs) is None)

    # mixed dtypes, on the device and on the host
    stored = [rows(100, "bf16", 1), rows(57, "f32", 2), rows(300, "f64", 3)]
    seqs = [to_dev(X) for X in stored]
    assert falls_back(seqs)
    check(model.transform(seqs), stored, True)
    assert falls_back(stored[1:])
    check(model.transform(stored[1:]), stored[1:], False)
    # a misaligned device view in the list
    stored = [rows(100, "f32", 4), rows(129, "f32", 5)]
    flat = to_dev(np.concatenate([stored[1].reshape(-1)[:1], stored[1].reshape(-1)]))
    view = flat[1:].view(129, F)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    seqs = [to_dev(stored[0]), view]
    assert falls_back(seqs)
    check(model.transform(seqs), stored, True)
    # a non-contiguous numpy trajectory
    wide = R.poison_like((129, F + 3), "f32")
    wide[:, :F] = stored[1]
    seqs = [stored[0], wide[:, :F]]
    assert not seqs[1].flags.c_contiguous and falls_back(seqs)
    check(model.transform(seqs), stored, False)
    # back-to-back views: the joined route, device and host
    joined = rows(3 * 70, "f32", 6)
    stored = [joined[0:70], joined[70:140], joined[140:210]]
    seqs = list(to_dev(joined).view(3, 70, F).unbind(0))
    assert _lib.adjacent_view(seqs) is not None
    check(model.transform(seqs), stored, True)
    seqs = np.split(joined, 3)
    assert _lib.adjacent_view(seqs) is not None
    check(model.transform(seqs), stored, False)
    # separately allocated trajectories: the batch entry and the host list
    stored = [rows(257, "f32", 7), rows(0, "f32", 8), rows(31, "f32", 9)]
    seqs = [to_dev(X) for X in stored]
    assert _lib.adjacent_view(seqs) is None and model._transform_device_list(seqs) is not None
    check(model.transform(seqs), stored, True)
    assert _lib.adjacent_view(stored) is None and model._transform_host_list(stored) is not None
    check(model.transform(stored), stored, False)
