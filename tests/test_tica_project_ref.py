"""CPU tier of the tICA projection: the library's one dispatch (msm_tica_project_plan: needs no device) against the dispatch
restated in tests/tica_project_ref.py; the restated tile table and host-list grouping against cases written out by hand;
and the yardstick of tests/test_gpu_tica_project_paths.py checked on itself -- a plain float64 numpy evaluation stays
inside `project_bound` on every input of the GPU module, and three wrong evaluations do not."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tica_project_ref as R  # noqa: E402


def library_plan(dtype_bytes, F, ld, aligned16):
    from msmbuilder_amd import _lib
    kernel, vec = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.check(_lib.lib().msm_tica_project_plan(dtype_bytes, F, ld, int(aligned16), ctypes.byref(kernel), ctypes.byref(vec)))
    return kernel.value, vec.value


def test_library_plan_equals_the_restated_dispatch():
    from msmbuilder_amd import _lib
    assert (_lib.MSM_PJ_MFMA, _lib.MSM_PJ_ROWS) == (R.PJ_MFMA, R.PJ_ROWS)
    checked, seen = 0, set()
    for nbytes in (2, 4, 8):
        cw, lim = 16 // nbytes, R.stride_limit(nbytes)
        for F in list(range(1, 261)) + [512, 2044, 2048]:
            lds = [F + d for d in list(range(10)) + [16]]
            lds += [lim - cw, lim - 1, lim, lim + 1, lim + cw]   # either side of 256 * ld * dtype_bytes = 2^32
            for ld, aligned in itertools.product(lds, (0, 1)):
                want = R.plan_ref(nbytes, F, ld, aligned)
                assert library_plan(nbytes, F, ld, aligned) == want, (nbytes, F, ld, aligned, want)
                seen.add(want)
                checked += 1
    assert checked == 3 * 263 * 16 * 2
    assert seen == {(R.PJ_MFMA, 1), (R.PJ_ROWS, 1), (R.PJ_ROWS, 0)}


def test_plan_names_the_kernels_of_known_rows():
    """The restated dispatch itself, on rows whose kernel the headers state."""
    assert R.plan_ref(4, 512, 512, 1) == (R.PJ_MFMA, 1)            # the benchmark's rows
    assert R.plan_ref(4, 512, 512, 0) == (R.PJ_ROWS, 0)            # a base pointer off the 16-byte grid
    assert R.plan_ref(4, 36, 40, 1) == (R.PJ_MFMA, 1) and R.plan_ref(4, 36, 37, 1) == (R.PJ_ROWS, 0)
    assert R.plan_ref(8, 17, 17, 1) == (R.PJ_ROWS, 0) and R.plan_ref(2, 72, 72, 1) == (R.PJ_MFMA, 1)
    for nbytes in (2, 4, 8):
        lim, cw = R.stride_limit(nbytes), 16 // nbytes
        assert lim * nbytes == 16 << 20                            # rows of 16 MiB
        assert R.plan_ref(nbytes, 8 * cw, lim, 1) == (R.PJ_ROWS, 1)
        assert R.plan_ref(nbytes, 8 * cw, lim - cw, 1) == (R.PJ_MFMA, 1)
        # the largest byte offset the fp64-MFMA kernel forms (row 255 of a tile, the row's last vector) fits 32 bits
        assert 255 * (lim - cw) * nbytes + (lim - cw) * nbytes - 16 < 2 ** 32


def test_plan_rejects_what_no_projection_accepts():
    from msmbuilder_amd import _lib
    k, v = ctypes.c_int(), ctypes.c_int()
    L = _lib.lib()
    for args in ((3, 4, 4, 1), (4, 0, 4, 1), (4, 8, 7, 1)):
        assert L.msm_tica_project_plan(*args, ctypes.byref(k), ctypes.byref(v)) == _lib.MSM_ERR_INVALID
    assert L.msm_tica_project_plan(4, 4, 4, 1, None, ctypes.byref(v)) == _lib.MSM_ERR_INVALID
    assert L.msm_tica_project_last_stats(None) == _lib.MSM_ERR_INVALID


def test_tiles_and_groups_of_hand_written_cases():
    assert R.tiles_ref([]) == [] and R.tiles_ref([0, 0]) == []
    assert R.tiles_ref([1]) == [(0, 0, 1)]
    assert R.tiles_ref([256]) == [(0, 0, 256)]
    assert R.tiles_ref([257]) == [(0, 0, 257), (0, 256, 1)]
    assert R.tiles_ref([0, 513, 0, 2]) == [(1, 0, 513), (1, 256, 257), (1, 512, 1), (3, 0, 2)]
    assert len(R.tiles_ref(R.BATCH_LENS)) == 0 + 1 + 1 + 1 + 2 + 2 + 3

    rb = 16
    assert R.groups_ref([], rb, 100 * rb) == [] and R.groups_ref([0, 0], rb, 100 * rb) == []
    assert R.groups_ref([5], rb, 100 * rb) == [(0, 1)]
    assert R.groups_ref([50, 50], rb, 100 * rb) == [(0, 2)]                    # exactly the budget: one group
    assert R.groups_ref([50, 51], rb, 100 * rb) == [(0, 1), (1, 2)]
    assert R.groups_ref([500], rb, 100 * rb) == [(0, 1)]                       # larger than the budget: a group of its own
    assert R.groups_ref([500, 1], rb, 100 * rb) == [(0, 1), (1, 2)]
    assert R.groups_ref([0, 500], rb, 100 * rb) == [(0, 2)]                    # leading empties cost nothing
    assert R.groups_ref([500, 0], rb, 100 * rb) == [(0, 1), (1, 2)]            # ... one behind a full group opens the next
    assert R.groups_ref([500, 0, 500], rb, 100 * rb) == [(0, 1), (1, 3)]
    # the GPU module's list: empties on both sides of a boundary, one trajectory beyond the budget, a trailing empty
    assert R.groups_ref(R.GROUP_LENS, rb, R.GROUP_BUDGET_ROWS * rb) == [(0, 3), (3, 4), (4, 5), (5, 9)]
    assert R.groups_ref(R.GROUP_LENS, rb, 512 << 20) == [(0, 9)]


def test_element_types_round_trip():
    rs = np.random.RandomState(5)
    x = rs.randn(1000) * 10.0 ** rs.uniform(-3, 3, 1000)
    for dt in R.DTYPES:
        s = R.store(x, dt)
        assert s.dtype == {"bf16": np.uint16, "f32": np.float32, "f64": np.float64}[dt]
        w = R.widen(s)
        assert np.array_equal(R.widen(R.store(w, dt)), w)          # stored values are fixed points
        assert np.all(np.abs(w - x) <= np.abs(x) * 2.0 ** -{"bf16": 8, "f32": 24, "f64": 53}[dt])
    assert R.store([1.0, 1.00390625, 1.01171875], "bf16").tolist() == [0x3f80, 0x3f80, 0x3f82]   # ties go to even
    for dt in R.DTYPES:
        p = R.widen(R.poison_like((3, 5), dt))
        assert not np.isfinite(p).any() and np.isnan(p).sum() in (7, 8) and (p == np.inf).any() and (p == -np.inf).any()


def _cases():
    for dt in R.DTYPES:
        for n, F, k in R.all_shapes(dt):
            for family in R.FAMILIES:
                yield dt, family, n, F, k


def test_float64_evaluation_meets_the_bound_on_every_input():
    """The reference alone: numpy's float64 X . V^T - mean . V^T (whatever order its dot sums in) is inside the bound."""
    worst, count = 0.0, 0
    for dt, family, n, F, k in _cases():
        X, mean, V = R.make_case(family, n, F, k, dt)
        ok, w = R.within(R.project_f64(X, mean, V), X, mean, V)
        assert ok, (dt, family, n, F, k, w)
        worst = max(worst, w)
        count += 1
    assert count > 300 and 0.0 < worst <= 1.0
    print("float64 evaluation: worst error / bound %.3f over %d inputs" % (worst, count))


def test_offset_family_cancels():
    """The family is what it claims: the result is three orders of magnitude below its terms (plain data: the same order)."""
    for dt in ("f32", "f64"):
        X, mean, V = R.make_case("offset", 257, 100, 17, dt)
        V = V.astype(np.float64)
        ratio = np.abs(R.project_ref(X, mean, V)).astype(np.float64).max() / (R.project_bound(X, mean, V).max() / ((100 + 8) * R.U))
        assert ratio < 2e-3, ratio
        X, mean, V = R.make_case("plain", 257, 100, 17, dt)
        assert np.abs(R.project_ref(X, mean, V)).astype(np.float64).max() / (R.project_bound(X, mean, V).max() / ((100 + 8) * R.U)) > 0.05


def _f32_accumulation(X, mean, V):
    V32 = V.astype(np.float32)
    return (R.widen(X).astype(np.float32).dot(V32.T) - mean.astype(np.float32).dot(V32.T)[None, :]).astype(np.float64)


def _padding_column(X, mean, V, dt):
    """Rows at stride F + 1 whose padding column is poisoned, and an evaluation that takes the padding for the last feature."""
    n, F = X.shape
    big = R.poison_like((n, F + 1), dt)
    big[:, :F] = X
    wrong = big[:, :F].copy()
    wrong[:, F - 1] = big[:, F]
    with np.errstate(invalid="ignore"):
        return R.project_f64(wrong, mean, V)


def _row_before(X, mean, V):
    got = R.project_f64(X, mean, V)
    got[-1] = got[-2]
    return got


def test_impostors_fall_outside_the_bound():
    """float32 accumulation, a padding column read for the last feature, and row n - 2 delivered for row n - 1: each is
    outside the bound on every input it can be formed on (the last needs two rows, and rows that differ as stored:
    bfloat16 keeps 8 bits of a value, so rows of the `offset` family -- offsets of 10^3 spreads and more -- may coincide)."""
    count = [0, 0, 0]
    for dt, family, n, F, k in _cases():
        X, mean, V = R.make_case(family, n, F, k, dt)
        assert not R.within(_f32_accumulation(X, mean, V), X, mean, V)[0], ("float32", dt, family, n, F, k)
        assert not R.within(_padding_column(X, mean, V, dt), X, mean, V)[0], ("padding", dt, family, n, F, k)
        count[0] += 1
        count[1] += 1
        if n >= 2 and not (dt == "bf16" and family == "offset"):
            assert not np.array_equal(X[-1], X[-2])
            assert not R.within(_row_before(X, mean, V), X, mean, V)[0], ("row", dt, family, n, F, k)
            count[2] += 1
    assert min(count) > 200, count


@pytest.mark.parametrize("dt", R.DTYPES)
def test_shape_lists_cover_every_listed_value(dt):
    m = R.mfma_shapes(dt)
    assert {s[0] for s in m} == set(R.MFMA_N) and {s[1] for s in m} == set(R.MFMA_F[dt]) and {s[2] for s in m} == set(R.MFMA_K)
    r = R.rows_shapes()
    assert {s[0] for s in r} == set(R.ROWS_N) and {s[1] for s in r} == set(R.ROWS_F) and {s[2] for s in r} == set(R.ROWS_K)
    nb, cw = R.NBYTES[dt], R.CW[dt]
    chunk = 128 // nb
    assert sorted(-(-F // chunk) for F in R.MFMA_F[dt]) == [1, 2, 3, 4]                  # chunk counts
    assert [F % chunk == 0 for F in R.MFMA_F[dt]] == [False, False, True, False]         # whole and partial last chunks
    for n, F, k in m:
        assert R.plan_ref(nb, F, F + cw, 1) == (R.PJ_MFMA, 1)
    for n, F, k in r:
        assert R.plan_ref(nb, F, F + 1, 1) == (R.PJ_ROWS, 0)
    assert R.plan_ref(nb, R.BATCH_F[dt], R.BATCH_F[dt], 1)[0] == R.PJ_MFMA
    assert R.plan_ref(nb, R.BATCH_F[dt] - 1, R.BATCH_F[dt] - 1, 1)[0] == R.PJ_ROWS
    assert R.plan_ref(nb, R.WIDE_F[dt], R.stride_limit(nb), 1) == (R.PJ_ROWS, 1) and R.WIDE_F[dt] % 64 == 8
