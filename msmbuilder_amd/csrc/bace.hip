// bace.hip -- msm_bace_fit / msm_bace_pairs: the Bayes-factor matrix and the merge loop of BACE lumping on the device
// (replaces the nested Python loops of lumping/bace.py:228-327: _calcDMat / _multiDist / _multiDistHelper over all connected
// pairs, then _mergeTwoClosestStates once per merge).  Kernels and the definition: bace_dev.h.
//
// The loop is QUEUED: per merge an update, a row evaluation, a refresh of the stale per-row maxima and a selection, with
// nothing read back in between; the record of selections comes back once at the end.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "bace_dev.h"

namespace msm {

// MSM_BACE_MAX_GRID (read at every call; for the tests): a cap on the workgroups of the three grid-stride kernels, so that
// their strides are taken at sizes a test can afford.  The results do not depend on it.
static long long bace_grid_cap(long long cap)
{
    const char* e = getenv("MSM_BACE_MAX_GRID");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? std::min(v, cap) : cap;
}

static int bace_grid_tiles(long long n)
{
    const long long t = ceil_div(n, BC_TI);
    return (int)std::min<long long>(t * t, bace_grid_cap(1 << 20));
}

static int bace_grid_rows(long long n) { return (int)std::min<long long>(ceil_div(n, BC_RP), bace_grid_cap(1 << 16)); }

static int bace_grid_rowmax(long long n) { return (int)std::min<long long>(n, bace_grid_cap(2048)); }

// The four events of msm_bace_fit's timings, destroyed on every way out.
struct BaceEvents {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~BaceEvents()
    {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// w, unm and alive are HOST arrays; refuses what neither entry point accepts.  *n_alive: the number of kept states.
static int bace_check_host(const char* who, const void* c, const double* w, const int32_t* unm, const int32_t* alive, msm_idx_t n,
                           long long* n_alive)
{
    if (!c || !w || !alive || !unm) return fail(MSM_ERR_INVALID, "%s: null pointer", who);
    if (n < 2) return fail(MSM_ERR_INVALID, "%s: at least 2 states are needed, got %lld", who, (long long)n);
    if (n > BC_MAX_N) return fail(MSM_ERR_INVALID, "%s: at most %d states are supported, got %lld", who, BC_MAX_N, (long long)n);
    long long kept = 0;
    for (msm_idx_t i = 0; i < n; ++i) {
        if (!alive[i]) continue;
        ++kept;
        if (!(w[i] > 0.0) || !std::isfinite(w[i]))
            return fail(MSM_ERR_INVALID, "%s: the weight of kept state %lld is not positive and finite", who, (long long)i);
    }
    *n_alive = kept;
    return MSM_OK;
}

// The counts into `dst` (device), checked there or here: negative and non-finite counts are refused.  Device
// counts are checked by a kernel and the stream is synchronised; host counts are checked here and nothing is synchronised.
static int bace_stage_counts(const char* who, const double* c, msm_idx_t n, int on_device, double* dst, int* dbad)
{
    int rc;
    const size_t total = (size_t)n * (size_t)n;
    if (on_device) {
        MSM_HIP_CHECK(hipMemcpyAsync(dst, c, total * sizeof(double), hipMemcpyDeviceToDevice, stream()));
    } else {
        for (size_t i = 0; i < total; ++i)
            if (!(c[i] >= 0.0) || !std::isfinite(c[i])) return fail(MSM_ERR_NONFINITE, "%s: counts must be non-negative and finite", who);
        if ((rc = h2d_bulk(dst, c, total * sizeof(double)))) return rc;
        return MSM_OK;
    }
    int bad = 0;
    MSM_HIP_CHECK(hipMemsetAsync(dbad, 0, sizeof(int), stream()));
    hipLaunchKernelGGL(bace_check_kernel, dim3((unsigned)std::min<long long>(ceil_div((long long)total, BC_T), 4096)), dim3(BC_T), 0,
                       stream(), dst, (long long)total, dbad);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(&bad, dbad, sizeof(int), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (bad) return fail(MSM_ERR_NONFINITE, "%s: counts must be non-negative and finite", who);
    return MSM_OK;
}

// Device layout of the small per-state arrays in one pool slot (ints): unm | alive | stale | rmax_col | cur | bad
struct BaceInts {
    int *unm, *alive, *stale, *rmax_col, *cur, *bad;
};

static int bace_ints(msm_idx_t n, const int32_t* unm, const int32_t* alive, BaceInts* out)
{
    int rc;
    DevBuf& b = pool(PS_LAB);
    if ((rc = b.reserve(((size_t)4 * n + BC_CUR_COUNT + 1) * sizeof(int)))) return rc;
    int* p = b.as<int>();
    out->unm = p;
    out->alive = p + n;
    out->stale = p + 2 * n;
    out->rmax_col = p + 3 * n;
    out->cur = p + 4 * n;
    out->bad = out->cur + BC_CUR_COUNT;
    std::vector<int> flags(2 * (size_t)n);
    for (msm_idx_t i = 0; i < n; ++i) {
        flags[i] = unm[i] != 0 && alive[i] != 0;
        flags[n + i] = alive[i] != 0;
    }
    MSM_HIP_CHECK(hipMemcpyAsync(p, flags.data(), flags.size() * sizeof(int), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemsetAsync(out->cur, 0, (BC_CUR_COUNT + 1) * sizeof(int), stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // (flags is a local)
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_bace_pairs(const double* counts, const double* w, const int32_t* unmerged, const int32_t* alive, msm_idx_t n, msm_idx_t row,
                   float* out, double* d_out, int on_device)
{
    int rc;
    long long kept = 0;
    if ((rc = bace_check_host("msm_bace_pairs", counts, w, unmerged, alive, n, &kept))) return rc;
    if (!out) return fail(MSM_ERR_INVALID, "msm_bace_pairs: null pointer");
    if (row >= n || (row >= 0 && !alive[row])) return fail(MSM_ERR_INVALID, "msm_bace_pairs: row %lld is not a kept state", (long long)row);
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const size_t total = (size_t)n * (size_t)n;
    BaceInts I;
    if ((rc = bace_ints(n, unmerged, alive, &I))) return rc;
    DevBuf &bC = pool(PS_X), &bW = pool(PS_W), &bD = pool(PS_OUT), &bDD = pool(PS_Y);
    if ((rc = bC.reserve(total * sizeof(double)))) return rc;
    if ((rc = bW.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = bace_stage_counts("msm_bace_pairs", counts, n, on_device, bC.as<double>(), I.bad))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(bW.p, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream()));
    float* dmat = out;
    double* dd = d_out;
    if (!on_device) {
        if ((rc = bD.reserve(total * sizeof(float)))) return rc;
        dmat = bD.as<float>();
        if (d_out) {
            if ((rc = bDD.reserve(total * sizeof(double)))) return rc;
            dd = bDD.as<double>();
        }
    }
    MSM_HIP_CHECK(hipMemsetAsync(dmat, 0, total * sizeof(float), stream()));
    if (dd) MSM_HIP_CHECK(hipMemsetAsync(dd, 0, total * sizeof(double), stream()));
    BaceArgs P;
    memset(&P, 0, sizeof(P));
    P.c = bC.as<double>();
    P.w = bW.as<double>();
    P.unm = I.unm;
    P.alive = I.alive;
    P.n = n;
    P.inv_n = 1.0 / (double)n;
    P.dmat = dmat;
    P.dout = dd;
    if (row < 0)
        hipLaunchKernelGGL(bace_tile_kernel, dim3(bace_grid_tiles(n)), dim3(BC_T), 0, stream(), P);
    else
        hipLaunchKernelGGL(bace_row_kernel, dim3(bace_grid_rows(n)), dim3(BC_T), 0, stream(), P, (const int*)nullptr, (int)row);
    MSM_HIP_CHECK(hipGetLastError());
    if (!on_device) {
        if ((rc = d2h_bulk(out, dmat, total * sizeof(float)))) return rc;
        if (d_out && (rc = d2h_bulk(d_out, dd, total * sizeof(double)))) return rc;
    }
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_bace_fit(const double* counts, const double* w, const int32_t* keep, msm_idx_t n, msm_idx_t n_macrostates, int32_t* merges,
                 float* values, msm_idx_t capacity, msm_idx_t* n_records, float* ms3, int on_device)
{
    int rc;
    long long kept = 0;
    if (ms3) ms3[0] = ms3[1] = ms3[2] = 0.0f;
    if ((rc = bace_check_host("msm_bace_fit", counts, w, keep, keep, n, &kept))) return rc;
    if (!merges || !values || !n_records) return fail(MSM_ERR_INVALID, "msm_bace_fit: null pointer");
    if (n_macrostates < 1) return fail(MSM_ERR_INVALID, "msm_bace_fit: n_macrostates must be at least 1, got %lld", (long long)n_macrostates);
    if (kept < 1) return fail(MSM_ERR_INVALID, "msm_bace_fit: no state is kept");
    const long long M = std::max<long long>(kept - n_macrostates, 0);   // merges; one selection more is recorded
    if (capacity < M + 1) return fail(MSM_ERR_INVALID, "msm_bace_fit: the record holds %lld selections, %lld are needed", (long long)capacity, M + 1);
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const size_t total = (size_t)n * (size_t)n;
    BaceInts I;
    if ((rc = bace_ints(n, keep, keep, &I))) return rc;
    DevBuf &bC = pool(PS_X), &bW = pool(PS_W), &bD = pool(PS_OUT), &bMax = pool(PS_MIN), &bRec = pool(PS_PAR);
    if ((rc = bC.reserve(total * sizeof(double)))) return rc;
    if ((rc = bW.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = bD.reserve(total * sizeof(float)))) return rc;
    if ((rc = bMax.reserve((size_t)n * sizeof(float)))) return rc;
    if ((rc = bRec.reserve((size_t)(M + 1) * 3 * sizeof(int)))) return rc;
    if ((rc = bace_stage_counts("msm_bace_fit", counts, n, on_device, bC.as<double>(), I.bad))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(bW.p, w, (size_t)n * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemsetAsync(bD.p, 0, total * sizeof(float), stream()));
    BaceLoop L;
    memset(&L, 0, sizeof(L));
    L.c = bC.as<double>();
    L.w = bW.as<double>();
    L.unm = I.unm;
    L.alive = I.alive;
    L.dmat = bD.as<float>();
    L.rmax_val = bMax.as<float>();
    L.rmax_col = I.rmax_col;
    L.stale = I.stale;
    L.cur = I.cur;
    L.rec_xy = bRec.as<int>();
    L.rec_val = reinterpret_cast<float*>(L.rec_xy + 2 * (M + 1));
    L.n = n;
    L.inv_n = 1.0 / (double)n;
    BaceArgs P;
    memset(&P, 0, sizeof(P));
    P.c = L.c;
    P.w = L.w;
    P.unm = L.unm;
    P.alive = L.alive;
    P.n = n;
    P.inv_n = L.inv_n;
    P.dmat = L.dmat;
    BaceEvents events;
    hipEvent_t* ev = events.ev;
    if (ms3)
        for (int e = 0; e < 4; ++e) MSM_HIP_CHECK(hipEventCreate(&ev[e]));
    const dim3 block(BC_T), g_state((unsigned)ceil_div(n, BC_T)), g_rows(bace_grid_rows(n)), g_max(bace_grid_rowmax(n));
    // every row's maximum is taken once: stale = 1 everywhere (the bytes 0x01010101 would not do: one int each)
    {
        std::vector<int> ones((size_t)n, 1);
        MSM_HIP_CHECK(hipMemcpyAsync(L.stale, ones.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // (ones is a local; still before the loop)
    }
    if (ms3) (void)hipEventRecord(ev[0], stream());
    hipLaunchKernelGGL(bace_tile_kernel, dim3(bace_grid_tiles(n)), block, 0, stream(), P);
    if (ms3) (void)hipEventRecord(ev[1], stream());
    hipLaunchKernelGGL(bace_rowmax_kernel, g_max, block, 0, stream(), L);
    hipLaunchKernelGGL(bace_select_kernel, dim3(1), block, 0, stream(), L, 0, M > 0 ? 1 : 0);
    MSM_HIP_CHECK(hipGetLastError());
    if (ms3) (void)hipEventRecord(ev[2], stream());
    for (long long s = 1; s <= M; ++s) {
        hipLaunchKernelGGL(bace_update_kernel, g_state, block, 0, stream(), L);
        hipLaunchKernelGGL(bace_row_kernel, g_rows, block, 0, stream(), P, (const int*)L.cur, 0);
        hipLaunchKernelGGL(bace_rowmax_kernel, g_max, block, 0, stream(), L);
        hipLaunchKernelGGL(bace_select_kernel, dim3(1), block, 0, stream(), L, (int)s, s < M ? 1 : 0);
        MSM_HIP_CHECK(hipGetLastError());
    }
    if (ms3) (void)hipEventRecord(ev[3], stream());
    std::vector<int> rec((size_t)(M + 1) * 3);
    MSM_HIP_CHECK(hipMemcpyAsync(rec.data(), L.rec_xy, rec.size() * sizeof(int), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    memcpy(merges, rec.data(), (size_t)(M + 1) * 2 * sizeof(int));
    memcpy(values, rec.data() + 2 * (M + 1), (size_t)(M + 1) * sizeof(float));
    *n_records = M + 1;
    if (ms3) {
        (void)hipEventElapsedTime(&ms3[0], ev[0], ev[1]);
        (void)hipEventElapsedTime(&ms3[1], ev[2], ev[3]);
        (void)hipEventElapsedTime(&ms3[2], ev[0], ev[3]);
    }
    return MSM_OK;
}

int msm_bace_plan(msm_idx_t* out6)
{
    if (!out6) return fail(MSM_ERR_INVALID, "msm_bace_plan: null pointer");
    out6[0] = BC_TI;
    out6[1] = BC_CH;
    out6[2] = BC_RP;
    out6[3] = BC_RC;
    out6[4] = BC_T;
    out6[5] = BC_MAX_N;
    return MSM_OK;
}

}  // extern "C"
