// regspatial.hip -- regular spatial (leader) clustering, msm_regspatial_fit_* (replaces the per-row Python loop of
// the reference's cluster/regularspatial.py:69-81).
//
// Exact block form of the sequential definition (row i is a centre iff every centre chosen before it is farther than
// d_min): whether row i is covered by a centre chosen BEFORE its block does not depend on anything inside the block, so
// those tests run for all rows of the block at once (the screen).  What is left -- the survivors -- can only be covered
// by centres chosen inside the block, which are survivors themselves: the resolve step walks them in row order, exactly
// the sequential loop restricted to the survivors.  The host loop synchronises once per block to learn K, grows the
// centre list if K has outgrown it, queues the append of the block's centres and picks the next block size.  Exact arithmetic: built with -ffp-contract=off like distance.hip.
#include "common.h"

#include <algorithm>

#include "distance_dev.h"
#include "regspatial_dev.h"

namespace msm {

constexpr long long RS_CAP0 = 4096;            // initial capacity of the centre list, in centres
constexpr long long RS_B0 = 4096;              // first block
constexpr long long RS_BMIN = 1024, RS_BMAX = 1LL << 22;

// the last fit's result, owned by the library until the next fit (msm_regspatial_result_* copies it out)
struct RsResult {
    msm_idx_t* ids = nullptr;
    void* cen = nullptr;
    long long cap = 0, K = 0, m = 0;
    int elem = 0;   // sizeof(T) of the fit that filled it, 0: none
    long long stats[4] = {0, 0, 0, 0};   // blocks, survivors, resolve rounds, growths
};
static RsResult g_rs;

static int rs_grow(RsResult& R, long long need, size_t row_bytes)
{
    const long long cap = std::max(need, std::max(RS_CAP0, 2 * R.cap));
    msm_idx_t* ids = nullptr;
    void* cen = nullptr;
    MSM_HIP_CHECK(hipMalloc((void**)&ids, (size_t)cap * sizeof(msm_idx_t)));
    hipError_t e = hipMalloc(&cen, (size_t)cap * row_bytes);
    if (e != hipSuccess) {
        (void)hipFree(ids);
        return fail(MSM_ERR_HIP, "regspatial_fit: hipMalloc of %lld centres failed: %s", cap, hipGetErrorString(e));
    }
    if (R.K > 0) {
        MSM_HIP_CHECK(hipMemcpyAsync(ids, R.ids, (size_t)R.K * sizeof(msm_idx_t), hipMemcpyDeviceToDevice, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(cen, R.cen, (size_t)R.K * row_bytes, hipMemcpyDeviceToDevice, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    }
    if (R.ids) (void)hipFree(R.ids);
    if (R.cen) (void)hipFree(R.cen);
    R.ids = ids;
    R.cen = cen;
    R.cap = cap;
    return MSM_OK;
}

template <typename T>
static void rs_launch(int metric, bool small, const RsArgs& P)
{
    const int grid = (int)ceil_div(P.B, DT);
#define MSM_CASE(MM)                                                                                      \
    case MM:                                                                                              \
        if (small)                                                                                        \
            hipLaunchKernelGGL((rs_screen_small_kernel<T, MM>), dim3(grid), dim3(DT), 0, stream(), P);    \
        else                                                                                              \
            hipLaunchKernelGGL((rs_screen_tile_kernel<T, MM>), dim3(grid), dim3(DT), 0, stream(), P);     \
        hipLaunchKernelGGL((rs_resolve_kernel<T, MM>), dim3(1), dim3(RS_RT), 0, stream(), P);             \
        break;
    switch (metric) {
        MSM_CASE(M_EUCLIDEAN)
        MSM_CASE(M_SQEUCLIDEAN)
        MSM_CASE(M_CITYBLOCK)
        MSM_CASE(M_CHEBYSHEV)
        MSM_CASE(M_CANBERRA)
        MSM_CASE(M_BRAYCURTIS)
        MSM_CASE(M_HAMMING)
        MSM_CASE(M_JACCARD)
    }
#undef MSM_CASE
}

template <typename T>
static int regspatial_impl(const T* X, msm_idx_t n, msm_idx_t m, const char* metric, double d_min, msm_idx_t block_rows,
                           int on_device, msm_idx_t* n_centers)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!X || !n_centers) return fail(MSM_ERR_INVALID, "regspatial_fit: null pointer");
    if (n < 1 || m < 1) return fail(MSM_ERR_INVALID, "regspatial_fit: bad shape");
    if (block_rows < 0 || block_rows > RS_BMAX) return fail(MSM_ERR_INVALID, "regspatial_fit: block_rows out of range");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    const size_t row_bytes = (size_t)m * sizeof(T);
    const T* dX = X;
    if (!on_device) {
        DevBuf& bx = pool(PS_X);
        if ((rc = bx.reserve((size_t)n * row_bytes))) return rc;
        if ((rc = h2d_bulk(bx.p, X, (size_t)n * row_bytes))) return rc;
        dX = bx.as<T>();
    }
    RsResult& R = g_rs;
    // every fit starts from an empty list of RS_CAP0 centres of ITS row length (the last fit's buffers were sized for its
    // rows, and the growth count of a fit must not depend on the fits before it)
    if (R.ids) (void)hipFree(R.ids);
    if (R.cen) (void)hipFree(R.cen);
    R.ids = nullptr;
    R.cen = nullptr;
    R.cap = 0;
    R.K = 0;
    R.m = m;
    R.elem = 0;   // (no result to copy out until this fit has finished)
    for (long long& s : R.stats) s = 0;

    long long Bnext = block_rows > 0 ? block_rows : RS_B0;
    DevBuf &dMask = pool(PS_IDX), &dSurv = pool(PS_LAB), &dStat = pool(PS_SUM), &dNew = pool(PS_IDS);
    if ((rc = rs_grow(R, RS_CAP0, row_bytes))) return rc;
    if ((rc = dStat.reserve(RS_NSTAT * sizeof(long long)))) return rc;
    // per-block scratch for the largest block this fit can run, once (a reserve that grows frees, and that synchronises)
    const long long Bcap = std::min<long long>(n, block_rows > 0 ? block_rows : RS_BMAX);
    if ((rc = dNew.reserve((size_t)Bcap * sizeof(msm_idx_t)))) return rc;
    if ((rc = dMask.reserve((size_t)ceil_div(Bcap, DT) * 4 * sizeof(unsigned long long)))) return rc;
    if ((rc = dSurv.reserve((size_t)Bcap * sizeof(int)))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(dStat.p, 0, RS_NSTAT * sizeof(long long), stream()));

    RsArgs P;
    memset(&P, 0, sizeof(P));
    P.X = dX;
    P.m = m;
    P.d_min = d_min;
    P.stat = dStat.as<long long>();
    const bool small = m <= FeatChunk<T>::FC;
    if (small) {
        const uintptr_t a = (uintptr_t)dX;
        P.vecw = (a % 16 == 0 && row_bytes % 16 == 0) ? 16 : (a % 8 == 0 && row_bytes % 8 == 0) ? 8 : (int)sizeof(T);
    }
    long long K = 0;
    for (long long row = 0; row < n;) {
        const long long B = std::min(Bnext, n - row);
        P.row0 = row;
        P.B = (int)B;
        P.K = K;
        P.cen = R.cen;
        P.ids = R.ids;
        P.mask = dMask.as<unsigned long long>();
        P.surv = dSurv.as<int>();
        P.newids = dNew.as<msm_idx_t>();
        rs_launch<T>(mid, small, P);
        MSM_HIP_CHECK(hipGetLastError());
        long long hstat[RS_NSTAT];
        MSM_HIP_CHECK(hipMemcpyAsync(hstat, dStat.p, sizeof(hstat), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        const long long found = hstat[RS_K] - K;
        if (found > 0) {
            // the list grows only when K really outgrows it (the old list is copied while R.K is still the old count)
            if (K + found > R.cap) {
                ++R.stats[3];
                if ((rc = rs_grow(R, K + found, row_bytes))) return rc;
                P.cen = R.cen;
                P.ids = R.ids;
            }
            hipLaunchKernelGGL((rs_append_kernel<T>), dim3((unsigned)std::min<long long>(found, 4096)), dim3(DT), 0, stream(), P, found);
            MSM_HIP_CHECK(hipGetLastError());
        }
        K = R.K = hstat[RS_K];
        R.stats[0] += 1;
        R.stats[1] = hstat[RS_SURV];
        R.stats[2] = hstat[RS_ROUNDS];
        row += B;
        // Block-size rule: a centre found inside a block costs the screen nothing, but every later row of
        // the block that it would have covered reaches the one-workgroup resolve step instead of dying in the screen.
        // So blocks grow while centres are rare (at most one per 64 rows: x 4) and shrink while they are frequent (more
        // than one per 8 rows: / 2).
        if (block_rows == 0) {
            if (found * 64 <= B) Bnext = std::min(RS_BMAX, B * 4);
            else if (found * 8 > B) Bnext = std::max(RS_BMIN, B / 2);
            else Bnext = B;
        }
    }
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // the last append: the scratch slots are shared with other entry points
    R.elem = (int)sizeof(T);
    *n_centers = K;
    return MSM_OK;
}

template <typename T>
static int regspatial_result(msm_idx_t* ids, T* centers)
{
    const RsResult& R = g_rs;
    if (!ids || !centers) return fail(MSM_ERR_INVALID, "regspatial_result: null pointer");
    if (R.elem != (int)sizeof(T)) return fail(MSM_ERR_STATE, "regspatial_result: no finished fit of this element type");
    int rc;
    if ((rc = d2h_bulk(ids, R.ids, (size_t)R.K * sizeof(msm_idx_t)))) return rc;
    return d2h_bulk(centers, R.cen, (size_t)R.K * R.m * sizeof(T));
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_regspatial_fit_f32(const float* X, msm_idx_t n, msm_idx_t m, const char* metric, double d_min, msm_idx_t block_rows,
                           int on_device, msm_idx_t* n_centers)
{
    return regspatial_impl<float>(X, n, m, metric, d_min, block_rows, on_device, n_centers);
}

int msm_regspatial_fit_f64(const double* X, msm_idx_t n, msm_idx_t m, const char* metric, double d_min, msm_idx_t block_rows,
                           int on_device, msm_idx_t* n_centers)
{
    return regspatial_impl<double>(X, n, m, metric, d_min, block_rows, on_device, n_centers);
}

int msm_regspatial_result_f32(msm_idx_t* ids, float* centers) { return regspatial_result<float>(ids, centers); }

int msm_regspatial_result_f64(msm_idx_t* ids, double* centers) { return regspatial_result<double>(ids, centers); }

int msm_regspatial_last_stats(msm_idx_t* out4)
{
    if (!out4) return fail(MSM_ERR_INVALID, "msm_regspatial_last_stats: null pointer");
    for (int i = 0; i < 4; ++i) out4[i] = g_rs.stats[i];
    return MSM_OK;
}

}  // extern "C"
