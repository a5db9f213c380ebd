// tica_project.hip -- tICA.transform on gfx950: out = (X - mean) comps^T in float64 (tica.py:329-352) for one matrix, a list
// of host trajectories or a list of device-resident ones.  The kernels are tica_project_dev.h; this file chooses between
// them (proj_plan) and queues them.  Nothing here touches a tICA handle.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "tica_project_dev.h"   // tica_project_kernel / tica_project_mfma_kernel, ProjTile

using namespace msm;

// ---- parameters on the device (once per call) and the launches for one device-resident matrix
struct ProjParams {
    double* dmean = nullptr;    // mean @ comps^T (k values)
    double* dcomps = nullptr;   // [k][F] (null: not uploaded, the fp64-MFMA path alone)
    double* dVp = nullptr;      // [ceil(k / 16)][F][16] panels of the fp64-MFMA path
    int* dflag = nullptr;       // non-finite input seen
    std::vector<double> muV, vp;   // host sources of the uploads: alive until the caller has synchronised
};

// host sources of the projection's uploads: muV = mean @ comps^T, and the components in blocks of 16 as panels Vp[F][16]
// (feature-major, zero padded) for the fp64-MFMA path
static void proj_host_params(const double* mean, const double* comps, msm_idx_t k, msm_idx_t n_features, std::vector<double>& muV,
                             std::vector<double>& vp)
{
    muV.assign((size_t)k, 0.0);
    vp.assign((size_t)ceil_div(k, 16) * n_features * 16, 0.0);
    for (msm_idx_t c = 0; c < k; ++c) {
        double sacc = 0.0;
        for (msm_idx_t f = 0; f < n_features; ++f) {
            sacc += mean[f] * comps[c * n_features + f];
            vp[((size_t)(c / 16) * n_features + f) * 16 + (c % 16)] = comps[c * n_features + f];
        }
        muV[(size_t)c] = sacc;
    }
}

// PS_PAR = [dmean k | dcomps k F, `with_comps` | dflag], PS_W = dVp: reserved, uploaded and the flag cleared on stream()
static int proj_upload(ProjParams& Q, const double* mean, const double* comps, msm_idx_t k, msm_idx_t n_features, bool with_comps = true)
{
    DevBuf &dPar = pool(PS_PAR), &dVp = pool(PS_W);
    int rc;
    const size_t comps_n = with_comps ? (size_t)k * n_features : 0;
    if ((rc = dPar.reserve(((size_t)k + comps_n) * sizeof(double) + 16))) return rc;
    if ((rc = dVp.reserve((size_t)ceil_div(k, 16) * n_features * 16 * sizeof(double)))) return rc;
    proj_host_params(mean, comps, k, n_features, Q.muV, Q.vp);
    Q.dmean = dPar.as<double>();
    Q.dcomps = with_comps ? Q.dmean + k : nullptr;
    Q.dflag = reinterpret_cast<int*>(Q.dmean + k + comps_n);
    Q.dVp = dVp.as<double>();
    MSM_HIP_CHECK(hipMemcpyAsync(Q.dmean, Q.muV.data(), k * sizeof(double), hipMemcpyHostToDevice, stream()));
    if (with_comps) MSM_HIP_CHECK(hipMemcpyAsync(Q.dcomps, comps, comps_n * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(Q.dVp, Q.vp.data(), Q.vp.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemsetAsync(Q.dflag, 0, sizeof(int), stream()));
    return MSM_OK;
}

// dtype_bytes 2 / 4 / 8 -> fn(a value of the kernels' element type)
template <typename Fn>
static void proj_type_visit(int dtype_bytes, Fn&& fn)
{
    if (dtype_bytes == 2) fn(Bf16Raw{});
    else if (dtype_bytes == 4) fn(float{});
    else fn(double{});
}
// components per wave 1 .. 8 of the lane-per-row kernel -> fn(std::integral_constant<int, npw>)
template <int NPW = 1, typename Fn>
static void proj_npw_visit(int npw, Fn&& fn)
{
    if constexpr (NPW == 8) fn(std::integral_constant<int, 8>{});
    else if (npw == NPW) fn(std::integral_constant<int, NPW>{});
    else proj_npw_visit<NPW + 1>(npw, fn);
}

// the fp64-MFMA projection, one launch of `grid` workgroups per block of 16 components: rows of X[n_rows][ldd] into outd, or
// -- `tiles` -- one tile of up to 256 rows per workgroup
static int proj_launch_mfma(int dtype_bytes, unsigned grid, const void* Xd, long long n_rows, msm_idx_t n_features, long long ldd,
                            const ProjParams& Q, msm_idx_t k, double* outd, const ProjTile* tiles)
{
    proj_type_visit(dtype_bytes, [&](auto t) {
        using T = decltype(t);
        for (msm_idx_t kb = 0; kb < ceil_div(k, 16); ++kb)
            hipLaunchKernelGGL((tica_project_mfma_kernel<T>), dim3(grid), dim3(NT), 0, stream(), (const T*)Xd, n_rows, (int)n_features, ldd,
                               Q.dmean, Q.dVp + (size_t)kb * n_features * 16, (int)std::min<msm_idx_t>(16, k - kb * 16), (int)(kb * 16), (int)k,
                               outd, Q.dflag, tiles);
    });
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// Which projection kernel rows of n_features elements at row stride ld take, decided in ONE place (exported to the tests as
// msm_tica_project_plan; pure).  Rows that are whole 16-byte vectors at 16-byte aligned addresses are read with vector
// loads; they go to the fp64-MFMA kernel while a 256-row tile spans less than 2^32 bytes (its row offsets are 32-bit), to the
// lane-per-row kernel with vector loads beyond, and every other row to the lane-per-row kernel element by element.
struct ProjPlan {
    int kernel, vec;
};
static ProjPlan proj_plan(int dtype_bytes, msm_idx_t n_features, msm_idx_t ld, bool aligned16)
{
    const int cw = 16 / dtype_bytes;
    const int vec = aligned16 && (ld % cw == 0) && (n_features % cw == 0);
    const bool mfma = vec && (size_t)256 * ld * dtype_bytes < ((size_t)1 << 32);
    return ProjPlan{mfma ? MSM_PJ_MFMA : MSM_PJ_ROWS, vec};
}

static long long g_pj_stats[2] = {0, 0};   // groups of the last host-list call, tiles of the last batch call

// out[n_rows][k] (device) = (X - mean) comps^T for the device-resident X[n_rows][ldd]; queued on stream(), nothing synchronised
static int proj_launch(const ProjParams& Q, const void* Xd, int dtype_bytes, msm_idx_t n_rows, msm_idx_t n_features, msm_idx_t ldd,
                       msm_idx_t k, double* outd)
{
    const ProjPlan pl = proj_plan(dtype_bytes, n_features, ldd, ((uintptr_t)Xd) % 16 == 0);
    if (pl.kernel == MSM_PJ_MFMA)
        return proj_launch_mfma(dtype_bytes, (unsigned)ceil_div(n_rows, 256), Xd, n_rows, n_features, ldd, Q, k, outd, nullptr);
    const unsigned grid = (unsigned)ceil_div(n_rows, 128);
    const int npw = (int)std::min<msm_idx_t>(8, ceil_div(k, 4));  // components per wave
    proj_type_visit(dtype_bytes, [&](auto t) {
        using T = decltype(t);
        proj_npw_visit(npw, [&](auto c) {
            hipLaunchKernelGGL((tica_project_kernel<T, decltype(c)::value>), dim3(grid), dim3(NT), 0, stream(), (const T*)Xd,
                               (long long)n_rows, (int)n_features, (long long)ldd, Q.dmean, Q.dcomps, (int)k, outd, Q.dflag, pl.vec);
        });
    });
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// The argument checks the projection entries share, in their order: `who` names the entry in the null-pointer message,
// `bf16` admits bfloat16 rows (dtype_bytes 2), and a device is asked for only when there is work (`need_device`).
static int proj_check_args(const char* who, bool pointers_ok, int dtype_bytes, bool bf16, bool shape_ok, bool need_device = true)
{
    if (!pointers_ok) return fail(MSM_ERR_INVALID, "%s: null pointer", who);
    if (dtype_bytes != 4 && dtype_bytes != 8 && !(bf16 && dtype_bytes == 2))
        return fail(MSM_ERR_INVALID, bf16 ? "dtype_bytes must be 2 (bfloat16), 4 or 8" : "dtype_bytes must be 4 or 8");
    if (!shape_ok) return fail(MSM_ERR_INVALID, "bad shape");
    if (need_device && msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    return MSM_OK;
}

// The tail of a projection call: reads the non-finite flag if asked, synchronises -- also behind a failed read: the uploads'
// host sources and the scratch buffers die with the caller's frame --, then reports a non-finite input.
static int proj_finish(const ProjParams& Q, int check_finite)
{
    int f = 0;
    const hipError_t read = check_finite ? hipMemcpyAsync(&f, Q.dflag, sizeof(int), hipMemcpyDeviceToHost, stream()) : hipSuccess;
    const hipError_t sync = hipStreamSynchronize(stream());
    MSM_HIP_CHECK(read);
    MSM_HIP_CHECK(sync);
    if (check_finite && f) return fail(MSM_ERR_NONFINITE, "Input contains NaN, infinity or a value too large");
    return MSM_OK;
}

// Groups of whole trajectories under `budget` bytes, rows packed back to back (a trajectory larger than the budget is a group
// of its own): gend[g] is the trajectory after group g's last; returns the bytes of the largest group, rounded up to 256.  Pure.
static size_t proj_groups(const msm_idx_t* n_rows, msm_idx_t n_seq, size_t row_bytes, size_t budget, std::vector<msm_idx_t>& gend)
{
    size_t half = 0, bytes = 0;
    for (msm_idx_t s = 0; s < n_seq; ++s) {
        const size_t b = (size_t)n_rows[s] * row_bytes;
        if (bytes > 0 && bytes + b > budget) {
            gend.push_back(s);
            half = std::max(half, bytes);
            bytes = 0;
        }
        bytes += b;
    }
    gend.push_back(n_seq);
    return (std::max(half, bytes) + 255) & ~(size_t)255;
}

extern "C" {

int msm_tica_project(const void* X, int dtype_bytes, msm_idx_t n_rows, msm_idx_t n_features,
                     msm_idx_t ld, const double* mean, const double* comps, msm_idx_t k,
                     double* out, int on_device, int check_finite)
{
    int rc = proj_check_args("msm_tica_project", X && mean && comps && out, dtype_bytes, true,
                             n_rows >= 0 && n_features >= 1 && k >= 1 && ld >= n_features, n_rows != 0);
    if (rc) return rc;
    if (n_rows == 0) return MSM_OK;
    DevBuf &dX = pool(PS_X), &dOut = pool(PS_OUT);
    ProjParams Q;
    if ((rc = proj_upload(Q, mean, comps, k, n_features))) return rc;
    const void* Xd = X;
    double* outd = out;
    msm_idx_t ldd = ld;
    if (!on_device) {
        if ((rc = dX.reserve((size_t)n_rows * n_features * dtype_bytes))) return rc;
        if ((rc = dOut.reserve((size_t)n_rows * k * sizeof(double)))) return rc;
        if (ld == n_features) {
            if ((rc = h2d_bulk(dX.p, X, (size_t)n_rows * n_features * dtype_bytes))) return rc;
        } else {
            MSM_HIP_CHECK(hipMemcpy2DAsync(dX.p, (size_t)n_features * dtype_bytes, X, (size_t)ld * dtype_bytes,
                                           (size_t)n_features * dtype_bytes, (size_t)n_rows, hipMemcpyHostToDevice, stream()));
        }
        Xd = dX.p;
        outd = dOut.as<double>();
        ldd = n_features;
    }
    if ((rc = proj_launch(Q, Xd, dtype_bytes, n_rows, n_features, ldd, k, outd))) return rc;
    if (!on_device && (rc = d2h_bulk(out, outd, (size_t)n_rows * k * sizeof(double)))) return rc;
    return proj_finish(Q, check_finite);
}

/* msm_tica_project for a LIST of HOST trajectories (contiguous rows of n_features values): out (host) is ONE
 * [sum of n_rows][k] float64 array, trajectory after trajectory.  The rows are staged in groups of 512 MiB through the two
 * halves of a device buffer -- group g + 1 is copied while group g is projected (one launch per group: the projection is
 * row by row) --, the result stays on the device until ONE copy at the end.  A call per trajectory (msm_tica_project) is
 * copy, kernel, copy back, synchronise: 27 GB/s on 100 x (10,000 x 512 f32) against the link's 56 (scripts/apiprobe.py). */
int msm_tica_project_host_list(const void* const* X_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int dtype_bytes,
                               msm_idx_t n_features, const double* mean, const double* comps, msm_idx_t k, double* out,
                               int check_finite)
{
    int rc = proj_check_args("msm_tica_project_host_list", X_ptrs && n_rows && mean && comps && out, dtype_bytes, false,
                             n_seq >= 0 && n_features >= 1 && k >= 1);
    if (rc) return rc;
    size_t total = 0;
    for (msm_idx_t s = 0; s < n_seq; ++s) {
        if (n_rows[s] < 0 || (n_rows[s] > 0 && !X_ptrs[s])) return fail(MSM_ERR_INVALID, "bad sequence %lld", (long long)s);
        total += (size_t)n_rows[s];
    }
    g_pj_stats[0] = 0;
    if (total == 0) return MSM_OK;
    const size_t row_bytes = (size_t)n_features * dtype_bytes;
    size_t budget = (size_t)512 << 20;
    if (const char* be = getenv("MSM_TICA_PROJ_GROUP_BYTES")) {   // bytes per group (the tests' group seams at small sizes); read per call
        const long long b = atoll(be);
        if (b > 0) budget = (size_t)b;
    }
    std::vector<msm_idx_t> gend;
    const size_t half = proj_groups(n_rows, n_seq, row_bytes, budget, gend);   // the two halves of the staging buffer
    g_pj_stats[0] = (long long)gend.size();
    DevBuf &dX = pool(PS_X), &dOut = pool(PS_OUT);
    if ((rc = dX.reserve(2 * half))) return rc;
    if ((rc = dOut.reserve(total * k * sizeof(double)))) return rc;
    ProjParams Q;
    if ((rc = proj_upload(Q, mean, comps, k, n_features))) return rc;
    hipEvent_t evk[2] = {nullptr, nullptr};   // the projection of the group that last used a half has finished
    for (auto& e : evk) MSM_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    auto drop_events = [&](int code) {
        for (auto& e : evk)
            if (e) (void)hipEventDestroy(e);
        return code;
    };
    auto cleanup = [&](int code) {
        (void)hipStreamSynchronize(stream());
        return drop_events(code);
    };
    auto copy_group = [&](size_t g, bool first) -> int {
        char* d = dX.as<char>() + (g & 1) * half;
        for (msm_idx_t s = g ? gend[g - 1] : 0; s < gend[g]; ++s) {
            const size_t b = (size_t)n_rows[s] * row_bytes;
            if (b) {
                const int rcb = h2d_bulk(d, X_ptrs[s], b, first);
                if (rcb) return rcb;
            }
            d += b;
        }
        return MSM_OK;
    };
    if ((rc = copy_group(0, true))) return cleanup(rc);
    size_t row0 = 0;
    for (size_t g = 0; g < gend.size(); ++g) {
        size_t rows = 0;
        for (msm_idx_t s = g ? gend[g - 1] : 0; s < gend[g]; ++s) rows += (size_t)n_rows[s];
        if (rows) {
            rc = proj_launch(Q, dX.as<char>() + (g & 1) * half, dtype_bytes, (msm_idx_t)rows, n_features, n_features, k,
                             dOut.as<double>() + row0 * k);
            if (rc) return cleanup(rc);
        }
        if (hipEventRecord(evk[g & 1], stream()) != hipSuccess) return cleanup(fail(MSM_ERR_HIP, "hipEventRecord failed"));
        row0 += rows;
        if (g + 1 < gend.size()) {
            // the other half was last read by the projection of group g - 1 (queued before this one)
            if (g >= 1 && hipEventSynchronize(evk[(g + 1) & 1]) != hipSuccess) return cleanup(fail(MSM_ERR_HIP, "hipEventSynchronize failed"));
            if ((rc = copy_group(g + 1, false))) return cleanup(rc);
        }
    }
    if ((rc = d2h_bulk(out, dOut.p, total * k * sizeof(double)))) return cleanup(rc);
    return drop_events(proj_finish(Q, check_finite));   // (synchronises)
}

/* msm_tica_project for a LIST of device-resident trajectories in one launch per block of 16 components: X_ptrs[s] is
 * [n_rows[s], n_features] (row stride n_features), out_ptrs[s] its [n_rows[s], k] float64 output.  Needs 16-byte aligned
 * rows (n_features a multiple of 16 / dtype_bytes, aligned base pointers); returns MSM_ERR_INVALID otherwise and the
 * caller projects trajectory by trajectory.  (tica.py:329-352 walks the list; a launch per 10,000-frame trajectory keeps a
 * sixth of the GPU busy.) */
int msm_tica_project_batch(const void* const* X_ptrs, double* const* out_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int dtype_bytes,
                           msm_idx_t n_features, const double* mean, const double* comps, msm_idx_t k, int check_finite)
{
    int rc = proj_check_args("msm_tica_project_batch", X_ptrs && out_ptrs && n_rows && mean && comps, dtype_bytes, true,
                             n_seq >= 0 && n_features >= 1 && k >= 1);
    if (rc) return rc;
    g_pj_stats[1] = 0;
    if (proj_plan(dtype_bytes, n_features, n_features, true).kernel != MSM_PJ_MFMA)   // whole 16-byte vectors, 32-bit tile offsets
        return fail(MSM_ERR_INVALID, "msm_tica_project_batch: rows must be whole 16-byte vectors");
    std::vector<ProjTile> tiles;
    for (msm_idx_t s = 0; s < n_seq; ++s) {
        if (n_rows[s] < 0) return fail(MSM_ERR_INVALID, "bad shape");
        if (n_rows[s] == 0) continue;
        if (!X_ptrs[s] || !out_ptrs[s]) return fail(MSM_ERR_INVALID, "msm_tica_project_batch: null pointer");
        if (((uintptr_t)X_ptrs[s]) % 16 != 0) return fail(MSM_ERR_INVALID, "msm_tica_project_batch: rows must be 16-byte aligned");
        for (msm_idx_t r = 0; r < n_rows[s]; r += 256) {
            ProjTile t;
            t.x = static_cast<const char*>(X_ptrs[s]) + (size_t)r * n_features * dtype_bytes;
            t.out = out_ptrs[s] + (size_t)r * k;
            t.rows = n_rows[s] - r;
            tiles.push_back(t);
        }
    }
    g_pj_stats[1] = (long long)tiles.size();
    if (tiles.empty()) return MSM_OK;
    DevBuf& dT = pool(PS_IDX);
    if ((rc = dT.reserve(tiles.size() * sizeof(ProjTile)))) return rc;
    ProjParams Q;
    if ((rc = proj_upload(Q, mean, comps, k, n_features, false))) return rc;   // the fp64-MFMA path reads the panels alone: no k x F components
    MSM_HIP_CHECK(hipMemcpyAsync(dT.p, tiles.data(), tiles.size() * sizeof(ProjTile), hipMemcpyHostToDevice, stream()));
    if ((rc = proj_launch_mfma(dtype_bytes, (unsigned)tiles.size(), nullptr, 0LL, n_features, (long long)n_features, Q, k, nullptr,
                               dT.as<ProjTile>())))
        return rc;
    return proj_finish(Q, check_finite);   // `tiles` and Q's host sources die with this frame
}

int msm_tica_project_plan(int dtype_bytes, msm_idx_t n_features, msm_idx_t ld, int aligned16, int* kernel, int* vec)
{
    if ((dtype_bytes != 2 && dtype_bytes != 4 && dtype_bytes != 8) || n_features < 1 || ld < n_features || !kernel || !vec)
        return fail(MSM_ERR_INVALID, "msm_tica_project_plan: bad argument");
    const ProjPlan pl = proj_plan(dtype_bytes, n_features, ld, aligned16 != 0);
    *kernel = pl.kernel;
    *vec = pl.vec;
    return MSM_OK;
}

int msm_tica_project_last_stats(msm_idx_t* out2)
{
    if (!out2) return fail(MSM_ERR_INVALID, "msm_tica_project_last_stats: null pointer");
    for (int i = 0; i < 2; ++i) out2[i] = g_pj_stats[i];
    return MSM_OK;
}

}  // extern "C"
