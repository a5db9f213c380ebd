// distance.hip -- exact-arithmetic libdistance for gfx950: assign_nearest, cdist, dist, pdist, sumdist.
// (The k-centers fits, which share its kernels' arithmetic and its host helpers -- distance_host.h --, are kcenters.hip.)
//
// Replaces /root/reference/msmbuilder/libdistance/src/{distance_kernels.h:41-293,
// dist.hpp:4-80, cdist.hpp:4-49, assign.hpp:6-91}.
//
// Bit-exactness contract (what makes integer labels identical to the CPU path):
// every (row, centre) pair is owned by ONE lane, which visits the features in
// order i = 0..m-1 with ONE fp64 accumulator; for float inputs u-v / u+v are
// fp32 operations widened afterwards; multiply and add are separately rounded
// (this file is compiled with -ffp-contract=off); euclidean takes the sqrt
// before comparing; comparisons are strict `<` in ascending centre order, so
// the lowest index wins.  Parallelism is over rows (and centre tiles), never
// over the feature axis.  This is HBM/L2- and fp64-VALU-bound work: no MFMA.
//
// Tiling: a workgroup stages a [256 rows x FC features] tile of X through LDS
// (coalesced in, row stride FC+1 so that lane-per-row reads are conflict-free)
// and a [CJ centres x FC] tile of Y (wave-uniform broadcast reads).
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "distance_dev.h"

#include "distance_pair_dev.h"   // pair_kernel / pair_small_kernel / assign_small2_kernel: assign_nearest, cdist, dist in exact arithmetic
#include "distance_pdist_dev.h"   // pdist_kernel, sumdist_kernel
#include "distance_host.h"   // row_vecw, wide_ok, launch_wide (wide_kernel: the streaming path for wide rows), pad_rows, sum_partials_host
namespace msm {

// ---- host-side dispatch ----------------------------------------------------
template <typename T, int MODE>
void launch_pair(int metric, int grid, const PairArgs& P)
{
    const bool wide = wide_ok<T>(P.X, P.Y, P.m, P.X_indices != nullptr);
    WideArgs A;
    memset(&A, 0, sizeof(A));
    A.pa = P;
    metric_visit(metric, [&](auto mm) {
        constexpr int MM = decltype(mm)::value;
        if (P.vecw > 0 && MODE == 0 && (MM == M_EUCLIDEAN || MM == M_SQEUCLIDEAN) &&
            (sizeof(T) == 4 ? launch_small3_f32(MM, grid, P) : launch_small3_f64(MM, grid, P))) {
        } else if (P.vecw > 0 && MODE == 0)
            hipLaunchKernelGGL((assign_small2_kernel<T, MM>), dim3(grid), dim3(DT), 0, stream(), P); /* every block writes its partial */
        else if (P.vecw > 0)
            hipLaunchKernelGGL((pair_small_kernel<T, MM, MODE>), dim3(grid), dim3(DT), 0, stream(), P);
        else if (wide)
            launch_wide<T, MM, MODE>(grid, A);
        else
            hipLaunchKernelGGL((pair_kernel<T, MM, MODE>), dim3(grid), dim3(DT), 0, stream(), P);
    });
}

template <typename T, int WHICH>
void launch_pd(int metric, int grid, const PdArgs& P)
{
    metric_visit(metric, [&](auto mm) {
        if (WHICH == 0)
            hipLaunchKernelGGL((pdist_kernel<T, decltype(mm)::value>), dim3(grid), dim3(DT), 0, stream(), P);
        else
            hipLaunchKernelGGL((sumdist_kernel<T, decltype(mm)::value>), dim3(grid), dim3(DT), 0, stream(), P);
    });
}

template <typename T>
int assign_nearest_impl(const T* X, const T* Y, const char* metric, const msm_idx_t* X_indices,
                        msm_idx_t n_X, msm_idx_t n_Y, msm_idx_t m, msm_idx_t n_idx,
                        msm_idx_t* assignments, double* min_dist, double* inertia, int on_device)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!X || !Y || !assignments) return fail(MSM_ERR_INVALID, "assign_nearest: null pointer");
    if (n_X < 0 || n_Y < 0 || m < 1) return fail(MSM_ERR_INVALID, "assign_nearest: bad shape");
    const long long n = X_indices ? n_idx : n_X;
    if (inertia) *inertia = 0.0;
    if (n == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    DevBuf &dX = pool(PS_X), &dY = pool(PS_Y), &dIdx = pool(PS_IDX), &dLab = pool(PS_LAB), &dMin = pool(PS_MIN),
           &dPart = pool(PS_PART);
    int grid = (int)std::min<long long>(ceil_div(n, DT), 2048);
    if ((rc = dY.reserve((size_t)(n_Y ? n_Y : 1) * m * sizeof(T)))) return rc;
    if (n_Y) MSM_HIP_CHECK(hipMemcpyAsync(dY.p, Y, (size_t)n_Y * m * sizeof(T), hipMemcpyHostToDevice, stream()));
    if ((rc = dPart.reserve((size_t)grid * sizeof(double)))) return rc;
    PairArgs P;
    memset(&P, 0, sizeof(P));
    P.Y = dY.p;
    P.n = n;
    P.K = n_Y;
    P.m = m;
    P.partial = dPart.as<double>();
    if (on_device) {
        P.X = X;
        P.X_indices = X_indices;
        P.labels = assignments;
        P.min_dist = min_dist;
    } else {
        if ((rc = dX.reserve((size_t)n_X * m * sizeof(T)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n_X * m * sizeof(T)))) return rc;
        P.X = dX.p;
        if (X_indices) {
            if ((rc = dIdx.reserve((size_t)n * sizeof(msm_idx_t)))) return rc;
            MSM_HIP_CHECK(hipMemcpyAsync(dIdx.p, X_indices, (size_t)n * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
            P.X_indices = dIdx.as<msm_idx_t>();
        }
        if ((rc = dLab.reserve((size_t)n * sizeof(msm_idx_t)))) return rc;
        P.labels = dLab.as<msm_idx_t>();
        if (min_dist) {
            if ((rc = dMin.reserve((size_t)n * sizeof(double)))) return rc;
            P.min_dist = dMin.as<double>();
        }
    }
    if (pad_rows_pays<T>(mid, m, n_X, P.X_indices != nullptr)) {
        const T *xp = nullptr, *yp = nullptr;
        long long mp = m;
        if ((rc = pad_rows<T>(static_cast<const T*>(P.X), n_X, m, pool(PS_PADX), &xp, &mp))) return rc;
        if ((rc = pad_rows<T>(static_cast<const T*>(P.Y), n_Y, m, pool(PS_PADY), &yp, &mp))) return rc;
        P.X = xp;
        P.Y = yp;
        P.m = m = mp;
    }
    P.vecw = row_vecw<T>(P.X, m, P.X_indices != nullptr);
    if (P.vecw == 0 && wide_ok<T>(P.X, P.Y, m, P.X_indices != nullptr)) grid = wide_grid(n);
    launch_pair<T, 0>(mid, grid, P);
    MSM_HIP_CHECK(hipGetLastError());
    if (!on_device) {
        MSM_HIP_CHECK(hipMemcpyAsync(assignments, P.labels, (size_t)n * sizeof(msm_idx_t), hipMemcpyDeviceToHost, stream()));
        if (min_dist)
            MSM_HIP_CHECK(hipMemcpyAsync(min_dist, P.min_dist, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    double s = 0.0;
    if ((rc = sum_partials_host(P.partial, grid, &s))) return rc;  // synchronises
    if (inertia) *inertia = s;
    return MSM_OK;
}

template <typename T>
int cdist_impl(const T* XA, const T* XB, const char* metric, msm_idx_t na, msm_idx_t nb,
               msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t n_idx, double* out, int on_device)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!XA || !XB || !out) return fail(MSM_ERR_INVALID, "cdist/dist: null pointer");
    if (na < 0 || nb < 0 || m < 1) return fail(MSM_ERR_INVALID, "cdist/dist: bad shape");
    const long long n = X_indices ? n_idx : na;
    if (n == 0 || nb == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    DevBuf &dX = pool(PS_X), &dY = pool(PS_Y), &dIdx = pool(PS_IDX), &dOut = pool(PS_OUT);
    int grid = (int)std::min<long long>(ceil_div(n, DT), 2048);
    if ((rc = dY.reserve((size_t)nb * m * sizeof(T)))) return rc;
    if ((rc = h2d_bulk(dY.p, XB, (size_t)nb * m * sizeof(T)))) return rc;
    PairArgs P;
    memset(&P, 0, sizeof(P));
    P.Y = dY.p;
    P.n = n;
    P.K = nb;
    P.m = m;
    if (on_device) {
        P.X = XA;
        P.X_indices = X_indices;
        P.out = out;
    } else {
        if ((rc = dX.reserve((size_t)na * m * sizeof(T)))) return rc;
        if ((rc = h2d_bulk(dX.p, XA, (size_t)na * m * sizeof(T)))) return rc;
        P.X = dX.p;
        if (X_indices) {
            if ((rc = dIdx.reserve((size_t)n * sizeof(msm_idx_t)))) return rc;
            MSM_HIP_CHECK(hipMemcpyAsync(dIdx.p, X_indices, (size_t)n * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
            P.X_indices = dIdx.as<msm_idx_t>();
        }
        if ((rc = dOut.reserve((size_t)n * nb * sizeof(double)))) return rc;
        P.out = dOut.as<double>();
    }
    P.vecw = row_vecw<T>(P.X, m, P.X_indices != nullptr);
    if (P.vecw == 0 && wide_ok<T>(P.X, P.Y, m, P.X_indices != nullptr)) grid = wide_grid(n);
    launch_pair<T, 1>(mid, grid, P);
    MSM_HIP_CHECK(hipGetLastError());
    if (!on_device)
        MSM_HIP_CHECK(hipMemcpyAsync(out, P.out, (size_t)n * nb * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));  // scratch (and the staged Y) die with this frame
    return MSM_OK;
}

// Stages the inputs of a pdist (host rows / indices are uploaded to the PS_X / PS_IDX slots, device ones used in place) and
// queues the kernel that writes the nn(nn-1)/2 condensed distances to the DEVICE buffer dout.  Nothing is synchronised.
// Shared by pdist_impl and the k-medoids fit (kmedoids.hip), whose matrix never leaves HBM.
template <typename T>
int pdist_queue(const T* X, int mid, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t nn, int on_device,
                double* dout)
{
    int rc;
    DevBuf &dX = pool(PS_X), &dIdx = pool(PS_IDX);
    PdArgs P;
    memset(&P, 0, sizeof(P));
    P.n = nn;
    P.m = m;
    P.out = dout;
    if (on_device) {
        P.X = X;
        P.X_indices = X_indices;
    } else {
        if ((rc = dX.reserve((size_t)n * m * sizeof(T)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n * m * sizeof(T)))) return rc;
        P.X = dX.p;
        if (X_indices) {
            if ((rc = dIdx.reserve((size_t)nn * sizeof(msm_idx_t)))) return rc;
            MSM_HIP_CHECK(hipMemcpyAsync(dIdx.p, X_indices, (size_t)nn * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
            P.X_indices = dIdx.as<msm_idx_t>();
        }
    }
    launch_pd<T, 0>(mid, (int)std::min<long long>(nn - 1, 4096), P);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}
template int pdist_queue<float>(const float*, int, msm_idx_t, msm_idx_t, const msm_idx_t*, msm_idx_t, int, double*);
template int pdist_queue<double>(const double*, int, msm_idx_t, msm_idx_t, const msm_idx_t*, msm_idx_t, int, double*);

template <typename T>
int pdist_impl(const T* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices,
               msm_idx_t n_idx, double* out, int on_device)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!X || !out) return fail(MSM_ERR_INVALID, "pdist: null pointer");
    if (n < 0 || m < 1) return fail(MSM_ERR_INVALID, "pdist: bad shape");
    const long long nn = X_indices ? n_idx : n;
    if (nn < 2) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    const size_t npairs = (size_t)nn * (size_t)(nn - 1) / 2;
    double* dout = out;
    if (!on_device) {
        DevBuf& dOut = pool(PS_OUT);
        if ((rc = dOut.reserve(npairs * sizeof(double)))) return rc;
        dout = dOut.as<double>();
    }
    if ((rc = pdist_queue<T>(X, mid, n, m, X_indices, nn, on_device, dout))) return rc;
    if (!on_device && (rc = d2h_bulk(out, dout, npairs * sizeof(double)))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <typename T>
int sumdist_impl(const T* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* pairs,
                 msm_idx_t p, double* sum, int on_device)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!X || !sum || (p > 0 && !pairs)) return fail(MSM_ERR_INVALID, "sumdist: null pointer");
    if (n < 0 || m < 1 || p < 0) return fail(MSM_ERR_INVALID, "sumdist: bad shape");
    *sum = 0.0;
    if (p == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    DevBuf &dX = pool(PS_X), &dIdx = pool(PS_IDX), &dPart = pool(PS_PART);
    const int grid = (int)std::min<long long>(ceil_div(p, DT), 1024);
    if ((rc = dPart.reserve((size_t)grid * sizeof(double)))) return rc;
    PdArgs P;
    memset(&P, 0, sizeof(P));
    P.n = n;
    P.m = m;
    P.p = p;
    P.partial = dPart.as<double>();
    if (on_device) {
        P.X = X;
        P.pairs = pairs;
    } else {
        if ((rc = dX.reserve((size_t)n * m * sizeof(T)))) return rc;
        if ((rc = dIdx.reserve((size_t)p * 2 * sizeof(msm_idx_t)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n * m * sizeof(T)))) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(dIdx.p, pairs, (size_t)p * 2 * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
        P.X = dX.p;
        P.pairs = dIdx.as<msm_idx_t>();
    }
    launch_pd<T, 1>(mid, grid, P);
    MSM_HIP_CHECK(hipGetLastError());
    return sum_partials_host(P.partial, grid, sum);
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_pdist_f32(const float* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices,
                  msm_idx_t n_X_indices, double* out, int on_device)
{
    return pdist_impl<float>(X, metric, n, m, X_indices, n_X_indices, out, on_device);
}

int msm_pdist_f64(const double* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices,
                  msm_idx_t n_X_indices, double* out, int on_device)
{
    return pdist_impl<double>(X, metric, n, m, X_indices, n_X_indices, out, on_device);
}

int msm_sumdist_f32(const float* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* pairs,
                    msm_idx_t p, double* sum, int on_device)
{
    return sumdist_impl<float>(X, metric, n, m, pairs, p, sum, on_device);
}

int msm_sumdist_f64(const double* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* pairs,
                    msm_idx_t p, double* sum, int on_device)
{
    return sumdist_impl<double>(X, metric, n, m, pairs, p, sum, on_device);
}

int msm_dist_f32(const float* X, const float* y, const char* metric, msm_idx_t n, msm_idx_t m,
                 const msm_idx_t* X_indices, msm_idx_t n_X_indices, double* out, int on_device)
{
    return cdist_impl<float>(X, y, metric, n, 1, m, X_indices, n_X_indices, out, on_device);
}

int msm_dist_f64(const double* X, const double* y, const char* metric, msm_idx_t n, msm_idx_t m,
                 const msm_idx_t* X_indices, msm_idx_t n_X_indices, double* out, int on_device)
{
    return cdist_impl<double>(X, y, metric, n, 1, m, X_indices, n_X_indices, out, on_device);
}

int msm_cdist_f32(const float* XA, const float* XB, const char* metric, msm_idx_t na, msm_idx_t nb,
                  msm_idx_t m, double* out, int on_device)
{
    return cdist_impl<float>(XA, XB, metric, na, nb, m, nullptr, 0, out, on_device);
}

int msm_cdist_f64(const double* XA, const double* XB, const char* metric, msm_idx_t na,
                  msm_idx_t nb, msm_idx_t m, double* out, int on_device)
{
    return cdist_impl<double>(XA, XB, metric, na, nb, m, nullptr, 0, out, on_device);
}

int msm_assign_nearest_f32(const float* X, const float* Y, const char* metric,
                           const msm_idx_t* X_indices, msm_idx_t n_X, msm_idx_t n_Y,
                           msm_idx_t n_features, msm_idx_t n_X_indices, msm_idx_t* assignments,
                           double* min_dist, double* inertia, int on_device)
{
    return assign_nearest_impl<float>(X, Y, metric, X_indices, n_X, n_Y, n_features, n_X_indices,
                                      assignments, min_dist, inertia, on_device);
}

int msm_assign_nearest_f64(const double* X, const double* Y, const char* metric,
                           const msm_idx_t* X_indices, msm_idx_t n_X, msm_idx_t n_Y,
                           msm_idx_t n_features, msm_idx_t n_X_indices, msm_idx_t* assignments,
                           double* min_dist, double* inertia, int on_device)
{
    return assign_nearest_impl<double>(X, Y, metric, X_indices, n_X, n_Y, n_features, n_X_indices,
                                       assignments, min_dist, inertia, on_device);
}

}  // extern "C"
