// kmedoids.hip -- k-medoids clustering on a condensed distance matrix, msm_kmedoids and msm_kmedoids_fit_* (replaces
// cluster/src/kmedoids.cc:74-260, reached through _kmedoids.pyx, and the pdist call in front of it in
// cluster/kmedoids.py:91 and minibatchkmedoids.py:83).
//
// The reference runs the loop on one CPU thread over the matrix on the host.  Here the matrix stays where pdist wrote it,
// in HBM, and every iteration is a handful of launches over it (kmedoids_dev.h): costs, medoids, assignment, total and the
// stop test, the host reading one small record per iteration.  A matrix that fits one workgroup's LDS (the mini-batch
// step) runs the whole pass in ONE launch instead.  The random initial assignments come from the caller (the reference
// draws them from a numpy RandomState inside the C loop; the draws do not depend on the data), so the library is
// deterministic.  What a pass leaves in clusterid / error / ifound follows kmedoids.cc:237-250, including its quirk for
// npass <= 1 (the pass works in place, so labels are compared with medoid ids).
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "distance_dev.h"
#include "kmedoids_dev.h"

namespace msm {

static long long g_km_stats[4] = {0, 0, 0, 0};   // passes, iterations of the last pass, path (1: small), snapshots of it

static bool km_small_allowed()
{
    const char* e = getenv("MSM_KMEDOIDS_SMALL");
    return !(e && e[0] == '0');
}

static int km_validate(msm_idx_t n, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init, const msm_idx_t* clusterid,
                       const double* error, const msm_idx_t* ifound)
{
    if (!init || !clusterid || !error || !ifound) return fail(MSM_ERR_INVALID, "kmedoids: null pointer");
    if (n < 1 || n > INT32_MAX / 2) return fail(MSM_ERR_INVALID, "kmedoids: bad number of elements %lld", (long long)n);
    if (K < 1) return fail(MSM_ERR_INVALID, "kmedoids: n_clusters must be at least 1, got %lld", (long long)K);
    if (K > n)
        return fail(MSM_ERR_INVALID, "Number of clusters requested (%lld) greater than number of elements (%lld)", (long long)K,
                    (long long)n);
    if (npass < 0) return fail(MSM_ERR_INVALID, "n_pass must be greater than or equal to zero.");
    std::vector<char> seen((size_t)K);
    for (msm_idx_t p = 0; p < std::max<msm_idx_t>(npass, 1); ++p) {
        std::fill(seen.begin(), seen.end(), 0);
        for (msm_idx_t i = 0; i < n; ++i) {
            const msm_idx_t c = init[p * n + i];
            if (c < 0 || c >= K) return fail(MSM_ERR_INVALID, "kmedoids: initial label %lld of element %lld is outside [0, %lld)", (long long)c, (long long)i, (long long)K);
            seen[(size_t)c] = 1;
        }
        for (msm_idx_t c = 0; c < K; ++c)
            if (!seen[(size_t)c]) return fail(MSM_ERR_INVALID, "kmedoids: cluster %lld is empty in the initial assignment (the reference reads an unset medoid there)", (long long)c);
    }
    return MSM_OK;
}

// The loop on a DEVICE matrix.  Outputs (host) are written only on success.
static int km_run(const double* dD, msm_idx_t n, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init, msm_idx_t* clusterid,
                  double* error, msm_idx_t* ifound)
{
    int rc;
    DevBuf &bT = pool(PS_LAB), &bSaved = pool(PS_IDS), &bCost = pool(PS_MIN), &bDist = pool(PS_SUM), &bBest = pool(PS_PART),
           &bMed = pool(PS_W), &bSt = pool(PS_PAR);
    if ((rc = bT.reserve((size_t)n * sizeof(int)))) return rc;
    if ((rc = bSaved.reserve((size_t)n * sizeof(int)))) return rc;
    if ((rc = bCost.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = bDist.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = bBest.reserve((size_t)K * sizeof(unsigned long long)))) return rc;
    if ((rc = bMed.reserve((size_t)K * sizeof(int)))) return rc;
    if ((rc = bSt.reserve(sizeof(KmState) + sizeof(KmRecord) + sizeof(long long)))) return rc;
    KmArgs P;
    memset(&P, 0, sizeof(P));
    P.D = dD;
    P.n = n;
    P.K = K;
    P.t = bT.as<int>();
    P.saved = bSaved.as<int>();
    P.cost = bCost.as<double>();
    P.dist = bDist.as<double>();
    P.best = bBest.as<unsigned long long>();
    P.med = bMed.as<int>();
    P.st = bSt.as<KmState>();
    P.rec = reinterpret_cast<KmRecord*>(bSt.as<char>() + sizeof(KmState));
    P.flag = reinterpret_cast<int*>(bSt.as<char>() + sizeof(KmState) + sizeof(KmRecord));

    const bool small = n <= KM_SMALL_MAXN && km_small_allowed();
    const long long len = (long long)n * (n - 1) / 2;
    MSM_HIP_CHECK(hipMemsetAsync(P.flag, 0, sizeof(long long), stream()));
    if (!small && len > 0) {
        // the loop is only defined for finite distances: look once, before anything is decided on them
        const int grid = (int)std::min<long long>(ceil_div(len, KM_T), 4096);
        hipLaunchKernelGGL(km_finite_kernel, dim3(grid), dim3(KM_T), 0, stream(), dD, len, P.flag);
        MSM_HIP_CHECK(hipGetLastError());
        int hflag[2] = {0, 0};
        MSM_HIP_CHECK(hipMemcpyAsync(hflag, P.flag, sizeof(hflag), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        if (hflag[0]) return fail(MSM_ERR_NONFINITE, "kmedoids: the distance matrix holds a NaN or infinite distance");
        if (hflag[1]) return fail(MSM_ERR_INVALID, "kmedoids: the distance matrix holds a negative distance");
    }

    const msm_idx_t passes = std::max<msm_idx_t>(npass, 1);
    std::vector<int> t32((size_t)n), med((size_t)K);
    std::vector<msm_idx_t> result((size_t)n, 0), fresh((size_t)n);   // npass > 1: the caller's clusterid starts as zeros
    double err = DBL_MAX;
    msm_idx_t found = -1;
    KmRecord R;
    memset(&R, 0, sizeof(R));
    const int gridN = (int)ceil_div(n, KM_T), gridB = (int)ceil_div(std::max(n, K), KM_T), gridC = (int)ceil_div(n, KM_TI);
    for (msm_idx_t p = 0; p < passes; ++p) {
        for (msm_idx_t i = 0; i < n; ++i) t32[(size_t)i] = (int)init[p * n + i];
        KmState S;
        memset(&S, 0, sizeof(S));
        S.total = DBL_MAX;
        S.period = 10;
        MSM_HIP_CHECK(hipMemcpyAsync(P.t, t32.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(P.saved, t32.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(P.st, &S, sizeof(S), hipMemcpyHostToDevice, stream()));
        do {
            if (small) {
                hipLaunchKernelGGL(km_small_kernel, dim3(1), dim3(KM_T), 0, stream(), P);
            } else {
                hipLaunchKernelGGL(km_begin_kernel, dim3(gridB), dim3(KM_T), 0, stream(), P);
                hipLaunchKernelGGL(km_cost_kernel, dim3(gridC), dim3(KM_T), 0, stream(), P);
                hipLaunchKernelGGL(km_select_kernel, dim3(gridN), dim3(KM_T), 0, stream(), P);
                hipLaunchKernelGGL(km_assign_kernel, dim3(gridN), dim3(KM_T), 0, stream(), P);
                hipLaunchKernelGGL(km_finish_kernel, dim3(1), dim3(KM_T), 0, stream(), P);
            }
            MSM_HIP_CHECK(hipGetLastError());
            MSM_HIP_CHECK(hipMemcpyAsync(&R, P.rec, sizeof(R), hipMemcpyDeviceToHost, stream()));
            MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        } while (!R.stop);
        if (R.bad & 1)
            return fail(MSM_ERR_NONFINITE, "kmedoids: a NaN or infinite distance, or a sum of distances that is not finite");
        if (R.bad & 2) return fail(MSM_ERR_INVALID, "kmedoids: the distance matrix holds a negative distance");
        MSM_HIP_CHECK(hipMemcpyAsync(t32.data(), P.t, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(med.data(), P.med, (size_t)K * sizeof(int), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        // kmedoids.cc:237-250.  npass <= 1: the pass worked in place, `result` IS the final labels.
        if (npass <= 1)
            for (msm_idx_t i = 0; i < n; ++i) result[(size_t)i] = t32[(size_t)i];
        bool differs = false;
        for (msm_idx_t i = 0; i < n; ++i) {
            fresh[(size_t)i] = med[(size_t)t32[(size_t)i]];
            differs |= fresh[(size_t)i] != result[(size_t)i];
        }
        if (differs) {
            if (R.total < err) {
                found = 1;
                err = R.total;
                result = fresh;
            }
        } else {
            ++found;
        }
    }
    g_km_stats[0] = passes;
    g_km_stats[1] = R.counter;
    g_km_stats[2] = small ? 1 : 0;
    g_km_stats[3] = R.snapshots;
    memcpy(clusterid, result.data(), (size_t)n * sizeof(msm_idx_t));
    *error = err;
    *ifound = found;
    return MSM_OK;
}

template <typename T>
static int kmedoids_fit_impl(const T* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                             msm_idx_t n_idx, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init, msm_idx_t* clusterid,
                             double* error, msm_idx_t* ifound, int on_device)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!X) return fail(MSM_ERR_INVALID, "kmedoids_fit: null pointer");
    if (n < 0 || m < 1 || (X_indices && n_idx < 0)) return fail(MSM_ERR_INVALID, "kmedoids_fit: bad shape");
    const msm_idx_t nn = X_indices ? n_idx : n;
    int rc;
    if ((rc = km_validate(nn, K, npass, init, clusterid, error, ifound))) return rc;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    DevBuf& dOut = pool(PS_OUT);
    if ((rc = dOut.reserve(std::max<size_t>((size_t)nn * (size_t)(nn - 1) / 2, 1) * sizeof(double)))) return rc;
    if (nn >= 2 && (rc = pdist_queue<T>(X, mid, n, m, X_indices, nn, on_device, dOut.as<double>()))) return rc;
    return km_run(dOut.as<double>(), nn, K, npass, init, clusterid, error, ifound);
}

}  // namespace msm

using namespace msm;

extern "C" {

msm_idx_t msm_kmedoids_condensed_index(msm_idx_t i, msm_idx_t j, msm_idx_t n) { return km_condensed_index(i, j, n); }

int msm_kmedoids(const double* dmat, msm_idx_t n, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init, msm_idx_t* clusterid,
                 double* error, msm_idx_t* ifound, int on_device)
{
    int rc;
    if ((rc = km_validate(n, K, npass, init, clusterid, error, ifound))) return rc;
    if (n >= 2 && !dmat) return fail(MSM_ERR_INVALID, "kmedoids: null pointer");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const double* dD = dmat;
    if (!on_device || n < 2) {
        DevBuf& dOut = pool(PS_OUT);
        const size_t bytes = (size_t)n * (size_t)(n - 1) / 2 * sizeof(double);
        if ((rc = dOut.reserve(std::max<size_t>(bytes, sizeof(double))))) return rc;
        if (bytes && (rc = h2d_bulk(dOut.p, dmat, bytes))) return rc;
        dD = dOut.as<double>();
    }
    return km_run(dD, n, K, npass, init, clusterid, error, ifound);
}

int msm_kmedoids_fit_f32(const float* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                         msm_idx_t n_X_indices, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init, msm_idx_t* clusterid,
                         double* error, msm_idx_t* ifound, int on_device)
{
    return kmedoids_fit_impl<float>(X, n, m, metric, X_indices, n_X_indices, K, npass, init, clusterid, error, ifound, on_device);
}

int msm_kmedoids_fit_f64(const double* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                         msm_idx_t n_X_indices, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init, msm_idx_t* clusterid,
                         double* error, msm_idx_t* ifound, int on_device)
{
    return kmedoids_fit_impl<double>(X, n, m, metric, X_indices, n_X_indices, K, npass, init, clusterid, error, ifound, on_device);
}

int msm_kmedoids_last_stats(msm_idx_t* out4)
{
    if (!out4) return fail(MSM_ERR_INVALID, "msm_kmedoids_last_stats: null pointer");
    for (int i = 0; i < 4; ++i) out4[i] = g_km_stats[i];
    return MSM_OK;
}

}  // extern "C"
