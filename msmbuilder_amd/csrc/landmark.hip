// landmark.hip -- landmark agglomerative clustering: msm_linkage / msm_linkage_fit_*, msm_landmark_within and
// msm_landmark_predict_* (replaces, in cluster/agglomerative.py, the fastcluster linkage call at :184/:209 over the pdist
// at :183/:208, the Python loop over all pairs at :191-196/:216-221, and the cdist + numpy pooling of predict at :248-273).
//
// The reference runs the O(L^2) linkage on one CPU thread, walks the L(L-1)/2 pairs in Python and forms the N x L
// distance matrix of predict on the host.  Here the condensed matrix stays where pdist wrote it, in HBM; the linkage runs
// on a square working copy beside it as three small launches per merge, all queued before the host reads Z; the
// within-cluster sums are two launches with a fixed summation order; and predict is one fused kernel that never forms
// the N x L matrix (landmark_dev.h).
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "divergence_dev.h"
#include "landmark_dev.h"

namespace msm {

// The condensed matrix of the last msm_linkage_fit_* call, for msm_landmark_within(dmat = NULL).  A buffer of this unit's
// own (no other entry point writes to it); one above FIT_KEEP_BYTES is released once the sums have been taken.
static DevBuf& fit_buf()
{
    static DevBuf b;
    return b;
}
static long long g_fit_n = 0;   // 0: no matrix
constexpr size_t FIT_KEEP_BYTES = (size_t)64 << 20;

static int linkage_method(const char* name)
{
    static const char* names[LK_COUNT] = {"single", "complete", "average", "ward"};
    if (!name) return -1;
    for (int k = 0; k < LK_COUNT; ++k)
        if (!strcmp(name, names[k])) return k;
    return -1;
}

// A metric name of msm_linkage_fit_* / msm_landmark_predict_*: one of libdistance's vector metrics (*mid >= 0) or one of
// the three symmetric divergences (*kind >= 0).  kl_divergence is refused: it is not symmetric.
static int lm_metric(const char* metric, int* mid, int* kind)
{
    *kind = divergence_kind(metric);
    *mid = *kind >= 0 ? -1 : metric_id(metric);
    if (*kind == DV_KL) return fail(MSM_ERR_METRIC, "metric 'kl_divergence' is not symmetric: use sym_kl_divergence, js_divergence or js_metric");
    if (*kind < 0 && *mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    return MSM_OK;
}

static int lk_validate(msm_idx_t n, const char* method, const double* Z)
{
    if (!Z) return fail(MSM_ERR_INVALID, "linkage: null pointer");
    if (n < 2 || n > INT32_MAX / 2) return fail(MSM_ERR_INVALID, "linkage: needs at least 2 observations (and at most 2^30), got %lld", (long long)n);
    if (linkage_method(method) < 0) return fail(MSM_ERR_INVALID, "linkage: unknown method '%s'", method ? method : "(null)");
    return MSM_OK;
}

// The loop on a DEVICE condensed matrix.  Z (host) is written only on success.
static int lk_run(const double* dC, msm_idx_t n, int method, double* Z)
{
    int rc;
    DevBuf square;   // 8 n^2 bytes, released when the call returns
    if ((rc = square.reserve((size_t)n * (size_t)n * sizeof(double)))) return rc;
    DevBuf &bInt = pool(PS_LAB), &bNn = pool(PS_MIN), &bZ = pool(PS_SUM), &bSt = pool(PS_PAR);
    if ((rc = bInt.reserve((size_t)n * 4 * sizeof(int)))) return rc;
    if ((rc = bNn.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = bZ.reserve((size_t)(n - 1) * 4 * sizeof(double)))) return rc;
    if ((rc = bSt.reserve(sizeof(LkSel) + 16))) return rc;
    LkArgs P;
    memset(&P, 0, sizeof(P));
    P.D = square.as<double>();
    P.n = n;
    P.method = method;
    P.active = bInt.as<int>();
    P.size = P.active + n;
    P.id = P.size + n;
    P.nnc = P.id + n;
    P.nnv = bNn.as<double>();
    P.Z = bZ.as<double>();
    P.flag = bSt.as<int>();   // 16 bytes of flags, then the selection record
    P.sel = reinterpret_cast<LkSel*>(bSt.as<char>() + 16);
    MSM_HIP_CHECK(hipMemsetAsync(bSt.p, 0, sizeof(LkSel) + 16, stream()));

    const int gridE = (int)std::min<long long>(ceil_div((long long)n * n, LK_T), 65536);
    const int gridK = (int)ceil_div(n, LK_T), gridR = (int)ceil_div(n, LK_ROWS);
    hipLaunchKernelGGL(lk_expand_kernel, dim3(gridE), dim3(LK_T), 0, stream(), dC, P);
    hipLaunchKernelGGL(lk_refresh_kernel, dim3(gridR), dim3(LK_T), 0, stream(), P, 1);
    for (long long s = 0; s < n - 1; ++s) {
        hipLaunchKernelGGL(lk_select_kernel, dim3(1), dim3(LK_T), 0, stream(), P, s);
        hipLaunchKernelGGL(lk_update_kernel, dim3(gridK), dim3(LK_T), 0, stream(), P, s);
        if (s + 1 < n - 1) hipLaunchKernelGGL(lk_refresh_kernel, dim3(gridR), dim3(LK_T), 0, stream(), P, 0);
    }
    MSM_HIP_CHECK(hipGetLastError());
    std::vector<double> z((size_t)(n - 1) * 4);
    int hflag[2] = {0, 0};
    MSM_HIP_CHECK(hipMemcpyAsync(z.data(), P.Z, z.size() * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(hflag, P.flag, sizeof(hflag), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (hflag[0]) return fail(MSM_ERR_NONFINITE, "linkage: the distance matrix holds a NaN or infinite distance");
    if (hflag[1]) return fail(MSM_ERR_NONFINITE, "linkage: a distance between merged clusters is not finite");
    memcpy(Z, z.data(), z.size() * sizeof(double));
    return MSM_OK;
}

template <typename T>
static int linkage_fit_impl(const T* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                            msm_idx_t n_idx, const char* method, double* Z, int on_device)
{
    int mid, kind, rc;
    if ((rc = lm_metric(metric, &mid, &kind))) return rc;
    if (!X) return fail(MSM_ERR_INVALID, "linkage_fit: null pointer");
    if (n < 0 || m < 1 || (X_indices && n_idx < 0)) return fail(MSM_ERR_INVALID, "linkage_fit: bad shape");
    const msm_idx_t nn = X_indices ? n_idx : n;
    if ((rc = lk_validate(nn, method, Z))) return rc;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    g_fit_n = 0;
    DevBuf& dOut = fit_buf();
    if ((rc = dOut.reserve((size_t)nn * (size_t)(nn - 1) / 2 * sizeof(double)))) return rc;
    if (kind >= 0)
        rc = divergence_pdist_queue<T>(X, kind, n, m, X_indices, nn, on_device, dOut.as<double>());
    else
        rc = pdist_queue<T>(X, mid, n, m, X_indices, nn, on_device, dOut.as<double>());
    if (rc) return rc;
    if ((rc = lk_run(dOut.as<double>(), nn, linkage_method(method), Z))) return rc;
    g_fit_n = nn;
    return MSM_OK;
}

// ---- predict -------------------------------------------------------------------------------------------------------
template <typename T>
static void lp_plan(long long m, int* TL, int* FCH)
{
    const long long E = LP_LDS / (long long)sizeof(T);
    if (m <= E) {
        *TL = (int)std::min<long long>(E / m, LP_TL_MAX);
        *FCH = (int)m;
    } else {
        *TL = 1;
        *FCH = (int)E;
    }
}

template <typename T, int M>
static void launch_lp1(int grid, const LpArgs& P)
{
    if (P.m <= FeatChunk<T>::FC)
        hipLaunchKernelGGL((lp_predict_kernel<T, M, true>), dim3(grid), dim3(LP_T), 0, stream(), P);
    else
        hipLaunchKernelGGL((lp_predict_kernel<T, M, false>), dim3(grid), dim3(LP_T), 0, stream(), P);
}

template <typename T>
static void launch_lp(int mid, int grid, const LpArgs& P)
{
    switch (mid) {
        case M_EUCLIDEAN: launch_lp1<T, M_EUCLIDEAN>(grid, P); break;
        case M_SQEUCLIDEAN: launch_lp1<T, M_SQEUCLIDEAN>(grid, P); break;
        case M_CITYBLOCK: launch_lp1<T, M_CITYBLOCK>(grid, P); break;
        case M_CHEBYSHEV: launch_lp1<T, M_CHEBYSHEV>(grid, P); break;
        case M_CANBERRA: launch_lp1<T, M_CANBERRA>(grid, P); break;
        case M_BRAYCURTIS: launch_lp1<T, M_BRAYCURTIS>(grid, P); break;
        case M_HAMMING: launch_lp1<T, M_HAMMING>(grid, P); break;
        default: launch_lp1<T, M_JACCARD>(grid, P); break;
    }
}

static int pooling_id(const char* name)
{
    return linkage_method(name);   // the same four names, in LpPool's order
}

// The checks on the permuted landmarks' offsets that both predict forms share.
static int lp_validate_offsets(const msm_idx_t* offsets, msm_idx_t K, msm_idx_t L)
{
    if (offsets[0] != 0 || offsets[K] != L) return fail(MSM_ERR_INVALID, "landmark_predict: offsets must run from 0 to the number of landmarks");
    for (msm_idx_t c = 0; c < K; ++c)
        if (offsets[c + 1] < offsets[c]) return fail(MSM_ERR_INVALID, "landmark_predict: offsets must not decrease");
    return MSM_OK;
}

// Rows of an n x L float64 block whose pooled labels one launch takes: the library's scratch for the divergence predict
// holds at most LD_SCRATCH_BYTES, or LP_T rows where one block of LP_T rows is larger than that.
constexpr size_t LD_SCRATCH_BYTES = (size_t)64 << 20;
static long long ld_block_rows(long long n, long long L)
{
    const long long fit = (long long)(LD_SCRATCH_BYTES / ((size_t)L * sizeof(double)));
    return std::min<long long>(n, std::max<long long>(fit / LP_T * LP_T, LP_T));
}

static void launch_ld(const double* dD, long long n, long long L, long long ld, const long long* dOff, const double* dIntra, int pool_id,
                      msm_idx_t* dLabels, double* dPooled, int* dNeg)
{
    LdArgs A;
    memset(&A, 0, sizeof(A));
    A.D = dD;
    A.n = n;
    A.L = L;
    A.ld = ld;
    A.off = dOff;
    A.intra = dIntra;
    A.labels = dLabels;
    A.pooled = dPooled;
    A.neg = dNeg;
    A.pool = pool_id;
    hipLaunchKernelGGL(lp_predict_dmat_kernel, dim3((int)ceil_div(n, LP_T)), dim3(LP_T), 0, stream(), A);
}

// The pooled labels of n rows from a distance matrix, queued; *dNeg is the device flag for ld_finish.  The matrix is one of
//   D  (n x L at row stride ld): a device matrix is pooled in place, a host one travels in blocks of rows through the scratch;
//   dC (DEVICE condensed matrix of n = L elements) with perm (host): blocks of rows of its square form, columns in perm's
//      order and a zero diagonal, are expanded into the scratch.
// labels and pooled follow on_device.
static int ld_run(const double* D, const double* dC, const msm_idx_t* perm, long long n, long long L, long long ld,
                  const msm_idx_t* offsets, msm_idx_t K, const double* intra, int pool_id, msm_idx_t* labels, double* pooled,
                  int on_device, int** dNeg)
{
    int rc;
    DevBuf &dOff = pool(PS_IDX), &dPar = pool(PS_PAR), &dLab = pool(PS_LAB), &dMin = pool(PS_MIN), &dD = pool(PS_OUT), &dPerm = pool(PS_IDS);
    if ((rc = dOff.reserve((size_t)(K + 1) * sizeof(msm_idx_t)))) return rc;
    if ((rc = dPar.reserve(16 + (size_t)K * sizeof(double)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(dOff.p, offsets, (size_t)(K + 1) * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemsetAsync(dPar.p, 0, 16, stream()));
    if (intra)
        MSM_HIP_CHECK(hipMemcpyAsync(dPar.as<char>() + 16, intra, (size_t)K * sizeof(double), hipMemcpyHostToDevice, stream()));
    const long long* off = dOff.as<long long>();
    const double* dIntra = reinterpret_cast<const double*>(dPar.as<char>() + 16);
    *dNeg = dPar.as<int>();
    msm_idx_t* dLabels = labels;
    double* dPooled = pooled;
    if (!on_device) {
        if ((rc = dLab.reserve((size_t)n * sizeof(msm_idx_t)))) return rc;
        if (pooled && (rc = dMin.reserve((size_t)n * sizeof(double)))) return rc;
        dLabels = dLab.as<msm_idx_t>();
        dPooled = pooled ? dMin.as<double>() : nullptr;
    }
    if (D && on_device) {
        launch_ld(D, n, L, ld, off, dIntra, pool_id, dLabels, dPooled, *dNeg);
    } else {
        const long long RB = ld_block_rows(n, L);
        if ((rc = dD.reserve((size_t)RB * (size_t)L * sizeof(double)))) return rc;
        if (dC) {
            if ((rc = dPerm.reserve((size_t)L * sizeof(msm_idx_t)))) return rc;
            MSM_HIP_CHECK(hipMemcpyAsync(dPerm.p, perm, (size_t)L * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
        }
        for (long long r0 = 0; r0 < n; r0 += RB) {
            const long long rb = std::min<long long>(RB, n - r0);
            if (dC)
                hipLaunchKernelGGL(lp_expand_rows_kernel, dim3((int)std::min<long long>(ceil_div(rb * L, LP_T), 65536)), dim3(LP_T), 0, stream(),
                                   dC, n, dPerm.as<long long>(), r0, rb, dD.as<double>());
            else
                MSM_HIP_CHECK(hipMemcpy2DAsync(dD.p, (size_t)L * sizeof(double), D + r0 * ld, (size_t)ld * sizeof(double),
                                               (size_t)L * sizeof(double), (size_t)rb, hipMemcpyHostToDevice, stream()));
            launch_ld(dD.as<double>(), rb, L, L, off, dIntra, pool_id, dLabels + r0, dPooled ? dPooled + r0 : nullptr, *dNeg);
        }
    }
    MSM_HIP_CHECK(hipGetLastError());
    if (!on_device) {
        MSM_HIP_CHECK(hipMemcpyAsync(labels, dLabels, (size_t)n * sizeof(msm_idx_t), hipMemcpyDeviceToHost, stream()));
        if (pooled) MSM_HIP_CHECK(hipMemcpyAsync(pooled, dPooled, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    return MSM_OK;
}

static int ld_finish(const int* dNeg, int* negative)
{
    int neg = 0;
    MSM_HIP_CHECK(hipMemcpyAsync(&neg, dNeg, sizeof(int), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    *negative = neg;
    return MSM_OK;
}

template <typename T>
static int predict_impl(const T* X, msm_idx_t n, msm_idx_t m, const T* landmarks, msm_idx_t L, const msm_idx_t* offsets,
                        msm_idx_t K, const double* intra, const char* metric, const char* pooling, msm_idx_t* labels,
                        double* pooled, int* negative, int on_device)
{
    int mid, kind, rc;
    if ((rc = lm_metric(metric, &mid, &kind))) return rc;
    const int pool_id = pooling_id(pooling);
    if (pool_id < 0) return fail(MSM_ERR_INVALID, "linkage %s is not supported", pooling ? pooling : "(null)");
    if (!landmarks || !offsets || !negative || (n > 0 && (!X || !labels)))
        return fail(MSM_ERR_INVALID, "landmark_predict: null pointer");
    if (pool_id == LP_WARD && !intra) return fail(MSM_ERR_INVALID, "landmark_predict: ward pooling needs the within-cluster sums");
    if (n < 0 || m < 1 || L < 1 || K < 1 || m > INT32_MAX / 2 || L > INT32_MAX / 2)
        return fail(MSM_ERR_INVALID, "landmark_predict: bad shape");
    if ((rc = lp_validate_offsets(offsets, K, L))) return rc;
    *negative = 0;
    if (n == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    DevBuf &dX = pool(PS_X), &dY = pool(PS_Y), &dOff = pool(PS_IDX), &dPar = pool(PS_PAR), &dLab = pool(PS_LAB), &dMin = pool(PS_MIN);
    if ((rc = dY.reserve((size_t)L * m * sizeof(T)))) return rc;
    if ((rc = dOff.reserve((size_t)(K + 1) * sizeof(msm_idx_t)))) return rc;
    if ((rc = dPar.reserve(16 + (size_t)K * sizeof(double)))) return rc;
    if ((rc = h2d_bulk(dY.p, landmarks, (size_t)L * m * sizeof(T)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(dOff.p, offsets, (size_t)(K + 1) * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemsetAsync(dPar.p, 0, 16, stream()));
    if (intra)
        MSM_HIP_CHECK(hipMemcpyAsync(dPar.as<char>() + 16, intra, (size_t)K * sizeof(double), hipMemcpyHostToDevice, stream()));
    LpArgs P;
    memset(&P, 0, sizeof(P));
    P.Lm = dY.p;
    P.n = n;
    P.L = L;
    P.K = K;
    P.m = m;
    P.off = dOff.as<long long>();
    P.intra = reinterpret_cast<const double*>(dPar.as<char>() + 16);
    P.neg = dPar.as<int>();
    P.pool = pool_id;
    lp_plan<T>(m, &P.TL, &P.FCH);
    if (on_device) {
        P.X = X;
        P.labels = labels;
        P.pooled = pooled;
    } else {
        if ((rc = dX.reserve((size_t)n * m * sizeof(T)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n * m * sizeof(T)))) return rc;
        if ((rc = dLab.reserve((size_t)n * sizeof(msm_idx_t)))) return rc;
        P.X = dX.p;
        P.labels = dLab.as<msm_idx_t>();
        if (pooled) {
            if ((rc = dMin.reserve((size_t)n * sizeof(double)))) return rc;
            P.pooled = dMin.as<double>();
        }
    }
    if (kind >= 0) {
        // a divergence: its cdist in blocks of rows into the library's scratch, each block pooled by the matrix kernel
        const long long RB = ld_block_rows(n, L);
        DevBuf& dD = pool(PS_OUT);
        if ((rc = dD.reserve((size_t)RB * (size_t)L * sizeof(double)))) return rc;
        for (long long r0 = 0; r0 < n; r0 += RB) {
            const long long rb = std::min<long long>(RB, n - r0);
            if ((rc = divergence_tile_queue<T>(kind, static_cast<const T*>(P.X) + r0 * m, nullptr, rb, static_cast<const T*>(P.Lm), nullptr,
                                               L, m, dD.as<double>(), 0)))
                return rc;
            launch_ld(dD.as<double>(), rb, L, L, P.off, P.intra, pool_id, P.labels + r0, P.pooled ? P.pooled + r0 : nullptr, P.neg);
        }
    } else {
        launch_lp<T>(mid, (int)ceil_div(n, LP_T), P);
    }
    MSM_HIP_CHECK(hipGetLastError());
    if (!on_device) {
        MSM_HIP_CHECK(hipMemcpyAsync(labels, P.labels, (size_t)n * sizeof(msm_idx_t), hipMemcpyDeviceToHost, stream()));
        if (pooled) MSM_HIP_CHECK(hipMemcpyAsync(pooled, P.pooled, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    int neg = 0;
    MSM_HIP_CHECK(hipMemcpyAsync(&neg, P.neg, sizeof(int), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    *negative = neg;
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_linkage(const double* dmat, msm_idx_t n, const char* method, double* Z, int on_device)
{
    int rc;
    if ((rc = lk_validate(n, method, Z))) return rc;
    if (!dmat) return fail(MSM_ERR_INVALID, "linkage: null pointer");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const double* dC = dmat;
    if (!on_device) {
        DevBuf& dOut = pool(PS_OUT);
        const size_t bytes = (size_t)n * (size_t)(n - 1) / 2 * sizeof(double);
        if ((rc = dOut.reserve(bytes))) return rc;
        if ((rc = h2d_bulk(dOut.p, dmat, bytes))) return rc;
        dC = dOut.as<double>();
    }
    return lk_run(dC, n, linkage_method(method), Z);
}

int msm_linkage_fit_f32(const float* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                        msm_idx_t n_X_indices, const char* method, double* Z, int on_device)
{
    return linkage_fit_impl<float>(X, n, m, metric, X_indices, n_X_indices, method, Z, on_device);
}

int msm_linkage_fit_f64(const double* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                        msm_idx_t n_X_indices, const char* method, double* Z, int on_device)
{
    return linkage_fit_impl<double>(X, n, m, metric, X_indices, n_X_indices, method, Z, on_device);
}

int msm_linkage_plan(msm_idx_t* out2)
{
    if (!out2) return fail(MSM_ERR_INVALID, "msm_linkage_plan: null pointer");
    out2[0] = LK_T;
    out2[1] = LK_ROWS;
    return MSM_OK;
}

int msm_landmark_within(const double* dmat, msm_idx_t n, const msm_idx_t* labels, msm_idx_t K, double* out, int on_device)
{
    if (!labels || !out) return fail(MSM_ERR_INVALID, "landmark_within: null pointer");
    if (n < 1 || n > INT32_MAX / 2 || K < 1 || K > INT32_MAX / 2) return fail(MSM_ERR_INVALID, "landmark_within: bad shape");
    if (n >= 2 && !dmat && (g_fit_n != n || !fit_buf().p))
        return fail(MSM_ERR_STATE, "landmark_within: no matrix of %lld elements is left from msm_linkage_fit_*", (long long)n);
    std::vector<int> lab32((size_t)n);
    for (msm_idx_t i = 0; i < n; ++i) {
        if (labels[i] < 0 || labels[i] >= K)
            return fail(MSM_ERR_INVALID, "landmark_within: label %lld of element %lld is outside [0, %lld)", (long long)labels[i], (long long)i, (long long)K);
        lab32[(size_t)i] = (int)labels[i];
    }
    if (n < 2) {   // no pair
        std::fill(out, out + K, 0.0);
        return MSM_OK;
    }
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    const size_t bytes = (size_t)n * (size_t)(n - 1) / 2 * sizeof(double);
    const double* dC = dmat ? dmat : fit_buf().as<double>();
    if (dmat && !on_device) {
        DevBuf& dOut = pool(PS_OUT);
        if ((rc = dOut.reserve(bytes))) return rc;
        if ((rc = h2d_bulk(dOut.p, dmat, bytes))) return rc;
        dC = dOut.as<double>();
    }
    DevBuf &bLab = pool(PS_LAB), &bRow = pool(PS_MIN), &bOut = pool(PS_SUM);
    if ((rc = bLab.reserve((size_t)n * sizeof(int)))) return rc;
    if ((rc = bRow.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = bOut.reserve((size_t)K * sizeof(double)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(bLab.p, lab32.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(lm_rowsum_kernel, dim3((int)std::min<long long>(n, 65536)), dim3(LK_T), 0, stream(), dC, (long long)n,
                       bLab.as<int>(), bRow.as<double>());
    hipLaunchKernelGGL(lm_clustersum_kernel, dim3((int)std::min<long long>(K, 65536)), dim3(LK_T), 0, stream(), bRow.as<double>(),
                       (long long)n, bLab.as<int>(), (long long)K, bOut.as<double>());
    MSM_HIP_CHECK(hipGetLastError());
    std::vector<double> h((size_t)K);
    MSM_HIP_CHECK(hipMemcpyAsync(h.data(), bOut.p, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    memcpy(out, h.data(), (size_t)K * sizeof(double));
    if (!dmat && fit_buf().cap > FIT_KEEP_BYTES) {
        fit_buf().release();
        g_fit_n = 0;
    }
    return MSM_OK;
}

int msm_landmark_predict_f32(const float* X, msm_idx_t n, msm_idx_t m, const float* landmarks, msm_idx_t L,
                             const msm_idx_t* offsets, msm_idx_t K, const double* intra, const char* metric, const char* pooling,
                             msm_idx_t* labels, double* pooled, int* negative, int on_device)
{
    return predict_impl<float>(X, n, m, landmarks, L, offsets, K, intra, metric, pooling, labels, pooled, negative, on_device);
}

int msm_landmark_predict_f64(const double* X, msm_idx_t n, msm_idx_t m, const double* landmarks, msm_idx_t L,
                             const msm_idx_t* offsets, msm_idx_t K, const double* intra, const char* metric, const char* pooling,
                             msm_idx_t* labels, double* pooled, int* negative, int on_device)
{
    return predict_impl<double>(X, n, m, landmarks, L, offsets, K, intra, metric, pooling, labels, pooled, negative, on_device);
}

int msm_landmark_predict_dmat(const double* D, msm_idx_t n, msm_idx_t L, msm_idx_t ld, const msm_idx_t* offsets, msm_idx_t K,
                              const double* intra, const char* pooling, msm_idx_t* labels, double* pooled, int* negative, int on_device)
{
    const int pool_id = pooling_id(pooling);
    if (pool_id < 0) return fail(MSM_ERR_INVALID, "linkage %s is not supported", pooling ? pooling : "(null)");
    if (!offsets || !negative || (n > 0 && (!D || !labels))) return fail(MSM_ERR_INVALID, "landmark_predict_dmat: null pointer");
    if (pool_id == LP_WARD && !intra) return fail(MSM_ERR_INVALID, "landmark_predict_dmat: ward pooling needs the within-cluster sums");
    if (n < 0 || L < 1 || K < 1 || ld < L || L > INT32_MAX / 2) return fail(MSM_ERR_INVALID, "landmark_predict_dmat: bad shape");
    int rc;
    if ((rc = lp_validate_offsets(offsets, K, L))) return rc;
    *negative = 0;
    if (n == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int* dNeg = nullptr;
    if ((rc = ld_run(D, nullptr, nullptr, n, L, ld, offsets, K, intra, pool_id, labels, pooled, on_device, &dNeg))) return rc;
    return ld_finish(dNeg, negative);
}

int msm_landmark_predict_condensed(const double* dmat, msm_idx_t n, const msm_idx_t* perm, const msm_idx_t* offsets, msm_idx_t K,
                                   const double* intra, const char* pooling, msm_idx_t* labels, double* pooled, int* negative,
                                   int on_device)
{
    const int pool_id = pooling_id(pooling);
    if (pool_id < 0) return fail(MSM_ERR_INVALID, "linkage %s is not supported", pooling ? pooling : "(null)");
    if (!dmat || !perm || !offsets || !negative || !labels) return fail(MSM_ERR_INVALID, "landmark_predict_condensed: null pointer");
    if (pool_id == LP_WARD && !intra) return fail(MSM_ERR_INVALID, "landmark_predict_condensed: ward pooling needs the within-cluster sums");
    if (n < 2 || K < 1 || n > INT32_MAX / 2) return fail(MSM_ERR_INVALID, "landmark_predict_condensed: bad shape");
    for (msm_idx_t i = 0; i < n; ++i)
        if (perm[i] < 0 || perm[i] >= n) return fail(MSM_ERR_INVALID, "landmark_predict_condensed: perm[%lld] is outside [0, %lld)", (long long)i, (long long)n);
    int rc;
    if ((rc = lp_validate_offsets(offsets, K, n))) return rc;
    *negative = 0;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const double* dC = dmat;
    if (!on_device) {
        DevBuf& bC = pool(PS_X);
        const size_t bytes = (size_t)n * (size_t)(n - 1) / 2 * sizeof(double);
        if ((rc = bC.reserve(bytes))) return rc;
        if ((rc = h2d_bulk(bC.p, dmat, bytes))) return rc;
        dC = bC.as<double>();
    }
    int* dNeg = nullptr;
    if ((rc = ld_run(nullptr, dC, perm, n, n, n, offsets, K, intra, pool_id, labels, pooled, on_device, &dNeg))) return rc;
    return ld_finish(dNeg, negative);
}

int msm_landmark_predict_plan(msm_idx_t m, int elem_size, msm_idx_t* out4)
{
    if (!out4 || m < 1 || (elem_size != 4 && elem_size != 8)) return fail(MSM_ERR_INVALID, "msm_landmark_predict_plan: bad argument");
    int TL, FCH;
    if (elem_size == 4)
        lp_plan<float>(m, &TL, &FCH);
    else
        lp_plan<double>(m, &TL, &FCH);
    out4[0] = LP_T;
    out4[1] = TL;
    out4[2] = FCH;
    out4[3] = m <= (elem_size == 4 ? FeatChunk<float>::FC : FeatChunk<double>::FC);
    return MSM_OK;
}

}  // extern "C"
