// divergence.hip -- msm_divergence_cdist_* / _pdist_* / _rows_*: the KL-family divergences of utils/divergence.py between
// the rows of one or two matrices (replaces the nested Python loops of utils/divergence.py:14-31 under
// cluster/agglomerative.py:50-69, which MVCA runs over all pairs of rows of the transition matrix).  Kernels and the
// definition: divergence_dev.h.
#include "common.h"

#include <algorithm>

#include "divergence_dev.h"

namespace msm {

int divergence_kind(const char* name)
{
    static const char* names[DV_COUNT] = {"kl_divergence", "sym_kl_divergence", "js_divergence", "js_metric"};
    if (!name) return -1;
    for (int k = 0; k < DV_COUNT; ++k)
        if (!strcmp(name, names[k])) return k;
    return -1;
}

static int dv_kind_checked(const char* name, const char* who)
{
    const int kind = divergence_kind(name);
    if (kind < 0) fail(MSM_ERR_METRIC, "%s: unknown divergence '%s'", who, name ? name : "(null)");
    return kind;
}

// reps == 1: out[i] = log(x[i]) (the accuracy probe).  reps > 1: a sum of reps logs of slowly growing arguments per
// element (the throughput floor of the tile kernel: the same log, nothing else).
static __global__ __launch_bounds__(DV_T) void dv_log_probe_kernel(const double* __restrict__ x, long long n, int reps, double* __restrict__ out)
{
    for (long long i = (long long)blockIdx.x * DV_T + threadIdx.x; i < n; i += (long long)gridDim.x * DV_T) {
        double v = x[i], acc = log(v);
#pragma unroll 1
        for (int r = 1; r < reps; ++r) {
            v = v * 1.0000001;
            acc = acc + log(v);
        }
        out[i] = acc;
    }
}

template <typename T>
int divergence_tile_queue(int kind, const T* dA, const msm_idx_t* dIdxA, long long nA, const T* dB, const msm_idx_t* dIdxB,
                          long long nB, long long m, double* dOut, int pd)
{
    if (nA < 1 || nB < 1) return MSM_OK;
    DvArgs P;
    memset(&P, 0, sizeof(P));
    P.A = dA;
    P.B = dB;
    P.idxA = dIdxA;
    P.idxB = dIdxB;
    P.nA = nA;
    P.nB = nB;
    P.m = m;
    P.out = dOut;
    P.pd = pd;
    const long long tiles = ceil_div(nA, DV_TI) * ceil_div(nB, DV_TJ);
    const dim3 grid((unsigned)std::min<long long>(tiles, 1 << 20)), block(DV_T);
    switch (kind) {
        case DV_KL: hipLaunchKernelGGL((dv_tile_kernel<T, DV_KL>), grid, block, 0, stream(), P); break;
        case DV_SYM_KL: hipLaunchKernelGGL((dv_tile_kernel<T, DV_SYM_KL>), grid, block, 0, stream(), P); break;
        case DV_JS: hipLaunchKernelGGL((dv_tile_kernel<T, DV_JS>), grid, block, 0, stream(), P); break;
        default: hipLaunchKernelGGL((dv_tile_kernel<T, DV_JS_METRIC>), grid, block, 0, stream(), P); break;
    }
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}
template int divergence_tile_queue<float>(int, const float*, const msm_idx_t*, long long, const float*, const msm_idx_t*, long long,
                                          long long, double*, int);
template int divergence_tile_queue<double>(int, const double*, const msm_idx_t*, long long, const double*, const msm_idx_t*, long long,
                                           long long, double*, int);

template <typename T>
int divergence_pdist_queue(const T* X, int kind, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t nn, int on_device,
                           double* dout)
{
    int rc;
    const T* dX = X;
    const msm_idx_t* dIdx = X_indices;
    if (!on_device) {
        DevBuf &bX = pool(PS_X), &bIdx = pool(PS_IDX);
        if (X_indices)
            for (msm_idx_t i = 0; i < nn; ++i)
                if (X_indices[i] < 0 || X_indices[i] >= n)
                    return fail(MSM_ERR_INVALID, "divergence_pdist: index %lld is outside [0, %lld)", (long long)X_indices[i], (long long)n);
        if ((rc = bX.reserve((size_t)n * m * sizeof(T)))) return rc;
        if ((rc = h2d_bulk(bX.p, X, (size_t)n * m * sizeof(T)))) return rc;
        dX = bX.as<T>();
        if (X_indices) {
            if ((rc = bIdx.reserve((size_t)nn * sizeof(msm_idx_t)))) return rc;
            MSM_HIP_CHECK(hipMemcpyAsync(bIdx.p, X_indices, (size_t)nn * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
            dIdx = bIdx.as<msm_idx_t>();
        }
    }
    return divergence_tile_queue<T>(kind, dX, dIdx, nn, dX, dIdx, nn, m, dout, 1);
}
template int divergence_pdist_queue<float>(const float*, int, msm_idx_t, msm_idx_t, const msm_idx_t*, msm_idx_t, int, double*);
template int divergence_pdist_queue<double>(const double*, int, msm_idx_t, msm_idx_t, const msm_idx_t*, msm_idx_t, int, double*);

template <typename T>
static int dv_cdist_impl(const T* XA, msm_idx_t nA, const T* XB, msm_idx_t nB, msm_idx_t m, const char* kind_name, double* out,
                         int on_device)
{
    const int kind = dv_kind_checked(kind_name, "divergence_cdist");
    if (kind < 0) return MSM_ERR_METRIC;
    if (nA < 0 || nB < 0 || m < 1) return fail(MSM_ERR_INVALID, "divergence_cdist: bad shape");
    if ((nA > 0 && !XA) || (nB > 0 && !XB) || (nA > 0 && nB > 0 && !out)) return fail(MSM_ERR_INVALID, "divergence_cdist: null pointer");
    if (nA == 0 || nB == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    const T *dA = XA, *dB = XB;
    double* dout = out;
    const size_t bytes = (size_t)nA * (size_t)nB * sizeof(double);
    if (!on_device) {
        DevBuf &bA = pool(PS_X), &bB = pool(PS_Y), &bOut = pool(PS_OUT);
        if ((rc = bA.reserve((size_t)nA * m * sizeof(T)))) return rc;
        if ((rc = bB.reserve((size_t)nB * m * sizeof(T)))) return rc;
        if ((rc = bOut.reserve(bytes))) return rc;
        if ((rc = h2d_bulk(bA.p, XA, (size_t)nA * m * sizeof(T)))) return rc;
        if ((rc = h2d_bulk(bB.p, XB, (size_t)nB * m * sizeof(T)))) return rc;
        dA = bA.as<T>();
        dB = bB.as<T>();
        dout = bOut.as<double>();
    }
    if ((rc = divergence_tile_queue<T>(kind, dA, nullptr, nA, dB, nullptr, nB, m, dout, 0))) return rc;
    if (!on_device && (rc = d2h_bulk(out, dout, bytes))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <typename T>
static int dv_pdist_impl(const T* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t n_idx, const char* kind_name,
                         double* out, int on_device)
{
    const int kind = dv_kind_checked(kind_name, "divergence_pdist");
    if (kind < 0) return MSM_ERR_METRIC;
    if (n < 0 || m < 1 || (X_indices && n_idx < 0)) return fail(MSM_ERR_INVALID, "divergence_pdist: bad shape");
    if (!X) return fail(MSM_ERR_INVALID, "divergence_pdist: null pointer");
    const long long nn = X_indices ? n_idx : n;
    if (nn < 2) return MSM_OK;
    if (!out) return fail(MSM_ERR_INVALID, "divergence_pdist: null pointer");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    const size_t bytes = (size_t)nn * (size_t)(nn - 1) / 2 * sizeof(double);
    double* dout = out;
    if (!on_device) {
        DevBuf& bOut = pool(PS_OUT);
        if ((rc = bOut.reserve(bytes))) return rc;
        dout = bOut.as<double>();
    }
    if ((rc = divergence_pdist_queue<T>(X, kind, n, m, X_indices, nn, on_device, dout))) return rc;
    if (!on_device && (rc = d2h_bulk(out, dout, bytes))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <typename T, int KIND>
static void launch_rows(const T* dP, const T* dQ, long long n, long long m, double* dout)
{
    const int grid = (int)std::min<long long>(ceil_div(n, DV_T), 65536);
    hipLaunchKernelGGL((dv_rows_kernel<T, KIND>), dim3(grid), dim3(DV_T), 0, stream(), dP, dQ, n, m, dout);
}

// P, Q and out are HOST arrays: this is the small two-argument form of the reference's pair functions.
template <typename T>
static int dv_rows_impl(const T* Pm, const T* Qm, msm_idx_t n, msm_idx_t m, const char* kind_name, double* out)
{
    const int kind = dv_kind_checked(kind_name, "divergence_rows");
    if (kind < 0) return MSM_ERR_METRIC;
    if (n < 0 || m < 1) return fail(MSM_ERR_INVALID, "divergence_rows: bad shape");
    if (n > 0 && (!Pm || !Qm || !out)) return fail(MSM_ERR_INVALID, "divergence_rows: null pointer");
    if (n == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    DevBuf &bP = pool(PS_X), &bQ = pool(PS_Y), &bOut = pool(PS_OUT);
    const size_t bytes = (size_t)n * m * sizeof(T);
    if ((rc = bP.reserve(bytes))) return rc;
    if ((rc = bQ.reserve(bytes))) return rc;
    if ((rc = bOut.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = h2d_bulk(bP.p, Pm, bytes))) return rc;
    if ((rc = h2d_bulk(bQ.p, Qm, bytes))) return rc;
    switch (kind) {
        case DV_KL: launch_rows<T, DV_KL>(bP.as<T>(), bQ.as<T>(), n, m, bOut.as<double>()); break;
        case DV_SYM_KL: launch_rows<T, DV_SYM_KL>(bP.as<T>(), bQ.as<T>(), n, m, bOut.as<double>()); break;
        case DV_JS: launch_rows<T, DV_JS>(bP.as<T>(), bQ.as<T>(), n, m, bOut.as<double>()); break;
        default: launch_rows<T, DV_JS_METRIC>(bP.as<T>(), bQ.as<T>(), n, m, bOut.as<double>()); break;
    }
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(out, bOut.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_divergence_cdist_f32(const float* XA, msm_idx_t nA, const float* XB, msm_idx_t nB, msm_idx_t m, const char* kind, double* out,
                             int on_device)
{
    return dv_cdist_impl<float>(XA, nA, XB, nB, m, kind, out, on_device);
}

int msm_divergence_cdist_f64(const double* XA, msm_idx_t nA, const double* XB, msm_idx_t nB, msm_idx_t m, const char* kind,
                             double* out, int on_device)
{
    return dv_cdist_impl<double>(XA, nA, XB, nB, m, kind, out, on_device);
}

int msm_divergence_pdist_f32(const float* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t n_idx, const char* kind,
                             double* out, int on_device)
{
    return dv_pdist_impl<float>(X, n, m, X_indices, n_idx, kind, out, on_device);
}

int msm_divergence_pdist_f64(const double* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t n_idx, const char* kind,
                             double* out, int on_device)
{
    return dv_pdist_impl<double>(X, n, m, X_indices, n_idx, kind, out, on_device);
}

int msm_divergence_rows_f32(const float* P, const float* Q, msm_idx_t n, msm_idx_t m, const char* kind, double* out)
{
    return dv_rows_impl<float>(P, Q, n, m, kind, out);
}

int msm_divergence_rows_f64(const double* P, const double* Q, msm_idx_t n, msm_idx_t m, const char* kind, double* out)
{
    return dv_rows_impl<double>(P, Q, n, m, kind, out);
}

int msm_divergence_plan(msm_idx_t* out4)
{
    if (!out4) return fail(MSM_ERR_INVALID, "msm_divergence_plan: null pointer");
    out4[0] = DV_TI;
    out4[1] = DV_TJ;
    out4[2] = DV_CH;
    out4[3] = DV_T;
    return MSM_OK;
}

int msm_divergence_log_probe(const double* x, msm_idx_t n, int reps, double* out, float* ms)
{
    if (n < 0 || reps < 1) return fail(MSM_ERR_INVALID, "msm_divergence_log_probe: bad argument");
    if (n > 0 && (!x || !out)) return fail(MSM_ERR_INVALID, "msm_divergence_log_probe: null pointer");
    if (ms) *ms = 0.0f;
    if (n == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc;
    DevBuf &bX = pool(PS_X), &bOut = pool(PS_OUT);
    if ((rc = bX.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = bOut.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = h2d_bulk(bX.p, x, (size_t)n * sizeof(double)))) return rc;
    hipEvent_t e0, e1;
    MSM_HIP_CHECK(hipEventCreate(&e0));
    MSM_HIP_CHECK(hipEventCreate(&e1));
    const int grid = (int)std::min<long long>(ceil_div(n, DV_T), 65536);
    (void)hipEventRecord(e0, stream());
    hipLaunchKernelGGL(dv_log_probe_kernel, dim3(grid), dim3(DV_T), 0, stream(), bX.as<double>(), (long long)n, reps, bOut.as<double>());
    (void)hipEventRecord(e1, stream());
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(out, bOut.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream());
    if (err == hipSuccess) err = hipStreamSynchronize(stream());
    float t = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&t, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) return fail(MSM_ERR_HIP, "msm_divergence_log_probe: %s", hipGetErrorString(err));
    if (ms) *ms = t;
    return MSM_OK;
}

}  // extern "C"
