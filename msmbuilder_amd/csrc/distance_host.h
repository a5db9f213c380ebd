// distance_host.h -- host-side helpers shared by distance.hip (libdistance proper) and kcenters.hip (the k-centers fits):
// the choice between the register, wide-row and scalar-staged kernels, the wide kernel's launcher, the zero-padded aligned
// copy of odd rows and the host sum of per-block partials.
#pragma once
#include "common.h"

#include <algorithm>
#include <type_traits>
#include <vector>

#include "distance_dev.h"
#include "distance_kcpass_dev.h"   // KcArgs: a member of WideArgs
#include "distance_wide_dev.h"

namespace msm {

// metric id -> fn(std::integral_constant<int, id>): the caller's kernels, instantiated once per metric
template <int MM = 0, typename Fn>
static void metric_visit(int metric, Fn&& fn)
{
    if (metric == MM) fn(std::integral_constant<int, MM>{});
    else if constexpr (MM + 1 < M_COUNT) metric_visit<MM + 1>(metric, fn);
}

// widest aligned per-lane vector load for a [*, m] row-major array, 0 if the fast path does not apply
template <typename T>
static int row_vecw(const void* X, long long m, bool has_indices)
{
    if (has_indices || m > FeatChunk<T>::FC) return 0;
    const size_t rb = (size_t)m * sizeof(T);
    const uintptr_t a = (uintptr_t)X;
    if (a % 16 == 0 && rb % 16 == 0) return 16;
    if (a % 8 == 0 && rb % 8 == 0) return 8;
    return (a % sizeof(T) == 0) ? (int)sizeof(T) : 0;
}

constexpr size_t wide_lds(int ncl) { return (size_t)2 * DT * WP * 4 + (size_t)2 * ncl * 32 * 4 + (size_t)DT * 16; }

// wide-row streaming path applies: long rows, 16-byte aligned vectors, no row gather
template <typename T>
static bool wide_ok(const void* X, const void* Y, long long m, bool has_indices)
{
    constexpr int E = 16 / (int)sizeof(T);
    return !has_indices && m > FeatChunk<T>::FC && (m % E) == 0 && (((uintptr_t)X | (uintptr_t)Y) & 15) == 0 &&
           (size_t)m * sizeof(T) < ((size_t)1 << 24);
}

static int wide_grid(long long n)
{
    return (int)std::min<long long>(ceil_div(n, DT), 2LL * num_cus());  // one resident round (2 workgroups / CU)
}

template <typename T, int MM, int MODE, int NCT>
static void launch_wide_nc(int grid, const WideArgs& A)
{
    constexpr size_t lds = wide_lds(MODE == 2 ? WNC : NCT);
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(wide_kernel<T, MM, MODE, NCT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((wide_kernel<T, MM, MODE, NCT>), dim3(grid), dim3(DT), lds, stream(), A);
}

template <typename T, int MM, int MODE>
static void launch_wide(int grid, const WideArgs& A)
{
    // assign_nearest picks its centre-group size by shape (constexpr: the k-centers unit does not carry the assign kernels)
    if constexpr (MODE == 0) {
        if (A.pa.K <= 8) return launch_wide_nc<T, MM, 0, 8>(grid, A);
        // (32-centre groups for float64 rows were measured too: 2M x 256 x K = 100 8.74 ms against 8.31 ms with 16 -- the
        //  4 KiB of extra LDS cost the second workgroup of a CU and more than the halved re-streaming of the row tile gains)
    }
    launch_wide_nc<T, MM, MODE, WNC>(grid, A);
}

static int sum_partials_host(const double* dpartial, int n, double* out)
{
    std::vector<double> h((size_t)n);
    MSM_HIP_CHECK(hipMemcpyAsync(h.data(), dpartial, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += h[i];
    *out = s;
    return MSM_OK;
}

// Rows whose length is not a multiple of 16 bytes (171 float32 contact features: SURVEY 8(d)'s C3 stress variant) cannot take
// the wide-row streaming kernels and fell to the scalar-staged pair kernel -- 20x slower per pair-element (280,000 x 171 x
// K = 200: assign_nearest 32.7 ms, a k-centers pass 134 us at 1.4 TB/s; profiles/r04_pmc_all_first.txt).  For the NORM
// metrics a zero column is an exact no-op in the reference's arithmetic (a float difference 0 - 0 = +0, then s + 0*0 = s,
// s + |0| = s, max(s, 0) = s for s >= 0), so such rows are copied once into a buffer zero-padded to the next multiple of 16
// bytes -- one streaming pass, 2 x the input bytes -- and everything downstream sees aligned rows.  Bit-identical outputs.
template <typename T>
static bool pad_rows_pays(int mid, long long m, long long n, bool has_indices)
{
    constexpr int E = 16 / (int)sizeof(T);
    return !has_indices && (mid == M_EUCLIDEAN || mid == M_SQEUCLIDEAN || mid == M_CITYBLOCK || mid == M_CHEBYSHEV) &&
           m > FeatChunk<T>::FC && (m % E) != 0 && n * m >= (1LL << 20);
}

template <typename T>
__global__ void pad_rows_kernel(const T* __restrict__ X, long long n, long long m, long long mp, T* __restrict__ out)
{
    constexpr int E = 16 / (int)sizeof(T);
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x, per = mp / E;   // 16-byte groups
    if (g >= n * per) return;
    const long long i = g / per, c = (g - i * per) * E;
    T v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) v[e] = c + e < m ? X[i * m + c + e] : (T)0;
#pragma unroll
    for (int e = 0; e < E; ++e) out[i * mp + c + e] = v[e];
}

template <typename T>
static int pad_rows(const T* X, long long n, long long m, DevBuf& buf, const T** out, long long* mp_out)
{
    constexpr int E = 16 / (int)sizeof(T);
    const long long mp = (m + E - 1) / E * E;
    int rc = buf.reserve((size_t)std::max<long long>(n, 1) * mp * sizeof(T));
    if (rc) return rc;
    if (n > 0) {
        const long long groups = n * (mp / E);
        hipLaunchKernelGGL(pad_rows_kernel<T>, dim3((unsigned)ceil_div(groups, 256)), dim3(256), 0, stream(), X, n, m, mp, buf.as<T>());
        MSM_HIP_CHECK(hipGetLastError());
    }
    *out = buf.as<T>();
    *mp_out = mp;
    return MSM_OK;
}

}  // namespace msm
