// nystroem.hip -- msm_kernel_map_{f32,f64} and msm_kernel_map_plan: the Nystroem kernel feature map
// out[i, :] = k(x_i, landmarks) . B - c on the device (replaces, in decomposition/kernel_approximation.py, scikit-learn's
// pairwise_kernels(X, components_) followed by np.dot(embedded, normalization_.T) on the host over every frame, and in
// decomposition/ktica.py:209-211 that map followed by the tICA projection).  Kernels: nystroem_dev.h.
#include "common.h"

#include <algorithm>
#include <cstdlib>

#include "nystroem_dev.h"

namespace msm {

constexpr long long NY_LDS_TWO = 80 * 1024;        // a block up to here leaves room for two workgroups on a CU
constexpr long long NY_LDS_BUDGET = 144 * 1024;    // the largest block one workgroup may hold (of 160 KiB, less the static part)
constexpr long long NY_SCRATCH_BYTES = (long long)64 << 20;   // the scratch route's block of kernel values
constexpr size_t NY_STAGE_BYTES = (size_t)256 << 20;          // host rows: rows + result staged per group

struct NyPlan {
    int fused, RB, Lpad, pitch;
    long long lds, chunk_rows;
};

// Decided in ONE place (exported to the tests as msm_kernel_map_plan; pure but for MSM_NYSTROEM_FUSED).
static NyPlan ny_plan(long long L, bool allow_fused)
{
    NyPlan p;
    p.Lpad = (int)(ceil_div(L, 16) * 16);
    p.pitch = p.Lpad + NY_PAD;
    const long long row16 = 16LL * p.pitch * (long long)sizeof(double);
    p.fused = 0;
    p.RB = NY_RB_MAX;
    p.lds = 0;
    if (allow_fused) {
        for (int rb = NY_RB_MAX; rb >= 1; rb >>= 1)
            if (rb * row16 <= (rb == 1 ? NY_LDS_BUDGET : NY_LDS_TWO)) {
                p.fused = 1;
                p.RB = rb;
                p.lds = rb * row16;
                break;
            }
    }
    const long long unit = 16 * NY_RB_MAX;
    p.chunk_rows = std::max<long long>(unit, NY_SCRATCH_BYTES / (p.pitch * (long long)sizeof(double)) / unit * unit);
    return p;
}

static bool fused_allowed()
{
    const char* e = getenv("MSM_NYSTROEM_FUSED");
    return !(e && e[0] == '0');
}

static DevBuf& ny_scratch()
{
    static DevBuf b;   // the scratch route's block: this unit's own, grow-only
    return b;
}

template <typename T, typename TO>
static int ny_launch(NyArgs A, const NyPlan& pl, long long scratch_rows)
{
    const long long R = 16LL * pl.RB;
    if (pl.fused) {
        static long long attr_set = 0;   // per instantiation
        if (pl.lds > attr_set) {
            MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(ny_fused_kernel<T, TO>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
            attr_set = pl.lds;
        }
        A.RB = pl.RB;
        hipLaunchKernelGGL((ny_fused_kernel<T, TO>), dim3((unsigned)ceil_div(A.n, R)), dim3(NY_T), (size_t)pl.lds, stream(), A);
        MSM_HIP_CHECK(hipGetLastError());
        return MSM_OK;
    }
    long long chunk = scratch_rows > 0 ? ceil_div(scratch_rows, R) * R : pl.chunk_rows;
    chunk = std::min(chunk, ceil_div(A.n, R) * R);
    int rc;
    if ((rc = ny_scratch().reserve((size_t)chunk * pl.pitch * sizeof(double)))) return rc;
    const T* X = static_cast<const T*>(A.X);
    TO* out = static_cast<TO*>(A.out);
    const long long n = A.n;
    A.RB = pl.RB;
    A.scratch = ny_scratch().as<double>();
    for (long long r0 = 0; r0 < n; r0 += chunk) {
        A.n = std::min(chunk, n - r0);
        A.X = X + r0 * A.ld;
        A.out = out + r0 * A.P;
        const unsigned grid = (unsigned)ceil_div(A.n, R);
        hipLaunchKernelGGL((ny_phase1_kernel<T>), dim3(grid), dim3(NY_T), 0, stream(), A);
        hipLaunchKernelGGL((ny_phase2_kernel<TO>), dim3(grid), dim3(NY_T), 0, stream(), A);
    }
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

template <typename T>
static int kernel_map_impl(const T* rows, msm_idx_t n, msm_idx_t F, msm_idx_t ld, const T* landmarks, msm_idx_t L, const double* B,
                           msm_idx_t P, const double* c, int kid, double gamma, double coef0, double degree, void* out, int out_f64,
                           int on_device, msm_idx_t scratch_rows)
{
    if (kid < 0 || kid >= NK_COUNT)
        return fail(MSM_ERR_INVALID, "kernel_map: unknown kernel id %d (callable and precomputed kernels have no host path here)", kid);
    if (!landmarks || !B || (n > 0 && (!rows || !out))) return fail(MSM_ERR_INVALID, "kernel_map: null pointer");
    if (n < 0 || F < 1 || L < 1 || P < 1 || ld < F || F > INT32_MAX / 2 || L > INT32_MAX / 2 || P > INT32_MAX / 2 || scratch_rows < 0)
        return fail(MSM_ERR_INVALID, "kernel_map: bad shape");
    if (n == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const NyPlan pl = ny_plan(L, fused_allowed());
    const bool o64 = out_f64 || sizeof(T) == 8;
    const size_t osz = o64 ? sizeof(double) : sizeof(T);
    int rc;
    DevBuf &dX = pool(PS_X), &dOut = pool(PS_OUT), &dLm = pool(PS_Y), &dB = pool(PS_W), &dPar = pool(PS_PAR);
    if ((rc = dLm.reserve((size_t)L * F * sizeof(T)))) return rc;
    if ((rc = dB.reserve((size_t)L * P * sizeof(double)))) return rc;
    if ((rc = dPar.reserve(16 + (size_t)(P + L) * sizeof(double)))) return rc;
    if ((rc = h2d_bulk(dLm.p, landmarks, (size_t)L * F * sizeof(T)))) return rc;
    if ((rc = h2d_bulk(dB.p, B, (size_t)L * P * sizeof(double)))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(dPar.p, 0, 16, stream()));
    double* dc = reinterpret_cast<double*>(dPar.as<char>() + 16);
    if (c) MSM_HIP_CHECK(hipMemcpyAsync(dc, c, (size_t)P * sizeof(double), hipMemcpyHostToDevice, stream()));
    NyArgs A;
    memset(&A, 0, sizeof(A));
    A.F = (int)F;
    A.Lm = dLm.p;
    A.L = (int)L;
    A.Lpad = pl.Lpad;
    A.pitch = pl.pitch;
    A.lmn = dc + P;
    A.B = dB.as<double>();
    A.P = (int)P;
    A.c = c ? dc : nullptr;
    A.gamma = gamma;
    A.coef0 = coef0;
    A.degree = degree;
    A.kid = kid;
    A.flag = dPar.as<int>();
    hipLaunchKernelGGL((ny_lnorm_kernel<T>), dim3((unsigned)(pl.Lpad / 16)), dim3(64), 0, stream(), dLm.as<T>(), (int)L, (int)F, kid,
                       dc + P, A.flag);
    MSM_HIP_CHECK(hipGetLastError());
#define MSM_NY_RUN() (o64 ? ny_launch<T, double>(A, pl, scratch_rows) : ny_launch<T, T>(A, pl, scratch_rows))
    if (on_device) {
        A.X = rows;
        A.n = n;
        A.ld = ld;
        A.out = out;
        if ((rc = MSM_NY_RUN())) return rc;
    } else {
        // host rows: staged in groups (compacted to ld = F), each group's result copied back before the next is uploaded
        const size_t per_row = (size_t)F * sizeof(T) + (size_t)P * osz;
        const msm_idx_t group = (msm_idx_t)std::max<size_t>(1, std::min<size_t>((size_t)n, NY_STAGE_BYTES / per_row));
        if ((rc = dX.reserve((size_t)group * F * sizeof(T)))) return rc;
        if ((rc = dOut.reserve((size_t)group * P * osz))) return rc;
        for (msm_idx_t r0 = 0; r0 < n; r0 += group) {
            const msm_idx_t m = std::min(group, n - r0);
            if (ld == F) {
                if ((rc = h2d_bulk(dX.p, rows + r0 * ld, (size_t)m * F * sizeof(T)))) return rc;
            } else {
                MSM_HIP_CHECK(hipMemcpy2DAsync(dX.p, (size_t)F * sizeof(T), rows + r0 * ld, (size_t)ld * sizeof(T), (size_t)F * sizeof(T),
                                               (size_t)m, hipMemcpyHostToDevice, stream()));
            }
            A.X = dX.p;
            A.n = m;
            A.ld = F;
            A.out = dOut.p;
            if ((rc = MSM_NY_RUN())) return rc;
            if ((rc = d2h_bulk(static_cast<char*>(out) + (size_t)r0 * P * osz, dOut.p, (size_t)m * P * osz))) return rc;
        }
    }
#undef MSM_NY_RUN
    int f = 0;
    MSM_HIP_CHECK(hipMemcpyAsync(&f, A.flag, sizeof(int), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // the uploads' host sources and the pool slots die with this frame
    if (f) return fail(MSM_ERR_NONFINITE, "Input contains NaN, infinity or a value too large");
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_kernel_map_f32(const float* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const float* landmarks, msm_idx_t L,
                       const double* B, msm_idx_t P, const double* c, int kernel, double gamma, double coef0, double degree, void* out,
                       int out_f64, int on_device, msm_idx_t scratch_rows)
{
    return kernel_map_impl<float>(rows, n, n_features, ld, landmarks, L, B, P, c, kernel, gamma, coef0, degree, out, out_f64, on_device,
                                  scratch_rows);
}

int msm_kernel_map_f64(const double* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const double* landmarks, msm_idx_t L,
                       const double* B, msm_idx_t P, const double* c, int kernel, double gamma, double coef0, double degree, void* out,
                       int out_f64, int on_device, msm_idx_t scratch_rows)
{
    return kernel_map_impl<double>(rows, n, n_features, ld, landmarks, L, B, P, c, kernel, gamma, coef0, degree, out, out_f64, on_device,
                                   scratch_rows);
}

int msm_kernel_map_plan(msm_idx_t L, msm_idx_t P, msm_idx_t n_features, int itemsize, msm_idx_t* out9)
{
    if (!out9 || L < 1 || P < 1 || n_features < 1 || (itemsize != 4 && itemsize != 8) || L > INT32_MAX / 2)
        return fail(MSM_ERR_INVALID, "msm_kernel_map_plan: bad argument");
    const NyPlan pl = ny_plan(L, fused_allowed());
    out9[0] = pl.fused;
    out9[1] = 16 * pl.RB;     // R: rows of a workgroup
    out9[2] = 16;             // landmark tile
    out9[3] = 4;              // feature depth of one MFMA
    out9[4] = 16;             // tile of B's columns
    out9[5] = pl.Lpad;
    out9[6] = pl.pitch;
    out9[7] = pl.lds;         // bytes of the LDS block (0: scratch route)
    out9[8] = pl.chunk_rows;  // rows of a scratch chunk unless the call names its own
    return MSM_OK;
}

}  // extern "C"
