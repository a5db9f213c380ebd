// speigh.hip -- host side of the sparse generalized eigenpair solver (SparseTICA; kernels in speigh_dev.h).
//
//   msm_speigh_project   the projection onto { z : z^T B z <= 1 } alone
//   msm_speigh_admm      one ADMM solve of  min 1/2 |x - b|^2 + |D(w) x|_1  s.t. x^T B x <= 1
//   msm_speigh           the whole sparse pair: lambda_min(A), the start vector and eigh(B) from the device solves when not
//                        supplied, the persistent launch (relaunched every `budget` ADMM iterations), the final
//                        unconstrained pair on the masked submatrices
//   msm_scdeflate        A - (A x)(x^T A)^T / (x^T A x)
//
// Switches, read per call: MSM_SPEIGH_BUDGET=<ADMM iterations per launch>, MSM_SPEIGH_GRID=<workgroups> (1: the
// single-workgroup layout where E fits in LDS; N: the row-owning layout on N workgroups; unset: by width).
#include "speigh_dev.h"

#include <cmath>
#include <cstdlib>
#include <vector>

namespace msm {

constexpr long long SPG_BUDGET_DEFAULT = 2048;   // sized in profiles/speigh_probe.txt: a launch stays well under a second at 2,048 features

static DevBuf g_spg;   // this file's own workspace: the entry points below call msm_syev_top / msm_sygv_top, which use the pool

struct SpgWork {
    double *A, *B, *E, *Et, *ev, *vec, *pub, *tvals, *tvecs;
    SpgState* S;
    int* flag;
};

static int spg_reserve(int n, bool pair, SpgWork& W)
{
    const size_t nn = (size_t)n * n;
    const size_t doubles = (pair ? 5 : 2) * nn + (size_t)14 * n + 64;
    int rc = g_spg.reserve(doubles * sizeof(double) + sizeof(SpgState) + 64);
    if (rc) return rc;
    double* p = g_spg.as<double>();
    W.E = p, p += nn;
    W.Et = p, p += nn;
    W.A = W.B = W.tvecs = nullptr;
    if (pair) {
        W.A = p, p += nn;
        W.B = p, p += nn;
        W.tvecs = p, p += nn;
    }
    W.ev = p, p += n;
    W.tvals = p, p += n;
    W.vec = p, p += (size_t)5 * n;
    W.pub = p, p += (size_t)6 * n;
    W.flag = reinterpret_cast<int*>(p), p += 8;
    W.S = reinterpret_cast<SpgState*>(p);
    return MSM_OK;
}

static long long spg_env(const char* name)
{
    const char* e = getenv(name);
    if (!e || !e[0]) return 0;
    const long long v = atoll(e);
    return v > 0 ? v : 0;
}

// the layout of a launch: ldsv (one workgroup, E in LDS) or NB workgroups of rpw rows
static void spg_plan(int n, bool& ldsv, int& NB, int& rpw)
{
    const long long g = spg_env("MSM_SPEIGH_GRID");
    if ((g == 0 || g == 1) && n <= SPG_LDS_N) {
        ldsv = true, NB = 1, rpw = n;
        return;
    }
    ldsv = false;
    const int cap = num_cus() < n ? num_cus() : n;
    NB = g > 0 && g < cap ? (int)g : cap;
    rpw = (int)ceil_div(n, NB);
    NB = (int)ceil_div(n, rpw);   // (no workgroup without a row)
}

// Runs the solve described by hs (uploaded to W.S) to its end, a launch per `budget` ADMM iterations.
static int spg_run(const SpgWork& W, int n, SpgState& hs, long long& launches, int& grid)
{
    bool ldsv;
    int NB, rpw;
    spg_plan(n, ldsv, NB, rpw);
    grid = ldsv ? 0 : NB;
    static bool attr_set = false;
    if (!attr_set) {
        MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(speigh_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)((SPG_NVEC * SPG_LDS_N + SPG_LDS_N * (SPG_LDS_N | 1)) * sizeof(double))));
        MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(speigh_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)(SPG_NVEC * SPG_MAXN * sizeof(double))));
        attr_set = true;
    }
    long long budget = spg_env("MSM_SPEIGH_BUDGET");
    if (budget == 0) budget = SPG_BUDGET_DEFAULT;
    if (budget > 1000000) budget = 1000000;   // (the barrier counter is 32 bits wide: 256 workgroups x 2 barriers x budget)
    SpgArgs P;
    P.A = W.A, P.E = W.E, P.Et = W.Et, P.ev = W.ev, P.vec = W.vec, P.pub = W.pub, P.S = W.S;
    P.n = n, P.rpw = rpw, P.budget = budget;
    const size_t lds = ((size_t)SPG_NVEC * n + (ldsv ? (size_t)n * (n | 1) : 0)) * sizeof(double);
    hs.bar = hs.timed_out = 0;
    hs.status = SPG_RUNNING;
    MSM_HIP_CHECK(hipMemcpyAsync(W.S, &hs, sizeof(hs), hipMemcpyHostToDevice, stream()));
    launches = 0;
    for (;;) {
        const long long before = hs.total;
        if (ldsv)
            hipLaunchKernelGGL(speigh_kernel<true>, dim3(1), dim3(SPG_T), lds, stream(), P);
        else
            hipLaunchKernelGGL(speigh_kernel<false>, dim3((unsigned)NB), dim3(SPG_T), lds, stream(), P);
        MSM_HIP_CHECK(hipGetLastError());
        ++launches;
        MSM_HIP_CHECK(hipMemcpyAsync(&hs, W.S, sizeof(hs), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        if (hs.timed_out) {
            hs.status = SPG_TIMEOUT;
            return fail(MSM_ERR_STATE, "speigh: the grid barrier of the persistent launch timed out (%d workgroups were not all resident)", NB);
        }
        if (hs.status != SPG_RUNNING) break;
        if (hs.total == before) return fail(MSM_ERR_STATE, "speigh: a launch made no progress");
        MSM_HIP_CHECK(hipMemsetAsync(&W.S->bar, 0, sizeof(unsigned), stream()));
    }
    return MSM_OK;
}

static int spg_put(double* dst, const double* src, size_t count, int on_device)
{
    MSM_HIP_CHECK(hipMemcpyAsync(dst, src, count * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
    return MSM_OK;
}

static int spg_transpose(const SpgWork& W, int n)
{
    const size_t nn = (size_t)n * n;
    hipLaunchKernelGGL(spg_transpose_kernel, dim3((unsigned)ceil_div((int64_t)nn, 256)), dim3(256), 0, stream(), W.E, n, W.Et);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_speigh_project(const double* a, const double* evals, const double* evecs, msm_idx_t n, double* out, int on_device)
{
    if (!a || !evals || !evecs || !out) return fail(MSM_ERR_INVALID, "msm_speigh_project: null pointer");
    if (n < 1 || n > SPG_MAXN) return fail(MSM_ERR_INVALID, "msm_speigh_project: need 1 <= n <= %d", SPG_MAXN);
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    SpgWork W;
    int rc;
    if ((rc = spg_reserve((int)n, false, W))) return rc;
    if ((rc = spg_put(W.E, evecs, (size_t)n * n, on_device))) return rc;
    if ((rc = spg_put(W.ev, evals, n, on_device))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(W.vec, 0, (size_t)5 * n * sizeof(double), stream()));
    if ((rc = spg_put(W.vec, a, n, on_device))) return rc;
    if ((rc = spg_transpose(W, (int)n))) return rc;
    SpgState hs;
    memset(&hs, 0, sizeof(hs));
    hs.mode = SPG_PROJECT;
    hs.maxiter = 1;
    long long launches;
    int grid;
    if ((rc = spg_run(W, (int)n, hs, launches, grid))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(out, W.vec + n, n * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_speigh_admm(const double* b, const double* w, const double* evals, const double* evecs, double* x_inout, msm_idx_t n,
                    double tol, msm_idx_t maxiter, double* info, int on_device)
{
    if (!b || !w || !evals || !evecs || !x_inout || !info) return fail(MSM_ERR_INVALID, "msm_speigh_admm: null pointer");
    if (n < 1 || n > SPG_MAXN) return fail(MSM_ERR_INVALID, "msm_speigh_admm: need 1 <= n <= %d", SPG_MAXN);
    if (!(tol > 0.0) || maxiter < 1) return fail(MSM_ERR_INVALID, "msm_speigh_admm: need tol > 0 and maxiter >= 1");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    SpgWork W;
    int rc;
    if ((rc = spg_reserve((int)n, false, W))) return rc;
    if ((rc = spg_put(W.E, evecs, (size_t)n * n, on_device))) return rc;
    if ((rc = spg_put(W.ev, evals, n, on_device))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(W.vec, 0, (size_t)5 * n * sizeof(double), stream()));
    if ((rc = spg_put(W.vec, x_inout, n, on_device))) return rc;           // x
    if ((rc = spg_put(W.vec + n, x_inout, n, on_device))) return rc;       // z = x  (u = 0)
    if ((rc = spg_put(W.vec + 3 * n, b, n, on_device))) return rc;
    if ((rc = spg_put(W.vec + 4 * n, w, n, on_device))) return rc;
    if ((rc = spg_transpose(W, (int)n))) return rc;
    SpgState hs;
    memset(&hs, 0, sizeof(hs));
    hs.mode = SPG_ADMM;
    hs.phase = 1;
    hs.rho = 16.0;
    hs.tol = tol;
    hs.maxiter = maxiter;
    long long launches;
    int grid;
    if ((rc = spg_run(W, (int)n, hs, launches, grid))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(x_inout, W.vec, n * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    info[0] = (double)hs.total;
    info[1] = (double)launches;
    info[2] = (double)hs.status;
    info[3] = hs.rho;
    return MSM_OK;
}

int msm_speigh(const double* A, const double* B, msm_idx_t n, double rho, double eps, double tol, msm_idx_t maxiter, const double* x0,
               const double* evalsB, const double* evecsB, double* u, double* v, double* x_out, double* info, int on_device)
{
    if (!A || !B || !u || !v || !info) return fail(MSM_ERR_INVALID, "msm_speigh: null pointer");
    if ((evalsB == nullptr) != (evecsB == nullptr)) return fail(MSM_ERR_INVALID, "msm_speigh: the eigenvalues and eigenvectors of B come together");
    if (n < 1 || n > SPG_MAXN) return fail(MSM_ERR_INVALID, "msm_speigh: need 1 <= n <= %d", SPG_MAXN);
    if (!(eps > 0.0) || !(tol > 0.0) || maxiter < 1 || !(rho >= 0.0) || !std::isfinite(rho) || !std::isfinite(eps) || !std::isfinite(tol))
        return fail(MSM_ERR_INVALID, "msm_speigh: need rho >= 0, eps > 0, tol > 0 (finite) and maxiter >= 1");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    SpgWork W;
    int rc;
    const int N = (int)n;
    const size_t nn = (size_t)n * n;
    if ((rc = spg_reserve(N, true, W))) return rc;
    if ((rc = spg_put(W.A, A, nn, on_device))) return rc;
    if ((rc = spg_put(W.B, B, nn, on_device))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(W.flag, 0, 2 * sizeof(int), stream()));
    hipLaunchKernelGGL(spg_nonfinite_kernel, dim3((unsigned)ceil_div((int64_t)nn, 256)), dim3(256), 0, stream(), W.A, nn, W.flag);
    hipLaunchKernelGGL(spg_nonfinite_kernel, dim3((unsigned)ceil_div((int64_t)nn, 256)), dim3(256), 0, stream(), W.B, nn, W.flag + 1);
    MSM_HIP_CHECK(hipGetLastError());
    int bad[2] = {0, 0};
    MSM_HIP_CHECK(hipMemcpyAsync(bad, W.flag, sizeof(bad), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (bad[0] || bad[1]) return fail(MSM_ERR_NONFINITE, "array must not contain infs or NaNs (%s)", bad[0] ? "A" : "B");

    // tau = 0.1 + max(0, -lambda_min(A))
    double lmin = 0.0;
    if ((rc = msm_syev_top(W.A, n, n, W.tvals, W.tvecs, 1))) return rc;
    MSM_HIP_CHECK(hipMemcpy(&lmin, W.tvals + (n - 1), sizeof(double), hipMemcpyDeviceToHost));
    const double tau = 0.1 + (lmin < 0.0 ? -lmin : 0.0);
    // the start: the top generalized eigenvector (this is also where a B that is not positive definite is refused)
    MSM_HIP_CHECK(hipMemsetAsync(W.vec, 0, (size_t)5 * n * sizeof(double), stream()));
    if (x0) {
        if ((rc = spg_put(W.vec, x0, n, on_device))) return rc;
    } else if ((rc = msm_sygv_top(W.A, W.B, n, 1, W.tvals, W.vec, 1))) {
        return rc;
    }
    // B = E^T diag(ev) E
    if (evalsB) {
        if ((rc = spg_put(W.ev, evalsB, n, on_device))) return rc;
        if ((rc = spg_put(W.E, evecsB, nn, on_device))) return rc;
    } else if ((rc = msm_syev_top(W.B, n, n, W.ev, W.E, 1))) {
        return rc;
    }
    if ((rc = spg_transpose(W, N))) return rc;

    SpgState hs;
    memset(&hs, 0, sizeof(hs));
    hs.mode = SPG_PAIR;
    hs.phase = 0;
    hs.rho = 16.0;
    hs.f = hs.f_old = INFINITY;
    hs.tau = tau;
    hs.rho_e = rho / log1p(1.0 / eps);
    hs.eps = eps;
    hs.tol = tol;
    hs.maxiter = maxiter;
    long long launches = 0;
    int grid = 0;
    if ((rc = spg_run(W, N, hs, launches, grid))) return rc;

    // the sparsity pattern of the iterate, then the unconstrained top pair on the submatrices it selects
    std::vector<double> x(n), hv(n, 0.0), hA, hB;
    MSM_HIP_CHECK(hipMemcpy(x.data(), W.vec, n * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<msm_idx_t> idx;
    for (msm_idx_t i = 0; i < n; ++i)
        if (fabs(x[i]) > 0.0) idx.push_back(i);
    const msm_idx_t m = (msm_idx_t)idx.size();
    double hu = 0.0;
    if (m > 0) {
        hA.resize(nn), hB.resize(nn);
        MSM_HIP_CHECK(hipMemcpy(hA.data(), W.A, nn * sizeof(double), hipMemcpyDeviceToHost));
        MSM_HIP_CHECK(hipMemcpy(hB.data(), W.B, nn * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (m == 1) {
        const size_t d = (size_t)idx[0] * n + idx[0];
        hv[idx[0]] = 1.0 / sqrt(hB[d]);
        hu = hA[d] / hB[d];
    } else if (m > 1) {
        std::vector<double> Ak((size_t)m * m), Bk((size_t)m * m), vk(m);
        for (msm_idx_t r = 0; r < m; ++r)
            for (msm_idx_t c = 0; c < m; ++c) {
                Ak[(size_t)r * m + c] = hA[(size_t)idx[r] * n + idx[c]];
                Bk[(size_t)r * m + c] = hB[(size_t)idx[r] * n + idx[c]];
            }
        if ((rc = msm_sygv_top(Ak.data(), Bk.data(), m, 1, &hu, vk.data(), 0))) return rc;
        double sum = 0.0;
        for (msm_idx_t r = 0; r < m; ++r) sum += vk[r];
        const double sign = sum > 0.0 ? 1.0 : (sum < 0.0 ? -1.0 : 0.0);
        for (msm_idx_t r = 0; r < m; ++r) {
            const double val = vk[r] * sign;
            hv[idx[r]] = val == 0.0 ? 0.0 : val;   // (no negative zeros)
        }
    }
    *u = hu;
    if (x_out) MSM_HIP_CHECK(hipMemcpy(x_out, x.data(), n * sizeof(double), on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
    MSM_HIP_CHECK(hipMemcpy(v, hv.data(), n * sizeof(double), on_device ? hipMemcpyHostToDevice : hipMemcpyHostToHost));
    info[0] = (double)hs.outer;
    info[1] = (double)hs.total;
    info[2] = (double)launches;
    info[3] = hs.f;
    info[4] = (double)m;
    info[5] = (double)hs.status;
    info[6] = (double)grid;
    info[7] = tau;
    return MSM_OK;
}

int msm_scdeflate(const double* A, const double* x, msm_idx_t n, double* out, int on_device)
{
    if (!A || !x || !out) return fail(MSM_ERR_INVALID, "msm_scdeflate: null pointer");
    if (n < 1 || n > 32768) return fail(MSM_ERR_INVALID, "msm_scdeflate: need 1 <= n <= 32768");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const size_t nn = (size_t)n * n;
    DevBuf& buf = pool(PS_W);
    int rc = buf.reserve((2 * nn + 3 * (size_t)n) * sizeof(double));
    if (rc) return rc;
    double* dA = buf.as<double>();
    double* dO = dA + nn;
    double* dx = dO + nn;
    double* pv = dx + n;
    const double* srcA = A;
    const double* srcx = x;
    double* dst = out;
    if (!on_device) {
        if ((rc = spg_put(dA, A, nn, 0))) return rc;
        if ((rc = spg_put(dx, x, n, 0))) return rc;
        srcA = dA, srcx = dx, dst = dO;
    }   // (on the device out may be A itself: every thread of the second kernel reads and writes its own element only)
    const int N = (int)n;
    hipLaunchKernelGGL(scdeflate_products_kernel, dim3((unsigned)ceil_div(n, 4)), dim3(256), 0, stream(), srcA, srcx, N, pv);
    hipLaunchKernelGGL(scdeflate_apply_kernel, dim3((unsigned)ceil_div((int64_t)nn, 256)), dim3(256), 0, stream(), srcA, srcx, N, pv, dst);
    MSM_HIP_CHECK(hipGetLastError());
    if (!on_device) MSM_HIP_CHECK(hipMemcpyAsync(out, dO, nn * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

}  // extern "C"
