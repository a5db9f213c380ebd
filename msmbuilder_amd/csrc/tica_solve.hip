// tica_solve.hip -- the device-resident tICA solve on gfx950: finalise the moments of a handle, reduce the generalised
// problem to a standard one, and solve it for the top k pairs (tica.py:167-259, 492-524).  The kernels of the finalisation are
// tica_solve_dev.h; the factorisation, the iteration and the checks are eigsolve.hip, toppairs.hip and subspace.hip.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "tica_handle.h"      // struct msm_tica, tica_export_queue
#include "tica_solve_dev.h"   // finalise / RBLW / shrink / top-pairs kernels

using namespace msm;

namespace {

struct SolveBufs {
    double *A, *B, *mu, *D, *E, *scal, *part, *scale, *Y, *vals, *trdw;
    double *Winv, *T;             // U^-T of the factorisation (n <= 1024: reduction by GEMMs, back-transformation by a thin product), GEMM scratch
    double* sswork;               // subspace iteration workspace (subspace.hip)
    double *lam, *S, *Yk, *res;   // top-k tail (toppairs.hip): eigenvalues [64], back-transformed vectors [64][F], reduced vectors [64][F], checks [320]
    int* ints;  // [0..1] non-finite flags (OC, S), [2] potrf info, [3] syevd info; [8 ..] sytrd barrier flags + status
    int nblk;
};

// Carves h->solve into its regions by taking them off the buffer one after the other: once on a null base to count the
// doubles they need -- the ints follow them --, and again on the reserved buffer.
int solve_bufs(msm_tica* h, SolveBufs* b)
{
    const size_t F = (size_t)h->g.F, FF = F * F;
    b->nblk = (int)ceil_div((int64_t)FF, 256);
    double* base = nullptr;
    size_t used = 0;
    auto take = [&](size_t n) {
        double* p = base ? base + used : nullptr;
        used += n;
        return p;
    };
    auto carve = [&] {
        used = 0;
        b->A = take(FF), b->B = take(FF), b->Y = take(FF);
        b->mu = take(F), b->D = take(F), b->E = take(F), b->scale = take(F), b->vals = take(F);
        b->scal = take(4), b->part = take(2 * (size_t)b->nblk);
        b->trdw = take(8 * F);                  // sytrd exchange records
        b->lam = take(64), b->res = take(320);   // res: 2k + k^2 doubles, k <= 16
        b->S = take(64 * F), b->Yk = take(64 * F);
        b->sswork = take(subspace_work_doubles((int)F));
        b->Winv = take(FF), b->T = take(FF);
        b->ints = reinterpret_cast<int*>(take(0));
    };
    carve();
    int rc = h->solve.reserve(used * sizeof(double) + (8 + F / 16 + 4) * sizeof(int));
    if (rc) return rc;
    base = h->solve.as<double>();
    carve();
    return MSM_OK;
}

// the handle's pinned host buffer, at least n doubles of it (what it held is not kept)
int solve_pin_reserve(msm_tica* h, size_t n)
{
    if (h->solve_pin_n >= n) return MSM_OK;
    if (h->solve_pin) (void)hipHostFree(h->solve_pin);
    h->solve_pin = nullptr;
    h->solve_pin_n = 0;
    MSM_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&h->solve_pin), n * sizeof(double), hipHostMallocDefault));
    h->solve_pin_n = n;
    return MSM_OK;
}

// export -> finalise -> shrink -> B = L L^T -> A <- L^-1 A L^-T, all queued on the stream (no synchronisation)
int tica_reduce_device(msm_tica* h, double shrinkage, long long n_rblw, const double* scale_host, SolveBufs* b)
{
    int rc = solve_bufs(h, b);
    if (rc) return rc;
    const long long npairs = h->n_obs - (long long)h->g.lag * h->n_seq;
    if (h->n_obs <= 0 || npairs <= 0) return fail(MSM_ERR_STATE, "the model must be fit() before use");
    // the packed raw moments (slab sums, un-shifted) stay on the device
    if ((rc = tica_export_queue(h))) return rc;
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemsetAsync(b->ints, 0, 8 * sizeof(int), stream()));
    if (scale_host) MSM_HIP_CHECK(hipMemcpyAsync(b->scale, scale_host, h->g.F * sizeof(double), hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(tica_finalise_kernel, dim3((unsigned)b->nblk), dim3(256), 0, stream(), h->packed,
                       scale_host ? b->scale : (const double*)nullptr, 2.0 * (double)npairs, h->g.F, b->A, b->B, b->mu, b->part, b->ints);
    hipLaunchKernelGGL(tica_rblw_kernel, dim3(1), dim3(256), 0, stream(), b->part, b->nblk, shrinkage, (double)n_rblw, h->g.F, b->scal);
    hipLaunchKernelGGL(tica_shrink_kernel, dim3((unsigned)b->nblk), dim3(256), 0, stream(), b->B, b->scal, h->g.F);
    MSM_HIP_CHECK(hipGetLastError());
    if ((rc = sygv_reduce_device(b->A, b->B, h->g.F, b->ints + 2, b->Winv, b->T))) return rc;
    h->reduced = true;
    return MSM_OK;
}

// status of the queued reduction, after the stream was synchronised: info = {rho, tr S, flags...}
int tica_reduce_status(const double scal[4], const int ints[8], double* info)
{
    if (info) {
        info[0] = scal[0];
        info[1] = scal[1];
        info[2] = (double)ints[2];
        info[3] = (double)ints[3];
        info[4] = (double)ints[0];
        info[5] = (double)ints[1];
    }
    if (ints[0]) return fail(MSM_ERR_NONFINITE, "offset correlation matrix is not symmetric");
    if (ints[1]) return fail(MSM_ERR_NONFINITE, "correlation matrix is not symmetric");
    if (ints[2] != 0)
        return fail(MSM_ERR_INVALID, "The leading minor of order %d of B is not positive definite. The factorization of B "
                    "could not be completed and no eigenvalues or eigenvectors were computed.", ints[2]);
    return MSM_OK;
}

// The outcome of a queued reduction: the reduced matrix (to Cs, when given), the means and the status words (to ints8, when
// given) are copied to the host behind whatever is queued, the stream is synchronised ONCE, and the status is reported.
int tica_reduce_fetch(msm_tica* h, const SolveBufs& b, double* Cs, double* mu, double* info, int* ints8 = nullptr)
{
    const size_t F = (size_t)h->g.F;
    double scal[4];
    int ints[8];
    if (Cs) MSM_HIP_CHECK(hipMemcpyAsync(Cs, b.A, F * F * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(mu, b.mu, F * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(scal, b.scal, sizeof(scal), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(ints, b.ints, sizeof(ints), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (ints8) memcpy(ints8, ints, sizeof(ints));
    return tica_reduce_status(scal, ints, info);
}

// The results of a top-k solve gathered into ONE buffer for one device-to-host copy (seven small copies into pageable host
// arrays cost 20-40 us each): [vals k | checks 2k + k^2 | scal 4 | ints 8 | mu n | vecs k n].  The offsets of the parts, in doubles.
struct SolvePacked {
    size_t res, scal, ints, mu, vecs, total;
    __host__ __device__ SolvePacked(int n, int k)
        : res(k), scal(res + (2 * k + k * k)), ints(scal + 4), mu(ints + 8), vecs(mu + n), total(vecs + (size_t)k * n) {}
};

__global__ void tica_solve_emit_kernel(const double* __restrict__ lam, const double* __restrict__ res, const double* __restrict__ scal,
                                       const int* __restrict__ ints, const double* __restrict__ mu, const double* __restrict__ vecs,
                                       int n, int k, double* __restrict__ out)
{
    const SolvePacked o(n, k);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < o.total; e += (size_t)gridDim.x * blockDim.x) {
        double v;
        if (e < o.res) v = lam[e];
        else if (e < o.scal) v = res[e - o.res];
        else if (e < o.ints) v = scal[e - o.scal];
        else if (e < o.mu) v = (double)ints[e - o.ints];
        else if (e < o.vecs) v = mu[e - o.mu];
        else v = vecs[e - o.vecs];
        out[e] = v;
    }
}

}  // namespace

extern "C" {

int msm_tica_reduce(msm_tica_t* h, double shrinkage, msm_idx_t n_rblw, const double* scale, double* Cs, double* mu, double* info)
{
    if (!h || !Cs || !mu) return fail(MSM_ERR_STATE, "msm_tica_reduce: null argument");
    SolveBufs b;
    int rc = tica_reduce_device(h, shrinkage, n_rblw, scale, &b);
    if (rc) return rc;
    return tica_reduce_fetch(h, b, Cs, mu, info);
}

int msm_tica_solve_topk(msm_tica_t* h, double shrinkage, msm_idx_t n_rblw, const double* scale, msm_idx_t k, double* vals,
                        double* vecs, double* Cs, double* mu, double* info, int* status)
{
    if (!h || !vals || !vecs || !Cs || !mu || !status) return fail(MSM_ERR_STATE, "msm_tica_solve_topk: null argument");
    if (h->g.F > 1024 || h->g.F < 128) return fail(MSM_ERR_INVALID, "msm_tica_solve_topk: need 128 <= n_features <= 1024");
    if (k < 1 || k > 16) return fail(MSM_ERR_INVALID, "msm_tica_solve_topk: need 1 <= k <= 16");
    SolveBufs b;
    int rc = tica_reduce_device(h, shrinkage, n_rblw, scale, &b);
    if (rc) return rc;
    const int n = h->g.F;
    const size_t FF = (size_t)n * n;
    // Chebyshev-filtered subspace iteration (subspace.hip): a few short launch chains when the spectrum has the gap tICA is
    // run for; the reduced tICA matrix has its spectrum in [-1, 1].  When it does not converge (flat spectra: white-noise
    // features) the reduced matrix goes back to the caller, whose verified fallback is LAPACK's dsyevr on it (round 3 had a
    // second device route in between -- cooperative tridiagonalisation + multisection + inverse iteration; removed in round
    // 4: two routes, one fallback).
    int conv = 0, outer = 0;
    // pinned host memory of the handle: [results of the solve, at the largest k | staging of the iteration's Rayleigh-Ritz steps]
    const size_t pin_res = SolvePacked(n, 16).total;
    if ((rc = solve_pin_reserve(h, pin_res + subspace_pin_doubles()))) return rc;
    // (Round 5 built the iteration QUEUED -- the 32 x 32 Rayleigh-Ritz problems by one-sided Jacobi in one workgroup, every decision
    //  on the device, one synchronisation per solve -- and removed it again: a Jacobi round is a chain of shuffles, square roots
    //  and divisions, ~0.5 us of latency, 31 rounds a sweep, and the kernel took 0.2 ms per Rayleigh-Ritz round against ~0.13 ms
    //  for the two copies, two synchronisations and 25 us of host arithmetic it replaced: solve 1.26 ms against 1.08 ms.  DESIGN 3.9.)
    if ((rc = subspace_topk_device(b.A, n, (int)k, -1.02, 5e-12, 10, 6, b.lam, b.Yk, b.sswork, h->solve_pin + pin_res, &conv, &outer,
                                   0.0, 1.0)))   // prior: the reduced tICA matrix has its spectrum in [-1, 1], the noise bulk near 0
        return rc;
    if (!conv) {
        if ((rc = tica_reduce_fetch(h, b, Cs, mu, info))) return rc;
        if (info) {
            info[8] = 0.0;
            info[9] = (double)outer;
        }
        *status = 1;
        return MSM_OK;
    }
    if ((rc = pair_residual_device(b.A, n, b.Yk, b.lam, (int)k, b.res))) return rc;
    // the vectors of the original problem: S = U^-1 Yk = W^T Yk (n <= 1024 here: W = U^-T was formed with the factor)
    if ((rc = winv_back_device(b.Winv, n, b.Yk, (int)k, b.S))) return rc;
    // one packed copy of everything the caller gets (b.Y, n^2 doubles, is free at this point)
    const SolvePacked o(n, (int)k);
    if (o.total > pin_res) return fail(MSM_ERR_STATE, "msm_tica_solve_topk: result staging too small");
    hipLaunchKernelGGL(tica_solve_emit_kernel, dim3((unsigned)ceil_div(o.total, 256)), dim3(256), 0, stream(), b.lam, b.res, b.scal, b.ints, b.mu,
                       b.S, n, (int)k, b.Y);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(h->solve_pin, b.Y, o.total * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    const double* hp = h->solve_pin;
    const double* res = hp + o.res;
    int ints[8];
    for (int i = 0; i < 8; ++i) ints[i] = (int)hp[o.ints + i];
    memcpy(vals, hp, (size_t)k * sizeof(double));
    memcpy(mu, hp + o.mu, (size_t)n * sizeof(double));
    memcpy(vecs, hp + o.vecs, (size_t)k * n * sizeof(double));
    if ((rc = tica_reduce_status(hp + o.scal, ints, info))) return rc;
    if (info) {
        info[8] = 1.0;                // the pairs came from the subspace iteration
        info[9] = (double)outer;      // filtered iterations spent (also when they did not converge)
    }
    // self-check on the reduced matrix: every returned pair must satisfy C y = lambda y to rounding, be normalised, and the
    // k vectors must be mutually orthogonal (a rank-deficient block would pass the per-pair checks; the Gram
    // matrix of the vectors comes from the residual kernel).  A failure hands the reduced matrix to the caller's LAPACK
    // route instead of returning a wrong pair.
    constexpr double RES_TOL = 1e-11;    // |C y - lambda y|, relative to the largest |lambda| (at least 1)
    constexpr double NORM_TOL = 1e-10;   // | |y|^2 - 1 |
    constexpr double ORTH_TOL = 1e-8;    // |y_i . y_j|, i != j
    double lmax = 1.0, rmax = 0.0, nmax = 0.0, omax = 0.0;
    for (int j = 0; j < (int)k; ++j) {
        lmax = std::max(lmax, std::fabs(vals[j]));
        rmax = std::max(rmax, res[j]);
        nmax = std::max(nmax, res[k + j]);
        for (int i = 0; i < j; ++i) {
            const double dot = res[2 * k + (size_t)j * k + i];
            omax = std::max(omax, (dot == dot) ? std::fabs(dot) : INFINITY);
        }
    }
    if (info) {
        info[6] = rmax;
        info[7] = std::max(nmax, omax);
    }
    *status = (!(rmax <= RES_TOL * lmax) || !(nmax <= NORM_TOL) || !(omax <= ORTH_TOL)) ? 2 : 0;
    if (*status) {
        MSM_HIP_CHECK(hipMemcpyAsync(Cs, b.A, FF * sizeof(double), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    }
    return MSM_OK;
}

int msm_tica_backsolve(msm_tica_t* h, const double* Y, msm_idx_t k, double* V)
{
    if (!h || !Y || !V) return fail(MSM_ERR_STATE, "msm_tica_backsolve: null argument");
    if (!h->reduced) return fail(MSM_ERR_STATE, "msm_tica_backsolve: no reduced problem (call msm_tica_reduce first)");
    if (k < 1 || k > h->g.F) return fail(MSM_ERR_INVALID, "msm_tica_backsolve: need 1 <= k <= n_features");
    SolveBufs b;
    int rc = solve_bufs(h, &b);
    if (rc) return rc;
    const size_t bytes = (size_t)k * h->g.F * sizeof(double);
    MSM_HIP_CHECK(hipMemcpyAsync(b.Y, Y, bytes, hipMemcpyHostToDevice, stream()));
    if (h->g.F <= 1024 && k <= 64) {
        if ((rc = winv_back_device(b.Winv, h->g.F, b.Y, (int)k, b.S))) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(V, b.S, bytes, hipMemcpyDeviceToHost, stream()));
    } else {
        if ((rc = sygv_back_device(b.B, b.Y, h->g.F, (int)k))) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(V, b.Y, bytes, hipMemcpyDeviceToHost, stream()));
    }
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_tica_solve_device(msm_tica_t* h, double shrinkage, msm_idx_t n_rblw, const double* scale, msm_idx_t k,
                          double* vals, double* vecs, double* mu, double* info)
{
    if (!h || !vals || !vecs || !mu) return fail(MSM_ERR_STATE, "msm_tica_solve_device: null argument");
    if (k < 1 || k > h->g.F) return fail(MSM_ERR_INVALID, "msm_tica_solve_device: need 1 <= k <= n_features");
    SolveBufs b;
    int rc = tica_reduce_device(h, shrinkage, n_rblw, scale, &b);
    if (rc) return rc;
    const int n = h->g.F;
    h->reduced = false;  // A is overwritten by the eigenvectors
    if ((rc = syevd_device(b.A, n, b.D, b.E, b.ints + 3))) return rc;
    if ((rc = sygv_back_device(b.B, b.A + (size_t)(n - k) * n, n, (int)k))) return rc;
    hipLaunchKernelGGL(tica_top_pairs_kernel, dim3((unsigned)ceil_div(n, 256), (unsigned)k), dim3(256), 0, stream(), b.A, b.D, n,
                       (int)k, b.Y, b.vals);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(vecs, b.Y, (size_t)k * n * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(vals, b.vals, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, stream()));
    int ints[8];
    if ((rc = tica_reduce_fetch(h, b, nullptr, mu, info, ints))) return rc;   // (no Cs: the reduced matrix is gone)
    if (ints[3] != 0) return fail(MSM_ERR_INVALID, "eigenvalue iteration did not converge (info = %d)", ints[3]);
    return MSM_OK;
}

}  // extern "C"
