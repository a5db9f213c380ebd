// msm_mle.hip -- reversible maximum-likelihood transition matrix (Prinz et al. 2011, the estimator behind
// MarkovStateModel(reversible_type='mle')), solved on the device.
//
// The likelihood's stationarity conditions, written on the unnormalised populations x, are a fixed point:
//     Cs = C + C^T,  c_i = sum_j C_ij,  d_j = c_j / x_j,  g_i(x) = sum_j Cs_ij / (d_i + d_j),  x = g(x).
// g is homogeneous of degree 1, so x is iterated on the simplex (normalised after every step), and the plain
// iteration -- slow on metastable data, where it contracts like the chain mixes -- is Anderson-accelerated over
// the last MLE_AM iterates.  The m x m least-squares problem of the mixing is solved by one thread from an
// incrementally updated Gram matrix (normal equations, no ridge: a ridge biases the mixing once the residuals are
// small, and the iteration stalls -- 1e-10 relative stalled a 3,000-state banded chain near 1e-10); a mixed step
// with any x_i <= 0, or a singular or non-finite solve, falls back to the plain step.  Stopping rule:
// max|g(x) - x| / max g(x) < tol AND max_i |g_i(x) - x_i| / g_i(x) < MLE_STATE_TOL.  The first alone leaves a state of
// population p converged only to tol / p of itself (measured: 1e-4 relative on the rarest state of a ten-decade range, and
// T, formed from x, 4e-12 off its closed form in pi = g(x) / sum g on a 6,145-state hub); the second is 1e-13, above the
// rounding of a K-term row sum (~sqrt(K) eps <= 1.4e-14) and below what T's closed form needs.
// On exit X_ij = Cs_ij / (d_i + d_j), x_rs = row sums of X, T = X / x_rs, pi = x_rs / sum(x_rs), and the
// symmetric S = D^-1/2 X D^-1/2 (D = diag(x_rs)), which has T's eigenvalues.
//
// The whole solve is ONE workgroup of 1024 threads in one launch: every iteration is a handful of dependent
// block-wide reductions, and a grid barrier per reduction costs more than the matrix-vector product it would
// spread (K = 3000 sparse: ~1.5 MB of pattern per iteration, L2-resident).  Storage:
//   sparse  sliced ELL over the symmetric nonzero pattern of Cs: slices of 64 rows (one wave), each padded to
//           the slice's longest row and stored column-major, so a thread per row reads coalesced; padding
//           entries carry value 0 and their own row as column;
//   dense   Cs as K x K; thread i reads Cs[j][i] (= Cs[i][j], symmetric) for all j -- coalesced as well.
// prior_counts > 0 fills every entry: dense.  MSM_MLE_DENSE=1 forces the dense form (the tests' A/B switch).
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

namespace msm {
namespace {

constexpr int MLE_T = 1024;         // threads of the one workgroup
constexpr int MLE_WAVES = MLE_T / 64;
constexpr int MLE_AM = 6;           // Anderson depth
constexpr int MLE_LDS_K = 6144;     // d lives in LDS up to this many states (48 KiB), in global memory beyond
constexpr int MLE_MAX_K = 16384;
constexpr double MLE_STATE_TOL = 1e-13;   // per-state relative residual at convergence

struct MleArgs {
    int K;
    int dense;
    const int* slice_ptr;   // sparse: [ceil(K/64) + 1] element offset of each 64-row slice
    const int* col;         // sparse: column of the k-th entry of row 64 s + r at slice_ptr[s] + 64 k + r
    const double* val;      // sparse: Cs at the same place; dense: Cs, K x K
    const double* c;        // [K] row sums of C
    double* x;              // [K] iterate (sum 1); on exit the converged x
    double* dg;             // [K] d when K > MLE_LDS_K
    double* g;              // [K] g(x); on exit x_rs
    double* Fp;             // [K] previous residual G - x
    double* Gp;             // [K] previous normalised image G = g / sum g
    double* dF;             // [MLE_AM][K] residual differences
    double* dG;             // [MLE_AM][K] image differences
    double* pi;             // [K] out
    double* info;           // out: iterations, converged (0/1), last step, KKT residual at pi; then the counts of mixed
                            // steps accepted, mixed steps rejected as not positive, solves rejected (singular / non-finite)
    int max_iter;
    double tol;
};

__device__ __forceinline__ double row_g(const MleArgs& A, const double* d, int i, double di)
{
    double acc = 0.0;
    if (A.dense) {
        const double* v = A.val + i;
        for (int j = 0; j < A.K; ++j) acc += v[(size_t)j * A.K] / (di + d[j]);
    } else {
        const int s = i >> 6;
        const int e = A.slice_ptr[s + 1];
        for (int p = A.slice_ptr[s] + (i & 63); p < e; p += 64) acc += A.val[p] / (di + d[A.col[p]]);
    }
    return acc;
}

__device__ __forceinline__ double row_cs(const MleArgs& A, int i)
{
    double acc = 0.0;
    if (A.dense) {
        const double* v = A.val + i;
        for (int j = 0; j < A.K; ++j) acc += v[(size_t)j * A.K];
    } else {
        const int s = i >> 6;
        const int e = A.slice_ptr[s + 1];
        for (int p = A.slice_ptr[s] + (i & 63); p < e; p += 64) acc += A.val[p];
    }
    return acc;
}

// NV block-wide sums (MAX = false) or maxima (MAX = true); every thread gets the results in tot[0 .. NV)
template <int NV, bool MAX>
__device__ __forceinline__ void block_reduce(double (&v)[NV], double (*red)[2 * MLE_AM], double* tot)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double a = v[q];
        for (int o = 32; o > 0; o >>= 1) {
            const double b = __shfl_xor(a, o);
            a = MAX ? fmax(a, b) : a + b;
        }
        if (lane == 0) red[w][q] = a;
    }
    __syncthreads();
    if ((int)threadIdx.x < NV) {
        double a = red[0][threadIdx.x];
        for (int u = 1; u < MLE_WAVES; ++u) a = MAX ? fmax(a, red[u][threadIdx.x]) : a + red[u][threadIdx.x];
        tot[threadIdx.x] = a;
    }
    __syncthreads();
}

// gam <- M^-1 r for the n x n leading block (Gaussian elimination, partial pivoting); false if singular
__device__ bool small_solve(const double (*M)[MLE_AM], const double* r, int n, double* gam)
{
    double a[MLE_AM][MLE_AM + 1];
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < n; ++j) a[i][j] = M[i][j];
        a[i][n] = r[i];
    }
    for (int k = 0; k < n; ++k) {
        int p = k;
        for (int i = k + 1; i < n; ++i)
            if (fabs(a[i][k]) > fabs(a[p][k])) p = i;
        if (!(fabs(a[p][k]) > 0.0)) return false;
        if (p != k)
            for (int j = k; j <= n; ++j) {
                const double t = a[k][j];
                a[k][j] = a[p][j];
                a[p][j] = t;
            }
        for (int i = k + 1; i < n; ++i) {
            const double f = a[i][k] / a[k][k];
            for (int j = k; j <= n; ++j) a[i][j] -= f * a[k][j];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = a[i][n];
        for (int j = i + 1; j < n; ++j) s -= a[i][j] * gam[j];
        gam[i] = s / a[i][i];
        if (!isfinite(gam[i])) return false;
    }
    return true;
}

__global__ __launch_bounds__(MLE_T) void mle_solve_kernel(MleArgs A)
{
    __shared__ double sd[MLE_LDS_K];
    __shared__ double red[MLE_WAVES][2 * MLE_AM];
    __shared__ double tot[2 * MLE_AM];
    __shared__ double gram[MLE_AM][MLE_AM];
    __shared__ double gam[MLE_AM];
    __shared__ int mix;
    const int K = A.K, tid = threadIdx.x;
    double* d = K <= MLE_LDS_K ? sd : A.dg;

    {   // start from the row sums of Cs (the reference's initial X = Cs), normalised
        double s[1] = {0.0};
        for (int i = tid; i < K; i += MLE_T) {
            const double v = row_cs(A, i);
            A.x[i] = v;
            s[0] += v;
        }
        block_reduce<1, false>(s, red, tot);
        const double inv = 1.0 / tot[0];
        for (int i = tid; i < K; i += MLE_T) A.x[i] *= inv;
    }
    int it = 0, mk = 0, slot = 0, conv = 0;
    int n_mixed = 0, n_nonpos = 0, n_sing = 0;   // uniform over the workgroup: they follow shared decisions
    double step = INFINITY, sg = 0.0;
    for (;; ++it) {
        for (int i = tid; i < K; i += MLE_T) d[i] = A.c[i] / A.x[i];
        __syncthreads();
        double mm[3] = {0.0, 0.0, 0.0}, ss[1] = {0.0};
        for (int i = tid; i < K; i += MLE_T) {
            const double gi = row_g(A, d, i, d[i]);
            A.g[i] = gi;
            ss[0] += gi;
            mm[0] = fmax(mm[0], gi);
            mm[1] = fmax(mm[1], fabs(gi - A.x[i]));
            mm[2] = fmax(mm[2], fabs(gi - A.x[i]) / gi);
        }
        block_reduce<3, true>(mm, red, tot);
        step = tot[1] / tot[0];
        const double state_step = tot[2];
        block_reduce<1, false>(ss, red, tot);
        sg = tot[0];
        if (step < A.tol && state_step < MLE_STATE_TOL) {
            conv = 1;
            break;
        }
        if (!(step == step) || it >= A.max_iter) break;
        // G = g / sum g, F = G - x; the newest differences go to ring slot `slot`
        const double inv = 1.0 / sg;
        const int mn = it > 0 ? min(mk + 1, MLE_AM) : 0;
        double dots[2 * MLE_AM];
#pragma unroll
        for (int q = 0; q < 2 * MLE_AM; ++q) dots[q] = 0.0;
        for (int i = tid; i < K; i += MLE_T) {
            const double Gi = A.g[i] * inv, Fi = Gi - A.x[i];
            if (mn > 0) {
                const double dFi = Fi - A.Fp[i];
                A.dF[(size_t)slot * K + i] = dFi;
                A.dG[(size_t)slot * K + i] = Gi - A.Gp[i];
#pragma unroll
                for (int j = 0; j < MLE_AM; ++j) {
                    if (j < mn) {
                        const double dFj = j == slot ? dFi : A.dF[(size_t)j * K + i];
                        dots[j] += dFi * dFj;
                        dots[MLE_AM + j] += dFj * Fi;
                    }
                }
            }
            A.Fp[i] = Fi;
            A.Gp[i] = Gi;
        }
        if (mn > 0) {
            block_reduce<2 * MLE_AM, false>(dots, red, tot);
            if (tid == 0) {
                for (int j = 0; j < mn; ++j) gram[slot][j] = gram[j][slot] = tot[j];
                mix = small_solve(gram, tot + MLE_AM, mn, gam) ? 1 : 0;
            }
            mk = mn;
            slot = (slot + 1) % MLE_AM;
        } else if (tid == 0) {
            mix = 0;
        }
        __syncthreads();
        int use = mix;
        if (mn > 0 && !use) ++n_sing;
        if (use) {   // x_new = G - dG gam; accepted only if every entry is positive (and finite)
            double acc[2] = {0.0, 0.0};
            for (int i = tid; i < K; i += MLE_T) {
                double v = A.Gp[i];
                for (int j = 0; j < mk; ++j) v -= gam[j] * A.dG[(size_t)j * K + i];
                A.g[i] = v;   // g is dead until the next product: holds the candidate
                acc[0] += v;
                if (!(v > 0.0)) acc[1] += 1.0;
            }
            block_reduce<2, false>(acc, red, tot);
            use = tot[1] == 0.0 && tot[0] > 0.0 && isfinite(tot[0]);
            const double s = tot[0];
            if (use)
                for (int i = tid; i < K; i += MLE_T) A.x[i] = A.g[i] / s;
            use ? ++n_mixed : ++n_nonpos;
        }
        if (!use)
            for (int i = tid; i < K; i += MLE_T) A.x[i] = A.Gp[i];
        __syncthreads();
    }
    // populations, then the certificate: the fixed-point residual evaluated at pi itself
    const double inv = 1.0 / sg;
    for (int i = tid; i < K; i += MLE_T) A.pi[i] = A.g[i] * inv;
    __syncthreads();
    for (int i = tid; i < K; i += MLE_T) d[i] = A.c[i] / A.pi[i];
    __syncthreads();
    double mm[2] = {0.0, 0.0};
    for (int i = tid; i < K; i += MLE_T) {
        const double gi = row_g(A, d, i, d[i]);
        mm[0] = fmax(mm[0], A.pi[i]);
        mm[1] = fmax(mm[1], fabs(gi - A.pi[i]));
    }
    block_reduce<2, true>(mm, red, tot);
    if (tid == 0) {
        A.info[0] = (double)it;
        A.info[1] = (double)conv;
        A.info[2] = step;
        A.info[3] = tot[1] / tot[0];
        A.info[4] = (double)n_mixed;
        A.info[5] = (double)n_nonpos;
        A.info[6] = (double)n_sing;
    }
}

// T = X / x_rs and S = X / sqrt(x_rs_i x_rs_j), X_ij = Cs_ij / (d_i + d_j), d = c / x (the solve's last iterate).
// Sparse: a thread per row writes its pattern entries (T and S zeroed beforehand); dense: a thread per entry.
__global__ void mle_out_sparse_kernel(MleArgs A, double* __restrict__ T, double* __restrict__ S)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.K) return;
    const int K = A.K;
    const double di = A.c[i] / A.x[i], ri = A.g[i];
    const int s = i >> 6;
    const int e = A.slice_ptr[s + 1];
    for (int p = A.slice_ptr[s] + (i & 63); p < e; p += 64) {
        const double v = A.val[p];
        if (v == 0.0) continue;   // padding
        const int j = A.col[p];
        const double X = v / (di + A.c[j] / A.x[j]);
        T[(size_t)i * K + j] = X / ri;
        S[(size_t)i * K + j] = X / sqrt(ri * A.g[j]);
    }
}

__global__ void mle_out_dense_kernel(MleArgs A, double* __restrict__ T, double* __restrict__ S)
{
    const int K = A.K;
    const int i = blockIdx.y;
    const double di = A.c[i] / A.x[i], ri = A.g[i];
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < K; j += gridDim.x * blockDim.x) {
        const double X = A.val[(size_t)i * K + j] / (di + A.c[j] / A.x[j]);
        T[(size_t)i * K + j] = X / ri;
        S[(size_t)i * K + j] = X / sqrt(ri * A.g[j]);
    }
}

int64_t g_mle_stats[3] = {0, 0, 0};   // the last solve's info[4 .. 7)

}  // namespace
}  // namespace msm

using namespace msm;

extern "C" {

int msm_transmat_mle(const double* C, msm_idx_t n, double prior, msm_idx_t max_iter, double* T, double* pi, double* S,
                     double* info)
{
    if (!C || !T || !pi || !info) return fail(MSM_ERR_INVALID, "msm_transmat_mle: null pointer");
    if (n < 1 || n > MLE_MAX_K) return fail(MSM_ERR_INVALID, "msm_transmat_mle: need 1 <= n <= %d", MLE_MAX_K);
    if (max_iter < 0 || max_iter > (msm_idx_t)1 << 30) return fail(MSM_ERR_INVALID, "msm_transmat_mle: bad max_iter");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const int K = (int)n;
    const size_t KK = (size_t)K * K;
    // row sums and the domain checks (the reference's error codes and messages)
    std::vector<double> c(K, 0.0), colsum(K, 0.0);
    bool negative = false, zero_row = false, nonfinite = false;
    for (int i = 0; i < K; ++i) {
        double s = 0.0;
        for (int j = 0; j < K; ++j) {
            const double v = C[(size_t)i * K + j] + prior;
            negative |= v < 0.0;
            nonfinite |= !std::isfinite(v);
            s += v;
            colsum[j] += v;
        }
        c[i] = s;
        zero_row |= s == 0.0;
    }
    // the reference's codes: -1 when a row sum of C or of C + C^T is not positive, -2 when negative entries get
    // past that check (its sweep fails on them); the messages are the ones its wrapper composes
    bool rows_bad = false;
    for (int i = 0; i < K && !rows_bad; ++i) rows_bad = !(c[i] > 0.0) || !(c[i] + colsum[i] > 0.0);
    const bool dense = prior != 0.0 || (getenv("MSM_MLE_DENSE") && atoi(getenv("MSM_MLE_DENSE")) == 1);   // read per call
    // Cs = (C + p) + (C + p)^T, row-major, built in 64 x 64 tiles (the transposed read stays in cache)
    std::vector<double> cs(KK);
    for (int i0 = 0; i0 < K; i0 += 64)
        for (int j0 = 0; j0 < K; j0 += 64)
            for (int i = i0; i < std::min(K, i0 + 64); ++i)
                for (int j = j0; j < std::min(K, j0 + 64); ++j)
                    cs[(size_t)i * K + j] = (C[(size_t)i * K + j] + prior) + (C[(size_t)j * K + i] + prior);
    // NaN or infinite counts: the reference's solver returns -2 on them (its sweep fails), and its wrapper has no text of
    // its own for that; they are a domain error like the negative entries that share the code
    if (nonfinite) return fail(MSM_ERR_INVALID, "Domain error. C must be positive. Error code=-2");
    if (rows_bad || negative) {
        std::string msg = rows_bad ? " Error code=-1" : " Error code=-2";
        if (negative) msg = "Domain error. C must be positive." + msg;
        if (zero_row) msg = "Row-sums of C must be positive." + msg;
        return fail(MSM_ERR_INVALID, "%s", msg.c_str());
    }
    // sliced ELL of the pattern (sparse form)
    const int ns = (int)ceil_div(K, 64);
    std::vector<int> sptr(ns + 1, 0), col;
    std::vector<double> val;
    if (!dense) {
        std::vector<int> len(K, 0);
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) len[i] += cs[(size_t)i * K + j] != 0.0;
        for (int s = 0; s < ns; ++s) {
            int w = 0;
            for (int r = 0; r < 64 && 64 * s + r < K; ++r) w = std::max(w, len[64 * s + r]);
            sptr[s + 1] = sptr[s] + 64 * w;
        }
        col.assign(sptr[ns], 0);   // rows past K in the last slice: column 0, value 0 (never read)
        val.assign(sptr[ns], 0.0);
        for (int i = 0; i < K; ++i) {
            const int s = i >> 6, r = i & 63;
            const int w = (sptr[s + 1] - sptr[s]) / 64;
            int k = 0;
            for (int j = 0; j < K; ++j) {
                const double v = cs[(size_t)i * K + j];
                if (v == 0.0) continue;
                col[sptr[s] + 64 * k + r] = j;
                val[sptr[s] + 64 * k + r] = v;
                ++k;
            }
            for (; k < w; ++k) col[sptr[s] + 64 * k + r] = i;   // padding: value 0, own column
        }
    }
    const size_t nval = dense ? KK : (size_t)sptr[ns];
    int rc;
    DevBuf &dV = pool(PS_X), &dI = pool(PS_IDX), &dW = pool(PS_W), &dO = pool(PS_OUT);
    const size_t nvec = (size_t)(8 + 2 * MLE_AM) * K;
    if ((rc = dV.reserve(std::max<size_t>(nval, 1) * sizeof(double)))) return rc;
    if ((rc = dI.reserve(((size_t)ns + 1 + col.size()) * sizeof(int) + 16))) return rc;
    if ((rc = dW.reserve((nvec + 8) * sizeof(double)))) return rc;
    if ((rc = dO.reserve(2 * KK * sizeof(double)))) return rc;
    MleArgs A;
    A.K = K;
    A.dense = dense ? 1 : 0;
    int* ip = dI.as<int>();
    A.slice_ptr = ip;
    A.col = ip + ns + 1;
    A.val = dV.as<double>();
    double* w = dW.as<double>();
    A.c = w;
    A.x = w + (size_t)K;
    A.dg = w + (size_t)2 * K;
    A.g = w + (size_t)3 * K;
    A.Fp = w + (size_t)4 * K;
    A.Gp = w + (size_t)5 * K;
    A.pi = w + (size_t)6 * K;
    A.dF = w + (size_t)8 * K;
    A.dG = A.dF + (size_t)MLE_AM * K;
    A.info = w + nvec;
    A.max_iter = (int)max_iter;
    A.tol = 1e-14;
    if (dense) {
        if ((rc = h2d_bulk(dV.p, cs.data(), KK * sizeof(double)))) return rc;
    } else {
        MSM_HIP_CHECK(hipMemcpyAsync(ip, sptr.data(), (ns + 1) * sizeof(int), hipMemcpyHostToDevice, stream()));
        if (!col.empty()) {
            MSM_HIP_CHECK(hipMemcpyAsync(ip + ns + 1, col.data(), col.size() * sizeof(int), hipMemcpyHostToDevice, stream()));
            MSM_HIP_CHECK(hipMemcpyAsync(dV.p, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
        }
    }
    MSM_HIP_CHECK(hipMemcpyAsync(w, c.data(), K * sizeof(double), hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(mle_solve_kernel, dim3(1), dim3(MLE_T), 0, stream(), A);
    MSM_HIP_CHECK(hipGetLastError());
    double hinfo[7];
    MSM_HIP_CHECK(hipMemcpyAsync(hinfo, A.info, sizeof(hinfo), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    for (int q = 0; q < 4; ++q) info[q] = hinfo[q];
    for (int q = 0; q < 3; ++q) g_mle_stats[q] = (int64_t)hinfo[4 + q];
    if (hinfo[1] != 1.0) return fail(MSM_ERR_INVALID, "Likelihood not converged. Error code=-3");
    double* dT = dO.as<double>();
    double* dS = dT + KK;
    if (dense) {
        hipLaunchKernelGGL(mle_out_dense_kernel, dim3((unsigned)std::min<int64_t>(ceil_div(K, 256), 16), (unsigned)K), dim3(256), 0,
                           stream(), A, dT, dS);
    } else {
        MSM_HIP_CHECK(hipMemsetAsync(dT, 0, 2 * KK * sizeof(double), stream()));
        hipLaunchKernelGGL(mle_out_sparse_kernel, dim3((unsigned)ceil_div(K, 256)), dim3(256), 0, stream(), A, dT, dS);
    }
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(pi, A.pi, K * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if ((rc = d2h_bulk(T, dT, KK * sizeof(double)))) return rc;
    if (S && (rc = d2h_bulk(S, dS, KK * sizeof(double)))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_mle_last_stats(msm_idx_t* out3)
{
    if (!out3) return fail(MSM_ERR_INVALID, "msm_mle_last_stats: null pointer");
    for (int q = 0; q < 3; ++q) out3[q] = g_mle_stats[q];
    return MSM_OK;
}

}  // extern "C"
