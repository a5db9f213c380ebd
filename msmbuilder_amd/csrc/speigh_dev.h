// speigh_dev.h -- the sparse generalized eigenpair solver of SparseTICA as ONE persistent launch.
//
//   maximise  x^T A x - rho_e sum_j log(|x_j| + eps)   subject to  x^T B x <= 1
//
// by majorisation-minimisation (Sriperumbudur, Torres, Lanckriet 2011): every outer step linearises the penalty at x and
// solves  min 1/2 |x - b|^2 + |D(w) x|_1  s.t. x^T B x <= 1  by ADMM, whose every iteration is a soft threshold, a
// projection onto the ellipsoid (c = E a, Newton on the multiplier mu, z = E^T (c / (mu lambda + 1)) with B = E^T diag(lambda) E)
// and the residual / penalty bookkeeping.  Everything is float64 and every step depends on the one before it, so the
// launch is a loop over two matrix-vector products with F-vectors of state in LDS.
//
// Two layouts, one code:
//   LDSV = true    one workgroup, E staged in LDS (n <= SPG_LDS_N), no grid barrier
//   LDSV = false   NB <= CU count workgroups, each owning rows [r0, r1) of A, E and the stored E^T: a product is one row dot
//                  per owned row, published to device memory (agent scope), a grid barrier, and every workgroup reads the
//                  whole F-vector back.  All the O(F) work -- soft threshold, Newton's sums, residual norms, penalty update,
//                  stop tests -- is recomputed by EVERY workgroup from the published vectors, so all take the same branches.
//
// Determinism: a row dot is formed by one wavefront (lane l adds the terms l, l + 64, ... in order, then a butterfly over
// the lanes) and every sum over F by the same rule, so the order of every sum depends on F only -- not on the grid, the
// layout or where a launch was cut.
#pragma once
#include "common.h"

namespace msm {

constexpr int SPG_T = 512;        // threads per workgroup (8 wavefronts)
constexpr int SPG_MAXN = 2048;    // 8 F-vectors of doubles in LDS: 128 KiB at 2,048
constexpr int SPG_LDS_N = 128;    // widest E (pitch n | 1) that fits beside them: 129 KiB + 8 KiB at 128
constexpr int SPG_NVEC = 8;

enum { SPG_RUNNING = -1, SPG_CONVERGED = 0, SPG_MAXITER = 1, SPG_TIMEOUT = 2 };
enum { SPG_PAIR = 0, SPG_ADMM = 1, SPG_PROJECT = 2 };

struct SpgState {                 // device memory; carries a solve from one launch to the next
    double rho, f, f_old, tau, rho_e, eps, tol;
    long long maxiter, outer, total, k;   // outer steps done, ADMM iterations done (all / in the current solve)
    int phase;                    // 0: at the head of an outer step, 1: inside an ADMM solve
    int status, mode, pad;
    unsigned bar, timed_out;      // grid barrier: arrivals of this launch, the timeout word
};

struct SpgArgs {
    const double* A;              // n x n (pair mode)
    const double* E;              // n x n, row j = eigenvector j of B
    const double* Et;             // its transpose (LDSV = false)
    const double* ev;             // eigenvalues of B
    double* vec;                  // x | z | u | b | w, n each: the state vectors
    double* pub;                  // c[2] | z[2] | Ax[2], n each: published products, double-buffered by parity
    SpgState* S;
    int n, rpw;                   // rows per workgroup
    long long budget;             // ADMM iterations this launch may run
};

// Arrivals are counted from zero in every launch (the host clears the word); the wait is bounded (~2 s) and a workgroup
// that gives up raises the timeout word, which ends the others' waits too.
__device__ __forceinline__ bool spg_barrier(SpgState* S, unsigned target)
{
    __hip_atomic_fetch_add(&S->bar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    for (long long spin = 0; spin < 2000000LL; ++spin) {
        if (__hip_atomic_load(&S->bar, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= target) return true;
        if (__hip_atomic_load(&S->timed_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return false;
        __builtin_amdgcn_s_sleep(2);
    }
    __hip_atomic_store(&S->timed_out, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return false;
}

__device__ __forceinline__ double spg_lanes(double v)   // sum over the 64 lanes, the same bits in every lane
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <bool LDSV>
__global__ __launch_bounds__(SPG_T) void speigh_kernel(SpgArgs P)
{
    extern __shared__ __attribute__((aligned(16))) double spg_smem[];
    __shared__ int bc_ok;
    const int n = P.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NB = LDSV ? 1 : (int)gridDim.x, wg = LDSV ? 0 : (int)blockIdx.x;
    constexpr int NW = SPG_T / 64;
    double* sx = spg_smem;
    double* sz = sx + n;
    double* su = sz + n;
    double* sb = su + n;
    double* sw = sb + n;
    double* sev = sw + n;
    double* sc = sev + n;
    double* sat = sc + n;
    double* sE = sat + n;         // LDSV: [n][pitch]
    const int pitch = n | 1;
    const long long lo = (long long)wg * P.rpw;
    const int r0 = lo < n ? (int)lo : n, r1 = r0 + P.rpw < n ? r0 + P.rpw : n;
    SpgState* S = P.S;

    for (int j = tid; j < n; j += SPG_T) {
        sx[j] = P.vec[j];
        sz[j] = P.vec[n + j];
        su[j] = P.vec[2 * n + j];
        sb[j] = P.vec[3 * n + j];
        sw[j] = P.vec[4 * n + j];
        sev[j] = P.ev[j];
    }
    if (LDSV)
        for (int q = tid; q < n * n; q += SPG_T) sE[(q / n) * pitch + q % n] = P.E[q];
    double rho = S->rho, f = S->f, f_old = S->f_old;
    const double tau = S->tau, rho_e = S->rho_e, eps = S->eps, tol = S->tol;
    const long long maxiter = S->maxiter;
    long long outer = S->outer, total = S->total, k = S->k;
    int phase = S->phase;
    const int mode = S->mode;
    int status = SPG_RUNNING;
    unsigned nbar = 0;
    long long left = P.budget;
    __syncthreads();

    // sum over j < n of term(j): the same order in every wavefront of every workgroup
    auto wsum = [&](auto term) {
        double acc = 0.0;
        for (int j = lane; j < n; j += 64) acc += term(j);
        return spg_lanes(acc);
    };
    // dst (LDS, whole vector) = M src, M's row r at base + r * rs with element stride es.  false: the barrier timed out.
    auto product = [&](const double* base, size_t rs, size_t es, const double* src, double* dst, double* pub) -> bool {
        if (LDSV) {
            for (int r = wave; r < n; r += NW) {
                const double* row = base + (size_t)r * rs;
                double acc = 0.0;
                for (int j = lane; j < n; j += 64) acc += row[(size_t)j * es] * src[j];
                acc = spg_lanes(acc);
                if (lane == 0) dst[r] = acc;
            }
            __syncthreads();
            return true;
        }
        for (int r = r0 + wave; r < r1; r += NW) {
            const double* row = base + (size_t)r * rs;
            double acc = 0.0;
            for (int j = lane; j < n; j += 64) acc += row[(size_t)j * es] * src[j];
            acc = spg_lanes(acc);
            if (lane == 0) {
                __hip_atomic_store(pub + r, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __threadfence();
            }
        }
        __syncthreads();
        ++nbar;
        if (tid == 0) bc_ok = spg_barrier(S, (unsigned)NB * nbar) ? 1 : 0;
        __syncthreads();
        if (!bc_ok) return false;
        for (int j = tid; j < n; j += SPG_T) dst[j] = __hip_atomic_load(pub + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        return true;
    };
    // sc <- the point of { z : z^T B z <= 1 } nearest to sat (sat is overwritten).  par: which published pair to use.
    auto project = [&](int par) -> bool {
        const bool ok1 = LDSV ? product(sE, (size_t)pitch, 1, sat, sc, nullptr) : product(P.E, (size_t)n, 1, sat, sc, P.pub + (size_t)par * n);
        if (!ok1) return false;
        const double inside = wsum([&](int j) { return sc[j] * sc[j] * sev[j]; });
        if (inside < 1.0) {
            __syncthreads();   // (every wavefront has read sc)
            for (int j = tid; j < n; j += SPG_T) sc[j] = sat[j];
            __syncthreads();
            return true;
        }
        double mu = 0.0;
        for (int it = 0; it < 100; ++it) {
            double g = 0.0, gp = 0.0;
            for (int j = lane; j < n; j += 64) {
                const double c2w = sc[j] * sc[j] * sev[j], m1 = mu * sev[j] + 1.0;
                g += c2w / (m1 * m1);
                gp += 2.0 * c2w * sev[j] / (m1 * m1 * m1);
            }
            g = spg_lanes(g) - 1.0;
            gp = -spg_lanes(gp);
            const double delta = -g / gp;
            mu += delta;
            if (fabs(delta) < 1e-12) break;
        }
        for (int j = tid; j < n; j += SPG_T) sat[j] = sc[j] / (mu * sev[j] + 1.0);
        __syncthreads();
        return LDSV ? product(sE, 1, (size_t)pitch, sat, sc, nullptr) : product(P.Et, (size_t)n, 1, sat, sc, P.pub + (size_t)(2 + par) * n);
    };

    bool alive = true;
    if (mode == SPG_PROJECT) {
        for (int j = tid; j < n; j += SPG_T) sat[j] = sx[j];
        __syncthreads();
        alive = project(0);
        for (int j = tid; j < n; j += SPG_T) sz[j] = sc[j];
        __syncthreads();
        status = SPG_CONVERGED;
    } else {
        for (;;) {
            if (phase == 0) {
                if (outer >= maxiter) {
                    status = SPG_MAXITER;
                    break;
                }
                if (!(alive = product(P.A, (size_t)n, 1, sx, sc, P.pub + (size_t)(4 + (int)(outer & 1)) * n))) break;
                const double quad = wsum([&](int j) { return sc[j] * sx[j]; });
                const double pen = wsum([&](int j) { return rho_e * log(fabs(sx[j]) + eps); });
                f_old = f;
                f = quad - pen;
                if (fabs(f_old - f) < tol) {
                    status = SPG_CONVERGED;
                    break;
                }
                for (int j = tid; j < n; j += SPG_T) {
                    const double xj = sx[j];
                    sb[j] = sc[j] / tau + xj;
                    sw[j] = rho_e / (2.0 * tau * (fabs(xj) + eps));
                    sz[j] = xj;
                    su[j] = 0.0;
                }
                rho = 16.0;
                k = 0;
                phase = 1;
                __syncthreads();
            }
            if (left == 0) break;   // the budget is spent: the state goes to device memory and the host launches again
            --left;
            for (int j = tid; j < n; j += SPG_T) {
                const double q = sb[j] + rho * (sz[j] - su[j]), th = fabs(sw[j]);
                double xs = q > th ? q - th : (q < -th ? q + th : 0.0);
                xs = xs / (rho + 1.0);
                sx[j] = xs;
                sat[j] = xs + su[j];
            }
            __syncthreads();
            if (!(alive = project((int)(total & 1)))) break;
            for (int j = tid; j < n; j += SPG_T) {
                const double zn = sc[j], r = sx[j] - zn, s = rho * (zn - sz[j]);
                su[j] = su[j] + r;
                sz[j] = zn;
                sat[j] = r;
                sc[j] = s;
            }
            __syncthreads();
            const double r2 = wsum([&](int j) { return sat[j] * sat[j]; });
            const double s2 = wsum([&](int j) { return sc[j] * sc[j]; });
            __syncthreads();   // (sat and sc are rewritten at the head of the next iteration)
            ++k;
            ++total;
            const double bound = (double)n * tol * tol;
            bool done = r2 < bound && s2 < bound;
            const bool met = done;
            if (!done) {
                double scale = 1.0;
                if (r2 > 100.0 * s2 && rho < 1024.0) {
                    rho *= 2.0;
                    scale *= 0.5;
                }
                if (s2 > 100.0 * r2 && rho > 1.0 / 1024.0) {
                    rho /= 2.0;
                    scale *= 2.0;
                }
                if (scale != 1.0) {
                    for (int j = tid; j < n; j += SPG_T) su[j] *= scale;   // (a power of two: exact, as the division is)
                    __syncthreads();
                }
                done = k >= maxiter;
            }
            if (done) {
                if (mode == SPG_ADMM) {
                    status = met ? SPG_CONVERGED : SPG_MAXITER;
                    break;
                }
                ++outer;
                phase = 0;
            }
        }
    }
    if (!alive || wg != 0) return;
    for (int j = tid; j < n; j += SPG_T) {
        P.vec[j] = sx[j];
        P.vec[n + j] = sz[j];
        P.vec[2 * n + j] = su[j];
        P.vec[3 * n + j] = sb[j];
        P.vec[4 * n + j] = sw[j];
    }
    if (tid == 0) {
        S->rho = rho;
        S->f = f;
        S->f_old = f_old;
        S->outer = outer;
        S->total = total;
        S->k = k;
        S->phase = phase;
        S->status = status;
    }
}

// ---- Schur complement deflation: out = A - (A x)(x^T A)^T / (x^T A x), the two products kept apart as written -----------
// pv[0 .. n) = A x (a wavefront per row), pv[n .. 2n) = x^T A (a thread per column: coalesced over the column index)
__global__ __launch_bounds__(256) void scdeflate_products_kernel(const double* __restrict__ A, const double* __restrict__ x, int n,
                                                                 double* __restrict__ pv)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = blockIdx.x * 4 + wave;
    if (r < n) {
        double acc = 0.0;
        for (int j = lane; j < n; j += 64) acc += A[(size_t)r * n + j] * x[j];
        acc = spg_lanes(acc);
        if (lane == 0) pv[r] = acc;
    }
    const int c = blockIdx.x * 256 + tid;
    if (c < n) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += x[i] * A[(size_t)i * n + c];
        pv[n + c] = acc;
    }
}

__global__ __launch_bounds__(256) void scdeflate_apply_kernel(const double* __restrict__ A, const double* __restrict__ x, int n,
                                                              const double* __restrict__ pv, double* __restrict__ out)
{
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int j = lane; j < n; j += 64) acc += pv[n + j] * x[j];
    const double d = spg_lanes(acc);
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < (size_t)n * n) out[q] = A[q] - pv[q / n] * pv[n + q % n] / d;
}

// E^T for the row-owning layout
__global__ void spg_transpose_kernel(const double* __restrict__ E, int n, double* __restrict__ Et)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < (size_t)n * n) Et[q] = E[(q % n) * n + q / n];
}

// flag <- 1 if any of the m doubles is NaN or infinite
__global__ void spg_nonfinite_kernel(const double* __restrict__ M, size_t m, int* __restrict__ flag)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < m && !(fabs(M[q]) <= 1.79769313486231570815e308)) *flag = 1;
}

}  // namespace msm
