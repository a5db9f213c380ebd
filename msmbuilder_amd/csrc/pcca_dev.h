// pcca_dev.h -- the kernels of pcca.hip: the PCCA+ objectives (lumping/pcca_plus.py) on a transition matrix that stays on
// the device.  Everything is float64.
//
// Definitions (A is m x m, V is n x m row-major, alpha = A[1:, 1:] row-major):
//   fill:   A[k, 0] = -(A[k, 1] + ... + A[k, m-1]) for k >= 1, added in ascending column;
//           A[0, c] = -min_s d[s, c],  d[s, c] = V[s, 1] A[1, c] + ... + V[s, m-1] A[m-1, c], added in ascending k;
//           A /= A[0, 0] + ... + A[0, m-1]  (ascending, every element divided).
//   chi:    chi[s, c] = V[s, 0] A[0, c] + e[s, c],  e[s, c] = V[s, 1] A[1, c] + ... (ascending k) with the scaled A.
//   map:    the first maximum of a row of chi; a row with a NaN maps to its first NaN.
//   blocks: S_a = sum of T[a, b] over the b with map[b] == map[a]; num_i = sum of pi_a S_a and den_i = sum of pi_a over the a
//           with map[a] == i.
// A minimum is taken under the total order -0 < +0 and is NaN once a NaN is met, so it does not depend on the order in
// which the states are visited.  Every sum has ONE order, fixed by n and m:
//   S_a:    lane l of a wave adds its columns 2 l, 2 l + 1, 2 l + PC_CP, 2 l + PC_CP + 1, ... in ascending order, and the 64
//           partial sums are added in a butterfly (xor 32, 16, 8, 4, 2, 1).  Whether a row is read with 16-byte or with 8-byte
//           loads changes no operand and no order.
//   num_i, den_i, G, w: thread t of 256 adds the states t, t + 256, ... in ascending order; the 256 partial sums are added in a
//           binary tree (t += t + 128, 64, ..., 1).
// No floating-point atomics anywhere; the integer flags (macrostates used, mapping changed) are combined with LDS atomics,
// which commute.
#pragma once
#include "common.h"

namespace msm {

constexpr int PC_T = 256;        // threads per workgroup
constexpr int PC_WAVES = PC_T / 64;
constexpr int PC_RP = 8;         // rows of T per workgroup of the row kernels (2 per wave)
constexpr int PC_CP = 128;       // columns per pass of a wave: 64 lanes x 2 doubles = 64 x 16 bytes
constexpr int PC_MAX_N = 16384;
constexpr int PC_MAX_M = 64;
constexpr int PC_MAX_PARTS = 256;   // workgroups of the two kernels over V, one slot of partial results each
constexpr int PC_TV = 8;         // columns of V per sweep of a row of T in the set-up kernel

// What one evaluation leaves on the device.
struct PccaOut {
    double value;
    int info[4];      // feasible, macrostates used, mapping equal to the previous evaluation's, passes over T
    int compute;      // kind 2: the value is a block sum (feasible and every macrostate used)
    int do_pass;      // kind 2: the row kernel runs
};

__device__ __forceinline__ double pc_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ double pc_min(double a, double b)
{
    if (a != a || b != b) return pc_nan();
    if (b < a) return b;
    if (a < b) return a;
    return (__double_as_longlong(b) < 0) ? b : a;   // equal: -0 before +0
}

template <bool ALIGNED>
__device__ __forceinline__ void pc_load2(const double* __restrict__ p, double& x0, double& x1)
{
    if (ALIGNED) {
        const double2 v = *reinterpret_cast<const double2*>(p);
        x0 = v.x;
        x1 = v.y;
    } else {
        x0 = p[0];
        x1 = p[1];
    }
}

__device__ __forceinline__ double pc_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The 256 partial sums of a workgroup, added in a binary tree; the total is returned to every thread.
__device__ __forceinline__ double pc_tree_sum(double v, double* red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = PC_T / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// ---- the row kernel: S_a for every state, pi_a S_a to rowval ------------------------------------------------------------
template <bool ALIGNED>
__device__ __forceinline__ double pc_row_sum(const double* __restrict__ row, const unsigned char* smap, int n, int lane, unsigned char ma)
{
    double acc = 0.0;
    const int full = n / PC_CP;   // passes in which every lane has both of its columns
    int c = 2 * lane;
#pragma unroll 4
    for (int p = 0; p < full; ++p, c += PC_CP) {
        double x0, x1;
        pc_load2<ALIGNED>(row + c, x0, x1);
        if (smap[c] == ma) acc += x0;
        if (smap[c + 1] == ma) acc += x1;
    }
    if (c + 1 < n) {
        double x0, x1;
        pc_load2<ALIGNED>(row + c, x0, x1);
        if (smap[c] == ma) acc += x0;
        if (smap[c + 1] == ma) acc += x1;
    } else if (c < n) {
        if (smap[c] == ma) acc += row[c];
    }
    return pc_wave_sum(acc);
}

// gate (nullable): the evaluation's decision; the kernel does nothing where no pass is wanted.
__global__ __launch_bounds__(PC_T) void pcca_row_kernel(const double* __restrict__ T, const double* __restrict__ pi,
                                                        const int* __restrict__ map, int n, double* __restrict__ rowval,
                                                        const PccaOut* gate)
{
    __shared__ unsigned char smap[PC_MAX_N];
    if (gate && !gate->do_pass) return;
    for (int i = threadIdx.x; i < n; i += PC_T) smap[i] = (unsigned char)map[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nblocks = (n + PC_RP - 1) / PC_RP;
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        for (int r = wave; r < PC_RP; r += PC_WAVES) {
            const int a = blk * PC_RP + r;
            if (a >= n) break;
            const double* row = T + (size_t)a * (size_t)n;
            const unsigned char ma = smap[a];
            const double s = (((uintptr_t)row & 15) == 0) ? pc_row_sum<true>(row, smap, n, lane, ma)
                                                          : pc_row_sum<false>(row, smap, n, lane, ma);
            if (lane == 0) rowval[a] = pi[a] * s;
        }
    }
}

// num_i and den_i from rowval: one workgroup per macrostate at a time.
__global__ __launch_bounds__(PC_T) void pcca_block_kernel(const double* __restrict__ rowval, const double* __restrict__ pi,
                                                          const int* __restrict__ map, int n, int m, double* __restrict__ num,
                                                          double* __restrict__ den, const PccaOut* gate)
{
    __shared__ double red[PC_T];
    if (gate && !gate->do_pass) return;
    for (int i = blockIdx.x; i < m; i += gridDim.x) {
        double an = 0.0, ad = 0.0;
        for (int a = threadIdx.x; a < n; a += PC_T)
            if (map[a] == i) {
                an += rowval[a];
                ad += pi[a];
            }
        an = pc_tree_sum(an, red);
        ad = pc_tree_sum(ad, red);
        if (threadIdx.x == 0) {
            num[i] = an;
            den[i] = ad;
        }
    }
}

// ---- set-up: Y = T V, then G = V^T diag(pi) Y and w = V^T pi ---------------------------------------------------------------
template <bool ALIGNED>
__device__ __forceinline__ void pc_row_tv(const double* __restrict__ row, const double* __restrict__ V, int n, int m, int c0, int lane,
                                          double* acc)
{
    int cj[PC_TV];
#pragma unroll
    for (int j = 0; j < PC_TV; ++j) {
        acc[j] = 0.0;
        cj[j] = min(c0 + j, m - 1);   // (the clamped columns are computed and dropped)
    }
    for (int c = 2 * lane; c < n; c += PC_CP) {
        double x0, x1 = 0.0;
        const bool two = c + 1 < n;
        if (two)
            pc_load2<ALIGNED>(row + c, x0, x1);
        else
            x0 = row[c];
        const double* v0 = V + (size_t)c * m;
#pragma unroll
        for (int j = 0; j < PC_TV; ++j) acc[j] += x0 * v0[cj[j]];
        if (two) {
#pragma unroll
            for (int j = 0; j < PC_TV; ++j) acc[j] += x1 * v0[m + cj[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < PC_TV; ++j) acc[j] = pc_wave_sum(acc[j]);
}

// One wave per row: T is read from memory once; for m > PC_TV the row is swept again per group of PC_TV columns, out of the
// cache.
__global__ __launch_bounds__(PC_T) void pcca_tv_kernel(const double* __restrict__ T, const double* __restrict__ V, int n, int m,
                                                       double* __restrict__ Y)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nblocks = (n + PC_RP - 1) / PC_RP;
    for (int blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
        for (int r = wave; r < PC_RP; r += PC_WAVES) {
            const int a = blk * PC_RP + r;
            if (a >= n) break;
            const double* row = T + (size_t)a * (size_t)n;
            const bool aligned = ((uintptr_t)row & 15) == 0;
            for (int c0 = 0; c0 < m; c0 += PC_TV) {
                double acc[PC_TV];
                if (aligned)
                    pc_row_tv<true>(row, V, n, m, c0, lane, acc);
                else
                    pc_row_tv<false>(row, V, n, m, c0, lane, acc);
                if (lane == 0) {
#pragma unroll
                    for (int j = 0; j < PC_TV; ++j)
                        if (c0 + j < m) Y[(size_t)a * m + c0 + j] = acc[j];
                }
            }
        }
    }
}

// item < m * m: G[j, c] = sum_a (V[a, j] pi[a]) Y[a, c];  item = m * m + j: w[j] = sum_a V[a, j] pi[a].
__global__ __launch_bounds__(PC_T) void pcca_moment_kernel(const double* __restrict__ V, const double* __restrict__ pi,
                                                           const double* __restrict__ Y, int n, int m, double* __restrict__ G,
                                                           double* __restrict__ w)
{
    __shared__ double red[PC_T];
    const int items = m * m + m;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
        const bool is_w = it >= m * m;
        const int j = is_w ? it - m * m : it / m, c = is_w ? 0 : it % m;
        double acc = 0.0;
        for (int a = threadIdx.x; a < n; a += PC_T) {
            const double vp = V[(size_t)a * m + j] * pi[a];
            acc += is_w ? vp : vp * Y[(size_t)a * m + c];
        }
        acc = pc_tree_sum(acc, red);
        if (threadIdx.x == 0) (is_w ? w[j] : G[it]) = acc;
    }
}

// ---- the two kernels over V ------------------------------------------------------------------------------------------------
// Thread layout of both: cp = the power of two >= m columns side by side, PC_T / cp states per step.
__device__ __forceinline__ int pc_cols(int m)
{
    int cp = 2;
    while (cp < m) cp <<= 1;
    return cp;
}

// Rows 1 .. m-1 of A in LDS (pitch PC_MAX_M) from alpha, the first column by the row-sum condition.
__device__ __forceinline__ void pc_fill_tail(double* As, const double* __restrict__ alpha, int m)
{
    for (int idx = threadIdx.x; idx < (m - 1) * (m - 1); idx += PC_T) {
        const int k = idx / (m - 1) + 1, c = idx % (m - 1) + 1;
        As[k * PC_MAX_M + c] = alpha[idx];
    }
    __syncthreads();
    for (int k = threadIdx.x + 1; k < m; k += PC_T) {
        double s = 0.0;
        for (int c = 1; c < m; ++c) s += As[k * PC_MAX_M + c];
        As[k * PC_MAX_M] = -s;
    }
    __syncthreads();
}

__device__ __forceinline__ double pc_tail_dot(const double* __restrict__ v, const double* As, int m, int c)
{
    double acc = 0.0;
    for (int k = 1; k < m; ++k) acc += v[k] * As[k * PC_MAX_M + c];
    return acc;
}

// colpart[p * m + c] = the minimum of d[s, c] over the states workgroup p visits.
__global__ __launch_bounds__(PC_T) void pcca_colmin_kernel(const double* __restrict__ alpha, const double* __restrict__ V, int n, int m,
                                                           double* __restrict__ colpart)
{
    __shared__ double As[PC_MAX_M * PC_MAX_M];
    __shared__ double red[PC_T];
    pc_fill_tail(As, alpha, m);
    const int cp = pc_cols(m), g = PC_T / cp;
    const int c = threadIdx.x % cp, rl = threadIdx.x / cp;
    const int steps = (n + g - 1) / g;
    double mn = INFINITY;
    if (c < m)
        for (int st = blockIdx.x; st < steps; st += gridDim.x) {
            const int s = st * g + rl;
            if (s < n) mn = pc_min(mn, pc_tail_dot(V + (size_t)s * m, As, m, c));
        }
    red[threadIdx.x] = mn;
    __syncthreads();
    if (threadIdx.x < m) {
        double v = red[threadIdx.x];
        for (int r = 1; r < g; ++r) v = pc_min(v, red[r * cp + threadIdx.x]);
        colpart[(size_t)blockIdx.x * m + threadIdx.x] = v;
    }
}

struct PccaChiArgs {
    const double* alpha;
    const double* V;
    const double* colpart;   // nparts x m, from pcca_colmin_kernel at the same grid
    int n, m, nparts;
    double* A;               // m x m out
    double* chi;             // n x m out, nullable
    int* map;                // n out
    const int* prev;         // n, nullable: the previous evaluation's mapping
    double* emin;            // nparts out: min over the workgroup's states of e[s, 0]
    int* differ;             // nparts out
    unsigned long long* used;   // nparts out: bit i set where macrostate i received a state
};

__global__ __launch_bounds__(PC_T) void pcca_chi_kernel(PccaChiArgs P)
{
    __shared__ double As[PC_MAX_M * PC_MAX_M];
    __shared__ double Cs[PC_T];
    __shared__ double red[PC_T];
    __shared__ unsigned long long s_used;
    __shared__ int s_differ;
    const int m = P.m, n = P.n, tid = threadIdx.x;
    pc_fill_tail(As, P.alpha, m);
    if (tid == 0) {
        s_used = 0ull;
        s_differ = 0;
    }
    if (tid < m) {
        double mn = INFINITY;
        for (int p = 0; p < P.nparts; ++p) mn = pc_min(mn, P.colpart[(size_t)p * m + tid]);
        As[tid] = -mn;
    }
    __syncthreads();
    double scale = 0.0;
    for (int c = 0; c < m; ++c) scale += As[c];
    __syncthreads();
    for (int idx = tid; idx < m * m; idx += PC_T) {
        const int k = idx / m, c = idx % m;
        const double v = As[k * PC_MAX_M + c] / scale;
        As[k * PC_MAX_M + c] = v;
        if (blockIdx.x == 0) P.A[idx] = v;
    }
    __syncthreads();
    const int cp = pc_cols(m), g = PC_T / cp;
    const int c = tid % cp, rl = tid / cp;
    const int steps = (n + g - 1) / g;
    double mn = INFINITY;
    for (int st = blockIdx.x; st < steps; st += gridDim.x) {
        const int s = st * g + rl;
        if (c < m && s < n) {
            const double* v = P.V + (size_t)s * m;
            const double e = pc_tail_dot(v, As, m, c);
            const double x = v[0] * As[c] + e;
            Cs[rl * cp + c] = x;
            if (P.chi) P.chi[(size_t)s * m + c] = x;
            if (c == 0) mn = pc_min(mn, e);
        }
        __syncthreads();
        if (tid < g && st * g + tid < n) {
            const double* row = Cs + tid * cp;
            int best = 0;
            double bv = row[0];
            for (int k = 1; k < m; ++k) {
                const double x = row[k];
                if (bv == bv && (x > bv || x != x)) {
                    best = k;
                    bv = x;
                }
            }
            const int s2 = st * g + tid;
            P.map[s2] = best;
            if (P.prev && P.prev[s2] != best) atomicOr(&s_differ, 1);
            atomicOr(&s_used, 1ull << best);
        }
        __syncthreads();
    }
    red[tid] = (c == 0) ? mn : INFINITY;
    __syncthreads();
    if (tid == 0) {
        double v = red[0];
        for (int r = 1; r < g; ++r) v = pc_min(v, red[r * cp]);
        P.emin[blockIdx.x] = v;
        P.differ[blockIdx.x] = s_differ;
        P.used[blockIdx.x] = s_used;
    }
}

// ---- the decision and the values -----------------------------------------------------------------------------------------
struct PccaEvalArgs {
    const double* A;
    const double* G;
    const double* w;
    const double* emin;
    const int* differ;
    const unsigned long long* used;
    int nparts, m, kind, reuse;
    int* sums_valid;     // the remembered block sums belong to the previous evaluation's mapping
    const double* num;   // the remembered block sums
    const double* den;
    PccaOut* out;
};

// One workgroup.  Feasibility, the macrostates used, whether the mapping changed; the values of kinds 0 and 1; for kind 2
// whether the row kernel has to run.
__global__ __launch_bounds__(PC_T) void pcca_decide_kernel(PccaEvalArgs E)
{
    __shared__ double q[PC_MAX_M];
    __shared__ int s_state[4];
    const int m = E.m, tid = threadIdx.x;
    if (tid == 0) {
        double mn = INFINITY;
        int differ = 0;
        unsigned long long used = 0ull;
        for (int p = 0; p < E.nparts; ++p) {
            mn = pc_min(mn, E.emin[p]);
            differ |= E.differ[p];
            used |= E.used[p];
        }
        double first = 0.0;
        for (int c = 1; c < m; ++c) first += E.A[c];
        const double lhs = 1.0 - first, rhs = -mn;
        s_state[0] = fabs(lhs - rhs) <= 1e-8;   // (a NaN fails)
        s_state[1] = __popcll(used);
        s_state[2] = !differ;
    }
    __syncthreads();
    const bool ok = s_state[0] && s_state[1] == m;
    if (ok && E.kind != 2 && tid < m) {
        double top = 0.0, bottom;
        if (E.kind == 0) {
            for (int k = 0; k < m; ++k) top += E.A[k * m + tid] * E.A[k * m + tid];
            bottom = E.A[tid];
        } else {
            bottom = 0.0;
            for (int j = 0; j < m; ++j) {
                double inner = 0.0;
                for (int k = 0; k < m; ++k) inner += E.G[j * m + k] * E.A[k * m + tid];
                top += E.A[j * m + tid] * inner;
                bottom += E.A[j * m + tid] * E.w[j];
            }
        }
        q[tid] = top / bottom;
    }
    __syncthreads();
    if (tid == 0) {
        PccaOut o;
        o.info[0] = s_state[0];
        o.info[1] = s_state[1];
        o.info[2] = s_state[2];
        if (!s_state[2]) *E.sums_valid = 0;
        o.compute = ok && E.kind == 2;
        o.do_pass = o.compute && !(E.reuse && s_state[2] && *E.sums_valid);
        o.info[3] = o.do_pass;
        o.value = -INFINITY;
        if (ok && E.kind != 2) {
            double v = 0.0;
            for (int i = 0; i < m; ++i) v += q[i];
            o.value = v;
        }
        *E.out = o;
    }
}

// Kind 2: the value from the block sums, this call's or the remembered ones (the same arrays).
__global__ void pcca_crisp_value_kernel(const double* __restrict__ num, const double* __restrict__ den, int m, int* sums_valid,
                                        PccaOut* out)
{
    if (threadIdx.x != 0 || !out->compute) return;
    double v = 0.0;
    for (int i = 0; i < m; ++i) v += num[i] / den[i];
    out->value = v;
    *sums_valid = 1;
}

}  // namespace msm
