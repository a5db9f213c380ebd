// hmm_dev.h -- device side of the Gaussian HMM E-step (hmm.hip): forward-backward made parallel in time.
//
// The step matrix of a frame is M_t = A . diag(b_t), b_t(k) = exp(l_t(k) - max_k l_t(k)) (the maximum goes to a log scale);
// the first frame of a trajectory has M_0 = diag(b_0).  These compose associatively and serve both directions:
//   alpha_end^T = alpha_entry^T . prod M,     beta_entry = prod M . beta_exit.
// Every trajectory is cut into segments of S frames:
//   hmm_oper_kernel     one workgroup per segment: its K x K product, renormalised by its largest entry at every step
//   hmm_stitch_kernel   one workgroup per trajectory: a sweep over its segment operators (K^2 each) -> every segment's
//                       entry alpha and exit beta, and the trajectory's log probability
//   hmm_fused_kernel    a workgroup walks a contiguous run of segments: emissions again from X, alpha through the segment
//                       kept in LDS, beta swept backwards forming gamma_t and the xi sums on the way, gamma^T X and
//                       gamma^T X^2 from the LDS block; ONE partial per workgroup
//   hmm_reduce_kernel   the partials summed in workgroup order
// Neither the N x K emissions nor a lattice nor the posteriors reach HBM; nothing is atomic, every sum has one fixed order.
// All arithmetic is float64; a float32 element is widened exactly.
//
// The emission term has two flavours, chosen at compile time (HmmEmission):
//   HMM_GAUSS    l_t(k) = cst[k] - 1/2 sum_f (x_tf - mu[k, f])^2 iv[k, f]          rows of T, F columns
//   HMM_LINEAR   l_t(k) = cst[k] + sum_j z_tj w[k, j]                               rows of float64, D columns (F holds D,
//                                                                                   mu holds w, iv is unused)
// The linear one serves the von Mises model over the image Z = [cos X | sin X] that hmm_trig_kernel forms once per fit;
// its fused pass forms gamma^T [1, Z] only (no squares).
#pragma once
#include "common.h"

namespace msm {

constexpr int HMM_T = 256;                          // threads of a workgroup (operators, fused pass)
constexpr int HMM_KMAX = 64;                        // one lane of a wave per state in the vector steps
constexpr int HMM_EPT = HMM_KMAX * HMM_KMAX / HMM_T;   // entries of a K x K matrix one thread owns at most
constexpr int HMM_EC = 16;                          // frames whose emissions the operator kernel forms at a time
constexpr int HMM_VC = 64;                          // frames of a Viterbi chunk (emissions ahead, back-pointers behind)
constexpr int HMM_G = 1024;                         // workgroups of the fused pass at most (= partials to reduce)
constexpr double HMM_DROP = -708.0;                 // exp() below this is under the smallest normal double: the state is dropped
constexpr int HMM_TRIG_WAVES = 8;                   // workgroups per CU of the image kernel's grid at most

enum HmmEmission { HMM_GAUSS = 0, HMM_LINEAR = 1 };

struct HmmArgs {
    const void* X;               // rows, N x F at stride ld elements
    long long ld;
    int K, F, KP;                // KP: pitch of the transition matrix in LDS (odd: rows and columns both conflict-free)
    int S;                       // frames of a segment
    long long n_traj, n_seg;
    const long long* off;        // n_traj + 1 row offsets
    const long long* seg0;       // n_traj + 1: first segment of every trajectory
    const double* mu;            // K x F (linear emission: the weights w, K x D)
    const double* iv;            // K x F, 1 / variance (linear emission: unused)
    const double* cst;           // K: -0.5 (F log 2pi + sum log variance) (linear emission: the constant of the state)
    const double* A;             // K x K, clamped at 1e-20
    const double* logA;          // K x K, log of A
    const double* lsp;           // K: what the recursion adds at the first frame (HMMFitter's log_startprob)
    double* ops;                 // n_seg x K x K
    double* opscale;             // n_seg
    double* alpha_in;            // n_seg x K
    double* beta_out;            // n_seg x K (null: forward half only)
    double* traj_lp;             // n_traj
    double* part;                // G x psz partials: post K, obs K F, obs2 K F, trans K K (linear emission: no obs2)
    double* out;                 // psz
    long long psz;
    int G;
    int* flag;                   // set when a row element is not finite
    unsigned char* bp;           // Viterbi back-pointers, N x K bytes
    int* states;                 // Viterbi path, N
    double* loglik;              // N x K (loglik kernel)
    long long n;
};

__device__ __forceinline__ double hmm_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ double hmm_wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// The segment g: its trajectory (binary search in seg0), first row, frames, and whether it opens the trajectory.
__device__ __forceinline__ void hmm_locate(const HmmArgs& A, long long g, long long* row0, int* len, bool* first)
{
    long long lo = 0, hi = A.n_traj;   // seg0[lo] <= g < seg0[hi]
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (A.seg0[mid] <= g) lo = mid; else hi = mid;
    }
    const long long s = g - A.seg0[lo];
    *row0 = A.off[lo] + s * A.S;
    const long long left = A.off[lo + 1] - *row0;
    *len = (int)(left < A.S ? left : A.S);
    *first = s == 0;
}

template <typename T>
__device__ __forceinline__ double hmm_loglik1(const T* x, const double* mu, const double* iv, int F, double cst, bool* bad)
{
    double s = 0.0;
    for (int f = 0; f < F; ++f) {
        const double xv = (double)x[f];
        *bad |= !isfinite(xv);
        const double d = xv - mu[f];
        s += d * d * iv[f];
    }
    return cst - 0.5 * s;
}

// The linear emission over a row of the image; a NaN in it (a non-finite angle) raises the flag like a non-finite row.
__device__ __forceinline__ double hmm_linear1(const double* z, const double* w, int D, double cst, bool* bad)
{
    double s = 0.0;
    for (int j = 0; j < D; ++j) {
        const double zv = z[j];
        *bad |= !isfinite(zv);
        s += zv * w[j];
    }
    return cst + s;
}

// Emissions of nt frames from row x0 on: b[t * K + k] = exp(l - max_k l) (or l itself when LOG), m[t] = max_k l.
// Every thread of the workgroup calls it; ends on a barrier.
template <typename T, bool LOG, int EM>
__device__ __forceinline__ void hmm_emis(const HmmArgs& A, const T* x0, int nt, double* b, double* m)
{
    const int K = A.K, F = A.F;
    for (int idx = threadIdx.x; idx < nt * K; idx += blockDim.x) {
        const int t = idx / K, k = idx - t * K;
        bool bad = false;
        if constexpr (EM == HMM_LINEAR)
            b[idx] = hmm_linear1(x0 + (long long)t * A.ld, A.mu + (long long)k * F, F, A.cst[k], &bad);
        else
            b[idx] = hmm_loglik1(x0 + (long long)t * A.ld, A.mu + (long long)k * F, A.iv + (long long)k * F, F, A.cst[k], &bad);
        if (bad) *A.flag = 1;
    }
    __syncthreads();
    if (!LOG) {
        for (int t = threadIdx.x; t < nt; t += blockDim.x) {
            double* bt = b + t * K;
            double mx = bt[0];
            for (int k = 1; k < K; ++k) mx = fmax(mx, bt[k]);
            m[t] = mx;
            for (int k = 0; k < K; ++k) {
                const double d = bt[k] - mx;
                bt[k] = d < HMM_DROP ? 0.0 : exp(d);
            }
        }
        __syncthreads();
    }
}

// LDS doubles of the two kernels (the host sizes the launch with the same expressions)
__host__ __device__ inline long long hmm_oper_lds(int K, int KP) { return (long long)K * KP + 2LL * K * K + (long long)HMM_EC * K + HMM_EC + 8; }
__host__ __device__ inline long long hmm_fused_lds(int K, int KP, int S) { return (long long)K * KP + 2LL * S * K + S + 4LL * K + 8; }

template <typename T, int EM = HMM_GAUSS>
__global__ __launch_bounds__(HMM_T) void hmm_oper_kernel(HmmArgs A)
{
    extern __shared__ double hmm_sm[];
    const int K = A.K, KP = A.KP, K2 = K * K, tid = threadIdx.x;
    double* sA = hmm_sm;
    double* cur = sA + K * KP;
    double* nxt = cur + K2;
    double* sb = nxt + K2;
    double* smx = sb + HMM_EC * K;
    double* red = smx + HMM_EC;
    long long row0;
    int len;
    bool first;
    hmm_locate(A, blockIdx.x, &row0, &len, &first);
    int ei[HMM_EPT], ej[HMM_EPT];
#pragma unroll
    for (int r = 0; r < HMM_EPT; ++r) {
        const int e = tid + r * HMM_T;
        ei[r] = e < K2 ? e / K : -1;
        ej[r] = e < K2 ? e - ei[r] * K : 0;
        if (e < K2) {
            sA[ei[r] * KP + ej[r]] = A.A[e];
            cur[e] = ei[r] == ej[r] ? 1.0 : 0.0;
        }
    }
    double logscale = 0.0;
    const T* X = static_cast<const T*>(A.X) + row0 * A.ld;
    for (int c0 = 0; c0 < len; c0 += HMM_EC) {
        const int nt = len - c0 < HMM_EC ? len - c0 : HMM_EC;
        hmm_emis<T, false, EM>(A, X + (long long)c0 * A.ld, nt, sb, smx);   // (its first barrier also covers sA / cur above)
        for (int t = 0; t < nt; ++t) {
            const bool head = first && c0 + t == 0;
            double v[HMM_EPT], mx = 0.0;
#pragma unroll
            for (int r = 0; r < HMM_EPT; ++r) {
                v[r] = 0.0;
                if (ei[r] >= 0) {
                    double acc;
                    if (head) {
                        acc = cur[ei[r] * K + ej[r]];
                    } else {
                        acc = 0.0;
                        const double* pr = cur + ei[r] * K;
                        const double* pa = sA + ej[r];
                        for (int l = 0; l < K; ++l) acc += pr[l] * pa[l * KP];
                    }
                    acc *= sb[t * K + ej[r]];
                    v[r] = acc;
                    mx = fmax(mx, acc);
                }
            }
            mx = hmm_wave_max(mx);
            if ((tid & 63) == 0) red[tid >> 6] = mx;
            __syncthreads();
            mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
            const double inv = 1.0 / mx;
#pragma unroll
            for (int r = 0; r < HMM_EPT; ++r)
                if (ei[r] >= 0) nxt[ei[r] * K + ej[r]] = v[r] * inv;
            logscale += smx[t] + log(mx);
            __syncthreads();
            double* sw = cur;
            cur = nxt;
            nxt = sw;
        }
    }
    double* op = A.ops + (long long)blockIdx.x * K2;
#pragma unroll
    for (int r = 0; r < HMM_EPT; ++r)
        if (ei[r] >= 0) op[tid + r * HMM_T] = cur[tid + r * HMM_T];
    if (tid == 0) A.opscale[blockIdx.x] = logscale;
}

// Operators (K^2 doubles and a log scale each) the stitch stages into LDS at a time: with its static K-vector the block
// stays under 48 KiB, what a launch may ask for without raising the kernel's limit; one operator at K = 64
__host__ __device__ inline int hmm_stitch_chunk(int K) { return (6144 - HMM_KMAX) / (K * K + 1) > 0 ? (6144 - HMM_KMAX) / (K * K + 1) : 1; }

// One wave per trajectory; lane = state.  The sweep is sequential over the trajectory's segments, so the operators are
// staged into LDS a chunk at a time (coalesced, all loads in flight at once): a step then costs K LDS reads, not the
// latency of a dependent global load.
__global__ __launch_bounds__(64) void hmm_stitch_kernel(HmmArgs A)
{
    extern __shared__ double hmm_sm[];
    __shared__ double sv[HMM_KMAX];
    const int K = A.K, K2 = K * K, j = threadIdx.x, C = hmm_stitch_chunk(K);
    const long long tr = blockIdx.x, g0 = A.seg0[tr], g1 = A.seg0[tr + 1];
    const bool on = j < K;
    double lmax = hmm_wave_max(on ? A.lsp[j] : -INFINITY);
    double a = on ? exp(A.lsp[j] - lmax) : 0.0;
    double ls = lmax;
    {   // normalised like every later entry vector
        const double n = hmm_wave_sum(a);
        a /= n;
        ls += log(n);
    }
    for (long long c0 = g0; c0 < g1; c0 += C) {
        const int nc = (int)(g1 - c0 < C ? g1 - c0 : C);
        __syncthreads();
        for (int e = j; e < nc * K2; e += 64) hmm_sm[e] = A.ops[c0 * K2 + e];
        for (int c = j; c < nc; c += 64) hmm_sm[C * K2 + c] = A.opscale[c0 + c];
        for (int c = 0; c < nc; ++c) {
            const long long g = c0 + c;
            if (on) {
                A.alpha_in[g * K + j] = a;
                sv[j] = a;
            }
            __syncthreads();
            const double* op = hmm_sm + c * K2;
            double u = 0.0;
            if (on)
                for (int i = 0; i < K; ++i) u += sv[i] * op[i * K + j];
            const double n = hmm_wave_sum(u);
            a = u / n;
            ls += hmm_sm[C * K2 + c] + log(n);
            __syncthreads();
        }
    }
    if (j == 0) A.traj_lp[tr] = ls;
    if (!A.beta_out) return;
    double b = 1.0;
    for (long long c1 = g1; c1 > g0; c1 -= C) {
        const long long c0 = c1 - C > g0 ? c1 - C : g0;
        const int nc = (int)(c1 - c0);
        __syncthreads();
        for (int e = j; e < nc * K2; e += 64) hmm_sm[e] = A.ops[c0 * K2 + e];
        for (int c = nc - 1; c >= 0; --c) {
            const long long g = c0 + c;
            if (on) {
                A.beta_out[g * K + j] = b;
                sv[j] = b;
            }
            __syncthreads();
            const double* op = hmm_sm + c * K2 + j * K;
            double v = 0.0;
            if (on)
                for (int i = 0; i < K; ++i) v += op[i] * sv[i];
            const double mx = hmm_wave_max(v);
            b = v / mx;
            __syncthreads();
        }
    }
}

template <typename T, int EM = HMM_GAUSS>
__global__ __launch_bounds__(HMM_T) void hmm_fused_kernel(HmmArgs A)
{
    extern __shared__ double hmm_sm[];
    const int K = A.K, KP = A.KP, K2 = K * K, F = A.F, S = A.S, tid = threadIdx.x;
    double* sA = hmm_sm;
    double* sal = sA + K * KP;      // alpha_t, overwritten by gamma_t on the way back
    double* sb = sal + S * K;       // b_t
    double* sn = sb + S * K;        // max_k l_t, then the normaliser n_t of alpha_t
    double* sae = sn + S;           // entry alpha
    double* sbe = sae + K;          // beta_t
    double* sw = sbe + K;           // b_t beta_t / (n_t g_t)
    double* sbb = sw + K;           // b_t beta_t
    int ei[HMM_EPT], ej[HMM_EPT];
    double xi[HMM_EPT];
#pragma unroll
    for (int r = 0; r < HMM_EPT; ++r) {
        const int e = tid + r * HMM_T;
        ei[r] = e < K2 ? e / K : -1;
        ej[r] = e < K2 ? e - ei[r] * K : 0;
        xi[r] = 0.0;
        if (e < K2) sA[ei[r] * KP + ej[r]] = A.A[e];
    }
    const long long w = blockIdx.x;
    const long long g0 = w * A.n_seg / A.G, g1 = (w + 1) * A.n_seg / A.G;
    double* part = A.part + w * A.psz;
    double* ppost = part;
    double* pobs = part + K;
    double* pobs2 = pobs + (long long)K * F;
    double* ptrans = EM == HMM_LINEAR ? pobs2 : pobs2 + (long long)K * F;
    const bool lane = tid < K;
    for (long long g = g0; g < g1; ++g) {
        long long row0;
        int len;
        bool first;
        hmm_locate(A, g, &row0, &len, &first);
        const T* X = static_cast<const T*>(A.X) + row0 * A.ld;
        __syncthreads();   // the previous segment's block is read no more
        if (lane) {
            sae[tid] = A.alpha_in[g * K + tid];
            sbe[tid] = A.beta_out[g * K + tid];
        }
        hmm_emis<T, false, EM>(A, X, len, sb, sn);
        // alpha through the segment (wave 0 works, the others keep step)
        for (int t = 0; t < len; ++t) {
            if (tid < 64) {
                const double* prev = t == 0 ? sae : sal + (t - 1) * K;
                double u = 0.0;
                if (lane) {
                    if (first && t == 0) {
                        u = prev[tid];
                    } else {
                        const double* pa = sA + tid;
                        for (int i = 0; i < K; ++i) u += prev[i] * pa[i * KP];
                    }
                    u *= sb[t * K + tid];
                }
                const double n = hmm_wave_sum(u);
                if (lane) sal[t * K + tid] = u / n;
                if (tid == 0) sn[t] = n;
            }
            __syncthreads();
        }
        // beta backwards: gamma_t into the alpha block, xi sums in registers
        for (int t = len - 1; t >= 0; --t) {
            if (tid < 64) {
                double ab = 0.0, bb = 0.0;
                if (lane) {
                    bb = sb[t * K + tid] * sbe[tid];
                    ab = sal[t * K + tid] * sbe[tid];
                }
                const double gs = hmm_wave_sum(ab);
                if (lane) {
                    sal[t * K + tid] = ab / gs;
                    sbb[tid] = bb;
                    sw[tid] = bb / (sn[t] * gs);
                }
            }
            __syncthreads();
            if (!(first && t == 0)) {
                const double* prev = t == 0 ? sae : sal + (t - 1) * K;
#pragma unroll
                for (int r = 0; r < HMM_EPT; ++r)
                    if (ei[r] >= 0) xi[r] += prev[ei[r]] * sw[ej[r]];
                if (tid < 64) {
                    double v = 0.0;
                    if (lane) {
                        const double* pa = sA + tid * KP;
                        for (int jj = 0; jj < K; ++jj) v += pa[jj] * sbb[jj];
                    }
                    const double mx = hmm_wave_max(v);
                    if (lane) sbe[tid] = v / mx;   // (sbb, not sbe, was read above)
                }
            }
            __syncthreads();
        }
        // gamma^T [1, X, X^2] (linear emission: gamma^T [1, Z]) from the LDS block, added to this workgroup's partial in
        // segment order
        const bool open = g == g0;
        if (lane) {
            double s = 0.0;
            for (int t = 0; t < len; ++t) s += sal[t * K + tid];
            ppost[tid] = open ? s : ppost[tid] + s;
        }
        for (int e = tid; e < K * F; e += HMM_T) {
            const int k = e / F, f = e - k * F;
            double s1 = 0.0, s2 = 0.0;
            for (int t = 0; t < len; ++t) {
                const double x = (double)X[(long long)t * A.ld + f], gm = sal[t * K + k];
                s1 += x * gm;
                if constexpr (EM == HMM_GAUSS) s2 += x * x * gm;
            }
            pobs[e] = open ? s1 : pobs[e] + s1;
            if constexpr (EM == HMM_GAUSS) pobs2[e] = open ? s2 : pobs2[e] + s2;
        }
    }
#pragma unroll
    for (int r = 0; r < HMM_EPT; ++r)
        if (ei[r] >= 0) ptrans[tid + r * HMM_T] = xi[r] * sA[ei[r] * KP + ej[r]];
}

__global__ __launch_bounds__(HMM_T) void hmm_reduce_kernel(HmmArgs A)
{
    const long long e = (long long)blockIdx.x * HMM_T + threadIdx.x;
    if (e >= A.psz) return;
    double s = 0.0;
    for (int w = 0; w < A.G; ++w) s += A.part[w * A.psz + e];
    A.out[e] = s;
}

template <typename T, int EM = HMM_GAUSS>
__global__ __launch_bounds__(HMM_T) void hmm_loglik_kernel(HmmArgs A)
{
    const long long idx = (long long)blockIdx.x * HMM_T + threadIdx.x;
    if (idx >= A.n * A.K) return;
    const long long row = idx / A.K;
    const int k = (int)(idx - row * A.K);
    bool bad = false;
    if constexpr (EM == HMM_LINEAR)
        A.loglik[idx] = hmm_linear1(static_cast<const T*>(A.X) + row * A.ld, A.mu + (long long)k * A.F, A.F, A.cst[k], &bad);
    else
        A.loglik[idx] = hmm_loglik1(static_cast<const T*>(A.X) + row * A.ld, A.mu + (long long)k * A.F, A.iv + (long long)k * A.F, A.F,
                                    A.cst[k], &bad);
    if (bad) *A.flag = 1;
}

// Viterbi in log space, one wave per trajectory, sequential in time; lane = state.  The induction takes the FIRST maximum
// over the previous state, which is also what the reference's traceback (its own argmax over the same sums) arrives at;
// the last frame takes the first maximum too.  One back-pointer byte per (frame, state).
template <typename T, int EM = HMM_GAUSS>
__global__ __launch_bounds__(64) void hmm_viterbi_kernel(HmmArgs A)
{
    extern __shared__ double hmm_sm[];
    const int K = A.K, i = threadIdx.x;
    double* sL = hmm_sm;                 // log A, row-major: lane i reads sL[j * K + i]
    double* se = sL + K * K;             // emissions of a chunk, HMM_VC x K
    double* sv = se + HMM_VC * K;        // the previous frame's lattice row
    unsigned char* sbp = reinterpret_cast<unsigned char*>(sv + K);   // a chunk of back-pointers, HMM_VC x K
    const long long tr = blockIdx.x, row0 = A.off[tr], len = A.off[tr + 1] - row0;
    for (int e = i; e < K * K; e += 64) sL[e] = A.logA[e];
    const T* X = static_cast<const T*>(A.X) + row0 * A.ld;
    const bool on = i < K;
    double v = 0.0;
    for (long long c0 = 0; c0 < len; c0 += HMM_VC) {
        const int nt = (int)(len - c0 < HMM_VC ? len - c0 : HMM_VC);
        __syncthreads();
        hmm_emis<T, true, EM>(A, X + c0 * A.ld, nt, se, nullptr);
        for (int t = 0; t < nt; ++t) {
            if (c0 + t == 0) {
                if (on) v = A.lsp[i] + se[i];
            } else {
                int arg = 0;
                double best = 0.0;
                if (on) {
                    best = sv[0] + sL[i];
                    for (int j = 1; j < K; ++j) {
                        const double c = sv[j] + sL[j * K + i];
                        if (c > best) {
                            best = c;
                            arg = j;
                        }
                    }
                    v = best + se[t * K + i];
                    A.bp[(row0 + c0 + t) * K + i] = (unsigned char)arg;
                }
            }
            __syncthreads();
            if (on) sv[i] = v;
            __syncthreads();
        }
    }
    // traceback: chunks of back-pointers through LDS, lane 0 walks them
    int s = 0;
    if (i == 0) {
        for (int k = 1; k < K; ++k)
            if (sv[k] > sv[s]) s = k;
        A.traj_lp[tr] = sv[s];
        A.states[row0 + len - 1] = s;
    }
    for (long long c1 = len; c1 > 1; c1 -= HMM_VC) {   // frames (c0, c1) excluding 0: pointers of frames c0 .. c1 - 1, c0 >= 1
        const long long c0 = c1 - HMM_VC > 1 ? c1 - HMM_VC : 1;
        __syncthreads();
        const unsigned char* src = A.bp + (row0 + c0) * K;
        const int nb = (int)(c1 - c0) * K;
        for (int e = i; e < nb; e += 64) sbp[e] = src[e];
        __syncthreads();
        if (i == 0)
            for (long long t = c1 - 1; t >= c0; --t) {
                s = sbp[(t - c0) * K + s];
                A.states[row0 + t - 1] = s;
            }
    }
}

// The image of the angles: Z[t, f] = cos(x_tf), Z[t, F + f] = sin(x_tf), the element widened exactly and the
// trigonometry in float64.  Elementwise, bound by HBM (itemsize in, 16 bytes out per element); a grid-stride loop.  A
// non-finite angle gives NaN in Z, which the linear emission's own check reports.
template <typename T>
__global__ __launch_bounds__(HMM_T) void hmm_trig_kernel(const T* X, long long ld, long long n, int F, double* Z, long long ldz)
{
    const long long total = n * F, step = (long long)gridDim.x * HMM_T;
    for (long long e = (long long)blockIdx.x * HMM_T + threadIdx.x; e < total; e += step) {
        const long long t = e / F;
        const int f = (int)(e - t * F);
        double s, c;
        sincos((double)X[t * ld + f], &s, &c);
        Z[t * ldz + f] = c;
        Z[t * ldz + F + f] = s;
    }
}

}  // namespace msm
