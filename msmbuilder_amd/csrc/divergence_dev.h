// divergence_dev.h -- the kernels of divergence.hip: Kullback-Leibler, symmetrised KL, Jensen-Shannon divergence and the
// Jensen-Shannon metric between non-negative rows (utils/divergence.py:14-52), as a cdist / condensed pdist tile kernel and
// a paired-rows kernel.
//
// The definition is the reference's manual loop, in float64 (float32 rows are widened exactly):
//     kl(P, Q) = max(sum_k [P_k * Q_k != 0] P_k * log(P_k / Q_k), 0)      ascending k, a NaN sum stays NaN
//     sym_kl   = kl(P, Q) + kl(Q, P)
//     js       = 0.5 * kl(P, M) + 0.5 * kl(Q, M),   M_k = (P_k + Q_k) / 2
//     js_metric = sqrt(js)
// A term is skipped where the float64 product is zero (an underflowing product included), so q = 0 under p > 0 adds
// nothing.  Every pair's sum is built by ONE thread in ascending k (dv_update), so the order is the reference's and the tile
// kernel, the paired-rows kernel and both output layouts give the same bits; the only differences to the host loop are the
// device's log and division.  The unit is built with -ffp-contract=off: products and sums stay separately rounded.
//
// Symmetry by construction: M, the product test and the two final sums are commutative in (P, Q), so d(i, j) and d(j, i)
// are the same bits for the three symmetric kinds, and P == Q gives M == P, ratio 1, log 0: d(i, i) == 0 exactly.
#pragma once
#include "common.h"

namespace msm {

enum DvKind : int { DV_KL = 0, DV_SYM_KL, DV_JS, DV_JS_METRIC, DV_COUNT };
int divergence_kind(const char* name);   // -1 if unknown

constexpr int DV_T = 256;               // threads per workgroup: 16 x 16
constexpr int DV_TX = 16;
constexpr int DV_R = 2;                 // each thread owns DV_R x DV_R pairs: rows ty, ty + 16, columns tx, tx + 16
constexpr int DV_TI = DV_TX * DV_R;     // 32 rows of A per tile
constexpr int DV_TJ = DV_TX * DV_R;     // 32 rows of B per tile
constexpr int DV_CH = 32;               // columns staged per pass
constexpr int DV_PITCH = DV_CH + 1;     // doubles: the 16 B-rows a wave reads at one k fall into 16 different bank pairs

template <int KIND>
__device__ __forceinline__ void dv_update(double& a, double& b, double p, double q)
{
    if constexpr (KIND == DV_KL) {
        if (p * q != 0.0) a = a + p * log(p / q);
    } else if constexpr (KIND == DV_SYM_KL) {
        if (p * q != 0.0) {
            a = a + p * log(p / q);
            b = b + q * log(q / p);
        }
    } else {
        const double m = (p + q) / 2.0;
        if (p * m != 0.0) a = a + p * log(p / m);
        if (q * m != 0.0) b = b + q * log(q / m);
    }
}

// np.max([x, 0]): a NaN stays
__device__ __forceinline__ double dv_clamp(double x)
{
    return x != x ? x : (x > 0.0 ? x : 0.0);
}

template <int KIND>
__device__ __forceinline__ double dv_final(double a, double b)
{
    if constexpr (KIND == DV_KL) return dv_clamp(a);
    if constexpr (KIND == DV_SYM_KL) return dv_clamp(a) + dv_clamp(b);
    const double js = 0.5 * dv_clamp(a) + 0.5 * dv_clamp(b);
    if constexpr (KIND == DV_JS) return js;
    return sqrt(js);
}

struct DvArgs {
    const void* A;            // rows of A (indexed through idxA when given), m columns
    const void* B;
    const msm_idx_t* idxA;    // nullable
    const msm_idx_t* idxB;
    long long nA, nB, m;
    double* out;              // pd == 0: nA x nB row-major; pd != 0: condensed (i < j), nA == nB
    int pd;
};

// One workgroup per 32 x 32 tile of pairs (grid-stride over the tiles; in the condensed form tiles below the diagonal are
// skipped).  The rows go through LDS as float64 in chunks of DV_CH columns; rows past the end are staged as zeros, whose
// products are zero and add nothing.
template <typename T, int KIND>
__global__ __launch_bounds__(DV_T) void dv_tile_kernel(DvArgs P)
{
    __shared__ double As[DV_TI * DV_PITCH];
    __shared__ double Bs[DV_TJ * DV_PITCH];
    const T* __restrict__ A = static_cast<const T*>(P.A);
    const T* __restrict__ B = static_cast<const T*>(P.B);
    const int tid = threadIdx.x, tx = tid % DV_TX, ty = tid / DV_TX;
    const long long nA = P.nA, nB = P.nB, m = P.m;
    const long long tiles_j = (nB + DV_TJ - 1) / DV_TJ, total = ((nA + DV_TI - 1) / DV_TI) * tiles_j;
    for (long long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const long long bi = tile / tiles_j, bj = tile - bi * tiles_j;
        if (P.pd && bj < bi) continue;   // (uniform over the workgroup)
        double a[DV_R][DV_R], b[DV_R][DV_R];
#pragma unroll
        for (int u = 0; u < DV_R; ++u)
#pragma unroll
            for (int v = 0; v < DV_R; ++v) a[u][v] = b[u][v] = 0.0;
        for (long long k0 = 0; k0 < m; k0 += DV_CH) {
            const int kw = (int)(m - k0 < DV_CH ? m - k0 : DV_CH);
            __syncthreads();   // the previous chunk has been read
            for (int e = tid; e < DV_TI * DV_CH; e += DV_T) {
                const int r = e / DV_CH, c = e - r * DV_CH;
                const long long gi = bi * DV_TI + r, gj = bj * DV_TJ + r;
                double x = 0.0, y = 0.0;
                if (c < kw) {
                    if (gi < nA) x = (double)A[(P.idxA ? P.idxA[gi] : gi) * m + k0 + c];
                    if (gj < nB) y = (double)B[(P.idxB ? P.idxB[gj] : gj) * m + k0 + c];
                }
                As[r * DV_PITCH + c] = x;
                Bs[r * DV_PITCH + c] = y;
            }
            __syncthreads();
#pragma unroll 1
            for (int k = 0; k < kw; ++k) {
                double p[DV_R], q[DV_R];
#pragma unroll
                for (int u = 0; u < DV_R; ++u) {
                    p[u] = As[(ty + u * DV_TX) * DV_PITCH + k];
                    q[u] = Bs[(tx + u * DV_TX) * DV_PITCH + k];
                }
#pragma unroll
                for (int u = 0; u < DV_R; ++u)
#pragma unroll
                    for (int v = 0; v < DV_R; ++v) dv_update<KIND>(a[u][v], b[u][v], p[u], q[v]);
            }
        }
#pragma unroll
        for (int u = 0; u < DV_R; ++u)
#pragma unroll
            for (int v = 0; v < DV_R; ++v) {
                const long long i = bi * DV_TI + ty + u * DV_TX, j = bj * DV_TJ + tx + v * DV_TX;
                if (i >= nA || j >= nB) continue;
                const double d = dv_final<KIND>(a[u][v], b[u][v]);
                if (!P.pd)
                    P.out[i * nB + j] = d;
                else if (i < j)
                    P.out[nA * i - i * (i + 1) / 2 + j - 1 - i] = d;
            }
    }
}

// out[r] = div(P[r], Q[r]): one thread per pair of rows, the same dv_update chain.
template <typename T, int KIND>
__global__ __launch_bounds__(DV_T) void dv_rows_kernel(const T* __restrict__ Pm, const T* __restrict__ Qm, long long n, long long m,
                                                       double* __restrict__ out)
{
    for (long long r = (long long)blockIdx.x * DV_T + threadIdx.x; r < n; r += (long long)gridDim.x * DV_T) {
        double a = 0.0, b = 0.0;
        for (long long k = 0; k < m; ++k) dv_update<KIND>(a, b, (double)Pm[r * m + k], (double)Qm[r * m + k]);
        out[r] = dv_final<KIND>(a, b);
    }
}

// Host side (divergence.hip).  Queues the tile kernel on DEVICE pointers; nothing is synchronised.
template <typename T>
int divergence_tile_queue(int kind, const T* dA, const msm_idx_t* dIdxA, long long nA, const T* dB, const msm_idx_t* dIdxB,
                          long long nB, long long m, double* dOut, int pd);
// The divergence counterpart of pdist_queue (distance_dev.h): stages host rows / indices in the PS_X / PS_IDX slots and
// queues the condensed form into the DEVICE buffer dout.
template <typename T>
int divergence_pdist_queue(const T* X, int kind, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t nn, int on_device,
                           double* dout);

}  // namespace msm
