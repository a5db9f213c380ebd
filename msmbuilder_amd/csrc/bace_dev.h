// bace_dev.h -- the kernels of bace.hip: the Bayes factors of BACE lumping (lumping/bace.py:303-327) between the rows of a
// count matrix, as a tile kernel over all candidate pairs and a row kernel for one state against all others, and the four
// small kernels of the merge loop (lumping/bace.py:228-256).
//
// The definition is the reference's, in float64.  Over the columns k of the states still kept, in ascending order,
//     c1_k = c[i, k] + (unmerged[i] && unmerged[k] ? 1 / n : 0)          p1_k = c1_k / w[i]          (likewise c2, p2 for j)
//     cp_k = (c1_k + c2_k) / (w[i] + w[j])
//     a = sum_k c1_k * log(p1_k / cp_k)        b = sum_k c2_k * log(p2_k / cp_k)        d = a + b
// and what is stored is float32(1 / float32(d)), both roundings to nearest (the quotient of two float32 taken in float64
// and rounded once more is the correctly rounded float32 quotient: 53 >= 2 * 24 + 2).  A column whose state has been merged
// away or pruned is SKIPPED: its counts are zero in both rows and would give 0 * log(0 / 0).
//
// Every pair's two sums are built by ONE thread in ascending k from terms formed by bace_terms, in both kernels, so a pair
// has the same bits whichever kernel evaluated it; (i, j) and (j, i) agree as well: the sums of counts and of weights and
// the final a + b are commutative.  The unit is built with -ffp-contract=off.
#pragma once
#include "common.h"

namespace msm {

constexpr int BC_T = 256;               // threads per workgroup
constexpr int BC_TX = 16;               // tile kernel: 16 x 16 threads, each owns BC_R x BC_R pairs
constexpr int BC_R = 2;
constexpr int BC_TI = BC_TX * BC_R;     // 32 x 32 pairs per tile
constexpr int BC_CH = 32;               // tile kernel: columns staged per pass
constexpr int BC_PITCH = BC_CH + 1;
constexpr int BC_RP = 16;               // row kernel: pairs per workgroup
constexpr int BC_RC = 128;              // row kernel: columns per pass (BC_T / BC_RC threads share one column)
constexpr int BC_RPITCH = BC_RC + 1;
constexpr int BC_MAX_N = 16384;

struct BaceArgs {
    const double* c;        // n x n counts
    const double* w;        // n weights
    const int* unm;         // n: 1 while the state has not merged
    const int* alive;       // n: 1 while the state is kept
    long long n;
    double inv_n;           // 1.0 / n
    float* dmat;            // n x n stored values
    double* dout;           // nullable: n x n, d itself where a value is stored
};

// The state of the merge loop in device memory.
struct BaceLoop {
    double* c;
    double* w;
    int* unm;
    int* alive;
    float* dmat;
    float* rmax_val;        // per row: the first maximum among the positive entries (0 if none)
    int* rmax_col;          // its column (-1 if none)
    int* stale;             // rows whose maximum must be taken again
    int* cur;               // {x, y, dead, unmerged[x], unmerged[y]} of the selection being merged
    int* rec_xy;            // 2 ints per selection
    float* rec_val;
    long long n;
    double inv_n;
};
enum { BC_CUR_X = 0, BC_CUR_Y, BC_CUR_DEAD, BC_CUR_UX, BC_CUR_UY, BC_CUR_COUNT };

__device__ __forceinline__ void bace_terms(double c1, double p1, double c2, double p2, double wsum, double& ta, double& tb)
{
    const double cp = (c1 + c2) / wsum;
    ta = c1 * log(p1 / cp);
    tb = c2 * log(p2 / cp);
}

__device__ __forceinline__ float bace_stored(double d)
{
    const float f = (float)d;
    return (float)(1.0 / (double)f);
}

// One workgroup per 32 x 32 tile of pairs on or above the diagonal (grid-stride).  Counts (pseudo-count added) and their
// quotients by the row's weight go through LDS in chunks of BC_CH columns; rows past the end are staged as zeros and never
// written.  A value is stored for i < j, both kept, c[i, j] > 1; everything else of dmat is left as it was (zeroed by the host).
__global__ __launch_bounds__(BC_T) void bace_tile_kernel(BaceArgs P)
{
    __shared__ double Ac[BC_TI * BC_PITCH], Ap[BC_TI * BC_PITCH], Bc[BC_TI * BC_PITCH], Bp[BC_TI * BC_PITCH];
    __shared__ int Ks[BC_CH];
    const int tid = threadIdx.x, tx = tid % BC_TX, ty = tid / BC_TX;
    const long long n = P.n;
    const long long tiles = (n + BC_TI - 1) / BC_TI, total = tiles * tiles;
    for (long long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        const long long bi = tile / tiles, bj = tile - bi * tiles;
        if (bj < bi) continue;   // (uniform over the workgroup)
        double a[BC_R][BC_R], b[BC_R][BC_R], wsum[BC_R][BC_R];
#pragma unroll
        for (int u = 0; u < BC_R; ++u)
#pragma unroll
            for (int v = 0; v < BC_R; ++v) {
                const long long i = bi * BC_TI + ty + u * BC_TX, j = bj * BC_TI + tx + v * BC_TX;
                a[u][v] = b[u][v] = 0.0;
                wsum[u][v] = (i < n ? P.w[i] : 0.0) + (j < n ? P.w[j] : 0.0);
            }
        for (long long k0 = 0; k0 < n; k0 += BC_CH) {
            const int kw = (int)(n - k0 < BC_CH ? n - k0 : BC_CH);
            __syncthreads();   // the previous chunk has been read
            if (tid < BC_CH) Ks[tid] = tid < kw ? P.alive[k0 + tid] : 0;
            for (int e = tid; e < BC_TI * BC_CH; e += BC_T) {
                const int r = e / BC_CH, cc = e - r * BC_CH;
                const long long gi = bi * BC_TI + r, gj = bj * BC_TI + r, k = k0 + cc;
                double x = 0.0, px = 0.0, y = 0.0, py = 0.0;
                if (cc < kw && P.alive[k]) {
                    const int uk = P.unm[k];
                    if (gi < n && P.alive[gi]) {
                        x = P.c[gi * n + k] + ((P.unm[gi] && uk) ? P.inv_n : 0.0);
                        px = x / P.w[gi];
                    }
                    if (gj < n && P.alive[gj]) {
                        y = P.c[gj * n + k] + ((P.unm[gj] && uk) ? P.inv_n : 0.0);
                        py = y / P.w[gj];
                    }
                }
                Ac[r * BC_PITCH + cc] = x;
                Ap[r * BC_PITCH + cc] = px;
                Bc[r * BC_PITCH + cc] = y;
                Bp[r * BC_PITCH + cc] = py;
            }
            __syncthreads();
#pragma unroll 1
            for (int k = 0; k < kw; ++k) {
                if (!Ks[k]) continue;   // a state merged away or pruned: skipped (uniform)
                double c1[BC_R], p1[BC_R], c2[BC_R], p2[BC_R];
#pragma unroll
                for (int u = 0; u < BC_R; ++u) {
                    c1[u] = Ac[(ty + u * BC_TX) * BC_PITCH + k];
                    p1[u] = Ap[(ty + u * BC_TX) * BC_PITCH + k];
                    c2[u] = Bc[(tx + u * BC_TX) * BC_PITCH + k];
                    p2[u] = Bp[(tx + u * BC_TX) * BC_PITCH + k];
                }
#pragma unroll
                for (int u = 0; u < BC_R; ++u)
#pragma unroll
                    for (int v = 0; v < BC_R; ++v) {
                        double ta, tb;
                        bace_terms(c1[u], p1[u], c2[v], p2[v], wsum[u][v], ta, tb);
                        a[u][v] = a[u][v] + ta;
                        b[u][v] = b[u][v] + tb;
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < BC_R; ++u)
#pragma unroll
            for (int v = 0; v < BC_R; ++v) {
                const long long i = bi * BC_TI + ty + u * BC_TX, j = bj * BC_TI + tx + v * BC_TX;
                if (i >= n || j >= n || i >= j) continue;
                if (!P.alive[i] || !P.alive[j] || !(P.c[i * n + j] > 1.0)) continue;
                const double d = a[u][v] + b[u][v];
                P.dmat[i * n + j] = bace_stored(d);
                if (P.dout) P.dout[i * n + j] = d;
            }
    }
}

// State x (from cur when given, else fixed_x) against every kept j != x with c[x, j] > 1, stored at [x, j].  One workgroup
// per BC_RP consecutive j.  Per pass of BC_RC columns the threads form the terms of all BC_RP pairs side by side (rows read
// coalesced), then one thread per sum adds its BC_RC terms in ascending order: the order and the terms of the tile kernel.
__global__ __launch_bounds__(BC_T) void bace_row_kernel(BaceArgs P, const int* cur, int fixed_x)
{
    __shared__ double Ta[BC_RP * BC_RPITCH], Tb[BC_RP * BC_RPITCH];
    __shared__ double fin[2 * BC_RP];
    __shared__ int Ks[BC_RC];
    if (cur && cur[BC_CUR_DEAD]) return;
    const long long n = P.n, x = cur ? cur[BC_CUR_X] : fixed_x;
    const int tid = threadIdx.x, col = tid % BC_RC, part = tid / BC_RC;
    constexpr int PARTS = BC_T / BC_RC;
    const double wx = P.w[x];
    const int ux = P.unm[x];
    const long long groups = (n + BC_RP - 1) / BC_RP;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long j0 = g * BC_RP;
        unsigned cand = 0;   // (every thread takes the same 16 flags: uniform without a barrier)
        for (int r = 0; r < BC_RP; ++r) {
            const long long j = j0 + r;
            if (j < n && j != x && P.alive[j] && P.c[x * n + j] > 1.0) cand |= 1u << r;
        }
        if (!cand) continue;
        double acc = 0.0;   // threads 0 .. 15: a of pair tid; threads 16 .. 31: b of pair tid - 16
        for (long long k0 = 0; k0 < n; k0 += BC_RC) {
            const int kw = (int)(n - k0 < BC_RC ? n - k0 : BC_RC);
            __syncthreads();   // the previous terms have been added
            const long long k = k0 + col;
            const int live = col < kw && P.alive[k];
            if (part == 0) Ks[col] = live;
            if (live) {
                const int uk = P.unm[k];
                const double cx = P.c[x * n + k] + ((ux && uk) ? P.inv_n : 0.0);
                const double px = cx / wx;
                for (int r = part; r < BC_RP; r += PARTS) {
                    if (!(cand >> r & 1)) continue;
                    const long long j = j0 + r;
                    const double wj = P.w[j];
                    const double cj = P.c[j * n + k] + ((P.unm[j] && uk) ? P.inv_n : 0.0);
                    const double pj = cj / wj;
                    double ta, tb;
                    bace_terms(cx, px, cj, pj, wx + wj, ta, tb);
                    Ta[r * BC_RPITCH + col] = ta;
                    Tb[r * BC_RPITCH + col] = tb;
                }
            }
            __syncthreads();
            if (tid < 2 * BC_RP && (cand >> (tid % BC_RP) & 1)) {
                const double* T = (tid < BC_RP ? Ta : Tb) + (tid % BC_RP) * BC_RPITCH;
                for (int kk = 0; kk < kw; ++kk)
                    if (Ks[kk]) acc = acc + T[kk];
            }
        }
        if (tid < 2 * BC_RP) fin[tid] = acc;
        __syncthreads();
        if (tid < BC_RP && (cand >> tid & 1)) {
            const double d = fin[tid] + fin[tid + BC_RP];
            const long long j = j0 + tid;
            P.dmat[x * n + j] = bace_stored(d);
            if (P.dout) P.dout[x * n + j] = d;
        }
        __syncthreads();   // fin is free again
    }
}

// ---- the merge loop ---------------------------------------------------------------------------------------------------
// Greater value first; among equal values (two inf included) the lower index: the first maximum.  A NaN is never chosen.
__device__ __forceinline__ bool bace_better(float v, int i, float bv, int bi)
{
    return v > bv || (v == bv && v > 0.0f && (bi < 0 || i < bi));
}

// Rows marked stale: the first maximum among the positive entries of the row.  One workgroup per row (grid-stride).
__global__ __launch_bounds__(BC_T) void bace_rowmax_kernel(BaceLoop L)
{
    __shared__ float sv[BC_T];
    __shared__ int si[BC_T];
    if (L.cur[BC_CUR_DEAD]) return;
    const int tid = threadIdx.x;
    const long long n = L.n;
    for (long long r = blockIdx.x; r < n; r += gridDim.x) {
        if (!L.stale[r]) continue;   // (uniform)
        float bv = 0.0f;
        int bc = -1;
        for (long long k = tid; k < n; k += BC_T) {
            const float v = L.dmat[r * n + k];
            if (v > bv) {   // ascending k: the first of equal values stays
                bv = v;
                bc = (int)k;
            }
        }
        sv[tid] = bv;
        si[tid] = bc;
        __syncthreads();
        for (int s = BC_T / 2; s > 0; s >>= 1) {
            if (tid < s && bace_better(sv[tid + s], si[tid + s], sv[tid], si[tid])) {
                sv[tid] = sv[tid + s];
                si[tid] = si[tid + s];
            }
            __syncthreads();
        }
        if (tid == 0) {
            L.rmax_val[r] = sv[0];
            L.rmax_col[r] = si[0];
            L.stale[r] = 0;
        }
        __syncthreads();
    }
}

// ONE workgroup: the first maximum of the matrix in row-major order from the per-row maxima, appended to the record at
// `step`.  With do_merge the selection is the next merge: it becomes cur and the weights move.  No positive entry: the
// record gets (-1, -1, 0) and the loop is dead from here on (every later kernel returns at once).
__global__ __launch_bounds__(BC_T) void bace_select_kernel(BaceLoop L, int step, int do_merge)
{
    __shared__ float sv[BC_T];
    __shared__ int si[BC_T];
    const int tid = threadIdx.x;
    const long long n = L.n;
    float bv = 0.0f;
    int br = -1;
    if (!L.cur[BC_CUR_DEAD])
        for (long long r = tid; r < n; r += BC_T) {
            const float v = L.rmax_val[r];
            if (L.rmax_col[r] >= 0 && v > bv) {
                bv = v;
                br = (int)r;
            }
        }
    sv[tid] = bv;
    si[tid] = br;
    __syncthreads();
    for (int s = BC_T / 2; s > 0; s >>= 1) {
        if (tid < s && bace_better(sv[tid + s], si[tid + s], sv[tid], si[tid])) {
            sv[tid] = sv[tid + s];
            si[tid] = si[tid + s];
        }
        __syncthreads();
    }
    if (tid != 0) return;
    const int x = si[0];
    if (x < 0) {
        L.rec_xy[2 * step] = L.rec_xy[2 * step + 1] = -1;
        L.rec_val[step] = 0.0f;
        L.cur[BC_CUR_DEAD] = 1;
        return;
    }
    const int y = L.rmax_col[x];
    L.rec_xy[2 * step] = x;
    L.rec_xy[2 * step + 1] = y;
    L.rec_val[step] = sv[0];
    if (!do_merge) return;
    L.cur[BC_CUR_X] = x;
    L.cur[BC_CUR_Y] = y;
    L.cur[BC_CUR_UX] = L.unm[x];
    L.cur[BC_CUR_UY] = L.unm[y];
    L.w[x] = L.w[x] + L.w[y];
    L.w[y] = 0.0;
}

// Merge cur's y into x, one thread per state k: the pseudo-counts of a first merge, row and column y added to row and
// column x and zeroed, rows and columns x and y of the stored matrix zeroed, the flags, and the rows whose cached maximum
// is gone marked stale.  Thread k touches only [x, k], [y, k], [k, x], [k, y] (k == x: the 2 x 2 block where they meet, in the
// reference's order of statements) and its own flags, so no two threads meet.
__global__ __launch_bounds__(BC_T) void bace_update_kernel(BaceLoop L)
{
    if (L.cur[BC_CUR_DEAD]) return;
    const long long n = L.n, k = (long long)blockIdx.x * BC_T + threadIdx.x;
    if (k >= n) return;
    const long long x = L.cur[BC_CUR_X], y = L.cur[BC_CUR_Y];
    const int ux = L.cur[BC_CUR_UX], uy = L.cur[BC_CUR_UY];
    const double pc = L.inv_n;
    L.dmat[x * n + k] = 0.0f;
    L.dmat[y * n + k] = 0.0f;
    L.dmat[k * n + x] = 0.0f;
    L.dmat[k * n + y] = 0.0f;
    if (k == y) {
        L.rmax_val[k] = 0.0f;
        L.rmax_col[k] = -1;
        L.stale[k] = 0;
    } else if (k == x || L.rmax_col[k] == x || L.rmax_col[k] == y) {
        L.stale[k] = 1;
    }
    if (!L.alive[k]) return;
    double* c = L.c;
    if (k != x && k != y) {
        const double pk = L.unm[k] ? pc : 0.0;
        double cxk = c[x * n + k], cyk = c[y * n + k], ckx = c[k * n + x], cky = c[k * n + y];
        if (ux) {
            cxk = cxk + pk;
            ckx = ckx + pk;
        }
        if (uy) {
            cyk = cyk + pk;
            cky = cky + pk;
        }
        c[x * n + k] = cxk + cyk;
        c[k * n + x] = ckx + cky;
        c[y * n + k] = 0.0;
        c[k * n + y] = 0.0;
    } else if (k == x) {
        double xx = c[x * n + x], xy = c[x * n + y], yx = c[y * n + x], yy = c[y * n + y];
        int fx = ux, fy = uy;
        if (fx) {
            xx = xx + pc;                     // row x, while x still counts as unmerged
            xy = xy + (fy ? pc : 0.0);
            fx = 0;
            yx = yx + (fy ? pc : 0.0);        // column x
        }
        if (fy) {
            yy = yy + pc;                     // row y (x has merged: nothing at [y, x]); column y adds nothing here
            fy = 0;
        }
        xx = xx + yx;                         // row x += row y
        xy = xy + yy;
        xx = xx + xy;                         // column x += column y
        c[x * n + x] = xx;
        c[x * n + y] = 0.0;
        c[y * n + x] = 0.0;
        c[y * n + y] = 0.0;
        L.unm[x] = 0;
    } else {
        L.unm[y] = 0;
        L.alive[y] = 0;
    }
}

__global__ __launch_bounds__(BC_T) void bace_check_kernel(const double* __restrict__ c, long long total, int* bad)
{
    for (long long i = (long long)blockIdx.x * BC_T + threadIdx.x; i < total; i += (long long)gridDim.x * BC_T) {
        const double v = c[i];
        if (!(v >= 0.0) || v > 1.7976931348623157e308) *bad = 1;
    }
}

}  // namespace msm
