// regspatial_dev.h -- rs_screen_small_kernel / rs_screen_tile_kernel / rs_resolve_kernel: regular spatial (leader)
// clustering in row blocks (cluster/regularspatial.py:69-81 of the reference, one libdistance.dist call per row there).
//
// A block of B consecutive rows is SCREENED against the K centres known when the block starts: a row is covered as soon
// as one distance fails `d > d_min` (a NaN distance fails it).  The rows no centre covers (the survivors) are COMPACTED
// in ascending order and RESOLVED by one workgroup: the first live survivor becomes a centre, every later live survivor
// is tested against it and dies if it is covered; repeat until none is live.  The block's new centres are APPENDED to the
// device centre list (ids and coordinates) by a third kernel once the host has made room for them.  Every distance is m_update / m_final in
// feature order with one fp64 accumulator per (centre, row) pair, the centre as first argument -- the reference's
// arithmetic, so every decision is the reference's (built with -ffp-contract=off).
#pragma once
#include "common.h"
#include "distance_dev.h"

namespace msm {

constexpr int RS_RT = 1024;                       // threads of the resolve workgroup
constexpr int RS_LDS_BYTES = 16384;               // centre tile of the register-path screen
enum RsStat { RS_K = 0, RS_SURV, RS_ROUNDS, RS_NSTAT };

struct RsArgs {
    const void* X;             // [n, m] rows
    long long m;
    long long row0;            // first row of the block
    int B;                     // rows in the block
    int vecw;                  // register path: vector width in bytes of the per-lane row loads
    void* cen;                 // centre list, coordinates [capacity, m]
    msm_idx_t* ids;            // centre list, row ids [capacity]
    long long K;               // centres known when the block starts
    msm_idx_t* newids;         // [B] rows the resolve step chose in this block, in order
    double d_min;
    unsigned long long* mask;  // one word per wave of the screen grid: bit l = row 64 w + l is uncovered
    int* surv;                 // [B] block-relative rows of the survivors, ascending; -1 once covered in the resolve
    long long* stat;           // RsStat counters
};

// Screen, rows in registers (m <= FC).  A tile of centres is staged once per workgroup; a wave whose 64 rows are all
// covered skips the arithmetic (checked every 8 centres), the workgroup leaves when all four are.
template <typename T, int M>
__global__ __launch_bounds__(DT) void rs_screen_small_kernel(RsArgs P)
{
    constexpr int FC = FeatChunk<T>::FC;
    constexpr int YCAP = RS_LDS_BYTES / (int)sizeof(T);
    constexpr int GS = 16 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) T Ys[YCAP];
    const T* X = static_cast<const T*>(P.X);
    const T* Y = static_cast<const T*>(P.cen);
    const int tid = threadIdx.x;
    const int m = (int)P.m;
    const int mp = (m + GS - 1) / GS * GS;   // centre pitch: whole 16-byte groups, zero padded (exact for every metric)
    const int KT = YCAP / mp;
    const long long r = (long long)blockIdx.x * DT + tid;
    bool covered = r >= P.B;
    T x[FC];
    load_row_regs<T>(x, X + (P.row0 + (covered ? P.B - 1 : r)) * P.m, m, P.vecw);
    for (long long j0 = 0; j0 < P.K; j0 += KT) {
        if (!__syncthreads_or(!covered)) break;   // (also: everyone is done reading the previous tile)
        const int kt = (int)((P.K - j0) < KT ? (P.K - j0) : KT);
        for (int e = tid; e < kt * mp; e += DT) {
            const int c = e / mp, ff = e - c * mp;
            Ys[e] = ff < m ? Y[(j0 + c) * P.m + ff] : (T)0;
        }
        __syncthreads();
        if (__any(!covered)) {
            for (int c = 0; c < kt; ++c) {
                const T* yc = Ys + c * mp;
                double a = 0.0, b = 0.0;
#pragma unroll
                for (int g = 0; g < FC / GS; ++g)
                    if (g * GS < m) {
#pragma unroll
                        for (int q = 0; q < GS; ++q) m_update<T, M>(a, b, yc[g * GS + q], x[g * GS + q]);
                    }
                const double d = m_final<M>(a, b, P.m);
                if (!(d > P.d_min)) covered = true;
                if ((c & 7) == 7 && !__any(!covered)) break;
            }
        }
    }
    const unsigned long long live = __ballot(!covered);
    if ((tid & 63) == 0) P.mask[r >> 6] = live;
}

// Screen, wider rows: a [256 rows x FC features] tile through LDS per feature chunk, CJ centres per register tile, as
// pair_kernel.  The workgroup leaves between centre groups once all its rows are covered; a covered wave skips the arithmetic.
template <typename T, int M>
__global__ __launch_bounds__(DT) void rs_screen_tile_kernel(RsArgs P)
{
    constexpr int FC = FeatChunk<T>::FC;
    __shared__ T Xs[DT * (FC + 1)];
    __shared__ T Ys[CJ * FC];
    const T* Xb = static_cast<const T*>(P.X) + P.row0 * P.m;
    const T* Y = static_cast<const T*>(P.cen);
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * DT;
    const long long r = t0 + tid;
    bool covered = r >= P.B;
    for (long long j0 = 0; j0 < P.K; j0 += CJ) {
        if (!__syncthreads_or(!covered)) break;
        const bool wave_live = __any(!covered);
        double a[CJ], b[CJ];
#pragma unroll
        for (int c = 0; c < CJ; ++c) {
            a[c] = 0.0;
            b[c] = 0.0;
        }
        for (long long f0 = 0; f0 < P.m; f0 += FC) {
            const int fw = (int)((P.m - f0) < FC ? (P.m - f0) : FC);
            __syncthreads();
            stage_rows<T>(Xs, Xb, nullptr, t0, P.B, P.m, (int)f0, fw, tid);
            for (int e = tid; e < CJ * fw; e += DT) {
                const int c = e / fw, ff = e - c * fw;
                Ys[c * FC + ff] = (j0 + c < P.K) ? Y[(j0 + c) * P.m + f0 + ff] : (T)0;
            }
            __syncthreads();
            if (wave_live)
                for (int ff = 0; ff < fw; ++ff) {
                    const T x = Xs[tid * (FC + 1) + ff];
#pragma unroll
                    for (int c = 0; c < CJ; ++c) m_update<T, M>(a[c], b[c], Ys[c * FC + ff], x);
                }
        }
        if (wave_live) {
#pragma unroll
            for (int c = 0; c < CJ; ++c)
                if (j0 + c < P.K) {
                    const double d = m_final<M>(a[c], b[c], P.m);
                    if (!(d > P.d_min)) covered = true;
                }
        }
    }
    const unsigned long long live = __ballot(!covered);
    if ((tid & 63) == 0) P.mask[r >> 6] = live;
}

// Compact + resolve, ONE workgroup.  Compact: every thread owns a run of consecutive mask words; a block scan of the
// popcounts gives its first output slot, so `surv` is ascending.  Resolve: thread t owns the survivors t, t + 1024, ...
// and a cursor over them; a round is one block-wide minimum of the cursors (the first live survivor = the new centre,
// noted in newids), then every thread tests its later live survivors against that row.  Only the owner ever writes
// a survivor's slot, the minimum's scratch alternates between rounds: one barrier per round.
template <typename T, int M>
__global__ __launch_bounds__(RS_RT) void rs_resolve_kernel(RsArgs P)
{
    __shared__ int scan[RS_RT];
    __shared__ int red[2][RS_RT / 64];
    const T* X = static_cast<const T*>(P.X);
    const int tid = threadIdx.x;
    const int nwords = (P.B + 63) / 64;
    const int wpt = (nwords + RS_RT - 1) / RS_RT;
    const int w0 = tid * wpt < nwords ? tid * wpt : nwords;
    const int w1 = w0 + wpt < nwords ? w0 + wpt : nwords;
    int cnt = 0;
    for (int w = w0; w < w1; ++w) cnt += (int)__popcll(P.mask[w]);
    scan[tid] = cnt;
    __syncthreads();
    for (int off = 1; off < RS_RT; off <<= 1) {
        const int v = tid >= off ? scan[tid - off] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const int S = scan[RS_RT - 1];
    int pos = scan[tid] - cnt;
    for (int w = w0; w < w1; ++w) {
        unsigned long long bits = P.mask[w];
        while (bits) {
            const int l = __ffsll(bits) - 1;
            P.surv[pos++] = w * 64 + l;   // < B: the screen sets no bit for a row outside the block
            bits &= bits - 1;
        }
    }
    __threadfence_block();
    __syncthreads();

    int cur = tid;
    int round = 0;
    for (;;) {
        while (cur < S && P.surv[cur] < 0) cur += RS_RT;
        int cand = cur < S ? cur : 0x7fffffff;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(cand, off);
            cand = o < cand ? o : cand;
        }
        if ((tid & 63) == 0) red[round & 1][tid >> 6] = cand;
        __syncthreads();
        int best = 0x7fffffff;
#pragma unroll
        for (int w = 0; w < RS_RT / 64; ++w) best = red[round & 1][w] < best ? red[round & 1][w] : best;
        if (best == 0x7fffffff) break;
        const long long crow = P.row0 + P.surv[best];   // (its owner only steps over it: the slot is not written again)
        const T* y = X + crow * P.m;
        if (tid == 0) P.newids[round] = crow;   // round < S <= B
        ++round;
        if (cur == best) cur += RS_RT;
        for (int s = cur; s < S; s += RS_RT) {
            const int rel = P.surv[s];
            if (rel < 0) continue;
            const T* x = X + (P.row0 + rel) * P.m;
            double a = 0.0, b = 0.0;
            for (long long f = 0; f < P.m; ++f) m_update<T, M>(a, b, y[f], x[f]);
            const double d = m_final<M>(a, b, P.m);
            if (!(d > P.d_min)) P.surv[s] = -1;
        }
    }
    if (tid == 0) {
        P.stat[RS_K] = P.K + round;
        P.stat[RS_SURV] += S;
        P.stat[RS_ROUNDS] += round;
    }
}

// Append: centre list slots K .. K + found - 1 <- the rows the resolve step chose (one workgroup per row, grid-strided).
template <typename T>
__global__ __launch_bounds__(DT) void rs_append_kernel(RsArgs P, long long found)
{
    const T* X = static_cast<const T*>(P.X);
    T* cen = static_cast<T*>(P.cen);
    for (long long j = blockIdx.x; j < found; j += gridDim.x) {
        const msm_idx_t row = P.newids[j];
        if (threadIdx.x == 0) P.ids[P.K + j] = row;
        for (long long f = threadIdx.x; f < P.m; f += DT) cen[(P.K + j) * P.m + f] = X[row * P.m + f];
    }
}

}  // namespace msm
