// kmeans_lloyd_dev.h -- the centre update of full-batch (Lloyd) k-means (included by kmeans.hip): a stable counting sort of
// the row numbers by label, a segmented float64 sum over the sorted rows and the per-cluster finish with the stop rules of
// scikit-learn's _kmeans_single_lloyd.  Every float64 sum has ONE order, fixed by the shape alone (no floating-point
// atomics; the only atomics are integer counters), so two runs on the same input give the same bits.
//
//   lloyd_hist_kernel     one wave per LH_SPAN consecutive rows: its label histogram into column g of hist[K][G], and the
//                         number of its rows whose label differs from the previous iteration's (integer atomicAdd)
//   lloyd_scan_kernel     one workgroup per cluster: exclusive prefix over the G columns in place, the cluster's size
//   lloyd_base_kernel     one workgroup: cluster starts, piece starts (a piece = LL_PIECE consecutive members), the number of
//                         empty clusters (> 0: the queued run stops with LLOYD_EMPTY, the host runs the relocation)
//   lloyd_piecemap_kernel piece -> cluster
//   lloyd_scatter_kernel  one wave per LH_SPAN rows again: row numbers to their sorted places, ascending inside a cluster
//   lloyd_segsum_kernel   one workgroup per (piece, feature tile): fp64 sums of the piece's rows, read once, 16-byte loads
//                         when the rows allow
//   lloyd_finish_kernel   one workgroup per cluster: pieces merged in piece order, relocated rows taken out / put in,
//                         centre = sum / count rounded once, ||c||^2 as kmeans_cnorm_kernel computes it, ||c_new - c_old||^2;
//                         the last workgroup to arrive plays the stop rules
#pragma once
#include "kmeans_common_dev.h"

namespace msm {

constexpr int LH_SPAN = 4096;   // rows of one histogram / scatter wave
constexpr int LH_KCH = 2048;    // labels counted per pass over the wave's rows (LDS counters)
constexpr int LL_PIECE = 256;   // members of one piece of the segmented sum
constexpr int LL_TU = 128;      // load units (16 bytes, or one element) of one feature tile, at most

enum { LLOYD_RUNNING = 0, LLOYD_STRICT = 1, LLOYD_TOL = 2, LLOYD_EMPTY = 3 };

// device state of a run: st[0] stop flag (LLOYD_*), [1] arrival counter, [2] changed-label accumulator, [3] changed labels
// of the iteration in flight, [4] iterations completed, [5] empty clusters of the iteration in flight
constexpr int LS_STOP = 0, LS_ARRIVE = 1, LS_CHACC = 2, LS_CHANGED = 3, LS_ITERS = 4, LS_EMPTY = 5, LS_COUNT = 8;

template <typename T>
struct LloydArgs {
    const T* X;
    long long n, m, K;
    T* C;                         // [K, m] centres, updated in place
    T* cnorm;                     // [K]
    const unsigned* order;        // [n] row numbers sorted by label (stable)
    const long long* count;       // [K]
    const long long* start;       // [K + 1]
    const int* pstart;            // [K + 1]
    const int* pk;                // [pieces] piece -> cluster
    double* partial;              // [pieces][m]
    double* shiftsq;              // [K]
    int* st;                      // LS_*
    double* shift_out;            // sum of shiftsq of the last finished iteration
    double tol;
    long long units;              // load units per row
    int tu;                       // units per feature tile (a power of two <= LL_TU)
    int n_reloc;                  // relocation (rare): rows taken from their clusters and given to empty ones
    const long long* reloc_row;
    const int* reloc_donor;
    const int* reloc_target;
};

// exclusive prefix of one value per thread over the workgroup (KNT threads); *total: the sum.  buf: KNT entries.
__device__ __forceinline__ long long lloyd_block_scan(long long v, long long* buf, long long* total)
{
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < KNT; d <<= 1) {
        const long long add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const long long incl = buf[t];
    *total = buf[KNT - 1];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(64) void lloyd_hist_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ prev,
                                                        long long n, long long K, long long G, unsigned* __restrict__ hist,
                                                        int* __restrict__ st)
{
    if (st[LS_STOP]) return;
    __shared__ unsigned cnt[LH_KCH];
    const long long g = blockIdx.x, base = g * LH_SPAN;
    const int lane = threadIdx.x;
    unsigned ch = 0;
    for (long long kc0 = 0; kc0 < K; kc0 += LH_KCH) {
        const unsigned kw = (unsigned)(K - kc0 < LH_KCH ? K - kc0 : LH_KCH);
        for (unsigned j = lane; j < kw; j += 64) cnt[j] = 0;
        __syncthreads();
        for (int r = 0; r < LH_SPAN / 64; ++r) {
            const long long i = base + r * 64 + lane;
            if (i < n) {
                const int l = lab[i];
                if (kc0 == 0 && l != prev[i]) ++ch;
                const unsigned rel = (unsigned)((long long)l - kc0);
                if (l >= 0 && rel < kw) atomicAdd(&cnt[rel], 1u);
            }
        }
        __syncthreads();
        for (unsigned j = lane; j < kw; j += 64) hist[(kc0 + j) * G + g] = cnt[j];
        __syncthreads();
    }
#pragma unroll
    for (int msk = 32; msk > 0; msk >>= 1) ch += __shfl_xor(ch, msk, 64);
    if (lane == 0 && ch) atomicAdd(reinterpret_cast<unsigned*>(st + LS_CHACC), ch);
}

__global__ __launch_bounds__(KNT) void lloyd_scan_kernel(unsigned* __restrict__ hist, long long G, long long* __restrict__ count,
                                                         const int* __restrict__ st)
{
    if (st[LS_STOP]) return;
    __shared__ long long buf[KNT];
    unsigned* row = hist + (long long)blockIdx.x * G;
    const long long per = (G + KNT - 1) / KNT;
    const long long a = threadIdx.x * per, b = a + per < G ? a + per : G;
    long long s = 0;
    for (long long q = a; q < b; ++q) s += row[q];
    long long total;
    long long run = lloyd_block_scan(s, buf, &total);
    for (long long q = a; q < b; ++q) {
        const unsigned v = row[q];
        row[q] = (unsigned)run;
        run += v;
    }
    if (threadIdx.x == 0) count[blockIdx.x] = total;
}

__global__ __launch_bounds__(KNT) void lloyd_base_kernel(const long long* __restrict__ count, long long K,
                                                         long long* __restrict__ start, int* __restrict__ pstart,
                                                         int* __restrict__ st)
{
    if (st[LS_STOP]) return;
    __shared__ long long buf[KNT];
    long long carry = 0, pcarry = 0, empty = 0;
    for (long long k0 = 0; k0 < K; k0 += KNT) {
        const long long k = k0 + threadIdx.x;
        const long long c = k < K ? count[k] : 0;
        const long long pc = (c + LL_PIECE - 1) / LL_PIECE;
        long long tot, ptot, etot;
        const long long ex = lloyd_block_scan(c, buf, &tot);
        const long long pex = lloyd_block_scan(pc, buf, &ptot);
        (void)lloyd_block_scan((k < K && c == 0) ? 1 : 0, buf, &etot);
        if (k < K) {
            start[k] = carry + ex;
            pstart[k] = (int)(pcarry + pex);
        }
        carry += tot;
        pcarry += ptot;
        empty += etot;
    }
    if (threadIdx.x == 0) {
        start[K] = carry;
        pstart[K] = (int)pcarry;
        st[LS_CHANGED] = st[LS_CHACC];
        st[LS_CHACC] = 0;
        st[LS_EMPTY] = (int)empty;
        if (empty > 0) st[LS_STOP] = LLOYD_EMPTY;
    }
}

__global__ __launch_bounds__(KNT) void lloyd_piecemap_kernel(const int* __restrict__ pstart, long long K, int* __restrict__ pk,
                                                             const int* __restrict__ st)
{
    if (st[LS_STOP]) return;
    const long long p = (long long)blockIdx.x * KNT + threadIdx.x;
    if (p >= pstart[K]) return;
    // the last k with pstart[k] <= p (empty clusters repeat their neighbour's start: the last one owns the piece)
    long long lo = 0, hi = K - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (pstart[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    pk[p] = (int)lo;
}

// Stable: a wave walks its rows 64 at a time in ascending order; inside a round the lanes of one label take consecutive
// places in lane order (one ballot per distinct label of the round).
__global__ __launch_bounds__(64) void lloyd_scatter_kernel(const int32_t* __restrict__ lab, long long n, long long K, long long G,
                                                           const unsigned* __restrict__ hist, const long long* __restrict__ start,
                                                           unsigned* __restrict__ order, const int* __restrict__ st)
{
    if (st[LS_STOP]) return;
    __shared__ unsigned cursor[LH_KCH];
    const long long g = blockIdx.x, base = g * LH_SPAN;
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long kc0 = 0; kc0 < K; kc0 += LH_KCH) {
        const unsigned kw = (unsigned)(K - kc0 < LH_KCH ? K - kc0 : LH_KCH);
        for (unsigned j = lane; j < kw; j += 64) cursor[j] = (unsigned)start[kc0 + j] + hist[(kc0 + j) * G + g];
        __syncthreads();
        for (int r = 0; r < LH_SPAN / 64; ++r) {
            const long long i = base + r * 64 + lane;
            int l = -1;
            if (i < n) l = lab[i];
            const unsigned rel = (unsigned)((long long)l - kc0);
            bool pending = l >= 0 && rel < kw;
            unsigned long long pm = __ballot(pending);
            while (pm) {   // uniform
                const int leader = __ffsll((long long)pm) - 1;
                const unsigned lrel = (unsigned)__shfl((int)rel, leader, 64);
                const bool mine = pending && rel == lrel;
                const unsigned long long mm = __ballot(mine);
                const unsigned at = cursor[lrel];
                if (mine) {
                    const unsigned pos = at + (unsigned)__popcll(mm & below);
                    if (pos < (unsigned long long)n) order[pos] = (unsigned)i;
                    pending = false;
                }
                __syncthreads();   // (one wave: orders the LDS read above before the write below)
                if (lane == leader) cursor[lrel] = at + (unsigned)__popcll(mm);
                __syncthreads();
                pm &= ~mm;
            }
        }
        __syncthreads();
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(KNT) void lloyd_segsum_kernel(LloydArgs<T> A)
{
    if (A.st[LS_STOP]) return;
    constexpr int E = VEC ? 16 / (int)sizeof(T) : 1;
    struct alignas(VEC ? 16 : sizeof(T)) V { T e[E]; };
    __shared__ double red[KNT * 4];   // [rowlanes][tu * E]
    const int p = blockIdx.x;
    if (p >= A.pstart[A.K]) return;   // uniform
    const int k = A.pk[p];
    if (k < 0 || k >= A.K) return;   // (cannot happen: the piece map is written by the launch before; keeps the loads in bounds)
    const long long c_end = A.start[k] + A.count[k];
    const long long a = A.start[k] + (long long)(p - A.pstart[k]) * LL_PIECE;
    const long long b = a + LL_PIECE < c_end ? a + LL_PIECE : c_end;
    const int tu = A.tu, R = KNT / tu;
    const int u = threadIdx.x & (tu - 1), r = threadIdx.x / tu;
    const long long unit = (long long)blockIdx.y * tu + u;
    double acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.0;
    if (unit < A.units) {
        const V* Xv = reinterpret_cast<const V*>(A.X);
        for (long long q = a + r; q < b; q += 4LL * R) {   // four rows in flight, added in row order
            const long long q1 = q + R, q2 = q + 2LL * R, q3 = q + 3LL * R;
            const unsigned i0 = A.order[q];
            const unsigned i1 = A.order[q1 < b ? q1 : q], i2 = A.order[q2 < b ? q2 : q], i3 = A.order[q3 < b ? q3 : q];
            const V v0 = Xv[(long long)i0 * A.units + unit], v1 = Xv[(long long)i1 * A.units + unit];
            const V v2 = Xv[(long long)i2 * A.units + unit], v3 = Xv[(long long)i3 * A.units + unit];
#pragma unroll
            for (int e = 0; e < E; ++e) {
                acc[e] += (double)v0.e[e];
                if (q1 < b) acc[e] += (double)v1.e[e];
                if (q2 < b) acc[e] += (double)v2.e[e];
                if (q3 < b) acc[e] += (double)v3.e[e];
            }
        }
    }
    const int width = tu * E;
#pragma unroll
    for (int e = 0; e < E; ++e) red[r * width + u * E + e] = acc[e];
    __syncthreads();
    for (int c = threadIdx.x; c < width; c += KNT) {
        const long long f = (long long)blockIdx.y * width + c;
        if (f >= A.m) continue;
        double s = 0.0;
        for (int rr = 0; rr < R; ++rr) s += red[rr * width + c];
        A.partial[(long long)p * A.m + f] = s;
    }
}

template <typename T>
__global__ __launch_bounds__(KNT) void lloyd_finish_kernel(LloydArgs<T> A)
{
    if (A.st[LS_STOP]) return;
    __shared__ double red[KNT];
    __shared__ int is_last;
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = A.pstart[k], p1 = A.pstart[k + 1];
    long long cnt = A.count[k];
    for (int q = 0; q < A.n_reloc; ++q) {
        if (A.reloc_donor[q] == k) --cnt;
        if (A.reloc_target[q] == k) cnt = 1;
    }
    double sq = 0.0;
    for (long long f = tid; f < A.m; f += KNT) {
        double s = 0.0;
        for (int p = p0; p < p1; ++p) s += A.partial[(long long)p * A.m + f];
        for (int q = 0; q < A.n_reloc; ++q) {
            const double x = (double)A.X[A.reloc_row[q] * A.m + f];
            if (A.reloc_donor[q] == k) s -= x;
            if (A.reloc_target[q] == k) s = x;
        }
        if (cnt > 0) {
            const T cn = (T)(s / (double)cnt);
            const double d = (double)cn - (double)A.C[(long long)k * A.m + f];
            sq += d * d;
            A.C[(long long)k * A.m + f] = cn;
        }
    }
    red[tid] = sq;
    __syncthreads();   // (also: the centre row is complete, workgroup-scope visibility)
    for (int d = KNT / 2; d > 0; d >>= 1) {
        if (tid < d) red[tid] += red[tid + d];
        __syncthreads();
    }
    if (wave == 0) {   // same lane partition and butterfly as kmeans_cnorm_kernel
        const volatile T* c = A.C + (long long)k * A.m;
        T s = 0;
        for (long long f = lane; f < A.m; f += 64) {
            const T v = c[f];
            s += v * v;
        }
#pragma unroll
        for (int msk = 32; msk > 0; msk >>= 1) s += __shfl_xor(s, msk, 64);
        if (lane == 0) A.cnorm[k] = s;
    }
    // the last workgroup to arrive closes the iteration (release before the arrival, acquire after it: the shifts of the
    // other workgroups come from other XCDs)
    if (tid == 0) {
        A.shiftsq[k] = red[0];
        __threadfence();
        is_last = (atomicAdd(reinterpret_cast<unsigned*>(A.st + LS_ARRIVE), 1u) == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (is_last && wave == 0) {
        __threadfence();
        const volatile double* sh = A.shiftsq;
        double s = 0.0;
        for (long long j = lane; j < A.K; j += 64) s += sh[j];
#pragma unroll
        for (int msk = 32; msk > 0; msk >>= 1) s += __shfl_xor(s, msk, 64);
        if (lane == 0) {
            A.st[LS_ARRIVE] = 0;
            A.st[LS_ITERS] += 1;
            *A.shift_out = s;
            if (A.st[LS_CHANGED] == 0) A.st[LS_STOP] = LLOYD_STRICT;
            else if (s <= A.tol) A.st[LS_STOP] = LLOYD_TOL;
        }
    }
}

// ---- relocation of empty clusters (rare; queued by the host after a run stopped with LLOYD_EMPTY) ----

// dist[i] = ||x_i - c_label(i)||^2 in the inertia kernel's arithmetic (difference in the rows' type, square and sum in fp64)
template <typename T>
__global__ __launch_bounds__(KNT) void lloyd_dist_kernel(const T* __restrict__ X, long long n, long long m, const T* __restrict__ C,
                                                         const int32_t* __restrict__ lab, double* __restrict__ dist)
{
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const T* x = X + i * m;
    const T* c = C + (long long)lab[i] * m;
    double s = 0.0;
    for (long long f = lane; f < m; f += 64) {
        const T d = x[f] - c[f];
        s += (double)d * (double)d;
    }
#pragma unroll
    for (int msk = 32; msk > 0; msk >>= 1) s += __shfl_xor(s, msk, 64);
    if (lane == 0) dist[i] = s;
}

__device__ __forceinline__ bool lloyd_farther(double v, long long i, double bv, long long bi)
{
    return v > bv || (v == bv && i < bi);   // equally far: the lowest row wins
}

// the farthest row not yet taken (taken rows carry -1): per-workgroup candidates, then one workgroup picks
__global__ __launch_bounds__(KNT) void lloyd_far_kernel(const double* __restrict__ dist, long long n, double* __restrict__ bv,
                                                        long long* __restrict__ bi)
{
    __shared__ double sv[KNT];
    __shared__ long long si[KNT];
    double v = -2.0;
    long long ix = 0x7fffffffffffffffLL;
    for (long long i = (long long)blockIdx.x * KNT + threadIdx.x; i < n; i += (long long)gridDim.x * KNT)
        if (lloyd_farther(dist[i], i, v, ix)) {
            v = dist[i];
            ix = i;
        }
    sv[threadIdx.x] = v;
    si[threadIdx.x] = ix;
    __syncthreads();
    for (int d = KNT / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d && lloyd_farther(sv[threadIdx.x + d], si[threadIdx.x + d], sv[threadIdx.x], si[threadIdx.x])) {
            sv[threadIdx.x] = sv[threadIdx.x + d];
            si[threadIdx.x] = si[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        bv[blockIdx.x] = sv[0];
        bi[blockIdx.x] = si[0];
    }
}

__global__ __launch_bounds__(KNT) void lloyd_take_kernel(const double* __restrict__ bv, const long long* __restrict__ bi, int nb,
                                                         long long n, double* __restrict__ dist, const int32_t* __restrict__ lab,
                                                         int q, long long* __restrict__ reloc_row, int* __restrict__ reloc_donor)
{
    __shared__ double sv[KNT];
    __shared__ long long si[KNT];
    double v = -2.0;
    long long ix = 0x7fffffffffffffffLL;
    for (int b = threadIdx.x; b < nb; b += KNT)
        if (lloyd_farther(bv[b], bi[b], v, ix)) {
            v = bv[b];
            ix = bi[b];
        }
    sv[threadIdx.x] = v;
    si[threadIdx.x] = ix;
    __syncthreads();
    for (int d = KNT / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d && lloyd_farther(sv[threadIdx.x + d], si[threadIdx.x + d], sv[threadIdx.x], si[threadIdx.x])) {
            sv[threadIdx.x] = sv[threadIdx.x + d];
            si[threadIdx.x] = si[threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        long long row = si[0];
        if (row < 0 || row >= n) row = 0;   // (fewer rows than empty clusters: cannot happen, n >= K)
        reloc_row[q] = row;
        reloc_donor[q] = lab[row];
        dist[row] = -1.0;
    }
}

}  // namespace msm
