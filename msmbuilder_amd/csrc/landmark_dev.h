// landmark_dev.h -- the kernels of landmark.hip: agglomerative linkage on a square float64 working copy of a condensed
// distance matrix, the within-cluster sums of squared distances, and the pooled landmark predict.
//
// Linkage is plain global-minimum agglomeration.  Per slot the state is `active`, `size`, the id scipy gives the cluster
// that lives there, and a cached nearest neighbour among the ACTIVE columns ABOVE the row: (value, column), the lowest
// column at a tie.  A step is three launches, queued back to back with no host synchronisation:
//   select   the lowest cached value over the active rows, the lowest row at a tie -> the pair (i < j) and Z's row;
//   update   every other active slot k gets its Lance-Williams distance to the merged cluster, which keeps slot j;
//   refresh  one wave per row: rows whose cached column was i or j (and row j) are rescanned, rows below j compare their
//            cache against the one new value, rows above j have nothing to do.
// No workgroup waits for another inside a launch.
#pragma once
#include "common.h"

#include <cfloat>

#include "distance_dev.h"

namespace msm {

constexpr int LK_T = 256;            // threads per workgroup of the linkage kernels
constexpr int LK_ROWS = LK_T / 64;   // rows one refresh workgroup covers: one wave each

enum LkMethod : int { LK_SINGLE = 0, LK_COMPLETE, LK_AVERAGE, LK_WARD, LK_COUNT };

// Entry (i, j), i != j, of a condensed matrix of n elements; 64-bit throughout.
__host__ __device__ inline long long lm_condensed_index(long long i, long long j, long long n)
{
    const long long a = i < j ? i : j, b = i < j ? j : i;
    return n * a - a * (a + 1) / 2 + b - 1 - a;
}

struct LkSel {
    double d;        // the height of the merge
    int i, j;        // the slots, i < j; i < 0: there was no pair to merge
    int ni, nj;      // their sizes before the merge
};

struct LkArgs {
    double* D;        // n x n working copy, symmetric over the active slots
    long long n;
    int method;
    int* active;      // n
    int* size;        // n
    int* id;          // n: scipy's id of the cluster in the slot
    double* nnv;      // n: cached nearest neighbour among the active columns above the row: value,
    int* nnc;         // n:   column (-1: none)
    LkSel* sel;
    double* Z;        // (n - 1) x 4
    int* flag;        // [0]: the input holds a NaN or an infinite entry; [1]: a merged distance is not finite / no pair left
};

// condensed -> square, the finite check and the initial state
__global__ __launch_bounds__(LK_T) void lk_expand_kernel(const double* __restrict__ C, LkArgs P)
{
    const long long n = P.n, total = n * n;
    bool bad = false;
    for (long long p = (long long)blockIdx.x * LK_T + threadIdx.x; p < total; p += (long long)gridDim.x * LK_T) {
        const long long r = p / n, c = p - r * n;
        double x = 0.0;
        if (r != c) {
            x = C[lm_condensed_index(r, c, n)];
            bad |= !(fabs(x) <= DBL_MAX);
        }
        P.D[p] = x;
        if (p < n) {
            P.active[p] = 1;
            P.size[p] = 1;
            P.id[p] = (int)p;
        }
    }
    if (bad) P.flag[0] = 1;
}

// (value, column) of the lowest active entry of row r among the columns above r, the lowest column at a tie; one wave.
__device__ __forceinline__ void lk_rescan_row(const LkArgs& P, long long r, int lane)
{
    const long long n = P.n;
    const double* row = P.D + r * n;
    double best = INFINITY;
    int bc = -1;
    for (long long c = r + 1 + lane; c < n; c += 64) {
        if (!P.active[c]) continue;
        const double v = row[c];
        if (v < best) {   // ascending c within a lane: strict < keeps the lowest column
            best = v;
            bc = (int)c;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(best, off, 64);
        const int oc = __shfl_down(bc, off, 64);
        if (ov < best || (ov == best && oc >= 0 && oc < bc)) {
            best = ov;
            bc = oc;
        }
    }
    if (lane == 0) {
        P.nnv[r] = best;
        P.nnc[r] = bc;
    }
}

// all != 0: every row is scanned (the start).  Otherwise the refresh after the merge recorded in *P.sel.
__global__ __launch_bounds__(LK_T) void lk_refresh_kernel(LkArgs P, int all)
{
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * LK_ROWS + (threadIdx.x >> 6);
    if (r >= P.n || P.flag[0]) return;   // (uniform over the wave, like every exit below)
    if (all) {
        lk_rescan_row(P, r, lane);
        return;
    }
    const int i = P.sel->i, j = P.sel->j;
    if (i < 0 || r > j || !P.active[r]) return;   // rows above j: no column above them changed
    const int c = P.nnc[r];
    if (r == j || c == i || c == j || c < 0) {
        lk_rescan_row(P, r, lane);
        return;
    }
    if (lane == 0) {
        // every other column's value is what it was, and the cached one is still there: only the new value can beat it
        const double v = P.D[r * P.n + j];
        if (v < P.nnv[r] || (v == P.nnv[r] && j < c)) {
            P.nnv[r] = v;
            P.nnc[r] = j;
        }
    }
}

// One workgroup: the active row of lowest cached value, the lowest row at a tie; writes the pair and Z's row.
__global__ __launch_bounds__(LK_T) void lk_select_kernel(LkArgs P, long long step)
{
    __shared__ double sv[LK_T];
    __shared__ int sr[LK_T];
    const int tid = threadIdx.x;
    if (P.flag[0]) {
        if (tid == 0) P.sel->i = -1;
        return;
    }
    double best = INFINITY;
    int br = -1;
    for (long long r = tid; r < P.n; r += LK_T) {
        if (!P.active[r] || P.nnc[r] < 0) continue;
        const double v = P.nnv[r];
        if (v < best) {
            best = v;
            br = (int)r;
        }
    }
    sv[tid] = best;
    sr[tid] = br;
    __syncthreads();
    for (int k = LK_T / 2; k > 0; k >>= 1) {
        if (tid < k) {
            const double ov = sv[tid + k];
            const int orow = sr[tid + k];
            if (ov < sv[tid] || (ov == sv[tid] && orow >= 0 && orow < sr[tid])) {
                sv[tid] = ov;
                sr[tid] = orow;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        LkSel s;
        s.d = sv[0];
        s.i = sr[0];
        s.j = s.i >= 0 ? P.nnc[s.i] : -1;
        if (s.i < 0 || s.j <= s.i || s.j >= P.n) {   // nothing finite left to merge (never an address)
            s.i = s.j = -1;
            s.ni = s.nj = 0;
            P.flag[1] = 1;
        } else {
            s.ni = P.size[s.i];
            s.nj = P.size[s.j];
            const int a = P.id[s.i], b = P.id[s.j];
            double* z = P.Z + step * 4;
            z[0] = (double)(a < b ? a : b);
            z[1] = (double)(a < b ? b : a);
            z[2] = s.d;
            z[3] = (double)(s.ni + s.nj);
        }
        *P.sel = s;
    }
}

// Lance-Williams, float64, every product and sum left to right as written (the unit is built with -ffp-contract=off).
__device__ __forceinline__ double lk_merge(int method, double a, double b, double dij, double ni, double nj, double nk)
{
    if (method == LK_SINGLE) return a < b ? a : b;
    if (method == LK_COMPLETE) return a > b ? a : b;
    if (method == LK_AVERAGE) return (ni * a + nj * b) / (ni + nj);
    const double t = 1.0 / (ni + nj + nk);
    return sqrt((ni + nk) * t * a * a + (nj + nk) * t * b * b - nk * t * dij * dij);
}

__global__ __launch_bounds__(LK_T) void lk_update_kernel(LkArgs P, long long step)
{
    const long long n = P.n, k = (long long)blockIdx.x * LK_T + threadIdx.x;
    const LkSel s = *P.sel;
    if (s.i < 0 || k >= n) return;
    if (k == s.i) {
        P.active[k] = 0;
        return;
    }
    if (k == s.j) {   // the merged cluster keeps the higher slot (sizes of i and j travel in *P.sel: no one reads these here)
        P.size[k] = s.ni + s.nj;
        P.id[k] = (int)(n + step);
        return;
    }
    if (!P.active[k]) return;
    const double v = lk_merge(P.method, P.D[(long long)s.i * n + k], P.D[(long long)s.j * n + k], s.d, (double)s.ni,
                              (double)s.nj, (double)P.size[k]);
    P.D[(long long)s.j * n + k] = v;
    P.D[k * n + s.j] = v;
    if (!(fabs(v) <= DBL_MAX)) P.flag[1] = 1;
}

// ---- within-cluster sums of squared distances ---------------------------------------------------------------------
// rowsum[i] = sum over j > i with label[j] == label[i] of d(i, j)^2: thread t adds its columns i + 1 + t, + 256, ... in
// ascending order, then the 256 partial sums are added in a fixed binary tree.  out[c] = the rowsums of cluster c's rows,
// added the same way.  No atomics: two runs give the same bits.
__device__ __forceinline__ double lm_block_sum(double s, double* red, int tid)
{
    red[tid] = s;
    __syncthreads();
    for (int k = LK_T / 2; k > 0; k >>= 1) {
        if (tid < k) red[tid] += red[tid + k];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(LK_T) void lm_rowsum_kernel(const double* __restrict__ C, long long n, const int* __restrict__ lab,
                                                         double* __restrict__ rowsum)
{
    __shared__ double red[LK_T];
    const int tid = threadIdx.x;
    for (long long i = blockIdx.x; i < n; i += gridDim.x) {
        const int li = lab[i];
        const long long base = i * n - i * (i + 1) / 2 - i - 1;   // + j gives the condensed index
        double s = 0.0;
        for (long long j = i + 1 + tid; j < n; j += LK_T)
            if (lab[j] == li) {
                const double d = C[base + j];
                s = s + d * d;
            }
        s = lm_block_sum(s, red, tid);
        if (tid == 0) rowsum[i] = s;
    }
}

__global__ __launch_bounds__(LK_T) void lm_clustersum_kernel(const double* __restrict__ rowsum, long long n,
                                                             const int* __restrict__ lab, long long K, double* __restrict__ out)
{
    __shared__ double red[LK_T];
    const int tid = threadIdx.x;
    for (long long c = blockIdx.x; c < K; c += gridDim.x) {
        double s = 0.0;
        for (long long i = tid; i < n; i += LK_T)
            if (lab[i] == c) s = s + rowsum[i];
        s = lm_block_sum(s, red, tid);
        if (tid == 0) out[c] = s;
    }
}

// ---- pooled predict --------------------------------------------------------------------------------------------------
// One lane per row.  The landmarks, permuted so that cluster c's are off[c] .. off[c + 1] - 1, go through LDS in tiles
// of TL whole landmarks (rows wider than the tile: one landmark at a time in chunks of FCH features, the metric's
// accumulators carried across the chunks).  Each distance is one float64 accumulator over the features in order, the
// arithmetic of msm_cdist_* (m_update / m_final).  A cluster's pooled value is built one landmark at a time in ASCENDING
// landmark index -- min, max, or a running float64 sum of d (average) or d * d (ward), started at 0 -- and closed at the
// cluster's last landmark; the winner is a strict < over the clusters in ascending id from (+inf, 0), clusters with no
// landmark skipped.  min and max keep a NaN once they meet one (numpy's), and a NaN pooled value never wins.
constexpr int LP_T = 256;          // rows per workgroup
constexpr int LP_LDS = 32768;      // bytes of the landmark tile
constexpr int LP_TL_MAX = 512;     // landmarks per tile at most

enum LpPool : int { LP_SINGLE = 0, LP_COMPLETE, LP_AVERAGE, LP_WARD, LP_COUNT };

struct LpArgs {
    const void* X;          // n x m
    const void* Lm;         // L x m, permuted
    long long n, L, K, m;
    const long long* off;   // K + 1
    const double* intra;    // K (ward)
    msm_idx_t* labels;      // n
    double* pooled;         // n, nullable
    int* neg;               // set to 1 when a ward value is negative
    int pool;
    int TL, FCH;
};

// The pooling state of one row: the landmark l's distance d joins its cluster, and the cluster is closed at its last
// landmark.  Shared by the fused kernel below and the distance-matrix form (lp_predict_dmat_kernel).
struct LpPooler {
    const long long* off;
    const double* intra;
    int pool;
    double best = INFINITY, acc = 0.0;
    long long label = 0, c = -1, cstart = 0, cend = 0;
    bool negative = false;

    __device__ __forceinline__ LpPooler(const long long* off_, const double* intra_, int pool_) : off(off_), intra(intra_), pool(pool_) {}

    __device__ __forceinline__ void step(long long l, double d)
    {
        if (l >= cend) {
            do {   // the next cluster with a landmark (l < L = off[K]: there is one)
                ++c;
                cstart = cend;
                cend = off[c + 1];
            } while (l >= cend);
            acc = pool == LP_SINGLE ? INFINITY : pool == LP_COMPLETE ? -INFINITY : 0.0;
        }
        if (pool == LP_SINGLE)
            acc = (d < acc || d != d) ? d : acc;
        else if (pool == LP_COMPLETE)
            acc = (d > acc || d != d) ? d : acc;
        else if (pool == LP_AVERAGE)
            acc = acc + d;
        else
            acc = acc + d * d;
        if (l + 1 == cend) {
            const double cnt = (double)(cend - cstart);
            double v = acc;
            if (pool == LP_AVERAGE) v = acc / cnt;
            if (pool == LP_WARD) {
                v = (cnt * acc - intra[c]) / (cnt * (cnt + 1.0) / 2.0);
                negative |= v < 0.0;
            }
            if (v < best) {
                best = v;
                label = c;
            }
        }
    }
};

template <typename T, int M, bool REG>
__global__ __launch_bounds__(LP_T) void lp_predict_kernel(LpArgs P)
{
    constexpr int E = LP_LDS / (int)sizeof(T);
    constexpr int FC = FeatChunk<T>::FC;
    __shared__ T Ls[E];
    const T* __restrict__ X = static_cast<const T*>(P.X);
    const T* __restrict__ Lm = static_cast<const T*>(P.Lm);
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x * LP_T + tid, m = P.m, L = P.L;
    const bool valid = row < P.n;
    const T* xr = X + (valid ? row : 0) * m;
    T x[REG ? FC : 1];   // narrow rows stay in registers
    if constexpr (REG) {
#pragma unroll
        for (int f = 0; f < FC; ++f) x[f] = (valid && f < m) ? xr[f] : (T)0;
    }

    LpPooler pl(P.off, P.intra, P.pool);

    if (P.FCH == m) {
        for (long long l0 = 0; l0 < L; l0 += P.TL) {
            const int tl = (int)(L - l0 < P.TL ? L - l0 : P.TL);
            const int cnt = tl * (int)m;
            __syncthreads();   // the previous tile has been read
            for (int e = tid; e < cnt; e += LP_T) Ls[e] = Lm[l0 * m + e];
            __syncthreads();
            if (!valid) continue;
            for (int t = 0; t < tl; ++t) {
                const T* lv = Ls + t * (int)m;
                double a = 0.0, b = 0.0;
                if constexpr (REG) {
#pragma unroll
                    for (int f = 0; f < FC; ++f)
                        if (f < m) m_update<T, M>(a, b, x[f], lv[f]);
                } else {
                    for (int f = 0; f < (int)m; ++f) m_update<T, M>(a, b, xr[f], lv[f]);
                }
                pl.step(l0 + t, m_final<M>(a, b, m));
            }
        }
    } else {
        for (long long l = 0; l < L; ++l) {
            double a = 0.0, b = 0.0;
            for (long long f0 = 0; f0 < m; f0 += P.FCH) {
                const int fw = (int)(m - f0 < P.FCH ? m - f0 : P.FCH);
                __syncthreads();
                for (int e = tid; e < fw; e += LP_T) Ls[e] = Lm[l * m + f0 + e];
                __syncthreads();
                if (valid)
                    for (int f = 0; f < fw; ++f) m_update<T, M>(a, b, xr[f0 + f], Ls[f]);
            }
            if (valid) pl.step(l, m_final<M>(a, b, m));
        }
    }
    if (valid) {
        P.labels[row] = pl.label;
        if (P.pooled) P.pooled[row] = pl.best;
        if (pl.negative) *P.neg = 1;
    }
}

// The same pooling over a row-major n x L float64 distance matrix (row stride ld) whose columns are the landmarks permuted
// by cluster: for metrics whose distances are computed by another kernel (the divergences).  One lane per row; the matrix
// goes through LDS in tiles of LD_TC columns so that the loads run along the rows.
constexpr int LD_TC = 16;

struct LdArgs {
    const double* D;
    long long n, L, ld;
    const long long* off;
    const double* intra;
    msm_idx_t* labels;
    double* pooled;
    int* neg;
    int pool;
};

__global__ __launch_bounds__(LP_T) void lp_predict_dmat_kernel(LdArgs P)
{
    __shared__ double Ds[LP_T * (LD_TC + 1)];
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * LP_T, row = row0 + tid;
    const bool valid = row < P.n;
    LpPooler pl(P.off, P.intra, P.pool);
    for (long long l0 = 0; l0 < P.L; l0 += LD_TC) {
        const int tc = (int)(P.L - l0 < LD_TC ? P.L - l0 : LD_TC);
        __syncthreads();   // the previous tile has been read
        for (int e = tid; e < LP_T * LD_TC; e += LP_T) {
            const int r = e / LD_TC, c = e - r * LD_TC;
            Ds[r * (LD_TC + 1) + c] = (row0 + r < P.n && c < tc) ? P.D[(row0 + r) * P.ld + l0 + c] : 0.0;
        }
        __syncthreads();
        if (valid)
            for (int t = 0; t < tc; ++t) pl.step(l0 + t, Ds[tid * (LD_TC + 1) + t]);
    }
    if (valid) {
        P.labels[row] = pl.label;
        if (P.pooled) P.pooled[row] = pl.best;
        if (pl.negative) *P.neg = 1;
    }
}

// Rows r0 .. r0 + rb - 1 of the square form of a condensed matrix of n elements, the columns taken in the order perm
// (the landmarks permuted by cluster), the diagonal exactly zero: out is rb x n, row-major.
__global__ __launch_bounds__(LP_T) void lp_expand_rows_kernel(const double* __restrict__ C, long long n, const long long* __restrict__ perm,
                                                              long long r0, long long rb, double* __restrict__ out)
{
    const long long total = rb * n;
    for (long long p = (long long)blockIdx.x * LP_T + threadIdx.x; p < total; p += (long long)gridDim.x * LP_T) {
        const long long r = r0 + p / n, c = perm[p % n];
        out[p] = r == c ? 0.0 : C[lm_condensed_index(r, c, n)];
    }
}

}  // namespace msm
