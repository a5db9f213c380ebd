// kmedoids_dev.h -- the kernels of the k-medoids loop (kmedoids.hip): one pass of cluster/src/kmedoids.cc's while(1)
// loop on a condensed distance matrix that is already in HBM.  Every sum is taken in the reference's order by ONE lane
// (float64 addition does not associate, and every decision of the loop -- which member is the medoid, whether the total
// still falls -- compares such sums), so the results are the reference's bit for bit.
#pragma once
#include "common.h"

#include <cfloat>

namespace msm {

constexpr int KM_T = 256;          // threads per workgroup of every kernel here
constexpr int KM_TI = 64;          // cost kernel: elements (lanes of wave 0) per workgroup
constexpr int KM_TK = 64;          // cost kernel: columns of one LDS tile
constexpr int KM_LD = KM_TK + 1;   // padded LDS row, in doubles
constexpr int KM_SMALL_MAXN = 180; // small path: 180*179/2 doubles = 128,880 B of the 160 KiB one workgroup may hold
constexpr int KM_SMALL_MAXIT = 4096;   // iterations one small launch may run before it hands back to the host
constexpr long long KM_PERIOD_MAX = INT64_MAX / 2;

// Entry (i, j), i != j, of a condensed matrix of n elements (kmedoids.cc:60-69).  64-bit throughout: at n = 3,000,000
// the index passes 2^42.
__host__ __device__ inline long long km_condensed_index(long long i, long long j, long long n)
{
    const long long a = i < j ? i : j, b = i < j ? j : i;
    return n * a - a * (a + 1) / 2 + b - 1 - a;
}

// The loop's state between launches (device memory; the host reads only `rec`).
struct KmState {
    double total;        // the last iteration's total (DBL_MAX before the first)
    long long counter;   // iterations run
    long long period;    // the snapshot period (10, then doubled at every snapshot)
    long long snapshots;
};
// What the host reads once per iteration (general path) / per launch (small path).
struct KmRecord {
    double total;
    long long counter, snapshots;
    int stop;       // the pass has ended
    int bad;        // bit 0: a distance is not finite, or a cost or the total is not below DBL_MAX: the loop is undefined;
                    // bit 1: a negative distance (the costs' bit order is only their value order for sums >= +0)
};

struct KmArgs {
    const double* D;      // condensed matrix
    long long n, K;
    int* t;               // labels, n
    int* saved;           // the snapshot, n
    double* cost;         // n
    double* dist;         // n
    unsigned long long* best;   // K: bits of the lowest cost of a member
    int* med;             // K: the medoids
    KmState* st;
    KmRecord* rec;
    int* flag;            // [0]: a non-finite distance seen, [1]: a negative one
};

// ---- general path ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KM_T) void km_finite_kernel(const double* __restrict__ D, long long len, int* flag)
{
    bool bad = false, neg = false;
    for (long long p = (long long)blockIdx.x * KM_T + threadIdx.x; p < len; p += (long long)gridDim.x * KM_T) {
        const double x = D[p];
        bad |= !(fabs(x) <= DBL_MAX);
        neg |= x < 0.0;
    }
    if (bad) flag[0] = 1;
    if (neg) flag[1] = 1;
}

// Snapshot (when this iteration's counter is a multiple of the period) and reset of the per-cluster minima.
__global__ __launch_bounds__(KM_T) void km_begin_kernel(KmArgs P)
{
    const bool snap = P.st->counter % P.st->period == 0;
    const long long g = (long long)blockIdx.x * KM_T + threadIdx.x;
    if (g < P.n && snap) P.saved[g] = P.t[g];
    if (g < P.K) {
        P.best[g] = ~0ULL;
        P.med[g] = INT32_MAX;
    }
}

// cost[i] = sum over k ascending of (k != i && t[k] == t[i]) ? D(i, k) : +0.0 -- one lane of wave 0 per element, the same
// float64 additions in the same order as kmedoids.cc:298-303 (its early exit cannot change a sum that only grows; +0.0
// leaves every partial sum's bits alone).  All four waves stage the 64 x 64 tile of the matrix through LDS with
// coalesced loads: below the diagonal row k is contiguous in i (lanes along i), above it row i is contiguous in k (lanes
// along k).  The next tile's loads are in flight while wave 0 adds.
__global__ __launch_bounds__(KM_T) void km_cost_kernel(KmArgs P)
{
    __shared__ double tile[KM_TI * KM_LD];
    __shared__ int tk[KM_TK];
    constexpr int PER = KM_TI * KM_TK / KM_T;   // 16 entries per thread
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long n = P.n, i0 = (long long)blockIdx.x * KM_TI;
    const long long i = i0 + tid;   // (wave 0 only)
    const int mine = (tid < KM_TI && i < n) ? P.t[i] : -1;
    double v[PER];
    int lab = 0;
    double d = 0.0;

    auto load = [&](long long k0) {
        const bool below = k0 + KM_TK <= i0;   // every k of the tile is below every i of the block
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            // below: this wave's rows k = k0 + w*16 + r, lanes along i; otherwise rows i = i0 + w*16 + r, lanes along k
            const long long ii = below ? i0 + lane : i0 + w * PER + r;
            const long long kk = below ? k0 + w * PER + r : k0 + lane;
            double x = 0.0;
            if (ii < n && kk < n && ii != kk) x = P.D[km_condensed_index(ii, kk, n)];
            v[r] = x;
        }
        lab = (tid < KM_TK && k0 + tid < n) ? P.t[k0 + tid] : -2;
    };
    auto store = [&](long long k0) {
        const bool below = k0 + KM_TK <= i0;
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int ri = below ? lane : w * PER + r;
            const int rk = below ? w * PER + r : lane;
            tile[ri * KM_LD + rk] = v[r];
        }
        if (tid < KM_TK) tk[tid] = lab;
    };

    load(0);
    for (long long k0 = 0; k0 < n; k0 += KM_TK) {
        __syncthreads();   // wave 0 has finished with the previous tile
        store(k0);
        __syncthreads();
        if (k0 + KM_TK < n) load(k0 + KM_TK);
        if (tid < KM_TI) {
            const double* row = tile + tid * KM_LD;
#pragma unroll 8
            for (int kk = 0; kk < KM_TK; ++kk) {
                const bool same = (tk[kk] == mine) & (k0 + kk != i);
                d += same ? row[kk] : 0.0;
            }
        }
    }
    if (tid < KM_TI && i < n) {
        P.cost[i] = d;
        atomicMin(&P.best[mine], (unsigned long long)__double_as_longlong(d));   // d >= +0: bit order is value order
    }
}

// The lowest index among a cluster's members of lowest cost (kmedoids.cc:304-307: strict <, ascending i).
__global__ __launch_bounds__(KM_T) void km_select_kernel(KmArgs P)
{
    const long long i = (long long)blockIdx.x * KM_T + threadIdx.x;
    if (i >= P.n) return;
    const int c = P.t[i];
    if ((unsigned long long)__double_as_longlong(P.cost[i]) == P.best[c]) atomicMin(&P.med[c], (int)i);
}

// kmedoids.cc:207-227: the first cluster, in cluster order, at the strict minimum of D(i, medoid); a medoid gets its own
// cluster and distance 0 (and the scan ends there).
__device__ __forceinline__ void km_assign_one(const double* D, long long n, long long K, const int* med, long long i, int& label,
                                              double& dist)
{
    double best = DBL_MAX;
    for (long long c = 0; c < K; ++c) {
        const long long j = med[c];
        if (j < 0 || j >= n) continue;   // (no medoid: the finish step reports it; never an address)
        if (j == i) {
            best = 0.0;
            label = (int)c;
            break;
        }
        const double td = D[km_condensed_index(i, j, n)];
        if (td < best) {
            best = td;
            label = (int)c;
        }
    }
    dist = best;
}

__global__ __launch_bounds__(KM_T) void km_assign_kernel(KmArgs P)
{
    const long long i = (long long)blockIdx.x * KM_T + threadIdx.x;
    if (i >= P.n) return;
    int label = P.t[i];
    double dist;
    km_assign_one(P.D, P.n, P.K, P.med, i, label, dist);
    P.t[i] = label;
    P.dist[i] = dist;
}

// One workgroup: total = dist[0] + dist[1] + ... by one lane (kmedoids.cc:226), the comparison with the snapshot, the stop
// test (kmedoids.cc:228-234) and the record the host reads.
__global__ __launch_bounds__(KM_T) void km_finish_kernel(KmArgs P)
{
    __shared__ double ds[KM_T];
    __shared__ int differs, badcost;
    const int tid = threadIdx.x;
    if (tid == 0) differs = 0, badcost = 0;
    __syncthreads();
    int diff = 0, bad = 0;
    for (long long i = tid; i < P.n; i += KM_T) diff |= P.t[i] != P.saved[i];
    for (long long c = tid; c < P.K; c += KM_T) {
        const int j = P.med[c];
        bad |= j < 0 || j >= P.n || !(P.cost[(j < 0 || j >= P.n) ? 0 : j] < DBL_MAX);
    }
    if (diff) differs = 1;
    if (bad) badcost = 1;
    double total = 0.0;
    for (long long i0 = 0; i0 < P.n; i0 += KM_T) {
        __syncthreads();
        ds[tid] = i0 + tid < P.n ? P.dist[i0 + tid] : 0.0;
        __syncthreads();
        if (tid == 0) {
            const int cnt = (int)(P.n - i0 < KM_T ? P.n - i0 : KM_T);
            for (int r = 0; r < cnt; ++r) total += ds[r];
        }
    }
    __syncthreads();
    if (tid == 0) {
        KmState& S = *P.st;
        const double previous = S.total;
        if (S.counter % S.period == 0) {
            if (S.period < KM_PERIOD_MAX) S.period *= 2;
            S.snapshots += 1;
        }
        S.counter += 1;
        S.total = total;
        KmRecord R;
        R.total = total;
        R.counter = S.counter;
        R.snapshots = S.snapshots;
        R.bad = (badcost || !(total < DBL_MAX) || P.flag[0]) ? 1 : 0;   // (negative entries were refused before the loop)
        R.stop = total >= previous || !differs || R.bad;
        *P.rec = R;
    }
}

// ---- small path ------------------------------------------------------------------------------------------------------
// The whole pass on one workgroup: matrix, labels, snapshot, costs and medoids live in LDS (n <= KM_SMALL_MAXN), so an
// iteration costs a few barriers instead of five launches and a synchronisation.  The loop is bounded: after
// KM_SMALL_MAXIT iterations the state goes back to global memory and the host launches again.
__global__ __launch_bounds__(KM_T) void km_small_kernel(KmArgs P)
{
    constexpr int NMAX = KM_SMALL_MAXN;
    __shared__ double Ds[NMAX * (NMAX - 1) / 2];
    __shared__ double cost[NMAX], dist[NMAX];
    __shared__ int t[NMAX], saved[NMAX], med[NMAX];
    __shared__ double s_total;
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int n = (int)P.n, K = (int)P.K;
    const int len = n * (n - 1) / 2;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool nonfinite = false, negative = false;
    for (int p = tid; p < len; p += KM_T) {
        const double x = P.D[p];
        nonfinite |= !(fabs(x) <= DBL_MAX);
        negative |= x < 0.0;
        Ds[p] = x;
    }
    if (nonfinite) atomicOr(&s_bad, 1);
    if (negative) atomicOr(&s_bad, 2);
    if (tid < n) {
        t[tid] = P.t[tid];
        saved[tid] = P.saved[tid];
    }
    double total = P.st->total;
    long long counter = P.st->counter, period = P.st->period, snapshots = P.st->snapshots;
    int stop = 0;
    __syncthreads();
    int bad = s_bad;
    if (bad) stop = 1;
    for (int it = 0; it < KM_SMALL_MAXIT && !stop; ++it) {
        const double previous = total;
        if (counter % period == 0) {
            if (tid < n) saved[tid] = t[tid];
            if (period < KM_PERIOD_MAX) period *= 2;
            ++snapshots;
        }
        ++counter;
        // costs, in ascending k
        if (tid < n) {
            const int mine = t[tid];
            double d = 0.0;
            for (int k = 0; k < n; ++k) {
                double x = 0.0;
                if ((t[k] == mine) & (k != tid)) x = Ds[km_condensed_index(tid, k, n)];
                d += x;
            }
            cost[tid] = d;
        }
        __syncthreads();
        // medoids: cluster c's thread walks the elements in order (errors[c] starts at DBL_MAX, strict <)
        if (tid < K) {
            double e = DBL_MAX;
            int j = -1;
            for (int i = 0; i < n; ++i)
                if (t[i] == tid && cost[i] < e) {
                    e = cost[i];
                    j = i;
                }
            med[tid] = j;
            if (j < 0) atomicOr(&s_bad, 1);
        }
        __syncthreads();
        bad = s_bad;
        if (bad) {
            stop = 1;
            break;
        }
        int diff = 0;
        if (tid < n) {
            int label = t[tid];
            double dd;
            km_assign_one(Ds, n, K, med, tid, label, dd);
            dist[tid] = dd;
            t[tid] = label;   // (the scan reads med and Ds only)
            diff = label != saved[tid];
        }
        const int differs = __syncthreads_or(diff);
        if (tid == 0) {
            double s = 0.0;
            for (int i = 0; i < n; ++i) s += dist[i];
            s_total = s;
        }
        __syncthreads();
        total = s_total;
        if (!(total < DBL_MAX)) bad |= 1;
        stop = total >= previous || !differs || bad;
    }
    __syncthreads();
    if (tid < n) {
        P.t[tid] = t[tid];
        P.saved[tid] = saved[tid];
    }
    if (tid < K) P.med[tid] = med[tid];
    if (tid == 0) {
        KmState& S = *P.st;
        S.total = total;
        S.counter = counter;
        S.period = period;
        S.snapshots = snapshots;
        KmRecord R;
        R.total = total;
        R.counter = counter;
        R.snapshots = snapshots;
        R.stop = stop;
        R.bad = bad;
        *P.rec = R;
    }
}

}  // namespace msm
