// kmeans_update_dev.h -- everything of a k-means call that is not labelling (included by kmeans.hip): the inertia kernel
// (which also merges a split launch's candidates), the centre update with the device-side convergence bookkeeping of
// msm_mbk_run, and the small gather / reduce / norm / finish / apply / reassign kernels.
#pragma once
#include "kmeans_common_dev.h"

#include <algorithm>

namespace msm {

// per-row ||x - c_label||^2 (fp32 difference, fp64 accumulate), one wave per row;
// per-block fp64 partial sums for the inertia.
// nsplit > 1 (centre-split labelling of a small batch): the row's label is first picked from the splits' candidates
// (lowest value, then lowest index -- what kmeans_label_reduce_kernel does as a launch of its own) and written out.
// Two rows per wave in flight and 16-byte loads when the rows allow it (m % 4 == 0, 16-byte aligned bases) -- one row
// at a time with 4-byte loads and three dependent round trips per row (candidates -> centre row -> sum) ran at 1.7 TB/s
// (1.5 ms per 1.25M x 512 pass beside a 10.4 ms labelling kernel; profiles/r05_label_wide.txt).
template <typename T>
__global__ __launch_bounds__(KNT) void kmeans_inertia_kernel(KmArgsT<T> P, double* __restrict__ partial, int nsplit)
{
    if (P.stop && *P.stop) return;  // uniform
    __shared__ double red[KNT / 64];
    constexpr int E = 16 / (int)sizeof(T);   // elements of a 16-byte load: 4 floats / 2 doubles
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool vec4 = (P.m % E) == 0 && ((((uintptr_t)P.X) | ((uintptr_t)P.C)) & 15) == 0;
    const long long m4 = P.m / E;
    // the row's label: from the splits' candidates (lane q fetches split q's: one round trip, then a butterfly for the lowest
    // (value, index)) or as the labelling kernel wrote it
    auto cand_load = [&](long long i, T& bv, int& bi) {
        bv = (T)INFINITY;
        bi = 0x7fffffff;
        if (nsplit > 1) {
            for (int q0 = 0; q0 < nsplit; q0 += 64) {
                const int q = q0 + lane;
                const int qc = q < nsplit ? q : nsplit - 1;
                const T v = P.pv[(long long)qc * P.n + i];
                const int ix = P.pi[(long long)qc * P.n + i];
                if (q < nsplit && (v < bv || (v == bv && ix < bi))) {
                    bv = v;
                    bi = ix;
                }
            }
        } else {
            bi = P.labels[i];
        }
    };
    auto cand_finish = [&](long long i, bool live, T bv, int bi) -> int {
        if (nsplit <= 1) return bi;
#pragma unroll
        for (int msk = 32; msk > 0; msk >>= 1) {
            const T ov = __shfl_xor(bv, msk, 64);
            const int oi = __shfl_xor(bi, msk, 64);
            if (ov < bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (bi == 0x7fffffff) bi = 0;  // all-NaN row: sklearn's argmin returns 0
        if (live && lane == 0) P.labels[i] = bi;
        return bi;
    };
    // (float rows: the difference in fp32, its square and the sum in fp64; double rows: all of it in fp64 -- scikit-learn's
    //  _euclidean_dense_dense works in the rows' own type)
    auto row_sum = [&](const T* x, const T* c) -> double {
        double s = 0.0;
        if (vec4) {
            struct alignas(16) V { T e[E]; };
            const V* x4 = reinterpret_cast<const V*>(x);
            const V* c4 = reinterpret_cast<const V*>(c);
            for (long long k = lane; k < m4; k += 64) {
                const V a = x4[k], b = c4[k];
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const T d = a.e[e] - b.e[e];
                    s += (double)d * (double)d;
                }
            }
        } else {
            for (long long k = lane; k < P.m; k += 64) {
                const T d = x[k] - c[k];
                s += (double)d * (double)d;
            }
        }
        return s;
    };
    double tot = 0.0;
    const long long stride = (long long)gridDim.x * 4;
    for (long long i0 = (long long)blockIdx.x * 4 + wave; i0 < P.n; i0 += 2 * stride) {
        const long long i1 = i0 + stride;
        const bool has1 = i1 < P.n;
        const long long i1c = has1 ? i1 : i0;
        T v0, v1;
        int b0, b1;
        cand_load(i0, v0, b0);
        cand_load(i1c, v1, b1);
        const int lab0 = cand_finish(i0, true, v0, b0), lab1 = cand_finish(i1c, has1, v1, b1);
        const long long r0 = P.rows ? P.rows[i0] : i0, r1 = P.rows ? P.rows[i1c] : i1c;
        double s0 = row_sum(P.X + r0 * P.m, P.C + (long long)lab0 * P.m);
        double s1 = row_sum(P.X + r1 * P.m, P.C + (long long)lab1 * P.m);
        if (!has1) s1 = 0.0;
#pragma unroll
        for (int msk = 32; msk > 0; msk >>= 1) {
            s0 += __shfl_xor(s0, msk, 64);
            s1 += __shfl_xor(s1, msk, 64);
        }
        tot += s0;
        tot += s1;
    }
    if (lane == 0) red[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// msm_mbk_run: end of one queued step.  Sums the inertia partials, then plays sklearn's _mini_batch_convergence
// (_kmeans.py:1963-2027, tol = 0 and verbose = 0 branch) in float64 on the device so that the host does not have to
// look at every step: st = {ewa, ewa_min, no_improvement, have_ewa, have_min, steps_done}.  Plain IEEE operations in
// the host's order: contraction is switched off for the function by pragma (HIP's __dmul_rn / __dadd_rn are plain `*` and
// `+` once inlined, and the compiler fused ewa * (1 - alpha) + bi * alpha into one fma: an ulp or two off scikit-learn's
// moving average, enough to decide `ewa < ewa_min` the other way on a tie).  Executed by the LAST workgroup of mbk_update_kernel to
// finish (an arrival counter), not by a launch of its own: between dependent launches the GPU idles for ~10-15 us,
// which at 85 us of work per step is what a launch costs.
struct MbkConv {
    const double* partial;  // inertia partials of the step
    int nb;
    double* st;             // nullptr: no convergence bookkeeping (plain msm_mbk_step)
    int* stop;
    double* inertias;
    unsigned* done;         // arrival counter, zero between launches
    long long step_index;
    double batch_size, alpha;
    long long max_no_improvement;
};

__device__ __forceinline__ void mbk_converge(const MbkConv& cv, double* red)
{
#pragma clang fp contract(off)
    double s = 0.0;
    for (int i = threadIdx.x; i < cv.nb; i += KNT) s += cv.partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = KNT / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    double* st = cv.st;
    const double inertia = red[0];
    cv.inertias[(long long)st[5]] = inertia;
    st[5] += 1.0;
    if (cv.step_index == 0) return;  // "ignore first iteration because it's inertia from initialization"
    const double bi = inertia / cv.batch_size;
    double ewa;
    if (st[3] == 0.0) {
        ewa = bi;
        st[3] = 1.0;
    } else {
        ewa = st[0] * (1.0 - cv.alpha) + bi * cv.alpha;
    }
    st[0] = ewa;
    if (st[4] == 0.0 || ewa < st[1]) {
        st[2] = 0.0;
        st[1] = ewa;
        st[4] = 1.0;
    } else {
        st[2] += 1.0;
    }
    if (cv.max_no_improvement >= 0 && st[2] >= (double)cv.max_no_improvement) *cv.stop = 1;
}

// One workgroup per centre: find the centre's members in the batch (ordered compaction by the whole workgroup:
// wave ballots + a 4-entry prefix; the first version let thread 0 walk the labels alone, 183 us per step at
// K = 1000, B = 1024), visit them in batch order.
// apply != 0: sklearn's streaming-mean update in fp32, in place on centers/counts, and the centre's new ||c||^2
//             (same lane partition and butterfly as kmeans_cnorm_kernel: bit-identical to a separate launch).
// sums/cnts (nullable): fp64 batch sums and counts for the multi-GPU all-reduce.
template <typename T>   // T: the rows' type = the type scikit-learn updates in (acc32 / w_old / alpha are "floating" there)
__global__ __launch_bounds__(KNT) void mbk_update_kernel(KmArgsT<T> P, T* __restrict__ centers,
                                                         T* __restrict__ counts, T* __restrict__ cnorm,
                                                         double* __restrict__ sums,
                                                         double* __restrict__ cnts, int apply, MbkConv cv)
{
    if (P.stop && *P.stop) return;
    extern __shared__ int members[];  // compacted member positions of one chunk
    __shared__ int wcnt[KNT / 64];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int CH = 4096;
    const T w_old = counts[j];
    long long total = 0;
    for (long long f0 = 0; f0 < P.m; f0 += KNT) {
        const long long f = f0 + tid;
        T acc32 = (f < P.m) ? centers[(long long)j * P.m + f] * w_old : (T)0;
        double acc64 = 0.0;
        long long cnt = 0;
        for (long long b0 = 0; b0 < P.n; b0 += CH) {
            const long long be = std::min<long long>(P.n, b0 + CH);
            int nmem = 0;
            for (long long sb = b0; sb < be; sb += KNT) {
                const long long pos = sb + tid;
                const bool mine = pos < be && P.labels[pos] == j;
                const unsigned long long bal = __ballot(mine);
                __syncthreads();  // wcnt / members of the previous round are consumed
                if (lane == 0) wcnt[wave] = __popcll(bal);
                __syncthreads();
                int base = nmem;
                for (int w = 0; w < wave; ++w) base += wcnt[w];
                if (mine) members[base + __popcll(bal & ((1ull << lane) - 1ull))] = (int)(pos - b0);
                nmem += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            }
            __syncthreads();
            cnt += nmem;
            if (f < P.m) {
                for (int k = 0; k < nmem; ++k) {
                    const long long b = b0 + members[k];
                    const long long r = P.rows ? P.rows[b] : b;
                    const T x = P.X[r * P.m + f];
                    acc32 += x;
                    acc64 += (double)x;
                }
            }
        }
        total = cnt;
        if (f < P.m) {
            if (sums) sums[(long long)j * P.m + f] = acc64;
            if (apply && cnt > 0) {
                const T w_new = w_old + (T)cnt;
                const T alpha = (T)1 / w_new;
                centers[(long long)j * P.m + f] = acc32 * alpha;
            }
        }
    }
    __syncthreads();  // the centre row is complete (workgroup-scope visibility)
    if (tid == 0) {
        if (cnts) cnts[j] = (double)total;
        if (apply && total > 0) counts[j] = w_old + (T)total;
    }
    if (apply && cnorm && total > 0 && wave == 0) {
        const volatile T* c = centers + (long long)j * P.m;
        T sq = 0;
        for (long long f = lane; f < P.m; f += 64) {
            const T v = c[f];
            sq += v * v;
        }
#pragma unroll
        for (int msk = 32; msk > 0; msk >>= 1) sq += __shfl_xor(sq, msk, 64);
        if (lane == 0) cnorm[j] = sq;
    }
    if (cv.st) {  // uniform: the last workgroup to arrive closes the step
        __shared__ int is_last;
        __shared__ double cred[KNT];
        __syncthreads();
        if (tid == 0) is_last = (atomicAdd(cv.done, 1u) == gridDim.x - 1) ? 1 : 0;
        __syncthreads();
        if (is_last) {
            mbk_converge(cv, cred);
            if (tid == 0) *cv.done = 0u;
        }
    }
}

// Mini-batch rows copied once into a compact [rows][m] buffer: the batch's rows are scattered over the whole data set (one
// page each for wide rows), and the label, inertia and update kernels of a step each paid those address translations again
// -- ~35 us per kernel at 1.25M x 512 whatever the arithmetic.  One wave per row, 16-byte lanes when the row allows.
template <typename T>
__global__ __launch_bounds__(KNT) void mbk_gather_kernel(const T* __restrict__ X, const msm_idx_t* __restrict__ rows,
                                                         long long nrows, long long m, T* __restrict__ out)
{
    constexpr int E = 16 / (int)sizeof(T);
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nrows) return;
    const T* src = X + rows[i] * m;
    T* dst = out + i * m;
    if ((m % E) == 0 && ((((uintptr_t)X) | ((uintptr_t)out)) & 15) == 0) {
        for (long long f = lane * (long long)E; f < m; f += 64 * E) *reinterpret_cast<float4*>(dst + f) = *reinterpret_cast<const float4*>(src + f);
    } else {
        for (long long f = lane; f < m; f += 64) dst[f] = src[f];
    }
}

// finish a centre-split labelling: lowest (value, index) over the splits
template <typename T>
__global__ void kmeans_label_reduce_kernel(const T* __restrict__ pv, const int* __restrict__ pi, long long n,
                                           int nsplit, int32_t* __restrict__ labels, const int* __restrict__ stop)
{
    if (stop && *stop) return;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    T bv = pv[i];
    int bi = pi[i];
    for (int s = 1; s < nsplit; ++s) {
        const T v = pv[(long long)s * n + i];
        const int ix = pi[(long long)s * n + i];
        if (v < bv || (v == bv && ix < bi)) {
            bv = v;
            bi = ix;
        }
    }
    labels[i] = (bi == 0x7fffffff) ? 0 : bi;
}

// ||c_j||^2 in the centres' own type, one wave per centre
template <typename T>
__global__ __launch_bounds__(KNT) void kmeans_cnorm_kernel(const T* __restrict__ C, long long K, long long m,
                                                           T* __restrict__ cnorm)
{
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= K) return;
    T s = 0;
    for (long long f = lane; f < m; f += 64) s += C[j * m + f] * C[j * m + f];
#pragma unroll
    for (int msk = 32; msk > 0; msk >>= 1) s += __shfl_xor(s, msk, 64);
    if (lane == 0) cnorm[j] = s;
}

// [inertia (double) | counts (K values of the rows' type)] gathered into one small buffer for a single D2H per step
template <typename T>
__global__ __launch_bounds__(KNT) void mbk_finish_kernel(const double* __restrict__ partial, int nb,
                                                         const T* __restrict__ counts, long long K,
                                                         double* __restrict__ out_inertia, T* __restrict__ out_counts)
{
    __shared__ double red[KNT];
    double s = 0.0;
    for (int i = threadIdx.x; i < nb; i += KNT) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = KNT / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out_inertia = red[0];
    for (long long j = threadIdx.x; j < K; j += KNT) out_counts[j] = counts[j];
}

// centres (+counts) <- (centres * w + batch sums) / (w + n) from all-reduced fp64 sums (multi-GPU)
template <typename T>
__global__ void mbk_apply_kernel(T* __restrict__ centers, T* __restrict__ counts,
                                 const double* __restrict__ packed, long long K, long long m, const int* __restrict__ stop = nullptr)
{
    if (stop && *stop) return;   // a queued run that has converged: the remaining steps are no-ops on every rank
    const long long j = blockIdx.x;
    const double n = packed[K * m + j];
    if (n <= 0.0) return;
    const T w_old = counts[j];
    const T w_new = (T)((double)w_old + n);
    for (long long f = threadIdx.x; f < m; f += blockDim.x)
        centers[j * m + f] = (T)(((double)centers[j * m + f] * (double)w_old + packed[j * m + f]) / (double)w_new);
    __syncthreads();
    if (threadIdx.x == 0) counts[j] = w_new;
}

// sharded run: the convergence bookkeeping of a step on the ALL-REDUCED batch inertia (cv.partial points at it, nb = 1)
__global__ __launch_bounds__(KNT) void mbk_conv_kernel(MbkConv cv)
{
    __shared__ double red[KNT];
    if (*cv.stop) return;
    mbk_converge(cv, red);
}

template <typename T>
__global__ void mbk_reassign_kernel(T* __restrict__ centers, T* __restrict__ counts,
                                    const T* __restrict__ X, long long m, const msm_idx_t* __restrict__ rows,
                                    const msm_idx_t* __restrict__ which, T new_count)
{
    const msm_idx_t r = rows[blockIdx.x], j = which[blockIdx.x];
    for (long long f = threadIdx.x; f < m; f += blockDim.x) centers[j * m + f] = X[r * m + f];
    if (threadIdx.x == 0) counts[j] = new_count;
}

}  // namespace msm
