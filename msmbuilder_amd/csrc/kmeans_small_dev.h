// kmeans_small_dev.h -- the two-launch small-batch step of MiniBatchKMeans (included by kmeans.hip).
#pragma once
#include "kmeans_label_dev.h"
#include "kmeans_update_dev.h"

namespace msm {

// ---------------------------------------------------------------------------
// Small-batch step (MiniBatchKMeans' inner loop: B ~ 1000 rows, m <= 32 features, K ~ 1000 centres).  A step is
// ~10^7 multiply-adds: the three general kernels above spent 26 + 7 + 38 us on it, all of it latency (MFMA tiles that
// are 70% padding, a 160-shuffle argmin, a 1000-label scan with 8 barriers in each of K workgroups) plus ~20 us of
// dependent-launch gaps.  Two launches instead:
//  * mbk_small_label_kernel: lane = row (64 rows per workgroup), the centres split over blockIdx.y and then over the 4
//    waves, the split's centres in LDS read as broadcast 16-byte fragments, v = ||c||^2 - 2 x.c in fp32 (the same
//    quantity the MFMA kernel minimises; sequential fma over the features).  The LAST workgroup of a row block to arrive
//    (an agent-scope counter) reduces the splits' candidates (lowest value, then lowest index), writes the labels and
//    the block's fp64 inertia partial (one wave per row, lanes over features, butterfly -- as kmeans_inertia_kernel).
//  * mbk_small_update_kernel: one WAVE per centre; the batch's labels (and row indices) are fetched with 16 + 16
//    independent loads per lane, members found by ballot, their rows read through v_readlane'd indices up to 8 loads in
//    flight, added in batch order (sklearn's order, _k_means_minibatch.pyx) by lane f < m.
// ---------------------------------------------------------------------------
constexpr int SBC = 128;  // centres per split (LDS slice)

struct SmallArgs {
    unsigned* arrive;          // [row blocks], zero between launches
    unsigned long long* cand;  // [rows] (value, index) candidates, all-ones between launches
    double* partial;           // [row blocks] inertia partials
    int ns, cper;              // centre splits, centres per split
};

// (value, index) -> one unsigned word whose order is (value ascending, index ascending); -0 counts as +0
__device__ __forceinline__ unsigned long long mbk_key(float v, int idx)
{
    unsigned u = __float_as_uint(v + 0.f);
    u ^= (u & 0x80000000u) ? 0xffffffffu : 0x80000000u;
    return ((unsigned long long)u << 32) | (unsigned)idx;
}

template <int G>  // feature groups of 4: m <= 4 G
__global__ __launch_bounds__(KNT) void mbk_small_label_kernel(KmArgs P, SmallArgs S)
{
    if (P.stop && *P.stop) return;  // uniform
    constexpr int MP = 4 * G;
    __shared__ __attribute__((aligned(16))) float Cs[SBC * MP];
    __shared__ float cn[SBC];
    __shared__ float wv[4][64];
    __shared__ int wi[4][64];
    __shared__ int is_last;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long rb = blockIdx.x;
    const int sp = blockIdx.y;
    const int m = (int)P.m;
    const long long i = rb * 64 + lane;
    const long long ic = i < P.n ? i : P.n - 1;
    const long long r = P.rows ? P.rows[ic] : ic;
    float x[MP];  // unconditional loads at clamped columns, masked afterwards (a load under a select is waited for at once)
#pragma unroll
    for (int f = 0; f < MP; ++f) x[f] = P.X[r * P.m + (f < m ? f : m - 1)];
#pragma unroll
    for (int f = 0; f < MP; ++f)
        if (f >= m) x[f] = 0.f;
    const long long j0 = (long long)sp * S.cper;
    const int nc = (int)(P.K - j0 < S.cper ? P.K - j0 : S.cper);
    for (int e = tid; e < nc * MP; e += KNT) {
        const int c = e / MP, f = e - c * MP;
        Cs[e] = f < m ? P.C[(j0 + c) * P.m + f] : 0.f;
    }
    for (int c = tid; c < nc; c += KNT) cn[c] = P.cnorm[j0 + c];
    __syncthreads();
    const int per = (nc + 3) / 4;
    const int c0 = wave * per, c1 = (c0 + per < nc) ? c0 + per : nc;
    float best = INFINITY;
    int bidx = 0x7fffffff;
    for (int c = c0; c < c1; ++c) {
        const float4* cp = reinterpret_cast<const float4*>(Cs + c * MP);
        float dot = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float4 q = cp[g];
            dot = fmaf(x[4 * g + 0], q.x, dot);
            dot = fmaf(x[4 * g + 1], q.y, dot);
            dot = fmaf(x[4 * g + 2], q.z, dot);
            dot = fmaf(x[4 * g + 3], q.w, dot);
        }
        const float v = cn[c] - 2.f * dot;
        if (v < best) {  // ascending index, strict
            best = v;
            bidx = (int)(j0 + c);
        }
    }
    wv[wave][lane] = best;
    wi[wave][lane] = bidx;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float ov = wv[w][lane];
            const int oi = wi[w][lane];
            if (ov < best || (ov == best && oi < bidx)) {
                best = ov;
                bidx = oi;
            }
        }
        // The splits' candidates meet in ONE 64-bit word per row: (order-preserving image of the value, index), reduced
        // by an agent-scope atomic min -- lowest value, then lowest index.  Candidates cross workgroups and XCDs (whose
        // L2s are not coherent) inside one launch; agent-scope atomics are performed at the memory side.  (Device-wide
        // fences instead -- an L2 write-back + invalidate per workgroup -- made this kernel 50 us; per-split candidate
        // arrays read back by the last workgroup with 2 x 32 dependent coherent loads per row, 30 us.)
        if (i < P.n) __hip_atomic_fetch_min(S.cand + i, mbk_key(best, bidx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // arrival: the workgroup's candidate atomics -> workgroup barrier -> agent-scope RELEASE fence (one lane) -> ticket;
    // the last arriver takes an agent-scope ACQUIRE fence before the barrier that lets its wave read the candidates
    // (a ticket published behind a workgroup-scope fence is not enough)
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        is_last = (__hip_atomic_fetch_add(&S.arrive[rb], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(S.ns - 1)) ? 1 : 0;
        if (is_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    if (!is_last || wave != 0) return;
    // last workgroup of the row block, one wave: labels, and the block's inertia (lane = row, x still in registers;
    // fp32 difference, exact fp64 squares added in feature order, then a butterfly over the 64 rows)
    int lab = 0;
    double sq = 0.0;
    if (i < P.n) {
        const unsigned long long key = __hip_atomic_load(S.cand + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(S.cand + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next step
        lab = (int)(unsigned)(key & 0xffffffffull);
        if (lab == 0x7fffffff) lab = 0;  // all-NaN row: sklearn's argmin returns 0
        P.labels[i] = lab;
        const float* c = P.C + (long long)lab * P.m;
#pragma unroll
        for (int f = 0; f < MP; ++f)
            if (f < m) {
                const float d = x[f] - c[f];
                sq += (double)d * (double)d;
            }
    }
#pragma unroll
    for (int msk = 32; msk > 0; msk >>= 1) sq += __shfl_xor(sq, msk, 64);
    if (lane == 0) {
        S.partial[rb] = sq;
        __hip_atomic_store(&S.arrive[rb], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

constexpr int MSU_CAP = 1024;  // batch rows at most (a wave's member list in LDS)

template <typename T>
__global__ __launch_bounds__(KNT) void mbk_small_update_kernel(KmArgsT<T> P, T* __restrict__ centers,
                                                               T* __restrict__ counts, T* __restrict__ cnorm,
                                                               double* __restrict__ sums, double* __restrict__ cnts,
                                                               int apply, MbkConv cv)
{
    if (P.stop && *P.stop) return;
    __shared__ long long mrow[4][MSU_CAP];  // per wave: the centre's member rows in batch order
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long j = (long long)blockIdx.x * 4 + wave;
    if (j < P.K) {  // uniform over the wave
        constexpr int NCH = 8;  // 64-feature blocks per round (lane = feature of each block)
        const T w_old = counts[j];
        T c_first[NCH];  // the first round's centre values: requested before the label scan, not after it
        // (all loads of this kernel are unconditional at clamped addresses and masked afterwards: a load under a select
        //  is waited for on the spot, which turns every batch of independent loads into a chain of round trips)
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const long long f = (long long)c * 64 + lane;
            c_first[c] = centers[j * P.m + (f < P.m ? f : P.m - 1)];
        }
        // members: 16 + 16 independent loads per lane, then ballots; rows through v_readlane
        int cnt = 0;
        {
            int lab[16];
            long long rowv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long pos = (long long)r * 64 + lane;
                const long long pc = pos < P.n ? pos : P.n - 1;
                lab[r] = P.labels[pc];
                rowv[r] = P.rows ? P.rows[pc] : pc;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool in = (long long)r * 64 + lane < P.n;
                unsigned long long bal = __ballot(in && lab[r] == (int)j);
                const int rlo = (int)(rowv[r] & 0xffffffffLL), rhi = (int)(rowv[r] >> 32);
                while (bal) {  // uniform
                    const int k = __builtin_ctzll(bal);
                    bal &= bal - 1ull;
                    const long long row = ((long long)__builtin_amdgcn_readlane(rhi, k) << 32) |
                                          (unsigned)__builtin_amdgcn_readlane(rlo, k);
                    if (lane == 0) mrow[wave][cnt] = row;
                    ++cnt;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        T sqn = 0;  // ||c_new||^2, lane partition of kmeans_cnorm_kernel
        for (long long f0 = 0; f0 < P.m; f0 += NCH * 64) {
            bool fl[NCH];
            T c_old[NCH], acc32[NCH];
            double acc64[NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const long long f = f0 + c * 64 + lane;
                fl[c] = f < P.m;
                c_old[c] = f0 == 0 ? c_first[c] : centers[j * P.m + (fl[c] ? f : P.m - 1)];
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                if (!fl[c]) c_old[c] = 0;
                acc32[c] = c_old[c] * w_old;
                acc64[c] = 0.0;
            }
            for (int q0 = 0; q0 < cnt; q0 += 4) {  // up to 4 x NCH row loads in flight
                T xv[4][NCH];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const long long row = mrow[wave][q0 + t < cnt ? q0 + t : cnt - 1];
#pragma unroll
                    for (int c = 0; c < NCH; ++c) {
                        const long long f = f0 + c * 64 + lane;
                        xv[t][c] = P.X[row * P.m + (f < P.m ? f : P.m - 1)];
                    }
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (q0 + t < cnt) {
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            const T xq = fl[c] ? xv[t][c] : (T)0;
                            acc32[c] += xq;
                            acc64[c] += (double)xq;
                        }
                    }
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const long long f = f0 + c * 64 + lane;
                T c_new = c_old[c];
                if (apply && cnt > 0) {
                    const T w_new = w_old + (T)cnt;
                    const T alpha = (T)1 / w_new;
                    c_new = acc32[c] * alpha;
                }
                if (fl[c]) {
                    if (sums) sums[j * P.m + f] = acc64[c];
                    if (apply && cnt > 0) centers[j * P.m + f] = c_new;
                    sqn += c_new * c_new;
                }
            }
        }
        if (lane == 0) {
            if (cnts) cnts[j] = (double)cnt;
            if (apply && cnt > 0) counts[j] = w_old + (T)cnt;
        }
        if (apply && cnorm && cnt > 0) {  // same lane partition and butterfly as kmeans_cnorm_kernel
#pragma unroll
            for (int msk = 32; msk > 0; msk >>= 1) sqn += __shfl_xor(sqn, msk, 64);
            if (lane == 0) cnorm[j] = sqn;
        }
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

}  // namespace msm
