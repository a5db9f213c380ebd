// kmeans_label_dev.h -- the three float32 labelling kernels on v_mfma_f32_32x32x2_f32 and their helpers (included by
// kmeans.hip): kmeans_label_kernel (any row pitch), kmeans_label64_kernel (small batches of wide rows, 64 x 64 tiles),
// kmeans_label_v4_kernel (16-byte rows).  Which shape launches which: km_plan in kmeans.hip.
#pragma once
#include "kmeans_common_dev.h"

namespace msm {

constexpr int KR = 128;   // rows per workgroup
constexpr int KCT = 128;  // centres per tile
constexpr int KBK = 32;   // features per K-step
constexpr int KP = KBK + 1;

typedef float f32x16 __attribute__((ext_vector_type(16)));

using KmArgs = KmArgsT<float>;

__device__ __forceinline__ void km_load(float4 (&xa)[4], float4 (&ca)[4], const KmArgs& P,
                                        long long row0, long long j0, int k0, int tid)
{
    const int c4 = (tid & 7) * 4;
    const int r0 = tid >> 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int rr = r0 + 32 * j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), w = v;
        const long long i = row0 + rr;
        if (i < P.n) {
            const long long r = P.rows ? P.rows[i] : i;
            const float* p = P.X + r * P.m + k0 + c4;
            if (k0 + c4 + 3 < P.m && ((P.m & 3) == 0)) {
                v = *reinterpret_cast<const float4*>(p);
            } else {
                if (k0 + c4 + 0 < P.m) v.x = p[0];
                if (k0 + c4 + 1 < P.m) v.y = p[1];
                if (k0 + c4 + 2 < P.m) v.z = p[2];
                if (k0 + c4 + 3 < P.m) v.w = p[3];
            }
        }
        const long long jc = j0 + rr;
        if (jc < P.K) {
            const float* p = P.C + jc * P.m + k0 + c4;
            if (k0 + c4 + 3 < P.m && ((P.m & 3) == 0)) {
                w = *reinterpret_cast<const float4*>(p);
            } else {
                if (k0 + c4 + 0 < P.m) w.x = p[0];
                if (k0 + c4 + 1 < P.m) w.y = p[1];
                if (k0 + c4 + 2 < P.m) w.z = p[2];
                if (k0 + c4 + 3 < P.m) w.w = p[3];
            }
        }
        xa[j] = v;
        ca[j] = w;
    }
}

__device__ __forceinline__ void km_store(const float4 (&xa)[4], const float4 (&ca)[4], float* Xs,
                                         float* Cs, int tid)
{
    const int c4 = (tid & 7) * 4;
    const int r0 = tid >> 3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float* px = Xs + (r0 + 32 * j) * KP + c4;
        float* pc = Cs + (r0 + 32 * j) * KP + c4;
        px[0] = xa[j].x; px[1] = xa[j].y; px[2] = xa[j].z; px[3] = xa[j].w;
        pc[0] = ca[j].x; pc[1] = ca[j].y; pc[2] = ca[j].z; pc[3] = ca[j].w;
    }
}

// running argmin over one finished centre tile (ascending j per lane, strict <); clears acc
__device__ __forceinline__ void km4_argmin(f32x16 (&acc)[2][2], float (&best)[2][16], int (&bidx)[2][16],
                                           const KmArgs& P, long long j0, int wc, int cl)
{
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
        const long long j = j0 + wc * 64 + bj * 32 + cl;
        if (j < P.K) {
            const float cn = P.cnorm[j];
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = cn - 2.f * acc[bi][bj][r];
                    if (v < best[bi][r]) {
                        best[bi][r] = v;
                        bidx[bi][r] = (int)j;
                    }
                }
        }
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.f;
    }
}

// wavefront min-reduction over the 32 lanes that share a row (value, lowest index), then the two
// centre halves; writes labels (or the split launch's candidates)
__device__ __forceinline__ void km_finish_rows(const float (&best)[2][16], const int (&bidx)[2][16], const KmArgs& P,
                                               float* redv, int* redi, long long row0, int tid, int wr, int wc,
                                               int kl, int cl, int split)
{
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = best[bi][r];
            int ix = bidx[bi][r];
#pragma unroll
            for (int msk = 1; msk < 32; msk <<= 1) {
                const float ov = __shfl_xor(v, msk, 64);
                const int oi = __shfl_xor(ix, msk, 64);
                if (ov < v || (ov == v && oi < ix)) {
                    v = ov;
                    ix = oi;
                }
            }
            if (cl == 0) {
                const int row = wr * 64 + bi * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
                redv[wc * KR + row] = v;
                redi[wc * KR + row] = ix;
            }
        }
    __syncthreads();
    if (tid < KR) {
        const long long i = row0 + tid;
        if (i < P.n) km_write_row<float>(P, i, redv[tid], redv[KR + tid], redi[tid], redi[KR + tid], split);
    }
}

__global__ __launch_bounds__(KNT, 2) void kmeans_label_kernel(KmArgs P)
{
    if (P.stop && *P.stop) return;  // uniform
    __shared__ float Xs[2][KR * KP];
    __shared__ float Cs[2][KCT * KP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, kl = lane >> 5, cl = lane & 31;
    const long long row0 = (long long)blockIdx.x * KR;
    const int nk = (int)((P.m + KBK - 1) / KBK);

    float best[2][16];
    int bidx[2][16];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            best[bi][r] = INFINITY;
            bidx[bi][r] = 0x7fffffff;
        }

    const long long jbeg = P.jspan ? (long long)blockIdx.y * P.jspan : 0;
    const long long jend = P.jspan ? (jbeg + P.jspan < P.K ? jbeg + P.jspan : P.K) : P.K;
    for (long long j0 = jbeg; j0 < jend; j0 += KCT) {
        f32x16 acc[2][2];
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
            for (int bj = 0; bj < 2; ++bj)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.f;
        float4 xa[4], ca[4];
        km_load(xa, ca, P, row0, j0, 0, tid);
        __syncthreads();  // previous centre tile's last fragment reads are done
        km_store(xa, ca, Xs[0], Cs[0], tid);
        __syncthreads();
        for (int s = 0; s < nk; ++s) {
            const int buf = s & 1;
            if (s + 1 < nk) km_load(xa, ca, P, row0, j0, (s + 1) * KBK, tid);
            const float* Ab = Xs[buf] + (wr * 64 + cl) * KP + kl;
            const float* Bb = Cs[buf] + (wc * 64 + cl) * KP + kl;
#pragma unroll 4
            for (int kk = 0; kk < KBK / 2; ++kk) {
                const float a0 = Ab[2 * kk], a1 = Ab[32 * KP + 2 * kk];
                const float b0 = Bb[2 * kk], b1 = Bb[32 * KP + 2 * kk];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
            if (s + 1 < nk) km_store(xa, ca, Xs[buf ^ 1], Cs[buf ^ 1], tid);
            __syncthreads();
        }
        // running argmin over this centre tile (ascending j per lane, strict <).  Spelled out: a call of km4_argmin here
        // costs this kernel a VGPR and 16 more spilled SGPRs
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
            const long long j = j0 + wc * 64 + bj * 32 + cl;
            if (j < P.K) {
                const float cn = P.cnorm[j];
#pragma unroll
                for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float v = cn - 2.f * acc[bi][bj][r];
                        if (v < best[bi][r]) {
                            best[bi][r] = v;
                            bidx[bi][r] = (int)j;
                        }
                    }
            }
        }
    }
    km_finish_rows(best, bidx, P, Xs[0], reinterpret_cast<int*>(Cs[0]), row0, tid, wr, wc, kl, cl, (int)blockIdx.y);
}

// ---------------------------------------------------------------------------
// Small batches of wide rows (MiniBatchKMeans' step at F = 512: B = 1024 rows, K = 1000 centres): 128 x 128 tiles make 8 x 8
// = 64 workgroups -- a quarter of the chip, each MFMA-bound for 27 us.  Same arithmetic on 64 x 64 tiles (one 32 x 32
// MFMA block per wave): 16 x 16 = 256 workgroups.  Simple double-buffered K-loop (the panels are L2-resident).
// ---------------------------------------------------------------------------
constexpr int KS64 = 64;
constexpr int KB64 = 128;  // features per K-step: few, long steps (a step costs ~1.5 us of latency whatever its length)
constexpr int KP64 = KB64 + 4;  // 16-byte aligned rows; 16 lanes x 16 bytes at this pitch cover the 64 banks once
constexpr size_t KM64_LDS = (size_t)2 * 2 * KS64 * KP64 * sizeof(float);

struct Km64Stage {
    float4 x[KB64 / 16], c[KB64 / 16];
};

// Loads are UNCONDITIONAL on the 16-byte path (rows clamped into the batch, centres into [0, K), columns into the row;
// what lies outside is zeroed when the stage goes to LDS, or never read back): a load under a branch or a select is
// followed at once by s_waitcnt vmcnt(0), and sixteen serialised L2 round trips made a K-step 6 us instead of 1.7.
__device__ __forceinline__ void km64_load(Km64Stage& st, const KmArgs& P, const long long (&xrow)[KB64 / 16], long long j0,
                                          int k0, int tid)
{
    constexpr int CPR = KB64 / 4;       // threads per row
    constexpr int RPP = KNT / CPR;      // rows per pass
    const int c4 = (tid % CPR) * 4;
    const int r0 = tid / CPR;
    const bool vec = (P.m & 3) == 0 && ((((uintptr_t)P.X) | ((uintptr_t)P.C)) & 15) == 0;
    if (vec) {  // uniform
        const long long col = (k0 + c4 + 3 < P.m) ? (long long)(k0 + c4) : P.m - 4;
#pragma unroll
        for (int j = 0; j < KS64 / RPP; ++j) {
            const long long jc = j0 + r0 + RPP * j;
            st.x[j] = *reinterpret_cast<const float4*>(P.X + xrow[j] * P.m + col);
            st.c[j] = *reinterpret_cast<const float4*>(P.C + (jc < P.K ? jc : P.K - 1) * P.m + col);
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < KS64 / RPP; ++j) {
        const int rr = r0 + RPP * j;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f), w = v;
        {
            const float* p = P.X + xrow[j] * P.m + k0 + c4;
            if (k0 + c4 + 0 < P.m) v.x = p[0];
            if (k0 + c4 + 1 < P.m) v.y = p[1];
            if (k0 + c4 + 2 < P.m) v.z = p[2];
            if (k0 + c4 + 3 < P.m) v.w = p[3];
        }
        const long long jc = j0 + rr;
        if (jc < P.K) {
            const float* p = P.C + jc * P.m + k0 + c4;
            if (k0 + c4 + 0 < P.m) w.x = p[0];
            if (k0 + c4 + 1 < P.m) w.y = p[1];
            if (k0 + c4 + 2 < P.m) w.z = p[2];
            if (k0 + c4 + 3 < P.m) w.w = p[3];
        }
        st.x[j] = v;
        st.c[j] = w;
    }
}

// `inb`: the first of this thread's four columns of the step lies inside the row (else the stage holds clamped-address data:
// zeros go to LDS).  16-byte path: m % 4 == 0, so the four are inside or outside together.  Other widths: km64_load has
// zeroed the columns past the row one by one, and the last, partial group of four must go to LDS as it is -- asking for
// all four columns to be inside dropped the last m % 4 features from every dot product.
__device__ __forceinline__ void km64_store(const Km64Stage& st, float* Xs, float* Cs, int tid, bool inb)
{
    constexpr int CPR = KB64 / 4, RPP = KNT / CPR;
    const int c4 = (tid % CPR) * 4, r0 = tid / CPR;
#pragma unroll
    for (int j = 0; j < KS64 / RPP; ++j) {
        float* px = Xs + (r0 + RPP * j) * KP64 + c4;
        float* pc = Cs + (r0 + RPP * j) * KP64 + c4;
        *reinterpret_cast<float4*>(px) = inb ? st.x[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(pc) = inb ? st.c[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

__global__ __launch_bounds__(KNT) void kmeans_label64_kernel(KmArgs P)
{
    if (P.stop && *P.stop) return;  // uniform
    extern __shared__ __attribute__((aligned(16))) char km64_smem[];
    float* Xs = reinterpret_cast<float*>(km64_smem);  // [2][KS64 * KP64]
    float* Cs = Xs + 2 * KS64 * KP64;                 // [2][KS64 * KP64]
    __shared__ float redv[2][KS64];
    __shared__ int redi[2][KS64];
    constexpr int CPR = KB64 / 4, RPP = KNT / CPR;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, kl = lane >> 5, cl = lane & 31;
    const long long row0 = (long long)blockIdx.x * KS64;
    const int nk = (int)((P.m + KB64 - 1) / KB64);
    const int r0 = tid / CPR;
    long long xrow[KS64 / RPP];  // this thread's staging rows (fixed for the workgroup's life)
#pragma unroll
    for (int j = 0; j < KS64 / RPP; ++j) {
        long long i = row0 + r0 + RPP * j;
        if (i > P.n - 1) i = P.n - 1;  // rows past the batch: clamped (their results are never written)
        xrow[j] = P.rows ? P.rows[i] : i;
    }
    const int c4s = (tid % CPR) * 4;  // this thread's first column inside a K-step
    float best[16];
    int bidx[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        best[r] = INFINITY;
        bidx[r] = 0x7fffffff;
    }
    const long long jbeg = P.jspan ? (long long)blockIdx.y * P.jspan : 0;
    const long long jend = P.jspan ? (jbeg + P.jspan < P.K ? jbeg + P.jspan : P.K) : P.K;
    for (long long j0 = jbeg; j0 < jend; j0 += KS64) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        // The panels come from the fabric side (the centres were rewritten by the previous step, the batch rows are fresh):
        // ~4 us a round trip, against 1.7 us of MFMA per K-step.  Four K-steps of loads are in flight (128 VGPRs; the
        // workgroup has a CU to itself), refilled as each stage goes to LDS.
        Km64Stage st[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nk) km64_load(st[q], P, xrow, j0, q * KB64, tid);
        __syncthreads();  // the previous centre tile's last fragment reads are done
        km64_store(st[0], Xs, Cs, tid, c4s < P.m);
        __syncthreads();
        for (int s0 = 0; s0 < nk; s0 += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int s = s0 + q;
                if (s < nk) {  // uniform
                    const int buf = q & 1;
                    if (s + 4 < nk) km64_load(st[q], P, xrow, j0, (s + 4) * KB64, tid);  // st[q] went to LDS a step ago
                    // feature order of kmeans_label_v4_kernel (MFMA q of every group of 8 features contracts {q, 4 + q}):
                    // the two kernels then form bit-identical dot products, and a row gets the same label from either
                    const float* Ab = Xs + buf * (KS64 * KP64) + (wr * 32 + cl) * KP64 + 4 * kl;
                    const float* Bb = Cs + buf * (KS64 * KP64) + (wc * 32 + cl) * KP64 + 4 * kl;
#pragma unroll
                    for (int g = 0; g < KB64 / 8; ++g) {  // a lane's 16-byte fragment: its 4 features of the group
                        const float4 a = *reinterpret_cast<const float4*>(Ab + 8 * g), b = *reinterpret_cast<const float4*>(Bb + 8 * g);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
                    }
                    if (s + 1 < nk)
                        km64_store(st[(q + 1) & 3], Xs + (buf ^ 1) * (KS64 * KP64), Cs + (buf ^ 1) * (KS64 * KP64), tid,
                                   (s + 1) * KB64 + c4s < P.m);
                    __syncthreads();
                }
            }
        }
        const long long j = j0 + wc * 32 + cl;  // running argmin over this centre tile (ascending j per lane, strict <)
        if (j < jend) {
            const float cn = P.cnorm[j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float v = cn - 2.f * acc[r];
                if (v < best[r]) {
                    best[r] = v;
                    bidx[r] = (int)j;
                }
            }
        }
    }
    // min over the 32 lanes that share a row (value, lowest index), then over the two centre halves
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = best[r];
        int ix = bidx[r];
#pragma unroll
        for (int msk = 1; msk < 32; msk <<= 1) {
            const float ov = __shfl_xor(v, msk, 64);
            const int oi = __shfl_xor(ix, msk, 64);
            if (ov < v || (ov == v && oi < ix)) {
                v = ov;
                ix = oi;
            }
        }
        if (cl == 0) {
            const int row = wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * kl;
            redv[wc][row] = v;
            redi[wc][row] = ix;
        }
    }
    __syncthreads();
    if (tid < KS64) {
        const long long i = row0 + tid;
        if (i < P.n) km_write_row<float>(P, i, redv[0][tid], redv[1][tid], redi[0][tid], redi[1][tid], (int)blockIdx.y);
    }
}

// ---------------------------------------------------------------------------
// Fast path (m % 4 == 0, 16-byte aligned rows): same tiling, restructured for the MFMA pipe.
//  * LDS tiles stay row-major [128][KP4=36] (16-byte aligned rows -> ds_write_b128 in,
//    ds_read_b128 out).  A lane's b128 fragment holds 4 CONSECUTIVE features of its row; the
//    32x32x2 MFMA wants features (k, k+1) from lanes (kl=0, kl=1), so within every group of 8
//    features MFMA q contracts features {q, 4+q}: a permutation of the summation order applied
//    to rows and centres alike (the reference arithmetic is an sgemm whose order is unspecified).
//    Pitch 36 words: 16 lanes x b128 cover all 64 banks exactly once.
//  * (centre tile, K-step) pairs form ONE flat iteration stream; the register pipeline is two
//    iterations deep and never drains at a centre-tile boundary.  Loads are unconditional
//    (rows/centres/columns clamped, out-of-range columns zeroed at LDS-store time) and the
//    4 feature groups of a step are fully unrolled: branches or loops around in-flight loads
//    make the compiler wait vmcnt(0) (see tica.hip).
// ---------------------------------------------------------------------------
constexpr int KP4 = KBK + 4;

struct KmStage {
    float4 x[4], c[4];
};

// Like the tICA kernel (tica.hip, "staging with an INTERIOR fast path"): a wave's non-MFMA instructions
// crawl while the co-resident wave streams MFMAs, so a K-step carries as few of them as possible and
// issues its 8 global loads and 8 LDS writes from INSIDE its own MFMA stream.  Interior steps (all 32
// columns inside [0, m), every step but a partial last one) load through per-lane offsets that are
// constant per centre tile on top of scalar bases, and write the loaded registers to LDS unchanged;
// clamps and zero-masks live in uniform branches that hold VALU work only.
template <bool GATHER>
__global__ __launch_bounds__(KNT, 2) void kmeans_label_v4_kernel(KmArgs P)
{
    if (P.stop && *P.stop) return;  // uniform
    extern __shared__ __attribute__((aligned(16))) char km_smem[];
    float* Xs = reinterpret_cast<float*>(km_smem);  // [2][KR * KP4]
    float* Cs = Xs + 2 * KR * KP4;                  // [2][KCT * KP4]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, kl = lane >> 5, cl = lane & 31;
    // P.xcd_ns: a workgroup that walks ALL centre tiles streams its 128 rows once per tile, and with 64 workgroups
    // per XCD those 8 x 256 KB re-reads never hit the 4 MB L2 (1M x 512, K = 1000: 16 GB fetched per pass for 2 GB of rows).
    // Instead one workgroup per (row block, centre tile), numbered so that the tiles of a row block are consecutive
    // workgroups of ONE XCD (workgroup b runs on XCD b % 8): they run side by side, the row block is fetched once and
    // served to the other tiles from that XCD's L2; the per-tile candidates are merged by the inertia / reduce kernel.
    long long rb = blockIdx.x;
    int split = (int)blockIdx.y;
    if (P.xcd_ns) {
        const unsigned b = blockIdx.x, q = b >> 3;
        split = (int)(q % (unsigned)P.xcd_ns);
        rb = (long long)(q / (unsigned)P.xcd_ns) * 8 + (b & 7);
        if (rb * KR >= P.n) return;   // (the grid is rounded up to whole groups of 8 row blocks)
    }
    const long long row0 = rb * KR;
    const int m = (int)P.m;
    const int nk = (m + KBK - 1) / KBK;
    const unsigned ldb = (unsigned)m * 4u;
    const int c4 = (tid & 7) * 4, r0 = tid >> 3;

    float best[2][16];
    int bidx[2][16];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            best[bi][r] = INFINITY;
            bidx[bi][r] = 0x7fffffff;
        }

    // this thread's 4 staging rows of X (fixed for the workgroup's life; clamped into [0, n)):
    // contiguous rows -> one scalar base + 32-bit lane offsets; gathered rows -> 64-bit lane pointers
    const global_ptr<char> Xg = as_global<char>(P.X) + (GATHER ? (size_t)0 : (size_t)row0 * ldb);
    global_ptr<char> xp[4];
    unsigned xo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        long long i = row0 + r0 + 32 * j;
        if (i > P.n - 1) i = P.n - 1;
        if (GATHER) {
            xp[j] = Xg + (size_t)as_global<msm_idx_t>(P.rows)[i] * ldb + 4u * (unsigned)c4;
            xo[j] = 0;
        } else {
            xp[j] = Xg;
            xo[j] = (unsigned)(i - row0) * ldb + 4u * (unsigned)c4;
        }
    }
    const global_ptr<char> Cg = as_global<char>(P.C);

    const long long jbeg = P.jspan ? (long long)split * P.jspan : 0;
    const long long jend = P.jspan ? (jbeg + P.jspan < P.K ? jbeg + P.jspan : P.K) : P.K;
    const long long total = ((jend - jbeg + KCT - 1) / KCT) * nk;

    f32x16 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[bi][bj][r] = 0.f;

    // load cursor (runs two iterations ahead of the compute cursor; parks on the last tile) and the
    // centre-row lane offsets of its tile (rows clamped to K - 1: recomputed when the tile changes)
    int ls = 0;
    long long lj0 = jbeg;
    unsigned co[4];
#define KM4_TILE_OFFS                                                                             \
    {                                                                                             \
        const long long lim = P.K - 1 - lj0;                                                      \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                           \
            const int rr = r0 + 32 * j;                                                           \
            co[j] = (unsigned)(rr < lim ? rr : (int)lim) * ldb + 4u * (unsigned)c4;               \
        }                                                                                         \
    }
    KM4_TILE_OFFS
    // addresses of the load cursor's step: scalar byte offset of its first column + (partial last step
    // only) a per-lane column correction; `un` = the step needs no zero-masking when it reaches LDS
#define KM4_ADDR(KOFF, CADJ, UN)                                                                  \
    {                                                                                             \
        KOFF = (unsigned)ls * (KBK * 4u);                                                         \
        CADJ = 0;                                                                                 \
        UN = 1;                                                                                   \
        if (ls * KBK + KBK > m) { /* partial last K-step: clamp this lane's columns into the row */ \
            const int col = ls * KBK + c4;                                                        \
            CADJ = col < m ? 0u : 4u * (unsigned)(col - (m - 4));                                 \
            UN = 0;                                                                               \
        }                                                                                         \
    }
#define KM4_ADVANCE                                                                               \
    if (++ls == nk) {                                                                             \
        ls = 0;                                                                                   \
        if (lj0 + KCT < jend) {                                                                   \
            lj0 += KCT;                                                                           \
            KM4_TILE_OFFS                                                                         \
        }                                                                                         \
    }
#define KM4_LD_X(J, KOFF, CADJ)                                                                   \
    (GATHER ? load16_global<char>(xp[J] + ((long long)(KOFF) - (long long)(CADJ)))                \
            : load16_global<char>(xp[J] + (size_t)(KOFF) + (xo[J] - (CADJ))))
#define KM4_LD_C(J, KOFF, CADJ) load16_global<char>(Cg + (size_t)lj0c * ldb + (size_t)(KOFF) + (co_c[J] - (CADJ)))
    // zero this lane's out-of-range columns of a loaded stage (partial last K-step only)
#define KM4_MASK(ST, INB)                                                                         \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                               \
        ST.x[j] = make_float4(INB ? ST.x[j].x : 0.f, INB ? ST.x[j].y : 0.f, INB ? ST.x[j].z : 0.f, INB ? ST.x[j].w : 0.f); \
        ST.c[j] = make_float4(INB ? ST.c[j].x : 0.f, INB ? ST.c[j].y : 0.f, INB ? ST.c[j].z : 0.f, INB ? ST.c[j].w : 0.f); \
    }
    KmStage st0, st1;
    int un0 = 1, un1 = 1, inb0 = 1, inb1 = 1;
    {   // prologue: step 0 -> LDS, step 1 -> registers
        unsigned koff, cadj;
        int un;
        long long lj0c = lj0;
        unsigned co_c[4] = {co[0], co[1], co[2], co[3]};
        KM4_ADDR(koff, cadj, un)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st0.x[j] = KM4_LD_X(j, koff, cadj);
            st0.c[j] = KM4_LD_C(j, koff, cadj);
        }
        const bool inb = cadj == 0;
        if (!un) { KM4_MASK(st0, inb) }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<float4*>(Xs + (r0 + 32 * j) * KP4 + c4) = st0.x[j];
            *reinterpret_cast<float4*>(Cs + (r0 + 32 * j) * KP4 + c4) = st0.c[j];
        }
        KM4_ADVANCE
        lj0c = lj0;
        co_c[0] = co[0]; co_c[1] = co[1]; co_c[2] = co[2]; co_c[3] = co[3];
        KM4_ADDR(koff, cadj, un0)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st0.x[j] = KM4_LD_X(j, koff, cadj);
            st0.c[j] = KM4_LD_C(j, koff, cadj);
        }
        inb0 = cadj == 0;
        KM4_ADVANCE
    }
    __syncthreads();

    int s = 0;
    long long j0 = jbeg;
#define KM4_MFMA4(A0, A1, B0, B1)                                                                 \
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0, B0, acc[0][0], 0, 0, 0);                 \
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0, B1, acc[0][1], 0, 0, 0);                 \
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1, B0, acc[1][0], 0, 0, 0);                 \
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1, B1, acc[1][1], 0, 0, 0);
#define KM4_STEP(SNEXT, UNEXT, INEXT, SLOAD, ULOAD, ILOAD, BUF)                                   \
    {                                                                                             \
        /* addresses of iteration it+2 (no loads yet); the cursor moves on */                     \
        unsigned koff, cadj;                                                                      \
        const long long lj0c = lj0;                                                               \
        const unsigned co_c[4] = {co[0], co[1], co[2], co[3]};                                    \
        KM4_ADDR(koff, cadj, ULOAD)                                                               \
        ILOAD = cadj == 0;                                                                        \
        KM4_ADVANCE                                                                               \
        /* iteration it+1's panel is about to go to LDS: zero-mask it if it is a partial step */  \
        if (!UNEXT) { const bool inb = INEXT != 0; KM4_MASK(SNEXT, inb) }                         \
        const float* Ab = Xs + (BUF) * (KR * KP4) + (wr * 64 + cl) * KP4 + kl * 4;                \
        const float* Bb = Cs + (BUF) * (KCT * KP4) + (wc * 64 + cl) * KP4 + kl * 4;               \
        float* Xw = Xs + ((BUF) ^ 1) * (KR * KP4) + r0 * KP4 + c4;                                \
        float* Cw = Cs + ((BUF) ^ 1) * (KCT * KP4) + r0 * KP4 + c4;                               \
        float4 a0 = *reinterpret_cast<const float4*>(Ab), a1 = *reinterpret_cast<const float4*>(Ab + 32 * KP4); \
        float4 b0 = *reinterpret_cast<const float4*>(Bb), b1 = *reinterpret_cast<const float4*>(Bb + 32 * KP4); \
        _Pragma("unroll") for (int g = 0; g < KBK / 8; ++g) {                                     \
            const int gn = (g + 1 < KBK / 8) ? g + 1 : g;                                         \
            const float4 na0 = *reinterpret_cast<const float4*>(Ab + gn * 8);                     \
            const float4 na1 = *reinterpret_cast<const float4*>(Ab + 32 * KP4 + gn * 8);          \
            const float4 nb0 = *reinterpret_cast<const float4*>(Bb + gn * 8);                     \
            const float4 nb1 = *reinterpret_cast<const float4*>(Bb + 32 * KP4 + gn * 8);          \
            /* memory ops of this step, spread over the four MFMA quads of each feature group:   */ \
            /* groups 0-1: the 8 loads of iteration it+2; groups 2-3: the 8 LDS writes of it+1    */ \
            if (g < 2) { SLOAD.x[2 * g] = KM4_LD_X(2 * g, koff, cadj); SLOAD.c[2 * g] = KM4_LD_C(2 * g, koff, cadj); } \
            if (g >= 2) { *reinterpret_cast<float4*>(Xw + (2 * (g - 2)) * 32 * KP4) = SNEXT.x[2 * (g - 2)];           \
                          *reinterpret_cast<float4*>(Cw + (2 * (g - 2)) * 32 * KP4) = SNEXT.c[2 * (g - 2)]; }         \
            __builtin_amdgcn_sched_barrier(0);                                                    \
            KM4_MFMA4(a0.x, a1.x, b0.x, b1.x)                                                     \
            KM4_MFMA4(a0.y, a1.y, b0.y, b1.y)                                                     \
            __builtin_amdgcn_sched_barrier(0);                                                    \
            if (g < 2) { SLOAD.x[2 * g + 1] = KM4_LD_X(2 * g + 1, koff, cadj); SLOAD.c[2 * g + 1] = KM4_LD_C(2 * g + 1, koff, cadj); } \
            if (g >= 2) { *reinterpret_cast<float4*>(Xw + (2 * (g - 2) + 1) * 32 * KP4) = SNEXT.x[2 * (g - 2) + 1];   \
                          *reinterpret_cast<float4*>(Cw + (2 * (g - 2) + 1) * 32 * KP4) = SNEXT.c[2 * (g - 2) + 1]; } \
            __builtin_amdgcn_sched_barrier(0);                                                    \
            KM4_MFMA4(a0.z, a1.z, b0.z, b1.z)                                                     \
            KM4_MFMA4(a0.w, a1.w, b0.w, b1.w)                                                     \
            __builtin_amdgcn_sched_barrier(0);                                                    \
            a0 = na0; a1 = na1; b0 = nb0; b1 = nb1;                                               \
        }                                                                                         \
        __syncthreads();                                                                          \
        if (++s == nk) {                                                                          \
            s = 0;                                                                                \
            km4_argmin(acc, best, bidx, P, j0, wc, cl);                                           \
            j0 += KCT;                                                                            \
        }                                                                                         \
    }
    for (long long it = 0; it < total; it += 2) {
        KM4_STEP(st0, un0, inb0, st1, un1, inb1, 0)
        ++it;
        if (it < total) KM4_STEP(st1, un1, inb1, st0, un0, inb0, 1)
        --it;
    }
#undef KM4_STEP
#undef KM4_MFMA4
#undef KM4_MASK
#undef KM4_LD_C
#undef KM4_LD_X
#undef KM4_ADVANCE
#undef KM4_ADDR
#undef KM4_TILE_OFFS
    km_finish_rows(best, bidx, P, Xs, reinterpret_cast<int*>(Cs), row0, tid, wr, wc, kl, cl, split);
}

constexpr size_t KM4_LDS = (size_t)2 * (KR + KCT) * KP4 * sizeof(float);

}  // namespace msm
