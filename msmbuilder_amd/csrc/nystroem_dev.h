// nystroem_dev.h -- the kernel feature map out[i, :] = k(x_i, landmarks) . B - c (msm_kernel_map_*, nystroem.hip).
//
// A workgroup of four waves owns R = 16 * RB rows and works in two phases that share one block of R x Lpad float64 kernel
// values, pitch Lpad + 4 doubles:
//   phase 1  builds the block 16 x 16 tile by tile.  x . l is a chain of v_mfma_f64_16x16x4_f64 over the feature depth
//            (float32 rows are widened exactly); the kernel function is the tile's epilogue.  `laplacian` has no
//            product form: its tile is a VALU loop over |x - l|.  The squared row norms that `rbf` and `cosine` need are
//            the diagonal of the same MFMA chain run on the rows against themselves, so that a row EQUAL to a landmark has
//            |x|^2 + |l|^2 - 2 x.l == 0 exactly; the landmarks' norms come from ny_lnorm_kernel, once per call.
//   phase 2  multiplies the block by B[L x P] (float64, read from L2 16 columns at a time), again 16 x 16 x 4 per MFMA,
//            in landmark order, subtracts c and writes R x P.
// Fused route: the block lives in LDS and never reaches HBM (ny_fused_kernel).  Scratch route: the same two device
// functions run as two launches over a row chunk with the block in a global buffer.  An output element is accumulated in the
// same order whichever route and whichever R computed it: the routes are bit-identical.
#pragma once
#include "common.h"

namespace msm {

enum NyKernel : int { NK_LINEAR = 0, NK_POLY, NK_SIGMOID, NK_COSINE, NK_RBF, NK_LAPLACIAN, NK_COUNT };

constexpr int NY_T = 256;        // threads of a workgroup (4 waves)
constexpr int NY_RB_MAX = 4;     // row blocks of 16 per workgroup, at most
constexpr int NY_PAD = 4;        // doubles added to the block's pitch

typedef double ny_f64x4 __attribute__((ext_vector_type(4)));

struct NyArgs {
    const void* X;        // rows [n][ld]
    long long n, ld;
    int F;
    const void* Lm;       // landmarks [L][F]
    int L, Lpad, pitch;
    const double* lmn;    // per landmark: |l|^2 (cosine: |l|)
    const double* B;      // [L][P]
    int P;
    const double* c;      // [P] or null
    void* out;            // [n][P]
    double gamma, coef0, degree;
    int kid, RB;
    double* scratch;      // scratch route: [rows of the chunk][pitch]
    int* flag;            // bit 0: a row value is not finite; bit 1: a landmark value is not finite
};

// |l|^2 (cosine: |l|) of 16 landmarks per wave: the diagonal of the tile's MFMA chain against itself.
template <typename T>
__global__ __launch_bounds__(64) void ny_lnorm_kernel(const T* __restrict__ Lm, int L, int F, int kid, double* __restrict__ lmn,
                                                      int* flag)
{
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    const int col = blockIdx.x * 16 + r;
    ny_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    int bad = 0;
    for (int f0 = 0; f0 < F; f0 += 4) {
        const int f = f0 + g;
        double b = 0.0;
        if (f < F && col < L) {
            b = (double)Lm[(size_t)col * F + f];
            bad |= !isfinite(b);
        }
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(b, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (g + 4 * q == r && col < L) lmn[col] = kid == NK_COSINE ? sqrt(acc[q]) : acc[q];
    if (bad) atomicOr(flag, 2);
}

__device__ __forceinline__ double ny_apply(int kid, double v, double nx, double nl, double gamma, double coef0, double degree)
{
    switch (kid) {
        case NK_LINEAR: return v;
        case NK_POLY: return pow(gamma * v + coef0, degree);
        case NK_SIGMOID: return tanh(gamma * v + coef0);
        case NK_COSINE: {
            const double a = sqrt(nx);
            return v / ((a == 0.0 ? 1.0 : a) * (nl == 0.0 ? 1.0 : nl));   // a zero vector is left as it is (scikit-learn's normalize)
        }
        default: {   // NK_RBF
            const double d2 = (nx + nl) - 2.0 * v;
            return exp(-gamma * (d2 < 0.0 ? 0.0 : d2));   // (a NaN, from norms that overflow, stays a NaN)
        }
    }
}

// Phase 1: Kd[16 * RB][pitch] <- k(rows row0 .., landmarks); columns L .. Lpad - 1 are written as zeros.
template <typename T>
__device__ __forceinline__ void ny_phase1(const NyArgs& A, long long row0, double* Kd, double* rown)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const T* __restrict__ X = static_cast<const T*>(A.X);
    const T* __restrict__ Lm = static_cast<const T*>(A.Lm);
    const int F = A.F, L = A.L, RB = A.RB, pitch = A.pitch;
    int bad = 0;
    // squared norms of the block's rows; every value of the block is read here once and checked
    for (int rb = wave; rb < RB; rb += 4) {
        const long long i = row0 + rb * 16 + r;
        ny_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int f0 = 0; f0 < F; f0 += 4) {
            const int f = f0 + g;
            double a = 0.0;
            if (f < F && i < A.n) {
                a = (double)X[i * A.ld + f];
                bad |= !isfinite(a);
            }
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (g + 4 * q == r) rown[rb * 16 + r] = acc[q];
    }
    if (bad) atomicOr(A.flag, 1);
    __syncthreads();
    const int Lt = A.Lpad / 16;
    for (int t = wave; t < RB * Lt; t += 4) {
        const int rb = t % RB, lt = t / RB;
        const int col = lt * 16 + r;
        ny_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        if (A.kid == NK_LAPLACIAN) {
            for (int f = 0; f < F; ++f) {
                const double l = col < L ? (double)Lm[(size_t)col * F + f] : 0.0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long long i = row0 + rb * 16 + g + 4 * q;
                    const double x = i < A.n ? (double)X[i * A.ld + f] : 0.0;
                    acc[q] += fabs(x - l);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = exp(-A.gamma * acc[q]);
        } else {
            // 16 features per trip: the eight loads are issued before the four MFMAs (unconditional, from clamped addresses,
            // zeroed afterwards), which stay ONE chain in ascending feature order; a depth step wholly past F adds 0 * 0
            const long long i = row0 + rb * 16 + r;
            const T* __restrict__ xr = X + (i < A.n ? i : A.n - 1) * A.ld;
            const T* __restrict__ lr = Lm + (size_t)(col < L ? col : L - 1) * F;
            for (int f0 = 0; f0 < F; f0 += 16) {
                T av[4], bv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = f0 + 4 * j + g, fc = f < F ? f : F - 1;
                    av[j] = xr[fc];
                    bv[j] = lr[fc];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int f = f0 + 4 * j + g;
                    const double a = (f < F && i < A.n) ? (double)av[j] : 0.0;
                    const double b = (f < F && col < L) ? (double)bv[j] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
                }
            }
            const double nl = col < L ? A.lmn[col] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[q] = ny_apply(A.kid, acc[q], rown[rb * 16 + g + 4 * q], nl, A.gamma, A.coef0, A.degree);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) Kd[(size_t)(rb * 16 + g + 4 * q) * pitch + col] = col < L ? acc[q] : 0.0;
    }
}

// Phase 2: out[rows row0 ..][P] <- Ks[16 * RB][pitch] . B - c
template <typename TO>
__device__ __forceinline__ void ny_phase2(const NyArgs& A, long long row0, const double* Ks)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
    const int L = A.L, P = A.P, RB = A.RB, pitch = A.pitch;
    const double* __restrict__ B = A.B;
    TO* __restrict__ out = static_cast<TO*>(A.out);
    const int Pt = (P + 15) / 16;
    for (int t = wave; t < RB * Pt; t += 4) {
        const int rb = t % RB, pt = t / RB;
        const int p = pt * 16 + r;
        const double* ka = Ks + (size_t)(rb * 16 + r) * pitch + g;
        ny_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        // 16 landmarks (one tile of the block; Lpad is a multiple of 16) per trip: the four loads of B and of the block are
        // issued before the four MFMAs, which stay ONE chain in ascending landmark order.  Loads are unconditional (clamped
        // addresses, the value zeroed afterwards) so that they can be in flight together.
        const int pc = p < P ? p : P - 1;
        for (int l0 = 0; l0 < A.Lpad; l0 += 16) {
            double kv[4], bv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int l = l0 + 4 * j + g;
                bv[j] = B[(size_t)(l < L ? l : L - 1) * P + pc];
                kv[j] = ka[l0 + 4 * j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int l = l0 + 4 * j + g;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(kv[j], (l < L && p < P) ? bv[j] : 0.0, acc, 0, 0, 0);
            }
        }
        if (p < P) {
            const double cv = A.c ? A.c[p] : 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const long long i = row0 + rb * 16 + g + 4 * q;
                if (i < A.n) out[i * P + p] = (TO)(acc[q] - cv);
            }
        }
    }
}

template <typename T, typename TO>
__global__ __launch_bounds__(NY_T) void ny_fused_kernel(NyArgs A)
{
    extern __shared__ __attribute__((aligned(16))) char ny_smem[];
    __shared__ double rown[16 * NY_RB_MAX];
    double* Ks = reinterpret_cast<double*>(ny_smem);
    const long long row0 = (long long)blockIdx.x * (16 * A.RB);
    ny_phase1<T>(A, row0, Ks, rown);
    __syncthreads();
    ny_phase2<TO>(A, row0, Ks);
}

// the scratch route's two launches over the rows [0, A.n) of a chunk
template <typename T>
__global__ __launch_bounds__(NY_T) void ny_phase1_kernel(NyArgs A)
{
    __shared__ double rown[16 * NY_RB_MAX];
    const long long row0 = (long long)blockIdx.x * (16 * A.RB);
    ny_phase1<T>(A, row0, A.scratch + (size_t)row0 * A.pitch, rown);
}

template <typename TO>
__global__ __launch_bounds__(NY_T) void ny_phase2_kernel(NyArgs A)
{
    const long long row0 = (long long)blockIdx.x * (16 * A.RB);
    ny_phase2<TO>(A, row0, A.scratch + (size_t)row0 * A.pitch);
}

}  // namespace msm
