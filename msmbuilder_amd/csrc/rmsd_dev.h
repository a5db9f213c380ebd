// rmsd_dev.h -- device side of the rmsd metric: the ONE definition of the distance (rmsd_qcp) and the two kernels
// that feed it the 3 x 3 inner-product matrix of a pair of centred conformations.
//
//   image   T[c][a][n_pad] float32, c = x, y, z: atom-major, frame-fastest, frames zero-padded to a multiple of 64;
//           G[n_pad] float64 = the sum of squares of a frame's (centred, float32) coordinates
//   pair    M_ab = sum_k x_ka * y_kb: a float32 fmaf chain over the atoms from atom 0; an odd atom count ends with one
//           fmaf(0, 0, .) step (the tile kernel's zero-padded k-step, repeated by the row kernel)
//   rmsd    coefficients of the 4 x 4 key matrix's characteristic quartic in float64 from the nine floats, Newton from
//           (G_x + G_y) / 2, msd = max((G_x + G_y - 2 lambda) / A, 0), sqrt in float64
//
// Every path (dist, cdist, pdist, sumdist, assign_nearest, the k-centers pass) hands rmsd_qcp the same nine floats and
// the same two doubles for the same pair, so the distances agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace msm {

typedef float rmsd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int RMSD_BLOCK = 256;     // threads per workgroup of every kernel here
constexpr int RMSD_FRAME_PAD = 64;  // frames are padded to a multiple of this (one wave of lanes, two MFMA tiles)
constexpr int RMSD_KU = 6;          // k-steps (of two atoms) whose operands the tile kernel fetches as one group
constexpr int RMSD_NEWTON_MAX = 50;
constexpr double RMSD_NEWTON_TOL = 1e-11;

struct RmsdImage {
    const float* T;   // [3][A][n_pad]
    const double* G;  // [n_pad]
    long long n;      // frames
    long long n_pad;
    long long A;      // atoms
};

// The distance of one pair from its inner-product matrix m[3 * a + b] = M_ab (a: x's axis, b: y's axis).
__device__ __forceinline__ double rmsd_qcp(const float (&m)[9], double Gx, double Gy, long long A)
{
    const double Sxx = m[0], Sxy = m[1], Sxz = m[2];
    const double Syx = m[3], Syy = m[4], Syz = m[5];
    const double Szx = m[6], Szy = m[7], Szz = m[8];
    // lambda^4 + C2 lambda^2 + C1 lambda + C0 = det(lambda I - K), K the symmetric traceless key matrix below
    const double C2 = -2.0 * (Sxx * Sxx + Sxy * Sxy + Sxz * Sxz + Syx * Syx + Syy * Syy + Syz * Syz + Szx * Szx + Szy * Szy +
                              Szz * Szz);
    const double C1 = -8.0 * (Sxx * (Syy * Szz - Syz * Szy) - Sxy * (Syx * Szz - Syz * Szx) + Sxz * (Syx * Szy - Syy * Szx));
    const double k00 = Sxx + Syy + Szz, k01 = Syz - Szy, k02 = Szx - Sxz, k03 = Sxy - Syx;
    const double k11 = Sxx - Syy - Szz, k12 = Sxy + Syx, k13 = Szx + Sxz;
    const double k22 = -Sxx + Syy - Szz, k23 = Syz + Szy;
    const double k33 = -Sxx - Syy + Szz;
    // det K by the 2 x 2 minors of rows (0, 1) and rows (2, 3)
    const double s0 = k00 * k11 - k01 * k01, s1 = k00 * k12 - k02 * k01, s2 = k00 * k13 - k03 * k01;
    const double s3 = k01 * k12 - k02 * k11, s4 = k01 * k13 - k03 * k11, s5 = k02 * k13 - k03 * k12;
    const double c5 = k22 * k33 - k23 * k23, c4 = k12 * k33 - k23 * k13, c3 = k12 * k23 - k22 * k13;
    const double c2 = k02 * k33 - k23 * k03, c1 = k02 * k23 - k22 * k03, c0 = k02 * k13 - k12 * k03;
    const double C0 = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;

    const double Gs = Gx + Gy;
    double lam = Gs / 2.0;
    for (int it = 0; it < RMSD_NEWTON_MAX; ++it) {
        const double l2 = lam * lam;
        const double b = (l2 + C2) * lam;
        const double a = b + C1;
        const double P = a * lam + C0;
        const double dP = 2.0 * l2 * lam + b + a;
        if (dP == 0.0) break;
        const double step = P / dP;
        lam = lam - step;
        if (fabs(step) < RMSD_NEWTON_TOL * fabs(lam)) break;
    }
    const double msd = (Gs - 2.0 * lam) / (double)A;
    return sqrt(msd < 0.0 ? 0.0 : msd);   // (a NaN stays a NaN: fmax would drop it)
}

// ---- prepare: xyz[n][A][3] -> image, one lane per frame --------------------------------------------------------------
__global__ __launch_bounds__(RMSD_BLOCK) void rmsd_prepare_kernel(const float* __restrict__ xyz, long long n, long long n_pad,
                                                                   long long A, float* __restrict__ T, double* __restrict__ G)
{
    const long long f = (long long)blockIdx.x * RMSD_BLOCK + threadIdx.x;
    if (f >= n_pad) return;
    const size_t plane = (size_t)A * (size_t)n_pad;
    if (f >= n) {   // the padding frames: all zero
        for (long long a = 0; a < A; ++a) {
            const size_t o = (size_t)a * (size_t)n_pad + (size_t)f;
            T[o] = 0.0f;
            T[plane + o] = 0.0f;
            T[2 * plane + o] = 0.0f;
        }
        G[f] = 0.0;
        return;
    }
    const float* p = xyz + (size_t)f * (size_t)A * 3;
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (long long a = 0; a < A; ++a) {
        c0 = c0 + (double)p[3 * a];
        c1 = c1 + (double)p[3 * a + 1];
        c2 = c2 + (double)p[3 * a + 2];
    }
    c0 = c0 / (double)A;
    c1 = c1 / (double)A;
    c2 = c2 / (double)A;
    double g = 0.0;
    for (long long a = 0; a < A; ++a) {
        const float x = (float)((double)p[3 * a] - c0);
        const float y = (float)((double)p[3 * a + 1] - c1);
        const float z = (float)((double)p[3 * a + 2] - c2);
        const size_t o = (size_t)a * (size_t)n_pad + (size_t)f;
        T[o] = x;
        T[plane + o] = y;
        T[2 * plane + o] = z;
        g = g + (double)x * (double)x;
        g = g + (double)y * (double)y;
        g = g + (double)z * (double)z;
    }
    G[f] = g;
}

// flag[0] = 1 if any idx[i] lies outside [0, n)
__global__ void rmsd_check_index_kernel(const long long* __restrict__ idx, long long count, long long n, int* __restrict__ flag)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && (idx[i] < 0 || idx[i] >= n)) flag[0] = 1;
}

// ---- tile kernel: a wave owns 32 rows x 32 columns, nine fp32 MFMA accumulators -----------------------------------------
enum { RMSD_EPI_CDIST = 0, RMSD_EPI_PDIST = 1, RMSD_EPI_ASSIGN = 2 };

struct RmsdTileArgs {
    RmsdImage R, C;              // rows (the MFMA's A operand, i) and columns (B operand, j)
    const long long* ridx;       // gather of the rows / columns through an index (or null)
    const long long* cidx;
    long long nr, nc;            // logical rows / columns
    double* out;                 // cdist: [nr][nc]; pdist: condensed
    long long* labels;           // assign (rows = centres, columns = frames): [nc]
    double* min_dist;            // assign: [nc]
};

// accumulate the nine planes of tile (ti, tj) over the atoms; lane l feeds row (l & 31) and column (l & 31) at atom 2 s + (l >> 5)
__device__ __forceinline__ void rmsd_tile_products(const RmsdTileArgs& P, long long ti, long long tj, rmsd_f32x16 (&acc)[9])
{
    const int lane = threadIdx.x & 63;
    const int half = lane >> 5;
    const long long r = ti * 32 + (lane & 31), c = tj * 32 + (lane & 31);
    // rows / columns past the end read frame 0 (n >= 1) and are masked where the result is used
    const long long fr = r < P.nr ? (P.ridx ? P.ridx[r] : r) : 0;
    const long long fc = c < P.nc ? (P.cidx ? P.cidx[c] : c) : 0;
    const long long A = P.R.A;
    const size_t rplane = (size_t)A * (size_t)P.R.n_pad, cplane = (size_t)A * (size_t)P.C.n_pad;
    const float* pr = P.R.T + (size_t)fr;
    const float* pc = P.C.T + (size_t)fc;
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[q][e] = 0.0f;
    // One wave per SIMD fits (nine accumulators), so the loads must run far ahead of the MFMAs on their own: the operands of
    // RMSD_KU k-steps are fetched as a group while the previous group's 9 * RMSD_KU MFMAs (64 cycles each) issue.
    const long long steps = (A + 1) / 2;
    const long long groups = (steps + RMSD_KU - 1) / RMSD_KU;
    float x[RMSD_KU][3], y[RMSD_KU][3];
#pragma unroll
    for (int u = 0; u < RMSD_KU; ++u) {
        const long long a = 2 * u + half;
        const bool ok = a < A;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x[u][d] = ok ? pr[d * rplane + (size_t)a * (size_t)P.R.n_pad] : 0.0f;
            y[u][d] = ok ? pc[d * cplane + (size_t)a * (size_t)P.C.n_pad] : 0.0f;
        }
    }
    for (long long g = 0; g < groups; ++g) {
        float xn[RMSD_KU][3], yn[RMSD_KU][3];
#pragma unroll
        for (int u = 0; u < RMSD_KU; ++u) {
            const long long a = 2 * ((g + 1) * RMSD_KU + u) + half;   // an atom past the end: zero, the odd count's padded step
            const bool ok = a < A;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                xn[u][d] = ok ? pr[d * rplane + (size_t)a * (size_t)P.R.n_pad] : 0.0f;
                yn[u][d] = ok ? pc[d * cplane + (size_t)a * (size_t)P.C.n_pad] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < RMSD_KU; ++u) {
            if (g * RMSD_KU + u < steps) {   // (uniform: whole k-steps past the last one are not issued)
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        acc[3 * p + q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u][p], y[u][q], acc[3 * p + q], 0, 0, 0);
            }
        }
#pragma unroll
        for (int u = 0; u < RMSD_KU; ++u)
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                x[u][d] = xn[u][d];
                y[u][d] = yn[u][d];
            }
    }
}

// the nine entries of a lane's pair number `reg` (uniform over the wave): a select chain over the sixteen accumulator
// registers of each plane, so the rolled epilogue loop holds ONE copy of rmsd_qcp and the accumulators are never copied
__device__ __forceinline__ void rmsd_take(const rmsd_f32x16 (&acc)[9], int reg, float (&m)[9], bool transpose)
{
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float v = acc[3 * p + q][0];
#pragma unroll
            for (int e = 1; e < 16; ++e) v = reg == e ? acc[3 * p + q][e] : v;
            m[transpose ? 3 * q + p : 3 * p + q] = v;
        }
}

template <int EPI>
__global__ __launch_bounds__(RMSD_BLOCK) void rmsd_tile_kernel(RmsdTileArgs P)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5;
    rmsd_f32x16 acc[9];
    float m[9];
    if (EPI == RMSD_EPI_ASSIGN) {
        // rows = centres, columns = frames: a lane keeps ONE frame and walks the centres in ascending order
        const long long tj = (long long)blockIdx.x * (RMSD_BLOCK / 64) + wave;
        if (tj * 32 >= P.nc) return;
        const long long c = tj * 32 + (lane & 31);
        const long long fc = c < P.nc ? (P.cidx ? P.cidx[c] : c) : 0;
        const double Gframe = P.C.G[fc];
        double best = (double)FLT_MAX;
        long long best_i = 0;
        const long long tiles = (P.nr + 31) / 32;
        for (long long ti = 0; ti < tiles; ++ti) {
            rmsd_tile_products(P, ti, tj, acc);
#pragma unroll 1
            for (int reg = 0; reg < 16; ++reg) {
                rmsd_take(acc, reg, m, true);
                const long long r = ti * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
                if (r < P.nr) {
                    const long long fr = P.ridx ? P.ridx[r] : r;
                    const double d = rmsd_qcp(m, Gframe, P.R.G[fr], P.R.A);
                    if (d < best) {   // strict: the lowest centre wins a tie, a NaN never wins
                        best = d;
                        best_i = r;
                    }
                }
            }
        }
        const double other = __shfl_xor(best, 32);
        const long long other_i = __shfl_xor(best_i, 32);
        if (other < best || (other == best && other_i < best_i)) {
            best = other;
            best_i = other_i;
        }
        if (half == 0 && c < P.nc) {
            P.labels[c] = best_i;
            P.min_dist[c] = best;
        }
        return;
    }
    const long long ti = (long long)blockIdx.x * (RMSD_BLOCK / 64) + wave, tj = blockIdx.y;
    if (ti * 32 >= P.nr) return;
    if (EPI == RMSD_EPI_PDIST && tj < ti) return;
    rmsd_tile_products(P, ti, tj, acc);
    const long long c = tj * 32 + (lane & 31);
    const long long fc = c < P.nc ? (P.cidx ? P.cidx[c] : c) : 0;
    const double Gcol = P.C.G[fc];
#pragma unroll 1
    for (int reg = 0; reg < 16; ++reg) {
        rmsd_take(acc, reg, m, false);
        const long long r = ti * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * half;
        if (r >= P.nr || c >= P.nc) continue;
        if (EPI == RMSD_EPI_PDIST && r >= c) continue;
        const long long fr = P.ridx ? P.ridx[r] : r;
        const double d = rmsd_qcp(m, P.R.G[fr], Gcol, P.R.A);
        if (EPI == RMSD_EPI_PDIST)
            P.out[(size_t)(P.nr * r - r * (r + 1) / 2 + (c - r - 1))] = d;
        else
            P.out[(size_t)r * (size_t)P.nc + (size_t)c] = d;
    }
}

// ---- row kernel: a lane per frame (or per listed pair), nine fmaf chains -------------------------------------------------
enum { RMSD_ROW_DIST = 0, RMSD_ROW_PAIRS = 1, RMSD_ROW_KCENTERS = 2 };

struct RmsdRowArgs {
    RmsdImage X, Y;              // DIST: Y's frame yframe against X's (indexed) frames; PAIRS, KCENTERS: Y == X
    const long long* idx;        // DIST: gather of X's frames (or null); PAIRS: [n][2]
    long long n;                 // lanes with work
    long long yframe;            // DIST
    const long long* centre;     // KCENTERS: device pointer to the current centre's frame
    long long k;                 // KCENTERS: which centre this pass is
    double* out;                 // DIST, PAIRS: [n]; KCENTERS: distances_ [n]
    long long* labels;           // KCENTERS
    double* part_val;            // KCENTERS: per-workgroup first maximum of distances_ after the update
    long long* part_idx;
};

// (value, index) -> the larger value, the lower index among equals: numpy's argmax
__device__ __forceinline__ void rmsd_first_max(double& v, long long& i, double ov, long long oi)
{
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

template <int MODE>
__global__ __launch_bounds__(RMSD_BLOCK) void rmsd_row_kernel(RmsdRowArgs P)
{
    const long long i = (long long)blockIdx.x * RMSD_BLOCK + threadIdx.x;
    const bool live = i < P.n;
    double d = 0.0;
    if (live) {
        long long fx, fy;
        if (MODE == RMSD_ROW_PAIRS) {
            fx = P.idx[2 * i];
            fy = P.idx[2 * i + 1];
        } else {
            fx = P.idx ? P.idx[i] : i;
            fy = MODE == RMSD_ROW_KCENTERS ? P.centre[0] : P.yframe;
        }
        const long long A = P.X.A;
        const size_t xplane = (size_t)A * (size_t)P.X.n_pad, yplane = (size_t)A * (size_t)P.Y.n_pad;
        const float* px = P.X.T + (size_t)fx;
        const float* py = P.Y.T + (size_t)fy;
        float m[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
        for (long long a = 0; a < A; ++a) {
            float x[3], y[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                x[c] = px[c * xplane + (size_t)a * (size_t)P.X.n_pad];
                y[c] = py[c * yplane + (size_t)a * (size_t)P.Y.n_pad];
            }
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) m[3 * p + q] = fmaf(x[p], y[q], m[3 * p + q]);
        }
        if (A & 1) {   // the tile kernel's zero-padded last k-step
            const float zero = 0.0f;
#pragma unroll
            for (int q = 0; q < 9; ++q) m[q] = fmaf(zero, zero, m[q]);
        }
        d = rmsd_qcp(m, P.X.G[fx], P.Y.G[fy], A);
    }
    if (MODE != RMSD_ROW_KCENTERS) {
        if (live) P.out[i] = d;
        return;
    }
    // kcenters.py:91-97: strict running minimum of distances_ / labels_, then this workgroup's first maximum
    double v = -1.0;
    long long vi = 0x7fffffffffffffffLL;
    if (live) {
        const double old = P.k == 0 ? (double)INFINITY : P.out[i];
        const bool upd = d < old;   // false for a NaN
        v = upd ? d : old;
        vi = i;
        if (upd || P.k == 0) {
            P.out[i] = v;
            P.labels[i] = upd ? P.k : 0;
        }
    }
    __shared__ double sv[RMSD_BLOCK];
    __shared__ long long si[RMSD_BLOCK];
    sv[threadIdx.x] = v;
    si[threadIdx.x] = vi;
    __syncthreads();
    for (int w = RMSD_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            rmsd_first_max(v, vi, sv[threadIdx.x + w], si[threadIdx.x + w]);
            sv[threadIdx.x] = v;
            si[threadIdx.x] = vi;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        P.part_val[blockIdx.x] = v;
        P.part_idx[blockIdx.x] = vi;
    }
}

// one workgroup: the first maximum over the workgroups' candidates becomes centre k + 1
__global__ __launch_bounds__(RMSD_BLOCK) void rmsd_select_kernel(const double* __restrict__ part_val,
                                                                  const long long* __restrict__ part_idx, long long nparts,
                                                                  long long* __restrict__ next)
{
    double v = -1.0;
    long long vi = 0x7fffffffffffffffLL;
    for (long long p = threadIdx.x; p < nparts; p += RMSD_BLOCK) rmsd_first_max(v, vi, part_val[p], part_idx[p]);
    __shared__ double sv[RMSD_BLOCK];
    __shared__ long long si[RMSD_BLOCK];
    sv[threadIdx.x] = v;
    si[threadIdx.x] = vi;
    __syncthreads();
    for (int w = RMSD_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            rmsd_first_max(v, vi, sv[threadIdx.x + w], si[threadIdx.x + w]);
            sv[threadIdx.x] = v;
            si[threadIdx.x] = vi;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) next[0] = vi;
}

// one workgroup: sum of v[0 .. n) in a fixed order (lane t adds v[t], v[t + 256], ..., then a tree) -- no atomics, the
// same bits every run
__global__ __launch_bounds__(RMSD_BLOCK) void rmsd_ordered_sum_kernel(const double* __restrict__ v, long long n,
                                                                       double* __restrict__ out)
{
    double s = 0.0;
    for (long long p = threadIdx.x; p < n; p += RMSD_BLOCK) s = s + v[p];
    __shared__ double ss[RMSD_BLOCK];
    ss[threadIdx.x] = s;
    __syncthreads();
    for (int w = RMSD_BLOCK / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) ss[threadIdx.x] = ss[threadIdx.x] + ss[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = ss[0];
}

}  // namespace msm
