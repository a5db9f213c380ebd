// timeseries_dev.h -- device side of timeseries.hip: one linear recurrence along the time axis of row-major (n, F) rows,
// parallel in time.  scipy's lfilter in transposed direct form II with state z in R^P:
//     y    = z[0] + b[0] x
//     z[k] = (z[k+1] + b[k+1] x) - a[k+1] y        (z[P] = 0)
// every product and sum rounded on its own (the unit is built with -ffp-contract=off), float64 throughout.
//
// A pass sees each trajectory as a sequence u[0 .. next) in PASS order (what that is depends on the mode, below) cut into
// segments of S elements.  Three launches, each over (trajectory, segment, column) with the column fastest so that adjacent
// lanes read adjacent columns and, where F is narrow, the lanes of a wave spread over segments:
//   ts_pass<.., false>  every segment but a trajectory's last runs from a LOCAL start state zi * u[segment start] (the
//                       filter's steady state for a constant input of that height -- see DESIGN for why not zero) and keeps
//                       its end state;
//   ts_stitch           one wave per (trajectory, column) walks the segments: the true end state of a segment is its local
//                       end state plus A^S (true start - local start), A^S formed on the host in long double;
//   ts_pass<.., true>   every segment reruns from its true start state and stores.
// With one segment per trajectory only the last launch runs, from z0 * u[0]: the recurrence serial in time.
#pragma once
#include "common.h"

namespace msm {

constexpr int TS_PMAX = 8;    // largest order served
constexpr int TS_T = 256;     // threads of a workgroup
constexpr int TS_U = 8;       // elements a thread loads before it runs them through the recurrence

enum TsMode : int {
    TS_BW_FWD = 0,   // u = the reflect-padded, odd-extended input (index maps, nothing materialised); stores float64 scratch
    TS_BW_BWD,       // u = that scratch read backwards; stores the cropped rows in the input's dtype
    TS_EW_FWD,       // u = the input; stores float64 rows
    TS_EW_REV        // u = the input read backwards; out[r] = (out[r] + v[r]) / 2: DoubleEWMA's un-reversed backward half
};

struct TsTraj {
    const void* x;      // n rows at stride ldx
    void* out;          // n rows at stride ldo
    long long n;        // frames
    long long next;     // elements of a pass: n + 2 (width - 1) + 2 padlen for Butterworth, n otherwise
    long long seg0;     // index of its first segment among all segments of the launch
    long long yoff;     // its first row in the float64 scratch
};

struct TsSeg {
    int traj, seg;
};

struct TsArgs {
    const TsTraj* traj;
    const TsSeg* segs;
    long long nsegs, ntraj;
    int F;
    long long ldx, ldo;
    long long S;            // segment length in elements of a pass
    long long w1, pl;       // Butterworth: width - 1 and padlen
    long long minp;         // EWMA: rows below minp - 1 are NaN
    int adjust;             // EWMA: divide by the running sum of weights
    double b[TS_PMAX + 1], a[TS_PMAX + 1], zi[TS_PMAX], z0[TS_PMAX];   // zero beyond the order
    double AS[TS_PMAX * TS_PMAX];                                         // A^S, P x P row-major
    double* yf;             // [rows of the group][F] forward output
    double* ends;           // [nsegs][P][F]
    double* starts;         // [nsegs][P][F]; nullptr: every trajectory is one segment
    const double* den0;     // EWMA adjust: sum of weights before a segment's first element, by segment index
    int* flag;              // EWMA: set to 1 when an element is not finite
    int* colflag;           // Butterworth: [ntraj][F], 1 where the column holds a non-finite element
};

// the reflect-padded signal p[0 .. n + 2 w1): x[w1], .., x[1], x[0], .., x[n-1], x[n-1], .., x[n-w1]
template <typename T>
__device__ __forceinline__ double ts_reflect(const T* __restrict__ x, long long ld, long long n, long long w1, long long i)
{
    const long long t = i < w1 ? w1 - i : (i < w1 + n ? i - w1 : 2 * n + w1 - 1 - i);
    return (double)x[t * ld];
}

// its odd extension by pl elements at both ends: 2 p[0] - p[pl], .., 2 p[0] - p[1], p, 2 p[M-1] - p[M-2], ..
template <typename T>
__device__ __forceinline__ double ts_extended(const T* __restrict__ x, long long ld, long long n, long long w1, long long pl,
                                              long long e)
{
    const long long M = n + 2 * w1;
    if (e < pl) return 2.0 * ts_reflect(x, ld, n, w1, 0) - ts_reflect(x, ld, n, w1, pl - e);
    e -= pl;
    if (e < M) return ts_reflect(x, ld, n, w1, e);
    return 2.0 * ts_reflect(x, ld, n, w1, M - 1) - ts_reflect(x, ld, n, w1, 2 * M - 2 - e);
}

template <typename T, int MODE>
__device__ __forceinline__ double ts_load(const TsArgs& A, const TsTraj& tr, long long e, int col)
{
    if (MODE == TS_BW_FWD) {
        const T* x = (const T*)tr.x + col;
        const long long lo = A.pl + A.w1;
        if (e >= lo && e < lo + tr.n) return (double)x[(e - lo) * A.ldx];
        return ts_extended(x, A.ldx, tr.n, A.w1, A.pl, e);
    }
    if (MODE == TS_BW_BWD) return A.yf[(tr.yoff + tr.next - 1 - e) * A.F + col];
    if (MODE == TS_EW_FWD) return (double)((const T*)tr.x)[e * A.ldx + col];
    return (double)((const T*)tr.x)[(tr.n - 1 - e) * A.ldx + col];
}

template <typename T, int MODE, int P, bool WRITE>
__global__ __launch_bounds__(TS_T) void ts_pass(const TsArgs A)
{
    const long long gid = (long long)blockIdx.x * TS_T + threadIdx.x;
    const long long g = gid / A.F;
    if (g >= A.nsegs) return;
    const int col = (int)(gid - g * A.F);
    const TsSeg sg = A.segs[g];
    const TsTraj tr = A.traj[sg.traj];
    const long long e0 = (long long)sg.seg * A.S;
    const long long e1 = e0 + A.S < tr.next ? e0 + A.S : tr.next;
    if (!WRITE && e1 == tr.next) return;   // nobody needs the end state of a trajectory's last segment
    constexpr bool EW = MODE == TS_EW_FWD || MODE == TS_EW_REV;

    double z[P];
    if (WRITE && A.starts) {
#pragma unroll
        for (int k = 0; k < P; ++k) z[k] = A.starts[((size_t)g * P + k) * A.F + col];
    } else {
        const double u0 = ts_load<T, MODE>(A, tr, e0, col);
        const double* zs = sg.seg == 0 ? A.z0 : A.zi;
#pragma unroll
        for (int k = 0; k < P; ++k) z[k] = zs[k] * u0;
    }
    double den = 0.0;
    const double q = -A.a[1];
    if (EW && A.adjust) den = A.den0[sg.seg];
    bool bad = false;
    int dead = 0;
    if (MODE == TS_BW_BWD && WRITE) dead = A.colflag[(size_t)sg.traj * A.F + col];

    for (long long e = e0; e < e1; e += TS_U) {
        const int cnt = (int)(e1 - e < TS_U ? e1 - e : TS_U);
        double u[TS_U], v[TS_U];
#pragma unroll
        for (int i = 0; i < TS_U; ++i) u[i] = i < cnt ? ts_load<T, MODE>(A, tr, e + i, col) : 0.0;
#pragma unroll
        for (int i = 0; i < TS_U; ++i) {
            if (i < cnt) {
                const double x = u[i];
                if (MODE != TS_BW_BWD) bad = bad || !(fabs(x) <= 1.79769313486231570815e308);
                const double y = z[0] + A.b[0] * x;
#pragma unroll
                for (int k = 0; k + 1 < P; ++k) z[k] = (z[k + 1] + A.b[k + 1] * x) - A.a[k + 1] * y;
                z[P - 1] = A.b[P] * x - A.a[P] * y;
                v[i] = y;
                if (EW && A.adjust) {
                    den = q * den + 1.0;
                    v[i] = y / den;
                }
            }
        }
        if (WRITE) {
#pragma unroll
            for (int i = 0; i < TS_U; ++i) {
                if (i >= cnt) continue;
                const long long r = e + i;
                if (MODE == TS_BW_FWD) {
                    A.yf[(tr.yoff + r) * A.F + col] = v[i];
                } else if (MODE == TS_BW_BWD) {
                    const long long t = tr.next - 1 - r - A.pl - A.w1;
                    if (t >= 0 && t < tr.n) ((T*)tr.out)[t * A.ldo + col] = (T)(dead ? (double)NAN : v[i]);
                } else {
                    double* o = (double*)tr.out + r * A.ldo + col;
                    const double val = r < A.minp - 1 ? (double)NAN : v[i];
                    *o = MODE == TS_EW_FWD ? val : (*o + val) / 2.0;
                }
            }
        }
    }
    if (WRITE && bad) {
        if (EW) *A.flag = 1;
        if (MODE == TS_BW_FWD) A.colflag[(size_t)sg.traj * A.F + col] = 1;
    }
    if (!WRITE) {
#pragma unroll
        for (int k = 0; k < P; ++k) A.ends[((size_t)g * P + k) * A.F + col] = z[k];
    }
}

// the value lane `lane` (wave-uniform) holds, through the scalar unit (v_readlane) rather than the LDS crossbar of __shfl
__device__ __forceinline__ double ts_broadcast(double v, int lane)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// One WAVE per (trajectory, column): the true start state of every segment, in segment order.  The chain over the segments
// is serial, its loads are not: each lane fetches what ONE segment needs (its local end state, the element at its start),
// then the chain runs over registers with lane i's values broadcast at step i and every lane doing the same arithmetic --
// one memory latency per 64 segments, and the next 64 are requested before the chain runs (a thread per chain paid one
// latency per segment: 4.6 ms per call on one trajectory of 1,000,000 x 4 against 1.9 ms).
template <typename T, int MODE, int P>
__global__ __launch_bounds__(TS_T) void ts_stitch(const TsArgs A)
{
    constexpr int W = 64;   // gfx950 runs wave64
    const long long gid = (long long)blockIdx.x * TS_T + threadIdx.x;
    const long long chain = gid / W;
    const int lane = (int)(threadIdx.x % W);
    const long long ti = chain / A.F;
    if (ti >= A.ntraj) return;   // (a whole wave at a time)
    const int col = (int)(chain - ti * A.F);
    const TsTraj tr = A.traj[ti];
    const long long nseg = (tr.next + A.S - 1) / A.S;
    double zt[P];
    {   // segment 0 starts from its true state
        const double u0 = ts_load<T, MODE>(A, tr, 0, col);
#pragma unroll
        for (int k = 0; k < P; ++k) zt[k] = A.z0[k] * u0;
    }
    // what lane `lane` needs of segment j: its local end state and the element at its start
    auto fetch = [&](long long j, double* en, double& uj) {
        uj = 0.0;
#pragma unroll
        for (int k = 0; k < P; ++k) en[k] = 0.0;
        if (j + 1 < nseg) {   // a trajectory's last segment keeps no end state
            const size_t g = (size_t)(tr.seg0 + j);
            uj = ts_load<T, MODE>(A, tr, j * A.S, col);
#pragma unroll
            for (int k = 0; k < P; ++k) en[k] = A.ends[(g * P + k) * A.F + col];
        }
    };
    double en[P], uj;
    fetch(lane, en, uj);
    for (long long j0 = 0; j0 < nseg; j0 += W) {
        const long long j = j0 + lane;
        double en_next[P], uj_next, mine[P];
        fetch(j + W, en_next, uj_next);   // requested before the chain runs over this batch: its latency hides behind it
#pragma unroll
        for (int k = 0; k < P; ++k) mine[k] = 0.0;
        const int cnt = (int)(nseg - j0 < W ? nseg - j0 : W);
        for (int i = 0; i < cnt; ++i) {   // uniform over the wave
#pragma unroll
            for (int k = 0; k < P; ++k) mine[k] = lane == i ? zt[k] : mine[k];
            if (j0 + i + 1 == nseg) break;
            const double ui = ts_broadcast(uj, i);
            const double* zs = j0 + i == 0 ? A.z0 : A.zi;   // the local start state of the segment (segment 0's is the true one)
            double d[P], zn[P];
#pragma unroll
            for (int k = 0; k < P; ++k) d[k] = zt[k] - zs[k] * ui;
#pragma unroll
            for (int k = 0; k < P; ++k) {
                double acc = ts_broadcast(en[k], i);
#pragma unroll
                for (int m = 0; m < P; ++m) acc = acc + A.AS[k * P + m] * d[m];
                zn[k] = acc;
            }
#pragma unroll
            for (int k = 0; k < P; ++k) zt[k] = zn[k];
        }
        if (j < nseg) {
            const size_t g = (size_t)(tr.seg0 + j);
#pragma unroll
            for (int k = 0; k < P; ++k) A.starts[(g * P + k) * A.F + col] = mine[k];
        }
        uj = uj_next;
#pragma unroll
        for (int k = 0; k < P; ++k) en[k] = en_next[k];
    }
}

}  // namespace msm
