// timeseries.hip -- msm_ts_filter: the smoothers of msmbuilder.preprocessing.timeseries (Butterworth, EWMA, DoubleEWMA) over a
// list of trajectories, parallel in time (timeseries_dev.h has the recurrence and the three launches of a pass).
//
//   Butterworth  scipy.signal.filtfilt's defaults over the column reflect-padded by width - 1 rows: odd extension by
//                padlen = 3 (order + 1), forward from zi * ext[0], backward from zi * y[last], both paddings cropped.  Neither
//                padded signal exists in memory: the forward pass reads the input through two index maps.  Its float64
//                output is the one intermediate (a unit-owned buffer, at most TS_GROUP_BYTES at a time).
//   EWMA         adjust: num_t = q num_{t-1} + x_t over den_t = q den_{t-1} + 1, q = 1 - alpha (den at a segment's start comes
//                from the host in closed form); otherwise y_t = q y_{t-1} + alpha x_t from y_0 = x_0.  Rows below
//                min_periods - 1 are NaN; float64 output.
//   DoubleEWMA   (fwd + bwd) / 2 where bwd is the EWMA of the time-reversed rows, NOT reversed back (the reference's recipe).
// All arithmetic is float64 whatever the rows' type; the only rounding to the output's type is the final store.
#include "timeseries_dev.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace msm {

constexpr size_t TS_GROUP_BYTES = (size_t)2 << 30;   // float64 image of the trajectories in flight at once

static DevBuf& ts_scratch()
{
    static DevBuf b;   // the forward pass's output: this unit's own, grow-only
    return b;
}

// A^S in long double by repeated squaring; A is the recurrence's state matrix: A[k][0] = -a[k+1], A[k][k+1] = 1
static void ts_state_power(const double* a, int P, long long S, double* out)
{
    std::vector<long double> R((size_t)P * P, 0.0L), B((size_t)P * P, 0.0L), Tm((size_t)P * P);
    for (int k = 0; k < P; ++k) {
        R[(size_t)k * P + k] = 1.0L;
        B[(size_t)k * P + 0] = -(long double)a[k + 1];
        if (k + 1 < P) B[(size_t)k * P + k + 1] = 1.0L;
    }
    auto mul = [&](std::vector<long double>& X, const std::vector<long double>& Y) {   // X <- X Y
        for (int i = 0; i < P; ++i)
            for (int j = 0; j < P; ++j) {
                long double s = 0.0L;
                for (int m = 0; m < P; ++m) s += X[(size_t)i * P + m] * Y[(size_t)m * P + j];
                Tm[(size_t)i * P + j] = s;
            }
        X = Tm;
    };
    for (long long e = S; e > 0; e >>= 1) {
        if (e & 1) mul(R, B);
        if (e > 1) {
            std::vector<long double> B2 = B;
            mul(B, B2);
        }
    }
    for (int i = 0; i < P * P; ++i) out[i] = (double)R[i];
}

template <typename T, int MODE, int P>
static int ts_run_pass(const TsArgs& A, bool segmented)
{
    const unsigned grid = (unsigned)ceil_div(A.nsegs * A.F, TS_T);
    if (segmented) {
        hipLaunchKernelGGL((ts_pass<T, MODE, P, false>), dim3(grid), dim3(TS_T), 0, stream(), A);
        MSM_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL((ts_stitch<T, MODE, P>), dim3((unsigned)ceil_div(A.ntraj * A.F * 64, TS_T)), dim3(TS_T), 0, stream(), A);
        MSM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL((ts_pass<T, MODE, P, true>), dim3(grid), dim3(TS_T), 0, stream(), A);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

template <typename T, int P>
static int ts_run(TsArgs A, int kind, bool segmented)
{
    int rc;
    if (kind == MSM_TS_BUTTERWORTH) {
        if ((rc = ts_run_pass<T, TS_BW_FWD, P>(A, segmented))) return rc;
        return ts_run_pass<T, TS_BW_BWD, P>(A, segmented);
    }
    if (P == 1) {
        if ((rc = ts_run_pass<T, TS_EW_FWD, 1>(A, segmented))) return rc;
        if (kind == MSM_TS_DOUBLE_EWMA) return ts_run_pass<T, TS_EW_REV, 1>(A, segmented);
        return MSM_OK;
    }
    return fail(MSM_ERR_INVALID, "msm_ts_filter: an EWMA is an order-1 recurrence");
}

template <typename T>
static int ts_dispatch(const TsArgs& A, int P, int kind, bool segmented)
{
    switch (P) {
    case 1: return ts_run<T, 1>(A, kind, segmented);
    case 2: return ts_run<T, 2>(A, kind, segmented);
    case 3: return ts_run<T, 3>(A, kind, segmented);
    case 4: return ts_run<T, 4>(A, kind, segmented);
    default: return ts_run<T, 8>(A, kind, segmented);
    }
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_ts_filter(const void* const* X_ptrs, void* const* out_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int dtype_bytes,
                  msm_idx_t n_features, msm_idx_t ld, msm_idx_t ld_out, int on_device, int kind, int order, const double* b,
                  const double* a, const double* zi, msm_idx_t width, double alpha, int adjust, msm_idx_t min_periods,
                  msm_idx_t segment)
{
    if (n_seq < 0 || (n_seq > 0 && (!X_ptrs || !out_ptrs || !n_rows))) return fail(MSM_ERR_INVALID, "msm_ts_filter: null pointer");
    if (dtype_bytes != 4 && dtype_bytes != 8) return fail(MSM_ERR_INVALID, "dtype_bytes must be 4 or 8");
    if (n_features < 1 || n_features > INT32_MAX / 2 || ld < n_features || ld_out < n_features)
        return fail(MSM_ERR_INVALID, "msm_ts_filter: bad shape");
    if (segment < 0) return fail(MSM_ERR_INVALID, "msm_ts_filter: segment must be 0 (one per trajectory) or a number of frames");
    if (kind != MSM_TS_BUTTERWORTH && kind != MSM_TS_EWMA && kind != MSM_TS_DOUBLE_EWMA)
        return fail(MSM_ERR_INVALID, "msm_ts_filter: unknown kind %d", kind);
    const int F = (int)n_features;
    TsArgs A;
    memset(&A, 0, sizeof(A));
    int P;
    if (kind == MSM_TS_BUTTERWORTH) {
        if (order < 1 || order > TS_PMAX) return fail(MSM_ERR_INVALID, "msm_ts_filter: order %d is outside 1 .. %d", order, TS_PMAX);
        if (!b || !a || !zi) return fail(MSM_ERR_INVALID, "msm_ts_filter: null coefficients");
        if (width < 3 || width % 2 == 0) return fail(MSM_ERR_INVALID, "msm_ts_filter: width must be an odd number of frames above 2");
        if (a[0] != 1.0) return fail(MSM_ERR_INVALID, "msm_ts_filter: the denominator must be normalised (a[0] = 1)");
        for (int k = 0; k <= order; ++k)
            if (!std::isfinite(b[k]) || !std::isfinite(a[k]) || (k < order && !std::isfinite(zi[k])))
                return fail(MSM_ERR_INVALID, "msm_ts_filter: coefficients must be finite");
        P = order <= 4 ? order : TS_PMAX;   // the orders between run as order 8 with zero coefficients: the same sums
        for (int k = 0; k <= order; ++k) {
            A.b[k] = b[k];
            A.a[k] = a[k];
        }
        for (int k = 0; k < order; ++k) A.zi[k] = A.z0[k] = zi[k];
        A.w1 = width - 1;
        A.pl = 3 * (order + 1);
    } else {
        if (!(alpha > 0.0 && alpha <= 1.0)) return fail(MSM_ERR_INVALID, "msm_ts_filter: alpha must lie in (0, 1]");
        P = 1;
        const double q = 1.0 - alpha;
        A.a[0] = 1.0;
        A.a[1] = -q;
        A.adjust = adjust ? 1 : 0;
        if (adjust) {
            A.b[0] = 1.0;   // the numerator's recurrence from an empty sum; local passes start empty too (positive weights)
        } else {
            A.b[0] = alpha;
            A.zi[0] = A.z0[0] = q;   // y_0 = x_0
        }
        A.minp = min_periods;
    }
    const bool bw = kind == MSM_TS_BUTTERWORTH;
    const long long pad = bw ? 2 * (A.w1 + A.pl) : 0;
    long long longest = 0;
    for (msm_idx_t i = 0; i < n_seq; ++i) {
        if (n_rows[i] < 0 || (n_rows[i] > 0 && (!X_ptrs[i] || !out_ptrs[i])))
            return fail(MSM_ERR_INVALID, "msm_ts_filter: bad sequence %lld", (long long)i);
        if (bw && n_rows[i] < width)
            return fail(MSM_ERR_INVALID, "msm_ts_filter: sequence %lld has %lld frames and is shorter than the filter's width %lld",
                        (long long)i, (long long)n_rows[i], (long long)width);
        if (bw && n_rows[i] + 2 * A.w1 <= A.pl)
            return fail(MSM_ERR_INVALID, "The length of the input vector x must be greater than padlen, which is %lld.", A.pl);
        if (n_rows[i] + pad >= (long long)INT32_MAX * 16) return fail(MSM_ERR_INVALID, "msm_ts_filter: sequence %lld is too long", (long long)i);
        longest = std::max<long long>(longest, n_rows[i] + pad);
    }
    if (longest == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const long long S = segment > 0 ? std::min<long long>(segment, longest) : longest;
    const bool segmented = S < longest;
    A.S = S;
    A.F = F;
    if (segmented) ts_state_power(A.a, P, S, A.AS);

    int rc;
    DevBuf &dX = pool(PS_X), &dO = pool(PS_OUT), &dTab = pool(PS_IDS), &dState = pool(PS_PART), &dDen = pool(PS_PAR), &dFlag = pool(PS_SUM);
    const int out_bytes = bw ? dtype_bytes : 8;
    const size_t in_row = (size_t)F * dtype_bytes, out_row = (size_t)F * out_bytes;
    // the sum of weights in front of segment j: (1 - q^(j S)) / alpha, in long double
    const long long max_segs = ceil_div(longest, S);
    if (!bw && A.adjust) {
        std::vector<double> den((size_t)max_segs);
        const long double ql = (long double)(1.0 - alpha);   // the float64 q the recurrence multiplies by
        for (long long j = 0; j < max_segs; ++j) den[(size_t)j] = (double)((1.0L - powl(ql, (long double)(j * S))) / (long double)alpha);
        if ((rc = dDen.reserve(den.size() * sizeof(double)))) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(dDen.p, den.data(), den.size() * sizeof(double), hipMemcpyHostToDevice, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // `den` dies with this scope
        A.den0 = dDen.as<double>();
    }
    int any_bad = 0;
    msm_idx_t s = 0;
    while (s < n_seq) {
        // a group: trajectories whose float64 image fits TS_GROUP_BYTES (one at least)
        msm_idx_t e = s;
        size_t rows_ext = 0, in_bytes = 0, out_bytes_total = 0;
        while (e < n_seq && (e == s || (rows_ext + (size_t)(n_rows[e] + pad)) * F * sizeof(double) <= TS_GROUP_BYTES)) {
            rows_ext += (size_t)(n_rows[e] + pad);
            in_bytes += ((size_t)n_rows[e] * in_row + 255) & ~(size_t)255;
            out_bytes_total += ((size_t)n_rows[e] * out_row + 255) & ~(size_t)255;
            ++e;
        }
        if (!on_device) {
            if ((rc = dX.reserve(in_bytes ? in_bytes : 256))) return rc;
            if ((rc = dO.reserve(out_bytes_total ? out_bytes_total : 256))) return rc;
        }
        std::vector<TsTraj> trajs;
        std::vector<TsSeg> segs;
        std::vector<msm_idx_t> src;   // index of trajs[k] in the caller's list
        size_t in_off = 0, out_off = 0;
        long long yoff = 0;
        for (msm_idx_t i = s; i < e; ++i) {
            if (n_rows[i] == 0) continue;
            TsTraj t;
            t.n = n_rows[i];
            t.next = t.n + pad;
            t.x = X_ptrs[i];
            t.out = out_ptrs[i];
            if (!on_device) {
                char* d = dX.as<char>() + in_off;
                if (ld == F) {
                    if ((rc = h2d_bulk(d, X_ptrs[i], (size_t)t.n * in_row))) return rc;
                } else {
                    MSM_HIP_CHECK(hipMemcpy2DAsync(d, in_row, X_ptrs[i], (size_t)ld * dtype_bytes, in_row, (size_t)t.n,
                                                   hipMemcpyHostToDevice, stream()));
                }
                t.x = d;
                t.out = dO.as<char>() + out_off;
                in_off += ((size_t)t.n * in_row + 255) & ~(size_t)255;
                out_off += ((size_t)t.n * out_row + 255) & ~(size_t)255;
            }
            t.seg0 = (long long)segs.size();
            t.yoff = yoff;
            yoff += t.next;
            const long long ns = ceil_div(t.next, S);
            for (long long j = 0; j < ns; ++j) segs.push_back(TsSeg{(int)trajs.size(), (int)j});
            trajs.push_back(t);
            src.push_back(i);
        }
        if (!trajs.empty()) {
            A.ntraj = (long long)trajs.size();
            A.nsegs = (long long)segs.size();
            A.ldx = on_device ? ld : F;
            A.ldo = on_device ? ld_out : F;
            if (A.nsegs * F >= (long long)INT32_MAX * TS_T / 2 || A.ntraj * F >= (long long)INT32_MAX * TS_T / 128)
                return fail(MSM_ERR_INVALID, "msm_ts_filter: too many segments for one launch");
            const size_t tab_traj = (trajs.size() * sizeof(TsTraj) + 255) & ~(size_t)255;
            if ((rc = dTab.reserve(tab_traj + segs.size() * sizeof(TsSeg)))) return rc;
            MSM_HIP_CHECK(hipMemcpyAsync(dTab.p, trajs.data(), trajs.size() * sizeof(TsTraj), hipMemcpyHostToDevice, stream()));
            MSM_HIP_CHECK(hipMemcpyAsync(dTab.as<char>() + tab_traj, segs.data(), segs.size() * sizeof(TsSeg), hipMemcpyHostToDevice, stream()));
            A.traj = dTab.as<TsTraj>();
            A.segs = reinterpret_cast<const TsSeg*>(dTab.as<char>() + tab_traj);
            const size_t flag_bytes = sizeof(int) * ((size_t)trajs.size() * F + 1);
            if ((rc = dFlag.reserve(flag_bytes))) return rc;
            MSM_HIP_CHECK(hipMemsetAsync(dFlag.p, 0, flag_bytes, stream()));
            A.flag = dFlag.as<int>();
            A.colflag = dFlag.as<int>() + 1;
            if (segmented) {
                const size_t state = (size_t)A.nsegs * P * F;
                if ((rc = dState.reserve(2 * state * sizeof(double)))) return rc;
                A.ends = dState.as<double>();
                A.starts = dState.as<double>() + state;
            }
            if (bw) {
                if ((rc = ts_scratch().reserve((size_t)yoff * F * sizeof(double)))) return rc;
                A.yf = ts_scratch().as<double>();
            }
            rc = dtype_bytes == 4 ? ts_dispatch<float>(A, P, kind, segmented) : ts_dispatch<double>(A, P, kind, segmented);
            if (rc) return rc;
            if (!on_device) {
                for (size_t k = 0; k < trajs.size(); ++k) {
                    void* dst = out_ptrs[src[k]];
                    if (ld_out == F) {
                        if ((rc = d2h_bulk(dst, trajs[k].out, (size_t)trajs[k].n * out_row))) return rc;
                    } else {
                        MSM_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)ld_out * out_bytes, trajs[k].out, out_row, out_row, (size_t)trajs[k].n,
                                                       hipMemcpyDeviceToHost, stream()));
                    }
                }
            }
            int f = 0;
            if (!bw) MSM_HIP_CHECK(hipMemcpyAsync(&f, A.flag, sizeof(int), hipMemcpyDeviceToHost, stream()));
            MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // the tables die with this scope; the pool's slots are shared
            any_bad |= f;
        }
        s = e;
    }
    if (any_bad) return fail(MSM_ERR_NONFINITE, "Input contains NaN, infinity or a value too large");
    return MSM_OK;
}

}  // extern "C"
