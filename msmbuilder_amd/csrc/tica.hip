// tica.hip -- time-lagged second-moment accumulation for tICA on gfx950.
//
// Replaces the body of tICA._fit (/root/reference/msmbuilder/decomposition/tica.py:401-424):
//   C  += X[:-tau].T @ X[tau:]                                  (:417)
//   G  += X[:-tau].T @ X[:-tau] + X[tau:].T @ X[tau:]           (:421-422; only the sum is read, :245)
//   s0 += X[:-tau].sum(0),  stau += X[tau:].sum(0)              (:418-419)
// The reference does three float64 dgemm per trajectory; here C and G are ONE
// MFMA kernel over frame-major X (X is read as both operands: A = X^T needs no
// transpose because the MFMA A and B fragments are both k-major):
//   * C tile (I,J):  sum_t  a(t) * X[t, I]^T X[t+tau, J],  a(t) = [t < len-tau]
//   * G tile (I<=J): sum_t  w(t) * X[t, I]^T X[t, J],      w(t) = [t < len-tau] + [t >= tau]
//     (w in {0,1,2} is exact in fp32, so S0+Stau needs no head/tail correction pass;
//      the lower triangle is mirrored at export).
// Decomposition: a persistent grid of S cohorts x ntiles workgroups (<= resident
// slots, one round, no tail).  Every workgroup owns ONE 128x128 output tile for
// its whole life and walks the frame chunks c = cohort, cohort+S, ...; a chunk is
// <= 4096 frames of one trajectory, accumulated in fp32 MFMA registers and then
// merged in fp64 into the workgroup's private slab (no atomics, deterministic).
// The cohort's workgroups read the same frames at the same time and are placed on
// one XCD where possible, so the 13x panel re-read (F=512) is L2 traffic, not HBM.
#include "common.h"
#include "tica_img_dev.h"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <functional>
#include <vector>

#include "tica_plan.h"         // TicaGeom / TicaLaunch / TicaPlan and tica_plan: which kernel a launch takes, decided once
#include "tica_common_dev.h"   // constants, chunk / argument structs and block-id helpers shared by the tICA kernels
#include "tica_handle.h"       // ChunkTable, struct msm_tica; tica_export_queue, which tica_solve.hip calls
#include "tica_cg_dev.h"   // staging helpers (ChunkCtx, Stage32) and tica_mfma_f32_kernel, the fp32 C/G kernel
#include "tica_sym_dev.h"   // tica_sym_f32_kernel (sum/difference form, the bench kernel) and tica_export_sym_kernel
#include "tica_symw_dev.h"   // tica_symw_f32_kernel (sum/difference form for F <= 256: a workgroup owns all of H and D) and its export
#include "tica_f64_dev.h"   // tica_mfma_f64_kernel (fp64 MFMA)
#include "tica_img_pack_dev.h"   // tica_img_kernel (packing pre-pass of the bf16 image path) and tica_img_steps_kernel
#include "tica_colsum_dev.h"   // column sums, folded sums, mean shift and export kernels

using namespace msm;

namespace {

// Sets a kernel's dynamic-LDS limit and, with `min_slots`, folds its resident workgroups of the whole chip into a running
// minimum (the flavours of one path must all be resident in one round: the cohorts are sized by the tightest).
template <typename K>
int prep_kernel(K kernel, int threads, size_t lds, int* min_slots, int at_least = 1)
{
    MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (!min_slots) return MSM_OK;
    int occ = 0;
    MSM_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds));
    *min_slots = std::min(*min_slots, std::max(occ, at_least) * num_cus());
    return MSM_OK;
}

constexpr size_t LDS32 = 2 * 2 * BK32 * TM * sizeof(float);  // 64 KiB
constexpr size_t LDSSYM = 4 * BK32 * TM * sizeof(float) + 2 * TM * sizeof(float);  // 64 KiB: the (u, d) images for columns I and J, + 1 KiB: the shift row
constexpr int IMG_LAG = 1;                                    // tica_img_pp_kernel: load batches left in flight (tica_img_dev.h)
constexpr size_t IMG_PP_LDS = (size_t)(3 + IMG_LAG) * IMG_SLOT;  // 128 KiB: a ring of four K-steps
constexpr size_t IMG_PP_CARRY_LDS = IMG_PP_LDS + 4 * 8192;       // + the carrier waves' private 8 KiB each: all 160 KiB
constexpr size_t LDS64 = 2 * 2 * BK64 * P64 * sizeof(double);  // 72 KiB (double-buffered, pitch 144)

// variant id -> its Symw* config (tica_symw_dev.h); ids by width: tica_symw_variant
template <typename Fn>
void symw_visit(int var, Fn&& fn)
{
    switch (var) {
        case 0: fn(SymwA{}); break;
        case 1: fn(SymwB{}); break;
        case 2: fn(SymwC{}); break;
        case 3: fn(SymwD{}); break;
        case 4: fn(SymwE{}); break;
        case 6: fn(SymwG{}); break;
        case 7: fn(SymwH{}); break;
        default: fn(SymwF{}); break;
    }
}
template <typename Cfg>
constexpr bool symw_has64 = Cfg::FP <= 128;   // float64 rows: the variants of up to 128 features

int tica_zero(msm_tica* h)
{
    const TicaGeom& g = h->g;
    const size_t FF2 = 2 * (size_t)g.F * g.F + 2 * (size_t)g.F;
    MSM_HIP_CHECK(hipMemsetAsync(h->slabs, 0, (size_t)h->G * TM * TM * sizeof(double), stream()));
    if (h->slabs_sym) MSM_HIP_CHECK(hipMemsetAsync(h->slabs_sym, 0, h->sym_slab_bytes(), stream()));
    if (h->slabs_w && h->symw_used > 0)   // (only the rows a launch has touched: 512 slabs of 2 x 192 x 192 doubles are 300 MB)
        MSM_HIP_CHECK(hipMemsetAsync(h->slabs_w, 0, (size_t)h->symw_used * 2 * h->symw_FP * h->symw_FP * sizeof(double), stream()));
    h->symw_used = 0;
    MSM_HIP_CHECK(hipMemsetAsync(h->base, 0, FF2 * sizeof(double), stream()));
    MSM_HIP_CHECK(hipMemsetAsync(h->colpart, 0, h->colbytes(), stream()));
    MSM_HIP_CHECK(hipMemsetAsync(h->coltmp, 0, h->colbytes(), stream()));
    MSM_HIP_CHECK(hipMemsetAsync(h->flag, 0, 2 * sizeof(int), stream()));
    MSM_HIP_CHECK(hipMemsetAsync(h->shsum, 0, 3 * (size_t)g.F * sizeof(double), stream()));
    h->have_shift = false;
    h->slabs_dirty = false;
    h->cg_dirty = false;
    h->reduced = false;
    h->n_sh = h->nw_sh = 0;
    {
        const char* sh_env = getenv("MSM_TICA_SHIFT");  // 0: accumulate raw moments (A/B switch for the tests); read per reset
        h->g.shift_on = !(sh_env && atoi(sh_env) == 0);
    }
    h->n_obs = 0;
    h->n_seq = 0;
    return MSM_OK;
}

// ---- one accumulation launch: tica_accumulate_device sequences the steps below, each of which reads the plan -----------

struct Acc {
    msm_tica* h;
    const void* const* ptrs;
    int check_finite;
    TicaLaunch L;
    TicaPlan pl;
    TicaArgs P;                       // arguments of the MFMA kernel (the column-sum passes run on copies)
    unsigned long long key = 0;       // what the chunk tables are a function of (0: segments, no key)
    long long img_groups = 0;         // bf16 image path: 8-pair groups of the packed image (whole K-steps per chunk)
    std::vector<TicaChunk> img_tab;   // ... and its chunk table on the host (cut into ring slots)
    bool snapshot = false;            // h->snap holds the sum/difference slabs as they were before this launch
    // virtual row 0 of trajectory s (never dereferenced outside the slice: rows are clamped to [row0, last]), its last addressable row
    const void* base(long long s, const SegInfo& t) const { return (const char*)ptrs[s] - (ptrdiff_t)t.off * (ptrdiff_t)L.ld * L.dtype_bytes; }
    long long last(long long s, const SegInfo& t) const { return t.off + L.n_rows[s] - 1; }
};

// FNV-1a over the pointer / length tables and the launch's parameters (never 0)
unsigned long long table_key(const Acc& a)
{
    unsigned long long hsh = 1469598103934665603ULL;
    auto mix = [&](unsigned long long v) {
        for (int b = 0; b < 8; ++b) {
            hsh ^= (v >> (8 * b)) & 0xffULL;
            hsh *= 1099511628211ULL;
        }
    };
    mix((unsigned long long)a.L.n_seq);
    mix((unsigned long long)a.L.dtype_bytes);
    mix((unsigned long long)a.L.ld);
    mix((unsigned long long)a.pl.kc);
    mix((unsigned long long)a.h->g.lag);
    mix((unsigned long long)a.pl.bk);
    mix(a.pl.img() ? 1ULL : 0ULL);
    for (long long s = 0; s < a.L.n_seq; ++s) {
        mix((unsigned long long)(uintptr_t)a.ptrs[s]);
        mix((unsigned long long)a.L.n_rows[s]);
    }
    return hsh ? hsh : 1ULL;
}

// Appends rows [b0, b1) of one trajectory to a chunk table, `piece` rows a chunk.  `len` is the length the kernels weigh
// the rows by (1 << 60: every row counts as a left frame).  img_groups: the image path's running count of 8-pair groups.
void add_chunks(std::vector<TicaChunk>& tab, const void* base, long long last, long long b0, long long b1, long long piece,
                long long len, long long* img_groups = nullptr, int lag = 0)
{
    for (long long r0 = b0; r0 < b1; r0 += piece) {
        TicaChunk ch;
        ch.base = base;
        ch.row0 = r0;
        ch.len = len;
        ch.n = (int)std::min(piece, b1 - r0);
        ch.pad = 0;
        ch.last = last;
        ch.g0 = img_groups ? *img_groups : 0;
        if (img_groups) *img_groups += ceil_div(std::max<long long>(0, std::min<long long>(ch.n, len - lag - r0)), 32) * 4;
        tab.push_back(ch);
    }
}
constexpr long long EVERY_ROW = (long long)1 << 60;

// the launch's own chunks: none (one whole trajectory), the table of the last launch, or a new one
int main_table(Acc& a)
{
    msm_tica* h = a.h;
    const TicaPlan& pl = a.pl;
    TicaArgs& P = a.P;
    if (pl.single) {
        P.chunks = nullptr;
        P.single.base = a.ptrs[0];
        P.single.row0 = 0;
        P.single.len = a.L.n_rows[0];
        P.single.last = a.L.n_rows[0] - 1;
        P.single.n = 0;
        P.nchunks = ceil_div(a.L.n_rows[0], pl.kc);
        return MSM_OK;
    }
    if (h->table.hit(a.key, pl.total)) {   // the same trajectories as the last launch: its table is still on the device
        a.img_groups = h->table_img_groups;
        if (pl.img()) a.img_tab = h->table_host;
    } else {
        std::vector<TicaChunk> tab;
        tab.reserve((size_t)(pl.total / pl.kc + pl.nvalid + 1));
        for (long long s = 0; s < a.L.n_seq; ++s) {
            const SegInfo t = a.L.seg(s);
            if (!a.L.valid(t, h->g.lag)) continue;
            const long long own = t.oe - t.ob, nch = ceil_div(own, pl.kc);
            add_chunks(tab, a.base(s, t), a.last(s, t), t.ob, t.oe, ceil_div(ceil_div(own, nch), pl.bk) * pl.bk, t.len,
                       pl.img() ? &a.img_groups : nullptr, h->g.lag);
        }
        int rc = h->table.upload(tab, a.key, pl.total);
        if (rc) return rc;
        h->table_img_groups = a.img_groups;
        if (h->sym_units) {
            h->table_rows.resize(tab.size());
            for (size_t c = 0; c < tab.size(); ++c) h->table_rows[c] = tab[c].n;
            h->walk_key = 0;
        }
        if (pl.img()) {
            if (a.key) h->table_host = tab;
            a.img_tab.swap(tab);
        }
    }
    P.chunks = h->table.chunks();
    P.nchunks = h->table.n;
    return MSM_OK;
}

int launch_colsum(int dtype_bytes, const TicaArgs& A)
{
    if (dtype_bytes == 4)
        hipLaunchKernelGGL(tica_colsum_kernel<float>, dim3(NCB), dim3(NT), 0, stream(), A);
    else if (dtype_bytes == 2)
        hipLaunchKernelGGL(tica_colsum_kernel<__bf16>, dim3(NCB), dim3(NT), 0, stream(), A);
    else
        hipLaunchKernelGGL(tica_colsum_kernel<double>, dim3(NCB), dim3(NT), 0, stream(), A);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// Reads the non-finite flag (a host wait).  Set: the launch is rejected and the handle left as it was before it -- partials
// and flag cleared and, `undo_slabs`, the sum/difference slabs restored from the snapshot (or zeroed: nothing was in them).
int check_finite_flag(Acc& a, bool undo_slabs)
{
    msm_tica* h = a.h;
    int f[2] = {0, 0};
    MSM_HIP_CHECK(hipMemcpyAsync(f, h->flag, sizeof(f), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (!f[0]) return MSM_OK;
    if (undo_slabs) {
        if (a.snapshot)
            MSM_HIP_CHECK(hipMemcpyAsync(h->slabs_sym, h->snap.p, h->sym_slab_bytes(), hipMemcpyDeviceToDevice, stream()));
        else
            MSM_HIP_CHECK(hipMemsetAsync(h->slabs_sym, 0, h->sym_slab_bytes(), stream()));
    }
    MSM_HIP_CHECK(hipMemsetAsync(h->coltmp, 0, h->colbytes(), stream()));
    MSM_HIP_CHECK(hipMemsetAsync(h->flag, 0, sizeof(int), stream()));
    if (undo_slabs) MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return fail(MSM_ERR_NONFINITE, "Input contains NaN, infinity or a value too large");
}

// mean shift bookkeeping (fp32 / bf16 kernels): the raw column sums of what this launch accumulates under the shift, and
// -- first shifted launch of the handle, `set_r` -- the reference row r = this launch's column means; then the temporary
// partials are merged into the handle's
int shift_and_merge(Acc& a, int set_r)
{
    msm_tica* h = a.h;
    const int F = h->g.F, lag = h->g.lag;
    if (a.pl.shifted) {
        const bool segs = a.L.segs != nullptr, pairsem = a.pl.pairsem;
        long long n_call = 0, nw_call = 0, nmean = 0;
        for (long long s = 0; s < a.L.n_seq; ++s) {
            const SegInfo t = a.L.seg(s);
            if (!a.L.valid(t, lag)) continue;
            const long long n0 = std::max<long long>(0, std::min<long long>(t.oe, t.len - lag) - t.ob);
            const long long nt = std::max<long long>(0, t.oe - std::max<long long>(t.ob, lag));
            n_call += n0;
            nmean += n0 + nt;
            nw_call += (segs && !pairsem) ? n0 + nt : 2 * n0;
        }
        const int what = !segs ? (SH_A_a | SH_B_b | SH_W_ab) : pairsem ? (SH_A_a | SH_W_a) : (SH_A_a | SH_W_ab);
        hipLaunchKernelGGL(tica_shift_kernel, dim3((unsigned)ceil_div(F, 64)), dim3(512), 0, stream(), h->coltmp,
                           h->shsum, h->shift, F, 1.0 / (double)std::max<long long>(1, nmean), set_r, what);
        MSM_HIP_CHECK(hipGetLastError());
        h->have_shift = true;
        h->n_sh += n_call;
        h->nw_sh += nw_call;
    }
    const size_t n = (size_t)NCB * 2 * F;
    hipLaunchKernelGGL(tica_colmerge_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, stream(), h->colpart, h->coltmp, n);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// 1) column sums + finite check into the temporary partials
int colsum_pass(Acc& a)
{
    msm_tica* h = a.h;
    int rc = launch_colsum(a.L.dtype_bytes, a.P);
    if (rc) return rc;
    if (a.check_finite && (rc = check_finite_flag(a, false))) return rc;
    if (a.pl.shifted) a.P.shift = h->shift;
    return shift_and_merge(a, h->have_shift ? 0 : 1);
}

// 1') folded column sums, the boundary rows: [0, lag) count as left frames only (chunk length "infinite"), [len - lag, len)
//     as right frames only, so the temporary partials receive a = sum of the first rows | b = sum of the last rows
int boundary_pass(Acc& a)
{
    msm_tica* h = a.h;
    const TicaGeom& g = h->g;
    TicaArgs& P = a.P;
    int rc = MSM_OK;
    if (!h->table2.hit(a.key, a.pl.total)) {   // (else the boundary table of the same trajectories: still there)
        std::vector<TicaChunk> tab;
        for (long long s = 0; s < a.L.n_seq; ++s) {
            const long long len = a.L.n_rows[s];
            if (len <= g.lag) continue;
            add_chunks(tab, a.ptrs[s], len - 1, 0, g.lag, a.pl.kc, EVERY_ROW);
            add_chunks(tab, a.ptrs[s], len - 1, len - g.lag, len, a.pl.kc, len);
        }
        if ((rc = h->table2.upload(tab, a.key, a.pl.total))) return rc;
    }
    TicaArgs Q = P;
    Q.chunks = h->table2.chunks();
    Q.nchunks = h->table2.n;
    if ((rc = launch_colsum(a.L.dtype_bytes, Q))) return rc;
    if (a.pl.shifted) {
        if (!h->have_shift) {
            double* sp = h->fold + (size_t)g.S_sym * g.F;
            if (a.L.dtype_bytes == 4)
                hipLaunchKernelGGL(tica_fold_sample_kernel<float>, dim3((unsigned)ceil_div(g.F, 64), FOLD_NB), dim3(256), 0, stream(), P, sp);
            else
                hipLaunchKernelGGL(tica_fold_sample_kernel<__bf16>, dim3((unsigned)ceil_div(g.F, 64), FOLD_NB), dim3(256), 0, stream(), P, sp);
            hipLaunchKernelGGL(tica_fold_setr_kernel, dim3((unsigned)ceil_div(g.F, 256)), dim3(256), 0, stream(), sp, h->shift, g.F);
            MSM_HIP_CHECK(hipGetLastError());
        }
        P.shift = h->shift;
    }
    if (a.pl.img()) {
        if ((rc = h->foldimg.reserve((size_t)P.nchunks * g.F * sizeof(double)))) return rc;   // every word is written by the pre-pass
    } else {
        P.colA = h->fold;
        P.zrow = reinterpret_cast<const float*>(h->fold + (size_t)(g.S_sym + FOLD_NB) * g.F);   // zeroed at creation, never written
        MSM_HIP_CHECK(hipMemsetAsync(h->fold, 0, (size_t)g.S_sym * g.F * sizeof(double), stream()));
    }
    if (a.check_finite && h->slabs_dirty) {   // a rejected launch leaves the state untouched (utils/validation.py:68-74 raises
        if ((rc = h->snap.reserve(h->sym_slab_bytes()))) return rc;   // before tica.py:401 accumulates anything)
        MSM_HIP_CHECK(hipMemcpyAsync(h->snap.p, h->slabs_sym, h->sym_slab_bytes(), hipMemcpyDeviceToDevice, stream()));
        a.snapshot = true;
    }
    return MSM_OK;
}

// A trajectory split over ranks: the RIGHT frames of the owned pairs, rows [own_begin + lag, min(own_end, len - lag) + lag),
// are not the owned rows the column-sum pass summed -- one more pass over exactly those rows (into the temporary partials,
// which the merge has just zeroed; they are zeroed again afterwards)
int right_frames_pass(Acc& a)
{
    msm_tica* h = a.h;
    const TicaGeom& g = h->g;
    std::vector<TicaChunk> tab;
    for (long long s = 0; s < a.L.n_seq; ++s) {
        const SegInfo t = a.L.seg(s);
        if (!a.L.valid(t, g.lag)) continue;
        add_chunks(tab, a.base(s, t), a.last(s, t), t.ob + g.lag, std::min<long long>(t.oe, t.len - g.lag) + g.lag, a.pl.kc, EVERY_ROW);
    }
    if (tab.empty()) return MSM_OK;
    int rc = h->table2.upload(tab, 0, a.pl.total);
    if (rc) return rc;
    TicaArgs Q = a.P;
    Q.chunks = h->table2.chunks();
    Q.nchunks = h->table2.n;
    Q.flag = h->flag + 1;  // these rows were (or will be) checked by the launch that owns them
    if ((rc = launch_colsum(a.L.dtype_bytes, Q))) return rc;
    hipLaunchKernelGGL(tica_shift_kernel, dim3((unsigned)ceil_div(g.F, 64)), dim3(512), 0, stream(), h->coltmp, h->shsum, h->shift,
                       g.F, 0.0, 0, a.pl.pairsem ? (SH_B_a | SH_W_a) : SH_B_a);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemsetAsync(h->coltmp, 0, h->colbytes(), stream()));
    return MSM_OK;
}

// what the fused and the ring multiply kernels' arguments share, once `nsteps` is set.  The merge interval in K-steps: fp32
// partials of bf16 inputs (8 significant bits) can run 8x longer than the fp32 kernels' before the merge costs accuracy that
// matters (stated tolerance of the mode: 1e-3)
template <typename A>
void img_multiply_args(A& args, const Acc& a, bool x2)
{
    const TicaGeom& g = a.h->g;
    args.T = g.T;
    args.T2 = g.T2;
    args.ntiles_sym = a.h->slab_tiles();
    args.ntile2 = g.ntile2;
    args.S = g.S_img;
    args.main_steps = img_main_steps(args.nsteps, g.img_grid, g.ntile2);
    args.kflush_steps = std::max(1, x2 ? a.P.kflush / 16 : 8 * a.P.kflush / 32);
    args.slabs = a.h->slabs_sym;
}

// ONE launch over every K-step of the call: step records from the chunk table, then the fused kernel
int launch_img_fused(Acc& a)
{
    msm_tica* h = a.h;
    const TicaGeom& g = h->g;
    const bool x2 = a.pl.flavour & TICA_FL_X2;
    const long long nsteps = x2 ? a.img_groups / 2 : a.img_groups / 4;
    int rc = h->imgsteps.reserve((size_t)nsteps * sizeof(ImgStep));
    if (rc) return rc;
    if (h->ev0) MSM_HIP_CHECK(hipEventRecord(h->ev0, stream()));
    hipLaunchKernelGGL(tica_img_steps_kernel, dim3((unsigned)a.P.nchunks), dim3(64), 0, stream(), a.P.chunks, (long long)a.L.ld * 2, g.lag,
                       x2 ? 1 : 0, h->imgsteps.as<ImgStep>());
    MSM_HIP_CHECK(hipGetLastError());
    ImgFusedArgs FA;
    memset(&FA, 0, sizeof(FA));
    FA.steps = h->imgsteps.as<ImgStep>();
    FA.shift = a.P.shift;
    FA.row_bytes = (long long)a.L.ld * 2;
    FA.lag_bytes = (long long)g.lag * (long long)a.L.ld * 2;
    FA.nsteps = (int)nsteps;
    img_multiply_args(FA, a, x2);
    if (x2)
        hipLaunchKernelGGL((tica_img_fused_kernel<true>), dim3((unsigned)g.img_grid), dim3(IMG_NT), IMG_FUSED_LDS, stream(), FA);
    else
        hipLaunchKernelGGL((tica_img_fused_kernel<false>), dim3((unsigned)g.img_grid), dim3(IMG_NT), IMG_FUSED_LDS, stream(), FA);
    h->last_fused = 1;
    return MSM_OK;
}

struct SuperChunk {
    size_t c0, c1;      // chunks [c0, c1) of the table
    long long g0, g1;   // ... which are groups [g0, g1) of the image
};

// Cuts the chunk table (its g0 values; img_groups closes the last chunk) into super-chunks of whole chunks, as many as a
// ring slot holds: the ring of `ring_bytes` holds `nimg` images of Fp columns, whole (turns) or in halves (carried pack).
// Carried: the first one short (its pre-pass is the only one the matrix pipes wait for; rho = share of multiply steps that
// carry) but long enough to carry the second, and at most an eighth of the launch each so that short launches overlap as
// well.  `*carry` comes in as "the carried pack can run" and goes out as "it does".  False: the ring cannot hold one chunk.
bool plan_super_chunks(const std::vector<TicaChunk>& tab, long long img_groups, size_t ring_bytes, int Fp, int nimg, long long kc,
                       double rho, bool* carry, long long* slot_groups_out, std::vector<SuperChunk>* scs)
{
    const size_t gbytes = (size_t)Fp * 16;   // one 8-pair group of ONE image
    const long long max_chunk_groups = ceil_div(kc, 32) * 4;
    long long slot_groups = (long long)((*carry ? ring_bytes / 2 : ring_bytes) / (gbytes * nimg));
    slot_groups -= slot_groups % 4;
    if (*carry && (slot_groups < 2 * max_chunk_groups || img_groups <= 2 * max_chunk_groups)) {   // (nothing to take turns with)
        *carry = false;
        slot_groups = (long long)(ring_bytes / (gbytes * nimg));
        slot_groups -= slot_groups % 4;
    }
    if (slot_groups < max_chunk_groups) return false;
    long long cap = slot_groups;
    if (*carry) {
        long long want = ceil_div(ceil_div(img_groups, 8), 4) * 4;
        want = std::max<long long>(want, 4 * max_chunk_groups);
        cap = std::min(cap, want);
    }
    const long long first_cap = *carry ? std::max<long long>(max_chunk_groups, (long long)(cap * std::max(0.25, std::min(1.0, 1.15 * rho)))) : cap;
    for (size_t c0 = 0; c0 < tab.size() && img_groups > 0;) {
        const long long lim = (*carry && scs->empty()) ? first_cap : cap;
        SuperChunk sc;
        sc.c0 = c0;
        sc.g0 = tab[c0].g0;
        sc.c1 = c0;
        sc.g1 = sc.g0;
        while (sc.c1 < tab.size()) {
            const long long ge = sc.c1 + 1 < tab.size() ? tab[sc.c1 + 1].g0 : img_groups;
            if (ge - sc.g0 > lim && sc.c1 > c0) break;
            if (ge - sc.g0 > slot_groups) break;
            sc.g1 = ge;
            ++sc.c1;
        }
        scs->push_back(sc);
        c0 = sc.c1;
    }
    if (scs->size() < 2) *carry = false;
    *slot_groups_out = slot_groups;
    return true;
}

// the images of one ring half: [u_hi | d_hi | u_mid | d_mid], `one` bytes each (the mid images in bf16x2 only)
template <typename A>
void ring_images(A& args, char* half, size_t one, bool x2)
{
    args.u_hi = reinterpret_cast<bf16x8*>(half);
    args.d_hi = reinterpret_cast<bf16x8*>(half + one);
    args.u_mid = x2 ? reinterpret_cast<bf16x8*>(half + 2 * one) : nullptr;
    args.d_mid = x2 ? reinterpret_cast<bf16x8*>(half + 3 * one) : nullptr;
}

// The image is produced and consumed in SUPER-CHUNKS through a ring that the library owns (runtime.hip, img_ring):
// tica_img_kernel packs as many chunks as the ring holds, tica_img_pp_kernel multiplies them, and so on, all on stream().
// (Packing super-chunk k + 1 WHILE super-chunk k is multiplied on other CUs was built and measured and is slower than
// taking turns: the packing pass needs the whole chip's memory pipelines, 40 - 64 CUs deliver 1.0 - 1.6 TB/s)
int launch_img_ring(Acc& a)
{
    msm_tica* h = a.h;
    const TicaGeom& g = h->g;
    const TicaArgs& P = a.P;
    const int dtype_bytes = a.L.dtype_bytes;
    const long long ld = a.L.ld;
    const bool x2 = a.pl.flavour & TICA_FL_X2, fold = a.pl.fold;
    const int Fp = g.T2 * 256;
    ImgRing* ring = img_ring();
    if (!ring) return MSM_ERR_HIP;
    // The CARRIED pack (tica_img_dev.h): the multiply of super-chunk k packs super-chunk k + 1 into the other half of the
    // ring in its load role; only the first (short) super-chunk takes the pre-pass kernel.  Whole 256-feature panels of
    // 16-byte aligned rows, launches of more than one super-chunk, and few enough items per multiply step: a workgroup starts
    // a quad of items in one multiply step and converts it in the next, so rho = (quads per pack step) / (units x multiply
    // steps per pack step) is the share of its steps that carry when two consecutive super-chunks are equally long -- beyond
    // ~0.9 the drain loop would do the packing with the matrix pipes idle (float32 rows of 256 features in mode bf16).
    // Default from 1,024 features (bf16x2: 512), where it wins with the folded column sums (scripts/carryabl.py,
    // profiles/r06_carry.txt: fit of 1M x 2048 bfloat16 rows 11.1 -> 10.5 ms, bf16x2 32.8 -> 28.8 ms; 768 features 7.15 ->
    // 7.31 ms: the items' fp64 column sums cost what the overlap saves; bf16x2 has three times the multiply to hide behind --
    // 768 features 18.3 -> 16.0 ms, 512 15.4 -> 13.7 ms).  MSM_TICA_IMG_CARRY=0 restores pack / multiply turns, =1 forces it
    // at any width it can run, =2 (A/B switch of the tests): the carried pack's super-chunks and ring halves, every one
    // packed by the pre-pass kernel.
    const char* ce = getenv("MSM_TICA_IMG_CARRY");
    const int cmode = ce ? atoi(ce) : -1;
    const bool prepass_all = cmode == 2;
    const int cy_nb = Fp / (dtype_bytes == 2 ? 64 : 32);
    const double rho = 1.0 * cy_nb / (4.0 * g.ntile2 * (x2 ? 2 : 1));
    bool carry = g.F % 256 == 0 && (ld * dtype_bytes) % 16 == 0 && g.ntile2 <= g.img_grid && a.L.ptr16 && cmode != 0 &&
                 (ce || g.F >= (x2 ? 512 : 1024)) && rho <= 0.9;
    long long slot_groups = 0;
    std::vector<SuperChunk> scs;
    if (!plan_super_chunks(a.img_tab, a.img_groups, ring->bytes, Fp, x2 ? 4 : 2, a.pl.kc, rho, &carry, &slot_groups, &scs))
        return fail(MSM_ERR_INVALID, "bf16 image ring too small for %d features (MSM_TICA_IMG_RING_MB)", g.F);
    const size_t one = (size_t)slot_groups * Fp * 16;   // bytes of one image inside the ring (half)
    h->last_super = (long long)scs.size();
    if (h->ev0) MSM_HIP_CHECK(hipEventRecord(h->ev0, stream()));
    if (carry) {
        // the launch's 32-pair step records (the table the fused kernel uses, with this launch's row size)
        int rc = h->imgsteps.reserve((size_t)(a.img_groups / 4) * sizeof(ImgStep));
        if (rc) return rc;
        hipLaunchKernelGGL(tica_img_steps_kernel, dim3((unsigned)P.nchunks), dim3(64), 0, stream(), P.chunks, ld * dtype_bytes, g.lag, 0,
                           h->imgsteps.as<ImgStep>());
        MSM_HIP_CHECK(hipGetLastError());
        if (fold) {
            long long np_max = 0;
            for (const SuperChunk& sc : scs) np_max = std::max(np_max, (sc.g1 - sc.g0) / 4);
            if ((rc = h->colsteps.reserve((size_t)np_max * Fp * sizeof(double)))) return rc;
        }
    }
    for (size_t k = 0; k < scs.size(); ++k) {
        const SuperChunk& sc = scs[k];
        char* const half = ring->p + ((carry && (k & 1)) ? ring->bytes / 2 : 0);
        if (!carry || k == 0 || prepass_all) {
            ImgArgs IA;
            memset(&IA, 0, sizeof(IA));
            IA.chunks = P.chunks + sc.c0;
            IA.nchunks = (long long)(sc.c1 - sc.c0);
            IA.ld = ld;
            IA.F = g.F;
            IA.Fp = Fp;
            IA.lag = g.lag;
            IA.dtype_bytes = dtype_bytes;
            IA.shift = P.shift;
            IA.colA = fold ? h->foldimg.as<double>() + sc.c0 * (size_t)g.F : nullptr;
            IA.g_off = sc.g0;
            ring_images(IA, half, one, x2);
            const dim3 g1((unsigned)(sc.c1 - sc.c0), (unsigned)g.T2);
            if (x2)
                hipLaunchKernelGGL(tica_img_kernel<true>, g1, dim3(256), 0, stream(), IA);
            else
                hipLaunchKernelGGL(tica_img_kernel<false>, g1, dim3(256), 0, stream(), IA);
            MSM_HIP_CHECK(hipGetLastError());
        }
        ImgMfmaArgs MA;
        memset(&MA, 0, sizeof(MA));
        ring_images(MA, half, one, x2);
        MA.nsteps = x2 ? (sc.g1 - sc.g0) / 2 : (sc.g1 - sc.g0) / 4;
        MA.Fp = Fp;
        img_multiply_args(MA, a, x2);
        const bool carries = carry && !prepass_all && k + 1 < scs.size();
        if (carries) {
            const SuperChunk& nx = scs[k + 1];
            MA.cy.psteps = h->imgsteps.as<ImgStep>() + nx.g0 / 4;
            MA.cy.shift = P.shift;
            ring_images(MA.cy, ring->p + ((k & 1) ? 0 : ring->bytes / 2), one, x2);
            MA.cy.colS = fold ? h->colsteps.as<double>() : nullptr;
            MA.cy.row_bytes = ld * dtype_bytes;
            MA.cy.lag_bytes = (long long)g.lag * ld * dtype_bytes;
            MA.cy.np = (int)((nx.g1 - nx.g0) / 4);
            MA.cy.nb = cy_nb;
            // a workgroup's multiply steps / its quads (every workgroup multiplies ~ nsteps x units / grid steps)
            const long long wsteps = MA.nsteps * g.ntile2 / g.img_grid;
            const long long wquads = ceil_div(ceil_div((long long)MA.cy.np * cy_nb, 4), g.img_grid);
            MA.cy.stride = (int)std::max<long long>(1, wsteps / std::max<long long>(1, wquads));
            {
                const char* ae = getenv("MSM_TICA_IMG_CARRY_ABL");   // timing ablations only (tica_img_dev.h, img_carry_phase)
                MA.cy.pad = ae ? atoi(ae) : 0;
            }
            h->last_carried = 1;
        }
#define MSM_IMG_PP_LAUNCH(X2_, CY_) \
        hipLaunchKernelGGL((tica_img_pp_kernel<X2_, IMG_LAG, false, 0, CY_>), dim3((unsigned)g.img_grid), dim3(IMG_NT), (CY_) ? IMG_PP_CARRY_LDS : IMG_PP_LDS, stream(), MA)
        if (!carries) {
            if (x2) MSM_IMG_PP_LAUNCH(true, 0);
            else MSM_IMG_PP_LAUNCH(false, 0);
        } else if (dtype_bytes == 2) {
            if (x2) MSM_IMG_PP_LAUNCH(true, 2);
            else MSM_IMG_PP_LAUNCH(false, 2);
        } else {
            if (x2) MSM_IMG_PP_LAUNCH(true, 4);
            else MSM_IMG_PP_LAUNCH(false, 4);
        }
#undef MSM_IMG_PP_LAUNCH
        MSM_HIP_CHECK(hipGetLastError());
        if (carries && fold) {
            const SuperChunk& nx = scs[k + 1];
            hipLaunchKernelGGL(tica_img_colsum_steps_kernel, dim3((unsigned)(nx.c1 - nx.c0), (unsigned)ceil_div(g.F, 256)), dim3(256), 0, stream(),
                               P.chunks + nx.c0, (long long)(nx.c1 - nx.c0), nx.g0, nx.g1, h->colsteps.as<double>(), g.F, Fp,
                               h->foldimg.as<double>() + nx.c0 * (size_t)g.F);
            MSM_HIP_CHECK(hipGetLastError());
        }
    }
    return MSM_OK;
}

// whole-matrix sum/difference kernel, float or double rows: the handle's variant, or the element-wise SymwA for rows too
// short for a 16-byte piece
int launch_symw(Acc& a)
{
    msm_tica* h = a.h;
    SymwArgs WA;
    WA.T = a.P;
    WA.slabs = h->slabs_w;
    const dim3 grid(a.pl.G);
    const bool f64 = a.pl.path == TICA_SYMW64;
    if (!(a.pl.flavour & TICA_FL_VEC)) {
        if (f64) hipLaunchKernelGGL((tica_symw_f64_kernel<SymwA, false>), grid, dim3(SymwA::NTH), SymwA::LDS64, stream(), WA);
        else hipLaunchKernelGGL((tica_symw_f32_kernel<SymwA, false>), grid, dim3(SymwA::NTH), SymwA::LDS, stream(), WA);
    } else {
        symw_visit(h->g.symw_var, [&](auto cfg) {
            using Cfg = decltype(cfg);
            if (!f64) hipLaunchKernelGGL((tica_symw_f32_kernel<Cfg, true>), grid, dim3(Cfg::NTH), Cfg::LDS, stream(), WA);
            else if constexpr (symw_has64<Cfg>) hipLaunchKernelGGL((tica_symw_f64_kernel<Cfg, true>), grid, dim3(Cfg::NTH), Cfg::LDS64, stream(), WA);
        });
    }
    h->symw_used = std::max(h->symw_used, (int)std::min<long long>(a.pl.G, a.P.nchunks));
    return MSM_OK;
}

// a packed handle's chunk walks (tica_sym_walk) for this launch's chunks: the last launch's when they are the same
int sym_walk(Acc& a)
{
    msm_tica* h = a.h;
    const TicaPlan& pl = a.pl;
    if (!(a.key && h->walk_key == a.key && h->walk_total == pl.total && h->walk_kflush == pl.kflush)) {
        std::vector<int> single;
        if (pl.single) {
            const long long len = a.L.n_rows[0];
            for (long long r0 = 0; r0 < len; r0 += pl.kc) single.push_back((int)std::min<long long>(pl.kc, len - r0));
        }
        const std::vector<int>& rows = pl.single ? single : h->table_rows;
        if ((long long)rows.size() != a.P.nchunks) return fail(MSM_ERR_STATE, "sum/difference launch: %lld chunks, rows of %lld", a.P.nchunks, (long long)rows.size());
        std::vector<int> w;
        tica_sym_walk(rows.data(), (long long)rows.size(), h->sym_cohorts_unpacked, h->g.sym_cohorts, pl.kc, pl.kflush, w);
        h->walk_key = 0;
        int rc = h->walk.reserve(w.size() * sizeof(int));
        if (rc) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(h->walk.p, w.data(), w.size() * sizeof(int), hipMemcpyHostToDevice, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // `w` is pageable host memory
        h->walk_key = a.key;
        h->walk_total = pl.total;
        h->walk_kflush = pl.kflush;
    }
    a.P.walk = static_cast<const int*>(h->walk.p);
    return MSM_OK;
}

int launch_sym(Acc& a)
{
    const dim3 grid(a.pl.G);
    TicaArgs& P = a.P;
#define MSM_SYM_LAUNCH(...) hipLaunchKernelGGL((tica_sym_f32_kernel<__VA_ARGS__>), grid, dim3(NT), LDSSYM, stream(), P); break
    if (a.h->sym_units) {   // a packed handle: full tiles, no remainder cohort -- the plan's flavour is folded or plain
        P.units = a.h->sym_units;   // (P.walk: set by sym_walk ahead of the timed launch)
        switch (a.pl.flavour) {
            case TICA_FL_FOLD: MSM_SYM_LAUNCH(false, true, false, true);
            case 0: MSM_SYM_LAUNCH(false, false, false, true);
            default: return fail(MSM_ERR_STATE, "sum/difference launch: flavour %d on a packed handle", a.pl.flavour);
        }
        return MSM_OK;
    }
    switch (a.pl.flavour) {
        case TICA_FL_FOLD | TICA_FL_REM: MSM_SYM_LAUNCH(false, true, true);
        case TICA_FL_REM: MSM_SYM_LAUNCH(false, false, true);
        case TICA_FL_EDGE | TICA_FL_REM: MSM_SYM_LAUNCH(true, false, true);
        case TICA_FL_FOLD: MSM_SYM_LAUNCH(false, true);
        case 0: MSM_SYM_LAUNCH(false, false);
        default: MSM_SYM_LAUNCH(true, false);
#undef MSM_SYM_LAUNCH
    }
    return MSM_OK;
}

int launch_cg32(Acc& a)
{
    const dim3 grid(a.pl.G);
    const TicaArgs& P = a.P;
    if (a.pl.flavour == TICA_FL_ALIGNED)
        hipLaunchKernelGGL((tica_mfma_f32_kernel<true, false>), grid, dim3(NT), LDS32, stream(), P);
    else if (a.pl.flavour & TICA_FL_ALIGNED)
        hipLaunchKernelGGL((tica_mfma_f32_kernel<true, true>), grid, dim3(NT), LDS32, stream(), P);
    else
        hipLaunchKernelGGL((tica_mfma_f32_kernel<false, true>), grid, dim3(NT), LDS32, stream(), P);
    return MSM_OK;
}

int launch_cg64(Acc& a)
{
    if (a.L.dtype_bytes == 4)
        hipLaunchKernelGGL(tica_mfma_f64_kernel<float>, dim3(a.pl.G), dim3(NT), LDS64, stream(), a.P);
    else
        hipLaunchKernelGGL(tica_mfma_f64_kernel<double>, dim3(a.pl.G), dim3(NT), LDS64, stream(), a.P);
    return MSM_OK;
}

// 3') folded column sums: temporary partials -> [left sums | right sums] per slot, finite check of the folded sums (a
//     rejected launch is undone: the slabs as they were, nothing of it in the column sums or the shift), shift and merge
int fold_fixup(Acc& a)
{
    msm_tica* h = a.h;
    const TicaGeom& g = h->g;
    const dim3 grid((unsigned)ceil_div((size_t)NCB * g.F, 256));
    if (a.pl.img())
        hipLaunchKernelGGL(tica_fold_fix_img_kernel, grid, dim3(256), 0, stream(), h->coltmp, h->foldimg.as<double>(), g.F, a.P.nchunks, h->flag);
    else
        hipLaunchKernelGGL(tica_fold_fix_kernel, grid, dim3(256), 0, stream(), h->coltmp, h->fold, g.F, g.S_sym, h->flag);
    MSM_HIP_CHECK(hipGetLastError());
    int rc = MSM_OK;
    if (a.check_finite && (rc = check_finite_flag(a, true))) return rc;
    return shift_and_merge(a, 0);
}

int env_switch(const char* name)   // an integer switch of the environment: -1 unset (or negative), else its value
{
    const char* e = getenv(name);
    return e ? std::max(-1, atoi(e)) : -1;
}

// Device-resident trajectories only.  The sequencer: validate and count, plan, chunk table, column sums or boundary pass,
// extra pass for segments, the MFMA launch of the plan's path, after_launch, folded fix-up and check, bookkeeping.
// after_launch: host work to run once the accumulation kernel is queued and before this call's first wait for it (the
// staged host path copies its NEXT group of trajectories there)
int tica_accumulate_device(msm_tica* h, const void* const* ptrs, const msm_idx_t* n_rows,
                           msm_idx_t n_seq, int dtype_bytes, msm_idx_t ld, int check_finite,
                           msm_idx_t* n_skipped, const SegInfo* segs = nullptr, const std::function<int()>* after_launch = nullptr)
{
    const TicaGeom& g = h->g;
    Acc a{h, ptrs, check_finite};
    TicaLaunch& L = a.L;
    L.dtype_bytes = dtype_bytes;
    L.ld = ld;
    L.n_seq = n_seq;
    L.n_rows = n_rows;
    L.segs = segs;
    L.dims4 = (g.F % 4 == 0) && (ld % 4 == 0);
    long long skipped = 0;
    for (msm_idx_t s = 0; s < n_seq; ++s) {
        const SegInfo t = L.seg(s);
        if (((uintptr_t)ptrs[s]) & 15) L.ptr16_all = false;
        if (L.valid(t, g.lag)) {
            if (((uintptr_t)ptrs[s]) & 15) L.ptr16 = false;
        } else if (t.len <= g.lag) {
            ++skipped;
        }
    }
    if (n_skipped) *n_skipped = skipped;
    L.fold_switch = env_switch("MSM_TICA_FOLD");   // read per launch (A/B switches of the tests); 0 = never, 2 = always
    {
        const char* fe = getenv("MSM_TICA_IMG_FUSED");   // 1 forces the fused kernel, any other value the image ring
        L.fused_switch = fe ? (atoi(fe) == 1 ? 1 : 0) : -1;
    }
    const TicaPlan& pl = a.pl = tica_plan(g, L);
    if (pl.nvalid == 0) return MSM_OK;
    h->reduced = false;

    TicaArgs& P = a.P;
    memset(&P, 0, sizeof(P));
    P.ld = ld;
    P.kc = (int)pl.kc;
    P.F = g.F;
    P.lag = g.lag;
    P.T = g.T;
    P.ntiles = pl.sym_slabs() ? g.ntiles_sym : g.ntiles;
    P.slab_tiles = h->slab_tiles();
    P.S = pl.S;
    P.slabs = pl.sym_slabs() ? h->slabs_sym : h->slabs;
    P.colpart = h->coltmp;
    P.flag = h->flag;
    P.dbg = h->dbg;
    P.kflush = pl.kflush;
    P.cosync = pl.pace ? h->cosync : nullptr;
    if (!segs) a.key = table_key(a);
    int rc = main_table(a);
    if (rc) return rc;
    P.n_main = pl.n_main(P.nchunks);
    if (pl.path == TICA_SYM && h->sym_units && (rc = sym_walk(a))) return rc;
    h->last_plan = pl;
    h->last_nchunks = P.nchunks;
    h->last_super = 0;

    if ((rc = pl.fold ? boundary_pass(a) : colsum_pass(a))) return rc;
    if (pl.shifted && segs && (rc = right_frames_pass(a))) return rc;
    // 2) the MFMA pass
    MSM_HIP_CHECK(hipMemsetAsync(h->cosync, 0, (size_t)(std::max(h->S, g.S_sym) + 1) * sizeof(unsigned), stream()));
    if (!pl.img() && h->ev0) MSM_HIP_CHECK(hipEventRecord(h->ev0, stream()));   // (image paths: recorded around the whole pipeline)
    h->last_fused = 0;
    h->last_carried = 0;
    switch (pl.path) {
        case TICA_IMG_FUSED:   // (a launch of more K-steps than an int counts goes through the ring)
            rc = a.img_groups > 0 && a.img_groups / 2 < 0x7fffffffLL ? launch_img_fused(a) : launch_img_ring(a);
            break;
        case TICA_IMG_RING: rc = launch_img_ring(a); break;
        case TICA_SYMW:
        case TICA_SYMW64: rc = launch_symw(a); break;
        case TICA_SYM: rc = launch_sym(a); break;
        case TICA_CG32: rc = launch_cg32(a); break;
        default: rc = launch_cg64(a); break;
    }
    if (rc) return rc;
    MSM_HIP_CHECK(hipGetLastError());
    if (h->ev1) {
        MSM_HIP_CHECK(hipEventRecord(h->ev1, stream()));
        h->timed = true;
    }
    if (after_launch) {
        const int rch = (*after_launch)();
        if (rch) return rch;
    }
    if (pl.fold && (rc = fold_fixup(a))) return rc;
    if (pl.sym_slabs()) h->slabs_dirty = true;
    else if (!pl.symw()) h->cg_dirty = true;
    h->last_folded = pl.fold;
    for (msm_idx_t s = 0; s < n_seq; ++s) {
        const SegInfo t = L.seg(s);
        if (L.valid(t, g.lag)) {
            h->n_obs += t.oe - t.ob;       // summed over the ranks sharing a trajectory this is its length
            h->n_seq += (t.ob == 0) ? 1 : 0;  // ... and the rank owning row 0 counts the sequence
        }
    }
    return MSM_OK;
}

}  // namespace

// queues slabs / column partials / base -> h->packed (raw moments, un-shifted); no synchronisation (tica_handle.h)
int msm::tica_export_queue(msm_tica* h)
{
    const size_t total = 2 * (size_t)h->g.F * h->g.F + 2 * (size_t)h->g.F;
    hipLaunchKernelGGL(tica_export_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, stream(),
                       h->slabs, h->colpart, h->base, h->packed, h->g.F, h->g.T, h->g.ntiles, h->cg_dirty ? h->S : 0);
    hipLaunchKernelGGL(tica_export_cols_kernel, dim3((unsigned)ceil_div(2 * (int64_t)h->g.F, 64)), dim3(256), 0, stream(), h->colpart, h->base,
                       h->packed, h->g.F);
    MSM_HIP_CHECK(hipGetLastError());
    if (h->g.sym && h->slabs_sym) {
        hipLaunchKernelGGL(tica_export_sym_kernel, dim3((unsigned)ceil_div((size_t)h->slab_tiles() * TM * TM, 256)), dim3(256), 0, stream(),
                           h->slabs_sym, h->packed, h->g.F, h->g.T, h->slab_tiles(), h->g.S_sym);
        MSM_HIP_CHECK(hipGetLastError());
    }
    if (h->symw_used > 0) {
        hipLaunchKernelGGL(tica_export_symw_kernel, dim3((unsigned)ceil_div((size_t)h->g.F * h->g.F, 256)), dim3(256), 0, stream(),
                           h->slabs_w, h->packed, h->g.F, h->symw_FP, h->symw_W, h->symw_IL, h->symw_used);
        MSM_HIP_CHECK(hipGetLastError());
    }
    if (h->have_shift) {  // restore the raw moments from the shifted ones (fp64)
        const size_t ff2 = 2 * (size_t)h->g.F * h->g.F;
        hipLaunchKernelGGL(tica_unshift_kernel, dim3((unsigned)ceil_div(ff2, 256)), dim3(256), 0, stream(), h->packed,
                           h->shsum, h->shift, (double)h->n_sh, (double)h->nw_sh, h->g.F, h->g.sym);
        MSM_HIP_CHECK(hipGetLastError());
    }
    return MSM_OK;
}

namespace {

int tica_export_device(msm_tica* h)
{
    const size_t total = 2 * (size_t)h->g.F * h->g.F + 2 * (size_t)h->g.F;
    const int rcq = tica_export_queue(h);
    if (rcq) return rcq;
    const double cnt[2] = {(double)h->n_obs, (double)h->n_seq};
    MSM_HIP_CHECK(hipMemcpyAsync(h->packed + total, cnt, sizeof(cnt), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

}  // namespace

// whole-matrix sum/difference kernel: the variant of the width, its kernels' resident workgroups (float rows, and
// float64 rows up to 128 features unless MSM_TICA_SYMW64=0: the same variant on doubles, the same slabs)
static int create_symw(msm_tica* h)
{
    TicaGeom& g = h->g;
    g.symw_var = tica_symw_variant(g.F);
    int rc = MSM_OK, slots = INT_MAX, slots64 = INT_MAX;
    const char* e64 = getenv("MSM_TICA_SYMW64");   // (A/B switch of the tests)
    const bool want64 = g.F <= 128 && !(e64 && atoi(e64) == 0);
    symw_visit(g.symw_var, [&](auto cfg) {
        using Cfg = decltype(cfg);
        h->symw_FP = Cfg::FP;
        h->symw_W = Cfg::W;
        h->symw_IL = Cfg::IL;
        g.symw_KS = Cfg::KS;
        // rows of 1-3 floats (a single double) go element by element through SymwA
        if (g.F >= 4) rc = prep_kernel(tica_symw_f32_kernel<Cfg, true>, Cfg::NTH, Cfg::LDS, &slots);
        else rc = prep_kernel(tica_symw_f32_kernel<SymwA, false>, SymwA::NTH, SymwA::LDS, &slots);
        if constexpr (symw_has64<Cfg>) {
            if (rc || !want64) return;
            if (g.F >= 2) rc = prep_kernel(tica_symw_f64_kernel<Cfg, true>, Cfg::NTH, Cfg::LDS64, &slots64, 0);
            else rc = prep_kernel(tica_symw_f64_kernel<SymwA, false>, SymwA::NTH, SymwA::LDS64, &slots64, 0);
        }
    });
    if (rc) return rc;
    if (slots64 != INT_MAX && slots64 >= 1) {   // (a variant that is not resident on doubles leaves them to the fp64 C/G kernel)
        g.symw64 = 1;
        g.symw_S64 = slots64;
    }
    g.symw_S = slots;
    g.symw = 1;
    g.sym = 1;   // the exported lagged moment is the symmetrised one
    return MSM_OK;
}

// symmetric fp32 kernel (H/D blocks of the upper tiles): two 64-KiB workgroups per CU
static int create_sym(msm_tica* h)
{
    TicaGeom& g = h->g;
    int rc = MSM_OK, slots = INT_MAX;
    if ((rc = prep_kernel(tica_sym_f32_kernel<false, false>, NT, LDSSYM, &slots))) return rc;
    if ((rc = prep_kernel(tica_sym_f32_kernel<true, false>, NT, LDSSYM, &slots))) return rc;
    if ((rc = prep_kernel(tica_sym_f32_kernel<false, true>, NT, LDSSYM, &slots))) return rc;
    if ((rc = prep_kernel(tica_sym_f32_kernel<false, false, true>, NT, LDSSYM, &slots))) return rc;
    if ((rc = prep_kernel(tica_sym_f32_kernel<true, false, true>, NT, LDSSYM, &slots))) return rc;
    if ((rc = prep_kernel(tica_sym_f32_kernel<false, true, true>, NT, LDSSYM, &slots))) return rc;
    if ((rc = prep_kernel(tica_sym_f32_kernel<false, false, false, true>, NT, LDSSYM, &slots))) return rc;
    if ((rc = prep_kernel(tica_sym_f32_kernel<false, true, false, true>, NT, LDSSYM, &slots))) return rc;
    g.sym_cohorts = slots / g.ntiles_sym;
    g.sym = g.sym_cohorts >= 1;  // at least one whole cohort resident (F <= 3968 on 256 CUs), else the C/G kernel
    // remainder cohort: the slots beyond the whole cohorts, when they are worth a launch flavour of their own --
    // at least a sixteenth of the chip and at most three rounds over the tiles (2,048 features: 104 of 512 slots,
    // two rounds; 512 features: 2 slots, not worth it)
    const int R = slots - g.sym_cohorts * g.ntiles_sym;
    const bool rem = g.sym && R * 16 >= slots && 3 * R >= g.ntiles_sym;
    g.sym_grid = rem ? slots : g.sym_cohorts * g.ntiles_sym;
    g.S_sym = g.sym_cohorts + (rem ? 1 : 0);
    // Packed diagonal blocks (tica_sym_units.h): full tiles, no remainder cohort before or after, and only where the fewer
    // workgroups per cohort buy a cohort -- on 512 slots F = 512 (51 -> 56 cohorts), 640 (34 -> 36), 768 (24 -> 25) and
    // 1024 (14 -> 15).  The geometry says it through ntiles_sym (workgroups per cohort) and what follows from it; the plan
    // does not know.  MSM_TICA_SYM_PACK=0 (read here, A/B switch of the tests and of scripts/ablate.py): never.
    const char* pack_env = getenv("MSM_TICA_SYM_PACK");
    const int up = sym_units_per_cohort(g.T, true), rp = slots - slots / up * up;
    const bool rem_packed = rp * 16 >= slots && 3 * rp >= up;
    if (g.sym && g.F % TM == 0 && !(pack_env && atoi(pack_env) == 0) && !rem && !rem_packed && slots / up > g.sym_cohorts) {
        const std::vector<SymUnit> units = tica_sym_units(g.T, true);
        MSM_HIP_CHECK(hipMalloc((void**)&h->sym_units, units.size() * sizeof(SymUnit)));
        MSM_HIP_CHECK(hipMemcpyAsync(h->sym_units, units.data(), units.size() * sizeof(SymUnit), hipMemcpyHostToDevice, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // `units` is pageable host memory
        h->sym_cohorts_unpacked = g.sym_cohorts;
        g.ntiles_sym = up;
        g.sym_cohorts = slots / up;
        g.sym_grid = g.sym_cohorts * up;
        g.S_sym = g.sym_cohorts;
    }
    return MSM_OK;
}

// bf16 image path (256 x 256 tiles of H and D on the upper triangle, one 8-wave workgroup per CU)
static int create_img(msm_tica* h)
{
    TicaGeom& g = h->g;
    int rc = MSM_OK;
    if ((rc = prep_kernel(tica_img_pp_kernel<false, IMG_LAG>, IMG_NT, IMG_PP_LDS, nullptr))) return rc;
    if ((rc = prep_kernel(tica_img_pp_kernel<true, IMG_LAG>, IMG_NT, IMG_PP_LDS, nullptr))) return rc;
    if ((rc = prep_kernel(tica_img_pp_kernel<false, IMG_LAG, false, 0, 2>, IMG_NT, IMG_PP_CARRY_LDS, nullptr))) return rc;
    if ((rc = prep_kernel(tica_img_pp_kernel<true, IMG_LAG, false, 0, 2>, IMG_NT, IMG_PP_CARRY_LDS, nullptr))) return rc;
    if ((rc = prep_kernel(tica_img_pp_kernel<false, IMG_LAG, false, 0, 4>, IMG_NT, IMG_PP_CARRY_LDS, nullptr))) return rc;
    if ((rc = prep_kernel(tica_img_pp_kernel<true, IMG_LAG, false, 0, 4>, IMG_NT, IMG_PP_CARRY_LDS, nullptr))) return rc;
    if ((rc = prep_kernel(tica_img_fused_kernel<false>, IMG_NT, IMG_FUSED_LDS, nullptr))) return rc;
    if ((rc = prep_kernel(tica_img_fused_kernel<true>, IMG_NT, IMG_FUSED_LDS, nullptr))) return rc;
    if (!img_ring()) return MSM_ERR_HIP;   // the process's image ring exists before any fit is timed
    g.img_on = 1;
    g.img_grid = std::max(num_cus(), g.ntile2);   // one workgroup per CU: whole cohorts + a remainder cohort (tica_img_dev.h)
    g.S_img = g.img_grid / g.ntile2;
    g.sym = 1;                 // the exported lagged moment is the symmetrised one
    g.S_sym = g.S_img + 1;     // slab rows: the cohorts' and the remainder cohort's
    g.sym_cohorts = g.S_img;
    return MSM_OK;
}

// what a handle is made of: the kernels' resident slots -> cohorts per path (one resident round per launch)
static int create_geometry(msm_tica* h)
{
    TicaGeom& g = h->g;
    g.T = (int)ceil_div(g.F, TM);
    g.ntiles = g.T * g.T + g.T * (g.T + 1) / 2;
    g.T2 = (int)ceil_div(g.F, 256);
    g.ntile2 = g.T2 * (g.T2 + 1);
    int rc = MSM_OK, slots32 = INT_MAX, slots64 = INT_MAX;
    if ((rc = prep_kernel(tica_mfma_f32_kernel<true, false>, NT, LDS32, &slots32))) return rc;
    if ((rc = prep_kernel(tica_mfma_f32_kernel<true, true>, NT, LDS32, &slots32))) return rc;
    if ((rc = prep_kernel(tica_mfma_f32_kernel<false, true>, NT, LDS32, &slots32))) return rc;
    if ((rc = prep_kernel(tica_mfma_f64_kernel<float>, NT, LDS64, &slots64))) return rc;
    if ((rc = prep_kernel(tica_mfma_f64_kernel<double>, NT, LDS64, &slots64))) return rc;
    g.S32 = std::max(1, slots32 / g.ntiles);
    g.S64 = std::max(1, slots64 / g.ntiles);
    // MSM_TICA_SYM=0 (raw lagged moment wanted) leaves the C/G kernels in charge; MSM_TICA_SYMW=0 (A/B switch of the tests)
    // the 128-wide sum/difference kernel where the whole-matrix one (fp32 mode, F <= 256) would run
    const char* sym_env = getenv("MSM_TICA_SYM");
    const char* symw_env = getenv("MSM_TICA_SYMW");
    const bool sym_off = sym_env && atoi(sym_env) == 0, symw_off = symw_env && atoi(symw_env) == 0;
    constexpr int tmax = 64;  // and one resident cohort must fit (create_sym)
    if (g.mode == MSM_TICA_F32 && !sym_off && !symw_off && g.F <= 256) {
        rc = create_symw(h);
    } else {
        g.ntiles_sym = g.T * (g.T + 1) / 2;
        if (g.mode == MSM_TICA_F32 && !sym_off && g.T >= 2 && g.T <= tmax && g.F % 4 == 0) rc = create_sym(h);
    }
    if (rc) return rc;
    if ((g.mode == MSM_TICA_BF16 || g.mode == MSM_TICA_BF16X2) && g.ntile2 <= num_cus()) rc = create_img(h);
    return rc;
}

extern "C" {

int msm_tica_create(msm_tica_t** out, msm_idx_t n_features, msm_idx_t lag_time, int mode)
{
    if (!out) return fail(MSM_ERR_INVALID, "msm_tica_create: null handle pointer");
    if (n_features < 1 || n_features > (1 << 15)) return fail(MSM_ERR_INVALID, "n_features=%lld out of range", (long long)n_features);
    if (lag_time < 1) return fail(MSM_ERR_INVALID, "lag_time must be >= 1");
    if (mode < MSM_TICA_F32 || mode > MSM_TICA_BF16X2) return fail(MSM_ERR_INVALID, "unknown tica mode %d", mode);
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    msm_tica* h = new msm_tica();
    TicaGeom& g = h->g;
    g.F = (int)n_features;
    g.lag = (int)lag_time;
    g.mode = mode;
    g.shift_on = 1;
    int rc = create_geometry(h);
    if (rc) {
        if (h->sym_units) (void)hipFree(h->sym_units);
        delete h;
        return rc;
    }
    h->S = std::max(g.S32, g.S64);  // slabs exist for the largest; unused ones stay zero
    h->G = h->S * g.ntiles;
    const size_t FF2 = 2 * (size_t)g.F * g.F + 2 * (size_t)g.F;
    const size_t wb = (size_t)g.symw_S * 2 * h->symw_FP * h->symw_FP * sizeof(double);
    const size_t foldb = (size_t)(g.S_sym + FOLD_NB + 1) * g.F * sizeof(double);
    hipError_t e = hipSuccess;
    auto alloc = [&](auto** p, size_t bytes) {
        if (e == hipSuccess) e = hipMalloc((void**)p, bytes);
    };
    alloc(&h->slabs, (size_t)h->G * TM * TM * sizeof(double));
    if (g.sym && !g.symw) alloc(&h->slabs_sym, h->sym_slab_bytes());
    if (g.symw) {
        alloc(&h->slabs_w, wb);
        if (e == hipSuccess) e = hipMemsetAsync(h->slabs_w, 0, wb, stream());   // (once: a reset zeroes only the rows a launch has used)
    }
    alloc(&h->base, FF2 * sizeof(double));
    alloc(&h->colpart, h->colbytes());
    alloc(&h->coltmp, h->colbytes());
    alloc(&h->packed, (FF2 + 2) * sizeof(double));
    alloc(&h->flag, 2 * sizeof(int));
    alloc(&h->dbg, 64 * sizeof(long long));
    alloc(&h->cosync, (size_t)(std::max(h->S, g.S_sym) + 1) * sizeof(unsigned));
    alloc(&h->shift, (size_t)g.F * sizeof(float));
    alloc(&h->shsum, 3 * (size_t)g.F * sizeof(double));
    if (g.sym) alloc(&h->fold, foldb);
    if (e == hipSuccess) e = hipEventCreate(&h->ev0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev1);
    if (e != hipSuccess) {
        msm_tica_destroy(h);
        return fail(MSM_ERR_HIP, "msm_tica_create: hipMalloc failed: %s", hipGetErrorString(e));
    }
    g.have_fold = h->fold != nullptr;
    if (h->fold) (void)hipMemsetAsync(h->fold, 0, foldb, stream());
    rc = tica_zero(h);
    if (rc) {
        msm_tica_destroy(h);
        return rc;
    }
    *out = h;
    return MSM_OK;
}

int msm_tica_destroy(msm_tica_t* h)
{
    if (!h) return MSM_OK;
    (void)hipStreamSynchronize(stream());
    for (void* p : {(void*)h->slabs, (void*)h->slabs_sym, (void*)h->slabs_w, (void*)h->base, (void*)h->colpart, (void*)h->coltmp,
                    (void*)h->packed, (void*)h->flag, (void*)h->dbg, (void*)h->cosync, (void*)h->shift, (void*)h->shsum, (void*)h->fold,
                    (void*)h->sym_units})
        if (p) (void)hipFree(p);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    if (h->solve_pin) (void)hipHostFree(h->solve_pin);
    delete h;
    return MSM_OK;
}

int msm_tica_reset(msm_tica_t* h)
{
    if (!h) return fail(MSM_ERR_STATE, "null tica handle");
    return tica_zero(h);
}

static int tica_accumulate_any(msm_tica_t* h, const void* const* X_ptrs, const msm_idx_t* n_rows,
                               msm_idx_t n_seq, int dtype_bytes, msm_idx_t ld, int on_device,
                               int check_finite, msm_idx_t* n_skipped, const SegInfo* segs)
{
    if (!h) return fail(MSM_ERR_STATE, "null tica handle");
    if (n_seq < 0 || (n_seq > 0 && (!X_ptrs || !n_rows))) return fail(MSM_ERR_INVALID, "bad sequence table");
    if (dtype_bytes != 4 && dtype_bytes != 8 && dtype_bytes != 2) return fail(MSM_ERR_INVALID, "dtype_bytes must be 2 (bfloat16), 4 or 8");
    if (dtype_bytes == 2 && !h->g.img_on)
        return fail(MSM_ERR_INVALID, "bfloat16 trajectories need MSM_TICA_BF16 / MSM_TICA_BF16X2 mode (got mode %d)", h->g.mode);
    if (ld < h->g.F) return fail(MSM_ERR_INVALID, "ld=%lld < n_features=%d", (long long)ld, h->g.F);
    for (msm_idx_t s = 0; s < n_seq; ++s)
        if (n_rows[s] < 0 || (n_rows[s] > 0 && !X_ptrs[s])) return fail(MSM_ERR_INVALID, "bad sequence %lld", (long long)s);
    if (n_skipped) *n_skipped = 0;
    if (n_seq == 0) return MSM_OK;
    if (on_device) return tica_accumulate_device(h, X_ptrs, n_rows, n_seq, dtype_bytes, ld, check_finite, n_skipped, segs);

    // host trajectories: staged in groups (compacted to ld = F) through the two halves of a device buffer.  The copies of
    // group g + 1 are issued right after the accumulation kernel of group g is queued (tica_accumulate_device's
    // after_launch hook), on the copy stream, so the PCIe transfer runs beside the kernel instead of in front of it
    // (round 5: 42.4 -> 50.0 GB/s on the bench's h2d_inclusive leg, 4.1 GB in 82 ms: 68 ms of copies + 1.6 ms per group of
    // launch / check / merge that the host cannot copy beside; pinned -> device alone delivers 56-57 GB/s here:
    // profiles/r05_h2d_rate.txt).  The Python layer hands a materialised list down whole for this reason.
    const size_t row_bytes = (size_t)h->g.F * dtype_bytes;
    const size_t budget = (size_t)512 << 20;
    struct Group {
        msm_idx_t s = 0, e = 0;
        std::vector<const void*> dptrs;
    };
    auto plan = [&](msm_idx_t s0) {   // the group that starts at trajectory s0
        Group g;
        g.s = g.e = s0;
        size_t bytes = 0;
        while (g.e < n_seq && (g.e == g.s || bytes + (size_t)n_rows[g.e] * row_bytes <= budget)) {
            bytes += ((size_t)n_rows[g.e] * row_bytes + 255) & ~(size_t)255;
            ++g.e;
        }
        return std::make_pair(g, bytes);
    };
    // capacity: the largest group (a single trajectory may exceed the budget), twice
    size_t half = 256;
    for (msm_idx_t s0 = 0; s0 < n_seq;) {
        auto pg = plan(s0);
        half = std::max(half, pg.second);
        s0 = pg.first.e;
    }
    half = (half + 255) & ~(size_t)255;
    int rc = h->staging.reserve(2 * half);
    if (rc) return rc;
    // copies of one group into half `which`; `first`: ordered after the work already queued on the library stream (the
    // buffer's previous reader), later groups: their half's last reader has been waited for by the host already
    auto copy_group = [&](Group& g, int which, bool first) -> int {
        g.dptrs.assign((size_t)(g.e - g.s), nullptr);
        size_t off = 0;
        for (msm_idx_t i = g.s; i < g.e; ++i) {
            char* d = h->staging.as<char>() + (size_t)which * half + off;
            g.dptrs[(size_t)(i - g.s)] = d;
            if (n_rows[i] > 0) {
                if (ld == h->g.F) {
                    int rcb = h2d_bulk(d, X_ptrs[i], (size_t)n_rows[i] * row_bytes, first);
                    if (rcb) return rcb;
                } else {
                    MSM_HIP_CHECK(hipMemcpy2DAsync(d, row_bytes, X_ptrs[i], (size_t)ld * dtype_bytes, row_bytes,
                                                   (size_t)n_rows[i], hipMemcpyHostToDevice, stream()));
                }
            }
            off += ((size_t)n_rows[i] * row_bytes + 255) & ~(size_t)255;
        }
        return MSM_OK;
    };
    msm_idx_t skipped_total = 0;
    Group cur = plan(0).first, nxt;
    int which = 0;
    if ((rc = copy_group(cur, which, true))) return rc;
    while (cur.s < n_seq) {
        const bool more = cur.e < n_seq;
        if (more) nxt = plan(cur.e).first;
        const std::function<int()> hook = [&]() -> int { return copy_group(nxt, which ^ 1, false); };
        msm_idx_t sk = 0;
        rc = tica_accumulate_device(h, cur.dptrs.data(), n_rows + cur.s, cur.e - cur.s, dtype_bytes, h->g.F, check_finite, &sk,
                                    segs ? segs + cur.s : nullptr, more ? &hook : nullptr);
        if (rc) {
            (void)hipStreamSynchronize(stream());   // (copies of the next group may be in flight into the staging buffer)
            return rc;
        }
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));  // this half is rewritten by the group after the next
        skipped_total += sk;
        if (!more) break;
        if (nxt.dptrs.empty() && (rc = copy_group(nxt, which ^ 1, false))) return rc;   // (the call returned before its kernel: nothing valid in the group)
        cur = std::move(nxt);
        nxt = Group();
        which ^= 1;
    }
    if (n_skipped) *n_skipped = skipped_total;
    return MSM_OK;
}

int msm_tica_accumulate_batch(msm_tica_t* h, const void* const* X_ptrs, const msm_idx_t* n_rows,
                              msm_idx_t n_seq, int dtype_bytes, msm_idx_t ld, int on_device,
                              int check_finite, msm_idx_t* n_skipped)
{
    return tica_accumulate_any(h, X_ptrs, n_rows, n_seq, dtype_bytes, ld, on_device, check_finite, n_skipped, nullptr);
}

int msm_tica_accumulate_segments(msm_tica_t* h, const void* const* X_ptrs, const msm_idx_t* n_rows,
                                 const msm_idx_t* seg4, msm_idx_t n_seq, int dtype_bytes, msm_idx_t ld,
                                 int on_device, int check_finite, msm_idx_t* n_skipped)
{
    if (!h) return fail(MSM_ERR_STATE, "null tica handle");
    if (n_seq < 0 || (n_seq > 0 && (!X_ptrs || !n_rows || !seg4))) return fail(MSM_ERR_INVALID, "bad segment table");
    std::vector<SegInfo> segs((size_t)n_seq);
    for (msm_idx_t s = 0; s < n_seq; ++s) {
        SegInfo g;
        g.len = seg4[4 * s + 0];
        g.off = seg4[4 * s + 1];
        g.ob = seg4[4 * s + 2];
        g.oe = seg4[4 * s + 3];
        if (g.len < 0 || g.off < 0 || n_rows[s] < 0 || g.off + n_rows[s] > g.len)
            return fail(MSM_ERR_INVALID, "segment %lld: slice [%lld, %lld) is not inside a trajectory of %lld rows",
                        (long long)s, (long long)g.off, (long long)(g.off + n_rows[s]), (long long)g.len);
        if (g.oe > g.ob) {
            const long long need = (g.oe + h->g.lag < g.len ? g.oe + h->g.lag : g.len);  // right halo
            if (g.ob < g.off || need > g.off + n_rows[s])
                return fail(MSM_ERR_INVALID, "segment %lld: owned rows [%lld, %lld) + lag %d need rows [%lld, %lld) but the slice holds [%lld, %lld)",
                            (long long)s, (long long)g.ob, (long long)g.oe, h->g.lag, (long long)g.ob, need,
                            (long long)g.off, (long long)(g.off + n_rows[s]));
        }
        segs[(size_t)s] = g;
    }
    return tica_accumulate_any(h, X_ptrs, n_rows, n_seq, dtype_bytes, ld, on_device, check_finite, n_skipped, segs.data());
}

int msm_tica_accumulate(msm_tica_t* h, const void* X, int dtype_bytes, msm_idx_t n_rows,
                        msm_idx_t ld, int on_device, int check_finite, int* skipped)
{
    msm_idx_t sk = 0;
    const void* ptrs[1] = {X};
    int rc = msm_tica_accumulate_batch(h, ptrs, &n_rows, 1, dtype_bytes, ld, on_device, check_finite, &sk);
    if (skipped) *skipped = (int)sk;
    return rc;
}

int msm_tica_nonfinite(msm_tica_t* h, int* flag)
{
    if (!h || !flag) return fail(MSM_ERR_STATE, "null argument");
    int f[2];
    MSM_HIP_CHECK(hipMemcpyAsync(f, h->flag, sizeof(f), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    *flag = f[0];
    return MSM_OK;
}

int msm_tica_lagged_symmetrised(msm_tica_t* h, int* flag)
{
    if (!h || !flag) return fail(MSM_ERR_STATE, "null argument");
    *flag = h->g.sym ? 1 : 0;
    return MSM_OK;
}

int msm_tica_last_kernel_ms(msm_tica_t* h, float* ms)
{
    if (!h || !ms) return fail(MSM_ERR_STATE, "null argument");
    if (!h->timed) return fail(MSM_ERR_STATE, "no accumulation launch recorded yet");
    MSM_HIP_CHECK(hipEventSynchronize(h->ev1));
    MSM_HIP_CHECK(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return MSM_OK;
}

int msm_tica_last_folded(msm_tica_t* h, int* flag)
{
    if (!h || !flag) return fail(MSM_ERR_STATE, "null argument");
    *flag = h->last_folded ? 1 : 0;
    return MSM_OK;
}

int msm_tica_plan(const int* geom, int dtype_bytes, msm_idx_t ld, const msm_idx_t* n_rows, msm_idx_t n_seq, int ptr_aligned16,
                  int dims_aligned4, int fold_switch, int fused_switch, long long* out)
{
    if (!geom || !out || n_seq < 0 || (n_seq > 0 && !n_rows)) return fail(MSM_ERR_INVALID, "msm_tica_plan: bad argument");
    TicaGeom g;
    memcpy(&g, geom, sizeof(g));
    if (!tica_geom_valid(g)) return fail(MSM_ERR_INVALID, "msm_tica_plan: not a handle's geometry");
    TicaLaunch L;
    L.dtype_bytes = dtype_bytes;
    L.ld = ld;
    L.n_seq = n_seq;
    L.n_rows = n_rows;
    L.ptr16 = (ptr_aligned16 & 1) != 0;
    L.ptr16_all = (ptr_aligned16 & 2) != 0;
    L.dims4 = dims_aligned4 != 0;
    L.fold_switch = fold_switch;
    L.fused_switch = fused_switch;
    tica_plan_ints(tica_plan(g, L), out);
    return MSM_OK;
}

int msm_tica_sym_units(int T, int pack, int* out, int cap)
{
    if (T < 1 || T > 256 || cap < 0 || (cap > 0 && !out)) return fail(MSM_ERR_INVALID, "msm_tica_sym_units: bad argument");
    const std::vector<SymUnit> units = tica_sym_units(T, pack != 0);
    const size_t n = std::min(units.size(), (size_t)cap);
    if (n) memcpy(out, units.data(), n * sizeof(SymUnit));
    return (int)units.size();
}

int msm_tica_sym_walk(const int* chunk_rows, msm_idx_t n_chunks, int S0, int S, msm_idx_t kc, msm_idx_t kflush, int* out, msm_idx_t cap)
{
    if (n_chunks < 0 || n_chunks >= 0x7fffffff || (n_chunks > 0 && !chunk_rows) || S0 < 1 || S < 1 || kc < 1 || kflush < 1 || !out ||
        cap < (msm_idx_t)S + 1 + n_chunks)
        return fail(MSM_ERR_INVALID, "msm_tica_sym_walk: bad argument");
    std::vector<int> w;
    const bool kept = tica_sym_walk(chunk_rows, n_chunks, S0, S, kc, kflush, w);
    std::copy(w.begin(), w.end(), out);
    return kept ? 1 : 0;
}

int msm_tica_last_plan(msm_tica_t* h, long long* out)
{
    if (!h || !out) return fail(MSM_ERR_INVALID, "msm_tica_last_plan: null argument");
    int gi[TICA_GEOM_INTS];
    memcpy(gi, &h->g, sizeof(gi));
    std::copy(gi, gi + TICA_GEOM_INTS, out);
    tica_plan_ints(h->last_plan, out + TICA_GEOM_INTS);
    out[TICA_GEOM_INTS + TICA_PLAN_INTS] = h->last_nchunks;
    out[TICA_GEOM_INTS + TICA_PLAN_INTS + 1] = h->last_super;
    return MSM_OK;
}

int msm_tica_last_img_carried(msm_tica_t* h, int* flag)
{
    if (!h || !flag) return fail(MSM_ERR_INVALID, "msm_tica_last_img_carried: null argument");
    *flag = h->last_carried;
    return MSM_OK;
}

int msm_tica_last_img_fused(msm_tica_t* h, int* flag)
{
    if (!h || !flag) return fail(MSM_ERR_INVALID, "msm_tica_last_img_fused: null argument");
    *flag = h->last_fused;
    return MSM_OK;
}

int msm_tica_debug_clocks(msm_tica_t* h, long long* out4)
{
    if (!h || !out4) return fail(MSM_ERR_STATE, "null argument");
    MSM_HIP_CHECK(hipMemcpyAsync(out4, h->dbg, 4 * sizeof(long long), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_tica_debug_profile(msm_tica_t* h, long long* out64)
{
    if (!h || !out64) return fail(MSM_ERR_STATE, "null argument");
    MSM_HIP_CHECK(hipMemcpyAsync(out64, h->dbg, 64 * sizeof(long long), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

msm_idx_t msm_tica_packed_size(msm_tica_t* h) { return h ? (msm_idx_t)h->packed_len() : 0; }

int msm_tica_export_packed(msm_tica_t* h, double* buf, int on_device)
{
    if (!h || !buf) return fail(MSM_ERR_STATE, "null argument");
    int rc = tica_export_device(h);
    if (rc) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(buf, h->packed, h->packed_len() * sizeof(double),
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_tica_import_packed(msm_tica_t* h, const double* buf, int on_device)
{
    if (!h || !buf) return fail(MSM_ERR_STATE, "null argument");
    const size_t FF2 = 2 * (size_t)h->g.F * h->g.F + 2 * (size_t)h->g.F;
    int rc = tica_zero(h);
    if (rc) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(h->base, buf, FF2 * sizeof(double),
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
    double cnt[2];
    MSM_HIP_CHECK(hipMemcpyAsync(cnt, buf + FF2, sizeof(cnt),
                                 on_device ? hipMemcpyDeviceToHost : hipMemcpyHostToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    h->n_obs = (long long)(cnt[0] + 0.5);
    h->n_seq = (long long)(cnt[1] + 0.5);
    return MSM_OK;
}

int msm_tica_export(msm_tica_t* h, double* C, double* G, double* s0, double* stau,
                    msm_idx_t* n_observations, msm_idx_t* n_sequences)
{
    if (!h) return fail(MSM_ERR_STATE, "null tica handle");
    int rc = tica_export_device(h);
    if (rc) return rc;
    const size_t FF = (size_t)h->g.F * h->g.F;
    if (C) MSM_HIP_CHECK(hipMemcpyAsync(C, h->packed, FF * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if (G) MSM_HIP_CHECK(hipMemcpyAsync(G, h->packed + FF, FF * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if (s0) MSM_HIP_CHECK(hipMemcpyAsync(s0, h->packed + 2 * FF, h->g.F * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if (stau) MSM_HIP_CHECK(hipMemcpyAsync(stau, h->packed + 2 * FF + h->g.F, h->g.F * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (n_observations) *n_observations = h->n_obs;
    if (n_sequences) *n_sequences = h->n_seq;
    return MSM_OK;
}

int msm_tica_import(msm_tica_t* h, const double* C, const double* G, const double* s0,
                    const double* stau, msm_idx_t n_observations, msm_idx_t n_sequences)
{
    if (!h || !C || !G || !s0 || !stau) return fail(MSM_ERR_STATE, "null argument");
    int rc = tica_zero(h);
    if (rc) return rc;
    const size_t FF = (size_t)h->g.F * h->g.F;
    MSM_HIP_CHECK(hipMemcpyAsync(h->base, C, FF * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(h->base + FF, G, FF * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(h->base + 2 * FF, s0, h->g.F * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(h->base + 2 * FF + h->g.F, stau, h->g.F * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    h->n_obs = n_observations;
    h->n_seq = n_sequences;
    return MSM_OK;
}

int msm_tica_counts(msm_tica_t* h, msm_idx_t* n_observations, msm_idx_t* n_sequences)
{
    if (!h) return fail(MSM_ERR_STATE, "null tica handle");
    if (n_observations) *n_observations = h->n_obs;
    if (n_sequences) *n_sequences = h->n_seq;
    return MSM_OK;
}

/* one all-reduce of the packed accumulators over the library communicator, device to device */
int msm_tica_allreduce(msm_tica_t* h)
{
    if (!h) return fail(MSM_ERR_STATE, "null tica handle");
    if (!comm_active()) return MSM_OK;
    int rc = tica_export_device(h);  // h->packed = [C | G | s0 | stau | n_obs | n_seq], raw (un-shifted) moments
    if (rc) return rc;
    if ((rc = comm_allreduce_f64(h->packed, h->packed_len()))) return rc;
    return msm_tica_import_packed(h, h->packed, 1);  // resets the local state, keeps the reduced sums as the base
}

/* s0 / stau alone (F doubles each, host): the column sums without the F x F moments */
int msm_tica_export_sums(msm_tica_t* h, double* s0, double* stau)
{
    if (!h || !s0 || !stau) return fail(MSM_ERR_STATE, "null argument");
    return msm_tica_export(h, nullptr, nullptr, s0, stau, nullptr, nullptr);
}

}  // extern "C"
