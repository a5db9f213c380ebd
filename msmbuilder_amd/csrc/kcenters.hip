// kcenters.hip -- the host side of the k-centers fits for gfx950: the single-process fit, the externally driven passes and
// the row-sharded fit.  The kernels are the distance_*_dev.h families; this file chooses between them and queues them.
//
// Replaces the k-pass loop of the reference (msmbuilder/cluster/kcenters.py:91-97).  The arithmetic is libdistance's
// (distance.hip's bit-exactness contract; this file is compiled with -ffp-contract=off too).
// A fit runs ONE loop, a function of its own: the single fit kc_run_plain, kc_run_narrow_screen or kc_run_wide_screen
// (both screens end in batched rounds -- several centres per pass -- or in one centre per pass), the sharded fit
// kcs_run_batched, kcs_run_fused or kcs_run_generic.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "distance_host.h"          // row_vecw, wide_ok, launch_wide, pad_rows, sum_partials_host; kcenters_pass_kernel, wide_kernel
#include "distance_kcsel_dev.h"     // kc_finalize / kc_candidate / kc_select kernels: the argmax exchange of the k-centers loops
#include "distance_screen_dev.h"    // kcenters_screen_pass_kernel, ksc_convert_kernel: k-centers passes screened on a low-precision copy
#include "distance_kcbatch_dev.h"   // kcb_* kernels: several centres per pass (threshold lists), single GPU and row-sharded
#include "distance_wscreen_dev.h"   // kcenters_wscreen_pass_kernel: screened passes of wide rows / float32 rows on a feature-major byte copy
#include "distance_wbatch_dev.h"    // kwb_*: several centres per screened pass of wide rows (threshold lists)

namespace msm {

// a pass goes to the wide-row kernel (on a grid of at most one resident round: kc_wide_cut), else to kcenters_pass_kernel
template <typename T>
static bool kc_is_wide(const KcArgs& P) { return P.vecw == 0 && wide_ok<T>(P.X, P.ycenter ? P.ycenter : P.X, P.m, false); }
template <typename T>
static int kc_wide_cut(int nblk, const KcArgs& P) { return kc_is_wide<T>(P) ? std::min(nblk, wide_grid(P.n)) : nblk; }

template <typename T>
void launch_kc(int metric, int grid, const KcArgs& P)
{
    const bool wide = kc_is_wide<T>(P);
    WideArgs A;
    memset(&A, 0, sizeof(A));
    A.kc = P;
    metric_visit(metric, [&](auto mm) {
        constexpr int MM = decltype(mm)::value;
        if (wide)
            launch_wide<T, MM, 2>(grid, A);
        else if (P.vecw > 0)
            hipLaunchKernelGGL((kcenters_pass_kernel<T, MM, true>), dim3(grid), dim3(DT), 0, stream(), P);
        else
            hipLaunchKernelGGL((kcenters_pass_kernel<T, MM, false>), dim3(grid), dim3(DT), 0, stream(), P);
    });
}

template <typename T, int JB, int R, int U>
static void launch_kwb(int grid, size_t lds, const KwsArgs& A, KcbState* St)
{
    static bool attr_set = false;
    if (!attr_set) {   // up to 64 KiB of centres beside the kernel's own ~40 KiB
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kwb_pass_kernel<T, JB, R, U>), hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
        attr_set = true;
    }
    hipLaunchKernelGGL((kwb_pass_kernel<T, JB, R, U>), dim3(grid), dim3(DT), lds, stream(), A, St);
}

// deterministic per-block fp64 sums of a vector (inertia = np.sum(distances_))
__global__ __launch_bounds__(DT) void sum_partial_kernel(const double* __restrict__ v, long long n,
                                                         double* __restrict__ partial)
{
    __shared__ double red[DT];
    double s = 0.0;
    for (long long i = (long long)blockIdx.x * DT + threadIdx.x; i < n; i += (long long)gridDim.x * DT) s += v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = DT / 2; k > 0; k >>= 1) {
        if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// out[k][:] = X[ids[k]][:] -- the chosen rows themselves (cluster_centers_), gathered on the device so that they travel
// with the ids in the fit's one final synchronisation (torch indexing with a Python list is three round trips)
template <typename T>
__global__ void kc_gather_centres_kernel(const T* __restrict__ X, long long m, const msm_idx_t* __restrict__ ids, T* __restrict__ out)
{
    const msm_idx_t row = ids[blockIdx.x];
    for (long long f = threadIdx.x; f < m; f += blockDim.x) out[(size_t)blockIdx.x * m + f] = X[(size_t)row * m + f];
}

// centre 0 of a sharded fit: the rank that owns the seed row publishes it through the same record exchange
template <typename T>
__global__ __launch_bounds__(DT) void kc_seed_candidate_kernel(const T* __restrict__ X, long long m, long long local_row,
                                                               long long global_row, double* __restrict__ cand)
{
    if (threadIdx.x == 0) {
        cand[0] = local_row >= 0 ? 1.0 : -1.0;
        cand[1] = local_row >= 0 ? (double)global_row : -1.0;
    }
    for (long long f = threadIdx.x; f < m; f += DT) cand[2 + f] = local_row >= 0 ? (double)X[local_row * m + f] : 0.0;
}

// what the last k-centers fit streamed (for bench.py's bytes-per-pass figure): pass counts and the bytes a pass reads per row
struct KcStats {
    long long rows = 0, plain_passes = 0, screened_passes = 0, plain_row_bytes = 0, screen_row_bytes = 0, batch_fallbacks = 0;
    long long wide_candidates = 0, wide_updates = 0;   // wide screened passes: rows re-evaluated exactly / rows that changed
};
static KcStats g_kc_stats;

template <typename T>
static void kc_stats_begin(long long n, long long m)
{
    g_kc_stats = KcStats();
    g_kc_stats.rows = n;
    g_kc_stats.plain_row_bytes = (long long)(m * sizeof(T) + 16);   // the row, distances_, labels_ (pruning test)
}

// The MSM_KC_* switches of the fits: A/B switches of the tests and scripts.  Read at the top of EVERY fit and never kept --
// the tests flip them between fits of one process.
struct KcSwitches {
    bool batch;         // MSM_KC_BATCH=0: one centre per screened pass / per exchange
    bool wscreen;       // MSM_KC_WSCREEN=0: no screen on the byte copy
    int wbatch;         // MSM_KC_WBATCH: 0 one centre per screened pass of wide rows, other values the batches; -1 (unset): by row length
    bool wselect_one;   // MSM_KC_WSELECT=1: the wide batches' selector on one workgroup
    bool stats;         // MSM_KC_STATS=1: read the wide screen's candidate counters back (diagnostics: scripts/kcwide.py)
};
static KcSwitches kc_switches()
{
    const auto is = [](const char* name, int value) { const char* v = getenv(name); return v && atoi(v) == value; };
    KcSwitches sw;
    sw.batch = !is("MSM_KC_BATCH", 0);
    sw.wscreen = !is("MSM_KC_WSCREEN", 0);
    sw.wbatch = !getenv("MSM_KC_WBATCH") ? -1 : is("MSM_KC_WBATCH", 0) ? 0 : 1;
    sw.wselect_one = is("MSM_KC_WSELECT", 1);
    sw.stats = is("MSM_KC_STATS", 1);
    return sw;
}

static int kc_blocks(long long n) { return (int)std::min<long long>(ceil_div(std::max<long long>(n, 1), DT), KC_MAXBLK); }

// The two partial arrays of a single fit: pass (or round) `step` writes one and reads the other, which the step before it
// wrote.  They lie nblk0 apart -- the block count BEFORE the wide-grid cut, the stride the buffer was sized for --,
// whatever grid a pass runs on: the screened passes of wide rows run on grids of their own, larger than the cut one.
struct KcParts {
    KcPartial* base;
    int nblk0;
    KcPartial* next(long long step) const { return base + (size_t)(step & 1) * nblk0; }
    const KcPartial* prev(long long step) const { return next(step + 1); }
    template <typename Args> void aim(Args& A, long long step) const { A.prev = prev(step), A.next = next(step); }
};

// np = 1 .. 8 (pairs of features of a narrow float64 row) -> fn(std::integral_constant<int, np>)
template <int NP = 1, typename Fn>
static void ksc_np_visit(int np, Fn&& fn)
{
    if (np == NP) fn(std::integral_constant<int, NP>{});
    else if constexpr (NP < 8) ksc_np_visit<NP + 1>(np, fn);
}

// The screen copy in use is FMT 2 (bytes + a row scale); the float32 / bfloat16 formats of the kernels' FMT parameter were
// measured in round 3 and are no longer instantiated.
constexpr int KSC_FMT = 2;

struct KscBufs {
    DevBuf xf, curf, misc;
};
static KscBufs& ksc_bufs() { static KscBufs b; return b; }

static int ksc_np(long long m) { return (int)((m + 1) / 2); }
static long long ksc_row_bytes(long long m) { return (long long)(ksc_words(ksc_np(m), KSC_FMT) * 4 + 4); }   // the screen copy's row + curf

// Opens the narrow screen copy of the fit whose plain passes run on P: reserves it, zeroes its header and fills the screened
// kernels' arguments (`ids`: the fit's centres; `exchange`: the passes select and record in-kernel, as the fused sharded
// loop's do).  The copy itself is written by ksc_queue_copy, once the fit's first centre is fixed.
static int ksc_open(const KcArgs& P, long long seed, msm_idx_t* ids, bool exchange, KscArgs* S)
{
    KscBufs& B = ksc_bufs();
    int rc;
    if ((rc = B.misc.reserve(64 + 16 * sizeof(double)))) return rc;  // [gmax2[2] | ... | c0[16]]
    if ((rc = B.xf.reserve((size_t)P.n * (ksc_words(ksc_np(P.m), KSC_FMT) + 1) * sizeof(float)))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(B.misc.p, 0, 64, stream()));
    memset(S, 0, sizeof(*S));
    S->X = static_cast<const double*>(P.X);
    S->xs = B.xf.p;
    S->gmax2 = B.misc.as<unsigned long long>();
    S->c0 = reinterpret_cast<double*>(static_cast<char*>(B.misc.p) + 64);
    S->n = P.n;
    S->m = P.m;
    S->nblk = P.nblk;
    S->vecw = P.vecw;
    S->seed = seed;
    S->next = P.next;
    S->dist = P.dist;
    S->labels = P.labels;
    S->ids = ids;
    S->row_offset = P.row_offset;
    if (exchange) {
        S->sel_cands = P.sel_cands;
        S->sel_world = P.sel_world;
        S->sel_centers = static_cast<double*>(P.sel_centers);
        S->sel_ids = P.sel_ids;
        S->cand_out = P.cand_out;
        S->counter = P.counter;
    }
    return MSM_OK;
}

// Writes the copy: its origin is centre 0 -- row ids[0], or `centre0` where the row may be another rank's -- then the rows.
static void ksc_queue_copy(const KscArgs& S, const double* centre0)
{
    hipLaunchKernelGGL(ksc_origin_kernel, dim3(1), dim3(64), 0, stream(), S.X, S.ids, (long long)S.m, S.c0, centre0);
    const int gconv = (int)std::min<long long>(ceil_div(S.n, DT), 8LL * num_cus());
    ksc_np_visit(ksc_np(S.m), [&](auto np) {
        hipLaunchKernelGGL((ksc_convert_kernel<decltype(np)::value, KSC_FMT>), dim3(gconv), dim3(DT), 0, stream(), S);
    });
}

static void ksc_queue_pass(const KscArgs& S)
{
    ksc_np_visit(ksc_np(S.m), [&](auto np) {
        hipLaunchKernelGGL((kcenters_screen_pass_kernel<decltype(np)::value, KSC_FMT>), dim3(S.nblk), dim3(DT), 0, stream(), S);
    });
}

// Rounds the host queues before it looks at the progress counter again.  A synchronisation costs 35-50 us of idle GPU, an
// empty round (all K centres fixed: three early-returning launches) about 14: so the first group aims at the whole fit at
// a typical 12 centres per round, and the later ones at what is left at the rate seen so far, plus one.  The value depends
// on nothing but K and the counter, which every rank of a sharded fit holds identically.
static int kcb_group(int K, int done, int rounds_so_far, int done_at_start)
{
    const int left = K - done;
    if (left <= 0) return 0;
    int per = 12;
    if (rounds_so_far > 0) per = std::max(1, (done - done_at_start) / rounds_so_far);
    const int g = (left + per - 1) / per + (rounds_so_far > 0 ? 1 : 0);
    return std::min(std::max(g, 1), 24);
}

// The batched loops: rounds are queued a group at a time -- a round whose selector finds all K centres fixed is a few
// empty launches -- and the host looks at the head of KcbState between the groups: one synchronisation per group.
// queue_round(round, last) queues round number `round` (from 0); `last`: the host synchronises after it.  synced() runs
// after each group's synchronisation.  Both return a status.
template <typename Round, typename Synced = int (*)()>
static int kcb_run_rounds(int K, int done_at_start, KcbState* St, const char* no_progress, Round&& queue_round,
                          Synced synced = [] { return (int)MSM_OK; })
{
    int rc, rounds = 0;
    int head4[4] = {done_at_start, 0, 0, 0};   // k_done, J, rounds, fallbacks: the head of KcbState
    while (head4[0] < K) {
        const int group = kcb_group(K, head4[0], rounds, done_at_start);
        for (int r = 0; r < group; ++r, ++rounds)
            if ((rc = queue_round(rounds, r + 1 == group))) return rc;
        MSM_HIP_CHECK(hipGetLastError());
        MSM_HIP_CHECK(hipMemcpyAsync(head4, St, sizeof(head4), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        if ((rc = synced())) return rc;
        if (rounds > 4 * K) return fail(MSM_ERR_HIP, "%s", no_progress);
    }
    g_kc_stats.screened_passes = head4[2];   // passes that streamed the copy (the empty rounds of the last group are not counted)
    g_kc_stats.batch_fallbacks = head4[3];
    return MSM_OK;
}

// ---- the single fit's loops ----------------------------------------------------------------------------------------
// plain passes first .. last - 1
template <typename T>
static void kc_run_plain(int mid, KcArgs& P, const KcParts& parts, msm_idx_t first, msm_idx_t last)
{
    for (msm_idx_t it = first; it < last; ++it) {
        P.it = (int)it;
        parts.aim(P, it);
        launch_kc<T>(mid, P.nblk, P);
    }
}

// float64 rows in registers, euclidean, n >= 65536, K > 8 (so screened passes always follow the plain ones)
static int kc_run_narrow_screen(int mid, msm_idx_t K, KcArgs& P, const KcParts& parts, const KcSwitches& sw)
{
    // A few plain passes first (in the first passes most rows change, and a candidate costs the screen's bytes on top of
    // the plain pass's), then the screened ones.  Measured on 10M x 10 float64, K = 200 (scripts/kcperf.py, kcblobs.py),
    // plain / screened from pass 16 / from pass 4 / from pass 1: tICA projection 26.6 / 13.1 / 11.8 / 11.8 ms, white
    // noise 33.7 / 15.1 / 13.3 / 17.6 ms, 40 separated blobs (where per-row pruning is at its best) 17.9 / 17.1 / 17.1 /
    // 17.5 ms -- so no decision is needed.
    // (with several centres per pass the early centres are cheap on the copy too -- one pass applies a batch of them to
    //  every row, whatever fraction changes: 2 plain passes, tICA projection 4.53 -> 4.26 ms; 4 for one centre per pass)
    const bool kcb_on = sw.batch && P.nblk <= 1024;
    const msm_idx_t probe = kcb_on ? 2 : 4;
    KscArgs S;
    int rc;
    if ((rc = ksc_open(P, P.seed, P.ids, false, &S))) return rc;
    kc_run_plain<double>(mid, P, parts, 0, probe);
    g_kc_stats.plain_passes = probe;
    g_kc_stats.screened_passes = K - probe;
    g_kc_stats.screen_row_bytes = ksc_row_bytes(P.m);
    ksc_queue_copy(S, nullptr);
    if (!kcb_on) {
        for (msm_idx_t it = probe; it < K; ++it) {
            S.it = (int)it;
            parts.aim(S, it);
            ksc_queue_pass(S);
        }
        return MSM_OK;
    }
    // several centres per pass (kcb_select_kernel / kcenters_batch_pass_kernel): rounds of {selector, pass}
    DevBuf& SB = pool(PS_W);
    if ((rc = SB.reserve(sizeof(KcbState)))) return rc;
    KcbState* St = SB.as<KcbState>();
    hipLaunchKernelGGL(kcb_init_kernel, dim3(1), dim3(64), 0, stream(), St, (int)probe);
    return kcb_run_rounds((int)K, (int)probe, St, "k-centers: the batched passes made no progress", [&](int round, bool) {
        parts.aim(S, probe + round);   // reads the partials of the last pass that ran
        ksc_np_visit(ksc_np(S.m), [&](auto np) {
            hipLaunchKernelGGL((kcb_select_kernel<decltype(np)::value>), dim3(1), dim3(1024), 0, stream(), S, St, (int)K);
            hipLaunchKernelGGL((kcenters_batch_pass_kernel<decltype(np)::value>), dim3(S.nblk), dim3(DT), 0, stream(), S, St);
        });
        return (int)MSM_OK;
    });
}

// grids and LDS of the wide screen's passes
struct KwsSizes {
    int kr, gpass;              // one centre per pass: rows per thread, grid
    int jmax, kr2, gp2;         // batched rounds: centres per round (0: none), rows per thread, grid
    int nbsel;                  // their selector's workgroups (0: one workgroup, kwb_select_kernel)
    size_t lds, lds2, ldssel;   // dynamic LDS of the pass, the batched pass, the selector
};

template <typename T>
static KwsSizes kws_sizes(long long n, long long m, int nb4, int nblk0, const KcSwitches& sw)
{
    KwsSizes Z;
    Z.lds = (size_t)4 * nb4 * sizeof(float) + (size_t)m * sizeof(T);
    Z.kr = nb4 <= 4 ? 8 : nb4 <= 16 ? 4 : 2;   // rows per thread (x 4 / 8 / 16 planes per trip: distance_wscreen_dev.h)
    Z.gpass = (int)std::min<long long>(ceil_div(n, (long long)Z.kr * DT), nblk0);
    // Several centres per pass (distance_wbatch_dev.h): as many as fit 64 KiB of LDS beside the pass's own 40 KiB --
    // 16 up to 256 float32 / 170 float64 features, 8 up to twice that, one beyond.  MSM_KC_WBATCH=0: one centre per pass.
    Z.jmax = 0;
    {
        const size_t per = (size_t)4 * nb4 * sizeof(float) + ((size_t)m * sizeof(T) + 15) / 16 * 16;   // float32 copy + the row at a 16-byte pitch
        if (16 * per <= 65536) Z.jmax = 16;
        else if (8 * per <= 65536) Z.jmax = 8;
        // (First version: a round cost ~250 us on top of its streaming and the batches only paid for passes of >= 90 MB.
        //  The cost was the exact re-evaluation -- one lane per candidate walking its row element by element out of LDS,
        //  ~10 us per row and centre -- and the one-workgroup selector; with 16-byte fetches ahead of the chain
        //  (kwb_exact_euclid) and the selector on several workgroups the batches win at every shape of scripts/kcwide.py:
        //  280,000 x 171 K = 200 6.6 -> 4.3 ms, 1M x 171 K = 500 28.2 -> 13.9 ms, 500,000 x 512 27.4 -> 24.4 ms.)
        // Default for rows of up to 1 KiB; MSM_KC_WBATCH=0 / 1 (read per fit) forces one centre per screened pass / the batches.
        const bool pays = (size_t)m * sizeof(T) <= 1024;   // (500,000 x 512 float32: 24.5 ms batched against 19.7 ms one centre per pass -- 16 accumulators per row over 128 words, and the union of 16 centres' candidates at 2 KiB per row)
        if (sw.wbatch >= 0 ? sw.wbatch == 0 : !pays) Z.jmax = 0;
        Z.lds2 = (size_t)Z.jmax * per;
    }
    Z.kr2 = nb4 <= 16 ? 4 : 2;   // rows per thread: 16 (8) accumulators each
    Z.gp2 = (int)std::min<long long>(ceil_div(n, (long long)Z.kr2 * DT), nblk0);
    // the selector on several workgroups (kwb_select_multi_kernel): as many as it takes for a slice of a full list
    // to fit the LDS beside the centre, one row per thread; 0: one workgroup (rows beyond ~9 KiB; MSM_KC_WSELECT=1)
    Z.nbsel = 0;
    Z.ldssel = 0;
    const size_t pitch = (size_t)(m | 1), cpad = (size_t)((m + 3) & ~3LL);
    for (int nb = 8; nb <= 64 && !sw.wselect_one; nb += 8) {
        const size_t rpw = (size_t)ceil_div(KCB_CAP, nb);
        const size_t bytes = (cpad + rpw * pitch) * sizeof(T);
        if (rpw <= (size_t)DT && bytes <= 150000) {
            Z.nbsel = nb;
            Z.ldssel = bytes;
            break;
        }
    }
    return Z;
}

// euclidean, n >= 65536, K > 8, rows of more than 64 bytes and at most 4096 features that the narrow screen does not take
template <typename T>
static int kc_run_wide_screen(int mid, msm_idx_t K, KcArgs& P, const KcParts& parts, const KcSwitches& sw)
{
    // Round 6: everything the register-resident screen above does not take -- float32 rows of any length, float64 rows of
    // more than 16 features -- is screened on a FEATURE-major byte copy (distance_wscreen_dev.h): a few plain passes
    // (most rows still change), then m + 8 bytes per row and pass instead of m sizeof(T) + 16.  Bit-identical results.
    constexpr msm_idx_t KWS_PROBE = 4;
    const long long n = P.n, m = P.m;
    const int nblk = P.nblk;
    const int nb4 = (int)((m + 3) / 4);   // words of a row's byte copy
    const KwsSizes Z = kws_sizes<T>(n, m, nb4, parts.nblk0, sw);
    kc_run_plain<T>(mid, P, parts, 0, KWS_PROBE);
    // the copy, once the plain passes have fixed centre 0: reserve, arguments of the screened kernels, origin, conversion
    KscBufs& B = ksc_bufs();
    int rc;
    const size_t qbytes = (size_t)nb4 * n * sizeof(unsigned);
    if ((rc = B.xf.reserve(qbytes + (size_t)n * sizeof(float) + (size_t)n * sizeof(unsigned short) + 64))) return rc;
    if ((rc = B.misc.reserve(64 + (size_t)m * sizeof(double)))) return rc;   // [gmax2 | stats[2] | ... | c0[m]]
    MSM_HIP_CHECK(hipMemsetAsync(B.misc.p, 0, 64, stream()));
    KwsArgs S;
    memset(&S, 0, sizeof(S));
    S.X = P.X;
    S.q = B.xf.as<unsigned>();
    S.curf = reinterpret_cast<float*>(static_cast<char*>(B.xf.p) + qbytes);
    S.sf = reinterpret_cast<unsigned short*>(static_cast<char*>(B.xf.p) + qbytes + (size_t)n * sizeof(float));
    S.gmax2 = B.misc.as<unsigned long long>();
    S.stats = sw.stats ? S.gmax2 + 1 : nullptr;   // (every candidate lane adds to ONE word: tens of thousands of atomics per pass)
    S.c0 = reinterpret_cast<double*>(static_cast<char*>(B.misc.p) + 64);
    S.n = n;
    S.m = m;
    S.nb4 = nb4;
    S.nblk = P.nblk;
    S.dist = P.dist;
    S.labels = P.labels;
    S.ids = P.ids;
    hipLaunchKernelGGL(kws_origin_kernel<T>, dim3(1), dim3(256), 0, stream(), static_cast<const T*>(P.X), P.ids, (long long)m,
                       const_cast<double*>(S.c0), S.gmax2);
    const int crows = std::max(1, std::min(KWS_CROWS, KWS_CWORDS / (nb4 + 1)));   // rows a workgroup transposes at a time
    const int gconv = (int)std::min<long long>(ceil_div(n, crows), 16LL * num_cus());
    if ((size_t)m * sizeof(T) <= 192)   // short rows: a thread per row (2M x 17 float64: convert 0.99 -> 0.6 ms; from 256-byte rows the strided walks lose: 1M x 64 float32 fit 3.9 -> 4.5 ms)
        hipLaunchKernelGGL(kws_convert_rowthread_kernel<T>, dim3((unsigned)std::min<long long>(ceil_div(n, DT), 16LL * num_cus())), dim3(DT),
                           (size_t)m * sizeof(double), stream(), S);
    else
        hipLaunchKernelGGL(kws_convert_kernel<T>, dim3(gconv), dim3(DT), (size_t)m * sizeof(double), stream(), S, crows);
    MSM_HIP_CHECK(hipGetLastError());
    g_kc_stats.plain_passes = KWS_PROBE;
    g_kc_stats.screened_passes = K - KWS_PROBE;
    g_kc_stats.screen_row_bytes = (long long)(4 * nb4 + 2 + 4);   // byte planes + scale + rounded-up distance
    // (the screened passes write `gpass` / `gp2` partials, the plain passes before them `nblk`: S.nblk is what the last pass wrote)
    if (Z.jmax > 0) {
        DevBuf& SB = pool(PS_W);
        if ((rc = SB.reserve(sizeof(KcbState) + sizeof(KwbSync)))) return rc;
        KcbState* St = SB.as<KcbState>();
        KwbSync* Sy = reinterpret_cast<KwbSync*>(static_cast<char*>(SB.p) + sizeof(KcbState));
        hipLaunchKernelGGL(kcb_init_kernel, dim3(1), dim3(64), 0, stream(), St, (int)KWS_PROBE);
        MSM_HIP_CHECK(hipMemsetAsync(Sy, 0, sizeof(KwbSync), stream()));
        static bool attr_set = false;
        if (Z.nbsel && !attr_set) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kwb_select_multi_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, 150016);
            attr_set = true;
        }
        const int wcap = KCB_CAP;   // (shorter lists were tried: 512 rows -> three centres per round instead of twelve)
        unsigned sy4[4] = {0, 0, 0, 0};
        rc = kcb_run_rounds(
            (int)K, (int)KWS_PROBE, St, "k-centers: the batched wide passes made no progress",
            [&](int round, bool last) {
                parts.aim(S, KWS_PROBE + round);
                S.nblk = round == 0 ? nblk : Z.gp2;
                if (Z.nbsel) hipLaunchKernelGGL((kwb_select_multi_kernel<T>), dim3(Z.nbsel), dim3(DT), Z.ldssel, stream(), S, St, Sy, (int)K, Z.jmax, wcap);
                else hipLaunchKernelGGL((kwb_select_kernel<T>), dim3(1), dim3(1024), (size_t)m * sizeof(T), stream(), S, St, (int)K, Z.jmax, wcap);
                if (Z.jmax == 16 && Z.kr2 == 4) launch_kwb<T, 16, 4, 8>(Z.gp2, Z.lds2, S, St);
                else if (Z.jmax == 16) launch_kwb<T, 16, 2, 24>(Z.gp2, Z.lds2, S, St);
                else if (Z.kr2 == 4) launch_kwb<T, 8, 4, 8>(Z.gp2, Z.lds2, S, St);
                else launch_kwb<T, 8, 2, 24>(Z.gp2, Z.lds2, S, St);
                if (last) MSM_HIP_CHECK(hipMemcpyAsync(sy4, Sy, sizeof(sy4), hipMemcpyDeviceToHost, stream()));   // read with the group's head
                return (int)MSM_OK;
            },
            [&] {
                return sy4[2] ? fail(MSM_ERR_HIP, "k-centers: the selector's workgroups did not meet at their barrier (MSM_KC_WSELECT=1 runs it on one workgroup)") : (int)MSM_OK;
            });
        if (rc) return rc;
    } else {
        for (msm_idx_t it = KWS_PROBE; it < K; ++it) {
            S.it = (int)it;
            parts.aim(S, it);
            S.nblk = it == KWS_PROBE ? nblk : Z.gpass;
            if (Z.kr == 8) hipLaunchKernelGGL((kcenters_wscreen_pass_kernel<T, 8, 4>), dim3(Z.gpass), dim3(DT), Z.lds, stream(), S);
            else if (Z.kr == 4) hipLaunchKernelGGL((kcenters_wscreen_pass_kernel<T, 4, 8>), dim3(Z.gpass), dim3(DT), Z.lds, stream(), S);
            else hipLaunchKernelGGL((kcenters_wscreen_pass_kernel<T, 2, 24>), dim3(Z.gpass), dim3(DT), Z.lds, stream(), S);
        }
    }
    if (sw.stats) {   // one more round trip
        unsigned long long hs[2] = {0, 0};
        MSM_HIP_CHECK(hipMemcpyAsync(hs, S.stats, sizeof(hs), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        g_kc_stats.wide_candidates = (long long)hs[0];
        g_kc_stats.wide_updates = (long long)hs[1];
    }
    return MSM_OK;
}

template <typename T>
int kcenters_impl(const T* X, msm_idx_t n, msm_idx_t m, msm_idx_t K, const char* metric,
                  msm_idx_t seed, msm_idx_t* ids, msm_idx_t* labels, double* distances,
                  double* inertia, int on_device, T* centers_out = nullptr)
{
    const msm_idx_t m_rows = m;   // the caller's row length (the fit may run on a zero-padded copy)
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!X || !ids || !labels || !distances) return fail(MSM_ERR_INVALID, "kcenters_fit: null pointer");
    if (n < 1 || m < 1 || K < 1) return fail(MSM_ERR_INVALID, "kcenters_fit: bad shape");
    if (seed < 0 || seed >= n) return fail(MSM_ERR_INVALID, "kcenters_fit: seed_index out of range");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const KcSwitches sw = kc_switches();
    int rc = MSM_OK;
    DevBuf &dX = pool(PS_X), &dLab = pool(PS_LAB), &dDist = pool(PS_MIN), &dPart = pool(PS_PART), &dIds = pool(PS_IDS),
           &dSum = pool(PS_SUM);
    const int nblk0 = kc_blocks(n);
    if ((rc = dPart.reserve((size_t)2 * nblk0 * sizeof(KcPartial)))) return rc;
    if ((rc = dIds.reserve((size_t)K * sizeof(msm_idx_t)))) return rc;
    if ((rc = dSum.reserve((size_t)nblk0 * sizeof(double)))) return rc;
    const KcParts parts = {dPart.as<KcPartial>(), nblk0};
    KcArgs P;
    memset(&P, 0, sizeof(P));
    P.n = n;
    P.m = m;
    P.seed = seed;
    P.ids = dIds.as<msm_idx_t>();
    P.prune = 1;
    if (on_device) {
        P.X = X;
        P.labels = labels;
        P.dist = distances;
    } else {
        if ((rc = dX.reserve((size_t)n * m * sizeof(T)))) return rc;
        if ((rc = dLab.reserve((size_t)n * sizeof(msm_idx_t)))) return rc;
        if ((rc = dDist.reserve((size_t)n * sizeof(double)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n * m * sizeof(T)))) return rc;
        P.X = dX.p;
        P.labels = dLab.as<msm_idx_t>();
        P.dist = dDist.as<double>();
    }
    if (pad_rows_pays<T>(mid, m, n, false)) {   // odd rows, norm metric: a zero-padded aligned copy (see pad_rows_pays)
        const T* xp = nullptr;
        long long mp = m;
        if ((rc = pad_rows<T>(static_cast<const T*>(P.X), n, m, pool(PS_PADX), &xp, &mp))) return rc;
        P.X = xp;
        P.m = m = mp;
    }
    P.vecw = row_vecw<T>(P.X, m, false);
    const int nblk = P.nblk = kc_wide_cut<T>(nblk0, P);
    kc_stats_begin<T>(n, m);
    g_kc_stats.plain_passes = K;
    const bool screenable = mid == M_EUCLIDEAN && n >= 65536 && K > 8;
    if (screenable && sizeof(T) == 8 && P.vecw > 0) {
        if constexpr (sizeof(T) == 8) rc = kc_run_narrow_screen(mid, K, P, parts, sw);
    } else if (screenable && m <= 4096 && (size_t)m * sizeof(T) > 64 && sw.wscreen) {
        rc = kc_run_wide_screen<T>(mid, K, P, parts, sw);
    } else {
        kc_run_plain<T>(mid, P, parts, 0, K);
    }
    if (rc) return rc;
    MSM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(sum_partial_kernel, dim3(nblk), dim3(DT), 0, stream(), P.dist, (long long)n, dSum.as<double>());
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(ids, P.ids, (size_t)K * sizeof(msm_idx_t), hipMemcpyDeviceToHost, stream()));
    if (centers_out) {
        DevBuf& dCen = pool(PS_Y);
        if ((rc = dCen.reserve((size_t)K * m_rows * sizeof(T)))) return rc;
        const T* Xsrc = on_device ? X : static_cast<const T*>(dX.p);
        hipLaunchKernelGGL((kc_gather_centres_kernel<T>), dim3((unsigned)K), dim3(64), 0, stream(), Xsrc, (long long)m_rows, P.ids, dCen.as<T>());
        MSM_HIP_CHECK(hipGetLastError());
        MSM_HIP_CHECK(hipMemcpyAsync(centers_out, dCen.p, (size_t)K * m_rows * sizeof(T), hipMemcpyDeviceToHost, stream()));
    }
    if (!on_device) {
        MSM_HIP_CHECK(hipMemcpyAsync(labels, P.labels, (size_t)n * sizeof(msm_idx_t), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(distances, P.dist, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    double s = 0.0;
    if ((rc = sum_partials_host(dSum.as<double>(), nblk, &s))) return rc;  // synchronises
    if (inertia) *inertia = s;
    return MSM_OK;
}

// ---- externally driven passes --------------------------------------------------------------------------------------
// Queues pass `it` against the centre y_dev (device coordinates); its *nblk partials go to *part.  An empty shard queues
// nothing and has no partials.  centers_dev: centres 0 .. it of the fit (pruning table); null: no pruning.
template <typename T>
static int kc_queue_pass(int mid, const T* X, msm_idx_t n, msm_idx_t m, const T* y_dev, msm_idx_t it, msm_idx_t* labels,
                         double* distances, const T* centers_dev, KcPartial** part, int* nblk)
{
    int rc;
    DevBuf &dPart = pool(PS_PART), &dIds = pool(PS_IDS);
    if ((rc = dPart.reserve((size_t)kc_blocks(n) * sizeof(KcPartial)))) return rc;
    if ((rc = dIds.reserve(sizeof(msm_idx_t)))) return rc;
    KcArgs P;
    memset(&P, 0, sizeof(P));
    P.X = X;
    P.n = n;
    P.m = m;
    P.it = (int)it;
    *part = P.next = dPart.as<KcPartial>();
    P.dist = distances;
    P.labels = labels;
    P.ids = dIds.as<msm_idx_t>();
    P.ycenter = y_dev;
    P.centers = centers_dev;
    P.prune = centers_dev ? 1 : 0;
    *nblk = 0;
    if (n > 0) {
        P.vecw = row_vecw<T>(P.X, m, false);
        *nblk = P.nblk = kc_wide_cut<T>(kc_blocks(n), P);
        launch_kc<T>(mid, P.nblk, P);
        MSM_HIP_CHECK(hipGetLastError());
    }
    return MSM_OK;
}

// One externally driven pass (multi-rank k-centers): centre coordinates come from the host,
// the local (max distance, lowest local row) comes back.
template <typename T>
int kcenters_pass_impl(const T* X, msm_idx_t n, msm_idx_t m, const T* y, msm_idx_t it, const char* metric,
                       msm_idx_t* labels, double* distances, double* max_dist, msm_idx_t* argmax,
                       T* argmax_row, int on_device)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!X || !y || !labels || !distances || !max_dist || !argmax) return fail(MSM_ERR_INVALID, "kcenters_pass: null pointer");
    if (n < 1 || m < 1 || it < 0) return fail(MSM_ERR_INVALID, "kcenters_pass: bad shape");
    if (!on_device) return fail(MSM_ERR_INVALID, "kcenters_pass: per-row arrays must be device resident");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc, nblk;
    DevBuf& dY = pool(PS_Y);
    if ((rc = dY.reserve((size_t)m * sizeof(T)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(dY.p, y, (size_t)m * sizeof(T), hipMemcpyHostToDevice, stream()));
    KcPartial* part;
    if ((rc = kc_queue_pass<T>(mid, X, n, m, dY.as<T>(), it, labels, distances, nullptr, &part, &nblk))) return rc;
    // device-side final reduce + fetch of the winning row: ONE small D2H per pass
    DevBuf& dBest = pool(PS_SUM);
    if ((rc = dBest.reserve(sizeof(KcPartial) + (size_t)m * sizeof(T)))) return rc;
    KcPartial* dbest = dBest.as<KcPartial>();
    T* drow = reinterpret_cast<T*>(dbest + 1);
    hipLaunchKernelGGL((kc_finalize_kernel<T>), dim3(1), dim3(DT), 0, stream(), part, nblk, X, (long long)m, dbest, drow);
    MSM_HIP_CHECK(hipGetLastError());
    std::vector<char> hb(sizeof(KcPartial) + (size_t)m * sizeof(T));
    MSM_HIP_CHECK(hipMemcpyAsync(hb.data(), dbest, hb.size(), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    const KcPartial* hp = reinterpret_cast<const KcPartial*>(hb.data());
    *max_dist = hp->v;
    *argmax = hp->i;
    if (argmax_row && hp->i >= 0) memcpy(argmax_row, hb.data() + sizeof(KcPartial), (size_t)m * sizeof(T));
    return MSM_OK;
}

// one pass + candidate record, everything on the stream, no synchronisation
template <typename T>
int kcenters_pass_dev_impl(const T* X, msm_idx_t n, msm_idx_t m, const T* y_dev, msm_idx_t it, const char* metric,
                           msm_idx_t* labels, double* distances, msm_idx_t row_offset, double* cand_dev,
                           const T* centers_dev = nullptr)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!y_dev || !cand_dev || (n > 0 && (!X || !labels || !distances))) return fail(MSM_ERR_INVALID, "kcenters_pass_dev: null pointer");
    if (n < 0 || m < 1 || it < 0) return fail(MSM_ERR_INVALID, "kcenters_pass_dev: bad shape");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    int rc, nblk;
    KcPartial* part;
    if ((rc = kc_queue_pass<T>(mid, X, n, m, y_dev, it, labels, distances, centers_dev, &part, &nblk))) return rc;
    hipLaunchKernelGGL((kc_candidate_kernel<T>), dim3(1), dim3(DT), 0, stream(), part, nblk, X, (long long)m,
                       (long long)row_offset, cand_dev);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

template <typename T>
int kcenters_select_impl(const double* cands_dev, msm_idx_t world, msm_idx_t m, T* y_dev, T* centers_dev,
                         msm_idx_t* ids_dev, msm_idx_t slot)
{
    if (!cands_dev || !y_dev || !centers_dev || !ids_dev || world < 1 || m < 1 || slot < 0)
        return fail(MSM_ERR_INVALID, "kcenters_select: bad argument");
    hipLaunchKernelGGL((kc_select_kernel<T>), dim3(1), dim3(DT), 0, stream(), cands_dev, (int)world, (long long)m, y_dev,
                       centers_dev, ids_dev, (long long)slot);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// ---- the sharded fit's loops ---------------------------------------------------------------------------------------
// a rank's arguments of the sharded fit
template <typename T>
struct KcsShard {
    const T* X;
    msm_idx_t n, m, K;
    int mid;
    const char* metric;
    msm_idx_t seed, row_offset;
    msm_idx_t* labels;
    double* distances;
    int world;
};

// the PS_S buffer: [cand rec | cands world*rec | sums 1024 + 1] doubles, [y m | cen K*m] T, [dids K] int64
template <typename T>
struct KcsBufs {
    size_t rec;        // doubles of a candidate record
    double *cand, *cands, *sums;   // the shard's record; every rank's; the inertia partials
    T *y, *cen;        // the current centre; the centres so far
    msm_idx_t* dids;
    int gather() const { return comm_allgather(cand, cands, rec * sizeof(double)); }
};

template <typename T>
static int kcs_carve(msm_idx_t m, msm_idx_t K, int world, KcsBufs<T>* B)
{
    const size_t rec = B->rec = (size_t)(2 + m);
    DevBuf& dS = pool(PS_S);
    const size_t nd = rec + (size_t)world * rec + 1032;
    const size_t tbytes = ((size_t)(K + 1) * m * sizeof(T) + 15) / 16 * 16;
    if (int rc = dS.reserve(nd * sizeof(double) + tbytes + (size_t)K * sizeof(msm_idx_t))) return rc;
    B->cand = dS.as<double>();
    // without a communicator (a world of one: bench.py's strong-scaling model, single-process use) the "gathered" records
    // ARE the shard's record: no copy per centre
    B->cands = comm_active() ? B->cand + rec : B->cand;
    B->sums = B->cands + (size_t)world * rec;
    B->y = reinterpret_cast<T*>(B->sums + 1032);
    B->cen = B->y + m;
    B->dids = reinterpret_cast<msm_idx_t*>(reinterpret_cast<char*>(B->y) + tbytes);
    return MSM_OK;
}

// The arguments of a sharded pass that selects its centre from the gathered records and writes the shard's record itself
// (register path), with the partials and the arrival counter it needs.
template <typename T>
static int kcs_pass_args(const KcsShard<T>& F, const KcsBufs<T>& B, KcArgs* P)
{
    DevBuf& dPart = pool(PS_PART);
    const int nblk = kc_blocks(F.n);
    int rc;
    if ((rc = dPart.reserve((size_t)nblk * sizeof(KcPartial) + 16))) return rc;
    unsigned* counter = reinterpret_cast<unsigned*>(dPart.as<KcPartial>() + nblk);
    MSM_HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned), stream()));
    memset(P, 0, sizeof(*P));
    P->X = F.X;
    P->n = F.n;
    P->m = F.m;
    P->nblk = nblk;
    P->next = dPart.as<KcPartial>();
    P->dist = F.distances;
    P->labels = F.labels;
    P->vecw = row_vecw<T>(F.X, F.m, false);
    P->centers = B.cen;
    P->prune = 1;
    P->sel_cands = B.cands;
    P->sel_world = F.world;
    P->sel_centers = B.cen;
    P->sel_ids = B.dids;
    P->cand_out = B.cand;
    P->row_offset = F.row_offset;
    P->counter = counter;
    return MSM_OK;
}

// Centres 0 .. count - 1 by the generic kernels: pass, candidate record, all-gather, select -- rows wider than the register
// path, or an empty shard.  Leaves the stats untouched.  `gather_last`: the exchange goes on after these centres (the
// batched loop's probe on an empty shard), so the last record is gathered too.
template <typename T>
static int kcs_run_generic(const KcsShard<T>& F, const KcsBufs<T>& B, msm_idx_t count, bool gather_last)
{
    int rc;
    if ((rc = kcenters_select_impl<T>(B.cands, F.world, F.m, B.y, B.cen, B.dids, 0))) return rc;
    for (msm_idx_t it = 0; it < count; ++it) {
        if ((rc = kcenters_pass_dev_impl<T>(F.X, F.n, F.m, B.y, it, F.metric, F.labels, F.distances, F.row_offset, B.cand, B.cen))) return rc;
        if ((it + 1 < count || gather_last) && (rc = B.gather())) return rc;
        if (it + 1 < count && (rc = kcenters_select_impl<T>(B.cands, F.world, F.m, B.y, B.cen, B.dids, it + 1))) return rc;
    }
    return MSM_OK;
}

// Several centres per exchange (kcb_*: threshold lists, an identical selection on every rank): PROBE all-gathers of one
// candidate, then one all-gather of a round record per round.
static int kcs_run_batched(const KcsShard<double>& F, const KcsBufs<double>& B)
{
    constexpr msm_idx_t PROBE = 2;
    const msm_idx_t n = F.n, m = F.m;
    const int world = F.world;
    int rc;
    KcArgs P;
    if ((rc = kcs_pass_args(F, B, &P))) return rc;
    kc_stats_begin<double>(n, m);
    g_kc_stats.screen_row_bytes = ksc_row_bytes(m);
    g_kc_stats.plain_passes = PROBE;
    // ---- the first PROBE centres: one candidate per exchange, plain passes (a rank without rows keeps the pattern) ----
    if (n > 0) {
        for (msm_idx_t it = 0; it < PROBE; ++it) {
            P.it = (int)it;
            launch_kc<double>(F.mid, P.nblk, P);
            if ((rc = B.gather())) return rc;
        }
    } else if ((rc = kcs_run_generic(F, B, PROBE, true)))
        return rc;
    MSM_HIP_CHECK(hipGetLastError());
    // ---- rounds ----
    const size_t RD = kcb_rec_doubles(m);
    DevBuf& W = pool(PS_W);
    const size_t stb = (sizeof(KcbState) + 15) / 16 * 16;
    if ((rc = W.reserve(stb + (size_t)(1 + world) * RD * sizeof(double)))) return rc;
    KcbState* St = W.as<KcbState>();
    double* recL = reinterpret_cast<double*>(static_cast<char*>(W.p) + stb);
    double* recsG = comm_active() ? recL + RD : recL;   // a world of one: the gathered records ARE the rank's record
    hipLaunchKernelGGL(kcb_init_kernel, dim3(1), dim3(64), 0, stream(), St, (int)PROBE);
    hipLaunchKernelGGL(kcb_boot_records_kernel, dim3((unsigned)world), dim3(64), 0, stream(), B.cands, world, (long long)m, recsG);
    KscArgs S;
    memset(&S, 0, sizeof(S));
    if (n > 0) {
        if ((rc = ksc_open(P, F.seed, B.dids, false, &S))) return rc;
        ksc_queue_copy(S, B.cen);
    }
    MSM_HIP_CHECK(hipGetLastError());
    return kcb_run_rounds((int)F.K, (int)PROBE, St, "k-centers: the batched rounds made no progress", [&](int, bool) {
        ksc_np_visit(ksc_np(m), [&](auto np) {
            hipLaunchKernelGGL((kcb_select_sharded_kernel<decltype(np)::value>), dim3(1), dim3(1024), 0, stream(), recsG, world, (long long)m, St,
                               (int)F.K, B.cen, B.dids);
            if (n > 0) {
                hipLaunchKernelGGL((kcenters_batch_pass_kernel<decltype(np)::value>), dim3(S.nblk), dim3(DT), 0, stream(), S, St);
                hipLaunchKernelGGL((kcb_pack_kernel<decltype(np)::value>), dim3(1), dim3(DT), 0, stream(), S, St, recL);
            }
        });
        if (n <= 0) hipLaunchKernelGGL(kcb_empty_record_kernel, dim3(1), dim3(64), 0, stream(), recL);
        MSM_HIP_CHECK(hipGetLastError());
        return comm_allgather(recL, recsG, RD * sizeof(double));
    });
}

// Register path (m <= FC), a shard with rows: one kernel and one all-gather per centre.
template <typename T>
static int kcs_run_fused(const KcsShard<T>& F, const KcsBufs<T>& B)
{
    int rc;
    KcArgs P;
    if ((rc = kcs_pass_args(F, B, &P))) return rc;
    // Screened passes (float64 rows, euclidean; see kcenters_screen_pass_kernel) after a few plain ones, as in the
    // single-process fit.  The decision is LOCAL to a rank: the exchange pattern (one all-gather per centre) is the same
    // for both kernels, so a rank with a small shard may keep the plain kernel while its peers screen.
    constexpr int KSC_PROBE = 4;
    const bool screen = sizeof(T) == 8 && F.mid == M_EUCLIDEAN && F.n >= 65536 && F.K > 8;
    KscArgs S;
    memset(&S, 0, sizeof(S));
    if (screen && (rc = ksc_open(P, F.seed, B.dids, true, &S))) return rc;
    kc_stats_begin<T>(F.n, F.m);
    g_kc_stats.screen_row_bytes = ksc_row_bytes(F.m);
    for (msm_idx_t it = 0; it < F.K; ++it) {
        if (screen && it >= KSC_PROBE) {
            // the copy's origin is centre 0 as every rank selected it (possibly another rank's row)
            if (it == KSC_PROBE) ksc_queue_copy(S, reinterpret_cast<const double*>(B.cen));
            S.it = (int)it;
            ksc_queue_pass(S);
            ++g_kc_stats.screened_passes;
        } else {
            P.it = (int)it;
            launch_kc<T>(F.mid, P.nblk, P);
            ++g_kc_stats.plain_passes;
        }
        if (it + 1 < F.K && (rc = B.gather())) return rc;
    }
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// The whole row-sharded fit: K x (pass, candidate record, all-gather over the library communicator, select), all
// queued on the stream -- the host enqueues and synchronises once at the end (the batched loop: once per round group).
template <typename T>
int kcenters_fit_sharded_impl(const T* X, msm_idx_t n, msm_idx_t m, msm_idx_t K, const char* metric, msm_idx_t seed,
                              msm_idx_t row_offset, msm_idx_t* labels, double* distances, msm_idx_t* ids, T* centers,
                              double* inertia)
{
    const int mid = metric_id(metric);
    if (mid < 0) return fail(MSM_ERR_METRIC, "unknown metric '%s'", metric ? metric : "(null)");
    if (!ids || !centers || (n > 0 && (!X || !labels || !distances))) return fail(MSM_ERR_INVALID, "kcenters_fit_sharded: null pointer");
    if (n < 0 || m < 1 || K < 1 || seed < 0 || row_offset < 0) return fail(MSM_ERR_INVALID, "kcenters_fit_sharded: bad shape");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const KcSwitches sw = kc_switches();
    const KcsShard<T> F = {X, n, m, K, mid, metric, seed, row_offset, labels, distances, comm_world()};
    KcsBufs<T> B;
    int rc;
    if ((rc = kcs_carve<T>(m, K, F.world, &B))) return rc;
    const long long local_seed = (seed >= row_offset && seed < row_offset + n) ? (long long)(seed - row_offset) : -1;
    hipLaunchKernelGGL((kc_seed_candidate_kernel<T>), dim3(1), dim3(DT), 0, stream(), X, (long long)m, local_seed, (long long)seed, B.cand);
    MSM_HIP_CHECK(hipGetLastError());
    if ((rc = B.gather())) return rc;
    // Every rank must take the same loop or the all-gathers would not match.  The batched decision (float64 rows of <= 16
    // features, euclidean) uses nothing a rank knows alone -- not its shard size, which may be zero --, because it changes
    // the exchange pattern (MSM_KC_BATCH=0, the tests' A/B switch: one centre per exchange).  The fused loop is a property
    // of the data type and width only, except for an EMPTY shard -- which runs the generic kernels in the same pattern.
    const bool batched = sizeof(T) == 8 && mid == M_EUCLIDEAN && m <= FeatChunk<T>::FC && K > 8 && sw.batch;
    const bool fused = n > 0 && row_vecw<T>(X, m, false) > 0;  // register path (m <= FC): one kernel per centre
    if (batched) {
        if constexpr (sizeof(T) == 8) rc = kcs_run_batched(F, B);
    } else
        rc = fused ? kcs_run_fused<T>(F, B) : kcs_run_generic<T>(F, B, K, false);
    if (rc) return rc;
    // inertia = sum of ALL ranks' distances_: local fp64 tree sum, then one all-reduce of a single double
    const int nblk = kc_blocks(n);
    hipLaunchKernelGGL(sum_partial_kernel, dim3(nblk), dim3(DT), 0, stream(), distances, (long long)n, B.sums);
    hipLaunchKernelGGL(sum_partial_kernel, dim3(1), dim3(DT), 0, stream(), B.sums, (long long)nblk, B.sums + 1024);
    MSM_HIP_CHECK(hipGetLastError());
    if ((rc = comm_allreduce_f64(B.sums + 1024, 1))) return rc;
    double tot = 0.0;
    MSM_HIP_CHECK(hipMemcpyAsync(&tot, B.sums + 1024, sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(ids, B.dids, (size_t)K * sizeof(msm_idx_t), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(centers, B.cen, (size_t)K * m * sizeof(T), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (inertia) *inertia = tot;
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

/* fit2: the same fit, also returning the chosen rows: centers[n_clusters][m] (HOST) = X[ids] (kcenters.py:98 cluster_centers_) */
#define MSM_KC_ENTRY(SFX, T)                                                                                                          \
    int msm_kcenters_fit_##SFX(const T* X, msm_idx_t n, msm_idx_t m, msm_idx_t n_clusters, const char* metric, msm_idx_t seed_index,  \
                               msm_idx_t* ids, msm_idx_t* labels, double* distances, double* inertia, int on_device)                  \
    {                                                                                                                                 \
        return kcenters_impl<T>(X, n, m, n_clusters, metric, seed_index, ids, labels, distances, inertia, on_device);                 \
    }                                                                                                                                 \
    int msm_kcenters_fit2_##SFX(const T* X, msm_idx_t n, msm_idx_t m, msm_idx_t n_clusters, const char* metric, msm_idx_t seed_index, \
                                msm_idx_t* ids, msm_idx_t* labels, double* distances, double* inertia, int on_device, T* centers)     \
    {                                                                                                                                 \
        return kcenters_impl<T>(X, n, m, n_clusters, metric, seed_index, ids, labels, distances, inertia, on_device, centers);        \
    }                                                                                                                                 \
    int msm_kcenters_fit_sharded_##SFX(const T* X, msm_idx_t n_local, msm_idx_t m, msm_idx_t n_clusters, const char* metric,          \
                                       msm_idx_t seed_index, msm_idx_t row_offset, msm_idx_t* labels, double* distances,              \
                                       msm_idx_t* ids, T* centers, double* inertia)                                                   \
    {                                                                                                                                 \
        return kcenters_fit_sharded_impl<T>(X, n_local, m, n_clusters, metric, seed_index, row_offset, labels, distances, ids,        \
                                            centers, inertia);                                                                        \
    }                                                                                                                                 \
    int msm_kcenters_pass_##SFX(const T* X, msm_idx_t n, msm_idx_t m, const T* y, msm_idx_t it, const char* metric,                   \
                                msm_idx_t* labels, double* distances, double* max_dist, msm_idx_t* argmax, T* argmax_row,             \
                                int on_device)                                                                                        \
    {                                                                                                                                 \
        return kcenters_pass_impl<T>(X, n, m, y, it, metric, labels, distances, max_dist, argmax, argmax_row, on_device);             \
    }                                                                                                                                 \
    int msm_kcenters_pass_dev_##SFX(const T* X, msm_idx_t n, msm_idx_t m, const T* y_dev, msm_idx_t it, const char* metric,           \
                                    msm_idx_t* labels, double* distances, msm_idx_t row_offset, double* cand_dev)                     \
    {                                                                                                                                 \
        return kcenters_pass_dev_impl<T>(X, n, m, y_dev, it, metric, labels, distances, row_offset, cand_dev);                        \
    }                                                                                                                                 \
    int msm_kcenters_select_##SFX(const double* cands_dev, msm_idx_t world, msm_idx_t m, T* y_dev, T* centers_dev,                    \
                                  msm_idx_t* ids_dev, msm_idx_t slot)                                                                 \
    {                                                                                                                                 \
        return kcenters_select_impl<T>(cands_dev, world, m, y_dev, centers_dev, ids_dev, slot);                                       \
    }
MSM_KC_ENTRY(f32, float)
MSM_KC_ENTRY(f64, double)
#undef MSM_KC_ENTRY

int msm_kcenters_last_stats(msm_idx_t* out5)
{
    if (!out5) return fail(MSM_ERR_INVALID, "msm_kcenters_last_stats: null pointer");
    out5[0] = g_kc_stats.rows;
    out5[1] = g_kc_stats.plain_passes;
    out5[2] = g_kc_stats.screened_passes;
    out5[3] = g_kc_stats.plain_row_bytes;
    out5[4] = g_kc_stats.screen_row_bytes;
    return MSM_OK;
}

int msm_kcenters_last_wide_stats(msm_idx_t* out2)
{
    if (!out2) return fail(MSM_ERR_INVALID, "msm_kcenters_last_wide_stats: null pointer");
    out2[0] = g_kc_stats.wide_candidates;
    out2[1] = g_kc_stats.wide_updates;
    return MSM_OK;
}

int msm_kcenters_last_batch_fallbacks(msm_idx_t* out1)
{
    if (!out1) return fail(MSM_ERR_INVALID, "msm_kcenters_last_batch_fallbacks: null pointer");
    out1[0] = g_kc_stats.batch_fallbacks;
    return MSM_OK;
}

}  // extern "C"
