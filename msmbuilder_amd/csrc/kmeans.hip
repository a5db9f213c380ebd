// kmeans.hip -- host side of k-means labelling (GEMM form on MFMA) and the MiniBatchKMeans step for gfx950: the launch
// plan, the stateless and the handle drivers and the C entry points.  The kernels are in kmeans_label_dev.h (float32
// tiles), kmeans_f64_dev.h (float64 tiles), kmeans_small_dev.h (small-batch step) and kmeans_update_dev.h (inertia,
// centre update, convergence, the small helpers) and kmeans_lloyd_dev.h (the full-batch centre update of KMeans); this file
// is their one translation unit.
//
// msmbuilder.cluster.MiniBatchKMeans is a 3-line subclass of scikit-learn's (msmbuilder/cluster/__init__.py:67-69); the
// arithmetic restated here is scikit-learn's (third-party, unpinned by the reference -- DESIGN.md):
//   labels  = argmin_j ( ||c_j||^2 - 2 x.c_j )   in the rows' type, first minimum wins
//             (sklearn/cluster/_k_means_lloyd.pyx chunked sgemm + argmin)
//   inertia = sum_i ||x_i - c_label(i)||^2       (sklearn _k_means_common.pyx _inertia_dense)
//   update  : c <- (c*w + sum_{i in batch, label=j} x_i) / (w + n_j), w += n_j,
//             samples visited in batch order (sklearn _k_means_minibatch.pyx:59-109)
// Which kernel a shape launches, and in how many centre splits, is decided in ONE place: km_plan (exported to the tests
// as msm_kmeans_label_plan).  km_run_label carries a plan out for both drivers.
#include "common.h"
#include "kmeans_label_dev.h"
#include "kmeans_f64_dev.h"
#include "kmeans_update_dev.h"
#include "kmeans_small_dev.h"
#include "kmeans_lloyd_dev.h"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace msm {

template <typename T>
static KmArgsT<T> km_args(const T* X, const msm_idx_t* rows, long long n, long long m, long long K, const T* C, const T* cnorm,
                          int32_t* labels, const int* stop = nullptr)
{
    KmArgsT<T> P;
    memset(&P, 0, sizeof(P));
    P.X = X;
    P.rows = rows;
    P.n = n;
    P.m = m;
    P.K = K;
    P.C = C;
    P.cnorm = cnorm;
    P.labels = labels;
    P.stop = stop;
    return P;
}

// host rows X[idx[i]] gathered into `dst` on the device (only those rows are shipped); synchronised, the staging vector is local
template <typename T>
static int gather_rows_host(DevBuf& dst, const T* X, const msm_idx_t* idx, msm_idx_t count, msm_idx_t m)
{
    std::vector<T> xb((size_t)count * m);
    for (msm_idx_t b = 0; b < count; ++b) memcpy(xb.data() + (size_t)b * m, X + idx[b] * m, (size_t)m * sizeof(T));
    const int rc = dst.reserve(xb.size() * sizeof(T));
    if (rc) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(dst.p, xb.data(), xb.size() * sizeof(T), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <typename T>
static int km_prepare(const T* centers, msm_idx_t K, msm_idx_t m, DevBuf& dC, T** dCent, T** dNorm)
{
    int rc = dC.reserve(((size_t)K * m + (size_t)K) * sizeof(T));
    if (rc) return rc;
    std::vector<T> cn((size_t)K);
    // (eight centres side by side: every centre's sum keeps its sequential order, the eight dependent chains overlap --
    //  one chain of 512 fp64 adds per centre was 0.6 ms of a K = 1000 x 512 call)
    msm_idx_t j = 0;
    for (; j + 8 <= K; j += 8) {
        double s8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const T* c0 = centers + j * m;
        for (msm_idx_t f = 0; f < m; ++f)
            for (int q = 0; q < 8; ++q) s8[q] += (double)c0[q * m + f] * (double)c0[q * m + f];
        for (int q = 0; q < 8; ++q) cn[(size_t)(j + q)] = (T)s8[q];
    }
    for (; j < K; ++j) {
        double s = 0.0;
        for (msm_idx_t f = 0; f < m; ++f) s += (double)centers[j * m + f] * (double)centers[j * m + f];
        cn[(size_t)j] = (T)s;
    }
    *dCent = dC.as<T>();
    *dNorm = *dCent + (size_t)K * m;
    // (2 MB of centres from pageable memory: 0.32 ms through hipMemcpyAsync's own staging, 0.1 ms through the library's pinned ring)
    {
        const int rcu = h2d_bulk(*dCent, centers, (size_t)K * m * sizeof(T));
        if (rcu) return rcu;
    }
    MSM_HIP_CHECK(hipMemcpyAsync(*dNorm, cn.data(), (size_t)K * sizeof(T), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));  // `cn` is a stack-frame vector
    return MSM_OK;
}

// small-batch step kernels of the handle entries (MSM_MBK_SMALL=0: general kernels)
static bool mbk_small_off()
{
    static const bool off = getenv("MSM_MBK_SMALL") && atoi(getenv("MSM_MBK_SMALL")) == 0;
    return off;
}

// What one labelling call launches.  `span` goes to the kernel as jspan when the launch is split.
struct KmPlan {
    int kernel = MSM_KM_SCALAR;   // MSM_KM_*
    int nsplit = 1;               // centre splits (1: none)
    long long span = 0;           // centres per split
    dim3 grid;
    int nb = 0;                   // inertia partials (0: labels only)
};

// The ONE place where a shape picks its kernel.  Pure: no HIP call, no device pointer (aligned16: the rows' and the
// centres' base addresses are 16-byte aligned; gathered: rows are read through an index list; handle_entry: msm_mbk_label /
// _step / _run* as against the stateless msm_kmeans_label_* / msm_mbk_step_*).
static KmPlan km_plan(long long n, long long m, long long K, bool f64, bool aligned16, bool gathered, bool handle_entry,
                      bool want_inertia)
{
    KmPlan pl;
    const long long rowblocks = ceil_div(n, KR), ctiles = ceil_div(K, KCT);   // (KR = DKR = 128, KCT = DKC = 128)
    // ENTRY-DEPENDENT: handle entries sum the inertia over min(n/4, 1024) partials, stateless ones over min(n/8, 2048); the inertia's bits depend on it
    if (want_inertia) pl.nb = (int)(handle_entry ? std::min<long long>(ceil_div(n, 4), 1024) : std::min<long long>(ceil_div(n, 8), 2048));
    const bool small_on = handle_entry && !f64 && !mbk_small_off();
    if (small_on && want_inertia && m <= 32 && n <= 65536) {  // MiniBatchKMeans' inner loop: the two-launch small-batch step
        const long long rb = ceil_div(n, 64);   // at most 1024 row blocks of 64
        const long long ns = std::max<long long>(1, std::min<long long>(ceil_div(512, rb), ceil_div(K, 16)));
        pl.kernel = MSM_KM_SMALL;
        pl.span = std::min<long long>(ceil_div(K, ns), SBC);
        pl.nsplit = (int)ceil_div(K, pl.span);
        pl.grid = dim3((unsigned)rb, (unsigned)pl.nsplit);
        pl.nb = (int)rb;   // (one partial per row block, written by the label kernel itself)
        return pl;
    }
    if (small_on && n <= 4096 && m > 32) {  // small batch of wide rows: 64 x 64 tiles fill the chip
        const long long rb = ceil_div(n, KS64), ct = ceil_div(K, KS64);
        const long long tiles_per = ceil_div(ct, std::min<long long>(ct, std::max<long long>(1, ceil_div(512, rb))));
        pl.kernel = MSM_KM_LABEL64;
        pl.nsplit = (int)ceil_div(ct, tiles_per);
        pl.span = tiles_per * KS64;
        pl.grid = dim3((unsigned)rb, (unsigned)pl.nsplit);
        return pl;
    }
    // the 16-byte fast path: when the row pitch and both base pointers allow it
    const bool v4 = aligned16 && m >= 4 && (m & 3) == 0 && m < (1 << 22);
    pl.kernel = f64 ? MSM_KM_F64 : v4 ? MSM_KM_V4 : MSM_KM_SCALAR;
    // Centre splits of a SMALL batch (fewer row blocks than the chip has workgroup slots): the centre tiles are spread over
    // blockIdx.y so that the launch fills the chip.  float64 rows: ONE kernel for every shape, this is all there is to decide.
    // ENTRY-DEPENDENT: float32 rows are split like this by the handle entries only, the stateless ones walk all centres; labels near a tie and the inertia's bits depend on it
    if (f64 || handle_entry) {
        int ns = 1;
        if (rowblocks < 256 && ctiles > 1) ns = (int)std::min<long long>(ctiles, std::max<long long>(1, 512 / rowblocks));
        const long long tiles_per = ceil_div(ctiles, ns);
        pl.nsplit = (int)ceil_div(ctiles, tiles_per);
        pl.span = tiles_per * KCT;
        pl.grid = dim3((unsigned)rowblocks, (unsigned)pl.nsplit);
        if (f64 || pl.nsplit > 1) return pl;
    }
    // Large batches of wide rows (the final labelling pass of BASELINE configs[3]: 1.25M x 512 per rank, K = 1000): one workgroup
    // per (row block, centre tile group), the groups of a row block side by side on one XCD, so that the rows are fetched ONCE
    // (kmeans_label_v4_kernel, P.xcd_ns); a workgroup takes FOUR tiles, the later passes over its rows being L2 hits.
    // MSM_LABEL_XCD = centre tiles per workgroup (0 = off: one workgroup walks all tiles; read per call: the A/B switch of
    // the tests, labels are identical either way).  Measured at 1.25M x 512, K = 1000 (fetched + written bytes per pass |
    // kernel | label + inertia call):
    //   all 8 tiles  21.3 GB = 8.3x the rows |  9.9 ms | 10.6 ms
    //   4 tiles      11.2 GB = 4.4x          | 10.1 ms | 10.9 ms      <- default
    //   2 tiles       5.3 GB = 2.1x          | 10.6 ms | 11.4 ms
    //   1 tile        3.4 GB                 | 11.8 ms | 12.7 ms
    // The kernel is MFMA-bound: the re-reads of the all-tiles form come out of the Infinity Cache and cost no time, while
    // every split pays the pipeline fill and the argmin epilogue once more per row block and adds a candidate merge to
    // the inertia pass.  Four tiles halve the traffic for 2-3 % of the call; two tiles cost 7 %.
    const char* xe = getenv("MSM_LABEL_XCD");
    const int xcd_tiles = xe ? atoi(xe) : 4;
    if (xcd_tiles > 0 && v4 && !f64 && !gathered && ctiles >= 2 && ctiles <= 16 && rowblocks >= 512 && m >= 64 &&
        ceil_div(rowblocks, 8) * 8 * ctiles < 0x7fffffffLL && ceil_div(ctiles, xcd_tiles) > 1) {
        pl.kernel = MSM_KM_V4_XCD;
        pl.nsplit = (int)ceil_div(ctiles, xcd_tiles);
        pl.span = ceil_div(ctiles, pl.nsplit) * KCT;
        pl.grid = dim3((unsigned)(ceil_div(rowblocks, 8) * 8 * pl.nsplit));
        return pl;
    }
    pl.nsplit = 1;
    pl.span = K;
    pl.grid = dim3((unsigned)rowblocks);
    return pl;
}

template <typename T>
static bool km_aligned16(const KmArgsT<T>& P)
{
    return (((uintptr_t)P.X | (uintptr_t)P.C) & 15) == 0;
}

// Carries a plan out on stream(): kernel attributes, the label launch (candidates of a split launch into pv / pi, [nsplit][n]
// each), then the merge -- kmeans_label_reduce_kernel when `partial` is null (labels only), else kmeans_inertia_kernel, which
// picks the labels from the candidates itself and leaves pl.nb partial sums in `partial`.  `small`: the handle's small-batch state.
template <typename T>
static int km_run_label(KmArgsT<T> P, const KmPlan& pl, DevBuf& pv, DevBuf& pi, double* partial, const SmallArgs* small = nullptr)
{
    int rc;
    // One split: the kernel writes the labels itself (jspan = 0).  The 64 x 64 kernel used to be handed a span here
    // whatever the number of its splits; with one split (K <= 64) it then wrote a candidate that kmeans_inertia_kernel
    // (which merges only when nsplit > 1) never read, and the step ran on whatever the label buffer held.
    const bool cand = pl.nsplit > 1;
    if (cand && pl.kernel != MSM_KM_SMALL) {
        if ((rc = pv.reserve((size_t)pl.nsplit * P.n * sizeof(T)))) return rc;
        if ((rc = pi.reserve((size_t)pl.nsplit * P.n * sizeof(int)))) return rc;
        P.jspan = pl.span;
        P.xcd_ns = pl.kernel == MSM_KM_V4_XCD ? pl.nsplit : 0;
        P.pv = pv.as<T>();
        P.pi = pi.as<int>();
    }
    if constexpr (std::is_same<T, double>::value) {
        static bool attr_set = false;
        if (!attr_set) {
            MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_label_f64_kernel),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)DK_LDS));
            attr_set = true;
        }
        hipLaunchKernelGGL(kmeans_label_f64_kernel, pl.grid, dim3(KNT), DK_LDS, stream(), P);
    } else if (pl.kernel == MSM_KM_SMALL) {
        if (!small || !partial) return fail(MSM_ERR_STATE, "kmeans: the small-batch step needs a handle and an inertia");
        SmallArgs S = *small;
        S.partial = partial;
        S.ns = pl.nsplit;
        S.cper = (int)pl.span;
        switch ((int)ceil_div(P.m, 4)) {
#define MSM_SL(G_) case G_: hipLaunchKernelGGL(mbk_small_label_kernel<G_>, pl.grid, dim3(KNT), 0, stream(), P, S); break;
            MSM_SL(1) MSM_SL(2) MSM_SL(3) MSM_SL(4) MSM_SL(5) MSM_SL(6) MSM_SL(7) MSM_SL(8)
#undef MSM_SL
        }
        MSM_HIP_CHECK(hipGetLastError());
        return MSM_OK;   // (labels and partials are written by the last workgroup of each row block)
    } else if (pl.kernel == MSM_KM_LABEL64) {
        static bool attr64 = false;
        if (!attr64) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_label64_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)KM64_LDS);
            attr64 = true;
        }
        hipLaunchKernelGGL(kmeans_label64_kernel, pl.grid, dim3(KNT), KM64_LDS, stream(), P);
    } else if (pl.kernel == MSM_KM_SCALAR) {
        hipLaunchKernelGGL(kmeans_label_kernel, pl.grid, dim3(KNT), 0, stream(), P);
    } else {
        static bool attr_set = false;
        if (!attr_set) {
            MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_label_v4_kernel<false>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)KM4_LDS));
            MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kmeans_label_v4_kernel<true>),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)KM4_LDS));
            attr_set = true;
        }
        if (P.rows)
            hipLaunchKernelGGL(kmeans_label_v4_kernel<true>, pl.grid, dim3(KNT), KM4_LDS, stream(), P);
        else
            hipLaunchKernelGGL(kmeans_label_v4_kernel<false>, pl.grid, dim3(KNT), KM4_LDS, stream(), P);
    }
    MSM_HIP_CHECK(hipGetLastError());
    if (cand && !partial)
        hipLaunchKernelGGL(kmeans_label_reduce_kernel<T>, dim3((unsigned)ceil_div(P.n, 256)), dim3(256), 0, stream(), P.pv, P.pi, P.n,
                           pl.nsplit, P.labels, P.stop);
    if (partial)
        hipLaunchKernelGGL(kmeans_inertia_kernel<T>, dim3(pl.nb), dim3(KNT), 0, stream(), P, partial, pl.nsplit);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// the inertia: the partial sums of km_run_label added up on the host, in order (synchronises)
static int km_sum_partials(const double* partial, int nb, double* inertia)
{
    std::vector<double> h((size_t)nb);
    MSM_HIP_CHECK(hipMemcpyAsync(h.data(), partial, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    double s = 0.0;
    for (int i = 0; i < nb; ++i) s += h[(size_t)i];
    *inertia = s;
    return MSM_OK;
}

// stateless entries: candidates in the pool's PS_W / PS_S, partials in PS_PART
template <typename T>
static int km_label_and_inertia(const KmArgsT<T>& P, double* inertia)
{
    const KmPlan pl = km_plan(P.n, P.m, P.K, sizeof(T) == 8, km_aligned16(P), P.rows != nullptr, false, inertia != nullptr);
    DevBuf& dPart = pool(PS_PART);
    int rc;
    if (inertia && (rc = dPart.reserve((size_t)pl.nb * sizeof(double)))) return rc;
    if ((rc = km_run_label<T>(P, pl, pool(PS_W), pool(PS_S), inertia ? dPart.as<double>() : nullptr))) return rc;
    return inertia ? km_sum_partials(dPart.as<double>(), pl.nb, inertia) : MSM_OK;
}

}  // namespace msm

using namespace msm;

// Device-resident MiniBatchKMeans state: centres, cumulative counts and ||c||^2 live in HBM for the
// whole fit; a step moves only the batch indices in and [inertia | counts] out.  `f64`: the rows' (and therefore the
// centres', counts' and norms') type -- scikit-learn works in the type of X (float32 stays float32, everything else is
// float64); the typed pointers below are `float*` or `double*` accordingly (cen<T>() ...).
struct msm_mbk {
    long long K = 0, m = 0;
    int f64 = 0;
    void* centers = nullptr;
    void* counts = nullptr;
    void* cnorm = nullptr;
    double* packed = nullptr;  // [K*m | K | 1] batch sums, counts, inertia (fp64)
    char* outbuf = nullptr;    // [8 + sizeof(T) K]
    DevBuf labels, idx, xb, pv, pi, part, rows, which;
    DevBuf arrive;             // small-batch step: per-row-block arrival counters (zero between launches)
    size_t arrive_zeroed = 0;
    // msm_mbk_run: [6 doubles of convergence state | S inertias] and the stop flag on the device; pinned host mirror
    DevBuf runbuf;
    int* stop = nullptr;
    char* pinned = nullptr;
    size_t pinned_bytes = 0;
    const char* run_out = nullptr;   // msm_mbk_run_begin .. _end: where the run in flight leaves its results (in `pinned`)
    size_t run_st_bytes = 0;
    size_t esz() const { return f64 ? sizeof(double) : sizeof(float); }
    template <typename T> T* cen() { return static_cast<T*>(centers); }
    template <typename T> T* cnt() { return static_cast<T*>(counts); }
    template <typename T> T* nrm() { return static_cast<T*>(cnorm); }
};

namespace {

// argument block of the handle's kernels on n rows of X: its centres and norms, labels into h->labels
template <typename T>
KmArgsT<T> mbk_args(msm_mbk* h, const T* X, const msm_idx_t* rows, long long n, const int* stop)
{
    return km_args<T>(X, rows, n, h->m, h->K, h->cen<T>(), h->nrm<T>(), h->labels.as<int32_t>(), stop);
}

// centre update of a step: one wave per centre for small batches (at most MSU_CAP rows), else one workgroup per centre
template <typename T>
void mbk_launch_update(msm_mbk* h, const KmArgsT<T>& P, double* sums, double* cnts, int apply, const MbkConv& cv)
{
    if (!mbk_small_off() && P.n <= MSU_CAP)
        hipLaunchKernelGGL(mbk_small_update_kernel<T>, dim3((unsigned)ceil_div(h->K, 4)), dim3(KNT), 0, stream(), P, h->cen<T>(),
                           h->cnt<T>(), h->nrm<T>(), sums, cnts, apply, cv);
    else
        hipLaunchKernelGGL(mbk_update_kernel<T>, dim3((unsigned)h->K), dim3(KNT), 4096 * sizeof(int), stream(), P, h->cen<T>(),
                           h->cnt<T>(), h->nrm<T>(), sums, cnts, apply, cv);
}

// handle entries: label P's rows (into P.labels) with candidates in h->pv / h->pi; want_inertia: *nb partials into h->part
template <typename T>
int mbk_run_label(msm_mbk* h, const KmArgsT<T>& P, bool want_inertia, int* nb)
{
    const KmPlan pl = km_plan(P.n, P.m, P.K, sizeof(T) == 8, km_aligned16(P), P.rows != nullptr, true, want_inertia);
    int rc;
    SmallArgs S{};
    if (pl.kernel == MSM_KM_SMALL) {
        if (h->arrive_zeroed == 0) {  // [1024 arrival counters = 0 | 65536 candidate words = all ones], once
            if ((rc = h->arrive.reserve((size_t)1024 * sizeof(unsigned) + (size_t)65536 * sizeof(unsigned long long)))) return rc;
            MSM_HIP_CHECK(hipMemsetAsync(h->arrive.p, 0, 1024 * sizeof(unsigned), stream()));
            MSM_HIP_CHECK(hipMemsetAsync(static_cast<char*>(h->arrive.p) + 1024 * sizeof(unsigned), 0xff, (size_t)65536 * sizeof(unsigned long long), stream()));
            h->arrive_zeroed = 1;
        }
        S.arrive = h->arrive.as<unsigned>();
        S.cand = reinterpret_cast<unsigned long long*>(static_cast<char*>(h->arrive.p) + 1024 * sizeof(unsigned));
    }
    if ((rc = h->part.reserve(1024 * sizeof(double)))) return rc;
    *nb = pl.nb;
    return km_run_label<T>(P, pl, h->pv, h->pi, want_inertia ? h->part.as<double>() : nullptr, &S);
}

// stage the batch in h->xb: device X -> gathered by a kernel through the uploaded indices; host X -> gathered on the host
template <typename T>
int mbk_stage_batch(msm_mbk* h, const T* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t B, int on_device)
{
    int rc;
    for (msm_idx_t b = 0; b < B; ++b)
        if (batch_idx[b] < 0 || batch_idx[b] >= n) return fail(MSM_ERR_INVALID, "mbk: batch index out of range");
    if (!on_device) return gather_rows_host<T>(h->xb, X, batch_idx, B, h->m);
    if ((rc = h->idx.reserve((size_t)B * sizeof(msm_idx_t)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(h->idx.p, batch_idx, (size_t)B * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));  // batch_idx is caller-owned pageable memory
    if ((rc = h->xb.reserve((size_t)B * h->m * sizeof(T)))) return rc;
    hipLaunchKernelGGL(mbk_gather_kernel<T>, dim3((unsigned)ceil_div(B, 4)), dim3(KNT), 0, stream(), X, h->idx.as<msm_idx_t>(),
                       (long long)B, (long long)h->m, h->xb.as<T>());
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

template <typename T>
void mbk_launch_cnorm(msm_mbk* h)
{
    hipLaunchKernelGGL(kmeans_cnorm_kernel<T>, dim3((unsigned)ceil_div(h->K, 4)), dim3(KNT), 0, stream(), h->cen<T>(), h->K, h->m, h->nrm<T>());
}
template <typename T>
void mbk_launch_apply(msm_mbk* h, const int* stop)
{
    hipLaunchKernelGGL(mbk_apply_kernel<T>, dim3((unsigned)h->K), dim3(256), 0, stream(), h->cen<T>(), h->cnt<T>(), h->packed, h->K, h->m, stop);
    mbk_launch_cnorm<T>(h);
}
template <typename T>
void mbk_launch_finish(msm_mbk* h, int nb, double* d_inertia)
{
    hipLaunchKernelGGL(mbk_finish_kernel<T>, dim3(1), dim3(KNT), 0, stream(), h->part.as<double>(), nb, h->cnt<T>(), h->K,
                       d_inertia, reinterpret_cast<T*>(h->outbuf + 8));
}

template <typename T>
int mbk_step_t(msm_mbk* h, const T* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t B,
               double* batch_inertia, T* counts_out, int apply_update, int on_device)
{
    int rc;
    if ((rc = mbk_stage_batch<T>(h, X, n, batch_idx, B, on_device))) return rc;
    if ((rc = h->labels.reserve((size_t)B * sizeof(int32_t)))) return rc;
    const KmArgsT<T> P = mbk_args<T>(h, h->xb.as<T>(), nullptr, B, nullptr);
    int nb = 0;
    if ((rc = mbk_run_label<T>(h, P, true, &nb))) return rc;
    mbk_launch_update<T>(h, P, apply_update ? (double*)nullptr : h->packed,
                         apply_update ? (double*)nullptr : h->packed + (size_t)h->K * h->m, apply_update, MbkConv{});
    MSM_HIP_CHECK(hipGetLastError());
    double* d_inertia = apply_update ? reinterpret_cast<double*>(h->outbuf) : h->packed + (size_t)h->K * h->m + h->K;
    mbk_launch_finish<T>(h, nb, d_inertia);
    MSM_HIP_CHECK(hipGetLastError());
    std::vector<char> hb(8 + (size_t)h->K * sizeof(T));
    if (apply_update) {
        MSM_HIP_CHECK(hipMemcpyAsync(hb.data(), h->outbuf, hb.size(), hipMemcpyDeviceToHost, stream()));
    } else {
        MSM_HIP_CHECK(hipMemcpyAsync(hb.data(), d_inertia, 8, hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(hb.data() + 8, h->outbuf + 8, (size_t)h->K * sizeof(T), hipMemcpyDeviceToHost, stream()));
    }
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (batch_inertia) memcpy(batch_inertia, hb.data(), 8);
    if (counts_out) memcpy(counts_out, hb.data() + 8, (size_t)h->K * sizeof(T));
    return MSM_OK;
}

// ---- the scaffold of a queued run (msm_mbk_run_begin / msm_mbk_run_sharded) ----
// Pinned mirror: [indices (idx_bytes) | initial state (64) | results: 6 state doubles + S inertias (st_bytes) | stop flag (8) | counts].

// everything a run allocates but its batch rows: the pinned mirror (regrown), the {stop flag, arrival counter} pair, the device buffers
template <typename T>
int mbk_run_reserve(msm_mbk* h, size_t idx_bytes, msm_idx_t S, msm_idx_t B, size_t* st_bytes)
{
    int rc;
    *st_bytes = (6 + (size_t)S) * sizeof(double);
    const size_t need = idx_bytes + 64 + *st_bytes + sizeof(int) + 4 + (size_t)h->K * sizeof(T);
    if (h->pinned_bytes < need) {
        if (h->pinned) (void)hipHostFree(h->pinned);
        h->pinned = nullptr;
        h->pinned_bytes = 0;
        MSM_HIP_CHECK(hipHostMalloc((void**)&h->pinned, need, hipHostMallocDefault));
        h->pinned_bytes = need;
    }
    if (!h->stop) MSM_HIP_CHECK(hipMalloc((void**)&h->stop, 2 * sizeof(int)));
    if ((rc = h->idx.reserve(idx_bytes))) return rc;
    if ((rc = h->runbuf.reserve(*st_bytes))) return rc;
    if ((rc = h->labels.reserve((size_t)B * sizeof(int32_t)))) return rc;
    return h->part.reserve(1024 * sizeof(double));
}

// in: the indices of all batches, the convergence state (steps_done restarts at 0), a zeroed stop pair -- through the pinned mirror
int mbk_run_upload(msm_mbk* h, const msm_idx_t* idx, msm_idx_t count, size_t idx_bytes, const double* state6)
{
    if (count > 0) {
        memcpy(h->pinned, idx, (size_t)count * sizeof(msm_idx_t));
        MSM_HIP_CHECK(hipMemcpyAsync(h->idx.p, h->pinned, (size_t)count * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
    }
    double* st0 = reinterpret_cast<double*>(h->pinned + idx_bytes);
    for (int i = 0; i < 5; ++i) st0[i] = state6[i];
    st0[5] = 0.0;
    MSM_HIP_CHECK(hipMemcpyAsync(h->runbuf.p, st0, 6 * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemsetAsync(h->stop, 0, 2 * sizeof(int), stream()));
    return MSM_OK;
}

// the convergence bookkeeping of step `step_index` over the nb inertia partials at `partial`
MbkConv mbk_conv_for_step(msm_mbk* h, const double* partial, int nb, msm_idx_t step_index, msm_idx_t B, double alpha,
                          msm_idx_t max_no_improvement)
{
    MbkConv cv;
    cv.partial = partial;
    cv.nb = nb;
    cv.st = h->runbuf.as<double>();
    cv.stop = h->stop;
    cv.inertias = cv.st + 6;
    cv.done = reinterpret_cast<unsigned*>(h->stop + 1);
    cv.step_index = (long long)step_index;
    cv.batch_size = (double)B;
    cv.alpha = alpha;
    cv.max_no_improvement = (long long)max_no_improvement;
    return cv;
}

// out: [state | inertias | stop | counts] into the pinned mirror, queued; mbk_run_finish waits for them
template <typename T>
int mbk_run_download(msm_mbk* h, size_t idx_bytes, size_t st_bytes)
{
    char* o = h->pinned + idx_bytes + 64;
    MSM_HIP_CHECK(hipMemcpyAsync(o, h->runbuf.p, st_bytes, hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(o + st_bytes, h->stop, sizeof(int), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(o + st_bytes + 8, h->counts, (size_t)h->K * sizeof(T), hipMemcpyDeviceToHost, stream()));
    h->run_out = o;
    h->run_st_bytes = st_bytes;
    return MSM_OK;
}

// one synchronisation for the whole run, then the results go from the pinned mirror to the caller
int mbk_run_finish(msm_mbk* h, double* state6, msm_idx_t* steps_done, int* converged, double* inertias, void* counts_out)
{
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    const char* o = h->run_out;
    const size_t st_bytes = h->run_st_bytes;
    h->run_out = nullptr;
    const double* so = reinterpret_cast<const double*>(o);
    for (int i = 0; i < 6; ++i) state6[i] = so[i];
    *steps_done = (msm_idx_t)so[5];
    memcpy(inertias, so + 6, (size_t)(*steps_done) * sizeof(double));
    *converged = *reinterpret_cast<const int*>(o + st_bytes);
    if (counts_out) memcpy(counts_out, o + st_bytes + 8, (size_t)h->K * h->esz());
    return MSM_OK;
}

template <typename T>
int mbk_run_begin_t(msm_mbk* h, const T* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t S, msm_idx_t B,
                    msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement, const double* state6)
{
    for (msm_idx_t b = 0; b < S * B; ++b)
        if (batch_idx[b] < 0 || batch_idx[b] >= n) return fail(MSM_ERR_INVALID, "mbk: batch index out of range");
    int rc;
    const size_t idx_bytes = (size_t)S * B * sizeof(msm_idx_t);
    size_t st_bytes = 0;
    if ((rc = mbk_run_reserve<T>(h, idx_bytes, S, B, &st_bytes))) return rc;
    if ((rc = mbk_run_upload(h, batch_idx, S * B, idx_bytes, state6))) return rc;
    // all S batches into one compact buffer (one launch), so that a step's kernels read contiguous rows
    if ((rc = h->xb.reserve((size_t)S * B * h->m * sizeof(T)))) return rc;
    hipLaunchKernelGGL(mbk_gather_kernel<T>, dim3((unsigned)ceil_div(S * B, 4)), dim3(KNT), 0, stream(), X, h->idx.as<msm_idx_t>(),
                       (long long)(S * B), (long long)h->m, h->xb.as<T>());
    MSM_HIP_CHECK(hipGetLastError());
    for (msm_idx_t s = 0; s < S; ++s) {
        const KmArgsT<T> P = mbk_args<T>(h, h->xb.as<T>() + (size_t)s * B * h->m, nullptr, B, h->stop);
        int nb = 0;
        if ((rc = mbk_run_label<T>(h, P, true, &nb))) return rc;
        mbk_launch_update<T>(h, P, nullptr, nullptr, 1,
                             mbk_conv_for_step(h, h->part.as<double>(), nb, first_step + s, B, alpha, max_no_improvement));
        MSM_HIP_CHECK(hipGetLastError());
    }
    return mbk_run_download<T>(h, idx_bytes, st_bytes);
}

template <typename T>
int mbk_run_sharded_t(msm_mbk* h, const T* X, msm_idx_t n_local, const msm_idx_t* local_idx, const msm_idx_t* offsets,
                      msm_idx_t S, msm_idx_t B, msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement,
                      double* state6, msm_idx_t* steps_done, int* converged, double* inertias, T* counts_out)
{
    // Everything that can fail on ONE rank -- argument checks, allocations -- happens before the first collective, and the
    // ranks agree on the outcome with one all-reduced flag: a rank that returned early on its own would leave the others
    // blocked inside the first step's all-reduce.
    msm_idx_t total = 0;
    size_t idx_bytes = 0, st_bytes = 0;
    auto prepare = [&]() -> int {
        if (n_local < 0 || B < 1 || S < 1 || S > 4096) return fail(MSM_ERR_INVALID, "msm_mbk_run_sharded: bad shape");
        total = offsets[S];
        if (offsets[0] != 0 || total < 0 || (total > 0 && (!local_idx || !X))) return fail(MSM_ERR_INVALID, "msm_mbk_run_sharded: bad offsets");
        for (msm_idx_t s = 0; s < S; ++s)
            if (offsets[s + 1] < offsets[s]) return fail(MSM_ERR_INVALID, "msm_mbk_run_sharded: offsets must not decrease");
        for (msm_idx_t b = 0; b < total; ++b)
            if (local_idx[b] < 0 || local_idx[b] >= n_local) return fail(MSM_ERR_INVALID, "mbk: batch index out of range");
        int rc;
        idx_bytes = (size_t)std::max<msm_idx_t>(total, 1) * sizeof(msm_idx_t);
        if ((rc = mbk_run_reserve<T>(h, idx_bytes, S, B, &st_bytes))) return rc;
        if (total > 0 && (rc = h->xb.reserve((size_t)total * h->m * sizeof(T)))) return rc;
        return MSM_OK;
    };
    int rc = prepare();
    if (comm_active()) {
        const double mine = rc ? 1.0 : 0.0;
        double failed = 0.0;
        MSM_HIP_CHECK(hipMemcpyAsync(h->packed, &mine, sizeof(double), hipMemcpyHostToDevice, stream()));
        const int rca = comm_allreduce_f64(h->packed, 1);
        if (rca) return rca;
        MSM_HIP_CHECK(hipMemcpyAsync(&failed, h->packed, sizeof(double), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        if (!rc && failed > 0.0) return fail(MSM_ERR_STATE, "msm_mbk_run_sharded: %d other rank(s) rejected their arguments or ran out of memory", (int)failed);
    }
    if (rc) return rc;
    if ((rc = mbk_run_upload(h, local_idx, total, idx_bytes, state6))) return rc;
    if (total > 0) {
        hipLaunchKernelGGL(mbk_gather_kernel<T>, dim3((unsigned)ceil_div(total, 4)), dim3(KNT), 0, stream(), X, h->idx.as<msm_idx_t>(),
                           (long long)total, (long long)h->m, h->xb.as<T>());
        MSM_HIP_CHECK(hipGetLastError());
    }
    const size_t psz = (size_t)msm_mbk_packed_size(h);
    double* d_inertia = h->packed + (size_t)h->K * h->m + h->K;
    for (msm_idx_t s = 0; s < S; ++s) {
        const msm_idx_t Bs = offsets[s + 1] - offsets[s];
        MSM_HIP_CHECK(hipMemsetAsync(h->packed, 0, psz * sizeof(double), stream()));
        if (Bs > 0) {
            const KmArgsT<T> P = mbk_args<T>(h, h->xb.as<T>() + (size_t)offsets[s] * h->m, nullptr, Bs, h->stop);
            int nb = 0;
            if ((rc = mbk_run_label<T>(h, P, true, &nb))) return rc;
            mbk_launch_update<T>(h, P, h->packed, h->packed + (size_t)h->K * h->m, 0, MbkConv{});
            MSM_HIP_CHECK(hipGetLastError());
            mbk_launch_finish<T>(h, nb, d_inertia);
            MSM_HIP_CHECK(hipGetLastError());
        }
        if ((rc = comm_allreduce_f64(h->packed, psz))) return rc;
        mbk_launch_apply<T>(h, h->stop);
        // the convergence bookkeeping of the step on the ALL-REDUCED batch inertia
        hipLaunchKernelGGL(mbk_conv_kernel, dim3(1), dim3(KNT), 0, stream(),
                           mbk_conv_for_step(h, d_inertia, 1, first_step + s, B, alpha, max_no_improvement));
        MSM_HIP_CHECK(hipGetLastError());
    }
    if ((rc = mbk_run_download<T>(h, idx_bytes, st_bytes))) return rc;
    return mbk_run_finish(h, state6, steps_done, converged, inertias, counts_out);
}

template <typename T>
int mbk_reassign_t(msm_mbk* h, const T* X, msm_idx_t n, const msm_idx_t* rows, const msm_idx_t* which, msm_idx_t n_reassign,
                   double new_count, int on_device)
{
    int rc;
    const T* Xd = X;
    std::vector<msm_idx_t> r2(rows, rows + n_reassign);
    if (!on_device) {  // ship only the chosen rows
        if ((rc = gather_rows_host<T>(h->xb, X, rows, n_reassign, h->m))) return rc;
        for (msm_idx_t i = 0; i < n_reassign; ++i) r2[(size_t)i] = i;
        Xd = h->xb.as<T>();
    }
    if ((rc = h->rows.reserve((size_t)n_reassign * sizeof(msm_idx_t)))) return rc;
    if ((rc = h->which.reserve((size_t)n_reassign * sizeof(msm_idx_t)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(h->rows.p, r2.data(), (size_t)n_reassign * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(h->which.p, which, (size_t)n_reassign * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(mbk_reassign_kernel<T>, dim3((unsigned)n_reassign), dim3(256), 0, stream(), h->cen<T>(), h->cnt<T>(), Xd,
                       h->m, h->rows.as<msm_idx_t>(), h->which.as<msm_idx_t>(), (T)new_count);
    MSM_HIP_CHECK(hipGetLastError());
    mbk_launch_cnorm<T>(h);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <typename T>
int mbk_label_t(msm_mbk* h, const T* X, msm_idx_t n, int32_t* labels, double* inertia, int on_device)
{
    int rc;
    const T* Xd = X;
    int32_t* lab_d = labels;
    DevBuf &dX = pool(PS_X), &dL = pool(PS_LAB);
    if (!on_device) {
        if ((rc = dX.reserve((size_t)n * h->m * sizeof(T)))) return rc;
        if ((rc = dL.reserve((size_t)n * sizeof(int32_t)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n * h->m * sizeof(T)))) return rc;
        Xd = dX.as<T>();
        lab_d = dL.as<int32_t>();
    }
    KmArgsT<T> P = mbk_args<T>(h, Xd, nullptr, n, nullptr);
    P.labels = lab_d;
    int nb = 0;
    if ((rc = mbk_run_label<T>(h, P, inertia != nullptr, &nb))) return rc;
    if (!on_device) MSM_HIP_CHECK(hipMemcpyAsync(labels, lab_d, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    if (inertia) return km_sum_partials(h->part.as<double>(), nb, inertia);
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <typename T>
int kmeans_label_t(const T* X, msm_idx_t n, msm_idx_t m, const T* centers, msm_idx_t K, int32_t* labels, double* inertia, int on_device)
{
    if (!X || !centers || !labels) return fail(MSM_ERR_INVALID, "kmeans_label: null pointer");
    if (n < 0 || m < 1 || K < 1) return fail(MSM_ERR_INVALID, "kmeans_label: bad shape");
    if (inertia) *inertia = 0.0;
    if (n == 0) return MSM_OK;
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    DevBuf &dC = pool(PS_Y), &dX = pool(PS_X), &dL = pool(PS_LAB);
    T *dCent, *dNorm;
    int rc = km_prepare<T>(centers, K, m, dC, &dCent, &dNorm);
    if (rc) return rc;
    const T* Xd = X;
    int32_t* lab_d = labels;
    if (!on_device) {
        if ((rc = dX.reserve((size_t)n * m * sizeof(T)))) return rc;
        if ((rc = dL.reserve((size_t)n * sizeof(int32_t)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n * m * sizeof(T)))) return rc;
        Xd = dX.as<T>();
        lab_d = dL.as<int32_t>();
    }
    if ((rc = km_label_and_inertia<T>(km_args<T>(Xd, nullptr, n, m, K, dCent, dNorm, lab_d), inertia))) return rc;
    if (!on_device)
        MSM_HIP_CHECK(hipMemcpyAsync(labels, lab_d, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <typename T>
int mbk_step_stateless_t(const T* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* batch_idx, msm_idx_t B, T* centers, T* counts,
                         msm_idx_t K, double* batch_inertia, double* batch_sums, double* batch_counts, int apply_update, int on_device)
{
    if (!X || !batch_idx || !centers || !counts) return fail(MSM_ERR_INVALID, "mbk_step: null pointer");
    if (n < 1 || m < 1 || K < 1 || B < 1) return fail(MSM_ERR_INVALID, "mbk_step: bad shape");
    for (msm_idx_t b = 0; b < B; ++b)
        if (batch_idx[b] < 0 || batch_idx[b] >= n) return fail(MSM_ERR_INVALID, "mbk_step: batch index out of range");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    DevBuf &dC = pool(PS_Y), &dXb = pool(PS_X), &dIdx = pool(PS_IDX), &dL = pool(PS_LAB), &dW = pool(PS_PADX), &dS = pool(PS_PADY);
    T *dCent, *dNorm;
    int rc = km_prepare<T>(centers, K, m, dC, &dCent, &dNorm);
    if (rc) return rc;
    if ((rc = dL.reserve((size_t)B * sizeof(int32_t)))) return rc;
    const T* Xd = X;
    const msm_idx_t* rows_d = nullptr;
    if (on_device) {
        if ((rc = dIdx.reserve((size_t)B * sizeof(msm_idx_t)))) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(dIdx.p, batch_idx, (size_t)B * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
        rows_d = dIdx.as<msm_idx_t>();
    } else {
        if ((rc = gather_rows_host<T>(dXb, X, batch_idx, B, m))) return rc;
        Xd = dXb.as<T>();
    }
    const KmArgsT<T> P = km_args<T>(Xd, rows_d, B, m, K, dCent, dNorm, dL.as<int32_t>());
    if ((rc = km_label_and_inertia<T>(P, batch_inertia))) return rc;   // (uses PS_W / PS_S for split candidates)
    if ((rc = dW.reserve((size_t)K * sizeof(T)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(dW.p, counts, (size_t)K * sizeof(T), hipMemcpyHostToDevice, stream()));
    double *dSums = nullptr, *dCnts = nullptr;
    if (batch_sums || batch_counts) {
        if ((rc = dS.reserve(((size_t)K * m + (size_t)K) * sizeof(double)))) return rc;
        dSums = dS.as<double>();
        dCnts = dSums + (size_t)K * m;
    }
    hipLaunchKernelGGL(mbk_update_kernel<T>, dim3((unsigned)K), dim3(KNT), 4096 * sizeof(int), stream(), P,
                       dCent, dW.as<T>(), (T*)nullptr, dSums, dCnts, apply_update, MbkConv{});
    MSM_HIP_CHECK(hipGetLastError());
    if (apply_update) {
        MSM_HIP_CHECK(hipMemcpyAsync(centers, dCent, (size_t)K * m * sizeof(T), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(counts, dW.p, (size_t)K * sizeof(T), hipMemcpyDeviceToHost, stream()));
    }
    if (batch_sums)
        MSM_HIP_CHECK(hipMemcpyAsync(batch_sums, dSums, (size_t)K * m * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if (batch_counts)
        MSM_HIP_CHECK(hipMemcpyAsync(batch_counts, dCnts, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int mbk_create(msm_mbk_t** out, msm_idx_t K, msm_idx_t m, int f64)
{
    if (!out || K < 1 || m < 1) return fail(MSM_ERR_INVALID, "msm_mbk_create: bad argument");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    msm_mbk* h = new msm_mbk();
    h->K = K;
    h->m = m;
    h->f64 = f64 ? 1 : 0;
    const size_t e = h->esz();
    hipError_t er = hipMalloc(&h->centers, (size_t)K * m * e);
    if (er == hipSuccess) er = hipMalloc(&h->counts, (size_t)K * e);
    if (er == hipSuccess) er = hipMalloc(&h->cnorm, (size_t)K * e);
    if (er == hipSuccess) er = hipMalloc((void**)&h->packed, ((size_t)K * m + K + 1) * sizeof(double));
    if (er == hipSuccess) er = hipMalloc((void**)&h->outbuf, 8 + (size_t)K * e);
    if (er != hipSuccess) {
        msm_mbk_destroy(h);
        return fail(MSM_ERR_HIP, "msm_mbk_create: hipMalloc failed: %s", hipGetErrorString(er));
    }
    *out = h;
    return MSM_OK;
}

}  // namespace

// ---- KMeans: full-batch Lloyd iterations queued on the device ----
// The centres, their norms and the labelling scratch are those of an msm_mbk handle (labelling goes through mbk_run_label,
// exactly as msm_mbk_label does); the update's scratch is owned here, sized at the first run and reused.
struct msm_lloyd {
    msm_mbk* mbk = nullptr;
    DevBuf lab[2], order, hist, tabs, pk, partial, shiftsq, st, dist, far, reloc;
};

namespace msm {

// What the update of one iteration launches.  Pure: no HIP call.
struct LloydPlan {
    long long hist_span, groups, piece, pieces_max, ftiles, tile_features, vec, scratch_bytes;
    long long units;
    int tu;
};

static LloydPlan lloyd_plan(long long n, long long m, long long K, bool f64, bool aligned16)
{
    LloydPlan pl;
    const long long esz = f64 ? 8 : 4;
    pl.hist_span = LH_SPAN;
    pl.groups = ceil_div(n, LH_SPAN);
    pl.piece = LL_PIECE;
    pl.pieces_max = ceil_div(n, LL_PIECE) + K;
    pl.vec = (aligned16 && (m * esz) % 16 == 0) ? 1 : 0;
    const long long E = pl.vec ? 16 / esz : 1;
    pl.units = m / E;
    int tu = 1;
    while (tu < LL_TU && tu < pl.units) tu <<= 1;
    pl.tu = tu;
    pl.ftiles = ceil_div(pl.units, tu);
    pl.tile_features = tu * E;
    pl.scratch_bytes = 2 * n * 4 + n * 4 + K * pl.groups * 4 + (2 * (K + 1) * 8 + (K + 1) * 4) + pl.pieces_max * 4 +
                       pl.pieces_max * m * 8 + (K + 1) * 8 + LS_COUNT * 4;
    return pl;
}

}  // namespace msm

namespace {

template <typename T>
struct LloydRun {
    msm_lloyd* h;
    const T* X;
    long long n;
    LloydPlan pl;
    LloydArgs<T> A;
    long long* count;
    long long* start;
    int* pstart;
    int* st;
};

template <typename T>
int lloyd_reserve(LloydRun<T>& R, double tol_abs)
{
    msm_lloyd* h = R.h;
    msm_mbk* b = h->mbk;
    const long long K = b->K, m = b->m, n = R.n;
    int rc;
    for (int q = 0; q < 2; ++q)
        if ((rc = h->lab[q].reserve((size_t)n * sizeof(int32_t)))) return rc;
    if ((rc = h->order.reserve((size_t)n * sizeof(unsigned)))) return rc;
    if ((rc = h->hist.reserve((size_t)K * R.pl.groups * sizeof(unsigned)))) return rc;
    if ((rc = h->tabs.reserve((size_t)(2 * (K + 1)) * sizeof(long long) + (size_t)(K + 1) * sizeof(int)))) return rc;
    if ((rc = h->pk.reserve((size_t)R.pl.pieces_max * sizeof(int)))) return rc;
    if ((rc = h->partial.reserve((size_t)R.pl.pieces_max * m * sizeof(double)))) return rc;
    if ((rc = h->shiftsq.reserve((size_t)(K + 1) * sizeof(double)))) return rc;
    if ((rc = h->st.reserve(LS_COUNT * sizeof(int)))) return rc;
    R.count = h->tabs.as<long long>();
    R.start = R.count + (K + 1);
    R.pstart = reinterpret_cast<int*>(R.start + (K + 1));
    R.st = h->st.as<int>();
    LloydArgs<T>& A = R.A;
    memset(&A, 0, sizeof(A));
    A.X = R.X;
    A.n = n;
    A.m = m;
    A.K = K;
    A.C = b->cen<T>();
    A.cnorm = b->nrm<T>();
    A.order = h->order.as<unsigned>();
    A.count = R.count;
    A.start = R.start;
    A.pstart = R.pstart;
    A.pk = h->pk.as<int>();
    A.partial = h->partial.as<double>();
    A.shiftsq = h->shiftsq.as<double>();
    A.shift_out = A.shiftsq + K;
    A.st = R.st;
    A.tol = tol_abs;
    A.units = R.pl.units;
    A.tu = R.pl.tu;
    return MSM_OK;
}

// piece map -> sorted row numbers -> piece sums -> centres, norms, stop rules: everything behind lloyd_base_kernel, which a
// run that stopped for empty clusters has skipped and the relocation therefore queues again
template <typename T>
int lloyd_queue_sums(LloydRun<T>& R, const int32_t* cur)
{
    const LloydPlan& pl = R.pl;
    hipLaunchKernelGGL(lloyd_piecemap_kernel, dim3((unsigned)ceil_div(pl.pieces_max, KNT)), dim3(KNT), 0, stream(), R.pstart, R.A.K,
                       static_cast<int*>(R.h->pk.p), R.st);
    hipLaunchKernelGGL(lloyd_scatter_kernel, dim3((unsigned)pl.groups), dim3(64), 0, stream(), cur, R.n, R.A.K, pl.groups,
                       static_cast<const unsigned*>(R.h->hist.p), R.start, static_cast<unsigned*>(R.h->order.p), R.st);
    const dim3 grid((unsigned)pl.pieces_max, (unsigned)pl.ftiles);
    if (pl.vec) hipLaunchKernelGGL((lloyd_segsum_kernel<T, true>), grid, dim3(KNT), 0, stream(), R.A);
    else hipLaunchKernelGGL((lloyd_segsum_kernel<T, false>), grid, dim3(KNT), 0, stream(), R.A);
    hipLaunchKernelGGL(lloyd_finish_kernel<T>, dim3((unsigned)R.A.K), dim3(KNT), 0, stream(), R.A);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

template <typename T>
int lloyd_queue_iter(LloydRun<T>& R, long long it)
{
    msm_lloyd* h = R.h;
    int32_t* cur = h->lab[it & 1].as<int32_t>();
    const int32_t* prev = h->lab[(it + 1) & 1].as<int32_t>();
    KmArgsT<T> P = mbk_args<T>(h->mbk, R.X, nullptr, R.n, R.st + LS_STOP);
    P.labels = cur;
    int nb = 0, rc;
    if ((rc = mbk_run_label<T>(h->mbk, P, false, &nb))) return rc;
    const LloydPlan& pl = R.pl;
    hipLaunchKernelGGL(lloyd_hist_kernel, dim3((unsigned)pl.groups), dim3(64), 0, stream(), cur, prev, R.n, R.A.K, pl.groups,
                       h->hist.as<unsigned>(), R.st);
    hipLaunchKernelGGL(lloyd_scan_kernel, dim3((unsigned)R.A.K), dim3(KNT), 0, stream(), h->hist.as<unsigned>(), pl.groups, R.count, R.st);
    hipLaunchKernelGGL(lloyd_base_kernel, dim3(1), dim3(KNT), 0, stream(), R.count, R.A.K, R.start, R.pstart, R.st);
    MSM_HIP_CHECK(hipGetLastError());
    return lloyd_queue_sums<T>(R, cur);
}

// scikit-learn's _relocate_empty_clusters_dense for the iteration that stopped with LLOYD_EMPTY: the n_empty rows farthest
// from their own (old) centre, lowest row first among equals, leave their clusters and become the empty clusters, in
// ascending cluster order; then the iteration is finished.  X stays on the device; the K cluster sizes come to the host.
template <typename T>
int lloyd_relocate(LloydRun<T>& R, long long it)
{
    msm_lloyd* h = R.h;
    const long long K = R.A.K, n = R.n;
    std::vector<long long> cnt((size_t)K);
    MSM_HIP_CHECK(hipMemcpyAsync(cnt.data(), R.count, (size_t)K * sizeof(long long), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    std::vector<int> target;
    for (long long k = 0; k < K; ++k)
        if (cnt[(size_t)k] == 0) target.push_back((int)k);
    const int ne = (int)target.size();
    if (ne == 0) return fail(MSM_ERR_STATE, "msm_lloyd_run: a relocation without an empty cluster");
    const int NB = 256;
    int rc;
    if ((rc = h->dist.reserve((size_t)n * sizeof(double)))) return rc;
    if ((rc = h->far.reserve((size_t)NB * (sizeof(double) + sizeof(long long))))) return rc;
    if ((rc = h->reloc.reserve((size_t)ne * (sizeof(long long) + 2 * sizeof(int))))) return rc;
    long long* d_row = h->reloc.as<long long>();
    int* d_donor = reinterpret_cast<int*>(d_row + ne);
    int* d_target = d_donor + ne;
    MSM_HIP_CHECK(hipMemcpyAsync(d_target, target.data(), (size_t)ne * sizeof(int), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemsetAsync(R.st + LS_STOP, 0, sizeof(int), stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // `target` is a local vector
    const int32_t* cur = h->lab[it & 1].as<int32_t>();
    double* bv = h->far.as<double>();
    long long* bi = reinterpret_cast<long long*>(bv + NB);
    hipLaunchKernelGGL(lloyd_dist_kernel<T>, dim3((unsigned)ceil_div(n, 4)), dim3(KNT), 0, stream(), R.X, n, R.A.m, R.A.C, cur,
                       h->dist.as<double>());
    for (int q = 0; q < ne; ++q) {
        hipLaunchKernelGGL(lloyd_far_kernel, dim3(NB), dim3(KNT), 0, stream(), h->dist.as<double>(), n, bv, bi);
        hipLaunchKernelGGL(lloyd_take_kernel, dim3(1), dim3(KNT), 0, stream(), bv, bi, NB, n, h->dist.as<double>(), cur, q, d_row, d_donor);
    }
    MSM_HIP_CHECK(hipGetLastError());
    R.A.n_reloc = ne;
    R.A.reloc_row = d_row;
    R.A.reloc_donor = d_donor;
    R.A.reloc_target = d_target;
    rc = lloyd_queue_sums<T>(R, cur);
    R.A.n_reloc = 0;
    return rc;
}

template <typename T>
int lloyd_run_t(msm_lloyd* h, const T* X, msm_idx_t n, msm_idx_t max_iter, double tol_abs, int32_t* labels_out, int on_device,
                double* inertia, msm_idx_t* n_iter, int* status)
{
    msm_mbk* b = h->mbk;
    int rc;
    const T* Xd = X;
    int32_t* lab_d = labels_out;
    DevBuf &dX = pool(PS_X), &dL = pool(PS_LAB);
    if (!on_device) {
        if ((rc = dX.reserve((size_t)n * b->m * sizeof(T)))) return rc;
        if ((rc = dL.reserve((size_t)n * sizeof(int32_t)))) return rc;
        if ((rc = h2d_bulk(dX.p, X, (size_t)n * b->m * sizeof(T)))) return rc;
        Xd = dX.as<T>();
        lab_d = dL.as<int32_t>();
    }
    LloydRun<T> R;
    R.h = h;
    R.X = Xd;
    R.n = n;
    R.pl = lloyd_plan(n, b->m, b->K, sizeof(T) == 8, ((((uintptr_t)Xd) | ((uintptr_t)b->centers)) & 15) == 0);
    if ((rc = lloyd_reserve<T>(R, tol_abs))) return rc;
    if ((rc = b->part.reserve(1024 * sizeof(double)))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(R.st, 0, LS_COUNT * sizeof(int), stream()));
    MSM_HIP_CHECK(hipMemsetAsync(h->lab[1].p, 0xff, (size_t)n * sizeof(int32_t), stream()));   // "previous" labels of iteration 0: -1
    int hst[LS_COUNT];
    long long it = 0;
    for (int guard = 0;; ++guard) {
        for (long long i = it; i < max_iter; ++i)
            if ((rc = lloyd_queue_iter<T>(R, i))) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(hst, R.st, sizeof(hst), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        if (hst[LS_STOP] != LLOYD_EMPTY) break;
        if (guard > max_iter) return fail(MSM_ERR_STATE, "msm_lloyd_run: relocation does not advance");
        if ((rc = lloyd_relocate<T>(R, hst[LS_ITERS]))) return rc;
        it = (long long)hst[LS_ITERS] + 1;
    }
    const long long done = hst[LS_ITERS];
    *n_iter = done;
    *status = hst[LS_STOP];
    // the labels that are returned and the inertia: strict convergence keeps the last iteration's labels, every other end
    // labels once more against the final centres
    KmArgsT<T> P = mbk_args<T>(b, Xd, nullptr, n, nullptr);
    P.labels = lab_d;
    int nb = 0;
    if (hst[LS_STOP] == LLOYD_STRICT) {
        MSM_HIP_CHECK(hipMemcpyAsync(lab_d, h->lab[(done - 1) & 1].p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, stream()));
        nb = (int)std::min<long long>(ceil_div(n, 4), 1024);
        hipLaunchKernelGGL(kmeans_inertia_kernel<T>, dim3(nb), dim3(KNT), 0, stream(), P, b->part.as<double>(), 1);
        MSM_HIP_CHECK(hipGetLastError());
    } else if ((rc = mbk_run_label<T>(b, P, true, &nb))) {
        return rc;
    }
    if (!on_device) MSM_HIP_CHECK(hipMemcpyAsync(labels_out, lab_d, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream()));
    return km_sum_partials(b->part.as<double>(), nb, inertia);
}

}  // namespace

// dispatch on the handle's element type
#define MBK_TYPED(h, CALL_F32, CALL_F64) ((h)->f64 ? (CALL_F64) : (CALL_F32))

extern "C" {

int msm_mbk_create(msm_mbk_t** out, msm_idx_t K, msm_idx_t m) { return mbk_create(out, K, m, 0); }
int msm_mbk_create_f64(msm_mbk_t** out, msm_idx_t K, msm_idx_t m) { return mbk_create(out, K, m, 1); }
int msm_mbk_is_f64(msm_mbk_t* h) { return h ? h->f64 : 0; }

int msm_mbk_destroy(msm_mbk_t* h)
{
    if (!h) return MSM_OK;
    (void)hipStreamSynchronize(stream());
    if (h->centers) (void)hipFree(h->centers);
    if (h->counts) (void)hipFree(h->counts);
    if (h->cnorm) (void)hipFree(h->cnorm);
    if (h->packed) (void)hipFree(h->packed);
    if (h->outbuf) (void)hipFree(h->outbuf);
    if (h->stop) (void)hipFree(h->stop);
    if (h->pinned) (void)hipHostFree(h->pinned);
    delete h;
    return MSM_OK;
}

int msm_mbk_set(msm_mbk_t* h, const void* centers, const void* counts)
{
    if (!h || !centers || !counts) return fail(MSM_ERR_STATE, "msm_mbk_set: null argument");
    MSM_HIP_CHECK(hipMemcpyAsync(h->centers, centers, (size_t)h->K * h->m * h->esz(), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(h->counts, counts, (size_t)h->K * h->esz(), hipMemcpyHostToDevice, stream()));
    if (h->f64) mbk_launch_cnorm<double>(h);
    else mbk_launch_cnorm<float>(h);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_mbk_get(msm_mbk_t* h, void* centers, void* counts)
{
    if (!h) return fail(MSM_ERR_STATE, "msm_mbk_get: null handle");
    if (centers) MSM_HIP_CHECK(hipMemcpyAsync(centers, h->centers, (size_t)h->K * h->m * h->esz(), hipMemcpyDeviceToHost, stream()));
    if (counts) MSM_HIP_CHECK(hipMemcpyAsync(counts, h->counts, (size_t)h->K * h->esz(), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_mbk_step(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t B,
                 double* batch_inertia, void* counts_out, int apply_update, int on_device)
{
    if (!h || !X || !batch_idx) return fail(MSM_ERR_STATE, "msm_mbk_step: null argument");
    if (n < 1 || B < 1) return fail(MSM_ERR_INVALID, "msm_mbk_step: bad shape");
    return MBK_TYPED(h, mbk_step_t<float>(h, (const float*)X, n, batch_idx, B, batch_inertia, (float*)counts_out, apply_update, on_device),
                     mbk_step_t<double>(h, (const double*)X, n, batch_idx, B, batch_inertia, (double*)counts_out, apply_update, on_device));
}

/* msm_mbk_run in two halves: _begin queues the whole run (indices in, S steps, results out) and returns without waiting,
 * _end waits for it and hands the results over.  Between the two the host is free -- MiniBatchKMeans draws the NEXT run's
 * batch indices there (a quarter of a millisecond per 65,536 indices with the legacy RandomState, as long as a large-batch
 * step takes on the device). */
int msm_mbk_run_begin(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t S, msm_idx_t B,
                      msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement, const double* state6)
{
    if (!h || !X || !batch_idx || !state6) return fail(MSM_ERR_STATE, "msm_mbk_run: null argument");
    if (n < 1 || B < 1 || S < 1 || S > 4096) return fail(MSM_ERR_INVALID, "msm_mbk_run: bad shape");
    return MBK_TYPED(h, mbk_run_begin_t<float>(h, (const float*)X, n, batch_idx, S, B, first_step, alpha, max_no_improvement, state6),
                     mbk_run_begin_t<double>(h, (const double*)X, n, batch_idx, S, B, first_step, alpha, max_no_improvement, state6));
}

int msm_mbk_run_end(msm_mbk_t* h, double* state6, msm_idx_t* steps_done, int* converged, double* inertias, void* counts_out)
{
    if (!h || !state6 || !steps_done || !converged || !inertias) return fail(MSM_ERR_STATE, "msm_mbk_run_end: null argument");
    if (!h->run_out) return fail(MSM_ERR_STATE, "msm_mbk_run_end: no run in flight");
    return mbk_run_finish(h, state6, steps_done, converged, inertias, counts_out);
}

int msm_mbk_run(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t S, msm_idx_t B,
                msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement, double* state6,
                msm_idx_t* steps_done, int* converged, double* inertias, void* counts_out)
{
    if (!steps_done || !converged || !inertias) return fail(MSM_ERR_STATE, "msm_mbk_run: null argument");
    const int rc = msm_mbk_run_begin(h, X, n, batch_idx, S, B, first_step, alpha, max_no_improvement, state6);
    if (rc) return rc;
    return msm_mbk_run_end(h, state6, steps_done, converged, inertias, counts_out);
}

/* msm_mbk_run for a ROW-SHARDED fit (one process per GPU): the S batches are GLOBAL (identical on every rank); this rank
 * passes the rows of each batch that it owns as local row numbers -- local_idx (host) holds them back to back, offsets[S + 1]
 * (host) delimits the steps -- and the batch size B of the whole batch.  Per step: label + fp64 sums / counts / inertia of
 * the local rows, ONE all-reduce of the packed [K m sums | K counts | inertia] buffer over the library communicator (RCCL on
 * the library stream), the identical update and convergence step on every rank.  Nothing returns to the host inside the
 * run; every rank stops at the same step (the criterion sees the all-reduced inertia).  Outputs as msm_mbk_run. */
int msm_mbk_run_sharded(msm_mbk_t* h, const void* X, msm_idx_t n_local, const msm_idx_t* local_idx, const msm_idx_t* offsets,
                        msm_idx_t S, msm_idx_t B, msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement,
                        double* state6, msm_idx_t* steps_done, int* converged, double* inertias, void* counts_out)
{
    if (!h || !offsets || !state6 || !steps_done || !converged || !inertias) return fail(MSM_ERR_STATE, "msm_mbk_run_sharded: null argument");
    return MBK_TYPED(h, mbk_run_sharded_t<float>(h, (const float*)X, n_local, local_idx, offsets, S, B, first_step, alpha, max_no_improvement,
                                                 state6, steps_done, converged, inertias, (float*)counts_out),
                     mbk_run_sharded_t<double>(h, (const double*)X, n_local, local_idx, offsets, S, B, first_step, alpha, max_no_improvement,
                                                  state6, steps_done, converged, inertias, (double*)counts_out));
}

msm_idx_t msm_mbk_packed_size(msm_mbk_t* h) { return h ? (msm_idx_t)(h->K * h->m + h->K + 1) : 0; }

int msm_mbk_export_packed(msm_mbk_t* h, double* buf, int on_device)
{
    if (!h || !buf) return fail(MSM_ERR_STATE, "msm_mbk_export_packed: null argument");
    MSM_HIP_CHECK(hipMemcpyAsync(buf, h->packed, (size_t)msm_mbk_packed_size(h) * sizeof(double),
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_mbk_apply_packed(msm_mbk_t* h, const double* buf, void* counts_out, int on_device)
{
    if (!h || !buf) return fail(MSM_ERR_STATE, "msm_mbk_apply_packed: null argument");
    MSM_HIP_CHECK(hipMemcpyAsync(h->packed, buf, (size_t)msm_mbk_packed_size(h) * sizeof(double),
                                 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream()));
    if (h->f64) mbk_launch_apply<double>(h, nullptr);
    else mbk_launch_apply<float>(h, nullptr);
    MSM_HIP_CHECK(hipGetLastError());
    if (counts_out) MSM_HIP_CHECK(hipMemcpyAsync(counts_out, h->counts, (size_t)h->K * h->esz(), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

/* sharded step, exchange half: msm_mbk_step(apply_update = 0) left this rank's [K*m sums | K counts | inertia] of ITS
 * batch rows in the handle's device buffer (msm_mbk_zero_packed for a rank that owns none of them); one all-reduce over
 * the library communicator (RCCL on the library stream, device buffer, in place) and the reduced buffer is applied
 * identically on every rank.  *batch_inertia / counts_out (host, K): the global batch inertia and the updated counts. */
int msm_mbk_zero_packed(msm_mbk_t* h)
{
    if (!h) return fail(MSM_ERR_STATE, "msm_mbk_zero_packed: null handle");
    MSM_HIP_CHECK(hipMemsetAsync(h->packed, 0, (size_t)msm_mbk_packed_size(h) * sizeof(double), stream()));
    return MSM_OK;
}

int msm_mbk_allreduce(msm_mbk_t* h, double* batch_inertia, void* counts_out)
{
    if (!h) return fail(MSM_ERR_STATE, "msm_mbk_allreduce: null handle");
    int rc = comm_allreduce_f64(h->packed, (size_t)msm_mbk_packed_size(h));
    if (rc) return rc;
    if (h->f64) mbk_launch_apply<double>(h, nullptr);
    else mbk_launch_apply<float>(h, nullptr);
    MSM_HIP_CHECK(hipGetLastError());
    if (batch_inertia)
        MSM_HIP_CHECK(hipMemcpyAsync(batch_inertia, h->packed + (size_t)h->K * h->m + h->K, sizeof(double), hipMemcpyDeviceToHost, stream()));
    if (counts_out) MSM_HIP_CHECK(hipMemcpyAsync(counts_out, h->counts, (size_t)h->K * h->esz(), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_mbk_reassign(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* rows, const msm_idx_t* which,
                     msm_idx_t n_reassign, double new_count, int on_device)
{
    if (!h || !X || !rows || !which) return fail(MSM_ERR_STATE, "msm_mbk_reassign: null argument");
    if (n_reassign <= 0) return MSM_OK;
    for (msm_idx_t i = 0; i < n_reassign; ++i)
        if (rows[i] < 0 || rows[i] >= n || which[i] < 0 || which[i] >= h->K) return fail(MSM_ERR_INVALID, "msm_mbk_reassign: index out of range");
    return MBK_TYPED(h, mbk_reassign_t<float>(h, (const float*)X, n, rows, which, n_reassign, new_count, on_device),
                     mbk_reassign_t<double>(h, (const double*)X, n, rows, which, n_reassign, new_count, on_device));
}

int msm_mbk_set_counts(msm_mbk_t* h, const void* counts)
{
    if (!h || !counts) return fail(MSM_ERR_STATE, "msm_mbk_set_counts: null argument");
    MSM_HIP_CHECK(hipMemcpyAsync(h->counts, counts, (size_t)h->K * h->esz(), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_mbk_label(msm_mbk_t* h, const void* X, msm_idx_t n, int32_t* labels, double* inertia, int on_device)
{
    if (!h || !X || !labels) return fail(MSM_ERR_STATE, "msm_mbk_label: null argument");
    if (inertia) *inertia = 0.0;
    if (n <= 0) return MSM_OK;
    return MBK_TYPED(h, mbk_label_t<float>(h, (const float*)X, n, labels, inertia, on_device),
                     mbk_label_t<double>(h, (const double*)X, n, labels, inertia, on_device));
}

int msm_kmeans_label_plan(msm_idx_t n, msm_idx_t m, msm_idx_t K, int f64, int handle_entry, int want_inertia, int aligned, int gathered,
                          int* kernel, int* nsplit, msm_idx_t* span)
{
    if (n < 1 || m < 1 || K < 1 || !kernel || !nsplit || !span) return fail(MSM_ERR_INVALID, "msm_kmeans_label_plan: bad argument");
    const KmPlan pl = km_plan(n, m, K, f64 != 0, aligned != 0, gathered != 0, handle_entry != 0, want_inertia != 0);
    *kernel = pl.kernel;
    *nsplit = pl.nsplit;
    *span = pl.span;
    return MSM_OK;
}

int msm_kmeans_label_f32(const float* X, msm_idx_t n, msm_idx_t m, const float* centers,
                         msm_idx_t K, int32_t* labels, double* inertia, int on_device)
{
    return kmeans_label_t<float>(X, n, m, centers, K, labels, inertia, on_device);
}

int msm_kmeans_label_f64(const double* X, msm_idx_t n, msm_idx_t m, const double* centers,
                         msm_idx_t K, int32_t* labels, double* inertia, int on_device)
{
    return kmeans_label_t<double>(X, n, m, centers, K, labels, inertia, on_device);
}

int msm_mbk_step_f32(const float* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* batch_idx,
                     msm_idx_t B, float* centers, float* counts, msm_idx_t K,
                     double* batch_inertia, double* batch_sums, double* batch_counts,
                     int apply_update, int on_device)
{
    return mbk_step_stateless_t<float>(X, n, m, batch_idx, B, centers, counts, K, batch_inertia, batch_sums, batch_counts, apply_update, on_device);
}

int msm_mbk_step_f64(const double* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* batch_idx,
                     msm_idx_t B, double* centers, double* counts, msm_idx_t K,
                     double* batch_inertia, double* batch_sums, double* batch_counts,
                     int apply_update, int on_device)
{
    return mbk_step_stateless_t<double>(X, n, m, batch_idx, B, centers, counts, K, batch_inertia, batch_sums, batch_counts, apply_update, on_device);
}

/* ---- KMeans (full-batch Lloyd): see include/msmhip.h ---- */
static int lloyd_create(msm_lloyd_t** out, msm_idx_t K, msm_idx_t m, int f64)
{
    if (!out) return fail(MSM_ERR_INVALID, "msm_lloyd_create: bad argument");
    msm_mbk* b = nullptr;
    const int rc = mbk_create(&b, K, m, f64);
    if (rc) return rc;
    msm_lloyd* h = new msm_lloyd();
    h->mbk = b;
    *out = h;
    return MSM_OK;
}

int msm_lloyd_create(msm_lloyd_t** out, msm_idx_t K, msm_idx_t m) { return lloyd_create(out, K, m, 0); }
int msm_lloyd_create_f64(msm_lloyd_t** out, msm_idx_t K, msm_idx_t m) { return lloyd_create(out, K, m, 1); }

int msm_lloyd_destroy(msm_lloyd_t* h)
{
    if (!h) return MSM_OK;
    (void)msm_mbk_destroy(h->mbk);   // (synchronises the stream first)
    delete h;
    return MSM_OK;
}

int msm_lloyd_set_centers(msm_lloyd_t* h, const void* centers)
{
    if (!h || !centers) return fail(MSM_ERR_STATE, "msm_lloyd_set_centers: null argument");
    const std::vector<double> zero((size_t)h->mbk->K, 0.0);   // (all-zero bits: K zero counts of either type)
    return msm_mbk_set(h->mbk, centers, zero.data());
}

int msm_lloyd_get_centers(msm_lloyd_t* h, void* centers)
{
    if (!h || !centers) return fail(MSM_ERR_STATE, "msm_lloyd_get_centers: null argument");
    return msm_mbk_get(h->mbk, centers, nullptr);
}

int msm_lloyd_run(msm_lloyd_t* h, const void* X, msm_idx_t n, msm_idx_t max_iter, double tol_abs, int32_t* labels_out,
                  int on_device, double* inertia, msm_idx_t* n_iter, int* status)
{
    if (!h || !X || !labels_out || !inertia || !n_iter || !status) return fail(MSM_ERR_STATE, "msm_lloyd_run: null argument");
    if (n < 1 || n >= 0x7fffffffLL || max_iter < 1) return fail(MSM_ERR_INVALID, "msm_lloyd_run: bad shape");
    return MBK_TYPED(h->mbk, lloyd_run_t<float>(h, (const float*)X, n, max_iter, tol_abs, labels_out, on_device, inertia, n_iter, status),
                     lloyd_run_t<double>(h, (const double*)X, n, max_iter, tol_abs, labels_out, on_device, inertia, n_iter, status));
}

int msm_lloyd_plan(msm_idx_t n, msm_idx_t m, msm_idx_t K, int f64, int aligned, msm_idx_t* out8)
{
    if (n < 1 || m < 1 || K < 1 || !out8) return fail(MSM_ERR_INVALID, "msm_lloyd_plan: bad argument");
    const LloydPlan pl = lloyd_plan(n, m, K, f64 != 0, aligned != 0);
    out8[0] = pl.hist_span;
    out8[1] = pl.groups;
    out8[2] = pl.piece;
    out8[3] = pl.pieces_max;
    out8[4] = pl.ftiles;
    out8[5] = pl.tile_features;
    out8[6] = pl.vec;
    out8[7] = pl.scratch_bytes;
    return MSM_OK;
}

}  // extern "C"

