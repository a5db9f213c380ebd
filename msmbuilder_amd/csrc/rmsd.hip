// rmsd.hip -- the rmsd metric's C ABI (include/msmhip.h, "rmsd"): prepared frames and the six distance entry points over
// them.  Kernels and the one definition of the distance: rmsd_dev.h.  Built with -ffp-contract=off: every fused
// multiply-add here is written as fmaf or issued as an MFMA.
#include "common.h"
#include "rmsd_dev.h"

#include <algorithm>
#include <vector>

struct msm_rmsd {
    float* T = nullptr;
    double* G = nullptr;
    long long n = 0, n_pad = 0, A = 0;
};

namespace msm {
namespace {

RmsdImage image_of(const msm_rmsd* h)
{
    RmsdImage I;
    I.T = h->T;
    I.G = h->G;
    I.n = h->n;
    I.n_pad = h->n_pad;
    I.A = h->A;
    return I;
}

int grid_for(long long n) { return (int)ceil_div(n, RMSD_BLOCK); }

// Index arrays reach the kernels as device pointers whose every entry was checked against [0, n): a gather through an
// unchecked index would read outside the image.  Synchronises.
int checked_indices(const msm_idx_t* idx, long long count, long long n, int on_device, const msm_idx_t** dev)
{
    int rc;
    const msm_idx_t* d = idx;
    if (!on_device) {
        for (long long i = 0; i < count; ++i)
            if (idx[i] < 0 || idx[i] >= n) return fail(MSM_ERR_INVALID, "rmsd: index %lld outside [0, %lld)", (long long)idx[i], n);
        DevBuf& b = pool(PS_IDX);
        if ((rc = b.reserve((size_t)count * sizeof(msm_idx_t)))) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(b.p, idx, (size_t)count * sizeof(msm_idx_t), hipMemcpyHostToDevice, stream()));
        d = b.as<msm_idx_t>();
    } else {
        DevBuf& f = pool(PS_PAR);
        if ((rc = f.reserve(sizeof(int)))) return rc;
        MSM_HIP_CHECK(hipMemsetAsync(f.p, 0, sizeof(int), stream()));
        hipLaunchKernelGGL(rmsd_check_index_kernel, dim3(grid_for(count)), dim3(RMSD_BLOCK), 0, stream(),
                           (const long long*)idx, count, n, f.as<int>());
        MSM_HIP_CHECK(hipGetLastError());
        int flag = 0;
        MSM_HIP_CHECK(hipMemcpyAsync(&flag, f.p, sizeof(int), hipMemcpyDeviceToHost, stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(stream()));
        if (flag) return fail(MSM_ERR_INVALID, "rmsd: an index lies outside [0, %lld)", n);
    }
    *dev = d;
    return MSM_OK;
}

int need_device()
{
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    return MSM_OK;
}

int same_atoms(const msm_rmsd* a, const msm_rmsd* b, const char* what)
{
    if (a->A != b->A) return fail(MSM_ERR_INVALID, "%s: %lld and %lld atoms", what, a->A, b->A);
    return MSM_OK;
}

// the caller's output: its own pointer on the device, a pool slot (copied back by finish_output) on the host
template <typename T>
int stage_output(T* user, size_t count, int on_device, int slot, T** dev)
{
    if (on_device) {
        *dev = user;
        return MSM_OK;
    }
    int rc;
    if ((rc = pool(slot).reserve(count * sizeof(T)))) return rc;
    *dev = pool(slot).as<T>();
    return MSM_OK;
}

template <typename T>
int finish_output(T* user, const T* dev, size_t count, int on_device)
{
    if (!on_device) MSM_HIP_CHECK(hipMemcpyAsync(user, dev, count * sizeof(T), hipMemcpyDeviceToHost, stream()));
    return MSM_OK;
}

int ordered_sum(const double* dv, long long n, double* host_out)
{
    int rc;
    DevBuf& s = pool(PS_SUM);
    if ((rc = s.reserve(sizeof(double)))) return rc;
    hipLaunchKernelGGL(rmsd_ordered_sum_kernel, dim3(1), dim3(RMSD_BLOCK), 0, stream(), dv, n, s.as<double>());
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(host_out, s.p, sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

template <int EPI>
int launch_tiles(const RmsdTileArgs& P)
{
    if (EPI == RMSD_EPI_ASSIGN) {
        const long long tiles = ceil_div(P.nc, 32);
        hipLaunchKernelGGL(rmsd_tile_kernel<EPI>, dim3((unsigned)ceil_div(tiles, RMSD_BLOCK / 64)), dim3(RMSD_BLOCK), 0, stream(), P);
    } else {
        const long long tr = ceil_div(P.nr, 32), tc = ceil_div(P.nc, 32);
        if (tc > 65535) return fail(MSM_ERR_INVALID, "rmsd: more than %d columns in one call", 65535 * 32);
        hipLaunchKernelGGL(rmsd_tile_kernel<EPI>, dim3((unsigned)ceil_div(tr, RMSD_BLOCK / 64), (unsigned)tc), dim3(RMSD_BLOCK), 0,
                           stream(), P);
    }
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

}  // namespace
}  // namespace msm

using namespace msm;

extern "C" {

int msm_rmsd_prepare(msm_rmsd_t** out, const float* xyz, msm_idx_t n_frames, msm_idx_t n_atoms, int on_device)
{
    if (!out) return fail(MSM_ERR_INVALID, "rmsd_prepare: null handle pointer");
    *out = nullptr;
    if (!xyz || n_frames < 1 || n_atoms < 1) return fail(MSM_ERR_INVALID, "rmsd_prepare: needs at least one frame and one atom");
    if (n_atoms > (1LL << 24)) return fail(MSM_ERR_INVALID, "rmsd_prepare: more than 2^24 atoms");
    int rc;
    if ((rc = need_device())) return rc;
    msm_rmsd* h = new msm_rmsd();
    h->n = n_frames;
    h->A = n_atoms;
    h->n_pad = ceil_div(n_frames, RMSD_FRAME_PAD) * RMSD_FRAME_PAD;
    const size_t cells = (size_t)3 * (size_t)h->A * (size_t)h->n_pad;
    hipError_t e = hipMalloc((void**)&h->T, cells * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->G, (size_t)h->n_pad * sizeof(double));
    if (e != hipSuccess) {
        msm_rmsd_destroy(h);
        return fail(MSM_ERR_HIP, "rmsd_prepare: hipMalloc failed: %s", hipGetErrorString(e));
    }
    const float* dx = xyz;
    if (!on_device) {
        const size_t bytes = (size_t)n_frames * (size_t)n_atoms * 3 * sizeof(float);
        if ((rc = pool(PS_X).reserve(bytes)) || (rc = h2d_bulk(pool(PS_X).p, xyz, bytes))) {
            msm_rmsd_destroy(h);
            return rc;
        }
        dx = pool(PS_X).as<float>();
    }
    hipLaunchKernelGGL(rmsd_prepare_kernel, dim3(grid_for(h->n_pad)), dim3(RMSD_BLOCK), 0, stream(), dx, h->n, h->n_pad, h->A,
                       h->T, h->G);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream());
    if (e != hipSuccess) {
        msm_rmsd_destroy(h);
        return fail(MSM_ERR_HIP, "rmsd_prepare: %s", hipGetErrorString(e));
    }
    *out = h;
    return MSM_OK;
}

int msm_rmsd_destroy(msm_rmsd_t* h)
{
    if (!h) return MSM_OK;
    if (h->T) (void)hipFree(h->T);
    if (h->G) (void)hipFree(h->G);
    delete h;
    return MSM_OK;
}

int msm_rmsd_shape(const msm_rmsd_t* h, msm_idx_t* n_frames, msm_idx_t* n_atoms, msm_idx_t* n_pad)
{
    if (!h) return fail(MSM_ERR_INVALID, "rmsd_shape: null handle");
    if (n_frames) *n_frames = h->n;
    if (n_atoms) *n_atoms = h->A;
    if (n_pad) *n_pad = h->n_pad;
    return MSM_OK;
}

int msm_rmsd_dist(const msm_rmsd_t* X, const msm_rmsd_t* Y, msm_idx_t y_frame, const msm_idx_t* X_indices,
                  msm_idx_t n_X_indices, double* out, int on_device)
{
    if (!X || !Y || !out) return fail(MSM_ERR_INVALID, "rmsd_dist: null pointer");
    if (y_frame < 0 || y_frame >= Y->n) return fail(MSM_ERR_INVALID, "rmsd_dist: frame %lld outside [0, %lld)", (long long)y_frame, Y->n);
    if (X_indices && n_X_indices < 0) return fail(MSM_ERR_INVALID, "rmsd_dist: bad shape");
    int rc;
    if ((rc = same_atoms(X, Y, "rmsd_dist"))) return rc;
    const long long n = X_indices ? n_X_indices : X->n;
    if (n == 0) return MSM_OK;
    if ((rc = need_device())) return rc;
    RmsdRowArgs P;
    memset(&P, 0, sizeof(P));
    P.X = image_of(X);
    P.Y = image_of(Y);
    P.n = n;
    P.yframe = y_frame;
    if (X_indices && (rc = checked_indices(X_indices, n, X->n, on_device, (const msm_idx_t**)&P.idx))) return rc;
    if ((rc = stage_output(out, (size_t)n, on_device, PS_OUT, &P.out))) return rc;
    hipLaunchKernelGGL(rmsd_row_kernel<RMSD_ROW_DIST>, dim3(grid_for(n)), dim3(RMSD_BLOCK), 0, stream(), P);
    MSM_HIP_CHECK(hipGetLastError());
    if ((rc = finish_output(out, P.out, (size_t)n, on_device))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_rmsd_cdist(const msm_rmsd_t* XA, const msm_rmsd_t* XB, double* out, int on_device)
{
    if (!XA || !XB || !out) return fail(MSM_ERR_INVALID, "rmsd_cdist: null pointer");
    int rc;
    if ((rc = same_atoms(XA, XB, "rmsd_cdist"))) return rc;
    if ((rc = need_device())) return rc;
    RmsdTileArgs P;
    memset(&P, 0, sizeof(P));
    P.R = image_of(XA);
    P.C = image_of(XB);
    P.nr = XA->n;
    P.nc = XB->n;
    const size_t count = (size_t)P.nr * (size_t)P.nc;
    if ((rc = stage_output(out, count, on_device, PS_OUT, &P.out))) return rc;
    if ((rc = launch_tiles<RMSD_EPI_CDIST>(P))) return rc;
    if ((rc = finish_output(out, P.out, count, on_device))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_rmsd_pdist(const msm_rmsd_t* X, const msm_idx_t* X_indices, msm_idx_t n_X_indices, double* out, int on_device)
{
    if (!X) return fail(MSM_ERR_INVALID, "rmsd_pdist: null pointer");
    if (X_indices && n_X_indices < 0) return fail(MSM_ERR_INVALID, "rmsd_pdist: bad shape");
    const long long n = X_indices ? n_X_indices : X->n;
    if (n < 2) return MSM_OK;
    if (!out) return fail(MSM_ERR_INVALID, "rmsd_pdist: null pointer");
    int rc;
    if ((rc = need_device())) return rc;
    RmsdTileArgs P;
    memset(&P, 0, sizeof(P));
    P.R = image_of(X);
    P.C = P.R;
    P.nr = P.nc = n;
    if (X_indices) {
        if ((rc = checked_indices(X_indices, n, X->n, on_device, (const msm_idx_t**)&P.ridx))) return rc;
        P.cidx = P.ridx;
    }
    const size_t count = (size_t)n * (size_t)(n - 1) / 2;
    if ((rc = stage_output(out, count, on_device, PS_OUT, &P.out))) return rc;
    if ((rc = launch_tiles<RMSD_EPI_PDIST>(P))) return rc;
    if ((rc = finish_output(out, P.out, count, on_device))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_rmsd_sumdist(const msm_rmsd_t* X, const msm_idx_t* pair_indices, msm_idx_t n_pairs, double* sum, int on_device)
{
    if (!X || !sum) return fail(MSM_ERR_INVALID, "rmsd_sumdist: null pointer");
    if (n_pairs < 0) return fail(MSM_ERR_INVALID, "rmsd_sumdist: bad shape");
    *sum = 0.0;
    if (n_pairs == 0) return MSM_OK;
    if (!pair_indices) return fail(MSM_ERR_INVALID, "rmsd_sumdist: null pointer");
    int rc;
    if ((rc = need_device())) return rc;
    RmsdRowArgs P;
    memset(&P, 0, sizeof(P));
    P.X = image_of(X);
    P.Y = P.X;
    P.n = n_pairs;
    if ((rc = checked_indices(pair_indices, 2 * n_pairs, X->n, on_device, (const msm_idx_t**)&P.idx))) return rc;
    if ((rc = pool(PS_MIN).reserve((size_t)n_pairs * sizeof(double)))) return rc;
    P.out = pool(PS_MIN).as<double>();
    hipLaunchKernelGGL(rmsd_row_kernel<RMSD_ROW_PAIRS>, dim3(grid_for(n_pairs)), dim3(RMSD_BLOCK), 0, stream(), P);
    MSM_HIP_CHECK(hipGetLastError());
    return ordered_sum(P.out, n_pairs, sum);
}

int msm_rmsd_assign_nearest(const msm_rmsd_t* X, const msm_rmsd_t* Y, const msm_idx_t* X_indices, msm_idx_t n_X_indices,
                            msm_idx_t* assignments, double* min_dist, double* inertia, int on_device)
{
    if (!X || !Y || !assignments) return fail(MSM_ERR_INVALID, "rmsd_assign_nearest: null pointer");
    if (X_indices && n_X_indices < 0) return fail(MSM_ERR_INVALID, "rmsd_assign_nearest: bad shape");
    int rc;
    if ((rc = same_atoms(X, Y, "rmsd_assign_nearest"))) return rc;
    const long long n = X_indices ? n_X_indices : X->n;
    if (inertia) *inertia = 0.0;
    if (n == 0) return MSM_OK;
    if ((rc = need_device())) return rc;
    RmsdTileArgs P;
    memset(&P, 0, sizeof(P));
    P.R = image_of(Y);   // rows = centres, columns = frames
    P.C = image_of(X);
    P.nr = Y->n;
    P.nc = n;
    if (X_indices && (rc = checked_indices(X_indices, n, X->n, on_device, (const msm_idx_t**)&P.cidx))) return rc;
    if ((rc = stage_output((long long*)assignments, (size_t)n, on_device, PS_LAB, &P.labels))) return rc;
    if (min_dist && on_device) {
        P.min_dist = min_dist;
    } else {
        if ((rc = pool(PS_MIN).reserve((size_t)n * sizeof(double)))) return rc;
        P.min_dist = pool(PS_MIN).as<double>();
    }
    if ((rc = launch_tiles<RMSD_EPI_ASSIGN>(P))) return rc;
    if ((rc = finish_output((long long*)assignments, P.labels, (size_t)n, on_device))) return rc;
    if (min_dist && !on_device && (rc = finish_output(min_dist, P.min_dist, (size_t)n, 0))) return rc;
    double s = 0.0;
    if ((rc = ordered_sum(P.min_dist, n, &s))) return rc;   // synchronises
    if (inertia) *inertia = s;
    return MSM_OK;
}

int msm_rmsd_kcenters_fit(const msm_rmsd_t* X, msm_idx_t K, msm_idx_t seed, msm_idx_t* ids, msm_idx_t* labels,
                          double* distances, double* inertia, int on_device)
{
    if (!X || !ids || !labels || !distances) return fail(MSM_ERR_INVALID, "rmsd_kcenters_fit: null pointer");
    if (K < 1) return fail(MSM_ERR_INVALID, "rmsd_kcenters_fit: n_clusters must be at least 1");
    if (seed < 0 || seed >= X->n) return fail(MSM_ERR_INVALID, "rmsd_kcenters_fit: seed %lld outside [0, %lld)", (long long)seed, X->n);
    int rc;
    if ((rc = need_device())) return rc;
    const long long n = X->n;
    const int grid = grid_for(n);
    RmsdRowArgs P;
    memset(&P, 0, sizeof(P));
    P.X = image_of(X);
    P.Y = P.X;
    P.n = n;
    if ((rc = stage_output(distances, (size_t)n, on_device, PS_MIN, &P.out))) return rc;
    if ((rc = stage_output((long long*)labels, (size_t)n, on_device, PS_LAB, &P.labels))) return rc;
    DevBuf &dIds = pool(PS_IDS), &dPart = pool(PS_PART);
    if ((rc = dIds.reserve((size_t)(K + 1) * sizeof(long long)))) return rc;
    if ((rc = dPart.reserve((size_t)grid * (sizeof(double) + sizeof(long long))))) return rc;
    P.part_val = dPart.as<double>();
    P.part_idx = (long long*)(P.part_val + grid);
    long long* dids = dIds.as<long long>();
    const long long first = seed;
    MSM_HIP_CHECK(hipMemcpyAsync(dids, &first, sizeof(long long), hipMemcpyHostToDevice, stream()));
    // all K passes queued back to back: pass k reads centre k from the device, the select that follows writes centre k + 1
    for (long long k = 0; k < K; ++k) {
        P.centre = dids + k;
        P.k = k;
        hipLaunchKernelGGL(rmsd_row_kernel<RMSD_ROW_KCENTERS>, dim3(grid), dim3(RMSD_BLOCK), 0, stream(), P);
        hipLaunchKernelGGL(rmsd_select_kernel, dim3(1), dim3(RMSD_BLOCK), 0, stream(), (const double*)P.part_val,
                           (const long long*)P.part_idx, (long long)grid, dids + k + 1);
    }
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(ids, dids, (size_t)K * sizeof(long long), hipMemcpyDeviceToHost, stream()));
    if ((rc = finish_output(distances, P.out, (size_t)n, on_device))) return rc;
    if ((rc = finish_output((long long*)labels, P.labels, (size_t)n, on_device))) return rc;
    double s = 0.0;
    if ((rc = ordered_sum(P.out, n, &s))) return rc;   // synchronises
    if (inertia) *inertia = s;
    return MSM_OK;
}

}  // extern "C"
