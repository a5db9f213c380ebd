// pcca.hip -- msm_pcca_*: the PCCA+ objectives of lumping/pcca_plus.py (metastability, crisp_metastability, crispness) on a
// handle that keeps T, pi and V on the device between the 10^3 .. 10^5 evaluations of a search.  Kernels and the
// definitions: pcca_dev.h.
//
// An evaluation is QUEUED: one upload of alpha, three kernels (kinds 0 and 1) or six (kind 2), one read-back of the value and
// the four flags.  Whether the row kernel of kind 2 runs is decided on the device; the host never waits in between.
#include "common.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "pcca_dev.h"

struct msm_pcca {
    int n = 0, m = 0;
    double *T = nullptr, *pi = nullptr, *V = nullptr;
    double *G = nullptr, *w = nullptr;
    double* chi = nullptr;         // n x m: T V at set-up, chi for msm_pcca_chi
    double* small = nullptr;       // alpha | A | colpart | emin | num | den | num2 | den2 | rowval
    unsigned long long* used = nullptr;
    int* ints = nullptr;           // map[3][n] | differ[PC_MAX_PARTS] | sums_valid
    msm::PccaOut* out = nullptr;   // device
    void* pinned = nullptr;        // host: alpha staging, then a PccaOut
    int cur = 0;                   // ints' map[cur] holds the previous evaluation's mapping
};

namespace msm {

// MSM_PCCA_MAX_GRID (read at every call; for the tests): a cap on the workgroups of the grid-stride kernels.
static long long pcca_grid(long long want, long long cap)
{
    const char* e = getenv("MSM_PCCA_MAX_GRID");
    const long long v = e ? atoll(e) : 0;
    return std::max<long long>(1, std::min(want, v > 0 ? std::min(v, cap) : cap));
}

static bool pcca_reuse()
{
    const char* e = getenv("MSM_PCCA_REUSE");
    return !(e && atoi(e) == 0 && e[0] != '\0');
}

struct PccaSmall {
    double *alpha, *A, *colpart, *emin, *num, *den, *num2, *den2, *rowval;
};

static size_t pcca_small_doubles(int n) { return (size_t)2 * PC_MAX_M * PC_MAX_M + (size_t)PC_MAX_PARTS * (PC_MAX_M + 1) + 4 * PC_MAX_M + n; }

static PccaSmall pcca_small(const msm_pcca* h)
{
    PccaSmall s;
    s.alpha = h->small;
    s.A = s.alpha + PC_MAX_M * PC_MAX_M;
    s.colpart = s.A + PC_MAX_M * PC_MAX_M;
    s.emin = s.colpart + (size_t)PC_MAX_PARTS * PC_MAX_M;
    s.num = s.emin + PC_MAX_PARTS;
    s.den = s.num + PC_MAX_M;
    s.num2 = s.den + PC_MAX_M;
    s.den2 = s.num2 + PC_MAX_M;
    s.rowval = s.den2 + PC_MAX_M;
    return s;
}

static int* pcca_map(const msm_pcca* h, int which) { return h->ints + (size_t)which * h->n; }
static int* pcca_differ(const msm_pcca* h) { return h->ints + (size_t)3 * h->n; }
static int* pcca_valid(const msm_pcca* h) { return pcca_differ(h) + PC_MAX_PARTS; }

static void pcca_release(msm_pcca* h)
{
    void* dev[] = {h->T, h->pi, h->V, h->G, h->w, h->chi, h->small, h->used, h->ints, h->out};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (h->pinned) (void)hipHostFree(h->pinned);
    delete h;
}

static int pcca_parts(const msm_pcca* h)
{
    const int g = PC_T / std::max(2, 1 << (32 - __builtin_clz((unsigned)std::max(h->m - 1, 1))));
    return (int)pcca_grid(ceil_div(h->n, g), PC_MAX_PARTS);
}

// alpha (in the pinned buffer) -> A, chi (where wanted), map[dst]; the partial flags against map[prev] (or none).
static int pcca_queue_chi(msm_pcca* h, int dst, int prev, double* chi)
{
    const PccaSmall s = pcca_small(h);
    const int m = h->m, parts = pcca_parts(h);
    MSM_HIP_CHECK(hipMemcpyAsync(s.alpha, h->pinned, (size_t)(m - 1) * (m - 1) * sizeof(double), hipMemcpyHostToDevice, stream()));
    hipLaunchKernelGGL(pcca_colmin_kernel, dim3(parts), dim3(PC_T), 0, stream(), (const double*)s.alpha, (const double*)h->V, h->n, m,
                       s.colpart);
    PccaChiArgs P;
    P.alpha = s.alpha;
    P.V = h->V;
    P.colpart = s.colpart;
    P.n = h->n;
    P.m = m;
    P.nparts = parts;
    P.A = s.A;
    P.chi = chi;
    P.map = pcca_map(h, dst);
    P.prev = prev < 0 ? nullptr : pcca_map(h, prev);
    P.emin = s.emin;
    P.differ = pcca_differ(h);
    P.used = h->used;
    hipLaunchKernelGGL(pcca_chi_kernel, dim3(parts), dim3(PC_T), 0, stream(), P);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

// The block sums of map[which] into num, den.
static int pcca_queue_blocks(msm_pcca* h, int which, double* num, double* den, const PccaOut* gate)
{
    const PccaSmall s = pcca_small(h);
    hipLaunchKernelGGL(pcca_row_kernel, dim3((unsigned)pcca_grid(ceil_div(h->n, PC_RP), 1 << 16)), dim3(PC_T), 0, stream(),
                       (const double*)h->T, (const double*)h->pi, (const int*)pcca_map(h, which), h->n, s.rowval, gate);
    hipLaunchKernelGGL(pcca_block_kernel, dim3((unsigned)pcca_grid(h->m, PC_MAX_M)), dim3(PC_T), 0, stream(), (const double*)s.rowval,
                       (const double*)h->pi, (const int*)pcca_map(h, which), h->n, h->m, num, den, gate);
    MSM_HIP_CHECK(hipGetLastError());
    return MSM_OK;
}

static int pcca_setup(msm_pcca* h, const double* T, const double* pi, const double* V, int on_device)
{
    int rc;
    const size_t n = h->n, m = h->m;
    MSM_HIP_CHECK(hipMalloc(&h->T, n * n * sizeof(double)));
    MSM_HIP_CHECK(hipMalloc(&h->pi, n * sizeof(double)));
    MSM_HIP_CHECK(hipMalloc(&h->V, n * m * sizeof(double)));
    MSM_HIP_CHECK(hipMalloc(&h->G, m * m * sizeof(double)));
    MSM_HIP_CHECK(hipMalloc(&h->w, m * sizeof(double)));
    MSM_HIP_CHECK(hipMalloc(&h->chi, n * m * sizeof(double)));
    MSM_HIP_CHECK(hipMalloc(&h->small, pcca_small_doubles(h->n) * sizeof(double)));
    MSM_HIP_CHECK(hipMalloc(&h->used, PC_MAX_PARTS * sizeof(unsigned long long)));
    MSM_HIP_CHECK(hipMalloc(&h->ints, (3 * n + PC_MAX_PARTS + 1) * sizeof(int)));
    MSM_HIP_CHECK(hipMalloc(&h->out, sizeof(PccaOut)));
    MSM_HIP_CHECK(hipHostMalloc(&h->pinned, PC_MAX_M * PC_MAX_M * sizeof(double), hipHostMallocDefault));
    if (on_device) {
        MSM_HIP_CHECK(hipMemcpyAsync(h->T, T, n * n * sizeof(double), hipMemcpyDeviceToDevice, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(h->pi, pi, n * sizeof(double), hipMemcpyDeviceToDevice, stream()));
        MSM_HIP_CHECK(hipMemcpyAsync(h->V, V, n * m * sizeof(double), hipMemcpyDeviceToDevice, stream()));
    } else {
        if ((rc = h2d_bulk(h->T, T, n * n * sizeof(double)))) return rc;
        if ((rc = h2d_bulk(h->pi, pi, n * sizeof(double)))) return rc;
        if ((rc = h2d_bulk(h->V, V, n * m * sizeof(double)))) return rc;
    }
    // no mapping yet: every map is -1 (all bits set), the remembered sums are not valid
    MSM_HIP_CHECK(hipMemsetAsync(h->ints, 0xff, 3 * n * sizeof(int), stream()));
    MSM_HIP_CHECK(hipMemsetAsync(pcca_differ(h), 0, (PC_MAX_PARTS + 1) * sizeof(int), stream()));
    hipLaunchKernelGGL(pcca_tv_kernel, dim3((unsigned)pcca_grid(ceil_div(h->n, PC_RP), 1 << 16)), dim3(PC_T), 0, stream(),
                       (const double*)h->T, (const double*)h->V, h->n, h->m, h->chi);
    hipLaunchKernelGGL(pcca_moment_kernel, dim3((unsigned)pcca_grid((long long)(m * m + m), 1 << 16)), dim3(PC_T), 0, stream(),
                       (const double*)h->V, (const double*)h->pi, (const double*)h->chi, h->n, h->m, h->G, h->w);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // (the caller's arrays are free again)
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

int msm_pcca_create(const double* T, const double* pi, const double* V, msm_idx_t n, msm_idx_t m, int on_device, msm_pcca_t** handle)
{
    if (handle) *handle = nullptr;
    if (!T || !pi || !V || !handle) return fail(MSM_ERR_INVALID, "msm_pcca_create: null pointer");
    if (m < 2 || m > PC_MAX_M) return fail(MSM_ERR_INVALID, "msm_pcca_create: 2 to %d macrostates are supported, got %lld", PC_MAX_M, (long long)m);
    if (n < m) return fail(MSM_ERR_INVALID, "msm_pcca_create: %lld states cannot form %lld macrostates", (long long)n, (long long)m);
    if (n > PC_MAX_N) return fail(MSM_ERR_INVALID, "msm_pcca_create: at most %d states are supported, got %lld", PC_MAX_N, (long long)n);
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    msm_pcca* h = new msm_pcca();
    h->n = (int)n;
    h->m = (int)m;
    const int rc = pcca_setup(h, T, pi, V, on_device);
    if (rc) {
        pcca_release(h);
        return rc;
    }
    *handle = h;
    return MSM_OK;
}

int msm_pcca_destroy(msm_pcca_t* h)
{
    if (!h) return MSM_OK;
    (void)hipStreamSynchronize(stream());
    pcca_release(h);
    return MSM_OK;
}

int msm_pcca_moments(msm_pcca_t* h, double* G, double* w)
{
    if (!h || !G || !w) return fail(MSM_ERR_INVALID, "msm_pcca_moments: null pointer");
    MSM_HIP_CHECK(hipMemcpyAsync(G, h->G, (size_t)h->m * h->m * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(w, h->w, (size_t)h->m * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_pcca_chi(msm_pcca_t* h, const double* A_in, double* A_out, double* chi_out, int32_t* mapping_out)
{
    int rc;
    if (!h || !A_in || !A_out || !mapping_out) return fail(MSM_ERR_INVALID, "msm_pcca_chi: null pointer");
    const int m = h->m;
    double* alpha = static_cast<double*>(h->pinned);
    for (int k = 1; k < m; ++k)
        for (int c = 1; c < m; ++c) alpha[(k - 1) * (m - 1) + c - 1] = A_in[k * m + c];
    const int scratch = 2;   // the third map: the remembered mapping is left alone
    if ((rc = pcca_queue_chi(h, scratch, -1, chi_out ? h->chi : nullptr))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(A_out, pcca_small(h).A, (size_t)m * m * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(mapping_out, pcca_map(h, scratch), (size_t)h->n * sizeof(int), hipMemcpyDeviceToHost, stream()));
    if (chi_out && (rc = d2h_bulk(chi_out, h->chi, (size_t)h->n * m * sizeof(double)))) return rc;
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_pcca_objective(msm_pcca_t* h, int kind, const double* alpha, double* value, int32_t* info)
{
    int rc;
    if (!h || !alpha || !value || !info) return fail(MSM_ERR_INVALID, "msm_pcca_objective: null pointer");
    if (kind < 0 || kind > 2) return fail(MSM_ERR_INVALID, "msm_pcca_objective: kind must be 0, 1 or 2, got %d", kind);
    const int m = h->m, prev = h->cur, dst = 1 - h->cur;
    memcpy(h->pinned, alpha, (size_t)(m - 1) * (m - 1) * sizeof(double));
    if ((rc = pcca_queue_chi(h, dst, prev, nullptr))) return rc;
    const PccaSmall s = pcca_small(h);
    PccaEvalArgs E;
    E.A = s.A;
    E.G = h->G;
    E.w = h->w;
    E.emin = s.emin;
    E.differ = pcca_differ(h);
    E.used = h->used;
    E.nparts = pcca_parts(h);
    E.m = m;
    E.kind = kind;
    E.reuse = pcca_reuse();
    E.sums_valid = pcca_valid(h);
    E.num = s.num;
    E.den = s.den;
    E.out = h->out;
    hipLaunchKernelGGL(pcca_decide_kernel, dim3(1), dim3(PC_T), 0, stream(), E);
    if (kind == 2) {
        if ((rc = pcca_queue_blocks(h, dst, s.num, s.den, h->out))) return rc;
        hipLaunchKernelGGL(pcca_crisp_value_kernel, dim3(1), dim3(64), 0, stream(), (const double*)s.num, (const double*)s.den, m,
                           pcca_valid(h), h->out);
    }
    MSM_HIP_CHECK(hipGetLastError());
    h->cur = dst;
    PccaOut* back = static_cast<PccaOut*>(h->pinned);   // (alpha has been uploaded in stream order before this lands)
    MSM_HIP_CHECK(hipMemcpyAsync(back, h->out, sizeof(PccaOut), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    *value = back->value;
    for (int i = 0; i < 4; ++i) info[i] = back->info[i];
    return MSM_OK;
}

int msm_pcca_crisp(msm_pcca_t* h, const int32_t* mapping, double* num, double* den)
{
    int rc;
    if (!h || !mapping || !num || !den) return fail(MSM_ERR_INVALID, "msm_pcca_crisp: null pointer");
    for (int i = 0; i < h->n; ++i)
        if (mapping[i] < 0 || mapping[i] >= h->m)
            return fail(MSM_ERR_INVALID, "msm_pcca_crisp: mapping[%d] = %d is not in [0, %d)", i, (int)mapping[i], h->m);
    const int scratch = 2;
    const PccaSmall s = pcca_small(h);
    MSM_HIP_CHECK(hipMemcpyAsync(pcca_map(h, scratch), mapping, (size_t)h->n * sizeof(int), hipMemcpyHostToDevice, stream()));
    if ((rc = pcca_queue_blocks(h, scratch, s.num2, s.den2, nullptr))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(num, s.num2, (size_t)h->m * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipMemcpyAsync(den, s.den2, (size_t)h->m * sizeof(double), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    return MSM_OK;
}

int msm_pcca_plan(msm_idx_t* out5)
{
    if (!out5) return fail(MSM_ERR_INVALID, "msm_pcca_plan: null pointer");
    out5[0] = PC_RP;
    out5[1] = PC_CP;
    out5[2] = PC_T;
    out5[3] = PC_MAX_N;
    out5[4] = PC_MAX_M;
    return MSM_OK;
}

}  // extern "C"
