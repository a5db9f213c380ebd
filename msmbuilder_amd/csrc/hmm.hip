// hmm.hip -- msm_hmm_{estep,score,loglik,viterbi}_{f32,f64} and msm_hmm_plan: the E-step of the Gaussian hidden Markov
// model (what hmm/src/include/HMMFitter.h:75-110 and hmm/src/GaussianHMMFitter.cpp accumulate per trajectory, serially in
// time) as a time-parallel forward-backward on the device.  Kernels and the scheme: hmm_dev.h.
// msm_hmm_trig_{f32,f64} and msm_hmm_lin_{estep,score,loglik,viterbi}: the same passes for the von Mises model
// (hmm/src/VonMisesHMMFitter.cpp), whose emission is linear in the image [cos X | sin X] of the angles; the image is formed
// once and every later call reads it.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "hmm_dev.h"

namespace msm {

constexpr long long HMM_LDS_BUDGET = 144 * 1024;   // of 160 KiB per CU
constexpr int HMM_S_DEFAULT = 128;

struct HmmPlan {
    int KP, S_default, S_max;
    long long lds_oper;
};

static HmmPlan hmm_plan(int K)
{
    HmmPlan p;
    p.KP = K | 1;
    p.lds_oper = hmm_oper_lds(K, p.KP) * (long long)sizeof(double);
    // hmm_fused_lds(K, KP, S) * 8 <= budget, solved for S
    const long long fixed = (long long)K * p.KP + 4LL * K + 8;
    p.S_max = (int)((HMM_LDS_BUDGET / (long long)sizeof(double) - fixed) / (2LL * K + 1));
    p.S_default = std::min(HMM_S_DEFAULT, p.S_max);
    return p;
}

struct HmmBufs {
    DevBuf par, idx, ops, vec, part, x, bp, out;
};
static HmmBufs& bufs()
{
    static HmmBufs* b = new HmmBufs();   // intentionally leaked (outlives HIP teardown)
    return *b;
}

template <typename K>
static int raise_lds(K kernel, long long bytes, long long* set)
{
    if (bytes > *set) {
        MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        *set = bytes;
    }
    return MSM_OK;
}

enum HmmMode { HM_ESTEP, HM_SCORE, HM_LOGLIK, HM_VITERBI };

// The checks both emission flavours share, in the order the messages have always come: sizes, n_states, pointers (ptrs: the
// flavour's own are all there), shape, offsets.  F is the number of columns the kernels read (the image's D for the linear one).
static int hmm_check_shape(const char* who, msm_idx_t n, msm_idx_t F, msm_idx_t ld, const msm_idx_t* offsets, msm_idx_t n_traj,
                           msm_idx_t K, bool ptrs, const double* transmat, const double* log_startprob, bool need_chain)
{
    if (n < 1 || (need_chain && n_traj < 1)) return fail(MSM_ERR_INVALID, "%s: sequences is empty", who);
    if (K < 1 || K > HMM_KMAX)
        return fail(MSM_ERR_INVALID, "%s: n_states = %lld is outside 1 .. %d, the largest number of states this build serves", who,
                    (long long)K, HMM_KMAX);
    if (!ptrs || (need_chain && (!transmat || !log_startprob || !offsets))) return fail(MSM_ERR_INVALID, "%s: null pointer", who);
    if (F < 1 || ld < F || F > (1 << 20)) return fail(MSM_ERR_INVALID, "%s: bad shape", who);
    if (need_chain) {
        if (offsets[0] != 0 || offsets[n_traj] != n) return fail(MSM_ERR_INVALID, "%s: offsets do not span the rows", who);
        for (msm_idx_t j = 0; j < n_traj; ++j)
            if (offsets[j + 1] <= offsets[j]) return fail(MSM_ERR_INVALID, "%s: trajectory %lld is empty", who, (long long)j);
    }
    return MSM_OK;
}

// The chain part of the setup, shared by both flavours: transition matrix and start vector finite, a device present, then
// ONE upload of h = [emission parameters (n_emis doubles, filled by the caller) | A clamped at 1e-20 | log A | lsp] and the
// common part of the kernel arguments.  A->mu points at the emission parameters; the caller places iv and cst in them.
static int hmm_chain_setup(const char* who, msm_idx_t n, msm_idx_t F, msm_idx_t K, std::vector<double>& h, size_t n_emis,
                           const double* transmat, const double* log_startprob, bool need_chain, HmmArgs* A)
{
    if (need_chain) {
        for (msm_idx_t e = 0; e < K * K; ++e)
            if (!std::isfinite(transmat[e])) return fail(MSM_ERR_INVALID, "%s: the transition matrix is not finite", who);
        for (msm_idx_t k = 0; k < K; ++k)
            if (!std::isfinite(log_startprob[k])) return fail(MSM_ERR_INVALID, "%s: the start vector is not finite", who);
    }
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const size_t np = n_emis + (size_t)(2 * K * K + K);
    h.resize(np, 0.0);
    double* hA = h.data() + n_emis;
    double* hL = hA + K * K;
    double* lsp = hL + K * K;
    if (need_chain) {
        for (msm_idx_t e = 0; e < K * K; ++e) {
            hA[e] = std::max(transmat[e], 1e-20);   // set_transmat's clamp (HMMFitter.h:40)
            hL[e] = std::log(hA[e]);
        }
        for (msm_idx_t k = 0; k < K; ++k) lsp[k] = log_startprob[k];
    }
    HmmBufs& B = bufs();
    int rc;
    if ((rc = B.par.reserve(np * sizeof(double) + 16))) return rc;
    MSM_HIP_CHECK(hipMemsetAsync(B.par.p, 0, 16, stream()));
    double* dpar = reinterpret_cast<double*>(B.par.as<char>() + 16);
    MSM_HIP_CHECK(hipMemcpyAsync(dpar, h.data(), np * sizeof(double), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // h may die with the caller's frame

    memset(A, 0, sizeof(*A));
    A->K = (int)K;
    A->F = (int)F;
    A->KP = (int)K | 1;
    A->n = n;
    A->flag = B.par.as<int>();
    A->mu = dpar;
    A->A = dpar + n_emis;
    A->logA = A->A + K * K;
    A->lsp = A->logA + K * K;
    return MSM_OK;
}

// Gaussian emission: validates, stages the parameters (and host rows) and fills the common part of the kernel arguments.
template <typename T>
static int hmm_setup(const char* who, const T* rows, msm_idx_t n, msm_idx_t F, msm_idx_t ld, const msm_idx_t* offsets, msm_idx_t n_traj,
                     msm_idx_t K, const double* means, const double* vars, const double* transmat, const double* log_startprob,
                     int on_device, bool need_chain, HmmArgs* A)
{
    int rc;
    if ((rc = hmm_check_shape(who, n, F, ld, offsets, n_traj, K, rows && means && vars, transmat, log_startprob, need_chain))) return rc;
    for (msm_idx_t e = 0; e < K * F; ++e) {
        if (!std::isfinite(means[e])) return fail(MSM_ERR_INVALID, "%s: a mean is not finite", who);
        if (!(vars[e] > 0.0) || !std::isfinite(vars[e])) return fail(MSM_ERR_INVALID, "%s: variances must be positive and finite", who);
    }
    // emission parameters: mu, 1/var, cst
    const size_t n_emis = (size_t)(2 * K * F + K);
    std::vector<double> h(n_emis, 0.0);
    double* mu = h.data();
    double* iv = mu + K * F;
    double* cst = iv + K * F;
    // the reference keeps log(2 pi) in a float (GaussianHMMFitter.cpp:47); every log probability carries that constant
    const double log_2pi = (double)(float)std::log(2.0 * M_PI);
    for (msm_idx_t k = 0; k < K; ++k) {
        double sl = 0.0;
        for (msm_idx_t f = 0; f < F; ++f) {
            mu[k * F + f] = means[k * F + f];
            iv[k * F + f] = 1.0 / vars[k * F + f];
            sl += std::log(vars[k * F + f]);
        }
        cst[k] = -0.5 * ((double)F * log_2pi + sl);
    }
    if ((rc = hmm_chain_setup(who, n, F, K, h, n_emis, transmat, log_startprob, need_chain, A))) return rc;
    A->iv = A->mu + K * F;
    A->cst = A->iv + K * F;
    HmmBufs& B = bufs();
    if (on_device) {
        A->X = rows;
        A->ld = ld;
    } else {
        if ((rc = B.x.reserve((size_t)n * F * sizeof(T)))) return rc;
        if (ld == F) {
            if ((rc = h2d_bulk(B.x.p, rows, (size_t)n * F * sizeof(T)))) return rc;
        } else {
            MSM_HIP_CHECK(hipMemcpy2DAsync(B.x.p, (size_t)F * sizeof(T), rows, (size_t)ld * sizeof(T), (size_t)F * sizeof(T), (size_t)n,
                                           hipMemcpyHostToDevice, stream()));
        }
        A->X = B.x.p;
        A->ld = F;
    }
    return MSM_OK;
}

static int hmm_flag(const HmmArgs& A)
{
    int f = 0;
    MSM_HIP_CHECK(hipMemcpyAsync(&f, A.flag, sizeof(int), hipMemcpyDeviceToHost, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    if (f) return fail(MSM_ERR_NONFINITE, "Input contains NaN, infinity or a value too large");
    return MSM_OK;
}

// offsets and every trajectory's first segment -> device; returns n_seg through A
static int hmm_segments(HmmArgs* A, const msm_idx_t* offsets, msm_idx_t n_traj, int S)
{
    std::vector<long long> h(2 * (size_t)(n_traj + 1));
    long long* off = h.data();
    long long* seg0 = off + n_traj + 1;
    seg0[0] = 0;
    for (msm_idx_t j = 0; j <= n_traj; ++j) off[j] = offsets[j];
    for (msm_idx_t j = 0; j < n_traj; ++j) seg0[j + 1] = seg0[j] + ceil_div(off[j + 1] - off[j], S);
    HmmBufs& B = bufs();
    int rc;
    if ((rc = B.idx.reserve(h.size() * sizeof(long long)))) return rc;
    MSM_HIP_CHECK(hipMemcpyAsync(B.idx.p, h.data(), h.size() * sizeof(long long), hipMemcpyHostToDevice, stream()));
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));
    A->S = S;
    A->n_traj = n_traj;
    A->n_seg = seg0[n_traj];
    A->off = B.idx.as<long long>();
    A->seg0 = A->off + n_traj + 1;
    return MSM_OK;
}

// Linear emission over the image Z (device memory by contract: nothing is staged): w and cst finite, then the chain part.
static int hmm_lin_setup(const char* who, const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets,
                         msm_idx_t n_traj, msm_idx_t K, const double* w, const double* cst, const double* transmat,
                         const double* log_startprob, bool need_chain, HmmArgs* A)
{
    int rc;
    if ((rc = hmm_check_shape(who, n, D, ldz, offsets, n_traj, K, Z && w && cst, transmat, log_startprob, need_chain))) return rc;
    for (msm_idx_t e = 0; e < K * D; ++e)
        if (!std::isfinite(w[e])) return fail(MSM_ERR_INVALID, "%s: a weight is not finite", who);
    for (msm_idx_t k = 0; k < K; ++k)
        if (!std::isfinite(cst[k])) return fail(MSM_ERR_INVALID, "%s: a constant is not finite", who);
    const size_t n_emis = (size_t)(K * D + K);
    std::vector<double> h(n_emis, 0.0);
    std::copy(w, w + K * D, h.data());
    std::copy(cst, cst + K, h.data() + K * D);
    if ((rc = hmm_chain_setup(who, n, D, K, h, n_emis, transmat, log_startprob, need_chain, A))) return rc;
    A->cst = A->mu + K * D;
    A->X = Z;
    A->ld = ldz;
    return MSM_OK;
}

// The passes of an E-step (or of its forward half) over rows of T under the emission flavour EM, after the setup.
template <typename T, int EM>
static int estep_run(const char* who, HmmArgs& A, const msm_idx_t* offsets, msm_idx_t n_traj, msm_idx_t segment, double* traj_logprob,
                     double* post, double* obs, double* obs2, double* trans, double* logprob, HmmMode mode)
{
    const msm_idx_t K = A.K, F = A.F;
    constexpr bool GAUSS = EM == HMM_GAUSS;
    int rc;
    if (!traj_logprob || !logprob || (mode == HM_ESTEP && (!post || !obs || (GAUSS && !obs2) || !trans)))
        return fail(MSM_ERR_INVALID, "%s: null output", who);
    const HmmPlan pl = hmm_plan((int)K);
    if (segment < 0 || segment > (1 << 30) || (mode == HM_ESTEP && segment > pl.S_max))   // (the forward half keeps nothing per frame)
        return fail(MSM_ERR_INVALID, "%s: segment = %lld is outside 0 .. %d, the longest whose alpha block fits LDS at n_states = %lld", who,
                    (long long)segment, pl.S_max, (long long)K);
    const int S = segment ? (int)segment : pl.S_default;
    if ((rc = hmm_segments(&A, offsets, n_traj, S))) return rc;
    if (A.n_seg > INT32_MAX) return fail(MSM_ERR_INVALID, "%s: too many segments", who);
    const long long K2 = K * K;
    HmmBufs& B = bufs();
    if ((rc = B.ops.reserve((size_t)A.n_seg * K2 * sizeof(double)))) return rc;
    if ((rc = B.vec.reserve((size_t)(A.n_seg * (2 * K + 1) + n_traj) * sizeof(double)))) return rc;
    A.ops = B.ops.as<double>();
    A.opscale = B.vec.as<double>();
    A.alpha_in = A.opscale + A.n_seg;
    double* beta = A.alpha_in + A.n_seg * K;
    A.traj_lp = beta + A.n_seg * K;
    A.beta_out = mode == HM_ESTEP ? beta : nullptr;

    static long long oper_set = 48 * 1024, fused_set = 48 * 1024;   // per instantiation
    if ((rc = raise_lds(hmm_oper_kernel<T, EM>, pl.lds_oper, &oper_set))) return rc;
    hipLaunchKernelGGL((hmm_oper_kernel<T, EM>), dim3((unsigned)A.n_seg), dim3(HMM_T), (size_t)pl.lds_oper, stream(), A);
    hipLaunchKernelGGL(hmm_stitch_kernel, dim3((unsigned)n_traj), dim3(64), (size_t)hmm_stitch_chunk((int)K) * (K2 + 1) * sizeof(double), stream(), A);
    MSM_HIP_CHECK(hipGetLastError());
    std::vector<double> hout;
    if (mode == HM_ESTEP) {
        A.psz = K + (GAUSS ? 2 : 1) * K * F + K2;
        A.G = (int)std::min<long long>(HMM_G, A.n_seg);
        if ((rc = B.part.reserve((size_t)A.G * A.psz * sizeof(double)))) return rc;
        if ((rc = B.out.reserve((size_t)A.psz * sizeof(double)))) return rc;
        A.part = B.part.as<double>();
        A.out = B.out.as<double>();
        const long long lds = hmm_fused_lds((int)K, A.KP, S) * (long long)sizeof(double);
        if ((rc = raise_lds(hmm_fused_kernel<T, EM>, lds, &fused_set))) return rc;
        hipLaunchKernelGGL((hmm_fused_kernel<T, EM>), dim3((unsigned)A.G), dim3(HMM_T), (size_t)lds, stream(), A);
        hipLaunchKernelGGL(hmm_reduce_kernel, dim3((unsigned)ceil_div(A.psz, HMM_T)), dim3(HMM_T), 0, stream(), A);
        MSM_HIP_CHECK(hipGetLastError());
        hout.resize((size_t)A.psz);
        MSM_HIP_CHECK(hipMemcpyAsync(hout.data(), A.out, (size_t)A.psz * sizeof(double), hipMemcpyDeviceToHost, stream()));
    }
    MSM_HIP_CHECK(hipMemcpyAsync(traj_logprob, A.traj_lp, (size_t)n_traj * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if ((rc = hmm_flag(A))) return rc;   // synchronises
    double total = 0.0;
    for (msm_idx_t j = 0; j < n_traj; ++j) total += traj_logprob[j];   // in trajectory order
    *logprob = total;
    if (mode == HM_ESTEP) {
        const double* o = hout.data();
        memcpy(post, o, (size_t)K * sizeof(double));
        memcpy(obs, o + K, (size_t)K * F * sizeof(double));
        if (GAUSS) memcpy(obs2, o + K + K * F, (size_t)K * F * sizeof(double));
        memcpy(trans, o + A.psz - K2, (size_t)K2 * sizeof(double));
    }
    return MSM_OK;
}

template <typename T>
static int estep_impl(const T* rows, msm_idx_t n, msm_idx_t F, msm_idx_t ld, const msm_idx_t* offsets, msm_idx_t n_traj, msm_idx_t K,
                      const double* means, const double* vars, const double* transmat, const double* log_startprob,
                      msm_idx_t segment, double* traj_logprob, double* post, double* obs, double* obs2, double* trans,
                      double* logprob, int on_device, HmmMode mode)
{
    const char* who = mode == HM_ESTEP ? "hmm_estep" : "hmm_score";
    HmmArgs A;
    int rc;
    if ((rc = hmm_setup<T>(who, rows, n, F, ld, offsets, n_traj, K, means, vars, transmat, log_startprob, on_device, true, &A)))
        return rc;
    return estep_run<T, HMM_GAUSS>(who, A, offsets, n_traj, segment, traj_logprob, post, obs, obs2, trans, logprob, mode);
}

static int lin_estep_impl(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets, msm_idx_t n_traj,
                          msm_idx_t K, const double* w, const double* cst, const double* transmat, const double* log_startprob,
                          msm_idx_t segment, double* traj_logprob, double* post, double* obs, double* trans, double* logprob,
                          HmmMode mode)
{
    const char* who = mode == HM_ESTEP ? "hmm_lin_estep" : "hmm_lin_score";
    HmmArgs A;
    int rc;
    if ((rc = hmm_lin_setup(who, Z, n, D, ldz, offsets, n_traj, K, w, cst, transmat, log_startprob, true, &A))) return rc;
    return estep_run<double, HMM_LINEAR>(who, A, offsets, n_traj, segment, traj_logprob, post, obs, nullptr, trans, logprob, mode);
}

template <typename T, int EM>
static int loglik_run(const char* who, HmmArgs& A, double* out, int on_device)
{
    const msm_idx_t n = A.n, K = A.K;
    int rc;
    if (!out) return fail(MSM_ERR_INVALID, "%s: null output", who);
    HmmBufs& B = bufs();
    if (on_device) {
        A.loglik = out;
    } else {
        if ((rc = B.out.reserve((size_t)n * K * sizeof(double)))) return rc;
        A.loglik = B.out.as<double>();
    }
    hipLaunchKernelGGL((hmm_loglik_kernel<T, EM>), dim3((unsigned)ceil_div(n * K, HMM_T)), dim3(HMM_T), 0, stream(), A);
    MSM_HIP_CHECK(hipGetLastError());
    if (!on_device && (rc = d2h_bulk(out, A.loglik, (size_t)n * K * sizeof(double)))) return rc;
    return hmm_flag(A);
}

template <typename T>
static int loglik_impl(const T* rows, msm_idx_t n, msm_idx_t F, msm_idx_t ld, msm_idx_t K, const double* means, const double* vars,
                       double* out, int on_device)
{
    HmmArgs A;
    int rc;
    if ((rc = hmm_setup<T>("hmm_loglik", rows, n, F, ld, nullptr, 0, K, means, vars, nullptr, nullptr, on_device, false, &A))) return rc;
    return loglik_run<T, HMM_GAUSS>("hmm_loglik", A, out, on_device);
}

template <typename T, int EM>
static int viterbi_run(const char* who, HmmArgs& A, const msm_idx_t* offsets, msm_idx_t n_traj, int* states, double* traj_logprob,
                       double* logprob)
{
    const msm_idx_t n = A.n, K = A.K;
    int rc;
    if (!states || !traj_logprob || !logprob) return fail(MSM_ERR_INVALID, "%s: null output", who);
    if ((rc = hmm_segments(&A, offsets, n_traj, 1 << 30))) return rc;
    HmmBufs& B = bufs();
    if ((rc = B.bp.reserve((size_t)n * K))) return rc;
    if ((rc = B.out.reserve((size_t)n * sizeof(int)))) return rc;
    if ((rc = B.vec.reserve((size_t)n_traj * sizeof(double)))) return rc;
    A.bp = B.bp.as<unsigned char>();
    A.states = B.out.as<int>();
    A.traj_lp = B.vec.as<double>();
    const long long lds = (K * K + (long long)HMM_VC * K + K) * (long long)sizeof(double) + (long long)HMM_VC * K;
    static long long vit_set = 48 * 1024;   // per instantiation
    if ((rc = raise_lds(hmm_viterbi_kernel<T, EM>, lds, &vit_set))) return rc;
    hipLaunchKernelGGL((hmm_viterbi_kernel<T, EM>), dim3((unsigned)n_traj), dim3(64), (size_t)lds, stream(), A);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpyAsync(traj_logprob, A.traj_lp, (size_t)n_traj * sizeof(double), hipMemcpyDeviceToHost, stream()));
    if ((rc = d2h_bulk(states, A.states, (size_t)n * sizeof(int)))) return rc;
    if ((rc = hmm_flag(A))) return rc;
    double total = 0.0;
    for (msm_idx_t j = 0; j < n_traj; ++j) total += traj_logprob[j];
    *logprob = total;
    return MSM_OK;
}

template <typename T>
static int viterbi_impl(const T* rows, msm_idx_t n, msm_idx_t F, msm_idx_t ld, const msm_idx_t* offsets, msm_idx_t n_traj, msm_idx_t K,
                        const double* means, const double* vars, const double* transmat, const double* log_startprob, int* states,
                        double* traj_logprob, double* logprob, int on_device)
{
    HmmArgs A;
    int rc;
    if ((rc = hmm_setup<T>("hmm_viterbi", rows, n, F, ld, offsets, n_traj, K, means, vars, transmat, log_startprob, on_device, true, &A)))
        return rc;
    return viterbi_run<T, HMM_GAUSS>("hmm_viterbi", A, offsets, n_traj, states, traj_logprob, logprob);
}

// The image Z = [cos X | sin X] of rows of T (host rows are staged first); Z is device memory.
template <typename T>
static int trig_impl(const T* rows, msm_idx_t n, msm_idx_t F, msm_idx_t ld, double* Z, msm_idx_t ldz, int on_device)
{
    if (n < 1) return fail(MSM_ERR_INVALID, "hmm_trig: sequences is empty");
    if (!rows || !Z) return fail(MSM_ERR_INVALID, "hmm_trig: null pointer");
    if (F < 1 || ld < F || F > (1 << 19) || ldz < 2 * F) return fail(MSM_ERR_INVALID, "hmm_trig: bad shape");
    if (msm_device_count() == 0) return fail(MSM_ERR_NODEVICE, "no HIP device visible");
    const T* X = rows;
    long long ldx = ld;
    if (!on_device) {
        HmmBufs& B = bufs();
        int rc;
        if ((rc = B.x.reserve((size_t)n * F * sizeof(T)))) return rc;
        if (ld == F) {
            if ((rc = h2d_bulk(B.x.p, rows, (size_t)n * F * sizeof(T)))) return rc;
        } else {
            MSM_HIP_CHECK(hipMemcpy2DAsync(B.x.p, (size_t)F * sizeof(T), rows, (size_t)ld * sizeof(T), (size_t)F * sizeof(T), (size_t)n,
                                           hipMemcpyHostToDevice, stream()));
        }
        X = B.x.as<T>();
        ldx = F;
    }
    // bound by HBM: a grid from the element count, capped at a multiple of the CUs, and a grid-stride loop
    const long long grid = std::min<long long>(ceil_div(n * F, HMM_T), (long long)HMM_TRIG_WAVES * num_cus());
    hipLaunchKernelGGL((hmm_trig_kernel<T>), dim3((unsigned)grid), dim3(HMM_T), 0, stream(), X, ldx, (long long)n, (int)F, Z, (long long)ldz);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipStreamSynchronize(stream()));   // (a staged host array may be reused by the next call)
    return MSM_OK;
}

}  // namespace msm

using namespace msm;

extern "C" {

#define MSM_HMM_ENTRY(SFX, T)                                                                                                        \
    int msm_hmm_estep_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const msm_idx_t* offsets,                 \
                            msm_idx_t n_traj, msm_idx_t n_states, const double* means, const double* vars, const double* transmat,   \
                            const double* log_startprob, msm_idx_t segment, double* traj_logprob, double* post, double* obs,         \
                            double* obs2, double* trans, double* logprob, int on_device)                                             \
    {                                                                                                                                \
        return estep_impl<T>(rows, n, n_features, ld, offsets, n_traj, n_states, means, vars, transmat, log_startprob, segment,      \
                             traj_logprob, post, obs, obs2, trans, logprob, on_device, HM_ESTEP);                                    \
    }                                                                                                                                \
    int msm_hmm_score_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const msm_idx_t* offsets,                 \
                            msm_idx_t n_traj, msm_idx_t n_states, const double* means, const double* vars, const double* transmat,   \
                            const double* log_startprob, msm_idx_t segment, double* traj_logprob, double* logprob, int on_device)    \
    {                                                                                                                                \
        return estep_impl<T>(rows, n, n_features, ld, offsets, n_traj, n_states, means, vars, transmat, log_startprob, segment,      \
                             traj_logprob, nullptr, nullptr, nullptr, nullptr, logprob, on_device, HM_SCORE);                        \
    }                                                                                                                                \
    int msm_hmm_loglik_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, msm_idx_t n_states,                     \
                             const double* means, const double* vars, double* out, int on_device)                                   \
    {                                                                                                                                \
        return loglik_impl<T>(rows, n, n_features, ld, n_states, means, vars, out, on_device);                                       \
    }                                                                                                                                \
    int msm_hmm_viterbi_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const msm_idx_t* offsets,               \
                              msm_idx_t n_traj, msm_idx_t n_states, const double* means, const double* vars,                        \
                              const double* transmat, const double* log_startprob, int* states, double* traj_logprob,               \
                              double* logprob, int on_device)                                                                        \
    {                                                                                                                                \
        return viterbi_impl<T>(rows, n, n_features, ld, offsets, n_traj, n_states, means, vars, transmat, log_startprob, states,     \
                               traj_logprob, logprob, on_device);                                                                    \
    }

MSM_HMM_ENTRY(f32, float)
MSM_HMM_ENTRY(f64, double)
#undef MSM_HMM_ENTRY

#define MSM_HMM_TRIG(SFX, T)                                                                                                         \
    int msm_hmm_trig_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, double* Z, msm_idx_t ldz, int on_device)  \
    {                                                                                                                                \
        return trig_impl<T>(rows, n, n_features, ld, Z, ldz, on_device);                                                             \
    }
MSM_HMM_TRIG(f32, float)
MSM_HMM_TRIG(f64, double)
#undef MSM_HMM_TRIG

int msm_hmm_lin_estep(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets, msm_idx_t n_traj,
                      msm_idx_t n_states, const double* w, const double* cst, const double* transmat, const double* log_startprob,
                      msm_idx_t segment, double* traj_logprob, double* post, double* obs, double* trans, double* logprob)
{
    return lin_estep_impl(Z, n, D, ldz, offsets, n_traj, n_states, w, cst, transmat, log_startprob, segment, traj_logprob, post, obs,
                          trans, logprob, HM_ESTEP);
}

int msm_hmm_lin_score(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets, msm_idx_t n_traj,
                      msm_idx_t n_states, const double* w, const double* cst, const double* transmat, const double* log_startprob,
                      msm_idx_t segment, double* traj_logprob, double* logprob)
{
    return lin_estep_impl(Z, n, D, ldz, offsets, n_traj, n_states, w, cst, transmat, log_startprob, segment, traj_logprob, nullptr,
                          nullptr, nullptr, logprob, HM_SCORE);
}

int msm_hmm_lin_loglik(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, msm_idx_t n_states, const double* w,
                       const double* cst, double* out)
{
    HmmArgs A;
    int rc;
    if ((rc = hmm_lin_setup("hmm_lin_loglik", Z, n, D, ldz, nullptr, 0, n_states, w, cst, nullptr, nullptr, false, &A))) return rc;
    return loglik_run<double, HMM_LINEAR>("hmm_lin_loglik", A, out, 1);
}

int msm_hmm_lin_viterbi(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets, msm_idx_t n_traj,
                        msm_idx_t n_states, const double* w, const double* cst, const double* transmat, const double* log_startprob,
                        int* states, double* traj_logprob, double* logprob)
{
    HmmArgs A;
    int rc;
    if ((rc = hmm_lin_setup("hmm_lin_viterbi", Z, n, D, ldz, offsets, n_traj, n_states, w, cst, transmat, log_startprob, true, &A)))
        return rc;
    return viterbi_run<double, HMM_LINEAR>("hmm_lin_viterbi", A, offsets, n_traj, states, traj_logprob, logprob);
}

int msm_hmm_plan(msm_idx_t n_states, msm_idx_t n_features, int itemsize, msm_idx_t* out8)
{
    if (!out8 || n_features < 1 || (itemsize != 4 && itemsize != 8)) return fail(MSM_ERR_INVALID, "msm_hmm_plan: bad argument");
    if (n_states < 1 || n_states > HMM_KMAX)
        return fail(MSM_ERR_INVALID, "msm_hmm_plan: n_states = %lld is outside 1 .. %d, the largest number of states this build serves",
                    (long long)n_states, HMM_KMAX);
    const HmmPlan pl = hmm_plan((int)n_states);
    out8[0] = pl.S_default;
    out8[1] = pl.S_max;
    out8[2] = HMM_KMAX;
    out8[3] = HMM_T;      // threads of a workgroup: a thread owns ceil(K^2 / this) entries of a K x K matrix
    out8[4] = HMM_EC;     // frames of an emission chunk in the operator pass
    out8[5] = HMM_G;      // workgroups (= partials) of the fused pass at most
    out8[6] = HMM_VC;     // frames of a Viterbi chunk
    out8[7] = hmm_fused_lds((int)n_states, pl.KP, pl.S_default) * (long long)sizeof(double);
    return MSM_OK;
}

}  // extern "C"
