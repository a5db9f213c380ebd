/*
 * msmhip.h -- C ABI of libmsmhip.so, the MI355X (gfx950) implementation of the
 * MSMBuilder tICA + geometric-clustering hot path.
 *
 * Plain C, caller-owned buffers, no exceptions, no stdout/stderr chatter.
 * Every entry point returns an int status (MSM_OK == 0, negative = error; the
 * message is available from msm_last_error()) unless noted.
 *
 * Pointer placement.  Functions that take `on_device` accept either host
 * pointers (on_device = 0: the library stages through its own device buffers)
 * or device pointers in the current HIP device's address space (on_device = 1:
 * e.g. torch.Tensor.data_ptr()).  `on_device` applies to the PER-ROW arrays
 * (X, X_indices, assignments, per-row distances, cdist's `out`); per-centre
 * arrays (y, Y, ids) and scalar outputs are always host memory.
 *
 * Threading: one host thread drives one device; handles are not thread-safe.
 * All work is enqueued on the stream set with msm_set_stream() (default: the
 * null stream, which is torch's default current stream).
 *
 * What each group replaces in the reference (paths under
 * /root/reference/msmbuilder):
 *   msm_tica_*        decomposition/tica.py:150-165 (_initialize), :401-424 (_fit),
 *                     :228-259 (the sums those properties read), :312-354 (transform)
 *   msm_dist_*        libdistance/src/dist.hpp:4-80     (via libdistance.pyx:229-270)
 *   msm_cdist_*       libdistance/src/cdist.hpp:4-49    (via libdistance.pyx:134-179)
 *   msm_assign_nearest_*  libdistance/src/assign.hpp:6-91 (via libdistance.pyx:82-131)
 *   msm_pdist_* / msm_sumdist_*  libdistance/src/pdist.hpp:4-88, sumdist.hpp:4-44 (via libdistance.pyx:182-226, 273-310)
 *   msm_kcenters_fit_*    cluster/kcenters.py:79-102 (_KCenters.fit's k-pass loop)
 *   msm_regspatial_fit_*  cluster/regularspatial.py:69-81 (_RegularSpatial.fit's per-row loop)
 *   msm_kmedoids*     cluster/src/kmedoids.cc:74-260 (via _kmedoids.pyx:23-107), with the pdist call in front of it
 *                     (cluster/kmedoids.py:91, cluster/minibatchkmedoids.py:83)
 *   msm_linkage* / msm_landmark_*  cluster/agglomerative.py:183-221 (pdist, the fastcluster linkage call, the loop over
 *                     all pairs) and :248-273 (predict: cdist + pooling per cluster)
 *   msm_divergence_*  utils/divergence.py:14-72 (the nested loops over rows and columns), as MVCA (lumping/mvca.py) runs them
 *                     through cluster/agglomerative.py:50-69
 *   msm_bace_*        lumping/bace.py:228-327 (the Bayes factors of all connected pairs and the merge loop)
 *   msm_kmeans_* / msm_mbk_*  sklearn MiniBatchKMeans arithmetic behind
 *                     cluster/__init__.py:67-69 (third-party)
 * The exact reference signatures of libdistance are additionally exported,
 * unprefixed, from include/msmhip_libdistance.h.
 */
#ifndef MSMHIP_H
#define MSMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int64_t msm_idx_t; /* npy_intp on LP64 */

enum msm_status {
    MSM_OK = 0,
    MSM_ERR_INVALID = -1,   /* bad argument (shape, null pointer, dtype code) */
    MSM_ERR_METRIC = -2,    /* unknown metric name (reference: prints "Error", returns -1) */
    MSM_ERR_HIP = -3,       /* a HIP runtime call failed */
    MSM_ERR_NODEVICE = -4,  /* no usable GPU */
    MSM_ERR_NONFINITE = -5, /* input contains NaN/Inf (reference: ValueError, validation.py:68-74) */
    MSM_ERR_STATE = -6      /* handle used before data / after destroy */
};

/* accumulate precision of the tICA covariance kernel */
enum msm_tica_mode {
    MSM_TICA_F32 = 0,  /* v_mfma_f32_32x32x2_f32, fp32 partials per <=4096-row chunk, fp64 merge */
    MSM_TICA_F64 = 1,  /* v_mfma_f64_16x16x4_f64 on fp64-widened inputs: the reference's arithmetic */
    MSM_TICA_BF16 = 2, /* v_mfma_f32_32x32x16_bf16 on inputs rounded to bf16, fp32 partials, fp64 merge */
    MSM_TICA_BF16X2 = 3 /* split x = hi + mid (two bf16 terms), four products on the bf16 MFMA: fp32-class sums */
};

/* ---- runtime ---------------------------------------------------------- */
const char* msm_last_error(void);
const char* msm_version(void);
int msm_device_count(void);          /* number of visible GPUs, 0 if none (never negative) */
int msm_init(int device);            /* hipSetDevice + arch check (gfx950) */
int msm_set_stream(void* hip_stream); /* hipStream_t; NULL = null stream */
int msm_synchronize(void);
int msm_device_info(char* name, int name_len, int* n_cu, int64_t* hbm_bytes);

/* device memory helpers (so callers without torch can keep data resident) */
int msm_malloc(void** dptr, size_t bytes);
int msm_free(void* dptr);
/* Blocking copies; bytes == 0 is a no-op whatever the pointers (an empty array has no address).  Large copies go through the
 * library's pinned staging ring, which has ONE submitter: like every other entry point these two must not be called from a
 * second host thread while another call of this library is in progress. */
int msm_memcpy_h2d(void* dst, const void* src, size_t bytes);
int msm_memcpy_d2h(void* dst, const void* src, size_t bytes);
int msm_memcpy_d2d(void* dst, const void* src, size_t bytes);
/* n host buffers back to back into one device buffer (dst must hold their sum), staged through the library's pinned ring
 * with no synchronisation between them; returns when the data is on the device.  What tICA.fit_transform uses to upload a
 * list of host trajectories ONCE for both passes. */
int msm_upload_list(void* dst, const void* const* src, const msm_idx_t* nbytes, msm_idx_t n);
/* out[i, :] = X[rows[i], :]  (X device or host per on_device; rows/out follow it) */
int msm_gather_rows(const void* X, int elem_size, msm_idx_t n_features, const msm_idx_t* rows,
                    msm_idx_t n_rows, void* out, int on_device);
/* HIP-event timing on the library's stream (bench.py's roofline leg) */
int msm_event_create(void** ev);
int msm_event_record(void* ev);
int msm_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
int msm_event_destroy(void* ev);

/* ---- communicator: RCCL over xGMI, one process per GPU ---------------
 * The reference is a single process (no collective exists in /root/reference); these are the exchange steps the
 * sharded hot path adds: msm_tica_allreduce, msm_kcenters_fit_sharded_*, msm_mbk_allreduce / msm_mbk_run.
 * Bootstrap: rank 0 calls msm_comm_unique_id and ships the 128 bytes to the other ranks by any means (parallel.py:
 * a torch.distributed broadcast); every rank then calls msm_comm_init_rccl AFTER msm_init(device).  The collectives
 * run on the library stream on device buffers.
 * msm_comm_init_host installs a host-side transport instead (buffers are staged through pinned memory and
 * fn(op, send, recv, nbytes) is called: op 0 = all-reduce(sum) of nbytes/8 doubles in place (send == recv), op 1 =
 * all-gather of nbytes from every rank into recv[world][nbytes]; non-zero return = failure).  It exists for runs
 * where RCCL cannot form a communicator -- several ranks on ONE GPU, gloo-only test runs. */
typedef int (*msm_host_collective_fn)(int op, void* send, void* recv, int64_t nbytes);
int msm_comm_rccl_available(void); /* 1: librccl loadable and a device visible.  Ranks must agree on this (an all-reduce
                                      MIN over the bootstrap channel) before ANY of them calls msm_comm_init_rccl, because
                                      ncclCommInitRank blocks until every rank has joined */
int msm_comm_unique_id(char* id128);
int msm_comm_init_rccl(const char* id128, int rank, int world); /* gives up after MSM_COMM_TIMEOUT_S seconds (180) with
                                      MSM_ERR_STATE and a message naming the rank: ncclCommInitRank cannot be cancelled, a rank
                                      that never joins must not hang the others for good */
int msm_comm_init_host(msm_host_collective_fn fn, int rank, int world);
int msm_comm_selftest(int timeout_s); /* one all-reduce + one all-gather of a few doubles through the installed communicator,
                                      checked and time-limited (0 ok; MSM_ERR_STATE: wrong numbers / no answer, message names the
                                      rank).  Every rank calls it right after the communicator is built */
int msm_comm_destroy(void);
int msm_comm_info(int* rank, int* world, int* kind); /* kind: 0 none, 1 RCCL, 2 host callback */
int msm_comm_allreduce_f64(double* dbuf, msm_idx_t n);                    /* device buffer, in place; synchronises */
int msm_comm_allgather(const void* dsend, void* drecv, msm_idx_t bytes);  /* device buffers; synchronises */
int msm_comm_measure(int kind, msm_idx_t bytes, int reps, float* us_per_call); /* latency of `reps` queued collectives of `bytes`
                                      per rank (kind 0: all-reduce of doubles, 1: all-gather), microseconds per call; every
                                      rank calls it (bench.py reports these instead of assumptions when it runs on N > 1) */

/* ---- tICA second-moment accumulation ---------------------------------- */
typedef struct msm_tica msm_tica_t;

int msm_tica_create(msm_tica_t** h, msm_idx_t n_features, msm_idx_t lag_time, int mode);
int msm_tica_destroy(msm_tica_t* h);
int msm_tica_reset(msm_tica_t* h); /* zero all accumulators and counters */

/* One trajectory X[n_rows, n_features] (row stride ld elements), dtype_bytes = 4 (f32) or 8 (f64).
 * Lagged pairs never span calls.  n_rows <= lag_time is a no-op with *skipped = 1
 * (tica.py:410-412).  check_finite != 0: the call synchronises and returns
 * MSM_ERR_NONFINITE, state unchanged, if X holds NaN/Inf; check_finite == 0: fully
 * asynchronous, a sticky flag is kept (msm_tica_nonfinite). */
/* dtype_bytes = 2: bfloat16-STORED trajectories (BASELINE configs[4]: half the bytes per frame), accepted by the
 * MSM_TICA_BF16 / MSM_TICA_BF16X2 modes (MSM_ERR_INVALID otherwise), device-resident or host. */
int msm_tica_accumulate(msm_tica_t* h, const void* X, int dtype_bytes, msm_idx_t n_rows,
                        msm_idx_t ld, int on_device, int check_finite, int* skipped);
/* Many trajectories in one launch: X_ptrs[s] -> n_rows[s] x n_features, common ld.
 * X_ptrs / n_rows are host arrays of length n_seq; the trajectories themselves are
 * device-resident (on_device = 1) or host (0).  *n_skipped counts too-short ones. */
int msm_tica_accumulate_batch(msm_tica_t* h, const void* const* X_ptrs, const msm_idx_t* n_rows,
                              msm_idx_t n_seq, int dtype_bytes, msm_idx_t ld, int on_device,
                              int check_finite, msm_idx_t* n_skipped);
/* Slices of trajectories, for splitting ONE long trajectory over ranks (the sum over
 * lagged pairs of tica.py:417-422 restricted to the pairs whose LEFT frame a rank owns).
 * seg4[4*s + {0,1,2,3}] = {trajectory length, trajectory row of X_ptrs[s][0], own_begin, own_end}:
 * the call adds the terms of the left frames t in [own_begin, own_end) only and needs the slice to
 * reach row min(own_end + lag_time, length) - 1 (right halo; MSM_ERR_INVALID otherwise).
 * n_observations grows by own_end - own_begin, n_sequences by 1 where own_begin == 0, so the
 * all-reduced counters equal the unsplit fit's.  {n, 0, 0, n} is msm_tica_accumulate_batch. */
int msm_tica_accumulate_segments(msm_tica_t* h, const void* const* X_ptrs, const msm_idx_t* n_rows,
                                 const msm_idx_t* seg4, msm_idx_t n_seq, int dtype_bytes, msm_idx_t ld,
                                 int on_device, int check_finite, msm_idx_t* n_skipped);
int msm_tica_nonfinite(msm_tica_t* h, int* flag); /* synchronises; sticky until reset */
/* 1 when this handle accumulates fp32 input with the symmetric sum/difference kernel (MSM_TICA_F32,
 * 128 < n_features <= 3968, n_features % 4 == 0; MSM_TICA_SYM=0 disables): the "C" it exports is then
 * already (C + C^T) / 2 -- the only form the estimator reads (tica.py:234-241) -- and the raw
 * X[:-tau].T @ X[tau:] is not kept. */
int msm_tica_lagged_symmetrised(msm_tica_t* h, int* flag);
/* HIP-event duration (ms) of the most recent MFMA accumulation launch of this handle,
 * measured on the stream it ran on (bench.py's roofline leg); synchronises on it.  bf16 modes: the whole pipeline --
 * float32 rows: pack, then multiply, super-chunk after super-chunk in turn on one stream (sequential: overlapping them
 * was measured slower); with MSM_TICA_IMG_FUSED=1 on bfloat16-stored rows: the step-record kernel + the fused kernel. */
int msm_tica_last_kernel_ms(msm_tica_t* h, float* ms);
/* 1 when the most recent accumulation launch had no column-sum pass over X of its own: the sum/difference kernel's
 * staging lanes summed the left frames (float32 input, whole trajectories of >= 2 lag frames, n_features % 128 == 0, at
 * least MSM_TICA_FOLD_MIN = 2^26 elements; MSM_TICA_FOLD=0 disables).  The sums (tica.py:418-419) and the finite check
 * (utils/validation.py:68-74; a rejected launch is undone) are the same either way. */
int msm_tica_last_folded(msm_tica_t* h, int* flag);
/* 1 when the most recent accumulation launch of a bf16 / bf16x2 handle ran the FUSED kernel (round 5; opt-in,
 * MSM_TICA_IMG_FUSED=1): bfloat16-stored rows, n_features % 256 == 0, ld % 8 == 0, 16-byte aligned trajectories -- the MFMA
 * kernel's load role stages the raw rows in LDS and forms the pair frames itself, no packed image is written
 * (tica.py:402-422 in one streamed pass + a column-sum pass).  Bit-identical accumulators to the packed-image pipeline on such
 * input, half its fabric traffic, no image ring -- and measured slower, hence not the default. */
int msm_tica_last_img_fused(msm_tica_t* h, int* flag);
/* 1 when the most recent accumulation launch of a bf16 / bf16x2 handle packed its later super-chunks of the image INSIDE the
 * multiply kernel (round 6, the carried pack: whole 256-feature panels, 16-byte aligned rows, more than one super-chunk;
 * MSM_TICA_IMG_CARRY=0 disables): the packets, and hence the accumulators, are the pre-pass kernel's bit for bit. */
int msm_tica_last_img_carried(msm_tica_t* h, int* flag);
/* What an accumulation launches -- the library's one dispatch (tica_plan, csrc/tica_plan.h), for tests to ask.
 * msm_tica_plan is pure (works with no device visible) and plans whole trajectories: geom[MSM_TICA_GEOM_INTS] is a handle's
 * geometry {F, lag, mode, T, ntiles, S32, S64, sym, ntiles_sym, sym_cohorts, sym_grid, S_sym, symw, symw_var, symw_KS, symw_S,
 * symw64, symw_S64, img_on, T2, ntile2, S_img, img_grid, have_fold, shift_on} (ntiles_sym: workgroups per cohort of the
 * sum/difference kernel -- upper tiles, fewer when the handle packs diagonal blocks, msm_tica_sym_units); ptr_aligned16: bit 0 = every trajectory longer
 * than the lag starts on a 16-byte boundary, bit 1 = the skipped ones do too; dims_aligned4: n_features % 4 == 0 && ld % 4 == 0; fold_switch / fused_switch: the
 * values of MSM_TICA_FOLD / MSM_TICA_IMG_FUSED (-1: unset).  out[MSM_TICA_PLAN_INTS] = {path (MSM_TICA_PATH_*), flavour
 * (MSM_TICA_FL_* bits), frames per K-step, cohorts S, workgroups G, remainder cohort, frames per chunk kc, remainder workgroups,
 * remainder rounds, pair semantics, shifted, folded column sums, kflush, cohort pacing, single (one trajectory, no chunk
 * table), owned frames, valid trajectories}.  MSM_ERR_INVALID for a geometry no handle has (no cohort for an enabled path).
 * msm_tica_last_plan: out[MSM_TICA_GEOM_INTS + MSM_TICA_PLAN_INTS + 2] = the handle's geometry, the plan of its most recent
 * accumulation launch, that launch's chunks and -- bf16 image ring -- super-chunks (else 0). */
enum { MSM_TICA_PATH_NONE = 0, MSM_TICA_PATH_CG64 = 1, MSM_TICA_PATH_CG32 = 2, MSM_TICA_PATH_SYM = 3, MSM_TICA_PATH_SYMW = 4,
       MSM_TICA_PATH_SYMW64 = 5, MSM_TICA_PATH_IMG_RING = 6, MSM_TICA_PATH_IMG_FUSED = 7 };
enum { MSM_TICA_FL_EDGE = 1, MSM_TICA_FL_ALIGNED = 2, MSM_TICA_FL_FOLD = 4, MSM_TICA_FL_REM = 8, MSM_TICA_FL_VEC = 16, MSM_TICA_FL_X2 = 32 };
enum { MSM_TICA_GEOM_INTS = 25, MSM_TICA_PLAN_INTS = 17 };
int msm_tica_plan(const int* geom, int dtype_bytes, msm_idx_t ld, const msm_idx_t* n_rows, msm_idx_t n_seq, int ptr_aligned16,
                  int dims_aligned4, int fold_switch, int fused_switch, long long* out);
int msm_tica_last_plan(msm_tica_t* h, long long* out);
/* The units of one cohort of the sum/difference kernel for T tiles per side (csrc/tica_sym_units.h; pure, no device): a unit
 * is one workgroup's work, MSM_TICA_SYM_UNIT_INTS ints {X column tile, Y column tile, writes the folded column sums of block X,
 * then for each of its four waves {row panel (0 = X, 1 = Y), row offset (0 | 64), column panel, column offset, slab tile}}.
 * pack = 0: the upper tiles in row-major order, T (T+1)/2 units; pack = 1: the diagonal tiles in groups of four give up the
 * mirrored 64 x 64 corner nobody reads -- one tile of a group lends its three blocks to the free waves of the other three --
 * T (T+1)/2 - T/4 units (what a handle launches when ntiles_sym of its geometry says so; MSM_TICA_SYM_PACK=0 at create: never).
 * Writes min(units, cap) units to out (may be null with cap = 0) and returns the number of units, or a negative MSM_ERR_*. */
enum { MSM_TICA_SYM_UNIT_INTS = 23 };
int msm_tica_sym_units(int T, int pack, int* out, int cap);
/* The chunk walks of a packed launch (csrc/tica_sym_units.h, tica_sym_walk; pure): chunk c holds chunk_rows[c] frames.  A
 * cohort v of `stride` takes the chunks v, v + stride, ... and merges its fp32 accumulators when another kc frames would pass
 * kflush, or at its end.  Either the S cohorts of the packed handle stride themselves, or -- where the fullest cohort is
 * within 1 % of that (frames + 16 per chunk) -- the groups between two merges are those S0 UNPACKED cohorts form, dealt whole
 * to the S cohorts, each to the lightest so far: the fp32 partials are then what they are without packing.
 * out[cap], cap >= S + 1 + n_chunks: S + 1 offsets into the entries, then one entry per chunk: its index, bit 31 set where the
 * cohort merges after it.  Returns 1 when the unpacked partials were kept, 0 when the cohorts stride, a negative MSM_ERR_*. */
int msm_tica_sym_walk(const int* chunk_rows, msm_idx_t n_chunks, int S0, int S, msm_idx_t kc, msm_idx_t kflush, int* out,
                      msm_idx_t cap);
/* profiling: {shader-clock start, end, 100 MHz wall-clock start, end} of workgroup 0 of that launch */
int msm_tica_debug_clocks(msm_tica_t* h, long long* out4);
/* profiling builds (csrc built with -DMSM_TICA_PROFILE) only: out64[8 + 8*slot + i] = shader cycles wave 0 of
 * five sample workgroups spent in section i of the fp32 kernel {chunk prologue, step head, MFMA loop,
 * step tail, final merge, inter-chunk merge}; zeros in a product build */
int msm_tica_debug_profile(msm_tica_t* h, long long* out64);

/* Accumulators as the reference defines them (float64, row-major F x F / F):
 *   C    = sum_traj X[:-tau].T @ X[tau:]                    (tica.py:417; its symmetric part only when
 *                                                            msm_tica_lagged_symmetrised says so)
 *   G    = sum_traj X[:-tau].T @ X[:-tau] + X[tau:].T @ X[tau:]   (tica.py:421-422, only their sum is ever read: :245)
 *   s0   = sum_traj X[:-tau].sum(0)   stau = sum_traj X[tau:].sum(0)   (tica.py:418-419)
 *   n_observations, n_sequences                               (tica.py:414-415)
 * Host pointers. */
int msm_tica_export(msm_tica_t* h, double* C, double* G, double* s0, double* stau,
                    msm_idx_t* n_observations, msm_idx_t* n_sequences);
int msm_tica_import(msm_tica_t* h, const double* C, const double* G, const double* s0,
                    const double* stau, msm_idx_t n_observations, msm_idx_t n_sequences);
/* Packed form for one RCCL all-reduce(sum) over xGMI (torch.distributed):
 * doubles [C (F*F) | G (F*F) | s0 (F) | stau (F) | n_observations | n_sequences]. */
msm_idx_t msm_tica_packed_size(msm_tica_t* h); /* number of doubles */
int msm_tica_export_packed(msm_tica_t* h, double* buf, int on_device);
int msm_tica_import_packed(msm_tica_t* h, const double* buf, int on_device);

/* s0 / stau alone (host, F doubles each): the means without the two F x F downloads. */
int msm_tica_export_sums(msm_tica_t* h, double* s0, double* stau);

/* Device-resident finalisation + solve of the generalized eigenproblem of tica.py:167-259 (replaces the host-side
 * `_solve` body: offset_correlation_, covariance_ incl. the Rao-Blackwell Ledoit-Wolf shrinkage of tica.py:492-524,
 * and scipy.linalg.eigh(lhs, b=rhs, eigvals=(F-k, F-1)) of tica.py:188-194).  Nothing F x F crosses PCIe except, in
 * the hybrid form, the one reduced matrix.
 *   shrinkage < 0 (or NaN): the RBLW estimate with n = n_rblw (= n_observations_); otherwise the given intensity.
 *   scale: NULL, or F host doubles s of a folded input scaling x' = (x - m) / s (moments scale by 1 / (s_i s_j)).
 *   mu (host, F): the RAW means (s0 + stau) / 2N'.   info (host, 8 doubles, nullable): {rho, tr S, potrf info,
 *   syevd info, OC non-finite, S non-finite}.
 * Errors: MSM_ERR_NONFINITE with the reference's RuntimeError texts ("... is not symmetric") when a moment is not
 * finite; MSM_ERR_INVALID with LAPACK's "leading minor ... not positive definite" text; MSM_ERR_STATE before any data.
 *
 * msm_tica_reduce: B = L L^T, Cs = L^-1 OC L^-T on the device; Cs (host, F x F, symmetric up to rounding) is returned
 * for a top-k standard eigensolver on the host (LAPACK dsyevr: its tridiagonalisation is latency-bound on a GPU at
 * F = 512); msm_tica_backsolve then maps k eigenvectors y of Cs (rows of Y, host k x F) to v = L^-T y (rows of V),
 * B-orthonormal like LAPACK's dsygvx.  msm_tica_solve_device does everything on the device (rocSOLVER dsyevd; wins
 * from F ~ 1024) and returns the k largest eigenvalues (descending) and their eigenvectors as rows. */
int msm_tica_reduce(msm_tica_t* h, double shrinkage, msm_idx_t n_rblw, const double* scale, double* Cs, double* mu,
                    double* info);
int msm_tica_backsolve(msm_tica_t* h, const double* Y, msm_idx_t k, double* V);
/* The top-k solve on the device (128 <= n_features <= 1024, k <= 16): msm_tica_reduce's finalisation and reduction
 * (Cholesky by the library's own blocked kernel), a Chebyshev-filtered subspace iteration on the reduced matrix
 * (csrc/subspace.hip; its 32 x 32 Rayleigh-Ritz problems are solved on the host, so it synchronises a few times),
 * v = L^-T y.  vals[k] descending, vecs[k][F] rows B-orthonormal like dsygvx's, mu[F], info[12]: [0..5] as
 * msm_tica_reduce, info[6] = max_j ||Cs y_j - lambda_j y_j||_inf, info[7] = max(max_j | ||y_j||^2 - 1 |, max_{i<j} |y_i.y_j|),
 * info[8] = 1 if pairs were returned, info[9] = filtered iterations spent.
 * *status = 0: pairs returned and verified on the reduced matrix (residual, norm, mutual orthogonality); 1: the iteration
 * did not converge (flat spectra); 2: the check failed -- in both cases Cs (host, F x F) holds the reduced matrix for the
 * caller's LAPACK route (msm_tica_backsolve afterwards). */
int msm_tica_solve_topk(msm_tica_t* h, double shrinkage, msm_idx_t n_rblw, const double* scale, msm_idx_t k, double* vals,
                        double* vecs, double* Cs, double* mu, double* info, int* status);
/* Building block, exported for the tests: Cholesky B = U^T U on the row-major upper triangle (LAPACK dpotrf 'L' on the
 * column-major view), *info = first non-positive pivot (1-based) or 0. */
int msm_potrf(double* B, msm_idx_t n, int* info, int on_device);
int msm_tica_solve_device(msm_tica_t* h, double shrinkage, msm_idx_t n_rblw, const double* scale, msm_idx_t k,
                          double* vals, double* vecs, double* mu, double* info);

/* Sum the accumulators over all ranks of the library communicator: ONE all-reduce of the packed float64
 * [C | G | s0 | stau | n_obs | n_seq] (4.2 MB at F = 512), device to device; every rank ends with the global model.
 * Without a communicator (or with one rank) it is a no-op. */
int msm_tica_allreduce(msm_tica_t* h);
int msm_tica_counts(msm_tica_t* h, msm_idx_t* n_observations, msm_idx_t* n_sequences); /* frames / trajectories seen */

/* out[n, k] (float64) = (X - mean) @ comps.T, comps is k x F row-major, mean/comps host
 * float64 (tica.py:329-333; any kinetic/commute column scaling is folded into comps by
 * the caller).  X / out follow on_device.  check_finite as above.  dtype_bytes = 2: bfloat16-STORED rows, widened
 * (exactly) inside the kernel -- the result equals the projection of their float32 images. */
int msm_tica_project(const void* X, int dtype_bytes, msm_idx_t n_rows, msm_idx_t n_features,
                     msm_idx_t ld, const double* mean, const double* comps, msm_idx_t k,
                     double* out, int on_device, int check_finite);
/* The same for a LIST of device-resident trajectories in one launch per block of 16 components (tica.py:329-352 walks the
 * list): X_ptrs[s] is [n_rows[s], n_features] with row stride n_features, out_ptrs[s] its [n_rows[s], k] float64 output.
 * Rows must be whole 16-byte vectors at 16-byte aligned addresses; MSM_ERR_INVALID otherwise (project one by one then). */
int msm_tica_project_batch(const void* const* X_ptrs, double* const* out_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq,
                           int dtype_bytes, msm_idx_t n_features, const double* mean, const double* comps, msm_idx_t k,
                           int check_finite);
/* The same for a LIST of HOST trajectories of float32 / float64 rows (dtype_bytes 4 / 8, row stride n_features): `out`
 * (host) is ONE [sum of n_rows][k] float64 array, trajectory after trajectory.  Staged over PCIe in groups through two
 * device buffers, group g + 1 copied while group g is projected, one copy back at the end (tica.py:329-352 walks the
 * list of numpy arrays one by one). */
int msm_tica_project_host_list(const void* const* X_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int dtype_bytes,
                               msm_idx_t n_features, const double* mean, const double* comps, msm_idx_t k, double* out,
                               int check_finite);
/* Which kernel a projection of rows of n_features elements of dtype_bytes (2 | 4 | 8) at row stride ld launches -- the
 * library's one dispatch, for tests to ask (pure: works with no device visible).  With cw = 16 / dtype_bytes elements per
 * 16-byte vector, rows are read with vector loads (*vec = 1) when the base pointer is 16-byte aligned (aligned16) and both
 * n_features and ld are multiples of cw, element by element (*vec = 0) otherwise.  Vector rows take the fp64-MFMA kernel
 * (MSM_PJ_MFMA) while 256 * ld * dtype_bytes < 2^32 -- its row offsets inside a 256-row tile are 32-bit -- and the
 * lane-per-row kernel (MSM_PJ_ROWS) from that stride on; rows without vector loads always take MSM_PJ_ROWS.
 * msm_tica_project_batch admits exactly the widths for which (n_features, ld = n_features, aligned16 = 1) is MSM_PJ_MFMA. */
enum { MSM_PJ_MFMA = 0, MSM_PJ_ROWS = 1 };
int msm_tica_project_plan(int dtype_bytes, msm_idx_t n_features, msm_idx_t ld, int aligned16, int* kernel, int* vec);
/* What the last projection calls of this process did: out2 = {groups the last msm_tica_project_host_list call staged its rows
 * in, 256-row tiles of the last msm_tica_project_batch call}; 0 for a call that had no rows or was refused.  The host list's
 * groups hold MSM_TICA_PROJ_GROUP_BYTES bytes of rows (read per call; unset or not positive: 512 MiB): whole trajectories in
 * order, a new group where the next trajectory would pass the budget of a group that already holds rows. */
int msm_tica_project_last_stats(msm_idx_t* out2);

/* ---- libdistance: exact-arithmetic vector metrics --------------------- */
/* metric in {"euclidean","sqeuclidean","cityblock","chebyshev","canberra",
 *            "braycurtis","hamming","jaccard"}; results are bit-identical to the
 * reference's scalar loops (float subtract -> double accumulate, feature order,
 * sqrt before compare, strict <, lowest index wins).  out/min_dist are float64. */
int msm_dist_f32(const float* X, const float* y, const char* metric, msm_idx_t n, msm_idx_t m,
                 const msm_idx_t* X_indices, msm_idx_t n_X_indices, double* out, int on_device);
int msm_dist_f64(const double* X, const double* y, const char* metric, msm_idx_t n, msm_idx_t m,
                 const msm_idx_t* X_indices, msm_idx_t n_X_indices, double* out, int on_device);
int msm_cdist_f32(const float* XA, const float* XB, const char* metric, msm_idx_t na,
                  msm_idx_t nb, msm_idx_t m, double* out, int on_device);
int msm_cdist_f64(const double* XA, const double* XB, const char* metric, msm_idx_t na,
                  msm_idx_t nb, msm_idx_t m, double* out, int on_device);
/* pdist.hpp:4-88: condensed upper triangle of the (indexed) rows, out has n(n-1)/2 entries;
 * sumdist.hpp:4-44: sum over the listed pairs (pairs is [p][2], follows on_device; the reference
 * sums sequentially, here an fp64 tree sum). */
int msm_pdist_f32(const float* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices,
                  msm_idx_t n_X_indices, double* out, int on_device);
int msm_pdist_f64(const double* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices,
                  msm_idx_t n_X_indices, double* out, int on_device);
int msm_sumdist_f32(const float* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* pairs,
                    msm_idx_t p, double* sum, int on_device);
int msm_sumdist_f64(const double* X, const char* metric, msm_idx_t n, msm_idx_t m, const msm_idx_t* pairs,
                    msm_idx_t p, double* sum, int on_device);
/* assignments[i] = argmin_j metric(X[i or X_indices[i]], Y[j]); min_dist nullable;
 * *inertia = sum_i min_dist[i] (fp64 tree sum; the reference sums sequentially). */
int msm_assign_nearest_f32(const float* X, const float* Y, const char* metric,
                           const msm_idx_t* X_indices, msm_idx_t n_X, msm_idx_t n_Y,
                           msm_idx_t n_features, msm_idx_t n_X_indices, msm_idx_t* assignments,
                           double* min_dist, double* inertia, int on_device);
int msm_assign_nearest_f64(const double* X, const double* Y, const char* metric,
                           const msm_idx_t* X_indices, msm_idx_t n_X, msm_idx_t n_Y,
                           msm_idx_t n_features, msm_idx_t n_X_indices, msm_idx_t* assignments,
                           double* min_dist, double* inertia, int on_device);

/* Gonzalez k-centers (kcenters.py:79-102): K fused dist + running-min + argmax passes,
 * no host round trip inside the loop.  ids (host, K) = chosen row indices, first =
 * seed_index; labels (int64) / distances (float64) per row follow on_device;
 * *inertia = sum(distances). */
int msm_kcenters_fit_f32(const float* X, msm_idx_t n, msm_idx_t m, msm_idx_t n_clusters,
                         const char* metric, msm_idx_t seed_index, msm_idx_t* ids,
                         msm_idx_t* labels, double* distances, double* inertia, int on_device);
int msm_kcenters_fit_f64(const double* X, msm_idx_t n, msm_idx_t m, msm_idx_t n_clusters,
                         const char* metric, msm_idx_t seed_index, msm_idx_t* ids,
                         msm_idx_t* labels, double* distances, double* inertia, int on_device);
/* the same fit, also returning the chosen rows themselves: centers[n_clusters][m] (HOST memory) = X[ids]
 * (kcenters.py:98 cluster_centers_), in the fit's final synchronisation */
int msm_kcenters_fit2_f32(const float* X, msm_idx_t n, msm_idx_t m, msm_idx_t n_clusters, const char* metric,
                          msm_idx_t seed_index, msm_idx_t* ids, msm_idx_t* labels, double* distances, double* inertia,
                          int on_device, float* centers);
int msm_kcenters_fit2_f64(const double* X, msm_idx_t n, msm_idx_t m, msm_idx_t n_clusters, const char* metric,
                          msm_idx_t seed_index, msm_idx_t* ids, msm_idx_t* labels, double* distances, double* inertia,
                          int on_device, double* centers);

/* One externally driven k-centers pass for row-sharded data (one process per GPU): the centre's
 * coordinates y (host, m values; it may live on another rank) are supplied, distances_/labels_
 * (device) get the strict running-min update with label `it`, and the shard-local
 * (max distance, lowest local row attaining it, that row's m coordinates -- host, nullable)
 * come back for the cross-rank argmax: one small D2H per pass. */
int msm_kcenters_pass_f32(const float* X, msm_idx_t n, msm_idx_t m, const float* y, msm_idx_t it,
                          const char* metric, msm_idx_t* labels, double* distances, double* max_dist,
                          msm_idx_t* argmax, float* argmax_row, int on_device);
int msm_kcenters_pass_f64(const double* X, msm_idx_t n, msm_idx_t m, const double* y, msm_idx_t it,
                          const char* metric, msm_idx_t* labels, double* distances, double* max_dist,
                          msm_idx_t* argmax, double* argmax_row, int on_device);

/* The same pass with NOTHING on the host (multi-GPU driver, one collective per centre and no
 * synchronisation): y_dev is the centre on the device; after the pass the shard's candidate record
 * cand_dev[2 + m] (device, float64) = {max distance, row_offset + lowest local row attaining it,
 * that row's coordinates}, or {-1, -1, 0...} for an empty shard.  Ranks all-gather their records
 * (RCCL) into cands_dev[world][2 + m]; msm_kcenters_select picks the winner (largest distance, ties
 * to the lowest global row = numpy's argmax on the concatenated array) and writes its coordinates
 * to y_dev and to row `slot` of centers_dev, its global row to ids_dev[slot].  All asynchronous on
 * the library stream. */
int msm_kcenters_pass_dev_f32(const float* X, msm_idx_t n, msm_idx_t m, const float* y_dev, msm_idx_t it,
                              const char* metric, msm_idx_t* labels, double* distances, msm_idx_t row_offset,
                              double* cand_dev);
int msm_kcenters_pass_dev_f64(const double* X, msm_idx_t n, msm_idx_t m, const double* y_dev, msm_idx_t it,
                              const char* metric, msm_idx_t* labels, double* distances, msm_idx_t row_offset,
                              double* cand_dev);
int msm_kcenters_select_f32(const double* cands_dev, msm_idx_t world, msm_idx_t m, float* y_dev, float* centers_dev,
                            msm_idx_t* ids_dev, msm_idx_t slot);
int msm_kcenters_select_f64(const double* cands_dev, msm_idx_t world, msm_idx_t m, double* y_dev, double* centers_dev,
                            msm_idx_t* ids_dev, msm_idx_t slot);

/* The whole row-sharded k-centers fit in one call (every rank of the library communicator calls it with ITS block of
 * rows; ranks own consecutive blocks of the global array, this one starting at global row row_offset): per centre one
 * pass kernel, one candidate record, ONE all-gather of the world's records (RCCL on the library stream) and one select
 * kernel -- nothing returns to the host inside the loop.  seed_index is the GLOBAL row of centre 0.  labels / distances
 * (device, n_local) stay sharded; ids (host, K global rows), centers (host, K x m) and *inertia (sum over ALL rows) are
 * the same on every rank and equal the single-process fit of the concatenated array bit for bit (ties go to the lowest
 * global row, numpy's argmax: kcenters.py:91-97). */
int msm_kcenters_fit_sharded_f32(const float* X, msm_idx_t n_local, msm_idx_t m, msm_idx_t n_clusters, const char* metric,
                                 msm_idx_t seed_index, msm_idx_t row_offset, msm_idx_t* labels, double* distances,
                                 msm_idx_t* ids, float* centers, double* inertia);
int msm_kcenters_fit_sharded_f64(const double* X, msm_idx_t n_local, msm_idx_t m, msm_idx_t n_clusters, const char* metric,
                                 msm_idx_t seed_index, msm_idx_t row_offset, msm_idx_t* labels, double* distances,
                                 msm_idx_t* ids, double* centers, double* inertia);

/* What the last k-centers fit of this process streamed: out5 = {rows, plain passes, screened passes, bytes a plain pass
 * reads per row (the row + distances_ + labels_), bytes a screened pass reads per row (the low-precision copy + the
 * rounded-up distance)}.  bench.py derives its bytes-per-pass figure from it (exact re-evaluations of screen candidates
 * and the updates are not counted: a lower bound on the traffic). */
int msm_kcenters_last_stats(msm_idx_t* out5);
/* Wide screened passes (round 6: float32 rows, float64 rows of more than 16 features; csrc/distance_wscreen_dev.h), with
 * MSM_KC_STATS=1 in the environment of the fit: out2 = {rows re-evaluated exactly over all screened passes, rows that changed}. */
int msm_kcenters_last_wide_stats(msm_idx_t* out2);
/* Batched screened passes of the last k-centers fit (several centres per pass): out1 = {rounds whose threshold list was
 * unusable, so that the pass applied one centre}; 0 when the fit ran no batches. */
int msm_kcenters_last_batch_fallbacks(msm_idx_t* out1);

/* Regular spatial (leader) clustering (cluster/regularspatial.py:69-81): row 0 is a centre, row i > 0 is a centre iff
 * metric(X[c], X[i]) > d_min for EVERY centre c chosen before it (a NaN distance or d == d_min makes none; d_min < 0
 * makes every row with finite distances one).  Runs in row blocks on the device -- screen against the known centres,
 * compact the uncovered rows, resolve them in row order in one workgroup -- with one host synchronisation per block;
 * every distance is the exact one of msm_dist_*, so ids equal the sequential loop's.  X (n x m) follows on_device.
 *   block_rows: 0 = the library's rule (4,096 rows first; x 4 after a block that found at most one centre per 64 rows,
 *   / 2 after one that found more than one per 8, within [1,024, 2^22]); > 0 = every block has this many rows (tests put
 *   block seams inside small inputs with it; at most 2^22).
 *   *n_centers (host) = K, which no one knows in advance: the centre list is owned by the library, grows by doubling
 *   (no cap on K), and stays valid until the next fit.  msm_regspatial_result_* then copies it out: ids (host, K) = the
 *   chosen rows in the order chosen (ascending), centers (host, K x m, X's element type) = X[ids].  MSM_ERR_STATE
 *   when the last finished fit was not of this element type.
 * On an error (MSM_ERR_METRIC for a null / unknown metric name, MSM_ERR_INVALID for a bad shape) nothing is written. */
int msm_regspatial_fit_f32(const float* X, msm_idx_t n, msm_idx_t m, const char* metric, double d_min,
                           msm_idx_t block_rows, int on_device, msm_idx_t* n_centers);
int msm_regspatial_fit_f64(const double* X, msm_idx_t n, msm_idx_t m, const char* metric, double d_min,
                           msm_idx_t block_rows, int on_device, msm_idx_t* n_centers);
int msm_regspatial_result_f32(msm_idx_t* ids, float* centers);
int msm_regspatial_result_f64(msm_idx_t* ids, double* centers);
/* What the last regular spatial fit of this process did: out4 = {blocks run, survivors handed to the resolve step,
 * resolve rounds (= centres chosen), growths of the centre list}. */
int msm_regspatial_last_stats(msm_idx_t* out4);

/* K-medoids clustering on a condensed distance matrix (cluster/src/kmedoids.cc:74-260): npass passes of {medoid of
 * every cluster = its lowest-index member of lowest summed distance to the other members; every element to the first
 * cluster, in cluster order, whose medoid is strictly nearest; total = sum of those distances} until the total stops
 * falling or a periodically saved assignment comes back.  Every sum is added in the reference's order by one lane, so
 * clusterid, error and ifound are the reference's bit for bit.  The matrix stays on the device: a handful of launches and
 * ONE host synchronisation per iteration, or -- n <= 180, the matrix fits one workgroup's LDS -- one launch per pass
 * (MSM_KMEDOIDS_SMALL=0: always the general path).
 *   dmat: n(n-1)/2 doubles, entry (i, j), i < j, at msm_kmedoids_condensed_index(i, j, n); follows on_device.
 *   init (host, max(npass, 1) x n): the assignment each pass starts from, values in [0, K), no cluster empty.  npass = 0
 *   runs one pass from the caller's assignment; for npass >= 1 the caller draws the random assignments the reference draws
 *   inside its loop (they do not depend on the data).
 *   clusterid (host, n, out): the medoid's element index for every element; *error: the best pass's total; *ifound: how
 *   often it was found.  For npass <= 1 the reference works in place and compares labels with medoid ids: when every
 *   label equals its medoid's index, *error stays DBL_MAX and *ifound is 0 (kept).
 * MSM_ERR_INVALID: K < 1, K > n, npass < 0, an init value outside [0, K), an empty cluster in init (the reference reads an
 * unset medoid there), a negative entry of dmat (distances are >= 0: the medoid selection orders the summed costs by their
 * bit patterns); MSM_ERR_METRIC: null / unknown metric; MSM_ERR_NONFINITE: a NaN or infinite distance or sum (the
 * reference's loop is not defined for them).  On an error nothing is written.
 * msm_kmedoids_fit_*: pdist of the (indexed) rows of X (n x m; X and X_indices follow on_device) into a device buffer of
 * the library, then the same loop: the matrix never leaves HBM. */
msm_idx_t msm_kmedoids_condensed_index(msm_idx_t i, msm_idx_t j, msm_idx_t n);   /* i != j; no device needed */
int msm_kmedoids(const double* dmat, msm_idx_t n, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init,
                 msm_idx_t* clusterid, double* error, msm_idx_t* ifound, int on_device);
int msm_kmedoids_fit_f32(const float* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                         msm_idx_t n_X_indices, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init,
                         msm_idx_t* clusterid, double* error, msm_idx_t* ifound, int on_device);
int msm_kmedoids_fit_f64(const double* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                         msm_idx_t n_X_indices, msm_idx_t K, msm_idx_t npass, const msm_idx_t* init,
                         msm_idx_t* clusterid, double* error, msm_idx_t* ifound, int on_device);
/* What the last successful k-medoids call of this process did: out4 = {passes run, iterations of the last pass,
 * path (1: one-workgroup, 0: general), snapshots taken in the last pass}. */
int msm_kmedoids_last_stats(msm_idx_t* out4);

/* ---- the rmsd metric: minimal RMSD after optimal superposition (libdistance's ninth metric) -------------------------
 * Conformations are float32 xyz[n_frames][n_atoms][3], C-contiguous.  msm_rmsd_prepare makes one pass over them (host or
 * device, never modified) and keeps, in device memory owned by the handle: every frame minus its centroid (centroid and
 * difference in float64, rounded once to float32) as an atom-major, frame-fastest image T[3][n_atoms][n_pad] with the
 * frames zero-padded to a multiple of 64, and G[n] = the float64 sum of squares of those rounded values.
 *
 * ONE definition of the distance of frames x, y (csrc/rmsd_dev.h: rmsd_qcp): M_ab = sum_k x_ka * y_kb as a float32 fmaf
 * chain over the atoms from atom 0; the characteristic quartic of the 4 x 4 key matrix (Theobald 2005) with float64
 * coefficients; its largest root lambda by Newton from (G_x + G_y) / 2, at most 50 steps, until |step| < 1e-11 |lambda|
 * or a zero derivative; msd = max((G_x + G_y - 2 lambda) / n_atoms, 0); the distance is sqrt(msd), float64.  Every
 * function below returns the same bits for the same ordered pair (x, y).  A frame with a NaN or infinite coordinate has
 * NaN distances.
 *
 * X_indices / pair_indices and the outputs follow on_device (all on the host or all on the device); every index is checked
 * against the frame count (MSM_ERR_INVALID).  Different atom counts: MSM_ERR_INVALID.  All calls synchronise.
 *   msm_rmsd_dist            out[i] = d(X[X_indices[i]] or X[i], Y[y_frame])
 *   msm_rmsd_cdist           out[i][j] = d(XA[i], XB[j]), row-major
 *   msm_rmsd_pdist           condensed d(X[ix[i]], X[ix[j]]), i < j, at msm_kmedoids_condensed_index(i, j, n)
 *   msm_rmsd_sumdist         *sum = sum_p d(X[pairs[p][0]], X[pairs[p][1]]), added in a fixed order
 *   msm_rmsd_assign_nearest  assignments[i] = the first j of strictly smallest d(X[i], Y[j]) below FLT_MAX (0 if none: a NaN
 *                            never wins), min_dist[i] (optional) that distance or FLT_MAX; *inertia = their sum in a fixed
 *                            order (no atomics: the same bits every run)
 *   msm_rmsd_kcenters_fit    kcenters.py:79-102 with every pass queued on the device: distances start at +inf, centre k
 *                            updates rows of strictly smaller distance, the next centre is the first maximum of distances;
 *                            ids (host, K), labels / distances (n, follow on_device), *inertia = ordered sum of distances */
typedef struct msm_rmsd msm_rmsd_t;
int msm_rmsd_prepare(msm_rmsd_t** h, const float* xyz, msm_idx_t n_frames, msm_idx_t n_atoms, int on_device);
int msm_rmsd_destroy(msm_rmsd_t* h);
int msm_rmsd_shape(const msm_rmsd_t* h, msm_idx_t* n_frames, msm_idx_t* n_atoms, msm_idx_t* n_pad);
int msm_rmsd_dist(const msm_rmsd_t* X, const msm_rmsd_t* Y, msm_idx_t y_frame, const msm_idx_t* X_indices,
                  msm_idx_t n_X_indices, double* out, int on_device);
int msm_rmsd_cdist(const msm_rmsd_t* XA, const msm_rmsd_t* XB, double* out, int on_device);
int msm_rmsd_pdist(const msm_rmsd_t* X, const msm_idx_t* X_indices, msm_idx_t n_X_indices, double* out, int on_device);
int msm_rmsd_sumdist(const msm_rmsd_t* X, const msm_idx_t* pair_indices, msm_idx_t n_pairs, double* sum, int on_device);
int msm_rmsd_assign_nearest(const msm_rmsd_t* X, const msm_rmsd_t* Y, const msm_idx_t* X_indices, msm_idx_t n_X_indices,
                            msm_idx_t* assignments, double* min_dist, double* inertia, int on_device);
int msm_rmsd_kcenters_fit(const msm_rmsd_t* X, msm_idx_t K, msm_idx_t seed, msm_idx_t* ids, msm_idx_t* labels,
                          double* distances, double* inertia, int on_device);

/* Landmark agglomerative clustering (cluster/agglomerative.py).
 *
 * msm_linkage: agglomerative linkage of n observations from their condensed float64 distance matrix (entry (i, j), i < j,
 * at n*i - i(i+1)/2 + j - 1 - i; follows on_device), method "single" | "complete" | "average" | "ward".  Plain
 * global-minimum agglomeration on a square float64 working copy in device memory (8 n^2 bytes, released on return):
 * each of the n - 1 steps merges the active pair of lowest distance -- at a tie the lowest row slot, then the lowest
 * column slot, i < j --, the merged cluster keeps slot j, and every other active slot k gets, in float64 with sizes
 * converted to double and every product and sum evaluated left to right as written (a = D[i,k], b = D[j,k]),
 *   single    min(a, b)                  complete   max(a, b)              average   (ni*a + nj*b)/(ni + nj)
 *   ward      t = 1.0/(ni + nj + nk);  sqrt((ni + nk)*t*a*a + (nj + nk)*t*b*b - nk*t*dij*dij).
 * A step is three launches (select, update, refresh of the cached nearest neighbours); all steps are queued and the host
 * synchronises once, to read Z.
 *   Z (host, (n - 1) x 4 doubles, out): scipy's convention -- row s = (id_a < id_b, height, size of the new cluster),
 *   observations are 0 .. n-1, the cluster made at step s is n + s, rows in merge order.
 * MSM_ERR_INVALID: n < 2, an unknown or null method, a null pointer; MSM_ERR_NONFINITE: a NaN or infinite entry of dmat,
 * or a merged distance that is not finite (overflow; ward's square root of a negative number for distances that are not
 * Euclidean); MSM_ERR_HIP: the working copy could not be allocated.  On an error nothing is written.
 * msm_linkage_fit_*: pdist of the (indexed) rows of X (n x m; X and X_indices follow on_device) into a device buffer of
 * the library, then the same loop; MSM_ERR_METRIC for a null / unknown metric.  The matrix is kept for
 * msm_landmark_within(dmat = NULL) until the next msm_linkage_fit_*; one above 64 MiB is released by that call.
 * msm_linkage_plan: out2 = {threads per workgroup, rows one workgroup of the refresh launch covers}. */
int msm_linkage(const double* dmat, msm_idx_t n, const char* method, double* Z, int on_device);
int msm_linkage_fit_f32(const float* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                        msm_idx_t n_X_indices, const char* method, double* Z, int on_device);
int msm_linkage_fit_f64(const double* X, msm_idx_t n, msm_idx_t m, const char* metric, const msm_idx_t* X_indices,
                        msm_idx_t n_X_indices, const char* method, double* Z, int on_device);
int msm_linkage_plan(msm_idx_t* out2);
/* out[c] (host, K doubles) = sum of d(i, j)^2 over the pairs i < j with labels[i] == labels[j] == c
 * (agglomerative.py:191-196).  Summation order, fixed: for row i, thread t of 256 adds its columns i+1+t, i+1+t+256, ...
 * in ascending order and the 256 partial sums are added in a binary tree; a cluster's row sums are added the same way.
 * No floating-point atomics: two runs give the same bits.
 *   dmat: condensed, n(n-1)/2 doubles, follows on_device; NULL = the matrix of the last msm_linkage_fit_* (MSM_ERR_STATE
 *   when there is none of n elements).  labels (host, n): values in [0, K) (MSM_ERR_INVALID otherwise). */
int msm_landmark_within(const double* dmat, msm_idx_t n, const msm_idx_t* labels, msm_idx_t K, double* out, int on_device);
/* Pooled landmark predict (agglomerative.py:248-273), one fused kernel: the n x L distance matrix is never formed.
 *   X (n x m, follows on_device); landmarks (host, L x m, X's element type), permuted so that cluster c's landmarks are
 *   rows offsets[c] .. offsets[c+1]-1 (offsets: host, K + 1, from 0 to L, not decreasing; a cluster may be empty);
 *   intra (host, K; needed for "ward"): msm_landmark_within's sums; pooling "single" | "complete" | "average" | "ward".
 * Every distance is msm_cdist_*'s bit for bit.  A cluster's pooled value: single = min, complete = max (both keep a NaN
 * once met, like numpy's), average = sum / cnt, ward = (cnt * sum of d*d - intra[c]) / (cnt*(cnt+1)/2), where the two
 * sums start at 0.0 and add ONE TERM PER LANDMARK IN ASCENDING (permuted) LANDMARK INDEX.  The label is a running strict
 * < over the clusters in ascending id from (+inf, 0); clusters without a landmark are skipped, a NaN value never wins, a
 * row whose values are all NaN or +inf gets label 0.
 *   labels (n, int64) and pooled (n doubles, nullable: the winning value) follow on_device; *negative (host) = 1 when
 *   some ward value was negative.
 * MSM_ERR_INVALID: unknown pooling ("linkage ... is not supported"), bad shapes or offsets; MSM_ERR_METRIC.
 * msm_landmark_predict_plan: out4 = {rows per workgroup, landmarks per LDS tile, features per chunk (m: whole landmarks),
 * 1 when the rows are held in registers} for rows of m elements of elem_size (4 | 8) bytes. */
int msm_landmark_predict_f32(const float* X, msm_idx_t n, msm_idx_t m, const float* landmarks, msm_idx_t L,
                             const msm_idx_t* offsets, msm_idx_t K, const double* intra, const char* metric,
                             const char* pooling, msm_idx_t* labels, double* pooled, int* negative, int on_device);
int msm_landmark_predict_f64(const double* X, msm_idx_t n, msm_idx_t m, const double* landmarks, msm_idx_t L,
                             const msm_idx_t* offsets, msm_idx_t K, const double* intra, const char* metric,
                             const char* pooling, msm_idx_t* labels, double* pooled, int* negative, int on_device);
int msm_landmark_predict_plan(msm_idx_t m, int elem_size, msm_idx_t* out4);
/* The same pooling over a distance matrix: D is n x L float64 at row stride ld >= L elements (follows on_device, like
 * labels and pooled), its columns the landmarks permuted by cluster as above; offsets and intra are host arrays.  The
 * pooling code is the one msm_landmark_predict_* runs: fed that metric's float64 cdist it returns the same labels and
 * pooled values.  A host matrix travels in blocks of rows through the scratch described below.
 *
 * The three symmetric divergences ("js_metric", "js_divergence", "sym_kl_divergence", see msm_divergence_*) are accepted
 * as `metric` by msm_linkage_fit_* (their condensed pdist takes the vector metric's place) and by
 * msm_landmark_predict_* (the divergence cdist of a block of rows against the landmarks is written to a scratch buffer
 * of the library and pooled by the matrix kernel, block after block).  The scratch holds at most 64 MiB, or 256 rows x L
 * doubles where that is larger.  "kl_divergence" is refused with MSM_ERR_METRIC: it is not symmetric. */
int msm_landmark_predict_dmat(const double* D, msm_idx_t n, msm_idx_t L, msm_idx_t ld, const msm_idx_t* offsets, msm_idx_t K,
                              const double* intra, const char* pooling, msm_idx_t* labels, double* pooled, int* negative,
                              int on_device);
/* Every row against every row, from the condensed matrix of the n rows themselves (n >= 2; follows on_device, like labels
 * and pooled): blocks of rows of its square form -- the columns in the order perm (host, n entries in [0, n): the rows
 * permuted by cluster), the diagonal exactly 0 -- are expanded into the same scratch and pooled.  For a symmetric distance
 * with d(i, i) = 0 this is msm_landmark_predict_* of the rows against themselves, bit for bit, without computing a
 * distance twice. */
int msm_landmark_predict_condensed(const double* dmat, msm_idx_t n, const msm_idx_t* perm, const msm_idx_t* offsets, msm_idx_t K,
                                   const double* intra, const char* pooling, msm_idx_t* labels, double* pooled, int* negative,
                                   int on_device);

/* ---- KL-family divergences between non-negative rows (utils/divergence.py) ----------------------------------------------
 * kind: "kl_divergence" | "sym_kl_divergence" | "js_divergence" | "js_metric".  In float64 (float32 rows are widened
 * exactly; the output is always float64), the reference's manual loop:
 *     kl(P, Q)  = max(sum_k [P_k * Q_k != 0] P_k * log(P_k / Q_k), 0)     ascending k; a NaN sum stays NaN
 *     sym_kl    = kl(P, Q) + kl(Q, P)
 *     js        = 0.5 * kl(P, M) + 0.5 * kl(Q, M),  M_k = (P_k + Q_k) / 2
 *     js_metric = sqrt(js)
 * A term is skipped where the float64 product is zero (an underflowing product included): q = 0 under p > 0 adds nothing.
 * Each pair's sum is built by one thread in ascending k; no atomics.  cdist, pdist and rows give the same bits for the
 * same pair of rows, d(i, j) == d(j, i) bit for bit for the three symmetric kinds, and d(i, i) == 0.
 *   msm_divergence_cdist_*: out[i * nB + j] = div(XA[i], XB[j]); XA, XB and out follow on_device.
 *   msm_divergence_pdist_*: condensed (i < j, scipy's order) over the rows of X or the rows X_indices names (may repeat a
 *     row; host indices are range-checked); X, X_indices and out follow on_device.
 *   msm_divergence_rows_*: out[r] = div(P[r], Q[r]) for n pairs of HOST rows.
 *   msm_divergence_plan: out4 = {tile rows, tile columns, columns per LDS chunk, threads per workgroup}.
 *   msm_divergence_log_probe: out[i] = log(x[i]) on the device for reps == 1, a sum of reps logs of slowly growing
 *     arguments otherwise (HOST arrays); *ms (nullable) = the kernel's time.  For the accuracy and throughput probe.
 * MSM_ERR_METRIC: unknown or null kind; MSM_ERR_INVALID: null pointers, m < 1, negative sizes. */
int msm_divergence_cdist_f32(const float* XA, msm_idx_t nA, const float* XB, msm_idx_t nB, msm_idx_t m, const char* kind,
                             double* out, int on_device);
int msm_divergence_cdist_f64(const double* XA, msm_idx_t nA, const double* XB, msm_idx_t nB, msm_idx_t m, const char* kind,
                             double* out, int on_device);
int msm_divergence_pdist_f32(const float* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t n_idx,
                             const char* kind, double* out, int on_device);
int msm_divergence_pdist_f64(const double* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* X_indices, msm_idx_t n_idx,
                             const char* kind, double* out, int on_device);
int msm_divergence_rows_f32(const float* P, const float* Q, msm_idx_t n, msm_idx_t m, const char* kind, double* out);
int msm_divergence_rows_f64(const double* P, const double* Q, msm_idx_t n, msm_idx_t m, const char* kind, double* out);
int msm_divergence_plan(msm_idx_t* out4);
int msm_divergence_log_probe(const double* x, msm_idx_t n, int reps, double* out, float* ms);

/* ---- BACE lumping (lumping/bace.py): Bayes factors between the rows of a count matrix and the merge loop ---------------
 * counts: n x n float64, row-major, non-negative and finite; w: n weights (positive and finite for every kept state);
 * the flags are int32, one per state.  w and the flags are HOST arrays; counts (and out, d_out) follow on_device.  Over the
 * columns k of the kept states, ascending, in float64:
 *     c1_k = counts[i, k] + (unmerged[i] && unmerged[k] ? 1 / n : 0),  p1_k = c1_k / w[i]      (likewise c2, p2 for j)
 *     cp_k = (c1_k + c2_k) / (w[i] + w[j]),   d = sum_k c1_k log(p1_k / cp_k) + sum_k c2_k log(p2_k / cp_k)
 * and the value stored for the pair is float32(1 / float32(d)), both correctly rounded.  One thread adds a pair's terms in
 * ascending k, in the tile kernel and in the row kernel alike: a pair has the same bits from both, and (i, j) == (j, i).
 *   msm_bace_pairs: row < 0: out[i, j] for i < j, both kept, counts[i, j] > 1 (the tile kernel); row >= 0: out[row, j] for
 *     every kept j != row with counts[row, j] > 1 (the row kernel).  Every other entry of out (n x n float32) is 0.  d_out
 *     (nullable, n x n float64) receives d itself at the same places.
 *   msm_bace_fit: keep marks the states that take part (all unmerged).  Computes the matrix, then merges
 *     max(kept - n_macrostates, 0) times: the first maximum of the matrix in row-major order (an inf counts) names (x, y); y
 *     is merged into x as the reference's _mergeTwoClosestStates does it; row x is evaluated again.  The loop is queued on
 *     the stream and nothing is read back until it ends.  merges[2 s], merges[2 s + 1], values[s] are the selection after s
 *     merges, the look-ahead after the last merge included: *n_records = merges + 1 <= capacity.  A selection that finds no
 *     positive entry is recorded as (-1, -1, 0) and ends the loop (so are all later ones).  ms3 (nullable): the times of the
 *     initial matrix, of the loop and of both in milliseconds.  The caller's counts are not changed.
 *   msm_bace_plan: out6 = {tile rows = tile columns, columns per LDS chunk of the tile kernel, pairs per workgroup and
 *     columns per pass of the row kernel, threads per workgroup, the largest n}.
 * The environment variable MSM_BACE_MAX_GRID (read at every call) caps the workgroups of the grid-stride kernels; it is
 * there for the tests and changes no result.
 * MSM_ERR_INVALID: null pointers, n < 2, n > 16384, n_macrostates < 1, no kept state, a bad weight, row not kept, capacity too small;
 * MSM_ERR_NONFINITE: a negative or non-finite count. */
int msm_bace_pairs(const double* counts, const double* w, const int32_t* unmerged, const int32_t* alive, msm_idx_t n, msm_idx_t row,
                   float* out, double* d_out, int on_device);
int msm_bace_fit(const double* counts, const double* w, const int32_t* keep, msm_idx_t n, msm_idx_t n_macrostates, int32_t* merges,
                 float* values, msm_idx_t capacity, msm_idx_t* n_records, float* ms3, int on_device);
int msm_bace_plan(msm_idx_t* out6);

/* ---- PCCA+ objectives (lumping/pcca_plus.py) on a transition matrix that stays on the device ------------------------------
 * A handle keeps T (n x n, row-major), pi (n) and V (n x m, row-major: the first m right eigenvectors, column 0 used as
 * given) on the device; everything is float64.  2 <= m <= 64, m <= n <= 16384.
 *   msm_pcca_create: T, pi and V follow on_device.  Also computes G = V^T diag(pi) T V (m x m) and w = V^T pi with one read
 *     of T from memory: for chi = V A, chi_i^T diag(pi) T chi_i = (A^T G A)_ii and chi_i^T pi = (A^T w)_i.
 *   msm_pcca_moments: G and w to host arrays.
 *   msm_pcca_chi: fill_A of the reference applied to A_in (host, m x m; only A_in[1:, 1:] is read), on the device:
 *       A[k, 0] = -sum_c A[k, c] (c >= 1);  A[0, c] = -min over the states of (V[:, 1:] A[1:])[., c];  A /= sum_c A[0, c];
 *     then chi = V A (n x m) and mapping = the first maximum of each row of chi, a row with a NaN mapping to its first NaN
 *     (numpy.argmax).  A_out, chi_out (nullable) and mapping_out (int32) are host arrays.
 *   msm_pcca_objective: alpha (host) = the (m-1)^2 entries of A[1:, 1:], row-major; kind 0 crispness, 1 metastability,
 *     2 crisp_metastability.  A, chi and the mapping as above.  *value = -inf where some macrostate receives no state or where
 *     |(1 - sum A[0, 1:]) - (-min_s V[s, 1:] . A[1:, 0])| > 1e-8 (a NaN there fails); otherwise
 *       crispness = sum_i (A^T A)_ii / A[0, i];   metastability = sum_i (A^T G A)_ii / (A^T w)_i;
 *       crisp_metastability = sum_i num_i / den_i,  num_i = sum_{a in i} pi_a sum_{b in i} T[a, b],  den_i = sum_{a in i} pi_a.
 *     The value is the objective itself (a minimiser negates it).  info (int32 x 4) = {feasible, macrostates used, mapping
 *     equal to the previous evaluation's, passes over T made by this call}.  One upload, a queue of kernels with no host
 *     synchronisation in between, one read-back.  The handle remembers the last mapping and its block sums: an equal mapping
 *     gets its kind-2 value from them without a pass over T.  MSM_PCCA_REUSE=0 (read at every call) forces the pass; the bits
 *     are the same.
 *   msm_pcca_crisp: num and den (host, m each) of any mapping (host int32, values in [0, m)): the row kernel alone.
 *   msm_pcca_plan: out5 = {rows of T per workgroup, columns per pass of a wave, threads per workgroup, largest n, largest m}.
 * Orders of the m-term formulas, every product and sum rounded on its own: (A^T A)_ii adds A[k, i]^2 in ascending k;
 * (A^T G A)_ii adds A[j, i] * (sum_k G[j, k] A[k, i], ascending k) in ascending j, (A^T w)_i adds A[j, i] w[j] in ascending j;
 * the quotients are added in ascending i.
 * No floating-point atomics: every sum is taken in an order fixed by n and m (pcca_dev.h), so results are the same bits from
 * run to run, for host and device inputs, and under MSM_PCCA_MAX_GRID (read at every call), which caps the workgroups of the
 * grid-stride kernels for the tests.
 * MSM_ERR_INVALID: null pointers, m or n out of range (before any device work), a mapping value out of range, a bad kind. */
typedef struct msm_pcca msm_pcca_t;
int msm_pcca_create(const double* T, const double* pi, const double* V, msm_idx_t n, msm_idx_t m, int on_device, msm_pcca_t** handle);
int msm_pcca_destroy(msm_pcca_t* handle);
int msm_pcca_moments(msm_pcca_t* handle, double* G, double* w);
int msm_pcca_chi(msm_pcca_t* handle, const double* A_in, double* A_out, double* chi_out, int32_t* mapping_out);
int msm_pcca_objective(msm_pcca_t* handle, int kind, const double* alpha, double* value, int32_t* info);
int msm_pcca_crisp(msm_pcca_t* handle, const int32_t* mapping, double* num, double* den);
int msm_pcca_plan(msm_idx_t* out5);

/* ---- Nystroem kernel feature map (decomposition/kernel_approximation.py, ktica.py) ------------------------------------
 * out[i, :] = k(rows[i], landmarks) . B - c     (rows: n x n_features at row stride ld elements; landmarks: L x
 * n_features of the rows' dtype; B: L x P float64; c: P float64 or NULL; landmarks, B and c are HOST arrays).
 *   kernel: enum msm_kernel below.  gamma arrives resolved (the estimators turn None into 1 / n_features); coef0 and degree
 *   are read by poly and sigmoid only.  cosine divides by the norms the way scikit-learn's normalize does (a zero vector is
 *   left as it is: its kernel values are 0).
 *   out (n x P) has the rows' dtype, or float64 when out_f64 is set; rows and out follow on_device (host rows are staged in
 *   groups; pitched host rows are compacted by the copy).  The call runs on the stream of msm_set_stream and synchronises it.
 *   Arithmetic: float64 for both row dtypes (float32 rows are widened exactly); the result is rounded once.
 *   Routes: while 16 rows x L kernel values fit the LDS budget one fused launch keeps them in LDS; above, two launches per
 *   chunk of scratch_rows rows (0: the plan's default) go through a library-owned buffer.  MSM_NYSTROEM_FUSED=0 forces the
 *   second route; both accumulate every output element in the same order and are bit-identical.
 * MSM_ERR_NONFINITE ("Input contains NaN, infinity or a value too large") when a row or landmark value is not finite;
 * MSM_ERR_INVALID for an unknown kernel id, null pointers and bad shapes.  n = 0 succeeds without a device.
 * msm_kernel_map_plan: out9 = {1 fused / 0 scratch, rows per workgroup R, landmark tile, feature depth per MFMA, tile of B's
 *   columns, L padded to the tile, pitch of the block in doubles, LDS bytes of the block, default rows per scratch chunk}. */
enum msm_kernel { MSM_K_LINEAR = 0, MSM_K_POLY = 1, MSM_K_SIGMOID = 2, MSM_K_COSINE = 3, MSM_K_RBF = 4, MSM_K_LAPLACIAN = 5 };
int msm_kernel_map_f32(const float* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const float* landmarks, msm_idx_t L,
                       const double* B, msm_idx_t P, const double* c, int kernel, double gamma, double coef0, double degree,
                       void* out, int out_f64, int on_device, msm_idx_t scratch_rows);
int msm_kernel_map_f64(const double* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const double* landmarks, msm_idx_t L,
                       const double* B, msm_idx_t P, const double* c, int kernel, double gamma, double coef0, double degree,
                       void* out, int out_f64, int on_device, msm_idx_t scratch_rows);
int msm_kernel_map_plan(msm_idx_t L, msm_idx_t P, msm_idx_t n_features, int itemsize, msm_idx_t* out9);

/* ---- Gaussian hidden Markov model: the E-step (hmm/gaussian.py) ----------------------------------------------------------
 * rows: n x n_features at row stride ld elements, the trajectories back to back; offsets: n_traj + 1 HOST row offsets
 * (offsets[0] = 0, offsets[n_traj] = n, no empty trajectory).  means, vars: n_states x n_features; transmat: n_states x
 * n_states (clamped at 1e-20 as HMMFitter::set_transmat does); log_startprob: n_states, ADDED to the first frame's log
 * likelihoods as HMMFitter does with its log_startprob (the reference's estimator hands it 1 / n_states, not the logarithm;
 * the estimator here does the same).  All parameters and all outputs but loglik's are HOST float64 arrays; rows follow
 * on_device (host rows are staged, pitched ones compacted by the copy).  Arithmetic: float64 for both row dtypes.  The
 * emission term is -0.5 (F c + sum_f (x - mu)^2 / var + log var) with c = log(2 pi) rounded to float as the reference has it.
 *   msm_hmm_estep:   traj_logprob (n_traj), post (K), obs and obs2 (K x F), trans (K x K) and *logprob, the sum of
 *                    traj_logprob in trajectory order.  Forward-backward runs parallel in time over segments of `segment`
 *                    frames (0: the plan's default; at most the plan's S_max): operators per segment, a stitch per
 *                    trajectory, a fused pass per segment, an ordered reduction of at most 1024 partials.  Neither emissions
 *                    nor lattices nor posteriors reach device memory; no atomics: the same call gives the same bits.  A state
 *                    whose emission weight in a frame is below the smallest normal double relative to the frame's largest is
 *                    dropped from that frame.
 *   msm_hmm_score:   the forward half (operators and stitch): the same traj_logprob and *logprob, bit for bit, for the same
 *                    segment.  It keeps nothing per frame, so any segment is served: one as long as the longest trajectory
 *                    is the forward recursion serial in time, one workgroup per trajectory.
 *   msm_hmm_loglik:  out (n x n_states float64, follows on_device) = the emission log-likelihoods.
 *   msm_hmm_viterbi: the reference's log-space recursion, one wave per trajectory, sequential in time, first maximum in the
 *                    induction, at the last frame and in the traceback; states (n, HOST int), traj_logprob (n_traj), *logprob.
 *                    One back-pointer byte per (frame, state) in a library-owned buffer.
 *   msm_hmm_plan:    out8 = {default segment S, S_max (the longest whose alpha block fits LDS), largest n_states served,
 *                    threads of a workgroup (one owns ceil(K^2 / threads) matrix entries), frames of an emission chunk in the
 *                    operator pass, partials of the fused pass at most, frames of a Viterbi chunk, LDS bytes of the fused pass
 *                    at the default S}.
 * MSM_ERR_INVALID: n_states above the served limit (the message names it), non-positive or non-finite variances, n = 0 or
 * no / an empty trajectory ("sequences is empty"), segment above S_max, null pointers, bad shapes.  MSM_ERR_NONFINITE
 * ("Input contains NaN, infinity or a value too large") when a row element is not finite. */
#define MSM_HMM_DECL(SFX, T)                                                                                                       \
    int msm_hmm_estep_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const msm_idx_t* offsets,               \
                            msm_idx_t n_traj, msm_idx_t n_states, const double* means, const double* vars, const double* transmat, \
                            const double* log_startprob, msm_idx_t segment, double* traj_logprob, double* post, double* obs,       \
                            double* obs2, double* trans, double* logprob, int on_device);                                          \
    int msm_hmm_score_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const msm_idx_t* offsets,               \
                            msm_idx_t n_traj, msm_idx_t n_states, const double* means, const double* vars, const double* transmat, \
                            const double* log_startprob, msm_idx_t segment, double* traj_logprob, double* logprob, int on_device); \
    int msm_hmm_loglik_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, msm_idx_t n_states,                   \
                             const double* means, const double* vars, double* out, int on_device);                                 \
    int msm_hmm_viterbi_##SFX(const T* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, const msm_idx_t* offsets,             \
                              msm_idx_t n_traj, msm_idx_t n_states, const double* means, const double* vars,                      \
                              const double* transmat, const double* log_startprob, int* states, double* traj_logprob,             \
                              double* logprob, int on_device);
MSM_HMM_DECL(f32, float)
MSM_HMM_DECL(f64, double)
#undef MSM_HMM_DECL
int msm_hmm_plan(msm_idx_t n_states, msm_idx_t n_features, int itemsize, msm_idx_t* out8);

/* ---- von Mises hidden Markov model: the image of the angles and the linear E-step (hmm/vonmises.py) ---------------------
 * The von Mises log-emission sum_f kappa cos(x - mu) - sum_f (log 2 pi + log I0(kappa)) is LINEAR in the image
 * Z = [cos X | sin X] (n x D, D = 2 n_features):  l_t(k) = cst[k] + sum_j Z[t, j] w[k, j]  with
 * w = [kappa cos mu | kappa sin mu] (n_states x D) and cst[k] = -sum_f (log 2 pi + log I0(kappa_kf)), both formed by the
 * caller.  The angles never change over a fit, so the image is formed once and every E-step reads it.
 *   msm_hmm_trig:       rows (n x n_features at stride ld, host or device by on_device; host rows are staged, pitched ones
 *                       compacted by the copy) -> Z (DEVICE float64, n rows at stride ldz >= 2 n_features):
 *                       Z[t, f] = cos(x_tf), Z[t, n_features + f] = sin(x_tf); the element is widened exactly and the
 *                       trigonometry is float64 for both row types.  16 n_features bytes per frame.  A non-finite angle
 *                       gives NaN in Z and is reported by whichever msm_hmm_lin_* call reads it.
 *   msm_hmm_lin_estep, msm_hmm_lin_score, msm_hmm_lin_loglik, msm_hmm_lin_viterbi: what the Gaussian entries of the same
 *                       names do, with the linear emission over Z (DEVICE memory, always; ldz >= D): the same passes,
 *                       segments, orders of summation and bit-stability, the same offsets / transmat / log_startprob
 *                       conventions and msm_hmm_plan (S_max depends on n_states only).  obs is n_states x D = gamma^T Z:
 *                       its left half is the reference's cosobs, its right half sinobs; there is no obs2.  loglik's out is
 *                       DEVICE memory, n x n_states.
 * The same status codes, refusals and messages as the Gaussian entries; w and cst must be finite.  MSM_ERR_NONFINITE
 * ("Input contains NaN, infinity or a value too large") when an element of Z is not finite. */
int msm_hmm_trig_f32(const float* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, double* Z, msm_idx_t ldz, int on_device);
int msm_hmm_trig_f64(const double* rows, msm_idx_t n, msm_idx_t n_features, msm_idx_t ld, double* Z, msm_idx_t ldz, int on_device);
int msm_hmm_lin_estep(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets, msm_idx_t n_traj,
                      msm_idx_t n_states, const double* w, const double* cst, const double* transmat, const double* log_startprob,
                      msm_idx_t segment, double* traj_logprob, double* post, double* obs, double* trans, double* logprob);
int msm_hmm_lin_score(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets, msm_idx_t n_traj,
                      msm_idx_t n_states, const double* w, const double* cst, const double* transmat, const double* log_startprob,
                      msm_idx_t segment, double* traj_logprob, double* logprob);
int msm_hmm_lin_loglik(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, msm_idx_t n_states, const double* w,
                       const double* cst, double* out);
int msm_hmm_lin_viterbi(const double* Z, msm_idx_t n, msm_idx_t D, msm_idx_t ldz, const msm_idx_t* offsets, msm_idx_t n_traj,
                        msm_idx_t n_states, const double* w, const double* cst, const double* transmat, const double* log_startprob,
                        int* states, double* traj_logprob, double* logprob);

/* ---- k-means labelling / mini-batch step (GEMM form on MFMA) ----
 * Element type: scikit-learn (the arithmetic behind msmbuilder.cluster.MiniBatchKMeans, cluster/__init__.py:67-69) works
 * in the type of X -- float32 rows give float32 centres / counts, everything else is float64 -- and the reference
 * pipeline feeds it the float64 output of tICA.transform (decomposition/tica.py:329-352).  Both types are built:
 * `_f32` entry points on v_mfma_f32_32x32x2_f32, `_f64` entry points on v_mfma_f64_16x16x4_f64 (round 6). */
/* labels[i] = argmin_j ||X[i]-C[j]||^2 computed as ||c||^2 - 2 x.c (+||x||^2 for the
 * inertia), in the rows' own type like scikit-learn's _labels_inertia; centers host [K, m].
 * labels int32 (sklearn's dtype) follow on_device; *inertia fp64 sum of per-row terms. */
int msm_kmeans_label_f32(const float* X, msm_idx_t n, msm_idx_t m, const float* centers,
                         msm_idx_t K, int32_t* labels, double* inertia, int on_device);
int msm_kmeans_label_f64(const double* X, msm_idx_t n, msm_idx_t m, const double* centers,
                         msm_idx_t K, int32_t* labels, double* inertia, int on_device);
/* What a labelling call of this shape launches -- the library's one dispatch, for tests to ask (pure: works with no device
 * visible).  handle_entry: msm_mbk_label / _step / _run* (else the stateless msm_kmeans_label_* / msm_mbk_step_*); aligned:
 * rows and centres start on 16-byte boundaries; gathered: rows are read through an index list.  MSM_LABEL_XCD is read per
 * call.  Out: *kernel (MSM_KM_*), *nsplit centre splits (1: none) of *span centres each. */
enum { MSM_KM_SCALAR = 0, MSM_KM_V4 = 1, MSM_KM_V4_XCD = 2, MSM_KM_LABEL64 = 3, MSM_KM_SMALL = 4, MSM_KM_F64 = 5 };
int msm_kmeans_label_plan(msm_idx_t n, msm_idx_t m, msm_idx_t K, int f64, int handle_entry, int want_inertia, int aligned,
                          int gathered, int* kernel, int* nsplit, msm_idx_t* span);
/* k-means++ seeds (scikit-learn `_kmeans_plusplus`, sklearn/cluster/_kmeans.py:163-259; reached from
 * msmbuilder/cluster/__init__.py:67-69) of the n x F rows X (host or device per on_device): centre 0 = row
 * `first`, then K - 1 rounds of L candidates drawn by inverse-CDF sampling of the current squared distances with the
 * uniforms u[(K - 1) * L] (host float64 in [0, 1): the caller's RandomState stream), the candidate of lowest potential
 * wins.  float32 rows: distances in scikit-learn's float64-upcast arithmetic rounded to float32; float64 rows: float64
 * throughout.  centers[K * F] (the rows' type) and ids[K] (rows of X): host. */
int msm_kmeans_plusplus_f32(const float* X, msm_idx_t n, msm_idx_t F, msm_idx_t K, msm_idx_t first, const double* u, int L,
                            float* centers, msm_idx_t* ids, int on_device);
int msm_kmeans_plusplus_f64(const double* X, msm_idx_t n, msm_idx_t F, msm_idx_t K, msm_idx_t first, const double* u, int L,
                            double* centers, msm_idx_t* ids, int on_device);
/* One MiniBatchKMeans step on the rows X[batch_idx[b]] (batch_idx host int64, length B):
 * label, then per-centre streaming mean c <- (c*w + sum x)/(w + n) with cumulative
 * counts (sklearn _k_means_minibatch.pyx:59-109, unit sample weights).  centers
 * [K, m] and counts [K] are host, updated in place; sums/counts partials are
 * exported for the multi-GPU all-reduce when apply_update == 0:
 *   batch_sums [K, m] float64, batch_counts [K] float64 (host, nullable). */
int msm_mbk_step_f32(const float* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* batch_idx,
                     msm_idx_t B, float* centers, float* counts, msm_idx_t K,
                     double* batch_inertia, double* batch_sums, double* batch_counts,
                     int apply_update, int on_device);
int msm_mbk_step_f64(const double* X, msm_idx_t n, msm_idx_t m, const msm_idx_t* batch_idx,
                     msm_idx_t B, double* centers, double* counts, msm_idx_t K,
                     double* batch_inertia, double* batch_sums, double* batch_counts,
                     int apply_update, int on_device);

/* Device-resident MiniBatchKMeans state (centres [K, m], cumulative counts [K] and ||c||^2 stay in
 * HBM for the whole fit).  A step ships the batch indices in and [inertia | counts] out.
 * The handle has an element type: msm_mbk_create -> float32, msm_mbk_create_f64 -> float64 (msm_mbk_is_f64 tells); every
 * `void*` below (X, centers, counts, counts_out) is an array of THAT type.
 *   msm_mbk_step(apply_update = 1): label the batch rows X[batch_idx[b]], streaming-mean update,
 *       *batch_inertia (before the update) and counts_out (host, K; nullable) after it.
 *   apply_update = 0 (multi-GPU): label + fp64 batch sums only; msm_mbk_export_packed() hands out
 *       [K*m sums | K counts | inertia] doubles for the RCCL all-reduce, msm_mbk_apply_packed()
 *       applies the reduced buffer identically on every rank.
 *   msm_mbk_reassign: centres[which[i]] = X[rows[i]], counts[which[i]] = new_count
 *       (scikit-learn's starved-centre reassignment, decided on the host with its RNG). */
typedef struct msm_mbk msm_mbk_t;
int msm_mbk_create(msm_mbk_t** h, msm_idx_t n_clusters, msm_idx_t n_features);
int msm_mbk_create_f64(msm_mbk_t** h, msm_idx_t n_clusters, msm_idx_t n_features);
int msm_mbk_is_f64(msm_mbk_t* h);
int msm_mbk_destroy(msm_mbk_t* h);
int msm_mbk_set(msm_mbk_t* h, const void* centers, const void* counts);
int msm_mbk_set_counts(msm_mbk_t* h, const void* counts);
int msm_mbk_get(msm_mbk_t* h, void* centers, void* counts);
int msm_mbk_step(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t B,
                 double* batch_inertia, void* counts_out, int apply_update, int on_device);
/* S consecutive plain steps (label + streaming-mean update, as msm_mbk_step with apply_update = 1) on device-resident X
 * with ONE host synchronisation: batch_idx is [S][B] (host), and sklearn's _mini_batch_convergence (_kmeans.py:1963-2027,
 * the tol == 0 / verbose == 0 branch) runs on the device after every step -- state6 = {ewa_inertia, ewa_inertia_min,
 * no_improvement, have_ewa, have_min, (out) steps executed}, alpha = min(1, 2 B / (n_samples + 1)), max_no_improvement < 0
 * = None.  Steps queued behind the one at which the criterion fires are not executed: *steps_done <= S says how many were,
 * inertias[0 .. steps_done) are their batch inertias, *converged the criterion.  first_step = index of the run's first
 * step in the fit (step 0 is excluded from the moving average, as in sklearn). */
int msm_mbk_run(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t S, msm_idx_t B,
                msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement, double* state6,
                msm_idx_t* steps_done, int* converged, double* inertias, void* counts_out);
/* msm_mbk_run in two halves: _begin queues the run and returns, _end waits and fetches (the host draws the next run's
 * indices in between); one run in flight per handle */
int msm_mbk_run_begin(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* batch_idx, msm_idx_t S, msm_idx_t B,
                      msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement, const double* state6);
int msm_mbk_run_end(msm_mbk_t* h, double* state6, msm_idx_t* steps_done, int* converged, double* inertias, void* counts_out);
/* The same for a ROW-SHARDED fit (one process per GPU, rows in consecutive blocks): the S batches are global and identical
 * on every rank; a rank passes the rows of each batch that IT owns as local row numbers -- local_idx (host) back to back,
 * offsets[S + 1] (host) delimiting the steps -- and the size B of the whole batch.  Per step: label + fp64 sums / counts /
 * inertia of the local rows, ONE all-reduce of the packed [K m | K | 1] buffer over the library communicator (RCCL on the
 * library stream, device to device), the identical update and convergence step on every rank (every rank stops at the same
 * step: the criterion sees the all-reduced inertia).  One host synchronisation per run; outputs as msm_mbk_run. */
int msm_mbk_run_sharded(msm_mbk_t* h, const void* X, msm_idx_t n_local, const msm_idx_t* local_idx, const msm_idx_t* offsets,
                        msm_idx_t S, msm_idx_t B, msm_idx_t first_step, double alpha, msm_idx_t max_no_improvement,
                        double* state6, msm_idx_t* steps_done, int* converged, double* inertias, void* counts_out);
msm_idx_t msm_mbk_packed_size(msm_mbk_t* h);
int msm_mbk_export_packed(msm_mbk_t* h, double* buf, int on_device);
int msm_mbk_apply_packed(msm_mbk_t* h, const double* buf, void* counts_out, int on_device);
/* Sharded step over the library communicator: every rank runs msm_mbk_step(apply_update = 0) on the batch rows it
 * owns (msm_mbk_zero_packed if it owns none), then msm_mbk_allreduce: ONE all-reduce of the device-resident
 * [K*m sums | K counts | inertia] (RCCL on the library stream, nothing staged through the host) and the identical
 * update on every rank.  *batch_inertia = global batch inertia, counts_out (host, K) = updated cumulative counts. */
int msm_mbk_zero_packed(msm_mbk_t* h);
int msm_mbk_allreduce(msm_mbk_t* h, double* batch_inertia, void* counts_out);
int msm_mbk_reassign(msm_mbk_t* h, const void* X, msm_idx_t n, const msm_idx_t* rows, const msm_idx_t* which,
                     msm_idx_t n_reassign, double new_count, int on_device);
int msm_mbk_label(msm_mbk_t* h, const void* X, msm_idx_t n, int32_t* labels, double* inertia, int on_device);

/* Full-batch (Lloyd) k-means, scikit-learn 1.7's _kmeans_single_lloyd on device-resident centres (float32 handle or
 * float64 handle, as msm_mbk_t).  msm_lloyd_run queues up to max_iter iterations on the n x F rows X (host or device per
 * on_device) and waits once: label (the msm_mbk_label path), then the centre update -- a stable counting sort of the row
 * numbers by label and a segmented float64 sum in a fixed order, centre = sum / count rounded once to the rows' type, so
 * that two runs give the same bits -- then the stop rules on the device: labels equal to the previous iteration's
 * (*status = MSM_LLOYD_STRICT), else sum ||c_new - c_old||^2 <= tol_abs in float64 (MSM_LLOYD_TOL), else max_iter reached
 * (MSM_LLOYD_MAXITER).  An iteration that leaves clusters empty stops the queue; the rows farthest from their own centre
 * (lowest row first among equals) are moved into the empty clusters on the device (scikit-learn's
 * _relocate_empty_clusters_dense) and the run goes on.  Unless the end was strict the rows are labelled once more against
 * the final centres.  Out: labels_out[n] (where X lives), *inertia (float64), *n_iter iterations run.
 * msm_lloyd_plan (pure, needs no device) reports what the update launches for a shape: out8 = {rows per histogram wave,
 * histogram waves, members per piece of the segmented sum, upper bound on pieces, feature tiles, features per tile,
 * 16-byte loads (0 / 1), scratch bytes}; aligned: rows and centres start on 16-byte boundaries. */
typedef struct msm_lloyd msm_lloyd_t;
enum { MSM_LLOYD_MAXITER = 0, MSM_LLOYD_STRICT = 1, MSM_LLOYD_TOL = 2 };
int msm_lloyd_create(msm_lloyd_t** h, msm_idx_t n_clusters, msm_idx_t n_features);
int msm_lloyd_create_f64(msm_lloyd_t** h, msm_idx_t n_clusters, msm_idx_t n_features);
int msm_lloyd_destroy(msm_lloyd_t* h);
int msm_lloyd_set_centers(msm_lloyd_t* h, const void* centers);
int msm_lloyd_get_centers(msm_lloyd_t* h, void* centers);
int msm_lloyd_run(msm_lloyd_t* h, const void* X, msm_idx_t n, msm_idx_t max_iter, double tol_abs, int32_t* labels_out,
                  int on_device, double* inertia, msm_idx_t* n_iter, int* status);
int msm_lloyd_plan(msm_idx_t n, msm_idx_t m, msm_idx_t K, int f64, int aligned, msm_idx_t* out8);

/* ------------------------------------------------------------------------------------------
 * Pre-tICA column scan and scaling.  Replaces the fit / transform arithmetic of
 * msmbuilder.preprocessing.{StandardScaler, MinMaxScaler, MaxAbsScaler}
 * (/root/reference/msmbuilder/preprocessing/__init__.py:56-83 -- mixins over scikit-learn's
 * scalers, base.py:14-199).
 * msm_colstats: one pass over n_seq trajectories X_ptrs[s] -> n_rows[s] x n_features (common row
 * stride ld, dtype_bytes 4 or 8; device-resident or host).  out5F[5][n_features] (host, float64) =
 * per-column {count of non-NaN values, mean, sum of squared deviations M2, min, max}; NaN is a
 * missing value (scikit-learn's convention), *has_inf != 0 if an infinity was seen.
 * msm_scale_apply: mode 0 out = (x - shift) / scale, mode 1 out = x * scale + shift, every step
 * computed in float64 and rounded to the array dtype like numpy's in-place operators; shift /
 * scale are host float64 [n_features] or NULL (step skipped); out may alias X. */
int msm_colstats(const void* const* X_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int dtype_bytes,
                 msm_idx_t n_features, msm_idx_t ld, int on_device, double* out5F, int* has_inf);
int msm_scale_apply(const void* X, int dtype_bytes, msm_idx_t n_rows, msm_idx_t n_features, msm_idx_t ld,
                    const double* shift, const double* scale, int mode, void* out, msm_idx_t ld_out,
                    int on_device);
/* One pass of the radix SELECT behind RobustScaler's per-column median / percentiles (exact order
 * statistics without a sort): DEVICE-resident trajectories only.  Values map to order-preserving keys
 * (sign-flipped IEEE bits, NaN skipped).  prefix == NULL: hist[0][f][d] = number of values of column f
 * whose key digit (key >> shift) & ((1 << bits) - 1) equals d.  prefix != NULL (host uint64
 * [n_targets][n_features]): hist[t][f][d] counts only the values whose higher bits
 * key >> (shift + bits) equal prefix[t][f].  hist is host int64 [n_targets or 1][n_features][1 << bits]. */
int msm_col_digit_hist(const void* const* X_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int dtype_bytes,
                       msm_idx_t n_features, msm_idx_t ld, const uint64_t* prefix, int n_targets, int shift, int bits,
                       int64_t* hist);

/* ------------------------------------------------------------------------------------------
 * Time-series smoothers in front of tICA (msmbuilder.preprocessing.timeseries): one linear recurrence
 * along the time axis of every column, parallel in time.  X_ptrs[s] -> n_rows[s] x n_features at row stride ld elements,
 * dtype_bytes 4 or 8, host or device by on_device (host rows are staged, pitched ones compacted by the copy); out_ptrs[s]
 * -> the same rows at stride ld_out, in the same place.  All arithmetic is float64; the recurrence is scipy's lfilter in
 * transposed direct form II, y = z[0] + b[0] x, z[k] = (z[k+1] + b[k+1] x) - a[k+1] y, every operation rounded on its own.
 *   MSM_TS_BUTTERWORTH  b, a (order + 1 each, a[0] = 1) and zi (order) are HOST float64 (scipy's butter and lfilter_zi);
 *                       order 1 .. 8; width odd, >= 3.  Per column: reflect-pad by width - 1 rows (x[w-1:0:-1], x,
 *                       x[-1:-w:-1]), then filtfilt's defaults on that signal (odd extension by 3 (order + 1), forward from
 *                       zi * ext[0], backward from zi * y[last]), both paddings cropped; out has the input's dtype, rounded
 *                       once.  A column holding a non-finite element comes out all NaN.  alpha, adjust, min_periods unused.
 *   MSM_TS_EWMA         DataFrame.ewm(alpha=alpha, adjust=adjust, min_periods=min_periods).mean() for finite rows: adjust:
 *                       sum_i (1-alpha)^i x_{t-i} / sum_i (1-alpha)^i; otherwise y_0 = x_0, y_t = (1-alpha) y_{t-1} +
 *                       alpha x_t; rows below min_periods - 1 are NaN.  out is float64 whatever dtype_bytes.  order, b, a,
 *                       zi, width unused.
 *   MSM_TS_DOUBLE_EWMA  (fwd + bwd) / 2 with bwd the EWMA of the time-reversed rows, not reversed back.
 * segment: frames of a pass (paddings included) per segment of the time-parallel form -- a local pass per (trajectory,
 * segment, column) from zi * x[segment start], a stitch per (trajectory, column) with A^segment (formed in long double),
 * a final pass --; 0, or at least the longest trajectory: one segment per trajectory, the recurrence serial in time.  The
 * same call gives the same bits; results for different `segment` differ by the reassociation at the seams.
 * MSM_ERR_INVALID: null pointers, bad shapes, dtype_bytes, kind, order, width, coefficients, alpha outside (0, 1], a
 * negative segment, a Butterworth trajectory shorter than width or whose padded length is not above 3 (order + 1).
 * MSM_ERR_NONFINITE ("Input contains NaN, infinity or a value too large"): EWMA kinds, a non-finite element (a flag raised
 * by the final pass, no pass of its own; out is then unspecified). */
#define MSM_TS_BUTTERWORTH 0
#define MSM_TS_EWMA 1
#define MSM_TS_DOUBLE_EWMA 2
int msm_ts_filter(const void* const* X_ptrs, void* const* out_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int dtype_bytes,
                  msm_idx_t n_features, msm_idx_t ld, msm_idx_t ld_out, int on_device, int kind, int order, const double* b,
                  const double* a, const double* zi, msm_idx_t width, double alpha, int adjust, msm_idx_t min_periods,
                  msm_idx_t segment);

/* ------------------------------------------------------------------------------------------
 * Post-clustering transition counts.  Replaces the counting loop of
 * msmbuilder.msm._transition_counts (/root/reference/msmbuilder/msm/core.py:487-596) for integer
 * labels: y_ptrs[s] -> n_rows[s] int64 labels (device-resident, e.g. KCenters.labels_, or host).
 * msm_label_range: min / max label over all sequences (*hi < *lo if there are no labels).
 * msm_label_histogram: hist[b] (host, int64[n_bins]) = #labels equal to lo + b -- the class discovery
 *   behind np.unique (core.py:544); labels outside [lo, lo + n_bins) are ignored.
 * msm_transition_counts: counts (host, int64 [n_states][n_states], row-major) [i][j] = number of
 *   (t, t + lag_time) pairs inside one sequence with state(y[t]) = i and state(y[t+lag]) = j, where
 *   state(v) = remap[v - lo] (host int32[n_bins], -1 = no mapping: the pair is dropped, as for
 *   NaN / None upstream) or v - lo when remap is NULL (then n_bins must equal n_states).  The caller
 *   divides by lag_time for the sliding-window normalisation (core.py:594). */
int msm_label_range(const msm_idx_t* const* y_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int on_device,
                    msm_idx_t* lo, msm_idx_t* hi, msm_idx_t* n_total);
int msm_label_histogram(const msm_idx_t* const* y_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int on_device,
                        msm_idx_t lo, msm_idx_t n_bins, int64_t* hist);
int msm_transition_counts(const msm_idx_t* const* y_ptrs, const msm_idx_t* n_rows, msm_idx_t n_seq, int on_device,
                          msm_idx_t lag_time, msm_idx_t lo, const int32_t* remap, msm_idx_t n_bins,
                          msm_idx_t n_states, int64_t* counts);

/* ------------------------------------------------------------------------------------------
 * dir-npy trajectories straight into HBM.  MSMBuilder's NumpyDirDataset is a directory
 * of %08d.npy files read with np.load (/root/reference/msmbuilder/dataset.py:290-331).
 * msm_npy_info: parse a .npy header (format 1.0-3.0, little-endian bool/int/uint/float): item size,
 *   kind ('f','i','u','b'), fortran_order, ndim, shape (up to 4), byte offset of the payload.
 * Loader: n_buffers reader threads, each with one pinned host buffer of buffer_bytes and its own
 *   stream, pread() buffer-sized pieces of the submitted files and copy them to the caller's device
 *   pointer; submit() validates the header, queues the pieces and returns a job id at once, wait(job)
 *   returns when that job and every earlier one are completely in HBM, so disk, PCIe and the kernels
 *   on previously loaded trajectories overlap.  nbytes must equal the file's payload size (from
 *   msm_npy_info); read / copy errors surface at wait(). */
typedef struct msm_npy_loader msm_npy_loader_t;
int msm_npy_info(const char* path, int* dtype_bytes, int* kind, int* fortran_order, int* ndim, msm_idx_t* shape4,
                 msm_idx_t* data_offset);
int msm_npy_loader_create(msm_npy_loader_t** out, int n_buffers, size_t buffer_bytes);
int msm_npy_loader_submit(msm_npy_loader_t* h, const char* path, void* dptr, msm_idx_t nbytes, msm_idx_t* job_id);
int msm_npy_loader_wait(msm_npy_loader_t* h, msm_idx_t job_id);
int msm_npy_loader_destroy(msm_npy_loader_t* h);

/* ------------------------------------------------------------------------------------------
 * Device-side generalized eigensolve.  Replaces scipy.linalg.eigh(A, b=B,
 * eigvals=(n-k, n-1)) of /root/reference/msmbuilder/decomposition/tica.py:188-194: the k LARGEST
 * solutions of A v = lambda B v (A symmetric, B symmetric positive definite, float64 n x n, host or
 * device), evals[k] descending, evecs[k][n] row j = eigenvector j, normalised v^T B v = 1, sign
 * arbitrary (LAPACK's conventions).  Runs dpotrf + dtrsm + dsyevd of rocSOLVER / rocBLAS; the library is dlopen'ed at first use
 * (MSM_ERR_STATE if it is not installed).  MSM_ERR_INVALID with LAPACK's message if B is not positive
 * definite. */
int msm_sygv_top(const double* A, const double* B, msm_idx_t n, msm_idx_t k, double* evals, double* evecs,
                 int on_device);

/* ------------------------------------------------------------------------------------------
 * Markov state model estimators (MarkovStateModel, msm/msm.py of msmbuilder).
 * msm_transmat_mle: the reversible maximum-likelihood transition matrix of the counts C (host, n x n
 *   row-major, C + prior is used), replacing _transmat_mle_prinz (msm/_markovstatemodel.pyx, Prinz et al.
 *   2011, Algorithm 1) by an Anderson-accelerated fixed-point iteration on the populations in one device
 *   launch (msm_mle.hip).  Outputs (host): T (n x n), pi (n), optionally S (n x n, NULL = skip) =
 *   D^-1/2 X D^-1/2 with X = diag(x_rs) T symmetric and D = diag(x_rs): symmetric, T's eigenvalues.
 *   info (host, 4 doubles): iterations, converged (1.0), last relative step max|g(x) - x| / max g(x),
 *   KKT residual max|g(pi) - pi| / max pi.  Stops at a step below 1e-14 with every state's own relative step
 *   |g_i(x) - x_i| / g_i(x) below 1e-13, or after max_iter iterations.
 *   MSM_ERR_INVALID with the reference's messages and codes: "Row-sums of C must be positive. Error code=-1" (a
 *   row sum of C or C + C^T not positive, prefixed to "Domain error. C must be positive." when there are also
 *   negative entries), "Domain error. C must be positive. Error code=-2" (negative entries, row sums positive),
 *   "Likelihood not converged. Error code=-3"; NaN or infinite entries are the -2 domain error.  1 <= n <= 16384 (the pattern is built densely on the host).
 *   Sparse (sliced ELL of the pattern of C + C^T) when prior == 0; dense when prior != 0 (every entry is filled)
 *   or with MSM_MLE_DENSE=1.
 * msm_mle_last_stats: how the last msm_transmat_mle of this process stepped (out3: mixed steps accepted, mixed
 *   steps rejected because an entry was not positive, mixing solves rejected as singular or non-finite; each
 *   rejection took the plain step x <- g(x) / sum g(x)).  For the tests of those branches.
 * msm_syev_top: the k largest eigenvalues (descending, evals[k]) and their eigenvectors (evecs[j * n + i],
 *   orthonormal) of the symmetric n x n S; rocSOLVER dsyevd, as msm_sygv_top.  on_device as msm_sygv_top. */
int msm_transmat_mle(const double* C, msm_idx_t n, double prior, msm_idx_t max_iter, double* T, double* pi, double* S,
                     double* info);
int msm_mle_last_stats(msm_idx_t* out3);
int msm_syev_top(const double* S, msm_idx_t n, msm_idx_t k, double* evals, double* evecs, int on_device);

/* ------------------------------------------------------------------------------------------
 * Sparse generalized eigenpairs (SparseTICA; decomposition/_speigh.pyx of msmbuilder): an approximate
 * solution of  max x^T A x - rho |x|_0  s.t. x^T B x <= 1  by majorisation-minimisation around an ADMM solve, all float64,
 * outer and inner loops in ONE persistent launch (relaunched every MSM_SPEIGH_BUDGET ADMM iterations with bit-identical
 * results; MSM_SPEIGH_GRID picks the layout).  1 <= n <= 2048.  on_device: every ARRAY argument is a device pointer (1) or a
 * host pointer (0); u and info are always host.  evals / evecs describe B = sum_j evals[j] e_j e_j^T with evecs[j * n + i] =
 * component i of e_j (msm_syev_top's layout).
 * msm_speigh_project: out = the point of { z : z^T B z <= 1 } nearest to a (a itself, bit for bit, when a lies inside).
 * msm_speigh_admm: min 1/2 |x - b|^2 + |D(w) x|_1 s.t. x^T B x <= 1, warm-started at x_inout, which receives the
 *   soft-thresholded iterate (its exact zeros are the sparsity pattern).  info (host, 4 doubles): iterations, launches,
 *   status (0 converged, 1 maxiter), final penalty parameter.
 * msm_speigh: the pair.  x0 (or NULL: the top generalized eigenvector from msm_sygv_top), evalsB / evecsB (both or neither;
 *   NULL: msm_syev_top of B).  *u = the pseudo-eigenvalue, v[n] = the sparse vector (v^T B v = 1, sum(v) >= 0, no negative
 *   zeros), x_out (or NULL) = the iterate before renormalisation.  info (host, 8 doubles): outer steps (ADMM solves), ADMM
 *   iterations, launches, last objective, nonzeros, status (0 converged, 1 maxiter), workgroups (0: single-workgroup
 *   layout), tau.  MSM_ERR_INVALID: null pointers, n, rho < 0, eps <= 0, tol <= 0, maxiter < 1 (before any device work),
 *   B not positive definite (LAPACK's text); MSM_ERR_NONFINITE: NaN / Inf in A or B; MSM_ERR_STATE: the grid barrier of the
 *   launch timed out (bounded wait).
 * msm_scdeflate: out = A - (A x)(x^T A)^T / (x^T A x), the two products kept apart (A need not be symmetric to rounding
 *   after a deflation); out may be A on the device. */
int msm_speigh_project(const double* a, const double* evals, const double* evecs, msm_idx_t n, double* out, int on_device);
int msm_speigh_admm(const double* b, const double* w, const double* evals, const double* evecs, double* x_inout, msm_idx_t n,
                    double tol, msm_idx_t maxiter, double* info, int on_device);
int msm_speigh(const double* A, const double* B, msm_idx_t n, double rho, double eps, double tol, msm_idx_t maxiter, const double* x0,
               const double* evalsB, const double* evecsB, double* u, double* v, double* x_out, double* info, int on_device);
int msm_scdeflate(const double* A, const double* x, msm_idx_t n, double* out, int on_device);

#ifdef __cplusplus
}
#endif
#endif /* MSMHIP_H */
