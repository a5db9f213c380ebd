// tica_handle.h -- struct msm_tica, the tICA handle: what tica.hip (accumulation, import / export) and tica_solve.hip (the
// device-resident solve) share.  Everything else of the accumulation stays private to tica.hip.
#pragma once
#include <vector>

#include "tica_plan.h"        // TicaGeom / TicaPlan; through it common.h and tica_common_dev.h (TicaChunk, TM, NCB)
#include "tica_sym_units.h"   // sym_slab_tiles

// a chunk table on the device, with the key of what it was built from
struct ChunkTable {
    msm::DevBuf buf;
    unsigned long long key = 0;   // 0: not to be found again
    long long total = -1, n = 0;  // frames of the keyed launch (a second guard), chunks
    bool hit(unsigned long long k, long long t) const { return k != 0 && key == k && total == t; }
    const msm::TicaChunk* chunks() const { return static_cast<const msm::TicaChunk*>(buf.p); }
    int upload(const std::vector<msm::TicaChunk>& tab, unsigned long long k, long long t)
    {
        key = 0;
        int rc = buf.reserve(tab.size() * sizeof(msm::TicaChunk));
        if (rc) return rc;
        MSM_HIP_CHECK(hipMemcpyAsync(buf.p, tab.data(), tab.size() * sizeof(msm::TicaChunk), hipMemcpyHostToDevice, msm::stream()));
        MSM_HIP_CHECK(hipStreamSynchronize(msm::stream()));  // `tab` is pageable host memory
        key = k;
        total = t;
        n = (long long)tab.size();
        return MSM_OK;
    }
};

struct msm_tica {
    msm::TicaGeom g{};          // what create decided and tica_plan reads (tica_plan.h)
    int S = 0, G = 0;           // C/G slabs: S = max(S32, S64) cohorts, G = S * ntiles
    double* slabs_sym = nullptr;                           // [S_sym * slab_tiles()][2][TM*TM]: H and D blocks
    int* sym_units = nullptr;   // the handle packs diagonal blocks (create_sym): [ntiles_sym] unit records of a cohort, tica_sym_units.h
    int sym_cohorts_unpacked = 0;   // ... the cohorts it would have unpacked: their fp32 partials are kept where that is free (tica_sym_walk)
    msm::DevBuf walk;               // ... the cohorts' chunk walks of the last sum/difference launch, with what they were built from
    unsigned long long walk_key = 0;
    long long walk_total = -1;
    int walk_kflush = 0;
    std::vector<int> table_rows;    // ... rows of every chunk of `table` (the walk is dealt by frames)
    // whole-matrix sum/difference kernel (tica_symw_dev.h): the variant's padded width / group width / interleave,
    // slabs [symw_S][2][FP*FP], rows in use since the last reset
    int symw_FP = 0, symw_W = 0, symw_IL = 0, symw_used = 0;
    double* slabs_w = nullptr;
    double* slabs = nullptr;    // [G][TM*TM]
    double* base = nullptr;     // packed [2FF+2F] imported state
    double* colpart = nullptr;  // [NCB][2][F]
    double* coltmp = nullptr;   // [NCB][2][F]
    double* packed = nullptr;   // [2FF+2F+2] export scratch
    int* flag = nullptr;        // [2]: [0] sticky, [1] per-call
    long long* dbg = nullptr;   // [4] profiling clocks
    unsigned* cosync = nullptr; // [S] cohort pacing counters
    float* shift = nullptr;     // [F] reference row r of the mean shift (fp32 / bf16 kernels); valid once have_shift
    double* shsum = nullptr;    // [3F] raw column sums [A | B | W] of everything accumulated under the shift
    bool have_shift = false;
    double* fold = nullptr;     // folded column sums: [S_sym][F] per-cohort sums of the left frames | [FOLD_NB][F] sample partials | [F] zeros
    bool last_folded = false;   // the most recent launch took the folded path
    bool cg_dirty = false;      // the C/G slabs (`slabs`) hold something since the last reset: only then does the export sum them
    bool slabs_dirty = false;   // slabs_sym hold something since the last reset (a rejected folded launch must be able to undo itself)
    msm::DevBuf snap;           // ... from this copy
    msm::DevBuf foldimg;        // bf16 image path: [nchunks][F] per-chunk sums of the left frames
    msm::DevBuf imgsteps;       // fused bf16 kernel / carried pack: the launch's K-step records (tica_img_steps_kernel)
    msm::DevBuf colsteps;       // carried pack: [pack steps of a super-chunk][Fp] fp64 column sums of the left frames
    int last_carried = 0;       // the last accumulate packed its later super-chunks inside the multiply (msm_tica_last_img_carried)
    int last_fused = 0;         // the last accumulate ran the fused kernel (msm_tica_last_img_fused)
    msm::TicaPlan last_plan;    // the plan of the last accumulate, its chunks and (image ring) super-chunks (msm_tica_last_plan)
    long long last_nchunks = 0, last_super = 0;
    long long n_sh = 0, nw_sh = 0;  // shifted pairs, and the total weight of their Gram terms (2 n_sh for whole trajectories)
    long long n_obs = 0, n_seq = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // bracket the most recent MFMA launch (bf16 image path: the whole pack + multiply pipeline)
    bool timed = false;
    // The chunk tables of the last launch stay on the device with a key of what they were built from.  Fitting the
    // SAME trajectories again (the bench's steps, partial_fit loops, cross-validated re-fits through a pooled handle) then
    // skips the table build, its upload and the two stream synchronisations that cover the pageable host vectors: ~0.3 ms
    // of idle GPU at 1,000 trajectories, and the host gets to the MFMA launch that much earlier.
    ChunkTable table, table2;   // the launch's chunks; boundary rows (folded sums) or right frames (segments)
    long long table_img_groups = 0;
    std::vector<msm::TicaChunk> table_host;   // bf16 image path: the super-chunk loop walks the table on the host
    msm::DevBuf staging;
    double* solve_pin = nullptr; // pinned host staging of the solve's results (one device-to-host copy per solve)
    size_t solve_pin_n = 0;
    msm::DevBuf solve;           // device-resident solve: the regions of SolveBufs (tica_solve.hip), carved in their order
    bool reduced = false;        // solve.A / solve.B hold the reduced matrix and the Cholesky factor of the current state
    size_t packed_len() const { return 2 * (size_t)g.F * g.F + 2 * (size_t)g.F + 2; }
    size_t colbytes() const { return (size_t)msm::NCB * 2 * g.F * sizeof(double); }   // colpart / coltmp
    // slab tiles per cohort: the upper tiles -- g.ntiles_sym is the WORKGROUPS per cohort, fewer on a packed handle
    int slab_tiles() const { return msm::sym_slab_tiles(g.T); }
    size_t sym_slab_bytes() const { return (size_t)g.S_sym * slab_tiles() * 2 * msm::TM * msm::TM * sizeof(double); }
};

// tica.hip: queues slabs / column partials / base -> h->packed (raw moments, un-shifted); no synchronisation.  (Hidden: it
// crosses a file boundary, not the library's, whose exported symbols stay what they were.)
namespace msm { __attribute__((visibility("hidden"))) int tica_export_queue(msm_tica* h); }
