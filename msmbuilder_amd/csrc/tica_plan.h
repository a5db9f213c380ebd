// tica_plan.h -- which kernel a tICA accumulation launches and how it is cut into chunks, decided in ONE place.
// Host only: no HIP call and no getenv.  msm_tica_create fills a TicaGeom, every launch describes itself in a TicaLaunch
// (the caller reads MSM_TICA_FOLD / MSM_TICA_IMG_FUSED and passes the values in), tica_plan turns the two into a TicaPlan,
// and tica_accumulate_device (tica.hip) only carries that plan out.  Exported to the tests as msm_tica_plan.
#pragma once
#include <algorithm>
#include <vector>

#include "tica_common_dev.h"   // TM, BK32, BK64, KCMAX, KFLUSH_SYM

namespace msm {

// What msm_tica_create decides about a handle (all int: msm_tica_plan takes it as an array in this order).
struct TicaGeom {
    int F, lag, mode, T, ntiles;   // T = tiles of TM features per side, ntiles = C and upper G tiles
    int S32, S64;                  // C/G kernels: resident cohorts per flavour
    int sym, ntiles_sym, sym_cohorts, sym_grid, S_sym;   // sum/difference kernel: workgroups per cohort (upper tiles, fewer when the
                                                         // handle packs diagonal blocks: tica_sym_units.h), whole cohorts, workgroups of a launch
                                                         // (sym_grid > sym_cohorts * ntiles_sym: remainder cohort), slab / column-sum rows
    int symw, symw_var, symw_KS, symw_S;   // whole-matrix kernel (fp32 mode, F <= 256): variant (SymwA ..), its K-step, workgroups of a launch
    int symw64, symw_S64;                  // ... float64 rows on the same variant (F <= 128); its resident workgroups
    int img_on, T2, ntile2, S_img, img_grid;   // bf16 image path: 256-wide tiles per side, H and D tiles, whole cohorts, workgroups
    int have_fold;                 // storage of the folded column sums exists
    int shift_on;                  // MSM_TICA_SHIFT as read at the last reset
};
constexpr int TICA_GEOM_INTS = MSM_TICA_GEOM_INTS;
static_assert(sizeof(TicaGeom) == TICA_GEOM_INTS * sizeof(int), "TicaGeom is passed as an int array");

// A slice of one trajectory: `ptr` is trajectory row `off`, the slice holds n_rows rows, and this
// call owns the LEFT indices t in [ob, oe) of the lagged pairs (t, t + lag) -- i.e. it adds
// w_t x_t x_t^T, [t < len - lag] x_t x_{t+lag}^T and the matching column sums for those t only.
// The slice must reach row min(oe + lag, len) - 1 (the right halo).  Whole trajectory: {n, 0, 0, n}.
struct SegInfo {
    long long len, off, ob, oe;
};

// What one call brings.
struct TicaLaunch {
    int dtype_bytes = 4;
    long long ld = 0;
    long long n_seq = 0;
    const msm_idx_t* n_rows = nullptr;   // whole trajectories ...
    const SegInfo* segs = nullptr;       // ... or segments (then n_rows only sizes the slices)
    bool ptr16 = true;    // every valid trajectory's pointer is 16-byte aligned
    bool ptr16_all = true;   // ... and every skipped one's too (the fused kernel asks it of the whole table)
    bool dims4 = true;    // F % 4 == 0 && ld % 4 == 0
    int fold_switch = -1;    // MSM_TICA_FOLD as read for this launch (-1: unset)
    int fused_switch = -1;   // MSM_TICA_IMG_FUSED (-1: unset)
    SegInfo seg(long long s) const { return segs ? segs[s] : SegInfo{n_rows[s], 0, 0, n_rows[s]}; }
    bool valid(const SegInfo& g, int lag) const { return g.len > lag && g.oe > g.ob; }
};

enum TicaPath { TICA_NONE = MSM_TICA_PATH_NONE, TICA_CG64 = MSM_TICA_PATH_CG64, TICA_CG32 = MSM_TICA_PATH_CG32, TICA_SYM = MSM_TICA_PATH_SYM,
                TICA_SYMW = MSM_TICA_PATH_SYMW, TICA_SYMW64 = MSM_TICA_PATH_SYMW64, TICA_IMG_RING = MSM_TICA_PATH_IMG_RING,
                TICA_IMG_FUSED = MSM_TICA_PATH_IMG_FUSED };
// template flavour of the chosen kernel (bits)
enum { TICA_FL_EDGE = MSM_TICA_FL_EDGE, TICA_FL_ALIGNED = MSM_TICA_FL_ALIGNED, TICA_FL_FOLD = MSM_TICA_FL_FOLD, TICA_FL_REM = MSM_TICA_FL_REM,
       TICA_FL_VEC = MSM_TICA_FL_VEC, TICA_FL_X2 = MSM_TICA_FL_X2 };

struct TicaPlan {
    int path = TICA_NONE, flavour = 0;
    int bk = 0, S = 0, G = 0;      // frames per K-step, cohorts of one resident round, workgroups
    bool symrem = false;           // sum/difference kernel: + a remainder cohort of rem_R workgroups, rem_rounds rounds over the tiles
    int rem_R = 0, rem_rounds = 0;
    long long kc = 0;              // frames per chunk (at most)
    bool pairsem = false;          // pair semantics: a frame counts once per valid pair it is in
    bool shifted = false, fold = false;
    int kflush = 0;
    bool pace = false;             // cohort pacing
    bool single = false;           // one whole trajectory: no chunk table, the kernels cut it arithmetically
    long long total = 0, nvalid = 0;   // owned frames and trajectories of the launch (nvalid == 0: nothing to do, path NONE)

    bool img() const { return path == TICA_IMG_RING || path == TICA_IMG_FUSED; }
    bool symw() const { return path == TICA_SYMW || path == TICA_SYMW64; }
    bool sym_slabs() const { return path == TICA_SYM || img(); }   // accumulates into the sum/difference slabs
    // chunks [0, n_main) belong to the whole cohorts, the rest to the remainder cohort: its R workgroups walk them once per
    // round, the whole cohorts share the others S ways -- equal time when n_rem x rounds = n_main / S
    long long n_main(long long nchunks) const
    {
        if (!symrem) return nchunks;
        const long long d = (long long)S * rem_rounds + 1;
        return nchunks - (nchunks + d / 2) / d;
    }
};
constexpr int TICA_PLAN_INTS = MSM_TICA_PLAN_INTS;

inline long long plan_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// a geometry msm_tica_create can have made: every path it enables has cohorts to divide the frames by
inline bool tica_geom_valid(const TicaGeom& g)
{
    if (g.F < 1 || g.lag < 1 || g.mode < MSM_TICA_F32 || g.mode > MSM_TICA_BF16X2 || g.ntiles < 1 || g.S32 < 1 || g.S64 < 1) return false;
    if (g.symw && (g.symw_S < 1 || g.symw_KS < 1 || (g.symw64 && g.symw_S64 < 1))) return false;
    if (g.img_on && (g.S_img < 1 || g.ntile2 < 1 || g.img_grid < 1)) return false;
    return !(g.sym && !g.symw && !g.img_on) || (g.sym_cohorts >= 1 && g.ntiles_sym >= 1);
}

// whole-matrix variant of a width (SymwA .. SymwH of tica_symw_dev.h by id), or -1 beyond 256 features
inline int tica_symw_variant(long long F)
{
    return F <= 16 ? 0 : F <= 32 ? 1 : F <= 64 ? 2 : F <= 96 ? 6 : F <= 128 ? 3 : F <= 160 ? 7 : F <= 192 ? 4 : F <= 256 ? 5 : -1;
}

// Few chunks per cohort (one rank's share of a strong-scaled fit: 1.25M frames = 7.35 chunks of 4096 per cohort, the
// busiest cohort does 8): cohorts take chunks round-robin, so the launch lasts as long as the fullest one.  Try smaller
// chunks and keep the size whose fullest cohort -- plus ~16 frames' worth of prologue per chunk -- is lightest.
inline long long tica_balance_kc(const TicaGeom& g, const TicaLaunch& L, int S, int bk, long long kc)
{
    long long best = -1, best_kc = kc;
    std::vector<long long> load((size_t)S);
    for (long long cand : {4096LL, 3072LL, 2560LL, 2048LL, 1536LL, 1024LL}) {
        std::fill(load.begin(), load.end(), 0LL);
        long long c = 0;
        for (long long s = 0; s < L.n_seq; ++s) {
            const SegInfo t = L.seg(s);
            if (!L.valid(t, g.lag)) continue;
            const long long own = t.oe - t.ob, nch = plan_ceil_div(own, cand);
            const long long piece = plan_ceil_div(plan_ceil_div(own, nch), bk) * bk;
            for (long long r0 = 0; r0 < own; r0 += piece, ++c) load[(size_t)(c % S)] += std::min(piece, own - r0) + 16;
        }
        const long long worst = *std::max_element(load.begin(), load.end());
        if (best < 0 || worst < best) {
            best = worst;
            best_kc = cand;
        }
    }
    return best_kc;
}

inline TicaPlan tica_plan(const TicaGeom& g, const TicaLaunch& L)
{
    TicaPlan p;
    for (long long s = 0; s < L.n_seq; ++s) {
        const SegInfo t = L.seg(s);
        if (L.valid(t, g.lag)) {
            p.total += t.oe - t.ob;
            ++p.nvalid;
        }
    }
    if (p.nvalid == 0) return p;
    const int db = L.dtype_bytes;
    const bool aligned = L.dims4 && L.ptr16;
    const bool f32mode = g.mode == MSM_TICA_F32;
    const bool bfmode = g.mode == MSM_TICA_BF16 || g.mode == MSM_TICA_BF16X2;
    const bool x2 = g.mode == MSM_TICA_BF16X2;
    const bool useimg = bfmode && g.img_on && (db == 4 || db == 2);   // packed bf16 image + 256 x 256 tiles
    // The FUSED kernel: bfloat16-STORED rows of whole 256-feature panels skip the image -- the MFMA kernel's load role stages
    // the raw rows in LDS and forms the packets itself (tica_img_fused_kernel; its slabs equal the packed-image pipeline's
    // bit for bit).  Half the fabric traffic and no ring.  It is the DEFAULT where it is faster -- up to 512 features -- and
    // the packed image from 768 (scripts/fusedprobe.py, profiles/r06_fused_probe.txt, fit wall time fused / image, bf16 |
    // bf16x2: F = 256 0.80 | 0.77, 512 0.88 | 0.84, 768 1.08 | 0.98, 1024 1.09 | 1.06, 1536 1.27 | 1.00, 2048 1.35 | 1.22: a
    // unit of H or D needs x_t AND x_{t+tau} of both panels, and from three panels per side the raw rows' three trips through
    // the LDS cost more than the image's write and read).  MSM_TICA_IMG_FUSED=0 / 1 forces either; 16-byte LDS-direct row pieces.
    bool usefused = false;
    if (useimg && db == 2 && g.F % 256 == 0 && L.ld % 8 == 0)
        usefused = (L.fused_switch >= 0 ? L.fused_switch == 1 : g.F <= 512) && L.ptr16_all;
    // (a bf16 mode whose 256-wide tiles do not fit one resident round -- beyond 3,840 features -- runs the fp32 C/G kernel:
    //  the mode is an accuracy floor, not a promise of the bf16 pipe; bfloat16-stored rows there take the fp64 kernel)
    const bool use32 = db == 4 && (f32mode || (bfmode && !useimg));
    // F <= 256, fp32 mode: the whole-matrix sum/difference kernel (any alignment a float row can have; tica_symw_dev.h)
    // ... and float64 rows of up to 128 features on the same slabs (tica_symw_f64_kernel: the fp64 matrix pipe)
    const bool symw64 = db == 8 && f32mode && g.symw64;
    const bool usesymw = (use32 && f32mode && g.symw) || symw64;
    // sum/difference slabs (H/D kernel: 16-byte aligned rows only; a handle has them unless it has the whole-matrix kernel's)
    const bool usesym = !usesymw && ((use32 && f32mode && g.sym && aligned) || useimg);
    p.path = usefused ? TICA_IMG_FUSED : useimg ? TICA_IMG_RING : symw64 ? TICA_SYMW64 : usesymw ? TICA_SYMW : usesym ? TICA_SYM
             : use32 ? TICA_CG32 : TICA_CG64;
    p.bk = usesymw ? g.symw_KS : (use32 || useimg) ? BK32 : BK64;
    p.pairsem = usesym || usesymw;
    p.S = symw64 ? std::min(g.symw_S, g.symw_S64) : usesymw ? g.symw_S : useimg ? g.S_img : usesym ? g.sym_cohorts : use32 ? g.S32 : g.S64;  // one resident round
    p.symrem = usesym && !useimg && g.sym_grid > p.S * g.ntiles_sym;   // ... + a remainder cohort
    p.G = usesymw ? p.S : p.symrem ? g.sym_grid : p.S * (usesym ? g.ntiles_sym : g.ntiles);
    if (p.symrem) {
        p.rem_R = p.G - p.S * g.ntiles_sym;
        p.rem_rounds = (int)plan_ceil_div(g.ntiles_sym, p.rem_R);
    }
    // chunk size: every cohort gets work, fp32 partials stay <= KCMAX frames
    const int bk = p.bk;
    long long kc = plan_ceil_div(p.total, p.S);
    kc = plan_ceil_div(kc, bk) * bk;
    if (kc > KCMAX) kc = KCMAX;
    // a chunk = one workgroup column of the packing pre-pass: finer chunks, more of them in flight (measured at 1M x 2048
    // bfloat16-stored, pack + multiply: 2048 -> 12.7 ms, 1024 -> 12.3, 512 -> 11.9, 256 -> 11.6; 1024 keeps the per-chunk
    // column sums of a 6.25M-frame fit at 100 MB)
    if (useimg && kc > 1024) kc = 1024;
    if (kc < bk) kc = bk;
    if (usesymw) {
        // every workgroup is a cohort of its own and a trajectory is cut into whole chunks: with about one chunk per
        // workgroup the launch lasts as long as the workgroups that got two (2M x 171 as 200 x 10,000: 600 chunks on 512
        // workgroups, 1.9 ms where the flops need 1.1).  Eight chunks per workgroup and more, but chunks of at least four
        // K-steps / 256 frames (a chunk starts with an exposed load).
        const long long kmin = std::min<long long>(KCMAX, std::max<long long>(256, 4LL * bk));
        kc = plan_ceil_div(plan_ceil_div(p.total, 8LL * p.S), bk) * bk;
        kc = std::min<long long>(KCMAX, std::max<long long>(kc, kmin));
    }
    if (kc == KCMAX && p.total < 16LL * KCMAX * p.S && !useimg && !usesymw) kc = tica_balance_kc(g, L, p.S, bk, kc);
    p.kc = kc;
    p.single = p.nvalid == 1 && L.n_seq == 1 && !L.segs && !useimg;
    // fp32 partial sums of the SHIFTED frames are sigma^2-sized, so two chunks (8192 frames) can share a merge; raw
    // moments (no shift) keep the 4096-frame partials
    p.kflush = g.shift_on ? 2 * KFLUSH_SYM : KFLUSH_SYM;
    // Cohort pacing (the workgroups of a cohort wait for each other at chunk boundaries, bounded).  C/G kernel, measured
    // at 10M x 512: the L2 fabric-side fetch drops from 207 GB to 79-82 GB per launch but the kernel is 4 % slower
    // (78.4 -> 81.7 ms): off there.  Sum/difference kernel WITH the wave-priority window: 110 GB -> 32 GB fetched per
    // launch (1.8x the algorithmic bytes instead of 5.5x) AND 1 % faster (50.45 -> 49.8 ms): on there.
    p.pace = usesym && !useimg;
    // Folded column sums (sum/difference kernel, whole trajectories of >= 2 lag frames, full tiles, launches big enough
    // for a pass over X to matter): no column-sum pass over X ahead of the MFMA kernel -- the kernel's staging lanes sum the
    // left frames, a column-sum pass over the first and last `lag` rows of every trajectory supplies what separates the
    // right frames' sums from the left frames' (and checks those rows), and the finite check is made on the sums afterwards.
    // (bf16 image path: the pre-pass sums while it packs; the fused kernel has no pre-pass: column-sum pass)
    if (usesym && !L.segs && g.have_fold && !usefused && (useimg || g.F % TM == 0)) {
        // MSM_TICA_FOLD: 0 = never, 2 = whatever the size; default: launches of at least 2^26 elements (frames x features)
        const int fmode = L.fold_switch >= 0 ? L.fold_switch : 1;
        p.fold = fmode != 0 && (fmode == 2 || (double)p.total * g.F >= 67108864.0);
        for (long long s = 0; s < L.n_seq && p.fold; ++s)
            if (L.n_rows[s] > g.lag && L.n_rows[s] < 2 * (long long)g.lag) p.fold = false;
        if (2 * (long long)g.lag * p.nvalid > p.total / 4) p.fold = false;   // the boundary rows would be a pass of their own
    }
    p.shifted = g.shift_on && (use32 || useimg || symw64);
    switch (p.path) {
    case TICA_IMG_FUSED:
    case TICA_IMG_RING: p.flavour = (x2 ? TICA_FL_X2 : 0) | (p.fold ? TICA_FL_FOLD : 0); break;
    case TICA_SYMW64: p.flavour = g.F >= 2 ? TICA_FL_VEC : 0; break;   // 16-byte pieces at any alignment of the element; rows of 1-3
    case TICA_SYMW: p.flavour = g.F >= 4 ? TICA_FL_VEC : 0; break;     // floats (a single double) element by element
    case TICA_SYM: p.flavour = (p.symrem ? TICA_FL_REM : 0) | (p.fold ? TICA_FL_FOLD : g.F % TM == 0 ? 0 : TICA_FL_EDGE); break;
    case TICA_CG32: p.flavour = aligned ? TICA_FL_ALIGNED | (g.F % TM == 0 ? 0 : TICA_FL_EDGE) : TICA_FL_EDGE; break;
    default: break;
    }
    return p;
}

inline void tica_plan_ints(const TicaPlan& p, long long* out)
{
    const long long v[TICA_PLAN_INTS] = {p.path, p.flavour, p.bk, p.S, p.G, p.symrem, p.kc, p.rem_R, p.rem_rounds, p.pairsem,
                                         p.shifted, p.fold, p.kflush, p.pace, p.single, p.total, p.nvalid};
    std::copy(v, v + TICA_PLAN_INTS, out);
}

}  // namespace msm
