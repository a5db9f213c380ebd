// tica_sym_units.h -- the units of one cohort of the sum/difference kernel (tica_sym_dev.h): which workgroup computes which
// 64 x 64 blocks of H and D.  Host only: no HIP call.  Exported to the tests as msm_tica_sym_units.
//
// A unit is one workgroup's work: the column tiles X and Y it stages (u/d planes of X, then of Y), whether it writes the
// folded column sums of block X, and for each of its four waves the block it accumulates -- row panel (X or Y planes) and row
// offset inside it, column panel and offset, and the slab tile the block belongs to.
//
// Without packing a unit is an upper tile (I <= J) in row-major order: X = I, Y = J, wave (wr, wc) takes rows X + 64 wr and
// columns Y + 64 wc of the unit's own tile, and the diagonal unit writes the column sums.
//
// A diagonal tile is symmetric: its block (1,0) mirrors (0,1) and tica_export_sym_kernel never reads it, so the tile needs
// the three blocks a = (0,0), b = (0,1), c = (1,1) and one wave of its workgroup computes for nothing.  With packing, the
// diagonal tiles are taken in groups of four {4g .. 4g+3}; the DONOR d = 4g+1 gives its three blocks to the free waves of the
// other three, so four workgroups become three:
//     P0: X = 4g,   Y = d: waves 0-2 = a, b, c of X, wave 3 = a of d
//     P1: X = 4g+2, Y = d: waves 0-2 = a, b, c of X, wave 3 = b of d
//     P2: X = 4g+3, Y = d: waves 0-2 = a, b, c of X, wave 3 = c of d
// Waves 0-2 read both fragments from the X planes, wave 3 both from the Y planes; every block lands in the slab tile of the
// diagonal tile it belongs to, so the slab layout and the export do not change (the never-read corner stays zero).  The
// T mod 4 last diagonal tiles and every off-diagonal unit stay as they are.  The donor's column sums are written by the
// off-diagonal unit (d, d+1), whose X is d.  T (T+1)/2 - floor(T/4) units.
#pragma once
#include <vector>

#include "../../include/msmhip.h"

namespace msm {

struct SymWave {
    int row_panel, row_off, col_panel, col_off, slab_tile;   // panels: 0 = the unit's X planes, 1 = its Y planes; offsets 0 | 64
};
struct SymUnit {
    int X, Y, colsum;   // column tiles staged; 1: this unit writes the folded column sums of block X
    SymWave w[4];
};
constexpr int TICA_SYM_UNIT_INTS = MSM_TICA_SYM_UNIT_INTS;
static_assert(sizeof(SymUnit) == TICA_SYM_UNIT_INTS * sizeof(int), "SymUnit is passed as an int array");

// index of the upper tile (I, J), I <= J, in the row-major order of the upper triangle (the slab layout)
inline int sym_slab_tile(int T, int I, int J) { return I * T - I * (I - 1) / 2 + (J - I); }
inline int sym_slab_tiles(int T) { return T * (T + 1) / 2; }
inline int sym_units_per_cohort(int T, bool pack) { return sym_slab_tiles(T) - (pack ? T / 4 : 0); }

inline std::vector<SymUnit> tica_sym_units(int T, bool pack)
{
    std::vector<SymUnit> units;
    const int groups = pack ? T / 4 : 0;
    for (int I = 0; I < T; ++I)
        for (int J = I; J < T; ++J) {
            const int tile = sym_slab_tile(T, I, J);
            const bool grouped = I == J && I / 4 < groups;
            const int d = 4 * (I / 4) + 1;   // the donor of I's group
            SymUnit u;
            if (!grouped) {   // a whole tile: off-diagonal, or a diagonal tile outside the groups
                u.X = I;
                u.Y = J;
                // the donor's own unit is gone: (d, d + 1) stages its columns as X and sums them
                u.colsum = I == J || (J == I + 1 && I / 4 < groups && I == d);
                for (int w = 0; w < 4; ++w) u.w[w] = SymWave{0, 64 * (w >> 1), 1, 64 * (w & 1), tile};
            } else if (I == d) {
                continue;     // its blocks ride on the three other units of the group
            } else {
                const int k = I % 4 == 0 ? 0 : I % 4 - 1;   // which block of the donor wave 3 takes: a, b, c
                u.X = I;
                u.Y = d;
                u.colsum = 1;
                u.w[0] = SymWave{0, 0, 0, 0, tile};
                u.w[1] = SymWave{0, 0, 0, 64, tile};
                u.w[2] = SymWave{0, 64, 0, 64, tile};
                u.w[3] = SymWave{1, k == 2 ? 64 : 0, 1, k == 0 ? 0 : 64, sym_slab_tile(T, d, d)};
            }
            units.push_back(u);
        }
    return units;
}

// The chunk walks of a packed launch: for every cohort the chunks it takes, in order, and where it merges its fp32
// accumulators into the fp64 slab.  Two candidates, both made of the kernel's own rule -- a cohort v of `stride` takes the
// chunks v, v + stride, ... and merges when another chunk of kc frames would pass kflush, or at its last chunk:
//   * stride S: the packed handle's S cohorts stride over the chunks themselves -- what the plan sized kc for;
//   * stride S0, dealt: the groups of chunks between two merges are formed as the S0 cohorts of the UNPACKED geometry form
//     them, and whole groups are dealt to the S cohorts, each to the cohort that is lightest so far.  Which frames share an
//     fp32 partial is then what it is without packing: the handle gives the same moments with the switch on or off, up to
//     the order of the fp64 additions (when the plan's chunk size is the same: from 16 KCMAX frames per cohort it is).
// A group is up to kflush frames, a coarser granule than a chunk, so the second is taken only where it costs nothing: when
// its fullest cohort is within 1 % of the strided walk's (a cohort's load: its frames + 16 per chunk, the prologue, as in
// tica_balance_kc).  That is the case from a few dozen groups per cohort; below, the cohorts stride.
// out = [S + 1 offsets into the entries][one entry per chunk: its index, bit 31 set where the cohort merges after it];
// returns whether the unpacked partials were kept.
constexpr int SYM_WALK_MERGE = (int)0x80000000u;
inline bool tica_sym_walk(const int* chunk_rows, long long n, int S0, int S, long long kc, long long kflush, std::vector<int>& out)
{
    // the groups of a strided geometry, in the order its cohorts form them: handed to `emit` with the cohort and the load
    auto groups_of = [&](int stride, auto&& emit) {
        std::vector<int> group;
        for (long long v = 0; v < stride && v < n; ++v) {
            long long rows_acc = 0, load = 0;
            for (long long c = v; c < n; c += stride) {
                group.push_back((int)c);
                rows_acc += chunk_rows[c];
                load += chunk_rows[c] + 16;
                if (rows_acc + kc > kflush || c + stride >= n) {
                    group.back() |= SYM_WALK_MERGE;
                    emit((int)v, group, load);
                    group.clear();
                    rows_acc = load = 0;
                }
            }
        }
    };
    std::vector<std::vector<int>> strided((size_t)S), dealt((size_t)S);
    std::vector<long long> load_s((size_t)S, 0), load_d((size_t)S, 0);
    groups_of(S, [&](int v, const std::vector<int>& g, long long load) {
        strided[(size_t)v].insert(strided[(size_t)v].end(), g.begin(), g.end());
        load_s[(size_t)v] += load;
    });
    groups_of(S0, [&](int, const std::vector<int>& g, long long load) {
        size_t to = 0;
        for (size_t s = 1; s < (size_t)S; ++s)
            if (load_d[s] < load_d[to]) to = s;
        dealt[to].insert(dealt[to].end(), g.begin(), g.end());
        load_d[to] += load;
    });
    long long worst_s = 0, worst_d = 0;
    for (int s = 0; s < S; ++s) {
        worst_s = load_s[(size_t)s] > worst_s ? load_s[(size_t)s] : worst_s;
        worst_d = load_d[(size_t)s] > worst_d ? load_d[(size_t)s] : worst_d;
    }
    const bool keep = worst_d * 100 <= worst_s * 101;
    const std::vector<std::vector<int>>& walk = keep ? dealt : strided;
    out.assign((size_t)S + 1, 0);
    for (int s = 0; s < S; ++s) out[(size_t)s + 1] = out[(size_t)s] + (int)walk[(size_t)s].size();
    for (int s = 0; s < S; ++s) out.insert(out.end(), walk[(size_t)s].begin(), walk[(size_t)s].end());
    return keep;
}

}  // namespace msm
