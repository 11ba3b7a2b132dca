// The grid and the workspace of a pass over all (trial, enrol) pairs: host code shared by trial_ranks.hip (trial_pass_kernel) and
// calibrate.hip (calib_pass_kernel), so that both read the unit rows the targets pass left at the same place.
#pragma once
#include "cos_tile.h"

namespace trial_plan {

constexpr int MAX_SLABS_PER_WG = 1 << 16;       // 32 x 128 x 2^16 = 2^28 pairs per workgroup: a 32-bit LDS count cannot wrap

struct Walk {
    int qtiles, slabs_per_wg, ranges;   // grid (qtiles, ranges); a workgroup walks slabs_per_wg slabs of enrol rows
    size_t tile_lds, unit_t, bytes;     // unit trial rows at ws + 0, unit enrol rows at ws + unit_t
};

inline bool shape_ok(int Nt, int Ne, int D) { return Nt >= 1 && Ne >= 1 && D >= 4 && D % 4 == 0 && D <= cos_tile::MAX_D; }

inline Walk walk(int Nt, int Ne, int D) {
    Walk p{};
    p.qtiles = (Nt + cos_tile::COLS - 1) / cos_tile::COLS;
    const int slabs = (Ne + cos_tile::SLAB - 1) / cos_tile::SLAB;
    // about a thousand workgroups where the shape has them; a workgroup walks at least two slabs (its tile is loaded once)
    const int want = (1024 + p.qtiles - 1) / p.qtiles;
    int spw = (slabs + want - 1) / want;
    const int least = slabs < 2 ? slabs : 2, by_grid = (slabs + 65534) / 65535;
    spw = spw > least ? spw : least;
    spw = spw > by_grid ? spw : by_grid;
    spw = spw < MAX_SLABS_PER_WG ? spw : MAX_SLABS_PER_WG;
    p.slabs_per_wg = spw;
    p.ranges = (slabs + spw - 1) / spw;
    const int Dp = (D + 7) / 8 * 8;
    p.tile_lds = (size_t)Dp * cos_tile::COLS * 4;
    p.unit_t = vp_align_up((size_t)Nt * D * 4, 256);
    p.bytes = p.unit_t + vp_align_up((size_t)Ne * D * 4, 256);
    return p;
}

}  // namespace trial_plan
