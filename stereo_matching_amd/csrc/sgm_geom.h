// sgm_geom.h -- a frame's geometry on the working grid and the slanted tiles'
// widths: what the kernels' launchers (sgm_internal.h) and the handle's plan
// (sgm_plan.h) both need.  Plain C++ with no HIP in it.
#pragma once

namespace sgm {

// Geometry of one frame on the working (decimated) grid.
struct Geom {
    int H, W, D;   // rows, cols, disparities
    int scale;     // 1 or 2
};

// elements of one view's cost volume
inline double vol_elems(Geom g) { return (double)g.H * g.W * g.D; }

// ----------------------------------------------- slanted tiles (sgm_slant.hip)
// Compute waves per tile; one more wave per workgroup, the receiver, turns
// the next tile's exit-state granules into LDS states (the compute waves 0
// and 1 store this tile's own exit states themselves).
// The bottom-up pass's tiles are 15 columns wide (16 waves, the workgroup
// maximum): its hand-off granules cost 3 / NW of a tile-step's bytes, and
// slant_up ran 3.9-4.0% faster at HD256 with 15 than with 14; the top-down
// pass keeps 14 (with 15 the H pair beside it lost more than it gained,
// profiles/r06_experiments/r06l_tile_width.txt).
constexpr int kSlantNW = 14;     // top-down
constexpr int kSlantNWUp = 15;   // bottom-up

}  // namespace sgm
