// lgr_grid_rule.h -- the cell size of a uniform grid as a function of (min, max, h0): plain C++, host side ("The cell
// size of a grid").  lgr_grid_build is its only user in the library; oracle/src/orc_grid.h restates it, and tests/test_gpu_grid_extents.py
// keeps the two equal on boxes that reach every branch.
//
//   dim[a] = floor(fl(fl(mx[a] - mn[a]) / h)) + 1     (lgr_cellc's float expression applied to the box's far corner), at least 1
//   h starts at h0 and is doubled (exact in float) while
//     (1) dim[0] * dim[1] * dim[2] > LGR_GRID_MAX_CELLS: the dense cell table is four bytes per cell, and the stack of lgr_nearest_far
//         (lgr_grid.cuh) is sized by the cap; or
//     (2) max dim > LGR_GRID_MAX_DIM_H0 while h == h0, > LGR_GRID_MAX_DIM after a doubling.  A cell coordinate fl(fl(v - o) / h) carries two
//         roundings of relative size 2^-24, an absolute error of up to 2^-23 * dim cells.  The 27-cell visit is complete only while twice that
//         stays below the cell's margin over the search radius, 1 - r / h: 0.000999 of a cell at h0 = fl(1.001f * r) -> dim + 1 <= 4189;
//         at least 0.5 of a cell after one doubling -> dim <= 2^21.
// The dims are compared as floats before they are cast: a box of more than 2^31 cells along an axis never reaches the cast.
#pragma once
#include <cmath>

constexpr double LGR_GRID_MAX_CELLS = 256e6;
constexpr float LGR_GRID_MAX_DIM_H0 = 4096.f, LGR_GRID_MAX_DIM = 1048576.f;

static inline float lgr_grid_cell_rule(const float mn[3], const float mx[3], float h0, int dim[3]) {
    float h = h0;
    for (;;) {
        float d[3], dmax = 1.f;
        double cells = 1;
        for (int a = 0; a < 3; ++a) {
            d[a] = std::floor((mx[a] - mn[a]) / h) + 1.f;   // same float expression as lgr_cellc
            if (!(d[a] >= 1.f)) d[a] = 1.f;
            cells *= d[a];
            dmax = d[a] > dmax ? d[a] : dmax;
        }
        if (cells <= LGR_GRID_MAX_CELLS && dmax <= (h == h0 ? LGR_GRID_MAX_DIM_H0 : LGR_GRID_MAX_DIM)) {
            for (int a = 0; a < 3; ++a) dim[a] = (int) d[a];
            return h;
        }
        h *= 2.f;
    }
}
