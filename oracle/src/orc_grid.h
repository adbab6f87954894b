// orc_grid.h -- uniform grid over a point cloud: exact radius / k-NN queries for the ORACLE.
//
// The reference uses pcl::KdTreeFLANN (exact search, results sorted by squared distance, FLANN L2_Simple
// distance ((dx*dx)+dy*dy)+dz*dz in float, radius test strict d2 < r*r).  Tie order among equidistant points is
// FLANN-internal (unspecified); the oracle orders by (d2, index).  See SURVEY.md A.3.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace orc {

static inline bool finite3(const float* p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

static inline float dist2(const float* a, const float* b) {
    float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

struct Grid {
    const float* pts = nullptr;  // stride 12 floats
    int n = 0;
    float origin[3] = {0, 0, 0};
    float h = 1.f;
    int dim[3] = {1, 1, 1};
    std::vector<int> cell_start;  // ncell + 1
    std::vector<int> order;       // point indices sorted by (cell id, index)

    // cell coordinate of a coordinate value along axis a (not clamped). Same float ops as the HIP grid.
    inline int cellc(float v, int a) const { return (int) std::floor((v - origin[a]) / h); }

    void build(const float* p, int n_, float h_) {
        pts = p; n = n_; h = h_;
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < n; ++i) {
            const float* q = pts + 12 * (size_t) i;
            if (!finite3(q)) continue;
            for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], q[a]); mx[a] = std::max(mx[a], q[a]); }
        }
        if (!(mn[0] <= mx[0])) { for (int a = 0; a < 3; ++a) { mn[a] = 0; mx[a] = 0; } }
        for (int a = 0; a < 3; ++a) origin[a] = mn[a];
        // The cell size rule of DESIGN.md section 4 (restated from csrc/lgr_grid_rule.h): h is doubled while the box holds more than 256e6
        // cells, or while its longest axis has more than 4096 cells at the caller's h (more than 2^20 after a doubling): past that the
        // rounding of cellc can exceed the cell's margin over the search radius and the 27-cell visit would miss neighbours.  The dims are
        // compared as floats before the cast, so an axis of more than 2^31 cells never reaches it.
        const float h0 = h;
        for (;;) {
            float d[3], dmax = 1.f;
            double cells = 1;
            for (int a = 0; a < 3; ++a) {
                d[a] = std::floor((mx[a] - origin[a]) / h) + 1.f;   // cellc(mx[a], a) + 1
                if (!(d[a] >= 1.f)) d[a] = 1.f;
                cells *= d[a];
                dmax = std::max(dmax, d[a]);
            }
            if (cells <= 256e6 && dmax <= (h == h0 ? 4096.f : 1048576.f)) {
                for (int a = 0; a < 3; ++a) dim[a] = (int) d[a];
                break;
            }
            h *= 2.f;
        }
        size_t ncell = (size_t) dim[0] * dim[1] * dim[2];
        cell_start.assign(ncell + 1, 0);
        std::vector<int> cid(n, -1);
        for (int i = 0; i < n; ++i) {
            const float* q = pts + 12 * (size_t) i;
            if (!finite3(q)) continue;
            int cx = cellc(q[0], 0), cy = cellc(q[1], 1), cz = cellc(q[2], 2);
            cx = std::min(std::max(cx, 0), dim[0] - 1); cy = std::min(std::max(cy, 0), dim[1] - 1); cz = std::min(std::max(cz, 0), dim[2] - 1);
            cid[i] = (cz * dim[1] + cy) * dim[0] + cx;
            cell_start[cid[i] + 1]++;
        }
        for (size_t c = 0; c < ncell; ++c) cell_start[c + 1] += cell_start[c];
        order.resize(cell_start[ncell]);
        std::vector<int> cur(cell_start.begin(), cell_start.end() - 1);
        for (int i = 0; i < n; ++i) if (cid[i] >= 0) order[cur[cid[i]]++] = i;  // ascending index within a cell
    }

    // visit all points of cells [c-1, c+1]^3 around q in canonical order: (cz, cy, cx) lexicographic, then index.
    template <class F> inline void visit27(const float* q, F&& f) const {
        int cx = cellc(q[0], 0), cy = cellc(q[1], 1), cz = cellc(q[2], 2);
        for (int z = std::max(cz - 1, 0); z <= std::min(cz + 1, dim[2] - 1); ++z)
            for (int y = std::max(cy - 1, 0); y <= std::min(cy + 1, dim[1] - 1); ++y)
                for (int x = std::max(cx - 1, 0); x <= std::min(cx + 1, dim[0] - 1); ++x) {
                    size_t c = ((size_t) z * dim[1] + y) * dim[0] + x;
                    for (int s = cell_start[c]; s < cell_start[c + 1]; ++s) f(order[s]);
                }
    }

    struct Cand { float d2; int idx; };
    static inline bool cand_less(const Cand& a, const Cand& b) { return a.d2 < b.d2 || (a.d2 == b.d2 && a.idx < b.idx); }

    // The ring centre of knn along axis a: cellc's float expression, held to +-RING_CELL_MAX = 2^29 before the cast (the same float ops as
    // lgr_ring_cellc on the device).  An axis has fewer than 2^28 cells, so centre +- ring stays inside int for every finite query.  A centre
    // that the clamp moved lies between the query's true cell and the grid, so a cell not reached after ring s is more than s cells from the
    // true cell too: s h only underestimates the separation, and the termination rule stays conservative.
    static constexpr float RING_CELL_MAX = 536870912.f;
    inline int ring_cellc(float v, int a) const {
        return (int) std::fmin(std::fmax(std::floor((v - origin[a]) / h), -RING_CELL_MAX), RING_CELL_MAX);
    }

    // exact k nearest by (d2, idx); out sorted ascending; returns count found (<= k).
    // Only cells that exist are walked, from the first ring that can touch the grid (the Chebyshev gap between the centre and the grid's
    // box of cells) on; rows whose two end cells lie outside the grid are jumped over -- the walk of lgr_knn_query, loop for loop.
    // visits (optional, [3]): the iterations of the z and y loops (the jumps included), the cells examined, the rings walked.
    int knn(const float* q, int k, Cand* out, long long* visits = nullptr) const {
        std::vector<Cand> heap;  // max-heap on cand_less
        heap.reserve(k + 1);
        long long n_iter = 0, n_cells = 0, n_rings = 0;
        if (visits) visits[0] = visits[1] = visits[2] = 0;
        if (!finite3(q)) return 0;
        const int c0[3] = {ring_cellc(q[0], 0), ring_cellc(q[1], 1), ring_cellc(q[2], 2)};
        int maxring = 0, s0 = 0;
        for (int a = 0; a < 3; ++a) {
            maxring = std::max(maxring, std::max(c0[a], dim[a] - 1 - c0[a]));
            s0 = std::max(s0, std::max(-c0[a], c0[a] - (dim[a] - 1)));
        }
        maxring = std::max(maxring, 0);
        auto scan_cell = [&](size_t c) {
            ++n_cells;
            for (int t = cell_start[c]; t < cell_start[c + 1]; ++t) {
                int i = order[t];
                Cand cd{dist2(q, pts + 12 * (size_t) i), i};
                if ((int) heap.size() < k) {
                    heap.push_back(cd);
                    std::push_heap(heap.begin(), heap.end(), cand_less);
                } else if (cand_less(cd, heap.front())) {
                    std::pop_heap(heap.begin(), heap.end(), cand_less);
                    heap.back() = cd;
                    std::push_heap(heap.begin(), heap.end(), cand_less);
                }
            }
        };
        for (int s = s0;; ++s) {
            // scan shell at Chebyshev distance s
            ++n_rings;
            const int zl = c0[2] - s, zr = c0[2] + s, yl = c0[1] - s, yr = c0[1] + s, xl = c0[0] - s, xr = c0[0] + s;
            const int z0 = std::max(zl, 0), z1 = std::min(zr, dim[2] - 1), y0 = std::max(yl, 0), y1 = std::min(yr, dim[1] - 1);
            const int x0 = std::max(xl, 0), x1 = std::min(xr, dim[0] - 1);
            const bool x_ends = xl >= 0 || xr < dim[0], y_edges = yl >= 0 || yr < dim[1];
            for (int z = z0; z <= z1; ++z) {
                ++n_iter;
                const bool face = (z == zl) || (z == zr);
                if (!face && !x_ends && !y_edges) { z = std::min(z1, zr - 1); continue; }
                for (int y = y0; y <= y1; ++y) {
                    ++n_iter;
                    const bool edge = face || (y == yl) || (y == yr);
                    if (!edge && !x_ends) { y = std::min(y1, yr - 1); continue; }
                    const size_t row = ((size_t) z * dim[1] + y) * dim[0];
                    if (edge) {
                        for (int x = x0; x <= x1; ++x) scan_cell(row + x);
                    } else {
                        for (int end = 0; end < 2; ++end) {
                            const int x = end ? xr : xl;
                            if (x < 0 || x >= dim[0]) continue;
                            scan_cell(row + x);
                        }
                    }
                }
            }
            if (visits) { visits[0] = n_iter; visits[1] = n_cells; visits[2] = n_rings; }
            if (s >= maxring) break;
            if ((int) heap.size() == k) {
                float lim = (float) s * h * 0.999f;
                if (heap.front().d2 <= lim * lim) break;
            }
        }
        std::sort_heap(heap.begin(), heap.end(), cand_less);
        for (size_t i = 0; i < heap.size(); ++i) out[i] = heap[i];
        return (int) heap.size();
    }
};

// pick a grid cell size so that the average occupied cell holds ~target points (2-D manifold heuristic)
static inline float auto_cell(const float* pts, int n, float target) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int cnt = 0;
    for (int i = 0; i < n; ++i) {
        const float* q = pts + 12 * (size_t) i;
        if (!finite3(q)) continue;
        ++cnt;
        for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], q[a]); mx[a] = std::max(mx[a], q[a]); }
    }
    if (cnt < 2) return 1.f;
    float e[3] = {mx[0] - mn[0], mx[1] - mn[1], mx[2] - mn[2]};
    std::sort(e, e + 3);
    float area = std::max(e[2] * e[1], 1e-12f);
    float h = std::sqrt(area * target / (float) cnt);
    float hmin = e[2] / 1024.f;
    return std::max(h, std::max(hmin, 1e-6f));
}

}  // namespace orc
