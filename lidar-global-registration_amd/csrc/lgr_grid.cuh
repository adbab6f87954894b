// lgr_grid.cuh -- device-side uniform-grid queries shared by the HIP translation units.
//
// Replaces the pcl::KdTreeFLANN queries of the reference (exact search).  Distances are FLANN L2_Simple:
// d2 = ((dx*dx) + dy*dy) + dz*dz in float (no contraction); neighbours are ordered by (d2, original index), the
// oracle's tie rule.  Radius queries are strict d2 < r*r (FLANN RadiusResultSet).
#pragma once
#include "lgr_internal.h"

// XCD-aware tile order for kernels whose workgroups walk the (cell, Morton)-sorted points: the hardware places workgroup b on XCD
// b % 8 (speed only -- any order gives the same results), so with the identity mapping the eight neighbours b .. b+7 of the sorted order
// pull the same candidate cells into eight different L2s.  lgr_xcd_tile hands XCD x the contiguous tile range [x * per, (x + 1) * per):
// consecutive tiles of the sorted order run back to back on ONE L2.  Launch lgr_xcd_grid(n_tiles) workgroups; a tile >= n_tiles has
// nothing to do.
__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }
__host__ __device__ __forceinline__ int lgr_xcd_grid(int n_tiles) { return ((n_tiles + 7) >> 3) << 3; }
__device__ __forceinline__ int lgr_xcd_tile(int b, int n_tiles) { return (b & 7) * ((n_tiles + 7) >> 3) + (b >> 3); }

__device__ __forceinline__ int lgr_cellc(float v, float o, float h) { return (int) floorf((v - o) / h); }

__device__ __forceinline__ float lgr_dist2(float ax, float ay, float az, float bx, float by, float bz) {
    float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ bool lgr_finite3(float x, float y, float z) {
    return fabsf(x) <= 3.4028234663852886e38f && fabsf(y) <= 3.4028234663852886e38f && fabsf(z) <= 3.4028234663852886e38f;
}

// Per-thread k-best list kept in LDS, slot-major [k][BLOCK] so lane i always hits bank (i % 32).  While the search runs
// it is a binary MAX-heap under the total order (d2, index): a candidate that beats the root replaces it and sifts down in at
// most log2(k) steps.  (A sorted list with insertion costs up to k shifts per accepted candidate, and a wave pays the longest
// shift of any of its lanes for nearly every candidate: 46 k vector + 57 k scalar instructions per wave in the normals
// kernel.)  finalize() heap-sorts in place, after which dist(j) / index(j) are in ascending (d2, index) order -- the same
// k entries in the same order as a sorted insertion would have produced, because the order is total.
template <int BLOCK>
struct KnnList {
    float* d2;   // [kcap][BLOCK]
    int* id;     // [kcap][BLOCK]
    int k, count, t;
    float wreg;   // register copy of the root's distance once the heap is full: most candidates are rejected without touching LDS
    __device__ __forceinline__ void init(float* d2s, int* ids, int k_, int tid) { d2 = d2s; id = ids; k = k_; count = 0; t = tid; wreg = 0.f; }
    __device__ __forceinline__ static bool less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }
    __device__ __forceinline__ float worst() const { return d2[t]; }   // root (valid when count == k)
    __device__ __forceinline__ void sift_down(int pos, int n, float d, int i) {   // place (d, i) at pos of the heap [0, n)
        for (;;) {
            int c = 2 * pos + 1;
            if (c >= n) break;
            float cd = d2[c * BLOCK + t];
            int ci = id[c * BLOCK + t];
            if (c + 1 < n) {
                float rd = d2[(c + 1) * BLOCK + t];
                int ri = id[(c + 1) * BLOCK + t];
                if (less(cd, ci, rd, ri)) { cd = rd; ci = ri; ++c; }
            }
            if (!less(d, i, cd, ci)) break;
            d2[pos * BLOCK + t] = cd; id[pos * BLOCK + t] = ci;
            pos = c;
        }
        d2[pos * BLOCK + t] = d; id[pos * BLOCK + t] = i;
    }
    __device__ __forceinline__ void push(float d, int i) {
        if (count < k) {
            int pos = count++;   // sift up
            while (pos > 0) {
                int par = (pos - 1) >> 1;
                float pd = d2[par * BLOCK + t];
                int pi = id[par * BLOCK + t];
                if (!less(pd, pi, d, i)) break;
                d2[pos * BLOCK + t] = pd; id[pos * BLOCK + t] = pi;
                pos = par;
            }
            d2[pos * BLOCK + t] = d; id[pos * BLOCK + t] = i;
            if (count == k) wreg = d2[t];
            return;
        }
        if (d > wreg) return;
        if (!less(d, i, wreg, id[t])) return;
        sift_down(0, k, d, i);
        wreg = d2[t];
    }
    __device__ __forceinline__ void finalize() {   // heap sort: ascending (d2, index)
        for (int n = count - 1; n > 0; --n) {
            float ld = d2[n * BLOCK + t];
            int li = id[n * BLOCK + t];
            d2[n * BLOCK + t] = d2[t]; id[n * BLOCK + t] = id[t];
            sift_down(0, n, ld, li);
        }
    }
    __device__ __forceinline__ float dist(int j) const { return d2[j * BLOCK + t]; }
    __device__ __forceinline__ int index(int j) const { return id[j * BLOCK + t]; }
};

// candidates [b, e) of the sorted point array, pushed in ascending position (the order the list's tie rule is defined on).  Four
// loads are issued before the first push: the query kernels run at ~2.5 waves per SIMD (the k-best lists fill the LDS), so a
// load per candidate, each waited for, was the kernels' critical path.
template <int BLOCK>
__device__ __forceinline__ void lgr_knn_scan(const GridDev& g, int b, int e, float qx, float qy, float qz, KnnList<BLOCK>& L) {
    for (int t = b; t < e; t += 4) {
        const int last = e - 1;
        const float4 p0 = g.pxyz[t], p1 = g.pxyz[min(t + 1, last)], p2 = g.pxyz[min(t + 2, last)], p3 = g.pxyz[min(t + 3, last)];
        L.push(lgr_dist2(qx, qy, qz, p0.x, p0.y, p0.z), __float_as_int(p0.w));
        if (t + 1 < e) L.push(lgr_dist2(qx, qy, qz, p1.x, p1.y, p1.z), __float_as_int(p1.w));
        if (t + 2 < e) L.push(lgr_dist2(qx, qy, qz, p2.x, p2.y, p2.z), __float_as_int(p2.w));
        if (t + 3 < e) L.push(lgr_dist2(qx, qy, qz, p3.x, p3.y, p3.z), __float_as_int(p3.w));
    }
}

// The ring centre of lgr_knn_query along one axis: lgr_cellc's float expression, held to +-LGR_RING_CELL_MAX before the cast.  An axis has
// fewer than 2^28 cells (the cell cap, lgr_grid_rule.h), so the last ring is below 2^29 + 2^28 and centre +- ring stays inside int for
// every finite query (the quotient may be +-inf: the clamp takes that too).  A query in or near the box is far below the bound and keeps
// its own cell.  A centre that the clamp moved lies between the query's true cell and the grid along that axis, so every grid cell is at
// most as many cells from it as from the true cell: a cell the walk has not reached after ring s is MORE than s cells from the query's own
// cell as well, and s h only underestimates the separation the termination rule needs.  The rule stays conservative (it stops later, never
// earlier), and since the list is the minimum under a total order, the result is the brute-force one either way.
constexpr float LGR_RING_CELL_MAX = 536870912.f;   // 2^29
__device__ __forceinline__ int lgr_ring_cellc(float v, float o, float h) {
    return (int) fminf(fmaxf(floorf((v - o) / h), -LGR_RING_CELL_MAX), LGR_RING_CELL_MAX);
}

// exact k-NN of (qx,qy,qz) in grid g: ring search with the same termination rule as the oracle
// (after ring s every point closer than s*h has been seen).
// Only cells that exist are walked.  The first ring is the Chebyshev gap between the centre and the grid's box of cells (0 for a query
// inside it): no earlier ring holds a cell, so the list is empty until then and no earlier ring could have ended the search.  From that
// ring on each of the three clamped ranges is non-empty, and a ring costs its in-grid cells: the z faces are whole rows; a z between them
// has the two y edge rows (whole x runs) and, between those, only the two x end cells of a row -- rows whose end cells both lie outside
// the grid are jumped over, and so is the whole stretch of z between the faces when it has neither.  Work per query: the in-grid cells of
// the rings walked (each row visited holds at least one) plus a constant per ring, wherever the query lies.
template <int BLOCK>
__device__ __forceinline__ void lgr_knn_query(const GridDev& g, float qx, float qy, float qz, KnnList<BLOCK>& L) {
    const int c0x = lgr_ring_cellc(qx, g.ox, g.h), c0y = lgr_ring_cellc(qy, g.oy, g.h), c0z = lgr_ring_cellc(qz, g.oz, g.h);
    const int maxring = max(max(max(c0x, g.dx - 1 - c0x), max(c0y, g.dy - 1 - c0y)), max(max(c0z, g.dz - 1 - c0z), 0));
    const int s0 = max(max(max(-c0x, c0x - (g.dx - 1)), max(-c0y, c0y - (g.dy - 1))), max(max(-c0z, c0z - (g.dz - 1)), 0));
    for (int s = s0;; ++s) {
        const int zl = c0z - s, zr = c0z + s, yl = c0y - s, yr = c0y + s, xl = c0x - s, xr = c0x + s;
        const int z0 = max(zl, 0), z1 = min(zr, g.dz - 1), y0 = max(yl, 0), y1 = min(yr, g.dy - 1), x0 = max(xl, 0), x1 = min(xr, g.dx - 1);
        const bool x_ends = xl >= 0 || xr < g.dx, y_edges = yl >= 0 || yr < g.dy;   // (s >= s0: xl <= dx - 1 and xr >= 0, y alike)
        for (int z = z0; z <= z1; ++z) {
            const bool face = (z == zl) || (z == zr);
            if (!face && !x_ends && !y_edges) { z = min(z1, zr - 1); continue; }   // nothing between the faces: on to zr, or out
            for (int y = y0; y <= y1; ++y) {
                const bool edge = face || (y == yl) || (y == yr);
                if (!edge && !x_ends) { y = min(y1, yr - 1); continue; }            // no end cell in the grid: on to the yr edge, or out
                const size_t row = ((size_t) z * g.dy + y) * g.dx;
                if (edge) {
                    // the whole x run of this (z, y) row belongs to the shell: its cells are contiguous in memory
                    int b = g.cell_start[row + x0], e = g.cell_start[row + x1 + 1];
                    lgr_knn_scan(g, b, e, qx, qy, qz, L);
                } else {
                    for (int end = 0; end < 2; ++end) {   // the two end cells of an interior row (s > 0 here: they differ)
                        const int x = end ? xr : xl;
                        if (x < 0 || x >= g.dx) continue;
                        int b = g.cell_start[row + x], e = g.cell_start[row + x + 1];
                        lgr_knn_scan(g, b, e, qx, qy, qz, L);
                    }
                }
            }
        }
        if (s >= maxring) break;
        if (L.count == L.k) {
            float lim = (float) s * g.h * 0.999f;
            if (L.worst() <= lim * lim) break;
        }
    }
    L.finalize();
}

// visit every point of the 27 cells around q in canonical order: cells (z, y, x) ascending, inside a cell
// ascending original index (the sort that built the grid is stable).  f(sorted_position, float4 xyz_idx)
template <class F>
__device__ __forceinline__ void lgr_visit27(const GridDev& g, float qx, float qy, float qz, F&& f) {
    int cx = lgr_cellc(qx, g.ox, g.h), cy = lgr_cellc(qy, g.oy, g.h), cz = lgr_cellc(qz, g.oz, g.h);
    for (int z = max(cz - 1, 0); z <= min(cz + 1, g.dz - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, g.dy - 1); ++y) {
            int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dx - 1);
            if (x0 > x1) continue;
            size_t c = ((size_t) z * g.dy + y) * g.dx;
            int b = g.cell_start[c + x0], e = g.cell_start[c + x1 + 1];   // three x-cells are contiguous
            // four loads in flight before the first callback (a load per candidate, each waited for, is a dependent round trip per
            // candidate: the closest-plane metric went from 38 to 16 ms per alignment with this, round 3); same visiting order
            for (int t = b; t < e; t += 4) {
                const int last = e - 1;
                const float4 q0 = g.pxyz[t], q1 = g.pxyz[min(t + 1, last)], q2 = g.pxyz[min(t + 2, last)], q3 = g.pxyz[min(t + 3, last)];
                f(t, q0);
                if (t + 1 < e) f(t + 1, q1);
                if (t + 2 < e) f(t + 2, q2);
                if (t + 3 < e) f(t + 3, q3);
            }
        }
}

// nearest grid point within r2 of p: sorted position or -1.  The candidate loop has no branch on the candidate: every lane offers every
// candidate of its cells and keeps the better one by selects, so a wave never serialises on which lanes found something.
__device__ __forceinline__ int nearest_within(const GridDev& g, float px, float py, float pz, float r2, float& best_d2, int& best_idx) {
    int nn = -1, nn_t = -1;
    float best = 0.f;
    if (g.n > 0 && lgr_finite3(px, py, pz))
        lgr_visit27(g, px, py, pz, [&](int t, const float4& Q) {
            const float d2 = lgr_dist2(px, py, pz, Q.x, Q.y, Q.z);
            const int qi = __float_as_int(Q.w);
            const bool take = (d2 < r2) && (nn < 0 || d2 < best || (d2 == best && qi < nn));
            nn = take ? qi : nn;
            nn_t = take ? t : nn_t;
            best = take ? d2 : best;
        });
    best_d2 = best;
    best_idx = nn;
    return nn_t;
}

// ---- exact nearest neighbour whose cost does not depend on where the query lies (lgr_debug.hip) ----
// lgr_knn_query centres its rings on the query's own cell and walks the cells of each ring that lie in the grid: bounded wherever the
// query is, but a query outside the cloud still pays for every in-grid cell of the rings between the first that touches the grid and the
// one that ends the search, empty cells included.  Here the search descends the grid itself.  cell_start is an exclusive prefix sum over
// the cells in (z, y, x) order, so the points of ANY contiguous cell range [lo, hi) are the contiguous sorted positions
// [cell_start[lo], cell_start[hi]): two loads say how many points a node holds.  Nodes are such ranges of three kinds -- whole z-slabs
// [z0, z1), rows [y0, y1) of one slab, cells [x0, x1) of one row -- each an axis-aligned box of cells.  A node is halved along its axis
// (a single slab turns into its rows, a single row into its cells), the nearer half is followed, the other pushed; a node with no point,
// or whose box lies farther than the best candidate, is dropped; a node of at most LGR_FAR_LEAF points is scanned.
//   * Order: candidates compete under (d2, original index) with d2 = lgr_dist2, the order of lgr_knn_query's list with k = 1.  The order is
//     total, so the result does not depend on the visiting order: it is the brute-force minimum, provided no node that could hold it is dropped.
//   * Bound: a point of cell a along one axis has u_p = fl(fl(p - o) / h) in [a, a + 1) (lgr_cellc, the expression that built the grid);
//     the query's u_q is the same expression.  Along that axis |q - p| >= (gap - m) h with gap = max(a0 - u_q, u_q - a1, 0) over the
//     node's cells [a0, a1) and m = 4e-7 (|u_q| + d) covering the rounding of both u (two roundings of relative size 2^-24 each, |u_p| <= d).
//     The squared bound is taken times 0.9999, which covers the roundings of lgr_dist2 and of the bound's own arithmetic.  A node is dropped
//     only when bound > best d2 (strictly): a dropped node holds no point of equal computed distance, so no lower index is lost.
//   * Work: every push halves a node, so the stack holds at most ceil(log2 dz) + ceil(log2 dy) + ceil(log2 dx) <= 31 entries (the grid has
//     at most 256e6 cells); should it be full the node at hand is scanned instead of split (still exact).  No ring is walked at all: the
//     number of nodes visited depends on the points near the answer, not on the separation -- an empty region costs two loads however
//     many cells it spans.  Queries farther than about 1.8e19 from the cloud make every squared distance +inf: all points tie, nothing
//     can be dropped, and the lowest index of all wins after a visit of every occupied node.
// Stack: three words per entry, slot-major [LGR_FAR_STACK][BLOCK] in LDS (lane i on bank i % 32).
constexpr int LGR_FAR_STACK = 32, LGR_FAR_LEAF = 8;

struct FarQuery { float ux, uy, uz, mx, my, mz; };

__device__ __forceinline__ float lgr_far_gap(int a0, int a1, float u, float m) {
    const float g = fmaxf(fmaxf((float) a0 - u, u - (float) a1), 0.f) - m;
    return fmaxf(g, 0.f);
}
// squared lower bound of the distance from the query to the box of node (kind, [lo, hi)); kind 0: slabs, 1: rows of a slab, 2: cells of a row
__device__ __forceinline__ float lgr_far_bound(const GridDev& g, const FarQuery& Q, int kind, int lo, int hi) {
    int x0 = 0, x1 = g.dx, y0 = 0, y1 = g.dy, z0, z1;
    if (kind == 0) {
        const int slab = g.dy * g.dx;
        z0 = lo / slab; z1 = hi / slab;
    } else if (kind == 1) {
        const int r0 = lo / g.dx, r1 = hi / g.dx;
        z0 = r0 / g.dy; z1 = z0 + 1;
        y0 = r0 - z0 * g.dy; y1 = r1 - z0 * g.dy;
    } else {
        const int row = lo / g.dx;
        x0 = lo - row * g.dx; x1 = hi - row * g.dx;
        z0 = row / g.dy; z1 = z0 + 1;
        y0 = row - z0 * g.dy; y1 = y0 + 1;
    }
    const float gx = lgr_far_gap(x0, x1, Q.ux, Q.mx) * g.h, gy = lgr_far_gap(y0, y1, Q.uy, Q.my) * g.h, gz = lgr_far_gap(z0, z1, Q.uz, Q.mz) * g.h;
    return ((gx * gx + gy * gy) + gz * gz) * 0.9999f;
}

// nearest grid point of the finite query (qx, qy, qz): its sorted position (-1: the grid is empty), squared distance and original index.
// st_lo / st_hi / st_b: this thread's stack columns (element e at [e * BLOCK]); hi carries the node kind in its top two bits.
template <int BLOCK>
__device__ __forceinline__ int lgr_nearest_far(const GridDev& g, float qx, float qy, float qz, int* st_lo, int* st_hi, float* st_b,
                                               float& best_d2, int& best_idx) {
    int nn = -1, nn_t = -1;
    float best = 0.f;
    best_d2 = 0.f; best_idx = -1;
    if (g.n <= 0) return -1;
    FarQuery Q;
    Q.ux = (qx - g.ox) / g.h; Q.uy = (qy - g.oy) / g.h; Q.uz = (qz - g.oz) / g.h;
    Q.mx = 4e-7f * (fabsf(Q.ux) + (float) g.dx); Q.my = 4e-7f * (fabsf(Q.uy) + (float) g.dy); Q.mz = 4e-7f * (fabsf(Q.uz) + (float) g.dz);
    auto scan = [&](int b, int e) {
        for (int t = b; t < e; ++t) {
            const float4 P = g.pxyz[t];
            const float d2 = lgr_dist2(qx, qy, qz, P.x, P.y, P.z);
            const int pi = __float_as_int(P.w);
            const bool take = nn < 0 || d2 < best || (d2 == best && pi < nn);
            nn = take ? pi : nn; nn_t = take ? t : nn_t; best = take ? d2 : best;
        }
    };
    int sp = 0, kind = 0, lo = 0, hi = g.dz * g.dy * g.dx;
    float bnd = 0.f;
    for (;;) {
        bool pop = true;
        if (!(nn >= 0 && bnd > best)) {
            const int b = g.cell_start[lo], e = g.cell_start[hi];
            if (e > b) {
                const int unit = kind == 0 ? g.dy * g.dx : (kind == 1 ? g.dx : 1);
                const int len = (hi - lo) / unit;
                if (e - b <= LGR_FAR_LEAF || (len == 1 && kind == 2) || (len > 1 && sp == LGR_FAR_STACK)) {
                    scan(b, e);
                } else if (len == 1) {
                    ++kind;   // one slab: its rows; one row: its cells (same range, same bound)
                    pop = false;
                } else {
                    const int mid = lo + (len >> 1) * unit;
                    const float ba = lgr_far_bound(g, Q, kind, lo, mid), bb = lgr_far_bound(g, Q, kind, mid, hi);
                    const bool a_first = !(bb < ba);
                    st_lo[sp * BLOCK] = a_first ? mid : lo;
                    st_hi[sp * BLOCK] = (a_first ? hi : mid) | (kind << 30);
                    st_b[sp * BLOCK] = a_first ? bb : ba;
                    ++sp;
                    if (a_first) { hi = mid; bnd = ba; } else { lo = mid; bnd = bb; }
                    pop = false;
                }
            }
        }
        if (pop) {
            if (sp == 0) break;
            --sp;
            lo = st_lo[sp * BLOCK];
            const int hk = st_hi[sp * BLOCK];
            hi = hk & 0x3fffffff; kind = (int) ((unsigned) hk >> 30);
            bnd = st_b[sp * BLOCK];
        }
    }
    best_d2 = best; best_idx = nn;
    return nn_t;
}
