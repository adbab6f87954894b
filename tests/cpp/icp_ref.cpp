// CPU statement of the point-to-plane ICP (include/lgr.h lgr_icp_plane*; DESIGN.md section 4, "Point-to-plane ICP").  The step's f64
// arithmetic -- the LDL^T solve, the rotation, the composition, the stop rule -- is csrc/lgr_icp_math.h, the one text the device compiles
// too.  Everything else is restated here on its own, by brute force:
//   * the moved point is ((c0 x + c1 y) + c2 z) + c3 per row in f32; a non-finite moved point has no pair;
//   * its nearest target within d_k: strict d2 < d_k * d_k, d2 = ((dx dx) + dy dy) + dz dz in f32, the smallest d2, then the lowest
//     index; non-finite target points never answer; a target whose normal is not finite answers but makes no pair;
//   * the 28 terms of a pair in f64 from the f32 values: u = p - c, r = (nx ex + ny ey) + nz ez with e = p - q, g = (u x n, n) with each
//     cross component a b - c d, then g_a g_b (a <= b, row by row), g_a r, r r; a point without a pair: 28 times +0.0;
//   * every sum is the balanced binary tree over the source index, padded with +0.0 to the next power of two:
//     S(lo, len) = len == 1 ? x[lo] : S(lo, len / 2) + S(lo + len / 2, len / 2);
//   * c = (min + max) * 0.5f per axis over the target points with three finite coordinates, 0 where that is not finite.
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared -I<csrc> (tests/icp_ref_lib.py).
#include <float.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "lgr_icp_math.h"

namespace {

struct Step { float T[16]; float dist; int32_t pairs; float rmse, rot, trans; int32_t reserved[3]; };                                  // lgr_icp_step
struct Result { float T[16]; int32_t iterations, stop; float max_dist; int32_t pairs; float rmse; int32_t pairs0; float rmse0; int32_t reserved[5]; };   // lgr_icp_result

bool finite3(float a, float b, float c) { return std::isfinite(a) && std::isfinite(b) && std::isfinite(c); }

// S(lo, len) over x[0, n) padded with +0.0 (a subtree wholly behind n is a sum of +0.0s: +0.0)
double tree(const double* x, long long n, long long lo, long long len) {
    if (lo >= n) return 0.0;
    if (len == 1) return x[lo];
    return tree(x, n, lo, len / 2) + tree(x, n, lo + len / 2, len / 2);
}

double tree_sum(const double* x, long long n) {
    long long len = 1;
    while (len < n) len <<= 1;
    return tree(x, n, 0, len);
}

}  // namespace

extern "C" {

double icpref_tree_sum(const double* x, long long n) { return tree_sum(x, n); }
int icpref_solve(const double* s27, double* xi6) { return icp_solve(s27, xi6) ? 1 : 0; }
void icpref_rotation(const double* w3, double* R9) { icp_rotation(w3, R9); }

// max_dist > 0 and 0 < min_dist <= max_dist: resolved by the caller (the entry points compute the target's density when asked to).
// trace: room for max_iterations entries.  returns the number of iterations evaluated.
int icpref_run(const float* src, int ns, const float* tgt, int nt, const float* T0, int max_iterations, float max_dist, float min_dist, float shrink, float rot_eps,
               float trans_eps, Result* out, Step* trace) {
    memset(out, 0, sizeof *out);
    memcpy(out->T, T0, 64);
    out->max_dist = max_dist;
    out->rmse = out->rmse0 = FLT_MAX;
    if (ns == 0 || max_iterations == 0) {
        out->stop = ns == 0 ? ICP_STOP_NO_PAIRS : ICP_STOP_MAX_ITERATIONS;
        return 0;
    }
    float c[3];
    for (int a = 0; a < 3; ++a) {
        float mn = INFINITY, mx = -INFINITY;
        for (int j = 0; j < nt; ++j) {
            const float* q = tgt + (size_t) j * 12;
            if (!finite3(q[0], q[1], q[2])) continue;
            if (q[a] < mn) mn = q[a];
            if (q[a] > mx) mx = q[a];
        }
        c[a] = (mn + mx) * 0.5f;
        if (!std::isfinite(c[a])) c[a] = 0.f;
    }
    std::vector<double> terms((size_t) ICP_TERMS * ns);
    std::vector<char> has(ns);
    float T[16], d = max_dist;
    memcpy(T, T0, 64);
    int k = 0, n_eval = 0;
    for (;;) {
#pragma omp parallel for schedule(dynamic, 64)
        for (int i = 0; i < ns; ++i) {
            const float* s = src + (size_t) i * 12;
            const float px = ((T[0] * s[0] + T[4] * s[1]) + T[8] * s[2]) + T[12];
            const float py = ((T[1] * s[0] + T[5] * s[1]) + T[9] * s[2]) + T[13];
            const float pz = ((T[2] * s[0] + T[6] * s[1]) + T[10] * s[2]) + T[14];
            const float r2 = d * d;
            int best = -1;
            float bd = 0.f;
            if (finite3(px, py, pz))
                for (int j = 0; j < nt; ++j) {
                    const float* q = tgt + (size_t) j * 12;
                    if (!finite3(q[0], q[1], q[2])) continue;
                    const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
                    const float d2 = (dx * dx + dy * dy) + dz * dz;
                    if (!(d2 < r2)) continue;
                    if (best < 0 || d2 < bd) { best = j; bd = d2; }   // ascending j: an equal distance keeps the lower index
                }
            double x[ICP_TERMS];
            for (int t = 0; t < ICP_TERMS; ++t) x[t] = 0.0;
            has[i] = 0;
            if (best >= 0) {
                const float* Q = tgt + (size_t) best * 12;
                if (finite3(Q[4], Q[5], Q[6])) {
                    has[i] = 1;
                    const double nx = Q[4], ny = Q[5], nz = Q[6];
                    const double ux = (double) px - (double) c[0], uy = (double) py - (double) c[1], uz = (double) pz - (double) c[2];
                    const double ex = (double) px - (double) Q[0], ey = (double) py - (double) Q[1], ez = (double) pz - (double) Q[2];
                    const double r = (nx * ex + ny * ey) + nz * ez;
                    const double g[6] = {uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz};
                    int t = 0;
                    for (int a = 0; a < 6; ++a)
                        for (int b = a; b < 6; ++b) x[t++] = g[a] * g[b];
                    for (int a = 0; a < 6; ++a) x[t++] = g[a] * r;
                    x[t] = r * r;
                }
            }
            for (int t = 0; t < ICP_TERMS; ++t) terms[(size_t) t * ns + i] = x[t];
        }
        double sums[ICP_TERMS];
        for (int t = 0; t < ICP_TERMS; ++t) sums[t] = tree_sum(terms.data() + (size_t) t * ns, ns);
        long long pairs = 0;
        for (int i = 0; i < ns; ++i) pairs += has[i];
        float Tn[16], rot, trans;
        bool stepped;
        const int stop = icp_step(sums, pairs, c, T, k, max_iterations, rot_eps, trans_eps, Tn, &stepped, &rot, &trans);
        const float rmse = icp_rmse(sums[ICP_TERMS - 1], pairs);
        Step& st = trace[k];
        memset(&st, 0, sizeof st);
        memcpy(st.T, T, 64);
        st.dist = d; st.pairs = (int32_t) pairs; st.rmse = rmse; st.rot = rot; st.trans = trans;
        n_eval = k + 1;
        out->pairs = (int32_t) pairs; out->rmse = rmse;
        if (k == 0) { out->pairs0 = (int32_t) pairs; out->rmse0 = rmse; }
        if (stepped) {
            memcpy(T, Tn, 64);
            k += 1;
        }
        if (stop >= 0) {
            out->stop = stop;
            break;
        }
        d = icp_next_dist(d, shrink, min_dist);
    }
    memcpy(out->T, T, 64);
    out->iterations = k;
    return n_eval;
}

}  // extern "C"
