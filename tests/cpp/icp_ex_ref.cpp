// CPU statement of the ICP variants (include/lgr.h lgr_icp_ex*; DESIGN.md section 4, "ICP variants").  The set-up, d_k, the tree, the step
// and the stop rule are those of tests/cpp/icp_ref.cpp, restated here so that this file stands on its own; the step's f64 arithmetic and
// the two shared pieces icp_inv_sym3 / icp_robust_weight are csrc/lgr_icp_math.h, the one text the device compiles too.  What a source
// point contributes is restated here by brute force, all in f64 from the f32 values converted exactly, one IEEE operation at a time:
//   * p' = ((c0 x + c1 y) + c2 z) + c3 per row in f32; its nearest target within d_k (strict d2 < d_k * d_k, smallest, lowest index);
//   * omega = weights ? weights[i] : 1; not finite or not > 0: no pair;
//   * n = the target's normal, m_a = (T[a] sx + T[4+a] sy) + T[8+a] sz from the source's normal s; read only where the variant or the
//     gate needs them (POINT_TO_PLANE: n; PLANE_TO_PLANE: n, m; the gate: n, m); a normal that is read and not finite: no pair;
//   * the gate: kept iff (mx nx + my ny) + mz nz >= (double) min_normal_cos;
//   * one row: r = (nx ex + ny ey) + nz ez, rho = |r|, g = (u x n, n); terms (W g_a) g_b, (W g_a) r, r r;
//   * three rows: M = I (POINT_TO_POINT) or the inverse of Sigma = 2 I - s (n n^T + m m^T), s = 1 - (double) eps, entries
//     2 - s (n_a n_a + m_a m_a) and -(s (n_a n_b + m_a m_b)); row q of M: M j_0 = Mq2 uy - Mq1 uz, M j_1 = Mq0 uz - Mq2 ux,
//     M j_2 = Mq1 ux - Mq0 uy, M j_3..5 = Mq0, Mq1, Mq2; M e = (Mq0 ex + Mq1 ey) + Mq2 ez; j_a . v = v2 uy - v1 uz, v0 uz - v2 ux,
//     v1 ux - v0 uy, v_(a-3); terms W (j_a . (M j_b)), W (j_a . (M e)), rr = (ex Me0 + ey Me1) + ez Me2; rho = sqrt(rr);
//   * W = icp_robust_weight(robust, rho, k) * omega (ROBUST_NONE without weights: exactly 1); not > 0: no pair.
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared -I<csrc> (tests/icp_ex_ref_lib.py).
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

double jdot(int a, const double* v, const double* u) {
    switch (a) {
        case 0: return v[2] * u[1] - v[1] * u[2];
        case 1: return v[0] * u[2] - v[2] * u[0];
        case 2: return v[1] * u[0] - v[0] * u[1];
        default: return v[a - 3];
    }
}

struct Ex { int variant, robust; double k; bool gate; double cos_min, s; const float* w; };

// the 28 terms of source point i paired with target row Q (its nearest); false: no pair
bool point_terms(const Ex& X, const float* T, const float* c, const float* s, int i, float px, float py, float pz, const float* Q, double* x) {
    double om = 1.0;
    if (X.w) {
        om = (double) X.w[i];
        if (!std::isfinite(om) || !(om > 0.0)) return false;
    }
    const bool one_row = X.variant == ICP_POINT_TO_PLANE, need_m = X.gate || X.variant == ICP_PLANE_TO_PLANE, need_n = one_row || need_m;
    double n[3] = {0, 0, 0}, m[3] = {0, 0, 0};
    if (need_n) {
        if (!finite3(Q[4], Q[5], Q[6])) return false;
        for (int a = 0; a < 3; ++a) n[a] = (double) Q[4 + a];
    }
    if (need_m) {
        if (!finite3(s[4], s[5], s[6])) return false;
        for (int a = 0; a < 3; ++a) m[a] = ((double) T[a] * (double) s[4] + (double) T[4 + a] * (double) s[5]) + (double) T[8 + a] * (double) s[6];
        if (X.gate && !((m[0] * n[0] + m[1] * n[1]) + m[2] * n[2] >= X.cos_min)) return false;
    }
    const double u[3] = {(double) px - (double) c[0], (double) py - (double) c[1], (double) pz - (double) c[2]};
    const double e[3] = {(double) px - (double) Q[0], (double) py - (double) Q[1], (double) pz - (double) Q[2]};
    const bool weighted = X.robust != ICP_ROBUST_NONE || X.w;
    if (one_row) {
        const double r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
        const double g[6] = {u[1] * n[2] - u[2] * n[1], u[2] * n[0] - u[0] * n[2], u[0] * n[1] - u[1] * n[0], n[0], n[1], n[2]};
        const double W = weighted ? icp_robust_weight(X.robust, std::fabs(r), X.k) * om : 1.0;
        if (!(W > 0.0)) return false;
        int t = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) x[t++] = (W * g[a]) * g[b];
        for (int a = 0; a < 6; ++a) x[t++] = (W * g[a]) * r;
        x[t] = r * r;
        return true;
    }
    double M[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (X.variant == ICP_PLANE_TO_PLANE) {
        const double S[6] = {2.0 - X.s * (n[0] * n[0] + m[0] * m[0]), -(X.s * (n[0] * n[1] + m[0] * m[1])), -(X.s * (n[0] * n[2] + m[0] * m[2])),
                             2.0 - X.s * (n[1] * n[1] + m[1] * m[1]), -(X.s * (n[1] * n[2] + m[1] * m[2])), 2.0 - X.s * (n[2] * n[2] + m[2] * m[2])};
        if (!icp_inv_sym3(S, M)) return false;
    }
    const double Mr[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
    double mj[6][3], me[3];
    for (int q = 0; q < 3; ++q) {
        mj[0][q] = Mr[q][2] * u[1] - Mr[q][1] * u[2];
        mj[1][q] = Mr[q][0] * u[2] - Mr[q][2] * u[0];
        mj[2][q] = Mr[q][1] * u[0] - Mr[q][0] * u[1];
        mj[3][q] = Mr[q][0]; mj[4][q] = Mr[q][1]; mj[5][q] = Mr[q][2];
        me[q] = (Mr[q][0] * e[0] + Mr[q][1] * e[1]) + Mr[q][2] * e[2];
    }
    const double rr = (e[0] * me[0] + e[1] * me[1]) + e[2] * me[2];
    const double W = weighted ? icp_robust_weight(X.robust, X.robust != ICP_ROBUST_NONE ? std::sqrt(rr) : 0.0, X.k) * om : 1.0;
    if (!(W > 0.0)) return false;
    int t = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) x[t++] = W * jdot(a, mj[b], u);
    for (int a = 0; a < 6; ++a) x[t++] = W * jdot(a, me, u);
    x[t] = rr;
    return true;
}

}  // namespace

extern "C" {

int icpexref_inv_sym3(const double* S6, double* M6) { return icp_inv_sym3(S6, M6) ? 1 : 0; }
double icpexref_robust_weight(int kind, double rho, double k) { return icp_robust_weight(kind, rho, k); }

// max_dist > 0 and 0 < min_dist <= max_dist: resolved by the caller.  gate: min_normal_cos > -1; eps: the plane_eps in use (1e-3f for 0).
// weights: null or ns floats.  trace: room for max_iterations entries.  returns the number of iterations evaluated.
int icpexref_run(const float* src, int ns, const float* tgt, int nt, const float* T0, int max_iterations, float max_dist, float min_dist, float shrink, float rot_eps,
                 float trans_eps, int variant, int robust, float robust_scale, float min_normal_cos, float eps, const float* weights, Result* out, Step* trace) {
    memset(out, 0, sizeof *out);
    memcpy(out->T, T0, 64);
    out->max_dist = max_dist;
    out->rmse = out->rmse0 = FLT_MAX;
    if (ns == 0 || max_iterations == 0) {
        out->stop = ns == 0 ? ICP_STOP_NO_PAIRS : ICP_STOP_MAX_ITERATIONS;
        return 0;
    }
    const Ex X{variant, robust, (double) robust_scale, min_normal_cos > -1.f, (double) min_normal_cos, 1.0 - (double) eps, weights};
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
            has[i] = best >= 0 && point_terms(X, T, c, s, i, px, py, pz, tgt + (size_t) best * 12, x);
            for (int t = 0; t < ICP_TERMS; ++t) terms[(size_t) t * ns + i] = has[i] ? x[t] : 0.0;
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
