// CPU statement of trimmed ICP (include/lgr.h lgr_icp_trim*; DESIGN.md section 4, "Trimmed ICP").  The set-up, d_k, the pairing, the tree,
// the step and the stop rule are those of tests/cpp/icp_ex_ref.cpp, which this file includes for its helpers (tree_sum, jdot, finite3, the
// structs) and for the neutral call, which forwards to icpexref_run as the library forwards to lgr_icp_ex*.  The scalar pieces -- the key,
// K from keep and P, the median rank, k of the iteration, the weight -- are csrc/lgr_icp_math.h, the text the device compiles too.  What is
// restated here, per iteration:
//   * a source point's pair and values exactly as in icp_ex_ref.cpp, except that rho is always formed (sqrt(rr) for the three-row variants
//     also without a robust kernel) and that no weight is applied yet; the point is a candidate iff it has a pair (a neighbour, omega > 0,
//     finite normals where read, the gate, a determinant > 0) and icp_trim_key(rho) holds;
//   * the candidates sorted by (key bits, i) -- std::sort over the 64-bit composites, where the device selects by radix;
//   * K, cut, the median key, k_it; the kept candidates' terms with W = icp_trim_weight(robust, rho, k_it) * omega; W not > 0: no pair.
// Build: g++ -O2 -ffp-contract=off -fopenmp -fPIC -shared -I<csrc> (tests/icp_trim_ref_lib.py).
#include <algorithm>

#include "icp_ex_ref.cpp"

namespace {

struct TrimStep { int32_t candidates, kept; float cut, scale; };   // lgr_icp_trim_step

struct Values {
    double om, rho, r, rr, u[3];
    double g[6];               // one row
    double mj[6][3], me[3];    // three rows
};

// the pair's values of source point i with target row Q, before any weight; false: no pair
bool point_values(const Ex& X, const float* T, const float* c, const float* s, int i, float px, float py, float pz, const float* Q, Values* v) {
    v->om = 1.0;
    if (X.w) {
        v->om = (double) X.w[i];
        if (!std::isfinite(v->om) || !(v->om > 0.0)) return false;
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
    double* u = v->u;
    u[0] = (double) px - (double) c[0]; u[1] = (double) py - (double) c[1]; u[2] = (double) pz - (double) c[2];
    const double e[3] = {(double) px - (double) Q[0], (double) py - (double) Q[1], (double) pz - (double) Q[2]};
    if (one_row) {
        v->r = (n[0] * e[0] + n[1] * e[1]) + n[2] * e[2];
        v->rr = v->r * v->r;
        v->rho = std::fabs(v->r);
        const double g[6] = {u[1] * n[2] - u[2] * n[1], u[2] * n[0] - u[0] * n[2], u[0] * n[1] - u[1] * n[0], n[0], n[1], n[2]};
        memcpy(v->g, g, sizeof g);
        return true;
    }
    double M[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (X.variant == ICP_PLANE_TO_PLANE) {
        const double S[6] = {2.0 - X.s * (n[0] * n[0] + m[0] * m[0]), -(X.s * (n[0] * n[1] + m[0] * m[1])), -(X.s * (n[0] * n[2] + m[0] * m[2])),
                             2.0 - X.s * (n[1] * n[1] + m[1] * m[1]), -(X.s * (n[1] * n[2] + m[1] * m[2])), 2.0 - X.s * (n[2] * n[2] + m[2] * m[2])};
        if (!icp_inv_sym3(S, M)) return false;
    }
    const double Mr[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
    for (int q = 0; q < 3; ++q) {
        v->mj[0][q] = Mr[q][2] * u[1] - Mr[q][1] * u[2];
        v->mj[1][q] = Mr[q][0] * u[2] - Mr[q][2] * u[0];
        v->mj[2][q] = Mr[q][1] * u[0] - Mr[q][0] * u[1];
        v->mj[3][q] = Mr[q][0]; v->mj[4][q] = Mr[q][1]; v->mj[5][q] = Mr[q][2];
        v->me[q] = (Mr[q][0] * e[0] + Mr[q][1] * e[1]) + Mr[q][2] * e[2];
    }
    v->rr = (e[0] * v->me[0] + e[1] * v->me[1]) + e[2] * v->me[2];
    v->rho = std::sqrt(v->rr);
    return true;
}

void point_terms_of(const Ex& X, const Values& v, double W, double* x) {
    int t = 0;
    if (X.variant == ICP_POINT_TO_PLANE) {
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) x[t++] = (W * v.g[a]) * v.g[b];
        for (int a = 0; a < 6; ++a) x[t++] = (W * v.g[a]) * v.r;
    } else {
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) x[t++] = W * jdot(a, v.mj[b], v.u);
        for (int a = 0; a < 6; ++a) x[t++] = W * jdot(a, v.me, v.u);
    }
    x[t] = v.rr;
}

}  // namespace

extern "C" {

long long icptrimref_k(float keep, long long P) { return icp_trim_k(keep, P); }
long long icptrimref_median_rank(long long P) { return icp_trim_median_rank(P); }
double icptrimref_scale(float scale_from_median, float key_median, float robust_scale) { return icp_trim_scale(scale_from_median, key_median, robust_scale); }
double icptrimref_weight(int kind, double rho, double k) { return icp_trim_weight(kind, rho, k); }
int icptrimref_key(double rho, uint32_t* bits) { return icp_trim_key(rho, bits) ? 1 : 0; }

// The arguments of icpexref_run, keep and scale_from_median; info: room for max_iterations entries.  returns the number of iterations
// evaluated == the entries of trace and info written.
int icptrimref_run(const float* src, int ns, const float* tgt, int nt, const float* T0, int max_iterations, float max_dist, float min_dist, float shrink, float rot_eps,
                   float trans_eps, int variant, int robust, float robust_scale, float min_normal_cos, float eps, const float* weights, float keep,
                   float scale_from_median, Result* out, Step* trace, TrimStep* info) {
    if ((keep == 1.f && scale_from_median == 0.f) || ns == 0 || max_iterations == 0) {   // the neutral call, the idle calls
        const int n = icpexref_run(src, ns, tgt, nt, T0, max_iterations, max_dist, min_dist, shrink, rot_eps, trans_eps, variant, robust, robust_scale, min_normal_cos,
                                   eps, weights, out, trace);
        for (int k = 0; k < n; ++k) info[k] = TrimStep{trace[k].pairs, trace[k].pairs, 0.f, robust == ICP_ROBUST_NONE ? 0.f : (float) (double) robust_scale};
        return n;
    }
    memset(out, 0, sizeof *out);
    memcpy(out->T, T0, 64);
    out->max_dist = max_dist;
    out->rmse = out->rmse0 = FLT_MAX;
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
    std::vector<Values> vals(ns);
    std::vector<char> cand(ns), has(ns);
    std::vector<uint32_t> key(ns);
    std::vector<unsigned long long> order;
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
            cand[i] = best >= 0 && point_values(X, T, c, s, i, px, py, pz, tgt + (size_t) best * 12, &vals[i]) && icp_trim_key(vals[i].rho, &key[i]);
        }
        order.clear();
        for (int i = 0; i < ns; ++i)
            if (cand[i]) order.push_back(icp_trim_composite(key[i], (uint32_t) i));
        std::sort(order.begin(), order.end());
        const long long P = (long long) order.size(), K = icp_trim_k(keep, P);
        const float cut = K > 0 ? icp_trim_key_value((uint32_t) (order[K - 1] >> 32)) : 0.f;
        const float key_m = P > 0 ? icp_trim_key_value((uint32_t) (order[icp_trim_median_rank(P)] >> 32)) : 0.f;
        const double k_it = icp_trim_scale(scale_from_median, key_m, robust_scale);
        for (int i = 0; i < ns; ++i) has[i] = 0;
        for (long long q = 0; q < K; ++q) has[(uint32_t) order[q]] = 1;   // the kept set: the first K of the order
#pragma omp parallel for schedule(static)
        for (int i = 0; i < ns; ++i) {
            double x[ICP_TERMS];
            if (has[i]) {
                const double W = icp_trim_weight(robust, vals[i].rho, k_it) * vals[i].om;
                if (W > 0.0) point_terms_of(X, vals[i], W, x);
                else has[i] = 0;
            }
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
        info[k] = TrimStep{(int32_t) P, (int32_t) K, cut, robust == ICP_ROBUST_NONE ? 0.f : (float) k_it};
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
