// teaser_ref.cpp -- the CPU statement of the TEASER alignment ("TEASER"): the whole call and its steps (clique from
// an adjacency matrix, GNC-TLS from TIM lists, TLS from a scalar list), plain sequential C++ over the arithmetic of lgr_teaser_math.h,
// which the device kernels include as well.  The 3x3 SVD is the oracle's c_svd3, op for op the device's lgr_svd3.  Compiled by
// tests/teaser_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../lidar-global-registration_amd/csrc/lgr_teaser_math.h"
#include "../../oracle/src/orc_math.h"

namespace {

struct Corr { int32_t index_query, index_match; float distance, threshold; };
struct P3 { float x, y, z; };

bool edge(const P3& su, const P3& tu, const P3& sv, const P3& tv, float two_beta) {
    return teaser_edge(su.x, su.y, su.z, tu.x, tu.y, tu.z, sv.x, sv.y, sv.z, tv.x, tv.y, tv.z, two_beta);
}

// steps 3 and 4 on a K x K 0/1 matrix (symmetric, zero diagonal): core numbers by removing a node of smallest degree at a time,
// then the greedy clique in V*.  Returns n_clique; clique: ascending positions.
int clique_step(const uint8_t* A, int K, int* core, int* max_core, int* n_core, int* clique) {
    std::vector<int> deg(K, 0);
    std::vector<char> alive(K, 1);
    for (int u = 0; u < K; ++u)
        for (int v = 0; v < K; ++v) deg[u] += (u != v && A[(size_t) u * K + v]) ? 1 : 0;
    int k = 0;
    for (int step = 0; step < K; ++step) {
        int x = -1;
        for (int u = 0; u < K; ++u)
            if (alive[u] && (x < 0 || deg[u] < deg[x])) x = u;
        k = std::max(k, deg[x]);
        core[x] = k;
        alive[x] = 0;
        for (int v = 0; v < K; ++v)
            if (alive[v] && v != x && A[(size_t) x * K + v]) --deg[v];
    }
    *max_core = k;
    int n_alive = 0;
    for (int u = 0; u < K; ++u) { alive[u] = core[u] == k; n_alive += alive[u]; }
    *n_core = n_alive;
    for (int u = 0; u < K; ++u) {
        deg[u] = 0;
        if (!alive[u]) continue;
        for (int v = 0; v < K; ++v) deg[u] += (alive[v] && u != v && A[(size_t) u * K + v]) ? 1 : 0;
    }
    while (n_alive > 0) {
        int x = -1;
        for (int u = 0; u < K; ++u)   // smallest degree, among equals the largest position
            if (alive[u] && (x < 0 || deg[u] <= deg[x])) x = u;
        if (deg[x] >= n_alive - 1) break;
        alive[x] = 0;
        --n_alive;
        for (int v = 0; v < K; ++v)
            if (alive[v] && A[(size_t) x * K + v]) --deg[v];
    }
    int n = 0;
    for (int u = 0; u < K; ++u)
        if (alive[u]) clique[n++] = u;
    return n;
}

// step 5 on n TIMs (a, b: n x 3).  w: n weights out.
void gnc_step(const float* a, const float* b, int n, float beta, int max_it, float gnc, float cost_thr, float R[9], float* w, int* solves_out, float* cost_out,
              int* n_inliers) {
    const float two_beta = 2.f * beta, e2 = teaser_e2(two_beta);
    std::vector<float> r(n);
    for (int k = 0; k < n; ++k) w[k] = 1.f;
    float mu = 0.f, prev = std::numeric_limits<float>::infinity(), cost = 0.f;
    int solves = 0;
    for (int it = 0; it < max_it; ++it) {
        float H[9];
        for (int rr = 0; rr < 3; ++rr)
            for (int s = 0; s < 3; ++s) {
                float acc = 0.f;
                for (int k = 0; k < n; ++k) acc += (w[k] * a[3 * k + rr]) * b[3 * k + s];
                H[3 * rr + s] = acc;
            }
        teaser_rotation(H, R, [](const float* A, float* U, float* S, float* V) { orc::c_svd3(A, U, S, V); });
        ++solves;
        float mx = 0.f;
        for (int k = 0; k < n; ++k) {
            r[k] = teaser_residual(R, a[3 * k], a[3 * k + 1], a[3 * k + 2], b[3 * k], b[3 * k + 1], b[3 * k + 2]);
            mx = teaser_max(mx, r[k]);
        }
        if (it == 0) {
            mu = teaser_mu0(mx, e2);
            if (!(mu > 0.f)) break;
        }
        cost = 0.f;
        for (int k = 0; k < n; ++k) cost += w[k] * r[k];
        bool any = false;
        for (int k = 0; k < n; ++k) { w[k] = teaser_weight(r[k], mu, e2); any = any || w[k] > 0.f; }
        const float diff = std::fabs(cost - prev);
        mu = mu * gnc;
        prev = cost;
        if (diff < cost_thr || !any) break;
    }
    int in = 0;
    for (int k = 0; k < n; ++k) in += w[k] >= 0.5f ? 1 : 0;
    *solves_out = solves; *cost_out = cost; *n_inliers = in;
}

// step 6 on one axis.  flags: the chosen centre's consensus.
void tls_step(const float* x, int n, float beta, float* shift, float* cost_out, uint8_t* flags) {
    std::vector<uint64_t> keys(2 * (size_t) n);
    for (int k = 0; k < n; ++k) { keys[2 * k] = teaser_end_key(x[k] - beta, 0, k); keys[2 * k + 1] = teaser_end_key(x[k] + beta, 1, k); }
    std::sort(keys.begin(), keys.end());
    bool found = false;
    float best_cost = 0.f, best_shift = 0.f, best_centre = 0.f;
    for (int i = 0; i + 1 < 2 * n; ++i) {
        const float centre = 0.5f * (teaser_key_value(keys[i]) + teaser_key_value(keys[i + 1]));
        float sum = 0.f;
        int cnt = 0;
        for (int k = 0; k < n; ++k)
            if (teaser_in_consensus(x[k], centre, beta)) { sum += x[k]; ++cnt; }
        if (!cnt) continue;
        const float xhat = sum / (float) cnt;
        float cost = 0.f;
        for (int k = 0; k < n; ++k) cost += teaser_tls_term(x[k], xhat, beta);
        if (!found || cost < best_cost) { found = true; best_cost = cost; best_shift = xhat; best_centre = centre; }
    }
    *shift = found ? best_shift : 0.f;
    *cost_out = found ? best_cost : (float) n;
    for (int k = 0; k < n; ++k) flags[k] = (found && teaser_in_consensus(x[k], best_centre, beta)) ? 1 : 0;
}

void degrees(const std::vector<P3>& S, const std::vector<P3>& T, float two_beta, int* deg) {
    const int c = (int) S.size();
    for (int i = 0; i < c; ++i) {
        int d = 0;
        for (int j = 0; j < c; ++j) {
            if (j == i) continue;
            const float ls = teaser_len(S[i].x - S[j].x, S[i].y - S[j].y, S[i].z - S[j].z), lt = teaser_len(T[i].x - T[j].x, T[i].y - T[j].y, T[i].z - T[j].z);
            d += std::fabs(ls - lt) < two_beta ? 1 : 0;   // GROR's node reliability: strict
        }
        deg[i] = d;
    }
}

bool pack(const float* src, int ns, const float* tgt, int nt, const Corr* corr, int c, std::vector<P3>& S, std::vector<P3>& T) {
    S.resize(c); T.resize(c);
    for (int i = 0; i < c; ++i) {
        if ((uint32_t) corr[i].index_query >= (uint32_t) ns || (uint32_t) corr[i].index_match >= (uint32_t) nt) return false;
        const float* s = src + 12 * (size_t) corr[i].index_query;
        const float* t = tgt + 12 * (size_t) corr[i].index_match;
        S[i] = P3{s[0], s[1], s[2]}; T[i] = P3{t[0], t[1], t[2]};
    }
    return true;
}

}  // namespace

extern "C" {

int teaser_ref_clique(const uint8_t* A, int K, int* core, int* max_core, int* n_core, int* clique) { return clique_step(A, K, core, max_core, n_core, clique); }

void teaser_ref_gnc(const float* a, const float* b, int n, float beta, int max_it, float gnc, float cost_thr, float* R9, float* w, int* solves, float* cost,
                    int* n_inliers) {
    gnc_step(a, b, n, beta, max_it, gnc, cost_thr, R9, w, solves, cost, n_inliers);
}

void teaser_ref_tls(const float* x, int n, float beta, float* shift, float* cost, uint8_t* flags) { tls_step(x, n, beta, shift, cost, flags); }

int teaser_ref_degrees(const float* src, int ns, const float* tgt, int nt, const Corr* corr, int c, float beta, int* deg) {
    std::vector<P3> S, T;
    if (!pack(src, ns, tgt, nt, corr, c, S, T)) return -1;
    degrees(S, T, 2.f * beta, deg);
    return 0;
}

// the whole call.  T16 column-major; info_i: valid n_nodes max_core n_core n_clique rotation_iterations n_rotation_inliers
// n_translation_inliers n_inliers; info_f: rotation_cost, three axis costs; lists: 2 x 2048 as lgr_teaser's clique argument; mask: c.
// Returns 0, or -1 for an index outside its cloud.
int teaser_ref(const float* src, int ns, const float* tgt, int nt, const Corr* corr, int c, float beta, int k_select, int max_it, float gnc, float cost_thr,
               float* T16, int32_t* info_i, float* info_f, int32_t* lists, uint8_t* mask) {
    for (int k = 0; k < 16; ++k) T16[k] = (k % 5 == 0) ? 1.f : 0.f;
    for (int k = 0; k < 9; ++k) info_i[k] = 0;
    for (int k = 0; k < 4; ++k) info_f[k] = 0.f;
    for (int k = 0; k < 2 * TEASER_NODES_MAX; ++k) lists[k] = -1;
    for (int i = 0; i < c; ++i) mask[i] = 0;
    if (k_select == 0) k_select = 1024;
    const int K = std::min(c, k_select);
    info_i[1] = K;
    if (c < 3) return 0;
    std::vector<P3> Sa, Ta;
    if (!pack(src, ns, tgt, nt, corr, c, Sa, Ta)) return -1;
    const float two_beta = 2.f * beta;
    // 1. nodes
    std::vector<int> deg(c), order(c);
    degrees(Sa, Ta, two_beta, deg.data());
    for (int i = 0; i < c; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return deg[p] > deg[q]; });
    std::vector<P3> S(K), T(K);
    for (int u = 0; u < K; ++u) { S[u] = Sa[order[u]]; T[u] = Ta[order[u]]; lists[TEASER_NODES_MAX + u] = order[u]; }
    // 2. graph
    std::vector<uint8_t> A((size_t) K * K, 0);
    for (int u = 0; u < K; ++u)
        for (int v = 0; v < K; ++v) A[(size_t) u * K + v] = (u != v && edge(S[u], T[u], S[v], T[v], two_beta)) ? 1 : 0;
    // 3. 4.
    std::vector<int> core(K), q(K);
    int max_core = 0, n_core = 0;
    const int nq = clique_step(A.data(), K, core.data(), &max_core, &n_core, q.data());
    info_i[2] = max_core; info_i[3] = n_core; info_i[4] = nq;
    for (int k = 0; k < nq; ++k) lists[k] = order[q[k]];
    if (nq < 3) return 0;
    info_i[0] = 1;
    // 5. rotation
    const int n = nq - 1;
    std::vector<float> a(3 * (size_t) n), b(3 * (size_t) n), w(n);
    for (int k = 0; k < n; ++k) {
        const P3 &s0 = S[q[k]], &s1 = S[q[k + 1]], &t0 = T[q[k]], &t1 = T[q[k + 1]];
        a[3 * k] = s1.x - s0.x; a[3 * k + 1] = s1.y - s0.y; a[3 * k + 2] = s1.z - s0.z;
        b[3 * k] = t1.x - t0.x; b[3 * k + 1] = t1.y - t0.y; b[3 * k + 2] = t1.z - t0.z;
    }
    float R[9];
    gnc_step(a.data(), b.data(), n, beta, max_it, gnc, cost_thr, R, w.data(), &info_i[5], &info_f[0], &info_i[6]);
    // 6. translation
    float t[3];
    std::vector<float> x(nq);
    std::vector<uint8_t> flags(3 * (size_t) nq);
    for (int axis = 0; axis < 3; ++axis) {
        for (int k = 0; k < nq; ++k) {
            const P3 &s = S[q[k]], &tt = T[q[k]];
            const float tv = axis == 0 ? tt.x : (axis == 1 ? tt.y : tt.z);
            x[k] = tv - teaser_rot_row(R, axis, s.x, s.y, s.z);
        }
        tls_step(x.data(), nq, beta, &t[axis], &info_f[1 + axis], flags.data() + (size_t) axis * nq);
    }
    for (int k = 0; k < nq; ++k) info_i[7] += (flags[k] && flags[nq + k] && flags[2 * (size_t) nq + k]) ? 1 : 0;
    // 7. outputs
    for (int row = 0; row < 3; ++row) {
        for (int col = 0; col < 3; ++col) T16[4 * col + row] = R[3 * row + col];
        T16[12 + row] = t[row];
    }
    for (int i = 0; i < c; ++i) {
        const P3 &s = Sa[i], &tt = Ta[i];
        const float mx = teaser_rot_row(R, 0, s.x, s.y, s.z) + t[0], my = teaser_rot_row(R, 1, s.x, s.y, s.z) + t[1], mz = teaser_rot_row(R, 2, s.x, s.y, s.z) + t[2];
        mask[i] = (std::fabs(tt.x - mx) <= beta && std::fabs(tt.y - my) <= beta && std::fabs(tt.z - mz) <= beta) ? 1 : 0;
        info_i[8] += mask[i];
    }
    return 0;
}

}  // extern "C"
