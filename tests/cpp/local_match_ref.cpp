// local_match_ref.cpp -- CPU statement of matchLocal with a KNNResult(randomness) list (include/matching.h:637-678, :44-94) and of the
// FLANN-contract distance (:586-588), generic in the row length and k, as DESIGN.md section 4 declares them.  An exhaustive loop over
// the train points per query; the list is built by the list rule itself (an entry goes behind every entry whose distance is not larger,
// the list keeps k entries) from the candidates in radiusSearch's order (ascending spatial distance; the index stands for FLANN's
// unspecified order among equals), which leaves the first k candidates in ascending (distance, s, index).  Test infrastructure: written
// on its own, compiled by tests/local_match_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>
#include <vector>

namespace {

struct List { std::vector<int> idx; std::vector<float> dist; };

// the list rule: ascending distances, a later equal distance behind an earlier one, at most k entries
void list_add(List& l, int k, float dist, int index) {
    size_t pos = l.idx.size();
    while (pos > 0 && l.dist[pos - 1] > dist) --pos;
    if ((int) pos >= k) return;
    l.idx.insert(l.idx.begin() + pos, index);
    l.dist.insert(l.dist.begin() + pos, dist);
    if ((int) l.idx.size() > k) { l.idx.resize(k); l.dist.resize(k); }
}

bool row_finite(const float* r, int n) {
    for (int j = 0; j < n; ++j)
        if (!std::isfinite(r[j])) return false;
    return true;
}

// pcl::L2_Norm / FLANN L2_Simple, then the square root
float l2_seq(const float* q, const float* t, int n) {
    float sum = 0.f;
    for (int j = 0; j < n; ++j) { const float d = q[j] - t[j]; sum += d * d; }
    return std::sqrt(sum);
}

}  // namespace

extern "C" {

// the reference's test_knn_result through the list rule: n adds of (dist, index) into a list of `capacity`; returns the list's length
int local_ref_list(int capacity, int n, const float* dists, const int* indices, int* out_idx, float* out_dist) {
    List l;
    for (int e = 0; e < n; ++e) list_add(l, capacity, dists[e], indices[e]);
    for (size_t e = 0; e < l.idx.size(); ++e) { out_idx[e] = l.idx[e]; out_dist[e] = l.dist[e]; }
    return (int) l.idx.size();
}

// points: rows of 12 floats (x y z first); G: column-major 4x4; idx / dist: mq x k, list order, then -1 / 0; n_cand (or NULL): the
// number of candidates of every query
void local_ref_match(int n, const float* qpts, int mq, const float* tpts, int mt, const float* q, const float* t, const float* G, float radius, int k,
                     int* idx, float* dist, int* n_cand) {
    const float r2 = radius * radius;
    std::vector<char> t_ok(mt);
    for (int j = 0; j < mt; ++j)
        t_ok[j] = std::isfinite(tpts[12 * (size_t) j]) && std::isfinite(tpts[12 * (size_t) j + 1]) && std::isfinite(tpts[12 * (size_t) j + 2]) &&
                  row_finite(t + (size_t) n * j, n);
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < mq; ++i) {
        List l;
        int cands = 0;
        const float* qi = q + (size_t) n * i;
        const float px = qpts[12 * (size_t) i], py = qpts[12 * (size_t) i + 1], pz = qpts[12 * (size_t) i + 2];
        const float x = G[0] * px + (G[4] * py + (G[8] * pz + G[12]));
        const float y = G[1] * px + (G[5] * py + (G[9] * pz + G[13]));
        const float z = G[2] * px + (G[6] * py + (G[10] * pz + G[14]));
        if (row_finite(qi, n) && std::isfinite(x) && std::isfinite(y) && std::isfinite(z)) {
            std::vector<std::pair<float, int>> found;   // (s, index): the radius search's result
            for (int j = 0; j < mt; ++j) {
                if (!t_ok[j]) continue;
                const float dx = x - tpts[12 * (size_t) j], dy = y - tpts[12 * (size_t) j + 1], dz = z - tpts[12 * (size_t) j + 2];
                const float s = (dx * dx + dy * dy) + dz * dz;
                if (s < r2) found.push_back({s, j});
            }
            std::sort(found.begin(), found.end());   // ascending spatial distance, then index
            cands = (int) found.size();
            for (const auto& f : found) list_add(l, k, l2_seq(qi, t + (size_t) n * f.second, n), f.second);
        }
        for (int e = 0; e < k; ++e) {
            idx[(size_t) k * i + e] = e < (int) l.idx.size() ? l.idx[e] : -1;
            dist[(size_t) k * i + e] = e < (int) l.idx.size() ? l.dist[e] : 0.f;
        }
        if (n_cand) n_cand[i] = cands;
    }
}

// the FLANN contract's distance of a chosen match: sqrt of the sequential sum; 0 where idx < 0
void local_ref_flann_dist(int n, const float* q, int mq, const float* t, const int* idx, float* dist) {
    for (int i = 0; i < mq; ++i) dist[i] = idx[i] < 0 ? 0.f : l2_seq(q + (size_t) n * i, t + (size_t) n * idx[i], n);
}

}  // extern "C"
