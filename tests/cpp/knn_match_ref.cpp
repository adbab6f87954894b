// knn_match_ref.cpp -- CPU statement of the k-nearest brute-force matcher (matchBF with randomness = k, include/matching.h:612-625),
// written as the literal procedure of DESIGN.md section 4: per train block the K-list of cv::batchDistance (OpenCV 4.5.1: a strict '<'
// against the k-th entry, a shift while '>'), then every block's list, in block and list order, through the insertion of
// updateMultivaluedCorrespondence (src/common.cpp:517-529).  knn_ref_closed is the closed form the library implements: the first k of
// the union of the blocks' lists in (distance ascending, block descending, index descending).  Test infrastructure: compiled by
// tests/knn_match_ref_lib.py with g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <vector>

namespace {

// cv::hal::normL2Sqr_ for n = 16 nb + tail (33: 2 + 1, 135: 8 + 7, 352: 22 + 0): the SSE baseline's four accumulators of four lanes,
// then the scalar tail
float l2sqr(const float* a, const float* b, int n) {
    const int nb = n / 16;
    float acc[4][4] = {};
    for (int blk = 0; blk < nb; ++blk)
        for (int k = 0; k < 4; ++k)
            for (int l = 0; l < 4; ++l) {
                const float t = a[16 * blk + 4 * k + l] - b[16 * blk + 4 * k + l];
                acc[k][l] = t * t + acc[k][l];
            }
    float s[4];
    for (int l = 0; l < 4; ++l) s[l] = ((acc[0][l] + acc[1][l]) + acc[2][l]) + acc[3][l];
    float d = (s[0] + s[2]) + (s[1] + s[3]);
    for (int j = 16 * nb; j < n; ++j) {
        const float t = a[j] - b[j];
        d += t * t;
    }
    return d;
}

struct List { std::vector<int> idx; std::vector<float> dist; };

// batchDistance with K = k over train rows [j0, j1): bestDist starts at FLT_MAX, bestIdx at -1
void block_list(const float* q, const float* t, int n, int j0, int j1, int k, List& out) {
    std::vector<float> bd(k, FLT_MAX);
    std::vector<int> bi(k, -1);
    for (int j = j0; j < j1; ++j) {
        const float d = std::sqrt(l2sqr(q, t + (size_t) n * j, n));
        if (d < bd[k - 1]) {
            int e = k - 2;
            for (; e >= 0 && bd[e] > d; --e) { bd[e + 1] = bd[e]; bi[e + 1] = bi[e]; }
            bd[e + 1] = d; bi[e + 1] = j;
        }
    }
    out.idx.clear(); out.dist.clear();
    for (int e = 0; e < k && bi[e] >= 0; ++e) { out.idx.push_back(bi[e]); out.dist.push_back(bd[e]); }
}

// one match enters the list in front of the first entry whose distance is not smaller; the list keeps k entries
void update(List& c, int k, int match, float distance) {
    size_t pos = 0;
    while (pos < c.idx.size() && c.dist[pos] < distance) ++pos;
    c.idx.insert(c.idx.begin() + pos, match);
    c.dist.insert(c.dist.begin() + pos, distance);
    if ((int) c.idx.size() > k) { c.idx.resize(k); c.dist.resize(k); }
}

void store(const List& c, int k, int* idx, float* dist) {
    for (int e = 0; e < k; ++e) {
        idx[e] = e < (int) c.idx.size() ? c.idx[e] : -1;
        dist[e] = e < (int) c.idx.size() ? c.dist[e] : 0.f;
    }
}

}  // namespace

extern "C" {

float knn_ref_l2sqr(const float* a, const float* b, int n) { return l2sqr(a, b, n); }

// idx / dist: mq x k, list order, then -1 / 0
void knn_ref_match(int n, const float* q, int mq, const float* t, int mt, int block, int k, int* idx, float* dist) {
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < mq; ++i) {
        List c, b;
        for (int j0 = 0; j0 < mt; j0 += block) {
            block_list(q + (size_t) n * i, t, n, j0, std::min(mt, j0 + block), k, b);
            for (size_t e = 0; e < b.idx.size(); ++e) update(c, k, b.idx[e], b.dist[e]);
            if (mt - j0 <= block) break;   // (j0 += block would overflow for a block near INT_MAX)
        }
        store(c, k, idx + (size_t) k * i, dist + (size_t) k * i);
    }
}

// the closed form: the union of the blocks' lists ordered by (d ascending, block descending, index descending), its first k
void knn_ref_closed(int n, const float* q, int mq, const float* t, int mt, int block, int k, int* idx, float* dist) {
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < mq; ++i) {
        List c, b;
        std::vector<std::pair<float, int>> u;
        for (int j0 = 0; j0 < mt; j0 += block) {
            block_list(q + (size_t) n * i, t, n, j0, std::min(mt, j0 + block), k, b);
            for (size_t e = 0; e < b.idx.size(); ++e) u.push_back({b.dist[e], b.idx[e]});
            if (mt - j0 <= block) break;
        }
        std::sort(u.begin(), u.end(), [&](const std::pair<float, int>& x, const std::pair<float, int>& y) {
            if (x.first != y.first) return x.first < y.first;
            if (x.second / block != y.second / block) return x.second / block > y.second / block;
            return x.second > y.second;
        });
        for (size_t e = 0; e < u.size() && (int) e < k; ++e) { c.idx.push_back(u[e].second); c.dist.push_back(u[e].first); }
        store(c, k, idx + (size_t) k * i, dist + (size_t) k * i);
    }
}

// the plain order some would expect: the first k of all rows in (d ascending, index ascending); the fixtures must differ from it
void knn_ref_plain(int n, const float* q, int mq, const float* t, int mt, int k, int* idx, float* dist) {
#pragma omp parallel for schedule(dynamic, 8)
    for (int i = 0; i < mq; ++i) {
        List b;
        block_list(q + (size_t) n * i, t, n, 0, mt, k, b);
        store(b, k, idx + (size_t) k * i, dist + (size_t) k * i);
    }
}

}  // extern "C"
