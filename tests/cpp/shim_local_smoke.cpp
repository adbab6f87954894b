// A reference-style caller of matchLocal and matchFLANN for all three descriptors (include/matching.h:294-312, tests/flann_bf_matcher.h:40-97)
// on hand-made rows: train row j holds 16 j in element 0 and small integers elsewhere, query i is train row i with element 1 raised by
// one -- so query i's nearest row is i at distance 1 and every other row is at least 15 away, in any summation order.  The three-way
// comparison: matchBF == matchFLANN == matchLocal(identity, FLT_MAX) on the match index of every query.  Also: matchLocal<FPFH> with
// randomness 3 returns three-entry lists in ascending distance, matchFLANN keeps throwing for randomness > 1.  Run by
// tests/test_host_shim_local.py.
#include <cstdio>
#include <limits>

#include "../../lidar-global-registration_amd/host/lgr_compat.hpp"

using namespace lgr;

template <class FeatureT, int N>
static std::shared_ptr<Cloud<FeatureT>> make_rows(int m, bool query) {
    auto f = std::make_shared<Cloud<FeatureT>>();
    f->points.resize(m);
    for (int j = 0; j < m; ++j) {
        float* row = reinterpret_cast<float*>(&f->points[j]);
        for (std::size_t e = 0; e < sizeof(FeatureT) / 4; ++e) row[e] = e < N ? (float) ((j * 7 + (int) e * 13) % 11) : (query ? 3.f : 7.f);   // (SHOT: the frame is not part of the row)
        row[0] = 16.f * j;
        if (query) row[1] += 1.f;
    }
    f->width = m;
    return f;
}

static PointNCloud::Ptr make_points(int m, float shift) {
    auto c = std::make_shared<PointNCloud>();
    for (int j = 0; j < m; ++j) c->points.push_back(PointN(0.25f * (j % 17) + shift, 0.5f * (j % 5), 0.125f * j));
    c->width = m;
    return c;
}

template <class FeatureT, int N>
static int three_way(int k) {
    const int m = 150;
    auto q = make_rows<FeatureT, N>(m, true), t = make_rows<FeatureT, N>(m, false);
    auto qp = make_points(m, 0.f), tp = make_points(m, 0.5f);
    AlignmentParameters p;
    p.bf_block_size = 64;
    auto bf = matchBF<FeatureT>(q, t, p);
    auto fl = matchFLANN<FeatureT>(q, t, p);
    p.randomness = k;
    p.guess = Matrix4f::Identity();
    p.match_search_radius = std::numeric_limits<float>::max();
    auto lo = matchLocal<FeatureT>(qp, tp, q, t, p, *p.guess);
    int ok = 0;
    for (int i = 0; i < m; ++i) {
        bool good = bf[i].match_indices.size() == 1 && fl[i].match_indices.size() == 1 && (int) lo[i].match_indices.size() == k &&
                    bf[i].match_indices[0] == i && fl[i].match_indices[0] == i && lo[i].match_indices[0] == i &&
                    fl[i].distances[0] == 1.f && lo[i].distances[0] == 1.f;
        for (int e = 1; e < k && good; ++e) good = lo[i].distances[e] >= lo[i].distances[e - 1] && lo[i].match_indices[e] != i;
        ok += good;
    }
    return ok == m;
}

int main(int argc, char**) {
    if (argc > 1) { std::printf("compiled\n"); return 0; }   // (no GPU)
    std::printf("fpfh=%d shot=%d rops=%d\n", three_way<FPFH, 33>(1), three_way<SHOT, 352>(1), three_way<RoPS135, 135>(1));
    std::printf("fpfh_k3=%d shot_k8=%d rops_k2=%d\n", three_way<FPFH, 33>(3), three_way<SHOT, 352>(8), three_way<RoPS135, 135>(2));
    AlignmentParameters p;
    p.randomness = 3;
    auto f = std::make_shared<SHOTCloud>();
    f->points.resize(4);
    bool threw = false;
    try { matchFLANN<SHOT>(f, f, p); } catch (const std::exception&) { threw = true; }
    std::printf("flann_shot_k3 threw=%d\n", (int) threw);
    p.randomness = 9;
    threw = false;
    auto pts = make_points(4, 0.f);
    try { matchLocal<SHOT>(pts, pts, f, f, p, Matrix4f::Identity()); } catch (const std::exception&) { threw = true; }
    std::printf("local_k9 threw=%d\n", (int) threw);
    return 0;
}
