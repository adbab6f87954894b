// A reference-style caller of matchBF with randomness = 3 (include/matching.h:594-634) on hand-made FPFH, SHOT and RoPS135 rows: row i
// is the integer i in every element, so the list of query i is known -- i itself at distance 0, then its two neighbours, the larger
// index first at equal distance (a later insertion goes in front).  Also: matchFLANN keeps throwing for randomness > 1.  Run by
// tests/test_host_shim_knn.py.
#include <cstdio>

#include "../../lidar-global-registration_amd/host/lgr_compat.hpp"

using namespace lgr;

template <class FeatureT, int N>
static int lists_ok(const AlignmentParameters& p) {
    const int m = 200;
    auto f = std::make_shared<Cloud<FeatureT>>();
    f->points.resize(m);
    for (int i = 0; i < m; ++i) {
        float* row = reinterpret_cast<float*>(&f->points[i]);
        for (std::size_t e = 0; e < sizeof(FeatureT) / 4; ++e) row[e] = e < N ? (float) i : 7.f;   // (SHOT: the frame is not part of the row)
    }
    f->width = m;
    auto mv = matchBF<FeatureT>(f, f, p);
    int ok = 0;
    for (int i = 1; i + 1 < m; ++i) {
        const auto& c = mv[i];
        ok += c.match_indices.size() == 3 && c.match_indices[0] == i && c.match_indices[1] == i + 1 && c.match_indices[2] == i - 1 &&
              c.distances[0] == 0.f && c.distances[1] == c.distances[2] && c.distances[1] > 0.f;
    }
    return ok == m - 2;
}

int main(int argc, char**) {
    if (argc > 1) { std::printf("compiled\n"); return 0; }   // (no GPU)
    AlignmentParameters p;
    p.bf_block_size = 64; p.randomness = 3;
    std::printf("fpfh_lists=%d shot_lists=%d rops_lists=%d\n", lists_ok<FPFH, 33>(p), lists_ok<SHOT, 352>(p), lists_ok<RoPS135, 135>(p));
    auto f = std::make_shared<FPFHCloud>();
    f->points.resize(4);
    bool threw = false;
    try { matchFLANN<FPFH>(f, f, p); } catch (const std::exception&) { threw = true; }
    std::printf("flann_k3 threw=%d\n", (int) threw);
    p.randomness = 9;
    threw = false;
    try { matchBF<FPFH>(f, f, p); } catch (const std::exception&) { threw = true; }
    std::printf("bf_k9 threw=%d\n", (int) threw);
    return 0;
}
