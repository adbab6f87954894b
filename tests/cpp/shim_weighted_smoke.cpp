// A reference-style caller with metric_id "weighted_closest_plane" and weight_id "nss": a synthetic pair written out by
// tests/test_host_shim_weighted.py (binary: n, then n x 12 floats per cloud, then the correspondences as n x 4 ints), alignRansac through
// the shim.  Prints the result for the test to compare with the C ABI call.  Also prints the metric id the shim maps each name to.
#include <cstdio>

#include "../../lidar-global-registration_amd/host/lgr_compat.hpp"

using namespace lgr;

static PointNCloud::Ptr read_cloud(FILE* f) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return nullptr;
    auto c = std::make_shared<PointNCloud>();
    c->points.resize(n);
    if (std::fread(c->points.data(), 48, n, f) != (size_t) n) return nullptr;
    return c;
}

int main(int argc, char** argv) {
    AlignmentParameters p;
    p.metric_id = "weighted_closest_plane";
    std::printf("metric_abi=%d\n", to_abi(p).metric_id);
    p.weight_id = "no_such_weight";
    std::printf("unknown_weight_abi=%d\n", to_metric_abi(p).weight_id);
    if (argc < 2) return 0;   // mapping only (no GPU)
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f);
    int c = 0;
    if (!src || !tgt || std::fread(&c, 4, 1, f) != 1) return 3;
    auto corr = std::make_shared<Correspondences>(c);
    if (std::fread(corr->data(), 16, c, f) != (size_t) c) return 4;
    std::fclose(f);
    p.weight_id = argc > 2 ? argv[2] : "nss";
    p.score_id = "mse"; p.matching_id = "lr"; p.max_iterations = 30000; p.distance_thr = 0.1f; p.fix_seed = true;
    AlignmentResult r = alignRansac(src, tgt, corr, p);
    std::printf("converged=%d iterations=%d T=", (int) r.converged, r.iterations);
    for (int i = 0; i < 16; ++i) {
        float v = r.transformation.data()[i];
        unsigned u;
        std::memcpy(&u, &v, 4);
        std::printf("%08x%s", u, i < 15 ? "," : "\n");
    }
    return 0;
}
