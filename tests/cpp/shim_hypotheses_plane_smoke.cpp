// A reference-style caller of SampleConsensusPrerejectiveOMP::align() under LGR_SAVE_MULTIPLE_HYPOTHESES with a PLANE metric, compiled by
// tests/test_host_shim_hypotheses_plane.py.  Input: a binary file with n, then n x 12 floats for the source and the target (normals
// included), the correspondences as n x 4 words, max_iterations; argv[2]: metric_id, argv[3]: weight_id.  It prints every figure as its bit
// pattern for the test to compare with lgr_ransac_multi_ex on the same input.
#define LGR_SAVE_MULTIPLE_HYPOTHESES
#include <cstdio>

#include "../../lidar-global-registration_amd/host/lgr_compat.hpp"

using namespace lgr;

static PointNCloud::Ptr read_cloud(FILE* f) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return nullptr;
    auto c = std::make_shared<PointNCloud>();
    c->points.resize(n);
    if (n && std::fread(c->points.data(), 48, n, f) != (size_t) n) return nullptr;
    return c;
}
static void show16(const char* name, int k, const float* v) {
    std::printf("%s%d=", name, k);
    for (int i = 0; i < 16; ++i) { unsigned u; std::memcpy(&u, &v[i], 4); std::printf("%08x", u); }
    std::printf("\n");
}
static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

int main(int argc, char** argv) {
    if (argc < 2) {   // compile and link check only (no GPU)
        AlignmentParameters p;
        p.metric_id = "weighted_closest_plane"; p.weight_id = "nss";
        SampleConsensusPrerejectiveOMP r(std::make_shared<PointNCloud>(), std::make_shared<PointNCloud>(), std::make_shared<Correspondences>(), p);
        if (!r.getHypotheses().empty() || r.getBestHypothesisIndex() != -1) return 1;
        std::printf("shim_hypotheses_plane_smoke: built ok\n");
        return 0;
    }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f);
    int c = 0, max_iterations = 0;
    if (!src || !tgt || std::fread(&c, 4, 1, f) != 1) return 3;
    auto corr = std::make_shared<Correspondences>(c);
    if (c && std::fread(corr->data(), 16, c, f) != (size_t) c) return 4;
    if (std::fread(&max_iterations, 4, 1, f) != 1) return 5;
    std::fclose(f);

    AlignmentParameters p;
    p.metric_id = argc > 2 ? argv[2] : "combination";
    p.weight_id = argc > 3 ? argv[3] : "constant";
    p.score_id = "mse"; p.distance_thr = 0.05f; p.max_iterations = max_iterations;
    SampleConsensusPrerejectiveOMP ransac(src, tgt, corr, p);
    AlignmentResult r = ransac.align();
    std::printf("iterations=%d\nconverged=%d\n", r.iterations, r.converged ? 1 : 0);
    show16("T", 0, r.transformation.data());
    const auto& hs = ransac.getHypotheses();
    std::printf("n_hypotheses=%d\nbest=%d\n", (int) hs.size(), ransac.getBestHypothesisIndex());
    for (size_t k = 0; k < hs.size(); ++k) {
        show16("H", (int) k, hs[k].transformation);
        show16("L", (int) k, hs[k].loop_transformation);
        std::printf("h%d=%d %08x %08x %d %d %08x\n", (int) k, hs[k].iteration, bits(hs[k].loop_metric), bits(hs[k].metric), hs[k].n_inliers, hs[k].converged,
                    bits(hs[k].uniformity));
    }
    return 0;
}
