// A reference-style caller of refineTransformation through the shim: a pair written out by tests/test_host_shim_refine.py (binary: n, then
// n x 12 floats for the source and the target; T as 16 floats, column-major).  It refines T under closest_plane and under
// weighted_closest_plane (exp_curvature weights), MSE score, through both overloads, and prints every figure as its bit pattern for the
// test to compare with the C ABI on the same pair.
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
static unsigned word(float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    return u;
}

int main(int argc, char** argv) {
    // the ABI's defaults as the shim sees them (no GPU needed)
    lgr_refine_params rp;
    lgr_default_refine_params(&rp);
    if (rp.score_id != LGR_SCORE_MSE || rp.max_steps != 10 || rp.threshold != 0.f) return 1;
    if (argc < 3) { std::printf("shim_refine_smoke: built\n"); return 0; }   // compile and link check only
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f);
    Matrix4f T;
    if (!src || !tgt || std::fread(T.data(), 4, 16, f) != 16) return 3;
    std::fclose(f);
    const int max_steps = std::atoi(argv[2]);

    for (const char* id : {"closest_plane", "weighted_closest_plane"}) {
        AlignmentParameters p;
        p.metric_id = id; p.score_id = "mse"; p.weight_id = "exp_curvature";
        lgr_refine_result r;
        const Matrix4f a = refineTransformation(src, tgt, T, p, max_steps, r);
        const Matrix4f b = refineTransformation(src, tgt, T, p, max_steps);
        if (std::memcmp(a.data(), b.data(), 64) != 0 || std::memcmp(a.data(), r.transformation, 64) != 0) return 4;
        std::printf("%s_steps=%d %s_stop=%d %s_inliers=%d %s_first_inliers=%d\n", id, r.steps, id, r.stop, id, r.n_inliers, id, r.first.n_inliers);
        std::printf("%s_metric=%08x %s_rmse=%08x %s_first_metric=%08x %s_threshold=%08x\n", id, word(r.metric), id, word(r.rmse), id, word(r.first.metric), id,
                    word(r.threshold));
        std::printf("%s_T=", id);
        for (int k = 0; k < 16; ++k) std::printf("%08x", word(a.data()[k]));
        std::printf("\n");
    }
    return 0;
}
