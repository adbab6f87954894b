// A reference-style caller of icpRegistration through the shim: a pair written out by tests/test_host_shim_icp_ex.py (binary: n, then
// n x 12 floats for the source and the target; T as 16 floats, column-major; n weights).  Every option comes from the command line; the
// program prints every figure as its bit pattern for the test to compare with the C ABI on the same pair.
#include <cstdio>
#include <vector>

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
    // the ABI's defaults and layout as the shim sees them (no GPU needed)
    lgr_icp_ex_params op;
    std::memset(&op, 0xff, sizeof op);
    lgr_default_icp_ex_params(&op);
    lgr_icp_params ip;
    lgr_default_icp_params(&ip);
    if (std::memcmp(&op.base, &ip, sizeof ip) != 0 || op.variant != LGR_ICP_POINT_TO_PLANE || op.robust != LGR_ICP_ROBUST_NONE || op.robust_scale != 0.f ||
        op.min_normal_cos != -1.f || op.plane_eps != 0.f || op.reserved[0] || op.reserved[1] || op.reserved[2] || op.weights != nullptr)
        return 1;
    if (sizeof(lgr_icp_ex_params) != 72 || sizeof(lgr_icp_result) != 112) return 1;
    if (argc < 10) { std::printf("shim_icp_ex_smoke: built\n"); return 0; }   // compile and link check only
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f);
    Matrix4f T;
    if (!src || !tgt || std::fread(T.data(), 4, 16, f) != 16) return 3;
    std::vector<float> w(src->size());
    if (std::fread(w.data(), 4, w.size(), f) != w.size()) return 3;
    std::fclose(f);
    op.base.max_dist = (float) std::atof(argv[2]);
    op.base.max_iterations = std::atoi(argv[3]);
    op.variant = std::atoi(argv[4]);
    op.robust = std::atoi(argv[5]);
    op.robust_scale = (float) std::atof(argv[6]);
    op.min_normal_cos = (float) std::atof(argv[7]);
    op.plane_eps = (float) std::atof(argv[8]);
    op.weights = std::atoi(argv[9]) ? w.data() : nullptr;

    lgr_icp_result r;
    const Matrix4f a = icpRegistration(src, tgt, T, op, r);
    const Matrix4f b = icpRegistration(src, tgt, T, op);
    if (std::memcmp(a.data(), b.data(), 64) != 0 || std::memcmp(a.data(), r.transformation, 64) != 0) return 4;
    std::printf("iterations=%d stop=%d pairs=%d pairs0=%d\n", r.iterations, r.stop, r.pairs, r.pairs0);
    std::printf("rmse=%08x rmse0=%08x max_dist=%08x\n", word(r.rmse), word(r.rmse0), word(r.max_dist));
    std::printf("T=");
    for (int k = 0; k < 16; ++k) std::printf("%08x", word(a.data()[k]));
    std::printf("\n");
    return 0;
}
