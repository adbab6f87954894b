// A reference-style caller of icpRegistrationTrimmed through the shim: a pair written out by tests/test_host_shim_icp_trim.py (binary: n,
// then n x 12 floats for the source and the target; T as 16 floats, column-major).  The options come from the command line; the program
// prints every figure as its bit pattern for the test to compare with the C ABI on the same pair.
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
    lgr_icp_trim_params tp;
    std::memset(&tp, 0xff, sizeof tp);
    lgr_default_icp_trim_params(&tp);
    lgr_icp_ex_params op;
    lgr_default_icp_ex_params(&op);
    if (std::memcmp(&tp.ex, &op, sizeof op) != 0 || tp.keep != 1.f || tp.scale_from_median != 0.f || tp.reserved[0] || tp.reserved[1]) return 1;
    if (sizeof(lgr_icp_trim_params) != 88 || sizeof(lgr_icp_trim_step) != 16) return 1;
    if (argc < 7) { std::printf("shim_icp_trim_smoke: built\n"); return 0; }   // compile and link check only
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f);
    Matrix4f T;
    if (!src || !tgt || std::fread(T.data(), 4, 16, f) != 16) return 3;
    std::fclose(f);
    op.base.max_dist = (float) std::atof(argv[2]);
    op.base.max_iterations = std::atoi(argv[3]);
    op.robust = std::atoi(argv[4]);
    const float keep = (float) std::atof(argv[5]), mult = (float) std::atof(argv[6]);

    lgr_icp_result r;
    std::vector<lgr_icp_trim_step> info;
    const Matrix4f a = icpRegistrationTrimmed(src, tgt, T, op, keep, mult, r, &info);
    const Matrix4f b = icpRegistrationTrimmed(src, tgt, T, op, keep, mult);
    if (std::memcmp(a.data(), b.data(), 64) != 0 || std::memcmp(a.data(), r.transformation, 64) != 0 || info.empty()) return 4;
    std::printf("iterations=%d stop=%d pairs=%d pairs0=%d evaluated=%d\n", r.iterations, r.stop, r.pairs, r.pairs0, (int) info.size());
    std::printf("rmse=%08x rmse0=%08x max_dist=%08x\n", word(r.rmse), word(r.rmse0), word(r.max_dist));
    std::printf("candidates=%d kept=%d cut=%08x scale=%08x\n", info.back().candidates, info.back().kept, word(info.back().cut), word(info.back().scale));
    std::printf("T=");
    for (int k = 0; k < 16; ++k) std::printf("%08x", word(a.data()[k]));
    std::printf("\n");
    return 0;
}
