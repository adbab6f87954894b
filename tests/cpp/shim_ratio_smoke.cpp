// A reference-style caller with matching_id "ratio" and ratio_k 3 (include/common.h:146, src/matching.cpp:26-36): the corner scene of
// tests/cpp/shim_shot_smoke.cpp at 40 x 40 points per face with a deterministic jitter (a bare lattice has equal descriptors, and equal
// distances never pass the test), FPFH on every point, single scale.  The shim's correspondences must be those of the C call with
// LGR_MATCH_RATIO and lgr_feature_params.ratio_k = 3, and differ from ratio_k = 2 and from "lr" (what the shim made of "ratio" before
// the matcher existed).  Run by tests/test_host_shim_ratio.py.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../lidar-global-registration_amd/host/lgr_compat.hpp"

using namespace lgr;

static float jitter(unsigned a, unsigned b, unsigned c) {   // in [-0.25, 0.25)
    unsigned h = a * 73856093u ^ b * 19349663u ^ c * 83492791u;
    h ^= h >> 13; h *= 0x5bd1e995u; h ^= h >> 15;
    return (float) (h & 0xffff) / 65536.f * 0.5f - 0.25f;
}

static std::vector<lgr_corr> c_call(const PointNCloud& src, const PointNCloud& tgt, const AlignmentParameters& p, int matching_id, int ratio_k) {
    lgr_params a = to_abi(p);
    a.matching_id = matching_id;
    lgr_feature_params f = to_feature_abi(p);
    f.ratio_k = ratio_k;
    std::vector<lgr_corr> out(src.size());
    int n = 0;
    check(lgr_correspondences_ex(context(), reinterpret_cast<const float*>(src.points.data()), (int) src.size(),
                                 reinterpret_cast<const float*>(tgt.points.data()), (int) tgt.size(), &a, &f, out.data(), &n), "lgr_correspondences_ex");
    out.resize(n);
    return out;
}

static bool same(const Correspondences& a, const std::vector<lgr_corr>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(lgr_corr)) == 0);
}

int main(int argc, char**) {
    AlignmentParameters p;
    p.descriptor_id = "fpfh"; p.keypoint_id = "any"; p.matching_id = "ratio"; p.ratio_k = 3;
    p.feature_radius = 8.f; p.distance_thr = 1.f; p.iss_radius_src = 1.f; p.iss_radius_tgt = 1.f; p.bf_block_size = 1000;
    lgr_params a = to_abi(p);
    lgr_feature_params f = to_feature_abi(p);
    std::printf("matching_id=%d ratio_k=%d\n", a.matching_id, f.ratio_k);
    if (argc > 1) { std::printf("compiled\n"); return 0; }   // (no GPU)
    const int n = 40, shift = 5;
    auto src = std::make_shared<PointNCloud>(), tgt = std::make_shared<PointNCloud>();
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const float s[3][3] = {{2.f * i, 2.f * j, 0}, {shift + 2.f * i, 0, shift + 2.f * j}, {0, 2.f * shift + 2.f * i, 2.f * shift + 2.f * j}};
            for (int k = 0; k < 3; ++k) {
                float q[3], t[3];
                for (int r = 0; r < 3; ++r) {
                    q[r] = s[k][r] + jitter(i, j, 3 * k + r);
                    t[r] = s[k][r] + jitter(i, j, 16 + 3 * k + r);
                }
                // the source is the scene moved by a small rigid motion (a rotation about z and a shift)
                const float cs = std::cos(0.3f), sn = std::sin(0.3f);
                src->points.emplace_back(cs * q[0] - sn * q[1] + 3.f, sn * q[0] + cs * q[1] - 2.f, q[2] + 1.f, 1.f);
                tgt->points.emplace_back(t[0], t[1], t[2], 1.f);
            }
        }
    p.vp_tgt = std::array<float, 3>{80.f, 80.f, 80.f};
    p.vp_src = std::array<float, 3>{80.f, 80.f, 80.f};
    FeatureBasedCorrespondenceSearch search(src, tgt, p);
    CorrespondencesPtr got = search.calculateCorrespondences();
    const auto k3 = c_call(*src, *tgt, p, LGR_MATCH_RATIO, 3), k2 = c_call(*src, *tgt, p, LGR_MATCH_RATIO, 2), lr = c_call(*src, *tgt, p, LGR_MATCH_LR, 3);
    std::printf("ratio3=%zu equal_to_c_call=%d differs_from_k2=%d differs_from_lr=%d k2=%zu lr=%zu\n", got->size(), (int) same(*got, k3),
                (int) !same(*got, k2), (int) !same(*got, lr), k2.size(), lr.size());
    return 0;
}
