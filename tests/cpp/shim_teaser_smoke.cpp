// A reference-style caller of alignTeaser and of alignPointClouds with alignment_id "teaser" (include/alignment.h:6-19,
// src/alignment.cpp:37-69, :92-101) through the header-only shim.  First on synthesised correspondences -- a jittered cloud, its copy under
// a known rigid motion, 60 true pairs and 90 false ones: alignTeaser must return the motion, iterations = 1, converged, and the numbers of
// the C call lgr_teaser with lgr_default_teaser_params.  Then end to end on the corner scene of tests/cpp/shim_ratio_smoke.cpp:
// alignPointClouds("teaser") must return what alignTeaser returns for the search's correspondences.  measureAlignment keeps
// its throw (lgr_measure knows no teaser).  Run by tests/test_host_shim_teaser.py.
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

int main(int argc, char**) {
    AlignmentParameters p;
    p.descriptor_id = "fpfh"; p.keypoint_id = "any"; p.matching_id = "one_sided"; p.alignment_id = "teaser";
    p.feature_radius = 8.f; p.distance_thr = 1.f; p.iss_radius_src = 1.f; p.iss_radius_tgt = 1.f; p.bf_block_size = 1000;
    lgr_teaser_params tp;
    lgr_default_teaser_params(&tp, p.distance_thr);
    std::printf("noise_bound=%g k_select=%d max_iterations=%d gnc_factor=%g cost_threshold=%g nodes_max=%d\n", tp.noise_bound, tp.k_select,
                tp.rotation_max_iterations, tp.rotation_gnc_factor, tp.rotation_cost_threshold, (int) LGR_TEASER_NODES_MAX);
    if (argc > 1) { std::printf("compiled\n"); return 0; }   // (no GPU)

    // ---- synthesised correspondences
    const float cs = std::cos(0.3f), sn = std::sin(0.3f), shift[3] = {3.f, -2.f, 1.f};
    auto src = std::make_shared<PointNCloud>(), tgt = std::make_shared<PointNCloud>();
    const int n = 200;
    for (int i = 0; i < n; ++i) {
        const float q[3] = {40.f * jitter(i, 1, 0), 40.f * jitter(i, 2, 0), 8.f * jitter(i, 3, 0)};
        src->points.emplace_back(q[0], q[1], q[2], 1.f);
        tgt->points.emplace_back(cs * q[0] - sn * q[1] + shift[0] + 0.1f * jitter(i, 4, 0), sn * q[0] + cs * q[1] + shift[1] + 0.1f * jitter(i, 5, 0),
                                 q[2] + shift[2] + 0.1f * jitter(i, 6, 0), 1.f);
    }
    auto corr = std::make_shared<Correspondences>();
    for (int i = 0; i < 150; ++i) {
        corr->emplace_back(i, i < 60 ? i : (i * 37 + 11) % n, 1.f, p.distance_thr);
    }
    lgr_teaser_info info;
    AlignmentResult r = alignTeaser(src, tgt, corr, p, &info);
    const float* T = r.transformation.data();   // column-major
    const float r_err = std::fmax(std::fmax(std::fabs(T[0] - cs), std::fabs(T[1] - sn)), std::fmax(std::fabs(T[4] + sn), std::fabs(T[10] - 1.f)));
    const float t_err = std::fmax(std::fmax(std::fabs(T[12] - shift[0]), std::fabs(T[13] - shift[1])), std::fabs(T[14] - shift[2]));
    lgr_result cr;
    lgr_teaser_info cinfo;
    check(lgr_teaser(context(), reinterpret_cast<const float*>(src->points.data()), (int) src->size(), reinterpret_cast<const float*>(tgt->points.data()),
                     (int) tgt->size(), reinterpret_cast<const lgr_corr*>(corr->data()), (int) corr->size(), &tp, &cr, &cinfo, nullptr, nullptr), "lgr_teaser");
    std::printf("teaser iterations=%d converged=%d clique=%d r_ok=%d t_ok=%d equal_to_c_call=%d\n", r.iterations, (int) r.converged, info.n_clique,
                (int) (r_err < 0.01f), (int) (t_err < 0.1f), (int) (std::memcmp(T, cr.transformation, 64) == 0 && std::memcmp(&info, &cinfo, sizeof info) == 0));

    // ---- too few correspondences: no solution, the identity, not converged, no exception
    auto two = std::make_shared<Correspondences>(corr->begin(), corr->begin() + 2);
    AlignmentResult none = alignTeaser(src, tgt, two, p);
    std::printf("two_pairs converged=%d identity=%d iterations=%d\n", (int) none.converged,
                (int) (none.transformation.data()[0] == 1.f && none.transformation.data()[12] == 0.f), none.iterations);

    // ---- end to end: the search, then alignTeaser
    const int m = 40, sh = 5;
    auto s2 = std::make_shared<PointNCloud>(), t2 = std::make_shared<PointNCloud>();
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            const float s[3][3] = {{2.f * i, 2.f * j, 0}, {sh + 2.f * i, 0, sh + 2.f * j}, {0, 2.f * sh + 2.f * i, 2.f * sh + 2.f * j}};
            for (int k = 0; k < 3; ++k) {
                float q[3], t[3];
                for (int a = 0; a < 3; ++a) { q[a] = s[k][a] + jitter(i, j, 3 * k + a); t[a] = s[k][a] + jitter(i, j, 16 + 3 * k + a); }
                s2->points.emplace_back(cs * q[0] - sn * q[1] + 3.f, sn * q[0] + cs * q[1] - 2.f, q[2] + 1.f, 1.f);
                t2->points.emplace_back(t[0], t[1], t[2], 1.f);
            }
        }
    p.vp_tgt = std::array<float, 3>{80.f, 80.f, 80.f};
    p.vp_src = std::array<float, 3>{80.f, 80.f, 80.f};
    AlignmentResult e2e = alignPointClouds(s2, t2, p);
    FeatureBasedCorrespondenceSearch search(s2, t2, p);
    CorrespondencesPtr found = search.calculateCorrespondences();
    AlignmentResult direct = alignTeaser(s2, t2, found, p);
    std::printf("end_to_end correspondences=%zu converged=%d equal_to_align_teaser=%d iterations=%d\n", found->size(), (int) e2e.converged,
                (int) (std::memcmp(e2e.transformation.data(), direct.transformation.data(), 64) == 0 && e2e.converged == direct.converged), e2e.iterations);

    // ---- what the shim refused for "teaser" before, it still refuses: the measure loop runs through lgr_measure, which knows no teaser
    bool threw = false;
    Matrix4f gt;
    std::memset(gt.data(), 0, 64);
    try { (void) measureAlignment(s2, t2, p, gt, 2); } catch (const std::runtime_error&) { threw = true; }
    std::printf("measure_throws=%d\n", (int) threw);
    return 0;
}
