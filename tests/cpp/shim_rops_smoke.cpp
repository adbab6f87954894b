// A reference-style caller with descriptor_id "rops" on gravity frames (the frames of the reference's own test job, data/tests.yaml):
// the corner scene of tests/point2plane_distance.cpp:29-96, normals with k = 30 towards the view points, alignPointClouds through the
// shim with lrf_id "Gravity" (compared case-insensitively).  Prints the transform's distance from GT, whether "rops" with the default
// frames throws, and sizeof(RoPS135).  Run by tests/test_host_shim_rops.py.
#include <cmath>
#include <cstdio>

#include "../../lidar-global-registration_amd/host/lgr_compat.hpp"

using namespace lgr;

int main(int argc, char**) {
    std::printf("sizeof_rops=%zu\n", sizeof(RoPS135));
    if (argc > 1) return 0;   // layout only (no GPU)
    const double G[4][4] = {{0.0803703, -0.996763, -0.00201846, 1.2143}, {0.996758, 0.080377, -0.00349969, -6.13404},
                            {0.00365057, -0.00173067, 0.999992, -1.17221}, {0, 0, 0, 1}};
    double Gi[3][4];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Gi[r][c] = G[c][r];
        Gi[r][3] = -(G[0][r] * G[0][3] + G[1][r] * G[1][3] + G[2][r] * G[2][3]);
    }
    const int n = 100, shift = 5;
    auto src = std::make_shared<PointNCloud>(), tgt = std::make_shared<PointNCloud>();
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const double s[3][3] = {{2.0 * i, 2.0 * j, 0}, {shift + 2.0 * i, 0, shift + 2.0 * j}, {0, 2.0 * shift + 2.0 * i, 2.0 * shift + 2.0 * j}};
            const double t[3][3] = {{2.0 * i + 1, 2.0 * j, 0}, {shift + 2.0 * i, 0, shift + 2.0 * j + 1}, {0, 2.0 * shift + 2.0 * i + 1, 2.0 * shift + 2.0 * j}};
            for (int k = 0; k < 3; ++k) {
                double q[3];
                for (int r = 0; r < 3; ++r) q[r] = Gi[r][0] * s[k][0] + Gi[r][1] * s[k][1] + Gi[r][2] * s[k][2] + Gi[r][3];
                src->points.emplace_back((float) q[0], (float) q[1], (float) q[2], 1.f);
                tgt->points.emplace_back((float) t[k][0], (float) t[k][1], (float) t[k][2], 1.f);
            }
        }
    AlignmentParameters p;
    p.distance_thr = 1.f; p.iss_radius_src = 1.f; p.iss_radius_tgt = 1.f; p.bf_block_size = 200000; p.alignment_id = "ransac";
    p.keypoint_id = "any"; p.metric_id = "closest_plane"; p.max_iterations = 10000; p.fix_seed = true;
    p.descriptor_id = "rops"; p.lrf_id = "Gravity";
    const float vt = 2.f * n;
    double vs[3];
    for (int r = 0; r < 3; ++r) vs[r] = G[0][r] * (vt - G[0][3]) + G[1][r] * (vt - G[1][3]) + G[2][r] * (vt - G[2][3]);
    p.vp_tgt = std::array<float, 3>{vt, vt, vt};
    p.vp_src = std::array<float, 3>{(float) vs[0], (float) vs[1], (float) vs[2]};
    estimateNormalsPoints(30, src, nullptr, p.vp_src, false);
    estimateNormalsPoints(30, tgt, nullptr, p.vp_tgt, false);
    AlignmentResult r = alignPointClouds(src, tgt, p);
    const Matrix4f& T = r.transformation;
    double rot = 0, tr = 0;
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) rot = std::fmax(rot, std::fabs(T(a, b) - G[a][b]));
        tr = std::fmax(tr, std::fabs(T(a, 3) - G[a][3]));
    }
    std::printf("descriptor=rops converged=%d correspondences=%zu rot_err=%g trans_err=%g\n", (int) r.converged, r.correspondences->size(), rot, tr);
    AlignmentParameters pd = p;
    pd.lrf_id = "default";
    bool threw = false;
    try { alignPointClouds(src, tgt, pd); } catch (const std::exception&) { threw = true; }
    std::printf("rops_default threw=%d\n", (int) threw);
    // estimateFeatures<RoPS135> / matchBF<RoPS135> as the reference's call sites use them
    auto down = std::make_shared<PointNCloud>();
    downsamplePointCloud(tgt, down, 1.5f);
    estimateNormalsPoints(30, down, nullptr, p.vp_tgt, false);
    auto f = std::make_shared<RoPS135Cloud>();
    estimateFeatures<RoPS135>(down, down, f, 4.f, p);
    auto m = matchBF<RoPS135>(f, f, p);
    int self = 0;
    for (std::size_t i = 0; i < f->size(); ++i) self += (!m[i].match_indices.empty() && m[i].distances[0] == 0.f) ? 1 : 0;
    std::printf("rops_rows=%zu self_distance_zero=%d\n", f->size(), self);
    return 0;
}
