// A reference-style caller of the debug layer through the shim: a pair written out by tests/test_host_shim_debug.py (binary: n, then
// n x 12 floats for the source and the target; key point indices as n ints; the correspondences, the correct ones and the inliers as
// n x 4 words each; the weights as n floats; T, T_gt as 16 floats each, column-major; distance_thr).  Writes the files of
// generateDebugFiles / compareHypotheses into argv[2] and prints compareOverlaps' numbers and calculateTemperatureMap's counts.
#include <cstdio>

#include "../../lidar-global-registration_amd/host/lgr_io.hpp"

using namespace lgr;

static PointNCloud::Ptr read_cloud(FILE* f) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return nullptr;
    auto c = std::make_shared<PointNCloud>();
    c->points.resize(n);
    if (n && std::fread(c->points.data(), 48, n, f) != (size_t) n) return nullptr;
    return c;
}
template <class T>
static bool read_list(FILE* f, std::vector<T>& v) {
    int n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return false;
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == (size_t) n;
}
static void show(const char* name, float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    std::printf("%s=%08x\n", name, u);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("shim_debug_smoke: built\n"); return 0; }   // compile and link check only (no GPU)
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f);
    auto kp = std::make_shared<std::vector<int>>();
    Correspondences corr, correct, inliers;
    std::vector<float> weights;
    if (!src || !tgt || !read_list(f, *kp) || !read_list(f, corr) || !read_list(f, correct) || !read_list(f, inliers) || !read_list(f, weights)) return 3;
    Matrix4f T, G;
    float thr = 0.f;
    if (std::fread(T.data(), 4, 16, f) != 16 || std::fread(G.data(), 4, 16, f) != 16 || std::fread(&thr, 4, 1, f) != 1) return 5;
    std::fclose(f);

    AlignmentParameters p;
    p.distance_thr = thr;
    p.dir_path = argv[2];
    saveTemperatureMaps(src, tgt, "temperature_gt", p, thr, G);
    saveTemperatureMaps(src, tgt, "temperature", p, thr, T);
    const OverlapComparison oc = compareOverlaps(src, tgt, T, G, p);
    std::printf("count0=%d count1=%d\n", oc.count[0], oc.count[1]);
    show("weighted0", oc.weighted_count[0]); show("weighted1", oc.weighted_count[1]);
    savePointCloudWithCorrespondences(src, kp, corr, correct, inliers, p, G, true);
    savePointCloudWithCorrespondences(tgt, nullptr, corr, correct, inliers, p, Matrix4f::Identity(), false);
    saveColorizedWeights(src, weights, "weights", p, T);
    saveColorizedPointCloud(src, G, COLOR_RED, debugPath(p, "red_src"));

    // calculateTemperatureMap on coloured clouds, one type at a time
    auto cs = std::make_shared<PointColoredNCloud>(), ct = std::make_shared<PointColoredNCloud>();
    PointNCloud moved;
    transformPointCloudWithNormals(*src, moved, T);
    cs->points.resize(src->size()); ct->points.resize(tgt->size());
    for (size_t i = 0; i < src->size(); ++i) copyPoint(moved.points[i], cs->points[i]);
    for (size_t i = 0; i < tgt->size(); ++i) copyPoint(tgt->points[i], ct->points[i]);
    std::vector<float> temps;
    const int nd = calculateTemperatureMap(cs, ct, TemperatureType::Distance, temps, 0.f, thr, thr);
    savePLYFileASCII(debugPath(p, "map_dists_src"), *cs);
    const int nn = calculateTemperatureMap(cs, ct, TemperatureType::NormalDifference, temps, 0.f, (float) M_PI / 2, thr);
    savePLYFileBinary(debugPath(p, "map_normal_diffs_src"), *cs);
    std::printf("below_distance=%d below_normal=%d\n", nd, nn);
    return 0;
}
