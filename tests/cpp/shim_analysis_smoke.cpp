// A reference-style caller of the ground-truth analysis through the shim: a pair written out by tests/test_host_shim_analysis.py (binary:
// n, then n x 12 floats for the source, the target and the source moved by the ground truth; the correspondences as n x 4 words; T, T_gt
// as 16 floats each, column-major; distance_thr).  Prints every figure as its bit pattern for the test to compare with lgr_evaluate_gt on
// the same pair, and writes mergeOverlaps' dst and buildCorrectCorrespondences' output to argv[2] (n, then the rows, each).
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
static void show(const char* name, float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    std::printf("%s=%08x\n", name, u);
}

int main(int argc, char** argv) {
    if (argc < 3) { std::printf("shim_analysis_smoke: built\n"); return 0; }   // compile and link check only (no GPU)
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f), moved = read_cloud(f);
    int c = 0;
    if (!src || !tgt || !moved || std::fread(&c, 4, 1, f) != 1) return 3;
    auto corr = std::make_shared<Correspondences>(c);
    if (c && std::fread(corr->data(), 16, c, f) != (size_t) c) return 4;
    Matrix4f T, G;
    float thr = 0.f;
    if (std::fread(T.data(), 4, 16, f) != 16 || std::fread(G.data(), 4, 16, f) != 16 || std::fread(&thr, 4, 1, f) != 1) return 5;
    std::fclose(f);

    AlignmentParameters p;
    p.distance_thr = thr;
    AlignmentResult r;
    r.src = src; r.tgt = tgt; r.correspondences = corr; r.transformation = T; r.converged = true; r.time_cs = 0.25; r.time_te = 0.5;
    AlignmentAnalysis none(r, p);
    none.start(std::nullopt, "no_gt");   // no ground truth: nothing is computed, the getters give NaN
    show("none_overlap_error", none.getOverlapError());
    AlignmentAnalysis a(r, p);
    a.start(G, "pair");
    std::printf("converged=%d\n", (int) a.alignmentHasConverged());
    show("running_time", a.getRunningTime());
    show("get_r_err", a.getRotationError());
    show("get_t_err", a.getTranslationError());
    show("get_overlap_rmse", a.getOverlapError());
    show("get_pcd_err", a.getPointCloudError());
    const lgr_gt_eval& e = a.evaluation();
    show("r_err", e.r_err); show("t_err", e.t_err); show("pcd_err", e.pcd_err); show("overlap_rmse", e.overlap_rmse);
    show("normal_diff", e.normal_diff); show("overlap", e.overlap); show("overlap_area", e.overlap_area); show("corr_uniformity", e.corr_uniformity);
    std::printf("overlap_size=%d n_normal_overlap=%d n_overlap_src=%d n_overlap_tgt=%d n_correct=%d ok=%d\n", e.overlap_size, e.n_normal_overlap,
                e.n_overlap_src, e.n_overlap_tgt, e.n_correct_correspondences, e.converged_and_overlap_ok);

    show("free_pcd_err", calculatePointCloudRmse(src, T, G));
    show("free_overlap_rmse", calculateOverlapRmse(src, tgt, T, G, thr));
    show("free_normal_diff", calculateNormalDifference(src, tgt, thr, G));
    Correspondences correct;
    buildCorrectCorrespondences(src, tgt, *corr, correct, G);
    auto dst = std::make_shared<PointNCloud>();
    dst->points.resize(3);   // mergeOverlaps clears dst first
    mergeOverlaps(moved, tgt, dst, thr);
    std::printf("free_n_correct=%d free_dst=%d\n", (int) correct.size(), (int) dst->size());

    FILE* o = std::fopen(argv[2], "wb");
    if (!o) return 6;
    int n = (int) dst->size();
    std::fwrite(&n, 4, 1, o);
    std::fwrite(dst->points.data(), 48, n, o);
    n = (int) correct.size();
    std::fwrite(&n, 4, 1, o);
    std::fwrite(correct.data(), 16, n, o);
    std::fclose(o);
    return 0;
}
