// A reference-style caller of the measure test type through the shim: a pair written out by tests/test_host_shim_measure.py (binary: n, then
// n x 12 floats for the source and the target; the ground truth as 16 floats, column-major; distance_thr; the two view points).  It runs
// measureAlignment for the seeds on the command line and prints the aggregate and every run's figures as bit patterns for the test to compare
// with the C ABI on the same pair.  Without arguments: the two aggregate templates on known lists (no GPU needed).
#include <cstdio>
#include <cstdlib>

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
    // the aggregates: a double sum for the mean (2^24 + 1 + 1 over 3 is 5592406, a float sum would give 5592405.5), a float sum for the
    // deviation (2^25 swallows the six ones: 2048, a double sum would give the float after it), quiet NaN for an empty list
    if (calculateMean<float>({16777216.f, 1.f, 1.f}) != 5592406.f) return 1;
    if (calculateStandardDeviation<float>({4096.f, -4096.f, 1.f, -1.f, 1.f, -1.f, 1.f, -1.f}) != 2048.f) return 1;
    if (calculateStandardDeviation<float>({1.f, 3.f}) != 1.f) return 1;
    const float e = calculateMean<float>({}), s = calculateStandardDeviation<float>({});
    if (e == e || s == s) return 1;
    if (sizeof(lgr_measurement) != 64 || LGR_GT_BATCH_MAX != 64) return 1;
    if (argc < 4) { std::printf("shim_measure_smoke: built\n"); return 0; }   // compile and link check only
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    auto src = read_cloud(f), tgt = read_cloud(f);
    Matrix4f G;
    float thr = 0.f;
    std::array<float, 3> vp_src, vp_tgt;
    if (!src || !tgt || std::fread(G.data(), 4, 16, f) != 16 || std::fread(&thr, 4, 1, f) != 1 || std::fread(vp_src.data(), 4, 3, f) != 3 ||
        std::fread(vp_tgt.data(), 4, 3, f) != 3)
        return 3;
    std::fclose(f);
    AlignmentParameters p;
    p.descriptor_id = "fpfh"; p.keypoint_id = "any"; p.matching_id = "one_sided"; p.metric_id = "uniformity"; p.score_id = "mse";
    p.bf_block_size = 200000; p.distance_thr = thr; p.max_iterations = std::atoi(argv[2]);
    p.feature_radius = 0.25f;   // single scale: the ABI's default radius
    p.vp_src = vp_src; p.vp_tgt = vp_tgt;
    std::vector<uint64_t> seeds;
    for (int k = 3; k < argc; ++k) seeds.push_back(std::strtoull(argv[k], nullptr, 10));
    const MeasurementResult r = measureAlignment(src, tgt, p, G, (int) seeds.size(), seeds);
    const lgr_measurement& m = r.measurement;
    if ((int) r.runs.size() != m.n_times) return 4;
    std::printf("n_times=%d n_success=%d\n", m.n_times, m.n_success);
    std::printf("success_rate=%08x mae=%08x sae=%08x mte=%08x ste=%08x mrmse=%08x srmse=%08x\n", word(m.success_rate), word(m.mae), word(m.sae), word(m.mte),
                word(m.ste), word(m.mrmse), word(m.srmse));
    // the same aggregates through the templates, over the runs' own lists
    std::vector<float> ok_r, times;
    for (const lgr_measure_run& run : r.runs) {
        if (run.eval.converged_and_overlap_ok) ok_r.push_back(run.eval.r_err);
        times.push_back((float) (run.result.time_cs + run.result.time_te));
    }
    const float mae = calculateMean(ok_r), sae = calculateStandardDeviation(ok_r), mtime = calculateMean(times), stime = calculateStandardDeviation(times);
    if (word(mae) != word(m.mae) && !(mae != mae && m.mae != m.mae)) return 5;
    if (word(sae) != word(m.sae) && !(sae != sae && m.sae != m.sae)) return 5;
    if (word(mtime) != word(m.mtime) || word(stime) != word(m.stime)) return 5;
    for (size_t i = 0; i < r.runs.size(); ++i) {
        const lgr_measure_run& run = r.runs[i];
        std::printf("run%zu_seed=%llu run%zu_converged=%d run%zu_ok=%d run%zu_inliers=%d run%zu_r_err=%08x run%zu_overlap_rmse=%08x run%zu_T=", i,
                    (unsigned long long) run.seed, i, run.result.converged, i, run.eval.converged_and_overlap_ok, i, run.result.n_inliers, i,
                    word(run.eval.r_err), i, word(run.eval.overlap_rmse), i);
        for (int k = 0; k < 16; ++k) std::printf("%08x", word(run.result.transformation[k]));
        std::printf("\n");
    }
    return 0;
}
