// A stand-alone driver of the trimmed ICP's CPU statement (tests/cpp/icp_trim_ref.cpp, which includes icp_ex_ref.cpp, + csrc/lgr_icp_math.h)
// for AddressSanitizer and UndefinedBehaviorSanitizer: tests/test_icp_trim_ref_sanitize.py compiles the two files into one program with
// -fsanitize=address,undefined -fno-sanitize-recover and runs it; any report aborts.  The pair is the bumpy surface of
// icp_ex_ref_sanitize.cpp with NaN points, NaN normals and weights that hold 0, a negative, NaN and inf; every variant x robust kernel runs
// trimmed, median-scaled and both, the sizes cross a power of two and reach P = 0, 1 and K = 0, and the neutral and idle paths run too.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

struct Step { float T[16]; float dist; int pairs; float rmse, rot, trans; int reserved[3]; };
struct Result { float T[16]; int iterations, stop; float max_dist; int pairs; float rmse; int pairs0; float rmse0; int reserved[5]; };
struct TrimStep { int candidates, kept; float cut, scale; };
extern "C" {
long long icptrimref_k(float keep, long long P);
long long icptrimref_median_rank(long long P);
double icptrimref_scale(float scale_from_median, float key_median, float robust_scale);
double icptrimref_weight(int kind, double rho, double k);
int icptrimref_key(double rho, unsigned* bits);
int icptrimref_run(const float* src, int ns, const float* tgt, int nt, const float* T0, int max_iterations, float max_dist, float min_dist, float shrink, float rot_eps,
                   float trans_eps, int variant, int robust, float robust_scale, float min_normal_cos, float eps, const float* weights, float keep,
                   float scale_from_median, Result* out, Step* trace, TrimStep* info);
}

static std::vector<float> surface(int n, float dx, float dz) {
    std::vector<float> c((size_t) n * n * 12, 0.f);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            float* p = &c[((size_t) i * n + j) * 12];
            const float x = 0.1f * i + dx, y = 0.1f * j;
            const float fx = 0.3f * std::cos(3.f * x), fy = -0.2f * std::sin(2.f * y), len = std::sqrt(fx * fx + fy * fy + 1.f);
            p[0] = x; p[1] = y; p[2] = 0.1f * std::sin(3.f * x) + 0.1f * std::cos(2.f * y) + dz; p[3] = 1.f;
            p[4] = -fx / len; p[5] = -fy / len; p[6] = 1.f / len;
        }
    return c;
}

int main() {
    int failures = 0, runs = 0;
    const float I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int n : {1, 3, 8, 9, 23}) {
        std::vector<float> src = surface(n, 0.02f, 0.01f), tgt = surface(23, 0.f, 0.f), w((size_t) n * n, 0.75f);
        if (n > 3) {
            src[12] = NAN; src[2 * 12 + 5] = NAN; tgt[4 * 12 + 5] = NAN; tgt[7 * 12] = NAN;
            w[3] = 0.f; w[4] = -1.f; w[5] = NAN; w[6] = INFINITY;
        }
        std::vector<Step> trace(8);
        std::vector<TrimStep> info(8);
        Result r;
        for (int variant = 0; variant < 3; ++variant)
            for (int robust = 0; robust < 4; ++robust)
                for (int opt = 0; opt < 4; ++opt)
                    for (int mode = 0; mode < 3; ++mode) {   // trimmed, median-scaled, both
                        if (robust == 0 && mode > 0) continue;
                        const float keep = mode == 1 ? 1.f : 0.7f, mult = mode == 0 ? 0.f : 1.4826f;
                        const int ev = icptrimref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 8, 0.3f, 0.05f, 0.8f, 1e-6f, 1e-6f, variant, robust,
                                                      variant == 2 ? 0.5f : 0.05f, opt & 1 ? 0.9f : -1.f, 1e-3f, opt & 2 ? w.data() : nullptr, keep, mult, &r, trace.data(),
                                                      info.data());
                        failures += ev < 1 || ev > 8 || r.pairs0 > n * n || info[0].candidates > n * n || info[0].kept != icptrimref_k(keep, info[0].candidates) ||
                                    r.pairs0 > info[0].kept || (n == 23 && r.pairs0 < 50);
                        ++runs;
                    }
        std::printf("n=%d: last run %d iterations, stop %d, pairs %d -> %d, candidates %d kept %d cut %g scale %g\n", n * n, r.iterations, r.stop, r.pairs0, r.pairs,
                    info[0].candidates, info[0].kept, info[0].cut, info[0].scale);
        // K = 0, the neutral call, the idle calls
        failures += icptrimref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 8, 0.3f, 0.3f, 1.f, 0.f, 0.f, 0, 0, 0.f, -1.f, 1e-3f, nullptr, 1e-4f, 0.f, &r, trace.data(),
                                   info.data()) != 1 || r.stop != 2 || info[0].kept != 0 || info[0].cut != 0.f;
        failures += icptrimref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 3, 0.3f, 0.3f, 1.f, 0.f, 0.f, 1, 2, 0.05f, -1.f, 1e-3f, nullptr, 1.f, 0.f, &r, trace.data(),
                                   info.data()) < 1 || info[0].candidates != trace[0].pairs || info[0].scale != 0.05f;
        failures += icptrimref_run(src.data(), 0, tgt.data(), 23 * 23, I4, 8, 0.3f, 0.3f, 1.f, 0.f, 0.f, 2, 3, 1.f, 0.5f, 1e-3f, w.data(), 0.5f, 2.f, &r, trace.data(),
                                   info.data()) != 0 || r.stop != 2;
        failures += icptrimref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 0, 0.3f, 0.3f, 1.f, 0.f, 0.f, 1, 2, 1.f, 0.5f, 1e-3f, w.data(), 0.5f, 2.f, &r, trace.data(),
                                   info.data()) != 0 || r.stop != 0;
    }
    unsigned bits = 7;
    failures += icptrimref_k(0.9f, 2069) != 1862 || icptrimref_k(1.f, 5) != 5 || icptrimref_k(0.5f, 1) != 0 || icptrimref_median_rank(1) != 0 || icptrimref_median_rank(4) != 1;
    failures += icptrimref_scale(2.f, 3.f, 9.f) != 6.0 || icptrimref_scale(0.f, 3.f, 9.f) != 9.0 || icptrimref_weight(3, 5.0, 0.0) != 1.0 || icptrimref_weight(3, 5.0, 1.0) != 0.0;
    failures += icptrimref_key(1.0, &bits) != 1 || bits != 0x3f800000u || icptrimref_key(NAN, &bits) != 0 || icptrimref_key(-1.0, &bits) != 0 || icptrimref_key(1e300, &bits) != 0;
    std::printf("icp_trim_ref_sanitize: %d runs, %d failures\n", runs, failures);
    return failures ? 1 : 0;
}
