// A stand-alone driver of the ICP variants' CPU statement (tests/cpp/icp_ex_ref.cpp + csrc/lgr_icp_math.h) for AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_icp_ex_ref_sanitize.py compiles the two files into one program with -fsanitize=address,undefined
// -fno-sanitize-recover and runs it; any report aborts.  The pair is a small bumpy surface and the same surface moved a little, with NaN
// points, NaN normals on both sides and weights that hold 0, a negative, NaN and inf; every variant x robust kernel runs with the gate
// and the weights on and off, the sizes cross a power of two, and the idle and stopping paths run too.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

struct Step { float T[16]; float dist; int pairs; float rmse, rot, trans; int reserved[3]; };
struct Result { float T[16]; int iterations, stop; float max_dist; int pairs; float rmse; int pairs0; float rmse0; int reserved[5]; };
extern "C" {
int icpexref_inv_sym3(const double* S6, double* M6);
double icpexref_robust_weight(int kind, double rho, double k);
int icpexref_run(const float* src, int ns, const float* tgt, int nt, const float* T0, int max_iterations, float max_dist, float min_dist, float shrink, float rot_eps,
                 float trans_eps, int variant, int robust, float robust_scale, float min_normal_cos, float eps, const float* weights, Result* out, Step* trace);
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
        Result r;
        for (int variant = 0; variant < 3; ++variant)
            for (int robust = 0; robust < 4; ++robust)
                for (int opt = 0; opt < 4; ++opt) {
                    const float k = variant == 2 ? 0.5f : 0.05f;
                    const int ev = icpexref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 8, 0.3f, 0.05f, 0.8f, 1e-6f, 1e-6f, variant, robust, k, opt & 1 ? 0.9f : -1.f,
                                                variant == 2 && robust == 1 ? 0.01f : 1e-3f, opt & 2 ? w.data() : nullptr, &r, trace.data());
                    failures += ev < 1 || ev > 8 || r.pairs0 > n * n || (n == 23 && r.pairs0 < 100);
                    ++runs;
                }
        std::printf("n=%d: last run %d iterations, stop %d, pairs %d -> %d, rmse %g -> %g\n", n * n, r.iterations, r.stop, r.pairs0, r.pairs, r.rmse0, r.rmse);
        failures += icpexref_run(src.data(), 0, tgt.data(), 23 * 23, I4, 8, 0.3f, 0.3f, 1.f, 0.f, 0.f, 2, 3, 1.f, 0.5f, 1e-3f, w.data(), &r, trace.data()) != 0 || r.stop != 2;
        failures += icpexref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 0, 0.3f, 0.3f, 1.f, 0.f, 0.f, 1, 2, 1.f, 0.5f, 1e-3f, w.data(), &r, trace.data()) != 0 || r.stop != 0;
    }
    const double S[6] = {2, 0, 0, 4, 0, 8}, Z[6] = {0, 0, 0, 0, 0, 0};
    double M[6];
    failures += icpexref_inv_sym3(S, M) != 1 || M[0] != 0.5 || M[3] != 0.25 || M[5] != 0.125 || icpexref_inv_sym3(Z, M) != 0;
    failures += icpexref_robust_weight(1, 1.5, 0.75) != 0.5 || icpexref_robust_weight(2, 0.75, 0.75) != 0.5 || icpexref_robust_weight(3, 0.75, 0.75) != 0.0 ||
                icpexref_robust_weight(0, 9.0, 0.75) != 1.0;
    std::printf("icp_ex_ref_sanitize: %d runs, %d failures\n", runs, failures);
    return failures ? 1 : 0;
}
