// A stand-alone driver of the ICP's CPU statement (tests/cpp/icp_ref.cpp + csrc/lgr_icp_math.h) for AddressSanitizer and
// UndefinedBehaviorSanitizer: tests/test_icp_ref_sanitize.py compiles the two files into one program with -fsanitize=address,undefined
// -fno-sanitize-recover and runs it; any report aborts.  The pair is a small bumpy surface and the same surface moved a little, with NaN
// points and normals mixed in; the sizes cross a power of two, and the idle and stopping paths run too.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

struct Step { float T[16]; float dist; int pairs; float rmse, rot, trans; int reserved[3]; };
struct Result { float T[16]; int iterations, stop; float max_dist; int pairs; float rmse; int pairs0; float rmse0; int reserved[5]; };
extern "C" {
double icpref_tree_sum(const double* x, long long n);
int icpref_solve(const double* s27, double* xi6);
void icpref_rotation(const double* w3, double* R9);
int icpref_run(const float* src, int ns, const float* tgt, int nt, const float* T0, int max_iterations, float max_dist, float min_dist, float shrink, float rot_eps,
               float trans_eps, Result* out, Step* trace);
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
    int failures = 0;
    const float I4[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int n : {1, 3, 8, 9, 23}) {
        std::vector<float> src = surface(n, 0.02f, 0.01f), tgt = surface(23, 0.f, 0.f);
        if (n > 3) { src[12] = NAN; tgt[4 * 12 + 5] = NAN; tgt[7 * 12] = NAN; }
        std::vector<Step> trace(20);
        Result r;
        const int ev = icpref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 20, 0.3f, 0.05f, 0.8f, 1e-6f, 1e-6f, &r, trace.data());
        std::printf("n=%d: %d evaluated, %d iterations, stop %d, pairs %d -> %d, rmse %g -> %g\n", n * n, ev, r.iterations, r.stop, r.pairs0, r.pairs, r.rmse0, r.rmse);
        failures += ev < 1 || ev > 20 || (n == 23 && !(r.rmse < r.rmse0));
        failures += icpref_run(src.data(), 0, tgt.data(), 23 * 23, I4, 20, 0.3f, 0.3f, 1.f, 0.f, 0.f, &r, trace.data()) != 0 || r.stop != 2;
        failures += icpref_run(src.data(), n * n, tgt.data(), 23 * 23, I4, 0, 0.3f, 0.3f, 1.f, 0.f, 0.f, &r, trace.data()) != 0 || r.stop != 0;
    }
    std::vector<double> x(5000, 0.25);
    failures += icpref_tree_sum(x.data(), 5000) != 1250.0 || icpref_tree_sum(x.data(), 1) != 0.25;
    double s[28] = {0}, xi[6], w[3] = {0.1, -0.2, 0.3}, R[9];
    failures += icpref_solve(s, xi) != 0;   // the zero matrix: no pivot
    icpref_rotation(w, R);
    failures += !(std::fabs(R[0] * R[0] + R[3] * R[3] + R[6] * R[6] - 1.0) < 1e-15);
    std::printf("icp_ref_sanitize: %d failures\n", failures);
    return failures ? 1 : 0;
}
