// lgr_hypotheses.hip -- the set of distinct hypotheses on the device: the left fold of updateHypotheses (src/hypotheses.cpp:14-48) over a
// list of (transform, metric) items in the caller's order.  The reference folds inside the RANSAC loop when SAVE_MULTIPLE_HYPOTHESES is set
// (src/sac_prerejective_omp.cpp:11, call sites :143, :230, :261); here the loop's items arrive in rounds (lgr_ransac_multi_dev,
// lgr_ransac.hip) and the set carries over between the launches in global memory.
//
// The fold is order-dependent, so ONE workgroup consumes the items strictly in order; what is parallel is the work per item: the lanes
// stride over the members of the set, which lives in LDS (12 floats of R|t, the metric and the source index per member, structure of
// arrays: LGR_HYPOTHESES_MAX = 2048 members are 112 KB of the 160 KB).  Per item:
//   early-out     new < 0.1 * best (best = the largest metric in the set: every accepted item raises it or leaves it, erased and pruned
//                 members are never above it)
//   similarity    calculateRotationAndTranslationDifferences (src/analysis.cpp:19-24) against every member in double, orc_rot_trans_diff's
//                 operation sequence; similar = angle < pi / 9 and distance < 20 * distance_thr on the values rounded to float
//   blocked       a similar member with a GREATER metric exists (workgroup-wide OR): the item is dropped
//   otherwise     one order-preserving compaction drops the similar members and -- when the item is a new best -- the members below
//                 0.1 * new (the reference erases, appends, then prunes: the appended item is never pruned and stays last, so pruning
//                 before the append leaves the same members in the same order), then the item is appended.
// atan2 / sqrt are the device's double-precision routines, the oracle's are libm's: both within an ulp, and the decision reads the result
// rounded to float.
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "lgr_host.h"
#include "lgr_internal.h"

namespace {

constexpr int FB = 1024;          // threads of the fold's one workgroup
constexpr int FOLD_FLOATS = 14;   // LDS words per member: R|t, metric, source index

__device__ __forceinline__ int fold_excl_scan(int v, int* scan /* [FB / 64 + 1] */, int tid, int* total) {
    const int lane = tid & 63, w = tid >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
    if (lane == 63) scan[w] = x;
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int i = 0; i < FB / 64; ++i) { const int t = scan[i]; scan[i] = acc; acc += t; } scan[FB / 64] = acc; }
    __syncthreads();
    const int base = scan[w];
    *total = scan[FB / 64];
    __syncthreads();
    return base + x - v;
}

// is member b "similar" to the new transform a (both 12 floats: R column-major, then t)?
__device__ __forceinline__ bool fold_similar(const float* a, const float* b, float t_thr) {
    double R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += (double) a[3 * i + k] * (double) b[3 * j + k];   // (R1^T R2)_ij
            R[3 * i + j] = s;
        }
    const double tr = R[0] + R[4] + R[8];
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double sn = 0.5 * sqrt(vx * vx + vy * vy + vz * vz), cs = 0.5 * (tr - 1.0);
    const float angle = (float) atan2(sn, cs);
    const double dx = (double) a[9] - b[9], dy = (double) a[10] - b[10], dz = (double) a[11] - b[11];
    const float td = (float) sqrt(dx * dx + dy * dy + dz * dz);
    return (double) angle < (M_PI / 9) && td < t_thr;
}

__global__ __launch_bounds__(FB) void fold_kernel(const float* __restrict__ T16, const float* __restrict__ metric, const int32_t* __restrict__ index,
                                                  int index_base, int n_host, const int* __restrict__ n_dev, float distance_thr, int cap,
                                                  float* __restrict__ set_rt, float* __restrict__ set_m, int32_t* __restrict__ set_idx,
                                                  lgr_fold_state* __restrict__ st) {
    extern __shared__ float lds[];   // [FOLD_FLOATS][cap]: field f of member k at lds[f * cap + k]
    __shared__ int scan[FB / 64 + 2];
    const int tid = threadIdx.x;
    if (st->overflow) return;
    int n_set = st->n, peak = st->peak;
    float best = st->best;
    const int n = n_dev ? min(n_dev[0], n_host) : n_host;
    float* const lm = lds + 12 * cap;
    int* const li = reinterpret_cast<int*>(lds + 13 * cap);
    for (int k = tid; k < n_set; k += FB) {
#pragma unroll
        for (int f = 0; f < 12; ++f) lds[f * cap + k] = set_rt[(size_t) k * 12 + f];
        lm[k] = set_m[k];
        li[k] = set_idx[k];
    }
    __syncthreads();
    const float t_thr = 20 * distance_thr;
    bool overflow = false;
    for (int i = 0; i < n; ++i) {
        const float m = metric[i];
        if ((double) m < 0.1 * (double) best) continue;
        float a[12];
        {
            const float* T = T16 + (size_t) i * 16;
#pragma unroll
            for (int col = 0; col < 4; ++col)
#pragma unroll
                for (int r = 0; r < 3; ++r) a[3 * col + r] = T[4 * col + r];
        }
        unsigned sim = 0u;
        int blocked = 0;
        for (int k = tid, q = 0; k < n_set; k += FB, ++q) {
            float b[12];
#pragma unroll
            for (int f = 0; f < 12; ++f) b[f] = lds[f * cap + k];
            if (fold_similar(a, b, t_thr)) {
                sim |= 1u << q;
                if (lm[k] > m) blocked = 1;
            }
        }
        if (__syncthreads_or(blocked)) continue;
        const bool new_best = m > best;
        unsigned drop = sim;
        if (new_best)
            for (int k = tid, q = 0; k < n_set; k += FB, ++q)
                if ((double) lm[k] < 0.1 * (double) m) drop |= 1u << q;
        if (__syncthreads_or(drop != 0u)) {
            // in place, chunk by chunk in ascending order: a member only moves down, and the scan's barriers stand between a chunk's reads and its writes
            int total = 0;
            for (int k0 = 0, q = 0; k0 < n_set; k0 += FB, ++q) {
                const int k = k0 + tid;
                const bool keep = k < n_set && !((drop >> q) & 1u);
                float v[12], vm = 0.f;
                int vi = 0;
                if (keep) {
#pragma unroll
                    for (int f = 0; f < 12; ++f) v[f] = lds[f * cap + k];
                    vm = lm[k]; vi = li[k];
                }
                int tot;
                const int pos = total + fold_excl_scan(keep ? 1 : 0, scan, tid, &tot);
                if (keep && pos != k) {
#pragma unroll
                    for (int f = 0; f < 12; ++f) lds[f * cap + pos] = v[f];
                    lm[pos] = vm; li[pos] = vi;
                }
                total += tot;
            }
            n_set = total;
        }
        if (n_set >= cap) { overflow = true; break; }   // (uniform: the set never leaves the kernel truncated)
        if (tid == 0) {
#pragma unroll
            for (int f = 0; f < 12; ++f) lds[f * cap + n_set] = a[f];
            lm[n_set] = m;
            li[n_set] = index ? index[i] : index_base + i;
        }
        n_set += 1;
        if (new_best) best = m;
        peak = max(peak, n_set);
        __syncthreads();
    }
    if (overflow) {
        if (tid == 0) st->overflow = 1;
        return;
    }
    for (int k = tid; k < n_set; k += FB) {
#pragma unroll
        for (int f = 0; f < 12; ++f) set_rt[(size_t) k * 12 + f] = lds[f * cap + k];
        set_m[k] = lm[k];
        set_idx[k] = li[k];
    }
    if (tid == 0) { st->n = n_set; st->best = best; st->peak = peak; }
}

// the set as the caller of lgr_fold_hypotheses* sees it: the members' own 16 floats out of the item list
__global__ void fold_gather_kernel(const float* __restrict__ T16, const lgr_fold_state* __restrict__ st, const float* __restrict__ set_m,
                                   const int32_t* __restrict__ set_idx, float* __restrict__ out_T16, float* __restrict__ out_m, int32_t* __restrict__ out_idx) {
    const int n = st->overflow ? 0 : st->n;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * 16; e += gridDim.x * blockDim.x) {
        const int k = e >> 4, f = e & 15;
        out_T16[e] = T16[(size_t) set_idx[k] * 16 + f];
        if (f == 0) { out_m[k] = set_m[k]; out_idx[k] = set_idx[k]; }
    }
}

}  // namespace

int lgr_fold_begin(lgr_ctx* ctx, int cap, lgr_fold_set* out) {
    LGR_CHECK(ctx, cap >= 1 && cap <= LGR_HYPOTHESES_MAX, LGR_ERR_INVALID_ARG);
    float* p;
    LGR_TRY(lgr_ws_t(ctx, WS_HYP_SET, (size_t) FOLD_FLOATS * cap + 16, &p));
    out->state = (lgr_fold_state*) p;
    out->rt = p + 16; out->metric = out->rt + (size_t) 12 * cap; out->index = (int32_t*) (out->metric + cap);
    out->cap = cap;
    LGR_HIP(ctx, hipMemsetAsync(out->state, 0, sizeof(lgr_fold_state), ctx->stream));
    return LGR_OK;
}

int lgr_fold_launch(lgr_ctx* ctx, const lgr_fold_set& set, const float* d_T16, const float* d_metric, const int32_t* d_index, int index_base, int n,
                    const int* d_n, float distance_thr) {
    if (n <= 0) return LGR_OK;
    const size_t smem = (size_t) FOLD_FLOATS * set.cap * sizeof(float);
    LGR_HIP(ctx, hipFuncSetAttribute((const void*) fold_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) smem));
    fold_kernel<<<1, FB, smem, ctx->stream>>>(d_T16, d_metric, d_index, index_base, n, d_n, distance_thr, set.cap, set.rt, set.metric, set.index, set.state);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// src/hypotheses.cpp:14-48 updateHypotheses folded over n items in the caller's order (the call sites src/sac_prerejective_omp.cpp:143,
// :230, :261 fold the loop's hypotheses one by one)
extern "C" int lgr_fold_hypotheses_dev(lgr_ctx* ctx, const float* d_tns16, const float* d_metrics, int n, float distance_thr, int max_set,
                                       float* d_set_tns16, float* d_set_metrics, int32_t* d_set_index, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, max_set >= 1 && max_set <= LGR_HYPOTHESES_MAX, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, n >= 0 && ((d_tns16 && d_metrics) || n == 0) && d_set_tns16 && d_set_metrics && d_set_index && n_out, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    *n_out = 0;
    if (n == 0) return LGR_OK;
    lgr_fold_set set;
    LGR_TRY(lgr_fold_begin(ctx, max_set, &set));
    LGR_TRY(lgr_fold_launch(ctx, set, d_tns16, d_metrics, nullptr, 0, n, nullptr, distance_thr));
    fold_gather_kernel<<<cdiv((long long) max_set * 16, 256), 256, 0, ctx->stream>>>(d_tns16, set.state, set.metric, set.index, d_set_tns16, d_set_metrics, d_set_index);
    LGR_HIP(ctx, hipGetLastError());
    lgr_fold_state* h;
    LGR_TRY(lgr_pinned(ctx, 64, (void**) &h));
    LGR_HIP(ctx, hipMemcpyAsync(h, set.state, sizeof(lgr_fold_state), hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h->overflow) return lgr_fail(ctx, LGR_ERR_UNSUPPORTED, "the set of hypotheses outgrew max_set during the fold (a truncated set is never returned)", __FILE__, __LINE__);
    *n_out = h->n;
    return LGR_OK;
}

extern "C" int lgr_fold_hypotheses(lgr_ctx* ctx, const float* tns16, const float* metrics, int n, float distance_thr, int max_set,
                                   float* set_tns16, float* set_metrics, int32_t* set_index, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, max_set >= 1 && max_set <= LGR_HYPOTHESES_MAX, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, n >= 0 && ((tns16 && metrics) || n == 0) && set_tns16 && set_metrics && set_index && n_out, LGR_ERR_INVALID_ARG);
    float *dT, *dM, *dO, *dOm;
    int32_t* dOi;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(tns16, (size_t) n * 16, &dT));
    LGR_TRY(hc.in(metrics, (size_t) n, &dM));
    LGR_TRY(hc.out((size_t) max_set * 16, &dO));
    LGR_TRY(hc.out((size_t) max_set, &dOm));
    LGR_TRY(hc.out((size_t) max_set, &dOi));
    LGR_TRY(lgr_fold_hypotheses_dev(ctx, dT, dM, n, distance_thr, max_set, dO, dOm, dOi, n_out));
    if (*n_out) {
        LGR_TRY(hc.fetch(set_tns16, dO, (size_t) *n_out * 16));
        LGR_TRY(hc.fetch(set_metrics, dOm, (size_t) *n_out));
        LGR_TRY(hc.fetch(set_index, dOi, (size_t) *n_out));
        LGR_TRY(hc.finish());
    }
    return LGR_OK;
}

// src/hypotheses.cpp:14-48 updateHypotheses: pure host bookkeeping (the call sites are compiled out in the reference,
// SAVE_MULTIPLE_HYPOTHESES false, src/sac_prerejective_omp.cpp:11); tns16 = n column-major 4x4, capacity cap.
extern "C" int lgr_update_hypotheses(float* tns16, float* metrics, int n, int cap, const float* new_T16, float new_metric, float distance_thr) {
    if (!tns16 || !metrics || !new_T16 || n < 0 || cap < n) return LGR_ERR_INVALID_ARG;
    auto diff = [](const float* T1, const float* T2, float& angle, float& td) {
        // src/analysis.cpp:19-24: angle of R1^-1 R2, |t1 - t2|
        double R[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                double s = 0;
                for (int k = 0; k < 3; ++k) s += (double) T1[4 * i + k] * (double) T2[4 * j + k];
                R[3 * i + j] = s;
            }
        double tr = R[0] + R[4] + R[8];
        double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
        angle = (float) std::atan2(0.5 * std::sqrt(vx * vx + vy * vy + vz * vz), 0.5 * (tr - 1.0));
        double dx = (double) T1[12] - T2[12], dy = (double) T1[13] - T2[13], dz = (double) T1[14] - T2[14];
        td = (float) std::sqrt(dx * dx + dy * dy + dz * dz);
    };
    std::vector<std::vector<float>> T(n, std::vector<float>(16));
    std::vector<float> M(metrics, metrics + n);
    for (int i = 0; i < n; ++i) memcpy(T[i].data(), tns16 + 16 * (size_t) i, 64);
    float best = n == 0 ? 0.f : *std::max_element(M.begin(), M.end());
    auto flush = [&]() {
        int m = (int) T.size();
        if (m > cap) return (int) LGR_ERR_INVALID_ARG;
        for (int i = 0; i < m; ++i) { memcpy(tns16 + 16 * (size_t) i, T[i].data(), 64); metrics[i] = M[i]; }
        return m;
    };
    if (new_metric < 0.1 * best) return flush();
    std::vector<int> similar;
    for (int i = (int) T.size() - 1; i >= 0; --i) {
        float r, t;
        diff(new_T16, T[i].data(), r, t);
        bool is_similar = r < (M_PI / 9) && t < 20 * distance_thr;
        if (is_similar) similar.push_back(i);
        if (is_similar && M[i] > new_metric) return flush();
    }
    for (int idx : similar) { T.erase(T.begin() + idx); M.erase(M.begin() + idx); }
    T.emplace_back(new_T16, new_T16 + 16);
    M.push_back(new_metric);
    if (new_metric > best)
        for (int i = (int) T.size() - 1; i >= 0; --i)
            if (M[i] < 0.1 * new_metric) { T.erase(T.begin() + i); M.erase(M.begin() + i); }
    return flush();
}
