// lgr_match_local.hip -- the two other matchers of match_multiscale's dispatch (include/matching.h:294-312) for gfx950:
//
//   matchFLANN<FPFH> (:565-592)  exact nearest neighbour in descriptor space = the row the brute-force kernel finds; only the
//                                reported distance follows FLANN's L2_Simple order (sequential sum of squares, then sqrt).
//   matchLocal<FPFH> (:637-678)  descriptor nearest neighbour restricted to the train points within match_search_radius of
//                                guess * query point.
//
// matchLocal is a guided refinement step (the caller already has a pose).  lgr_match_local* are lgr_match_local_knn* at (row_len 33,
// k 1): one kernel serves every row length and list length (lgr_match_local_knn.hip; the measurement behind that choice: DESIGN.md
// section 3.1k, profiles/match_local_knn.json).
#include <algorithm>
#include <cmath>

#include "lgr_host.h"
#include "lgr_internal.h"

namespace {

// pcl::L2_Norm_SQR / FLANN L2_Simple: result += diff * diff, sequentially from dimension 0
__device__ __forceinline__ float l2sqr33_seq(const float* q, const float* __restrict__ t) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 33; ++j) { float d = q[j] - t[j]; s += d * d; }
    return s;
}

// distance of the match the brute-force kernel found, in FLANN's order (include/matching.h:586-588: std::sqrt of the squared
// distance nearestKSearch returns)
__global__ void flann_dist_kernel(const float* __restrict__ q33, const float* __restrict__ t33, const int32_t* __restrict__ idx, int mq, float* __restrict__ dist) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mq) return;
    int j = idx[i];
    if (j < 0) { dist[i] = 0.f; return; }
    float q[33];
#pragma unroll
    for (int k = 0; k < 33; ++k) q[k] = q33[(size_t) i * 33 + k];
    dist[i] = __builtin_sqrtf(l2sqr33_seq(q, t33 + (size_t) j * 33));
}

}  // namespace

extern "C" int lgr_match_flann_dev(lgr_ctx* ctx, const float* d_q33, int mq, const float* d_t33, int mt, int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    // a single train block: the tie rule of the BF kernel is then "lowest index", the oracle's choice for FLANN's unspecified order
    LGR_TRY(lgr_match_bf_dev(ctx, d_q33, mq, d_t33, mt, std::max(mt, 1), d_idx, d_dist));
    if (mq > 0 && mt > 0) flann_dist_kernel<<<cdiv(mq, 128), 128, 0, ctx->stream>>>(d_q33, d_t33, d_idx, mq, d_dist);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

extern "C" int lgr_match_local_dev(lgr_ctx* ctx, const float* d_qpts, int mq, const float* d_tpts, int mt, const float* d_q33, const float* d_t33,
                                   const float guess16[16], float radius, int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return lgr_match_local_knn_dev(ctx, 33, d_qpts, mq, d_tpts, mt, d_q33, d_t33, guess16, radius, 1, d_idx, d_dist);
}

extern "C" int lgr_match_flann(lgr_ctx* ctx, const float* q33, int mq, const float* t33, int mt, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (q33 || mq == 0) && (t33 || mt == 0) && (idx || mq == 0) && (dist || mq == 0) && mq >= 0 && mt >= 0, LGR_ERR_INVALID_ARG);
    float *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q33, (size_t) mq * 33, &dq));
    LGR_TRY(hc.in(t33, (size_t) mt * 33, &dt));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_match_flann_dev(ctx, dq, mq, dt, mt, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}

extern "C" int lgr_match_local(lgr_ctx* ctx, const float* qpts, int mq, const float* tpts, int mt, const float* q33, const float* t33,
                               const float guess16[16], float radius, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (qpts || mq == 0) && (tpts || mt == 0) && (q33 || mq == 0) && (t33 || mt == 0) && (idx || mq == 0) && (dist || mq == 0) &&
                   guess16 && mq >= 0 && mt >= 0, LGR_ERR_INVALID_ARG);
    float *dqp, *dtp, *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q33, (size_t) mq * 33, &dq));
    LGR_TRY(hc.in(t33, (size_t) mt * 33, &dt));
    LGR_TRY(hc.in(qpts, (size_t) mq * 12, &dqp));
    LGR_TRY(hc.in(tpts, (size_t) mt * 12, &dtp));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_match_local_dev(ctx, dqp, mq, dtp, mt, dq, dt, guess16, radius, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}
