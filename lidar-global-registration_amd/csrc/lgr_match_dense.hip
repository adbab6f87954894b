// lgr_match_dense.hip -- the dense brute-force matcher of the long descriptors (SHOT352, RoPS135): the exact scan that defines the result,
// and behind lgr_ctx_set_dense_filter the MFMA filter of lgr_match_dense_mfma.cuh, which returns the same bytes.
//
//   include/matching.h matchBF<SHOT> on M x 352 rows                               -> lgr_match_shot*, lgr_match2_shot_dev
//   include/matching.h matchBF<RoPS135> on M x 135 rows                            -> lgr_match_rops*, lgr_match2_rops_dev
// Every (query, train) pair is evaluated with OpenCV's own float sequence, so the result is the reference's bit for bit and does not
// depend on scheduling.  The 33-d FPFH matcher is lgr_match.hip.
#include <cfloat>
#include <algorithm>

#include "lgr_host.h"
#include "lgr_match_dense.cuh"

namespace {

// rank of train row j among equal distances: a later bf block first, the lowest index inside a block
__device__ __forceinline__ unsigned dense_tie_rank(int j, int block, int nb) { return (unsigned) (nb - 1 - j / block) * (unsigned) block + (unsigned) (j % block); }

// 256 threads: a 64 x 64 tile, 4 x 4 pairs per thread.  Block (query tile, split): the split's train tiles one after the other.
template <int NB, int TAIL>
__global__ __launch_bounds__(256) void dense_match_kernel(const float* __restrict__ pa, int ma, int mpa, const float* __restrict__ pb, int mb, int mpb,
                                                         int block, int nb_a, int nb_b, int splits, unsigned long long* __restrict__ key_ab,
                                                         unsigned long long* __restrict__ key_ba) {
    __shared__ float4 sa[NB][MT / 4];
    __shared__ float4 sb[NB][MT / 4];
    __shared__ unsigned long long qmin[MT], tmin[MT];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int qt = blockIdx.x / splits, split = blockIdx.x % splits;
    const int q0 = qt * MT;
    if (tid < MT) qmin[tid] = ~0ull;
    const int n_tt = (mb + MT - 1) / MT;
    for (int tt = split; tt < n_tt; tt += splits) {
        const int t0 = tt * MT;
        if (tid < MT) tmin[tid] = ~0ull;
        float d4[4][4];
        dense_tile_distances<NB, TAIL>(pa, mpa, q0, pb, mpb, t0, sa, sb, d4);
        unsigned long long bq[4] = {~0ull, ~0ull, ~0ull, ~0ull}, bt[4] = {~0ull, ~0ull, ~0ull, ~0ull};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int qi = q0 + 4 * ty + i, tj = t0 + 4 * tx + j;
                const float d = d4[i][j];
                if (!(qi < ma && tj < mb && d < FLT_MAX)) continue;   // NaN never enters (batchDistance's strict '<' against FLT_MAX)
                const unsigned long long db = (unsigned long long) __float_as_uint(d) << 32;
                const unsigned long long kq = db | dense_tie_rank(tj, block, nb_b), kt = db | dense_tie_rank(qi, block, nb_a);
                bq[i] = kq < bq[i] ? kq : bq[i];
                bt[j] = kt < bt[j] ? kt : bt[j];
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) if (bq[i] != ~0ull) atomicMin(&qmin[4 * ty + i], bq[i]);
        if (key_ba) {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (bt[j] != ~0ull) atomicMin(&tmin[4 * tx + j], bt[j]);
        }
        __syncthreads();
        if (key_ba && tid < MT && tmin[tid] != ~0ull) atomicMin(&key_ba[t0 + tid], tmin[tid]);
    }
    __syncthreads();
    if (tid < MT && qmin[tid] != ~0ull) atomicMin(&key_ab[q0 + tid], qmin[tid]);
}

__global__ void dense_match_decode(const unsigned long long* __restrict__ keys, int m, int block, int nb, int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const unsigned long long k = keys[i];
    if (k == ~0ull) { idx[i] = -1; dist[i] = 0.f; return; }
    const unsigned r = (unsigned) k;
    const int bi = nb - 1 - (int) (r / (unsigned) block);
    idx[i] = bi * block + (int) (r % (unsigned) block);
    dist[i] = __uint_as_float((unsigned) (k >> 32));
}

// the exact scan on non-empty sides (ba_i == NULL: one direction): pack, one pass over the pair distances, decode
template <int NB, int TAIL>
int dense_exact(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d) {
    constexpr int LEN = 16 * NB + TAIL;
    const bool both = ba_i != nullptr;
    const int mpa = cdiv(ma, MT) * MT, mpb = cdiv(mb, MT) * MT;
    float *pa, *pb;
    unsigned long long* keys;
    LGR_TRY(lgr_ws_t(ctx, WS_DENSE_PACK_A, (size_t) mpa * LEN, &pa));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSE_PACK_B, (size_t) mpb * LEN, &pb));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSE_KEYS, (size_t) mpa + mpb, &keys));
    dense_pack_kernel<NB, TAIL><<<cdiv((long long) mpa * LEN, 256), 256, 0, ctx->stream>>>(d_a, ma, mpa, pa);
    dense_pack_kernel<NB, TAIL><<<cdiv((long long) mpb * LEN, 256), 256, 0, ctx->stream>>>(d_b, mb, mpb, pb);
    LGR_HIP(ctx, hipMemsetAsync(keys, 0xff, ((size_t) mpa + mpb) * 8, ctx->stream));
    const int nb_a = cdiv(ma, block), nb_b = cdiv(mb, block);
    const int n_qt = mpa / MT, n_tt = mpb / MT;
    const int splits = std::max(1, std::min(n_tt, cdiv(8 * ctx->n_cu, n_qt)));
    dense_match_kernel<NB, TAIL><<<n_qt * splits, 256, 0, ctx->stream>>>(pa, ma, mpa, pb, mb, mpb, block, nb_a, nb_b, splits, keys, both ? keys + mpa : nullptr);
    dense_match_decode<<<cdiv(ma, 256), 256, 0, ctx->stream>>>(keys, ma, block, nb_b, ab_i, ab_d);
    if (both) dense_match_decode<<<cdiv(mb, 256), 256, 0, ctx->stream>>>(keys + mpa, mb, block, nb_a, ba_i, ba_d);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

}  // namespace

#include "lgr_match_dense_mfma.cuh"

namespace {

// lgr_ctx_set_dense_filter: the filtered path, or the exact scan with the reason in densef_last[7]
template <int NB, int TAIL>
int dense_match(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d) {
    const unsigned long long fresh[8] = {0, 0, 0, 0, 0, 0, ~0ull, 0};
    memcpy(ctx->densef_last, fresh, sizeof fresh);
    ctx->densef_worst = -1;
    LGR_CHECK(ctx, (d_a || ma == 0) && (d_b || mb == 0) && ma >= 0 && mb >= 0 && block > 0 && (ab_i || ma == 0) && (ab_d || ma == 0), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const bool both = ba_i != nullptr;
    const bool want = ctx->densef_mode == 1 || (ctx->densef_mode == -1 && (long long) ma * mb >= DENSEF_AUTO_MIN_PAIRS);
    if (ma == 0 || mb == 0) {
        if (want) ctx->densef_last[7] = DENSEF_REASON_EMPTY;
        if (ma) { LGR_HIP(ctx, hipMemsetAsync(ab_i, 0xff, (size_t) ma * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(ab_d, 0, (size_t) ma * 4, ctx->stream)); }
        if (mb && both) { LGR_HIP(ctx, hipMemsetAsync(ba_i, 0xff, (size_t) mb * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(ba_d, 0, (size_t) mb * 4, ctx->stream)); }
        return LGR_OK;
    }
    if (want) {
        bool done = false;
        LGR_TRY((densef_match<NB, TAIL>(ctx, d_a, ma, d_b, mb, block, ab_i, ab_d, ba_i, ba_d, &done)));
        if (done) return LGR_OK;
    }
    LGR_TRY((dense_exact<NB, TAIL>(ctx, d_a, ma, d_b, mb, block, ab_i, ab_d, ba_i, ba_d)));
    ctx->densef_last[1] = (unsigned long long) ma * mb; ctx->densef_last[3] = (unsigned long long) ma + (both ? mb : 0);
    return LGR_OK;
}

// the shapes of a public entry point, by row length: device arrays in one or (both) in two directions; host arrays (upload, match, download)
int match_dev(lgr_ctx* ctx, int row_len, const float* d_a, int ma, const float* d_b, int mb, int block,
              int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist, bool both) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    if (both) LGR_CHECK(ctx, (d_ba_idx && d_ba_dist) || mb == 0, LGR_ERR_INVALID_ARG);
    if (mb == 0) d_ba_idx = nullptr;
    return lgr_match_dense(ctx, row_len, d_a, ma, d_b, mb, block, d_ab_idx, d_ab_dist, d_ba_idx, d_ba_dist);
}

int match_host(lgr_ctx* ctx, int row_len, const float* q, int mq, const float* t, int mt, int block, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (q || mq == 0) && (t || mt == 0) && (idx || mq == 0) && (dist || mq == 0) && mq >= 0 && mt >= 0, LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    float *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q, (size_t) mq * row_len, &dq));
    LGR_TRY(hc.in(t, (size_t) mt * row_len, &dt));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_match_dense(ctx, row_len, dq, mq, dt, mt, block, di, dd, nullptr, nullptr));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}

}  // namespace

int lgr_match_dense(lgr_ctx* ctx, int row_len, const float* d_a, int ma, const float* d_b, int mb, int block,
                    int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d) {
    if (row_len == 352) return dense_match<22, 0>(ctx, d_a, ma, d_b, mb, block, ab_i, ab_d, ba_i, ba_d);
    if (row_len == 135) return dense_match<8, 7>(ctx, d_a, ma, d_b, mb, block, ab_i, ab_d, ba_i, ba_d);
    return lgr_fail(ctx, LGR_ERR_UNSUPPORTED, "row_len == 352 || row_len == 135", __FILE__, __LINE__);
}

static void densef_propagate(lgr_ctx* ctx, int mode, int self_check) {
    ctx->densef_mode = mode; ctx->densef_check = self_check;
    if (ctx->aux) densef_propagate(ctx->aux, mode, self_check);
    if (ctx->aux2) densef_propagate(ctx->aux2, mode, self_check);
}

extern "C" int lgr_ctx_set_dense_filter(lgr_ctx* ctx, int mode, int self_check) {
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, mode >= -1 && mode <= 1 && (self_check == 0 || self_check == 1), LGR_ERR_INVALID_ARG);
    densef_propagate(ctx, mode, self_check);
    return LGR_OK;
}

extern "C" int lgr_ctx_get_dense_filter(lgr_ctx* ctx, int* mode, int* self_check) {
    if (!ctx || !mode || !self_check) return LGR_ERR_INVALID_ARG;
    *mode = ctx->densef_mode; *self_check = ctx->densef_check;
    return LGR_OK;
}

extern "C" int lgr_match_dense_last(lgr_ctx* ctx, unsigned long long* out8) {
    if (!ctx || !out8) return LGR_ERR_INVALID_ARG;
    memcpy(out8, ctx->densef_last, sizeof ctx->densef_last);
    return LGR_OK;
}

extern "C" int lgr_match_dense_last_check(lgr_ctx* ctx, double* worst_ratio) {
    if (!ctx || !worst_ratio) return LGR_ERR_INVALID_ARG;
    *worst_ratio = ctx->densef_worst;
    return LGR_OK;
}

extern "C" int lgr_match_shot_dev(lgr_ctx* ctx, const float* d_q, int mq, const float* d_t, int mt, int block, int32_t* d_idx, float* d_dist) {
    return match_dev(ctx, 352, d_q, mq, d_t, mt, block, d_idx, d_dist, nullptr, nullptr, false);
}
extern "C" int lgr_match2_shot_dev(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block,
                                   int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist) {
    return match_dev(ctx, 352, d_a, ma, d_b, mb, block, d_ab_idx, d_ab_dist, d_ba_idx, d_ba_dist, true);
}
extern "C" int lgr_match_shot(lgr_ctx* ctx, const float* q, int mq, const float* t, int mt, int block, int32_t* idx, float* dist) {
    return match_host(ctx, 352, q, mq, t, mt, block, idx, dist);
}
extern "C" int lgr_match_rops_dev(lgr_ctx* ctx, const float* d_q, int mq, const float* d_t, int mt, int block, int32_t* d_idx, float* d_dist) {
    return match_dev(ctx, 135, d_q, mq, d_t, mt, block, d_idx, d_dist, nullptr, nullptr, false);
}
extern "C" int lgr_match2_rops_dev(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block,
                                   int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist) {
    return match_dev(ctx, 135, d_a, ma, d_b, mb, block, d_ab_idx, d_ab_dist, d_ba_idx, d_ba_dist, true);
}
extern "C" int lgr_match_rops(lgr_ctx* ctx, const float* q, int mq, const float* t, int mt, int block, int32_t* idx, float* dist) {
    return match_host(ctx, 135, q, mq, t, mt, block, idx, dist);
}
