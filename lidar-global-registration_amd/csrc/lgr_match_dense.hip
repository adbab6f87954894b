// lgr_match_dense.hip -- the exact dense brute-force matcher of the long descriptors (SHOT352, RoPS135).
//
//   include/matching.h matchBF<SHOT> on M x 352 rows                               -> lgr_match_shot*, lgr_match2_shot_dev
//   include/matching.h matchBF<RoPS135> on M x 135 rows                            -> lgr_match_rops*, lgr_match2_rops_dev
// Every (query, train) pair is evaluated with OpenCV's own float sequence, so the result is the reference's bit for bit and does not
// depend on scheduling.  The 33-d FPFH matcher is lgr_match.hip.
#include <cfloat>

#include "lgr_internal.h"

namespace {

// cv::hal::normL2Sqr_ (OpenCV 4.5.1, SSE baseline) for n = 352: 22 blocks of 16; acc[k][lane] += t * t for element
// 16 b + 4 k + lane; s = ((acc0 + acc1) + acc2) + acc3 lane-wise; d2 = (s0 + s2) + (s1 + s3).  The 16 (k, lane) chains are independent,
// so the rows are packed with the elements of one chain contiguous -- group (lane, k) = 4 lane + k, 22 elements in block order -- and
// transposed (element-major, rows padded to 64) for coalesced tile loads.  A pair then runs the chains one after the other:
// sl = acc(lane, 0) + acc(lane, 1) + acc(lane, 2) + acc(lane, 3) in that order, A = s0 + s2, B = s1 + s3, d2 = A + B: the same
// operations on the same values as the SSE code.
// The kernels are templated on the block count NB and the scalar tail TAIL (row length 16 NB + TAIL): SHOT is <22, 0>, RoPS135
// <8, 7>, whose elements 128..134 follow the blocks as d2 += t * t one after the other (normL2Sqr_'s scalar loop).
constexpr int MT = 64;                // rows per tile side
template <int NB, int TAIL>
__global__ void dense_pack_kernel(const float* __restrict__ rows, int m, int mpad, float* __restrict__ packed) {
    constexpr int LEN = 16 * NB + TAIL;
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) mpad * LEN) return;
    const int r = (int) (e % mpad), p = (int) (e / mpad);   // p: packed element = group * NB + b, group = 4 lane + k; then the tail
    const int grp = p / NB, b = p % NB, lane = grp >> 2, k = grp & 3;
    const int col = (TAIL == 0 || p < 16 * NB) ? 16 * b + 4 * k + lane : p;
    packed[e] = r < m ? rows[(size_t) r * LEN + col] : __uint_as_float(0x7fc00000u);
}

// rank of train row j among equal distances: a later bf block first, the lowest index inside a block
__device__ __forceinline__ unsigned dense_tie_rank(int j, int block, int nb) { return (unsigned) (nb - 1 - j / block) * (unsigned) block + (unsigned) (j % block); }

// 256 threads: a 64 x 64 tile, 4 x 4 pairs per thread.  Block (query tile, split): the split's train tiles one after the other.
template <int NB, int TAIL>
__global__ __launch_bounds__(256) void dense_match_kernel(const float* __restrict__ pa, int ma, int mpa, const float* __restrict__ pb, int mb, int mpb,
                                                         int block, int nb_a, int nb_b, int splits, unsigned long long* __restrict__ key_ab,
                                                         unsigned long long* __restrict__ key_ba) {
    static_assert(TAIL <= NB, "the tail is staged in the block buffers");
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
        float sA[4][4], sB[4][4], sl[4][4], acc[4][4];
        for (int grp = 0; grp < 16; ++grp) {
            __syncthreads();
            for (int e = tid; e < NB * (MT / 4); e += 256) {
                const int b = e / (MT / 4), c = e % (MT / 4);
                sa[b][c] = reinterpret_cast<const float4*>(pa + (size_t) (grp * NB + b) * mpa + q0)[c];
                sb[b][c] = reinterpret_cast<const float4*>(pb + (size_t) (grp * NB + b) * mpb + t0)[c];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
            for (int b = 0; b < NB; ++b) {
                const float4 a4 = sa[b][ty], b4 = sb[b][tx];
                const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float t = av[i] - bv[j]; acc[i][j] = t * t + acc[i][j]; }
            }
            const int k = grp & 3, lane = grp >> 2;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sl[i][j] = k == 0 ? acc[i][j] : sl[i][j] + acc[i][j];
                    if (k == 3) {
                        if (lane == 0) sA[i][j] = sl[i][j];
                        else if (lane == 1) sB[i][j] = sl[i][j];
                        else if (lane == 2) sA[i][j] = sA[i][j] + sl[i][j];
                        else sB[i][j] = sB[i][j] + sl[i][j];
                    }
                }
        }
        if constexpr (TAIL > 0) {   // d2 = A + B, then d2 += t * t for the tail elements in order
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) sA[i][j] = sA[i][j] + sB[i][j];
            __syncthreads();
            for (int e = tid; e < TAIL * (MT / 4); e += 256) {
                const int b = e / (MT / 4), c = e % (MT / 4);
                sa[b][c] = reinterpret_cast<const float4*>(pa + (size_t) (16 * NB + b) * mpa + q0)[c];
                sb[b][c] = reinterpret_cast<const float4*>(pb + (size_t) (16 * NB + b) * mpb + t0)[c];
            }
            __syncthreads();
            for (int b = 0; b < TAIL; ++b) {
                const float4 a4 = sa[b][ty], b4 = sb[b][tx];
                const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float t = av[i] - bv[j]; sA[i][j] = sA[i][j] + t * t; }
            }
        }
        unsigned long long bq[4] = {~0ull, ~0ull, ~0ull, ~0ull}, bt[4] = {~0ull, ~0ull, ~0ull, ~0ull};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int qi = q0 + 4 * ty + i, tj = t0 + 4 * tx + j;
                const float d = TAIL > 0 ? sqrtf(sA[i][j]) : sqrtf(sA[i][j] + sB[i][j]);
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

template <int NB, int TAIL>
int dense_match(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d) {
    constexpr int LEN = 16 * NB + TAIL;
    LGR_CHECK(ctx, (d_a || ma == 0) && (d_b || mb == 0) && ma >= 0 && mb >= 0 && block > 0 && (ab_i || ma == 0) && (ab_d || ma == 0), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const bool both = ba_i != nullptr;
    if (ma == 0 || mb == 0) {
        if (ma) { LGR_HIP(ctx, hipMemsetAsync(ab_i, 0xff, (size_t) ma * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(ab_d, 0, (size_t) ma * 4, ctx->stream)); }
        if (mb && both) { LGR_HIP(ctx, hipMemsetAsync(ba_i, 0xff, (size_t) mb * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(ba_d, 0, (size_t) mb * 4, ctx->stream)); }
        return LGR_OK;
    }
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
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    float *dq, *dt, *dd;
    int32_t* di;
    LGR_TRY(lgr_ws_t(ctx, WS_HOST_A, (size_t) mq * row_len + 1, &dq));
    LGR_TRY(lgr_ws_t(ctx, WS_HOST_B, (size_t) mt * row_len + 1, &dt));
    LGR_TRY(lgr_ws_t(ctx, WS_HOST_C, (size_t) mq + 1, &di));
    LGR_TRY(lgr_ws_t(ctx, WS_HOST_D, (size_t) mq + 1, &dd));
    LGR_HIP(ctx, hipMemcpyAsync(dq, q, (size_t) mq * row_len * 4, hipMemcpyHostToDevice, ctx->stream));
    if (mt) LGR_HIP(ctx, hipMemcpyAsync(dt, t, (size_t) mt * row_len * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_TRY(lgr_match_dense(ctx, row_len, dq, mq, dt, mt, block, di, dd, nullptr, nullptr));
    LGR_HIP(ctx, hipMemcpyAsync(idx, di, (size_t) mq * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(dist, dd, (size_t) mq * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

}  // namespace

int lgr_match_dense(lgr_ctx* ctx, int row_len, const float* d_a, int ma, const float* d_b, int mb, int block,
                    int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d) {
    if (row_len == 352) return dense_match<22, 0>(ctx, d_a, ma, d_b, mb, block, ab_i, ab_d, ba_i, ba_d);
    if (row_len == 135) return dense_match<8, 7>(ctx, d_a, ma, d_b, mb, block, ab_i, ab_d, ba_i, ba_d);
    return lgr_fail(ctx, LGR_ERR_UNSUPPORTED, "row_len == 352 || row_len == 135", __FILE__, __LINE__);
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
