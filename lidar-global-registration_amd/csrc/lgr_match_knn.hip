// lgr_match_knn.hip -- the exact k-nearest brute-force matcher (randomness > 1), the proximity vote over a query's candidates and the
// ratio test over a query's list.
//
//   include/matching.h:612-625 matchBF with knnMatch(.., randomness), src/common.cpp:517-529 updateMultivaluedCorrespondence
//                                                                                    -> lgr_match_knn*, lgr_match_knn2_dev
//   include/matching.h:327-352 the vote of match_multiscale                          -> lgr_vote_matches*
//   include/matching.h:470-473 RatioMatcher (a TODO there: DESIGN.md section 4 states it) -> lgr_ratio_test*, lgr_match_ratio*
// The pair distances are lgr_match_dense.cuh's (OpenCV's float sequence); the selection is DESIGN.md section 4's two-stage order:
// inside a bf block the first k rows in ascending (d, index) -- order P --, across blocks the first k of the blocks' lists in ascending
// (d, index DESCENDING) -- order F: a later insertion goes in front of equal distances, blocks and their lists are fed ascending.
#include <cfloat>
#include <cmath>

#include "lgr_host.h"
#include "lgr_match_dense.cuh"
#include "lgr_match_densef.cuh"
#include "lgr_cloud.h"

namespace {

constexpr int KMAX = LGR_RANDOMNESS_MAX;
constexpr int CAP = 1024;             // candidate buffer: one row of 4 pairs per thread always fits (256 x 4)
constexpr unsigned long long NONE = ~0ull;

// insert into the ascending list lst[0..k)[r] (NONE-padded) unless key is not below its last entry
__device__ __forceinline__ void knn_insert(unsigned long long (*lst)[MT], int r, int k, unsigned long long key) {
    if (key >= lst[k - 1][r]) return;
    int pos = k - 1;
    while (pos > 0 && lst[pos - 1][r] > key) { lst[pos][r] = lst[pos - 1][r]; --pos; }
    lst[pos][r] = key;
}

// Block (query tile, split): the split's run of whole bf blocks, train tiles ascending.  Per query row two sorted lists of 64-bit keys
// in LDS: cur (the running bf block, order P: d bits << 32 | j) and mrg (the blocks before it, order F: d bits << 32 | ~j).  A tile is
// cut where a bf block ends; per piece the lanes whose pair can still enter (below cur's k-th key, and not above mrg's k-th distance:
// a later row goes in FRONT of an equal distance) append it to the candidate buffer, thread 0..63 drains the buffer into its row's
// list, and at a block's end folds cur into mrg.  When a piece has more candidates than the buffer holds it is offered in four
// rounds, one row of 4 pairs per thread and round, which always fit.  Keys of one list are distinct, so the order of arrival in the
// buffer cannot show in the result.
template <int NB, int TAIL>
__global__ __launch_bounds__(256) void knn_match_kernel(const float* __restrict__ pa, int ma, int mpa, const float* __restrict__ pb, int mb, int mpb,
                                                       int block, int k, int splits, int blocks_per_split, unsigned long long* __restrict__ part) {
    __shared__ float4 sa[NB][MT / 4];
    __shared__ float4 sb[NB][MT / 4];
    __shared__ unsigned long long cur[KMAX][MT], mrg[KMAX][MT], ckey[CAP];
    __shared__ unsigned char crow[CAP];
    __shared__ int cnt;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int qt = blockIdx.x / splits, split = blockIdx.x % splits;
    const int q0 = qt * MT;
    const long long lo_ll = (long long) split * blocks_per_split * block, hi_ll = lo_ll + (long long) blocks_per_split * block;
    const int j_lo = (int) (lo_ll < mb ? lo_ll : mb), j_hi = (int) (hi_ll < mb ? hi_ll : mb);
    for (int e = tid; e < KMAX * MT; e += 256) { cur[e / MT][e % MT] = NONE; mrg[e / MT][e % MT] = NONE; }
    if (tid == 0) cnt = 0;
    __syncthreads();
    for (int t0 = j_lo / MT * MT; t0 < j_hi; t0 += MT) {
        float d[4][4];
        dense_tile_distances<NB, TAIL>(pa, mpa, q0, pb, mpb, t0, sa, sb, d);
        unsigned dbits[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)   // NaN and distances not below FLT_MAX never enter (batchDistance's strict '<' from FLT_MAX)
                dbits[i][j] = (q0 + 4 * ty + i < ma && d[i][j] < FLT_MAX) ? __float_as_uint(d[i][j]) : 0xffffffffu;
        const int t_end = t0 + MT < j_hi ? t0 + MT : j_hi;
        int c = t0 > j_lo ? t0 : j_lo;
        while (c < t_end) {   // pieces [c, c_hi) of one bf block each
            const long long b_end_ll = ((long long) (c / block) + 1) * block;
            const int b_end = (int) (b_end_ll < j_hi ? b_end_ll : j_hi), c_hi = b_end < t_end ? b_end : t_end;
            // a pair passes when it is inside the piece and can still enter its row's lists
            auto offer = [&](int i_lo, int i_hi, bool write, int base) -> int {
                int n = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < i_lo || i >= i_hi) continue;
                    const int r = 4 * ty + i;
                    const unsigned long long lim_c = cur[k - 1][r];
                    const unsigned lim_m = (unsigned) (mrg[k - 1][r] >> 32);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int tj = t0 + 4 * tx + j;
                        const unsigned long long key = (unsigned long long) dbits[i][j] << 32 | (unsigned) tj;
                        if (dbits[i][j] == 0xffffffffu || tj < c || tj >= c_hi || key >= lim_c || dbits[i][j] > lim_m) continue;
                        if (write) { ckey[base + n] = key; crow[base + n] = (unsigned char) r; }
                        ++n;
                    }
                }
                return n;
            };
            auto drain = [&](int n) {
                if (tid < MT)
                    for (int e = 0; e < n; ++e)
                        if (crow[e] == tid) knn_insert(cur, tid, k, ckey[e]);
            };
            const int n_all = offer(0, 4, false, 0);
            const int base_all = n_all ? atomicAdd(&cnt, n_all) : 0;
            __syncthreads();
            const int total = cnt;
            if (total > 0 && total <= CAP) {
                offer(0, 4, true, base_all);
                __syncthreads();
                if (tid == 0) cnt = 0;
                drain(total);
            } else if (total > CAP) {
                for (int round = 0; round < 4; ++round) {
                    __syncthreads();   // every thread has read cnt; the drain before is complete
                    if (tid == 0) cnt = 0;
                    __syncthreads();
                    const int n = offer(round, round + 1, false, 0);
                    const int base = n ? atomicAdd(&cnt, n) : 0;
                    offer(round, round + 1, true, base);   // the limits are unchanged since the count: the same pairs
                    __syncthreads();
                    drain(cnt);
                }
                __syncthreads();
                if (tid == 0) cnt = 0;
            }
            if (c_hi == b_end && tid < MT) {   // the bf block is complete: its list enters the merged list, in list order
                for (int e = 0; e < k; ++e) {
                    const unsigned long long key = cur[e][tid];
                    if (key == NONE) break;
                    knn_insert(mrg, tid, k, (key & 0xffffffff00000000ull) | (unsigned) ~(unsigned) key);
                }
                for (int e = 0; e < k; ++e) cur[e][tid] = NONE;
            }
            __syncthreads();
            c = c_hi;
        }
    }
    // (the last piece ended at j_hi, a block end: cur is folded)
    for (int e = tid; e < k * MT; e += 256) part[((size_t) split * mpa + q0 + e % MT) * k + e / MT] = mrg[e / MT][e % MT];
}

// The ratio test: a list's first entry is the query's candidate iff the list has k entries and
// d_first * thr < d_kth -- one f32 multiply (no contraction: there is no add), a strict compare.  Equal distances and NaN never pass.
__device__ __forceinline__ bool ratio_passes(float d_first, float d_kth, float thr) { return __fmul_rn(d_first, thr) < d_kth; }

// the first k of the splits' lists in order F, decoded: 64 queries per block, the list in LDS.  RATIO: idx / dist hold one entry per
// query, the candidate of the ratio test on its list (or -1 / 0.f), instead of the m x k table.
template <bool RATIO>
__global__ __launch_bounds__(64) void knn_merge_kernel(const unsigned long long* __restrict__ part, int m, int mpa, int k, int splits, float thr,
                                                      int32_t* __restrict__ idx, float* __restrict__ dist) {
    __shared__ unsigned long long lst[KMAX][MT];
    const int tid = threadIdx.x, q = blockIdx.x * MT + tid;
    for (int e = 0; e < k; ++e) lst[e][tid] = NONE;
    if (q >= m) return;
    for (int s = 0; s < splits; ++s)
        for (int e = 0; e < k; ++e) {
            const unsigned long long key = part[((size_t) s * mpa + q) * k + e];
            if (key == NONE) break;
            knn_insert(lst, tid, k, key);
        }
    if (RATIO) {
        const unsigned long long first = lst[0][tid], kth = lst[k - 1][tid];
        const bool keep = kth != NONE && ratio_passes(__uint_as_float((unsigned) (first >> 32)), __uint_as_float((unsigned) (kth >> 32)), thr);
        idx[q] = keep ? (int32_t) ~(unsigned) first : -1;
        dist[q] = keep ? __uint_as_float((unsigned) (first >> 32)) : 0.f;
        return;
    }
    for (int e = 0; e < k; ++e) {
        const unsigned long long key = lst[e][tid];
        idx[(size_t) q * k + e] = key == NONE ? -1 : (int32_t) ~(unsigned) key;
        dist[(size_t) q * k + e] = key == NONE ? 0.f : __uint_as_float((unsigned) (key >> 32));
    }
}

template <int NB, int TAIL>
int knn_sweep(lgr_ctx* ctx, const float* pa, int ma, int mpa, const float* pb, int mb, int mpb, int block, int k, int slot, int32_t* idx, float* dist,
              const float* ratio_thr = nullptr) {
    // splits are runs of whole bf blocks (the two-stage order needs a block's rows in one list); at most 8 thread blocks per CU in all
    const int n_qt = mpa / MT, nb = cdiv(mb, block);
    const int want = std::max(1, std::min(std::min(nb, cdiv(mb, MT)), cdiv(8 * ctx->n_cu, n_qt)));
    const int bps = cdiv(nb, want), splits = cdiv(nb, bps);
    unsigned long long* part;
    LGR_TRY(lgr_ws_t(ctx, slot, (size_t) splits * mpa * k, &part));
    knn_match_kernel<NB, TAIL><<<n_qt * splits, 256, 0, ctx->stream>>>(pa, ma, mpa, pb, mb, mpb, block, k, splits, bps, part);
    if (ratio_thr) knn_merge_kernel<true><<<n_qt, MT, 0, ctx->stream>>>(part, ma, mpa, k, splits, *ratio_thr, idx, dist);
    else knn_merge_kernel<false><<<n_qt, MT, 0, ctx->stream>>>(part, ma, mpa, k, splits, 0.f, idx, dist);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

template <int NB, int TAIL>
int knn_match(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int k, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d,
              const float* ratio_thr) {
    constexpr int LEN = 16 * NB + TAIL;
    LGR_CHECK(ctx, (d_a || ma == 0) && (d_b || mb == 0) && ma >= 0 && mb >= 0 && block > 0 && (ab_i || ma == 0) && (ab_d || ma == 0), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const bool both = ba_i != nullptr;
    const size_t width = ratio_thr ? 1 : k;   // entries per query of ab_i / ab_d (the ratio form is one direction: ba_i is NULL)
    if (ma == 0 || mb == 0) {
        if (ma) { LGR_HIP(ctx, hipMemsetAsync(ab_i, 0xff, (size_t) ma * width * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(ab_d, 0, (size_t) ma * width * 4, ctx->stream)); }
        if (mb && both) { LGR_HIP(ctx, hipMemsetAsync(ba_i, 0xff, (size_t) mb * k * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(ba_d, 0, (size_t) mb * k * 4, ctx->stream)); }
        return LGR_OK;
    }
    const int mpa = cdiv(ma, MT) * MT, mpb = cdiv(mb, MT) * MT;
    float *pa, *pb;
    LGR_TRY(lgr_ws_t(ctx, WS_DENSE_PACK_A, (size_t) mpa * LEN, &pa));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSE_PACK_B, (size_t) mpb * LEN, &pb));
    dense_pack_kernel<NB, TAIL><<<cdiv((long long) mpa * LEN, 256), 256, 0, ctx->stream>>>(d_a, ma, mpa, pa);
    dense_pack_kernel<NB, TAIL><<<cdiv((long long) mpb * LEN, 256), 256, 0, ctx->stream>>>(d_b, mb, mpb, pb);
    LGR_TRY((knn_sweep<NB, TAIL>(ctx, pa, ma, mpa, pb, mb, mpb, block, k, WS_KNN_PART_A, ab_i, ab_d, ratio_thr)));
    // the other direction sweeps the same packed operands with the roles exchanged
    if (both) LGR_TRY((knn_sweep<NB, TAIL>(ctx, pb, mb, mpb, pa, ma, mpa, block, k, WS_KNN_PART_B, ba_i, ba_d)));
    return LGR_OK;
}

// One thread per query: the vote of include/matching.h:327-352 over its row of candidates, sums in list order.  A candidate outside
// [0, mt) that is not negative raises *bad and is skipped (the entry point reports it).
__global__ void vote_matches_kernel(const int32_t* __restrict__ cand, const float* __restrict__ cdist, int mq, int width, const float* __restrict__ pts, int mt,
                                    float r, int32_t* __restrict__ idx, float* __restrict__ dist, int* __restrict__ bad) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= mq) return;
    const int32_t* c = cand + (size_t) q * width;
    const float* cd = cdist + (size_t) q * width;
    const float win = 32 * r;
    float best_c = 0.f, best_d = 0.f;
    int best = -1;
    for (int m1 = 0; m1 < width; ++m1) {
        const int c1 = c[m1];
        if (c1 < 0) continue;
        if (c1 >= mt) { *bad = 1; continue; }
        const float ax = pts[12 * (size_t) c1], ay = pts[12 * (size_t) c1 + 1], az = pts[12 * (size_t) c1 + 2];
        float cnt = 0.f;
        for (int m2 = m1; m2 < width; ++m2) {
            const int c2 = c[m2];
            if (c2 < 0 || c2 >= mt) continue;
            const float dx = ax - pts[12 * (size_t) c2], dy = ay - pts[12 * (size_t) c2 + 1], dz = az - pts[12 * (size_t) c2 + 2];
            const float dl = sqrtf((dx * dx + dy * dy) + dz * dz);
            if (dl < win) cnt += r / fmaxf(dl, r);
        }
        const float dm = cd[m1];
        if (cnt > best_c || (cnt == best_c && dm < best_d)) { best_c = cnt; best_d = dm; best = m1; }
    }
    idx[q] = best >= 0 ? c[best] : -1;
    dist[q] = best >= 0 ? cd[best] : 0.f;
}

// One thread per query: the ratio test on its row of a caller's mq x k table (list order, then -1 / 0.f: a list shorter than k ends in -1)
__global__ void ratio_test_kernel(const int32_t* __restrict__ kidx, const float* __restrict__ kdist, int mq, int k, float thr,
                                  int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= mq) return;
    const int32_t first = kidx[(size_t) q * k];
    const float d_first = kdist[(size_t) q * k];
    const bool keep = first >= 0 && kidx[(size_t) q * k + k - 1] >= 0 && ratio_passes(d_first, kdist[(size_t) q * k + k - 1], thr);
    idx[q] = keep ? first : -1;
    dist[q] = keep ? d_first : 0.f;
}

}  // namespace

#include "lgr_match_knn_mfma.cuh"
#include "lgr_match_knn_dense_mfma.cuh"

namespace {

// a call under lgr_ctx_set_knn_filter: the filtered path of the row length (33 floats: lgr_match_knn_mfma.cuh, 135 and 352 floats:
// lgr_match_knn_dense_mfma.cuh), or the exact scan with the reason in knnf_last[7].  Every call writes knnf_last fresh.
template <int NB, int TAIL>
int knn_match_switched(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int k, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d,
                       const float* ratio_thr) {
    constexpr bool SHORT = NB == 2 && TAIL == 1;
    const unsigned long long fresh[8] = {0, 0, 0, 0, 0, 0, ~0ull, 0};
    memcpy(ctx->knnf_last, fresh, sizeof fresh);
    ctx->knnf_worst = -1;
    const bool args_ok = (d_a || ma == 0) && (d_b || mb == 0) && ma >= 0 && mb >= 0 && block > 0 && (ab_i || ma == 0) && (ab_d || ma == 0);
    const bool want = ctx->knnf_mode == 1 || (ctx->knnf_mode == -1 && (long long) ma * mb >= (SHORT ? KNNF_AUTO_MIN_PAIRS : KNND_AUTO_MIN_PAIRS));
    if (want && args_ok) {
        if (ma > 0 && mb > 0) {
            bool done = false;
            if constexpr (SHORT) LGR_TRY(knnf_match(ctx, d_a, ma, d_b, mb, block, k, ab_i, ab_d, ba_i, ba_d, ratio_thr, &done));
            else LGR_TRY((knnd_match<NB, TAIL>(ctx, d_a, ma, d_b, mb, block, k, ab_i, ab_d, ba_i, ba_d, ratio_thr, &done)));
            if (done) return LGR_OK;
        } else ctx->knnf_last[7] = KNNF_REASON_EMPTY;
    }
    const int rc = knn_match<NB, TAIL>(ctx, d_a, ma, d_b, mb, block, k, ab_i, ab_d, ba_i, ba_d, ratio_thr);
    if (rc == LGR_OK && args_ok) { ctx->knnf_last[1] = (unsigned long long) ma * mb * (ba_i ? 2 : 1); ctx->knnf_last[3] = (unsigned long long) ma + (ba_i ? mb : 0); }
    return rc;
}

int knn_dispatch(lgr_ctx* ctx, int row_len, const float* d_a, int ma, const float* d_b, int mb, int block, int k,
                 int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d, const float* ratio_thr) {
    if (row_len == 352) return knn_match_switched<22, 0>(ctx, d_a, ma, d_b, mb, block, k, ab_i, ab_d, ba_i, ba_d, ratio_thr);
    if (row_len == 135) return knn_match_switched<8, 7>(ctx, d_a, ma, d_b, mb, block, k, ab_i, ab_d, ba_i, ba_d, ratio_thr);
    if (row_len == 33) return knn_match_switched<2, 1>(ctx, d_a, ma, d_b, mb, block, k, ab_i, ab_d, ba_i, ba_d, ratio_thr);
    return lgr_fail(ctx, LGR_ERR_UNSUPPORTED, "row_len == 33 || row_len == 135 || row_len == 352", __FILE__, __LINE__);
}

}  // namespace

int lgr_match_knn_core(lgr_ctx* ctx, int row_len, const float* d_a, int ma, const float* d_b, int mb, int block, int k,
                       int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d) {
    LGR_CHECK(ctx, k >= 1 && k <= KMAX, LGR_ERR_UNSUPPORTED);
    return knn_dispatch(ctx, row_len, d_a, ma, d_b, mb, block, k, ab_i, ab_d, ba_i, ba_d, nullptr);
}

// the k-nearest sweep of one direction with the ratio test where its lists are decoded: d_idx / d_dist hold mq entries
int lgr_match_ratio_core(lgr_ctx* ctx, int row_len, const float* d_q, int mq, const float* d_t, int mt, int block, int k, float threshold,
                         int32_t* d_idx, float* d_dist) {
    LGR_CHECK(ctx, k >= 2 && k <= KMAX, LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, std::isfinite(threshold) && threshold > 0.f, LGR_ERR_INVALID_ARG);
    return knn_dispatch(ctx, row_len, d_q, mq, d_t, mt, block, k, d_idx, d_dist, nullptr, nullptr, &threshold);
}

int lgr_ratio_test_core(lgr_ctx* ctx, const int32_t* d_knn_idx, const float* d_knn_dist, int mq, int k, float threshold, int32_t* d_idx, float* d_dist) {
    LGR_CHECK(ctx, k >= 2 && k <= KMAX, LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, mq >= 0 && std::isfinite(threshold) && threshold > 0.f && ((d_knn_idx && d_knn_dist && d_idx && d_dist) || mq == 0), LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    ratio_test_kernel<<<cdiv(mq, 256), 256, 0, ctx->stream>>>(d_knn_idx, d_knn_dist, mq, k, threshold, d_idx, d_dist);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// the multi-scale path's vote (lgr_cloud.h): the width and radius the caller has -- the width bound and the radius check belong to the
// public entry points --, candidates that are the pipeline's own, so the flag is not read back
int lgr_vote_matches_launch(lgr_ctx* ctx, const int32_t* d_cand_idx, const float* d_cand_dist, int mq, int width, const float* d_train_pts, int mt,
                            float iss_radius, int32_t* d_idx, float* d_dist) {
    if (mq == 0) return LGR_OK;
    int* bad;
    LGR_TRY(lgr_ws_t(ctx, WS_KNN_FLAG, 1, &bad));
    vote_matches_kernel<<<cdiv(mq, 256), 256, 0, ctx->stream>>>(d_cand_idx, d_cand_dist, mq, width, d_train_pts, mt, iss_radius, d_idx, d_dist, bad);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

int lgr_vote_matches_core(lgr_ctx* ctx, const int32_t* d_cand_idx, const float* d_cand_dist, int mq, int width, const float* d_train_pts, int mt,
                          float iss_radius, int32_t* d_idx, float* d_dist) {
    LGR_CHECK(ctx, mq >= 0 && mt >= 0 && width >= 1 && width <= 64 && std::isfinite(iss_radius) && iss_radius > 0.f, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, ((d_cand_idx && d_cand_dist && d_idx && d_dist) || mq == 0) && (d_train_pts || mt == 0), LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    int* bad;
    LGR_TRY(lgr_ws_t(ctx, WS_KNN_FLAG, 1, &bad));
    LGR_HIP(ctx, hipMemsetAsync(bad, 0, 4, ctx->stream));
    LGR_TRY(lgr_vote_matches_launch(ctx, d_cand_idx, d_cand_dist, mq, width, d_train_pts, mt, iss_radius, d_idx, d_dist));
    int h_bad = 0;
    LGR_HIP(ctx, hipMemcpyAsync(&h_bad, bad, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    LGR_CHECK(ctx, h_bad == 0 /* a candidate >= mt */, LGR_ERR_INVALID_ARG);
    return LGR_OK;
}

static void knnf_propagate(lgr_ctx* ctx, int mode, int self_check) {
    ctx->knnf_mode = mode; ctx->knnf_check = self_check;
    if (ctx->aux) knnf_propagate(ctx->aux, mode, self_check);
    if (ctx->aux2) knnf_propagate(ctx->aux2, mode, self_check);
}

extern "C" int lgr_ctx_set_knn_filter(lgr_ctx* ctx, int mode, int self_check) {
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, mode >= -1 && mode <= 1 && (self_check == 0 || self_check == 1), LGR_ERR_INVALID_ARG);
    knnf_propagate(ctx, mode, self_check);
    return LGR_OK;
}

extern "C" int lgr_ctx_get_knn_filter(lgr_ctx* ctx, int* mode, int* self_check) {
    if (!ctx || !mode || !self_check) return LGR_ERR_INVALID_ARG;
    *mode = ctx->knnf_mode; *self_check = ctx->knnf_check;
    return LGR_OK;
}

extern "C" int lgr_match_knn_last(lgr_ctx* ctx, unsigned long long* out8) {
    if (!ctx || !out8) return LGR_ERR_INVALID_ARG;
    memcpy(out8, ctx->knnf_last, sizeof ctx->knnf_last);
    return LGR_OK;
}

extern "C" int lgr_match_knn_last_check(lgr_ctx* ctx, double* worst_ratio) {
    if (!ctx || !worst_ratio) return LGR_ERR_INVALID_ARG;
    *worst_ratio = ctx->knnf_worst;
    return LGR_OK;
}

extern "C" int lgr_match_knn_dev(lgr_ctx* ctx, int row_len, const float* d_q, int mq, const float* d_t, int mt, int block, int k, int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return lgr_match_knn_core(ctx, row_len, d_q, mq, d_t, mt, block, k, d_idx, d_dist, nullptr, nullptr);
}

extern "C" int lgr_match_knn2_dev(lgr_ctx* ctx, int row_len, const float* d_a, int ma, const float* d_b, int mb, int block, int k,
                                  int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (d_ba_idx && d_ba_dist) || mb == 0, LGR_ERR_INVALID_ARG);
    return lgr_match_knn_core(ctx, row_len, d_a, ma, d_b, mb, block, k, d_ab_idx, d_ab_dist, mb ? d_ba_idx : nullptr, d_ba_dist);
}

extern "C" int lgr_match_knn(lgr_ctx* ctx, int row_len, const float* q, int mq, const float* t, int mt, int block, int k, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, k >= 1 && k <= KMAX && (row_len == 33 || row_len == 135 || row_len == 352), LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, (q || mq == 0) && (t || mt == 0) && (idx || mq == 0) && (dist || mq == 0) && mq >= 0 && mt >= 0 && block > 0, LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    float *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q, (size_t) mq * row_len, &dq));
    LGR_TRY(hc.in(t, (size_t) mt * row_len, &dt));
    LGR_TRY(hc.out((size_t) mq * k, &di));
    LGR_TRY(hc.out((size_t) mq * k, &dd));
    LGR_TRY(lgr_match_knn_core(ctx, row_len, dq, mq, dt, mt, block, k, di, dd, nullptr, nullptr));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq * k));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq * k));
    return hc.finish();
}

extern "C" int lgr_vote_matches_dev(lgr_ctx* ctx, const int32_t* d_cand_idx, const float* d_cand_dist, int mq, int width, const float* d_train_pts, int mt,
                                    float iss_radius, int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return lgr_vote_matches_core(ctx, d_cand_idx, d_cand_dist, mq, width, d_train_pts, mt, iss_radius, d_idx, d_dist);
}

extern "C" int lgr_vote_matches(lgr_ctx* ctx, const int32_t* cand_idx, const float* cand_dist, int mq, int width, const float* train_pts, int mt,
                                float iss_radius, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, mq >= 0 && mt >= 0 && width >= 1 && width <= 64 && std::isfinite(iss_radius) && iss_radius > 0.f, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, ((cand_idx && cand_dist && idx && dist) || mq == 0) && (train_pts || mt == 0), LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    int32_t *dc, *di;
    float *dcd, *dp, *dd;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(cand_idx, (size_t) mq * width, &dc));
    LGR_TRY(hc.in(cand_dist, (size_t) mq * width, &dcd));
    LGR_TRY(hc.in(train_pts, (size_t) mt * 12, &dp));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_vote_matches_core(ctx, dc, dcd, mq, width, dp, mt, iss_radius, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}

extern "C" int lgr_ratio_test_dev(lgr_ctx* ctx, const int32_t* d_knn_idx, const float* d_knn_dist, int mq, int k, float threshold, int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return lgr_ratio_test_core(ctx, d_knn_idx, d_knn_dist, mq, k, threshold, d_idx, d_dist);
}

extern "C" int lgr_ratio_test(lgr_ctx* ctx, const int32_t* knn_idx, const float* knn_dist, int mq, int k, float threshold, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, k >= 2 && k <= KMAX, LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, mq >= 0 && std::isfinite(threshold) && threshold > 0.f && ((knn_idx && knn_dist && idx && dist) || mq == 0), LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    int32_t *dki, *di;
    float *dkd, *dd;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(knn_idx, (size_t) mq * k, &dki));
    LGR_TRY(hc.in(knn_dist, (size_t) mq * k, &dkd));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_ratio_test_core(ctx, dki, dkd, mq, k, threshold, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}

extern "C" int lgr_match_ratio_dev(lgr_ctx* ctx, int row_len, const float* d_q, int mq, const float* d_t, int mt, int block, int k, float threshold,
                                   int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return lgr_match_ratio_core(ctx, row_len, d_q, mq, d_t, mt, block, k, threshold, d_idx, d_dist);
}

extern "C" int lgr_match_ratio(lgr_ctx* ctx, int row_len, const float* q, int mq, const float* t, int mt, int block, int k, float threshold,
                               int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, k >= 2 && k <= KMAX && (row_len == 33 || row_len == 135 || row_len == 352), LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, (q || mq == 0) && (t || mt == 0) && (idx || mq == 0) && (dist || mq == 0) && mq >= 0 && mt >= 0 && block > 0, LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    float *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q, (size_t) mq * row_len, &dq));
    LGR_TRY(hc.in(t, (size_t) mt * row_len, &dt));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_match_ratio_core(ctx, row_len, dq, mq, dt, mt, block, k, threshold, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}
