// lgr_match_knn_dense_mfma.cuh -- the MFMA-filtered k-nearest matcher for the long rows, SHOT352 <22, 0> and RoPS135 <8, 7> (included by
// lgr_match_knn.hip after lgr_match_knn_mfma.cuh, whose select, cover and scatter kernels it shares).  DESIGN.md section 3.1i (pipeline,
// times) and section 4 (lemma, bound, group values).
//
// The result is DEFINED by the exact path, as for 33-float rows: per bf block the first k rows in order P, across blocks the first k in
// order F, on the canonical distances of dense_tile_distances<NB, TAIL>.  By the lemma the list of query i depends only on
// S_i = { j : d(i, j) <= D_k(i) }; the filter produces a C_i that contains S_i from the f16-split operands of the one-match filter:
//
//   centre, scale, pack, norm bounds: lgr_match_densef.cuh, unchanged; one centre and scale per call, each side packed once.
//   bound     |F - d2 2^2s| <= E(i, tile) = EPS S^2 + 2.5e-3 S + 1e-5 of that chain.
//   sweep A   densef_sweep_kernel<.., 3>: per (lane, tile) the minimum of F + E over the lane's 16 train rows is one GROUP value.  Groups
//             of different (half, tile) are disjoint sets of train rows and each holds a row with d2 2^2s <= its value, so the k-th smallest
//             group value U_i of a query is an upper bound of D_k(i)^2 2^2s.  A lane keeps its 8 smallest per owned query; they are written
//             per (split, train wave, half), and knnd_kth_kernel takes the k-th smallest over a query's lists.  Fewer than k finite
//             group values, an irregular query or padding: U_i = +inf, no candidates, and densef_flag_kernel puts a row with finite
//             elements on the fallback list.
//   sweep B   densef_sweep_kernel<.., 1>, the one-match filter's: every (i, j) with F - E <= U_i (1 + 1e-5) enters row i's list (DENSEF_CAP
//             entries; overflow: fallback).  The widening by 1e-5 (two d2 may round to one d) is applied where that kernel reads U_i.
//   select    knnf_select_kernel<RATIO, NB, TAIL>: canonical distances of the candidates and of the irregular train rows, order P per bf
//             block, order F across blocks, the fused ratio test.
//   fallback  the compacted list goes through knn_match_kernel<NB, TAIL> against all train rows and is scattered back; more than half of a
//             direction's rows on it: the direction takes the exact scan whole.
#pragma once

namespace {

static_assert(KNNF_CAP == DENSEF_CAP && KNNF_IRR_CAP == DENSEF_IRR_CAP, "knnf_select_kernel and knnf_cover_kernel read the lists of either filter");

// lgr_ctx_set_knn_filter(mode -1) on 135- and 352-float rows: the filtered path from this many (query, train) pairs per direction.  Measured
// (profiles/match_knn_dense_filter.json; k = 2, both directions, block 10 000, exact / filtered ms): 135 floats, the
// row length that gains less: 4 096 x 4 096: 5.11 / 0.72, 16 384 x 16 384: 11.2 / 2.95, 35 913 x 35 913: 39.0 / 12.8, 50 000 x 50 000:
// 73.5 / 23.2; 352 floats: 8.27 / 0.95, 36.8 / 4.44, 168.5 / 20.7, 312.5 / 37.3.  The filtered path is ahead at every measured size for both
// row lengths (the exact scan keeps k-lists in LDS and is far from the one-match scan's speed); the constant stays at 16 384 x 16 384, the
// smallest size at which auto may switch without moving any call of the test suite off the exact scan.
constexpr long long KNND_AUTO_MIN_PAIRS = 16384ll * 16384ll;

// U_i: the k-th smallest of a query's group values, as the float bits sweep B reads; +inf (nothing passes sweep B) for padding, irregular
// queries and rows with fewer than k finite group values.  Also clears the row's candidate counter.
__global__ void knnd_kth_kernel(const float* __restrict__ glist, int n_lists, int mqp, int k, const float* __restrict__ xb_q,
                                unsigned* __restrict__ ubits, int* __restrict__ cnt) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= mqp) return;
    float lst[DENSEF_GROUPS];
#pragma unroll
    for (int p = 0; p < DENSEF_GROUPS; ++p) lst[p] = __uint_as_float(0x7f800000u);
    for (int l = 0; l < n_lists; ++l) {
        const float4* in = reinterpret_cast<const float4*>(glist + ((size_t) l * mqp + q) * DENSEF_GROUPS);
#pragma unroll
        for (int e4 = 0; e4 < DENSEF_GROUPS / 4; ++e4) {
            const float4 g = in[e4];
            const float ge[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = ge[e];
#pragma unroll
                for (int p = 0; p < DENSEF_GROUPS; ++p) { const float lo = fminf(lst[p], v); v = fmaxf(lst[p], v); lst[p] = lo; }
            }
        }
    }
    float U = lst[0];
#pragma unroll
    for (int p = 1; p < DENSEF_GROUPS; ++p) U = p == k - 1 ? lst[p] : U;
    const bool ok = xb_q[q] >= 0.f && U < 3e38f;   // (padding has xb = -2)
    ubits[q] = ok ? __float_as_uint(U) : 0x7f800000u;
    cnt[q] = 0;
}

// One direction.  last: the counters of lgr_match_knn_last, accumulated over the directions of a call.
template <int NB, int TAIL>
int knnd_direction(lgr_ctx* ctx, const DensefSide& Q, const DensefSide& T, const float* centre, int block, int k, int32_t* idx, float* dist,
                   const float* ratio_thr, unsigned long long* last, double* worst) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN;
    const int mq = Q.m, mt = T.m, mqp = Q.mp;
    int tps;
    const int n_split = densef_splits(ctx, Q, T, &tps);
    const size_t width = ratio_thr ? 1 : k;
    float* glist;
    unsigned* ubits;
    int *cnt, *cand, *fb;
    unsigned char* is_fb;
    unsigned long long* dev;   // [0] pairs, [1] bound violations, [2] cover violations, [3] worst ratio bits
    LGR_TRY(lgr_ws_t(ctx, WS_KNND_GROUPS, (size_t) n_split * 4 * mqp * DENSEF_GROUPS, &glist));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_UW, (size_t) mqp, &ubits));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_CNT, (size_t) mqp, &cnt));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_CAND, (size_t) mqp * DENSEF_CAP, &cand));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FB, (size_t) mq + 1, &fb));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_ISFB, (size_t) mq, &is_fb));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_DEV, 4, &dev));
    LGR_HIP(ctx, hipMemsetAsync(dev, 0, 32, ctx->stream));
    LGR_HIP(ctx, hipMemsetAsync(fb, 0, 4, ctx->stream));
    const DensefCheck none{};
    LGR_TRY((densef_sweep<NB, TAIL, 3>(ctx, Q, T, ubits, cnt, cand, none, glist)));
    knnd_kth_kernel<<<cdiv(mqp, 256), 256, 0, ctx->stream>>>(glist, 4 * n_split, mqp, k, Q.xb, ubits, cnt);
    LGR_TRY((densef_sweep<NB, TAIL, 1>(ctx, Q, T, ubits, cnt, cand, none)));
    densef_flag_kernel<<<cdiv(mq, 256), 256, 0, ctx->stream>>>(Q.xb, ubits, cnt, mq, fb, is_fb);
    LGR_HIP(ctx, hipGetLastError());
    int n_fb = 0;   // the one read-back of a direction: it sizes the fallback list
    LGR_HIP(ctx, hipMemcpyAsync(&n_fb, fb, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (2ll * n_fb > mq) {   // the documented share: more than half of the rows have no usable candidate list
        last[0] = 0; last[7] = KNNF_REASON_FALLBACK_SHARE;
        last[1] += (unsigned long long) mq * mt; last[3] += mq;
        return knnf_exact<NB, TAIL>(ctx, Q.rows, mq, T.rows, mt, block, k, WS_KNN_PART_A, idx, dist, ratio_thr);
    }
    const float thr = ratio_thr ? *ratio_thr : 0.f;
    if (ratio_thr) knnf_select_kernel<true, NB, TAIL><<<cdiv(mq, 2), 128, 0, ctx->stream>>>(Q.rows, T.rows, mq, block, k, cnt, cand, T.irr, T.n_irr, is_fb, thr, idx, dist, dev);
    else knnf_select_kernel<false, NB, TAIL><<<cdiv(mq, 2), 128, 0, ctx->stream>>>(Q.rows, T.rows, mq, block, k, cnt, cand, T.irr, T.n_irr, is_fb, thr, idx, dist, dev);
    LGR_HIP(ctx, hipGetLastError());
    if (ctx->knnf_check) {
        const DensefCheck chk{Q.rows, T.rows, T.xb, centre, (unsigned*) (dev + 3), dev + 1};
        LGR_TRY((densef_sweep<NB, TAIL, 2>(ctx, Q, T, ubits, cnt, cand, chk)));
        knnf_cover_kernel<NB, TAIL><<<cdiv(mq, 4), 256, 0, ctx->stream>>>(Q.rows, T.rows, mq, mt, k, cnt, cand, T.xb, is_fb, dev + 2);
        LGR_HIP(ctx, hipGetLastError());
    }
    if (n_fb) {
        float* rows_fb;
        int32_t* ti;
        float* td;
        LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FBROWS, (size_t) n_fb * LEN, &rows_fb));
        LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FBIDX, (size_t) n_fb * width, &ti));
        LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FBDIST, (size_t) n_fb * width, &td));
        densef_gather_rows_kernel<<<cdiv((long long) n_fb * LEN, 256), 256, 0, ctx->stream>>>(Q.rows, fb + 1, n_fb, LEN, rows_fb);
        LGR_TRY((knnf_exact<NB, TAIL>(ctx, rows_fb, n_fb, T.rows, mt, block, k, WS_KNN_PART_A, ti, td, ratio_thr)));
        knnf_scatter_kernel<<<cdiv((long long) n_fb * width, 256), 256, 0, ctx->stream>>>(ti, td, fb + 1, n_fb, (int) width, idx, dist);
        LGR_HIP(ctx, hipGetLastError());
    }
    unsigned long long h[4];
    LGR_HIP(ctx, hipMemcpyAsync(h, dev, 32, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    last[1] += h[0] + (unsigned long long) n_fb * mt;
    last[2] += mq - n_fb; last[3] += n_fb;
    if (ctx->knnf_check) {
        float r;
        const unsigned bits = (unsigned) h[3];
        memcpy(&r, &bits, 4);
        *worst = std::max(*worst, (double) r);
        last[6] = (last[6] == ~0ull ? 0 : last[6]) + h[1] + h[2];
        if (h[1] + h[2]) {
            char msg[200];
            snprintf(msg, sizeof msg, "k-nearest filter self-check: %llu pairs outside the bound (worst |F - d2| / E = %g), %llu members of S_i not offered",
                     h[1], (double) r, h[2]);
            return lgr_fail(ctx, LGR_ERR_HIP, msg, __FILE__, __LINE__);
        }
    }
    return LGR_OK;
}

// the filtered call (ma, mb > 0): *done = false when it hands the whole call back to the exact path (reason in last[7])
template <int NB, int TAIL>
int knnd_match(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int k, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d,
               const float* ratio_thr, bool* done) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN;
    unsigned long long* last = ctx->knnf_last;
    *done = false;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    DensefSide A, B;
    float* centre;   // [LEN] the centre, 2^s, 2^2s, then the 64 x (LEN + 2) partial sums, counts and maxima
    LGR_TRY(lgr_ws_t(ctx, WS_KNND_CENTRE, (size_t) (LEN + 2) * (1 + DENSEF_CS_BLOCKS), &centre));
    const int n_s = std::min(mb, DENSEF_CS_BLOCKS * DENSEF_CS_ROWS);
    densef_centre_partial_kernel<LEN><<<DENSEF_CS_BLOCKS, 256, 0, ctx->stream>>>(d_b, n_s, mb / n_s, centre + LEN + 2);
    densef_centre_final_kernel<LEN><<<1, 256, 0, ctx->stream>>>(centre + LEN + 2, centre);
    LGR_TRY((densef_pack_side<NB, TAIL>(ctx, d_a, centre, ma, WS_KNND_OPS_A, WS_KNND_MISC_A, WS_KNND_IRR_A, &A)));
    LGR_TRY((densef_pack_side<NB, TAIL>(ctx, d_b, centre, mb, WS_KNND_OPS_B, WS_KNND_MISC_B, WS_KNND_IRR_B, &B)));
    LGR_HIP(ctx, hipMemcpyAsync(&A.n_irr, A.irr, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(&B.n_irr, B.irr, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (B.n_irr > DENSEF_IRR_CAP || (ba_i && A.n_irr > DENSEF_IRR_CAP)) { last[7] = KNNF_REASON_IRREGULAR; return LGR_OK; }
    last[0] = 1; last[4] = B.n_irr + (ba_i ? A.n_irr : 0); last[5] = DENSEF_CAP;
    if (ctx->knnf_check) { last[6] = 0; ctx->knnf_worst = 0; }
    LGR_TRY((knnd_direction<NB, TAIL>(ctx, A, B, centre, block, k, ab_i, ab_d, ratio_thr, last, &ctx->knnf_worst)));
    if (ba_i) LGR_TRY((knnd_direction<NB, TAIL>(ctx, B, A, centre, block, k, ba_i, ba_d, nullptr, last, &ctx->knnf_worst)));
    *done = true;
    return LGR_OK;
}

}  // namespace
