// lgr_match_dense_mfma.cuh -- the MFMA-filtered nearest-row matcher for the long rows, SHOT352 <22, 0> and RoPS135 <8, 7> (included by
// lgr_match_dense.hip after the exact scan, whose kernels answer what the filter gives up on).  DESIGN.md section 3.1a / 3.1b (pipeline,
// times) and section 4 (lemma for k = 1, bound).
//
// The result is DEFINED by the exact path: per query i the train row with the smallest key bits(d) << 32 | dense_tie_rank(j, block, nb)
// over all j with d < FLT_MAX, d = sqrtf(canonical d2) in the order of dense_tile_distances<NB, TAIL>.  It depends only on
// S_i = { j : d(i, j) <= D_1(i) }, and the same minimum over any candidate set C_i that contains S_i gives the same key.  The filter
// produces such a C_i:
//
//   centre    c = the mean of a fixed strided sample of the train rows (fixed summation order), and a scale 2^s, s in [-40, 40], that puts the
//             sample's largest |element| just below 2^13.  Both sides: x' = fl(x - c), X = x' 2^s.  A call of both directions uses one c, s.
//   pack      X = h1 + h2 + rho in f16, [h1 | h2] per row, stored as the 16-byte lane pieces of v_mfma_f32_32x32x16_f16 (lane l = row l & 31,
//             elements 16 chunk + 8 (l >> 5) + 0..7): piece ((tile NC + chunk) 2 + which) 64 + l.  The same form serves as the A (train) and
//             the B (query) operand; the chain of a chunk is t1.q1 + t1.q2 + t2.q1, 3 NC steps (66 / 27), nothing is stored a third time.
//             N = |X|^2 is summed in f64 and rounded once to f32; it stays outside the f16 chain: -N_a / 2 starts the accumulator,
//             F = N_b - 2 acc afterwards.  Rows the bound cannot carry are IRREGULAR (a non-finite element, an |X| element above 2^15 --
//             which also keeps N below 2^39): as operands they are zero rows with N = +inf (never a candidate, never in a minimum), as
//             queries they go to the exact scan, as train rows they are offered to every query (at most IRR_CAP, else the call takes the exact
//             path whole).  A row with a NON-FINITE element has no distance below FLT_MAX to any row: as a train row it is offered to nobody, as a
//             query its answer is -1 from the empty minimum.
//   bound     |F - d2 2^2s| <= E(i, tile) = EPS S^2 + 2.5e-3 S + 1e-5, S = x_i + y_tile (norm bounds of X, as xb / ymax of the k-nearest filter),
//             d2 the canonical sum on the UNCENTRED rows (2160 u for K = 1056, 910 u for K = 432, u = 2^-24).
//   sweep A   U_i = min over the regular train rows of F + E: an upper bound of D_1(i)^2 2^2s (atomicMin on the bits of a non-negative float:
//             an integer minimum, independent of arrival order).
//   sweep B   the same chain again; every (i, j) with F - E <= U_i (1 + 1e-5) is appended to row i's list (CAP entries, atomicAdd on the row's
//             counter; a row that overflows goes to the exact scan).  The 1e-5 covers the square root: two d2 may round to one d.
//   select    one wave per query: canonical distances of its candidates and of the irregular train rows (dense_canon_d2: bit-identical to
//             dense_tile_distances<NB, TAIL>), the wave-wide minimum of the exact path's keys, decoded as dense_match_decode does.
//   fallback  the compacted list of rows above goes through dense_match_kernel against all train rows and is scattered back; when more than
//             half of a direction's rows are on it the direction takes the exact path whole.
// Both directions: the sides are packed once, each direction sweeps for itself (as lgr_match_knn2_dev).
// The operand format, the sweep kernel and the packing of a side are in lgr_match_densef.cuh, shared with the k-nearest filter of these rows.
#pragma once

#include "lgr_match_densef.cuh"

namespace {

// lgr_ctx_set_dense_filter(mode -1): the filtered path from this many (query, train) pairs per direction.  Measured (DESIGN.md section 3.1a,
// profiles/match_dense_filter.json; both directions, block 10 000, exact / filtered ms): 135 floats, the row length that gains less:
// 4 096 x 4 096: 0.25 / 0.60, 16 384 x 16 384: 3.37 / 2.50, 35 913 x 35 913: 15.7 / 11.4, 50 000 x 50 000: 35.0 / 20.8; 352 floats:
// 0.95 / 0.85, 14.1 / 4.45, 72.1 / 20.8, 147.1 / 37.6.  16 384 x 16 384 is the smallest measured size from which the filtered path is ahead
// at every larger measured size for both row lengths (at 4 096 x 4 096 the 135-float call is a few launches and two read-backs behind).
constexpr long long DENSEF_AUTO_MIN_PAIRS = 16384ll * 16384ll;
enum { DENSEF_REASON_NONE = 0, DENSEF_REASON_IRREGULAR = 1, DENSEF_REASON_FALLBACK_SHARE = 2, DENSEF_REASON_EMPTY = 3 };

__device__ __forceinline__ unsigned long long densef_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}

// One wave per query that is not on the fallback list: the minimum of the exact path's keys over its candidates and the irregular train rows.
template <int NB, int TAIL>
__global__ __launch_bounds__(256) void densef_select_kernel(const float* __restrict__ rows_q, const float* __restrict__ rows_t, int mq, int block, int nb_t,
                                                           const int* __restrict__ cnt, const int* __restrict__ cand, const int* __restrict__ irr, int n_irr,
                                                           const unsigned char* __restrict__ is_fb, int32_t* __restrict__ idx, float* __restrict__ dist,
                                                           unsigned long long* __restrict__ pairs) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN;
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= mq || is_fb[q]) return;
    const int nc = min(cnt[q], DENSEF_CAP), n = nc + n_irr;
    unsigned long long best = ~0ull;
    for (int c = lane; c < n; c += 64) {
        const int j = c < nc ? cand[(size_t) q * DENSEF_CAP + c] : irr[1 + c - nc];
        const float d = sqrtf(dense_canon_d2<NB, TAIL>(rows_q + (size_t) q * LEN, rows_t + (size_t) j * LEN));
        if (d < FLT_MAX) {
            const unsigned long long key = (unsigned long long) __float_as_uint(d) << 32 | dense_tie_rank(j, block, nb_t);
            best = key < best ? key : best;
        }
    }
    best = densef_wave_min(best);
    if (lane != 0) return;
    atomicAdd(pairs, (unsigned long long) n);
    if (best == ~0ull) { idx[q] = -1; dist[q] = 0.f; return; }
    const unsigned r = (unsigned) best;
    const int bi = nb_t - 1 - (int) (r / (unsigned) block);
    idx[q] = bi * block + (int) (r % (unsigned) block);
    dist[q] = __uint_as_float((unsigned) (best >> 32));
}

// the self-check of the candidate sets: one wave per query that is not on the fallback list; D_1 from an exact scan, then every regular j with
// d(i, j) <= D_1 must be a candidate of i (the irregular train rows are offered to everyone)
template <int NB, int TAIL>
__global__ __launch_bounds__(256) void densef_cover_kernel(const float* __restrict__ rows_q, const float* __restrict__ rows_t, int mq, int mt,
                                                          const int* __restrict__ cnt, const int* __restrict__ cand, const float* __restrict__ xb_t,
                                                          const unsigned char* __restrict__ is_fb, unsigned long long* __restrict__ violations) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN;
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= mq || is_fb[q]) return;
    const float* a = rows_q + (size_t) q * LEN;
    unsigned best = 0xffffffffu;
    for (int j = lane; j < mt; j += 64) {
        const float d = sqrtf(dense_canon_d2<NB, TAIL>(a, rows_t + (size_t) j * LEN));
        if (d < FLT_MAX) best = min(best, __float_as_uint(d));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, (unsigned) __shfl_xor((int) best, o));
    if (best == 0xffffffffu) return;   // no entry below FLT_MAX: S_i is empty
    const float d1 = __uint_as_float(best);
    const int nc = min(cnt[q], DENSEF_CAP);
    for (int j = lane; j < mt; j += 64) {
        const float d = sqrtf(dense_canon_d2<NB, TAIL>(a, rows_t + (size_t) j * LEN));
        if (!(d <= d1) || xb_t[j] < 0.f) continue;
        bool found = false;
        for (int c = 0; c < nc; ++c) found = found || cand[(size_t) q * DENSEF_CAP + c] == j;
        if (!found) atomicAdd(violations, 1ull);
    }
}

__global__ void densef_scatter_kernel(const int32_t* __restrict__ ti, const float* __restrict__ td, const int* __restrict__ list, int n,
                                      int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    idx[list[e]] = ti[e];
    dist[list[e]] = td[e];
}

// One direction.  last: the counters of lgr_match_dense_last, accumulated over the directions of a call.
template <int NB, int TAIL>
int densef_direction(lgr_ctx* ctx, const DensefSide& Q, const DensefSide& T, const float* centre, int block, int32_t* idx, float* dist,
                     unsigned long long* last, double* worst) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN;
    const int mq = Q.m, mt = T.m, mqp = Q.mp;
    unsigned* ubits;
    int *cnt, *cand, *fb;
    unsigned char* is_fb;
    unsigned long long* dev;   // [0] pairs, [1] bound violations, [2] cover violations, [3] worst ratio bits
    LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_U, (size_t) mqp, &ubits));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_CNT, (size_t) mqp, &cnt));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_CAND, (size_t) mqp * DENSEF_CAP, &cand));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_FB, (size_t) mq + 1, &fb));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_ISFB, (size_t) mq, &is_fb));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_DEV, 4, &dev));
    LGR_HIP(ctx, hipMemsetAsync(dev, 0, 32, ctx->stream));
    LGR_HIP(ctx, hipMemsetAsync(fb, 0, 4, ctx->stream));
    LGR_HIP(ctx, hipMemsetAsync(cnt, 0, (size_t) mqp * 4, ctx->stream));
    LGR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t) ubits, 0x7f800000, (size_t) mqp, ctx->stream));
    const DensefCheck none{};
    LGR_TRY((densef_sweep<NB, TAIL, 0>(ctx, Q, T, ubits, cnt, cand, none)));
    LGR_TRY((densef_sweep<NB, TAIL, 1>(ctx, Q, T, ubits, cnt, cand, none)));
    densef_flag_kernel<<<cdiv(mq, 256), 256, 0, ctx->stream>>>(Q.xb, ubits, cnt, mq, fb, is_fb);
    LGR_HIP(ctx, hipGetLastError());
    int n_fb = 0;   // the one read-back of a direction: it sizes the fallback list
    LGR_HIP(ctx, hipMemcpyAsync(&n_fb, fb, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (2ll * n_fb > mq) {   // the documented share: more than half of the rows have no usable candidate list
        last[0] = 0; last[7] = DENSEF_REASON_FALLBACK_SHARE;
        last[1] += (unsigned long long) mq * mt; last[3] += mq;
        return dense_exact<NB, TAIL>(ctx, Q.rows, mq, T.rows, mt, block, idx, dist, nullptr, nullptr);
    }
    densef_select_kernel<NB, TAIL><<<cdiv(mq, 4), 256, 0, ctx->stream>>>(Q.rows, T.rows, mq, block, cdiv(mt, block), cnt, cand, T.irr, T.n_irr, is_fb, idx, dist, dev);
    LGR_HIP(ctx, hipGetLastError());
    if (ctx->densef_check) {
        const DensefCheck chk{Q.rows, T.rows, T.xb, centre, (unsigned*) (dev + 3), dev + 1};
        LGR_TRY((densef_sweep<NB, TAIL, 2>(ctx, Q, T, ubits, cnt, cand, chk)));
        densef_cover_kernel<NB, TAIL><<<cdiv(mq, 4), 256, 0, ctx->stream>>>(Q.rows, T.rows, mq, mt, cnt, cand, T.xb, is_fb, dev + 2);
        LGR_HIP(ctx, hipGetLastError());
    }
    if (n_fb) {
        float* rows_fb;
        int32_t* ti;
        float* td;
        LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_FBROWS, (size_t) n_fb * LEN, &rows_fb));
        LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_FBIDX, (size_t) n_fb, &ti));
        LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_FBDIST, (size_t) n_fb, &td));
        densef_gather_rows_kernel<<<cdiv((long long) n_fb * LEN, 256), 256, 0, ctx->stream>>>(Q.rows, fb + 1, n_fb, LEN, rows_fb);
        LGR_TRY((dense_exact<NB, TAIL>(ctx, rows_fb, n_fb, T.rows, mt, block, ti, td, nullptr, nullptr)));
        densef_scatter_kernel<<<cdiv(n_fb, 256), 256, 0, ctx->stream>>>(ti, td, fb + 1, n_fb, idx, dist);
        LGR_HIP(ctx, hipGetLastError());
    }
    unsigned long long h[4];
    LGR_HIP(ctx, hipMemcpyAsync(h, dev, 32, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    last[1] += h[0] + (unsigned long long) n_fb * mt;
    last[2] += mq - n_fb; last[3] += n_fb;
    if (ctx->densef_check) {
        float r;
        const unsigned bits = (unsigned) h[3];
        memcpy(&r, &bits, 4);
        *worst = std::max(*worst, (double) r);
        last[6] = (last[6] == ~0ull ? 0 : last[6]) + h[1] + h[2];
        if (h[1] + h[2]) {
            char msg[200];
            snprintf(msg, sizeof msg, "dense filter self-check: %llu pairs outside the bound (worst |F - d2| / E = %g), %llu members of S_i not offered",
                     h[1], (double) r, h[2]);
            return lgr_fail(ctx, LGR_ERR_HIP, msg, __FILE__, __LINE__);
        }
    }
    return LGR_OK;
}

// the filtered call (ma, mb > 0): *done = false when it hands the whole call back to the exact path (reason in last[7])
template <int NB, int TAIL>
int densef_match(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d, bool* done) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN;
    unsigned long long* last = ctx->densef_last;
    *done = false;
    DensefSide A, B;
    float* centre;   // [LEN] the centre, 2^s, 2^2s, then the 64 x (LEN + 2) partial sums, counts and maxima
    LGR_TRY(lgr_ws_t(ctx, WS_DENSEF_CENTRE, (size_t) (LEN + 2) * (1 + DENSEF_CS_BLOCKS), &centre));
    const int n_s = std::min(mb, DENSEF_CS_BLOCKS * DENSEF_CS_ROWS);
    densef_centre_partial_kernel<LEN><<<DENSEF_CS_BLOCKS, 256, 0, ctx->stream>>>(d_b, n_s, mb / n_s, centre + LEN + 2);
    densef_centre_final_kernel<LEN><<<1, 256, 0, ctx->stream>>>(centre + LEN + 2, centre);
    LGR_TRY((densef_pack_side<NB, TAIL>(ctx, d_a, centre, ma, WS_DENSEF_OPS_A, WS_DENSEF_MISC_A, WS_DENSEF_IRR_A, &A)));
    LGR_TRY((densef_pack_side<NB, TAIL>(ctx, d_b, centre, mb, WS_DENSEF_OPS_B, WS_DENSEF_MISC_B, WS_DENSEF_IRR_B, &B)));
    LGR_HIP(ctx, hipMemcpyAsync(&A.n_irr, A.irr, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(&B.n_irr, B.irr, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (B.n_irr > DENSEF_IRR_CAP || (ba_i && A.n_irr > DENSEF_IRR_CAP)) { last[7] = DENSEF_REASON_IRREGULAR; return LGR_OK; }
    last[0] = 1; last[4] = B.n_irr + (ba_i ? A.n_irr : 0); last[5] = DENSEF_CAP;
    if (ctx->densef_check) { last[6] = 0; ctx->densef_worst = 0; }
    LGR_TRY((densef_direction<NB, TAIL>(ctx, A, B, centre, block, ab_i, ab_d, last, &ctx->densef_worst)));
    if (ba_i) LGR_TRY((densef_direction<NB, TAIL>(ctx, B, A, centre, block, ba_i, ba_d, last, &ctx->densef_worst)));
    *done = true;
    return LGR_OK;
}

}  // namespace
