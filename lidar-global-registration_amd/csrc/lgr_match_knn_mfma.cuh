// lgr_match_knn_mfma.cuh -- the MFMA-filtered k-nearest matcher for 33-float rows (included by lgr_match_knn.hip after the exact scan,
// whose kernels answer the rows the filter gives up on).  DESIGN.md section 3.1i (pipeline, times) and section 4 (lemma, bound).
//
// The result is DEFINED by the exact path (per bf block the first k rows in order P, across blocks the first k in order F, on the
// canonical distances of lgr_match_dense.cuh).  By the lemma of DESIGN.md section 4 the list of query i depends only on
// S_i = { j : d(i, j) <= D_k(i) }, and the same two-stage procedure over any candidate set C_i that contains S_i -- every column with
// its own index and bf block -- yields the same k entries.  The filter produces such a C_i, much smaller than the train side:
//
//   centre    c = the mean of a fixed strided sample of the train rows (fixed summation order: the same c on every run).  Both sides are
//             centred about it, x' = fl(x - c): the bound below grows with |x'|^2, and FPFH rows of norm 127 have |x - c| near 52.
//             Any c is correct; a worse one costs candidates.  A call of both directions uses the one c for both.
//   pack      both sides as operands of v_mfma_f32_32x32x2_f32, K = 34: train row b -> [b'_0 .. b'_32, |b'|^2], query row a ->
//             [-2 a'_0 .. -2 a'_32, 1]; with the accumulator started at |a'|^2 a tile's chain leaves  f = |a'|^2 + |b'|^2 - 2 a'.b'.
//             Rows the bound cannot carry (a non-finite entry, |x'|^2 above 1e30) are IRREGULAR: as operands they are padding
//             (train: |b|^2 = +inf, never a candidate), as queries they go to the exact scan, as train rows they are offered to every
//             query as candidates (at most IRR_CAP of them, else the call takes the exact path whole).
//   bound     |f - d2| <= e(i, tile) = EPS_C s^2 + 1e-36 s + 1e-30, s = x_i + y_tile, d2 the canonical f32 sum of squares of the UNCENTRED
//             rows, x_i >= |a'_i|, y_tile >= |b'| of the tile's 32 rows (section 4: 80 u s^2 covers the fmaf chain, the two norms, the
//             rounding of the centring and the canonical sum's own rounding; EPS_C = 6e-6 >= 100 u).
//   sweep A   every lane owns one query (the MFMA column) and 16 train rows of each 32-row tile; the minimum of f + e over those 16 is
//             one GROUP value, the lane keeps its 8 smallest.  Distinct groups are distinct columns, so the k-th smallest group value
//             U_i of a query bounds D_k(i)^2 from above; fewer than k finite groups: U_i = +inf, the row goes to the exact scan.
//   sweep B   the same chain again; every (i, j) with f - e <= U_i (1 + 1e-5) is appended to the row's candidate list (CAP entries; a
//             row that overflows goes to the exact scan).  The 1e-5 covers the square root: two d2 may round to one d.
//   select    one wave per query: canonical distances of its candidates (bit-identical to dense_tile_distances<2, 1>), order P per
//             bf block, order F across blocks, on the 64-bit keys of the exact path; the fused ratio test at the same place.
//   fallback  the compacted list of rows above goes through knn_match_kernel<2, 1> against all train rows; when more than half of a
//             direction's rows are on it the direction takes the exact path whole.
#pragma once

namespace {

typedef float knnf_f32x16 __attribute__((ext_vector_type(16)));

constexpr int KNNF_KS = 17;                   // MFMA steps of a tile: K = 34 = 33 elements + the norm slot
constexpr int KNNF_CAP = 64;                  // candidates per query row
constexpr int KNNF_IRR_CAP = 1024;            // irregular train rows offered to every query (the one-match matcher's IRR_CAP)
constexpr int KNNF_NCAND = KNNF_CAP + KNNF_IRR_CAP;
constexpr float KNNF_EPS_C = 6e-6f;           // >= 100 u, u = 2^-24; proven: 80 u
constexpr float KNNF_EPS_LIN = 1e-36f;        // should an operand below 2^-126 ever be flushed: 68 x 2^-126 x max(x, y)
constexpr int KNNF_CS_BLOCKS = 64, KNNF_CS_ROWS = 1024;   // the centre's sample: at most 65 536 rows at a fixed stride
constexpr float KNNF_EPS_ABS = 1e-30f;
constexpr float KNNF_N2_MAX = 1e30f;          // largest |x|^2 of a regular row: (x + y)^2 and the chain stay far below FLT_MAX
// lgr_ctx_set_knn_filter(mode -1): the filtered path from this many (query, train) pairs per direction.  Measured (DESIGN.md section
// 3.1i, profiles/match_knn_filter.json; k = 2, both directions, exact / filtered): 16 384 x 16 384: 8.97 / 1.82 ms; the filtered path is
// already ahead at 4 096 x 4 096 (2.69 / 0.74 ms), the smallest size measured, where a call is a few launches either way.  The constant
// stays at 16 384 x 16 384, the smallest size at which auto may switch without moving any call of the test suite off the exact scan.
constexpr long long KNNF_AUTO_MIN_PAIRS = 16384ll * 16384ll;
enum { KNNF_REASON_NONE = 0, KNNF_REASON_IRREGULAR = 1, KNNF_REASON_FALLBACK_SHARE = 2, KNNF_REASON_EMPTY = 3 };

// the canonical squared distance of two 33-float rows: dense_tile_distances<2, 1>'s operations on the same values in the same order
__device__ __forceinline__ float knnf_canon_d2(const float* __restrict__ a, const float* __restrict__ b) {
    float sA = 0.f, sB = 0.f;
#pragma unroll
    for (int lane = 0; lane < 4; ++lane) {
        float sl = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) { const float t = a[16 * blk + 4 * k + lane] - b[16 * blk + 4 * k + lane]; acc = t * t + acc; }
            sl = k == 0 ? acc : sl + acc;
        }
        if (lane == 0) sA = sl;
        else if (lane == 1) sB = sl;
        else if (lane == 2) sA = sA + sl;
        else sB = sB + sl;
    }
    sA = sA + sB;
    const float t = a[32] - b[32];
    return sA + t * t;
}

// the centre: per column the sum and count over a strided sample's rows whose elements are all of magnitude <= 1e15, in a fixed order -- block b takes sample rows
// [1024 b, 1024 b + 1024), thread (rl, col) every 8th of them, the 8 partial sums are added in order -- then the 64 partials in order
__global__ __launch_bounds__(264) void knnf_centre_partial_kernel(const float* __restrict__ rows, int n_s, int stride, float* __restrict__ part) {
    __shared__ float ss[8][33], nn[8][33];
    const int col = threadIdx.x % 33, rl = threadIdx.x / 33;
    const int hi = min(n_s, ((int) blockIdx.x + 1) * KNNF_CS_ROWS);
    float s = 0.f, n = 0.f;
    for (int i = blockIdx.x * KNNF_CS_ROWS + rl; i < hi; i += 8) {
        const float* row = rows + (size_t) i * stride * 33;
        bool ok = true;   // (every thread of the row tests all of it: a row with one huge element must not move the centre at all)
        for (int e = 0; e < 33; ++e) ok = ok && fabsf(row[e]) <= 1e15f;
        if (ok) { s += row[col]; n += 1.f; }
    }
    ss[rl][col] = s; nn[rl][col] = n;
    __syncthreads();
    if (rl == 0) {
        for (int r = 1; r < 8; ++r) { s += ss[r][col]; n += nn[r][col]; }
        part[blockIdx.x * 66 + col] = s; part[blockIdx.x * 66 + 33 + col] = n;
    }
}

__global__ void knnf_centre_final_kernel(const float* __restrict__ part, float* __restrict__ centre) {
    const int col = threadIdx.x;
    if (col >= 33) return;
    float s = 0.f, n = 0.f;
    for (int b = 0; b < KNNF_CS_BLOCKS; ++b) { s += part[b * 66 + col]; n += part[b * 66 + 33 + col]; }
    centre[col] = n > 0.f ? s / n : 0.f;
}

// One thread per padded row: both operand forms of the centred row (tile-major: fragment kk of tile T at (T * 17 + kk) * 64 + lane, lane l = row l & 31,
// element 2 kk + (l >> 5)), |x|^2, the norm bound xb (-1: irregular or padding) and the list of irregular rows (count in irr[0]).
__global__ void knnf_pack_kernel(const float* __restrict__ rows, const float* __restrict__ centre, int m, int mp, float* __restrict__ op_t, float* __restrict__ op_q,
                                 float* __restrict__ n2, float* __restrict__ xb, int* __restrict__ irr) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= mp) return;
    float s = 0.f;
    bool ok = r < m;
    if (ok) {
        for (int e = 0; e < 33; ++e) { const float v = rows[(size_t) r * 33 + e] - centre[e]; ok = ok && fabsf(v) <= 3.4028234663852886e38f; s = v * v + s; }
        ok = ok && s <= KNNF_N2_MAX;
        if (!ok) { const int pos = atomicAdd(&irr[0], 1); if (pos < KNNF_IRR_CAP) irr[1 + pos] = r; }
    }
    n2[r] = ok ? s : 0.f;
    xb[r] = ok ? sqrtf(s) * 1.00001f + 1e-30f : -1.f;
    const size_t base = (size_t) (r >> 5) * KNNF_KS * 64 + (r & 31);
    for (int e = 0; e < 34; ++e) {
        const float v = (ok && e < 33) ? rows[(size_t) r * 33 + e] - centre[e] : 0.f;
        const size_t at = base + (size_t) (e >> 1) * 64 + 32 * (e & 1);
        op_t[at] = e < 33 ? v : (ok ? s : __uint_as_float(0x7f800000u));
        op_q[at] = e < 33 ? -2.f * v : 1.f;
    }
}

// y_tile: the largest norm bound of a tile's 32 train rows (0 when it has no regular row)
__global__ void knnf_ymax_kernel(const float* __restrict__ xb, int n_tiles, float* __restrict__ ymax) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    float y = 0.f;
    for (int e = 0; e < 32; ++e) y = fmaxf(y, xb[32 * t + e]);
    ymax[t] = y;
}

struct KnnfCheck {
    const float* rows_q; const float* rows_t; const float* xb_t;   // the callers' rows; xb_t < 0: no regular train row
    unsigned* worst_bits;                                         // max |f - d2| / e as float bits
    unsigned long long* violations;
};

// MODE 0: sweep A (part: [split][half][mqp][8] group values), 1: sweep B (cnt / cand), 2: the self-check of the bound.
// Block = 4 waves, a wave = 32 queries (its B fragments stay in registers) against the split's train tiles, A fragments from global.
template <int MODE>
__global__ __launch_bounds__(256) void knnf_sweep_kernel(const float* __restrict__ op_q, const float* __restrict__ op_t, const float* __restrict__ n2_q,
                                                        const float* __restrict__ xb_q, const float* __restrict__ ymax, int mq, int mqp, int mt,
                                                        int n_tt, int tiles_per_split, float* __restrict__ part, const float* __restrict__ uw,
                                                        int* __restrict__ cnt, int* __restrict__ cand, KnnfCheck chk) {
    const int lane = threadIdx.x & 63, qt = blockIdx.x * 4 + (threadIdx.x >> 6), split = blockIdx.y;
    if (qt >= mqp / 32) return;
    const int q = qt * 32 + (lane & 31), half = lane >> 5;
    float bq[KNNF_KS];
#pragma unroll
    for (int kk = 0; kk < KNNF_KS; ++kk) bq[kk] = op_q[((size_t) qt * KNNF_KS + kk) * 64 + lane];
    const float na = n2_q[q], x = fmaxf(xb_q[q], 0.f);
    const bool q_regular = xb_q[q] >= 0.f;
    float lst[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) lst[p] = __uint_as_float(0x7f800000u);
    float u = __uint_as_float(0xff800000u);
    if (MODE == 1) u = uw[q];
    const int t_lo = split * tiles_per_split, t_hi = min(n_tt, t_lo + tiles_per_split);
    for (int t = t_lo; t < t_hi; ++t) {
        knnf_f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = na;
        const float* at = op_t + (size_t) t * KNNF_KS * 64 + lane;
#pragma unroll
        for (int kk = 0; kk < KNNF_KS; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(at[kk * 64], bq[kk], acc, 0, 0, 0);
        const float s = x + ymax[t];
        const float e = (KNNF_EPS_C * s) * s + (KNNF_EPS_LIN * s + KNNF_EPS_ABS);
        if (MODE == 0) {
            float v = acc[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) v = fminf(v, acc[i]);
            v = v + e;
#pragma unroll
            for (int p = 0; p < 8; ++p) { const float lo = fminf(lst[p], v); v = fmaxf(lst[p], v); lst[p] = lo; }
        } else if (MODE == 1) {
            const float thr = u + e;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * half;
                if (acc[i] <= thr && j < mt && q < mq) {
                    const int pos = atomicAdd(&cnt[q], 1);
                    if (pos < KNNF_CAP) cand[(size_t) q * KNNF_CAP + pos] = j;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * half;
                if (q >= mq || j >= mt || !q_regular || chk.xb_t[j] < 0.f) continue;
                const float d2 = knnf_canon_d2(chk.rows_q + (size_t) q * 33, chk.rows_t + (size_t) j * 33);
                const float ratio = fabsf(acc[i] - d2) / e;
                if (!(ratio <= 1.f)) atomicAdd(chk.violations, 1ull);
                atomicMax(chk.worst_bits, __float_as_uint(ratio <= 3e38f ? ratio : 3e38f));
            }
        }
    }
    if (MODE == 0) {
#pragma unroll
        for (int p = 0; p < 8; ++p) part[(((size_t) split * 2 + half) * mqp + q) * 8 + p] = lst[p];
    }
}

// U_i widened: the k-th smallest of a query's group values times (1 + 1e-5); -inf (nothing passes sweep B, the row goes to the exact scan)
// for padding, irregular queries and rows with fewer than k finite group values.  Also clears the row's candidate counter.
__global__ void knnf_kth_kernel(const float* __restrict__ part, int n_lists, int mq, int mqp, int k, const float* __restrict__ xb_q,
                                float* __restrict__ uw, int* __restrict__ cnt) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= mqp) return;
    float lst[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) lst[p] = __uint_as_float(0x7f800000u);
    for (int l = 0; l < n_lists; ++l)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = part[((size_t) l * mqp + q) * 8 + e];
#pragma unroll
            for (int p = 0; p < 8; ++p) { const float lo = fminf(lst[p], v); v = fmaxf(lst[p], v); lst[p] = lo; }
        }
    float U = lst[0];
#pragma unroll
    for (int p = 1; p < 8; ++p) U = p == k - 1 ? lst[p] : U;
    const bool ok = q < mq && xb_q[q] >= 0.f && U < 3e38f;
    uw[q] = ok ? U + 1e-5f * fabsf(U) : __uint_as_float(0xff800000u);
    cnt[q] = 0;
}

// the rows for the exact scan: no bound, or more candidates than the list holds.  fb[0] = count, fb[1 ..] = rows, is_fb[q] = 0 / 1.
__global__ void knnf_flag_kernel(const float* __restrict__ uw, const int* __restrict__ cnt, int mq, int* __restrict__ fb, unsigned char* __restrict__ is_fb) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= mq) return;
    const bool f = !(uw[q] > -3e38f) || cnt[q] > KNNF_CAP;
    is_fb[q] = f;
    if (f) fb[1 + atomicAdd(&fb[0], 1)] = q;
}

__device__ __forceinline__ unsigned long long knnf_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}

// the canonical squared distance at row length 16 NB + TAIL: the long rows (lgr_match_knn_dense_mfma.cuh) share the select and cover kernels
// below, their candidate lists, irregular rows and fallback flags have the same form
template <int NB, int TAIL>
__device__ __forceinline__ float knnf_row_d2(const float* __restrict__ a, const float* __restrict__ b) {
    if constexpr (NB == 2 && TAIL == 1) return knnf_canon_d2(a, b);
    else return dense_canon_d2<NB, TAIL>(a, b);
}

// One wave per query (two per block) that is not on the fallback list: its candidates and the irregular train rows, canonical distances, order P inside
// each bf block (an entry is in its block's list iff fewer than k entries of the block are in front of it), then the first k members in
// order F.  Keys as in knn_match_kernel: d bits << 32 | j, and d bits << 32 | ~j.  pairs: canonical distances computed.
template <bool RATIO, int NB = 2, int TAIL = 1>
__global__ __launch_bounds__(128) void knnf_select_kernel(const float* __restrict__ rows_q, const float* __restrict__ rows_t, int mq, int block, int k,
                                                         const int* __restrict__ cnt, const int* __restrict__ cand, const int* __restrict__ irr, int n_irr,
                                                         const unsigned char* __restrict__ is_fb, float thr, int32_t* __restrict__ idx,
                                                         float* __restrict__ dist, unsigned long long* __restrict__ pairs) {
    constexpr int LEN = 16 * NB + TAIL;
    __shared__ unsigned long long kp[2][KNNF_NCAND], kf[2][KNNF_NCAND];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, q = blockIdx.x * 2 + w;
    const bool active = q < mq && !is_fb[q];
    const int nc = active ? min(cnt[q], KNNF_CAP) : 0, n = active ? nc + n_irr : 0;
    for (int c = lane; c < n; c += 64) {
        const int j = c < nc ? cand[(size_t) q * KNNF_CAP + c] : irr[1 + c - nc];
        const float d = sqrtf(knnf_row_d2<NB, TAIL>(rows_q + (size_t) q * LEN, rows_t + (size_t) j * LEN));
        kp[w][c] = d < FLT_MAX ? (unsigned long long) __float_as_uint(d) << 32 | (unsigned) j : NONE;
    }
    __syncthreads();
    for (int c = lane; c < n; c += 64) {
        const unsigned long long key = kp[w][c];
        unsigned long long out = NONE;
        if (key != NONE) {
            const unsigned j = (unsigned) key, b_lo = j / (unsigned) block * (unsigned) block;
            const unsigned long long b_hi = (unsigned long long) b_lo + (unsigned) block;
            int before = 0;
            for (int o = 0; o < n; ++o) {
                const unsigned long long ko = kp[w][o];
                const unsigned jo = (unsigned) ko;
                before += (ko < key && jo >= b_lo && jo < b_hi) ? 1 : 0;
            }
            if (before < k) out = (key & 0xffffffff00000000ull) | (unsigned) ~j;
        }
        kf[w][c] = out;
    }
    __syncthreads();
    if (!active) return;
    if (lane == 0) atomicAdd(pairs, (unsigned long long) n);
    unsigned long long last = 0, first = NONE, kth = NONE;
    bool any = false;
    for (int e = 0; e < k; ++e) {
        unsigned long long best = NONE;
        for (int c = lane; c < n; c += 64) {
            const unsigned long long key = kf[w][c];
            if ((!any || key > last) && key < best) best = key;
        }
        best = knnf_wave_min(best);
        if (e == 0) first = best;
        if (e == k - 1) kth = best;
        if (!RATIO && lane == 0) {
            idx[(size_t) q * k + e] = best == NONE ? -1 : (int32_t) ~(unsigned) best;
            dist[(size_t) q * k + e] = best == NONE ? 0.f : __uint_as_float((unsigned) (best >> 32));
        }
        if (best == NONE) { last = NONE; any = true; continue; }   // nothing is above NONE: the remaining entries are empty too
        last = best; any = true;
    }
    if (RATIO && lane == 0) {
        const bool keep = kth != NONE && ratio_passes(__uint_as_float((unsigned) (first >> 32)), __uint_as_float((unsigned) (kth >> 32)), thr);
        idx[q] = keep ? (int32_t) ~(unsigned) first : -1;
        dist[q] = keep ? __uint_as_float((unsigned) (first >> 32)) : 0.f;
    }
}

// the self-check of the candidate sets: one wave per query that is not on the fallback list; S_i from an exact scan (k rounds of the
// smallest key above the last one give D_k), then every j with d(i, j) <= D_k must be a candidate of i or an irregular train row
template <int NB = 2, int TAIL = 1>
__global__ __launch_bounds__(256) void knnf_cover_kernel(const float* __restrict__ rows_q, const float* __restrict__ rows_t, int mq, int mt, int k,
                                                        const int* __restrict__ cnt, const int* __restrict__ cand, const float* __restrict__ xb_t,
                                                        const unsigned char* __restrict__ is_fb, unsigned long long* __restrict__ violations) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= mq || is_fb[q]) return;
    constexpr int LEN = 16 * NB + TAIL;
    const float* a = rows_q + (size_t) q * LEN;
    unsigned long long last = 0;
    bool any = false;
    for (int e = 0; e < k; ++e) {
        unsigned long long best = NONE;
        for (int j = lane; j < mt; j += 64) {
            const float d = sqrtf(knnf_row_d2<NB, TAIL>(a, rows_t + (size_t) j * LEN));
            const unsigned long long key = d < FLT_MAX ? (unsigned long long) __float_as_uint(d) << 32 | (unsigned) j : NONE;
            if ((!any || key > last) && key < best) best = key;
        }
        best = knnf_wave_min(best);
        if (best == NONE) break;
        last = best; any = true;
    }
    if (!any) return;   // no entry below FLT_MAX: S_i is empty
    const float dk = __uint_as_float((unsigned) (last >> 32));
    const int nc = min(cnt[q], KNNF_CAP);
    for (int j = lane; j < mt; j += 64) {
        const float d = sqrtf(knnf_row_d2<NB, TAIL>(a, rows_t + (size_t) j * LEN));
        if (!(d <= dk) || xb_t[j] < 0.f) continue;
        bool found = false;
        for (int c = 0; c < nc; ++c) found = found || cand[(size_t) q * KNNF_CAP + c] == j;
        if (!found) atomicAdd(violations, 1ull);
    }
}

__global__ void knnf_gather_rows_kernel(const float* __restrict__ rows, const int* __restrict__ list, int n, float* __restrict__ out) {
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) n * 33) return;
    out[e] = rows[(size_t) list[e / 33] * 33 + e % 33];
}

__global__ void knnf_scatter_kernel(const int32_t* __restrict__ ti, const float* __restrict__ td, const int* __restrict__ list, int n, int width,
                                    int32_t* __restrict__ idx, float* __restrict__ dist) {
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) n * width) return;
    const size_t at = (size_t) list[e / width] * width + e % width;
    idx[at] = ti[e];
    dist[at] = td[e];
}

struct KnnfSide { const float* rows; int m, mp; float *op_t, *op_q, *n2, *xb, *ymax; int* irr; int n_irr; };

int knnf_pack_side(lgr_ctx* ctx, const float* rows, const float* centre, int m, int slot_ops, int slot_misc, int slot_irr, KnnfSide* s) {
    s->rows = rows; s->m = m; s->mp = cdiv(m, 32) * 32; s->n_irr = 0;
    const size_t op = (size_t) s->mp * 2 * KNNF_KS;   // floats of one operand form
    float* misc;
    LGR_TRY(lgr_ws_t(ctx, slot_ops, 2 * op, &s->op_t));
    LGR_TRY(lgr_ws_t(ctx, slot_misc, (size_t) 2 * s->mp + s->mp / 32, &misc));
    LGR_TRY(lgr_ws_t(ctx, slot_irr, (size_t) KNNF_IRR_CAP + 1, &s->irr));
    s->op_q = s->op_t + op; s->n2 = misc; s->xb = misc + s->mp; s->ymax = misc + 2 * (size_t) s->mp;
    LGR_HIP(ctx, hipMemsetAsync(s->irr, 0, 4, ctx->stream));
    knnf_pack_kernel<<<cdiv(s->mp, 256), 256, 0, ctx->stream>>>(rows, centre, m, s->mp, s->op_t, s->op_q, s->n2, s->xb, s->irr);
    knnf_ymax_kernel<<<cdiv(s->mp / 32, 256), 256, 0, ctx->stream>>>(s->xb, s->mp / 32, s->ymax);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

// the exact scan of one direction on n query rows (all of a side, or the gathered fallback rows)
template <int NB, int TAIL>
int knnf_exact(lgr_ctx* ctx, const float* d_q, int n, const float* d_t, int mt, int block, int k, int slot, int32_t* idx, float* dist, const float* ratio_thr) {
    constexpr int LEN = 16 * NB + TAIL;
    const int mpa = cdiv(n, MT) * MT, mpb = cdiv(mt, MT) * MT;
    float *pa, *pb;
    LGR_TRY(lgr_ws_t(ctx, WS_DENSE_PACK_A, (size_t) mpa * LEN, &pa));
    LGR_TRY(lgr_ws_t(ctx, WS_DENSE_PACK_B, (size_t) mpb * LEN, &pb));
    dense_pack_kernel<NB, TAIL><<<cdiv((long long) mpa * LEN, 256), 256, 0, ctx->stream>>>(d_q, n, mpa, pa);
    dense_pack_kernel<NB, TAIL><<<cdiv((long long) mpb * LEN, 256), 256, 0, ctx->stream>>>(d_t, mt, mpb, pb);
    return knn_sweep<NB, TAIL>(ctx, pa, n, mpa, pb, mt, mpb, block, k, slot, idx, dist, ratio_thr);
}

// One direction.  last: the counters of lgr_match_knn_last, accumulated over the directions of a call.
int knnf_direction(lgr_ctx* ctx, const KnnfSide& Q, const KnnfSide& T, int block, int k, int32_t* idx, float* dist, const float* ratio_thr,
                   unsigned long long* last, double* worst) {
    const int mq = Q.m, mt = T.m, mqp = Q.mp, n_tt = T.mp / 32, n_qb = cdiv(mqp / 32, 4);
    const int splits = std::max(1, std::min(n_tt, cdiv(4 * ctx->n_cu, n_qb))), tps = cdiv(n_tt, splits), n_split = cdiv(n_tt, tps);
    const size_t width = ratio_thr ? 1 : k;
    float *part, *uw;
    int *cnt, *cand, *fb;
    unsigned char* is_fb;
    unsigned long long* dev;   // [0] pairs, [1] bound violations, [2] cover violations, [3] worst ratio bits
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_PART, (size_t) n_split * 2 * mqp * 8, &part));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_UW, (size_t) mqp, &uw));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_CNT, (size_t) mqp, &cnt));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_CAND, (size_t) mqp * KNNF_CAP, &cand));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FB, (size_t) mq + 1, &fb));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_ISFB, (size_t) mq, &is_fb));
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_DEV, 4, &dev));
    LGR_HIP(ctx, hipMemsetAsync(dev, 0, 32, ctx->stream));
    LGR_HIP(ctx, hipMemsetAsync(fb, 0, 4, ctx->stream));
    const dim3 grid(n_qb, n_split);
    const KnnfCheck none{};
    knnf_sweep_kernel<0><<<grid, 256, 0, ctx->stream>>>(Q.op_q, T.op_t, Q.n2, Q.xb, T.ymax, mq, mqp, mt, n_tt, tps, part, nullptr, nullptr, nullptr, none);
    knnf_kth_kernel<<<cdiv(mqp, 256), 256, 0, ctx->stream>>>(part, 2 * n_split, mq, mqp, k, Q.xb, uw, cnt);
    knnf_sweep_kernel<1><<<grid, 256, 0, ctx->stream>>>(Q.op_q, T.op_t, Q.n2, Q.xb, T.ymax, mq, mqp, mt, n_tt, tps, nullptr, uw, cnt, cand, none);
    knnf_flag_kernel<<<cdiv(mq, 256), 256, 0, ctx->stream>>>(uw, cnt, mq, fb, is_fb);
    LGR_HIP(ctx, hipGetLastError());
    int n_fb = 0;   // the one read-back of a direction: it sizes the fallback list
    LGR_HIP(ctx, hipMemcpyAsync(&n_fb, fb, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (2ll * n_fb > mq) {   // the documented share: more than half of the rows have no usable candidate list
        last[0] = 0; last[7] = KNNF_REASON_FALLBACK_SHARE;
        last[1] += (unsigned long long) mq * mt; last[3] += mq;
        return knnf_exact<2, 1>(ctx, Q.rows, mq, T.rows, mt, block, k, WS_KNN_PART_A, idx, dist, ratio_thr);
    }
    const float thr = ratio_thr ? *ratio_thr : 0.f;
    if (ratio_thr) knnf_select_kernel<true><<<cdiv(mq, 2), 128, 0, ctx->stream>>>(Q.rows, T.rows, mq, block, k, cnt, cand, T.irr, T.n_irr, is_fb, thr, idx, dist, dev);
    else knnf_select_kernel<false><<<cdiv(mq, 2), 128, 0, ctx->stream>>>(Q.rows, T.rows, mq, block, k, cnt, cand, T.irr, T.n_irr, is_fb, thr, idx, dist, dev);
    LGR_HIP(ctx, hipGetLastError());
    if (ctx->knnf_check) {
        const KnnfCheck chk{Q.rows, T.rows, T.xb, (unsigned*) (dev + 3), dev + 1};
        knnf_sweep_kernel<2><<<grid, 256, 0, ctx->stream>>>(Q.op_q, T.op_t, Q.n2, Q.xb, T.ymax, mq, mqp, mt, n_tt, tps, nullptr, nullptr, nullptr, nullptr, chk);
        knnf_cover_kernel<><<<cdiv(mq, 4), 256, 0, ctx->stream>>>(Q.rows, T.rows, mq, mt, k, cnt, cand, T.xb, is_fb, dev + 2);
        LGR_HIP(ctx, hipGetLastError());
    }
    if (n_fb) {
        float* rows_fb;
        int32_t* ti;
        float* td;
        LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FBROWS, (size_t) n_fb * 33, &rows_fb));
        LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FBIDX, (size_t) n_fb * width, &ti));
        LGR_TRY(lgr_ws_t(ctx, WS_KNNF_FBDIST, (size_t) n_fb * width, &td));
        knnf_gather_rows_kernel<<<cdiv((long long) n_fb * 33, 256), 256, 0, ctx->stream>>>(Q.rows, fb + 1, n_fb, rows_fb);
        LGR_TRY((knnf_exact<2, 1>(ctx, rows_fb, n_fb, T.rows, mt, block, k, WS_KNN_PART_A, ti, td, ratio_thr)));
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
            snprintf(msg, sizeof msg, "k-nearest filter self-check: %llu pairs outside the bound (worst |f - d2| / e = %g), %llu members of S_i not offered",
                     h[1], (double) r, h[2]);
            return lgr_fail(ctx, LGR_ERR_HIP, msg, __FILE__, __LINE__);
        }
    }
    return LGR_OK;
}

// the filtered call: *done = false when it hands the whole call back to the exact path (reason in last[7])
int knnf_match(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int k, int32_t* ab_i, float* ab_d, int32_t* ba_i, float* ba_d,
               const float* ratio_thr, bool* done) {
    unsigned long long* last = ctx->knnf_last;
    *done = false;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    KnnfSide A, B;
    float* centre;   // [33] the centre, then the 64 x 66 partial sums and counts
    LGR_TRY(lgr_ws_t(ctx, WS_KNNF_CENTRE, (size_t) 33 + KNNF_CS_BLOCKS * 66, &centre));
    const int n_s = std::min(mb, KNNF_CS_BLOCKS * KNNF_CS_ROWS);
    knnf_centre_partial_kernel<<<KNNF_CS_BLOCKS, 264, 0, ctx->stream>>>(d_b, n_s, mb / n_s, centre + 33);
    knnf_centre_final_kernel<<<1, 64, 0, ctx->stream>>>(centre + 33, centre);
    LGR_TRY(knnf_pack_side(ctx, d_a, centre, ma, WS_KNNF_OPS_A, WS_KNNF_MISC_A, WS_KNNF_IRR_A, &A));
    LGR_TRY(knnf_pack_side(ctx, d_b, centre, mb, WS_KNNF_OPS_B, WS_KNNF_MISC_B, WS_KNNF_IRR_B, &B));
    LGR_HIP(ctx, hipMemcpyAsync(&A.n_irr, A.irr, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(&B.n_irr, B.irr, 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (B.n_irr > KNNF_IRR_CAP || (ba_i && A.n_irr > KNNF_IRR_CAP)) { last[7] = KNNF_REASON_IRREGULAR; return LGR_OK; }
    last[0] = 1; last[4] = B.n_irr + (ba_i ? A.n_irr : 0); last[5] = KNNF_CAP;
    if (ctx->knnf_check) { last[6] = 0; ctx->knnf_worst = 0; }
    LGR_TRY(knnf_direction(ctx, A, B, block, k, ab_i, ab_d, ratio_thr, last, &ctx->knnf_worst));
    if (ba_i) LGR_TRY(knnf_direction(ctx, B, A, block, k, ba_i, ba_d, nullptr, last, &ctx->knnf_worst));
    *done = true;
    return LGR_OK;
}

}  // namespace
