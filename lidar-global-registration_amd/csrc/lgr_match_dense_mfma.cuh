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
#pragma once

namespace {

typedef _Float16 densef_f16x8 __attribute__((ext_vector_type(8)));
typedef float densef_f32x16 __attribute__((ext_vector_type(16)));

constexpr int DENSEF_CAP = 64;                  // candidates per query row
constexpr int DENSEF_IRR_CAP = 1024;            // irregular train rows offered to every query
constexpr int DENSEF_BLK = 128;                 // rows of a workgroup's block on either side: 4 tiles of 32, 2 x 2 tiles per wave
constexpr int DENSEF_CS_BLOCKS = 64, DENSEF_CS_ROWS = 256;   // the centre's sample: at most 16 384 rows at a fixed stride
constexpr float DENSEF_X_MAX = 32768.f;         // largest |X| element of a regular row: h1 holds it with room to 65504
constexpr float DENSEF_EPS_LIN = 2.5e-3f;       // >= 2.002 x 2^-14 x sqrt(352) = 2.293e-3: f16 terms below 2^-14, should the MFMA flush them
constexpr float DENSEF_EPS_ABS = 1e-5f;         // >= 2 x 2^-28 x 352 = 2.7e-6, and f32 underflow of a square at s <= 40
// lgr_ctx_set_dense_filter(mode -1): the filtered path from this many (query, train) pairs per direction.  Measured (DESIGN.md section 3.1a,
// profiles/match_dense_filter.json; both directions, block 10 000, exact / filtered ms): 135 floats, the row length that gains less:
// 4 096 x 4 096: 0.25 / 0.60, 16 384 x 16 384: 3.37 / 2.50, 35 913 x 35 913: 15.7 / 11.4, 50 000 x 50 000: 35.0 / 20.8; 352 floats:
// 0.95 / 0.85, 14.1 / 4.45, 72.1 / 20.8, 147.1 / 37.6.  16 384 x 16 384 is the smallest measured size from which the filtered path is ahead
// at every larger measured size for both row lengths (at 4 096 x 4 096 the 135-float call is a few launches and two read-backs behind).
constexpr long long DENSEF_AUTO_MIN_PAIRS = 16384ll * 16384ll;
enum { DENSEF_REASON_NONE = 0, DENSEF_REASON_IRREGULAR = 1, DENSEF_REASON_FALLBACK_SHARE = 2, DENSEF_REASON_EMPTY = 3 };

template <int NB, int TAIL>
struct DenseF {
    static constexpr int LEN = 16 * NB + TAIL, KP = (LEN + 15) / 16 * 16, NC = KP / 16;   // 352 / 352 / 22; 135 / 144 / 9
    static constexpr int BK = NC % 2 == 0 ? 2 : 1;                                       // chunks of 16 per LDS stage
    // proven: (6 KP x 1.0012 + 40.1) u -> 2160 u = 1.2875e-4 at K = 1056, 910 u = 5.424e-5 at K = 432; the constants
    // below are 8.7 % and 10.6 % above them
    static constexpr float EPS = KP == 352 ? 1.4e-4f : 6e-5f;
    static_assert(KP == 352 || KP == 144, "derive EPS for this row length");
    static_assert(KP / 8 <= 64, "one wave packs a row");
};

// the canonical squared distance of two rows: dense_tile_distances<NB, TAIL>'s operations on the same values in the same order
template <int NB, int TAIL>
__device__ __forceinline__ float dense_canon_d2(const float* __restrict__ a, const float* __restrict__ b) {
    float sA = 0.f, sB = 0.f;
    for (int lane = 0; lane < 4; ++lane) {
        float sl = 0.f;
        for (int k = 0; k < 4; ++k) {
            float acc = 0.f;
            for (int blk = 0; blk < NB; ++blk) { const float t = a[16 * blk + 4 * k + lane] - b[16 * blk + 4 * k + lane]; acc = t * t + acc; }
            sl = k == 0 ? acc : sl + acc;
        }
        if (lane == 0) sA = sl;
        else if (lane == 1) sB = sl;
        else if (lane == 2) sA = sA + sl;
        else sB = sB + sl;
    }
    if (TAIL == 0) return sA + sB;
    sA = sA + sB;
    for (int e = 0; e < TAIL; ++e) { const float t = a[16 * NB + e] - b[16 * NB + e]; sA = sA + t * t; }
    return sA;
}

// the centre and the scale: block b takes sample rows [256 b, 256 b + 256); a row with an element that is not of magnitude <= 1e15 is left out
// whole; per column the rows are added in order, the 64 partials in order.  part: per block LEN sums, the row count, the largest |element|.
template <int LEN>
__global__ __launch_bounds__(256) void densef_centre_partial_kernel(const float* __restrict__ rows, int n_s, int stride, float* __restrict__ part) {
    __shared__ unsigned char ok_s[DENSEF_CS_ROWS];
    __shared__ float mx_s[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lo = blockIdx.x * DENSEF_CS_ROWS, hi = min(n_s, lo + DENSEF_CS_ROWS);
    float mx = 0.f;
    for (int i = lo + 64 * w; i < min(hi, lo + 64 * w + 64); ++i) {
        const float* row = rows + (size_t) i * stride * LEN;
        bool ok = true;
        float m = 0.f;
        for (int e = lane; e < LEN; e += 64) { const float v = fabsf(row[e]); ok = ok && v <= 1e15f; m = fmaxf(m, v); }
        ok = __ballot(!ok) == 0ull;
        if (ok) mx = fmaxf(mx, m);
        if (lane == 0) ok_s[i - lo] = ok;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if (lane == 0) mx_s[w] = mx;
    __syncthreads();
    float* out = part + (size_t) blockIdx.x * (LEN + 2);
    for (int col = tid; col < LEN; col += 256) {
        float s = 0.f;
        for (int i = lo; i < hi; ++i) if (ok_s[i - lo]) s += rows[(size_t) i * stride * LEN + col];
        out[col] = s;
    }
    if (tid == 0) {
        float n = 0.f;
        for (int i = lo; i < hi; ++i) n += ok_s[i - lo] ? 1.f : 0.f;
        out[LEN] = n;
        out[LEN + 1] = fmaxf(fmaxf(mx_s[0], mx_s[1]), fmaxf(mx_s[2], mx_s[3]));
    }
}

// centre[0 .. LEN) the mean, centre[LEN] = 2^s, centre[LEN + 1] = 2^2s.  |x - c| <= 2 max|x| over the sample (c is a mean of it), so with
// max|x| < 2^e the scale 2^(13 - e) keeps the sample's |X| below 2^14; s is clamped to [-40, 40], where neither 2^2s nor the canonical sum of
// two regular rows (|x'| <= 2^55) leaves the f32 range.
template <int LEN>
__global__ void densef_centre_final_kernel(const float* __restrict__ part, float* __restrict__ centre) {
    for (int col = threadIdx.x; col < LEN; col += blockDim.x) {
        float s = 0.f, n = 0.f;
        for (int b = 0; b < DENSEF_CS_BLOCKS; ++b) { s += part[(size_t) b * (LEN + 2) + col]; n += part[(size_t) b * (LEN + 2) + LEN]; }
        centre[col] = n > 0.f ? s / n : 0.f;
    }
    if (threadIdx.x == 0) {
        float mx = 0.f;
        for (int b = 0; b < DENSEF_CS_BLOCKS; ++b) mx = fmaxf(mx, part[(size_t) b * (LEN + 2) + LEN + 1]);
        int s = 0;
        if (mx > 0.f) s = 13 - ((int) ((__float_as_uint(mx) >> 23) & 0xffu) - 126);   // mx < 2^e, e = biased exponent - 126
        s = max(-40, min(40, s));
        centre[LEN] = __uint_as_float((unsigned) (127 + s) << 23);
        centre[LEN + 1] = __uint_as_float((unsigned) (127 + 2 * s) << 23);
    }
}

// One wave per padded row, lane p the elements 8 p .. 8 p + 7: the row's [h1 | h2] pieces, N (+inf unless regular), the norm bound xb (-1: irregular
// with finite elements, -2: a non-finite element or padding) and the list of the irregular rows with finite elements (count in irr[0]).
template <int NB, int TAIL>
__global__ __launch_bounds__(256) void densef_pack_kernel(const float* __restrict__ rows, const float* __restrict__ centre, int m, int mp,
                                                         densef_f16x8* __restrict__ ops, float* __restrict__ n2, float* __restrict__ xb, int* __restrict__ irr) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN, KP = DenseF<NB, TAIL>::KP, NC = DenseF<NB, TAIL>::NC;
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= mp) return;
    const float scale = centre[LEN];
    float X[8];
    bool fin = true, fits = true;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int e = 8 * lane + j;
        float v = 0.f;
        if (r < m && e < LEN) {
            const float raw = rows[(size_t) r * LEN + e];
            fin = fin && fabsf(raw) <= 3.4028234663852886e38f;
            const float c = raw - centre[e];
            v = c * scale;
            fits = fits && fabsf(v) <= DENSEF_X_MAX;
        }
        X[j] = v;
        s += (double) v * (double) v;
    }
    fin = __ballot(!fin) == 0ull && r < m;
    const bool ok = fin && __ballot(!fits) == 0ull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float N = (float) s;
    if (lane == 0) {
        n2[r] = ok ? N : __uint_as_float(0x7f800000u);
        xb[r] = ok ? sqrtf(N) * 1.00001f + 1e-30f : (fin ? -1.f : -2.f);
        if (fin && !ok) { const int pos = atomicAdd(&irr[0], 1); if (pos < DENSEF_IRR_CAP) irr[1 + pos] = r; }
    }
    if (lane < KP / 8) {
        densef_f16x8 h1, h2;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = ok ? X[j] : 0.f;
            h1[j] = (_Float16) v;
            h2[j] = (_Float16) (v - (float) h1[j]);
        }
        const size_t at = ((size_t) (r >> 5) * NC + (lane >> 1)) * 128 + (r & 31) + 32 * (lane & 1);
        ops[at] = h1;
        ops[at + 64] = h2;
    }
}

// y_tile: the largest norm bound of a tile's 32 train rows (0 when it has no regular row)
__global__ void densef_ymax_kernel(const float* __restrict__ xb, int n_tiles, float* __restrict__ ymax) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    float y = 0.f;
    for (int e = 0; e < 32; ++e) y = fmaxf(y, xb[32 * t + e]);
    ymax[t] = y;
}

struct DensefCheck {
    const float* rows_q; const float* rows_t; const float* xb_t;   // the callers' rows; xb_t < 0: not a regular train row
    const float* centre;                                          // [LEN + 1]: 2^2s
    unsigned* worst_bits;                                         // max |F - d2 2^2s| / E as float bits
    unsigned long long* violations;
};

// The sweep: an LDS-staged GEMM tile whose epilogue is the filter.  MODE 0: sweep A (ubits), 1: sweep B (cnt / cand), 2: the self-check of the
// bound.  Block = 4 waves = 128 queries x a stream of 128-row train blocks; wave (wq, wt) owns query tiles 2 wq, 2 wq + 1 and train tiles
// 2 wt, 2 wt + 1 of the block: four accumulator tiles.  The query is the MFMA column: a lane owns one query and 16 train rows of a tile.
// K goes through LDS in stages of BK chunks, both sides, double-buffered through registers: the pieces of stage n + 1 are loaded before the
// chains of stage n and stored behind them, one barrier per stage.  The operands are stored in the instruction's lane order, so a stage is a
// straight copy and every fragment read is one lane-linear 16-byte LDS read (conflict-free); per chunk a wave issues 8 reads for 12 MFMAs.
template <int NB, int TAIL, int MODE>
__global__ __launch_bounds__(256) void densef_sweep_kernel(const densef_f16x8* __restrict__ op_q, const densef_f16x8* __restrict__ op_t,
                                                          const float* __restrict__ n2_q, const float* __restrict__ xb_q, const float* __restrict__ n2_t,
                                                          const float* __restrict__ ymax, int mq, int mt, int n_tb, int tb_per_split,
                                                          unsigned* __restrict__ ubits, int* __restrict__ cnt, int* __restrict__ cand, DensefCheck chk) {
    constexpr int LEN = DenseF<NB, TAIL>::LEN, NC = DenseF<NB, TAIL>::NC, BK = DenseF<NB, TAIL>::BK, NS = NC / BK;
    constexpr int SIDE = 512 * BK, PIECES = 2 * SIDE, PER = PIECES / 256;   // 16-byte pieces of a stage: [side][tile 0..3][chunk][h1 | h2][lane]
    constexpr float EPS = DenseF<NB, TAIL>::EPS;
    extern __shared__ densef_f16x8 densef_sm[];   // [2][PIECES]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wq = w & 1, wt = w >> 1, half = lane >> 5;
    const int qb = blockIdx.x;
    const int tb_lo = blockIdx.y * tb_per_split, tb_hi = min(n_tb, tb_lo + tb_per_split);
    if (tb_lo >= tb_hi) return;

    int q[2];
    float x[2], acc0[2], um[2], uw[2];
    bool qreg[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        q[a] = qb * DENSEF_BLK + (2 * wq + a) * 32 + (lane & 31);
        const float xbq = xb_q[q[a]];
        qreg[a] = xbq >= 0.f && q[a] < mq;
        x[a] = fmaxf(xbq, 0.f);
        acc0[a] = qreg[a] ? -0.5f * n2_q[q[a]] : 0.f;
        um[a] = __uint_as_float(0x7f800000u);
        uw[a] = __uint_as_float(0xff800000u);
        if (MODE == 1) {
            const float U = __uint_as_float(ubits[q[a]]);
            if (qreg[a] && U < 3e38f) uw[a] = U + 1e-5f * U;
        }
    }
    float scale2 = 0.f;
    if (MODE == 2) scale2 = chk.centre[LEN + 1];

    densef_f16x8 pre[PER];
    auto load = [&](int tb, int st) {
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int p = tid + 256 * r, side = p / SIDE, rem = p % SIDE, tile = rem / (128 * BK), off = rem % (128 * BK);
            const densef_f16x8* src = side ? op_t + ((size_t) (tb * 4 + tile) * NC + st * BK) * 128 : op_q + ((size_t) (qb * 4 + tile) * NC + st * BK) * 128;
            pre[r] = src[off];
        }
    };
    auto store = [&](int buf) {
#pragma unroll
        for (int r = 0; r < PER; ++r) densef_sm[buf * PIECES + tid + 256 * r] = pre[r];
    };

    densef_f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[a][b][i] = acc0[a];

    const int total = (tb_hi - tb_lo) * NS;
    load(tb_lo, 0);
    store(0);
    __syncthreads();
    int tb = tb_lo, st = 0;
    for (int it = 0; it < total; ++it) {
        int ntb = tb, nst = st + 1;
        if (nst == NS) { nst = 0; ++ntb; }
        const bool more = it + 1 < total;
        if (more) load(ntb, nst);
        const densef_f16x8* sq = densef_sm + (it & 1) * PIECES + (2 * wq) * 128 * BK + lane;
        const densef_f16x8* stt = densef_sm + (it & 1) * PIECES + SIDE + (2 * wt) * 128 * BK + lane;
#pragma unroll
        for (int kc = 0; kc < BK; ++kc) {
            densef_f16x8 q1[2], q2[2], t1[2], t2[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                q1[a] = sq[a * 128 * BK + kc * 128];
                q2[a] = sq[a * 128 * BK + kc * 128 + 64];
                t1[a] = stt[a * 128 * BK + kc * 128];
                t2[a] = stt[a * 128 * BK + kc * 128 + 64];
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(t1[b], q1[a], acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(t1[b], q2[a], acc[a][b], 0, 0, 0);
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(t2[b], q1[a], acc[a][b], 0, 0, 0);
                }
        }
        if (more) store((it + 1) & 1);
        __syncthreads();
        if (st == NS - 1) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    const int tile = tb * 4 + 2 * wt + b;
                    const float s = x[a] + ymax[tile];
                    const float E = (EPS * s) * s + (DENSEF_EPS_LIN * s + DENSEF_EPS_ABS);
                    float F[16];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const float4 nb4 = *reinterpret_cast<const float4*>(n2_t + tile * 32 + 8 * g + 4 * half);
                        F[4 * g + 0] = nb4.x - 2.f * acc[a][b][4 * g + 0];
                        F[4 * g + 1] = nb4.y - 2.f * acc[a][b][4 * g + 1];
                        F[4 * g + 2] = nb4.z - 2.f * acc[a][b][4 * g + 2];
                        F[4 * g + 3] = nb4.w - 2.f * acc[a][b][4 * g + 3];
                    }
                    if (MODE == 0) {
                        float v = F[0];
#pragma unroll
                        for (int i = 1; i < 16; ++i) v = fminf(v, F[i]);
                        um[a] = fminf(um[a], fmaxf(v + E, 0.f));   // (v + E >= d2 2^2s >= 0: the clamp changes nothing the proof allows)
                    } else if (MODE == 1) {
                        const float thr = uw[a] + E;
#pragma unroll
                        for (int i = 0; i < 16; ++i) {
                            const int j = tile * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
                            if (F[i] <= thr && j < mt) {
                                const int pos = atomicAdd(&cnt[q[a]], 1);
                                if (pos < DENSEF_CAP) cand[(size_t) q[a] * DENSEF_CAP + pos] = j;
                            }
                        }
                    } else {
#pragma unroll 1
                        for (int i = 0; i < 16; ++i) {   // (one copy of the canonical sum; F[i] by a select chain, never an indexed register array)
                            const int j = tile * 32 + (i & 3) + 8 * (i >> 2) + 4 * half;
                            float Fi = F[0];
#pragma unroll
                            for (int k = 1; k < 16; ++k) Fi = i == k ? F[k] : Fi;
                            if (!qreg[a] || j >= mt || chk.xb_t[j] < 0.f) continue;
                            const float d2 = dense_canon_d2<NB, TAIL>(chk.rows_q + (size_t) q[a] * LEN, chk.rows_t + (size_t) j * LEN) * scale2;
                            const float ratio = fabsf(Fi - d2) / E;
                            if (!(ratio <= 1.f)) atomicAdd(chk.violations, 1ull);
                            atomicMax(chk.worst_bits, __float_as_uint(ratio <= 3e38f ? ratio : 3e38f));
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[a][b][i] = acc0[a];
                }
        }
        tb = ntb; st = nst;
    }
    if (MODE == 0) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
            if (qreg[a]) atomicMin(&ubits[q[a]], __float_as_uint(um[a]));
    }
}

// the rows for the exact scan: irregular rows with finite elements, regular rows without a bound (no regular train row) or with more candidates
// than the list holds.  fb[0] = count, fb[1 ..] = rows, is_fb[q] = 0 / 1.  A row with a non-finite element matches nothing: it stays off the list.
__global__ void densef_flag_kernel(const float* __restrict__ xb_q, const unsigned* __restrict__ ubits, const int* __restrict__ cnt, int mq,
                                   int* __restrict__ fb, unsigned char* __restrict__ is_fb) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= mq) return;
    const float xbq = xb_q[q];
    const bool f = xbq == -1.f || (xbq >= 0.f && (!(__uint_as_float(ubits[q]) < 3e38f) || cnt[q] > DENSEF_CAP));
    is_fb[q] = f;
    if (f) fb[1 + atomicAdd(&fb[0], 1)] = q;
}

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

__global__ void densef_gather_rows_kernel(const float* __restrict__ rows, const int* __restrict__ list, int n, int len, float* __restrict__ out) {
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) n * len) return;
    out[e] = rows[(size_t) list[e / len] * len + e % len];
}

__global__ void densef_scatter_kernel(const int32_t* __restrict__ ti, const float* __restrict__ td, const int* __restrict__ list, int n,
                                      int32_t* __restrict__ idx, float* __restrict__ dist) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    idx[list[e]] = ti[e];
    dist[list[e]] = td[e];
}

struct DensefSide { const float* rows; int m, mp; densef_f16x8* ops; float *n2, *xb, *ymax; int* irr; int n_irr; };

template <int NB, int TAIL>
int densef_pack_side(lgr_ctx* ctx, const float* rows, const float* centre, int m, int slot_ops, int slot_misc, int slot_irr, DensefSide* s) {
    constexpr int NC = DenseF<NB, TAIL>::NC;
    s->rows = rows; s->m = m; s->mp = cdiv(m, DENSEF_BLK) * DENSEF_BLK; s->n_irr = 0;
    float* misc;
    LGR_TRY(lgr_ws_t(ctx, slot_ops, (size_t) (s->mp / 32) * NC * 128, &s->ops));
    LGR_TRY(lgr_ws_t(ctx, slot_misc, (size_t) 2 * s->mp + s->mp / 32, &misc));
    LGR_TRY(lgr_ws_t(ctx, slot_irr, (size_t) DENSEF_IRR_CAP + 1, &s->irr));
    s->n2 = misc; s->xb = misc + s->mp; s->ymax = misc + 2 * (size_t) s->mp;
    LGR_HIP(ctx, hipMemsetAsync(s->irr, 0, 4, ctx->stream));
    densef_pack_kernel<NB, TAIL><<<s->mp / 4, 256, 0, ctx->stream>>>(rows, centre, m, s->mp, s->ops, s->n2, s->xb, s->irr);
    densef_ymax_kernel<<<cdiv(s->mp / 32, 256), 256, 0, ctx->stream>>>(s->xb, s->mp / 32, s->ymax);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

template <int NB, int TAIL, int MODE>
int densef_sweep(lgr_ctx* ctx, const DensefSide& Q, const DensefSide& T, unsigned* ubits, int* cnt, int* cand, const DensefCheck& chk) {
    constexpr int BK = DenseF<NB, TAIL>::BK;
    constexpr int lds = 2 * 1024 * BK * 16;
    const int n_qb = Q.mp / DENSEF_BLK, n_tb = T.mp / DENSEF_BLK;
    const int splits = std::max(1, std::min(n_tb, cdiv(4 * ctx->n_cu, n_qb))), tps = cdiv(n_tb, splits), n_split = cdiv(n_tb, tps);
    LGR_HIP(ctx, hipFuncSetAttribute((const void*) densef_sweep_kernel<NB, TAIL, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    densef_sweep_kernel<NB, TAIL, MODE><<<dim3(n_qb, n_split), 256, lds, ctx->stream>>>(Q.ops, T.ops, Q.n2, Q.xb, T.n2, T.ymax, Q.m, T.m, n_tb, tps,
                                                                                      ubits, cnt, cand, chk);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
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
