// lgr_match_densef.cuh -- what the two MFMA filters of the long rows, SHOT352 <22, 0> and RoPS135 <8, 7>, share: the one-match filter
// (lgr_match_dense_mfma.cuh, in lgr_match_dense.hip) and the k-nearest filter (lgr_match_knn_dense_mfma.cuh, in lgr_match_knn.hip).
// The f16-split operand format with its centre and scale, the canonical distance of two rows, the norm bounds, the LDS-staged sweep
// whose epilogue is the filter, the fallback list and the packing of a side.  The format, the chain t1.q1 + t1.q2 + t2.q1 and the bound
// E(i, tile) are described at the top of lgr_match_dense_mfma.cuh and proven in DESIGN.md section 4; both users rely on exactly them.
#pragma once

namespace {

typedef _Float16 densef_f16x8 __attribute__((ext_vector_type(8)));
typedef float densef_f32x16 __attribute__((ext_vector_type(16)));

constexpr int DENSEF_CAP = 64;                  // candidates per query row
constexpr int DENSEF_IRR_CAP = 1024;            // irregular train rows offered to every query
constexpr int DENSEF_GROUPS = LGR_RANDOMNESS_MAX;   // group values a lane keeps per query in the k-nearest sweep A
static_assert(DENSEF_GROUPS % 4 == 0, "the lists are written as float4");
constexpr int DENSEF_BLK = 128;                 // rows of a workgroup's block on either side: 4 tiles of 32, 2 x 2 tiles per wave
constexpr int DENSEF_CS_BLOCKS = 64, DENSEF_CS_ROWS = 256;   // the centre's sample: at most 16 384 rows at a fixed stride
constexpr float DENSEF_X_MAX = 32768.f;         // largest |X| element of a regular row: h1 holds it with room to 65504
constexpr float DENSEF_EPS_LIN = 2.5e-3f;       // >= 2.002 x 2^-14 x sqrt(352) = 2.293e-3: f16 terms below 2^-14, should the MFMA flush them
constexpr float DENSEF_EPS_ABS = 1e-5f;         // >= 2 x 2^-28 x 352 = 2.7e-6, and f32 underflow of a square at s <= 40

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

// The sweep: an LDS-staged GEMM tile whose epilogue is the filter.  MODE 0: sweep A of the one-match filter (ubits), 1: sweep B (cnt / cand),
// 2: the self-check of the bound, 3: sweep A of the k-nearest filter (glist: per (split, train wave, half) and query the DENSEF_GROUPS
// smallest group values, a group being the 16 train rows a lane owns of one tile).  Block = 4 waves = 128 queries x a stream of 128-row train blocks; wave (wq, wt) owns query tiles 2 wq, 2 wq + 1 and train tiles
// 2 wt, 2 wt + 1 of the block: four accumulator tiles.  The query is the MFMA column: a lane owns one query and 16 train rows of a tile.
// K goes through LDS in stages of BK chunks, both sides, double-buffered through registers: the pieces of stage n + 1 are loaded before the
// chains of stage n and stored behind them, one barrier per stage.  The operands are stored in the instruction's lane order, so a stage is a
// straight copy and every fragment read is one lane-linear 16-byte LDS read (conflict-free); per chunk a wave issues 8 reads for 12 MFMAs.
template <int NB, int TAIL, int MODE>
__global__ __launch_bounds__(256) void densef_sweep_kernel(const densef_f16x8* __restrict__ op_q, const densef_f16x8* __restrict__ op_t,
                                                          const float* __restrict__ n2_q, const float* __restrict__ xb_q, const float* __restrict__ n2_t,
                                                          const float* __restrict__ ymax, int mq, int mt, int n_tb, int tb_per_split,
                                                          unsigned* __restrict__ ubits, int* __restrict__ cnt, int* __restrict__ cand, DensefCheck chk,
                                                          float* __restrict__ glist) {
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
    float gl[2][DENSEF_GROUPS];   // MODE 3: ascending, +inf-padded; static indices only
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int p = 0; p < DENSEF_GROUPS; ++p) gl[a][p] = __uint_as_float(0x7f800000u);

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
                    } else if (MODE == 3) {
                        float v = F[0];
#pragma unroll
                        for (int i = 1; i < 16; ++i) v = fminf(v, F[i]);
                        v = fmaxf(v + E, 0.f);   // the group value: some row of the group has d2 2^2s <= v (an irregular or padded row has F = +inf)
#pragma unroll
                        for (int p = 0; p < DENSEF_GROUPS; ++p) { const float lo = fminf(gl[a][p], v); v = fmaxf(gl[a][p], v); gl[a][p] = lo; }
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
    if (MODE == 3) {
        const size_t mqp = (size_t) gridDim.x * DENSEF_BLK;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float4* out = reinterpret_cast<float4*>(glist + ((((size_t) blockIdx.y * 2 + wt) * 2 + half) * mqp + q[a]) * DENSEF_GROUPS);
#pragma unroll
            for (int p = 0; p < DENSEF_GROUPS / 4; ++p) out[p] = make_float4(gl[a][4 * p], gl[a][4 * p + 1], gl[a][4 * p + 2], gl[a][4 * p + 3]);
        }
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

__global__ void densef_gather_rows_kernel(const float* __restrict__ rows, const int* __restrict__ list, int n, int len, float* __restrict__ out) {
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) n * len) return;
    out[e] = rows[(size_t) list[e / len] * len + e % len];
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

// the runs of train blocks a query block's sweep is split into: splits x query blocks <= 4 x CUs + query blocks
inline int densef_splits(lgr_ctx* ctx, const DensefSide& Q, const DensefSide& T, int* tb_per_split) {
    const int n_qb = Q.mp / DENSEF_BLK, n_tb = T.mp / DENSEF_BLK;
    const int splits = std::max(1, std::min(n_tb, cdiv(4 * ctx->n_cu, n_qb)));
    *tb_per_split = cdiv(n_tb, splits);
    return cdiv(n_tb, *tb_per_split);
}

template <int NB, int TAIL, int MODE>
int densef_sweep(lgr_ctx* ctx, const DensefSide& Q, const DensefSide& T, unsigned* ubits, int* cnt, int* cand, const DensefCheck& chk, float* glist = nullptr) {
    constexpr int BK = DenseF<NB, TAIL>::BK;
    constexpr int lds = 2 * 1024 * BK * 16;
    const int n_qb = Q.mp / DENSEF_BLK, n_tb = T.mp / DENSEF_BLK;
    int tps;
    const int n_split = densef_splits(ctx, Q, T, &tps);
    LGR_HIP(ctx, hipFuncSetAttribute((const void*) densef_sweep_kernel<NB, TAIL, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    densef_sweep_kernel<NB, TAIL, MODE><<<dim3(n_qb, n_split), 256, lds, ctx->stream>>>(Q.ops, T.ops, Q.n2, Q.xb, T.n2, T.ymax, Q.m, T.m, n_tb, tps,
                                                                                      ubits, cnt, cand, chk, glist);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}


}  // namespace
