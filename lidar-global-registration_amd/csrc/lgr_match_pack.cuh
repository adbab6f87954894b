// lgr_match_pack.cuh -- 2. MFMA operand packing (f32, f16 split, rotated f16 split), norms.
// Part of the brute-force FPFH matcher; see the header of lgr_match.hip and DESIGN.md section 3.
#pragma once
#include "lgr_match_common.cuh"

namespace {

// 2. pack.  P layout: [tile][kk][half][i] floats (tile = 32 rows): MFMA lane l of step kk reads P[(tile*KK+kk)*64 + l].
// role 0 (rows): centre = the row's own cluster (blkcl[pos / 256]), operand [-2 x', 1], nrm = |x'|^2
// role 1 (cols): blockIdx.y = cluster set p, centre c_p for every column, operand [x', |x'|^2]
// padding positions (perm < 0): rows [0.., 1] / cols [0.., +inf], nrm = +inf
__global__ void pack_kernel(const float* __restrict__ X, const int* __restrict__ perm, int n_pad, int role,
                            const float* __restrict__ cen, const int* __restrict__ blkcl,
                            float* __restrict__ P, float* __restrict__ nrm, unsigned* __restrict__ ovf) {
    int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n_pad) return;
    int set = role == 1 ? blockIdx.y : 0;
    int o = perm[pos];
    int c = role == 1 ? set : blkcl[pos / BLOCK_ROWS];
    float v[33];
    float n2 = 0.f;
    if (o >= 0) {
#pragma unroll
        for (int k = 0; k < 33; ++k) { v[k] = X[(size_t) o * 33 + k] - cen[c * 33 + k]; n2 = n2 + v[k] * v[k]; }
    } else {
#pragma unroll
        for (int k = 0; k < 33; ++k) v[k] = 0.f;
        n2 = __uint_as_float(0x7f800000u);
    }
    nrm[(size_t) set * n_pad + pos] = n2;
    if (o >= 0 && !(n2 < FLT_BIG)) *ovf = 1u;   // |x'|^2 overflows float: the filter cannot represent this row
    int tile = pos >> 5, r = pos & 31;
    float* base = P + ((size_t) set * (n_pad / TILE) + tile) * KK * 64 + r;
#pragma unroll
    for (int k = 0; k < 34; ++k) {
        float val;
        if (k < 33) val = role == 0 ? -2.0f * v[k] : v[k];
        else val = role == 0 ? 1.0f : n2;
        base[(k >> 1) * 64 + (k & 1) * 32] = val;
    }
}

// f16-split operands (OpFmt<FMT_F16 / FMT_F16R>).  Same roles / sets / nrm output as pack_kernel; P holds f16x8 fragments:
// fragment (tile, f, lane) at ((set * tiles + tile) * NF + f) * 64 + lane, lane = row | (khalf << 5).
// Plain format (NF = 7 = KS): concatenated K index c: [0,33) a1.b1, [33,66) a1.b2, [66,99) a2.b1, 99..104 norm slots, rest 0;
// a norm enters as the three-term f16 expansion of N = |x'|^2 2^2s against the constants A1..A3 on the other side
// (N = A1 B1 + A2 B2 + A3 B3 up to 2^-33 N or the f16 flush limit).
// Rotated format (NF = 4 stored fragments, KS = 6 steps: OpFmt<FMT_F16R>): stored K index c of a row / column:
// [0,30) h1, 30..31 norm slots, [32,62) h2, 62..63 norm slots; a norm is the two-term expansion N ~ c0 (n1 + n2) against
// the one constant c0 = a_norm[0] (error bound: operand_scale, "rot").
// rows: h = split(-2 x' 2^s);  cols: h = split(x' 2^s).
// Helmert coordinates of one 11-bin block: y_k = (x_0 + .. + x_{k-1} - k x_k) / sqrt(k (k + 1)), k = 1..10 (orthonormal, all
// orthogonal to (1,..,1)); *u = (x_0 + .. + x_10) / sqrt(11) is the dropped coordinate.
__device__ __forceinline__ float helmert_rs(int k) {   // 1 / sqrt(k (k + 1)), k = 1..10
    const float rs[10] = {0.70710678118654752f, 0.40824829046386302f, 0.28867513459481288f, 0.22360679774997897f, 0.18257418583505537f,
                          0.15430334996209191f, 0.13363062095621219f, 0.11785113019775793f, 0.10540925533894598f, 0.09534625892455924f};
    return rs[k - 1];
}
__device__ __forceinline__ void helmert11(const float* __restrict__ x, float* __restrict__ y, float* u) {
    float pre = x[0];
#pragma unroll
    for (int k = 1; k <= 10; ++k) {
        y[k - 1] = (pre - (float) k * x[k]) * helmert_rs(k);
        pre = pre + x[k];
    }
    *u = pre * 0.30151134457776363f;
}

// The reference packing kernel: the whole row in registers (x0, v, y and the 64 halves live at once: 113 VGPRs), IEEE divisions by the
// norm constants, both shell roots in every lane.  pack16_kernel below writes the same bits; lgr_match_options.self_check packs with both
// and compares on the device (check_pack16).  Sets [set_lo, set_hi) of role 1 (role 0: 0, 1); set `set` goes to slot set - set_lo of P / nrm / shell.
template <bool ROT>
__global__ __launch_bounds__(256) void pack16_ref_kernel(const float* __restrict__ X, const int* __restrict__ perm, int n_pad, int role,
                              const float* __restrict__ cen, const int* __restrict__ blkcl, F16Scale sc, int set_lo, int set_hi,
                              _Float16* __restrict__ P, float* __restrict__ nrm, float2* __restrict__ shell /* [sets][n_pad / 32] or nullptr */) {
    int pos = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = pos < n_pad;
    if (!in_range) pos = n_pad - 1;           // (nothing is stored for these lanes)
    // the row is read once (a 132-byte gather) and packed for every set: 16 column sets, one per centre, or the row set
    const int o = perm[pos];
    float x0[33];
#pragma unroll
    for (int k = 0; k < 33; ++k) x0[k] = o >= 0 ? X[(size_t) o * 33 + k] : 0.f;
#pragma unroll 1
    for (int set = set_lo; set < set_hi; ++set) {
    const int c = role == 1 ? set : blkcl[pos / BLOCK_ROWS];
    const size_t slot = (size_t) (set - set_lo);
    float v[33];
    float n2 = 0.f;
    if (o >= 0) {
#pragma unroll
        for (int k = 0; k < 33; ++k) { v[k] = x0[k] - cen[c * 33 + k]; n2 = n2 + v[k] * v[k]; }
    } else {
#pragma unroll
        for (int k = 0; k < 33; ++k) v[k] = 0.f;
        n2 = __uint_as_float(0x7f800000u);
    }
    if (in_range) nrm[slot * n_pad + pos] = n2;   // |x'|^2 in all 33 coordinates: the magnitude the error bounds are stated in
    if (shell) {
        // radial shell of the 32-position tile about this centre: (min, max) of |x'| over its finite rows (min rounded down, max up; an
        // empty tile: (+inf, 0)) -- the 32 rows of a tile are the 32 lanes of a half wave (shell bound, lgr_match_rerank.cuh / match_mfma)
        const bool fin = in_range && n2 < FLT_BIG;
        float mn = fin ? n2 : __uint_as_float(0x7f800000u), mx = fin ? n2 : 0.f;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) { mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o)); }
        if (in_range && (pos & 31) == 0)
            shell[slot * (n_pad / TILE) + (pos >> 5)] = make_float2(mn < FLT_BIG ? sqrtf(mn) * 0.9999998f : mn, sqrtf(mx) * 1.0000002f);
    }
    float y[30], u0, u1, u2;
    if (ROT) { helmert11(v, y, &u0); helmert11(v + 11, y + 10, &u1); helmert11(v + 22, y + 20, &u2); }
    if (!in_range) continue;
    constexpr int nd = ROT ? 30 : 33, nf = ROT ? OpFmt<FMT_F16R>::NF : OpFmt<FMT_F16>::NF;
    int tile = pos >> 5, r = pos & 31;
    // the row's K = 16 nf stored halves are assembled in registers (all indices are compile-time constants) and leave as
    // 2 nf 16-byte pieces: piece (f, khalf) of row r sits at fragment (f * 64 + khalf * 32 + r)
    _Float16 hv[nf * 16];
    auto put = [&](int cidx, _Float16 h) { hv[cidx] = h; };
    const float mul = role == 0 ? -2.0f * sc.s_mul : sc.s_mul;
    float n2m = n2;                           // the norm the MFMA chain must see: of the operand coordinates
    if (ROT && o >= 0) {
        n2m = 0.f;
#pragma unroll
        for (int k = 0; k < 30; ++k) n2m = n2m + y[k] * y[k];
    }
    // K order.  Plain format: [0,nd) a1.b1, [nd,2nd) a1.b2, [2nd,3nd) a2.b1, then the six norm slots.  Rotated format: the
    // stored fragments 0-1 (K slots 0..31) hold h1 and the leading norm term, 2-3 (K slots 32..63) h2 and the second norm
    // term; the chain pairs them as h1.h1, h1.h2, h2.h1 (OpFmt<FMT_F16R>), and its first two steps -- a1.b1 and the leading
    // norm terms -- are a coarse d2~ the kernels test before they spend the other four steps on a tile (match_mfma, "coarse rejection").
    constexpr int o12 = ROT ? 32 : nd, o21 = ROT ? 32 : 2 * nd;
#pragma unroll
    for (int k = 0; k < nd; ++k) {
        float x = (ROT ? y[k] : v[k]) * mul;  // exact (power of two)
        _Float16 h1 = (_Float16) x;           // round to nearest
        _Float16 h2 = (_Float16) (x - (float) h1);
        if (ROT) { put(k, h1); put(o12 + k, h2); }
        else if (role == 0) { put(k, h1); put(o12 + k, h1); put(o21 + k, h2); }
        else { put(k, h1); put(o12 + k, h2); put(o21 + k, h1); }
    }
    // norm slots, so that d2~ 2^2s = |b'|^2 - 2 a'.b' + |a'|^2 comes out of the MFMA chain with C = 0
    const bool rows = role == 0;
    const _Float16 c0 = (_Float16) sc.a_norm[0], c1 = (_Float16) sc.a_norm[1], c2 = (_Float16) sc.a_norm[2];
    const float N = n2m * (sc.s_mul * sc.s_mul);
    if (ROT) {
        // two terms against c0: n1 = f16(N / c0) -- the same leading term as the three-term expansion, so the coarse d2~ of a
        // row is what it was -- and n2 = f16((N - c0 n1) / c0).  Stored:
        //     rows    [0,32): h1 | c0, n1     [32,64): h2 | 0, n2
        //     columns [0,32): h1 | n1, c0     [32,64): h2 | n2, 0
        // so the row norm meets c0 in steps 0-1 (n1) and 4-5 (n2), the column norm in steps 0-1 (n1) and 2-3 (n2), and the
        // zero slots meet the other side's n1 (steps 4-5: columns' n1 x rows' 0; steps 2-3: rows' n1 x columns' 0).  A padding
        // position (or a norm the f16 terms cannot hold) therefore keeps n1 FINITE -- the largest f16, 65504 -- and puts +inf
        // into n2: 0 x inf would make the product NaN.  Its full d2~ is +inf as before; its coarse d2~ (steps 0-1) is >= 65504 c0,
        // about 2 N_max, instead of +inf -- above the thresholds of any real data, and a tile kept on it ends at +inf: it can cost
        // a tile, never change a minimum.
        _Float16 n1 = (_Float16) 65504.f, n2 = (_Float16) __uint_as_float(0x7f800000u);
        if (o >= 0 && N / sc.a_norm[0] < 65504.f) {
            n1 = (_Float16) (N / sc.a_norm[0]);
            const float r1 = __builtin_fmaf(-sc.a_norm[0], (float) n1, N);   // exact
            n2 = (_Float16) (r1 / sc.a_norm[0]);
        }
        const _Float16 z = (_Float16) 0.f;
        put(30, rows ? c0 : n1); put(31, rows ? n1 : c0);
        put(62, rows ? z : n2); put(63, rows ? n2 : z);
    } else {
        _Float16 b1, b2, b3;
        if (o >= 0) {
            b1 = (_Float16) (N / sc.a_norm[0]);
            float r1 = __builtin_fmaf(-sc.a_norm[0], (float) b1, N);
            b2 = (_Float16) (r1 / sc.a_norm[1]);
            float r2 = __builtin_fmaf(-sc.a_norm[1], (float) b2, r1);
            b3 = (_Float16) (r2 / sc.a_norm[2]);
        } else {
            b1 = (_Float16) __uint_as_float(0x7f800000u); b2 = (_Float16) 0.f; b3 = (_Float16) 0.f;   // padding: +inf
        }
        // 3 nd .. 3 nd + 2 carry |b'|^2 (expansion on the column side, constants on the row side), the next three |a'|^2 the
        // other way round: columns [expansion | constants], rows [constants | expansion]
        put(3 * nd + 0, rows ? c0 : b1); put(3 * nd + 1, rows ? c1 : b2); put(3 * nd + 2, rows ? c2 : b3);
        put(3 * nd + 3, rows ? b1 : c0); put(3 * nd + 4, rows ? b2 : c1); put(3 * nd + 5, rows ? b3 : c2);
#pragma unroll
        for (int cidx = 3 * nd + 6; cidx < nf * 16; ++cidx) put(cidx, (_Float16) 0.f);
    }
    f16x8* base = reinterpret_cast<f16x8*>(P) + (slot * (n_pad / TILE) + tile) * nf * 64;
#pragma unroll
    for (int piece = 0; piece < 2 * nf; ++piece) {
        f16x8 w;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = hv[piece * 8 + j];
        base[(piece >> 1) * 64 + ((piece & 1) << 5) + r] = w;
    }
    }   // sets
}

// An f32 product on its way to an f16 conversion, hidden from the compiler: it would otherwise fuse the two into v_fma_mixlo_f16 (x mul + 0),
// which turns a zero product into +0 whatever its sign, where the multiply and v_cvt_pk_f16_f32 keep -0 (rows: mul < 0).  Harmless to the
// matcher, but the packing kernels are compared bit for bit.
__device__ __forceinline__ float unfused(float x) { asm("" : "+v"(x)); return x; }

// The packing kernel: the bits of pack16_ref_kernel, formed so that little is live at once.  A lane still owns a row and walks the sets, but
// every 16-byte piece leaves as soon as its eight halves exist: the rotated format's coordinate k yields h1 for piece k / 8 and h2 for piece
// 4 + k / 8 straight from the running Helmert prefix, so besides the row itself (x0, 33 registers) only two pieces, the prefix and the two
// norm sums are carried.  The sums n2 (33 terms) and n2m (30) stay ONE chain each, in the reference's order; the norm terms are multiplied by
// the reciprocals of the power-of-two constants (F16Scale::inv_a_norm: the same correctly rounded quotient, subnormals included); the
// shell's roots are taken by the one lane per tile that stores them.  Precondition the reference does not have: X holds at least one row -- a
// padding position (perm < 0) loads row 0 (one 132-byte gather per padding lane, unconditional so that the loads need no branches) and
// uses none of it; match_impl returns before the packing when a side is empty, and the leaf centres always have rows.  COLS: role 1 (the 16 sets; the role is a template parameter so that the
// columns' centre address is uniform and costs no vector registers), otherwise role 0.  (Non-temporal stores of the column fragments were
// tried and bought nothing: DESIGN.md section 11.)
template <bool ROT, bool COLS>
__global__ __launch_bounds__(256, 6) void pack16_kernel(const float* __restrict__ X, const int* __restrict__ perm, int n_pad,
                              const float* __restrict__ cen, const int* __restrict__ blkcl, F16Scale sc,
                              _Float16* __restrict__ P, float* __restrict__ nrm, float2* __restrict__ shell /* [sets][n_pad / 32] or nullptr */) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n_pad) return;                 // (n_pad is a multiple of TILE: whole half waves leave, and the shell's shuffles stay inside a half wave)
    constexpr int n_sets = COLS ? KCL : 1;
    const int o = perm[pos];
    const bool valid = o >= 0;
    float x0[33];                             // (a padding position reads row 0, see above: its coordinates are never used)
#pragma unroll
    for (int k = 0; k < 33; ++k) x0[k] = X[(size_t) (valid ? o : 0) * 33 + k];
    constexpr int nd = ROT ? 30 : 33, nf = ROT ? OpFmt<FMT_F16R>::NF : OpFmt<FMT_F16>::NF;
    const int tile = pos >> 5, r = pos & 31;
    constexpr bool rows = !COLS;
    const float mul = rows ? -2.0f * sc.s_mul : sc.s_mul;
    const float s2 = sc.s_mul * sc.s_mul;
    const float inf = __uint_as_float(0x7f800000u);
    const _Float16 c0 = (_Float16) sc.a_norm[0], c1 = (_Float16) sc.a_norm[1], c2 = (_Float16) sc.a_norm[2], z = (_Float16) 0.f;
#pragma unroll 1
    for (int set = 0; set < n_sets; ++set) {
        // the centre is uniform -- the set's, or that of the 256-row block this workgroup is -- and comes through the scalar cache
        static_assert(BLOCK_ROWS == 256, "a workgroup packs one row block");
        const float* __restrict__ cc = cen + (COLS ? set : __builtin_amdgcn_readfirstlane(blkcl[pos / BLOCK_ROWS])) * 33;
        f16x8* base = reinterpret_cast<f16x8*>(P) + ((size_t) set * (n_pad / TILE) + tile) * nf * 64 + r;
        // piece (f, khalf) of row r sits at fragment (f * 64 + khalf * 32 + r)
        auto store = [&](int piece, const f16x8& w) {
            f16x8* q = base + (piece >> 1) * 64 + ((piece & 1) << 5);
            *q = w;
        };
        float n2 = 0.f;
        if constexpr (ROT) {
            // stored K index: [0,30) h1, 30..31 norm slots, [32,62) h2, 62..63 norm slots (the layout comment above pack16_ref_kernel)
            float n2m = 0.f;
            f16x8 w1, w2;
            if (valid) {
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    float pre = 0.f;
#pragma unroll
                    for (int kk = 0; kk < 11; ++kk) {
                        const float vk = x0[11 * b + kk] - cc[11 * b + kk];
                        n2 = n2 + vk * vk;
                        if (kk == 0) pre = vk;
                        else {
                            const int k = 10 * b + kk - 1;
                            const float yk = (pre - (float) kk * vk) * helmert_rs(kk);
                            pre = pre + vk;
                            n2m = n2m + yk * yk;
                            const float x = unfused(yk * mul);  // exact (power of two)
                            const _Float16 h1 = (_Float16) x;
                            w1[k & 7] = h1; w2[k & 7] = (_Float16) (x - (float) h1);
                            if ((k & 7) == 7) {
                                store(k >> 3, w1); store(4 + (k >> 3), w2);
                                // keep the instruction scheduler from moving the two sum chains behind the pieces: it would then hold every
                                // v and y of the row until the end of the set, which is what this order is there to avoid
                                asm volatile("" : "+v"(n2), "+v"(n2m));
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        }
                    }
                }
            } else {
                // padding: x' = 0 (h1 = f16(0 * mul): -0 for rows), |x'|^2 = +inf
                const _Float16 h0 = (_Float16) unfused(0.f * mul);
#pragma unroll
                for (int j = 0; j < 8; ++j) { w1[j] = h0; w2[j] = z; }
#pragma unroll
                for (int p3 = 0; p3 < 3; ++p3) { store(p3, w1); store(4 + p3, w2); }
                n2 = inf; n2m = inf;
            }
            // two norm terms against c0; a padding position keeps n1 finite and puts +inf into n2 (pack16_ref_kernel)
            const float N = n2m * s2, q1 = N * sc.inv_a_norm[0];
            _Float16 n1 = (_Float16) 65504.f, nn2 = (_Float16) inf;
            if (valid && q1 < 65504.f) {
                n1 = (_Float16) q1;
                const float r1 = __builtin_fmaf(-sc.a_norm[0], (float) n1, N);   // exact
                nn2 = (_Float16) (r1 * sc.inv_a_norm[0]);
            }
            w1[6] = rows ? c0 : n1; w1[7] = rows ? n1 : c0;
            w2[6] = rows ? z : nn2; w2[7] = rows ? nn2 : z;
            store(3, w1); store(7, w2);
        } else {
            // concatenated K index: [0,nd) a1.b1, [nd,2nd) a1.b2, [2nd,3nd) a2.b1, six norm slots, zeros
#pragma unroll
            for (int k = 0; k < 33; ++k) { const float vk = x0[k] - cc[k]; n2 = n2 + vk * vk; }
            if (!valid) n2 = inf;
            const float N = n2 * s2;
            _Float16 b1 = (_Float16) inf, b2 = z, b3 = z;   // padding: +inf
            if (valid) {
                b1 = (_Float16) (N * sc.inv_a_norm[0]);
                const float r1 = __builtin_fmaf(-sc.a_norm[0], (float) b1, N);
                b2 = (_Float16) (r1 * sc.inv_a_norm[1]);
                const float r2 = __builtin_fmaf(-sc.a_norm[1], (float) b2, r1);
                b3 = (_Float16) (r2 * sc.inv_a_norm[2]);
            }
#pragma unroll
            for (int piece = 0; piece < 2 * nf; ++piece) {
                f16x8 w;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int cidx = piece * 8 + j;
                    _Float16 h = z;
                    if (cidx < 3 * nd) {
                        const int part = cidx / nd, k = cidx % nd;
                        const float d = x0[k] - cc[k];
                        const float dv = valid ? d : 0.f, x = unfused(dv * mul);
                        // (the reference kernel converts its coordinates in pairs and the odd 33rd one through v_fma_mixlo_f16: its h1 is +0
                        //  where the product is -0 -- a padding row, a row at its centre -- and is formed the same way here)
                        const _Float16 h1 = k == 32 ? (_Float16) __builtin_fmaf(dv, mul, 0.f) : (_Float16) x;
                        const bool second = rows ? part == 2 : part == 1;   // rows: h1 h1 h2, columns: h1 h2 h1
                        h = second ? (_Float16) (x - (float) h1) : h1;
                    } else if (cidx < 3 * nd + 3) {
                        const int t = cidx - 3 * nd;
                        h = rows ? (t == 0 ? c0 : t == 1 ? c1 : c2) : (t == 0 ? b1 : t == 1 ? b2 : b3);
                    } else if (cidx < 3 * nd + 6) {
                        const int t = cidx - 3 * nd - 3;
                        h = rows ? (t == 0 ? b1 : t == 1 ? b2 : b3) : (t == 0 ? c0 : t == 1 ? c1 : c2);
                    }
                    w[j] = h;
                }
                store(piece, w);
            }
        }
        nrm[(size_t) set * n_pad + pos] = n2;   // |x'|^2 in all 33 coordinates: the magnitude the error bounds are stated in
        if (shell) {
            // radial shell of the tile about this centre, as in pack16_ref_kernel; the roots only where they are stored
            const bool fin = n2 < FLT_BIG;
            float mn = fin ? n2 : inf, mx = fin ? n2 : 0.f;
#pragma unroll
            for (int d = 16; d > 0; d >>= 1) { mn = fminf(mn, __shfl_xor(mn, d)); mx = fmaxf(mx, __shfl_xor(mx, d)); }
            if (r == 0)
                shell[(size_t) set * (n_pad / TILE) + tile] = make_float2(mn < FLT_BIG ? sqrtf(mn) * 0.9999998f : mn, sqrtf(mx) * 1.0000002f);
        }
    }   // sets
}

// lgr_match_options.self_check: pieces (T = uint4: 16 bytes; uint2: a tile's shell) of two packings, bit for bit; counts[0] += pieces
// compared, counts[1] += pieces differing
__device__ __forceinline__ bool same_bits(const uint4& u, const uint4& v) { return u.x == v.x && u.y == v.y && u.z == v.z && u.w == v.w; }
__device__ __forceinline__ bool same_bits(const uint2& u, const uint2& v) { return u.x == v.x && u.y == v.y; }
template <class T>
__global__ void pack_compare_kernel(const T* __restrict__ a, const T* __restrict__ b, size_t n, unsigned long long* __restrict__ counts) {
    unsigned diff = 0u, seen = 0u;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t) gridDim.x * blockDim.x) {
        ++seen;
        diff += same_bits(a[i], b[i]) ? 0u : 1u;
    }
    for (int d = 32; d > 0; d >>= 1) { diff += __shfl_xor(diff, d); seen += __shfl_xor(seen, d); }
    if ((threadIdx.x & 63) == 0) {
        if (seen) atomicAdd(&counts[0], (unsigned long long) seen);
        if (diff) atomicAdd(&counts[1], (unsigned long long) diff);
    }
}

// original rows in padded (cluster-sorted) order, contiguous, for the exact rerank (padding rows are never read)
__global__ void gather_rows_kernel(const float* __restrict__ X, const int* __restrict__ perm, int n_pad, float* __restrict__ out) {
    size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) n_pad * 33) return;
    int pos = (int) (e / 33), k = (int) (e % 33);
    int o = perm[pos];
    out[e] = o >= 0 ? X[(size_t) o * 33 + k] : 0.f;
}

// per-group maxima of sqrt(norm) (finite entries only): out[set][g]; groups are [starts[g], starts[g+1]) or, with
// starts == nullptr, fixed windows of `group` positions
__global__ void group_max_kernel(const float* __restrict__ nrm, int n_pad, int group, const int* __restrict__ starts, float* __restrict__ out) {
    int g = blockIdx.x, set = blockIdx.y, n_groups = gridDim.x;
    float m = 0.f;
    int p0 = starts ? starts[g] : g * group, p1 = starts ? starts[g + 1] : min(n_pad, (g + 1) * group);
    for (int pos = p0 + threadIdx.x; pos < p1; pos += blockDim.x) {
        float v = nrm[(size_t) set * n_pad + pos];
        if (v < FLT_BIG) m = fmaxf(m, v);
    }
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    __shared__ float sh[4];
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int) (blockDim.x >> 6); ++w) m = fmaxf(m, sh[w]);
        out[(size_t) set * n_groups + g] = sqrtf(m) * 1.0000002f;   // rounded up
    }
}


// shells of windows of `group` consecutive tiles from the tiles' shells (pack16_kernel): out[set][g] = (min of the minima, max of the maxima);
// out_max (optional) = the maxima alone (the stage maxima of the coarse thresholds)
__global__ void shell_reduce_kernel(const float2* __restrict__ tile_shell, int n_sets, int n_tiles, int group, float2* __restrict__ out, float* __restrict__ out_max) {
    const int n_groups = (n_tiles + group - 1) / group;
    const long long id = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long long) n_sets * n_groups) return;
    const int set = (int) (id / n_groups), g = (int) (id % n_groups);
    float mn = __uint_as_float(0x7f800000u), mx = 0.f;
    for (int t = g * group; t < min(n_tiles, (g + 1) * group); ++t) {
        const float2 v = tile_shell[(size_t) set * n_tiles + t];
        mn = fminf(mn, v.x); mx = fmaxf(mx, v.y);
    }
    out[id] = make_float2(mn, mx);
    if (out_max) out_max[id] = mx;
}

}  // namespace
