// lgr_ransac_count.cuh -- the packing of the correspondences (pack_kernel) and phase 1 of a round, the O(H x C) verification: count_item
// (one wave = 64 hypotheses over a chunk of correspondences, fused evaluation with an exact re-test inside the decision band, inlier bit
// masks), count_chunk and the device-sized work list of count_list_kernel.
// Part of lgr_ransac.hip's one translation unit; see its header for the schedule and DESIGN.md section 5.
#pragma once
#include "lgr_ransac_common.cuh"

namespace {

// ---------------------------------------------------------------------------------------------------- packing
// pack[i] = {sx, sy, sz, thr | tx, ty, tz, bins}; sstar[i] = smallest float s with sqrt_rn(s) >= thr, so that the
// inlier test `sqrtf(s) < thr` (src/metric.cpp:141-144) is exactly `s < sstar` without a square root per pair.
__device__ __forceinline__ float next_up(float x) { return __uint_as_float(__float_as_uint(x) + 1u); }
__device__ __forceinline__ float next_down(float x) { return __uint_as_float(__float_as_uint(x) - 1u); }

__global__ void pack_kernel(const float* __restrict__ src, const float* __restrict__ tgt, const lgr_corr* __restrict__ corr, int c,
                            const unsigned* __restrict__ bbk /* lgr_bbox_launch's keys: [6..8] the reference's min, [9..11] its max of the source cloud */,
                            float4* __restrict__ P0, float4* __restrict__ P1, float* __restrict__ sstar,
                            float* __restrict__ PP, unsigned* __restrict__ pstats, int cpad) {
    // (bbk == nullptr: the caller does not use the uniformity bins -- unit box)
    const float mnx = bbk ? lgr_bbox_key_inv(bbk[6]) : 0.f, mny = bbk ? lgr_bbox_key_inv(bbk[7]) : 0.f, mnz = bbk ? lgr_bbox_key_inv(bbk[8]) : 0.f;
    const float mxx = bbk ? lgr_bbox_key_inv(bbk[9]) : 1.f, mxy = bbk ? lgr_bbox_key_inv(bbk[10]) : 1.f, mxz = bbk ? lgr_bbox_key_inv(bbk[11]) : 1.f;
    unsigned m0 = 0u, m1 = 0u, m2 = 0u;   // this lane's contribution to pstats (padding lanes: the neutral 0)
  for (int base = blockIdx.x * blockDim.x; base < cpad; base += gridDim.x * blockDim.x) {   // (a few hundred workgroups: their statistics meet in 3 atomics each)
    const int i = base + threadIdx.x;
    if (i >= c) {
        if (PP && i < cpad) {
            float* r = PP + (size_t) (i >> 1) * CP_FLOATS + (i & 1);
#pragma unroll
            for (int f = 0; f < 8; ++f) r[2 * f] = 0.f;   // s* = 0: d2 < 0 never holds
        }
    } else {
    lgr_corr cr = corr[i];
    P3 s = ldp(src, cr.index_query), t = ldp(tgt, cr.index_match);
    float thr = cr.threshold;
    // bins of calculateCorrespondenceUniformity (src/analysis.cpp:108-112); NaN/negative pinned to 0 like the oracle
    float f0 = floorf((s.x - mnx) / (mxx - mnx) * 100), f1 = floorf((s.y - mny) / (mxy - mny) * 100), f2 = floorf((s.z - mnz) / (mxz - mnz) * 100);
    f0 = (99.f < f0) ? 99.f : f0; f1 = (99.f < f1) ? 99.f : f1; f2 = (99.f < f2) ? 99.f : f2;   // std::min(f, 99.f)
    int b0 = (f0 >= 0.f) ? (int) f0 : 0, b1 = (f1 >= 0.f) ? (int) f1 : 0, b2 = (f2 >= 0.f) ? (int) f2 : 0;
    P0[i] = make_float4(s.x, s.y, s.z, thr);
    P1[i] = make_float4(t.x, t.y, t.z, __int_as_float(b0 | (b1 << 8) | (b2 << 16)));
    float ss;
    if (!(thr > 0.f)) ss = 0.f;                           // nothing is < thr (NaN thr: nothing either)
    else if (!(thr < 3.4028234663852886e38f)) ss = thr;   // inf: every finite s qualifies, s < inf
    else {
        float g = thr * thr;
        if (!(g < 3.4028234663852886e38f)) g = 3.4028234663852886e38f;
        if (g < 1.17549435e-38f) g = 1.17549435e-38f;
        // walk to the boundary: smallest g with sqrt(g) >= thr
        for (int it = 0; it < 8 && __builtin_sqrtf(g) >= thr && g > 0.f; ++it) g = next_down(g);
        for (int it = 0; it < 16 && __builtin_sqrtf(g) < thr; ++it) g = next_up(g);
        ss = g;
    }
    sstar[i] = ss;
    if (PP) {
        float* r = PP + (size_t) (i >> 1) * CP_FLOATS + (i & 1);
        r[0] = s.x; r[2] = s.y; r[4] = s.z; r[6] = t.x; r[8] = t.y; r[10] = t.z; r[12] = ss;
        // slope of the decision band of count_item's fused evaluation: 28 sqrt(s*), rounded up (inf for an infinite threshold)
        r[14] = (ss < 3.4028234663852886e38f) ? next_up(28.f * __builtin_sqrtf(ss)) * 1.000001f : __uint_as_float(0x7f800000u);
        const float sm = fmaxf(fmaxf(fabsf(s.x), fabsf(s.y)), fabsf(s.z)), qm = fmaxf(fmaxf(fabsf(t.x), fabsf(t.y)), fabsf(t.z));
        // NaN coordinates: the integer max of the bit pattern keeps them (a NaN pattern is above every finite one) -> the band becomes NaN
        // -> every chunk takes the exact path
        m0 = max(m0, __float_as_uint(sm)); m1 = max(m1, __float_as_uint(qm)); m2 = max(m2, (ss < 3.4028234663852886e38f) ? __float_as_uint(ss) : 0u);
    }
    }
  }
    // one atomic per wave and statistic (as one per thread: 3 x 282 k updates of the same three words on the bench pair -- even one per wave of a
    // thread-per-correspondence grid was 13 k same-address atomics, most of the kernel's 0.16 ms); every lane of the wave is here
    if (PP) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m0 = max(m0, (unsigned) __shfl_xor((int) m0, o)); m1 = max(m1, (unsigned) __shfl_xor((int) m1, o)); m2 = max(m2, (unsigned) __shfl_xor((int) m2, o));
        }
        if ((threadIdx.x & 63) == 0) {
            if (m0) atomicMax(&pstats[0], m0);
            if (m1) atomicMax(&pstats[1], m1);
            if (m2) atomicMax(&pstats[2], m2);
        }
    }
}

// ---------------------------------------------------------------------------------------------------- phase 1
// lane = hypothesis (T in registers), loop over a chunk of correspondences broadcast from LDS.
// counts[h] = {inliers (4-norm rule, src/metric.cpp:141), support (3-norm rule, src/metric.cpp:111)}
constexpr int CB = 64;        // hypotheses per workgroup (one wave)
constexpr int CCH = 2048;     // correspondences per workgroup (fewer when there are few hypotheses: count_chunk)
// The O(H x C) verification.  Round 3: per (hypothesis, correspondence) pair the reference's expressions (LGR_APPLY, the Eigen
// 4-vector and 3-vector norms: ~25 unfused multiply / add instructions per pair) are evaluated only where they can decide something.
// A FUSED evaluation -- e_k = fma(c_k0, x, fma(c_k1, y, fma(c_k2, z, c_k3 - q_k))), d2~ = fma(e_z, e_z, fma(e_y, e_y, e_x e_x)): 15 packed
// instructions per two correspondences -- differs from both reference values by at most
//     err(x) = 7u x + 3.5 eta sqrt(x) + 3 eta^2,   eta = 12u (max_k sum_j |c_kj| * max|s| + max_k |c_k3| + max|q|),  u = 2^-24
// (4 roundings per component in either order, 3 in either sum of squares), so the sign of d2~ - s* IS the
// reference's decision whenever |d2~ - s*| > 8 err(s*) + 16 eta^2.  Per correspondence the kernel keeps the sign bit (one v_alignbit);
// a pair of correspondences for which ANY lane of the wave comes within that band (hypotheses that survive the prerejection are good
// enough that ~1e-3 of the pairs do: ~10 % of the iterations) is re-evaluated on the spot with the reference's own expressions, for
// the inlier (4-norm) and the support (3-norm) rule.  The correspondences are wave-uniform: they arrive through scalar loads
// (s_load_dwordx16 per pair record), not through LDS.
// Inlier bit masks, hypothesis-major (round 5): row h = the mask of survivor h, mask_pitch(c) words -- a whole number of 128-correspondence groups,
// the unit count_item stores (one 16-byte store per lane and group).  The metric phase reads a candidate's row front to back; with the rows
// word-major ([word][hypothesis], coalesced stores) every word of a candidate was a cache line of its own: 14.9 GB of fetches per 1M cluster-filter
// alignment, 80 % of metric_kernel's wave cycles parked.
__host__ __device__ inline size_t mask_pitch(int c) { return (size_t) ((c + 127) >> 7) * 4; }
__device__ __forceinline__ void count_item(const int bx /* block of CB hypotheses */, const int by /* chunk of cch correspondences */,
                                           const float* Ts, const int* list, int nh,
                                           const CPair* __restrict__ PP, const unsigned* __restrict__ pstats, int c, int2* counts,
                                           unsigned* maskT /* [nh][mask_pitch(c)] inlier bits, or nullptr */, int cch, const int lane) {
    const int h = bx * CB + lane;
    const bool act = h < nh;
    float T[16];
    {
        const float4* tp = reinterpret_cast<const float4*>(Ts + (size_t) (act ? list[h] : 0) * 16);
        float4 a = tp[0], b = tp[1], cc = tp[2], d = tp[3];
        T[0] = a.x; T[1] = a.y; T[2] = a.z; T[3] = a.w; T[4] = b.x; T[5] = b.y; T[6] = b.z; T[7] = b.w;
        T[8] = cc.x; T[9] = cc.y; T[10] = cc.z; T[11] = cc.w; T[12] = d.x; T[13] = d.y; T[14] = d.z; T[15] = d.w;
    }
    // decision band of this hypothesis (see above); anything non-finite -> kh = +inf: every pair is evaluated with the reference's expressions
    const float smax = __uint_as_float(pstats[0]), qmax = __uint_as_float(pstats[1]), ssmax = __uint_as_float(pstats[2]);
    const float rowl1 = fmaxf(fmaxf(fabsf(T[0]) + fabsf(T[4]) + fabsf(T[8]), fabsf(T[1]) + fabsf(T[5]) + fabsf(T[9])), fabsf(T[2]) + fabsf(T[6]) + fabsf(T[10]));
    const float Ah = rowl1 * smax + fmaxf(fmaxf(fabsf(T[12]), fabsf(T[13])), fabsf(T[14])) + qmax;
    float eta = 7.152557373046875e-7f * Ah;                                  // 12 u
    float kh = (3.814697265625e-6f * ssmax + 56.f * eta * eta) * 1.0001f;    // 64 u s*max + 56 eta^2 >= 56 u s* + 40 eta^2
    if (!(kh < 3.4028234663852886e38f) || !(eta < 3.4028234663852886e38f)) { kh = __uint_as_float(0x7f800000u); eta = 0.f; }
    const float neg_eta = -eta;
    int ninl = 0, nsup = 0;
    uint4 wq = make_uint4(0u, 0u, 0u, 0u);   // the 128-correspondence group being assembled
    const int c0 = by * cch, c1 = min(c, c0 + cch);
    for (int base = c0; base < c1; base += 64) {
        const CPair* __restrict__ pp = PP + (base >> 1);   // wave-uniform: scalar loads
        unsigned w[2], sd[2] = {0u, 0u};                   // inlier bits; support bits that differ from them (borderline pairs only)
        CPair nxt = pp[0], nxt2 = pp[1];                   // two pair records are in flight while the current one is evaluated
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            unsigned bits = 0u;
#pragma unroll 4
            for (int jj = 0; jj < 16; ++jj) {
                const CPair p = nxt;
                nxt = nxt2;
                nxt2 = pp[min(half * 16 + jj + 2, 31)];
                v2f_c ex = T[12] - p.qx, ey = T[13] - p.qy, ez = T[14] - p.qz;
                ex = __builtin_elementwise_fma(v2f_c{T[8], T[8]}, p.sz, ex); ey = __builtin_elementwise_fma(v2f_c{T[9], T[9]}, p.sz, ey); ez = __builtin_elementwise_fma(v2f_c{T[10], T[10]}, p.sz, ez);
                ex = __builtin_elementwise_fma(v2f_c{T[4], T[4]}, p.sy, ex); ey = __builtin_elementwise_fma(v2f_c{T[5], T[5]}, p.sy, ey); ez = __builtin_elementwise_fma(v2f_c{T[6], T[6]}, p.sy, ez);
                ex = __builtin_elementwise_fma(v2f_c{T[0], T[0]}, p.sx, ex); ey = __builtin_elementwise_fma(v2f_c{T[1], T[1]}, p.sx, ey); ez = __builtin_elementwise_fma(v2f_c{T[2], T[2]}, p.sx, ez);
                v2f_c d2 = ex * ex;
                d2 = __builtin_elementwise_fma(ey, ey, d2);
                d2 = __builtin_elementwise_fma(ez, ez, d2);
                const v2f_c u = d2 - p.ss;
                // sign bit of u = "d2~ < s*" (u = -0 cannot occur: x - x is +0); correspondence 2 jj (+1) ends up at bit 31 - 2 jj (- 1)
                bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(u.x), 31);
                bits = __builtin_amdgcn_alignbit(bits, __float_as_uint(u.y), 31);
                const float t0 = __builtin_fmaf(neg_eta, p.rs.x, fabsf(u.x)), t1 = __builtin_fmaf(neg_eta, p.rs.y, fabsf(u.y));
                if (__any(!(t0 > kh) || !(t1 > kh))) {   // wave-uniform; NaN -> taken
                    const v2f_c ox = ((T[0] * p.sx + T[4] * p.sy) + T[8] * p.sz) + T[12];     // LGR_APPLY, elementwise
                    const v2f_c oy = ((T[1] * p.sx + T[5] * p.sy) + T[9] * p.sz) + T[13];
                    const v2f_c oz = ((T[2] * p.sx + T[6] * p.sy) + T[10] * p.sz) + T[14];
                    const v2f_c dx = ox - p.qx, dy = oy - p.qy, dz = oz - p.qz;
                    const v2f_c xx = dx * dx, yy = dy * dy, zz = dz * dz;
                    const v2f_c d4 = (xx + zz) + (yy + 0.f);   // Eigen 4-vector squaredNorm reduction
                    const v2f_c d3 = (xx + yy) + zz;           // 3-vector block norm
                    const unsigned in0 = d4.x < p.ss.x ? 1u : 0u, in1 = d4.y < p.ss.y ? 1u : 0u;
                    const unsigned s0 = d3.x < p.ss.x ? 1u : 0u, s1 = d3.y < p.ss.y ? 1u : 0u;
                    bits = (bits & ~3u) | (in0 << 1) | in1;
                    sd[half] |= ((in0 ^ s0) | ((in1 ^ s1) << 1)) << (2 * jj);
                }
            }
            w[half] = __builtin_bitreverse32(bits);
        }
        ninl += __popc(w[0]) + __popc(w[1]);
        nsup += __popc(w[0] ^ sd[0]) + __popc(w[1] ^ sd[1]);
        // inlier bits of this hypothesis for the correspondences [base, base + 64): word-major, so the lanes (consecutive
        // hypotheses) store consecutive words; phase 2 walks the set bits instead of testing every correspondence again
        // (chunks are whole groups: cch is a multiple of 128; the last group of the table may end behind c: its padding pairs are never inliers)
        if (maskT) {
            if (((base - c0) & 64) == 0) { wq.x = w[0]; wq.y = w[1]; wq.z = 0u; wq.w = 0u; }
            else { wq.z = w[0]; wq.w = w[1]; }
            if (act && ((((base - c0) & 64) != 0) || base + 64 >= c1))
                *reinterpret_cast<uint4*>(maskT + (size_t) h * mask_pitch(c) + ((size_t) ((base & ~127) >> 5))) = wq;
        }
    }
    if (act) { atomicAdd(&counts[h].x, ninl); atomicAdd(&counts[h].y, nsup); }
}
// correspondences per work item: shorter chunks when there are few hypotheses (the first round, the lr filter), so that the launch still
// has a few thousand waves
__host__ __device__ inline int count_chunk(int nh, int c) {
    const long long hb = (nh + CB - 1) / CB;
    return (hb * ((c + CCH - 1) / CCH) >= 4096) ? CCH : ((hb * ((c + 511) / 512) >= 4096) ? 512 : 128);
}
// the work list's size is known to the device only (device-driven schedule, lgr_ransac_dev): nh = *nh_dev hypotheses, a fixed
// grid of single-wave workgroups strides over the (hypothesis block, chunk) items, hypothesis blocks fastest (neighbouring workgroups
// read the same correspondences)
__global__ __launch_bounds__(CB) void count_list_kernel(const float* __restrict__ Ts, const int* __restrict__ list, const int* __restrict__ nh_dev,
                                                         const CPair* __restrict__ PP, const unsigned* __restrict__ pstats, int c, int2* __restrict__ counts,
                                                         unsigned* __restrict__ maskT, int mask_cap /* hypotheses maskT has room for */) {
    const int nh = *nh_dev;
    if (nh <= 0) return;
    const int hb_n = (nh + CB - 1) / CB, cch = count_chunk(nh, c);
    const long long items = (long long) hb_n * ((c + cch - 1) / cch);
    unsigned* const mt = nh <= mask_cap ? maskT : nullptr;
    for (long long it = blockIdx.x; it < items; it += gridDim.x)
        count_item((int) (it % hb_n), (int) (it / hb_n), Ts, list, nh, PP, pstats, c, counts, mt, cch, threadIdx.x);
}

}  // namespace
