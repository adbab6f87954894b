// lgr_ransac_metric.cuh -- phase 2 of a round, the metric of a hypothesis in the reference's summation order (inlier_hist_kernel,
// metric_body, metric_kernel), the sequential refit over the inliers (refit_kernel) and the small kernels around them: the ordered
// compaction of the inlier pairs, the plane pairs' packing, the range check of the correspondences.
// Part of lgr_ransac.hip's one translation unit; see its header for the schedule and DESIGN.md section 5.
#pragma once
#include "lgr_ransac_common.cuh"

namespace {

// ---------------------------------------------------------------------------------------------------- phase 2
// one workgroup per hypothesis with >= MIN_NR_INLIERS inliers: metric in the reference's exact summation order.
//   uniformity      : 3 x 100 x 100 int histogram of inlier source points (order-free), then
//                     entropy_k = -(sum_b p log p) in bin order, /log(1e4), cbrt of the product (src/analysis.cpp:114-129)
//   correspondences : score = sequential float sum over inliers in correspondence order (src/metric.cpp:55-81), /C
// mask (optional) receives the inlier flags; rmse_out (optional) the rmse of src/metric.cpp:147-155.
constexpr int MB = 1024;
#ifndef LGR_METRIC_GATHERS
#define LGR_METRIC_GATHERS 4   // (4 / 8 / 16 measured equal: the gathers are not what a candidate waits for)
#endif
__device__ __forceinline__ int block_excl_scan_1024(int v, int* scan /* [MB] */, int tid, int* total) {
    // wave-level inclusive scan by shuffles, then a scan over the 16 wave totals
    int lane = tid & 63, w = tid >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { int y = __shfl_up(x, o); if (lane >= o) x += y; }
    if (lane == 63) scan[w] = x;
    __syncthreads();
    if (tid == 0) { int acc = 0; for (int i = 0; i < MB / 64; ++i) { int t = scan[i]; scan[i] = acc; acc += t; } scan[MB / 64] = acc; }
    __syncthreads();
    int base = scan[w];
    *total = scan[MB / 64];
    __syncthreads();
    return base + x - v;
}

// Single-transform evaluation of the uniformity metric, first half: inlier test of every correspondence (the same expressions as
// metric_kernel), inlier mask, the three projection histograms and the inlier count -- integer counts, so any order gives the
// same numbers -- spread over the whole device; metric_kernel then does the entropy part from the finished histogram.  (One
// workgroup walking 3e5 correspondences for ONE hypothesis cost 0.19 ms per evaluation, two evaluations per alignment.)
__global__ __launch_bounds__(256) void inlier_hist_kernel(const float* __restrict__ T16, const float4* __restrict__ P0, const float4* __restrict__ P1,
                                                          const float* __restrict__ sstar, int c, uint8_t* __restrict__ mask, int* __restrict__ ghist /* [30000 + 1], zeroed */) {
    __shared__ float T[16];
    if (threadIdx.x < 16) T[threadIdx.x] = T16[threadIdx.x];
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool in = false;
    if (i < c) {
        float4 a = P0[i], b = P1[i];
        LGR_APPLY(T, a.x, a.y, a.z, ox, oy, oz)
        float dx = ox - b.x, dy = oy - b.y, dz = oz - b.z;
        float d4 = (dx * dx + dz * dz) + (dy * dy + 0.f);
        in = d4 < sstar[i];
        if (mask) mask[i] = in ? 1 : 0;
        if (in) {
            const int bins = __float_as_int(b.w);
            const int b0 = bins & 0xff, b1 = (bins >> 8) & 0xff, b2 = (bins >> 16) & 0xff;
            atomicAdd(&ghist[(0 * 100 + b1) * 100 + b2], 1);
            atomicAdd(&ghist[(1 * 100 + b2) * 100 + b0], 1);
            atomicAdd(&ghist[(2 * 100 + b0) * 100 + b1], 1);
        }
    }
    const unsigned long long m = __ballot(in);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ghist[30000], __popcll(m));
}

// (the body: one workgroup of MB threads = workgroup `wg` of `n_wg`; the resident RANSAC kernel runs it as one of its phases.  No __restrict__
// on what another phase of that kernel writes.)
__device__ __forceinline__ void metric_body(const int tid, const int wg, const int n_wg, const float* Ts, const int* list2, int nh2,
                                            const float4* __restrict__ P0, const float4* __restrict__ P1,
                                            const float* __restrict__ sstar, int c, int metric_id, int score_id,
                                            float* metric_out, int* ninl_out, float* rmse_out, uint8_t* mask,
                                            float2* scratch, const unsigned* maskT, const int* hpos, int mask_nh,
                                            const int* ghist, const int* nh2_dev, const int* mask_nh_dev) {
    extern __shared__ int hist[];   // 30000 ints (uniformity) + 64 ints scan scratch
    __shared__ float T[16];
    __shared__ int s_count;
    __shared__ int s_nnz[3];
    __shared__ float ent[3];
    if (nh2_dev) {
        nh2 = *nh2_dev;
        const int cols = *mask_nh_dev;   // hypotheses count_list_kernel wrote mask columns for (its stride)
        if (cols > mask_nh) maskT = nullptr;
        mask_nh = cols;
    }
  for (int hb = wg; hb < nh2; hb += n_wg) {
    __syncthreads();   // the previous candidate of this workgroup is finished with the shared arrays
    int hyp = list2 ? list2[hb] : hb;
    if (tid < 16) T[tid] = Ts[(size_t) hyp * 16 + tid];
    const bool uni = metric_id == LGR_METRIC_UNIFORMITY;
    if (uni) for (int i = tid; i < 30000; i += MB) hist[i] = 0;
    if (tid == 0) s_count = 0;
    int* scan = hist + 30000;
    float2* lst = scratch ? scratch + (size_t) wg * c : nullptr;   // one list per workgroup
    __syncthreads();
    const bool from_hist = ghist && uni && !lst;
    if (from_hist) {
        for (int i = tid; i < 30000; i += MB) hist[i] = ghist[i];
        if (tid == 0) s_count = ghist[30000];
    }
    const bool from_bits = !from_hist && maskT && uni && !lst && !mask;
    if (from_bits) {
        // uniformity needs the inlier SET only: walk the set bits of the masks the counting phase left (a candidate has a
        // few thousand inliers among hundreds of thousands of correspondences)
        // (a row is contiguous: consecutive lanes read consecutive words, four words per lane in flight; the bins of up to MG inliers are requested
        //  before the first of them is counted: the loop is a chain of dependent gathers, MG deep instead of one)
        constexpr int MG = LGR_METRIC_GATHERS;
        const unsigned* row = maskT + (size_t) hpos[hb] * mask_pitch(c);
        const int n_words = (c + 31) >> 5;
        int cnt = 0;
        for (int w0 = tid; w0 < n_words; w0 += 4 * MB) {
            unsigned mw[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) mw[k] = w0 + k * MB < n_words ? row[w0 + k * MB] : 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                unsigned m = mw[k];
                cnt += __popc(m);
                const int i0 = ((w0 + k * MB) << 5) - 1;
                while (m) {
                    int bins[MG];
                    bool on[MG];
#pragma unroll
                    for (int u = 0; u < MG; ++u) {
                        on[u] = m != 0u;
                        const int i = i0 + (on[u] ? __ffs((int) m) : 1);
                        m &= m - 1u;   // (0 stays 0)
                        bins[u] = on[u] ? __float_as_int(P1[i].w) : 0;
                    }
#pragma unroll
                    for (int u = 0; u < MG; ++u) {
                        if (!on[u]) continue;
                        const int b0 = bins[u] & 0xff, b1 = (bins[u] >> 8) & 0xff, b2 = (bins[u] >> 16) & 0xff;
                        atomicAdd(&hist[(0 * 100 + b1) * 100 + b2], 1);
                        atomicAdd(&hist[(1 * 100 + b2) * 100 + b0], 1);
                        atomicAdd(&hist[(2 * 100 + b0) * 100 + b1], 1);
                    }
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if ((tid & 63) == 0 && cnt) atomicAdd(&s_count, cnt);
    }
    for (int base = 0; base < c && !from_bits && !from_hist; base += MB) {
        int i = base + tid;
        bool in = false;
        float dist = 0.f, thr = 0.f;
        int bins = 0;
        if (i < c) {
            float4 a = P0[i], b = P1[i];
            LGR_APPLY(T, a.x, a.y, a.z, ox, oy, oz)
            float dx = ox - b.x, dy = oy - b.y, dz = oz - b.z;
            float d4 = (dx * dx + dz * dz) + (dy * dy + 0.f);
            in = d4 < sstar[i];
            thr = a.w; bins = __float_as_int(b.w);
            if (in && lst) dist = __builtin_sqrtf(d4);
            if (mask) mask[i] = in ? 1 : 0;
        }
        if (uni && in) {
            int b0 = bins & 0xff, b1 = (bins >> 8) & 0xff, b2 = (bins >> 16) & 0xff;
            atomicAdd(&hist[(0 * 100 + b1) * 100 + b2], 1);   // count[k][bin[(k+1)%3]][bin[(k+2)%3]]
            atomicAdd(&hist[(1 * 100 + b2) * 100 + b0], 1);
            atomicAdd(&hist[(2 * 100 + b0) * 100 + b1], 1);
        }
        if (!lst) {
            // uniformity without an ordered list: only the inlier count is needed (order-free)
            unsigned long long m = __ballot(in);
            if ((tid & 63) == 0 && m) atomicAdd(&s_count, __popcll(m));
        } else {
            // ordered compaction of the inliers of this tile
            int tot;
            int pos = block_excl_scan_1024(in ? 1 : 0, scan, tid, &tot);
            if (in) lst[s_count + pos] = make_float2(dist, thr);
            __syncthreads();
            if (tid == 0) s_count += tot;
            __syncthreads();
        }
    }
    __syncthreads();
    int n_inl = s_count;
    if (uni) {
        // entropy_k = -(sum over bins in ascending order of p log p) / log(1e4)   (src/analysis.cpp:114-127).
        // The terms are computed in parallel, compacted IN BIN ORDER over the (dead) histogram slab, then summed
        // sequentially by one lane per projection: the reference's summation order, without 10^4 serial steps.
        float n = (float) n_inl;
        for (int k = 0; k < 3; ++k) {
            int* hk = hist + k * 10000;
            int cntv[10];
            int nz = 0;
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                cntv[j] = tid < 1000 ? hk[tid * 10 + j] : 0;
                float p = (float) cntv[j] / n;
                nz += (cntv[j] != 0 && p != 0.f) ? 1 : 0;
            }
            int tot;
            int pos = block_excl_scan_1024(nz, scan, tid, &tot);   // its barriers retire every read of hk before the writes below
            float* tk = reinterpret_cast<float*>(hk);
#pragma unroll
            for (int j = 0; j < 10; ++j) {
                float p = (float) cntv[j] / n;
                if (cntv[j] != 0 && p != 0.f) { tk[pos] = p * lgr_logf(p); ++pos; }
            }
            if (tid == 0) s_nnz[k] = tot;
            __syncthreads();
        }
        if (tid == 0 || tid == 64 || tid == 128) {
            int k = tid >> 6;
            const float* tk = reinterpret_cast<const float*>(hist + k * 10000);
            float e = 0.f;
            int nn = s_nnz[k];
            // (the reference's order: one dependent subtraction per non-empty bin, up to 10 000 of them; the reads run ahead of the chain in blocks
            //  of sixteen -- as a plain loop every term waited for its own LDS read: 100 of the 140 us a candidate of 80 000 inliers took)
            int j = 0;
            for (; j + 16 <= nn; j += 16) {
                const float4 t0 = *reinterpret_cast<const float4*>(tk + j), t1 = *reinterpret_cast<const float4*>(tk + j + 4);
                const float4 t2 = *reinterpret_cast<const float4*>(tk + j + 8), t3 = *reinterpret_cast<const float4*>(tk + j + 12);
                e -= t0.x; e -= t0.y; e -= t0.z; e -= t0.w; e -= t1.x; e -= t1.y; e -= t1.z; e -= t1.w;
                e -= t2.x; e -= t2.y; e -= t2.z; e -= t2.w; e -= t3.x; e -= t3.y; e -= t3.z; e -= t3.w;
            }
            for (; j < nn; ++j) e -= tk[j];
            e /= 9.210340371976184f;
            ent[k] = e;
        }
        __syncthreads();
        if (tid == 0) {
            float m = n_inl == 0 ? 0.f : lgr_cbrtf(ent[0] * ent[1] * ent[2]);
            metric_out[hb] = m;
            ninl_out[hb] = n_inl;
        }
    }
    // The score and the rmse are sequential float sums over the inliers in correspondence order (src/metric.cpp:55-81, 147-155); their TERMS are not:
    // the whole workgroup turns the list's (distance, threshold) entries into (distance^2, score term) in place -- plane_score's expressions
    // (lgr_plane_point.cuh) with (d, t) for (dist, thr), by another thread; a copy, because the call changed the code of metric_kernel and
    // rs_resident_kernel -- and one lane adds them up with its reads running sixteen terms ahead of the two dependent chains.  (Round 5: as
    // one loop on one lane, every term waited for its own global load and its division.)
    if (lst && (!uni || rmse_out)) {   // (workgroup uniform)
        for (int j = tid; j < n_inl; j += MB) {
            const float2 dt = lst[j];
            const float d = dt.x, t = dt.y;
            float value = 1.f;
            if (score_id == LGR_SCORE_MAE) value = fabsf(d - t) / t;
            else if (score_id == LGR_SCORE_MSE) value = (d - t) * (d - t) / (t * t);
            else if (score_id == LGR_SCORE_EXP) value = lgr_expf(-d * d / (2 * t * t));
            lst[j] = make_float2(d * d, value);
        }
        __syncthreads();
    }
    if (tid == 0 && (!uni || rmse_out)) {
        float score = 0.f, rm = 0.f;
        if (lst) {
            int j = 0;
            for (; j + 8 <= n_inl; j += 8) {
                float2 e[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) e[u] = lst[j + u];
#pragma unroll
                for (int u = 0; u < 8; ++u) { rm += e[u].x; score += e[u].y; }
            }
            for (; j < n_inl; ++j) { const float2 e = lst[j]; rm += e.x; score += e.y; }
        }
        if (!uni) { metric_out[hb] = score / (float) c; ninl_out[hb] = n_inl; }
        if (rmse_out) rmse_out[hb] = n_inl ? __builtin_sqrtf(rm / (float) n_inl) : 3.4028234663852886e38f;
    }
  }
}
__global__ __launch_bounds__(MB) void metric_kernel(const float* __restrict__ Ts, const int* __restrict__ list2, int nh2,
                                                     const float4* __restrict__ P0, const float4* __restrict__ P1,
                                                     const float* __restrict__ sstar, int c, int metric_id, int score_id,
                                                     float* __restrict__ metric_out, int* __restrict__ ninl_out,
                                                     float* __restrict__ rmse_out, uint8_t* __restrict__ mask,
                                                     float2* __restrict__ scratch /* [gridDim.x][c] inlier (dist, thr) lists */,
                                                     const unsigned* __restrict__ maskT /* count_item's inlier bits [mask_nh][mask_pitch(c)], or nullptr */,
                                                     const int* __restrict__ hpos /* candidate -> row of maskT */, int mask_nh,
                                                     const int* __restrict__ ghist = nullptr /* [30000 + 1]: the uniformity histogram and the inlier count of the ONE
                                                        hypothesis, already counted by inlier_hist_kernel (single-transform evaluations) */,
                                                     const int* __restrict__ nh2_dev = nullptr /* device-driven schedule: the number of candidates lives on the
                                                        device and the grid strides over them; maskT is used when mask_nh_dev[0] <= mask_nh */,
                                                     const int* __restrict__ mask_nh_dev = nullptr) {
    metric_body(threadIdx.x, blockIdx.x, gridDim.x, Ts, list2, nh2, P0, P1, sstar, c, metric_id, score_id, metric_out, ninl_out, rmse_out, mask, scratch, maskT, hpos, mask_nh,
                ghist, nh2_dev, mask_nh_dev);
}

// ---------------------------------------------------------------------------------------------------- plumbing
__global__ void plane_pack_kernel(const float* __restrict__ src, const float* __restrict__ tgt, const int2* __restrict__ pairs, int n,
                                  float4* __restrict__ P0, float4* __restrict__ P1) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* s = src + (size_t) pairs[i].x * 12;
    const float* t = tgt + (size_t) pairs[i].y * 12;
    P0[i] = make_float4(s[0], s[1], s[2], 0.f);
    P1[i] = make_float4(t[0], t[1], t[2], 0.f);
}
__global__ void compact_kernel(const int* __restrict__ flags, const int* __restrict__ pos, int n, const int* __restrict__ map,
                               int* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flags[i]) out[pos[i]] = map ? map[i] : i;
}

// ordered compaction of the inlier pairs (mask -> flags -> exclusive scan -> scatter) ahead of the sequential refit
__global__ void mask_flags_kernel(const uint8_t* __restrict__ mask, int c, int* __restrict__ flags) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c) flags[i] = mask[i] ? 1 : 0;
}
__global__ void compact_pairs_kernel(const float4* __restrict__ P0, const float4* __restrict__ P1, const int* __restrict__ flags,
                                     const int* __restrict__ pos, int c, float4* __restrict__ Q0, float4* __restrict__ Q1) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < c && flags[i]) { Q0[pos[i]] = P0[i]; Q1[pos[i]] = P1[i]; }
}

__global__ void corr_range_kernel(const lgr_corr* __restrict__ corr, int c, int ns, int nt, int* __restrict__ bad) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool b = false;
    if (i < c) {
        lgr_corr cr = corr[i];
        b = (unsigned) cr.index_query >= (unsigned) ns || (unsigned) cr.index_match >= (unsigned) nt;
    }
    if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
}

// ---------------------------------------------------------------------------------------------------- refit
// src/transformation.cpp:4-38: sequential float sums over the inliers in correspondence order.  Lanes 0..5 own the
// six centroid accumulators, then lanes 0..8 the nine entries of H; the SVD and R, t follow on lane 0.
constexpr int RCH = 2048;   // pairs staged per chunk
__global__ __launch_bounds__(256) void refit_kernel(const float4* __restrict__ P0, const float4* __restrict__ P1, int c, float* __restrict__ Tout,
                                                    const int* __restrict__ n_a = nullptr, const int* __restrict__ n_b = nullptr) {
    // every pair of P0 / P1 counts: the callers compact the inliers first (refit_launch), so there is no per-element branch and the LDS
    // reads run ahead of the dependent adds
    if (n_a) c = n_a[0] + n_b[0];   // the number of compacted pairs stayed on the device: last exclusive-scan entry + last flag
    // the sums are sequential by definition; the pairs are staged through LDS by the whole block (coalesced loads), so the
    // summing lanes walk LDS instead of waiting on one global load per term
    // (round 5: the staged chunk is COMPONENT-major, so a summing lane reads consecutive words; in the second pass the whole block also forms the
    //  nine products per pair -- the same two subtractions and one multiplication, by another thread -- and the summing lanes are left with one LDS
    //  read and the one dependent addition per term: 80 000 inliers 2.0 -> ~1 ms, the lanes were bound by instruction issue, not by the chain)
    constexpr int RCH2 = 1024;        // pairs per chunk of the second pass (nine products per pair in the same array)
    __shared__ float sp[RCH * 8];     // pass 1: [6 components][RCH]; pass 2: [9 products][RCH2]
    __shared__ float cen[6];
    __shared__ float Hs[9];
    __shared__ int sn;
    const int l = threadIdx.x;
    {
        float acc = 0.f;
        int n = 0;
        for (int i0 = 0; i0 < c; i0 += RCH) {
            __syncthreads();
            for (int i = l; i < RCH && i0 + i < c; i += blockDim.x) {
                const float4 p = P0[i0 + i], q = P1[i0 + i];
                sp[0 * RCH + i] = p.x; sp[1 * RCH + i] = p.y; sp[2 * RCH + i] = p.z;
                sp[3 * RCH + i] = q.x; sp[4 * RCH + i] = q.y; sp[5 * RCH + i] = q.z;
            }
            __syncthreads();
            if (l < 6) {
                const int m = min(RCH, c - i0);
                const float* col = sp + l * RCH;
#pragma unroll 16
                for (int i = 0; i < m; ++i) acc += col[i];
                n += m;
            }
        }
        if (l < 6) cen[l] = acc / (float) n;
        if (l == 0) sn = n;
    }
    {
        float acc = 0.f;
        for (int i0 = 0; i0 < c; i0 += RCH2) {
            __syncthreads();   // (the first one also publishes cen[])
            float cc[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) cc[k] = cen[k];
            for (int i = l; i < RCH2 && i0 + i < c; i += blockDim.x) {
                const float4 p = P0[i0 + i], q = P1[i0 + i];
                const float da[3] = {p.x - cc[0], p.y - cc[1], p.z - cc[2]}, db[3] = {q.x - cc[3], q.y - cc[4], q.z - cc[5]};
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b = 0; b < 3; ++b) sp[(3 * a + b) * RCH2 + i] = da[a] * db[b];
            }
            __syncthreads();
            if (l < 9) {
                const int m = min(RCH2, c - i0);
                const float* col = sp + l * RCH2;
#pragma unroll 16
                for (int i = 0; i < m; ++i) acc += col[i];
            }
        }
        if (l < 9) Hs[l] = acc;
    }
    __syncthreads();
    if (l == 0) {
        float T[16];
        if (sn == 0) {
_Pragma("unroll")
            for (int i = 0; i < 16; ++i) T[i] = __uint_as_float(0x7fc00000u);   // 0/0 centroids in the reference
        } else {
            float H[9], U[9], Sg[3], V[9], R[9];
            _Pragma("unroll") for (int i = 0; i < 9; ++i) H[i] = Hs[i];
            lgr_svd3(H, U, Sg, V);
            _Pragma("unroll") for (int i = 0; i < 3; ++i)
                _Pragma("unroll") for (int j = 0; j < 3; ++j)
                    R[3 * i + j] = (V[3 * i + 0] * U[3 * j + 0] + V[3 * i + 1] * U[3 * j + 1]) + V[3 * i + 2] * U[3 * j + 2];
            if (lgr_det3(R) < 0.f) {
                V[2] = -V[2]; V[5] = -V[5]; V[8] = -V[8];
                _Pragma("unroll") for (int i = 0; i < 3; ++i)
                    _Pragma("unroll") for (int j = 0; j < 3; ++j)
                        R[3 * i + j] = (V[3 * i + 0] * U[3 * j + 0] + V[3 * i + 1] * U[3 * j + 1]) + V[3 * i + 2] * U[3 * j + 2];
            }
            float t[3];
            _Pragma("unroll") for (int i = 0; i < 3; ++i) t[i] = cen[3 + i] - ((R[3 * i + 0] * cen[0] + R[3 * i + 1] * cen[1]) + R[3 * i + 2] * cen[2]);
            _Pragma("unroll") for (int i = 0; i < 16; ++i) T[i] = 0.f;
            _Pragma("unroll") for (int i = 0; i < 3; ++i) {
                _Pragma("unroll") for (int j = 0; j < 3; ++j) T[4 * j + i] = R[3 * i + j];
                T[12 + i] = t[i];
            }
            T[15] = 1.f;
        }
_Pragma("unroll")
        for (int i = 0; i < 16; ++i) Tout[i] = T[i];
    }
}

}  // namespace
