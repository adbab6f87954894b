// lgr_match_local_knn.hip -- matchLocal with a KNNResult(randomness) list and matchFLANN, for FPFH (33), RoPS135 (135) and SHOT352 (352)
// rows on gfx950.
//
//   matchLocal<FeatureT>, randomness = k (include/matching.h:637-678, KNNResult :44-94) -> lgr_match_local_knn*
//   matchFLANN<FeatureT>, randomness = 1 (:562-592)                                     -> lgr_match_flann_rows*
//
// The statement.  matchLocal: the moved query point is x*c0 + (y*c1 + (z*c2 + c3)) per coordinate
// (pcl::detail::Transformer::se3).  A query row is valid when all row_len floats are finite; a non-finite moved point has no candidates; a candidate is a
// finite train point whose s = lgr_dist2(moved, point) satisfies strict s < r*r and whose row is all finite.  The descriptor distance is
// pcl::L2_Norm: sum = 0; for j ascending: d = q[j] - t[j]; sum += d * d (no contraction); sqrtf.  A query's list is the first k candidates
// in ascending (distance, s, train index), then -1 / 0.f: KNNResult puts a later equal distance behind an earlier one, radiusSearch
// visits by ascending spatial distance, and the index is the project's choice for FLANN's unspecified order.  A radius whose square is
// not finite (FLT_MAX) makes every finite train point with a finite s a candidate; radius 0 leaves none.  For (row_len 33, k 1) the result
// is what lgr_match_local*'s own kernel gave, bit for bit (they are this entry point now: lgr_match_local.hip).  matchFLANN: the row is the brute-force matcher's with a single train block (argmin under OpenCV's
// lane order, lowest index at equal distance), the reported distance sqrtf of the sequential sum above; -1 / 0.f for an invalid query.
//
// One thread per query with the row in registers (the FPFH-only kernel this replaces) works for 33 floats and cannot for 352: it would
// spill.  Here a wave owns a
// query: the query row lies in LDS and is read wave-uniformly (a broadcast, no bank conflicts), every lane computes ONE candidate's
// sequential distance, and the list is the k smallest 96-bit keys (distance bits, s bits, index) -- non-negative floats order like their
// bit patterns -- held one entry per lane in lanes 0..k-1.  The keys of one list are distinct, so the order in which candidates arrive
// cannot show in the result (the argument of knn_match_kernel).
//   GRID   the candidates of the 27 cells around the moved point (cell = 1.001 * radius), gathered through a per-wave LDS buffer so that
//          a full wave of points that passed the radius test computes distances; train rows are read from memory.
//   !GRID  every train point: 64-row train tiles with their points staged in LDS (row stride padded so that the lanes' 16-byte reads
//          fall on distinct slots), shared by the block's 4 waves x 4 queries.
// The per-pair arithmetic (pair_distance) is the same function in both.
#include <algorithm>
#include <cmath>

#include "lgr_grid.cuh"
#include "lgr_host.h"
#include "lgr_internal.h"

namespace {

constexpr int KMAX = LGR_RANDOMNESS_MAX;
constexpr int WAVES = 4;   // waves per block
constexpr int QPW = 4;     // queries per wave of the tiled scan
constexpr int TILE = 64;   // train rows per tile: one per lane

__device__ __forceinline__ bool finite1(float v) { return fabsf(v) <= 3.4028234663852886e38f; }

// (distance bits << 32 | s bits, train index); NONE sorts behind every candidate (a distance's bits are at most +inf's)
struct Key { unsigned long long ds; unsigned j; };
__device__ __forceinline__ Key key_none() { return Key{~0ull, ~0u}; }
__device__ __forceinline__ bool key_less(const Key& a, const Key& b) { return a.ds < b.ds || (a.ds == b.ds && a.j < b.j); }
__device__ __forceinline__ Key key_from_lane(const Key& v, int src) { return Key{__shfl(v.ds, src), __shfl(v.j, src)}; }

// the wave's ascending list, entry e in lane e: K enters in front of the first larger entry, the entries behind it move one lane up
__device__ __forceinline__ void list_insert(Key& mine, const Key& K, int lane) {
    const Key prev{__shfl_up(mine.ds, 1), __shfl_up(mine.j, 1)};
    if (key_less(K, mine)) mine = (lane == 0 || !key_less(K, prev)) ? K : prev;
}

// the lanes' candidates (has: this lane holds one) that are below the list's k-th entry enter it, lowest lane first
__device__ __forceinline__ void list_merge(Key& mine, bool has, const Key& cand, int k, int lane) {
    for (;;) {
        const Key worst = key_from_lane(mine, k - 1);
        const unsigned long long m = __ballot(has && key_less(cand, worst));
        if (!m) break;
        const int src = __ffsll(m) - 1;
        list_insert(mine, key_from_lane(cand, src), lane);
        if (lane == src) has = false;
    }
}

// pcl::L2_Norm of (query row in LDS, train row t), sequentially from dimension 0; false when the train row holds a non-finite float
template <int ROW>
__device__ __forceinline__ bool pair_distance(const float4* q4, const float* __restrict__ t, float& d) {
    float sum = 0.f;
    bool ok = true;
#pragma unroll 4
    for (int j = 0; j + 4 <= ROW; j += 4) {
        const float4 q = q4[j >> 2];
        const float t0 = t[j], t1 = t[j + 1], t2 = t[j + 2], t3 = t[j + 3];
        ok = ok && finite1(t0) && finite1(t1) && finite1(t2) && finite1(t3);
        float e = q.x - t0; sum += e * e;
        e = q.y - t1; sum += e * e;
        e = q.z - t2; sum += e * e;
        e = q.w - t3; sum += e * e;
    }
    const float* q = reinterpret_cast<const float*>(q4);
#pragma unroll
    for (int j = ROW / 4 * 4; j < ROW; ++j) {
        const float tj = t[j];
        ok = ok && finite1(tj);
        const float e = q[j] - tj; sum += e * e;
    }
    d = __builtin_sqrtf(sum);
    return ok;
}

__device__ __forceinline__ Key make_key(float d, float s, int j) {
    return Key{(unsigned long long) __float_as_uint(d) << 32 | __float_as_uint(s), (unsigned) j};
}

// lanes copy query row i into LDS; true when all of it is finite (wave-uniform)
template <int ROW>
__device__ __forceinline__ bool load_query_row(const float* __restrict__ qf, int i, float* qs, int lane) {
    bool fin = true;
    for (int j = lane; j < ROW; j += 64) {
        const float v = qf[(size_t) i * ROW + j];
        qs[j] = v;
        fin = fin && finite1(v);
    }
    return __all(fin);
}

// pcl::detail::Transformer::se3: x * c0 + (y * c1 + (z * c2 + c3))
__device__ __forceinline__ bool moved_point(const float* __restrict__ qpts, int i, const float* __restrict__ G, float& x, float& y, float& z) {
    const float px = qpts[(size_t) i * 12], py = qpts[(size_t) i * 12 + 1], pz = qpts[(size_t) i * 12 + 2];
    x = G[0] * px + (G[4] * py + (G[8] * pz + G[12]));
    y = G[1] * px + (G[5] * py + (G[9] * pz + G[13]));
    z = G[2] * px + (G[6] * py + (G[10] * pz + G[14]));
    return lgr_finite3(x, y, z);
}

__device__ __forceinline__ void store_list(const Key& mine, int i, int k, int lane, int32_t* __restrict__ idx, float* __restrict__ dist) {
    if (lane >= k) return;
    const bool none = mine.ds == ~0ull;
    idx[(size_t) i * k + lane] = none ? -1 : (int32_t) mine.j;
    dist[(size_t) i * k + lane] = none ? 0.f : __uint_as_float((unsigned) (mine.ds >> 32));
}

// the wave's LDS traffic is its own: order it without a block barrier
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

template <int ROW, bool GRID>
__global__ __launch_bounds__(WAVES * 64) void local_knn_kernel(GridDev g, const float* __restrict__ qpts, int mq, const float* __restrict__ tpts, int mt,
                                                               const float* __restrict__ qf, const float* __restrict__ tf,
                                                               const float* __restrict__ G /* 16, device */, float r2, int k,
                                                               int32_t* __restrict__ idx, float* __restrict__ dist) {
    constexpr int ROW4 = (ROW + 3) / 4;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if constexpr (GRID) {
        __shared__ float4 qrow[WAVES][ROW4];
        __shared__ int pend_j[WAVES][128];     // train points that passed the radius test and wait for a full wave
        __shared__ float pend_s[WAVES][128];
        const int i = blockIdx.x * WAVES + w;
        if (i >= mq) return;   // (wave-uniform; this branch has no block barrier)
        bool valid = load_query_row<ROW>(qf, i, reinterpret_cast<float*>(qrow[w]), lane);
        float x = 0.f, y = 0.f, z = 0.f;
        valid = moved_point(qpts, i, G, x, y, z) && valid;
        wave_sync();
        Key mine = key_none();
        // n (at most 64) waiting candidates from position base on: one per lane
        auto process = [&](int base, int n) {
            bool has = lane < n;
            Key c = key_none();
            if (has) {
                const int j = pend_j[w][base + lane];
                const float s = pend_s[w][base + lane];
                float d;
                has = pair_distance<ROW>(qrow[w], tf + (size_t) j * ROW, d);
                c = make_key(d, s, j);
            }
            list_merge(mine, has, c, k, lane);
        };
        if (valid && g.n > 0) {
            int npend = 0;
            // the cells of lgr_visit27, a wave's width of points at a time
            const int cx = lgr_cellc(x, g.ox, g.h), cy = lgr_cellc(y, g.oy, g.h), cz = lgr_cellc(z, g.oz, g.h);
            for (int zz = max(cz - 1, 0); zz <= min(cz + 1, g.dz - 1); ++zz)
                for (int yy = max(cy - 1, 0); yy <= min(cy + 1, g.dy - 1); ++yy) {
                    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dx - 1);
                    if (x0 > x1) continue;
                    const size_t c = ((size_t) zz * g.dy + yy) * g.dx;
                    const int b = g.cell_start[c + x0], e = g.cell_start[c + x1 + 1];   // three x-cells are contiguous
                    for (int t0 = b; t0 < e; t0 += 64) {
                        const int t = t0 + lane;
                        bool pass = false;
                        float s = 0.f;
                        int j = 0;
                        if (t < e) {
                            const float4 P = g.pxyz[t];
                            s = lgr_dist2(x, y, z, P.x, P.y, P.z);
                            pass = s < r2;
                            j = __float_as_int(P.w);
                        }
                        const unsigned long long m = __ballot(pass);
                        if (pass) {
                            const int pos = npend + __popcll(m & ((1ull << lane) - 1ull));   // < 64 waiting + at most 64 new <= 127
                            pend_j[w][pos] = j;
                            pend_s[w][pos] = s;
                        }
                        npend += __popcll(m);
                        wave_sync();
                        if (npend >= 64) {
                            npend -= 64;
                            process(npend, 64);   // the last 64: the rest stays where it is
                            wave_sync();
                        }
                    }
                }
            if (npend > 0) process(0, npend);
        }
        store_list(mine, i, k, lane, idx, dist);
    } else {
        constexpr int STRIDE = (ROW + 6) / 4 * 4;   // row, then x y z: 36 / 140 / 356 floats, a multiple of 4 that is 4 mod 8 (16 lanes' 16-byte reads on 16 slots)
        __shared__ float4 tile4[TILE * STRIDE / 4];
        __shared__ float4 qrow[WAVES * QPW][ROW4];
        float* tile = reinterpret_cast<float*>(tile4);
        const int q0 = blockIdx.x * (WAVES * QPW) + w * QPW;
        Key mine[QPW];
        float x[QPW], y[QPW], z[QPW];
        bool valid[QPW];
#pragma unroll
        for (int u = 0; u < QPW; ++u) {
            mine[u] = key_none();
            x[u] = y[u] = z[u] = 0.f;
            valid[u] = q0 + u < mq;
            if (valid[u]) {
                valid[u] = load_query_row<ROW>(qf, q0 + u, reinterpret_cast<float*>(qrow[w * QPW + u]), lane);
                valid[u] = moved_point(qpts, q0 + u, G, x[u], y[u], z[u]) && valid[u];
            }
        }
        for (int j0 = 0; j0 < mt; j0 += TILE) {
            const int nj = min(TILE, mt - j0);
            __syncthreads();
            for (int e = threadIdx.x; e < nj * ROW; e += WAVES * 64) {
                const int r = e / ROW, c = e - r * ROW;
                tile[r * STRIDE + c] = tf[(size_t) j0 * ROW + e];
            }
            for (int e = threadIdx.x; e < nj * 3; e += WAVES * 64) {
                const int r = e / 3, c = e - r * 3;
                tile[r * STRIDE + ROW + c] = tpts[(size_t) (j0 + r) * 12 + c];
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < QPW; ++u) {
                if (!valid[u]) continue;   // (wave-uniform)
                bool has = false;
                Key c = key_none();
                if (lane < nj) {
                    const float* t = tile + lane * STRIDE;
                    const float tx = t[ROW], ty = t[ROW + 1], tz = t[ROW + 2];
                    if (lgr_finite3(tx, ty, tz)) {
                        const float s = lgr_dist2(x[u], y[u], z[u], tx, ty, tz);
                        if (s < r2) {
                            float d;
                            has = pair_distance<ROW>(qrow[w * QPW + u], t, d);
                            c = make_key(d, s, j0 + lane);
                        }
                    }
                }
                list_merge(mine[u], has, c, k, lane);
            }
        }
#pragma unroll
        for (int u = 0; u < QPW; ++u)
            if (q0 + u < mq) store_list(mine[u], q0 + u, k, lane, idx, dist);
    }
}

// distance of an already chosen match in FLANN's order (include/matching.h:586-588: std::sqrt of the squared distance nearestKSearch
// returns): flann_dist_kernel for any row length, the rows read where they lie
template <int ROW>
__global__ void flann_dist_rows_kernel(const float* __restrict__ qf, const float* __restrict__ tf, const int32_t* __restrict__ idx, int mq, float* __restrict__ dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= mq) return;
    const int j = idx[i];
    if (j < 0) { dist[i] = 0.f; return; }
    const float* q = qf + (size_t) i * ROW;
    const float* t = tf + (size_t) j * ROW;
    float sum = 0.f;
#pragma unroll 8
    for (int e = 0; e < ROW; ++e) { const float d = q[e] - t[e]; sum += d * d; }
    dist[i] = __builtin_sqrtf(sum);
}

template <int ROW>
void launch_local_knn(lgr_ctx* ctx, bool use_grid, const GridDev& g, const float* d_qpts, int mq, const float* d_tpts, int mt, const float* d_q, const float* d_t,
                      const float* dG, float r2, int k, int32_t* d_idx, float* d_dist) {
    if (use_grid) local_knn_kernel<ROW, true><<<cdiv(mq, WAVES), WAVES * 64, 0, ctx->stream>>>(g, d_qpts, mq, d_tpts, mt, d_q, d_t, dG, r2, k, d_idx, d_dist);
    else local_knn_kernel<ROW, false><<<cdiv(mq, WAVES * QPW), WAVES * 64, 0, ctx->stream>>>(g, d_qpts, mq, d_tpts, mt, d_q, d_t, dG, r2, k, d_idx, d_dist);
}

bool row_len_built(int row_len) { return row_len == 33 || row_len == 135 || row_len == 352; }

int fill_none(lgr_ctx* ctx, int32_t* d_idx, float* d_dist, size_t n) {
    LGR_HIP(ctx, hipMemsetAsync(d_idx, 0xff, n * 4, ctx->stream));
    LGR_HIP(ctx, hipMemsetAsync(d_dist, 0, n * 4, ctx->stream));
    return LGR_OK;
}

}  // namespace

extern "C" int lgr_match_local_knn_dev(lgr_ctx* ctx, int row_len, const float* d_qpts, int mq, const float* d_tpts, int mt, const float* d_q, const float* d_t,
                                       const float guess16[16], float radius, int k, int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, k >= 1 && k <= KMAX && row_len_built(row_len), LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, mq >= 0 && mt >= 0 && (d_qpts || mq == 0) && (d_tpts || mt == 0) && (d_q || mq == 0) && (d_t || mt == 0) && (d_idx || mq == 0) &&
                   (d_dist || mq == 0) && guess16 && radius >= 0.f, LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const float r2 = radius * radius;
    if (mt == 0 || r2 == 0.f) return fill_none(ctx, d_idx, d_dist, (size_t) mq * k);   // strict s < 0 holds for no point
    float* dG;
    LGR_TRY(lgr_ws_t(ctx, WS_LOCAL_G, 64, &dG));
    LGR_HIP(ctx, hipMemcpyAsync(dG, guess16, 64, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));   // guess16 is the caller's
    GridDev g{};
    const bool use_grid = std::isfinite(r2);
    if (use_grid) LGR_TRY(lgr_grid_build(ctx, WS_GRID_C, d_tpts, mt, radius * 1.001f, 0.f, &g));
    if (row_len == 33) launch_local_knn<33>(ctx, use_grid, g, d_qpts, mq, d_tpts, mt, d_q, d_t, dG, r2, k, d_idx, d_dist);
    else if (row_len == 135) launch_local_knn<135>(ctx, use_grid, g, d_qpts, mq, d_tpts, mt, d_q, d_t, dG, r2, k, d_idx, d_dist);
    else launch_local_knn<352>(ctx, use_grid, g, d_qpts, mq, d_tpts, mt, d_q, d_t, dG, r2, k, d_idx, d_dist);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

extern "C" int lgr_match_flann_rows_dev(lgr_ctx* ctx, int row_len, const float* d_q, int mq, const float* d_t, int mt, int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, row_len_built(row_len), LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, mq >= 0 && mt >= 0 && (d_q || mq == 0) && (d_t || mt == 0) && (d_idx || mq == 0) && (d_dist || mq == 0), LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    if (mt == 0) return fill_none(ctx, d_idx, d_dist, (size_t) mq);
    // a single train block: the tie rule of the brute-force kernels is then "lowest index", the oracle's choice for FLANN's unspecified order
    if (row_len == 33) {
        LGR_TRY(lgr_match_bf_dev(ctx, d_q, mq, d_t, mt, mt, d_idx, d_dist));
        flann_dist_rows_kernel<33><<<cdiv(mq, 128), 128, 0, ctx->stream>>>(d_q, d_t, d_idx, mq, d_dist);
    } else if (row_len == 135) {
        LGR_TRY(lgr_match_rops_dev(ctx, d_q, mq, d_t, mt, mt, d_idx, d_dist));
        flann_dist_rows_kernel<135><<<cdiv(mq, 128), 128, 0, ctx->stream>>>(d_q, d_t, d_idx, mq, d_dist);
    } else {
        LGR_TRY(lgr_match_shot_dev(ctx, d_q, mq, d_t, mt, mt, d_idx, d_dist));
        flann_dist_rows_kernel<352><<<cdiv(mq, 128), 128, 0, ctx->stream>>>(d_q, d_t, d_idx, mq, d_dist);
    }
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

extern "C" int lgr_match_local_knn(lgr_ctx* ctx, int row_len, const float* qpts, int mq, const float* tpts, int mt, const float* q, const float* t,
                                   const float guess16[16], float radius, int k, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, k >= 1 && k <= KMAX && row_len_built(row_len), LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, mq >= 0 && mt >= 0 && (qpts || mq == 0) && (tpts || mt == 0) && (q || mq == 0) && (t || mt == 0) && (idx || mq == 0) && (dist || mq == 0) &&
                   guess16 && radius >= 0.f, LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    float *dqp, *dtp, *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q, (size_t) mq * row_len, &dq));
    LGR_TRY(hc.in(t, (size_t) mt * row_len, &dt));
    LGR_TRY(hc.in(qpts, (size_t) mq * 12, &dqp));
    LGR_TRY(hc.in(tpts, (size_t) mt * 12, &dtp));
    LGR_TRY(hc.out((size_t) mq * k, &di));
    LGR_TRY(hc.out((size_t) mq * k, &dd));
    LGR_TRY(lgr_match_local_knn_dev(ctx, row_len, dqp, mq, dtp, mt, dq, dt, guess16, radius, k, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq * k));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq * k));
    return hc.finish();
}

extern "C" int lgr_match_flann_rows(lgr_ctx* ctx, int row_len, const float* q, int mq, const float* t, int mt, int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, row_len_built(row_len), LGR_ERR_UNSUPPORTED);
    LGR_CHECK(ctx, mq >= 0 && mt >= 0 && (q || mq == 0) && (t || mt == 0) && (idx || mq == 0) && (dist || mq == 0), LGR_ERR_INVALID_ARG);
    if (mq == 0) return LGR_OK;
    float *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q, (size_t) mq * row_len, &dq));
    LGR_TRY(hc.in(t, (size_t) mt * row_len, &dt));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_match_flann_rows_dev(ctx, row_len, dq, mq, dt, mt, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}
