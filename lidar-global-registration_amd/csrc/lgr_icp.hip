// lgr_icp.hip -- ICP on the device for gfx950: lgr_icp_ex* (point-to-plane, point-to-point, plane-to-plane, robust kernels, the normal
// gate, point weights) and lgr_icp_plane*, its neutral configuration (include/lgr.h).  A statement of this library's own: DESIGN.md
// section 4, "Point-to-plane ICP" and "ICP variants"; the CPU statements are tests/cpp/icp_ref.cpp (the plain algorithm, on its own) and
// tests/cpp/icp_ex_ref.cpp; the step's f64 arithmetic is lgr_icp_math.h for all of them.
//
// Set-up, once per call: max_dist (the caller's, or 4 x the target's density), ONE grid over the target with cell 1.001 x max_dist, the
// centre of the target's bounding box.  An iteration, all on the stream:
//   icp_terms_kernel   <VARIANT, ROBUST, GATE, WEIGHTS>, one of 48 picked per call.  A source point per lane: plane_move by S.T,
//                      nearest_within(d_k^2), the pair's values, then the 28 f64 terms, each product formed immediately before its own
//                      wave butterfly; LDS tree over the four waves -> one partial per term and workgroup (and the workgroup's pair
//                      count).  Live across the 28 butterflies: one row (point-to-plane) W g, g and r (13 doubles; W g is g where W is
//                      the constant 1); three rows u, M j_b (mj: 18 doubles, of which the last nine are M's own entries), M e and W.
//   icp_tree_kernel    256 partials -> 1, level by level, until one is left (none up to 256 points, one up to 65 536, two beyond)
//   icp_step_kernel    the solve, T_{k+1}, d_{k+1}, the stop decision and the trace record (icp_step, lgr_icp_math.h)
// The tree.  The statement sums x[0, ns) padded with +0.0 to 2^m by S(lo, len) = S(lo, len / 2) + S(lo + len / 2, len / 2).  An xor
// butterfly with offsets 1, 2, 4, ... leaves in lane 0 exactly that tree over the wave's 64 contiguous indices (lane 0 always adds
// "its own + the higher half"), the LDS stage is (w0 + w1) + (w2 + w3), and a level of icp_tree_kernel is the same over 256 partials, so
// the kernels compute S(0, 256^levels).  Indices in [ns, 2^m) hold +0.0 as the statement says; indices from 2^m on hold -0.0, the additive
// identity (x + -0.0 == x for every x, -0.0 and +0.0 included): S(0, 256^levels) == S(0, 2^m) bit for bit, also where a sum is a zero.
// No float atomics, no sequential chain; the pair count is an integer sum.
// Iterations are enqueued blind in groups of LGR_ICP_GROUP with one read-back of S per group; once S.done is set every kernel of a later
// iteration returns at once and S and the trace stay as they are.
// lgr_icp_trim* (trimmed ICP, median-scaled robust kernels) and lgr_rank_select* are further down: the same loop with the terms kernel split
// around an exact rank select of the pairs' residuals (lgr_rank_select.cuh).
#include <algorithm>
#include <cfloat>

#include "lgr_grid.cuh"
#include "lgr_host.h"
#include "lgr_icp_math.h"
#include "lgr_internal.h"
#include "lgr_math.cuh"
#include "lgr_plane_point.cuh"
#include "lgr_pointpass.cuh"
#include "lgr_rank_select.cuh"

namespace {

constexpr int ICP_BLOCK = 256, ICP_WAVES = ICP_BLOCK / 64, ICP_SLOTS = ICP_TERMS + 1;   // slot 28: the pair count (long long)

struct IcpState {
    float T[16];          // T_k: T0 (uploaded), then each step's
    float d;              // d_k of the iteration about to run
    int k;                // steps taken == index of the iteration about to run
    int stop, done;       // LGR_ICP_STOP_*, the loop has ended
    int n_eval;           // iterations evaluated == trace entries written
    int pairs, pairs0;    // of the last evaluated iteration, of iteration 0
    float rmse, rmse0;
    int pad[7];
};
static_assert(sizeof(IcpState) == 128, "IcpState is copied and cleared in one piece");

struct IcpConst { float cx, cy, cz, min_dist, shrink, rot_eps, trans_eps; int max_iterations; };

// S(lo, 64) over the wave's lanes, valid in lane 0
__device__ __forceinline__ double icp_wave_tree(double x) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) x = x + __shfl_xor(x, o);
    return x;
}

// the four waves' values of one slot -> S(lo, 256)
__device__ __forceinline__ double icp_block_tree(const double (*sh)[ICP_SLOTS], int t) { return (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]); }

// what the options of lgr_icp_ex_params add to a point's contribution ("ICP variants")
struct IcpEx {
    double k;         // the robust scale
    double cos_min;   // the gate's cosine
    double s;         // 1 - eps of plane-to-plane
    const float* w;   // the point weights
};

// j_a . v for the columns of J = [-[u]x | I]: the two products of a rotational column, the entry itself of a translational one
__device__ __forceinline__ double icp_jdot(int a, const double* v, double ux, double uy, double uz) {
    return a == 0 ? v[2] * uy - v[1] * uz : a == 1 ? v[0] * uz - v[2] * ux : a == 2 ? v[1] * ux - v[0] * uy : v[a - 3];
}

// part: [ICP_SLOTS][stride] 8-byte words, slot-major; this workgroup writes column blockIdx.x.  pad_n = 2^m.  A parameter that is off
// costs nothing: no weight load, no source normal load, no sqrt, and W is the constant 1 (x * 1 == x: the plain algorithm's bits).
template <int VARIANT, int ROBUST, bool GATE, bool WEIGHTS>
__global__ __launch_bounds__(ICP_BLOCK) void icp_terms_kernel(GridDev g, const float4* __restrict__ src, int ns, long long pad_n, const IcpState* __restrict__ S, float cx,
                                                              float cy, float cz, IcpEx X, double* __restrict__ part, size_t stride) {
    if (S->done) return;
    constexpr bool ONE_ROW = VARIANT == ICP_POINT_TO_PLANE, NEED_M = GATE || VARIANT == ICP_PLANE_TO_PLANE, NEED_N = ONE_ROW || NEED_M;
    __shared__ double sh[ICP_WAVES][ICP_SLOTS];
    const long long i = (long long) blockIdx.x * ICP_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float d = S->d;
    bool has = false;
    double W = 1.0, ux = 0, uy = 0, uz = 0, r = 0, rr = 0;
    double gv[6] = {0, 0, 0, 0, 0, 0}, wg[6] = {0, 0, 0, 0, 0, 0};   // one row: g, W g
    double mj[6][3] = {}, me[3] = {0, 0, 0};                         // three rows: M j_b, M e
    if (i < ns) {
        const float4 P = src[(size_t) i * 3];
        float px, py, pz, d2;
        int j;
        plane_move(S->T, P.x, P.y, P.z, px, py, pz);
        const int t = nearest_within(g, px, py, pz, d * d, d2, j);   // (a non-finite moved point walks nothing: -1)
        bool ok = t >= 0;
        double om = 1.0;
        if (WEIGHTS && ok) {
            om = (double) X.w[i];
            ok = icp_finite(om) && om > 0.0;
        }
        double nx = 0, ny = 0, nz = 0, mx = 0, my = 0, mz = 0;
        if (NEED_N && ok) {
            const float4 N = g.pnrm[t];   // the grid's copy of tgt[j]'s normal: the same bits
            ok = lgr_finite3(N.x, N.y, N.z);
            nx = (double) N.x; ny = (double) N.y; nz = (double) N.z;
        }
        if (NEED_M && ok) {
            const float4 Ns = src[(size_t) i * 3 + 1];
            const float* T = S->T;
            ok = lgr_finite3(Ns.x, Ns.y, Ns.z);
            const double sx = (double) Ns.x, sy = (double) Ns.y, sz = (double) Ns.z;
            mx = ((double) T[0] * sx + (double) T[4] * sy) + (double) T[8] * sz;
            my = ((double) T[1] * sx + (double) T[5] * sy) + (double) T[9] * sz;
            mz = ((double) T[2] * sx + (double) T[6] * sy) + (double) T[10] * sz;
            if (GATE) ok = ok && (mx * nx + my * ny) + mz * nz >= X.cos_min;
        }
        if (ok) {
            const float4 Q = g.pxyz[t];
            ux = (double) px - (double) cx; uy = (double) py - (double) cy; uz = (double) pz - (double) cz;
            const double ex = (double) px - (double) Q.x, ey = (double) py - (double) Q.y, ez = (double) pz - (double) Q.z;
            double rho;
            if (ONE_ROW) {
                r = (nx * ex + ny * ey) + nz * ez;
                rr = r * r;
                rho = __builtin_fabs(r);
                gv[0] = uy * nz - uz * ny;
                gv[1] = uz * nx - ux * nz;
                gv[2] = ux * ny - uy * nx;
                gv[3] = nx; gv[4] = ny; gv[5] = nz;
            } else {
                double M[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};   // (xx, xy, xz, yy, yz, zz); point-to-point: I through the same expressions
                if (VARIANT == ICP_PLANE_TO_PLANE) {
                    const double s = X.s;
                    const double Sg[6] = {2.0 - s * (nx * nx + mx * mx), -(s * (nx * ny + mx * my)), -(s * (nx * nz + mx * mz)),
                                          2.0 - s * (ny * ny + my * my), -(s * (ny * nz + my * mz)), 2.0 - s * (nz * nz + mz * mz)};
                    ok = icp_inv_sym3(Sg, M);
                }
                const double Mr[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    mj[0][q] = Mr[q][2] * uy - Mr[q][1] * uz;
                    mj[1][q] = Mr[q][0] * uz - Mr[q][2] * ux;
                    mj[2][q] = Mr[q][1] * ux - Mr[q][0] * uy;
                    mj[3][q] = Mr[q][0]; mj[4][q] = Mr[q][1]; mj[5][q] = Mr[q][2];
                    me[q] = (Mr[q][0] * ex + Mr[q][1] * ey) + Mr[q][2] * ez;
                }
                rr = (ex * me[0] + ey * me[1]) + ez * me[2];
                rho = ROBUST != ICP_ROBUST_NONE ? __builtin_sqrt(rr) : 0.0;
            }
            if (ROBUST != ICP_ROBUST_NONE || WEIGHTS) {
                W = icp_robust_weight(ROBUST, rho, X.k) * om;
                ok = ok && W > 0.0;
            }
            if (ONE_ROW) {
#pragma unroll
                for (int a = 0; a < 6; ++a) wg[a] = W * gv[a];
            }
            has = ok;
        }
    }
    const double fill = i < pad_n ? 0.0 : -0.0;   // the statement's padding / the identity behind it
    int slot = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b, ++slot) {
            const double x = ONE_ROW ? wg[a] * gv[b] : W * icp_jdot(a, mj[b], ux, uy, uz);
            const double s = icp_wave_tree(has ? x : fill);
            if (lane == 0) sh[wave][slot] = s;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a, ++slot) {
        const double x = ONE_ROW ? wg[a] * r : W * icp_jdot(a, me, ux, uy, uz);
        const double s = icp_wave_tree(has ? x : fill);
        if (lane == 0) sh[wave][slot] = s;
    }
    {
        const double s = icp_wave_tree(has ? rr : fill);
        if (lane == 0) sh[wave][ICP_TERMS - 1] = s;
    }
    const long long cnt = __popcll(__ballot(has));
    if (lane == 0) sh[wave][ICP_TERMS] = __longlong_as_double(cnt);
    __syncthreads();
    if (threadIdx.x < ICP_TERMS) part[threadIdx.x * stride + blockIdx.x] = icp_block_tree(sh, threadIdx.x);
    else if (threadIdx.x == ICP_TERMS) {
        long long c = 0;
#pragma unroll
        for (int w = 0; w < ICP_WAVES; ++w) c += __double_as_longlong(sh[w][ICP_TERMS]);
        part[ICP_TERMS * stride + blockIdx.x] = __longlong_as_double(c);
    }
}

using IcpTermsFn = void (*)(GridDev, const float4*, int, long long, const IcpState*, float, float, float, IcpEx, double*, size_t);

template <int V, int R>
IcpTermsFn icp_pick2(bool gate, bool w) {
    return gate ? (w ? icp_terms_kernel<V, R, true, true> : icp_terms_kernel<V, R, true, false>)
                : (w ? icp_terms_kernel<V, R, false, true> : icp_terms_kernel<V, R, false, false>);
}
template <int V>
IcpTermsFn icp_pick1(int robust, bool gate, bool w) {
    switch (robust) {
        case ICP_ROBUST_HUBER: return icp_pick2<V, ICP_ROBUST_HUBER>(gate, w);
        case ICP_ROBUST_CAUCHY: return icp_pick2<V, ICP_ROBUST_CAUCHY>(gate, w);
        case ICP_ROBUST_TUKEY: return icp_pick2<V, ICP_ROBUST_TUKEY>(gate, w);
        default: return icp_pick2<V, ICP_ROBUST_NONE>(gate, w);
    }
}
IcpTermsFn icp_pick(int variant, int robust, bool gate, bool w) {
    switch (variant) {
        case ICP_POINT_TO_POINT: return icp_pick1<ICP_POINT_TO_POINT>(robust, gate, w);
        case ICP_PLANE_TO_PLANE: return icp_pick1<ICP_PLANE_TO_PLANE>(robust, gate, w);
        default: return icp_pick1<ICP_POINT_TO_PLANE>(robust, gate, w);
    }
}

// one level of the tree: entries [256 b, 256 b + 256) of slot blockIdx.y -> entry b.  Entries from n_in on are +0.0 below pad_in
// (= 2^m / 256^level: workgroups the statement's padding would have filled) and -0.0 from there.
__global__ __launch_bounds__(ICP_BLOCK) void icp_tree_kernel(const IcpState* __restrict__ S, const double* __restrict__ in, size_t stride_in, long long n_in, long long pad_in,
                                                             double* __restrict__ out, size_t stride_out) {
    if (S->done) return;
    __shared__ double sh[ICP_WAVES];
    const int slot = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long j = (long long) blockIdx.x * ICP_BLOCK + threadIdx.x;
    const double* col = in + slot * stride_in;
    if (slot == ICP_TERMS) {   // the pair count (the branch is uniform over the workgroup)
        long long c = j < n_in ? __double_as_longlong(col[j]) : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) c += __shfl_xor(c, o);
        if (lane == 0) sh[wave] = __longlong_as_double(c);
        __syncthreads();
        if (threadIdx.x == 0) {
            long long t = 0;
#pragma unroll
            for (int w = 0; w < ICP_WAVES; ++w) t += __double_as_longlong(sh[w]);
            out[slot * stride_out + blockIdx.x] = __longlong_as_double(t);
        }
        return;
    }
    const double x = j < n_in ? col[j] : (j < pad_in ? 0.0 : -0.0);
    const double s = icp_wave_tree(x);
    if (lane == 0) sh[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[slot * stride_out + blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one wave, one working lane: the iteration's decision from its sums (entry 0 of every slot of `fin`)
__global__ __launch_bounds__(64) void icp_step_kernel(IcpState* __restrict__ S, const double* __restrict__ fin, size_t stride, IcpConst K, lgr_icp_step* __restrict__ trace) {
    if (threadIdx.x != 0 || S->done) return;
    double s[ICP_TERMS];
#pragma unroll
    for (int t = 0; t < ICP_TERMS; ++t) s[t] = fin[t * stride];
    const long long pairs = __double_as_longlong(fin[ICP_TERMS * stride]);
    const int k = S->k;
    const float c[3] = {K.cx, K.cy, K.cz};
    float T[16], Tn[16], rot, trans;
#pragma unroll
    for (int e = 0; e < 16; ++e) T[e] = S->T[e];
    bool stepped;
    const int stop = icp_step(s, pairs, c, T, k, K.max_iterations, K.rot_eps, K.trans_eps, Tn, &stepped, &rot, &trans);
    const float rmse = icp_rmse(s[ICP_TERMS - 1], pairs);
    lgr_icp_step rec;
#pragma unroll
    for (int e = 0; e < 16; ++e) rec.transformation[e] = T[e];
    rec.dist = S->d; rec.pairs = (int) pairs; rec.rmse = rmse; rec.rot = rot; rec.trans = trans;
    rec.reserved[0] = rec.reserved[1] = rec.reserved[2] = 0;
    trace[k] = rec;   // k < max_iterations: iteration max_iterations - 1 always sets done
    S->n_eval = k + 1;
    S->pairs = (int) pairs; S->rmse = rmse;
    if (k == 0) { S->pairs0 = (int) pairs; S->rmse0 = rmse; }
    if (stepped) {
#pragma unroll
        for (int e = 0; e < 16; ++e) S->T[e] = Tn[e];
        S->k = k + 1;
    }
    if (stop >= 0) { S->stop = stop; S->done = 1; }
    else S->d = icp_next_dist(S->d, K.shrink, K.min_dist);
}

// ---- trimmed ICP (lgr_icp_trim*; DESIGN.md section 3.1q and section 4, "Trimmed ICP").  The iteration's terms kernel is replaced by
//   icp_pair_kernel        <VARIANT>: the search and the candidate test, once; stores the pair (grid slot t, p', rho, the key's bits)
//   sel_hist_kernel x passes, sel_finish_kernel   (lgr_rank_select.cuh): P, the composite at rank K - 1 and at the median rank
//   icp_trim_terms_kernel  <VARIANT>: the kept candidates' 28 terms from the stored pair, W from k_it; the iteration's info record
// and feeds the same icp_tree_kernel / icp_step_kernel.  icp_terms_kernel and the path of lgr_icp_ex* are untouched: the per-point
// values are written here a second time (icp_point_values), with the gate and the weights as run-time switches.

struct IcpPairs {
    float4* p;        // p' (w unused)
    double* rho;
    int* t;           // the neighbour's slot in the grid's copies; -1: no candidate
    uint32_t* key;    // (float) rho as bits; 0xffffffff: no candidate (the select skips it)
};

struct IcpTrim { int robust; bool gate; float keep, scale_from_median, robust_scale; };

struct IcpValues {
    double om, rho, ux, uy, uz, r, rr;
    double gv[6];             // one row: g
    double mj[6][3], me[3];   // three rows: M j_b, M e
};

// the values of source point i moved to p', paired with grid slot t, before any robust weight; false: no pair (steps 2 - 5 of the variants)
template <int VARIANT>
__device__ __forceinline__ bool icp_point_values(const GridDev& g, const float4* __restrict__ src, long long i, const float* __restrict__ T, float px, float py, float pz, int t,
                                                 float cx, float cy, float cz, const IcpEx& X, bool gate, IcpValues& v) {
    constexpr bool ONE_ROW = VARIANT == ICP_POINT_TO_PLANE;
    const bool need_m = gate || VARIANT == ICP_PLANE_TO_PLANE, need_n = ONE_ROW || need_m;
    v.om = 1.0;
    if (X.w) {
        v.om = (double) X.w[i];
        if (!(icp_finite(v.om) && v.om > 0.0)) return false;
    }
    double nx = 0, ny = 0, nz = 0, mx = 0, my = 0, mz = 0;
    if (need_n) {
        const float4 N = g.pnrm[t];
        if (!lgr_finite3(N.x, N.y, N.z)) return false;
        nx = (double) N.x; ny = (double) N.y; nz = (double) N.z;
    }
    if (need_m) {
        const float4 Ns = src[(size_t) i * 3 + 1];
        if (!lgr_finite3(Ns.x, Ns.y, Ns.z)) return false;
        const double sx = (double) Ns.x, sy = (double) Ns.y, sz = (double) Ns.z;
        mx = ((double) T[0] * sx + (double) T[4] * sy) + (double) T[8] * sz;
        my = ((double) T[1] * sx + (double) T[5] * sy) + (double) T[9] * sz;
        mz = ((double) T[2] * sx + (double) T[6] * sy) + (double) T[10] * sz;
        if (gate && !((mx * nx + my * ny) + mz * nz >= X.cos_min)) return false;
    }
    const float4 Q = g.pxyz[t];
    const double ux = (double) px - (double) cx, uy = (double) py - (double) cy, uz = (double) pz - (double) cz;
    const double ex = (double) px - (double) Q.x, ey = (double) py - (double) Q.y, ez = (double) pz - (double) Q.z;
    v.ux = ux; v.uy = uy; v.uz = uz;
    if (ONE_ROW) {
        v.r = (nx * ex + ny * ey) + nz * ez;
        v.rr = v.r * v.r;
        v.rho = __builtin_fabs(v.r);
        v.gv[0] = uy * nz - uz * ny;
        v.gv[1] = uz * nx - ux * nz;
        v.gv[2] = ux * ny - uy * nx;
        v.gv[3] = nx; v.gv[4] = ny; v.gv[5] = nz;
        return true;
    }
    double M[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
    if (VARIANT == ICP_PLANE_TO_PLANE) {
        const double s = X.s;
        const double Sg[6] = {2.0 - s * (nx * nx + mx * mx), -(s * (nx * ny + mx * my)), -(s * (nx * nz + mx * mz)),
                              2.0 - s * (ny * ny + my * my), -(s * (ny * nz + my * mz)), 2.0 - s * (nz * nz + mz * mz)};
        if (!icp_inv_sym3(Sg, M)) return false;
    }
    const double Mr[3][3] = {{M[0], M[1], M[2]}, {M[1], M[3], M[4]}, {M[2], M[4], M[5]}};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        v.mj[0][q] = Mr[q][2] * uy - Mr[q][1] * uz;
        v.mj[1][q] = Mr[q][0] * uz - Mr[q][2] * ux;
        v.mj[2][q] = Mr[q][1] * ux - Mr[q][0] * uy;
        v.mj[3][q] = Mr[q][0]; v.mj[4][q] = Mr[q][1]; v.mj[5][q] = Mr[q][2];
        v.me[q] = (Mr[q][0] * ex + Mr[q][1] * ey) + Mr[q][2] * ez;
    }
    v.rr = (ex * v.me[0] + ey * v.me[1]) + ez * v.me[2];
    v.rho = __builtin_sqrt(v.rr);
    return true;
}

template <int VARIANT>
__global__ __launch_bounds__(ICP_BLOCK) void icp_pair_kernel(GridDev g, const float4* __restrict__ src, int ns, const IcpState* __restrict__ S, float cx, float cy, float cz,
                                                             IcpEx X, bool gate, IcpPairs Pr) {
    if (S->done) return;
    const long long i = (long long) blockIdx.x * ICP_BLOCK + threadIdx.x;
    if (i >= ns) return;
    const float4 P = src[(size_t) i * 3];
    const float d = S->d;
    float px, py, pz, d2;
    int j;
    plane_move(S->T, P.x, P.y, P.z, px, py, pz);
    const int t = nearest_within(g, px, py, pz, d * d, d2, j);
    IcpValues v;
    v.rho = 0.0;
    uint32_t bits = 0xffffffffu;
    const bool ok = t >= 0 && icp_point_values<VARIANT>(g, src, i, S->T, px, py, pz, t, cx, cy, cz, X, gate, v) && icp_trim_key(v.rho, &bits);
    Pr.p[i] = make_float4(px, py, pz, 0.f);
    Pr.rho[i] = v.rho;
    Pr.t[i] = ok ? t : -1;
    Pr.key[i] = ok ? bits : 0xffffffffu;
}

// icp_terms_kernel's second half over the stored pairs: a candidate at or below the cut contributes with W = w(rho, k_it) omega
template <int VARIANT>
__global__ __launch_bounds__(ICP_BLOCK) void icp_trim_terms_kernel(GridDev g, const float4* __restrict__ src, int ns, long long pad_n, const IcpState* __restrict__ S, float cx,
                                                                   float cy, float cz, IcpEx X, IcpTrim A, IcpPairs Pr, const SelWork* __restrict__ sel,
                                                                   lgr_icp_trim_step* __restrict__ info, double* __restrict__ part, size_t stride) {
    if (S->done) return;
    constexpr bool ONE_ROW = VARIANT == ICP_POINT_TO_PLANE;
    __shared__ double sh[ICP_WAVES][ICP_SLOTS];
    const long long i = (long long) blockIdx.x * ICP_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const SelState* res = &sel->st[SEL_MAX_PASSES];
    const long long P = res->P, K = icp_trim_k(A.keep, P);
    const unsigned long long cut = res->prefix[0];
    const float key_m = res->ok[1] ? icp_trim_key_value((uint32_t) (res->prefix[1] >> 32)) : 0.f;
    const double k_it = icp_trim_scale(A.scale_from_median, key_m, A.robust_scale);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        lgr_icp_trim_step rec;
        rec.candidates = (int) P; rec.kept = (int) K;
        rec.cut = K > 0 ? icp_trim_key_value((uint32_t) (cut >> 32)) : 0.f;
        rec.scale = A.robust == ICP_ROBUST_NONE ? 0.f : (float) k_it;
        info[S->k] = rec;   // k < max_iterations, as the trace
    }
    bool has = false;
    double W = 1.0;
    IcpValues v;
    v.ux = v.uy = v.uz = v.r = v.rr = 0.0;
    double wg[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        v.gv[a] = 0.0;
        v.mj[a][0] = v.mj[a][1] = v.mj[a][2] = 0.0;
    }
    v.me[0] = v.me[1] = v.me[2] = 0.0;
    if (i < ns) {
        const int t = Pr.t[i];
        if (t >= 0 && K > 0 && res->ok[0] && icp_trim_composite(Pr.key[i], (uint32_t) i) <= cut) {
            const float4 p = Pr.p[i];
            bool ok = icp_point_values<VARIANT>(g, src, i, S->T, p.x, p.y, p.z, t, cx, cy, cz, X, A.gate, v);   // (true again: the same inputs)
            W = icp_trim_weight(A.robust, Pr.rho[i], k_it) * v.om;
            ok = ok && W > 0.0;
            if (ONE_ROW) {
#pragma unroll
                for (int a = 0; a < 6; ++a) wg[a] = W * v.gv[a];
            }
            has = ok;
        }
    }
    const double fill = i < pad_n ? 0.0 : -0.0;
    int slot = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b, ++slot) {
            const double x = ONE_ROW ? wg[a] * v.gv[b] : W * icp_jdot(a, v.mj[b], v.ux, v.uy, v.uz);
            const double s = icp_wave_tree(has ? x : fill);
            if (lane == 0) sh[wave][slot] = s;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a, ++slot) {
        const double x = ONE_ROW ? wg[a] * v.r : W * icp_jdot(a, v.me, v.ux, v.uy, v.uz);
        const double s = icp_wave_tree(has ? x : fill);
        if (lane == 0) sh[wave][slot] = s;
    }
    {
        const double s = icp_wave_tree(has ? v.rr : fill);
        if (lane == 0) sh[wave][ICP_TERMS - 1] = s;
    }
    const long long cnt = __popcll(__ballot(has));
    if (lane == 0) sh[wave][ICP_TERMS] = __longlong_as_double(cnt);
    __syncthreads();
    if (threadIdx.x < ICP_TERMS) part[threadIdx.x * stride + blockIdx.x] = icp_block_tree(sh, threadIdx.x);
    else if (threadIdx.x == ICP_TERMS) {
        long long c = 0;
#pragma unroll
        for (int w = 0; w < ICP_WAVES; ++w) c += __double_as_longlong(sh[w][ICP_TERMS]);
        part[ICP_TERMS * stride + blockIdx.x] = __longlong_as_double(c);
    }
}

using IcpPairFn = void (*)(GridDev, const float4*, int, const IcpState*, float, float, float, IcpEx, bool, IcpPairs);
using IcpTrimTermsFn = void (*)(GridDev, const float4*, int, long long, const IcpState*, float, float, float, IcpEx, IcpTrim, IcpPairs, const SelWork*, lgr_icp_trim_step*,
                                double*, size_t);

IcpPairFn icp_pick_pair(int variant) {
    return variant == ICP_POINT_TO_POINT ? icp_pair_kernel<ICP_POINT_TO_POINT> : variant == ICP_PLANE_TO_PLANE ? icp_pair_kernel<ICP_PLANE_TO_PLANE> : icp_pair_kernel<ICP_POINT_TO_PLANE>;
}
IcpTrimTermsFn icp_pick_trim_terms(int variant) {
    return variant == ICP_POINT_TO_POINT   ? icp_trim_terms_kernel<ICP_POINT_TO_POINT>
           : variant == ICP_PLANE_TO_PLANE ? icp_trim_terms_kernel<ICP_PLANE_TO_PLANE>
                                           : icp_trim_terms_kernel<ICP_POINT_TO_PLANE>;
}

// what icp_run needs to run the trimmed iteration in place of `terms`
struct IcpTrimRun { int variant; IcpTrim A; lgr_icp_trim_step* info; };

void fill_result(const IcpState& s, float max_dist, lgr_icp_result* out) {
    memset(out, 0, sizeof *out);
    memcpy(out->transformation, s.T, 64);
    out->iterations = s.k; out->stop = s.stop; out->max_dist = max_dist;
    out->pairs = s.pairs; out->rmse = s.rmse; out->pairs0 = s.pairs0; out->rmse0 = s.rmse0;
}

bool dist_ok(float d) { return d == d && fabsf(d) <= 1e18f; }   // finite, and its square stays finite

bool params_ok(const lgr_icp_params* p) {
    if (!p || p->max_iterations < 0 || p->max_iterations > LGR_ICP_MAX_ITERATIONS) return false;
    for (int r : p->reserved)
        if (r) return false;
    return dist_ok(p->max_dist) && dist_ok(p->min_dist) && p->shrink > 0.f && p->shrink <= 1.f && p->rot_eps >= 0.f && p->trans_eps >= 0.f;
}

bool ex_params_ok(const lgr_icp_ex_params* p) {
    if (!p || !params_ok(&p->base)) return false;
    if (p->variant < LGR_ICP_POINT_TO_PLANE || p->variant > LGR_ICP_PLANE_TO_PLANE || p->robust < LGR_ICP_ROBUST_NONE || p->robust > LGR_ICP_ROBUST_TUKEY) return false;
    for (int r : p->reserved)
        if (r) return false;
    if (p->robust != LGR_ICP_ROBUST_NONE && !(p->robust_scale > 0.f && p->robust_scale <= FLT_MAX)) return false;
    if (!(p->min_normal_cos >= -1.f && p->min_normal_cos <= 1.f)) return false;
    return p->plane_eps == 0.f || (p->plane_eps >= 1e-6f && p->plane_eps <= 1.f);
}

// nothing to evaluate (an empty source, no iteration allowed): T0 comes back
void idle_result(const float* T0, const lgr_icp_params* p, int stop, lgr_icp_result* out, int* n_trace) {
    IcpState s{};
    memcpy(s.T, T0, 64);
    s.stop = stop;
    s.rmse = s.rmse0 = FLT_MAX;
    fill_result(s, p->max_dist > 0.f ? p->max_dist : 0.f, out);
    if (n_trace) *n_trace = 0;
}

// The loop behind lgr_icp_ex_dev, the arguments checked by the caller: the set-up, then the iterations in groups.  `terms` is the call's
// instantiation of icp_terms_kernel, enqueued over ceil(ns / 256) workgroups with the options X.  With `trim` (lgr_icp_trim_dev) the pair
// kernel, the select and the trimmed terms kernel stand in its place, and n_trace counts the entries of the trace and of trim->info.
int icp_run(lgr_ctx* ctx, IcpTermsFn terms, const IcpEx& X, const float* d_src, int ns, const float* d_tgt, int nt, const float T0[16], const lgr_icp_params* p,
            lgr_icp_result* out, lgr_icp_step* trace, int* n_trace, const IcpTrimRun* trim = nullptr) {
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const int max_it = p->max_iterations;
    if (ns == 0 || max_it == 0) {
        idle_result(T0, p, ns == 0 ? LGR_ICP_STOP_NO_PAIRS : LGR_ICP_STOP_MAX_ITERATIONS, out, n_trace);
        return LGR_OK;
    }
    // ---- set-up: the distances, the grid, the centre, the buffers (every synchronisation that is not a group's read-back happens here)
    float max_dist = p->max_dist;
    if (!(max_dist > 0.f)) {
        float density;
        LGR_TRY(lgr_cloud_density_dev(ctx, d_tgt, nt, 0.8f, &density));
        max_dist = 4.f * density;
    }
    const float min_dist = p->min_dist > 0.f ? p->min_dist : max_dist;
    LGR_CHECK(ctx, max_dist > 0.f && dist_ok(max_dist) && min_dist <= max_dist, LGR_ERR_INVALID_ARG);
    lgr_plane_target pt;   // (its radius is 2 x the threshold it is given: the cell is 1.001 x max_dist, and no d_k exceeds max_dist)
    LGR_TRY(lgr_plane_target_setup(ctx, d_tgt, nt, max_dist * 0.5f, 1e18f, &pt));
    LGR_CHECK(ctx, pt.radius == max_dist, LGR_ERR_INVALID_ARG);   // (a max_dist whose half is not representable)
    const GridDev& g = pt.g;
    float bb[12];
    LGR_TRY(lgr_bbox_host(ctx, d_tgt, nt, bb));
    IcpConst K{};
    float* c3 = &K.cx;
    for (int a = 0; a < 3; ++a) {
        c3[a] = (bb[a] + bb[3 + a]) * 0.5f;
        if (!(fabsf(c3[a]) <= FLT_MAX)) c3[a] = 0.f;   // no finite target point, or a box whose centre overflows
    }
    K.min_dist = min_dist; K.shrink = p->shrink; K.rot_eps = p->rot_eps; K.trans_eps = p->trans_eps; K.max_iterations = max_it;
    // the levels: nb[0] workgroups of points, then 256 -> 1 until one entry is left
    long long pad_n = 1;
    while (pad_n < ns) pad_n <<= 1;
    size_t nb[5], off[5], words = 0;
    int levels = 0;
    for (size_t n = (size_t) ns;;) {
        n = cdivz(n, ICP_BLOCK);
        nb[levels] = n; off[levels] = words;
        words += ICP_SLOTS * n;
        ++levels;
        if (n == 1) break;
    }
    IcpState* S;
    double* part;
    lgr_icp_step* d_trace;
    char* h;
    LGR_TRY(lgr_ws_t(ctx, WS_ICP_STATE, 1, &S));
    LGR_TRY(lgr_ws_t(ctx, WS_ICP_PART, words, &part));
    LGR_TRY(lgr_ws_t(ctx, WS_ICP_TRACE, (size_t) max_it, &d_trace));
    IcpPairs Pr{};
    SelWork* sel = nullptr;
    lgr_icp_trim_step* d_info = nullptr;
    IcpPairFn pair_fn = nullptr;
    IcpTrimTermsFn trim_terms = nullptr;
    if (trim) {
        char* pw;
        LGR_TRY(lgr_ws_t(ctx, WS_ICP_PAIR, (size_t) ns * 32, &pw));   // 16 + 8 + 4 + 4 bytes a point, the widest first
        Pr.p = (float4*) pw;
        Pr.rho = (double*) (pw + (size_t) ns * 16);
        Pr.t = (int*) (pw + (size_t) ns * 24);
        Pr.key = (uint32_t*) (pw + (size_t) ns * 28);
        LGR_TRY(lgr_ws_t(ctx, WS_ICP_SEL, 1, &sel));
        LGR_TRY(lgr_ws_t(ctx, WS_ICP_INFO, (size_t) max_it, &d_info));
        LGR_HIP(ctx, hipMemsetAsync(sel, 0, sizeof(SelWork), ctx->stream));
        pair_fn = icp_pick_pair(trim->variant);
        trim_terms = icp_pick_trim_terms(trim->variant);
    }
    const SelRanks ranks{1, trim ? trim->A.keep : 1.f, {0, 0}};
    const size_t h_trace_off = (sizeof(IcpState) + 63) & ~(size_t) 63;
    LGR_TRY(lgr_pinned(ctx, h_trace_off + (size_t) max_it * sizeof(lgr_icp_step), (void**) &h));
    IcpState hs{};
    memcpy(hs.T, T0, 64);
    hs.d = max_dist;
    hs.rmse = hs.rmse0 = FLT_MAX;
    memcpy(h, &hs, sizeof hs);   // (pinned: the upload reads it in stream order, ahead of the first read-back that overwrites it)
    LGR_HIP(ctx, hipMemcpyAsync(S, h, sizeof(IcpState), hipMemcpyHostToDevice, ctx->stream));
    // ---- the iterations, LGR_ICP_GROUP at a time; nothing of an iteration passes through the host
    int enqueued = 0;
    for (;;) {
        const int group = std::min((int) LGR_ICP_GROUP, max_it - enqueued);
        for (int k = 0; k < group; ++k) {
            if (trim) {
                pair_fn<<<(unsigned) nb[0], ICP_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_src, ns, S, K.cx, K.cy, K.cz, X, trim->A.gate, Pr);
                sel_enqueue(ctx->stream, &S->done, Pr.key, nullptr, ns, ranks, sel);
                trim_terms<<<(unsigned) nb[0], ICP_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_src, ns, pad_n, S, K.cx, K.cy, K.cz, X, trim->A, Pr, sel, d_info, part,
                                                                             nb[0]);
            } else
                terms<<<(unsigned) nb[0], ICP_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_src, ns, pad_n, S, K.cx, K.cy, K.cz, X, part, nb[0]);
            long long pad = pad_n;
            for (int l = 1; l < levels; ++l) {
                pad >>= 8;   // >= 2 wherever level l exists: more than 256^l points
                icp_tree_kernel<<<dim3((unsigned) nb[l], ICP_SLOTS), ICP_BLOCK, 0, ctx->stream>>>(S, part + off[l - 1], nb[l - 1], (long long) nb[l - 1], pad, part + off[l], nb[l]);
            }
            icp_step_kernel<<<1, 64, 0, ctx->stream>>>(S, part + off[levels - 1], 1, K, d_trace);
        }
        LGR_HIP(ctx, hipGetLastError());
        LGR_HIP(ctx, hipMemcpyAsync(h, S, sizeof(IcpState), hipMemcpyDeviceToHost, ctx->stream));
        if (trace)   // the entries this group can have written
            LGR_HIP(ctx, hipMemcpyAsync(h + h_trace_off + (size_t) enqueued * sizeof(lgr_icp_step), d_trace + enqueued, (size_t) group * sizeof(lgr_icp_step),
                                        hipMemcpyDeviceToHost, ctx->stream));
        enqueued += group;
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(&hs, h, sizeof hs);
        if (hs.done) break;
        LGR_CHECK(ctx, enqueued < max_it, LGR_ERR_HIP);   // every iteration was evaluated: the device must have stopped
    }
    fill_result(hs, max_dist, out);
    if (trace) memcpy(trace, h + h_trace_off, (size_t) hs.n_eval * sizeof(lgr_icp_step));
    if (n_trace) *n_trace = trace || (trim && trim->info) ? hs.n_eval : 0;
    if (trim && trim->info && hs.n_eval) {   // (after the loop: one small copy, nothing of an iteration)
        LGR_HIP(ctx, hipMemcpyAsync(trim->info, d_info, (size_t) hs.n_eval * sizeof(lgr_icp_trim_step), hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return LGR_OK;
}

}  // namespace

extern "C" void lgr_default_icp_params(lgr_icp_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->max_iterations = 30;
    p->shrink = 1.f;
    p->rot_eps = 1e-6f;
    p->trans_eps = 1e-6f;
}

extern "C" int lgr_icp_plane_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T0[16], const lgr_icp_params* p,
                                 lgr_icp_result* out, lgr_icp_step* trace, int* n_trace) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, p, LGR_ERR_INVALID_ARG);
    lgr_icp_ex_params ex;
    lgr_default_icp_ex_params(&ex);   // point-to-plane, no robust kernel, gate off, no weights
    ex.base = *p;                     // every other argument is checked there
    return lgr_icp_ex_dev(ctx, d_src, ns, d_tgt, nt, T0, &ex, out, trace, n_trace);
}

extern "C" int lgr_icp_plane_host(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float T0[16], const lgr_icp_params* p,
                                  lgr_icp_result* out, lgr_icp_step* trace, int* n_trace) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, p, LGR_ERR_INVALID_ARG);
    lgr_icp_ex_params ex;
    lgr_default_icp_ex_params(&ex);
    ex.base = *p;
    return lgr_icp_ex_host(ctx, src, ns, tgt, nt, T0, &ex, out, trace, n_trace);
}

extern "C" void lgr_default_icp_ex_params(lgr_icp_ex_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    lgr_default_icp_params(&p->base);
    p->min_normal_cos = -1.f;
}

extern "C" int lgr_icp_ex_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T0[16], const lgr_icp_ex_params* p,
                              lgr_icp_result* out, lgr_icp_step* trace, int* n_trace) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, T0 && out && ns >= 0 && (d_src || ns == 0) && d_tgt && nt > 1 && ex_params_ok(p) && aligned16(d_src) && aligned16(d_tgt), LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, !trace || n_trace, LGR_ERR_INVALID_ARG);
    static_assert(LGR_ICP_POINT_TO_POINT == ICP_POINT_TO_POINT && LGR_ICP_PLANE_TO_PLANE == ICP_PLANE_TO_PLANE && LGR_ICP_ROBUST_HUBER == ICP_ROBUST_HUBER &&
                      LGR_ICP_ROBUST_CAUCHY == ICP_ROBUST_CAUCHY && LGR_ICP_ROBUST_TUKEY == ICP_ROBUST_TUKEY,
                  "lgr.h and lgr_icp_math.h number the variants and the robust kernels alike");
    const float eps = p->plane_eps == 0.f ? 1e-3f : p->plane_eps;
    const IcpEx X{(double) p->robust_scale, (double) p->min_normal_cos, 1.0 - (double) eps, p->weights};
    const IcpTermsFn terms = icp_pick(p->variant, p->robust, p->min_normal_cos > -1.f, p->weights != nullptr);
    return icp_run(ctx, terms, X, d_src, ns, d_tgt, nt, T0, &p->base, out, trace, n_trace);
}

extern "C" int lgr_icp_ex_host(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float T0[16], const lgr_icp_ex_params* p,
                               lgr_icp_result* out, lgr_icp_step* trace, int* n_trace) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, T0 && out && ns >= 0 && (src || ns == 0) && tgt && nt > 1 && ex_params_ok(p) && (!trace || n_trace), LGR_ERR_INVALID_ARG);
    float *ds, *dt, *dw;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    lgr_icp_ex_params staged = *p;
    if (p->weights) {
        LGR_TRY(hc.in(p->weights, (size_t) ns, &dw, 1));   // (one word of room: an empty source stages nothing)
        staged.weights = dw;
    }
    return lgr_icp_ex_dev(ctx, ds, ns, dt, nt, T0, &staged, out, trace, n_trace);
}

// ---- trimmed ICP (include/lgr.h lgr_icp_trim*)
namespace {

bool trim_params_ok(const lgr_icp_trim_params* p) {
    if (!p) return false;
    for (int r : p->reserved)
        if (r) return false;
    if (!(p->keep > 0.f && p->keep <= 1.f)) return false;
    if (!(p->scale_from_median >= 0.f && p->scale_from_median <= FLT_MAX)) return false;
    lgr_icp_ex_params ex = p->ex;
    if (p->scale_from_median > 0.f) {
        if (ex.robust == LGR_ICP_ROBUST_NONE) return false;
        ex.robust_scale = 1.f;   // not read: not validated
    }
    return ex_params_ok(&ex);
}

bool trim_neutral(const lgr_icp_trim_params* p) { return p->keep == 1.f && p->scale_from_median == 0.f; }

// the neutral call: lgr_icp_ex*'s bytes, and info from its trace
template <class Fn>
int trim_forward(lgr_ctx* ctx, Fn fn, const float* src, int ns, const float* tgt, int nt, const float T0[16], const lgr_icp_trim_params* p, lgr_icp_result* out,
                 lgr_icp_step* trace, lgr_icp_trim_step* info, int* n_trace) {
    std::vector<lgr_icp_step> own;
    lgr_icp_step* tr = trace;
    if (info && !trace) {
        own.resize((size_t) std::max(p->ex.base.max_iterations, 1));
        tr = own.data();
    }
    int n = 0;
    LGR_TRY(fn(ctx, src, ns, tgt, nt, T0, &p->ex, out, tr, tr ? &n : nullptr));
    for (int k = 0; info && k < n; ++k)
        info[k] = lgr_icp_trim_step{tr[k].pairs, tr[k].pairs, 0.f, p->ex.robust == LGR_ICP_ROBUST_NONE ? 0.f : (float) (double) p->ex.robust_scale};
    if (n_trace) *n_trace = n;
    return LGR_OK;
}

}  // namespace

extern "C" void lgr_default_icp_trim_params(lgr_icp_trim_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    lgr_default_icp_ex_params(&p->ex);
    p->keep = 1.f;
}

extern "C" int lgr_icp_trim_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T0[16], const lgr_icp_trim_params* p,
                                lgr_icp_result* out, lgr_icp_step* trace, lgr_icp_trim_step* info, int* n_trace) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, T0 && out && ns >= 0 && (d_src || ns == 0) && d_tgt && nt > 1 && trim_params_ok(p) && aligned16(d_src) && aligned16(d_tgt), LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, (!trace && !info) || n_trace, LGR_ERR_INVALID_ARG);
    if (trim_neutral(p)) return trim_forward(ctx, lgr_icp_ex_dev, d_src, ns, d_tgt, nt, T0, p, out, trace, info, n_trace);
    const lgr_icp_ex_params& ex = p->ex;
    const float eps = ex.plane_eps == 0.f ? 1e-3f : ex.plane_eps;
    const IcpEx X{(double) ex.robust_scale, (double) ex.min_normal_cos, 1.0 - (double) eps, ex.weights};
    const IcpTrimRun run{ex.variant, IcpTrim{ex.robust, ex.min_normal_cos > -1.f, p->keep, p->scale_from_median, ex.robust_scale}, info};
    return icp_run(ctx, nullptr, X, d_src, ns, d_tgt, nt, T0, &ex.base, out, trace, n_trace, &run);
}

extern "C" int lgr_icp_trim_host(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float T0[16], const lgr_icp_trim_params* p,
                                 lgr_icp_result* out, lgr_icp_step* trace, lgr_icp_trim_step* info, int* n_trace) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, T0 && out && ns >= 0 && (src || ns == 0) && tgt && nt > 1 && trim_params_ok(p) && ((!trace && !info) || n_trace), LGR_ERR_INVALID_ARG);
    if (trim_neutral(p)) return trim_forward(ctx, lgr_icp_ex_host, src, ns, tgt, nt, T0, p, out, trace, info, n_trace);
    float *ds, *dt, *dw;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    lgr_icp_trim_params staged = *p;
    if (p->ex.weights) {
        LGR_TRY(hc.in(p->ex.weights, (size_t) ns, &dw, 1));
        staged.ex.weights = dw;
    }
    return lgr_icp_trim_dev(ctx, ds, ns, dt, nt, T0, &staged, out, trace, info, n_trace);
}

// ---- the select alone (include/lgr.h lgr_rank_select*)
extern "C" int lgr_rank_select_dev(lgr_ctx* ctx, const float* d_keys, const uint8_t* d_valid, int n, const int64_t* ranks, int n_ranks, int32_t* out_index,
                                   float* out_key, uint8_t* d_below, int64_t* n_valid) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && (d_keys || n == 0) && ranks && n_ranks >= 1 && n_ranks <= 2 && out_index && out_key && n_valid, LGR_ERR_INVALID_ARG);
    SelState res{};
    if (n > 0) {
        LGR_HIP(ctx, hipSetDevice(ctx->device));
        SelWork* W;
        char* h;
        LGR_TRY(lgr_ws_t(ctx, WS_ICP_SEL, 1, &W));
        LGR_TRY(lgr_pinned(ctx, sizeof(SelState), (void**) &h));
        LGR_HIP(ctx, hipMemsetAsync(W, 0, sizeof(SelWork), ctx->stream));
        const SelRanks A{0, 1.f, {(long long) ranks[0], (long long) ranks[n_ranks - 1]}};
        sel_enqueue(ctx->stream, nullptr, (const uint32_t*) d_keys, d_valid, n, A, W);
        if (d_below) sel_below_kernel<<<(unsigned) cdivz((size_t) n, SEL_BLOCK), SEL_BLOCK, 0, ctx->stream>>>((const uint32_t*) d_keys, d_valid, n, W, (long long) ranks[0], d_below);
        LGR_HIP(ctx, hipGetLastError());
        LGR_HIP(ctx, hipMemcpyAsync(h, &W->st[SEL_MAX_PASSES], sizeof(SelState), hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(&res, h, sizeof res);
    }
    *n_valid = res.P;
    for (int q = 0; q < n_ranks; ++q) {
        const bool ok = n > 0 && ranks[q] >= 0 && ranks[q] < res.P && res.ok[q];
        if (!ok) {
            LGR_CHECK(ctx, q == 0 && ranks[0] == res.P, LGR_ERR_INVALID_ARG);
            out_index[0] = -1; out_key[0] = 0.f;
            continue;
        }
        out_index[q] = (int32_t) (uint32_t) res.prefix[q];
        out_key[q] = icp_trim_key_value((uint32_t) (res.prefix[q] >> 32));
    }
    return LGR_OK;
}

extern "C" int lgr_rank_select_host(lgr_ctx* ctx, const float* keys, const uint8_t* valid, int n, const int64_t* ranks, int n_ranks, int32_t* out_index, float* out_key,
                                    uint8_t* below, int64_t* n_valid) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && (keys || n == 0) && ranks && n_ranks >= 1 && n_ranks <= 2 && out_index && out_key && n_valid, LGR_ERR_INVALID_ARG);
    float* dk;
    uint8_t *dv = nullptr, *db = nullptr;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(keys, (size_t) n, &dk, 1));
    if (valid) LGR_TRY(hc.in(valid, (size_t) n, &dv, LGR_PAD_MASK));
    if (below) LGR_TRY(hc.out((size_t) n, &db, LGR_PAD_MASK));
    LGR_TRY(lgr_rank_select_dev(ctx, dk, dv, n, ranks, n_ranks, out_index, out_key, db, n_valid));
    LGR_TRY(hc.fetch(below, db, (size_t) n));
    return hc.finish();
}
