// lgr_refine.hip -- iterated closest-plane refinement of a transform for gfx950 (include/lgr.h lgr_refine_plane*).
//
// The step is the one the reference's final block takes once (src/sac_prerejective_omp.cpp:270-291): the closest-plane inliers of the
// transform, estimateOptimalRigidTransformation over those pairs, the evaluation of the result -- here in the DENSE form of the estimator
// (every source point, lgr_plane_dense.hip) and repeated while the metric rises.  Declared order: DESIGN.md section 4; the CPU statement is
// tests/refine_ref_lib.py.  The per-point body is plane_dense_kernel's (lgr_plane_point.cuh), the two sums are gt_seqsum_job's, the refit is
// lgr_refit_svd_dev's (lgr_refit_flagged_launch), so every evaluated transform and its figures carry the bits of
// lgr_evaluate_plane_dense_dev + lgr_refit_svd_dev driven from the host.
//
// Set-up, once per call: the threshold, the weights and their sum, ONE grid over the target, the source's half of the pairs (P0).
// A step, all on the stream:
//   refit over (P0[i], P1[i]) where flags[i]        -> S.Tc          (scan, compaction, refit_kernel; the pair count is S.n_pairs)
//   refine_dense_kernel: Tc from DEVICE memory      -> flags, terms, P1[i] = the nearest target of i, S.counter
//   refine_sum_kernel: the two sequential sums      -> S.sums
//   refine_decide_kernel: E' from the sums, the float compare, S.cur / steps / stop / done, the trace entry, S.n_pairs for the next refit
// flags, terms and P1 of an accepted candidate ARE the input of the next step's refit; those of a rejected one are never read.  Steps are
// enqueued blind in groups of LGR_REFINE_GROUP with one read-back of S per group; once S.done is set every kernel of a later step returns
// at once (the refit through a pair count of 0), and S.cur, S.first, S.rejected and the trace stay as they are.
#include <algorithm>
#include <cfloat>

#include "lgr_grid.cuh"
#include "lgr_host.h"
#include "lgr_internal.h"
#include "lgr_math.cuh"
#include "lgr_plane_point.cuh"
#include "lgr_pointpass.cuh"

namespace {

struct RfState {
    lgr_refine_step cur, first, rejected;   // the last accepted step, T0's evaluation, the candidate that lost
    float Tc[16];                           // the transform to evaluate: T0 (uploaded), then each refit's
    float sums[2];                          // score, squared distances of the evaluation in flight
    int counter;                            // ... and its inliers
    int n_pairs, zero;                      // the next refit's pair count as refit_kernel reads it (n_pairs + zero); 0 once done
    int steps, stop, done, n_eval;          // accepted steps, LGR_REFINE_STOP_*, the loop has ended, trace entries written
    int pad[3];
};
static_assert(sizeof(RfState) % 16 == 0, "RfState is copied and cleared in one piece");

// plane_dense_kernel's per-point body (plane_dense_point, lgr_plane_point.cuh) with the transform read from device memory and the target's
// half of the pair written next to the terms.  Tc and done are wave-uniform addresses: scalar loads, no divergence.
template <bool W>
__global__ __launch_bounds__(PP_BLOCK) void refine_dense_kernel(GridDev g, const float4* __restrict__ src, int ns, const int* __restrict__ done, const float* __restrict__ T,
                                                               int* __restrict__ counter, float thr, float r2, int score_id, const float* __restrict__ w, float* __restrict__ term_val,
                                                               float* __restrict__ term_sq, int* __restrict__ flags, float4* __restrict__ P1) {
    if (*done) return;
    const int i = blockIdx.x * PP_BLOCK + threadIdx.x;
    bool inl = false;
    if (i < ns) {
        const PlanePoint p = plane_dense_point<W>(g, src[(size_t) i * 3], T, thr, r2, score_id, w, i);
        inl = p.inl;
        term_val[i] = p.value;
        term_sq[i] = p.sq;
        flags[i] = inl ? 1 : 0;
        P1[i] = make_float4(p.Q.x, p.Q.y, p.Q.z, 0.f);   // the grid's copy of tgt[nn]: the same bits
    }
    wave_count(inl, counter);
}

// P0[i] = the source point, once per call (the refit's pack_pairs layout)
__global__ __launch_bounds__(PP_BLOCK) void refine_pack_src_kernel(const float4* __restrict__ src, int ns, float4* __restrict__ P0) {
    const int i = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (i >= ns) return;
    const float4 P = src[(size_t) i * 3];
    P0[i] = make_float4(P.x, P.y, P.z, 0.f);
}

// gt_seqsum_kernel's two jobs (block 0: the values, block 1: the squared distances), skipped behind the stop
__global__ __launch_bounds__(PP_BLOCK) void refine_sum_kernel(const float* __restrict__ val, const float* __restrict__ sq, int n, RfState* __restrict__ S) {
    if (S->done) return;
    const float sum = gt_seqsum_job(blockIdx.x ? sq : val, n, false);
    if (threadIdx.x == 0) S->sums[blockIdx.x] = sum;
}

// one thread: the figures of the evaluation in flight (lgr_plane_figures, as dense_eval takes them on the host), then the statement's compare
__global__ void refine_decide_kernel(RfState* __restrict__ S, lgr_refine_step* __restrict__ trace, float denom, int max_steps, int first) {
    if (threadIdx.x != 0 || S->done) return;
    lgr_refine_step c;
    for (int k = 0; k < 16; ++k) c.transformation[k] = S->Tc[k];
    const int n = S->counter;
    c.n_inliers = n;
    c.score = S->sums[0];
    lgr_plane_figures(S->sums[0], S->sums[1], n, denom, &c.rmse, &c.metric);
    trace[S->n_eval] = c;   // n_eval <= max_steps + 1 < the buffer's max_steps + 2
    S->n_eval += 1;
    S->counter = 0;
    int done = 0;
    if (first) {
        S->first = c;
        S->cur = c;
    } else if (c.metric > S->cur.metric) {
        S->cur = c;
        S->steps += 1;
    } else {
        S->rejected = c;
        S->stop = LGR_REFINE_STOP_NO_GAIN;
        done = 1;
    }
    if (!done) {   // the head of the next turn of the loop
        if (S->steps >= max_steps) { S->stop = LGR_REFINE_STOP_MAX_STEPS; done = 1; }
        else if (S->cur.n_inliers < 3) { S->stop = LGR_REFINE_STOP_NO_PAIRS; done = 1; }
    }
    S->n_pairs = done ? 0 : S->cur.n_inliers;
    S->done = done;
}

void fill_result(const RfState& s, float thr, lgr_refine_result* out) {
    memset(out, 0, sizeof *out);
    memcpy(out->transformation, s.cur.transformation, 64);
    out->metric = s.cur.metric; out->rmse = s.cur.rmse; out->score = s.cur.score; out->n_inliers = s.cur.n_inliers;
    out->threshold = thr; out->steps = s.steps; out->stop = s.stop;
    out->first = s.first; out->rejected = s.rejected;
}

bool params_ok(const lgr_refine_params* p) {
    if (!p || p->score_id < 0 || p->score_id > 3 || p->max_steps < 0 || p->max_steps > LGR_REFINE_MAX_STEPS) return false;
    for (int r : p->reserved)
        if (r) return false;
    return !(p->threshold != p->threshold) && p->threshold <= 1e18f;   // the squared radius stays finite
}

// an empty source: nothing to evaluate, T0 comes back
void empty_result(const float* T0, const lgr_refine_params* p, lgr_refine_result* out, lgr_refine_step* trace, int* n_trace) {
    RfState s{};
    memcpy(s.cur.transformation, T0, 64);
    s.cur.rmse = FLT_MAX;
    s.first = s.cur;
    s.stop = LGR_REFINE_STOP_NO_PAIRS;
    fill_result(s, p->threshold > 0.f ? p->threshold : 0.f, out);
    if (trace) trace[0] = s.first;
    if (n_trace) *n_trace = trace ? 1 : 0;
}

}  // namespace

extern "C" void lgr_default_refine_params(lgr_refine_params* p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->score_id = LGR_SCORE_MSE;
    p->max_steps = 10;
}

extern "C" int lgr_refine_plane_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const float T0[16], const lgr_refine_params* p,
                                    const lgr_metric_params* mp, lgr_refine_result* out, lgr_refine_step* trace, int* n_trace) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, T0 && out && ns >= 0 && (d_src || ns == 0) && d_tgt && nt > 1 && params_ok(p) && aligned16(d_src) && aligned16(d_tgt), LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, !trace || n_trace, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    const float* d_w = nullptr;
    float w_sum = 0.f, w_gate = 0.f;
    if (ns == 0) {
        empty_result(T0, p, out, trace, n_trace);
        return LGR_OK;
    }
    if (mp) LGR_TRY(lgr_weights_prepare(ctx, d_src, ns, mp, &d_w, &w_sum, &w_gate));   // harris / tomasi: LGR_ERR_UNSUPPORTED
    // ---- set-up: threshold, grid, buffers (every synchronisation that is not a group's read-back happens here)
    lgr_plane_target pt;
    LGR_TRY(lgr_plane_target_setup(ctx, d_tgt, nt, p->threshold, 2e18f, &pt));
    const float thr = pt.thr, radius = pt.radius;
    const GridDev& g = pt.g;
    const int max_steps = p->max_steps;
    const size_t nn = ((size_t) ns + 63) & ~(size_t) 63;
    RfState* S;
    int32_t* buf;
    float4* pairs;
    lgr_refine_step* d_trace;
    char* h;
    LGR_TRY(lgr_ws_t(ctx, WS_RF_STATE, 1, &S));
    LGR_TRY(lgr_ws_t(ctx, WS_RF_TERMS, 3 * nn + 16, &buf));
    LGR_TRY(lgr_ws_t(ctx, WS_RF_PAIRS, 2 * nn, &pairs));
    LGR_TRY(lgr_ws_t(ctx, WS_RF_TRACE, (size_t) max_steps + 2, &d_trace));
    LGR_TRY(lgr_refit_flagged_reserve(ctx, ns));
    const size_t h_trace_off = (sizeof(RfState) + 63) & ~(size_t) 63;
    LGR_TRY(lgr_pinned(ctx, h_trace_off + ((size_t) max_steps + 2) * sizeof(lgr_refine_step), (void**) &h));
    float *val = (float*) buf, *sq = (float*) (buf + nn);
    int* flags = buf + 2 * nn;
    float4 *P0 = pairs, *P1 = pairs + nn;
    const float denom = d_w ? w_sum : (float) ns;
    const int blocks = cdiv(ns, PP_BLOCK);
    auto evaluate = [&](int first) {
        if (d_w)
            refine_dense_kernel<true><<<blocks, PP_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_src, ns, &S->done, S->Tc, &S->counter, thr, radius * radius, p->score_id, d_w, val, sq, flags, P1);
        else
            refine_dense_kernel<false><<<blocks, PP_BLOCK, 0, ctx->stream>>>(g, (const float4*) d_src, ns, &S->done, S->Tc, &S->counter, thr, radius * radius, p->score_id, nullptr, val, sq, flags, P1);
        refine_sum_kernel<<<2, PP_BLOCK, 0, ctx->stream>>>(val, sq, ns, S);
        refine_decide_kernel<<<1, 64, 0, ctx->stream>>>(S, d_trace, denom, max_steps, first);
    };
    // ---- E0
    LGR_HIP(ctx, hipMemsetAsync(S, 0, sizeof(RfState), ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(S->Tc, T0, 64, hipMemcpyHostToDevice, ctx->stream));
    refine_pack_src_kernel<<<blocks, PP_BLOCK, 0, ctx->stream>>>((const float4*) d_src, ns, P0);
    evaluate(1);
    LGR_HIP(ctx, hipGetLastError());
    // ---- the steps, LGR_REFINE_GROUP at a time; nothing of a step passes through the host
    RfState hs;
    int enqueued = 0, copied = 0;
    for (;;) {
        const int group = std::min((int) LGR_REFINE_GROUP, max_steps - enqueued);
        for (int k = 0; k < group; ++k) {
            LGR_TRY(lgr_refit_flagged_launch(ctx, P0, P1, ns, flags, &S->n_pairs, S->Tc));
            evaluate(0);
        }
        LGR_HIP(ctx, hipGetLastError());
        enqueued += group;
        LGR_HIP(ctx, hipMemcpyAsync(h, S, sizeof(RfState), hipMemcpyDeviceToHost, ctx->stream));
        if (trace)   // the entries this group can have written
            LGR_HIP(ctx, hipMemcpyAsync(h + h_trace_off + (size_t) copied * sizeof(lgr_refine_step), d_trace + copied,
                                        (size_t) (enqueued + 1 - copied) * sizeof(lgr_refine_step), hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(&hs, h, sizeof hs);
        copied = enqueued + 1;
        if (hs.done) break;
        LGR_CHECK(ctx, enqueued < max_steps, LGR_ERR_HIP);   // every step was evaluated: the device must have stopped
    }
    fill_result(hs, thr, out);
    if (trace) memcpy(trace, h + h_trace_off, (size_t) hs.n_eval * sizeof(lgr_refine_step));
    if (n_trace) *n_trace = trace ? hs.n_eval : 0;
    return LGR_OK;
}

extern "C" int lgr_refine_plane(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const float T0[16], const lgr_refine_params* p,
                                const lgr_metric_params* mp, lgr_refine_result* out, lgr_refine_step* trace, int* n_trace) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, T0 && out && ns >= 0 && (src || ns == 0) && tgt && nt > 1 && params_ok(p) && (!trace || n_trace), LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_metric_params staged;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    if (ns) LGR_TRY(hc.weights(ns, &mp, &staged));   // (an empty source: the parameters go on as they came)
    return lgr_refine_plane_dev(ctx, ds, ns, dt, nt, T0, p, mp, out, trace, n_trace);
}
