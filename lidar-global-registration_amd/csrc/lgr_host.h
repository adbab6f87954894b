// lgr_host.h -- staging for the host entry points of include/lgr.h (the forms without the _dev suffix).  A host form checks its arguments,
// then uploads its arrays, calls the _dev twin, downloads and synchronises; the four steps go through one lgr_host_call:
//     lgr_host_call hc(ctx);
//     LGR_TRY(hc.in(pts, (size_t) n * 12, &dp));      // the next WS_HOST slot, count (+ pad) elements; copied up when pts && count
//     LGR_TRY(hc.out((size_t) n, &dout));             // the next WS_HOST slot, nothing copied
//     LGR_TRY(lgr_x_dev(ctx, dp, n, dout));
//     LGR_TRY(hc.fetch(out, dout, (size_t) n));       // copied down when out && count
//     return hc.finish();                             // hipStreamSynchronize
// Slots WS_HOST_0 .. WS_HOST_7 are handed out in the order of the calls, so two arrays of one call never share a buffer and nobody picks
// a slot by hand; a ninth is LGR_ERR_UNSUPPORTED.  Only this header names them: _dev code never touches a host slot (a _dev function
// that needs scratch has a slot named for what it holds).  A pointer handed out is never null, also for count 0 (lgr_ws); a caller whose
// twin wants null for an empty or absent array writes `n ? d : nullptr` at the call.  Several arrays may share one slot: stage one
// buffer and offset into it.  All copies are ordered on ctx->stream.  lgr_ws synchronises the stream when it grows a slot, and slots are
// grown here array by array, between the copies: a first call may synchronise more often than one that sizes all its slots before the
// first copy.  Results cannot depend on that.  The checks, early returns and error codes of an entry point stay in the entry point.
#pragma once
#include "lgr_internal.h"

// Slack, in elements, behind a staged cloud (floats) and a staged byte mask: what the _dev code gives its own buffers of these kinds
// (n * 12 + 4 for a cloud it copies: WS_HO_STAGE, WS_SELF_COPY; c + 16 for a mask it owns: WS_RANSAC_MASK, WS_PD_MASK, WS_MEASURE_MASKS),
// so that a staged array is never tighter than the buffers the kernels run on in the pipeline.
constexpr size_t LGR_PAD_CLOUD = 4, LGR_PAD_MASK = 16;

struct lgr_host_call {
    lgr_ctx* ctx;
    int used = 0;
    explicit lgr_host_call(lgr_ctx* c) : ctx(c) {}

    template <class T>
    int out(size_t count, T** d, size_t pad = 0) {
        if (used == 0) LGR_HIP(ctx, hipSetDevice(ctx->device));
        if (used > WS_HOST_7 - WS_HOST_0) return lgr_fail(ctx, LGR_ERR_UNSUPPORTED, "a host entry point stages at most 8 arrays", __FILE__, __LINE__);
        return lgr_ws_t(ctx, WS_HOST_0 + used++, count + pad, d);
    }
    template <class T>
    int in(const T* h, size_t count, T** d, size_t pad = 0) {
        LGR_TRY(out(count, d, pad));
        if (h && count) LGR_HIP(ctx, hipMemcpyAsync(*d, h, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        return LGR_OK;
    }
    template <class T>
    int fetch(T* h, const T* d, size_t count) {
        if (h && count) LGR_HIP(ctx, hipMemcpyAsync(h, d, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        return LGR_OK;
    }
    int finish() {
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return LGR_OK;
    }

    // the two clouds of a pair entry point (rows of 12 floats): null when empty, which is how the twins are handed an empty cloud
    int clouds(const float* src, int ns, const float* tgt, int nt, float** ds, float** dt) {
        LGR_TRY(in(src, (size_t) ns * 12, ds, LGR_PAD_CLOUD));
        LGR_TRY(in(tgt, (size_t) nt * 12, dt, LGR_PAD_CLOUD));
        if (!ns) *ds = nullptr;
        if (!nt) *dt = nullptr;
        return LGR_OK;
    }
    // the caller's per-point weights of a metric (lgr_metric_params.weights, ns host floats): *mp then points at `staged`, a copy of the
    // parameters that carries the device array; parameters without weights are left as they are
    int weights(int ns, const lgr_metric_params** mp, lgr_metric_params* staged) {
        if (!*mp || !(*mp)->weights) return LGR_OK;
        float* dw;
        LGR_TRY(in((*mp)->weights, (size_t) ns, &dw));
        *staged = **mp; staged->weights = dw; *mp = staged;
        return LGR_OK;
    }
};
