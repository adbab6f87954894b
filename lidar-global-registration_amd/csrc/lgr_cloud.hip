// lgr_cloud.hip -- the prepared cloud: the reference's per-cloud Storage (include/matching.h:132-146, filled by
// FeatureBasedMatcherImpl::initialize, :164-262) as an object that owns its device memory.  The stages that fill it are the
// correspondence search's own (lgr_align.hip: lgr_cloud_fill); this file holds the object, its memory and its getters.
#include "lgr_cloud.h"

int lgr_cloud_alloc(lgr_ctx* cx, lgr_cloud* c, size_t bytes, void** out) {
    if (bytes == 0) bytes = 16;
    void* p = nullptr;
    LGR_HIP(cx, hipMalloc(&p, bytes));
    c->blocks.push_back(p);
    c->bytes += bytes;
    *out = p;
    return LGR_OK;
}

extern "C" int lgr_cloud_destroy(lgr_cloud* c) {
    if (!c) return LGR_OK;
    int rc = LGR_OK;
    if (hipSetDevice(c->device) != hipSuccess) rc = LGR_ERR_HIP;
    for (void* p : c->blocks)
        if (hipFree(p) != hipSuccess) rc = LGR_ERR_HIP;
    delete c;
    return rc;
}

static int cloud_prepare(lgr_ctx* ctx, const float* pts, bool on_host, int n, int side, const lgr_params* p, const lgr_feature_params* fp, lgr_cloud** out) {
    LGR_CHECK(ctx, out != nullptr, LGR_ERR_INVALID_ARG);
    *out = nullptr;
    LGR_CHECK(ctx, (pts || n == 0) && n >= 0 && p && (side == 0 || side == 1), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    lgr_cloud* c = new (std::nothrow) lgr_cloud;
    LGR_CHECK(ctx, c != nullptr, LGR_ERR_OOM);
    c->device = ctx->device;
    c->n = n;
    int rc = lgr_cloud_alloc_t(ctx, c, (size_t) n * 12, &c->pts);
    if (rc == LGR_OK && n) {
        const hipError_t e = hipMemcpyAsync(c->pts, pts, (size_t) n * 48, on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) rc = lgr_fail(ctx, LGR_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
    }
    if (rc == LGR_OK) rc = lgr_cloud_fill(ctx, c, side, p, fp);
    // a borrowed host array must not be read after the call returns, and a failed object is freed under kernels that may still write it
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (rc == LGR_OK && e != hipSuccess) rc = lgr_fail(ctx, LGR_ERR_HIP, hipGetErrorString(e), __FILE__, __LINE__);
    if (rc != LGR_OK) { (void) lgr_cloud_destroy(c); return rc; }
    *out = c;
    return LGR_OK;
}

extern "C" int lgr_cloud_prepare_dev(lgr_ctx* ctx, const float* d_pts, int n, int side, const lgr_params* p, const lgr_feature_params* fp, lgr_cloud** out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return cloud_prepare(ctx, d_pts, false, n, side, p, fp, out);
}

extern "C" int lgr_cloud_prepare(lgr_ctx* ctx, const float* pts, int n, int side, const lgr_params* p, const lgr_feature_params* fp, lgr_cloud** out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return cloud_prepare(ctx, pts, true, n, side, p, fp, out);
}

// the levels that hold rows: none for a cloud without two points or without key points
static int n_levels(const lgr_cloud* c) {
    if (c->empty || c->m == 0) return 0;
    return c->multiscale ? (int) c->ms.levels.size() : 1;
}
static const lgr_cloud_lvl& level_of(const lgr_cloud* c, int level) { return c->multiscale ? c->ms.levels[level] : c->single; }

extern "C" int lgr_cloud_info(const lgr_cloud* c, struct lgr_cloud_info* out) {
    if (!c || !out) return LGR_ERR_INVALID_ARG;
    memset(out, 0, sizeof *out);
    out->n = c->n;
    out->keypoints = c->empty ? 0 : c->m;
    out->row_len = c->row_len;
    out->levels = n_levels(c);
    out->first_log2_radius = out->levels ? level_of(c, 0).log2_radius : 0;
    out->multiscale = c->multiscale ? 1 : 0;
    out->bytes = c->bytes;
    return LGR_OK;
}

extern "C" int lgr_cloud_keypoints_dev(const lgr_cloud* c, const int32_t** d_idx, int* m) {
    if (!c || !d_idx || !m) return LGR_ERR_INVALID_ARG;
    *d_idx = c->kidx;
    *m = c->empty ? 0 : c->m;
    return LGR_OK;
}

static void iota(int32_t* out, int m) { for (int i = 0; i < m; ++i) out[i] = i; }

extern "C" int lgr_cloud_keypoints(const lgr_cloud* c, int32_t* out, int* m) {
    if (!c || !m) return LGR_ERR_INVALID_ARG;
    *m = c->empty ? 0 : c->m;
    if (!out || *m == 0) return LGR_OK;
    if (!c->kidx) { iota(out, *m); return LGR_OK; }
    if (hipSetDevice(c->device) != hipSuccess || hipMemcpy(out, c->kidx, (size_t) *m * 4, hipMemcpyDeviceToHost) != hipSuccess) return LGR_ERR_HIP;
    return LGR_OK;
}

extern "C" int lgr_cloud_level_dev(const lgr_cloud* c, int level, lgr_cloud_level_info* info, const int32_t** d_list, const float** d_rows) {
    if (!c || level < 0 || level >= n_levels(c)) return LGR_ERR_INVALID_ARG;
    const lgr_cloud_lvl& l = level_of(c, level);
    if (info) {
        memset(info, 0, sizeof *info);
        info->log2_radius = l.log2_radius; info->radius = l.radius; info->voxel = l.voxel; info->rows = l.rows; info->surface = l.surface;
    }
    if (d_list) *d_list = c->multiscale ? c->ms.d_lists + l.off : nullptr;
    if (d_rows) *d_rows = c->multiscale ? c->ms.feat + l.off * c->row_len : c->feat;
    return LGR_OK;
}

extern "C" int lgr_cloud_level(const lgr_cloud* c, int level, lgr_cloud_level_info* info, int32_t* list_out, float* rows_out) {
    lgr_cloud_level_info li;
    const int32_t* d_list;
    const float* d_rows;
    const int rc = lgr_cloud_level_dev(c, level, &li, &d_list, &d_rows);
    if (rc != LGR_OK) return rc;
    if (info) *info = li;
    if (hipSetDevice(c->device) != hipSuccess) return LGR_ERR_HIP;
    if (list_out && li.rows) {
        if (!d_list) iota(list_out, li.rows);
        else if (hipMemcpy(list_out, d_list, (size_t) li.rows * 4, hipMemcpyDeviceToHost) != hipSuccess) return LGR_ERR_HIP;
    }
    if (rows_out && li.rows && hipMemcpy(rows_out, d_rows, (size_t) li.rows * c->row_len * 4, hipMemcpyDeviceToHost) != hipSuccess) return LGR_ERR_HIP;
    return LGR_OK;
}
