// lgr_rops.hip -- gravity-aligned local reference frames and the RoPS135 descriptor on given frames.
//
//   src/common.cpp:693-755 estimateReferenceFrames, lrf_id "gravity"                 -> lgr_gravity_lrf*
//   include/common.h estimateFeatures<RoPS135> with given frames = ROPSEstimationWithLocalReferenceFrames
//     (include/pcl/impl/rops_custom_lrf.hpp:96-186, :364-518; 5 bins, 3 rotations, support radius = radius)  -> lgr_rops*
// Canonical choices: Eigen's 3-term reductions and cross product of lgr_rops_math.h, glibc's logf restated
// there, and its rule for static_cast<unsigned>; tests/cpp/rops_ref.cpp states the stage on the CPU with the host's own libm and the
// -m gpu tests compare bit for bit.
//
// A RoPS row needs no neighbour order: it is a function of the support SET.  The 27 boxes are min / max with std::min / std::max's
// '(b < a) ? b : a', which a NaN coordinate never enters and which differs between orders only in the sign of a zero bound; a zero
// bound's sign cannot move a point to another cell (p - (+-0) == p for p != 0, +-0 / L == +-0 -> cell 0 for L != 0, and a degenerate
// box gives 0 / 0 = NaN -> cell 0 either way).  The cells are integer counts.  The moments, the entropy and the L1 norm then follow
// the reference's fixed (i, j) and feature orders.
#include <cfloat>
#include <cmath>

#include "lgr_grid.cuh"
#include "lgr_host.h"
#include "lgr_libm.cuh"
#include "lgr_rops_math.h"

namespace {

constexpr int ROPS_LEN = 135;      // 3 axes x 3 rotations x 3 projections x (4 moments + entropy)
constexpr int ROPS_CAP = 1024;     // transformed support points cached in LDS; a larger support is re-gathered from the grid
constexpr float RF_MIN_ANGLE_RAD = 0.04f;   // src/common.cpp:21

// gravity test of src/common.cpp:724: acos(|clamp(z . g, -1, 1)|) > 0.04 with g = (0, 0, 1); NaN normals fail it
__device__ __forceinline__ bool gravity_ok(const float* __restrict__ kp) {
    float d = rops_dot3(kp[4], kp[5], kp[6], 0.f, 0.f, 1.f);
    d = d < -1.f ? -1.f : (1.f < d ? 1.f : d);   // std::clamp (NaN passes through)
    return lgr_glibc::acosf_(fabsf(d)) > RF_MIN_ANGLE_RAD;
}

// the key points whose frame is SHOT's: a copy of the row, every other row NaN (shot_kernel gives those a NaN frame at once)
__global__ void gravity_mask_kernel(const float* __restrict__ kps, int m, float* __restrict__ masked) {
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) m * 12) return;
    const size_t i = e / 12;
    masked[e] = gravity_ok(kps + i * 12) ? __uint_as_float(0x7fc00000u) : kps[e];
}

// y = g x z, x = y x z (Eigen cross products, not normalized) where the test passes; other rows keep their SHOT frame
__global__ void gravity_frame_kernel(const float* __restrict__ kps, int m, float* __restrict__ lrf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const float* kp = kps + (size_t) i * 12;
    if (!gravity_ok(kp)) return;
    const float g[3] = {0.f, 0.f, 1.f}, z[3] = {kp[4], kp[5], kp[6]};
    float y[3], x[3];
    rops_cross(g, z, y);
    rops_cross(y, z, x);
    float* o = lrf + (size_t) i * 9;
    o[0] = x[0]; o[1] = x[1]; o[2] = x[2]; o[3] = y[0]; o[4] = y[1]; o[5] = y[2]; o[6] = z[0]; o[7] = z[1]; o[8] = z[2];
}

__device__ __forceinline__ float fmin_ref(float a, float b) { return b < a ? b : a; }   // std::min(a, b)
__device__ __forceinline__ float fmax_ref(float a, float b) { return a < b ? b : a; }   // std::max(a, b)

// One wave per key point.
//   gather  the support (d2 < r2 on the surface grid, shot_kernel's expression), transformed by the frame: lrf * (q - p), cached in
//           LDS up to ROPS_CAP points (a larger support is re-gathered, with the same arithmetic, by every pass that needs it);
//   boxes   per lane min / max of the 9 rotated copies, then a wave reduction;
//   cells   every point's 27 cells, counted with LDS integer atomics (order-free);
//   moments lanes 0..26 own one (rotation, projection): 4 central moments and the entropy; then the L1 normalization.
__global__ __launch_bounds__(64) void rops_kernel(GridDev g, const float* __restrict__ kps, int m, float radius, const float* __restrict__ lrf,
                                                  float* __restrict__ out) {
    __shared__ float sx[ROPS_CAP], sy[ROPS_CAP], sz[ROPS_CAP];
    __shared__ float rot[81];           // the 9 rotations (axis-major, then angle), row-major
    __shared__ float box[2][27];        // min / max of rotation r, coordinate c at [3 r + c]
    __shared__ unsigned cnt[27 * 25];   // (rotation, projection) x column-major 5 x 5 cells
    __shared__ float feat[ROPS_LEN];
    const int l = threadIdx.x;
    const int kp = blockIdx.x;
    if (kp >= m) return;
    const float x = kps[(size_t) kp * 12], y = kps[(size_t) kp * 12 + 1], z = kps[(size_t) kp * 12 + 2];
    const float r2 = radius * radius;
    const float* F = lrf + (size_t) kp * 9;
    const float f0 = F[0], f1 = F[1], f2 = F[2], f3 = F[3], f4 = F[4], f5 = F[5], f6 = F[6], f7 = F[7], f8 = F[8];
    if (l < 9) {   // rotateCloud: theta = 22.5, 45, 67.5 degrees; rad = (float) (M_PI / 180); cos / sin of the float product
        const float rad = (float) (3.14159265358979323846 / 180.0);
        const float theta = 22.5f * (float) (l % 3 + 1);
        float R[9];
        rops_rotation(l / 3, lgr_glibc::cosf_(theta * rad), lgr_glibc::sinf_(theta * rad), R);
        for (int k = 0; k < 9; ++k) rot[9 * l + k] = R[k];
    }
    for (int j = l; j < 27 * 25; j += 64) cnt[j] = 0u;
    const bool finite = lgr_finite3(x, y, z);   // (a non-finite key point has no support: the zero row)
    const int cx = finite ? min(max(lgr_cellc(x, g.ox, g.h), 0), g.dx - 1) : 0;
    const int cy = finite ? min(max(lgr_cellc(y, g.oy, g.h), 0), g.dy - 1) : 0;
    const int cz = finite ? min(max(lgr_cellc(z, g.oz, g.h), 0), g.dz - 1) : 0;
    // f(tx, ty, tz) for every support point in this lane's share; store: cache the first ROPS_CAP in LDS.  Returns the support size.
    auto scan = [&](bool store, auto&& f) -> int {
        int total = 0;
        if (!finite || g.n == 0) return 0;
        for (int zz = max(cz - 1, 0); zz <= min(cz + 1, g.dz - 1); ++zz)
            for (int yy = max(cy - 1, 0); yy <= min(cy + 1, g.dy - 1); ++yy) {
                const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dx - 1);
                const size_t c0 = ((size_t) zz * g.dy + yy) * g.dx;
                const int b = g.cell_start[c0 + x0], e = g.cell_start[c0 + x1 + 1];
                for (int t0 = b; t0 < e; t0 += 64) {
                    const int t = t0 + l;
                    bool in = false;
                    float tx = 0.f, ty = 0.f, tz = 0.f;
                    if (t < e) {
                        const float4 P = g.pxyz[t];
                        in = lgr_dist2(x, y, z, P.x, P.y, P.z) < r2;
                        const float dx = P.x - x, dy = P.y - y, dz = P.z - z;   // transformCloud: lrf_matrix * (q - p)
                        tx = rops_dot3(f0, f1, f2, dx, dy, dz);
                        ty = rops_dot3(f3, f4, f5, dx, dy, dz);
                        tz = rops_dot3(f6, f7, f8, dx, dy, dz);
                    }
                    const unsigned long long bm = __ballot(in);
                    if (bm == 0ull) continue;
                    if (in) {
                        if (store) {
                            const int slot = total + __builtin_amdgcn_mbcnt_hi((unsigned) (bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) bm, 0u));
                            if (slot < ROPS_CAP) { sx[slot] = tx; sy[slot] = ty; sz[slot] = tz; }
                        }
                        f(tx, ty, tz);
                    }
                    total += __popcll(bm);
                }
            }
        return total;
    };
    // ---- gather + boxes
    float mn[27], mx[27];
#pragma unroll
    for (int k = 0; k < 27; ++k) { mn[k] = FLT_MAX; mx[k] = -FLT_MAX; }
    __syncthreads();   // rot
    auto boxes = [&](float tx, float ty, float tz) {
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const float* R = rot + 9 * r;
            const float px = rops_dot3(R[0], R[1], R[2], tx, ty, tz), py = rops_dot3(R[3], R[4], R[5], tx, ty, tz),
                        pz = rops_dot3(R[6], R[7], R[8], tx, ty, tz);
            mn[3 * r] = fmin_ref(mn[3 * r], px); mn[3 * r + 1] = fmin_ref(mn[3 * r + 1], py); mn[3 * r + 2] = fmin_ref(mn[3 * r + 2], pz);
            mx[3 * r] = fmax_ref(mx[3 * r], px); mx[3 * r + 1] = fmax_ref(mx[3 * r + 1], py); mx[3 * r + 2] = fmax_ref(mx[3 * r + 2], pz);
        }
    };
    const int total = scan(true, boxes);
    const bool cached = total <= ROPS_CAP;
#pragma unroll
    for (int k = 0; k < 27; ++k)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            mn[k] = fmin_ref(mn[k], __shfl_xor(mn[k], o));
            mx[k] = fmax_ref(mx[k], __shfl_xor(mx[k], o));
        }
    if (l == 0) {
#pragma unroll
        for (int k = 0; k < 27; ++k) { box[0][k] = mn[k]; box[1][k] = mx[k]; }
    }
    __syncthreads();
    // ---- cells: getDistributionMatrix for projections XY, XZ, YZ; bin length (max - min) / 5 per coordinate
    auto cells = [&](float tx, float ty, float tz) {
        for (int r = 0; r < 9; ++r) {
            const float* R = rot + 9 * r;
            const float p[3] = {rops_dot3(R[0], R[1], R[2], tx, ty, tz), rops_dot3(R[3], R[4], R[5], tx, ty, tz),
                                rops_dot3(R[6], R[7], R[8], tx, ty, tz)};
#pragma unroll
            for (int pr = 0; pr < 3; ++pr) {
                const int cu = pr == 2 ? 1 : 0, cv = pr == 0 ? 1 : 2;
                const float lo_u = box[0][3 * r + cu], lo_v = box[0][3 * r + cv];
                const float bl_u = (box[1][3 * r + cu] - lo_u) / 5.f, bl_v = (box[1][3 * r + cv] - lo_v) / 5.f;
                const float pu = cu == 0 ? p[0] : p[1], pv = cv == 1 ? p[1] : p[2];
                const uint64_t c = rops_cell((pu - lo_u) / bl_u, (pv - lo_v) / bl_v);
                if (c < 25u) atomicAdd(&cnt[(3 * r + pr) * 25 + (int) c], 1u);
            }
        }
    };
    if (cached) {
        for (int q = l; q < total; q += 64) cells(sx[q], sy[q], sz[q]);
    } else {
        scan(false, cells);
    }
    __syncthreads();
    // ---- moments (feature order: axis, angle, projection, then the 5 values)
    if (l < 27) {
        float v[5];
        rops_moments(cnt + 25 * l, (uint32_t) total, v);
        for (int k = 0; k < 5; ++k) feat[5 * l + k] = v[k];
    }
    __syncthreads();
    // std::accumulate of |v| in feature order (float), then v * (1 / norm) unless norm < FLT_EPSILON
    float norm = 0.f;
    if (l == 0)
        for (int j = 0; j < ROPS_LEN; ++j) norm = norm + fabsf(feat[j]);
    norm = __shfl(norm, 0);
    const float inv = norm < FLT_EPSILON ? 1.0f : 1.0f / norm;
    for (int j = l; j < ROPS_LEN; j += 64) out[(size_t) kp * ROPS_LEN + j] = feat[j] * inv;
}

int gravity_frames(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, float* d_out9) {
    LGR_CHECK(ctx, (d_kps || m == 0) && (d_surf || n == 0) && m >= 0 && n >= 0 && radius > 0.f && radius <= 1e18f && (d_out9 || m == 0),
              LGR_ERR_INVALID_ARG);
    if (m == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    float* masked;
    LGR_TRY(lgr_ws_t(ctx, WS_ROPS_MASKED, (size_t) m * 12, &masked));
    gravity_mask_kernel<<<cdiv((long long) m * 12, 256), 256, 0, ctx->stream>>>(d_kps, m, masked);
    LGR_HIP(ctx, hipGetLastError());
    // the failing key points' SHOT frames (SHOTLocalReferenceFrameEstimation on the same surface and radius); NaN for the others
    LGR_TRY(lgr_shot_lrf_dev(ctx, masked, m, d_surf, n, radius, d_out9));
    gravity_frame_kernel<<<cdiv(m, 256), 256, 0, ctx->stream>>>(d_kps, m, d_out9);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

int rops_rows(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, const float* d_lrf, float* d_out) {
    LGR_CHECK(ctx, (d_kps || m == 0) && (d_surf || n == 0) && m >= 0 && n >= 0 && radius > 0.f && radius <= 1e18f && (d_lrf || m == 0) &&
                   (d_out || m == 0), LGR_ERR_INVALID_ARG);
    if (m == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    GridDev g;
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_B, d_surf, n, radius * 1.001f, 0.f, &g));
    rops_kernel<<<m, 64, 0, ctx->stream>>>(g, d_kps, m, radius, d_lrf, d_out);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

}  // namespace

extern "C" int lgr_gravity_lrf_dev(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, float* d_out9) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return gravity_frames(ctx, d_kps, m, d_surf, n, radius, d_out9);
}

extern "C" int lgr_rops_dev(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, const float* d_lrf, float* d_out135) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return rops_rows(ctx, d_kps, m, d_surf, n, radius, d_lrf, d_out135);
}

// the pipeline's RoPS stage: gravity frames (in the WS_ROPS_LRF workspace), then the rows on them
int lgr_rops_gravity_dev(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, float* d_out135) {
    if (m == 0) return LGR_OK;
    float* fr;
    LGR_TRY(lgr_ws_t(ctx, WS_ROPS_LRF, (size_t) m * 9, &fr));
    LGR_TRY(gravity_frames(ctx, d_kps, m, d_surf, n, radius, fr));
    return rops_rows(ctx, d_kps, m, d_surf, n, radius, fr, d_out135);
}

// host entry points: upload, run the device path, download
extern "C" int lgr_gravity_lrf(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, float* out9) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (kps || m == 0) && (surf || n == 0) && (out9 || m == 0) && m >= 0 && n >= 0, LGR_ERR_INVALID_ARG);
    if (m == 0) return LGR_OK;
    float *dk, *ds, *dl;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(kps, (size_t) m * 12, &dk));
    LGR_TRY(hc.in(surf, (size_t) n * 12, &ds, LGR_PAD_CLOUD));
    LGR_TRY(hc.out((size_t) m * 9, &dl));
    LGR_TRY(gravity_frames(ctx, dk, m, ds, n, radius, dl));
    LGR_TRY(hc.fetch(out9, dl, (size_t) m * 9));
    return hc.finish();
}

extern "C" int lgr_rops(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, const float* lrf, float* out135) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (kps || m == 0) && (surf || n == 0) && (lrf || m == 0) && (out135 || m == 0) && m >= 0 && n >= 0, LGR_ERR_INVALID_ARG);
    if (m == 0) return LGR_OK;
    float *dk, *ds, *dl, *dout;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(kps, (size_t) m * 12, &dk));
    LGR_TRY(hc.in(surf, (size_t) n * 12, &ds, LGR_PAD_CLOUD));
    LGR_TRY(hc.in(lrf, (size_t) m * 9, &dl));
    LGR_TRY(hc.out((size_t) m * ROPS_LEN, &dout));
    LGR_TRY(rops_rows(ctx, dk, m, ds, n, radius, dl, dout));
    LGR_TRY(hc.fetch(out135, dout, (size_t) m * ROPS_LEN));
    return hc.finish();
}
