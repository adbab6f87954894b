// lgr_shot.hip -- the SHOT352 descriptor: local reference frames and histograms (its matcher is lgr_match_dense.hip).
//
//   pcl::SHOTLocalReferenceFrameEstimation::getLocalRF [3P, PCL 1.12.1]           -> lgr_shot_lrf*
//   include/common.h estimateFeatures<SHOT> = SHOTEstimationOMP<PointXYZINormal, PointXYZINormal, SHOT352>
//     (the interpolation as src/pcl/shot_debug.cpp states it)                      -> lgr_shot*
// Canonical choices: neighbours in ascending (d2, index) order; the eigen-solver, acos and atan2 of
// lgr_shot_math.h; tests/cpp/shot_ref.cpp states the same sequences on the CPU and the -m gpu tests compare bit for bit.
#include <cfloat>
#include <cmath>

#include "lgr_grid.cuh"
#include "lgr_host.h"
#include "lgr_shot_math.h"

namespace {

constexpr int SHOT_LEN = 352;         // 32 volumes x 11 slots
constexpr int SHOT_BINS = 10;         // nr_shape_bins_
constexpr int SHOT_CAP = 1024;        // neighbours gathered and sorted at once; more are processed in shells of ascending keys

// Eigen Vector4f::dot with SSE packets: (p0 + p2) + (p1 + p3); the fourth coordinates are 0 here, so p3 = +0
__device__ __forceinline__ float dot4f(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (a0 * b0 + a2 * b2) + (a1 * b1 + 0.f);
}
// a row of Eigen::Matrix<double, Dynamic, 4> (strided: no packets) dot Vector4d: unrolled halves (p0 + p1) + (p2 + p3), p3 = +0
__device__ __forceinline__ double dot4d(double a0, double a1, double a2, double b0, double b1, double b2) {
    return (a0 * b0 + a1 * b1) + (a2 * b2 + 0.0);
}

__device__ void sort_keys(unsigned long long* skey, unsigned* spos, int cnt, int l) {
    int n_pad = 64;
    while (n_pad < cnt) n_pad <<= 1;
    for (int q = cnt + l; q < n_pad; q += 64) { skey[q] = ~0ull; spos[q] = 0u; }
    __syncthreads();
    for (int k2 = 2; k2 <= n_pad; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int q = l; q < (n_pad >> 1); q += 64) {
                const int i0 = ((q & ~(j - 1)) << 1) | (q & (j - 1)), i1 = i0 | j;
                const unsigned long long ka = skey[i0], kb = skey[i1];
                if ((ka > kb) == ((i0 & k2) == 0)) {
                    skey[i0] = kb; skey[i1] = ka;
                    const unsigned pa = spos[i0]; spos[i0] = spos[i1]; spos[i1] = pa;
                }
            }
            __syncthreads();
        }
}

// One wave per key point.  The neighbours (d2 < r2 on the surface grid) are gathered as (bits(d2) << 32 | original index, sorted position)
// and sorted ascending; a key point with more than SHOT_CAP of them is walked in shells of ascending key ranges, once per pass.
//   pass A  covariance of the frame: lanes 0..5 own one entry of C, lane 6 the weight sum, neighbour after neighbour (double);
//   pass B  sign disambiguation: counts over the valid neighbours and the five around the median position;
//   pass C  (desc != NULL) the histogram: every lane computes the <= 5 (slot, value) pairs of one neighbour, then the pairs are added
//           neighbour after neighbour (the slots of one neighbour are distinct), so every slot receives its float adds in neighbour order.
// lrf_in != NULL: its frames are used (pass A / B skipped).
__global__ __launch_bounds__(64) void shot_kernel(GridDev g, const float* __restrict__ kps, int m, float radius, const float* __restrict__ lrf_in,
                                                  float* __restrict__ lrf_out, float* __restrict__ desc_out) {
    __shared__ unsigned long long skey[SHOT_CAP];
    __shared__ unsigned spos[SHOT_CAP];
    __shared__ double sv[4][64];
    __shared__ int sflag[64];
    __shared__ int hslot[64 * 5];
    __shared__ float hval[64 * 5];
    __shared__ float hist[SHOT_LEN];
    const int l = threadIdx.x;
    const int kp = blockIdx.x;
    if (kp >= m) return;
    const float nanv = __uint_as_float(0x7fc00000u);
    const float x = kps[(size_t) kp * 12], y = kps[(size_t) kp * 12 + 1], z = kps[(size_t) kp * 12 + 2];
    const float r2 = radius * radius;
    const double rd = (double) radius;
    auto nan_out = [&](bool frame_too) {
        if (desc_out) for (int j = l; j < SHOT_LEN; j += 64) desc_out[(size_t) kp * SHOT_LEN + j] = nanv;
        if (lrf_out && frame_too && l < 9) lrf_out[(size_t) kp * 9 + l] = nanv;
    };
    if (!lgr_finite3(x, y, z)) { nan_out(true); return; }
    const int cx = min(max(lgr_cellc(x, g.ox, g.h), 0), g.dx - 1), cy = min(max(lgr_cellc(y, g.oy, g.h), 0), g.dy - 1), cz = min(max(lgr_cellc(z, g.oz, g.h), 0), g.dz - 1);
    const unsigned long long key_end = (unsigned long long) __float_as_uint(r2) << 32;
    auto scan = [&](unsigned long long lo, unsigned long long hi, bool store) -> int {
        int cnt = 0;
        for (int zz = max(cz - 1, 0); zz <= min(cz + 1, g.dz - 1); ++zz)
            for (int yy = max(cy - 1, 0); yy <= min(cy + 1, g.dy - 1); ++yy) {
                const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dx - 1);
                const size_t c0 = ((size_t) zz * g.dy + yy) * g.dx;
                const int b = g.cell_start[c0 + x0], e = g.cell_start[c0 + x1 + 1];
                for (int t0 = b; t0 < e; t0 += 64) {
                    const int t = t0 + l;
                    bool in = false;
                    unsigned long long key = 0ull;
                    if (t < e) {
                        const float4 P = g.pxyz[t];
                        const float d2 = lgr_dist2(x, y, z, P.x, P.y, P.z);
                        key = ((unsigned long long) __float_as_uint(d2) << 32) | (unsigned) __float_as_int(P.w);
                        in = d2 < r2 && key >= lo && key < hi;
                    }
                    const unsigned long long bm = __ballot(in);
                    if (bm == 0ull) continue;
                    if (store && in) {
                        const int slot = cnt + __builtin_amdgcn_mbcnt_hi((unsigned) (bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) bm, 0u));
                        if (slot < SHOT_CAP) { skey[slot] = key; spos[slot] = (unsigned) t; }
                    }
                    cnt += __popcll(bm);
                }
            }
        return cnt;
    };
    const int total = g.n ? scan(0ull, key_end, true) : 0;   // (an empty surface: no neighbours)
    const bool single = total <= SHOT_CAP;
    if (single) sort_keys(skey, spos, total, l);
    // f(cnt) sees skey / spos [0, cnt) sorted: the next cnt neighbours in ascending order
    auto for_each_shell = [&](auto&& f) {
        if (single) { f(total); return; }
        unsigned long long lo = 0ull;
        while (lo < key_end) {
            unsigned long long hi = key_end;
            __syncthreads();
            int cnt = scan(lo, hi, false);
            if (cnt > SHOT_CAP) {
                unsigned long long a = lo, bnd = hi;   // count(lo, a) <= SHOT_CAP < count(lo, bnd)
                for (;;) {
                    const unsigned long long mid = a + ((bnd - a) >> 1);
                    const int c = scan(lo, mid, false);
                    if (c > SHOT_CAP) bnd = mid;
                    else { a = mid; if (c >= SHOT_CAP / 4 || bnd - a <= 1ull) break; }
                }
                hi = a;
            }
            __syncthreads();
            cnt = scan(lo, hi, true);
            sort_keys(skey, spos, cnt, l);
            f(cnt);
            lo = hi;
        }
    };

    float fx[3], fy[3], fz[3];   // the frame's rows (float)
    if (lrf_in) {
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            fx[a] = lrf_in[(size_t) kp * 9 + a]; fy[a] = lrf_in[(size_t) kp * 9 + 3 + a]; fz[a] = lrf_in[(size_t) kp * 9 + 6 + a];
            ok = ok && lgr_finite3(fx[a], fy[a], fz[a]);
        }
        if (!ok) { nan_out(true); return; }
    } else {
        // ---- pass A: C += w v v^T, sum w += w (double, neighbour order); v = (q - p) in float, w = r - sqrt((double) d2); q == p skipped
        double cacc = 0.0;
        int n_valid = 0;
        const int ca = l < 3 ? 0 : (l < 5 ? 1 : 2), cb = l < 3 ? l : (l < 5 ? l - 2 : 2);   // lanes 0..5: xx xy xz yy yz zz
        for_each_shell([&](int cnt) {
            for (int c0 = 0; c0 < cnt; c0 += 64) {
                const int q = c0 + l;
                int valid = 0;
                if (q < cnt) {
                    const float4 P = g.pxyz[spos[q]];
                    const float d2 = __uint_as_float((unsigned) (skey[q] >> 32));
                    valid = !(P.x == x && P.y == y && P.z == z);
                    sv[0][l] = (double) (P.x - x); sv[1][l] = (double) (P.y - y); sv[2][l] = (double) (P.z - z);
                    sv[3][l] = rd - sqrt((double) d2);
                }
                sflag[l] = valid;
                __syncthreads();
                const int nq = min(64, cnt - c0);
                for (int j = 0; j < nq; ++j) {
                    if (!sflag[j]) continue;
                    if (l < 6) cacc += sv[3][j] * (sv[ca][j] * sv[cb][j]);
                    else if (l == 6) cacc += sv[3][j];
                }
                n_valid += __popcll(__ballot(q < cnt && valid));
                __syncthreads();
            }
        });
        if (n_valid < 5) { nan_out(true); return; }
        const double sw = __shfl(cacc, 6);
        double A[9];
        A[0] = __shfl(cacc, 0) / sw; A[1] = __shfl(cacc, 1) / sw; A[2] = __shfl(cacc, 2) / sw;
        A[4] = __shfl(cacc, 3) / sw; A[5] = __shfl(cacc, 4) / sw; A[8] = __shfl(cacc, 5) / sw;
        A[3] = A[1]; A[6] = A[2]; A[7] = A[5];
        double w[3], V[9];
        shot_eigen3(A, w, V);
        if (!(isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]))) { nan_out(true); return; }
        int lo_i, hi_i;
        shot_extremes(w, &lo_i, &hi_i);
        double v1[3], v3[3];
        for (int r = 0; r < 3; ++r) {   // (selects, not a run-time index into V: that would live in scratch)
            v1[r] = hi_i == 0 ? V[3 * r] : (hi_i == 1 ? V[3 * r + 1] : V[3 * r + 2]);
            v3[r] = lo_i == 0 ? V[3 * r] : (lo_i == 1 ? V[3 * r + 1] : V[3 * r + 2]);
        }
        // ---- pass B: s = 2 #{v.a >= 0} - n; s == 0: + #{v.a > 0} over valid positions n/2 - 2 .. n/2 + 2; flip when < 0
        const int med = n_valid / 2;
        int plus1 = 0, plus3 = 0, tie1 = 0, tie3 = 0, vbase = 0;
        const double v10 = v1[0], v11 = v1[1], v12 = v1[2], v30 = v3[0], v31 = v3[1], v32 = v3[2];
        for_each_shell([&](int cnt) {
            for (int c0 = 0; c0 < cnt; c0 += 64) {
                const int q = c0 + l;
                bool valid = false;
                double d1 = 0.0, d3 = 0.0;
                if (q < cnt) {
                    const float4 P = g.pxyz[spos[q]];
                    valid = !(P.x == x && P.y == y && P.z == z);
                    const double vx = (double) (P.x - x), vy = (double) (P.y - y), vz = (double) (P.z - z);
                    d1 = dot4d(vx, vy, vz, v10, v11, v12);
                    d3 = dot4d(vx, vy, vz, v30, v31, v32);
                }
                const unsigned long long vm = __ballot(valid);
                const int pos = vbase + __builtin_amdgcn_mbcnt_hi((unsigned) (vm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) vm, 0u));
                const bool win = valid && pos >= med - 2 && pos <= med + 2;
                plus1 += __popcll(__ballot(valid && d1 >= 0.0));
                plus3 += __popcll(__ballot(valid && d3 >= 0.0));
                tie1 += __popcll(__ballot(win && d1 > 0.0));
                tie3 += __popcll(__ballot(win && d3 > 0.0));
                vbase += __popcll(vm);
            }
        });
        int s1 = 2 * plus1 - n_valid, s3 = 2 * plus3 - n_valid;
        if (s1 == 0) s1 += tie1;
        if (s3 == 0) s3 += tie3;
        if (s1 < 0) for (int a = 0; a < 3; ++a) v1[a] = -v1[a];
        if (s3 < 0) for (int a = 0; a < 3; ++a) v3[a] = -v3[a];
        for (int a = 0; a < 3; ++a) { fx[a] = (float) v1[a]; fz[a] = (float) v3[a]; }
        // y = z x x (float, Eigen's generic cross)
        fy[0] = fz[1] * fx[2] - fz[2] * fx[1];
        fy[1] = fz[2] * fx[0] - fz[0] * fx[2];
        fy[2] = fz[0] * fx[1] - fz[1] * fx[0];
    }
    if (lrf_out && l < 9) lrf_out[(size_t) kp * 9 + l] = l < 3 ? fx[l] : (l < 6 ? fy[l - 3] : fz[l - 6]);
    if (!desc_out) return;
    if (total < 5) {   // computePointSHOT: fewer than 5 neighbours (the key point itself included)
        for (int j = l; j < SHOT_LEN; j += 64) desc_out[(size_t) kp * SHOT_LEN + j] = nanv;
        return;
    }
    // ---- pass C: the histogram (the frame as scalars: arrays captured by the pass's lambda would live in scratch memory)
    const float fx0 = fx[0], fx1 = fx[1], fx2 = fx[2], fy0 = fy[0], fy1 = fy[1], fy2 = fy[2], fz0 = fz[0], fz1 = fz[1], fz2 = fz[2];
    const double r1_2 = rd / 2, r1_4 = rd / 4, r3_4 = (rd * 3) / 4;
    const double RAD_45 = 0.78539816339744830961566084581988, RAD_90 = 1.5707963267948966192313216916398,
                 RAD_135 = 2.3561944901923449288469825374596, RAD_PI_7_8 = 2.7488935718910690836548129603691;
    for (int j = l; j < SHOT_LEN; j += 64) hist[j] = 0.f;
    __syncthreads();
    for_each_shell([&](int cnt) {
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int q = c0 + l;
            int sl0 = -1, sl1 = -1, sl2 = -1, sl3 = -1, sl4 = -1;   // (scalars: a per-lane array would live in scratch memory)
            float vl0 = 0.f, vl1 = 0.f, vl2 = 0.f, vl3 = 0.f, vl4 = 0.f;
            if (q < cnt) {
                const unsigned pos = spos[q];
                const float4 P = g.pxyz[pos];
                const float4 N = g.pnrm[pos];
                const float d2 = __uint_as_float((unsigned) (skey[q] >> 32));
                const double distance = sqrt((double) d2);
                if (lgr_finite3(N.x, N.y, N.z) && !(fabs(distance) < 1e-15)) {
                    double cosd = (double) dot4f(N.x, N.y, N.z, fz0, fz1, fz2);
                    if (cosd > 1.0) cosd = 1.0;
                    if (cosd < -1.0) cosd = -1.0;
                    double bd = ((1.0 + cosd) * SHOT_BINS) / 2;
                    const float dx = P.x - x, dy = P.y - y, dz = P.z - z;
                    double xr = (double) dot4f(dx, dy, dz, fx0, fx1, fx2);
                    double yr = (double) dot4f(dx, dy, dz, fy0, fy1, fy2);
                    double zr = (double) dot4f(dx, dy, dz, fz0, fz1, fz2);
                    if (fabs(yr) < 1e-30) yr = 0;
                    if (fabs(xr) < 1e-30) xr = 0;
                    if (fabs(zr) < 1e-30) zr = 0;
                    const int bit4 = ((yr > 0) || ((yr == 0.0) && (xr < 0))) ? 1 : 0;
                    const int bit3 = ((xr > 0) || ((xr == 0.0) && (yr > 0))) ? !bit4 : bit4;
                    int desc = ((bit4 << 3) + (bit3 << 2)) << 1;
                    if ((xr * yr > 0) || (xr == 0.0)) desc += (fabs(xr) >= fabs(yr)) ? 0 : 4;
                    else desc += (fabs(xr) > fabs(yr)) ? 4 : 0;
                    desc += zr > 0 ? 1 : 0;
                    desc += (distance > r1_2) ? 2 : 0;
                    const int step = (int) floor(bd + 0.5);
                    const int vol = desc * (SHOT_BINS + 1);
                    bd -= step;
                    double iw = 1 - fabs(bd);
                    if (bd > 0) { sl0 = vol + ((step + 1) % SHOT_BINS); vl0 = (float) bd; }
                    else { sl0 = vol + ((step - 1 + SHOT_BINS) % SHOT_BINS); vl0 = -(float) bd; }
                    if (distance > r1_2) {
                        const double rdist = (distance - r3_4) / r1_2;
                        if (distance > r3_4) iw += 1 - rdist;
                        else { iw += 1 + rdist; sl1 = (desc - 2) * (SHOT_BINS + 1) + step; vl1 = -(float) rdist; }
                    } else {
                        const double rdist = (distance - r1_4) / r1_2;
                        if (distance < r1_4) iw += 1 + rdist;
                        else { iw += 1 - rdist; sl1 = (desc + 2) * (SHOT_BINS + 1) + step; vl1 = (float) rdist; }
                    }
                    double ic = zr / distance;
                    if (ic < -1.0) ic = -1.0;
                    if (ic > 1.0) ic = 1.0;
                    const double incl = shot_acos(ic);
                    if (incl > RAD_90 || (fabs(incl - RAD_90) < 1e-30 && zr <= 0)) {
                        const double idist = (incl - RAD_135) / RAD_90;
                        if (incl > RAD_135) iw += 1 - idist;
                        else { iw += 1 + idist; sl2 = (desc + 1) * (SHOT_BINS + 1) + step; vl2 = -(float) idist; }
                    } else {
                        const double idist = (incl - RAD_45) / RAD_90;
                        if (incl < RAD_45) iw += 1 + idist;
                        else { iw += 1 - idist; sl2 = (desc - 1) * (SHOT_BINS + 1) + step; vl2 = (float) idist; }
                    }
                    if (yr != 0.0 || xr != 0.0) {
                        const double az = shot_atan2(yr, xr);
                        const int sel = desc >> 2;
                        double adist = (az - (-RAD_PI_7_8 + RAD_45 * sel)) / RAD_45;
                        adist = fmax(-0.5, fmin(adist, 0.5));   // (std::max)(-0.5, std::min(adist, 0.5)): adist is finite here
                        if (adist > 0) {
                            iw += 1 - adist;
                            sl3 = ((desc + 4) % 32) * (SHOT_BINS + 1) + step; vl3 = (float) adist;
                        } else {
                            sl3 = ((desc - 4 + 32) % 32) * (SHOT_BINS + 1) + step;
                            iw += 1 + adist;
                            vl3 = -(float) adist;
                        }
                    }
                    sl4 = vol + step; vl4 = (float) iw;
                }
            }
            hslot[5 * l] = sl0; hslot[5 * l + 1] = sl1; hslot[5 * l + 2] = sl2; hslot[5 * l + 3] = sl3; hslot[5 * l + 4] = sl4;
            hval[5 * l] = vl0; hval[5 * l + 1] = vl1; hval[5 * l + 2] = vl2; hval[5 * l + 3] = vl3; hval[5 * l + 4] = vl4;
            __syncthreads();
            const int nq = min(64, cnt - c0);
            for (int j = 0; j < nq; ++j) {
                if (l < 5) {
                    const int s = hslot[5 * j + l];
                    if ((unsigned) s < (unsigned) SHOT_LEN) hist[s] += hval[5 * j + l];
                }
                __syncthreads();
            }
        }
    });
    // normalizeHistogram: acc += shot[j] * shot[j] (float product, double sum, slot order); shot[j] /= (float) sqrt(acc)
    double acc = 0.0;
    if (l == 0)
        for (int j = 0; j < SHOT_LEN; ++j) { const float h = hist[j]; acc += (double) (h * h); }
    const float nrm = (float) sqrt(__shfl(acc, 0));
    for (int j = l; j < SHOT_LEN; j += 64) desc_out[(size_t) kp * SHOT_LEN + j] = hist[j] / nrm;
}

int shot_features(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, const float* d_lrf_in, float* d_out, float* d_lrf_out) {
    LGR_CHECK(ctx, (d_kps || m == 0) && (d_surf || n == 0) && m >= 0 && n >= 0 && radius > 0.f && radius <= 1e18f, LGR_ERR_INVALID_ARG);
    if (m == 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    GridDev g;
    LGR_TRY(lgr_grid_build(ctx, WS_GRID_B, d_surf, n, radius * 1.001f, 0.f, &g));
    shot_kernel<<<m, 64, 0, ctx->stream>>>(g, d_kps, m, radius, d_lrf_in, d_lrf_out, d_out);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

}  // namespace

extern "C" int lgr_shot_lrf_dev(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, float* d_out9) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_out9 || m == 0, LGR_ERR_INVALID_ARG);
    return shot_features(ctx, d_kps, m, d_surf, n, radius, nullptr, nullptr, d_out9);
}

extern "C" int lgr_shot_dev(lgr_ctx* ctx, const float* d_kps, int m, const float* d_surf, int n, float radius, const float* d_lrf,
                            float* d_out352, float* d_out_lrf) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_out352 || m == 0, LGR_ERR_INVALID_ARG);
    return shot_features(ctx, d_kps, m, d_surf, n, radius, d_lrf, d_out352, d_out_lrf);
}

// host entry points: upload, run the device path, download
static int shot_staged(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, const float* lrf, float* out352, float* out_lrf) {
    LGR_CHECK(ctx, (kps || m == 0) && (surf || n == 0) && m >= 0 && n >= 0, LGR_ERR_INVALID_ARG);
    if (m == 0) return LGR_OK;
    float *dk, *ds, *dl = nullptr, *dout = nullptr, *dlo = nullptr;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(kps, (size_t) m * 12, &dk));
    LGR_TRY(hc.in(surf, (size_t) n * 12, &ds, LGR_PAD_CLOUD));
    if (lrf) LGR_TRY(hc.in(lrf, (size_t) m * 9, &dl));   // (no frames stay null: they are then estimated)
    if (out352) LGR_TRY(hc.out((size_t) m * SHOT_LEN, &dout));
    if (out_lrf) LGR_TRY(hc.out((size_t) m * 9, &dlo));
    LGR_TRY(shot_features(ctx, dk, m, ds, n, radius, dl, dout, dlo));
    LGR_TRY(hc.fetch(out352, dout, (size_t) m * SHOT_LEN));
    LGR_TRY(hc.fetch(out_lrf, dlo, (size_t) m * 9));
    return hc.finish();
}

extern "C" int lgr_shot_lrf(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, float* out9) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, out9 || m == 0, LGR_ERR_INVALID_ARG);
    return shot_staged(ctx, kps, m, surf, n, radius, nullptr, nullptr, out9);
}

extern "C" int lgr_shot(lgr_ctx* ctx, const float* kps, int m, const float* surf, int n, float radius, const float* lrf, float* out352, float* out_lrf) {
    lgr_turn turn__(ctx);
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, out352 || m == 0, LGR_ERR_INVALID_ARG);
    return shot_staged(ctx, kps, m, surf, n, radius, lrf, out352, out_lrf);
}
