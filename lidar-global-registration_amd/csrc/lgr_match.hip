// lgr_match.hip -- brute-force FPFH matching (both directions from one MFMA pass) for gfx950.
//
// Replaces include/matching.h:594-634 matchBF<FPFH> (cv::BFMatcher(NORM_L2)::knnMatch, k = 1) and the cross-block
// merge src/common.cpp:517-529.  Result contract (bit-exact with the oracle): for every valid query row, the train
// row minimising the CANONICAL distance d = sqrtf(normL2Sqr) -- OpenCV 4.5.1 SSE lane order, see exact_l2() -- with
// ties broken "highest bf block, then lowest index inside the block"; NaN rows never match.
//
// Structure (DESIGN.md "matcher"):
//   1. cluster      : 16 k-means centres of the descriptors (Lloyd on a sample, on the device); every row is assigned
//                     to its nearest centre and both sets are sorted by (cluster, leaf, distance to the cluster centre) -- the
//                     last key makes every 32 / 128 / 256-row piece of a leaf a thin radial shell about that centre, which
//                     the skipping passes use as a second lower bound (| |a - c| - |b - c| | <= |a - b|: mask_kernel, match_mfma).
//   2. pack         : MFMA operands, K = 34: A' = [-2(a - c_p), 1] for a in cluster p, and one column set per cluster,
//                     B'(p) = [b - c_p, |b - c_p|^2].  Distances are translation invariant, so for a row of cluster p
//                     S = A'.B'(p) = |b - c_p|^2 - 2 (a - c_p).(b - c_p) = d2 - |a - c_p|^2 -- and its rounding error
//                     scales with (|a - c_p| + |b - c_p|)^2, i.e. it is tiny exactly for the near pairs that matter
//                     (FPFH data is full of near-duplicate "flat surface" rows far from the global mean).
//   3. match_mfma   : the brute-force contraction on v_mfma_f32_32x32x2_f32 with a fused epilogue that keeps only
//                     min_b d2~ per (row, column group) and min_a d2~ per (column, row group), d2~ = S + |a'|^2.
//                     FILTER only.  (f16 formats, the default: two-term f16 splits of the operands on v_mfma_f32_32x32x16_f16,
//                     K = 96 or 112, under the same kind of proven bound; bound-based tile skipping in masked passes: section 3b.)
//   4. rerank_*     : per query, a group is a candidate when its lower bound (value - proven error) does not exceed
//                     the smallest upper bound; candidate groups are rescanned with the exact canonical distance and
//                     a packed 64-bit atomicMin applies the reference's tie rules (order independent).
// Host side: match_impl is the list of a call's stages; every stage is a member of MatchCall, the call's explicit state (inputs, both
// Sides, derived sizes, operand format and scales, tables, streams).  Beside it: Fork (a helper stream with its fork / record / join
// state; the table of the matcher's events stands above it), operand_scale / coarse_constants (the host arithmetic behind every bound, as
// pure functions), PruneWs (the typed layout of the pruning workspace), launch_match_mfma (the one place that names the match_mfma
// instantiations), CheckView (what the self-check reads).  The LGR_MATCH_DEBUG report and the EXP_PROF read-out: lgr_match_debug.cuh.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <vector>

#include "lgr_host.h"
#include "lgr_internal.h"

#include "lgr_match_common.cuh"
#include "lgr_match_cluster.cuh"
#include "lgr_match_pack.cuh"
#include "lgr_match_mfma.cuh"
#include "lgr_match_sweep.cuh"
#include "lgr_match_bounds.cuh"
#include "lgr_match_rerank.cuh"

// diagnostics of a context's last match call (lgr_match_stats / mcheck live in the context: two contexts driven from one host thread
// keep separate figures, and the helper thread of the second rerank direction writes into the same object as the caller)
extern "C" int lgr_match_last_stats(lgr_ctx* ctx, unsigned* out6) {
    if (!ctx || !out6) return LGR_ERR_INVALID_ARG;
    const lgr_match_stats& s = ctx->mstats;
    out6[0] = s.items_ab; out6[1] = s.dense_ab; out6[2] = s.items_ba;
    out6[3] = s.dense_ba; out6[4] = (unsigned) s.sub_cols; out6[5] = (unsigned) s.rg_rows;
    return LGR_OK;
}
// fraction of the (row block x column stage) tiles of the last match call that the MFMA passes computed (1 = dense): every (row block,
// stage) counted ONCE, however many passes touched it (a stage that straddles two leaves is computed whole by each pass that schedules
// one of them) -- never above 1
extern "C" int lgr_match_last_work(lgr_ctx* ctx, double* executed_fraction) {
    if (!ctx || !executed_fraction) return LGR_ERR_INVALID_ARG;
    *executed_fraction = ctx->mstats.stages_all > 0 ? ctx->mstats.stages_unique / ctx->mstats.stages_all : 1.0;
    return LGR_OK;
}
// the same with every pass's stages summed: the work that was ISSUED (what the bench prices MFMA FLOP with); >= lgr_match_last_work
// out2[1]: the same as a number of (row, column) element pairs of the PADDED operands (stages x 256 rows x 128 columns) -- what the MFMA
// FLOP count is made of (clusters are padded to whole row blocks / column tiles: a few per cent more than Mq x Mt)
extern "C" int lgr_match_last_issued(lgr_ctx* ctx, double* out2) {
    if (!ctx || !out2) return LGR_ERR_INVALID_ARG;
    out2[0] = ctx->mstats.stages_all > 0 ? ctx->mstats.stages_done / ctx->mstats.stages_all : 1.0;
    out2[1] = ctx->mstats.stages_done * (double) BLOCK_ROWS * (double) STAGE_COLS;
    return LGR_OK;
}
extern "C" int lgr_match_last_pairs(lgr_ctx* ctx, unsigned* out2) {
    if (!ctx || !out2) return LGR_ERR_INVALID_ARG;
    out2[0] = ctx->mstats.pairs_ab; out2[1] = ctx->mstats.pairs_ba;
    return LGR_OK;
}
extern "C" int lgr_match_last_shell(lgr_ctx* ctx, double* tiles_skipped) {
    if (!ctx || !tiles_skipped) return LGR_ERR_INVALID_ARG;
    *tiles_skipped = ctx->mstats.shell_skipped;
    return LGR_OK;
}
// (row block, leaf) pairs of the last pruned match call whose lower bound is zero -- never excludable -- and pairs with a finite bound at all:
// what lgr_match_options.auto_dense decides on
extern "C" int lgr_match_last_lbstats(lgr_ctx* ctx, double* out2) {
    if (!ctx || !out2) return LGR_ERR_INVALID_ARG;
    out2[0] = ctx->mstats.lb_zero; out2[1] = ctx->mstats.lb_finite;
    return LGR_OK;
}
// irregular rows of the last match call that went through the exact side scan: [query side, train side, 1 = the lane gave up]
extern "C" int lgr_match_last_irregular(lgr_ctx* ctx, unsigned* out3) {
    if (!ctx || !out3) return LGR_ERR_INVALID_ARG;
    out3[0] = ctx->mstats.irr_a; out3[1] = ctx->mstats.irr_b; out3[2] = ctx->mstats.irr_gave_up;
    return LGR_OK;
}
extern "C" int lgr_match_last_coarse(lgr_ctx* ctx, double* out2) {
    if (!ctx || !out2) return LGR_ERR_INVALID_ARG;
    out2[0] = ctx->mstats.coarse_tested; out2[1] = ctx->mstats.coarse_rejected;
    return LGR_OK;
}
// MFMA operand format of the last match call: 2 / 1 = f16-split operands on v_mfma_f32_32x32x16_f16 (rotated: 192, plain: 224 FLOP per
// pair), 0 = f32 operands on v_mfma_f32_32x32x2_f32 (68 FLOP per pair)
extern "C" int lgr_match_last_format(lgr_ctx* ctx, int* f16) {
    if (!ctx || !f16) return LGR_ERR_INVALID_ARG;
    *f16 = ctx->mstats.f16;
    return LGR_OK;
}

// lgr_match_options.self_check (tests): worst |filtered - exact| / eps over the sampled table entries of the last call, per direction
// (rows, columns); -1 when the check did not run.  A proven bound: must be <= 1.
extern "C" int lgr_match_last_check(lgr_ctx* ctx, double* out2) {
    if (!ctx || !out2) return LGR_ERR_INVALID_ARG;
    out2[0] = ctx->mcheck[0]; out2[1] = ctx->mcheck[1];
    return LGR_OK;
}

// ... the packing kernel against its reference in the last call: 16-byte pieces of fragments and norms and tile shells compared / differing,
// over the call's packing launches (rows, the 16 column sets, the leaf centres); both ~0 when the check did not run
extern "C" int lgr_match_last_pack_check(lgr_ctx* ctx, unsigned long long* out2) {
    if (!ctx || !out2) return LGR_ERR_INVALID_ARG;
    out2[0] = ctx->mpack[0]; out2[1] = ctx->mpack[1];
    return LGR_OK;
}

// ... and what it covered, rows [0..3] then columns [4..7]: entries checked, entries whose upper side was tested, entries whose upper side
// was waived (coarse rejection), entries with a row guaranteed only through the per-stage column criterion (columns; 0 for rows);
// all ~0 when the check did not run, a direction's four when that direction was not matched.
extern "C" int lgr_match_last_check_cover(lgr_ctx* ctx, unsigned long long* out8) {
    if (!ctx || !out8) return LGR_ERR_INVALID_ARG;
    for (int k = 0; k < 8; ++k) out8[k] = ctx->mcover[k];
    return LGR_OK;
}

// environment: debug dumps only (LGR_MATCH_DEBUG); everything that selects a path is an lgr_match_options field
static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

struct Carve {   // consecutive 256-byte aligned pieces of one allocation
    size_t off = 0;
    char* base = nullptr;   // nullptr: sizes only
    size_t operator()(size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t) 255; return o; }
    template <class T> T* take(size_t bytes) { const size_t o = (*this)(bytes); return base ? (T*) (base + o) : nullptr; }
};

// Orthonormal basis for the box bounds: principal axes of the k-means sample (both sets).  Covariance on the device,
// cyclic Jacobi on the host (33 x 33), rows of V = eigenvectors, mu = sample mean.  box_bounds == 2: raw coordinates.
// `meanwhile` (optional): enqueues other work of the same stream after the covariance has been requested -- the host Jacobi
// (~0.3 ms) then runs while the device executes it instead of leaving the device idle.
template <class F>
static int box_basis(lgr_ctx* ctx, bool raw, const float* smp, const int* smp_ok, int ns, float* d_basis /* [34][33] + 1: V rows, then mu */, F&& meanwhile) {
    std::vector<float> h(34 * 33 + 1, 0.f);
    if (raw) LGR_TRY(meanwhile());
    // The covariance runs on the context's third stream: `meanwhile` (the ~45 short launches of the Lloyd steps, which everything after the
    // clustering waits for) then does not queue behind it.  Prepared ahead of the call, both compete with the other cloud's feature kernels for
    // the device, and the covariance -- 1.6 ms there, in FRONT of the Lloyd chain -- kept the chain on the critical path (round 3 timeline).
    hipStream_t sC = ctx->stream;
    if (!raw) {
        LGR_TRY(lgr_ctx_stream3(ctx, &sC));
        if (sC != ctx->stream) {
            LGR_HIP(ctx, hipEventRecord(ctx->ev[28], ctx->stream));   // (the sample rows come from km_sample on the context's stream)
            LGR_HIP(ctx, hipStreamWaitEvent(sC, ctx->ev[28], 0));
        }
        const int nb = cdiv(ns, COV_ROWS);
        float* part;
        LGR_TRY(lgr_ws_t(ctx, WS_MATCH_DENSE, (size_t) nb * (34 * 33 + 1) + 64, &part));   // scratch: the rerank buffers are not live yet
        LGR_HIP(ctx, hipMemsetAsync(part, 0, (size_t) nb * (34 * 33 + 1) * 4, sC));   // the a > b product slots are never written
        cov_kernel<<<nb, COV_THREADS, 0, sC>>>(smp, smp_ok, ns, part);
        cov_reduce<<<cdiv(34 * 33 + 1, 256), 256, 0, sC>>>(part, nb, d_basis);
        float* hp;
        LGR_TRY(lgr_pinned(ctx, (34 * 33 + 1) * 4, (void**) &hp));
        LGR_HIP(ctx, hipMemcpyAsync(hp, d_basis, (34 * 33 + 1) * 4, hipMemcpyDeviceToHost, sC));
        LGR_HIP(ctx, hipEventRecord(ctx->ev[30], sC));
        const int rc_m = meanwhile();
        LGR_HIP(ctx, hipEventSynchronize(ctx->ev[30]));   // (also when `meanwhile` failed: nothing of this call may stay queued on sC)
        LGR_TRY(rc_m);
        memcpy(h.data(), hp, (34 * 33 + 1) * 4);
    }
    const double n = h[34 * 33];
    std::vector<double> C(33 * 33, 0.0), mu(33, 0.0), Vd(33 * 33, 0.0);
    for (int i = 0; i < 33; ++i) Vd[i * 33 + i] = 1.0;
    if (!raw && n >= 2) {
        for (int k = 0; k < 33; ++k) mu[k] = h[k] / n;
        for (int a = 0; a < 33; ++a)
            for (int b = a; b < 33; ++b) {
                double c = h[33 + a * 33 + b] / n - mu[a] * mu[b];
                C[a * 33 + b] = c; C[b * 33 + a] = c;
            }
        // cyclic Jacobi; rows of Vd become the eigenvectors.  Whatever it converges to, Vd stays a product of plane
        // rotations, i.e. orthonormal -- which is all the bound needs.
        double tr = 0.0;
        for (int i = 0; i < 33; ++i) tr += std::fabs(C[i * 33 + i]);
        for (int sweep = 0; sweep < 12; ++sweep) {
            double off = 0.0;   // converged: the off-diagonal part is at rounding level (more sweeps would only cost host time)
            for (int p = 0; p < 32; ++p)
                for (int q = p + 1; q < 33; ++q) off = std::max(off, std::fabs(C[p * 33 + q]));
            if (off <= 1e-13 * tr) break;
            for (int p = 0; p < 32; ++p)
                for (int q = p + 1; q < 33; ++q) {
                    double apq = C[p * 33 + q];
                    if (std::fabs(apq) < 1e-300) continue;
                    double theta = (C[q * 33 + q] - C[p * 33 + p]) / (2.0 * apq);
                    double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                    double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
                    for (int k = 0; k < 33; ++k) {
                        double ckp = C[k * 33 + p], ckq = C[k * 33 + q];
                        C[k * 33 + p] = c * ckp - sn * ckq; C[k * 33 + q] = sn * ckp + c * ckq;
                    }
                    for (int k = 0; k < 33; ++k) {
                        double cpk = C[p * 33 + k], cqk = C[q * 33 + k];
                        C[p * 33 + k] = c * cpk - sn * cqk; C[q * 33 + k] = sn * cpk + c * cqk;
                    }
                    for (int k = 0; k < 33; ++k) {
                        double vpk = Vd[p * 33 + k], vqk = Vd[q * 33 + k];
                        Vd[p * 33 + k] = c * vpk - sn * vqk; Vd[q * 33 + k] = sn * vpk + c * vqk;
                    }
                }
        }
    }
    for (int i = 0; i < 33 * 33; ++i) h[i] = (float) Vd[i];
    for (int k = 0; k < 33; ++k) h[33 * 33 + k] = (float) mu[k];
    LGR_HIP(ctx, hipMemcpyAsync(d_basis, h.data(), 34 * 33 * 4, hipMemcpyHostToDevice, sC));
    LGR_HIP(ctx, hipStreamSynchronize(sC));   // h goes out of scope; the basis is in place before anything the host enqueues from here on
    return LGR_OK;
}

// Clustering of one call: centres, leaves, the box basis.  lgr_match_prepare (below) computes it from the query side ahead of the
// call, while the train side's descriptors are still being computed; match_impl consumes it.
struct MatchPrep {
    bool armed = false;            // prepared ahead of the call and not yet consumed
    const float* d_a = nullptr;    // what it was prepared for
    int ma = 0, mb = 0;
    bool both = false;
    lgr_match_options mopt{};
    int sub = 1, rg_rows = BLOCK_ROWS, ns = 0;
    float *cen = nullptr, *cen2 = nullptr, *smp = nullptr, *basis = nullptr;   // in WS_MATCH_MISC
    int* smp_ok = nullptr;
    IrrRef* irr = nullptr;         // the block-sum consensus (km_consensus / km_sample), or nullptr: irregular-row lane off
    bool basis_ready = false;
    Side A;
};
static void match_prep_free(void* p) { delete (MatchPrep*) p; }
static MatchPrep* match_prep_of(lgr_ctx* ctx) {
    if (!ctx->match_prep) { ctx->match_prep = new MatchPrep(); ctx->match_prep_free = match_prep_free; }
    return (MatchPrep*) ctx->match_prep;
}

// ---- 1. k-means centres on a sample: KCL clusters, then `sub` leaves inside every cluster; the basis of the box bounds from the
// same sample.  d_b == nullptr: the train side does not exist yet, the sample comes from the query side alone (any centres are
// valid; the two sides of a registration pair are scans of the same scene).  basis_side_by_side: covariance + host Jacobi on the
// second context while the Lloyd steps run on this one (only when the second context is free).
static int match_cluster(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, bool both, bool basis_side_by_side, MatchPrep* P) {
    const lgr_match_options& mo = ctx->mopt;
    // leaves per cluster: about 1024 rows per leaf on the larger side.  lgr_match_options (ctx->mopt: leaves / prune / near)
    // override the automatic choices (tests force the skipping path on small inputs); results never depend on them.
    int sub = 1;
    while (sub < SUBMAX && (long long) KCL * sub * 1024 < std::max(ma, mb)) sub *= 2;
    if (mo.leaves > 0) sub = mo.leaves;
    sub = std::min(SUBMAX, std::max(1, sub));
    const int n_leaves = KCL * sub;
    const int ns = 2 * KM_SAMPLE;
    char* misc;
    Carve carve{8192};
    const size_t o_cen2 = carve((size_t) MAXLEAF * 33 * 4);
    const size_t o_smp = carve((size_t) ns * 33 * 4), o_ok = carve((size_t) ns * 4), o_label = carve((size_t) ns * 4);
    const size_t o_cbuf = carve((size_t) 2 * KCL * 33 * 4), o_basis = carve((size_t) (34 * 33 + 64) * 4);
    const size_t o_skeys = carve((size_t) 2 * ns * 4), o_svals = carve((size_t) ns * 4), o_sidx = carve((size_t) ns * 4), o_coff = carve(256);
    const size_t o_zero = carve.off;   // zeroed once per call: largest sample magnitude, one set of level-1 sums per Lloyd step, the level-2 sums
    const size_t o_kmax = carve(256), o_irr = carve(sizeof(IrrRef)), o_acc1 = carve((size_t) KM_ITERS * KCL * sizeof(KmAcc)), o_acc2 = carve((size_t) MAXLEAF * sizeof(KmAcc));
    const size_t zero_bytes = carve.off - o_zero;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_MISC, carve.off, &misc));
    float* cen = (float*) (misc + 256);                 // [KCL][33]
    float* cen2 = (float*) (misc + o_cen2);             // [n_leaves][33]
    float* smp = (float*) (misc + o_smp);
    int* smp_ok = (int*) (misc + o_ok);
    int* label = (int*) (misc + o_label);
    float* cbuf = (float*) (misc + o_cbuf);             // two scratch copies of the level-1 centres (read one, write the other)
    float* basis = (float*) (misc + o_basis);           // V [33][33], mu [33], count; + 8: rmax2
    unsigned* skeys = (unsigned*) (misc + o_skeys);      // [2][ns]: level-1 labels as sort keys, sorted copy
    int* svals = (int*) (misc + o_svals);
    int* sidx = (int*) (misc + o_sidx);                  // sample indices in cluster order
    int* coff = (int*) (misc + o_coff);                  // [KCL + 1]
    unsigned* kmax = (unsigned*) (misc + o_kmax);
    KmAcc* acc1 = (KmAcc*) (misc + o_acc1);
    KmAcc* acc2 = (KmAcc*) (misc + o_acc2);
    LGR_HIP(ctx, hipMemsetAsync(misc + o_zero, 0, zero_bytes, ctx->stream));
    // irregular rows: a vote over the sample rows finds the consensus of the block sums; km_sample leaves rows off it out of the sample
    IrrRef* irr = mo.irregular_rows ? (IrrRef*) (misc + o_irr) : nullptr;
    if (irr) km_consensus<<<cdiv(ns, 256), 256, 0, ctx->stream>>>(d_a, ma, d_b, mb, KM_SAMPLE, irr);
    km_sample<<<cdiv(ns, 256), 256, 0, ctx->stream>>>(d_a, ma, d_b, mb, KM_SAMPLE, smp, smp_ok, kmax, irr);
    auto lloyd = [&](lgr_ctx* cx) -> int {
        km_init<<<1, 64, 0, cx->stream>>>(smp, smp_ok, ns, cbuf);
        for (int it = 0; it <= KM_ITERS; ++it) {   // Lloyd with order-free integer sums; the last launch labels with the final centres
            const bool last = it == KM_ITERS;
            km1_step<<<cdiv(ns, KM1_THREADS), KM1_THREADS, 0, cx->stream>>>(smp, smp_ok, ns, kmax, cbuf + (it & 1) * KCL * 33, it ? acc1 + (size_t) (it - 1) * KCL : nullptr,
                                                                            last ? nullptr : acc1 + (size_t) it * KCL, last ? cen : cbuf + ((it + 1) & 1) * KCL * 33, label);
        }
        // the samples in cluster order (stable: sample order inside a cluster)
        km_label_keys<<<cdiv(ns, 256), 256, 0, cx->stream>>>(label, ns, skeys, svals);
        LGR_TRY(lgr_sort_pairs_u32(cx, skeys, skeys + ns, svals, sidx, (size_t) ns, 0, 5));
        km_cluster_offsets<<<1, 64, 0, cx->stream>>>(skeys + ns, ns, coff);
        km2_init<<<KCL, 64, 0, cx->stream>>>(smp, sidx, coff, cen, sub, cen2);
        if (sub > 1) {
            for (int it = 0; it < KM2_ITERS; ++it) {
                km2_step<<<dim3(KM2_PIECES, KCL), KM2_THREADS, 0, cx->stream>>>(smp, sidx, coff, kmax, cen2, sub, acc2);
                km2_finalize<<<n_leaves, 64, 0, cx->stream>>>(acc2, kmax, cen2);
            }
        }
        LGR_HIP(cx, hipGetLastError());
        return LGR_OK;
    };
    const bool want_basis = mo.box_bounds != 0;
    if (want_basis && basis_side_by_side) {
        LGR_TRY(lgr_run_pair(ctx, lloyd, [&](lgr_ctx* cx) { return box_basis(cx, mo.box_bounds == 2, smp, smp_ok, ns, basis, []() { return (int) LGR_OK; }); }));
    } else if (want_basis) {
        LGR_TRY(box_basis(ctx, mo.box_bounds == 2, smp, smp_ok, ns, basis, [&]() { return lloyd(ctx); }));   // Jacobi on the host under the Lloyd steps
    } else {
        LGR_TRY(lloyd(ctx));
    }
    auto pick_group = [](size_t q_count, size_t t_count) {   // table [t/g][q] floats kept under ~6 GB
        int g = 1024;
        while (g < 4096 && (t_count / g + 1) * q_count * 4 > ((size_t) 6 << 30)) g *= 2;
        return g;
    };
    int rg_rows = both ? pick_group((size_t) mb, (size_t) ma) : BLOCK_ROWS;   // row groups (column direction table)
    if (ma <= 65536) rg_rows = BLOCK_ROWS;                                     // small inputs: keep the cluster padding small
    P->d_a = d_a; P->ma = ma; P->mb = mb; P->both = both; P->mopt = mo;
    P->sub = sub; P->rg_rows = rg_rows; P->ns = ns;
    P->cen = cen; P->cen2 = cen2; P->smp = smp; P->smp_ok = smp_ok; P->basis = basis; P->basis_ready = want_basis; P->irr = irr;
    return LGR_OK;
}

// Clustering for a coming lgr_match_bf*_dev(ctx, d_a, ma, <train side of mb rows>, both directions or not) from the query side's
// descriptors alone (a chain of ~60 short launches and one host Jacobi), so that the caller can run it while the train side's
// descriptors are still being computed on another context.  Consumed by the next matcher call on this context when
// (d_a, ma, mb, both, options) agree; lgr_match_prepare_cancel drops it (every exit path of the caller).
int lgr_match_prepare(lgr_ctx* ctx, const float* d_a, int ma, int mb, bool both) {
    MatchPrep* P = match_prep_of(ctx);
    P->armed = false;
    if (!d_a || ma <= 0 || mb <= 0) return LGR_OK;
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    LGR_TRY(match_cluster(ctx, d_a, ma, nullptr, mb, both, false, P));
    P->armed = true;
    return LGR_OK;
}
void lgr_match_prepare_cancel(lgr_ctx* ctx) {
    if (ctx && ctx->match_prep) ((MatchPrep*) ctx->match_prep)->armed = false;
}

// ---------------------------------------------------------------------------------------------------------------
// The host side of one match call: match_impl (at the end of this section) is the list of its stages, every stage is a member of
// MatchCall, and MatchCall holds what the stages share.
//
// Streams and events.  `main` is ctx->stream; `aux` is ctx->aux->stream (boxes, sorted copies); `sB` is the context's third stream
// (f16 formats: pruning workspace, column operands, the passes' table initialisation; with f32 operands or without helper contexts it IS
// main, and none of its events is used).  For every event the matcher touches: where it is recorded -> who waits for it.
//   aux_ev       main, start_aux                                         -> aux, in front of the box kernels
//                aux, behind the sorted copies (launch_sorted_copies)    -> main, join_sorted: in front of lb_kernel (f32 operands), otherwise
//                                                                           in front of the irregular scan / self-check / exact rerank
//   ev[26]       main, launch_sorted_copies(behind_main): where pass 0   -> aux, in front of the sorted copies
//                (or the dense pass) is queued
//   ev[30]       aux, behind the box kernels (start_aux)                 -> main, in front of box_lb_kernel (near_schedule)
//                stream3, behind the covariance's read-back (box_basis)  -> the host (box_basis)
//   ev[31]       main, prepare_prune_ws                                  -> sB, in front of the workspace's clear
//   ev[27]       sB, behind the clear and the packed leaf centres        -> main, in front of the ball bounds (lower_bounds)
//   ev3          main, behind the row operands (pack_operands)           -> sB, in front of the column operands
//                sB, behind its last producer of the set-up (sB.record:  -> main, sB.join: in front of pass 0's stage masks when they use
//                in front of the pass loop; dense mode: at the join)        the shells, otherwise in front of the first MFMA launch
//   ev[28]       main, behind a pass's schedule (init_pass_tables)       -> sB, in front of that pass's init_tables_sparse_kernel
//                main, behind km_sample (box_basis)                      -> stream3, in front of the covariance
//   ev[29]       sB, behind init_tables_sparse_kernel                    -> main, in front of that pass's work list and MFMA launch
//   ev[9 + 2k],  main, around the k-th MFMA launch group (launch_mfma)   -> the host, lgr_match_last_kernel_ms
//   ev[10 + 2k]
//
// A helper stream forked off the context's stream: `fork` makes it wait for what main holds so far, `record` marks its last producer,
// `join` makes main wait for that mark (once).  Whatever makes the call return early (an allocation failure, a HIP error): kernels queued on
// a helper stream read the caller's d_a / d_b and write this call's buffers, so the destructor drains it before the caller gets its buffers
// back -- and before the device's turn goes to another context (lgr_turn records its hand-over event on ctx->stream only).  On the normal
// path the stream has been joined into ctx->stream long before, and the synchronisation returns at once.
struct Fork {
    lgr_ctx* ctx = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t ev = nullptr;   // what record() records and join() waits for
    bool live = false;         // false: s is the context's own stream -- nothing is recorded or waited for
    bool recorded = false, joined = false;
    ~Fork() { if (s && s != ctx->stream) (void) hipStreamSynchronize(s); }
    void start(lgr_ctx* c, hipStream_t stream, hipEvent_t event, bool events) { ctx = c; s = stream; ev = event; live = events; }
    int fork(hipEvent_t at) {
        if (live) {
            LGR_HIP(ctx, hipEventRecord(at, ctx->stream));
            LGR_HIP(ctx, hipStreamWaitEvent(s, at, 0));
        }
        return LGR_OK;
    }
    int record() {
        if (live && !recorded) LGR_HIP(ctx, hipEventRecord(ev, s));
        recorded = true;
        return LGR_OK;
    }
    int join() {
        if (!joined) {
            LGR_TRY(record());
            if (live) LGR_HIP(ctx, hipStreamWaitEvent(ctx->stream, ev, 0));
        }
        joined = true;
        return LGR_OK;
    }
};

// MFMA operand format of a call and the error terms that go with it
struct OperandScale {
    bool rot;            // rotated 30-D format (FMT_F16R)
    F16Scale sc;
    EpsExtra ex;
    float c_scale, out_scale;
};
// r2 / drop2: the largest |x - c|^2 and the largest energy of the three coordinates the rotated 30-D format would drop, both sides
// (assign_kernel, build_side); operand_format: lgr_match_options (< 0: plain forced, 2: rotated forced, otherwise by the data)
static OperandScale operand_scale(bool f16, float r2, float drop2, int operand_format) {
    OperandScale o{false, {1.f, 1.f, {1.f, 1.f, 1.f}, {1.f, 1.f, 1.f}}, {0.f, 0.f, 1.f}, 1.f, 1.f};
    if (!f16) return o;
    F16Scale& sc = o.sc;
    EpsExtra& ex = o.ex;
    // the power-of-two scale 2^s puts the largest operand (2 |a'| 2^s, |b'| 2^s) just under 2^15
    // Rotated format (FMT_F16R) when what it drops is negligible: with u the dropped coordinates of a row relative to a
    // centre, d2 = d2_30 + |u_a - u_b|^2 and 0 <= |u_a - u_b|^2 <= 4 max |u|^2 -- that bound joins the absolute error
    // term, so the choice below only trades speed.  FPFH rows: every block sums to 100 -> max |u|^2 ~ 1e-7.
    const int rot_env = operand_format < 0 ? -1 : (operand_format == 2 ? 1 : 0);
    o.rot = rot_env >= 0 ? rot_env != 0 : (4.0 * (double) drop2 <= 1e-8 * (double) r2);
    double R = std::sqrt((double) r2);
    int sexp = R > 0 ? (int) std::floor(std::log2(16384.0 / R)) : 14;
    sexp = std::max(-40, std::min(14, sexp));
    double N_max = (double) r2 * std::ldexp(1.0, 2 * sexp);
    int e1 = N_max > 32768.0 ? (int) std::ceil(std::log2(N_max / 32768.0)) : 0;
    e1 = std::min(15, std::max(0, e1));
    sc.s_mul = (float) std::ldexp(1.0, sexp);
    sc.inv_s2 = (float) std::ldexp(1.0, -2 * sexp);
    sc.a_norm[0] = (float) std::ldexp(1.0, e1);
    sc.a_norm[1] = (float) std::ldexp(1.0, std::max(0, e1 - 11));
    sc.a_norm[2] = (float) std::ldexp(1.0, std::max(0, e1 - 22));
    for (int k = 0; k < 3; ++k) sc.inv_a_norm[k] = 1.f / sc.a_norm[k];   // exact: powers of two
    o.c_scale = (float) std::ldexp(1.0, 2 * sexp);
    o.out_scale = sc.inv_s2;
    // error terms of the split: elements whose second half would be an f16 subnormal may be flushed
    // (tau per element, linear term); three-term norm expansion (absolute term); the 112-product f32 accumulation
    // chain and the 2^-22 split residual are covered by doubling the quadratic term
    const double tau = std::ldexp(1.0, -14 - sexp);
    ex.lin = (float) (12.0 * tau);
    ex.abs = (float) (2.0 * std::ldexp(1.0, -14) * (sc.a_norm[2] + sc.a_norm[1] / 2048.0 + sc.a_norm[0] / 4194304.0) * (double) sc.inv_s2 * 1.01);   // both norms
    ex.quad = 2.f;
    if (o.rot) {
        // Helmert coordinates are computed in f32: |dy| <= 10.4 u |x'| per vector (prefix sums of <= 11 terms, one
        // rounded constant) -> 20.8 u (x + y)^2 on d2, 0.13 of the unit 4 g40 (x + y)^2; the dropped energy is absolute.
        // Norms: the rotated format stores a norm as TWO f16 terms against c0 = a_norm[0] (pack16_kernel): n1 = rn(N / c0),
        // r1 = N - c0 n1 (exact), n2 = rn(r1 / c0), error e = r1 - c0 n2, with N = |x'|^2 2^2s <= N_max <= 2^15 c0 (so n1 is finite):
        //   n1 normal (N >= 2^-14 c0):  |r1| <= 2^-11 N;  n1 subnormal: |r1| <= 2^-25 c0 (half the f16 subnormal spacing 2^-24, times c0);
        //   n2 (|r1 / c0| <= 16):       |e| <= 2^-11 |r1| + 2^-25 c0  ->  |e| <= 2^-22 N + 2^-25 c0 (1 + 2^-11);
        //   should the MFMA flush subnormal f16 inputs (hipcc's default mode keeps them), a flushed n2 loses |r1| < 2^-14 c0, a flushed
        //   n1 (with n2) N + |e| < 2^-14 c0 (1 + 2^-11) -- so, whatever the mode, per norm  |e| <= 2^-22 N + 2^-14 c0 (1 + 2^-10).
        // All products c0 n are exact in the f32 accumulator.  Both norms, back in d2 units (x 2^-2s): 2^-22 (|a'|^2 + |b'|^2) + 2^-13 c0 2^-2s.
        //   relative part: 2^-22 (x^2 + y^2) <= 2^-22 (x + y)^2 = 0.025 of the unit 4 g40 (x + y)^2 (9.54e-6) -> quad + 0.03;
        //   absolute part: c0 < 2^-14 N_max by the choice of e1 (or c0 = 1), so 2^-13 c0 2^-2s < 2^-27 max |x - c|^2 -- it replaces the
        //   three-term expansion's 2^-13 (a_norm[2] + ..) 2^-2s above (whose relative part, 2^-33 N, sat inside the doubled quad).
        ex.quad = 2.23f;
        ex.abs = (float) ((2.0 * std::ldexp(1.0, -14) * (double) sc.a_norm[0] * (1.0 + std::ldexp(1.0, -10)) * (double) sc.inv_s2) * 1.01
                          + 4.0 * (double) drop2 * 1.0001);
    }
    return o;
}
// the constant part of the coarse rejection's threshold (CoarseArgs, lgr_match_common.cuh): T = max(U) (1 + 1e-5) + quad (x + y)^2 + cross x y + lin (x + y) + abs
static CoarseArgs coarse_constants(const OperandScale& os) {
    const EpsExtra& ex = os.ex;
    const F16Scale& sc = os.sc;
    CoarseArgs ca{};
    const double c_quad = 9.5367477e-6 * (double) ex.quad * 1.00001;            // eps (group_eps)
    const double d11 = std::ldexp(1.0, -11) * (1.0 + std::ldexp(1.0, -9));      // delta: 2^-11 (x^2 + y^2) + 2^-10 x y
    ca.quad = (float) ((c_quad + d11) * 1.000001);                             // 2^-11 (x^2 + y^2) = 2^-11 (x + y)^2 - 2^-10 x y
    ca.cross = (float) (2.0 * d11 * 1.000001);                                  // 2^-9 x y (a1.b2 and a2.b1) - 2^-10 x y
    ca.lin = (float) (2.0 * (double) ex.lin * 1.00001 + 1e-30);
    ca.abs = (float) (((double) ex.abs * 1.00001 + 2.0 * (double) sc.a_norm[0] * std::ldexp(1.0, -25) * (double) sc.inv_s2) * 1.000001 + 1e-12);
    return ca;
}

// The pruning workspace (WS_MATCH_PRUNE): every table of the skipping bookkeeping, carved in this order with 256-byte rounding.
struct PruneWs {
    float* LBsq;                    // [n_rb][n_leaves] squared lower bounds
    uint8_t *done, *sched;          // [n_rb][n_leaves] tile states
    uint8_t* touched;               // ... and the pairs the sweep's tile list touched (final pass as sweep + listed tiles)
    unsigned *mask, *mask_acc;      // [n_rb][n_cc] stage masks of the pass / of all passes so far
    float *u_rb, *u_rt;             // largest U^2 per row block / per row tile
    unsigned* u_leaf;               // [MAXLEAF] float bits
    MaskStats* stats;
    uint2* lb_part;                 // box_lb_kernel's counts per row block (summed by near_kernel)
    int *leaf_first, *leaf_last;    // [MAXLEAF] first / last column stage of every leaf (mask_sparse_kernel)
    unsigned* mask_chk;             // self_check: mask_kernel's masks beside the sparse kernel's
    unsigned *u_stage, *u_ct;       // [column stages] / [column tiles] float bits
    uint8_t *comp_r, *comp_c;       // what the passes left computed, per (row block, group) / (leaf, row group)
    float* smaxB;                   // [KCL][column stages]
    unsigned long long* coarse_cnt;
    float *u_row, *u_colv;          // every row's own upper bound (the sweep's per-row thresholds) / every column's (the per-element re-test of the tiles the sweep keeps)
    float2 *stage_shell, *rb_shell;
    int* cperm;
    float* cnrm;
    f16x8* cop;                     // the leaf centres as packed train rows
    char *clear_begin, *clear_end;  // cleared at the start of a call: [done, comp_r) -- done, sched, touched, masks, bounds, stats
    size_t bytes;
    // self_check: mask_kernel's bookkeeping goes to scratch -- box_lb_kernel's partial counts, read by the near kernels, long done
    MaskStats* scratch_stats() const { return (MaskStats*) lb_part; }
};

struct CheckView {   // what the self-check reads of the pruned passes' bookkeeping (all nullptr: dense mode)
    const uint8_t *done = nullptr, *sched = nullptr;
    const float* lb = nullptr;
    const unsigned* ustage = nullptr;
    const float *uq_rows = nullptr, *uq_cols = nullptr;
};

// passes 1..: tiles within beta * U of the bounds known so far; the last pass (beta = 1) takes everything the bounds cannot exclude
static const float betas[] = {LGR_PRUNE_BETAS};
static const int n_beta = (int) (sizeof betas / sizeof betas[0]);
// (an intermediate sweeping pass whose tile list overflows would go unrepaired: the repair re-runs the LAST pass's mask only, and
//  every launch resets the list's counter -- seen as wrong matches with -DLGR_PRUNE_BETAS=0.5f,1.0f at pass-0 widths 6 and 12)
static_assert(sizeof betas / sizeof betas[0] == 1, "LGR_PRUNE_BETAS: one final pass only (lgr_match_common.cuh)");
static_assert(sizeof betas / sizeof betas[0] + 1 <= 7, "MaskStats: slot 7 holds the stages counted once");

struct MatchCall {
    // the call
    lgr_ctx* const ctx;
    const float* const d_a; const int ma;
    const float* const d_b; const int mb;
    const int block;
    int32_t* const d_ab_idx; float* const d_ab_dist; int32_t* const d_ba_idx; float* const d_ba_dist;
    const bool both;
    const lgr_match_options& mo;
    lgr_match_stats& st;             // in the context: the helper thread of the second rerank direction writes its own fields
    const int near_t;
    const bool prune;
    // 1. + 2. clustering and the two sides
    MatchPrep* const P;
    const Side& A;                   // P->A
    Side B;
    int sub = 1, n_leaves = 0, rg_rows = BLOCK_ROWS;
    float *cen = nullptr, *cen2 = nullptr;
    char* misc = nullptr;            // WS_MATCH_MISC: the first 8 KB hold small per-call scalars
    int ma_pad = 0, mb_pad = 0, ta = 0, tb = 0, n_rb = 0, n_stage_total = 0, n_cc = 0, n_rg = 0, n_groups = 0, n_cpad = 0;
    // the rows in sorted order and the boxes (aux stream)
    float *sortedA = nullptr, *sortedB = nullptr;
    bool boxes = false;
    float *boxA = nullptr, *boxBt = nullptr;
    unsigned* rmax2 = nullptr;
    Fork aux;                        // box_kernel / gather_rows_kernel
    // 3. operands
    bool f16 = false, force_dense = false;
    OperandScale os{};
    int KS = 0, NF = 0;              // MFMA steps of a tile; fragments stored per tile and side
    size_t bset_stride = 0, cset_stride = 0;   // fragments per column set / per set of packed leaf centres
    char *Aop = nullptr, *Bop = nullptr;
    float *nAp = nullptr, *nBp = nullptr;
    float2 *shellA = nullptr, *shellB = nullptr;   // radial shells of the 32-row / 32-column tiles about the centres they are packed against (written by the f16 packing kernels)
    unsigned* d_max = nullptr;       // [2]: norm overflow flag of the f32 packing (the f16 statistics come from assign_kernel)
    // group tables (WS_MATCH_BEST_B)
    float *gmaxB = nullptr, *gmaxA = nullptr;
    int *cl_of_rg = nullptr, *tile_group = nullptr, *tile_leaf = nullptr, *group_start = nullptr;
    int *group_leaf = nullptr, *leaf_g0 = nullptr;   // [n_groups]: leaf of a group; [n_leaves + 1]: first group of a leaf (the skipping schedule's tables)
    Fork sB;                         // the third stream: column operands, table initialisation
    PruneWs W{};
    // 4. the minimum tables, the persistent kernel's work items, the sweep's tile list
    int *rowmin = nullptr, *colmin = nullptr;
    unsigned long long *bestA = nullptr, *bestB = nullptr;
    int item_rb = 0, n_ir = 0, ccx = 0, n_flags = 0, mfma_grid = 0;
    int *iflags = nullptr, *ipos = nullptr;
    int2* ilist = nullptr;
    int *xcd_start = nullptr, *xcd_ctr = nullptr;   // [9] (+ 32 / + 48: the sweep's and the plain kernel's share, pass_select_kernel), [8]
    unsigned kept_cap = 0;
    uint2* kept = nullptr;
    unsigned long long* kept_count = nullptr;
    unsigned short* ucol16 = nullptr;
    bool split_used = false;
    // the pruned passes
    bool colstage = false, coarse = false;
    CoarseArgs ca_on{};              // coarse rejection without upper bounds (pass 0); with_bounds() adds them
    ShellArgs shell{}, shell0{};     // shell bound of the passes that have upper bounds / of pass 0
    const uint8_t* sched_final = nullptr;   // what the final pass left computed: its schedule, or -- sweep + listed tiles -- the pairs the list touched
    const unsigned long long* cur_pass_stages = nullptr;   // device: the stage count of the pass being launched (mask_kernel's statistics)
    bool defer_init = false;         // the pass being launched initialises its tables behind the sweep (init_touched_tables)
    CompView comp_rows{nullptr, 0, nullptr}, comp_cols{nullptr, 0, nullptr};
    CheckView chk;

    MatchCall(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block, int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist)
        : ctx(ctx), d_a(d_a), ma(ma), d_b(d_b), mb(mb), block(block), d_ab_idx(d_ab_idx), d_ab_dist(d_ab_dist), d_ba_idx(d_ba_idx), d_ba_dist(d_ba_dist),
          both(d_ba_idx != nullptr && mb > 0), mo(ctx->mopt), st(ctx->mstats), near_t(mo.near > 0 ? mo.near : NEAR_T),
          prune(mo.prune == 1 || (mo.prune != 0 && (double) ma * mb >= 65536.0 * 65536.0)),   // -1 auto, 0 off, 1 on
          P(match_prep_of(ctx)), A(P->A) {}

    int build_both(const IrrRef* irr);
    int build_sides();
    int start_aux();
    int launch_sorted_copies(bool behind_main);
    int join_sorted();
    int choose_format();
    int upload_group_tables();
    PruneWs carve_prune_ws(char* base) const;
    int prepare_prune_ws();
    int pack_operands();
    int check_pack16(const float* X, const int* perm, int n_pad, int role, const int* blkcl, const void* op, const float* nrm, const float2* shell_);
    int alloc_tables();
    int launch_mfma(const unsigned* mask, const CoarseArgs& ca, bool allow_split = true);
    int init_touched_tables();
    int run_dense();
    int lower_bounds();
    int coarse_setup();
    int near_schedule();
    CoarseArgs with_bounds() const;
    void build_comp();
    int upper_bounds_schedule(int pass);
    int init_pass_tables(int pass);
    int build_masks(int pass);
    int run_pruned();
    int read_back_stats();
    int irregular_rows();
    int self_check(const CheckView& v);
    int rerank();
};

#include "lgr_match_debug.cuh"

// ---- 1. + 2. clustering, then assign / sort / place both sides -- unless the query side was prepared ahead of this call
// the two sides are independent (assign, sort, two host read-backs each): side by side on the two contexts
int MatchCall::build_both(const IrrRef* irr) {
    return lgr_run_pair(ctx, [&](lgr_ctx* cx) { return build_side(cx, d_a, ma, P->cen, P->cen2, P->sub, 1, P->rg_rows, WS_MATCH_NA, WS_MATCH_AP, 0, irr, &P->A); },
                        [&](lgr_ctx* cx) { return build_side(cx, d_b, mb, P->cen, P->cen2, P->sub, TILE, PAD, WS_MATCH_NB, WS_MATCH_BP, 1, irr, &B); });
}
int MatchCall::build_sides() {
    const bool prepared = P->armed && P->d_a == d_a && P->ma == ma && P->mb == mb && P->both == both && memcmp(&P->mopt, &mo, sizeof mo) == 0;
    P->armed = false;
    if (!prepared) LGR_TRY(match_cluster(ctx, d_a, ma, d_b, mb, both, true, P));
    LGR_TRY(build_both(P->irr));
    // the irregular-row lane gives up when a side has more such rows than its list holds, or when they are all a side has (the centres then
    // come from the other side alone and nothing is left for the filter): both sides again with every finite row in the operands
    if (A.n_irr > IRR_CAP || B.n_irr > IRR_CAP || ((A.n_irr || B.n_irr) && (A.n_valid == 0 || B.n_valid == 0))) {
        st.irr_gave_up = 1u;
        LGR_TRY(build_both(nullptr));
    }
    st.irr_a = (unsigned) A.n_irr; st.irr_b = (unsigned) B.n_irr;
    sub = P->sub; n_leaves = KCL * sub; rg_rows = P->rg_rows;
    cen = P->cen; cen2 = P->cen2;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_MISC, 8192, &misc));   // (grown by match_cluster)
    if (A.n_valid == 0 || B.n_valid == 0) return LGR_OK;   // (nothing to match: match_impl returns)
    ma_pad = A.n_pad; mb_pad = B.n_pad;
    st.rg_rows = rg_rows;
    ta = ma_pad / TILE; tb = mb_pad / TILE;
    n_rb = ma_pad / BLOCK_ROWS; n_stage_total = mb_pad / STAGE_COLS;
    return LGR_OK;
}

// The rows in sorted order (exact rerank, box bounds) and the bounding boxes of the row blocks / leaves need nothing of the operand
// packing: four launches on the second stream, which run under the packing passes (joined before section 4).
int MatchCall::start_aux() {
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_SORTED_B, (size_t) mb_pad * 33, &sortedB));
    if (both || prune) LGR_TRY(lgr_ws_t(ctx, WS_MATCH_SORTED_A, (size_t) ma_pad * 33, &sortedA));
    boxes = prune && mo.box_bounds != 0;
    if (boxes) {
        LGR_TRY(lgr_ws_t(ctx, WS_MATCH_BOX, (size_t) n_rb * 66 + (size_t) n_leaves * 66 + 64, &boxA));
        boxBt = boxA + (size_t) n_rb * 66;
        rmax2 = (unsigned*) (boxBt + (size_t) n_leaves * 66);
    }
    LGR_TRY(lgr_ctx_aux(ctx));
    aux.start(ctx, ctx->aux->stream, ctx->aux_ev, true);
    LGR_TRY(aux.fork(ctx->aux_ev));
    if (boxes) {   // first (the bounds wait for them), reading the rows through the placement
        const float* basis = P->basis;   // V [33][33], mu [33] (match_cluster)
        LGR_HIP(ctx, hipMemsetAsync(rmax2, 0, 4, aux.s));
        box_kernel<<<n_rb, 256, 0, aux.s>>>(d_a, A.perm, nullptr, n_rb, basis, basis + 33 * 33, 0, boxA, rmax2);
        box_kernel<<<n_leaves, 256, 0, aux.s>>>(d_b, B.perm, B.leaf_start, n_leaves, basis, basis + 33 * 33, 1, boxBt, rmax2);
        LGR_HIP(ctx, hipEventRecord(ctx->ev[30], aux.s));
    }
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}
// The sorted copies are for the exact rerank (and the f32 ball bounds): with the f16 formats nothing before the MFMA passes reads them, so
// they are gathered UNDER pass 0 (called where that pass is queued: the set-up phase in front of it is bound by HBM -- 2.1 GB of column
// operands -- and the passes are not).  Once per call; behind_main: not before the work queued on the main stream so far.
int MatchCall::launch_sorted_copies(bool behind_main) {
    if (aux.recorded) return LGR_OK;
    if (behind_main) LGR_TRY(aux.fork(ctx->ev[26]));
    gather_rows_kernel<<<cdiv((long long) mb_pad * 33, 256), 256, 0, aux.s>>>(d_b, B.perm, mb_pad, sortedB);
    if (sortedA) gather_rows_kernel<<<cdiv((long long) ma_pad * 33, 256), 256, 0, aux.s>>>(d_a, A.perm, ma_pad, sortedA);
    LGR_HIP(ctx, hipGetLastError());
    return aux.record();
}
// in front of the first reader of sortedA / sortedB (a reader in front of the passes: the f32 ball bounds)
int MatchCall::join_sorted() {
    LGR_TRY(launch_sorted_copies(false));
    return aux.join();
}

// ---- 3. operand format and scales, the operand buffers
int MatchCall::choose_format() {
    f16 = mo.operand_format != 0;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_NORMS, (size_t) ma_pad + (size_t) KCL * mb_pad + 2 * ((size_t) ta + (size_t) KCL * tb) + 64, &nAp));
    nBp = nAp + ma_pad;
    shellA = (float2*) (nBp + (size_t) KCL * mb_pad);
    shellB = shellA + ta;
    d_max = (unsigned*) (misc + 128);
    LGR_HIP(ctx, hipMemsetAsync(d_max, 0, 12, ctx->stream));
    const float r2 = std::max(A.nstat_n2, B.nstat_n2), drop2 = std::max(A.nstat_drop, B.nstat_drop);
    if (f16) force_dense = A.nstat_ovf || B.nstat_ovf;
    os = operand_scale(f16, r2, drop2, mo.operand_format);
    if (f16 && env_int("LGR_MATCH_DEBUG", 0))
        fprintf(stderr, "[lgr] operand statistics: max |x - c|^2 %.6g, dropped energy %.6g (A %.6g, B %.6g) -> %s; irregular rows %d + %d\n", (double) r2, (double) drop2,
                (double) A.nstat_drop, (double) B.nstat_drop, os.rot ? "rotated" : "plain", A.n_irr, B.n_irr);
    st.f16 = f16 ? (os.rot ? 2 : 1) : 0;
    KS = !f16 ? OpFmt<FMT_F32>::KS : os.rot ? OpFmt<FMT_F16R>::KS : OpFmt<FMT_F16>::KS;
    NF = !f16 ? OpFmt<FMT_F32>::NF : os.rot ? OpFmt<FMT_F16R>::NF : OpFmt<FMT_F16>::NF;
    const size_t frag_bytes = f16 ? sizeof(f16x8) : sizeof(float);
    const size_t a_op_bytes = (size_t) ta * NF * 64 * frag_bytes;
    bset_stride = (size_t) tb * NF * 64;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_ROWMIN, a_op_bytes + 256, &Aop));
    const size_t b_op_bytes = KCL * bset_stride * frag_bytes;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_COLMIN, b_op_bytes + 256, &Bop));
    n_rg = cdiv(ma_pad, rg_rows);
    return LGR_OK;
}

// column groups of the row-minimum table: a leaf, cut into pieces of at most GROUP_COLS columns (k-means leaves of
// near-duplicate descriptors can hold tens of thousands of rows; the exact rerank scans a whole group per item).
// Every small host-built table of the call goes up HERE, before the operand packing is enqueued: the one host wait they need
// (the staging vectors go out of scope) then falls on the short placement kernels, not behind the packing.
int MatchCall::upload_group_tables() {
    std::vector<int> h_group_start, h_tiles(2 * (size_t) tb);   // [tile] -> group, [tb + tile] -> leaf
    int group_cols = GROUP_COLS;   // larger pieces for very large inputs: keep the table [groups][ma_pad] under ~24 GB
    while (group_cols < 65536 && ((size_t) mb_pad / group_cols + n_leaves) * (size_t) ma_pad * 4 > ((size_t) 24 << 30)) group_cols *= 2;
    for (int l = 0; l < n_leaves; ++l)
        for (int s0 = B.h_leaf_start[l]; s0 < B.h_leaf_start[l + 1]; s0 += group_cols) {
            int s1 = std::min(B.h_leaf_start[l + 1], s0 + group_cols), g = (int) h_group_start.size();
            h_group_start.push_back(s0);
            for (int t = s0 / TILE; t < s1 / TILE; ++t) { h_tiles[t] = g; h_tiles[tb + t] = l; }
        }
    n_groups = (int) h_group_start.size();
    st.sub_cols = n_groups;
    h_group_start.push_back(mb_pad);
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_BEST_B, (size_t) KCL * n_groups + 2 * (size_t) n_rg + 2 * (size_t) tb + 2 * (size_t) n_groups + n_leaves + 72, &gmaxB));
    gmaxA = gmaxB + (size_t) KCL * n_groups;
    cl_of_rg = (int*) (gmaxA + n_rg);
    tile_group = cl_of_rg + n_rg;
    tile_leaf = tile_group + tb;
    group_start = tile_leaf + tb;
    group_leaf = group_start + n_groups + 1;
    leaf_g0 = group_leaf + n_groups;
    std::vector<int> h(n_rg), hgl(n_groups), hl(n_leaves + 1, n_groups);
    for (int g = 0; g < n_rg; ++g) h[g] = A.h_blkcl[(size_t) g * (rg_rows / BLOCK_ROWS)];
    for (int g = 0; g < n_groups; ++g) hgl[g] = h_tiles[tb + h_group_start[g] / TILE];
    for (int g = n_groups - 1; g >= 0; --g) hl[hgl[g]] = g;                       // first group of every leaf that has one
    for (int l = n_leaves - 1; l >= 0; --l) hl[l] = std::min(hl[l], hl[l + 1]);   // empty leaves: g0 == g1
    LGR_HIP(ctx, hipMemcpyAsync(cl_of_rg, h.data(), h.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(tile_group, h_tiles.data(), h_tiles.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(group_start, h_group_start.data(), h_group_start.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(group_leaf, hgl.data(), hgl.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(leaf_g0, hl.data(), hl.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LGR_OK;
}

static void launch_pack16(bool rot, hipStream_t s, const float* X, const int* perm, int n_pad, int role, const float* cen, const int* blkcl, const F16Scale& sc,
                          void* op, float* nrm, float2* shell) {
    const dim3 grid(cdiv(n_pad, 256));
    _Float16* P = (_Float16*) op;
    if (role == 0) {
        if (rot) pack16_kernel<true, false><<<grid, 256, 0, s>>>(X, perm, n_pad, cen, blkcl, sc, P, nrm, shell);
        else pack16_kernel<false, false><<<grid, 256, 0, s>>>(X, perm, n_pad, cen, blkcl, sc, P, nrm, shell);
    } else {
        if (rot) pack16_kernel<true, true><<<grid, 256, 0, s>>>(X, perm, n_pad, cen, blkcl, sc, P, nrm, shell);
        else pack16_kernel<false, true><<<grid, 256, 0, s>>>(X, perm, n_pad, cen, blkcl, sc, P, nrm, shell);
    }
}
// lgr_match_options.self_check (tests): one packing launch again with the reference kernel, set by set into one set-sized scratch buffer (131 MB
// at 1M rows instead of 2.1 GB), and every 16-byte piece of the fragments and norms and every tile shell compared on the device.  The counts
// add up over the launches of a call (lgr_match_last_pack_check); a differing piece fails the call.
int MatchCall::check_pack16(const float* X, const int* perm, int n_pad, int role, const int* blkcl, const void* op, const float* nrm, const float2* shell_) {
    const int n_sets = role == 1 ? KCL : 1, tiles = n_pad / TILE;
    const size_t frag16 = (size_t) tiles * NF * 64;   // 16-byte pieces of a set
    Carve carve{0, nullptr};
    const size_t o_frag = carve(frag16 * 16), o_nrm = carve((size_t) n_pad * 4), o_shell = carve((size_t) tiles * 8), o_cnt = carve(16);
    char* scratch;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_DENSE, carve.off, &scratch));   // (the rerank's buffers are not live yet)
    unsigned long long* d_cnt = (unsigned long long*) (scratch + o_cnt);
    float* r_nrm = (float*) (scratch + o_nrm);
    float2* r_shell = shell_ ? (float2*) (scratch + o_shell) : nullptr;
    hipStream_t s = ctx->stream;
    LGR_HIP(ctx, hipMemsetAsync(d_cnt, 0, 16, s));
    for (int set = 0; set < n_sets; ++set) {
        if (os.rot) pack16_ref_kernel<true><<<cdiv(n_pad, 256), 256, 0, s>>>(X, perm, n_pad, role, cen, blkcl, os.sc, set, set + 1, (_Float16*) (scratch + o_frag), r_nrm, r_shell);
        else pack16_ref_kernel<false><<<cdiv(n_pad, 256), 256, 0, s>>>(X, perm, n_pad, role, cen, blkcl, os.sc, set, set + 1, (_Float16*) (scratch + o_frag), r_nrm, r_shell);
        pack_compare_kernel<uint4><<<(unsigned) std::min<size_t>(cdiv(frag16, 256), 4096), 256, 0, s>>>((const uint4*) op + set * frag16, (const uint4*) (scratch + o_frag), frag16, d_cnt);
        pack_compare_kernel<uint4><<<cdiv(n_pad / 4, 256), 256, 0, s>>>((const uint4*) (nrm + (size_t) set * n_pad), (const uint4*) r_nrm, (size_t) n_pad / 4, d_cnt);
        if (shell_) pack_compare_kernel<uint2><<<cdiv(tiles, 256), 256, 0, s>>>((const uint2*) (shell_ + (size_t) set * tiles), (const uint2*) r_shell, (size_t) tiles, d_cnt);
    }
    unsigned long long h_cnt[2] = {0ull, 0ull};
    LGR_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, s));
    LGR_HIP(ctx, hipStreamSynchronize(s));
    if (ctx->mpack[0] == ~0ull) ctx->mpack[0] = ctx->mpack[1] = 0ull;
    ctx->mpack[0] += h_cnt[0]; ctx->mpack[1] += h_cnt[1];
    if (h_cnt[1]) { ctx->err = "matcher self-check: pack16_kernel's operands differ from pack16_ref_kernel's"; return LGR_ERR_HIP; }
    return LGR_OK;
}

// base == nullptr: the sizes only (PruneWs::bytes)
PruneWs MatchCall::carve_prune_ws(char* base) const {
    Carve carve{0, base};
    PruneWs w{};
    const size_t n_pairs = (size_t) n_rb * n_leaves;
    w.LBsq = carve.take<float>(n_pairs * 4);
    w.done = carve.take<uint8_t>(n_pairs);
    w.sched = carve.take<uint8_t>(n_pairs);
    w.touched = carve.take<uint8_t>(n_pairs);
    w.mask = carve.take<unsigned>((size_t) n_rb * n_cc * 4);
    w.mask_acc = carve.take<unsigned>((size_t) n_rb * n_cc * 4);
    w.u_rb = carve.take<float>((size_t) n_rb * 4);
    w.u_rt = carve.take<float>((size_t) n_rb * (BLOCK_ROWS / TILE) * 4);
    w.u_leaf = carve.take<unsigned>((size_t) MAXLEAF * 4);
    w.stats = carve.take<MaskStats>(sizeof(MaskStats));
    w.lb_part = carve.take<uint2>((size_t) n_rb * sizeof(uint2));
    w.leaf_first = carve.take<int>((size_t) MAXLEAF * 4);
    w.leaf_last = carve.take<int>((size_t) MAXLEAF * 4);
    w.mask_chk = carve.take<unsigned>(mo.self_check ? (size_t) 2 * n_rb * n_cc * 4 + 256 : 0);
    w.u_stage = carve.take<unsigned>((size_t) n_stage_total * 4);
    w.u_ct = carve.take<unsigned>((size_t) tb * 4);
    w.comp_r = carve.take<uint8_t>((size_t) n_rb * n_groups);
    w.comp_c = carve.take<uint8_t>((size_t) n_leaves * n_rg);
    w.smaxB = carve.take<float>((size_t) KCL * n_stage_total * 4);
    w.coarse_cnt = carve.take<unsigned long long>(32);
    w.u_row = carve.take<float>((size_t) ma_pad * 4);
    w.u_colv = carve.take<float>((size_t) mb_pad * 4);
    w.stage_shell = carve.take<float2>((size_t) KCL * n_stage_total * 8);
    w.rb_shell = carve.take<float2>((size_t) n_rb * 8);
    w.cperm = carve.take<int>((size_t) (n_leaves + TILE) * 4);
    w.cnrm = carve.take<float>((size_t) KCL * (n_leaves + TILE) * 4);
    w.cop = carve.take<f16x8>((size_t) KCL * ((n_leaves + TILE) / TILE) * 7 * 64 * sizeof(f16x8));
    w.clear_begin = (char*) w.done; w.clear_end = (char*) w.comp_r;
    w.bytes = carve.off;
    return w;
}
// The third stream, and (3b ahead of time) the skipping bookkeeping's workspace, cleared on it, and the leaf centres packed as train rows for
// the ball bounds on the matrix cores -- both need nothing of the operand packing and used to sit on the critical chain behind it
// (a 12 MB memset and two short launches: 0.36 ms between pack16 and lb_mfma_kernel in the round-5 timeline)
int MatchCall::prepare_prune_ws() {
    hipStream_t s3 = ctx->stream;
    if (f16) LGR_TRY(lgr_ctx_stream3(ctx, &s3));
    sB.start(ctx, s3, ctx->ev3, s3 != ctx->stream);
    n_cc = cdiv(mb_pad, CHUNK_COLS);
    n_cpad = pad_to(n_leaves, TILE);
    cset_stride = (size_t) (n_cpad / TILE) * NF * 64;
    if (!prune) return LGR_OK;
    char* pb;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_PRUNE, carve_prune_ws(nullptr).bytes, &pb));
    W = carve_prune_ws(pb);
    LGR_TRY(sB.fork(ctx->ev[31]));
    LGR_HIP(ctx, hipMemsetAsync(W.clear_begin, 0, W.clear_end - W.clear_begin, sB.s));
    if (f16) {
        centre_perm_kernel<<<cdiv(n_cpad, 256), 256, 0, sB.s>>>(n_leaves, n_cpad, W.cperm);
        launch_pack16(os.rot, sB.s, cen2, W.cperm, n_cpad, 1, cen, nullptr, os.sc, W.cop, W.cnrm, nullptr);
    }
    if (sB.live) LGR_HIP(ctx, hipEventRecord(ctx->ev[27], sB.s));   // workspace cleared (+ centres packed, f16 formats): lower_bounds waits
    return LGR_OK;
}

// ---- 3. pack operands, group maxima
// The column (train-side) operands -- 16 sets, 2.1 GB at 1M rows, the longest piece of the set-up -- are packed on the third stream:
// nothing before the first MFMA pass reads them (the bounds of pass 0 need the ROW operands, the packed leaf centres and the
// boxes), so that chain runs beside the packing instead of behind it.  sB is joined in launch_mfma.
// (It starts BEHIND the row operands' packing: side by side the two packing kernels share the HBM write bandwidth and the row
// operands, which the bounds wait for, take as long as the 2.1 GB of column sets.)
int MatchCall::pack_operands() {
    if (!f16) {
        pack_kernel<<<cdiv(ma_pad, 256), 256, 0, ctx->stream>>>(d_a, A.perm, ma_pad, 0, cen, A.blkcl, (float*) Aop, nAp, d_max + 2);
        pack_kernel<<<dim3(cdiv(mb_pad, 256), KCL), 256, 0, ctx->stream>>>(d_b, B.perm, mb_pad, 1, cen, nullptr, (float*) Bop, nBp, d_max + 2);
        unsigned* h_ovf;
        LGR_TRY(lgr_pinned(ctx, 64, (void**) &h_ovf));
        LGR_HIP(ctx, hipMemcpyAsync(h_ovf, d_max + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        force_dense = h_ovf[0] != 0u;
    } else {
        launch_pack16(os.rot, ctx->stream, d_a, A.perm, ma_pad, 0, cen, A.blkcl, os.sc, Aop, nAp, shellA);
        // the column operands (f16 formats: 2.1 GB at 1M, HBM-write bound) and their group maxima, on the third stream right behind the row operands:
        // 1 ms of HBM writes that everything up to pass 0 crawls beside -- started later, pass 0 starts later.  (Round 5
        // measured the alternatives: behind lb_mfma_kernel -- which then runs alone in 0.18 ms instead of 0.85 -- box_lb_kernel crawls beside the
        // packing instead (0.07 -> 0.92 ms); behind the near kernels, with pass 0's stage selection from assign_kernel's distances so that
        // mask_kernel need not wait for the column norms: mask_kernel crawls (0.4 -> 1.04 ms) and pass 0 starts 0.1 ms later than with this order.
        // Measured again with the streaming pack16_kernel, 0.5 ms instead of 0.8: behind lb_mfma_kernel pass 0 starts no earlier -- DESIGN.md 11.)
        LGR_TRY(sB.fork(ctx->ev3));
        launch_pack16(os.rot, sB.s, d_b, B.perm, mb_pad, 1, cen, nullptr, os.sc, Bop, nBp, shellB);
        if (mo.self_check) {   // (tests) the three packing launches of the call against the reference kernel
            LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
            LGR_HIP(ctx, hipStreamSynchronize(sB.s));
            LGR_TRY(check_pack16(d_a, A.perm, ma_pad, 0, A.blkcl, Aop, nAp, shellA));
            LGR_TRY(check_pack16(d_b, B.perm, mb_pad, 1, nullptr, Bop, nBp, shellB));
            if (prune) LGR_TRY(check_pack16(cen2, W.cperm, n_cpad, 1, nullptr, W.cop, W.cnrm, nullptr));
        }
    }
    group_max_kernel<<<dim3(n_groups, KCL), 256, 0, sB.s>>>(nBp, mb_pad, 0, group_start, gmaxB);
    group_max_kernel<<<dim3(n_rg, 1), 256, 0, ctx->stream>>>(nAp, ma_pad, rg_rows, nullptr, gmaxA);
    return LGR_OK;
}

// ---- 4. the two minimum tables (+inf initialised), the persistent MFMA kernel's work items, the sweep's tile list
int MatchCall::alloc_tables() {
    const size_t tab_floats = (size_t) n_groups * ma_pad + (both ? (size_t) n_rg * mb_pad : 0);
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_BEST_A, tab_floats + 2 * ((size_t) ma + mb) + 64, &rowmin));
    if (both) colmin = rowmin + (size_t) n_groups * ma_pad;
    bestA = (unsigned long long*) (rowmin + tab_floats + (tab_floats & 1));
    bestB = bestA + ma;
    fill_u64<<<cdiv(ma + mb, 256), 256, 0, sB.s>>>(bestA, ma + mb, ~0ull);   // (the exact rerank's tables: joined with the column operands)
    // dense mode: +inf everywhere; skipping mode: init_tables_sparse_kernel covers what each pass computes (lgr_match_options.poison_tables, tests: the
    // rest is filled with 0 -- the most harmful value a stale entry could have -- to show that nothing reads it)
    if (!prune) LGR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t) rowmin, 0x7f800000, tab_floats, ctx->stream));
    else if (mo.poison_tables) LGR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t) rowmin, 0, tab_floats, ctx->stream));
    // work items of the persistent MFMA kernel: one row group (the owner of its column minima) x one column chunk
    item_rb = both ? std::min(rg_rows / BLOCK_ROWS, 16) : 4;
    n_ir = cdiv(n_rb, item_rb); ccx = cdiv(n_cc, 8); n_flags = 8 * ccx * n_ir;
    int* ibuf;
    LGR_TRY(lgr_ws_t(ctx, WS_MATCH_ITEMS2, (size_t) 4 * n_flags + 128, &ibuf));
    iflags = ibuf; ipos = ibuf + n_flags;
    ilist = (int2*) (ibuf + 2 * (size_t) n_flags);
    xcd_start = ibuf + 4 * (size_t) n_flags;
    xcd_ctr = xcd_start + 16;
    mfma_grid = 8 * (LGR_MM_OCC / 2) * std::max(1, ctx->n_cu / 8);   // resident workgroups: LGR_MM_OCC / 2 per CU
    // final pass as sweep + listed tiles (lgr_match_sweep.cuh): the list, its counter, the per-column thresholds as bf16
    kept_cap = mo.kept_cap > 0 ? (unsigned) mo.kept_cap : (16u << 20);
    if (f16 && os.rot && prune && mo.coarse_rejection != 0 && mo.split_sweep != 0) {
        char* kb;
        LGR_TRY(lgr_ws_t(ctx, WS_MATCH_KEPT, (size_t) kept_cap * sizeof(uint2) + (size_t) mb_pad * 2 + 512, &kb));
        kept = (uint2*) kb;
        kept_count = (unsigned long long*) (kb + (size_t) kept_cap * sizeof(uint2));
        ucol16 = (unsigned short*) (kb + (size_t) kept_cap * sizeof(uint2) + 256);
    }
    st.stages_all = (double) n_rb * n_stage_total;
    return LGR_OK;
}

// one match_mfma launch on the work list whose per-XCD shares start at xs: every instantiation is spelled here, once
template <bool BOTH, int FMT, bool CO>
static void launch_match_mfma_as(const MatchCall& c, const unsigned* mask, const int* xs, const CoarseArgs& ca) {
    typedef typename OpFmt<FMT>::frag frag;
    match_mfma<BOTH, FMT, CO><<<c.mfma_grid, NTHR, 0, c.ctx->stream>>>((const frag*) c.Aop, (const frag*) c.Bop, c.bset_stride, c.os.c_scale, c.os.out_scale, c.A.blkcl, c.nAp,
                                                                       c.ma_pad, c.mb_pad, c.rg_rows, c.tile_group, mask, c.rowmin, c.colmin, c.n_cc, c.item_rb, c.ilist, xs, c.xcd_ctr, ca);
}
template <int FMT, bool CO>
static void launch_match_mfma_fmt(const MatchCall& c, const unsigned* mask, const int* xs, const CoarseArgs& ca) {
    if (c.both) launch_match_mfma_as<true, FMT, CO>(c, mask, xs, ca);
    else launch_match_mfma_as<false, FMT, CO>(c, mask, xs, ca);
}
// (both, operand format, coarse rejection inside the kernel) -> the instantiation
static void launch_match_mfma(const MatchCall& c, bool co, const unsigned* mask, const int* xs, const CoarseArgs& ca) {
    if (!c.f16) launch_match_mfma_fmt<FMT_F32, false>(c, mask, xs, ca);
    else if (!c.os.rot) launch_match_mfma_fmt<FMT_F16, false>(c, mask, xs, ca);
    else if (co) launch_match_mfma_fmt<FMT_F16R, true>(c, mask, xs, ca);
    else launch_match_mfma_fmt<FMT_F16R, false>(c, mask, xs, ca);
}

// final pass as sweep + listed tiles: the tables are initialised behind the sweep, for the (row block, leaf) pairs the list touches
// (between match_sweep and match_tiles, on the context's stream)
int MatchCall::init_touched_tables() {
    LGR_HIP(ctx, hipMemsetAsync(W.touched, 0, (size_t) n_rb * n_leaves, ctx->stream));
    touched_kernel<<<4 * std::max(1, ctx->n_cu), 256, 0, ctx->stream>>>(kept, kept_count, kept_cap, xcd_start + 48, W.sched, tile_leaf, n_leaves, (size_t) n_rb * n_leaves, W.touched);
    init_tables_sparse_kernel<<<cdiv((long long) n_rb * n_leaves, 256), 256, 0, ctx->stream>>>(W.touched, W.done, n_rb, n_leaves, leaf_g0, group_start, rg_rows / BLOCK_ROWS, rowmin,
                                                                                               (size_t) ma_pad, colmin, (size_t) mb_pad);
    return LGR_OK;
}

// one MFMA pass over the stages of `mask` (nullptr: all): work list, the join of the column operands, the timed launch group
int MatchCall::launch_mfma(const unsigned* mask, const CoarseArgs& ca, bool allow_split) {
    items_flag_kernel<<<cdiv(n_flags, 256), 256, 0, ctx->stream>>>(mask, n_rb, n_cc, item_rb, n_ir, ccx, iflags);
    size_t sb = 0;
    LGR_HIP(ctx, rocprim::exclusive_scan(nullptr, sb, iflags, ipos, 0, (size_t) n_flags, rocprim::plus<int>(), ctx->stream));
    void* stmp;
    LGR_TRY(lgr_ws(ctx, WS_GRID_TMP, sb, &stmp));
    LGR_HIP(ctx, rocprim::exclusive_scan(stmp, sb, iflags, ipos, 0, (size_t) n_flags, rocprim::plus<int>(), ctx->stream));
    items_emit_kernel<<<cdiv(n_flags, 256), 256, 0, ctx->stream>>>(iflags, ipos, item_rb, n_ir, ccx, ilist, xcd_start);
    LGR_HIP(ctx, hipMemsetAsync(xcd_ctr, 0, 32, ctx->stream));
    LGR_CHECK(ctx, ctx->mfma_timed < 8, LGR_ERR_INVALID_ARG);
    LGR_TRY(sB.join());   // everything that reads the column operands, their norms or maxima comes after this
    (void) hipEventRecord(ctx->ev[9 + 2 * ctx->mfma_timed], ctx->stream);
    if (f16 && os.rot && ca.u_rb && kept && allow_split) {
        // the coarse sweep appends the tiles it keeps to a list, a second kernel finishes them
        split_used = true;
        LGR_HIP(ctx, hipMemsetAsync(kept_count, 0, 8, ctx->stream));
        if (ca.u_colv) ucol_pack_kernel<<<cdiv(mb_pad, 256), 256, 0, ctx->stream>>>(ca.u_colv, mb_pad, os.c_scale, ucol16);
        // Descriptors the bounds cannot separate (structureless rows: every stage is scheduled) gain nothing from the coarse sweep -- nearly every
        // tile passes it and is then computed a second time in full.  The device decides from the pass's stage count (no host round trip: a
        // synchronisation here cost the pass 2.6 ms): above half of all stages the work list goes to the plain six-step kernel, otherwise to
        // the sweep; the other kernel finds an empty list.
        int* xs_sweep = xcd_start + 32;
        int* xs_plain = xcd_start + 48;
        pass_select_kernel<<<1, 16, 0, ctx->stream>>>(mo.coarse_rejection == 2 ? nullptr : cur_pass_stages, 0.5 * st.stages_all, xcd_start, xs_sweep, xs_plain);
        const int sweep_grid = 8 * (SW_OCC / 2) * std::max(1, ctx->n_cu / 8);
        match_sweep<<<sweep_grid, NTHR, 0, ctx->stream>>>((const f16x8*) Aop, (const f16x8*) Bop, bset_stride, os.c_scale, A.blkcl, ma_pad, mb_pad, rg_rows, mask, n_cc,
                                                          item_rb, ilist, xs_sweep, xcd_ctr, ca, ca.u_colv ? ucol16 : nullptr, kept, kept_count, kept_cap);
        if (defer_init) LGR_TRY(init_touched_tables());
        const int tiles_grid = 8 * std::max(1, ctx->n_cu);
        if (both) match_tiles<true><<<tiles_grid, 64 * TL_WAVES, 0, ctx->stream>>>((const f16x8*) Aop, (const f16x8*) Bop, bset_stride, os.out_scale, A.blkcl, ma_pad, mb_pad,
                                                                                   rg_rows, tile_group, rowmin, colmin, kept, kept_count, kept_cap);
        else match_tiles<false><<<tiles_grid, 64 * TL_WAVES, 0, ctx->stream>>>((const f16x8*) Aop, (const f16x8*) Bop, bset_stride, os.out_scale, A.blkcl, ma_pad, mb_pad,
                                                                               rg_rows, tile_group, rowmin, colmin, kept, kept_count, kept_cap);
        launch_match_mfma(*this, false, mask, xs_plain, CoarseArgs{});   // the plain kernel on its share of the work list
    } else {
        launch_match_mfma(*this, ca.u_rb != nullptr, mask, xcd_start, ca);
    }
    (void) hipEventRecord(ctx->ev[10 + 2 * ctx->mfma_timed], ctx->stream);
    ctx->mfma_timed += 1;
    LGR_HIP(ctx, hipGetLastError());
#ifdef EXP_PROF
    LGR_TRY(match_prof_report(ctx, xcd_start));
#endif
    return LGR_OK;
}

int MatchCall::run_dense() {
    LGR_TRY(launch_sorted_copies(true));
    LGR_TRY(launch_mfma(nullptr, CoarseArgs{}));
    st.stages_done = st.stages_unique = st.stages_all;
    return LGR_OK;
}

// ---- section 3b: lower bounds, pass 0 (nearest tiles), upper bounds, the final pass (everything the bounds cannot exclude)
// ball bounds: on the matrix cores from the packed operands (f16 formats; the leaf centres were packed as train rows ahead of the operand
// packing, on the third stream), with packed FMAs from the sorted rows otherwise
int MatchCall::lower_bounds() {
    if (sB.live) LGR_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev[27], 0));   // the cleared workspace, the packed centres
    if (!f16) {
        LGR_TRY(join_sorted());   // lb_kernel reads sortedA
        lb_kernel<<<n_rb, 256, 0, ctx->stream>>>(sortedA, A.perm, cen2, B.r2max, B.leaf_count, n_leaves, W.LBsq);
    } else if (os.rot) {
        lb_mfma_kernel<FMT_F16R><<<n_rb, LBM_THREADS, 0, ctx->stream>>>((const f16x8*) Aop, W.cop, cset_stride, os.out_scale, A.blkcl, nAp, W.cnrm, os.ex,
                                                                        B.r2max, B.leaf_count, n_leaves, n_cpad, W.LBsq);
    } else {
        lb_mfma_kernel<FMT_F16><<<n_rb, LBM_THREADS, 0, ctx->stream>>>((const f16x8*) Aop, W.cop, cset_stride, os.out_scale, A.blkcl, nAp, W.cnrm, os.ex,
                                                                       B.r2max, B.leaf_count, n_leaves, n_cpad, W.LBsq);
    }
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}
// coarse rejection inside match_mfma (rotated format, passes with upper bounds): thresholds from u_rb / u_stage; and the shell bound of
// the masked passes that have upper bounds (with the coarse rejection: the same "an entry may miss what lies above the U^2 of its row and
// column" contract, and the same upper-bound tables)
int MatchCall::coarse_setup() {
    colstage = both && mo.column_stage != 0;
    coarse = f16 && os.rot && mo.coarse_rejection != 0;
    if (coarse) {
        // stage shells and stage maxima from the tiles' shells (behind the packing, on its stream)
        shell_reduce_kernel<<<cdiv((long long) KCL * n_stage_total, 256), 256, 0, sB.s>>>(shellB, KCL, tb, STAGE_TILES, W.stage_shell, W.smaxB);
        LGR_HIP(ctx, hipMemsetAsync(W.coarse_cnt, 0, 32, ctx->stream));
        ca_on = coarse_constants(os);
        ca_on.xmax = gmaxA; ca_on.ymax = W.smaxB; ca_on.n_stage_total = n_stage_total;
        ca_on.cnt = W.coarse_cnt;
    }
    if (coarse && mo.shell_bound != 0) {
        shell_reduce_kernel<<<cdiv(n_rb, 256), 256, 0, ctx->stream>>>(shellA, 1, ta, BLOCK_ROWS / TILE, W.rb_shell, nullptr);
        shell.rshA = W.rb_shell; shell.sshB = W.stage_shell;
        shell.blkcl = A.blkcl; shell.u_rb = W.u_rb; shell.cols = both ? 1 : 0;
        ca_on.rt_shell = shellA; ca_on.ct_shell = shellB;   // ... and per tile for the test inside the coarse sweep
    }
    shell0 = shell;   // pass 0: the stages of overlapping shells only
    shell0.u_rb = nullptr;
    sched_final = W.sched;
    comp_rows = CompView{W.comp_r, n_groups, nullptr};
    comp_cols = CompView{W.comp_c, n_rg, tile_leaf};
    return LGR_OK;
}
CoarseArgs MatchCall::with_bounds() const {
    CoarseArgs ca = ca_on;
    ca.u_rb = W.u_rb; ca.u_rt = W.u_rt; ca.u_row = W.u_row; ca.u_stage = both ? W.u_stage : nullptr; ca.u_ct = W.u_ct; ca.u_colv = both ? W.u_colv : nullptr; ca.n_ct_total = tb;
    return ca;
}
static int launch_near(const MatchCall& c, int n_vec, int len, size_t vs, size_t es, unsigned long long* lbstat, const uint2* lb_part) {
    const PruneWs& W = c.W;
    const float widen_frac = c.mo.auto_dense ? LGR_AUTO_DENSE_FRAC : 0.f;
    if (len <= NEAR_LDS_MAX) {
        if ((size_t) len * 4 > 64 * 1024)
            LGR_HIP(c.ctx, hipFuncSetAttribute((const void*) near_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, len * 4));
        near_kernel<true><<<n_vec, NEAR_THREADS, (size_t) len * 4, c.ctx->stream>>>(c.near_t, W.LBsq, n_vec, len, vs, es, W.sched, vs, es, lbstat, lb_part, c.n_rb, widen_frac);
    } else {
        near_kernel<false><<<n_vec, NEAR_THREADS, 0, c.ctx->stream>>>(c.near_t, W.LBsq, n_vec, len, vs, es, W.sched, vs, es, lbstat, lb_part, c.n_rb, widen_frac);
    }
    return LGR_OK;
}
// do the bounds separate anything?  (zero / finite lower bounds: counted by box_lb_kernel where it writes the final bounds, by lb_stats_kernel
// without boxes; near_kernel: when nearly every lower bound is zero, pass 0 takes everything)
// pass 0's schedule: the NEAR_T nearest leaves of every row block and the NEAR_T nearest row blocks of every leaf
int MatchCall::near_schedule() {
    unsigned long long* lbstat = &W.stats->stages[5];   // [5] zero, [6] finite lower bounds (MaskStats slots the passes do not use)
    uint2* lb_part = boxes ? W.lb_part : nullptr;
    if (boxes) {
        LGR_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev[30], 0));
        box_lb_kernel<<<n_rb, 256, 0, ctx->stream>>>(boxA, boxBt, n_leaves, rmax2, W.LBsq, lb_part);
    } else {
        lb_stats_kernel<<<std::min(cdiv((long long) n_rb * n_leaves, 1024), 1024), 256, 0, ctx->stream>>>(W.LBsq, (size_t) n_rb * n_leaves, lbstat);
    }
    LGR_TRY(launch_near(*this, n_rb, n_leaves, (size_t) n_leaves, 1, lbstat, lb_part));
    return launch_near(*this, n_leaves, n_rb, 1, (size_t) n_leaves, lbstat, lb_part);
}
void MatchCall::build_comp() {
    comp_rows_kernel<<<cdiv((long long) n_rb * n_groups, 256), 256, 0, ctx->stream>>>(W.done, sched_final, group_leaf, n_rb, n_leaves, n_groups, W.comp_r);
    if (both) comp_cols_kernel<<<cdiv((long long) n_leaves * n_rg, 256), 256, 0, ctx->stream>>>(W.done, sched_final, n_rb, n_leaves, n_rg, rg_rows / BLOCK_ROWS, W.comp_c);
}
// passes 1..: what the passes so far computed, the upper bounds from it, the pass's schedule
int MatchCall::upper_bounds_schedule(int pass) {
    build_comp();
    row_u_kernel<<<n_rb, BLOCK_ROWS, (size_t) (n_groups + 8) * 4, ctx->stream>>>((const float*) rowmin, n_groups, ma_pad, A.perm, nAp, A.blkcl, gmaxB, os.ex, comp_rows, W.u_rb, W.u_rt, coarse ? W.u_row : nullptr);
    if (both) {
        LGR_HIP(ctx, hipMemsetAsync(W.u_leaf, 0, (size_t) MAXLEAF * 4, ctx->stream));
        LGR_HIP(ctx, hipMemsetAsync(W.u_stage, 0, (size_t) n_stage_total * 4, ctx->stream));
        col_u_kernel<<<cdiv(mb_pad, 256), 256, (size_t) (n_rg + 8) * 4, ctx->stream>>>((const float*) colmin, n_rg, mb_pad, B.perm, nBp, gmaxA, cl_of_rg, tile_leaf, os.ex, comp_cols, W.u_leaf,
                                                                                       (colstage || coarse) ? W.u_stage : nullptr, coarse ? W.u_ct : nullptr, coarse ? W.u_colv : nullptr);
    }
    float bsq = betas[pass - 1] * betas[pass - 1];
    sched_kernel<<<cdiv((long long) n_rb * n_leaves, 256), 256, 0, ctx->stream>>>(both ? 1 : 0, bsq, W.LBsq, W.u_rb, W.u_leaf, n_rb, n_leaves,
                                                                                colstage && pass == n_beta ? 1 : 0, pass == 1 && shell0.rshA ? 1 : 0, W.done, W.sched);
    return LGR_OK;
}
// the table initialisation of the pass needs the schedule only: on the third stream, beside the stage masks (0.27 + 0.28 ms in a row
// in front of pass 0, 0.30 + 0.37 between the passes); build_masks makes the MFMA launch wait for both
// (the final pass as sweep + listed tiles: initialised behind the sweep, for the pairs its list touches -- init_touched_tables)
int MatchCall::init_pass_tables(int pass) {
    defer_init = pass == n_beta && pass > 0 && f16 && os.rot && coarse && kept != nullptr;
    if (defer_init) { sched_final = W.touched; return LGR_OK; }
    LGR_TRY(sB.fork(ctx->ev[28]));
    init_tables_sparse_kernel<<<cdiv((long long) n_rb * n_leaves, 256), 256, 0, sB.s>>>(W.sched, W.done, n_rb, n_leaves, leaf_g0, group_start, rg_rows / BLOCK_ROWS, rowmin,
                                                                                        (size_t) ma_pad, colmin, (size_t) mb_pad);
    if (sB.live) LGR_HIP(ctx, hipEventRecord(ctx->ev[29], sB.s));
    return LGR_OK;
}
// the pass's stage masks from the scheduled (row block, leaf) pairs (mask_sparse_kernel; 0.41 + 0.30 -> 2 x ~0.1 ms at 1M), their statistics,
// and the join of the pass's table initialisation
int MatchCall::build_masks(int pass) {
    if (pass == 0 && shell0.rshA) LGR_TRY(sB.join());   // (the stage shells come from the column norms, written by the packing)
    if (pass == 0) {
        LGR_HIP(ctx, hipMemsetAsync(W.leaf_first, 0x7f, (size_t) MAXLEAF * 4, ctx->stream));
        LGR_HIP(ctx, hipMemsetAsync(W.leaf_last, 0xff, (size_t) MAXLEAF * 4, ctx->stream));
        leaf_stage_range_kernel<<<cdiv(tb, 256), 256, 0, ctx->stream>>>(tile_leaf, tb, n_leaves, W.leaf_first, W.leaf_last);
    }
    const long long n_pairs_m = (long long) n_rb * n_cc;
    LGR_HIP(ctx, hipMemsetAsync(W.mask, 0, (size_t) n_pairs_m * 4, ctx->stream));
    mask_sparse_kernel<<<cdiv((long long) n_rb * n_leaves, 256), 256, 0, ctx->stream>>>(W.sched, W.leaf_first, W.leaf_last, n_rb, n_cc, n_leaves, n_stage_total, W.LBsq, W.u_stage,
                                                                                        pass > 0 ? shell : shell0, W.mask);
    if (mo.self_check) {   // (tests) mask_kernel's masks must be the same words; its bookkeeping goes to scratch
        unsigned* chk_mask = W.mask_chk;
        unsigned* chk_acc = chk_mask + n_pairs_m;
        unsigned* n_diff = chk_acc + n_pairs_m;
        LGR_HIP(ctx, hipMemsetAsync(chk_acc, 0, (size_t) n_pairs_m * 4 + 64, ctx->stream));
        mask_kernel<<<std::min(cdiv(n_pairs_m * 32, 256), 4096), 256, 0, ctx->stream>>>(pass, W.sched, tile_leaf, n_rb, n_cc, n_leaves, n_stage_total, W.LBsq, W.u_stage,
                                                                                         pass > 0 ? shell : shell0, chk_mask, chk_acc, W.scratch_stats());
        mask_compare_kernel<<<cdiv(n_pairs_m, 256), 256, 0, ctx->stream>>>(W.mask, chk_mask, n_pairs_m, n_diff);
        unsigned h_diff = 0;
        LGR_HIP(ctx, hipMemcpyAsync(&h_diff, n_diff, 4, hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (h_diff) { ctx->err = "matcher self-check: the sparse stage masks differ from mask_kernel's"; return LGR_ERR_HIP; }
    }
    mask_stats_kernel<<<std::min(cdiv(n_pairs_m, 256), 256), 256, 0, ctx->stream>>>(pass, W.mask, W.mask_acc, n_pairs_m, W.stats);
    if (sB.live && !defer_init) LGR_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev[29], 0));
    return LGR_OK;
}
int MatchCall::run_pruned() {
    LGR_TRY(lower_bounds());
    LGR_TRY(coarse_setup());
    LGR_TRY(near_schedule());
    LGR_TRY(sB.record());   // sB: the column operands, their maxima and shells, the rerank's tables -- everything a reader of sB.join() waits for.  (Recorded
                            //  behind the last PRODUCER, not where the first reader joins: by then sB also holds pass 0's init_tables_sparse_kernel, which
                            //  the stage masks are meant to run beside, not behind; it has an event of its own)
    for (int pass = 0; pass <= n_beta; ++pass) {
        if (pass > 0) LGR_TRY(upper_bounds_schedule(pass));
        LGR_TRY(init_pass_tables(pass));
        LGR_TRY(build_masks(pass));
        cur_pass_stages = &W.stats->stages[pass];
        if (pass == 0) LGR_TRY(launch_sorted_copies(true));
        LGR_TRY(launch_mfma(W.mask, coarse && pass > 0 ? with_bounds() : ca_on));
    }
    build_comp();   // final state for the rerank scans
    chk = CheckView{W.done, sched_final, W.LBsq, colstage ? W.u_stage : nullptr, coarse ? W.u_row : nullptr, coarse && both ? W.u_colv : nullptr};
    return read_back_stats();
}
// the passes' statistics; and the repair of a final pass whose sweep kept more tiles than its list holds
int MatchCall::read_back_stats() {
    MaskStats* hs;
    LGR_TRY(lgr_pinned(ctx, 256, (void**) &hs));
    LGR_HIP(ctx, hipMemcpyAsync(hs, W.stats, sizeof(MaskStats), hipMemcpyDeviceToHost, ctx->stream));
    unsigned long long* h_cc = (unsigned long long*) ((char*) hs + 128);
    h_cc[0] = h_cc[1] = h_cc[2] = 0ull;
    if (coarse) LGR_HIP(ctx, hipMemcpyAsync(h_cc, W.coarse_cnt, 24, hipMemcpyDeviceToHost, ctx->stream));
    unsigned long long* h_kept = (unsigned long long*) ((char*) hs + 192);
    h_kept[0] = 0ull;
    if (split_used) LGR_HIP(ctx, hipMemcpyAsync(h_kept, kept_count, 8, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (split_used && h_kept[0] > (unsigned long long) kept_cap) {
        // The sweep kept more tiles than the list holds (descriptors without structure): the last pass again on the fused kernel.  The
        // tables only ever take minima, so what the listed tiles already contributed stays valid.  (Statistics: the fused launch's.)
        LGR_HIP(ctx, hipMemsetAsync(W.coarse_cnt, 0, 32, ctx->stream));
        // (touched_kernel saw the overflow: it marked, and init_tables_sparse_kernel initialised, every scheduled pair -- the fused kernel finds its tables ready)
        LGR_TRY(launch_mfma(W.mask, with_bounds(), false));
        LGR_HIP(ctx, hipMemcpyAsync(h_cc, W.coarse_cnt, 24, hipMemcpyDeviceToHost, ctx->stream));
        LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    st.coarse_tested = (double) h_cc[0];
    st.coarse_rejected = (double) h_cc[1];
    st.shell_skipped = (double) h_cc[2];
    st.stages_done = 0;
    for (int k = 0; k <= n_beta; ++k) st.stages_done += (double) hs->stages[k];
    st.stages_unique = (double) hs->stages[7];
    st.lb_zero = (double) hs->stages[5]; st.lb_finite = (double) hs->stages[6];
    if (env_int("LGR_MATCH_DEBUG", 0)) LGR_TRY(match_debug_report(*this, hs, h_kept));
    return LGR_OK;
}

// irregular rows: every pair they are part of, both roles (irregular_scan); the exact rerank never sees them
int MatchCall::irregular_rows() {
    const int nb_a = (ma + block - 1) / block, nb_b = (mb + block - 1) / block;
    if (B.n_irr) irregular_scan<<<cdiv(ma, 256), 256, 0, ctx->stream>>>(d_a, A.valid, ma, d_b, B.irr_list, B.n_irr, block, nb_a, nb_b, bestA, both ? bestB : nullptr);
    if (A.n_irr) irregular_scan<<<cdiv(mb, 256), 256, 0, ctx->stream>>>(d_b, B.valid, mb, d_a, A.irr_list, A.n_irr, block, nb_b, nb_a, both ? bestB : nullptr, bestA);
    return LGR_OK;
}
// lgr_match_options.self_check (tests): the filtered tables against the exact distances, and what the check covered (lgr_match_last_check*)
int MatchCall::self_check(const CheckView& v) {
    unsigned* d_worst = (unsigned*) (misc + 192);
    unsigned long long* d_cover = (unsigned long long*) (misc + 3840);   // [2][CHECK_N] (behind the level-1 centres, inside the first 4 KB)
    static_assert(2 * CHECK_N == 8, "lgr_match_last_check_cover reports four counters per direction");
    LGR_HIP(ctx, hipMemsetAsync(d_worst, 0, 8, ctx->stream));
    LGR_HIP(ctx, hipMemsetAsync(d_cover, 0, 2 * CHECK_N * 8, ctx->stream));
    const int stride = mo.self_check >= 2 ? 1 : 37;   // 2: every query (test sizes); 1: every 37th
    check_kernel<true><<<cdiv(ma_pad, stride), 256, (size_t) (n_groups + 8) * 4, ctx->stream>>>(
        (const float*) rowmin, n_groups, ma_pad, 0, group_start, sortedA, A.perm, sortedB, B.perm, mb_pad, nAp, A.blkcl, nullptr, gmaxB, nullptr,
        os.ex, comp_rows, stride, nullptr, nullptr, 0, nullptr, nullptr, v.uq_rows, v.uq_cols, d_worst, d_cover);
    if (both)
        check_kernel<false><<<cdiv(mb_pad, stride), 256, (size_t) (n_rg + 8) * 4, ctx->stream>>>(
            (const float*) colmin, n_rg, mb_pad, rg_rows, nullptr, sortedB, B.perm, sortedA, A.perm, ma_pad, nullptr, nullptr, nBp, gmaxA, cl_of_rg,
            os.ex, comp_cols, stride, v.done, v.sched, n_leaves, v.lb, v.ustage, v.uq_rows, v.uq_cols, d_worst + 1, d_cover + CHECK_N);
    unsigned* hw;
    LGR_TRY(lgr_pinned(ctx, 128, (void**) &hw));
    LGR_HIP(ctx, hipMemcpyAsync(hw, d_worst, 8, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipMemcpyAsync(hw + 16, d_cover, 2 * CHECK_N * 8, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float r0, r1;
    memcpy(&r0, hw, 4); memcpy(&r1, hw + 1, 4);
    ctx->mcheck[0] = r0; ctx->mcheck[1] = r1;
    memcpy(ctx->mcover, hw + 16, (both ? 2 : 1) * CHECK_N * 8);
    return LGR_OK;
}
// ---- 5. exact rerank
int MatchCall::rerank() {
    // (the MFMA re-filter of the rerank items needs the f16 operand formats and the padded train copies)
    RefilterArgs ra{(const f16x8*) Aop, (const f16x8*) Bop, bset_stride, os.out_scale, (f16 && mo.rerank_refilter) ? KS : 0, A.blkcl, mo.pair_cap};
    auto rerank_ab = [&](lgr_ctx* cx) {
        return run_rerank<true>(cx, os.ex, comp_rows, (const float*) rowmin, n_groups, 0, group_start, d_a, A, nAp, nullptr, gmaxB, nullptr, d_b, sortedB, B, block, bestA,
                                d_ab_idx, d_ab_dist, &st.items_ab, &st.dense_ab, force_dense, ra, &st.pairs_ab);
    };
    auto rerank_ba = [&](lgr_ctx* cx) {
        return run_rerank<false>(cx, os.ex, comp_cols, (const float*) colmin, n_rg, rg_rows, nullptr, d_b, B, nullptr, nBp, gmaxA, cl_of_rg, d_a, sortedA, A, block, bestB,
                                 d_ba_idx, d_ba_dist, &st.items_ba, &st.dense_ba, force_dense, ra, &st.pairs_ba);
    };
    if (both) return lgr_run_pair(ctx, rerank_ab, rerank_ba);   // the two directions' exact reranks are independent
    return rerank_ab(ctx);
}

static int match_impl(lgr_ctx* ctx, const float* d_a, int ma, const float* d_b, int mb, int block,
                      int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist) {
    LGR_CHECK(ctx, ctx && (d_a || ma == 0) && (d_b || mb == 0) && (d_ab_idx || ma == 0) && (d_ab_dist || ma == 0), LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, ma >= 0 && mb >= 0 && block > 0, LGR_ERR_INVALID_ARG);
    if (d_ba_idx) LGR_CHECK(ctx, d_ba_dist != nullptr, LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    memset(&ctx->mstats, 0, sizeof ctx->mstats);
    ctx->mcheck[0] = ctx->mcheck[1] = -1;
    for (unsigned long long& c : ctx->mcover) c = ~0ull;
    ctx->mpack[0] = ctx->mpack[1] = ~0ull;
    ctx->mfma_timed = 0;
    // default result: unmatched
    if (ma) { LGR_HIP(ctx, hipMemsetAsync(d_ab_idx, 0xff, (size_t) ma * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(d_ab_dist, 0, (size_t) ma * 4, ctx->stream)); }
    if (mb && d_ba_idx) { LGR_HIP(ctx, hipMemsetAsync(d_ba_idx, 0xff, (size_t) mb * 4, ctx->stream)); LGR_HIP(ctx, hipMemsetAsync(d_ba_dist, 0, (size_t) mb * 4, ctx->stream)); }
    if (ma == 0 || mb == 0) return LGR_OK;

    MatchCall c(ctx, d_a, ma, d_b, mb, block, d_ab_idx, d_ab_dist, d_ba_idx, d_ba_dist);
    LGR_TRY(c.build_sides());            // 1. + 2. clusters, leaves, both sides sorted and placed
    if (c.A.n_valid == 0 || c.B.n_valid == 0) return LGR_OK;
    LGR_TRY(c.start_aux());              // aux stream: the boxes (the sorted copies follow under pass 0)
    LGR_TRY(c.choose_format());          // 3. operand format, scales, error terms
    LGR_TRY(c.upload_group_tables());    //    column groups; the one host wait of the set-up
    LGR_TRY(c.prepare_prune_ws());       //    third stream: the pruning workspace cleared, the leaf centres packed
    LGR_TRY(c.pack_operands());          //    row operands on the main stream, column operands on the third
    LGR_TRY(c.alloc_tables());           // 4. minimum tables, work items, the sweep's tile list
    LGR_TRY(c.prune ? c.run_pruned() : c.run_dense());
    LGR_HIP(ctx, hipGetLastError());
    LGR_TRY(c.join_sorted());            // the self-check and the exact rerank read the sorted rows
    LGR_TRY(c.irregular_rows());
    if (c.mo.self_check && c.sortedA) LGR_TRY(c.self_check(c.chk));
    return c.rerank();                   // 5. exact distances, the reference's tie rules
}

// duration of the match_mfma launch(es) of the last match call in ms (hipEvents on the ctx stream); -1 if none
extern "C" int lgr_match_last_kernel_ms(lgr_ctx* ctx, float* ms) {
    if (!ctx || !ms) return LGR_ERR_INVALID_ARG;
    *ms = -1.f;
    if (!ctx->mfma_timed) return LGR_OK;
    *ms = 0.f;
    for (int k = 0; k < ctx->mfma_timed; ++k) {   // one event pair per masked pass
        float t = 0.f;
        LGR_HIP(ctx, hipEventSynchronize(ctx->ev[10 + 2 * k]));
        LGR_HIP(ctx, hipEventElapsedTime(&t, ctx->ev[9 + 2 * k], ctx->ev[10 + 2 * k]));
        if (env_int("LGR_MATCH_DEBUG", 0)) fprintf(stderr, "[lgr] match_mfma pass %d: %.2f ms\n", k, t);
        *ms += t;
    }
    return LGR_OK;
}

extern "C" int lgr_match_bf_dev(lgr_ctx* ctx, const float* d_q33, int mq, const float* d_t33, int mt, int block,
                                int32_t* d_idx, float* d_dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    return match_impl(ctx, d_q33, mq, d_t33, mt, block, d_idx, d_dist, nullptr, nullptr);
}

extern "C" int lgr_match_bf2_dev(lgr_ctx* ctx, const float* d_a33, int ma, const float* d_b33, int mb, int block,
                                 int32_t* d_ab_idx, float* d_ab_dist, int32_t* d_ba_idx, float* d_ba_dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (d_ba_idx && d_ba_dist) || mb == 0, LGR_ERR_INVALID_ARG);
    return match_impl(ctx, d_a33, ma, d_b33, mb, block, d_ab_idx, d_ab_dist, d_ba_idx, d_ba_dist);
}

extern "C" int lgr_match_bf(lgr_ctx* ctx, const float* q33, int mq, const float* t33, int mt, int block,
                            int32_t* idx, float* dist) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (q33 || mq == 0) && (t33 || mt == 0) && (idx || mq == 0) && (dist || mq == 0) && mq >= 0 && mt >= 0, LGR_ERR_INVALID_ARG);
    float *dq, *dt, *dd;
    int32_t* di;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.in(q33, (size_t) mq * 33, &dq));
    LGR_TRY(hc.in(t33, (size_t) mt * 33, &dt));
    LGR_TRY(hc.out((size_t) mq, &di));
    LGR_TRY(hc.out((size_t) mq, &dd));
    LGR_TRY(lgr_match_bf_dev(ctx, dq, mq, dt, mt, block, di, dd));
    LGR_TRY(hc.fetch(idx, di, (size_t) mq));
    LGR_TRY(hc.fetch(dist, dd, (size_t) mq));
    return hc.finish();
}
