// lgr_ransac_schedule.cuh -- the loop of the prerejective RANSAC driven from the device: its state (RState), the bodies and kernels of a
// round's phases (rs_begin, rs_hyp, rs_cand, rs_replay), the resident kernel that runs them behind grid barriers, the plane metrics'
// rs_plane_* kernels and the second pass' mh_* kernels (the set of distinct hypotheses; mh_plane_*: its final block under a plane metric).
// Part of lgr_ransac.hip's one translation unit; see its header for the schedule and DESIGN.md section 5.
#pragma once
#include <climits>

#include "lgr_ransac_count.cuh"
#include "lgr_ransac_metric.cuh"

namespace {

constexpr int MAX_ROUND_BATCHES = 16;   // batches of the schedule evaluated per round of launches

// ---------------------------------------------------------------------------------------------------- device-driven schedule
// The whole loop of SampleConsensusPrerejectiveOMP::align (src/sac_prerejective_omp.cpp:156-257) without the host in it, for all five
// metrics (round 4; the plane metrics since round 5).  The schedule's state -- iterations done, the adaptive bound, the record inlier set,
// the best metric and transform -- lives in an RState on the device.  A ROUND (the first: one batch; then up to MAX_ROUND_BATCHES) is six
// launches whose sizes are upper bounds and whose real extents are read from the RState:
//   rs_begin    the round's iteration range, the candidate gate, counters cleared
//   rs_hyp      sample -> prerejection -> 3-point transform; survivors appended to a list (one atomic per wave; ANY list order gives the
//               same results: every later reduction carries the iteration number as its tie-break)
//   count_list  the O(H x C) verification over (hypothesis block, chunk) items, a fixed grid striding over them
//   rs_cand     hypotheses with enough inliers for the gate -> candidate list
//   metric      the metric of every candidate, a fixed grid striding over them
//   rs_replay   per-batch statistics, then ONE lane replays the round's batches in schedule order exactly as the reference's loop: best hypothesis
//               (strict >, ties -> lowest iteration), record inlier set -> estimateMaxIterations (src/metric.cpp:103-123, in double) ->
//               bound, batches behind the end of the loop discarded
// (the plane metrics add the plane evaluation and the rs_plane_* kernels below) and every kernel returns at once when the loop has ended.
// The host enqueues two rounds and, for uniformity / correspondences, the final block (evaluation of the best transform, refit over its
// inliers, evaluation of the refit: also sized on the device) blind and then reads ONE record; when the loop has not ended by then
// (max_iterations far above two rounds and no record yet) it repeats.  The plane metrics' final block is the caller's (lgr_ransac_ex_dev):
// its refit needs the plane pairs sorted by source index on the host.  The adaptive bound is evaluated with the
// device's double-precision log / pow, the oracle with libm's: both are accurate to an ulp, the bound is the integer part of a quotient of
// the two, so a difference needs a quotient within ~1e-15 of an integer.
struct RState {
    int done, bound, max_iterations, batch, round_cap;
    int largest, num_rejections, best_iter;
    float final_metric;
    int min_inliers;
    int round_first, round_nb, round_batches;
    int n_ok, n_cand;
    int stop;
    int rounds;
    int metric_id, c, nr_samples;
    float confidence;
    unsigned bar_count, bar_gen; int abort;                   // the resident kernel's grid barrier (arrivals, generation) and its time-out flag
    float best_T[16];
    float Tn[16];
    float e_metric; int e_ninl; float e_rmse; int pad1;       // evaluation of best_T (the final block, :265-296)
    float e2_metric; int e2_ninl; float e2_rmse; int pad2;    // evaluation of the refit
    int int_max, tot_ok, tot_cand, n_gated;                    // (int_max: a constant the plane gate reads where the records are not plane counts; tot_*: survivors / candidates over all rounds, for LGR_RANSAC_DEBUG; n_gated: hypotheses the plane gate abandoned, lgr_ransac_last_plane_gate)
    unsigned long long phase_ticks[8];                         // resident kernel: 100 MHz ticks workgroup 0 spent per phase incl. its barrier (begin/replay, hyp, count, cand, metric)
    unsigned long long busy_max[8], busy_sum[8];               // ... and the workgroups' own work per phase (without the barrier): maximum and sum over the workgroups
};

__device__ __noinline__ int est_from_support_dev(int count, int c, float confidence, int nr_samples) {   // src/metric.cpp:116-122 given the support count
    // (a real call: inlined, its double-precision log / pow bring ~100 registers of constants that the resident kernel's loop would carry)
    float frac = (float) count / (float) c;
    frac /= 4.f;
    if (frac <= 0.0 || log(1.0 - pow((double) frac, (double) nr_samples)) >= 0.0) return INT_MAX;
    const double iterations = log(1.0 - (double) confidence) / log(1.0 - pow((double) frac, (double) nr_samples));
    return (int) fmin((double) INT_MAX, iterations);
}

__device__ __noinline__ int rs_gate_dev(float final_metric, int metric_id, int c) {   // (a real call for the same reason as est_from_support_dev)
    int mi = MIN_NR_INLIERS;
    if (final_metric > 0.f && metric_id == LGR_METRIC_UNIFORMITY) mi = max(mi, (int) floor(pow(10000.0, (double) final_metric / 1.001)) - 1);
    else if (final_metric > 0.f && metric_id == LGR_METRIC_CORRESPONDENCES) mi = max(mi, (int) floor((double) final_metric * (double) c / 1.001) - 1);
    return mi;
}
__device__ __forceinline__ void rs_begin_body(RState* S, int first_round) {
    if (threadIdx.x != 0) return;
    S->n_ok = 0; S->n_cand = 0; S->round_nb = 0; S->round_batches = 0;
    if (S->stop) return;
    if (S->done >= S->bound || S->done >= S->max_iterations) { S->stop = 1; return; }
    const long long want = (long long) min(S->bound, S->max_iterations) - S->done;
    int n_batches = first_round ? 1 : (int) min((long long) S->round_cap, (want + S->batch - 1) / S->batch);
    const int nb = (int) min((long long) n_batches * S->batch, (long long) S->max_iterations - S->done);
    n_batches = (nb + S->batch - 1) / S->batch;
    // candidate gate (see lgr_ransac_dev): a hypothesis whose metric cannot reach the best one so far is not scored
    int mi = rs_gate_dev(S->final_metric, S->metric_id, S->c);
    // ... and it must not hide a RECORD inlier set (:224-228 feed the adaptive bound from every hypothesis with >= MIN_NR_INLIERS): only counts
    // up to the record so far are safe to drop.  When the best metric is a loop hypothesis's, its own count already is >= the gate and <= the
    // record, so this changes nothing; a GUESS (:134-147) sets the metric to beat without ever entering the record.
    mi = min(mi, max(MIN_NR_INLIERS, S->largest + 1));
    S->min_inliers = mi;
    S->round_first = S->done; S->round_nb = nb; S->round_batches = n_batches;
    S->rounds += 1;
}
__global__ void rs_begin_kernel(RState* __restrict__ S, int first_round) { rs_begin_body(S, first_round); }

// iteration `b` of the round (b - lane is wave-uniform; a wave wholly behind the round's end does nothing)
// (round 5: the sampled pairs come from the packed correspondences -- P0[i].xyz / P1[i].xyz ARE the source / target point of correspondence i, 32
// contiguous bytes per sample in a 9 MB array instead of a 16-byte record and two 12-byte gathers out of the 48 MB clouds)
template <int NS>
__device__ __forceinline__ void rs_hyp_item(const int b, const float4* __restrict__ P0, const float4* __restrict__ P1, int c,
                                            unsigned long long seed, RState* S, float edge_thr, float* Ts, int* list, int* posmap, int2* counts) {
    const int nb = S->round_nb;
    bool good = false;
    if (b < nb) {
        counts[b] = make_int2(0, 0);   // (list positions are < the survivors' number <= nb)
        int r[NS], smp[NS];
        draws_n<NS>(seed, (unsigned) (S->round_first + b), r);
        select_n<NS>(r, c, smp);
        P3 s[NS], t[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) { const float4 a = P0[smp[j]], q = P1[smp[j]]; s[j] = P3{a.x, a.y, a.z}; t[j] = P3{q.x, q.y, q.z}; }
        good = poly_ok<NS>(s, t, edge_thr * edge_thr);
        if (good) {
            float T[16];
            umeyama_n<NS>(s, t, T);
            float4* o = reinterpret_cast<float4*>(Ts + (size_t) b * 16);
            o[0] = make_float4(T[0], T[1], T[2], T[3]); o[1] = make_float4(T[4], T[5], T[6], T[7]);
            o[2] = make_float4(T[8], T[9], T[10], T[11]); o[3] = make_float4(T[12], T[13], T[14], T[15]);
        }
    }
    const unsigned long long m = __ballot(good);
    if (m == 0ull) return;
    int base = 0;
    const int lane = threadIdx.x & 63;
    if (lane == 0) base = atomicAdd(&S->n_ok, __popcll(m));
    base = __shfl(base, 0);
    if (good) {
        const int pos = base + __builtin_amdgcn_mbcnt_hi((unsigned) (m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) m, 0u));
        list[pos] = b;
        posmap[b] = pos;
    }
}
template <int NS>
__global__ void rs_hyp_kernel(const float4* __restrict__ P0, const float4* __restrict__ P1, int c,
                              unsigned long long seed, RState* __restrict__ S, float edge_thr, float* __restrict__ Ts, int* __restrict__ list,
                              int* __restrict__ posmap, int2* __restrict__ counts) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b - (int) threadIdx.x >= S->round_nb) return;   // (whole workgroup; S->stop leaves round_nb = 0)
    rs_hyp_item<NS>(b, P0, P1, c, seed, S, edge_thr, Ts, list, posmap, counts);
}

// candidates = survivors with enough inliers for the gate.  Up to 2^17 survivors ONE workgroup compacts them in list order (an ordered
// block scan per 1024 survivors): the metric kernel walks the inlier-mask column hpos[candidate] of every candidate, a 4-byte read per
// 128 KB row -- neighbouring workgroups then share the cache lines of neighbouring columns (with the candidates in arrival order of an
// atomic append the same launch took 1.9 instead of 0.5 ms at 9.5 k candidates).  Beyond that all workgroups append unordered.
__device__ __forceinline__ void rs_cand_body(const int tid, const int wg, const int n_wg, RState* S, const int2* counts, const int* list, int* list2, int* hpos) {
    __shared__ int scan[1024 / 64 + 2];
    const int n_ok = S->n_ok, mi = S->min_inliers;
    if (n_ok <= (1 << 17)) {
        if (wg != 0) return;
        int total = 0;
        for (int h0 = 0; h0 < n_ok; h0 += 1024) {
            const int h = h0 + tid;
            const bool cand = h < n_ok && counts[h].x >= mi;
            int tot;
            const int pos = total + block_excl_scan_1024(cand ? 1 : 0, scan, tid, &tot);
            if (cand) { list2[pos] = list[h]; hpos[pos] = h; }
            total += tot;
        }
        if (tid == 0) S->n_cand = total;
        return;
    }
    for (int h0 = wg * 1024; h0 < n_ok; h0 += n_wg * 1024) {
        const int h = h0 + tid;
        const bool cand = h < n_ok && counts[h].x >= mi;
        const unsigned long long m = __ballot(cand);
        if (m == 0ull) continue;
        int base = 0;
        if ((tid & 63) == 0) base = atomicAdd(&S->n_cand, __popcll(m));
        base = __shfl(base, 0);
        if (cand) {
            const int pos = base + __builtin_amdgcn_mbcnt_hi((unsigned) (m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned) m, 0u));
            list2[pos] = list[h];
            hpos[pos] = h;
        }
    }
}

__global__ __launch_bounds__(1024) void rs_cand_kernel(RState* __restrict__ S, const int2* __restrict__ counts, const int* __restrict__ list,
                                                       int* __restrict__ list2, int* __restrict__ hpos) {
    rs_cand_body(threadIdx.x, blockIdx.x, gridDim.x, S, counts, list, list2, hpos);
}

__device__ __forceinline__ void rs_replay_body(const int tid, RState* S, const int* list, const int* list2, const float* metric, const int* ninl, const int2* counts,
                                               const int* posmap, const float* Ts) {
    __shared__ unsigned long long best_key[MAX_ROUND_BATCHES], rec_key[MAX_ROUND_BATCHES];
    __shared__ int n_ok_b[MAX_ROUND_BATCHES];
    if (S->stop || S->round_nb == 0) return;
    if (tid == 0) { S->tot_ok += S->n_ok; S->tot_cand += S->n_cand; }
    if (tid < MAX_ROUND_BATCHES) { best_key[tid] = 0ull; rec_key[tid] = 0ull; n_ok_b[tid] = 0; }
    __syncthreads();
    const int batch = S->batch, n_ok = S->n_ok, n_cand = S->n_cand;
    for (int j = tid; j < n_cand; j += blockDim.x) {
        const unsigned off = (unsigned) list2[j];
        const int bi = (int) (off / (unsigned) batch);
        atomicMax(&best_key[bi], ((unsigned long long) __float_as_uint(metric[j]) << 32) | (0xffffffffu - off));
        atomicMax(&rec_key[bi], ((unsigned long long) (unsigned) ninl[j] << 32) | (0xffffffffu - off));
    }
    for (int h = tid; h < n_ok; h += blockDim.x) atomicAdd(&n_ok_b[list[h] / batch], 1);
    __syncthreads();
    if (tid != 0) return;
    int done = S->done, bound = S->bound, largest = S->largest, num_rej = S->num_rejections, best_iter = S->best_iter;
    float final_metric = S->final_metric;
    const int round_first = done, max_it = S->max_iterations;
    int best_off = -1;
    for (int j = 0; j < S->round_batches && done < bound; ++j) {
        const int nbj = min(batch, max_it - done);
        num_rej += nbj - n_ok_b[j];
        if (best_key[j]) {
            const float m = __uint_as_float((unsigned) (best_key[j] >> 32));
            const int off = (int) (0xffffffffu - (unsigned) (best_key[j] & 0xffffffffull));
            if (final_metric < m) { final_metric = m; best_iter = round_first + off; best_off = off; }   // src/sac_prerejective_omp.cpp:232-235 / :251-254
        }
        if (rec_key[j]) {
            const int rec_inl = (int) (rec_key[j] >> 32);
            if (rec_inl > largest) {   // :224-228
                largest = rec_inl;
                const int off = (int) (0xffffffffu - (unsigned) (rec_key[j] & 0xffffffffull));
                bound = min(bound, est_from_support_dev(counts[posmap[off]].y, S->c, S->confidence, S->nr_samples));
            }
        }
        done += nbj;
        if (done >= max_it) break;
    }
    if (best_off >= 0)
        for (int i = 0; i < 16; ++i) S->best_T[i] = Ts[(size_t) best_off * 16 + i];
    S->done = done; S->bound = bound; S->largest = largest; S->num_rejections = num_rej; S->best_iter = best_iter; S->final_metric = final_metric;
    if (done >= bound || done >= max_it) S->stop = 1;
}
__global__ __launch_bounds__(1024) void rs_replay_kernel(RState* __restrict__ S, const int* __restrict__ list, const int* __restrict__ list2,
                                                          const float* __restrict__ metric, const int* __restrict__ ninl, const int2* __restrict__ counts,
                                                          const int* __restrict__ posmap, const float* __restrict__ Ts) {
    rs_replay_body(threadIdx.x, S, list, list2, metric, ninl, counts, posmap, Ts);
}

// ---------------------------------------------------------------------------------------------------- the resident loop
// north_star's "persistent-thread RANSAC": the phases of a round above as ONE kernel whose workgroups stay resident for the whole loop and hand
// over at grid barriers.  One workgroup of 1024 threads per CU (the metric phase's shape: 117 KB of LDS for the uniformity histogram); the
// hypothesis phase strides threads over the round's iterations, the counting phase strides WAVES over the (hypothesis block, chunk) items,
// the candidate / replay phases run in workgroup 0, the metric phase strides workgroups over the candidates.  The state (RState) and every
// list live in global memory exactly as in the launch chain, so the results are the chain's bit for bit.
//   * barrier: arrivals counted with a device-scope atomic, the last arrival bumps a generation word the others poll with device-scope loads;
//     a release fence before arriving and an acquire fence after leaving carry the phase's plain stores across the XCDs' L2s.
//   * every wave reaches the end of the kernel: the loop runs at most `max_rounds` rounds (the host's bound: every round consumes at least one
//     batch), and a workgroup that polls longer than RS_BARRIER_TICKS of the 100 MHz wall clock sets `abort`, on which every workgroup leaves
//     at its next poll (the host then reports LGR_ERR_HIP; it cannot happen unless a workgroup of the grid never becomes resident).
constexpr unsigned long long RS_BARRIER_TICKS = 200000000ull;   // 2 s
__device__ __forceinline__ bool rs_grid_barrier(RState* S, const unsigned n_wg) {
    __shared__ int s_go;   // the workgroup's one reading of `abort` (every wave takes the same way out)
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();   // release: this workgroup's stores of the phase (the barrier above ordered the other waves' before this one)
        const unsigned gen = __hip_atomic_load(&S->bar_gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_fetch_add(&S->bar_count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == n_wg - 1u) {
            __hip_atomic_store(&S->bar_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&S->bar_gen, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            const unsigned long long t0 = wall_clock64();
            while (__hip_atomic_load(&S->bar_gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen) {
                __builtin_amdgcn_s_sleep(8);
                if (__hip_atomic_load(&S->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (wall_clock64() - t0 > RS_BARRIER_TICKS) { __hip_atomic_store(&S->abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
            }
        }
        __threadfence();   // acquire: the other workgroups' stores
        s_go = __hip_atomic_load(&S->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0;
    }
    __syncthreads();
    return s_go != 0;
}

// what the loop WRITES (and reads back in a later phase) travels in this struct; what it only reads are kernel arguments of their own with
// const __restrict__: only those may go through scalar loads (count_item's wave-uniform pair records) -- a pointer out of a struct carries
// no such promise, and the counting phase then fetched every record once per LANE (measured: twice the time, 80 spilled registers)
struct ResidentArgs {
    int c; int n_samples;
    unsigned long long seed; float edge_thr;
    RState* S;
    float* Ts; int* list; int* posmap; int2* counts; int* list2; int* hpos; float* metric; int* ninl;
    unsigned* maskT; int mask_cap; float2* scratch;
    int metric_id, score_id, max_rounds;
};

__global__ __launch_bounds__(MB) void rs_resident_kernel(const ResidentArgs a, const float* __restrict__ in_src, const float* __restrict__ in_tgt,
                                                         const lgr_corr* __restrict__ in_corr, const CPair* __restrict__ in_PP,
                                                         const unsigned* __restrict__ in_pstats, const float4* __restrict__ in_P0,
                                                         const float4* __restrict__ in_P1, const float* __restrict__ in_sstar) {
    const int wg = blockIdx.x, n_wg = gridDim.x, tid = threadIdx.x;
    RState* const S = a.S;
    if (wg == 0) rs_begin_body(S, 1);
    unsigned long long t_prev = wall_clock64();
    auto stamp = [&](int phase) {   // (workgroup 0's view of where the loop's time goes: LGR_RANSAC_DEBUG prints it)
        if (wg == 0 && tid == 0) { const unsigned long long t = wall_clock64(); S->phase_ticks[phase] += t - t_prev; t_prev = t; }
    };
    unsigned long long busy[5] = {0, 0, 0, 0, 0}, t_in = t_prev;
    auto work_begin = [&]() { if (tid == 0) t_in = wall_clock64(); };
    auto work_end = [&](int phase) { if (tid == 0) busy[phase] += wall_clock64() - t_in; };
    for (int round = 0; round < a.max_rounds; ++round) {
        if (!rs_grid_barrier(S, n_wg)) return;
        stamp(0);
        if (S->stop) {
            if (tid == 0)
                for (int k = 1; k < 5; ++k) { atomicMax(&S->busy_max[k], busy[k]); atomicAdd(&S->busy_sum[k], busy[k]); }
            return;
        }
        work_begin();   // (written by workgroup 0 in front of the barrier: every workgroup reads the same value)
        // ---- sample -> prerejection -> transform
        {
            const int nb = S->round_nb;
            int tid_h = tid;
            asm volatile("" : "+v"(tid_h));   // (opaque per round and phase: per-thread values are recomputed in the phase that uses them instead of being carried -- spilled -- through the others)
            for (int b0 = wg * MB + (tid_h & ~63); b0 < nb; b0 += n_wg * MB) {
                const int b = b0 + (tid_h & 63);
                LGR_NS_DISPATCH(a.n_samples, (rs_hyp_item<NS>(b, in_P0, in_P1, a.c, a.seed, S, a.edge_thr, a.Ts, a.list, a.posmap, a.counts)));
            }
        }
        work_end(1);
        if (!rs_grid_barrier(S, n_wg)) return;
        stamp(1);
        work_begin();
        // ---- inlier counts of the survivors
        {
            const int nh = S->n_ok;
            if (nh > 0) {
                const int hb_n = (nh + CB - 1) / CB, cch = count_chunk(nh, a.c);
                const long long items = (long long) hb_n * ((a.c + cch - 1) / cch);
                unsigned* const mt = nh <= a.mask_cap ? a.maskT : nullptr;
                int tid_c = tid;
                asm volatile("" : "+v"(tid_c));
                const int wave = __builtin_amdgcn_readfirstlane(tid_c >> 6);   // (uniform for the compiler too: the item's correspondences come through scalar loads)
                for (long long it = (long long) wg * (MB / 64) + wave; it < items; it += (long long) n_wg * (MB / 64))
                    count_item((int) (it % hb_n), (int) (it / hb_n), a.Ts, a.list, nh, in_PP, in_pstats, a.c, a.counts, mt, cch, tid_c & 63);
            }
        }
        work_end(2);
        if (!rs_grid_barrier(S, n_wg)) return;
        stamp(2);
        work_begin();
        int tid_m = tid;
        asm volatile("" : "+v"(tid_m));
        rs_cand_body(tid_m, wg, n_wg, S, a.counts, a.list, a.list2, a.hpos);
        work_end(3);
        if (!rs_grid_barrier(S, n_wg)) return;
        stamp(3);
        work_begin();
        asm volatile("" : "+v"(tid_m));
        metric_body(tid_m, wg, n_wg, a.Ts, a.list2, 0, in_P0, in_P1, in_sstar, a.c, a.metric_id, a.score_id, a.metric, a.ninl, nullptr, nullptr, a.scratch, a.maskT, a.hpos,
                    a.mask_cap, nullptr, &S->n_cand, &S->n_ok);
        work_end(4);
        if (!rs_grid_barrier(S, n_wg)) return;
        stamp(4);
        if (wg == 0) {
            asm volatile("" : "+v"(tid_m));
            rs_replay_body(tid_m, S, a.list, a.list2, a.metric, a.ninl, a.counts, a.posmap, a.Ts);
            __syncthreads();
            rs_begin_body(S, 0);   // the next round's range (or `stop`)
        }
    }
}
// closest-plane / combination metrics inside the device-driven schedule (round 5), extents read from the RState (fixed grids striding over
// them): the plane test's inlier counts replace the correspondence counts (the estimator's `inliers` are the plane pairs,
// src/metric.cpp:187-199); candidates pick up their plane metric; combination multiplies
__global__ void rs_plane_counts_kernel(const RState* __restrict__ S, const int* __restrict__ cnt, int2* __restrict__ counts) {
    const int n = S->n_ok;
    for (int h = blockIdx.x * blockDim.x + threadIdx.x; h < n; h += gridDim.x * blockDim.x) counts[h].x = cnt[h];
}
__global__ void rs_plane_pick_kernel(const RState* __restrict__ S, const int* __restrict__ hpos, const int* __restrict__ cnt, const float* __restrict__ cp,
                                     float* __restrict__ metric, int* __restrict__ ninl) {
    const int n = S->n_cand;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) { metric[j] = cp[hpos[j]]; ninl[j] = cnt[hpos[j]]; }
}
__global__ void rs_plane_mul_kernel(const RState* __restrict__ S, float* __restrict__ metric, const float* __restrict__ cp) {
    const int n = S->n_cand;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) metric[j] = metric[j] * cp[j];   // metric_cs * metric_cp (src/metric.cpp:248)
}
// the evaluation record of a single transform (metric, inliers, rmse as metric_kernel left them) into the RState
__global__ void rs_store_eval_kernel(const float* __restrict__ ev /* metric, n_inl bits, rmse */, float* __restrict__ dst3) {
    if (threadIdx.x < 3) dst3[threadIdx.x] = ev[threadIdx.x];
}
__global__ void rs_guess_kernel(RState* __restrict__ S, const float* __restrict__ ev) { S->final_metric = ev[0]; }

// ---------------------------------------------------------------------------------------------------- the set of distinct hypotheses
// SampleConsensusPrerejectiveOMP::align with SAVE_MULTIPLE_HYPOTHESES (src/sac_prerejective_omp.cpp:11): every accepted hypothesis goes
// through updateHypotheses (:143, :230, :261), the final block runs on every member of the set (:270-291) and chooseBestHypothesis picks
// the result (:293).  The loop above never scores a hypothesis that cannot beat the best one so far, so the set is built by a SECOND PASS
// over [0, iterations) once the loop has ended and its best metric M* is known: an item below 0.1 * M* can only block or erase other such
// items, and the prune after the last new best removes every one of them, so the fold of the items with !(metric < 0.1 * M*) is the fold of
// all items.  Hypothesis generation is a pure function of (seed, iteration): the pass regenerates the round's hypotheses with the loop's
// own kernels under the fixed gate that 0.1 * M* implies, keeps the candidates at or above 0.1 * M*, orders them by iteration (the
// candidate list arrives in the order of an atomic append) and hands them to the fold (lgr_hypotheses.hip).
__global__ void mh_begin_kernel(RState* __restrict__ S, int round_first, int nb, float gate_metric, int metric_id, int c) {
    if (threadIdx.x != 0) return;
    S->n_ok = 0; S->n_cand = 0; S->stop = 0;
    S->round_first = round_first; S->round_nb = nb; S->round_batches = 1;
    S->min_inliers = max(MIN_NR_INLIERS, rs_gate_dev(gate_metric, metric_id, c));
}
// candidate j (iteration offset list2[j]) is an item of the fold unless its metric is below 0.1 * M*
__global__ void mh_keep_kernel(const RState* __restrict__ S, const int* __restrict__ list2, const float* __restrict__ metric, float m_star, int* __restrict__ kslot) {
    const int n = S->n_cand;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
        if (!((double) metric[j] < 0.1 * (double) m_star)) kslot[list2[j]] = j;
}
// the round's items in iteration order: one workgroup, an ordered block scan per 1024 iteration offsets
__global__ __launch_bounds__(1024) void mh_order_kernel(const RState* __restrict__ S, const int* __restrict__ kslot, const float* __restrict__ Ts,
                                                         const float* __restrict__ metric, float* __restrict__ item_T, float* __restrict__ item_m,
                                                         int32_t* __restrict__ item_it, int* __restrict__ n_items) {
    __shared__ int scan[1024 / 64 + 2];
    const int tid = threadIdx.x, nb = S->round_nb, first = S->round_first;
    int total = 0;
    for (int o0 = 0; o0 < nb; o0 += 1024) {
        const int off = o0 + tid;
        const int j = off < nb ? kslot[off] : -1;
        int tot;
        const int pos = total + block_excl_scan_1024(j >= 0 ? 1 : 0, scan, tid, &tot);
        if (j >= 0) {
            const float4* s = reinterpret_cast<const float4*>(Ts + (size_t) off * 16);
            float4* d = reinterpret_cast<float4*>(item_T + (size_t) pos * 16);
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = s[3];
            item_m[pos] = metric[j];
            item_it[pos] = first + off;
        }
        total += tot;
    }
    if (tid == 0) n_items[0] = total;
}

// The final block of a member under closest_plane / weighted_closest_plane refits over the plane pairs (source point, nearest target point) in
// ASCENDING SOURCE INDEX; plane_kernel appends them with an atomic.  Source indices within a subset are distinct, so the place of a pair is
// the number of pairs with a smaller source index: every thread ranks one pair against all n keys, which the workgroup stages through LDS
// MH_RANK_TILE at a time (every lane reads the same word: a broadcast, no bank conflict), and writes the two points of its pair where
// plane_pack_kernel would have put them after a sort.  n = *n_pairs lives on the device; the grid covers its upper bound (the subset's
// size) and workgroups behind n return at once.  O(n^2 / 256) per workgroup, n <= 0.01 |src|: DESIGN.md section 3.1g has the measured cost.
constexpr int MH_RANK_TILE = 2048;
__global__ __launch_bounds__(256) void mh_plane_rank_pack_kernel(const float* __restrict__ src, const float* __restrict__ tgt, const int2* __restrict__ pairs,
                                                                  const int* __restrict__ n_pairs, float4* __restrict__ P0, float4* __restrict__ P1) {
    __shared__ __align__(16) int keys[MH_RANK_TILE];
    const int n = *n_pairs, tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    if (blockIdx.x * 256 >= n) return;   // (the whole workgroup)
    const int2 mine = i < n ? pairs[i] : make_int2(INT_MAX, 0);
    int rank = 0;
    for (int t0 = 0; t0 < n; t0 += MH_RANK_TILE) {
        const int m = min(MH_RANK_TILE, n - t0);
        __syncthreads();
        for (int t = tid; t < m; t += 256) keys[t] = pairs[t0 + t].x;
        __syncthreads();
        int k = 0;
        for (; k + 4 <= m; k += 4) {
            const int4 q = *reinterpret_cast<const int4*>(&keys[k]);
            rank += (q.x < mine.x) + (q.y < mine.x) + (q.z < mine.x) + (q.w < mine.x);
        }
        for (; k < m; ++k) rank += keys[k] < mine.x;
    }
    if (i >= n) return;
    const float* s = src + (size_t) mine.x * 12;
    const float* t = tgt + (size_t) mine.y * 12;
    P0[rank] = make_float4(s[0], s[1], s[2], 0.f);
    P1[rank] = make_float4(t[0], t[1], t[2], 0.f);
}
// the record of a single transform's evaluation under a plane metric, from the plane test's outputs pl = (count, metric, rmse):
// closest_plane / weighted_closest_plane: the plane test's own figures; combination: dst3 holds the correspondences evaluation
// (metric, inliers, rmse) and its metric takes the plane metric as a factor, in f32 (metric_cs * metric_cp, src/metric.cpp:248)
__global__ void mh_plane_store_kernel(const int* __restrict__ pl, float* __restrict__ dst3, int combination) {
    if (threadIdx.x != 0) return;
    const float cp = __int_as_float(pl[1]);
    if (combination) { dst3[0] = dst3[0] * cp; return; }
    dst3[0] = cp; dst3[1] = __int_as_float(pl[0]); dst3[2] = __int_as_float(pl[2]);
}
}  // namespace
