// lgr_rank_select.cuh -- exact order statistics on the device: the elements at up to two ranks of the order (key, i) over the valid
// elements of a float array, for lgr_rank_select* and the trimmed ICP loop (lgr_icp.hip).
//
// An element is valid iff its mask byte is non-zero (all where the mask is null) and its key's bits are <= 0x7f7fffff: finite, no sign bit,
// so that the bits order as the floats do.  Its composite is (key bits << 32) | i: unique, so "position < r" is "composite < the composite
// at rank r".  MSB-first radix select over the composite, 8 bits a pass: the four digits of the key, then those digits of the index that
// n - 1 reaches (three for a million elements: seven passes).  Pass p, one launch of sel_hist_kernel:
//   * every workgroup first derives the state of pass p (for both ranks: the prefix chosen so far, the rank left inside it) from the state
//     and the histogram of pass p - 1 -- a 256-entry scan, the same in every workgroup; workgroup 0 stores it for pass p + 1;
//   * then counts the digit of its 4096 elements whose higher bits equal the prefix, per rank, in LDS, and adds its non-empty bins to the
//     pass's global histogram with integer atomics: counts do not depend on the order of the additions.
// sel_finish_kernel derives the last state -- the two composites -- and clears the histograms for the next select.  The ranks may be given
// or, for trimmed ICP, follow from the count P found by pass 0 (K - 1 and the median rank, lgr_icp_math.h): nothing passes through the host.
// A rank outside [0, P) finds nothing (ok = 0) and reads nothing out of bounds: the scan has no matching bin.
#pragma once
#include "lgr_icp_math.h"
#include "lgr_internal.h"

namespace {

constexpr int SEL_BLOCK = 256, SEL_BINS = 256, SEL_PER_GROUP = 4096, SEL_MAX_PASSES = 8;

struct SelState {
    unsigned long long prefix[2];   // the composite's digits chosen so far; after the last pass: the composite at the rank
    long long rank[2];              // the rank left among the elements that carry the prefix
    long long P;                    // the number of valid elements (from pass 0 on)
    int ok[2];                      // the rank lies in [0, P)
    int pad[2];
};
static_assert(sizeof(SelState) == 56, "SelState is copied in one piece");

struct SelRanks {
    int from_keep;    // 1: r[0] = floor(keep P) - 1, r[1] = the median rank, from the device's own P
    float keep;
    long long r[2];   // the ranks otherwise
};

struct SelWork {
    SelState st[SEL_MAX_PASSES + 1];   // st[p]: entering pass p; st[SEL_MAX_PASSES]: the result
    unsigned hist[SEL_MAX_PASSES][2][SEL_BINS];
};

struct SelPlan { int n_pass; int shift[SEL_MAX_PASSES]; };

inline SelPlan sel_plan(int n) {
    SelPlan p{};
    for (int s = 56; s >= 32; s -= 8) p.shift[p.n_pass++] = s;
    for (int s = 24; s >= 0; s -= 8)
        if (((unsigned) (n - 1) >> s) != 0) p.shift[p.n_pass++] = s;   // a digit no index reaches is 0 everywhere: nothing to decide
    return p;
}

// state of pass p + 1 from W->st[p] and W->hist[p] (digit at `shift`), into st; all SEL_BLOCK threads, ends synchronised
__device__ __forceinline__ void sel_advance(const SelWork* __restrict__ W, int p, int shift, const SelRanks& A, SelState& st, unsigned long long (*sc)[SEL_BINS]) {
    const int t = threadIdx.x;
    const unsigned long long h[2] = {W->hist[p][0][t], W->hist[p][1][t]};
    sc[0][t] = h[0]; sc[1][t] = h[1];
    if (t == 0) st = W->st[p];
    __syncthreads();
    for (int o = 1; o < SEL_BINS; o <<= 1) {   // inclusive scan of both rows
        const unsigned long long a0 = t >= o ? sc[0][t - o] : 0ull, a1 = t >= o ? sc[1][t - o] : 0ull;
        __syncthreads();
        sc[0][t] += a0; sc[1][t] += a1;
        __syncthreads();
    }
    if (p == 0 && t == 0) {   // pass 0 counted every valid element for both ranks
        const long long P = (long long) sc[0][SEL_BINS - 1];
        st.P = P;
        st.rank[0] = A.from_keep ? icp_trim_k(A.keep, P) - 1 : A.r[0];
        st.rank[1] = A.from_keep ? icp_trim_median_rank(P) : A.r[1];
        st.ok[0] = st.rank[0] >= 0 && st.rank[0] < P;
        st.ok[1] = st.rank[1] >= 0 && st.rank[1] < P;
    }
    __syncthreads();
    const long long r[2] = {st.rank[0], st.rank[1]};
    const int ok[2] = {st.ok[0], st.ok[1]};
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const unsigned long long incl = sc[q][t], excl = incl - h[q];
        if (ok[q] && (unsigned long long) r[q] >= excl && (unsigned long long) r[q] < incl) {   // exactly one bin
            st.prefix[q] |= (unsigned long long) t << shift;
            st.rank[q] = r[q] - (long long) excl;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ bool sel_valid(uint32_t bits, const uint8_t* __restrict__ valid, long long i) { return bits <= 0x7f7fffffu && (!valid || valid[i] != 0); }

// pass `pass` of the select, its digit at `shift`; prev_shift: the digit of pass - 1.  `done`: null, or the flag of a loop that has ended.
__global__ __launch_bounds__(SEL_BLOCK) void sel_hist_kernel(const int* __restrict__ done, const uint32_t* __restrict__ keys, const uint8_t* __restrict__ valid, int n,
                                                              SelRanks A, int pass, int shift, int prev_shift, SelWork* __restrict__ W) {
    if (done && *done) return;
    __shared__ SelState st;
    __shared__ unsigned long long sc[2][SEL_BINS];
    __shared__ unsigned h[2][SEL_BINS];
    const int t = threadIdx.x;
    h[0][t] = 0; h[1][t] = 0;
    if (pass == 0) {
        if (t == 0) {
            st.prefix[0] = st.prefix[1] = 0; st.rank[0] = st.rank[1] = 0; st.P = 0;
            st.ok[0] = st.ok[1] = 1; st.pad[0] = st.pad[1] = 0;
        }
        __syncthreads();
    } else sel_advance(W, pass - 1, prev_shift, A, st, sc);
    if (blockIdx.x == 0 && t == 0) W->st[pass] = st;
    const unsigned long long pre[2] = {st.prefix[0], st.prefix[1]};
    const bool on[2] = {st.ok[0] != 0, st.ok[1] != 0};
    const int hs = shift + 8;   // the bits above this digit
    const long long base = (long long) blockIdx.x * SEL_PER_GROUP;
    for (int k = 0; k < SEL_PER_GROUP / SEL_BLOCK; ++k) {
        const long long i = base + (long long) k * SEL_BLOCK + t;
        if (i >= n) break;
        const uint32_t bits = keys[i];
        if (!sel_valid(bits, valid, i)) continue;
        const unsigned long long c = icp_trim_composite(bits, (uint32_t) i);
        const unsigned dgt = (unsigned) (c >> shift) & (SEL_BINS - 1);
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (on[q] && (hs >= 64 || (c >> hs) == (pre[q] >> hs))) atomicAdd(&h[q][dgt], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q)
        if (h[q][t]) atomicAdd(&W->hist[pass][q][t], h[q][t]);
}

// the last state -> W->st[SEL_MAX_PASSES]; every histogram back to 0.  One workgroup.
__global__ __launch_bounds__(SEL_BLOCK) void sel_finish_kernel(const int* __restrict__ done, SelRanks A, int last_pass, int last_shift, SelWork* __restrict__ W) {
    if (done && *done) return;
    __shared__ SelState st;
    __shared__ unsigned long long sc[2][SEL_BINS];
    sel_advance(W, last_pass, last_shift, A, st, sc);
    if (threadIdx.x == 0) W->st[SEL_MAX_PASSES] = st;
    unsigned* hist = &W->hist[0][0][0];
    for (int k = threadIdx.x; k < SEL_MAX_PASSES * 2 * SEL_BINS; k += SEL_BLOCK) hist[k] = 0u;
}

// below[i] = element i is valid and its position is < r0 (r0 == P: every valid element)
__global__ __launch_bounds__(SEL_BLOCK) void sel_below_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ valid, int n, const SelWork* __restrict__ W,
                                                               long long r0, uint8_t* __restrict__ below) {
    const long long i = (long long) blockIdx.x * SEL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const SelState* res = &W->st[SEL_MAX_PASSES];
    const uint32_t bits = keys[i];
    bool b = sel_valid(bits, valid, i);
    if (b && r0 != res->P) b = res->ok[0] && icp_trim_composite(bits, (uint32_t) i) < res->prefix[0];
    below[i] = b ? 1 : 0;
}

// the select over keys[0, n), n >= 1, on `stream`; the result is W->st[SEL_MAX_PASSES].  W->hist must be all 0 (as a finished select leaves it).
inline void sel_enqueue(hipStream_t stream, const int* done, const uint32_t* keys, const uint8_t* valid, int n, const SelRanks& A, SelWork* W) {
    const SelPlan plan = sel_plan(n);
    const unsigned groups = (unsigned) cdivz((size_t) n, SEL_PER_GROUP);
    for (int p = 0; p < plan.n_pass; ++p)
        sel_hist_kernel<<<groups, SEL_BLOCK, 0, stream>>>(done, keys, valid, n, A, p, plan.shift[p], p ? plan.shift[p - 1] : 0, W);
    sel_finish_kernel<<<1, SEL_BLOCK, 0, stream>>>(done, A, plan.n_pass - 1, plan.shift[plan.n_pass - 1], W);
}

}  // namespace
