// lgr_teaser.hip -- the TEASER alignment for gfx950: node selection, compatibility graph, maximum core and greedy clique, GNC-TLS rotation,
// per-axis TLS shift, inlier mask.  The reference names the estimator and fixes its parameters (src/alignment.cpp:37-69, alignTeaser and
// its commented-out body) without carrying it out; the statement computed here is this project's own ("TEASER")
// and is restated for the CPU in tests/cpp/teaser_ref.cpp from the same arithmetic (lgr_teaser_math.h).
//
// One call is a fixed chain of launches on the context's stream with one host read-back at its end:
//   nodes        GROR's pack / degree / ranking-key kernels and the radix sort (lgr_gror_nodes.cuh), then the gather of the K best
//   adjacency    a wave per (node, 64 columns): a lane tests one pair, the ballot is the bit word
//   clique       one workgroup: core peeling and the greedy removal, the alive mask in LDS, degrees by popcount(word & alive)
//   rotation     one workgroup: the terms of the sequential sums by all lanes, summed by lanes 0..8 (H) and lane 0 (cost) reading LDS
//                ahead; the SVD on lane 0
//   translation  one workgroup per axis: bitonic sort of the interval ends in LDS, a lane per centre, argmin by a packed key
//   mask         all correspondences under [R | t]
// No kernel waits for another workgroup: every dependency is a kernel boundary.
#include <chrono>
#include <cmath>

#include "lgr_host.h"
#include "lgr_internal.h"
#include "lgr_math.cuh"
#include "lgr_gror_nodes.cuh"
#include "lgr_teaser_math.h"

static_assert((int) TEASER_NODES_MAX == (int) LGR_TEASER_NODES_MAX, "lgr_teaser_math.h and lgr.h disagree");

namespace {

constexpr int TN = TEASER_NODES_MAX;   // nodes at most
constexpr int TW = TN / 64;            // 64-bit words per bit row at most
constexpr int TT = 1024;               // threads of the one-workgroup kernels
constexpr int NPT = TN / TT;           // nodes (TIMs, members) per thread
static_assert(NPT * TT == TN && TT % 64 == 0, "a wave owns whole bit words");

// what the kernels leave for the host (read back once) and for each other
struct TeaserState {
    float T[16];
    int bad, n_nodes, max_core, n_core, n_clique, valid, rot_iters, n_rot_in, n_tr_in, n_inliers;
    float rot_cost, tcost[3];
    float R[9], t[3];
};

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (unsigned) __shfl_xor((int) v, o));
    return v;
}

// ------------------------------------------------------------------------------------------------ adjacency
// The K x K bit matrix, rows of W = ceil(K / 64) 64-bit words.  It is symmetric (the predicate is: x - y and y - x have the same square),
// so word w of row u is stored at adj[w * K + u]: the one-workgroup kernel behind reads word w of 64 consecutive rows as one coalesced
// 512-byte access.  512 KB at K = 2048, L2-resident.
__global__ __launch_bounds__(256) void teaser_adj_kernel(const float4* __restrict__ sel, int K, int W, float two_beta, unsigned long long* __restrict__ adj) {
    const int wave = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave >= K * W) return;   // wave-uniform
    const int u = wave / W, w = wave - u * W, v = 64 * w + lane;
    const float4 su = sel[2 * u], tu = sel[2 * u + 1];
    bool e = false;
    if (v < K && v != u) {
        const float4 sv = sel[2 * v], tv = sel[2 * v + 1];
        e = teaser_edge(su.x, su.y, su.z, tu.x, tu.y, tu.z, sv.x, sv.y, sv.z, tv.x, tv.y, tv.z, two_beta);
    }
    const unsigned long long word = __ballot(e);
    if (lane == 0) adj[(size_t) w * K + u] = word;
}

// ------------------------------------------------------------------------------------------------ clique
__device__ __forceinline__ int row_degree(const unsigned long long* __restrict__ adj, int K, int W, int u, const unsigned long long* alive) {
    int d = 0;
    for (int w = 0; w < W; ++w) d += __popcll(adj[(size_t) w * K + u] & alive[w]);
    return d;
}

// Maximum core, then the greedy clique inside it.  Node u = i * TT + tid, so a wave's 64 nodes are one word of the alive mask and the
// wave's ballot IS that word.  Core peeling by rounds: with m the smallest alive degree, k = max(k, m); every alive node of degree <= k
// has core number k and leaves.  (The alive set always contains the (k + 1)-core, which such a node cannot belong to; and it is contained
// in the k-core, since it had minimum degree k when k was set.)  Every round removes a node: at most K rounds, plus the one that finds
// the mask empty.  The greedy step removes one node per round, at most K.
__global__ __launch_bounds__(TT) void teaser_clique_kernel(const unsigned long long* __restrict__ adj, int K, const float4* __restrict__ sel,
                                                           TeaserState* __restrict__ st, int* __restrict__ q_pos, int32_t* __restrict__ d_clique) {
    __shared__ unsigned long long alive[TW];
    __shared__ int s_min[2];
    __shared__ unsigned s_key[3];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid & 63, W = (K + 63) >> 6;
    if (tid < TW) {
        const int left = K - 64 * tid;
        alive[tid] = left >= 64 ? ~0ull : (left > 0 ? ((1ull << left) - 1ull) : 0ull);
    }
    if (tid == 0) { s_min[0] = s_min[1] = 0x7fffffff; s_key[0] = s_key[1] = s_key[2] = ~0u; s_cnt = 0; }
    __syncthreads();
    bool al[NPT];
    int deg[NPT], cr[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) { al[i] = i * TT + tid < K; deg[i] = 0; cr[i] = 0; }
    int k = 0;
    for (int r = 0; r <= K; ++r) {
        int mn = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < NPT; ++i)
            if (al[i]) { deg[i] = row_degree(adj, K, W, i * TT + tid, alive); mn = min(mn, deg[i]); }
        mn = wave_min_i(mn);
        if (lane == 0 && mn != 0x7fffffff) atomicMin(&s_min[r & 1], mn);
        if (tid == 0) s_min[(r + 1) & 1] = 0x7fffffff;   // last read before the second barrier of the round before
        __syncthreads();
        const int m = s_min[r & 1];
        if (m == 0x7fffffff) break;   // nobody is alive (the same in every thread)
        k = max(k, m);
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const bool stay = al[i] && deg[i] > k;
            if (al[i] && !stay) cr[i] = k;
            al[i] = stay;
            const unsigned long long word = __ballot(stay);
            if (lane == 0) alive[(i * TT + tid) >> 6] = word;
        }
        __syncthreads();
    }
    // V* = the nodes of core number K* = k
    int mine = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        al[i] = i * TT + tid < K && cr[i] == k;
        const unsigned long long word = __ballot(al[i]);
        if (lane == 0) { alive[(i * TT + tid) >> 6] = word; mine += __popcll(word); }
    }
    if (lane == 0 && mine) atomicAdd(&s_cnt, mine);
    __syncthreads();
    const int n_core = s_cnt;
    int n_alive = n_core;
#pragma unroll
    for (int i = 0; i < NPT; ++i) deg[i] = al[i] ? row_degree(adj, K, W, i * TT + tid, alive) : 0;
    // greedy: while the smallest alive degree is below |alive| - 1, the alive node of smallest degree leaves, among equals the one of
    // largest position.  key = degree << 11 | (TN - 1 - position), smallest first; three slots in turn, so that the reset of a slot (two
    // rounds after its use) cannot meet a late reader
    for (int r = 0; r < K; ++r) {
        unsigned key = ~0u;
#pragma unroll
        for (int i = 0; i < NPT; ++i)
            if (al[i]) key = min(key, ((unsigned) deg[i] << 11) | (unsigned) (TN - 1 - (i * TT + tid)));
        key = wave_min_u(key);
        if (lane == 0 && key != ~0u) atomicMin(&s_key[r % 3], key);
        if (tid == 0) s_key[(r + 1) % 3] = ~0u;
        __syncthreads();
        const unsigned best = s_key[r % 3];
        if (best == ~0u) break;
        const int dmin = (int) (best >> 11), x = TN - 1 - (int) (best & (TN - 1));
        if (dmin >= n_alive - 1) break;   // a clique
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            const int u = i * TT + tid;
            if (al[i]) {
                if (u == x) al[i] = false;
                else deg[i] -= (int) ((adj[(size_t) (x >> 6) * K + u] >> (x & 63)) & 1ull);
            }
        }
        --n_alive;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const unsigned long long word = __ballot(al[i]);
        if (lane == 0) alive[(i * TT + tid) >> 6] = word;
    }
    __syncthreads();
    // Q in ascending position; the caller's lists: [0, TN) the clique's correspondences, [TN, 2 TN) the nodes', unused entries -1
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int u = i * TT + tid, w = u >> 6;
        const int corr_index = u < K ? __float_as_int(sel[2 * u].w) : -1;
        if (d_clique) d_clique[TN + u] = corr_index;
        if (al[i]) {
            int pos = __popcll(alive[w] & ((1ull << lane) - 1ull));
            for (int v = 0; v < w; ++v) pos += __popcll(alive[v]);
            q_pos[pos] = u;
            if (d_clique) d_clique[pos] = corr_index;
        }
        if (d_clique && u >= n_alive) d_clique[u] = -1;
    }
    if (tid == 0) { st->n_nodes = K; st->max_core = k; st->n_core = n_core; st->n_clique = n_alive; st->valid = n_alive >= 3 ? 1 : 0; }
}

// ------------------------------------------------------------------------------------------------ rotation
// GNC-TLS over the TIMs of the open chain of Q.  TIM k = i * TT + tid lives in its thread's registers; per iteration the block stages the
// nine products (w a_r) b_s of every TIM in LDS, component-major, lanes 0..8 sum one column each in ascending k (consecutive LDS reads
// running ahead of the one dependent addition per term, as refit_kernel does), lane 0 solves for R, the block forms the residuals, and
// lane 0 sums the cost the same way.
__global__ __launch_bounds__(TT) void teaser_rotation_kernel(const float4* __restrict__ sel, const int* __restrict__ q_pos, TeaserState* __restrict__ st,
                                                             float two_beta, int max_it, float gnc, float cost_thr) {
    __shared__ float sp[9 * TT];
    __shared__ float Hs[9], Rs[9], s_cost, s_red[TT / 64];
    const int n_clique = st->n_clique;
    if (n_clique < 3) return;
    const int n = n_clique - 1, tid = threadIdx.x, lane = tid & 63;
    float a[NPT][3], b[NPT][3], w[NPT], res[NPT];
#pragma unroll
    for (int i = 0; i < NPT; ++i) {
        const int k = i * TT + tid;
        w[i] = 1.f; res[i] = 0.f;
#pragma unroll
        for (int d = 0; d < 3; ++d) { a[i][d] = 0.f; b[i][d] = 0.f; }
        if (k < n) {
            const int q0 = q_pos[k], q1 = q_pos[k + 1];
            const float4 s0 = sel[2 * q0], t0 = sel[2 * q0 + 1], s1 = sel[2 * q1], t1 = sel[2 * q1 + 1];
            a[i][0] = s1.x - s0.x; a[i][1] = s1.y - s0.y; a[i][2] = s1.z - s0.z;
            b[i][0] = t1.x - t0.x; b[i][1] = t1.y - t0.y; b[i][2] = t1.z - t0.z;
        }
    }
    const float e2 = teaser_e2(two_beta);
    float mu = 0.f, prev = __uint_as_float(0x7f800000u), cost = 0.f;
    int solves = 0;
    for (int it = 0; it < max_it; ++it) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            if (i * TT >= n) break;   // the same in every thread
            __syncthreads();
            if (i * TT + tid < n) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int s = 0; s < 3; ++s) sp[(3 * r + s) * TT + tid] = (w[i] * a[i][r]) * b[i][s];
            }
            __syncthreads();
            if (tid < 9) {
                const int m = min(TT, n - i * TT);
                const float* col = sp + tid * TT;
#pragma unroll 16
                for (int j = 0; j < m; ++j) acc += col[j];
            }
        }
        if (tid < 9) Hs[tid] = acc;
        __syncthreads();
        if (tid == 0) {
            float H[9], R[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) H[j] = Hs[j];
            teaser_rotation(H, R, [](const float* A, float* U, float* S, float* V) { lgr_svd3(A, U, S, V); });
#pragma unroll
            for (int j = 0; j < 9; ++j) Rs[j] = R[j];
        }
        __syncthreads();
        ++solves;
        float R[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) R[j] = Rs[j];
        float mx = 0.f;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            res[i] = teaser_residual(R, a[i][0], a[i][1], a[i][2], b[i][0], b[i][1], b[i][2]);
            if (i * TT + tid < n) mx = teaser_max(mx, res[i]);
        }
        if (it == 0) {   // the maximum is order-free: no NaN ever enters it
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = teaser_max(mx, __shfl_xor(mx, o));
            if (lane == 0) s_red[tid >> 6] = mx;
            __syncthreads();
            mx = 0.f;
#pragma unroll
            for (int j = 0; j < TT / 64; ++j) mx = teaser_max(mx, s_red[j]);
            mu = teaser_mu0(mx, e2);
            if (!(mu > 0.f)) break;   // the same in every thread; all weights stay 1
        }
        float cacc = 0.f;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            if (i * TT >= n) break;
            __syncthreads();
            if (i * TT + tid < n) sp[tid] = w[i] * res[i];
            __syncthreads();
            if (tid == 0) {
                const int m = min(TT, n - i * TT);
#pragma unroll 16
                for (int j = 0; j < m; ++j) cacc += sp[j];
            }
        }
        if (tid == 0) s_cost = cacc;
        int any = 0;
#pragma unroll
        for (int i = 0; i < NPT; ++i) {
            w[i] = teaser_weight(res[i], mu, e2);
            if (i * TT + tid < n && w[i] > 0.f) any = 1;
        }
        any = __syncthreads_or(any);
        cost = s_cost;
        const float diff = fabsf(cost - prev);
        mu = mu * gnc;
        prev = cost;
        if (diff < cost_thr || !any) break;
    }
    int in = 0;
#pragma unroll
    for (int i = 0; i < NPT; ++i) in += (i * TT + tid < n && w[i] >= 0.5f) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) in += __shfl_xor(in, o);
    if (lane == 0 && in) atomicAdd(&st->n_rot_in, in);
    if (tid < 9) st->R[tid] = Rs[tid];
    if (tid == 0) { st->rot_iters = solves; st->rot_cost = cost; }
}

// ------------------------------------------------------------------------------------------------ translation
// One axis per workgroup: x_k = T[q_k] - (R S[q_k]) on this axis, the 2 n interval ends sorted by their keys (bitonic, padded with the
// largest key to a power of two), a lane per centre: consensus mean and truncated cost as two sequential passes over the members in LDS.
__global__ __launch_bounds__(TT) void teaser_shift_kernel(const float4* __restrict__ sel, const int* __restrict__ q_pos, TeaserState* __restrict__ st, float beta,
                                                          uint8_t* __restrict__ tflags) {
    __shared__ unsigned long long keys[2 * TN];
    __shared__ float xs[TN];
    __shared__ unsigned long long s_best;
    __shared__ float s_shift, s_centre;
    const int n = st->n_clique, axis = blockIdx.x, tid = threadIdx.x;
    if (n < 3) return;
    float R[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) R[j] = st->R[j];
    int P = 2;
    while (P < 2 * n) P <<= 1;   // <= 2 TN
    for (int k = tid; k < P / 2; k += TT) {
        unsigned long long lo = ~0ull, hi = ~0ull;
        if (k < n) {
            const int q = q_pos[k];
            const float4 s = sel[2 * q], t = sel[2 * q + 1];
            const float tv = axis == 0 ? t.x : (axis == 1 ? t.y : t.z);
            const float x = tv - teaser_rot_row(R, axis, s.x, s.y, s.z);
            xs[k] = x;
            lo = teaser_end_key(x - beta, 0, k);
            hi = teaser_end_key(x + beta, 1, k);
        }
        keys[2 * k] = lo; keys[2 * k + 1] = hi;
    }
    if (tid == 0) s_best = ~0ull;
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < P / 2; t += TT) {
                const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const unsigned long long x = keys[lo], y = keys[hi];
                if ((x > y) == up) { keys[lo] = y; keys[hi] = x; }
            }
        }
    __syncthreads();
    unsigned long long best = ~0ull;
    float my_shift = 0.f, my_centre = 0.f;
    for (int ci = tid; ci < 2 * n - 1; ci += TT) {
        const float centre = 0.5f * (teaser_key_value(keys[ci]) + teaser_key_value(keys[ci + 1]));
        float sum = 0.f;
        int cnt = 0;
        for (int k = 0; k < n; ++k) {
            const float x = xs[k];
            if (teaser_in_consensus(x, centre, beta)) { sum += x; ++cnt; }
        }
        if (cnt == 0) continue;
        const float xhat = sum / (float) cnt;
        float cost = 0.f;
        for (int k = 0; k < n; ++k) cost += teaser_tls_term(xs[k], xhat, beta);
        const unsigned long long cand = ((unsigned long long) __float_as_uint(cost) << 32) | (unsigned) ci;   // cost >= 0: its bits are monotone
        if (cand < best) { best = cand; my_shift = xhat; my_centre = centre; }
    }
    if (best != ~0ull) atomicMin(&s_best, best);
    __syncthreads();
    const unsigned long long win = s_best;
    if (win != ~0ull && best == win) { s_shift = my_shift; s_centre = my_centre; }   // one thread: a centre index has one owner
    __syncthreads();
    const bool found = win != ~0ull;
    for (int k = tid; k < n; k += TT) tflags[axis * TN + k] = (found && teaser_in_consensus(xs[k], s_centre, beta)) ? 1 : 0;
    if (tid == 0) {
        st->t[axis] = found ? s_shift : 0.f;
        st->tcost[axis] = found ? __uint_as_float((unsigned) (win >> 32)) : (float) n;
    }
}

// ------------------------------------------------------------------------------------------------ mask
__global__ __launch_bounds__(256) void teaser_mask_kernel(const float4* __restrict__ S, const float4* __restrict__ T, int c, TeaserState* __restrict__ st,
                                                          const uint8_t* __restrict__ tflags, float beta, uint8_t* __restrict__ mask) {
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
    const int valid = st->valid;
    bool in = false;
    if (valid && i < c) {
        const float4 s = S[i], t = T[i];
        const float* R = st->R;
        const float mx = teaser_rot_row(R, 0, s.x, s.y, s.z) + st->t[0], my = teaser_rot_row(R, 1, s.x, s.y, s.z) + st->t[1],
                    mz = teaser_rot_row(R, 2, s.x, s.y, s.z) + st->t[2];
        in = fabsf(t.x - mx) <= beta && fabsf(t.y - my) <= beta && fabsf(t.z - mz) <= beta;
    }
    if (mask && i < c) mask[i] = in ? 1 : 0;
    const unsigned long long word = __ballot(in);
    if (lane == 0 && word) atomicAdd(&st->n_inliers, __popcll(word));
    if (blockIdx.x == 0) {
        if (valid) {
            const int n = st->n_clique;
            int cnt = 0;
            for (int k = threadIdx.x; k < n; k += 256) cnt += (tflags[k] && tflags[TN + k] && tflags[2 * TN + k]) ? 1 : 0;
            if (cnt) atomicAdd(&st->n_tr_in, cnt);
        }
        if (threadIdx.x < 16) {   // [R | t] column-major; the identity without a solution
            const int col = threadIdx.x >> 2, row = threadIdx.x & 3;
            float v = row == col ? 1.f : 0.f;
            if (valid && row < 3) v = col < 3 ? st->R[3 * row + col] : st->t[row];
            st->T[threadIdx.x] = v;
        }
    }
}

int teaser_check_params(lgr_ctx* ctx, const lgr_teaser_params* p, int* k_select) {
    LGR_CHECK(ctx, p != nullptr, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, std::isfinite(p->noise_bound) && p->noise_bound > 0.f && p->noise_bound <= 1e18f, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, p->rotation_max_iterations >= 1 && p->rotation_max_iterations <= 1000, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, std::isfinite(p->rotation_gnc_factor) && p->rotation_gnc_factor > 1.f, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, std::isfinite(p->rotation_cost_threshold) && p->rotation_cost_threshold >= 0.f, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, p->k_select == 0 || (p->k_select >= 3 && p->k_select <= LGR_TEASER_NODES_MAX), LGR_ERR_UNSUPPORTED);
    *k_select = p->k_select == 0 ? 1024 : p->k_select;
    return LGR_OK;
}

void teaser_tick(lgr_ctx* ctx, int i) { (void) hipEventRecord(ctx->ev[i], ctx->stream); }

}  // namespace

extern "C" void lgr_default_teaser_params(lgr_teaser_params* p, float distance_thr) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->noise_bound = distance_thr;            // src/alignment.cpp:48
    p->k_select = 0;                          // 1024 nodes
    p->rotation_max_iterations = 100;         // :53
    p->rotation_gnc_factor = 1.4f;            // :54
    p->rotation_cost_threshold = 0.005f;      // :55
}

extern "C" int lgr_teaser_dev(lgr_ctx* ctx, const float* d_src, int ns, const float* d_tgt, int nt, const lgr_corr* d_corr, int c,
                              const lgr_teaser_params* params, lgr_result* res, lgr_teaser_info* info, int32_t* d_clique, uint8_t* d_inlier_mask) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, d_src && d_tgt && res && ns > 0 && nt > 0 && (d_corr || c == 0) && c >= 0, LGR_ERR_INVALID_ARG);
    int k_select = 0;
    LGR_TRY(teaser_check_params(ctx, params, &k_select));
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    memset(res, 0, sizeof *res);
    if (info) memset(info, 0, sizeof *info);
    auto t0 = std::chrono::steady_clock::now();
    const float beta = params->noise_bound, two_beta = 2.f * beta;
    const int K = std::min(c, k_select);
    res->n_correspondences = c;
    res->estimated_iters = K;
    if (info) info->n_nodes = K;
    if (d_clique) LGR_HIP(ctx, hipMemsetAsync(d_clique, 0xff, (size_t) 2 * LGR_TEASER_NODES_MAX * 4, ctx->stream));
    if (c < 3) {   // no three nodes: no solution, nothing is read from the correspondences
        for (int k = 0; k < 4; ++k) res->transformation[5 * k] = 1.f;
        if (d_inlier_mask && c) LGR_HIP(ctx, hipMemsetAsync(d_inlier_mask, 0, (size_t) c, ctx->stream));
        return LGR_OK;
    }
    // every buffer first: a workspace that grows synchronises, and nothing may do so between the launches
    TeaserState* st;   // state | q_pos: TN ints | tflags: 3 TN bytes
    static_assert(sizeof(TeaserState) % 4 == 0, "q_pos follows the state");
    LGR_TRY(lgr_ws(ctx, WS_TEASER_STATE, sizeof(TeaserState) + (size_t) TN * 4 + 3 * TN, (void**) &st));
    int* q_pos = (int*) (st + 1);
    uint8_t* tflags = (uint8_t*) (q_pos + TN);
    const int W = (K + 63) / 64;
    unsigned long long* adj;
    LGR_TRY(lgr_ws_t(ctx, WS_TEASER_ADJ, (size_t) W * K + 8, &adj));
    GrorBuffers b;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_LIST, (size_t) c, &b.degree));
    unsigned long long* keys;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_HIST, (size_t) 2 * c + 8, &keys));
    unsigned long long* keys2 = keys + c;
    float4* d_sel;
    LGR_TRY(lgr_ws_t(ctx, WS_RANSAC_MISC, (size_t) 2 * K + 16, &d_sel));
    TeaserState* h_st;
    LGR_TRY(lgr_pinned(ctx, sizeof(TeaserState), (void**) &h_st));

    LGR_HIP(ctx, hipMemsetAsync(st, 0, sizeof(TeaserState), ctx->stream));
    teaser_tick(ctx, 0);
    LGR_TRY(gror_pack(ctx, d_src, d_tgt, d_corr, c, &b, ns, nt, &st->bad));   // range check on the device: *bad is read back at the end
    LGR_TRY(gror_degrees(ctx, b, c, beta, b.degree));
    LGR_TRY(gror_rank(ctx, b.degree, c, keys, keys2));
    gror_gather_kernel<<<cdiv(K, 256), 256, 0, ctx->stream>>>(keys2, K, 1, b.S, b.T, d_sel);
    teaser_tick(ctx, 1);
    teaser_adj_kernel<<<cdiv((long long) K * W, 4), 256, 0, ctx->stream>>>(d_sel, K, W, two_beta, adj);
    teaser_tick(ctx, 2);
    teaser_clique_kernel<<<1, TT, 0, ctx->stream>>>(adj, K, d_sel, st, q_pos, d_clique);
    teaser_tick(ctx, 3);
    teaser_rotation_kernel<<<1, TT, 0, ctx->stream>>>(d_sel, q_pos, st, two_beta, params->rotation_max_iterations, params->rotation_gnc_factor,
                                                      params->rotation_cost_threshold);
    teaser_tick(ctx, 4);
    teaser_shift_kernel<<<3, TT, 0, ctx->stream>>>(d_sel, q_pos, st, beta, tflags);
    teaser_tick(ctx, 5);
    teaser_mask_kernel<<<cdiv(c, 256), 256, 0, ctx->stream>>>(b.S, b.T, c, st, tflags, beta, d_inlier_mask);
    teaser_tick(ctx, 6);
    LGR_HIP(ctx, hipGetLastError());
    LGR_HIP(ctx, hipMemcpyAsync(h_st, st, sizeof(TeaserState), hipMemcpyDeviceToHost, ctx->stream));   // the call's one read-back
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    LGR_CHECK(ctx, h_st->bad == 0 /* an index_query outside [0, ns) or an index_match outside [0, nt) */, LGR_ERR_INVALID_ARG);
    memcpy(res->transformation, h_st->T, 64);
    res->iterations = h_st->rot_iters;
    res->converged = h_st->valid;
    res->n_inliers = h_st->n_inliers;
    res->metric = (float) h_st->n_clique;
    res->best_metric_before_refit = (float) h_st->n_clique;
    res->best_iteration = h_st->max_core;
    for (int s = 0; s < 6; ++s) (void) hipEventElapsedTime(&res->stage_ms[s], ctx->ev[s], ctx->ev[s + 1]);   // nodes adjacency clique rotation translation mask
    if (info) {
        info->valid = h_st->valid; info->n_nodes = h_st->n_nodes; info->max_core = h_st->max_core; info->n_core = h_st->n_core;
        info->n_clique = h_st->n_clique; info->rotation_iterations = h_st->rot_iters; info->n_rotation_inliers = h_st->n_rot_in;
        info->n_translation_inliers = h_st->n_tr_in; info->rotation_cost = h_st->rot_cost;
        for (int a = 0; a < 3; ++a) info->translation_cost[a] = h_st->tcost[a];
    }
    res->time_te = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return LGR_OK;
}

extern "C" int lgr_teaser(lgr_ctx* ctx, const float* src, int ns, const float* tgt, int nt, const lgr_corr* corr, int c, const lgr_teaser_params* params,
                          lgr_result* res, lgr_teaser_info* info, int32_t* clique, uint8_t* inlier_mask) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, src && tgt && res && ns > 0 && nt > 0 && (corr || c == 0) && c >= 0, LGR_ERR_INVALID_ARG);
    float *ds, *dt;
    lgr_corr* dc;
    uint8_t* dm = nullptr;
    int32_t* dq = nullptr;
    lgr_host_call hc(ctx);
    LGR_TRY(hc.clouds(src, ns, tgt, nt, &ds, &dt));
    LGR_TRY(hc.in(corr, (size_t) c, &dc));
    if (inlier_mask) LGR_TRY(hc.out((size_t) c, &dm));
    if (clique) LGR_TRY(hc.out((size_t) 2 * LGR_TEASER_NODES_MAX, &dq));
    LGR_TRY(lgr_teaser_dev(ctx, ds, ns, dt, nt, dc, c, params, res, info, dq, dm));
    LGR_TRY(hc.fetch(inlier_mask, dm, (size_t) c));
    LGR_TRY(hc.fetch(clique, dq, (size_t) 2 * LGR_TEASER_NODES_MAX));
    return hc.finish();
}
