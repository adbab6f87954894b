// lgr_hash_order.hip -- the iteration order of libstdc++'s hash containers as kernels (gfx950): what the reference numbers its points
// by after filterDuplicatePoints (std::unordered_set, src/common.cpp:417-427) and downsamplePointCloud (std::unordered_map,
// src/downsample.cpp:20,32-34).  lgr_stdhash.h states the rule and the hashes; here one EPOCH (one bucket count B) is
//   act[h % B] = min over the bucket's elements of their time      integer atomicMin on a B-entry table: order-free, deterministic
//   key        = (~act, ~time) on the 2 * ceil(log2 m') bits that can differ, value = element
//   one radix sort (lgr_sort_pairs_u64)                            the keys are distinct, the sorted values are the new list
// walked by TIME t (position in the previous list, or the element id of a new element), so no inverse permutation is needed.
// The epochs that fit (elements and buckets <= HO_SMALL: the first nine of a container that was not reserved) run inside ONE
// single-workgroup kernel that keeps list, table and keys in LDS and sorts them with a bitonic network; the later ones cost a memset,
// two launches and the sort's passes each.  The host part needs only n (the schedule comes from the runtime's rehash policy
// object): nothing is read back and nothing allocated besides the workspace slots.
#include <unordered_map>

#include "lgr_internal.h"
#include "lgr_stdhash.h"

namespace {

constexpr int HO_SMALL = 5120;       // elements and buckets of an epoch the one-workgroup kernel holds in LDS
constexpr int HO_SORT = 8192;        // its sort network: the next power of two
constexpr int HO_THREADS = 1024;
constexpr int HO_PER = HO_SMALL / HO_THREADS;
constexpr int HO_MAX_EP = 16;
struct HoSmall { int n_ep; int end[HO_MAX_EP]; unsigned buckets[HO_MAX_EP]; };

__device__ __forceinline__ int ho_bits(int m) { return m > 1 ? 32 - __clz(m - 1) : 1; }   // bits of the times 0..m-1 (at least 1)

__global__ __launch_bounds__(HO_THREADS) void ho_small_kernel(const unsigned long long* __restrict__ hash, HoSmall s, int32_t* __restrict__ order) {
    __shared__ unsigned key[HO_SORT];
    __shared__ unsigned act[HO_SMALL];
    __shared__ unsigned short P[HO_SMALL];
    const int tid = threadIdx.x;
    int m = 0;
    for (int ep = 0; ep < s.n_ep; ++ep) {
        const int m2 = s.end[ep];
        const unsigned B = s.buckets[ep];
        const int bits = ho_bits(m2);
        int np2 = 2;
        while (np2 < m2) np2 <<= 1;
        for (unsigned b = tid; b < B; b += HO_THREADS) act[b] = 0xffffffffu;
        __syncthreads();
        for (int t = tid; t < m2; t += HO_THREADS) {
            const int e = t < m ? (int) P[t] : t;
            const unsigned b = (unsigned) (hash[e] % (unsigned long long) B);
            atomicMin(&act[b], (unsigned) t);
            key[t] = b;
        }
        __syncthreads();
        for (int t = tid; t < np2; t += HO_THREADS)
            key[t] = t < m2 ? (((unsigned) (m2 - 1) - act[key[t]]) << bits) | (unsigned) (m2 - 1 - t) : 0xffffffffu;
        __syncthreads();
        for (int k = 2; k <= np2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < np2; i += HO_THREADS) {
                    const int x = i ^ j;
                    if (x > i) {
                        const unsigned a = key[i], c = key[x];
                        if ((a > c) == ((i & k) == 0)) { key[i] = c; key[x] = a; }
                    }
                }
                __syncthreads();
            }
        // position -> time -> element; the old list is read by every thread before anyone overwrites it
        int el[HO_PER];
#pragma unroll
        for (int r = 0; r < HO_PER; ++r) {
            const int pos = r * HO_THREADS + tid;
            el[r] = 0;
            if (pos < m2) {
                const int t = m2 - 1 - (int) (key[pos] & ((1u << bits) - 1u));
                el[r] = t < m ? (int) P[t] : t;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < HO_PER; ++r) {
            const int pos = r * HO_THREADS + tid;
            if (pos < m2) P[pos] = (unsigned short) el[r];
        }
        __syncthreads();
        m = m2;
    }
    for (int pos = tid; pos < m; pos += HO_THREADS) order[pos] = (int32_t) P[pos];
}

// one thread per time t of the epoch [m, m2): its element, that element's bucket, the bucket's earliest time
__global__ void ho_act_kernel(const unsigned long long* __restrict__ hash, const int32_t* __restrict__ order, int m, int m2, unsigned long long B,
                              unsigned* __restrict__ act, unsigned* __restrict__ bucket) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m2) return;
    const int e = t < m ? order[t] : t;
    const unsigned b = (unsigned) (hash[e] % B);
    atomicMin(&act[b], (unsigned) t);
    bucket[t] = b;
}
__global__ void ho_keys_kernel(const int32_t* __restrict__ order, int m, int m2, int bits, const unsigned* __restrict__ act, const unsigned* __restrict__ bucket,
                               unsigned long long* __restrict__ keys, int* __restrict__ vals) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m2) return;
    keys[t] = ((unsigned long long) ((unsigned) (m2 - 1) - act[bucket[t]]) << bits) | (unsigned long long) (unsigned) (m2 - 1 - t);
    vals[t] = t < m ? order[t] : t;
}

__global__ void ho_voxel_hash_kernel(const unsigned long long* __restrict__ vkeys, const int* __restrict__ by_first, int nv, unsigned long long* __restrict__ hash) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nv) return;
    const unsigned long long k = vkeys[by_first[e]];   // (iz, iy, ix) in 21-bit fields: lgr_features.hip voxel_keys
    hash[e] = lgr_hash_voxel((int) (k & 0x1fffff), (int) ((k >> 21) & 0x1fffff), (int) ((k >> 42) & 0x1fffff));
}
__global__ void ho_iota_kernel(const int* __restrict__ first, int n, unsigned* __restrict__ keys, int* __restrict__ vals) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = (unsigned) first[i];
    vals[i] = i;
}
// out[pos] = in[via ? via[order[pos]] : order[pos]], a point = three float4
__global__ void ho_gather_kernel(const float4* __restrict__ in, const int32_t* __restrict__ order, const int* __restrict__ via, int n, float4* __restrict__ out) {
    const long long q = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (long long) n * 3) return;
    const int pos = (int) (q / 3), f = (int) (q % 3);
    int src = order[pos];
    if (via) src = via[src];
    out[q] = in[(size_t) src * 3 + f];
}

struct Key3 { int x, y, z; bool operator==(const Key3& o) const { return x == o.x && y == o.y && z == o.z; } };
struct HashKey3 {   // include/common.h:212-223 HashEigen<Eigen::Vector3i>, through the library's own std::hash<int>
    std::size_t operator()(const Key3& k) const {
        std::size_t seed = 0;
        const int e[3] = {k.x, k.y, k.z};
        for (int i = 0; i < 3; ++i) seed ^= std::hash<int>()(e[i]) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
        return seed;
    }
};

}  // namespace

int lgr_hash_order_launch(lgr_ctx* ctx, const unsigned long long* d_hash, int n, long long reserve, int32_t* d_order) {
    if (n == 0) return LGR_OK;
    const std::vector<lgr_hash_epoch> eps = lgr_hash_schedule(n, reserve);
    unsigned long long bmax = 0;
    for (const lgr_hash_epoch& ep : eps) bmax = std::max(bmax, ep.buckets);
    LGR_CHECK(ctx, bmax > 0 && bmax < (1ull << 31), LGR_ERR_INVALID_ARG);   // a bucket index is a u32, the table one workspace slot
    // the leading epochs that fit into the one-workgroup kernel
    HoSmall sm{};
    size_t k = 0;
    while (k < eps.size() && sm.n_ep < HO_MAX_EP && eps[k].end <= HO_SMALL && eps[k].buckets <= (unsigned long long) HO_SMALL) {
        sm.end[sm.n_ep] = (int) eps[k].end;
        sm.buckets[sm.n_ep] = (unsigned) eps[k].buckets;
        ++sm.n_ep; ++k;
    }
    if (sm.n_ep) ho_small_kernel<<<1, HO_THREADS, 0, ctx->stream>>>(d_hash, sm, d_order);
    if (k < eps.size()) {
        unsigned *act, *bucket;
        unsigned long long* keys;
        const size_t nn = ((size_t) n + 1) & ~(size_t) 1;
        LGR_TRY(lgr_ws_t(ctx, WS_HO_ACT, (size_t) bmax, &act));
        LGR_TRY(lgr_ws_t(ctx, WS_HO_WORK, nn * 3, &keys));   // keys, sorted keys, (bucket | vals)
        unsigned long long* keys2 = keys + nn;
        bucket = (unsigned*) (keys2 + nn);
        int* vals = (int*) (bucket + nn);
        for (; k < eps.size(); ++k) {
            const int m = (int) eps[k].begin, m2 = (int) eps[k].end;
            int bits = 1;
            while ((1ll << bits) < m2) ++bits;
            LGR_HIP(ctx, hipMemsetAsync(act, 0xff, (size_t) eps[k].buckets * 4, ctx->stream));
            ho_act_kernel<<<cdiv(m2, 256), 256, 0, ctx->stream>>>(d_hash, d_order, m, m2, eps[k].buckets, act, bucket);
            ho_keys_kernel<<<cdiv(m2, 256), 256, 0, ctx->stream>>>(d_order, m, m2, bits, act, bucket, keys, vals);
            const int shift = 0, width = 2 * bits;
            LGR_TRY(lgr_sort_pairs_u64(ctx, keys, keys2, vals, d_order, (size_t) m2, &shift, &width, 1));
        }
    }
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

extern "C" int lgr_hash_order_dev(lgr_ctx* ctx, const uint64_t* d_hash, int n, long long reserve, int32_t* d_order) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, n >= 0 && (reserve == 0 || reserve >= (long long) n) && ((d_hash && d_order) || n == 0), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    return lgr_hash_order_launch(ctx, (const unsigned long long*) d_hash, n, reserve, d_order);
}

int lgr_gather_points_launch(lgr_ctx* ctx, const float* d_in, const int32_t* d_order, const int* d_via, int n, float* d_out) {
    if (n == 0) return LGR_OK;
    ho_gather_kernel<<<cdiv((long long) n * 3, 256), 256, 0, ctx->stream>>>((const float4*) d_in, d_order, d_via, n, (float4*) d_out);
    LGR_HIP(ctx, hipGetLastError());
    return LGR_OK;
}

extern "C" int lgr_downsample_order_dev(lgr_ctx* ctx, const float* d_pts, int n, float voxel, int order, float* d_out, int* n_out) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, (d_pts || n == 0) && (d_out || n == 0) && n_out && n >= 0, LGR_ERR_INVALID_ARG);
    LGR_CHECK(ctx, order == LGR_ORDER_REFERENCE || order == LGR_ORDER_CANONICAL, LGR_ERR_INVALID_ARG);
    if (order == LGR_ORDER_CANONICAL) return lgr_downsample_dev(ctx, d_pts, n, voxel, d_out, n_out);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    *n_out = 0;
    if (n == 0) return LGR_OK;
    // the voxel points in (iz,iy,ix) order into a staging buffer, with every voxel's key and first input index left on the device
    float* stage;
    LGR_TRY(lgr_ws_t(ctx, WS_HO_STAGE, (size_t) n * 12 + 4, &stage));
    const unsigned long long* vkeys = nullptr;
    const int* vfirst = nullptr;
    int nv = 0;
    LGR_TRY(lgr_downsample_keys(ctx, d_pts, n, voxel, stage, &nv, &vkeys, &vfirst));
    if (nv == 0) return LGR_OK;
    // elements = the voxels by first input index (the map's insertion sequence)
    const size_t nn = ((size_t) nv + 1) & ~(size_t) 1;
    unsigned long long* hash;
    LGR_TRY(lgr_ws_t(ctx, WS_HO_HASH, nn * 4, &hash));   // hash | first, iota, by_first | order, sorted first
    unsigned* fkeys = (unsigned*) (hash + nn);
    int* iota = (int*) (fkeys + nn);
    int* by_first = iota + nn;
    int32_t* ord = by_first + nn;
    unsigned* fsorted = (unsigned*) (ord + nn);
    ho_iota_kernel<<<cdiv(nv, 256), 256, 0, ctx->stream>>>(vfirst, nv, fkeys, iota);
    int bits = 1;
    while ((1ll << bits) < n) ++bits;
    LGR_TRY(lgr_sort_pairs_u32(ctx, fkeys, fsorted, iota, by_first, (size_t) nv, 0, bits));
    ho_voxel_hash_kernel<<<cdiv(nv, 256), 256, 0, ctx->stream>>>(vkeys, by_first, nv, hash);
    LGR_TRY(lgr_hash_order_launch(ctx, hash, nv, 0, ord));
    LGR_TRY(lgr_gather_points_launch(ctx, stage, ord, by_first, nv, d_out));   // d_out may be d_pts: everything that read d_pts is queued before
    *n_out = nv;
    return LGR_OK;
}

// lgr.h: voxel keys from the host through the real container and through the kernels
extern "C" int lgr_selfcheck_hash_order(lgr_ctx* ctx, int n, int spread, uint64_t seed, long long reserve, long long* mismatches) {
    lgr_turn turn__(ctx);   // contexts of one device take turns (lgr_internal.h)
    if (!ctx) return LGR_ERR_INVALID_ARG;
    LGR_CHECK(ctx, mismatches && n >= 0 && spread >= 1 && spread <= (1 << 21) && (reserve == 0 || reserve >= (long long) n), LGR_ERR_INVALID_ARG);
    LGR_HIP(ctx, hipSetDevice(ctx->device));
    *mismatches = 0;
    // n draws of a voxel key (splitmix64), coordinates in [0, spread); the container numbers the distinct ones by first insertion
    std::unordered_map<Key3, int, HashKey3> map;
    if (reserve > 0) map.reserve((size_t) reserve);
    std::vector<uint64_t> hashes;
    uint64_t st = seed;
    auto next = [&st]() {
        uint64_t z = (st += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    };
    for (int i = 0; i < n; ++i) {
        const Key3 k{(int) (next() % (uint64_t) spread), (int) (next() % (uint64_t) spread), (int) (next() % (uint64_t) spread)};
        if (map.emplace(k, (int) hashes.size()).second) hashes.push_back(lgr_hash_voxel(k.x, k.y, k.z));
    }
    const int ne = (int) hashes.size();
    if (ne == 0) return LGR_OK;
    std::vector<int32_t> want;
    want.reserve(ne);
    for (const auto& kv : map) {
        want.push_back(kv.second);
        if ((uint64_t) HashKey3()(kv.first) != hashes[kv.second]) ++*mismatches;   // the header's hash against the library's
    }
    std::vector<int32_t> rule(ne), got(ne);
    lgr_hash_order_host(hashes.data(), ne, reserve, rule.data());
    unsigned long long* d_hash;
    LGR_TRY(lgr_ws_t(ctx, WS_HO_HASH, (size_t) ne * 2 + 2, &d_hash));
    int32_t* d_order = (int32_t*) (d_hash + ne);
    LGR_HIP(ctx, hipMemcpyAsync(d_hash, hashes.data(), (size_t) ne * 8, hipMemcpyHostToDevice, ctx->stream));
    LGR_TRY(lgr_hash_order_launch(ctx, d_hash, ne, reserve, d_order));
    LGR_HIP(ctx, hipMemcpyAsync(got.data(), d_order, (size_t) ne * 4, hipMemcpyDeviceToHost, ctx->stream));
    LGR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < ne; ++i) *mismatches += (got[i] != want[i]) + (rule[i] != want[i]);
    return LGR_OK;
}
