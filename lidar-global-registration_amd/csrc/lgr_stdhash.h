// lgr_stdhash.h -- libstdc++'s hash containers restated: the two hashes the reference feeds them and the iteration order they end
// up in, shared by host and device code (and by tests/cpp/hash_order_ref.cpp, which pins every statement here against the real
// std::hash / std::unordered_map / std::unordered_set of the compiler at hand).
//
// The reference numbers its points by the iteration order of
//   std::unordered_set<PointN, PointHash, PointEqual>          filterDuplicatePoints,  src/common.cpp:417-427 (reserve(n))
//   std::unordered_map<Eigen::Vector3i, ..., HashEigen<...>>   downsamplePointCloud,   src/downsample.cpp:20,32-34
// Both hashes fold  seed ^= hash(elem) + 0x9e3779b9 + (seed << 6) + (seed >> 2)  in 64-bit arithmetic (include/common.h:202-223).
//
// The order rule.  Elements = the distinct keys, numbered 0..n-1 by first insertion, element e with hash code h[e].  The bucket
// count changes at the element counts the runtime's std::__detail::_Prime_rehash_policy names (lgr_hash_schedule drives the policy
// object itself, no prime table is copied); an EPOCH is one bucket count B, from one rehash up to just before the next.  With P
// the list over the m elements present when the rehash fires (empty for the first epoch), an old element's TIME is its position
// in P and a new element e (m <= e < m') has time e; act(b) = the smallest time among the elements with h % B == b.  The list
// after the epoch is all m' elements by (act(bucket) descending, time descending): libstdc++ puts a node into a non-empty bucket
// at the front of that bucket's run and into an empty bucket at the head of the whole list, and _M_rehash_aux does the same while
// it walks the old list from its head.  The iteration order is the list after the last epoch.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LGR_STDHASH_HD __host__ __device__ inline
#else
#define LGR_STDHASH_HD inline
#endif

// std::hash<int>: the value, sign-extended to size_t
LGR_STDHASH_HD uint64_t lgr_std_hash_int(int v) { return (uint64_t) (int64_t) v; }

// std::hash<float>: 0 for +-0, else the 64-bit _Hash_bytes (libsupc++ hash_bytes.cc, the Murmur-style mix) of the value's 4 bytes
// with seed 0xc70f6907: no 8-byte block, one tail of 4 bytes
LGR_STDHASH_HD uint64_t lgr_std_hash_float_bits(uint32_t bits) {
    if ((bits & 0x7fffffffu) == 0u) return 0ull;
    const uint64_t mul = 0xc6a4a7935bd1e995ull;
    uint64_t hash = 0xc70f6907ull ^ (4ull * mul);
    hash ^= (uint64_t) bits;
    hash *= mul;
    hash = (hash ^ (hash >> 47)) * mul;
    hash ^= hash >> 47;
    return hash;
}

LGR_STDHASH_HD uint64_t lgr_hash_fold(uint64_t seed, uint64_t h) { return seed ^ (h + 0x9e3779b9ull + (seed << 6) + (seed >> 2)); }

// HashEigen<Eigen::Vector3i> of a voxel index (include/common.h:212-223)
LGR_STDHASH_HD uint64_t lgr_hash_voxel(int ix, int iy, int iz) {
    uint64_t seed = 0;
    seed = lgr_hash_fold(seed, lgr_std_hash_int(ix));
    seed = lgr_hash_fold(seed, lgr_std_hash_int(iy));
    seed = lgr_hash_fold(seed, lgr_std_hash_int(iz));
    return seed;
}

// PointHash of a point's coordinates, given as bit patterns (include/common.h:202-210 + include/utils.h:28-32)
LGR_STDHASH_HD uint64_t lgr_hash_point_bits(uint32_t bx, uint32_t by, uint32_t bz) {
    uint64_t seed = 0;
    seed = lgr_hash_fold(seed, lgr_std_hash_float_bits(bx));
    seed = lgr_hash_fold(seed, lgr_std_hash_float_bits(by));
    seed = lgr_hash_fold(seed, lgr_std_hash_float_bits(bz));
    return seed;
}

// ---- host side ----
#include <algorithm>
#include <unordered_map>
#include <vector>

inline uint64_t lgr_std_hash_float(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return lgr_std_hash_float_bits(b);
}

// elements [begin, end) are inserted under `buckets` buckets; the rehash to that count fires when `begin` elements are present
struct lgr_hash_epoch { long long begin, end; unsigned long long buckets; };

// The bucket schedule of n insertions into an empty container, after reserve(reserve) when reserve > 0, from the runtime's own
// policy object.  _M_need_rehash(bkt, e, 1) is what every insertion of a new key asks; between two thresholds (_M_next_resize) it
// answers false without touching its state, so those calls are skipped.
inline std::vector<lgr_hash_epoch> lgr_hash_schedule(long long n, long long reserve) {
    std::vector<lgr_hash_epoch> ep;
    if (n <= 0) return ep;
    std::__detail::_Prime_rehash_policy pol;
    size_t bkt = 1;
    if (reserve > 0) bkt = pol._M_next_bkt(pol._M_bkt_for_elements((size_t) reserve));
    ep.push_back({0, n, (unsigned long long) bkt});
    long long e = 0;
    while (e < n) {
        const std::pair<bool, size_t> r = pol._M_need_rehash(bkt, (size_t) e, 1);
        if (r.first) {
            bkt = r.second;
            if (ep.back().begin == e) ep.back().buckets = bkt;   // nothing was inserted under the count before
            else { ep.back().end = e; ep.push_back({e, n, (unsigned long long) bkt}); }
        }
        e = std::max<long long>(e + 1, (long long) pol._M_next_resize);
    }
    return ep;
}

// The order rule above, plainly: order[0..n) = the element ids in iteration order
inline void lgr_hash_order_host(const uint64_t* h, long long n, long long reserve, int32_t* order) {
    std::vector<int32_t> P, next;
    std::vector<long long> time, act;
    for (const lgr_hash_epoch& ep : lgr_hash_schedule(n, reserve)) {
        const long long m = (long long) P.size(), m2 = ep.end;
        time.assign((size_t) m2, 0);
        for (long long t = 0; t < m; ++t) time[(size_t) P[(size_t) t]] = t;
        for (long long e = m; e < m2; ++e) time[(size_t) e] = e;
        act.assign((size_t) ep.buckets, m2);
        for (long long e = 0; e < m2; ++e) {
            long long& a = act[(size_t) (h[e] % ep.buckets)];
            a = std::min(a, time[(size_t) e]);
        }
        next.resize((size_t) m2);
        for (long long e = 0; e < m2; ++e) next[(size_t) e] = (int32_t) e;
        std::sort(next.begin(), next.end(), [&](int32_t a, int32_t b) {
            const long long aa = act[(size_t) (h[a] % ep.buckets)], ab = act[(size_t) (h[b] % ep.buckets)];
            return aa != ab ? aa > ab : time[(size_t) a] > time[(size_t) b];
        });
        P.swap(next);
    }
    for (long long i = 0; i < n; ++i) order[i] = P[(size_t) i];
}
