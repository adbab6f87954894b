// hash_order_ref.cpp -- the truth csrc/lgr_stdhash.h is held to: this compiler's std::hash<float> / std::hash<int>, the folded
// HashEigen / PointHash of the reference (include/common.h:202-223) and the iteration order of a real std::unordered_map /
// std::unordered_set, beside the header's restatement of each.  Built by tests/hash_order_ref_lib.py with g++.
#include <cstdint>
#include <cstring>
#include <functional>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../lidar-global-registration_amd/csrc/lgr_stdhash.h"

namespace {
struct Key3 { int x, y, z; bool operator==(const Key3& o) const { return x == o.x && y == o.y && z == o.z; } };
struct HashKey3 {   // HashEigen<Eigen::Vector3i>
    size_t operator()(const Key3& k) const {
        size_t seed = 0;
        const int e[3] = {k.x, k.y, k.z};
        for (int i = 0; i < 3; ++i) seed ^= std::hash<int>()(e[i]) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
        return seed;
    }
};
struct Pt { float v[3]; int id; };
struct PtHash {     // PointHash
    size_t operator()(const Pt& p) const {
        size_t seed = 0;
        for (int a = 0; a < 3; ++a) seed ^= std::hash<float>()(p.v[a]) + 0x9e3779b9 + (seed << 6) + (seed >> 2);
        return seed;
    }
};
struct PtEq {
    bool operator()(const Pt& a, const Pt& b) const { return a.v[0] == b.v[0] && a.v[1] == b.v[1] && a.v[2] == b.v[2]; }
};
}  // namespace

extern "C" {

void hor_hash_float(const uint32_t* bits, long long n, uint64_t* out_std, uint64_t* out_hdr) {
    for (long long i = 0; i < n; ++i) {
        float f;
        memcpy(&f, bits + i, 4);
        out_std[i] = (uint64_t) std::hash<float>()(f);
        out_hdr[i] = lgr_std_hash_float_bits(bits[i]);
    }
}

void hor_hash_voxel(const int* xyz, long long n, uint64_t* out_std, uint64_t* out_hdr) {
    for (long long i = 0; i < n; ++i) {
        out_std[i] = (uint64_t) HashKey3()(Key3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
        out_hdr[i] = lgr_hash_voxel(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    }
}

void hor_hash_point(const uint32_t* bits3, long long n, uint64_t* out_std, uint64_t* out_hdr) {
    for (long long i = 0; i < n; ++i) {
        Pt p{};
        memcpy(p.v, bits3 + 3 * i, 12);
        out_std[i] = (uint64_t) PtHash()(p);
        out_hdr[i] = lgr_hash_point_bits(bits3[3 * i], bits3[3 * i + 1], bits3[3 * i + 2]);
    }
}

// the element counts at which an insertion into a container without reserve() rehashes, from the policy object, up to `limit`
int hor_rehash_counts(long long limit, long long* out, int cap) {
    std::__detail::_Prime_rehash_policy pol;
    size_t bkt = 1;
    int c = 0;
    for (long long e = 0; e <= limit; ++e) {
        const auto r = pol._M_need_rehash(bkt, (size_t) e, 1);
        if (r.first) { bkt = r.second; if (c < cap) out[c] = e; ++c; }
    }
    return c;
}

// n_draws voxel keys -> unordered_map (reserve(reserve) first when > 0); elements are numbered by first insertion.  hashes,
// order_container, order_rule: n_draws entries each; returns the number of elements.
int hor_map_order(const int* xyz, int n_draws, long long reserve, uint64_t* hashes, int32_t* order_container, int32_t* order_rule) {
    std::unordered_map<Key3, int, HashKey3> m;
    if (reserve > 0) m.reserve((size_t) reserve);
    int n = 0;
    for (int i = 0; i < n_draws; ++i) {
        const Key3 k{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
        if (m.find(k) == m.end()) { m[k] = n; hashes[n] = lgr_hash_voxel(k.x, k.y, k.z); ++n; }
    }
    int o = 0;
    for (const auto& kv : m) order_container[o++] = kv.second;
    lgr_hash_order_host(hashes, n, reserve, order_rule);
    return n;
}

// n points (x, y, z) -> unordered_set after reserve(n), as filterDuplicatePoints does
int hor_set_order(const float* xyz, int n_pts, uint64_t* hashes, int32_t* order_container, int32_t* order_rule) {
    std::unordered_set<Pt, PtHash, PtEq> s;
    s.reserve((size_t) n_pts);
    int n = 0;
    for (int i = 0; i < n_pts; ++i) {
        Pt p{{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}, n};
        if (s.insert(p).second) {
            uint32_t b[3];
            memcpy(b, p.v, 12);
            hashes[n++] = lgr_hash_point_bits(b[0], b[1], b[2]);
        }
    }
    int o = 0;
    for (const Pt& p : s) order_container[o++] = p.id;
    lgr_hash_order_host(hashes, n, n_pts, order_rule);
    return n;
}

// caller-made hash codes through a real container (identity hash over the code, equality over the element id): the replay the GPU
// tests compare lgr_hash_order_dev with
void hor_replay(const uint64_t* hashes, int n, long long reserve, int32_t* order_container) {
    struct E { uint64_t h; int id; };
    struct EH { size_t operator()(const E& e) const { return (size_t) e.h; } };
    struct EE { bool operator()(const E& a, const E& b) const { return a.id == b.id; } };
    std::unordered_set<E, EH, EE> s;
    if (reserve > 0) s.reserve((size_t) reserve);
    for (int i = 0; i < n; ++i) s.insert(E{hashes[i], i});
    int o = 0;
    for (const E& e : s) order_container[o++] = e.id;
}

void hor_rule(const uint64_t* hashes, int n, long long reserve, int32_t* order_rule) { lgr_hash_order_host(hashes, n, reserve, order_rule); }

}  // extern "C"
