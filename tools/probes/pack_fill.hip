// Write-only yardstick of the matcher's column packing (pack16_kernel, role 1): the 16 column sets of a 1M-row train side, 2.1 GB,
// written with the packing kernel's store shape and nothing else -- 16-byte stores, 512 contiguous bytes per half wave, fragment order
// ((set * tiles + tile) * NF + f) * 64 + lane -- so that the kernel's time can be stated as a ratio to what the stores alone cost.
//   hipcc -O3 --offload-arch=gfx950 tools/probes/pack_fill.hip -o build/pack_fill && build/pack_fill [rows]
// Variants: a lane owns a row and walks the sets (the packing kernel's order) or one set per blockIdx.y; plain or non-temporal stores.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int KCL = 16, NF = 4, TILE = 32;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <bool NT, bool SET_Y>
__global__ __launch_bounds__(256) void fill_kernel(f16x8* __restrict__ P, int n_pad) {
    const int pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n_pad) return;
    const int tile = pos >> 5, r = pos & 31;
    const int set0 = SET_Y ? blockIdx.y : 0, set1 = SET_Y ? blockIdx.y + 1 : KCL;
#pragma unroll 1
    for (int set = set0; set < set1; ++set) {
        f16x8* base = P + ((size_t) set * (n_pad / TILE) + tile) * NF * 64 + r;
        f16x8 w;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = (_Float16) (float) ((pos + set + j) & 1023);
#pragma unroll
        for (int piece = 0; piece < 2 * NF; ++piece) {
            f16x8* q = base + (piece >> 1) * 64 + ((piece & 1) << 5);
            if (NT) __builtin_nontemporal_store(w, q); else *q = w;
        }
    }
}

template <bool NT, bool SET_Y>
static int run(const char* name, f16x8* P, int n_pad, size_t bytes) {
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    const dim3 grid((n_pad + 255) / 256, SET_Y ? KCL : 1);
    std::vector<float> ms;
    for (int rep = 0; rep < 12; ++rep) {
        CHECK(hipEventRecord(e0));
        fill_kernel<NT, SET_Y><<<grid, 256>>>(P, n_pad);
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float t;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 2) ms.push_back(t);   // two warm-up launches
    }
    std::sort(ms.begin(), ms.end());
    const float med = ms[ms.size() / 2];
    printf("%-34s min %.3f ms  median %.3f ms  max %.3f ms  -> %.2f TB/s at the median\n", name, ms.front(), med, ms.back(), bytes / med * 1e-9);
    return 0;
}

int main(int argc, char** argv) {
    const int rows = argc > 1 ? atoi(argv[1]) : 1000000;
    if (rows <= 0 || rows > 8000000) { fprintf(stderr, "rows out of range\n"); return 1; }
    const int n_pad = (rows + 255) / 256 * 256;
    const size_t bytes = (size_t) KCL * (n_pad / TILE) * NF * 64 * sizeof(f16x8);
    f16x8* P;
    CHECK(hipMalloc(&P, bytes));
    printf("%d rows (padded %d), %d sets, %.3f GB\n", rows, n_pad, KCL, bytes * 1e-9);
    if (run<false, false>("lane walks the sets, plain", P, n_pad, bytes)) return 1;
    if (run<true, false>("lane walks the sets, non-temporal", P, n_pad, bytes)) return 1;
    if (run<false, true>("one set per blockIdx.y, plain", P, n_pad, bytes)) return 1;
    if (run<true, true>("one set per blockIdx.y, non-temporal", P, n_pad, bytes)) return 1;
    CHECK(hipFree(P));
    return 0;
}
