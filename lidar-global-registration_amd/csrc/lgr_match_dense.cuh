// lgr_match_dense.cuh -- what the exact dense matchers share: the packed operand layout and the 64 x 64 tile of pair distances.
// Included by lgr_match_dense.hip (nearest row) and lgr_match_knn.hip (k nearest rows): one statement of the distance, two selections.
#pragma once
#include "lgr_internal.h"

namespace {

// cv::hal::normL2Sqr_ (OpenCV 4.5.1, SSE baseline) for n = 352: 22 blocks of 16; acc[k][lane] += t * t for element
// 16 b + 4 k + lane; s = ((acc0 + acc1) + acc2) + acc3 lane-wise; d2 = (s0 + s2) + (s1 + s3).  The 16 (k, lane) chains are independent,
// so the rows are packed with the elements of one chain contiguous -- group (lane, k) = 4 lane + k, 22 elements in block order -- and
// transposed (element-major, rows padded to 64) for coalesced tile loads.  A pair then runs the chains one after the other:
// sl = acc(lane, 0) + acc(lane, 1) + acc(lane, 2) + acc(lane, 3) in that order, A = s0 + s2, B = s1 + s3, d2 = A + B: the same
// operations on the same values as the SSE code.
// The kernels are templated on the block count NB and the scalar tail TAIL (row length 16 NB + TAIL): SHOT is <22, 0>, RoPS135
// <8, 7>, whose elements 128..134 follow the blocks as d2 += t * t one after the other (normL2Sqr_'s scalar loop), FPFH <2, 1>.
constexpr int MT = 64;                // rows per tile side
template <int NB, int TAIL>
__global__ void dense_pack_kernel(const float* __restrict__ rows, int m, int mpad, float* __restrict__ packed) {
    constexpr int LEN = 16 * NB + TAIL;
    const size_t e = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t) mpad * LEN) return;
    const int r = (int) (e % mpad), p = (int) (e / mpad);   // p: packed element = group * NB + b, group = 4 lane + k; then the tail
    const int grp = p / NB, b = p % NB, lane = grp >> 2, k = grp & 3;
    const int col = (TAIL == 0 || p < 16 * NB) ? 16 * b + 4 * k + lane : p;
    packed[e] = r < m ? rows[(size_t) r * LEN + col] : __uint_as_float(0x7fc00000u);
}

// The distances of one tile: 256 threads, rows q0 .. q0 + 63 of pa against rows t0 .. t0 + 63 of pb, 4 x 4 pairs per thread
// (tx = tid & 15, ty = tid >> 4): d[i][j] = sqrtf(normL2Sqr) of rows q0 + 4 ty + i and t0 + 4 tx + j.  sa / sb: the block's staging
// buffers.  Every thread of the block calls it (it synchronises); on return the buffers may still be read by other threads, the next
// call synchronises before it overwrites them.
template <int NB, int TAIL>
__device__ __forceinline__ void dense_tile_distances(const float* __restrict__ pa, int mpa, int q0, const float* __restrict__ pb, int mpb, int t0,
                                                     float4 (*sa)[MT / 4], float4 (*sb)[MT / 4], float (&d)[4][4]) {
    static_assert(TAIL <= NB, "the tail is staged in the block buffers");
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    float sA[4][4], sB[4][4], sl[4][4], acc[4][4];
    for (int grp = 0; grp < 16; ++grp) {
        __syncthreads();
        for (int e = tid; e < NB * (MT / 4); e += 256) {
            const int b = e / (MT / 4), c = e % (MT / 4);
            sa[b][c] = reinterpret_cast<const float4*>(pa + (size_t) (grp * NB + b) * mpa + q0)[c];
            sb[b][c] = reinterpret_cast<const float4*>(pb + (size_t) (grp * NB + b) * mpb + t0)[c];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
        for (int b = 0; b < NB; ++b) {
            const float4 a4 = sa[b][ty], b4 = sb[b][tx];
            const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float t = av[i] - bv[j]; acc[i][j] = t * t + acc[i][j]; }
        }
        const int k = grp & 3, lane = grp >> 2;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sl[i][j] = k == 0 ? acc[i][j] : sl[i][j] + acc[i][j];
                if (k == 3) {
                    if (lane == 0) sA[i][j] = sl[i][j];
                    else if (lane == 1) sB[i][j] = sl[i][j];
                    else if (lane == 2) sA[i][j] = sA[i][j] + sl[i][j];
                    else sB[i][j] = sB[i][j] + sl[i][j];
                }
            }
    }
    if constexpr (TAIL > 0) {   // d2 = A + B, then d2 += t * t for the tail elements in order
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) sA[i][j] = sA[i][j] + sB[i][j];
        __syncthreads();
        for (int e = tid; e < TAIL * (MT / 4); e += 256) {
            const int b = e / (MT / 4), c = e % (MT / 4);
            sa[b][c] = reinterpret_cast<const float4*>(pa + (size_t) (16 * NB + b) * mpa + q0)[c];
            sb[b][c] = reinterpret_cast<const float4*>(pb + (size_t) (16 * NB + b) * mpb + t0)[c];
        }
        __syncthreads();
        for (int b = 0; b < TAIL; ++b) {
            const float4 a4 = sa[b][ty], b4 = sb[b][tx];
            const float av[4] = {a4.x, a4.y, a4.z, a4.w}, bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) { const float t = av[i] - bv[j]; sA[i][j] = sA[i][j] + t * t; }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) d[i][j] = TAIL > 0 ? sqrtf(sA[i][j]) : sqrtf(sA[i][j] + sB[i][j]);
}

}  // namespace
