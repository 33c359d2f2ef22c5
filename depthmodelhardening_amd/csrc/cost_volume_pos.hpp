// What K30 (cost_volume.hip) and K38 (cost_volume_bwd.hip) share: the tile constants, the channels-last transposing pass and the
// fp32 position arithmetic of the plane sweep.  The backward must take every edge flag exactly as the forward took it, so both
// translation units compile these very functions; each gets its own internal copy (anonymous namespace).
#pragma once
#include "common.hpp"

namespace {

constexpr int NT = 256;
constexpr int GL = 16;               // lanes per group = float4 words per tap
constexpr int TILE = 32;             // pixels per workgroup (two per group)
constexpr int CH = 64;
constexpr int MAX_D = 128;
constexpr int MAX_L = 16;
constexpr int DP = MAX_D + 1;        // LDS row stride: odd, so a column walk over the 32 pixels is conflict-free

// [N][64][HW] -> [N][HW][64], 64 x 64 tiles through LDS
__global__ __launch_bounds__(NT) void cost_volume_nhwc_kernel(const float* __restrict__ x, float* __restrict__ y, int HW, int tiles) {
    __shared__ float t[CH][CH + 1];
    const int n = blockIdx.x / tiles, p0 = (blockIdx.x - n * tiles) * 64;
    const float* __restrict__ src = x + (int64_t)n * CH * HW;
    float* __restrict__ dst = y + (int64_t)n * CH * HW;
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    if (p0 + lo < HW) {
#pragma unroll 4
        for (int c = hi; c < CH; c += 4) t[c][lo] = src[(int64_t)c * HW + p0 + lo];
    }
    __syncthreads();
#pragma unroll 4
    for (int p = hi; p < 64; p += 4)
        if (p0 + p < HW) dst[(int64_t)(p0 + p) * CH + lo] = t[lo][p];
}

// P = (K @ T)[:3] (manydepth2/layers.py:185), row by row, the products summed in index order
__device__ __forceinline__ void project_matrix(const float* __restrict__ Kb, const float* __restrict__ T, float* P) {
#pragma clang fp contract(off)
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            float a = Kb[r * 4 + 0] * T[0 * 4 + c];
            a = a + Kb[r * 4 + 1] * T[1 * 4 + c];
            a = a + Kb[r * 4 + 2] * T[2 * 4 + c];
            a = a + Kb[r * 4 + 3] * T[3 * 4 + c];
            P[r * 4 + c] = a;
        }
}

// invK[:3, :3] @ (x, y, 1) (manydepth2/layers.py:165)
__device__ __forceinline__ void back_project(const float* __restrict__ iK, float x, float y, float& cx, float& cy, float& cz) {
#pragma clang fp contract(off)
    cx = iK[0] * x + iK[1] * y + iK[2];
    cy = iK[4] * x + iK[5] * y + iK[6];
    cz = iK[8] * x + iK[9] * y + iK[10];
}

// grid_sample's pixel position (align_corners = True) of the point (cx, cy, cz) * depth under P, or ix = -1 where the reference's
// edge mask is 0 (positions with the mask set have ix >= 2)
__device__ __forceinline__ void sample_pos(const float* P, float cx, float cy, float cz, float depth, float wm1, float hm1,
                                           float& ix, float& iy) {
#pragma clang fp contract(off)
    const float X = depth * cx, Y = depth * cy, Z = depth * cz;
    float px = P[0] * X;
    px = px + P[1] * Y;
    px = px + P[2] * Z;
    px = px + P[3];
    float py = P[4] * X;
    py = py + P[5] * Y;
    py = py + P[6] * Z;
    py = py + P[7];
    float pz = P[8] * X;
    pz = pz + P[9] * Y;
    pz = pz + P[10] * Z;
    pz = pz + P[11];
    const float den = pz + 1e-7f;
    float u = px / den, v = py / den;
    u = u / wm1;
    v = v / hm1;
    const float gx = (u - 0.5f) * 2.0f, gy = (v - 0.5f) * 2.0f;
    const float xv = (gx / 2.0f + 0.5f) * wm1, yv = (gy / 2.0f + 0.5f) * hm1;
    const bool edge = xv >= 2.0f && xv <= wm1 - 1.0f && yv >= 2.0f && yv <= hm1 - 1.0f;
    ix = edge ? ((gx + 1.0f) / 2.0f) * wm1 : -1.0f;
    iy = ((gy + 1.0f) / 2.0f) * hm1;
}

}  // namespace
