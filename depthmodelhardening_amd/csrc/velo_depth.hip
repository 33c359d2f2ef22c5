// K32 -- the sparse depth map of a velodyne scan, MD2/kitti_utils.py:46-98 (generate_depth_map) with the loader's nearest
// resize and flip (MD2/datasets/kitti_dataset.py:70-85), for a batch of frames, float32-equal to the reference (gfx950).
//
// The reference projects the points of one frame in float64 on the host and resolves pixels that several points hit in a Python
// loop over a Counter: 309 ms per 375 x 1242 frame of 120 k points.  Per point it is a 3 x 4 projection, a rounding and a
// scatter-min.
//
// What the reference computes, as this file restates it (ops.velo_depth_map_host is the same arithmetic in numpy):
//   a point (x, y, z, .) is kept if x >= 0 (float32; a NaN fails);
//   q = P (x, y, z, 1) in float64 with the fixed order ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3], no contraction;
//   u = rint(q0 / q2) - 1, v = rint(q1 / q2) - 1 (IEEE division, half to even), kept if 0 <= u < W and 0 <= v < H in float64;
//   the value is d = q2, or x under vel_depth; the map holds float32(max(d, 0)).
//   Every pixel holds the minimum over its own points -- rounding to float32 and the clamp are monotone, so each point clamps and
//   casts its own value and the minimum is an integer atomicMin on the bits of a non-negative float (order-independent) --
//   except for the reference's sub2ind, row * (W - 1) + col - 1, which gives A = (y, W - 1) and B = (y + 1, 0) the same key.
//   When both pixels of such a pair hold points, the one that holds the earliest point of the pair in file order receives the
//   minimum over both pixels' points, and the other keeps the value of the LAST point that fell on it (the plain scatter).
//   For the cells of columns 0 and W - 1 two more integer atomics therefore keep the smallest and the largest point index; the
//   finalise pass recomputes the last point's value from its index.
//
// Three launches: fill (workspace to all ones = "empty"), scatter (one thread per point), finalise (one thread per output
// element: pair rule, nearest resize with source index ((2 o + 1) in) / (2 out), mirrored read for flip, store).  Every output
// element is written.  Integer atomics only: bitwise reproducible.  Every index derived from data is checked before use.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t LAST_BASE = 0xFFFFFFFEu;      // the largest index is kept as the minimum of LAST_BASE - index

struct Frame {
    int H, W, cell_off, row_off;
    bool ok;
};

// desc: int32 [n][4] = rows, columns, offset of the frame's cells in the workspace (and in the native-size output), offset of
// its rows in the edge table.  A descriptor that points outside the workspace is a host bug; it must not become an access out
// of bounds.
__device__ __forceinline__ Frame load_frame(const int32_t* __restrict__ desc, int f, int total_cells, int total_rows) {
    Frame fr;
    fr.H = desc[f * 4 + 0];
    fr.W = desc[f * 4 + 1];
    fr.cell_off = desc[f * 4 + 2];
    fr.row_off = desc[f * 4 + 3];
    fr.ok = fr.H >= 1 && fr.W >= 2 && fr.cell_off >= 0 && fr.row_off >= 0 && (int64_t)fr.H * fr.W <= (int64_t)total_cells - fr.cell_off
            && fr.H <= total_rows - fr.row_off;
    return fr;
}

// the largest f in [0, n) with table[f * stride] <= i (table[0] <= i is the caller's)
__device__ __forceinline__ int find_frame(const int32_t* __restrict__ table, int stride, int n, int i) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid * stride] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// row r of P (x, y, z, 1): separate IEEE multiplications and additions in the reference's order, never fused
__device__ __forceinline__ double project_row(const double* __restrict__ P, int r, double x, double y, double z) {
#pragma clang fp contract(off)
    const double a = P[r * 4 + 0] * x;
    const double b = P[r * 4 + 1] * y;
    const double c = P[r * 4 + 2] * z;
    const double ab = a + b;
    const double abc = ab + c;
    return abc + P[r * 4 + 3];
}

// float32(max(d, 0)) as bits: non-negative floats order as their bit patterns do (a -0.0 becomes +0.0)
__device__ __forceinline__ uint32_t depth_bits(double d) {
    const float v = d > 0.0 ? (float)d : 0.f;
    return __float_as_uint(v);
}

__device__ __forceinline__ uint32_t point_value(const float4 p, const double* __restrict__ P, int vel_depth) {
    return depth_bits(vel_depth ? (double)p.x : project_row(P, 2, (double)p.x, (double)p.y, (double)p.z));
}

__global__ __launch_bounds__(NT) void velo_fill_kernel(uint32_t* __restrict__ ws, int words) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < words) ws[i] = EMPTY;
}

__global__ __launch_bounds__(NT) void velo_scatter_kernel(const float4* __restrict__ points, int npts, const int32_t* __restrict__ offsets,
                                                          const double* __restrict__ proj, const int32_t* __restrict__ desc, int n,
                                                          int vel_depth, int total_cells, int total_rows, uint32_t* __restrict__ ws) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= npts || offsets[0] > i) return;
    const int f = find_frame(offsets, 1, n, i);
    if (i >= offsets[f + 1]) return;                       // past the frame's end: offsets that do not ascend drop the point
    const Frame fr = load_frame(desc, f, total_cells, total_rows);
    if (!fr.ok) return;
    const float4 p = points[i];
    if (!(p.x >= 0.f)) return;
    const double* P = proj + f * 12;
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    const double q0 = project_row(P, 0, x, y, z), q1 = project_row(P, 1, x, y, z), q2 = project_row(P, 2, x, y, z);
    const double u = rint(__ddiv_rn(q0, q2)) - 1.0, v = rint(__ddiv_rn(q1, q2)) - 1.0;
    if (!(u >= 0.0 && v >= 0.0 && u < (double)fr.W && v < (double)fr.H)) return;      // NaN and inf fall out here
    const int ui = (int)u, vi = (int)v;
    const uint32_t bits = depth_bits(vel_depth ? x : q2);
    atomicMin(ws + fr.cell_off + vi * fr.W + ui, bits);
    if (ui == 0 || ui == fr.W - 1) {
        uint32_t* e = ws + total_cells + ((fr.row_off + vi) * 2 + (ui == 0 ? 0 : 1)) * 2;
        atomicMin(e, (uint32_t)i);
        atomicMin(e + 1, LAST_BASE - (uint32_t)i);
    }
}

// the reference's value of cell (y, x) of frame f: the minimum, or what the pair rule leaves
__device__ __forceinline__ float cell_value(const Frame fr, int f, int y, int x, const float4* __restrict__ points, int npts,
                                            const double* __restrict__ proj, int vel_depth, int total_cells,
                                            const uint32_t* __restrict__ ws) {
    const uint32_t m = ws[fr.cell_off + y * fr.W + x];
    if (m == EMPTY) return 0.f;
    const bool right = x == fr.W - 1, left = x == 0;
    const int py = right ? y + 1 : y - 1;                  // the partner's row; its column is the other edge
    if ((right || left) && py >= 0 && py < fr.H) {
        const uint32_t pm = ws[fr.cell_off + py * fr.W + (right ? 0 : fr.W - 1)];
        if (pm != EMPTY) {
            const uint32_t* mine = ws + total_cells + ((fr.row_off + y) * 2 + (left ? 0 : 1)) * 2;
            const uint32_t* theirs = ws + total_cells + ((fr.row_off + py) * 2 + (left ? 1 : 0)) * 2;
            if (mine[0] < theirs[0]) return __uint_as_float(min(m, pm));
            const uint32_t last = LAST_BASE - mine[1];
            if (last >= (uint32_t)npts) return 0.f;         // cannot happen: the scatter wrote an index < npts
            return __uint_as_float(point_value(points[last], proj + f * 12, vel_depth));
        }
    }
    return __uint_as_float(m);
}

// RESIZED: out [n][out_h][out_w]; otherwise the maps at their own sizes, frame f at desc[f].cell_off
template <bool RESIZED>
__global__ __launch_bounds__(NT) void velo_finalise_kernel(const float4* __restrict__ points, int npts, const double* __restrict__ proj,
                                                           const int32_t* __restrict__ desc, const int32_t* __restrict__ flip, int n,
                                                           int vel_depth, int total_cells, int total_rows, const uint32_t* __restrict__ ws,
                                                           int out_h, int out_w, int out_len, float* __restrict__ out) {
    const int o = blockIdx.x * NT + threadIdx.x;
    if (o >= out_len) return;
    int f, y, x;
    Frame fr;
    if (RESIZED) {
        f = o / (out_h * out_w);
        const int r = o - f * (out_h * out_w);
        const int oy = r / out_w;
        int ox = r - oy * out_w;
        fr = load_frame(desc, f, total_cells, total_rows);
        if (!fr.ok) { out[o] = 0.f; return; }
        if (flip != nullptr && flip[f] != 0) ox = out_w - 1 - ox;
        y = (int)(((int64_t)(2 * oy + 1) * fr.H) / (2 * out_h));
        x = (int)(((int64_t)(2 * ox + 1) * fr.W) / (2 * out_w));
    } else {
        if (desc[2] > o) { out[o] = 0.f; return; }
        f = find_frame(desc + 2, 4, n, o);
        fr = load_frame(desc, f, total_cells, total_rows);
        const int r = o - fr.cell_off;
        if (!fr.ok || r >= fr.H * fr.W) { out[o] = 0.f; return; }
        y = r / fr.W;
        x = r - y * fr.W;
        if (flip != nullptr && flip[f] != 0) x = fr.W - 1 - x;
    }
    out[o] = cell_value(fr, f, y, x, points, npts, proj, vel_depth, total_cells, ws);
}

}  // namespace

extern "C" {

int64_t dmh_velo_depth_ws_size(int64_t total_cells, int64_t total_rows) {
    if (total_cells < 1 || total_rows < 1 || total_cells + 4 * total_rows >= (1ll << 31)) return -1;
    return total_cells + 4 * total_rows;
}

int dmh_velo_depth_map(const float* points, int64_t npts, const int32_t* offsets, const double* proj, const int32_t* desc,
                       const int32_t* flip, int n, int vel_depth, int64_t total_cells, int64_t total_rows, int out_h, int out_w,
                       uint32_t* ws, float* out, void* stream) {
    DMH_REQUIRE(offsets && proj && desc && ws && out, "null pointer");
    DMH_REQUIRE(points || npts == 0, "null points");
    DMH_REQUIRE(n > 0 && n <= (1 << 20), "need 0 < n <= 2^20 frames");
    DMH_REQUIRE(npts >= 0 && npts < (1ll << 31) - NT, "need 0 <= npts < 2^31 - 256");
    DMH_REQUIRE(dmh_velo_depth_ws_size(total_cells, total_rows) > 0, "need total_cells, total_rows >= 1 and total_cells + 4 total_rows < 2^31");
    DMH_REQUIRE((out_h > 0 && out_w > 0) || (out_h == 0 && out_w == 0), "out_h and out_w must both be positive or both be 0 (native sizes)");
    const int64_t out_len = out_h > 0 ? (int64_t)n * out_h * out_w : total_cells;
    DMH_REQUIRE(out_len < (1ll << 31) - NT, "the output must hold fewer than 2^31 - 256 elements");
    DMH_REQUIRE(((uintptr_t)points & 15) == 0 && ((uintptr_t)proj & 7) == 0, "points must be 16-byte, proj 8-byte aligned");
    DMH_REQUIRE(((uintptr_t)offsets & 3) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)flip & 3) == 0 && ((uintptr_t)ws & 3) == 0
                    && ((uintptr_t)out & 3) == 0, "offsets, desc, flip, ws and out must be 4-byte aligned");
    DMH_REQUIRE((const void*)out != (const void*)ws && (const void*)out != (const void*)points, "out must not alias ws or points");
    const hipStream_t s = (hipStream_t)stream;
    const int words = (int)(total_cells + 4 * total_rows);
    // a fill kernel, not hipMemsetAsync: a captured graph must replay it
    hipLaunchKernelGGL(velo_fill_kernel, dim3((words + NT - 1) / NT), dim3(NT), 0, s, ws, words);
    if (npts > 0)
        hipLaunchKernelGGL(velo_scatter_kernel, dim3((unsigned)((npts + NT - 1) / NT)), dim3(NT), 0, s, (const float4*)points, (int)npts,
                           offsets, proj, desc, n, vel_depth != 0, (int)total_cells, (int)total_rows, ws);
    const dim3 grid((unsigned)((out_len + NT - 1) / NT));
    if (out_h > 0)
        hipLaunchKernelGGL(velo_finalise_kernel<true>, grid, dim3(NT), 0, s, (const float4*)points, (int)npts, proj, desc, flip, n,
                           vel_depth != 0, (int)total_cells, (int)total_rows, ws, out_h, out_w, (int)out_len, out);
    else
        hipLaunchKernelGGL(velo_finalise_kernel<false>, grid, dim3(NT), 0, s, (const float4*)points, (int)npts, proj, desc, flip, n,
                           vel_depth != 0, (int)total_cells, (int)total_rows, ws, out_h, out_w, (int)out_len, out);
    return check_launch("dmh_velo_depth_map");
}

}  // extern "C"
