// K30 -- ManyDepth's matching cost volume, forward only (gfx950).
//
// Replaces manydepth2/networks/resnet_encoder.py:157-236 (match_features), :258-265 (compute_confidence_mask) and the viz_cost_vol
// lines of forward (:294-296).  The reference loops over the batch on the host, repeats the lookup feature map D times (503 MB at
// 80 x 256 x 64, D = 96) for grid_sample and reads lookup_pose.sum() on the host per sample and lookup.  Here: one transposing
// pass over the lookup features and one launch that reads them and writes the volume; the "missing lookup" decision is taken from
// device memory, so the whole thing can be captured.
//
//   current   float [B][64][H][W]          layer-1 features of the current frame
//   lookup    float [B][L][64][H][W]       layer-1 features of the lookup frames (transposed to [B][L][H][W][64] into `nhwc`)
//   poses     float [Bp][L][4][4]          1 <= Bp <= B; samples b >= Bp and poses whose 16 entries sum to exactly 0 are missing
//   K, invK   float [B][4][4]
//   bins      float [D]                    depth hypotheses, D <= 128
//   outputs (each of the first two and `buffer` may be NULL):
//   cost_volume, missing   float [B][D][H][W]      what match_features returns
//   confidence             float [B][H][W]         ((cost * (1 - missing)) > 0).sum(bins) == D
//   argmin                 int   [B][H][W]         first minimum over bins of the cost with zeros read as 100
//   buffer                 float [B][64 + D][H][W] channels 64 .. 64 + D - 1 receive cost_volume * confidence (reduce_conv's input)
//
// Work split.  A workgroup of 256 threads owns 32 consecutive pixels of one row across all D bins: the maximum over bins, the
// confidence and the argmin are finished inside the launch from LDS, no atomics, no second launch.  The 256 threads are 16 groups
// of 16 lanes; a group owns two of the pixels.  Lane j of a group holds channels 4 j .. 4 j + 3 of the pixel's current-frame
// feature in registers for all bins and lookups, and reads one float4 of every tap: a tap of the channels-last map is 256
// contiguous bytes, one 16-byte word per lane.  The sample positions are NOT computed 16 times over: lane j computes the position
// of bin d0 + j, the group then walks the 16 bins with two lane broadcasts per bin, and the 16 x 16 partial sums are reduced by a
// halving exchange (15 shuffles for 16 bins) that leaves bin d0 + j's total in lane j -- a fixed order, so the result is the same
// bits on every run.  A sample whose edge flag is 0 contributes an exact zero whatever the taps hold (the reference multiplies by
// the mask), so its taps are not read; where the flag is 1 all four taps lie inside the map.
//
// The position arithmetic follows the reference's fp32 operation order (BackprojectDepth / Project3D / the x_vals re-derivation,
// manydepth2/layers.py:164-195) with contraction off: the edge flags sit on hard thresholds of these numbers.
#include "cost_volume_pos.hpp"      // the tile constants, the transposing pass and the position arithmetic, shared with K38

using namespace dmh;

namespace {

__global__ __launch_bounds__(NT) void cost_volume_kernel(const float* __restrict__ cur, const float* __restrict__ look,
                                                         const float* __restrict__ poses, const float* __restrict__ K,
                                                         const float* __restrict__ invK, const float* __restrict__ bins, int B, int L,
                                                         int Bp, int H, int W, int D, int set_max, int banded,
                                                         float* __restrict__ cost_volume, float* __restrict__ missing,
                                                         float* __restrict__ confidence, int* __restrict__ argmin,
                                                         float* __restrict__ buffer) {
    __shared__ float s_cost[TILE * DP];
    __shared__ float s_P[MAX_L][12];
    __shared__ int s_skip[MAX_L];
    __shared__ float s_max[TILE], s_conf[TILE];

    const int tilesW = (W + TILE - 1) / TILE;
    int id = blockIdx.x;
    if (banded) {       // workgroups i, i + 8, ... share an XCD: give each XCD one contiguous band of tiles (neighbouring taps)
        const int per = gridDim.x >> 3;
        if (id < per * 8) id = (id & 7) * per + (id >> 3);
    }
    const int tw = id % tilesW, h = (id / tilesW) % H, b = id / (tilesW * H);
    const int w0 = tw * TILE;
    const int grp = threadIdx.x / GL, lane = threadIdx.x & (GL - 1);
    const int HW = H * W;

    if (threadIdx.x < L) {
        const int l = threadIdx.x;
        int skip = 1;
        if (b < Bp) {
            const float* __restrict__ T = poses + ((int64_t)b * L + l) * 16;
            float s = 0.f;
            for (int i = 0; i < 16; ++i) s += T[i];
            skip = s == 0.f;
            float P[12];
            project_matrix(K + (int64_t)b * 16, T, P);
            for (int i = 0; i < 12; ++i) s_P[l][i] = P[i];
        }
        s_skip[l] = skip;
    }
    __syncthreads();

    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float* __restrict__ iK = invK + (int64_t)b * 16;

    for (int pp = 0; pp < TILE / (NT / GL); ++pp) {
        const int px = grp + pp * (NT / GL), w = w0 + px;
        if (w >= W) continue;                                           // (uniform over the group)
        const bool interior = h >= 2 && h < H - 2 && w >= 2 && w < W - 2;  // the current frame's own border is masked out
        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (interior) {
            const float* __restrict__ cp = cur + ((int64_t)b * CH + 4 * lane) * HW + (int64_t)h * W + w;
            c4 = make_float4(cp[0], cp[HW], cp[2 * (int64_t)HW], cp[3 * (int64_t)HW]);
            back_project(iK, (float)w, (float)h, cx, cy, cz);
        }
        for (int d0 = 0; d0 < D; d0 += GL) {
            const int d = d0 + lane;
            float sum = 0.f, cnt = 0.f;
            if (interior) {
                const float depth = d < D ? bins[d] : 1.0f;
                for (int l = 0; l < L; ++l) {
                    if (s_skip[l]) continue;
                    float P[12];
#pragma unroll
                    for (int i = 0; i < 12; ++i) P[i] = s_P[l][i];
                    float ix, iy;
                    sample_pos(P, cx, cy, cz, depth, wm1, hm1, ix, iy);
                    if (d >= D) ix = -1.0f;
                    const float* __restrict__ lk = look + ((int64_t)b * L + l) * HW * CH + 4 * lane;
                    float p[GL];
#pragma unroll
                    for (int j = 0; j < GL; ++j) {
                        const float x = __shfl(ix, j, GL), y = __shfl(iy, j, GL);
                        p[j] = 0.f;
                        if (x >= 0.f) {
                            const float x0f = floorf(x), y0f = floorf(y);
                            const float wx1 = x - x0f, wx0 = (x0f + 1.0f) - x, wy1 = y - y0f, wy0 = (y0f + 1.0f) - y;
                            const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
                            const int x0 = min(max((int)x0f, 0), W - 2), y0 = min(max((int)y0f, 0), H - 2);
                            const float* __restrict__ t0 = lk + ((int64_t)y0 * W + x0) * CH;
                            const float4 a = *reinterpret_cast<const float4*>(t0);
                            const float4 e = *reinterpret_cast<const float4*>(t0 + CH);
                            const float4 f = *reinterpret_cast<const float4*>(t0 + (int64_t)W * CH);
                            const float4 g = *reinterpret_cast<const float4*>(t0 + (int64_t)W * CH + CH);
                            const float vx = a.x * nw + e.x * ne + f.x * sw + g.x * se;
                            const float vy = a.y * nw + e.y * ne + f.y * sw + g.y * se;
                            const float vz = a.z * nw + e.z * ne + f.z * sw + g.z * se;
                            const float vw = a.w * nw + e.w * ne + f.w * sw + g.w * se;
                            p[j] = (fabsf(vx - c4.x) + fabsf(vy - c4.y)) + (fabsf(vz - c4.z) + fabsf(vw - c4.w));
                        }
                    }
                    // halving exchange: after the four steps p[0] of lane j is the sum over the 16 lanes of their p[j]
#pragma unroll
                    for (int s = GL / 2; s >= 1; s >>= 1) {
                        const bool up = (lane & s) != 0;
#pragma unroll
                        for (int i = 0; i < GL / 2; ++i)
                            if (i < s) {
                                const float send = up ? p[i] : p[i + s], keep = up ? p[i + s] : p[i];
                                p[i] = keep + __shfl_xor(send, s, GL);
                            }
                    }
                    const float diff = p[0] * (1.0f / CH);              // mean over the channels (times the edge flag, 1 here)
                    sum += diff;
                    cnt += diff > 0.f ? 1.0f : 0.f;
                }
            }
            if (d < D) s_cost[px * DP + d] = sum / (cnt + 1e-7f);
        }
    }
    __syncthreads();

    // per pixel: maximum over the bins, confidence, argmin (zeros read as 100; the first minimum wins)
    for (int pp = 0; pp < TILE / (NT / GL); ++pp) {
        const int px = grp + pp * (NT / GL), w = w0 + px;
        if (w >= W) continue;
        float mx = 0.f;         // costs are >= 0
        int pos = 0;
        for (int d = lane; d < D; d += GL) {
            const float c = s_cost[px * DP + d];
            mx = fmaxf(mx, c);
            pos += c > 0.f;
        }
#pragma unroll
        for (int s = GL / 2; s >= 1; s >>= 1) {
            mx = fmaxf(mx, __shfl_xor(mx, s, GL));
            pos += __shfl_xor(pos, s, GL);
        }
        float best = 3.0e38f;
        int bi = MAX_D;
        for (int d = lane; d < D; d += GL) {
            const float c = s_cost[px * DP + d];
            const float f = (c == 0.f && set_max) ? mx : c;
            const float v = f == 0.f ? 100.0f : f;
            if (v < best) {
                best = v;
                bi = d;
            }
        }
#pragma unroll
        for (int s = GL / 2; s >= 1; s >>= 1) {
            const float ob = __shfl_xor(best, s, GL);
            const int oi = __shfl_xor(bi, s, GL);
            if (ob < best || (ob == best && oi < bi)) {
                best = ob;
                bi = oi;
            }
        }
        if (lane == 0) {
            const float conf = pos == D ? 1.0f : 0.f;
            s_max[px] = mx;
            s_conf[px] = conf;
            const int64_t o = ((int64_t)b * H + h) * W + w;
            confidence[o] = conf;
            argmin[o] = bi;
        }
    }
    __syncthreads();

    for (int i = threadIdx.x; i < D * TILE; i += NT) {
        const int d = i / TILE, px = i - d * TILE, w = w0 + px;
        if (w >= W) continue;
        const float c = s_cost[px * DP + d];
        const bool m = c == 0.f;
        const float f = (m && set_max) ? s_max[px] : c;
        const int64_t o = (((int64_t)b * D + d) * H + h) * W + w;
        if (cost_volume) cost_volume[o] = f;
        if (missing) missing[o] = m ? 1.0f : 0.f;
        if (buffer) buffer[(((int64_t)b * (CH + D) + CH + d) * H + h) * W + w] = f * s_conf[px];
    }
}

}  // namespace

extern "C" {

int dmh_cost_volume_fwd(const float* current, const float* lookup, const float* poses, const float* K, const float* invK,
                        const float* bins, int B, int L, int Bp, int C, int H, int W, int D, int set_missing_to_max, int banded,
                        float* nhwc, float* cost_volume, float* missing, float* confidence, int32_t* argmin, float* buffer,
                        void* stream) {
    DMH_REQUIRE(current && lookup && poses && K && invK && bins && nhwc && confidence && argmin, "null pointer");
    DMH_REQUIRE(B > 0 && L > 0 && L <= MAX_L, "need B > 0 and 1 <= L <= 16");
    DMH_REQUIRE(Bp >= 1 && Bp <= B, "need 1 <= Bp <= B (rows of poses)");
    DMH_REQUIRE(C == CH, "need C = 64 (the layer-1 width of ResNet-18/34)");
    DMH_REQUIRE(D >= 1 && D <= MAX_D, "need 1 <= D <= 128");
    DMH_REQUIRE(H >= 5 && W >= 5, "need H, W >= 5");
    DMH_REQUIRE((int64_t)H * W * CH < (1ll << 31), "need H * W * 64 < 2^31");
    const int64_t tiles = (int64_t)B * H * ((W + TILE - 1) / TILE);
    const int ttiles = (H * W + 63) / 64;
    DMH_REQUIRE(tiles < (1ll << 31) && (int64_t)B * L * ttiles < (1ll << 31), "need fewer than 2^31 tiles");
    hipLaunchKernelGGL(cost_volume_nhwc_kernel, dim3((unsigned)(B * L * ttiles)), dim3(NT), 0, (hipStream_t)stream, lookup, nhwc,
                       H * W, ttiles);
    hipLaunchKernelGGL(cost_volume_kernel, dim3((unsigned)tiles), dim3(NT), 0, (hipStream_t)stream, current, nhwc, poses, K, invK,
                       bins, B, L, Bp, H, W, D, set_missing_to_max ? 1 : 0, banded ? 1 : 0, cost_volume, missing, confidence,
                       argmin, buffer);
    return check_launch("dmh_cost_volume_fwd");
}

}  // extern "C"
