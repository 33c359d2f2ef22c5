// K34 -- DepthHints' fused hint selection (depth-hints/precompute_depth_hints.py:151,247-252) and the loader's side of a stored
// hint (depth-hints/datasets/mono_dataset.py:382-388), for a batch of stereo pairs (gfx950).
//
// The reference warps the other view once per candidate depth map (BackprojectDepth, Project3D, F.grid_sample with its defaults:
// bilinear, align_corners=False, padding_mode='border'), takes 0.85 mean_c(SSIM) + 0.15 mean_c|base - sample| against the base
// image, the argmin over the N candidates per pixel and gathers the depth: about 60 launches over [12, 3, H, W] intermediates
// per image.  Here it is one launch for the batch.
//
// hint_fuse_kernel: one workgroup of 256 threads per 8 x 32 tile of one item, one pixel per thread.
//   once per tile   byte / 255 for the 256 byte values into LDS (the IEEE quotient, computed once instead of per tap); P = K T;
//                   the base image's 10 x 34 halo tile (ReflectionPad2d(1)) into LDS; per thread the base's window sums
//                   mu_y = pool(y), pool(y^2) of the three channels, kept in registers.
//   per candidate   every halo pixel: depth (from the raw int16 disparity or read as float), back-projection, projection, the
//                   border-clamped bilinear sample of the three channels -> LDS (3 planes + the depth); barrier; every thread:
//                   pool(x), pool(x^2), pool(x y) over its 3 x 3 window in avg_pool2d's order, SSIM, L1, the loss; the running
//                   minimum and its depth stay in registers (strict <: the lowest index wins among equal losses).
// Separate IEEE operations in the reference's order, never contracted (the pragma below); the quotients are correctly rounded.
// A halo pixel that reflects is warped at the pixel it reflects to, as padding the warped image does.  A coordinate is clamped
// to [0, size - 1] as a float (fmaxf / fminf: a NaN becomes 0) before it is converted to an integer: an invalid candidate
// (depth 0) projects to about +-6e8.  No atomics, no workspace, no host read: bitwise reproducible, capturable.
//
// hint_prepare_kernel: np.fliplr, then OpenCV's INTER_NEAREST to (W, H) through host-made index tables, and the mask (hint > 0).
#include "common.hpp"

#pragma clang fp contract(off)

using namespace dmh;

namespace {

constexpr int TH = 8, TW = 32, NT = TH * TW;
constexpr int HH = TH + 2, HW = TW + 2, HALO = HH * HW;

struct Cam {
    float ik[9];    // inv_K[:3, :3]
    float P[12];    // (K T)[:3, :]
};

// depth-hints/precompute_depth_hints.py:142,151: disp = raw / 16 (exact), fx 0.1 / (disp + 1e-7) * (disp > 0), float32 throughout
__device__ __forceinline__ float depth_of_raw(int raw, float fx01) {
    const float disp = (float)raw * 0.0625f;
    const float q = __fdiv_rn(fx01, disp + 1e-7f);
    return q * (disp > 0.f ? 1.f : 0.f);
}

template <bool RAW>
__device__ __forceinline__ float cand_depth(const void* __restrict__ cand, int64_t i, float fx01) {
    if (RAW) return depth_of_raw((int)((const int16_t*)cand)[i], fx01);
    return ((const float*)cand)[i];
}

// the pixel's sample position in the other view, un-normalised and border-clamped (grid_sample, align_corners=False)
__device__ __forceinline__ void project(const Cam& c, int x, int y, float d, int H, int W, float& ix, float& iy) {
    const float fx = (float)x, fy = (float)y;
    const float X = d * (c.ik[0] * fx + c.ik[1] * fy + c.ik[2]);
    const float Y = d * (c.ik[3] * fx + c.ik[4] * fy + c.ik[5]);
    const float Z = d * (c.ik[6] * fx + c.ik[7] * fy + c.ik[8]);
    const float u = c.P[0] * X + c.P[1] * Y + c.P[2] * Z + c.P[3];
    const float v = c.P[4] * X + c.P[5] * Y + c.P[6] * Z + c.P[7];
    const float w = (c.P[8] * X + c.P[9] * Y + c.P[10] * Z + c.P[11]) + 1e-7f;
    float gx = __fdiv_rn(__fdiv_rn(u, w), (float)(W - 1));
    float gy = __fdiv_rn(__fdiv_rn(v, w), (float)(H - 1));
    gx = (gx - 0.5f) * 2.f;
    gy = (gy - 0.5f) * 2.f;
    ix = (gx + 1.f) * ((float)W * 0.5f) - 0.5f;      // ATen's CPU form of ((g + 1) size - 1) / 2
    iy = (gy + 1.f) * ((float)H * 0.5f) - 0.5f;
    ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
    iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
}

__device__ __forceinline__ float pool9(const float* __restrict__ s, int o) {
    float a = s[o];
    a += s[o + 1];
    a += s[o + 2];
    a += s[o + HW];
    a += s[o + HW + 1];
    a += s[o + HW + 2];
    a += s[o + 2 * HW];
    a += s[o + 2 * HW + 1];
    a += s[o + 2 * HW + 2];
    return a;
}

template <bool RAW>
__global__ __launch_bounds__(NT) void hint_fuse_kernel(const uint8_t* __restrict__ base, const uint8_t* __restrict__ lookup,
                                                       const void* __restrict__ cand, const float* __restrict__ Kmat,
                                                       const float* __restrict__ inv_K, const float* __restrict__ Tmat, int N, int H,
                                                       int W, float* __restrict__ best_depth, float* __restrict__ losses) {
    __shared__ float s_lut[256];
    __shared__ float s_base[3][HALO];
    __shared__ float s_warp[3][HALO];
    __shared__ float s_depth[HALO];
    __shared__ Cam s_cam;

    const int tid = threadIdx.x, tx = tid % TW, ty = tid / TW;
    const int b = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t plane = (int64_t)H * W;
    const uint8_t* bimg = base + (int64_t)b * 3 * plane;
    const uint8_t* limg = lookup + (int64_t)b * 3 * plane;

    s_lut[tid] = __fdiv_rn((float)tid, 255.f);
    if (tid < 9) s_cam.ik[tid] = inv_K[b * 16 + (tid / 3) * 4 + tid % 3];
    if (tid >= 64 && tid < 76) {
        const int r = (tid - 64) / 4, c = (tid - 64) % 4;
        const float* Kb = Kmat + b * 16 + r * 4;
        const float* Tb = Tmat + b * 16 + c;
        s_cam.P[r * 4 + c] = Kb[0] * Tb[0] + Kb[1] * Tb[4] + Kb[2] * Tb[8] + Kb[3] * Tb[12];
    }
    __syncthreads();
    for (int h = tid; h < HALO; h += NT) {
        const int ry = reflect_idx(y0 + h / HW - 1, H), rx = reflect_idx(x0 + h % HW - 1, W);
        const int64_t o = (int64_t)ry * W + rx;
#pragma unroll
        for (int c = 0; c < 3; ++c) s_base[c][h] = s_lut[bimg[c * plane + o]];
    }
    __syncthreads();

    const int x = x0 + tx, y = y0 + ty;
    const bool inside = x < W && y < H;
    const int o = ty * HW + tx, oc = o + HW + 1;      // the window's corner and its centre in the halo tile
    float yc[3], mu_y[3], syy[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* s = s_base[c];
        yc[c] = s[oc];
        mu_y[c] = __fdiv_rn(pool9(s, o), 9.f);
        float a = s[o] * s[o];
        a += s[o + 1] * s[o + 1];
        a += s[o + 2] * s[o + 2];
        a += s[o + HW] * s[o + HW];
        a += s[o + HW + 1] * s[o + HW + 1];
        a += s[o + HW + 2] * s[o + HW + 2];
        a += s[o + 2 * HW] * s[o + 2 * HW];
        a += s[o + 2 * HW + 1] * s[o + 2 * HW + 1];
        a += s[o + 2 * HW + 2] * s[o + 2 * HW + 2];
        syy[c] = __fdiv_rn(a, 9.f);
    }
    const Cam cam = s_cam;
    const float fx01 = Kmat[b * 16] * 0.1f;
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);

    float best = 0.f, best_d = 0.f;
    for (int n = 0; n < N; ++n) {
        const int64_t cbase = ((int64_t)b * N + n) * plane;
        for (int h = tid; h < HALO; h += NT) {
            const int ry = reflect_idx(y0 + h / HW - 1, H), rx = reflect_idx(x0 + h % HW - 1, W);
            const float d = cand_depth<RAW>(cand, cbase + (int64_t)ry * W + rx, fx01);
            float ix, iy;
            project(cam, rx, ry, d, H, W, ix, iy);
            const float fx0 = floorf(ix), fy0 = floorf(iy);
            const int xa = min(max((int)fx0, 0), W - 1), ya = min(max((int)fy0, 0), H - 1);    // already inside: clamped as floats above
            const int xb = min(xa + 1, W - 1), yb = min(ya + 1, H - 1);    // weight 0 where the neighbour leaves the image
            const float wx1 = ix - fx0, wx0 = 1.f - wx1, wy1 = iy - fy0, wy0 = 1.f - wy1;
            const float nw = wy0 * wx0, ne = wy0 * wx1, sw = wy1 * wx0, se = wy1 * wx1;
            const int64_t o00 = (int64_t)ya * W + xa, o01 = (int64_t)ya * W + xb, o10 = (int64_t)yb * W + xa, o11 = (int64_t)yb * W + xb;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint8_t* p = limg + c * plane;
                s_warp[c][h] = s_lut[p[o00]] * nw + s_lut[p[o01]] * ne + s_lut[p[o10]] * sw + s_lut[p[o11]] * se;
            }
            s_depth[h] = d;
        }
        __syncthreads();
        float ssim_sum = 0.f, l1_sum = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float* sx = s_warp[c];
            const float* sy = s_base[c];
            const float mu_x = __fdiv_rn(pool9(sx, o), 9.f);
            float a = 0.f, m = 0.f;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const float xv = sx[o + dy * HW + dx];
                    if (dy == 0 && dx == 0) {
                        a = xv * xv;
                        m = xv * sy[o];
                    } else {
                        a += xv * xv;
                        m += xv * sy[o + dy * HW + dx];
                    }
                }
            const float sig_x = __fdiv_rn(a, 9.f) - mu_x * mu_x;
            const float sig_y = syy[c] - mu_y[c] * mu_y[c];
            const float sig_xy = __fdiv_rn(m, 9.f) - mu_x * mu_y[c];
            const float num = (2.f * mu_x * mu_y[c] + C1) * (2.f * sig_xy + C2);
            const float den = (mu_x * mu_x + mu_y[c] * mu_y[c] + C1) * (sig_x + sig_y + C2);
            const float v = (1.f - __fdiv_rn(num, den)) * 0.5f;
            const float cl = fminf(fmaxf(v, 0.f), 1.f);
            const float ad = fabsf(yc[c] - sx[oc]);
            if (c == 0) {
                ssim_sum = cl;
                l1_sum = ad;
            } else {
                ssim_sum += cl;
                l1_sum += ad;
            }
        }
        const float loss = 0.85f * __fdiv_rn(ssim_sum, 3.f) + 0.15f * __fdiv_rn(l1_sum, 3.f);
        const float d = s_depth[oc];
        if (n == 0 || loss < best) {
            best = loss;
            best_d = d;
        }
        if (losses != nullptr && inside) losses[cbase + (int64_t)y * W + x] = loss;
        __syncthreads();
    }
    if (inside) best_depth[(int64_t)b * plane + (int64_t)y * W + x] = best_d;
}

__global__ __launch_bounds__(256) void hint_prepare_kernel(const float* __restrict__ src, const int32_t* __restrict__ flip,
                                                           const int32_t* __restrict__ ytab, const int32_t* __restrict__ xtab, int B, int Hs,
                                                           int Ws, int H, int W, float* __restrict__ hint, float* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * H * W) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((int64_t)W * H));
    // a table entry outside the source is a host bug; it must not become an access out of bounds
    const int sy = min(max(ytab[y], 0), Hs - 1);
    int sx = min(max(xtab[x], 0), Ws - 1);
    if (flip != nullptr && flip[b] != 0) sx = Ws - 1 - sx;
    const float v = src[((int64_t)b * Hs + sy) * Ws + sx];
    hint[i] = v;
    mask[i] = v > 0.f ? 1.f : 0.f;
}

}  // namespace

extern "C" {

int dmh_depth_hint_fuse(const uint8_t* base, const uint8_t* lookup, const void* cand, int cand_is_raw, const float* K,
                        const float* inv_K, const float* T, int B, int N, int H, int W, float* best_depth, float* losses,
                        void* stream) {
    DMH_REQUIRE(base && lookup && cand && K && inv_K && T && best_depth, "null pointer");
    DMH_REQUIRE(N >= 1 && N <= DMH_HINT_MAX_CANDIDATES, "need 1 <= N <= 16 candidates");
    DMH_REQUIRE(B >= 1 && B <= 65535, "need 1 <= B <= 65535");
    DMH_REQUIRE(H >= 2 && W >= 2, "need H, W >= 2 (reflection padding, division by W - 1 and H - 1)");
    DMH_REQUIRE((int64_t)B * N * H * W < (1ll << 31) && (int64_t)B * 3 * H * W < (1ll << 31), "B N H W and B 3 H W must stay below 2^31");
    DMH_REQUIRE((H + TH - 1) / TH <= 65535, "H must fit 65535 tile rows");
    DMH_REQUIRE(cand_is_raw == 0 || cand_is_raw == 1, "cand_is_raw must be 0 (float32 depths) or 1 (int16 disparity x 16)");
    DMH_REQUIRE(((uintptr_t)cand & (cand_is_raw ? 1 : 3)) == 0, "cand must be aligned to its element (2 bytes raw, 4 bytes float)");
    DMH_REQUIRE(((uintptr_t)K & 3) == 0 && ((uintptr_t)inv_K & 3) == 0 && ((uintptr_t)T & 3) == 0 && ((uintptr_t)best_depth & 3) == 0
                    && ((uintptr_t)losses & 3) == 0, "K, inv_K, T, best_depth and losses must be 4-byte aligned");
    DMH_REQUIRE((const void*)best_depth != cand && (const void*)losses != cand && (const void*)losses != (const void*)best_depth,
                "best_depth and losses must not alias cand or each other");
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, B);
    if (cand_is_raw)
        hipLaunchKernelGGL(hint_fuse_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, base, lookup, cand, K, inv_K, T, N, H, W,
                           best_depth, losses);
    else
        hipLaunchKernelGGL(hint_fuse_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, base, lookup, cand, K, inv_K, T, N, H, W,
                           best_depth, losses);
    return check_launch("dmh_depth_hint_fuse");
}

int dmh_depth_hint_prepare(const float* src, const int32_t* flip, const int32_t* ytab, const int32_t* xtab, int64_t ytab_len,
                           int64_t xtab_len, int B, int Hs, int Ws, int H, int W, float* hint, float* mask, void* stream) {
    DMH_REQUIRE(src && ytab && xtab && hint && mask, "null pointer");
    DMH_REQUIRE(B >= 1 && Hs >= 1 && Ws >= 1 && H >= 1 && W >= 1, "need B, Hs, Ws, H, W >= 1");
    DMH_REQUIRE(ytab_len == H && xtab_len == W, "the index tables must hold H and W entries");
    DMH_REQUIRE((int64_t)B * H * W < (1ll << 31) - 256 && (int64_t)B * Hs * Ws < (1ll << 31), "B H W and B Hs Ws must stay below 2^31");
    DMH_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)flip & 3) == 0 && ((uintptr_t)ytab & 3) == 0 && ((uintptr_t)xtab & 3) == 0
                    && ((uintptr_t)hint & 3) == 0 && ((uintptr_t)mask & 3) == 0, "every pointer must be 4-byte aligned");
    DMH_REQUIRE(hint != mask && (const float*)hint != src && (const float*)mask != src, "hint, mask and src must not alias");
    const int64_t total = (int64_t)B * H * W;
    hipLaunchKernelGGL(hint_prepare_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, flip, ytab,
                       xtab, B, Hs, Ws, H, W, hint, mask);
    return check_launch("dmh_depth_hint_prepare");
}

}  // extern "C"
