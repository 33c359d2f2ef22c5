// K29 -- the pose head: the tail of the pose decoder and transformation_from_parameters as one launch per direction (gfx950).
//
// Replaces, per source frame, MD2/networks/pose_decoder.py:47-52 (out.mean(3).mean(2), 0.01 *, view, two slices) and
// MD2/layers.py:28-103 (norm, division, sin / cos, nine element writes into a zero matrix, a translation matrix, a matmul and
// for negative frame ids a transpose and a negation): about 25 eager launches forward and twice as many in autograd's backward,
// all of them on six numbers per sample.
//
//   x            float [B][6 nf][h][w]     the last convolution's output; channel 6 f + c is component c of frame f
//   axisangle    float [B][nf][1][3]       scale * mean over h x w of components 0 .. 2
//   translation  float [B][nf][1][3]       scale * mean of components 3 .. 5
//   T            float [B][nf][4][4]       Trans(t) Rot(a), or Rot(a)^T Trans(-t) where bit f of invert_mask is set
//
// Forward: one workgroup per (sample, frame).  Every thread sums its stride of the six planes, the wave sums by shuffles, thread 0
// adds the waves in index order: a fixed order, no atomics, the same bits on every run.  The sums are carried in double (six
// numbers per workgroup: free), so the mean is the correctly rounded fp32 mean.  Thread 0 then forms the matrix in the
// reference's own operation order with contraction off, so that what differs from the reference's fp32 result is sqrtf, the
// division and sinf / cosf (the precise ones) alone.
//
// Backward: one workgroup per (sample, frame).  Every thread recomputes the rotation from the saved axis-angle and the six scalars
// d / d (scale * mean) from g_T (and g_axisangle / g_translation where given) -- redundantly, which costs less than a barrier --
// and the block writes g_x = scalar * scale / (h w) over its 6 h w contiguous floats.  At an axis-angle of exactly zero the gradient
// of the norm is 0, as torch's norm backward has it.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int MAX_NF = 32;      // one bit of invert_mask per frame

struct Rot {
    float n[3];         // axis = a / (angle + 1e-7)
    float angle, ca, sa, C;
    float R[3][3];
};

// MD2/layers.py:64-103 rot_from_axisangle, operation by operation
__device__ __forceinline__ void rot_from_axisangle(const float a[3], Rot& r) {
#pragma clang fp contract(off)
    r.angle = sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const float d = r.angle + 1e-7f;
    r.n[0] = a[0] / d;
    r.n[1] = a[1] / d;
    r.n[2] = a[2] / d;
    r.ca = cosf(r.angle);
    r.sa = sinf(r.angle);
    r.C = 1.0f - r.ca;
    const float x = r.n[0], y = r.n[1], z = r.n[2];
    const float xs = x * r.sa, ys = y * r.sa, zs = z * r.sa;
    const float xC = x * r.C, yC = y * r.C, zC = z * r.C;
    const float xyC = x * yC, yzC = y * zC, zxC = z * xC;
    r.R[0][0] = x * xC + r.ca;
    r.R[0][1] = xyC - zs;
    r.R[0][2] = zxC + ys;
    r.R[1][0] = xyC + zs;
    r.R[1][1] = y * yC + r.ca;
    r.R[1][2] = yzC - xs;
    r.R[2][0] = zxC - ys;
    r.R[2][1] = yzC + xs;
    r.R[2][2] = z * zC + r.ca;
}

__global__ __launch_bounds__(NT) void pose_head_fwd_kernel(const float* __restrict__ x, int nf, int hw, float scale,
                                                           unsigned invert_mask, float* __restrict__ axisangle,
                                                           float* __restrict__ translation, float* __restrict__ T) {
#pragma clang fp contract(off)
    const int f = blockIdx.x, b = blockIdx.y;
    const int64_t bf = (int64_t)b * nf + f;
    const float* __restrict__ src = x + bf * 6 * hw;
    double acc[6] = {0., 0., 0., 0., 0., 0.};
    for (int i = threadIdx.x; i < hw; i += NT) {
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] += (double)src[(int64_t)c * hw + i];
    }
    __shared__ double red[6][NT / WAVE];
    const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = acc[c];
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_down(s, o, WAVE);
        if (lane == 0) red[c][wv] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    float v[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double s = red[c][0];
#pragma unroll
        for (int i = 1; i < NT / WAVE; ++i) s += red[c][i];
        v[c] = scale * (float)(s / (double)hw);
    }
    Rot r;
    rot_from_axisangle(v, r);
    float* __restrict__ aa = axisangle + bf * 3;
    float* __restrict__ tr = translation + bf * 3;
    float* __restrict__ M = T + bf * 16;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        aa[c] = v[c];
        tr[c] = v[3 + c];
    }
    const bool inv = (invert_mask >> f) & 1u;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) M[4 * i + j] = inv ? r.R[j][i] : r.R[i][j];
        // Trans(t) Rot: the last column is t.  Rot^T Trans(-t): row i of Rot^T times -t, summed in index order (layers.py:34-41)
        const float t0 = -v[3], t1 = -v[4], t2 = -v[5];
        M[4 * i + 3] = inv ? (r.R[0][i] * t0 + r.R[1][i] * t1) + r.R[2][i] * t2 : v[3 + i];
    }
    M[12] = 0.f;
    M[13] = 0.f;
    M[14] = 0.f;
    M[15] = 1.f;
}

__global__ __launch_bounds__(NT) void pose_head_bwd_kernel(const float* __restrict__ g_T, const float* __restrict__ g_axisangle,
                                                           const float* __restrict__ g_translation,
                                                           const float* __restrict__ axisangle,
                                                           const float* __restrict__ translation, int nf, int hw, float scale,
                                                           unsigned invert_mask, float* __restrict__ g_x) {
#pragma clang fp contract(off)
    const int f = blockIdx.x, b = blockIdx.y;
    const int64_t bf = (int64_t)b * nf + f;
    const float a[3] = {axisangle[bf * 3], axisangle[bf * 3 + 1], axisangle[bf * 3 + 2]};
    const float t[3] = {translation[bf * 3], translation[bf * 3 + 1], translation[bf * 3 + 2]};
    Rot r;
    rot_from_axisangle(a, r);
    float gR[3][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    float gt[3] = {0.f, 0.f, 0.f};
    if (g_T != nullptr) {
        const float* __restrict__ G = g_T + bf * 16;
        if ((invert_mask >> f) & 1u) {
            // M[i][j] = R[j][i];  M[i][3] = -sum_k R[k][i] t[k]
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    gR[k][i] = G[4 * i + k] - G[4 * i + 3] * t[k];
                    s += G[4 * i + 3] * r.R[k][i];
                }
                gt[k] = -s;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) gR[i][j] = G[4 * i + j];
                gt[i] = G[4 * i + 3];
            }
        }
    }
    // R[i][j] = n_i n_j C + delta_ij ca + sa [n]_x
    const float ax[3] = {gR[2][1] - gR[1][2], gR[0][2] - gR[2][0], gR[1][0] - gR[0][1]};
    float gC = 0.f, gn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            s += (gR[k][j] + gR[j][k]) * r.n[j];
            gC += gR[k][j] * (r.n[k] * r.n[j]);
        }
        gn[k] = r.C * s + r.sa * ax[k];
    }
    const float g_ca = (gR[0][0] + gR[1][1] + gR[2][2]) - gC;
    const float g_sa = (r.n[0] * ax[0] + r.n[1] * ax[1]) + r.n[2] * ax[2];
    const float d = r.angle + 1e-7f;
    const float g_na = (gn[0] * a[0] + gn[1] * a[1]) + gn[2] * a[2];
    const float g_angle = (g_sa * r.ca - g_ca * r.sa) - g_na / (d * d);
    float s6[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float via_norm = r.angle > 0.f ? g_angle * (a[k] / r.angle) : 0.f;
        s6[k] = gn[k] / d + via_norm;
        s6[3 + k] = gt[k];
        if (g_axisangle != nullptr) s6[k] += g_axisangle[bf * 3 + k];
        if (g_translation != nullptr) s6[3 + k] += g_translation[bf * 3 + k];
    }
    const float k = scale / (float)hw;
#pragma unroll
    for (int c = 0; c < 6; ++c) s6[c] = s6[c] * k;
    float* __restrict__ dst = g_x + bf * 6 * hw;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        for (int i = threadIdx.x; i < hw; i += NT) dst[(int64_t)c * hw + i] = s6[c];
    }
}

int shapes_ok(const char* fn, int B, int nf, int h, int w, float scale) {
    if (!(B > 0 && nf > 0 && h > 0 && w > 0)) return fail(DMH_EINVAL, "%s: requirement failed: need B, nf, h, w > 0", fn);
    if (!(B <= 65535 && nf <= MAX_NF)) return fail(DMH_EINVAL, "%s: requirement failed: need B <= 65535 and nf <= 32", fn);
    if (!((int64_t)h * w < (1ll << 24))) return fail(DMH_EINVAL, "%s: requirement failed: need h * w < 2^24", fn);
    if (!(scale == scale && scale - scale == 0.f)) return fail(DMH_EINVAL, "%s: requirement failed: scale must be finite", fn);
    return DMH_OK;
}

}  // namespace

extern "C" {

int dmh_pose_head_fwd(const float* x, int B, int nf, int h, int w, float scale, uint32_t invert_mask, float* axisangle,
                      float* translation, float* T, void* stream) {
    DMH_REQUIRE(x && axisangle && translation && T, "null pointer");
    if (int rc = shapes_ok(__func__, B, nf, h, w, scale)) return rc;
    DMH_REQUIRE(nf == MAX_NF || (invert_mask >> nf) == 0, "invert_mask names a frame >= nf");
    hipLaunchKernelGGL(pose_head_fwd_kernel, dim3(nf, B), dim3(NT), 0, (hipStream_t)stream, x, nf, h * w, scale, invert_mask,
                       axisangle, translation, T);
    return check_launch("dmh_pose_head_fwd");
}

int dmh_pose_head_bwd(const float* g_T, const float* g_axisangle, const float* g_translation, const float* axisangle,
                      const float* translation, int B, int nf, int h, int w, float scale, uint32_t invert_mask, float* g_x,
                      void* stream) {
    DMH_REQUIRE(axisangle && translation && g_x, "null pointer");
    DMH_REQUIRE(g_T || g_axisangle || g_translation, "null pointer: no output gradient given");
    if (int rc = shapes_ok(__func__, B, nf, h, w, scale)) return rc;
    DMH_REQUIRE(nf == MAX_NF || (invert_mask >> nf) == 0, "invert_mask names a frame >= nf");
    hipLaunchKernelGGL(pose_head_bwd_kernel, dim3(nf, B), dim3(NT), 0, (hipStream_t)stream, g_T, g_axisangle, g_translation,
                       axisangle, translation, nf, h * w, scale, invert_mask, g_x);
    return check_launch("dmh_pose_head_bwd");
}

}  // extern "C"
