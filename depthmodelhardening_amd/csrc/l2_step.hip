// K28 -- one L2 PGD step on a flat fp32 tensor, in two launches, with no host read and no float atomics (gfx950).
//
// Replaces torchattacks/attacks/phy_obj_atk_l2.py:110-120 in its shared-patch form (one norm over the whole tensor):
//
//   y   = x + alpha g / (||g||_2 + 1e-10)
//   d   = y - x0
//   out = clamp(x0 + d min(eps / ||d||_2, 1), 0, 1)
//
// about a dozen element-wise and reduction launches of the reference.
//
// Launch 1 (l2_partials_kernel): workgroup b writes three doubles, ws[3 b + {0, 1, 2}] = its share of sum(g g), sum((x - x0) g)
// and sum((x - x0)^2).  The products of two fp32 values are exact in double; the sums are taken in a fixed order (thread-serial,
// then the shuffle tree of block_sum_d), so a partial depends on nothing but its inputs.
//
// Launch 2 (l2_apply_kernel): every workgroup adds the partials in index order -- three lanes, one per sum -- so every workgroup
// holds the same bits and no second reduction launch, atomic or grid barrier is needed.  Then, in double,
//
//   s       = alpha / (sqrt(sum g g) + 1e-10)
//   ||d||^2 = sum((x - x0)^2) + 2 s sum((x - x0) g) + s^2 sum(g g)         (d = (x - x0) + s g, expanded: no third launch)
//   f       = ||d|| > eps ? eps / ||d|| : 1                                   (eps / 0 = inf -> 1, as torch.min(inf, 1))
//
// and element-wise out = clamp(x0 + ((x - x0) + s g) f, 0, 1), evaluated in double and rounded to fp32 once: the element-wise part
// is bound by its four memory streams, not by the ~6 double operations per element.
//
// The two launches differ in their grids: the partial grid is capped at L2_MAX_PARTS workgroups (229 at the workload's
// n = 234,000: one 16-byte load per thread and tensor), so that the serial sum of launch 2 stays short.
#include "common.hpp"

#include <math.h>

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int L2_MAX_PARTS = 256;       // partial workgroups of launch 1 = doubles x 3 in the workspace
constexpr int APPLY_MAX_BLOCKS = 2048;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
    return v;
}

// common.hpp's block_sum for doubles; result valid in thread 0.  Fixed order -> bitwise reproducible.
__device__ __forceinline__ double block_sum_d(double v, double* red) {
    v = wave_sum_d(v);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NT / WAVE; ++i) t += red[i];
    }
    return t;
}

__device__ __forceinline__ void acc1(float x, float x0, float g, double& gg, double& dg, double& dd) {
    const double d = (double)x - (double)x0, gd = (double)g;
    gg += gd * gd;
    dg += d * gd;
    dd += d * d;
}

__global__ __launch_bounds__(NT) void l2_partials_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                                         const float* __restrict__ g, int64_t n, int vec_ok,
                                                         double* __restrict__ ws) {
    __shared__ double red[NT / WAVE];
    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    double gg = 0.0, dg = 0.0, dd = 0.0;
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        const float4* y4 = reinterpret_cast<const float4*>(x0);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        for (int64_t j = i; j < n4; j += stride) {
            const float4 a = x4[j], b = y4[j], c = g4[j];
            acc1(a.x, b.x, c.x, gg, dg, dd);
            acc1(a.y, b.y, c.y, gg, dg, dd);
            acc1(a.z, b.z, c.z, gg, dg, dd);
            acc1(a.w, b.w, c.w, gg, dg, dd);
        }
        for (int64_t j = (n4 << 2) + i; j < n; j += stride) acc1(x[j], x0[j], g[j], gg, dg, dd);
    } else {
        for (int64_t j = i; j < n; j += stride) acc1(x[j], x0[j], g[j], gg, dg, dd);
    }
    const double t0 = block_sum_d(gg, red);
    const double t1 = block_sum_d(dg, red);
    const double t2 = block_sum_d(dd, red);
    if (threadIdx.x == 0) {
        ws[3 * blockIdx.x + 0] = t0;
        ws[3 * blockIdx.x + 1] = t1;
        ws[3 * blockIdx.x + 2] = t2;
    }
}

__device__ __forceinline__ float apply1(float x, float x0, float g, double s, double f) {
    const double o = (double)x0, d = ((double)x - o) + s * (double)g;
    return (float)fmin(fmax(o + d * f, 0.0), 1.0);
}

__global__ __launch_bounds__(NT) void l2_apply_kernel(const float* __restrict__ x, const float* __restrict__ x0,
                                                      const float* __restrict__ g, double alpha, double eps,
                                                      const double* __restrict__ ws, int parts, float* __restrict__ out,
                                                      int64_t n, int vec_ok) {
    __shared__ double tot[3];
    if (threadIdx.x < 3) {
        double t = 0.0;
        for (int b = 0; b < parts; ++b) t += ws[3 * b + threadIdx.x];      // index order: the same bits in every workgroup
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    const double gg = tot[0], dg = tot[1], dd = tot[2];
    const double s = alpha / (sqrt(gg) + 1e-10);
    const double d2 = dd + 2.0 * s * dg + s * s * gg;
    const double dn = sqrt(fmax(d2, 0.0));
    const double f = dn > eps ? eps / dn : 1.0;

    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        const float4* x4 = reinterpret_cast<const float4*>(x);
        const float4* y4 = reinterpret_cast<const float4*>(x0);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        float4* o4 = reinterpret_cast<float4*>(out);
        for (int64_t j = i; j < n4; j += stride) {
            const float4 a = x4[j], b = y4[j], c = g4[j];
            float4 r;
            r.x = apply1(a.x, b.x, c.x, s, f);
            r.y = apply1(a.y, b.y, c.y, s, f);
            r.z = apply1(a.z, b.z, c.z, s, f);
            r.w = apply1(a.w, b.w, c.w, s, f);
            o4[j] = r;
        }
        for (int64_t j = (n4 << 2) + i; j < n; j += stride) out[j] = apply1(x[j], x0[j], g[j], s, f);
    } else {
        for (int64_t j = i; j < n; j += stride) out[j] = apply1(x[j], x0[j], g[j], s, f);
    }
}

inline int parts_for(int64_t work) {
    const int64_t b = (work + NT - 1) / NT;
    return (int)(b < 1 ? 1 : (b > L2_MAX_PARTS ? L2_MAX_PARTS : b));
}

}  // namespace

extern "C" {

// bytes of the partials: three doubles per workgroup of launch 1 (the scalar form's count, which the 16-byte form never exceeds)
int64_t dmh_pgd_l2_workspace_size(int64_t n) { return n > 0 ? (int64_t)(3 * sizeof(double)) * parts_for(n) : 0; }

int dmh_pgd_l2_step(const float* x, const float* x0, const float* g, double alpha, double eps, float* out, int64_t n,
                    void* workspace, int64_t workspace_bytes, void* stream) {
    DMH_REQUIRE(x && x0 && g && out && workspace && n > 0, "null pointer or n <= 0");
    DMH_REQUIRE(eps >= 0.0, "eps must not be negative");
    DMH_REQUIRE(out != x && out != x0 && out != g, "out must be a buffer of its own");
    DMH_REQUIRE(((uintptr_t)workspace & 7) == 0 && workspace_bytes >= dmh_pgd_l2_workspace_size(n),
                "workspace must be 8-byte aligned and hold dmh_pgd_l2_workspace_size(n) bytes");
    const uintptr_t al = (uintptr_t)x | (uintptr_t)x0 | (uintptr_t)g | (uintptr_t)out;
    const int vec_ok = (al & 15) == 0;
    const int64_t work = vec_ok ? (n + 3) / 4 : n;
    const int parts = parts_for(work);
    const int64_t ab = (work + NT - 1) / NT;
    const int apply_blocks = (int)(ab < 1 ? 1 : (ab > APPLY_MAX_BLOCKS ? APPLY_MAX_BLOCKS : ab));
    double* ws = static_cast<double*>(workspace);
    hipLaunchKernelGGL(l2_partials_kernel, dim3(parts), dim3(NT), 0, (hipStream_t)stream, x, x0, g, n, vec_ok, ws);
    hipLaunchKernelGGL(l2_apply_kernel, dim3(apply_blocks), dim3(NT), 0, (hipStream_t)stream, x, x0, g, alpha, eps, ws,
                       parts, out, n, vec_ok);
    return check_launch("dmh_pgd_l2_step");
}

}  // extern "C"
