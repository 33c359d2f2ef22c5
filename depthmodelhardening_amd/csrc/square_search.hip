// K27 -- Square attack (L_inf) on the object patch, the one black-box attack of the evaluation whose candidate depends on the
// model's earlier answers: "absorb the previous decision" and "make the next candidate" in one launch (gfx950).
//
// Replaces torchattacks/attacks/phy_obj_atk_square.py:259-260 (the start stripes), :284-291 (the candidate: a zero tensor, a
// slice write, an add, a max, a min, a clamp) and :312-313 (x_best <- idx_improved x_new + (1 - idx_improved) x_best, after a
// host comparison).  Nothing here is read by the host while the search runs:
//
//   table    int32 [n][3 + C]   one row per query, made on the host from the CPU generator's draws: vh, vw, s, sign_0 ..
//                               sign_{C-1}.  Row 0 is not read: query 0 is the stripes.
//   stripes  float [C][W]       +-1, the start point of :259-260.
//   state    int32 [2]          K24's: 0 the cursor q, 1 the best query.  Only read here; K24's commit advances it.
//
// Query q - 1 was accepted iff K24's commit made it the best: state[1] == q - 1.  Every thread reads that one word and then
// touches only its own elements of x_best and x_new, so there is nothing to order between workgroups, and a second patch-sized
// launch (or a conditional copy) per query is never needed.  q == n is the absorb-only call after the last query.
//
// Arithmetic: one rounded fp32 add / max / min per step in the reference's order, contraction off (apgd_ops.hip says why), which
// makes the result bit-equal to the element-wise torch expression.  There is no product to contract but eps * stripe and
// 2 eps * sign, both exact.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;

struct Query {
    int q, n, vh, vw, s;
    bool accept;
};

// the wave-uniform part: cursor, decision, the square of row q
__device__ __forceinline__ Query load_query(const int32_t* __restrict__ table, const int32_t* __restrict__ state, int n, int C) {
    Query Q;
    Q.q = state[0];
    Q.n = n;
    Q.accept = Q.q > 0 && Q.q <= n && state[1] == Q.q - 1;
    Q.vh = Q.vw = Q.s = 0;
    if (Q.q > 0 && Q.q < n) {
        const int32_t* r = table + (int64_t)Q.q * (3 + C);
        Q.vh = r[0]; Q.vw = r[1]; Q.s = r[2];
    }
    return Q;
}

// is there anything to do?  (outside [0, n]: nothing; q == n: only after an accepted last query)
__device__ __forceinline__ bool idle(const Query& Q) { return Q.q < 0 || Q.q > Q.n || (Q.q == Q.n && !Q.accept); }

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// :259-260 for one texel
__device__ __forceinline__ float stripe1(float x0, float stripe, float eps) {
#pragma clang fp contract(off)
    const float d = eps * stripe;
    return clampf(x0 + d, 0.f, 1.f);
}

// :288-291 for one texel inside the square
__device__ __forceinline__ float square1(float xb, float x0, float d, float eps) {
#pragma clang fp contract(off)
    const float lo = x0 - eps, hi = x0 + eps;
    const float v = xb + d;
    return clampf(fminf(fmaxf(v, lo), hi), 0.f, 1.f);
}

// One thread = 4 neighbouring texels of one row, all channels (W % 4 == 0, every pointer 16-byte aligned: host check).
__global__ __launch_bounds__(NT) void square_propose_kernel(const float* __restrict__ x0, float* x_best, float* x_new,
                                                            const int32_t* __restrict__ table, const float* __restrict__ stripes,
                                                            const int32_t* __restrict__ state, int n, int C, int H, int W,
                                                            float eps) {
    const Query Q = load_query(table, state, n, C);
    if (idle(Q)) return;
    const int w4 = W >> 2;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= H * w4) return;
    const int y = i / w4, x = (i - y * w4) << 2;
    const bool row_in = y >= Q.vh && y < Q.vh + Q.s;
    bool in[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) in[j] = row_in && x + j >= Q.vw && x + j < Q.vw + Q.s;
    const int64_t hw = (int64_t)H * W, p = (int64_t)y * W + x;
    const float two_eps = 2.f * eps;
    for (int c = 0; c < C; ++c) {
        float4* b4 = reinterpret_cast<float4*>(x_best + c * hw + p);
        float4* n4 = reinterpret_cast<float4*>(x_new + c * hw + p);
        float4 xb = *b4;
        if (Q.accept) {
            xb = *n4;
            *b4 = xb;
        }
        if (Q.q == Q.n) continue;       // absorb only
        const float4 o = *reinterpret_cast<const float4*>(x0 + c * hw + p);
        float4 r;
        if (Q.q == 0) {
            const float4 st = *reinterpret_cast<const float4*>(stripes + (int64_t)c * W + x);
            r.x = stripe1(o.x, st.x, eps);
            r.y = stripe1(o.y, st.y, eps);
            r.z = stripe1(o.z, st.z, eps);
            r.w = stripe1(o.w, st.w, eps);
        } else {
            const float d = two_eps * (float)table[(int64_t)Q.q * (3 + C) + 3 + c];
            r.x = in[0] ? square1(xb.x, o.x, d, eps) : xb.x;
            r.y = in[1] ? square1(xb.y, o.y, d, eps) : xb.y;
            r.z = in[2] ? square1(xb.z, o.z, d, eps) : xb.z;
            r.w = in[3] ? square1(xb.w, o.w, d, eps) : xb.w;
        }
        *n4 = r;
    }
}

// Any W, any alignment: one thread = one texel, all channels.
__global__ __launch_bounds__(NT) void square_propose_scalar_kernel(const float* __restrict__ x0, float* x_best, float* x_new,
                                                                   const int32_t* __restrict__ table,
                                                                   const float* __restrict__ stripes,
                                                                   const int32_t* __restrict__ state, int n, int C, int H, int W,
                                                                   float eps) {
    const Query Q = load_query(table, state, n, C);
    if (idle(Q)) return;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const bool in = y >= Q.vh && y < Q.vh + Q.s && x >= Q.vw && x < Q.vw + Q.s;
    const int64_t hw = (int64_t)H * W;
    const float two_eps = 2.f * eps;
    for (int c = 0; c < C; ++c) {
        const int64_t e = c * hw + i;
        float xb = x_best[e];
        if (Q.accept) {
            xb = x_new[e];
            x_best[e] = xb;
        }
        if (Q.q == Q.n) continue;
        float r;
        if (Q.q == 0) {
            r = stripe1(x0[e], stripes[(int64_t)c * W + x], eps);
        } else {
            const float d = two_eps * (float)table[(int64_t)Q.q * (3 + C) + 3 + c];
            r = in ? square1(xb, x0[e], d, eps) : xb;
        }
        x_new[e] = r;
    }
}

}  // namespace

extern "C" {

int dmh_square_propose(const float* x0, float* x_best, float* x_new, const int32_t* table, const float* stripes,
                       const int32_t* state, int n_queries, int C, int H, int W, float eps, void* stream) {
    DMH_REQUIRE(x0 && x_best && x_new && table && stripes && state, "null pointer");
    DMH_REQUIRE(n_queries > 0 && C > 0 && C <= 16 && H > 0 && W > 0 && (int64_t)H * W < (1 << 28),
                "need n_queries > 0, 0 < C <= 16 and 0 < H * W < 2^28");
    DMH_REQUIRE(eps >= 0.f, "eps must not be negative");
    DMH_REQUIRE(x0 != x_best && x0 != x_new && x_best != x_new, "x0, x_best and x_new must be three different buffers");
    DMH_REQUIRE(((uintptr_t)table & 3) == 0 && ((uintptr_t)state & 3) == 0, "table and state must be 4-byte aligned");
    const uintptr_t al = (uintptr_t)x0 | (uintptr_t)x_best | (uintptr_t)x_new | (uintptr_t)stripes;
    const bool wide = (W & 3) == 0 && (al & 15) == 0;
    if (wide) {
        const int work = H * (W >> 2);
        hipLaunchKernelGGL(square_propose_kernel, dim3((work + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, x0, x_best, x_new,
                           table, stripes, state, n_queries, C, H, W, eps);
    } else {
        const int work = H * W;
        hipLaunchKernelGGL(square_propose_scalar_kernel, dim3((work + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, x0, x_best,
                           x_new, table, stripes, state, n_queries, C, H, W, eps);
    }
    return check_launch("dmh_square_propose");
}

}  // extern "C"
