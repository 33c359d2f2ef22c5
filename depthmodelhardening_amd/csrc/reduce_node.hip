// K36 -- the element-wise and reduction passes of ManyDepth's degenerate reduce_conv as one autograd node.
//
// Reference: manydepth2/networks/resnet_encoder.py:124-129,321 -- reduce_conv = Conv2d(64 + D, 64, 3, 1, 1) + ReLU over
// cat([features, cost_volume], 1).  The reference's trainer and wrapper call the encoder with lookup_images * 0 and a zero pose
// (manydepth2/trainer.py:371-385, depth_model.py:42-58): the D cost-volume channels are then exact zeros, and the layer is
//
//     y = relu(conv3x3(x, weight[:, :C]) + bias)
//
// with weight.grad[:, C:] == 0.  The convolutions are the existing launches (K10 forward / backward-data, K18 weight gradient);
// this file holds what is left:
//
//   bias_relu  : y = relu(z + bias[k])                 forward, behind a convolution that has no fused epilogue for the shape
//   bwd_mask   : g_pre = g * [y > 0]  and  part[k][s] = sum of g_pre over slab s of channel k (all images)
//   bwd_finish : g_bias[k] = sum_s part[k][s] (index order), g_weight[K][C+D][3][3] = (dw[K][C][3][3] | 0)
//
// No atomics, no host read; every sum has a fixed order, so two runs give the same bits.  Wave64, plain (vector-memory) stores.
//
// fp32 roundings on the longest path of one bias-gradient sum (dmh_reduce_bwd_rounds returns the same number):
//   HW % 4 == 0:  n = B * ceil(HW / (S * 1024))   one of a thread's four accumulators, one addition per (image, slab step)
//                   + 2                            (a0 + a1) + (a2 + a3)
//                   + 6                            wave64 butterfly (__shfl_down 32 .. 1)
//                   + 3                            the four waves of the block, added in order by thread 0 (block_sum)
//                   + 1                            the S partials are added in float64 and rounded to fp32 once
//   otherwise:    n = B * ceil(HW / (S * 256)) + 6 + 3 + 1      (one accumulator per thread)
// with S = min(64, ceil(HW / 1024)) slabs per channel.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;

inline int slabs_per_channel(int HW) {
    int64_t S = ((int64_t)HW + 4 * NT - 1) / (4 * NT);
    return (int)(S > 64 ? 64 : S);
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + NT - 1) / NT); }

template <bool VEC>
__global__ __launch_bounds__(NT) void bias_relu_kernel(const float* z, const float* __restrict__ bias, unsigned K, unsigned hw,
                                                       unsigned total, float* y) {
    // VEC: hw and total count float4s.  y may be z (in place): every thread reads its element before it writes it
    const unsigned i = blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const float b = bias[(i / hw) % K];
    if (VEC) {
        const float4 v = reinterpret_cast<const float4*>(z)[i];
        float4 r;
        r.x = v.x + b > 0.f ? v.x + b : 0.f;
        r.y = v.y + b > 0.f ? v.y + b : 0.f;
        r.z = v.z + b > 0.f ? v.z + b : 0.f;
        r.w = v.w + b > 0.f ? v.w + b : 0.f;
        reinterpret_cast<float4*>(y)[i] = r;
    } else {
        const float v = z[i] + b;
        y[i] = v > 0.f ? v : 0.f;
    }
}

// grid (S, K): block (s, k) walks slab steps s, s + S, ... of channel k in every image
template <bool VEC>
__global__ __launch_bounds__(NT) void bwd_mask_kernel(const float* __restrict__ g, const float* __restrict__ y, int B, int K, int HW,
                                                      int S, float* __restrict__ g_pre, float* __restrict__ part) {
    const int k = blockIdx.y, s = blockIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int b = 0; b < B; ++b) {
        const size_t base = ((size_t)b * K + k) * (size_t)HW;
        if (VEC) {
            for (int r = (s * NT + (int)threadIdx.x) * 4; r < HW; r += S * NT * 4) {      // HW % 4 == 0: r + 3 < HW
                const float4 gv = *reinterpret_cast<const float4*>(g + base + r);
                const float4 yv = *reinterpret_cast<const float4*>(y + base + r);
                const float4 p = make_float4(yv.x > 0.f ? gv.x : 0.f, yv.y > 0.f ? gv.y : 0.f, yv.z > 0.f ? gv.z : 0.f,
                                             yv.w > 0.f ? gv.w : 0.f);
                *reinterpret_cast<float4*>(g_pre + base + r) = p;
                a0 += p.x; a1 += p.y; a2 += p.z; a3 += p.w;
            }
        } else {
            for (int r = s * NT + (int)threadIdx.x; r < HW; r += S * NT) {
                const float p = y[base + r] > 0.f ? g[base + r] : 0.f;
                g_pre[base + r] = p;
                a0 += p;
            }
        }
    }
    __shared__ float red[NT / WAVE];
    const float u = block_sum<NT>(VEC ? (a0 + a1) + (a2 + a3) : a0, red);      // wave butterfly, then the four waves in order
    if (threadIdx.x == 0) part[(size_t)k * S + s] = u;
}

// threads [0, K * (C + D) * 9): one element of g_weight each; threads [that, + K): one bias gradient each
__global__ __launch_bounds__(NT) void bwd_finish_kernel(const float* __restrict__ part, const float* __restrict__ dw, int C, int K,
                                                        int D, int S, float* __restrict__ g_bias, float* __restrict__ g_weight) {
    const unsigned i = blockIdx.x * NT + threadIdx.x;
    const unsigned row = (unsigned)(C + D) * 9u, nw = (unsigned)K * row;
    if (i < nw) {
        const unsigned k = i / row, rem = i - k * row;
        g_weight[i] = rem < (unsigned)C * 9u ? dw[(size_t)k * C * 9 + rem] : 0.f;
    } else if (i < nw + (unsigned)K) {
        const unsigned k = i - nw;
        double t = 0.0;
        for (int s = 0; s < S; ++s) t += (double)part[(size_t)k * S + s];
        g_bias[k] = (float)t;
    }
}

// null pointers aside, what every entry point of this file refuses
inline const char* bad_sizes(int B, int C, int K, int HW) {
    if (B <= 0 || C <= 0 || K <= 0 || HW <= 0) return "sizes must be positive";
    if (C % 8) return "C must be a multiple of 8";
    if (K % 8) return "K must be a multiple of 8";
    if (K > 65535) return "K beyond the grid's second dimension";
    const int64_t m = (int64_t)B * (C > K ? C : K) * HW;
    if (m >= ((int64_t)1 << 31)) return "tensor beyond the 32-bit index range";
    return nullptr;
}

inline int fail_sizes(const char* fn, const char* why) {
    snprintf(g_err, sizeof(g_err), "%s: requirement failed: %s", fn, why);
    return DMH_EINVAL;
}

#define DMH_REDUCE_SIZES(B, C, K, HW)                          \
    do {                                                       \
        const char* why_ = bad_sizes(B, C, K, HW);             \
        if (why_) return fail_sizes(__func__, why_);           \
    } while (0)

}  // namespace

extern "C" {

int dmh_reduce_bias_relu(const float* z, const float* bias, int B, int C, int K, int HW, float* y, void* stream) {
    DMH_REQUIRE(z && bias && y, "null pointer");
    DMH_REDUCE_SIZES(B, C, K, HW);
    const int64_t total = (int64_t)B * K * HW;
    hipStream_t st = (hipStream_t)stream;
    if ((HW & 3) == 0 && ((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(y)) & 15) == 0)
        hipLaunchKernelGGL(bias_relu_kernel<true>, dim3(blocks_of(total / 4)), dim3(NT), 0, st, z, bias, (unsigned)K,
                           (unsigned)(HW / 4), (unsigned)(total / 4), y);
    else
        hipLaunchKernelGGL(bias_relu_kernel<false>, dim3(blocks_of(total)), dim3(NT), 0, st, z, bias, (unsigned)K, (unsigned)HW,
                           (unsigned)total, y);
    return check_launch("dmh_reduce_bias_relu");
}

int64_t dmh_reduce_bwd_partials_size(int B, int C, int K, int HW) {
    if (const char* why = bad_sizes(B, C, K, HW)) return fail_sizes(__func__, why), -1;
    return (int64_t)K * slabs_per_channel(HW);
}

int dmh_reduce_bwd_rounds(int B, int C, int K, int HW) {
    if (const char* why = bad_sizes(B, C, K, HW)) return fail_sizes(__func__, why), -1;
    const int64_t S = slabs_per_channel(HW);
    if ((HW & 3) == 0) return (int)(B * ((HW + S * NT * 4 - 1) / (S * NT * 4)) + 2 + 6 + 3 + 1);
    return (int)(B * ((HW + S * NT - 1) / (S * NT)) + 6 + 3 + 1);
}

int dmh_reduce_bwd_mask(const float* g, const float* y, int B, int C, int K, int HW, float* g_pre, float* partials, void* stream) {
    DMH_REQUIRE(g && y && g_pre && partials, "null pointer");
    DMH_REDUCE_SIZES(B, C, K, HW);
    const int S = slabs_per_channel(HW);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (HW & 3) == 0;     // (the rounding count goes by HW alone, so a misaligned plane is refused, not rerouted)
    DMH_REQUIRE(!vec || ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(g_pre)) & 15) == 0,
                "g, y and g_pre must be 16-byte aligned");
    if (vec) hipLaunchKernelGGL(bwd_mask_kernel<true>, dim3((unsigned)S, (unsigned)K), dim3(NT), 0, st, g, y, B, K, HW, S, g_pre, partials);
    else hipLaunchKernelGGL(bwd_mask_kernel<false>, dim3((unsigned)S, (unsigned)K), dim3(NT), 0, st, g, y, B, K, HW, S, g_pre, partials);
    return check_launch("dmh_reduce_bwd_mask");
}

int dmh_reduce_bwd_finish(const float* partials, const float* dw, int B, int C, int K, int D, int HW, float* g_bias,
                          float* g_weight, void* stream) {
    DMH_REQUIRE(partials && dw && g_bias && g_weight, "null pointer");
    DMH_REDUCE_SIZES(B, C, K, HW);
    DMH_REQUIRE(D >= 0 && (int64_t)K * ((int64_t)C + D) * 9 + K < ((int64_t)1 << 31), "weight beyond the 32-bit index range");
    const int64_t total = (int64_t)K * ((int64_t)C + D) * 9 + K;
    hipLaunchKernelGGL(bwd_finish_kernel, dim3(blocks_of(total)), dim3(NT), 0, (hipStream_t)stream, partials, dw, C, K, D,
                       slabs_per_channel(HW), g_bias, g_weight);
    return check_launch("dmh_reduce_bwd_finish");
}

}  // extern "C"
