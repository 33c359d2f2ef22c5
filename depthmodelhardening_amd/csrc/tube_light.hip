// K24 -- tube-light object attack (a black-box random search): the lit object patch and the "keep the best" step on the
// device (gfx950).
//
// Replaces torchattacks/attacks/phy_obj_atk_light.py:130-138 with light_simulation.py:23-28,:124-163 (a Python double loop over
// the patch, an OpenCV add, a PIL uint8 round trip and an upload per query) and :165-167 (a host comparison per query).
// Nothing here is read by the host while the search runs:
//
//   table  double [n][DMH_LIGHT_REC]   one record per query, made on the host in float64 exactly as the reference's Python makes
//                                      these scalars: 0 k, 1 b, 2 beta, 3 full_end, 4 light_end, 5 sqrt(1 + k k), 6-8 c[i] alpha,
//                                      9 zero.
//   index  int32 [>= 1]                compose reads index[0]: the search's cursor, or the best query after the search.
//   state  int32 [2]                   0 cursor, 1 best query (starts -1).  commit finishes query state[0] and advances it.
//   best   float [1]                   best cost, starts 1e10 (:105).
//   cost   float [n]                   the cost of every query; after the search it is the attack's trace.
//
// compose follows the reference's chain bit for bit: the distance, the two comparisons, beta / (d d) and (c att) 255.0 in
// double with contraction off, every operation rounded on its own as CPython's float arithmetic rounds it; then round to fp32,
// add the uint8 base in fp32, clip, truncate (astype(uint8)) and divide by 255 in fp32 (ToTensor).  Both divisions are IEEE
// (hipcc's default for fp64, and -fhip-fp32-correctly-rounded-divide-sqrt, also the default, for fp32).
// commit is one thread: the only launch that touches state / best / cost, so its read-modify-write needs no ordering beyond
// the stream's.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int REC = DMH_LIGHT_REC;

struct LightRec {
    double k, b, beta, full, end, s, c[3];
};

__device__ __forceinline__ LightRec load_rec(const double* __restrict__ table, int q) {
    const double* r = table + (int64_t)q * REC;
    LightRec L;
    L.k = r[0]; L.b = r[1]; L.beta = r[2]; L.full = r[3]; L.end = r[4]; L.s = r[5];
    L.c[0] = r[6]; L.c[1] = r[7]; L.c[2] = r[8];
    return L;
}

// light_simulation.py:150-161 for one pixel: the attenuation the three channels share (0 outside the beam).
__device__ __forceinline__ double attenuation(const LightRec& L, int x, int y) {
#pragma clang fp contract(off)
    const double kx = L.k * (double)x;
    const double t = kx - (double)y;
    const double d = fabs(t + L.b) / L.s;
    const double far = L.beta / (d * d);        // read only where full < d <= end (d > 0 there)
    return d <= L.full ? 1.0 : (d <= L.end ? far : 0.0);
}

// (c alpha att) * 255.0 -> fp32; + base in fp32; clip; truncate; / 255 in fp32
__device__ __forceinline__ float lit_texel(double c, double att, unsigned base) {
#pragma clang fp contract(off)
    const double v = (c * att) * 255.0;
    const float sum = (float)base + (float)v;
    const float clipped = fminf(fmaxf(sum, 0.f), 255.f);
    return (float)(unsigned)clipped / 255.f;
}

// One thread = 4 neighbouring pixels of one row (W % 4 == 0, base 4-byte and out 16-byte aligned: host check).
__global__ __launch_bounds__(NT) void tube_light_compose_kernel(const double* __restrict__ table, const int32_t* __restrict__ index,
                                                                const uint8_t* __restrict__ base, float* __restrict__ out,
                                                                int n_queries, int H, int W) {
    const int q = index[0];
    if (q < 0 || q >= n_queries) return;    // outside the search: nothing to do, nothing to index
    const int w4 = W >> 2;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= H * w4) return;
    const int y = i / w4, x = (i - y * w4) << 2;
    const LightRec L = load_rec(table, q);
    double att[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) att[j] = attenuation(L, x + j, y);
    const int64_t hw = (int64_t)H * W, p = (int64_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t b = *reinterpret_cast<const uint32_t*>(base + c * hw + p);
        float4 r;
        r.x = lit_texel(L.c[c], att[0], b & 0xffu);
        r.y = lit_texel(L.c[c], att[1], (b >> 8) & 0xffu);
        r.z = lit_texel(L.c[c], att[2], (b >> 16) & 0xffu);
        r.w = lit_texel(L.c[c], att[3], b >> 24);
        *reinterpret_cast<float4*>(out + c * hw + p) = r;
    }
}

// Any W, any alignment: one thread = one pixel.
__global__ __launch_bounds__(NT) void tube_light_compose_scalar_kernel(const double* __restrict__ table,
                                                                       const int32_t* __restrict__ index,
                                                                       const uint8_t* __restrict__ base, float* __restrict__ out,
                                                                       int n_queries, int H, int W) {
    const int q = index[0];
    if (q < 0 || q >= n_queries) return;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const LightRec L = load_rec(table, q);
    const double att = attenuation(L, x, y);
    const int64_t hw = (int64_t)H * W;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c * hw + i] = lit_texel(L.c[c], att, base[c * hw + i]);
}

// phy_obj_atk_light.py:165-167 on the device: strictly smaller wins, so the first of equal costs stays (a NaN never wins).
__global__ __launch_bounds__(WAVE) void tube_light_commit_kernel(const float* __restrict__ cost_in, float* cost, float* best,
                                                                 int32_t* state, int n_queries) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int q = state[0];
    if (q < 0 || q >= n_queries) return;
    const float c = cost_in[0];
    cost[q] = c;
    if (c < best[0]) {
        best[0] = c;
        state[1] = q;
    }
    state[0] = q + 1;
}

}  // namespace

extern "C" {

int dmh_tube_light_compose(const double* table, const int32_t* index, const uint8_t* base, float* out, int n_queries, int H,
                           int W, void* stream) {
    DMH_REQUIRE(table && index && base && out, "null pointer");
    DMH_REQUIRE(n_queries > 0 && H > 0 && W > 0 && (int64_t)H * W < (1 << 28), "need n_queries > 0 and 0 < H * W < 2^28");
    DMH_REQUIRE(((uintptr_t)table & 7) == 0 && ((uintptr_t)index & 3) == 0, "table must be 8-byte, index 4-byte aligned");
    const bool wide = (W & 3) == 0 && ((uintptr_t)base & 3) == 0 && ((uintptr_t)out & 15) == 0;
    if (wide) {
        const int work = H * (W >> 2);
        hipLaunchKernelGGL(tube_light_compose_kernel, dim3((work + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, table, index,
                           base, out, n_queries, H, W);
    } else {
        const int work = H * W;
        hipLaunchKernelGGL(tube_light_compose_scalar_kernel, dim3((work + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, table,
                           index, base, out, n_queries, H, W);
    }
    return check_launch("dmh_tube_light_compose");
}

int dmh_tube_light_commit(const float* cost_in, float* cost, float* best, int32_t* state, int n_queries, void* stream) {
    DMH_REQUIRE(cost_in && cost && best && state, "null pointer");
    DMH_REQUIRE(n_queries > 0, "need n_queries > 0");
    DMH_REQUIRE(cost_in != cost && cost_in != best, "cost_in must not alias cost or best");
    hipLaunchKernelGGL(tube_light_commit_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, cost_in, cost, best, state,
                       n_queries);
    return check_launch("dmh_tube_light_commit");
}

}  // extern "C"
