// K37 -- a batch of float maps (disparities) to magma-coloured bytes on the device (gfx950): the tail of MD2/test_simple.py:136-156
// and of the figures of my_utils.py:43-105.
//
// The reference does, per image on the host: a D2H copy, np.percentile(., 95) (a partition), matplotlib's Normalize and
// ScalarMappable (float64 temporaries), * 255, astype(uint8).  Here a call covers P panels in a fixed chain of launches
// (one memset, source, 3 x scan, 2 x histogram, colour), nothing is read by the host between them, there are no float atomics and
// two runs give the same bits.
//
//   source   per panel the float map [H, W] that the later stages read: src[a], or |src[a] - src[b]|, as it is (H, W == h, w: the
//            input bits) or resized with F.interpolate(mode="bilinear", align_corners=False) arithmetic in ONE expression order,
//            never contracted.  Fused: the panel's min and max (integer atomicMax on the order-preserving key and on its
//            complement) and pass 0 of the radix select.
//   select   K25's scheme (eigen_eval.hip): the two order statistics lo, hi by a most-significant-digit radix select on the key of
//            the float bits, 11 / 11 / 10 bits, LDS integer atomics per workgroup, the non-empty bins added to global memory with
//            integer atomics, one workgroup per panel walks the bins.  The key orders -0.0 before +0.0 and negative values by
//            value: the selected elements have the values of numpy's sort at those ranks.  After the last pass
//            p = a_lo + d g, or a_hi - d (1 - g) when g >= 0.5, d = a_hi - a_lo (numpy's _lerp, float32, no fma).
//   colour   x = 0 when vmin == vmax, (a - vmin) / (vmax - vmin) otherwise (the IEEE quotient); xa = 256 x; index 0 where xa < 0,
//            255 where xa >= 256, trunc(xa) otherwise; three table bytes at out + origin + y pitch + 3 x.  vmin, vmax come from the
//            statistics on the device by the panel's mode.  The 256 x 3 table is staged in LDS.
// lo, hi and g are numpy's own virtual index of n = H W, computed on the host (ops.percentile_plan) and passed as arguments.
// Every index a kernel uses derives from values the entry point checked on the host; the panels travel as a kernel argument.
#include "common.hpp"

#pragma clang fp contract(off)

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int CHUNK = 4096;                     // pixels of one panel per workgroup
constexpr int BINS = 2048;
constexpr int PASSES = 3;
constexpr int WS_IMG = PASSES * 2 * BINS;       // histogram words per panel
constexpr int ST = 8;                           // state words per panel: 0 prefix lo, 1 prefix hi, 2 rank lo, 3 rank hi,
                                                // 4 max of ~key (the minimum), 5 max of key
constexpr int NSTAT = DMH_COLORIZE_STATS;

struct Panels {
    dmh_colorize_panel p[DMH_COLORIZE_MAX_PANELS];
};

__device__ __forceinline__ uint32_t float_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

// one tap of the source stage: the map, or the absolute difference of two maps
__device__ __forceinline__ float tap(const float* __restrict__ a, const float* __restrict__ b, int i) {
    return b ? fabsf(a[i] - b[i]) : a[i];
}

// area_pixel_compute_source_index (align_corners=False): src = scale (dst + 0.5) - 0.5, negative -> 0; the second tap is clamped
__device__ __forceinline__ void lin_axis(int d, float scale, int size, int& i0, int& i1, float& l0, float& l1) {
    float s = scale * ((float)d + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    int i = (int)s;
    i = i > size - 1 ? size - 1 : i;
    i0 = i;
    i1 = i + (i < size - 1 ? 1 : 0);
    l1 = s - (float)i;
    l0 = 1.f - l1;
}

// ------------------------------------------------------------------------------------------------------------------ source
template <bool RESIZE>
__global__ __launch_bounds__(NT) void colorize_source_kernel(const float* __restrict__ src, int h, int w, int H, int W, Panels pn,
                                                             float sy, float sx, float* __restrict__ map, uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_hist[BINS];
    __shared__ uint32_t s_mm[2];
    const int p = blockIdx.y, P = gridDim.y;
    const dmh_colorize_panel r = pn.p[p];
    const int n = H * W;
    const float* a = src + (int64_t)r.a * h * w;
    const float* b = r.b >= 0 ? src + (int64_t)r.b * h * w : nullptr;
    float* out = map + (int64_t)p * n;
    for (int i = threadIdx.x; i < BINS; i += NT) s_hist[i] = 0u;
    if (threadIdx.x < 2) s_mm[threadIdx.x] = 0u;
    __syncthreads();
    const int p0 = (int)blockIdx.x * CHUNK, p1 = p0 + CHUNK < n ? p0 + CHUNK : n;
    uint32_t kmin = 0xffffffffu, kmax = 0u;
    for (int i = p0 + (int)threadIdx.x; i < p1; i += NT) {
        float v;
        if (RESIZE) {
            const int y = i / W, x = i - y * W;
            int y0, y1, x0, x1;
            float hl0, hl1, wl0, wl1;
            lin_axis(y, sy, h, y0, y1, hl0, hl1);
            lin_axis(x, sx, w, x0, x1, wl0, wl1);
            v = hl0 * (wl0 * tap(a, b, y0 * w + x0) + wl1 * tap(a, b, y0 * w + x1))
              + hl1 * (wl0 * tap(a, b, y1 * w + x0) + wl1 * tap(a, b, y1 * w + x1));
        } else {
            v = tap(a, b, i);
        }
        out[i] = v;
        const uint32_t key = float_key(v);
        kmin = key < kmin ? key : kmin;
        kmax = key > kmax ? key : kmax;
        atomicAdd(&s_hist[key >> 21], 1u);
    }
    atomicMax(&s_mm[0], ~kmin);
    atomicMax(&s_mm[1], kmax);
    __syncthreads();
    uint32_t* g = ws + (int64_t)p * WS_IMG;
    for (int i = threadIdx.x; i < BINS; i += NT) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&g[i], c);
    }
    if (threadIdx.x < 2 && p0 < p1) atomicMax(&ws[(int64_t)P * WS_IMG + p * ST + 4 + threadIdx.x], s_mm[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------------------------ select
// passes 1 and 2: the values under each rank's prefix
__global__ __launch_bounds__(NT) void colorize_hist_kernel(const float* __restrict__ map, int n, int pass, uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_hist[2 * BINS];
    const int p = blockIdx.y, P = gridDim.y;
    const uint32_t* st = ws + (int64_t)P * WS_IMG + p * ST;
    const uint32_t pre_lo = st[0], pre_hi = st[1];
    for (int i = threadIdx.x; i < 2 * BINS; i += NT) s_hist[i] = 0u;
    __syncthreads();
    const float* m = map + (int64_t)p * n;
    const int p0 = (int)blockIdx.x * CHUNK, p1 = p0 + CHUNK < n ? p0 + CHUNK : n;
    for (int i = p0 + (int)threadIdx.x; i < p1; i += NT) {
        const uint32_t key = float_key(m[i]);
        const uint32_t pre = pass == 1 ? key >> 21 : key >> 10;
        const uint32_t d = pass == 1 ? (key >> 10) & 0x7ffu : key & 0x3ffu;
        if (pre == pre_lo) atomicAdd(&s_hist[d], 1u);
        if (pre == pre_hi) atomicAdd(&s_hist[BINS + d], 1u);
    }
    __syncthreads();
    uint32_t* g = ws + ((int64_t)p * PASSES + pass) * 2 * BINS;
    for (int i = threadIdx.x; i < 2 * BINS; i += NT) {
        const uint32_t c = s_hist[i];
        if (c) atomicAdd(&g[i], c);
    }
}

// One workgroup per panel: the bin each of the two ranks falls into, the new prefixes and the ranks inside the bin.  After the
// last pass the prefixes are the two keys: stats = min, max, a_lo, a_hi, the percentile.
__global__ __launch_bounds__(NT) void colorize_scan_kernel(uint32_t* __restrict__ ws, int pass, int lo, int hi, float g,
                                                           float* __restrict__ stats) {
    __shared__ uint32_t s_sum[2][NT];
    const int p = blockIdx.x, P = gridDim.x;
    uint32_t* st = ws + (int64_t)P * WS_IMG + p * ST;
    const uint32_t* hist = ws + ((int64_t)p * PASSES + pass) * 2 * BINS;
    constexpr int PER = BINS / NT;
    for (int k = 0; k < 2; ++k) {
        const uint32_t* hh = hist + (pass == 0 ? 0 : k * BINS);
        uint32_t s = 0u;
        for (int i = 0; i < PER; ++i) s += hh[threadIdx.x * PER + i];
        s_sum[k][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (pass == 0) {
        st[0] = st[1] = 0u;
        st[2] = (uint32_t)lo;
        st[3] = (uint32_t)hi;
    }
    const int bits = pass == 2 ? 10 : 11;
    for (int k = 0; k < 2; ++k) {
        const uint32_t* hh = hist + (pass == 0 ? 0 : k * BINS);
        const uint32_t rank = st[2 + k];
        uint32_t cum = 0u;
        int i = 0;
        while (i < NT - 1 && cum + s_sum[k][i] <= rank) cum += s_sum[k][i++];
        int b = i * PER;
        while (b < i * PER + PER - 1 && cum + hh[b] <= rank) cum += hh[b++];
        st[k] = (st[k] << bits) | (uint32_t)b;
        st[2 + k] = rank - cum;
    }
    if (pass == PASSES - 1) {
        const float a_lo = key_float(st[0]), a_hi = key_float(st[1]);
        const float d = a_hi - a_lo;
        float q = a_lo + d * g;
        if (g >= 0.5f) q = a_hi - d * (1.f - g);
        float* o = stats + (int64_t)p * NSTAT;
        o[0] = key_float(~st[4]);
        o[1] = key_float(st[5]);
        o[2] = a_lo;
        o[3] = a_hi;
        o[4] = q;
    }
}

// ------------------------------------------------------------------------------------------------------------------ colour
__device__ __forceinline__ int color_index(float a, float vmin, float den, bool flat) {
    const float x = flat ? 0.f : __fdiv_rn(a - vmin, den);
    const float xa = x * 256.f;
    return xa < 0.f ? 0 : (xa >= 256.f ? 255 : (int)xa);
}

// One thread per 4 pixels of a row: three 32-bit stores where the 12 bytes are 4-byte aligned, byte stores otherwise.
__global__ __launch_bounds__(NT) void colorize_color_kernel(const float* __restrict__ map, int H, int W, Panels pn,
                                                            const float* __restrict__ stats, const uint8_t* __restrict__ table,
                                                            uint8_t* __restrict__ out, int64_t pitch) {
    __shared__ uint8_t s_tab[768];
    const int p = blockIdx.y;
    const dmh_colorize_panel r = pn.p[p];
    for (int i = threadIdx.x; i < 768; i += NT) s_tab[i] = table[i];
    __syncthreads();
    // every candidate is loaded and the limits are selected.  Not an if / else-if / else on the mode word: hipcc -O3 compiled
    // that form into a path that read vmax from the statistics' base for DMH_COLORIZE_MIN_MAX (tests/test_gpu_colorize.py).
    const float* own = stats + (int64_t)p * NSTAT;
    const int ref = r.mode == DMH_COLORIZE_ZERO_REF ? r.ref : p;
    const float own_min = own[0], own_max = own[1], own_q = own[4], ref_q = stats[(int64_t)ref * NSTAT + 4];
    const float vmin = r.mode == DMH_COLORIZE_ZERO_REF ? 0.f : own_min;
    const float vmax = r.mode == DMH_COLORIZE_MIN_P95 ? own_q : (r.mode == DMH_COLORIZE_ZERO_REF ? ref_q : own_max);
    const bool flat = vmin == vmax;
    const float den = vmax - vmin;
    const int gw = (W + 3) / 4;
    const int gid = (int)blockIdx.x * NT + (int)threadIdx.x;
    if (gid >= H * gw) return;
    const int y = gid / gw, x0 = (gid - y * gw) * 4;
    const int cnt = W - x0 < 4 ? W - x0 : 4;
    const float* m = map + (int64_t)p * H * W + (int64_t)y * W + x0;
    uint8_t* o = out + r.origin + (int64_t)y * pitch + (int64_t)x0 * 3;
    uint8_t px[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int idx = k < cnt ? color_index(m[k], vmin, den, flat) : 0;
        px[3 * k + 0] = s_tab[3 * idx + 0];
        px[3 * k + 1] = s_tab[3 * idx + 1];
        px[3 * k + 2] = s_tab[3 * idx + 2];
    }
    if (cnt == 4 && ((uintptr_t)o & 3u) == 0) {
        uint32_t* o4 = (uint32_t*)o;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            o4[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * cnt; ++k) o[k] = px[k];
    }
}

}  // namespace

extern "C" {

int64_t dmh_disp_colorize_ws_size(int n_panels) {
    return n_panels > 0 && n_panels <= DMH_COLORIZE_MAX_PANELS ? (int64_t)n_panels * (WS_IMG + ST) : -1;
}

int dmh_disp_colorize(const float* src, int n_src, int h, int w, const dmh_colorize_panel* panels, int n_panels, int H, int W,
                      int lo, int hi, float g, const uint8_t* table, float* map, uint32_t* ws, float* stats, uint8_t* out,
                      int64_t out_len, int64_t pitch, void* stream) {
    DMH_REQUIRE(src && panels && table && map && ws && stats && out, "null pointer");
    DMH_REQUIRE(n_src >= 1 && h >= 1 && w >= 1 && (int64_t)n_src * h * w < ((int64_t)1 << 31), "need B, h, w >= 1 and B h w < 2^31");
    DMH_REQUIRE(n_panels >= 1 && n_panels <= DMH_COLORIZE_MAX_PANELS, "1 <= panels <= DMH_COLORIZE_MAX_PANELS");
    DMH_REQUIRE(H >= 1 && W >= 1 && (int64_t)n_panels * H * W < ((int64_t)1 << 31), "need H, W >= 1 and panels H W < 2^31");
    const int n = H * W;
    DMH_REQUIRE(lo >= 0 && lo <= hi && hi < n && hi - lo <= 1, "the ranks must be 0 <= lo <= hi <= lo + 1 < H W");
    DMH_REQUIRE(g >= 0.f && g < 1.f, "the weight g must lie in [0, 1)");
    DMH_REQUIRE(((uintptr_t)src | (uintptr_t)map | (uintptr_t)ws | (uintptr_t)stats) % 4 == 0, "src, map, ws and stats must be 4-byte aligned");
    DMH_REQUIRE(pitch >= (int64_t)3 * W && out_len > 0, "the output pitch must hold a row of 3 W bytes");
    // a panel spans (H - 1) pitch + 3 W bytes from its origin (stated without a product that could overflow)
    const bool fits = out_len >= (int64_t)3 * W && (int64_t)(H - 1) <= (out_len - (int64_t)3 * W) / pitch;
    const int64_t span = fits ? (int64_t)(H - 1) * pitch + (int64_t)3 * W : 0;
    Panels pn;
    memset(&pn, 0, sizeof(pn));
    for (int i = 0; i < n_panels; ++i) {
        const dmh_colorize_panel& r = panels[i];
        DMH_REQUIRE(r.a >= 0 && r.a < n_src && r.b >= -1 && r.b < n_src, "a panel's maps a, b must lie in the batch (b = -1: none)");
        DMH_REQUIRE(r.mode == DMH_COLORIZE_MIN_P95 || r.mode == DMH_COLORIZE_ZERO_REF || r.mode == DMH_COLORIZE_MIN_MAX, "bad mode word");
        DMH_REQUIRE(r.mode != DMH_COLORIZE_ZERO_REF || (r.ref >= 0 && r.ref < n_panels), "a limit record names a panel outside the batch");
        DMH_REQUIRE(fits && r.origin >= 0 && r.origin <= out_len - span, "a panel must lie inside the output buffer");
        pn.p[i] = r;
    }
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)dmh_disp_colorize_ws_size(n_panels) * sizeof(uint32_t), s) != hipSuccess)
        return check_launch("dmh_disp_colorize");
    const dim3 grid((n + CHUNK - 1) / CHUNK, n_panels);
    if (H == h && W == w) {
        hipLaunchKernelGGL(colorize_source_kernel<false>, grid, dim3(NT), 0, s, src, h, w, H, W, pn, 1.f, 1.f, map, ws);
    } else {
        const float sy = (float)h / (float)H, sx = (float)w / (float)W;
        hipLaunchKernelGGL(colorize_source_kernel<true>, grid, dim3(NT), 0, s, src, h, w, H, W, pn, sy, sx, map, ws);
    }
    for (int pass = 0; pass < PASSES; ++pass) {
        if (pass > 0) hipLaunchKernelGGL(colorize_hist_kernel, grid, dim3(NT), 0, s, (const float*)map, n, pass, ws);
        hipLaunchKernelGGL(colorize_scan_kernel, dim3(n_panels), dim3(NT), 0, s, ws, pass, lo, hi, g, stats);
    }
    const int groups = H * ((W + 3) / 4);
    hipLaunchKernelGGL(colorize_color_kernel, dim3((groups + NT - 1) / NT, n_panels), dim3(NT), 0, s, (const float*)map, H, W, pn,
                       (const float*)stats, table, out, pitch);
    return check_launch("dmh_disp_colorize");
}

}  // extern "C"
