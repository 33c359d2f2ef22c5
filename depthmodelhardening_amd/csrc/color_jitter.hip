// K33 -- torchvision 0.8.2's ColorJitter on 8-bit PIL images (MD2/datasets/mono_dataset.py:344-348, :133, :144), Pillow's bytes,
// for a whole batch and all its keys in two launches (gfx950).
//
// The reference draws one transform per item and applies it, on the host, to the 8-bit level-0 image of every frame: the four
// operations in the drawn order, each ending in a byte.  What Pillow computes, as this file restates it (ops.pil_color_jitter_host
// is the same arithmetic in numpy, held to Pillow itself by tests/test_pil_jitter_ref.py):
//   L(r, g, b)          = (19595 r + 38470 g + 7471 b + 32768) >> 16                                  (convert("L"))
//   blend(deg, v, f)    = t = (float)deg + f * (float)(v - deg) in float32, product and sum rounded separately;
//                         (int)t for 0 <= f <= 1, otherwise 0 if t <= 0, 255 if t >= 255, (int)t between       (Image.blend)
//   brightness          = blend(0, v, f)
//   saturation          = blend(L, v, f) per channel
//   contrast            = blend(m, v, f), m = (int)((double)S / (double)(H W) + 0.5), S the sum of L over THIS image as the
//                         operations before the contrast left it
//   hue                 = RGB -> HSV bytes (Convert.c rgb2hsv: float32 quotients, the hue in double), H + shift modulo 256,
//                         HSV -> RGB bytes (hsv2rgb: double, C's round)
// The output is (float)byte / 255.f, K31's expression, and optionally the byte.
//
// Pass 1, jitter_lsum_kernel: for the images whose item has a contrast step, the operations before it per pixel, L, a sum over the
// wave and the workgroup, and one plain store of the workgroup's 32-bit sum into its own slot of the workspace.  Pass 2,
// jitter_apply_kernel: every workgroup adds the slots of its image (integer addition has no order: the sum is exact and the same
// in every run; 255 H W fits 32 bits, the launcher refuses larger images) and runs the whole chain per pixel.  No atomics and
// nothing to clear: every slot that is read was written by the pass before.  (A memset node in front of an atomic sum was tried
// first; replayed from a captured graph after other work it filled the sums with something else than zeros on this runtime.)
// An item with count 0 is only converted.  With H W a multiple of 4 (every width that is) and aligned pointers a thread takes four
// pixels: one 32-bit load per channel, one 16-byte float store and one 32-bit byte store per channel; otherwise one pixel.
// The records are read on the device: nothing here depends on their values, so a captured graph replays with new ones.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int MAX_BLOCKS = 2048;        // workgroups of one launch, about; the rest is a stride loop
enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };

struct Tensors {
    const uint8_t* src[DMH_JITTER_MAX_TENSORS];
    float* f32[DMH_JITTER_MAX_TENSORS];
    uint8_t* u8[DMH_JITTER_MAX_TENSORS];
};

struct Px {
    int r, g, b;
};

// rec: int32 [B][8] = count, the operation codes (one per byte, first in the low byte), the bits of the float32 brightness,
// contrast and saturation factors, the hue shift, 0, 0.  Whatever it holds, every result is a byte written inside the image.
struct Record {
    int count, shift;
    uint32_t ops;
    float f[3];
};

__device__ __forceinline__ Record load_record(const int32_t* __restrict__ rec, int item) {
    const int32_t* r = rec + (size_t)item * 8;
    Record o;
    o.count = min(max(r[0], 0), 4);
    o.ops = (uint32_t)r[1];
    o.f[0] = __int_as_float(r[2]);
    o.f[1] = __int_as_float(r[3]);
    o.f[2] = __int_as_float(r[4]);
    o.shift = r[5] & 255;
    return o;
}

// the position of the first contrast step, or -1
__device__ __forceinline__ int contrast_at(const Record rc) {
    for (int k = 0; k < rc.count; ++k)
        if (((rc.ops >> (8 * k)) & 255u) == OP_CONTRAST) return k;
    return -1;
}

__device__ __forceinline__ int lum(const Px p) { return (19595 * p.r + 38470 * p.g + 7471 * p.b + 32768) >> 16; }

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ int blend1(int deg, int v, float f, bool inside) {
#pragma clang fp contract(off)
    const float d = f * (float)(v - deg);
    const float t = (float)deg + d;
    if (inside) return clip8((int)t);       // t lies in [0, 255] already; the clip keeps a NaN factor a byte
    return t <= 0.f ? 0 : (t >= 255.f ? 255 : clip8((int)t));
}

__device__ __forceinline__ Px blend(int dr, int dg, int db, const Px p, float f) {
    const bool inside = f >= 0.f && f <= 1.f;
    Px o;
    o.r = blend1(dr, p.r, f, inside);
    o.g = blend1(dg, p.g, f, inside);
    o.b = blend1(db, p.b, f, inside);
    return o;
}

// C's round of a value in [0, 255.5), then CLIP8
__device__ __forceinline__ int round8(double v) { return clip8((int)round(v)); }

__device__ __forceinline__ Px hue(const Px p, int shift) {
#pragma clang fp contract(off)
    const int mx = max(p.r, max(p.g, p.b)), mn = min(p.r, min(p.g, p.b));
    int H = 0, S = 0;
    const int V = mx;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = cr / (float)mx;
        const float rc = (float)(mx - p.r) / cr, gc = (float)(mx - p.g) / cr, bc = (float)(mx - p.b) / cr;
        float h;
        if (p.r == mx) h = (float)((double)bc - (double)gc);
        else if (p.g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        const double x = (double)h / 6.0 + 1.0;               // in [5/6, 11/6]: fmod(x, 1.0) is x, or x - 1 (exact)
        const float hf = (float)(x >= 1.0 ? x - 1.0 : x);
        H = clip8((int)((double)hf * 255.0));
        S = clip8((int)((double)s * 255.0));
    }
    H = (H + shift) & 255;
    Px o;
    o.r = o.g = o.b = V;
    if (S != 0) {
        const double fs = (double)S / 255.0;
        const double x = (double)H * 6.0 / 255.0;
        const double fl = floor(x);
        const double fr = x - fl;
        const double v = (double)V;
        const int pp = round8(v * (1.0 - fs));
        const int q = round8(v * (1.0 - fs * fr));
        const int t = round8(v * (1.0 - fs * (1.0 - fr)));
        const int i = (int)fl % 6;                           // H <= 255: x <= 6
        o.r = (i == 0 || i == 5) ? V : (i == 1 ? q : (i == 4 ? t : pp));
        o.g = (i == 1 || i == 2) ? V : (i == 0 ? t : (i == 3 ? q : pp));
        o.b = (i == 3 || i == 4) ? V : (i == 2 ? t : (i == 5 ? q : pp));
    }
    return o;
}

// operations [first, last) of the record on one pixel; ``mean`` serves a contrast step among them
__device__ __forceinline__ Px chain(Px p, const Record rc, int first, int last, int mean) {
    for (int k = first; k < last; ++k) {
        const uint32_t op = (rc.ops >> (8 * k)) & 255u;       // the same in every lane of the workgroup
        if (op == OP_BRIGHTNESS) {
            p = blend(0, 0, 0, p, rc.f[0]);
        } else if (op == OP_CONTRAST) {
            p = blend(mean, mean, mean, p, rc.f[1]);
        } else if (op == OP_SATURATION) {
            const int l = lum(p);
            p = blend(l, l, l, p, rc.f[2]);
        } else if (op == OP_HUE) {
            p = hue(p, rc.shift);
        }
    }
    return p;
}

template <bool VEC>
__device__ __forceinline__ void load_px(const uint8_t* __restrict__ img, int hw, int p, Px (&px)[VEC ? 4 : 1]) {
    if constexpr (VEC) {
        const uint32_t r = *reinterpret_cast<const uint32_t*>(img + p), g = *reinterpret_cast<const uint32_t*>(img + hw + p),
                       b = *reinterpret_cast<const uint32_t*>(img + 2 * (size_t)hw + p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            px[j].r = (r >> (8 * j)) & 255u;
            px[j].g = (g >> (8 * j)) & 255u;
            px[j].b = (b >> (8 * j)) & 255u;
        }
    } else {
        px[0].r = img[p];
        px[0].g = img[hw + p];
        px[0].b = img[2 * (size_t)hw + p];
    }
}

// grid (workgroups per image, T B); image y = tensor y / B, item y % B
template <bool VEC>
__global__ __launch_bounds__(NT) void jitter_lsum_kernel(const Tensors ts, int B, int hw, const int32_t* __restrict__ rec,
                                                         uint32_t* __restrict__ ws) {
    constexpr int PER = VEC ? 4 : 1;
    const int image = blockIdx.y, t = image / B, item = image - t * B;
    const Record rc = load_record(rec, item);
    const int at = contrast_at(rc);
    if (at < 0) return;                                        // the whole workgroup
    const uint8_t* img = ts.src[t] + (size_t)item * 3 * hw;
    uint32_t acc = 0;
    for (int p = (blockIdx.x * NT + threadIdx.x) * PER; p < hw; p += gridDim.x * NT * PER) {
        Px px[PER];
        load_px<VEC>(img, hw, p, px);
#pragma unroll
        for (int j = 0; j < PER; ++j) acc += (uint32_t)lum(chain(px[j], rc, 0, at, 0));
    }
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, WAVE);
    __shared__ uint32_t red[NT / WAVE];
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t total = 0;
#pragma unroll
        for (int i = 0; i < NT / WAVE; ++i) total += red[i];
        ws[(size_t)image * gridDim.x + blockIdx.x] = total;
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void jitter_apply_kernel(const Tensors ts, int B, int hw, const int32_t* __restrict__ rec,
                                                          const uint32_t* __restrict__ ws, int with_u8) {
    constexpr int PER = VEC ? 4 : 1;
    const int image = blockIdx.y, t = image / B, item = image - t * B;
    const Record rc = load_record(rec, item);
    int mean = 0;
    if (ws != nullptr && contrast_at(rc) >= 0) {               // the whole workgroup: the slots of the first pass's workgroups
        uint32_t acc = 0;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += NT) acc += ws[(size_t)image * gridDim.x + i];
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) acc += __shfl_down(acc, o, WAVE);
        __shared__ uint32_t red[NT / WAVE];
        if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = acc;
        __syncthreads();
        uint32_t total = 0;
#pragma unroll
        for (int i = 0; i < NT / WAVE; ++i) total += red[i];
        mean = (int)((double)total / (double)hw + 0.5);
    }
    const size_t base = (size_t)item * 3 * hw;
    const uint8_t* img = ts.src[t] + base;
    float* of = ts.f32[t] + base;
    uint8_t* ob = with_u8 ? ts.u8[t] + base : nullptr;
    for (int p = (blockIdx.x * NT + threadIdx.x) * PER; p < hw; p += gridDim.x * NT * PER) {
        Px px[PER];
        load_px<VEC>(img, hw, p, px);
#pragma unroll
        for (int j = 0; j < PER; ++j) px[j] = chain(px[j], rc, 0, rc.count, mean);
        if constexpr (VEC) {
            const int c[3][4] = {{px[0].r, px[1].r, px[2].r, px[3].r}, {px[0].g, px[1].g, px[2].g, px[3].g},
                                 {px[0].b, px[1].b, px[2].b, px[3].b}};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const size_t o = (size_t)ch * hw + p;
                *reinterpret_cast<float4*>(of + o) = make_float4((float)c[ch][0] / 255.f, (float)c[ch][1] / 255.f,
                                                                 (float)c[ch][2] / 255.f, (float)c[ch][3] / 255.f);
                if (ob != nullptr)
                    *reinterpret_cast<uint32_t*>(ob + o) = (uint32_t)c[ch][0] | ((uint32_t)c[ch][1] << 8) | ((uint32_t)c[ch][2] << 16)
                                                           | ((uint32_t)c[ch][3] << 24);
            }
        } else {
            const int c[3] = {px[0].r, px[0].g, px[0].b};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const size_t o = (size_t)ch * hw + p;
                of[o] = (float)c[ch] / 255.f;
                if (ob != nullptr) ob[o] = (uint8_t)c[ch];
            }
        }
    }
}

}  // namespace

extern "C" {

// workgroups per image: enough for about MAX_BLOCKS in the launch, at least 4, never more than the image has rounds
static int blocks_per_image(int hw, int images, int per) { return min((hw + per - 1) / per, max(4, MAX_BLOCKS / images)); }

int64_t dmh_color_jitter_ws_size(int T, int B, int H, int W) {
    if (T < 1 || T > DMH_JITTER_MAX_TENSORS || B < 1 || H < 1 || W < 1 || (int64_t)T * B > 65535) return -1;
    if ((int64_t)H * W > DMH_JITTER_MAX_PIXELS || (int64_t)B * 3 * H * W >= (1ll << 31)) return -1;
    return (int64_t)T * B * blocks_per_image(H * W, T * B, NT);      // the one-pixel form has the most workgroups
}

int dmh_color_jitter(const uint8_t* const* src, float* const* out_f32, uint8_t* const* out_u8, int T, int B, int H, int W,
                     const int32_t* rec, int with_contrast, uint32_t* ws, void* stream) {
    DMH_REQUIRE(src && out_f32 && rec, "null pointer");
    DMH_REQUIRE(T >= 1 && T <= DMH_JITTER_MAX_TENSORS, "need 1 <= T <= 8 tensors");
    DMH_REQUIRE(B >= 1 && H >= 1 && W >= 1 && (int64_t)T * B <= 65535, "need B, H, W >= 1 and T B <= 65535");
    DMH_REQUIRE((int64_t)H * W <= DMH_JITTER_MAX_PIXELS, "255 H W must fit 32 bits: the sum of L is a 32-bit integer");
    DMH_REQUIRE((int64_t)B * 3 * H * W < (1ll << 31), "a tensor must hold fewer than 2^31 elements");
    DMH_REQUIRE(!with_contrast || ws, "the contrast pass needs its workspace (dmh_color_jitter_ws_size words)");
    DMH_REQUIRE(((uintptr_t)rec & 3) == 0 && ((uintptr_t)ws & 3) == 0, "rec and ws must be 4-byte aligned");
    const int hw = H * W;
    Tensors ts;
    memset(&ts, 0, sizeof(ts));
    bool vec = hw % 4 == 0;
    for (int t = 0; t < T; ++t) {
        DMH_REQUIRE(src[t] && out_f32[t] && (!out_u8 || out_u8[t]), "null tensor pointer");
        DMH_REQUIRE(((uintptr_t)out_f32[t] & 3) == 0, "out_f32 must be 4-byte aligned");
        DMH_REQUIRE((const void*)src[t] != (const void*)out_f32[t] && (!out_u8 || src[t] != out_u8[t]), "outputs must not alias the sources");
        ts.src[t] = src[t];
        ts.f32[t] = out_f32[t];
        ts.u8[t] = out_u8 ? out_u8[t] : nullptr;
        vec = vec && ((uintptr_t)src[t] & 3) == 0 && ((uintptr_t)out_f32[t] & 15) == 0 && (!out_u8 || ((uintptr_t)out_u8[t] & 3) == 0);
    }
    const hipStream_t s = (hipStream_t)stream;
    const int images = T * B;
    const dim3 grid((unsigned)blocks_per_image(hw, images, NT * (vec ? 4 : 1)), (unsigned)images);      // the same in both passes
    const uint32_t* sums = with_contrast ? ws : nullptr;       // without the first pass nothing is read
    if (with_contrast) {
        if (vec) hipLaunchKernelGGL(jitter_lsum_kernel<true>, grid, dim3(NT), 0, s, ts, B, hw, rec, ws);
        else hipLaunchKernelGGL(jitter_lsum_kernel<false>, grid, dim3(NT), 0, s, ts, B, hw, rec, ws);
    }
    if (vec) hipLaunchKernelGGL(jitter_apply_kernel<true>, grid, dim3(NT), 0, s, ts, B, hw, rec, sums, out_u8 != nullptr);
    else hipLaunchKernelGGL(jitter_apply_kernel<false>, grid, dim3(NT), 0, s, ts, B, hw, rec, sums, out_u8 != nullptr);
    return check_launch("dmh_color_jitter");
}

}  // extern "C"
