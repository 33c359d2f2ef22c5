// K31 -- Pillow's 8-bit separable resample on the device, bit for bit: Image.resize(size, LANCZOS / BILINEAR) of an RGB or L
// image with reducing_gap=None (gfx950).
//
// Replaces the PIL chain of the KITTI loader (MD2/datasets/mono_dataset.py:100-104,119-144): four levels per image, each from
// the previous level's 8-bit result, 34 ms of one CPU core per 375 x 1242 frame.
//
// Pillow's ImagingResample in 8 bits per channel is integer arithmetic once the coefficients exist:
//   horizontal   tmp[y][x] = clip8((2^21 + sum_t src[y][xmin(x) + t] * kh[x][t]) >> 22)
//   vertical     out[y][x] = clip8((2^21 + sum_t tmp[ymin(y) + t][x] * kv[y][t]) >> 22)
// with 32-bit sums, an arithmetic shift and clip8 = min(max(., 0), 255).  The coefficient tables (window start, tap count, taps
// with 22 fraction bits) are made on the host in float64 and arrive as int32 words: min[out] | count[out] | k[ksize][out], so
// that a wave reads consecutive words.  A pass whose size does not change has the table (x, 1, 2^22), which returns the pixel.
//
// One launch per level.  A workgroup takes TILE_ROWS output rows of one channel of one image: the horizontal pass runs for the
// source rows those output rows need (tv.min[first] .. tv.min[last] + tv.count[last]) into an LDS tile of 8-bit rows, and the
// vertical pass reads the tile.  The 8-bit intermediate never goes to memory, and the 3.5 .. 6 source rows per output row that
// two neighbouring tiles share are recomputed (17 rows for 8 at 375 -> 320; 28 for 8 at a halving).
//
// Sources: uint8 with arbitrary element strides (HWC as a decoded file lies, planar as the previous level wrote it), or float32
// quantised on read as torchvision's ToPILImage does, (uint8)(v * 255.f).  Every image of a batch has its own source size and
// its own pair of tables (desc); flip mirrors the read of the source column, which is transpose(FLIP_LEFT_RIGHT) before the
// resize, exactly: the rounded taps are not mirror-symmetric, so flipping the result would not be.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int TILE_ROWS = DMH_PIL_TILE_ROWS;
constexpr int ROWS_PER_PASS = 4;        // source rows one thread carries through the taps of its column: one tap load for four
constexpr int PRECISION_BITS = 22;      // Pillow: 32 - 8 - 2

__device__ __forceinline__ int clip8(int v) {
    v >>= PRECISION_BITS;
    return min(max(v, 0), 255);
}

template <bool F32>
__device__ __forceinline__ int load_px(const void* __restrict__ src, int off) {
    if (F32) {
        const float v = ((const float*)src)[off] * 255.f;        // ToPILImage: pic.mul(255).byte(), a truncation
        return min(max((int)v, 0), 255);
    }
    return ((const uint8_t*)src)[off];
}

template <bool F32>
__global__ __launch_bounds__(NT) void pil_resample_kernel(const void* __restrict__ src, int sn, int sc, int sy, int sx, int Hs, int Ws,
                                                          const int32_t* __restrict__ tables, int table_words,
                                                          const int32_t* __restrict__ desc, const int32_t* __restrict__ flip, int C,
                                                          int Ho, int Wo, int lds_rows, uint8_t* __restrict__ out_u8,
                                                          float* __restrict__ out_f32) {
    extern __shared__ __attribute__((aligned(16))) uint8_t tile[];      // [lds_rows][Wo]
    const int n = blockIdx.z, c = blockIdx.y;
    const int ty0 = blockIdx.x * TILE_ROWS, ty1 = min(ty0 + TILE_ROWS, Ho);
    const int32_t* d = desc + n * 8;
    const int in_h = min(max(d[0], 1), Hs), in_w = min(max(d[1], 1), Ws);
    const int h_off = d[2], kh = d[3], v_off = d[4], kv = d[5];
    // a descriptor that points outside the tables is a host bug; it must not become a read out of bounds
    if (h_off < 0 || kh < 1 || v_off < 0 || kv < 1 || (int64_t)h_off + (int64_t)Wo * (2 + kh) > table_words
        || (int64_t)v_off + (int64_t)Ho * (2 + kv) > table_words)
        return;
    const int32_t* th = tables + h_off;
    const int32_t* tv = tables + v_off;
    const bool fl = flip != nullptr && flip[n] != 0;

    const int y0 = min(max(tv[ty0], 0), in_h - 1);
    const int y1 = min(max(tv[ty1 - 1] + tv[Ho + ty1 - 1], y0 + 1), in_h);
    const int nrows = min(y1 - y0, lds_rows);
    const int base = n * sn + c * sc;

    // horizontal pass: thread = output column, ROWS_PER_PASS source rows per trip through the taps
    for (int x = threadIdx.x; x < Wo; x += NT) {
        const int xmin = min(max(th[x], 0), in_w - 1);
        const int cnt = min(min(max(th[Wo + x], 0), kh), in_w - xmin);
        const int32_t* k = th + 2 * Wo + x;
        for (int r0 = 0; r0 < nrows; r0 += ROWS_PER_PASS) {
            int acc[ROWS_PER_PASS], roff[ROWS_PER_PASS];
#pragma unroll
            for (int j = 0; j < ROWS_PER_PASS; ++j) {
                acc[j] = 1 << (PRECISION_BITS - 1);
                roff[j] = base + min(y0 + r0 + j, in_h - 1) * sy;
            }
            for (int t = 0; t < cnt; ++t) {
                const int kt = k[t * Wo];
                const int col = fl ? in_w - 1 - (xmin + t) : xmin + t;
#pragma unroll
                for (int j = 0; j < ROWS_PER_PASS; ++j) acc[j] += load_px<F32>(src, roff[j] + col * sx) * kt;
            }
#pragma unroll
            for (int j = 0; j < ROWS_PER_PASS; ++j)
                if (r0 + j < nrows) tile[(r0 + j) * Wo + x] = (uint8_t)clip8(acc[j]);
        }
    }
    __syncthreads();

    // vertical pass: thread = one output pixel of the tile, the column fastest
    const int work = (ty1 - ty0) * Wo;
    for (int i = threadIdx.x; i < work; i += NT) {
        const int ry = i / Wo, x = i - ry * Wo, ty = ty0 + ry;
        const int ymin = min(max(tv[ty] - y0, 0), nrows - 1);
        const int cnt = min(min(max(tv[Ho + ty], 0), kv), nrows - ymin);
        const int32_t* k = tv + 2 * Ho + ty;
        int acc = 1 << (PRECISION_BITS - 1);
        for (int t = 0; t < cnt; ++t) acc += (int)tile[(ymin + t) * Wo + x] * k[t * Ho];
        const int v = clip8(acc);
        const int o = ((n * C + c) * Ho + ty) * Wo + x;
        if (out_u8) out_u8[o] = (uint8_t)v;
        if (out_f32) out_f32[o] = __fdiv_rn((float)v, 255.f);      // torch's .float().div(255): an IEEE division, no reciprocal
    }
}

double filter_support(int filter) { return filter == DMH_PIL_LANCZOS ? 3.0 : (filter == DMH_PIL_BILINEAR ? 1.0 : 0.0); }

}  // namespace

extern "C" {

int64_t dmh_pil_resample_tables_size(int in_size, int out_size, int filter) {
    if (in_size < 1 || out_size < 1 || in_size >= (1 << 20) || out_size >= (1 << 20) || filter_support(filter) == 0.0) return -1;
    if (in_size == out_size) return 3ll * out_size;        // the pass Pillow skips: (x, 1, 2^22)
    double filterscale = (double)in_size / out_size;       // Pillow's precompute_coeffs
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = filter_support(filter) * filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    return (int64_t)out_size * (2 + ksize);
}

int dmh_pil_resample(const void* src, int src_f32, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int Hs, int Ws,
                     const int32_t* tables, int64_t table_words, const int32_t* desc, const int32_t* flip, int N, int C,
                     int H_out, int W_out, int lds_rows, uint8_t* out_u8, float* out_f32, void* stream) {
    DMH_REQUIRE(src && tables && desc, "null pointer");
    DMH_REQUIRE(out_u8 || out_f32, "need out_u8 or out_f32");
    DMH_REQUIRE(N > 0 && C > 0 && Hs > 0 && Ws > 0 && H_out > 0 && W_out > 0, "need N, C, Hs, Ws, H_out, W_out > 0");
    DMH_REQUIRE(N <= 65535 && C <= 65535, "need N, C <= 65535");
    DMH_REQUIRE(sn >= 0 && sc >= 0 && sy > 0 && sx > 0, "need strides sn, sc >= 0 and sy, sx > 0");
    // the last element any image can reach, in 32-bit offsets
    DMH_REQUIRE((N - 1) * sn + (C - 1) * sc + (int64_t)(Hs - 1) * sy + (int64_t)(Ws - 1) * sx < (1ll << 31),
                "the source must span fewer than 2^31 elements");
    DMH_REQUIRE((int64_t)N * C * H_out * W_out < (1ll << 31), "need N * C * H_out * W_out < 2^31");
    DMH_REQUIRE(table_words > 0 && table_words < (1ll << 31), "need 0 < table_words < 2^31");
    DMH_REQUIRE(lds_rows > 0 && (int64_t)lds_rows * W_out <= 65536, "need 0 < lds_rows and lds_rows * W_out <= 65536");
    DMH_REQUIRE(((uintptr_t)tables & 3) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)flip & 3) == 0
                    && ((uintptr_t)out_f32 & 3) == 0 && (!src_f32 || ((uintptr_t)src & 3) == 0),
                "tables, desc, flip and the float buffers must be 4-byte aligned");
    DMH_REQUIRE((const void*)out_u8 != src && (const void*)out_f32 != src, "the outputs must not alias the source");
    const dim3 grid((H_out + TILE_ROWS - 1) / TILE_ROWS, C, N);
    const size_t lds = ((size_t)lds_rows * W_out + 15) & ~(size_t)15;
    if (src_f32)
        hipLaunchKernelGGL(pil_resample_kernel<true>, grid, dim3(NT), lds, (hipStream_t)stream, src, (int)sn, (int)sc, (int)sy,
                           (int)sx, Hs, Ws, tables, (int)table_words, desc, flip, C, H_out, W_out, lds_rows, out_u8, out_f32);
    else
        hipLaunchKernelGGL(pil_resample_kernel<false>, grid, dim3(NT), lds, (hipStream_t)stream, src, (int)sn, (int)sc, (int)sy,
                           (int)sx, Hs, Ws, tables, (int)table_words, desc, flip, C, H_out, W_out, lds_rows, out_u8, out_f32);
    return check_launch("dmh_pil_resample");
}

}  // extern "C"
