// K25 -- benign depth evaluation (MD2/evaluate_depth.py:351-391) on the device (gfx950): predicted depth at every ground-truth
// map's own resolution, exact medians without a sort, the eight metrics per image.
//
// Replaces, per image, one cv2.resize, two boolean gathers, two np.median (a sort each) and eight numpy reductions on the host.
// Here a batch of n images is one chain of launches and nothing is read by the host while it runs.
//
//   gt      float [T]                 the ground-truth maps of the whole pack, one after the other.
//   table   int32 [N][DMH_EIGEN_REC]  one record per image: 0 offset into gt, 1 gt_h, 2 gt_w, 3 y0, 4 y1, 5 x0, 6 x1 (the crop,
//                                     the whole map for splits other than eigen), 7 the image's first work block.
//   blk_img int32 [blocks of the pack] the image a work block belongs to.  A work block is DMH_EIGEN_CHUNK pixels of ONE image,
//                                     so a workgroup's partial sums and histogram belong to one image; the blocks of the images
//                                     first .. first + n - 1 are consecutive, and a launch's grid is exactly those.
//   depth   float [pixels of the batch] scratch laid out like gt (index - offset of image ``first``): the predicted depth where
//                                     the pixel is valid, the bit pattern 0xffffffff where it is not.
//   ws      uint32                    n x 3 passes x 2 ranks x 2048 bins, then n x 8 words of selection state.
//
// Every kernel checks what it reads out of the tables against the sizes the host passed (a record that points outside gt or depth
// does nothing), so a wrong table cannot make a launch write or read out of bounds.
//
// Median: np.median = the fp32 mean of the elements of rank (n-1)/2 and n/2.  Both ranks are found by a most-significant-digit
// radix select on the order-preserving integer key of the float, 11 / 11 / 10 bits: a histogram pass (LDS integer atomics per
// workgroup, the non-empty bins added to global memory with integer atomics), then one workgroup per image walks the bins.
// Integer additions commute, so the result does not depend on the order the atomics arrive in.  Pass 0 of the predictions is
// fused into the depth kernel.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int CHUNK = DMH_EIGEN_CHUNK;
constexpr int REC = DMH_EIGEN_REC;
constexpr int BINS = 2048;
constexpr int PASSES = 3;
constexpr int WS_IMG = PASSES * 2 * BINS;       // histogram words per image
constexpr int ST = 8;                           // state words per image: 0 prefix lo, 1 prefix hi, 2 rank lo, 3 rank hi, 4 count
constexpr uint32_t MARK = 0xffffffffu;
constexpr int NQ = 9;                           // count, a1, a2, a3, abs_err, sq_err, log_sq_err, abs_rel, sq_rel

struct Tables {
    const int32_t* table;
    const int32_t* blk_img;
    int n_images, n_blocks;     // sizes of the two tables
    int first, n, b0;           // this launch: images first .. first + n - 1, whose first work block is b0
    int eigen;
};

struct Work {
    int li;                     // image index inside the batch, -1: nothing to do
    int64_t off;                // offset of the image in gt
    int gh, gw, y0, y1, x0, x1;
    int p0, p1;                 // this block's pixels of the image
};

__device__ __forceinline__ Work block_work(const Tables& t, int64_t gt_len) {
    Work w;
    w.li = -1;
    w.p0 = w.p1 = 0;
    const int b = t.b0 + (int)blockIdx.x;
    if (b < 0 || b >= t.n_blocks) return w;
    const int img = t.blk_img[b];
    if (img < t.first || img >= t.first + t.n || img >= t.n_images) return w;
    const int32_t* r = t.table + (int64_t)img * REC;
    w.off = r[0]; w.gh = r[1]; w.gw = r[2]; w.y0 = r[3]; w.y1 = r[4]; w.x0 = r[5]; w.x1 = r[6];
    const int c = b - r[7];
    if (w.gh <= 0 || w.gw <= 0 || c < 0 || w.off < 0) return w;
    const int64_t npx = (int64_t)w.gh * w.gw, p0 = (int64_t)c * CHUNK;
    if (p0 >= npx || w.off + npx > gt_len) return w;
    w.p0 = (int)p0;
    w.p1 = (int)(p0 + CHUNK < npx ? p0 + CHUNK : npx);
    w.li = img - t.first;
    return w;
}

// :360-370: the range mask and the Eigen crop, or gt > 0 for the other splits
__device__ __forceinline__ bool gt_valid(float g, int p, const Work& w, int eigen) {
    if (!eigen) return g > 0.f;
    const int y = p / w.gw, x = p - y * w.gw;
    return g > 1e-3f && g < 80.f && y >= w.y0 && y < w.y1 && x >= w.x0 && x < w.x1;
}

__device__ __forceinline__ uint32_t float_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ void hist_clear(uint32_t* h) {
    for (int i = threadIdx.x; i < 2 * BINS; i += NT) h[i] = 0u;
    __syncthreads();
}

// pass 0 counts every value (both ranks share histogram 0); passes 1 and 2 count the values under each rank's prefix
__device__ __forceinline__ void hist_add(uint32_t* h, uint32_t key, int pass, uint32_t pre_lo, uint32_t pre_hi) {
    if (pass == 0) {
        atomicAdd(&h[key >> 21], 1u);
    } else {
        const uint32_t pre = pass == 1 ? key >> 21 : key >> 10;
        const uint32_t d = pass == 1 ? (key >> 10) & 0x7ffu : key & 0x3ffu;
        if (pre == pre_lo) atomicAdd(&h[d], 1u);
        if (pre == pre_hi) atomicAdd(&h[BINS + d], 1u);
    }
}

__device__ __forceinline__ void hist_flush(const uint32_t* h, uint32_t* ws, int li, int pass) {
    __syncthreads();
    uint32_t* g = ws + ((int64_t)li * PASSES + pass) * 2 * BINS;
    for (int i = threadIdx.x; i < 2 * BINS; i += NT) {
        const uint32_t c = h[i];
        if (c) atomicAdd(&g[i], c);
    }
}

// ---------------------------------------------------------------------------------------------------- depth at gt resolution
// OpenCV's INTER_LINEAR coordinate of one axis: f = float((d + .5) * scale - .5) with scale = src / dst in double, s = floor(f),
// f -= s; clamped at both ends with f = 0; the second tap clamped to src - 1.
__device__ __forceinline__ void lin_axis(int d, double scale, int src, int& s0, int& s1, float& f) {
#pragma clang fp contract(off)
    float ff = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(ff);
    ff -= (float)s;
    if (s < 0) { s = 0; ff = 0.f; }
    if (s >= src - 1) { s = src - 1; ff = 0.f; }
    s0 = s;
    s1 = s + 1 < src ? s + 1 : src - 1;
    f = ff;
}

// :107-108: 1 - clip(20 (x / (w - 1) - 0.05), 0, 1) in double, rounded to fp32
__device__ __forceinline__ float left_mask(int x, int w) {
#pragma clang fp contract(off)
    const double t = w > 1 ? (double)x / (double)(w - 1) : 0.0;
    double c = 20.0 * (t - 0.05);
    c = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
    return (float)(1.0 - c);
}

// one tap: the disparity, or with PP the blend of batch_post_process_disparity (:102-110) of it and the mirrored flipped one
template <bool PP>
__device__ __forceinline__ float tap(const float* __restrict__ l, const float* __restrict__ r, int w, int yy, int xx) {
    const float lv = l[yy * w + xx];
    if (!PP) return lv;
    const float rv = r[yy * w + (w - 1 - xx)];
    const float lm = left_mask(xx, w), rm = left_mask(w - 1 - xx, w);
    return rm * lv + lm * rv + (1.f - lm - rm) * (0.5f * (lv + rv));
}

template <bool PP, bool HIST>
__global__ __launch_bounds__(NT) void eigen_depth_kernel(const float* __restrict__ pred, const float* __restrict__ flip, int h, int w,
                                                         const float* __restrict__ gt, int64_t gt_len, Tables t, float factor,
                                                         int64_t px0, float* __restrict__ depth, int64_t depth_len,
                                                         uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_hist[HIST ? 2 * BINS : 1];
    const Work wk = block_work(t, gt_len);
    if (wk.li < 0) return;
    const int64_t dbase = wk.off - px0;
    if (dbase < 0 || dbase + (int64_t)wk.gh * wk.gw > depth_len) return;
    if (HIST) hist_clear(s_hist);
    const double sx = (double)w / (double)wk.gw, sy = (double)h / (double)wk.gh;
    const float* l = pred + (int64_t)wk.li * h * w;
    const float* r = PP ? flip + (int64_t)wk.li * h * w : nullptr;
    for (int p = wk.p0 + (int)threadIdx.x; p < wk.p1; p += NT) {
        const float g = gt[wk.off + p];
        float d = __uint_as_float(MARK);
        if (gt_valid(g, p, wk, t.eigen)) {
            const int y = p / wk.gw, x = p - y * wk.gw;
            int xa, xb, ya, yb;
            float fx, fy;
            lin_axis(x, sx, w, xa, xb, fx);
            lin_axis(y, sy, h, ya, yb, fy);
            const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
            const float r0 = a0 * tap<PP>(l, r, w, ya, xa) + a1 * tap<PP>(l, r, w, ya, xb);
            const float r1 = a0 * tap<PP>(l, r, w, yb, xa) + a1 * tap<PP>(l, r, w, yb, xb);
            const float disp = b0 * r0 + b1 * r1;
            d = (1.f / disp) * factor;
            if (__float_as_uint(d) == MARK) d = __uint_as_float(0x7fc00000u);    // a NaN of the data stays a valid pixel
            if (HIST) hist_add(s_hist, float_key(d), 0, 0u, 0u);
        }
        depth[dbase + p] = d;
    }
    if (HIST) hist_flush(s_hist, ws, wk.li, 0);
}

// ---------------------------------------------------------------------------------------------------- histogram passes
// FROM_GT: the valid ground-truth values (when the pack is made); otherwise the valid predicted depths of the scratch buffer.
template <bool FROM_GT>
__global__ __launch_bounds__(NT) void eigen_hist_kernel(const float* __restrict__ src, int64_t src_len, int64_t px0, int64_t gt_len,
                                                        Tables t, int pass, uint32_t* __restrict__ ws) {
    __shared__ uint32_t s_hist[2 * BINS];
    const Work wk = block_work(t, gt_len);
    if (wk.li < 0) return;
    const int64_t base = FROM_GT ? wk.off : wk.off - px0;
    if (base < 0 || base + (int64_t)wk.gh * wk.gw > src_len) return;
    const uint32_t* st = ws + (int64_t)t.n * WS_IMG + wk.li * ST;
    if (pass > 0 && st[4] == 0u) return;
    const uint32_t pre_lo = st[0], pre_hi = st[1];
    hist_clear(s_hist);
    for (int p = wk.p0 + (int)threadIdx.x; p < wk.p1; p += NT) {
        const float v = src[base + p];
        const bool ok = FROM_GT ? gt_valid(v, p, wk, t.eigen) : __float_as_uint(v) != MARK;
        if (ok) hist_add(s_hist, float_key(v), pass, pre_lo, pre_hi);
    }
    hist_flush(s_hist, ws, wk.li, pass);
}

// One workgroup per image: the bin each of the two ranks falls into, the new prefixes and the ranks inside the bin.  After the
// last pass the prefixes are the two keys: the median, the count and (with med_gt) the ratio are written.
__global__ __launch_bounds__(NT) void eigen_scan_kernel(uint32_t* __restrict__ ws, int n, int pass, const float* __restrict__ med_gt,
                                                        int first, float* __restrict__ med_out, int32_t* __restrict__ cnt_out,
                                                        float* __restrict__ ratio) {
    __shared__ uint32_t s_sum[2][NT];
    const int li = blockIdx.x;
    if (li >= n) return;
    uint32_t* st = ws + (int64_t)n * WS_IMG + li * ST;
    const uint32_t* hist = ws + ((int64_t)li * PASSES + pass) * 2 * BINS;
    constexpr int PER = BINS / NT;
    for (int k = 0; k < 2; ++k) {
        const uint32_t* h = hist + (pass == 0 ? 0 : k * BINS);
        uint32_t s = 0u;
        for (int i = 0; i < PER; ++i) s += h[threadIdx.x * PER + i];
        s_sum[k][threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t total = st[4];
    if (pass == 0) {
        total = 0u;
        for (int i = 0; i < NT; ++i) total += s_sum[0][i];
        st[0] = st[1] = 0u;
        st[2] = total ? (total - 1u) / 2u : 0u;
        st[3] = total / 2u;
        st[4] = total;
    }
    if (total) {
        const int bits = pass == 2 ? 10 : 11;
        for (int k = 0; k < 2; ++k) {
            const uint32_t* h = hist + (pass == 0 ? 0 : k * BINS);
            const uint32_t rank = st[2 + k];
            uint32_t cum = 0u;
            int i = 0;
            while (i < NT - 1 && cum + s_sum[k][i] <= rank) cum += s_sum[k][i++];
            int b = i * PER;
            while (b < i * PER + PER - 1 && cum + h[b] <= rank) cum += h[b++];
            st[k] = (st[k] << bits) | (uint32_t)b;
            st[2 + k] = rank - cum;
        }
    }
    if (pass == PASSES - 1) {
        const float med = total ? (key_float(st[0]) + key_float(st[1])) / 2.f : __uint_as_float(0x7fc00000u);
        med_out[li] = med;
        if (cnt_out) cnt_out[li] = (int32_t)total;
        if (ratio) ratio[li] = med_gt[first + li] / med;
    }
}

// ---------------------------------------------------------------------------------------------------- metrics
// :375-384 with compute_errors :61-76: pred *= ratio, clamp to [1e-3, 80], nine fp32 sums per work block (K8's accumulators).
__global__ __launch_bounds__(NT) void eigen_metrics_kernel(const float* __restrict__ gt, int64_t gt_len, const float* __restrict__ depth,
                                                           int64_t depth_len, int64_t px0, Tables t, const float* __restrict__ ratio,
                                                           float* __restrict__ partials) {
    __shared__ float s_red[NT / WAVE];
    float acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = 0.f;
    Work wk = block_work(t, gt_len);
    const int64_t dbase = wk.li < 0 ? 0 : wk.off - px0;
    if (wk.li >= 0 && (dbase < 0 || dbase + (int64_t)wk.gh * wk.gw > depth_len)) wk.p0 = wk.p1 = 0;
    if (wk.li < 0) wk.p0 = wk.p1 = 0;
    const float rt = (ratio && wk.li >= 0) ? ratio[wk.li] : 1.f;
    for (int p = wk.p0 + (int)threadIdx.x; p < wk.p1; p += NT) {
        const float d = depth[dbase + p];
        if (__float_as_uint(d) == MARK) continue;
        const float g = gt[wk.off + p];
        float pr = ratio ? d * rt : d;
        pr = pr < 1e-3f ? 1e-3f : pr;       // :381-382 (a NaN stays)
        pr = pr > 80.f ? 80.f : pr;
        const float th = fmaxf(g / pr, pr / g), df = g - pr, ld = logf(g) - logf(pr);
        acc[0] += 1.f;
        acc[1] += th < 1.25f ? 1.f : 0.f;
        acc[2] += th < 1.25f * 1.25f ? 1.f : 0.f;
        acc[3] += th < 1.25f * 1.25f * 1.25f ? 1.f : 0.f;
        acc[4] += fabsf(df);
        acc[5] += df * df;
        acc[6] += ld * ld;
        acc[7] += fabsf(df) / g;
        acc[8] += df * df / g;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const float s = block_sum<NT>(acc[q], s_red);
        if (threadIdx.x == 0) partials[(int64_t)blockIdx.x * NQ + q] = s;
    }
}

// One workgroup per image: its blocks' partial sums in double, in a fixed order (K8's finalize).
__global__ __launch_bounds__(NT) void eigen_metrics_finalize_kernel(const float* __restrict__ partials, int grid, Tables t,
                                                                    float* __restrict__ errors) {
    __shared__ double s_red[NT];
    const int li = blockIdx.x, img = t.first + li;
    int lo = 0, nb = 0;
    if (li < t.n && img < t.n_images) {
        const int32_t* r = t.table + (int64_t)img * REC;
        const int64_t npx = (int64_t)r[1] * r[2];
        lo = r[7] - t.b0;
        nb = (r[1] > 0 && r[2] > 0) ? (int)((npx + CHUNK - 1) / CHUNK) : 0;
        if (lo < 0 || lo + nb > grid) nb = 0;
    }
    double tot[NQ];
    for (int q = 0; q < NQ; ++q) {
        double a = 0.0;
        for (int i = threadIdx.x; i < nb; i += NT) a += (double)partials[(int64_t)(lo + i) * NQ + q];
        __syncthreads();
        s_red[threadIdx.x] = a;
        __syncthreads();
        for (int o = NT / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
            __syncthreads();
        }
        tot[q] = s_red[0];
    }
    if (threadIdx.x == 0 && li < t.n) {
        const double c = tot[0];            // no valid pixel: 0 / 0, a row of NaN as numpy's mean of nothing
        float* out = errors + (int64_t)li * 8;
        out[0] = (float)(tot[4] / c);        // abs_err
        out[1] = (float)(tot[7] / c);        // abs_rel
        out[2] = (float)(tot[8] / c);        // sq_rel
        out[3] = (float)sqrt(tot[5] / c);    // rmse
        out[4] = (float)sqrt(tot[6] / c);    // rmse_log
        out[5] = (float)(tot[1] / c);        // a1
        out[6] = (float)(tot[2] / c);        // a2
        out[7] = (float)(tot[3] / c);        // a3
    }
}

int check_tables(const int32_t* table, const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int grid) {
    DMH_REQUIRE(table && blk_img, "null pointer");
    DMH_REQUIRE(n_images > 0 && n_blocks > 0, "empty pack");
    DMH_REQUIRE(first >= 0 && n > 0 && n <= DMH_EIGEN_MAX_BATCH && first + n <= n_images, "images first .. first + n - 1 must lie in the pack (n <= DMH_EIGEN_MAX_BATCH)");
    DMH_REQUIRE(b0 >= 0 && grid > 0 && b0 + grid <= n_blocks, "work blocks b0 .. b0 + grid - 1 must lie in the pack");
    return DMH_OK;
}

Tables make_tables(const int32_t* table, const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int eigen) {
    Tables t;
    t.table = table; t.blk_img = blk_img; t.n_images = n_images; t.n_blocks = n_blocks;
    t.first = first; t.n = n; t.b0 = b0; t.eigen = eigen;
    return t;
}

}  // namespace

extern "C" {

int64_t dmh_eigen_select_ws_size(int n) {
    return n > 0 && n <= DMH_EIGEN_MAX_BATCH ? (int64_t)n * (WS_IMG + ST) : -1;
}

int64_t dmh_eigen_partials_size(int grid) { return grid > 0 ? (int64_t)grid * NQ : -1; }

int dmh_eigen_gt_stats(const float* gt, int64_t gt_len, const int32_t* table, const int32_t* blk_img, int n_images, int n_blocks,
                       int first, int n, int b0, int grid, int eigen, uint32_t* ws, float* med, int32_t* count, void* stream) {
    DMH_REQUIRE(gt && ws && med && count && gt_len > 0, "null pointer or empty ground truth");
    if (int rc = check_tables(table, blk_img, n_images, n_blocks, first, n, b0, grid)) return rc;
    const Tables t = make_tables(table, blk_img, n_images, n_blocks, first, n, b0, eigen);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, (size_t)dmh_eigen_select_ws_size(n) * sizeof(uint32_t), s) != hipSuccess)
        return check_launch("dmh_eigen_gt_stats");
    for (int pass = 0; pass < PASSES; ++pass) {
        hipLaunchKernelGGL(eigen_hist_kernel<true>, dim3(grid), dim3(NT), 0, s, gt, gt_len, (int64_t)0, gt_len, t, pass, ws);
        hipLaunchKernelGGL(eigen_scan_kernel, dim3(n), dim3(NT), 0, s, ws, n, pass, (const float*)nullptr, 0, med, count,
                           (float*)nullptr);
    }
    return check_launch("dmh_eigen_gt_stats");
}

int dmh_eigen_pred_depth(const float* pred, const float* flip, int h, int w, const float* gt, int64_t gt_len, const int32_t* table,
                         const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int grid, int eigen,
                         float factor, int64_t px0, float* depth, int64_t depth_len, uint32_t* ws, void* stream) {
    DMH_REQUIRE(pred && gt && depth && gt_len > 0 && depth_len > 0, "null pointer or empty buffer");
    DMH_REQUIRE(h > 0 && w > 0 && (int64_t)n * h * w < ((int64_t)1 << 31), "need 0 < n * h * w < 2^31");
    DMH_REQUIRE(px0 >= 0 && px0 < gt_len, "px0 must be an offset into gt");
    if (int rc = check_tables(table, blk_img, n_images, n_blocks, first, n, b0, grid)) return rc;
    const Tables t = make_tables(table, blk_img, n_images, n_blocks, first, n, b0, eigen);
    hipStream_t s = (hipStream_t)stream;
    if (ws && hipMemsetAsync(ws, 0, (size_t)dmh_eigen_select_ws_size(n) * sizeof(uint32_t), s) != hipSuccess)
        return check_launch("dmh_eigen_pred_depth");
#define DMH_EIGEN_DEPTH(PP, HIST)                                                                                              \
    hipLaunchKernelGGL((eigen_depth_kernel<PP, HIST>), dim3(grid), dim3(NT), 0, s, pred, flip, h, w, gt, gt_len, t, factor, px0, \
                       depth, depth_len, ws)
    if (flip) {
        if (ws) DMH_EIGEN_DEPTH(true, true); else DMH_EIGEN_DEPTH(true, false);
    } else {
        if (ws) DMH_EIGEN_DEPTH(false, true); else DMH_EIGEN_DEPTH(false, false);
    }
#undef DMH_EIGEN_DEPTH
    return check_launch("dmh_eigen_pred_depth");
}

int dmh_eigen_pred_ratio(const float* depth, int64_t depth_len, int64_t px0, int64_t gt_len, const int32_t* table,
                         const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int grid, uint32_t* ws,
                         const float* med_gt, float* med_pred, float* ratio, void* stream) {
    DMH_REQUIRE(depth && ws && med_gt && med_pred && ratio && depth_len > 0, "null pointer or empty buffer");
    if (int rc = check_tables(table, blk_img, n_images, n_blocks, first, n, b0, grid)) return rc;
    const Tables t = make_tables(table, blk_img, n_images, n_blocks, first, n, b0, 0);
    hipStream_t s = (hipStream_t)stream;
    for (int pass = 0; pass < PASSES; ++pass) {     // pass 0's histogram was filled by dmh_eigen_pred_depth
        if (pass > 0)
            hipLaunchKernelGGL(eigen_hist_kernel<false>, dim3(grid), dim3(NT), 0, s, depth, depth_len, px0, gt_len, t, pass, ws);
        hipLaunchKernelGGL(eigen_scan_kernel, dim3(n), dim3(NT), 0, s, ws, n, pass, med_gt, first, med_pred, (int32_t*)nullptr,
                           ratio);
    }
    return check_launch("dmh_eigen_pred_ratio");
}

int dmh_eigen_metrics(const float* gt, int64_t gt_len, const float* depth, int64_t depth_len, int64_t px0, const int32_t* table,
                      const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int grid, const float* ratio,
                      float* partials, float* errors, void* stream) {
    DMH_REQUIRE(gt && depth && partials && errors && gt_len > 0 && depth_len > 0, "null pointer or empty buffer");
    if (int rc = check_tables(table, blk_img, n_images, n_blocks, first, n, b0, grid)) return rc;
    const Tables t = make_tables(table, blk_img, n_images, n_blocks, first, n, b0, 0);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(eigen_metrics_kernel, dim3(grid), dim3(NT), 0, s, gt, gt_len, depth, depth_len, px0, t, ratio, partials);
    hipLaunchKernelGGL(eigen_metrics_finalize_kernel, dim3(n), dim3(NT), 0, s, (const float*)partials, grid, t, errors);
    return check_launch("dmh_eigen_metrics");
}

}  // extern "C"
