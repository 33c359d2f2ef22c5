// K39 -- pseudo-LiDAR: depth / disparity maps (or the network's output) to velodyne-frame point clouds,
// preprocessing/generate_lidar.py:10-33 with preprocessing/kitti_util.py:159-175 (Calibration.project_image_to_velo), for a batch of
// frames that each have their own size and calibration, float32-equal to the reference (gfx950).
//
// The reference, per frame, builds a meshgrid, a [3, N] float64 stack, two np.dot and a boolean gather on the host.  Per pixel it
// is a dozen float64 operations and a stream compaction that keeps the row-major pixel order.
//
// What is computed (ops.pseudo_lidar_host is the same arithmetic in numpy, element by element), u the column, v the row:
//   d:  depth form   (double)src;                                             every pixel is a candidate
//       disp form    s = src < 0 ? 0 : src, mask = s > 0, d = (f_u * 0.54) / (((double)s + 1.) - mask); only masked pixels
//       net form     the sigmoid output [n][h][w]: tap = 0.01f + 9.99f * src (layers.disp_to_depth(., 0.1, 100) in fp32), the
//                    bilinear resize to (H, W) with K25's lin_axis arithmetic (csrc/eigen_eval.hip), fp32 products and sums
//                    unfused, depth = (1.f / disp) * 5.4f clamped to [1e-3, 80] (a NaN stays), with quantise
//                    float(uint16(depth * 256.f)) / 256.f (a NaN becomes 0), d = (double)depth;  every pixel is a candidate
//   x = ((u - c_u) * d) / f_u + b_x;  y = ((v - c_v) * d) / f_v + b_y;  z = d
//   r_i = (Ri[i][0] x + Ri[i][1] y) + Ri[i][2] z
//   o_i = ((C[i][0] r_0 + C[i][1] r_1) + C[i][2] r_2) + C[i][3]
//   valid = o_0 >= 0 && o_2 < max_high (a NaN is invalid);  row = (float)o_0, (float)o_1, (float)o_2, 1.f
// in float64 without contraction, IEEE division.  calib: 27 doubles per frame = f_u f_v c_u c_v b_x b_y, Ri[9], C[12]; the host
// inverts, the kernel never does.
//
// Launch plan: stream compaction in three launches, no atomics, no host read.
//   1. count: a workgroup owns one tile of TILE consecutive candidate pixels of ONE frame (tile_frame[block] names the frame, as
//      K25's blk_img does).  Pixel tile_base + it * NT + thread: ascending in (iteration, wave, lane).  Every wave counts its
//      valid lanes with __popcll(__ballot()) -- 64 bits wide here -- and the workgroup stores its count.
//   2. scan: ONE workgroup makes the exclusive integer prefix of the tile counts; offsets[f] is the prefix at frame f's first
//      tile, offsets[n] the total.
//   3. write: recomputes the chain (the same code: the same validity), ranks a valid lane by __popcll(ballot & lanes_below) on
//      top of the counts of the (iteration, wave) pairs before it in LDS and the tile's prefix, and stores the row as one float4.
// Recomputing costs a dozen float64 operations a pixel; a validity bitmask left by pass 1 would save none of them, since the
// values of the valid rows are needed either way.  Every index derived from a table is checked before use.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int ITERS = DMH_LIDAR_TILE / NT;
constexpr int TILE = DMH_LIDAR_TILE;
constexpr int NW = NT / WAVE;
constexpr int SCAN_NT = 1024;
constexpr int CAL = DMH_LIDAR_CALIB;
enum { FORM_DEPTH = DMH_LIDAR_DEPTH, FORM_DISP = DMH_LIDAR_DISP, FORM_NET = DMH_LIDAR_NET };

static_assert(TILE % NT == 0 && NT % WAVE == 0, "a tile is whole iterations of whole waves");

struct Source {
    const float* src;
    int64_t src_len;
    int h, w;               // net form: the size of the network's output
    int quantise;
};

struct Tile {
    int f;                  // frame, -1: nothing to do
    int H, W;
    int64_t off;            // depth / disp: the frame's first element in src; net: f * h * w
    int p0, p1;             // the tile's pixels of the frame
};

// desc: int32 [n][4] = H, W, the frame's first element in src (depth / disp; a frame of the net form starts at f h w), its first
// tile.  A record that points outside src leaves the tile empty.
template <int FORM>
__device__ __forceinline__ Tile load_tile(const int32_t* __restrict__ desc, const int32_t* __restrict__ tile_frame, int n, int n_tiles,
                                          const Source& s) {
    Tile t;
    t.f = -1;
    t.H = t.W = t.p0 = t.p1 = 0;
    t.off = 0;
    const int b = (int)blockIdx.x;
    if (b >= n_tiles) return t;
    const int f = tile_frame[b];
    if (f < 0 || f >= n) return t;
    const int H = desc[f * 4 + 0], W = desc[f * 4 + 1], c = b - desc[f * 4 + 3];
    const int64_t off = FORM == FORM_NET ? (int64_t)f * s.h * s.w : (int64_t)desc[f * 4 + 2];
    if (H <= 0 || W <= 0 || c < 0 || off < 0) return t;
    const int64_t npx = (int64_t)H * W, p0 = (int64_t)c * TILE;
    if (npx >= (1ll << 31) || p0 >= npx) return t;
    if (off + (FORM == FORM_NET ? (int64_t)s.h * s.w : npx) > s.src_len) return t;
    t.f = f; t.H = H; t.W = W; t.off = off;
    t.p0 = (int)p0;
    t.p1 = (int)(p0 + TILE < npx ? p0 + TILE : npx);
    return t;
}

// K25's lin_axis (csrc/eigen_eval.hip): OpenCV's INTER_LINEAR coordinate of one axis
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

// layers.disp_to_depth(., 0.1, 100) as torch evaluates it in fp32: min_disp + (max_disp - min_disp) * disp
__device__ __forceinline__ float scaled_tap(const float* __restrict__ l, int w, int yy, int xx) {
#pragma clang fp contract(off)
    constexpr float MIN_DISP = (float)(1.0 / 100.0), RANGE = (float)(1.0 / 0.1 - 1.0 / 100.0);
    const float prod = RANGE * l[yy * w + xx];
    return MIN_DISP + prod;
}

__device__ __forceinline__ float net_depth(const Source& s, const Tile& t, int y, int x) {
#pragma clang fp contract(off)
    const double sx = (double)s.w / (double)t.W, sy = (double)s.h / (double)t.H;
    const float* l = s.src + t.off;
    int xa, xb, ya, yb;
    float fx, fy;
    lin_axis(x, sx, s.w, xa, xb, fx);
    lin_axis(y, sy, s.h, ya, yb, fy);
    const float a0 = 1.f - fx, a1 = fx, b0 = 1.f - fy, b1 = fy;
    const float t00 = a0 * scaled_tap(l, s.w, ya, xa), t01 = a1 * scaled_tap(l, s.w, ya, xb);
    const float t10 = a0 * scaled_tap(l, s.w, yb, xa), t11 = a1 * scaled_tap(l, s.w, yb, xb);
    const float r0 = t00 + t01, r1 = t10 + t11;
    const float m0 = b0 * r0, m1 = b1 * r1;
    const float disp = m0 + m1;
    const float inv = 1.f / disp;
    float depth = inv * 5.4f;
    depth = depth < 1e-3f ? 1e-3f : depth;          // evaluate's clamp (a NaN stays)
    depth = depth > 80.f ? 80.f : depth;
    if (s.quantise) {                               // the 16-bit PNG round trip: depth <= 80, so depth * 256 fits 16 bits
        const float q = depth * 256.f;
        const uint32_t k = q == q ? ((uint32_t)(int)q & 0xffffu) : 0u;
        depth = (float)k / 256.f;
    }
    return depth;
}

// the candidate test and d of pixel p of the tile's frame
template <int FORM>
__device__ __forceinline__ bool candidate(const Source& s, const Tile& t, const double* __restrict__ cal, int y, int x, int p, double& d) {
#pragma clang fp contract(off)
    if (FORM == FORM_NET) {
        d = (double)net_depth(s, t, y, x);
        return true;
    }
    const float v = s.src[t.off + p];
    if (FORM == FORM_DEPTH) {
        d = (double)v;
        return true;
    }
    const float c = v < 0.f ? 0.f : v;              // disp[disp < 0] = 0 (a NaN stays and fails the mask)
    const bool mask = c > 0.f;
    const double num = cal[0] * 0.54;
    const double den = ((double)c + 1.0) - (mask ? 1.0 : 0.0);
    d = __ddiv_rn(num, den);
    return mask;
}

// project_image_to_velo of one candidate; returns the validity test of generate_lidar.py:22
__device__ __forceinline__ bool to_velo(const double* __restrict__ cal, int u, int v, double d, double max_high, float4& row) {
#pragma clang fp contract(off)
    const double f_u = cal[0], f_v = cal[1], c_u = cal[2], c_v = cal[3], b_x = cal[4], b_y = cal[5];
    const double* Ri = cal + 6;
    const double* Cm = cal + 15;
    const double du = (double)u - c_u, dv = (double)v - c_v;
    const double xn = du * d, yn = dv * d;
    const double x = __ddiv_rn(xn, f_u) + b_x;
    const double y = __ddiv_rn(yn, f_v) + b_y;
    const double z = d;
    double r[3], o[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = Ri[i * 3 + 0] * x, b = Ri[i * 3 + 1] * y, c = Ri[i * 3 + 2] * z;
        const double ab = a + b;
        r[i] = ab + c;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = Cm[i * 4 + 0] * r[0], b = Cm[i * 4 + 1] * r[1], c = Cm[i * 4 + 2] * r[2];
        const double ab = a + b;
        const double abc = ab + c;
        o[i] = abc + Cm[i * 4 + 3];
    }
    row = make_float4((float)o[0], (float)o[1], (float)o[2], 1.f);
    return o[0] >= 0.0 && o[2] < max_high;          // a NaN fails either comparison
}

// WRITE = false: pass 1, counts[block] = the tile's valid candidates.  WRITE = true: pass 3, the rows at their ranks.
template <int FORM, bool WRITE>
__global__ __launch_bounds__(NT) void pseudo_lidar_kernel(Source s, const double* __restrict__ calib, const int32_t* __restrict__ desc,
                                                          const int32_t* __restrict__ tile_frame, int n, int n_tiles, double max_high,
                                                          int32_t* __restrict__ counts, const int32_t* __restrict__ tile_off,
                                                          float4* __restrict__ out, int64_t cap) {
    __shared__ int s_cnt[ITERS * NW];
    const Tile t = load_tile<FORM>(desc, tile_frame, n, n_tiles, s);      // uniform over the workgroup
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const double* cal = calib + (int64_t)(t.f < 0 ? 0 : t.f) * CAL;
    float4 rows[ITERS];
    unsigned long long votes[ITERS];
    bool ok[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int p = t.p0 + it * NT + (int)threadIdx.x;
        bool valid = false;
        rows[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t.f >= 0 && p < t.p1) {
            const int y = p / t.W, x = p - y * t.W;
            double d;
            if (candidate<FORM>(s, t, cal, y, x, p, d)) valid = to_velo(cal, x, y, d, max_high, rows[it]);
        }
        const unsigned long long vote = __ballot(valid);                  // 64 lanes
        if (lane == 0) s_cnt[it * NW + wave] = __popcll(vote);
        votes[it] = vote;
        ok[it] = valid;
    }
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) {
            int total = 0;
#pragma unroll
            for (int i = 0; i < ITERS * NW; ++i) total += s_cnt[i];
            counts[blockIdx.x] = total;
        }
        return;
    }
    if (t.f < 0) return;
    const int64_t tile_base = tile_off[blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    int before = 0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int slot = it * NW + wave;
        // the counts of the (iteration, wave) pairs before this one
        for (int i = (it == 0 ? 0 : (it - 1) * NW + wave); i < slot; ++i) before += s_cnt[i];
        if (ok[it]) {
            const int64_t at = tile_base + before + __popcll(votes[it] & below);
            if (at >= 0 && at < cap) out[at] = rows[it];
        }
    }
}

// One workgroup: tile_off = the exclusive prefix of counts; offsets[f] = tile_off[first tile of f] (the total for a frame without
// tiles at the end), offsets[n] = the total.  Thread t sums the entries [t per, (t + 1) per), a Hillis-Steele scan joins the sums.
__global__ __launch_bounds__(SCAN_NT) void pseudo_lidar_scan_kernel(const int32_t* __restrict__ counts, int n_tiles,
                                                                    const int32_t* __restrict__ desc, int n, int32_t* __restrict__ tile_off,
                                                                    int64_t* __restrict__ offsets) {
    __shared__ int s_sum[SCAN_NT];
    const int tid = threadIdx.x;
    const int per = (n_tiles + SCAN_NT - 1) / SCAN_NT;
    const int lo = min(tid * per, n_tiles), hi = min(lo + per, n_tiles);
    int mine = 0;
    for (int i = lo; i < hi; ++i) mine += max(counts[i], 0);
    s_sum[tid] = mine;
    __syncthreads();
    for (int o = 1; o < SCAN_NT; o <<= 1) {
        const int add = tid >= o ? s_sum[tid - o] : 0;
        __syncthreads();
        s_sum[tid] += add;
        __syncthreads();
    }
    int run = s_sum[tid] - mine;
    for (int i = lo; i < hi; ++i) {
        tile_off[i] = run;
        run += max(counts[i], 0);
    }
    const int total = s_sum[SCAN_NT - 1];
    __syncthreads();                                // tile_off is read below by other threads of this workgroup
    for (int f = tid; f <= n; f += SCAN_NT) {
        int v = total;
        if (f < n) {
            const int first = desc[f * 4 + 3];
            if (first >= 0 && first < n_tiles) v = tile_off[first];
        }
        offsets[f] = (int64_t)v;
    }
}

template <int FORM>
void launch_form(const Source& s, const double* calib, const int32_t* desc, const int32_t* tile_frame, int n, int n_tiles, double max_high,
                 int32_t* ws, float* out, int64_t cap, int64_t* offsets, hipStream_t st) {
    int32_t* counts = ws;
    int32_t* tile_off = ws + n_tiles;
    if (n_tiles > 0)
        hipLaunchKernelGGL((pseudo_lidar_kernel<FORM, false>), dim3(n_tiles), dim3(NT), 0, st, s, calib, desc, tile_frame, n, n_tiles, max_high,
                           counts, (const int32_t*)tile_off, (float4*)out, cap);
    hipLaunchKernelGGL(pseudo_lidar_scan_kernel, dim3(1), dim3(SCAN_NT), 0, st, (const int32_t*)counts, n_tiles, desc, n, tile_off, offsets);
    if (n_tiles > 0)
        hipLaunchKernelGGL((pseudo_lidar_kernel<FORM, true>), dim3(n_tiles), dim3(NT), 0, st, s, calib, desc, tile_frame, n, n_tiles, max_high,
                           counts, (const int32_t*)tile_off, (float4*)out, cap);
}

}  // namespace

extern "C" {

int dmh_pseudo_lidar(const float* src, int64_t src_len, int form, int h, int w, int quantise, const double* calib, const int32_t* desc,
                     const int32_t* tile_frame, int n, int n_tiles, double max_high, int32_t* ws, float* out, int64_t cap,
                     int64_t* offsets, void* stream) {
    DMH_REQUIRE(calib && desc && offsets, "null pointer");
    DMH_REQUIRE(form == FORM_DEPTH || form == FORM_DISP || form == FORM_NET, "form must be DMH_LIDAR_DEPTH, _DISP or _NET");
    DMH_REQUIRE(n > 0 && n <= (1 << 20), "need 0 < n <= 2^20 frames");
    DMH_REQUIRE(n_tiles >= 0 && n_tiles <= (1 << 21), "need 0 <= n_tiles <= 2^21");
    DMH_REQUIRE(cap >= 0 && cap <= (int64_t)n_tiles * TILE && cap < (1ll << 31), "need 0 <= cap <= n_tiles * DMH_LIDAR_TILE, cap < 2^31");
    DMH_REQUIRE(src_len >= 0 && src_len < (1ll << 31), "need 0 <= src_len < 2^31");
    DMH_REQUIRE(n_tiles == 0 || (src && tile_frame && ws && out), "null pointer");
    if (form == FORM_NET) {
        DMH_REQUIRE(h > 0 && w > 0 && (int64_t)n * h * w == src_len, "the net form reads [n][h][w]: src_len must be n h w");
    } else {
        DMH_REQUIRE(h == 0 && w == 0 && quantise == 0, "h, w and quantise belong to the net form");
    }
    DMH_REQUIRE(max_high == max_high, "max_high is NaN");
    DMH_REQUIRE(((uintptr_t)out & 15) == 0 && ((uintptr_t)calib & 7) == 0 && ((uintptr_t)offsets & 7) == 0,
                "out must be 16-byte, calib and offsets 8-byte aligned");
    DMH_REQUIRE(((uintptr_t)src & 3) == 0 && ((uintptr_t)desc & 3) == 0 && ((uintptr_t)tile_frame & 3) == 0 && ((uintptr_t)ws & 3) == 0,
                "src, desc, tile_frame and ws must be 4-byte aligned");
    DMH_REQUIRE((const void*)out != (const void*)src && (const void*)out != (const void*)ws, "out must not alias src or ws");
    Source s;
    s.src = src; s.src_len = src_len; s.h = h; s.w = w; s.quantise = quantise != 0;
    const hipStream_t st = (hipStream_t)stream;
    if (form == FORM_DEPTH) launch_form<FORM_DEPTH>(s, calib, desc, tile_frame, n, n_tiles, max_high, ws, out, cap, offsets, st);
    else if (form == FORM_DISP) launch_form<FORM_DISP>(s, calib, desc, tile_frame, n, n_tiles, max_high, ws, out, cap, offsets, st);
    else launch_form<FORM_NET>(s, calib, desc, tile_frame, n, n_tiles, max_high, ws, out, cap, offsets, st);
    return check_launch("dmh_pseudo_lidar");
}

}  // extern "C"
