// K38 -- backward of ManyDepth's matching cost volume (gfx950).  This project's addition: the reference computes the volume under
// torch.no_grad() (manydepth2/networks/resnet_encoder.py:283-300) and has no such gradient.
//
// The function differentiated is reduce_conv's input, V[b][d][h][w] = cost_volume[b][d][h][w] * confidence[b][h][w], as torch
// autograd differentiates the module expression of it: the sample positions, the edge and border masks, counts, missing and
// confidence are constants.  confidence == 1 means all D bins were observed, so nothing is "missing" there and set_missing_to_max
// contributes nothing; only confident columns carry gradient.  With the upstream gradient g[b][d][h][w], in a confident column
//
//   dtotal[d]            = g[d] / (counts[d] + 1e-7)
//   d current[c]         = -(1/64) sum_{d, l} dtotal[d] edge_l[d] sgn(warped_l[c][d] - current[c])          sgn(0) = 0
//   d warped_l[c][d]     =  (1/64) dtotal[d] edge_l[d] sgn(...)             spread onto lookup[b][l][c] by the four bilinear weights
//
// A sample whose edge flag is 1 has all four taps inside the map; one whose flag is 0 (outside, non-finite position, masked
// border of the current frame) contributes nothing.  A lookup whose pose sums to exactly 0, or of a sample b >= Bp, is skipped on
// the device: its d lookup is exact zeros.
//
// Launches (all on `stream`, no host read: capturable).
//   0  (memset of the accumulators and of the word that receives max|dtotal|; only when d_lookup is asked for)
//   1  cost_volume_nhwc_kernel   K30's transposing pass: lookup -> channels-last
//   2  cvb_dtotal_kernel         K30's matching loop again (same tiles, same lanes, same position arithmetic, so every edge flag,
//                                count and confidence is the forward's); writes dtotal [B][D][H][W] (zeros outside confident
//                                columns) and the maximum of |dtotal| (an integer atomic max on the bits of a non-negative float)
//   3  cvb_grad_kernel           per column: samples every (lookup, bin) once more, sums d current in registers in the fixed order
//                                (l, d) and stores it; adds every tap's share of d lookup to a 64-bit fixed-point accumulator
//                                (the shares of consecutive bins that fall into the same quad of taps are added in registers first)
//   4  cvb_finish_kernel         accumulators [B][L][H][W][64] int64 -> d_lookup [B][L][64][H][W] float
//
// Determinism.  d_current is a gather.  d_lookup is a scatter (a lookup texel is hit by an unknown number of columns and bins);
// it is accumulated in 64-bit fixed point with integer vector atomics (global_atomic_add_x2), whose sum does not depend on the
// order, so two runs give the same bits.  No float atomics.  The scale is 2^k with k = 68 - n - e taken on the device, where
// max|dtotal| < 2^e and H W D <= 2^n: one contribution is |dtotal| / 64 times a weight <= 1, i.e. below 2^(e-6), so it is below
// 2^(62-n) in fixed point, and the at most H W D contributions to one texel, each rounded by at most 1/2, stay below 2^63.  Error:
// each contribution is rounded once to a multiple of 2^-k = 2^(n+e-68) <= max|dtotal| * 2^(n-67); a texel that receives m
// contributions is off by at most m * 2^(n+e-69) before the one final rounding to float (at 80 x 256, D = 96: n = 21, so below
// m * 2^-47 max|dtotal|).  g must be finite.
#include "cost_volume_pos.hpp"

using namespace dmh;

namespace {

// the shift k of the fixed-point scale 2^k from the bits of max|dtotal| and N = H W D
__device__ __forceinline__ int fixed_shift(unsigned maxbits, long long N) {
    const float M = __uint_as_float(maxbits);
    if (!(M > 0.f) || !(M < 3.0e38f)) return 0;        // nothing to add, or a non-finite g (the result is then meaningless)
    const int e = ilogbf(M) + 1;
    const int n = N > 1 ? 64 - __clzll(N - 1) : 0;
    return 68 - n - e;
}

__global__ __launch_bounds__(NT) void cvb_dtotal_kernel(const float* __restrict__ cur, const float* __restrict__ look,
                                                        const float* __restrict__ poses, const float* __restrict__ K,
                                                        const float* __restrict__ invK, const float* __restrict__ bins, int B, int L,
                                                        int Bp, int H, int W, int D, const float* __restrict__ g_up, int64_t g_bstride,
                                                        float* __restrict__ dtotal, unsigned* __restrict__ maxword) {
    __shared__ float s_cost[TILE * DP];
    __shared__ float s_cnt[TILE * DP];
    __shared__ float s_P[MAX_L][12];
    __shared__ int s_skip[MAX_L];
    __shared__ float s_conf[TILE];
    __shared__ float s_wmax[NT / 64];

    const int tilesW = (W + TILE - 1) / TILE;
    const int id = blockIdx.x;
    const int tw = id % tilesW, h = (id / tilesW) % H, b = id / (tilesW * H);
    const int w0 = tw * TILE;
    const int grp = threadIdx.x / GL, lane = threadIdx.x & (GL - 1);
    const int HW = H * W;

    if (threadIdx.x < L) {
        const int l = threadIdx.x;
        int skip = 1;
        if (b < Bp) {
            const float* __restrict__ T = poses + ((int64_t)b * L + l) * 16;
            float s = 0.f;
            for (int i = 0; i < 16; ++i) s += T[i];
            skip = s == 0.f;
            float P[12];
            project_matrix(K + (int64_t)b * 16, T, P);
            for (int i = 0; i < 12; ++i) s_P[l][i] = P[i];
        }
        s_skip[l] = skip;
    }
    __syncthreads();

    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float* __restrict__ iK = invK + (int64_t)b * 16;

    // K30's matching loop, character for character (tests/test_cost_volume_bwd_ref.py compares the two texts; sharing it as a
    // device function changes K30's register allocation and schedule); the count of positive diffs is kept beside the cost
    for (int pp = 0; pp < TILE / (NT / GL); ++pp) {
        const int px = grp + pp * (NT / GL), w = w0 + px;
        if (w >= W) continue;                                           // (uniform over the group)
        const bool interior = h >= 2 && h < H - 2 && w >= 2 && w < W - 2;
        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (interior) {
            const float* __restrict__ cp = cur + ((int64_t)b * CH + 4 * lane) * HW + (int64_t)h * W + w;
            c4 = make_float4(cp[0], cp[HW], cp[2 * (int64_t)HW], cp[3 * (int64_t)HW]);
            back_project(iK, (float)w, (float)h, cx, cy, cz);
        }
        for (int d0 = 0; d0 < D; d0 += GL) {
            const int d = d0 + lane;
            float sum = 0.f, cnt = 0.f;
            if (interior) {
                const float depth = d < D ? bins[d] : 1.0f;
                for (int l = 0; l < L; ++l) {
                    if (s_skip[l]) continue;
                    float P[12];
#pragma unroll
                    for (int i = 0; i < 12; ++i) P[i] = s_P[l][i];
                    float ix, iy;
                    sample_pos(P, cx, cy, cz, depth, wm1, hm1, ix, iy);
                    if (d >= D) ix = -1.0f;
                    const float* __restrict__ lk = look + ((int64_t)b * L + l) * HW * CH + 4 * lane;
                    float p[GL];
#pragma unroll
                    for (int j = 0; j < GL; ++j) {
                        const float x = __shfl(ix, j, GL), y = __shfl(iy, j, GL);
                        p[j] = 0.f;
                        if (x >= 0.f) {
                            const float x0f = floorf(x), y0f = floorf(y);
                            const float wx1 = x - x0f, wx0 = (x0f + 1.0f) - x, wy1 = y - y0f, wy0 = (y0f + 1.0f) - y;
                            const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
                            const int x0 = min(max((int)x0f, 0), W - 2), y0 = min(max((int)y0f, 0), H - 2);
                            const float* __restrict__ t0 = lk + ((int64_t)y0 * W + x0) * CH;
                            const float4 a = *reinterpret_cast<const float4*>(t0);
                            const float4 e = *reinterpret_cast<const float4*>(t0 + CH);
                            const float4 f = *reinterpret_cast<const float4*>(t0 + (int64_t)W * CH);
                            const float4 g = *reinterpret_cast<const float4*>(t0 + (int64_t)W * CH + CH);
                            const float vx = a.x * nw + e.x * ne + f.x * sw + g.x * se;
                            const float vy = a.y * nw + e.y * ne + f.y * sw + g.y * se;
                            const float vz = a.z * nw + e.z * ne + f.z * sw + g.z * se;
                            const float vw = a.w * nw + e.w * ne + f.w * sw + g.w * se;
                            p[j] = (fabsf(vx - c4.x) + fabsf(vy - c4.y)) + (fabsf(vz - c4.z) + fabsf(vw - c4.w));
                        }
                    }
                    // halving exchange: after the four steps p[0] of lane j is the sum over the 16 lanes of their p[j]
#pragma unroll
                    for (int s = GL / 2; s >= 1; s >>= 1) {
                        const bool up = (lane & s) != 0;
#pragma unroll
                        for (int i = 0; i < GL / 2; ++i)
                            if (i < s) {
                                const float send = up ? p[i] : p[i + s], keep = up ? p[i + s] : p[i];
                                p[i] = keep + __shfl_xor(send, s, GL);
                            }
                    }
                    const float diff = p[0] * (1.0f / CH);              // mean over the channels (times the edge flag, 1 here)
                    sum += diff;
                    cnt += diff > 0.f ? 1.0f : 0.f;
                }
            }
            if (d < D) {
                s_cost[px * DP + d] = sum / (cnt + 1e-7f);
                s_cnt[px * DP + d] = cnt;
            }
        }
    }
    __syncthreads();

    // confidence: all D bins observed
    for (int pp = 0; pp < TILE / (NT / GL); ++pp) {
        const int px = grp + pp * (NT / GL), w = w0 + px;
        if (w >= W) continue;
        int pos = 0;
        for (int d = lane; d < D; d += GL) pos += s_cost[px * DP + d] > 0.f;
#pragma unroll
        for (int s = GL / 2; s >= 1; s >>= 1) pos += __shfl_xor(pos, s, GL);
        if (lane == 0) s_conf[px] = pos == D ? 1.0f : 0.f;
    }
    __syncthreads();

    float mx = 0.f;
    for (int i = threadIdx.x; i < D * TILE; i += NT) {
        const int d = i / TILE, px = i - d * TILE, w = w0 + px;
        if (w >= W) continue;
        const int64_t pix = (int64_t)h * W + w;
        float dt = 0.f;
        if (s_conf[px] != 0.f) dt = g_up[(int64_t)b * g_bstride + (int64_t)d * HW + pix] / (s_cnt[px * DP + d] + 1e-7f);
        dtotal[((int64_t)b * D + d) * HW + pix] = dt;
        mx = fmaxf(mx, fabsf(dt));
    }
    if (maxword) {
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s, 64));
        if ((threadIdx.x & 63) == 0) s_wmax[threadIdx.x >> 6] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < NT / 64; ++i) mx = fmaxf(mx, s_wmax[i]);
            if (mx > 0.f) atomicMax(maxword, __float_as_uint(mx));     // non-negative floats order as their bits
        }
    }
}

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// The pending shares of one quad of taps (4 taps x the lane's 4 channels, fixed point) go to the accumulators; zeros are not sent.
// Neighbouring depth bins of a column mostly fall into the same quad, so their shares are added here, in registers, first:
// integer sums, so the grouping changes no bit of the result.
__device__ __forceinline__ void flush_quad(long long* __restrict__ acc, int64_t o, int W, long long* pend) {
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {
        long long* __restrict__ a = acc + o + (tp & 1) * CH + (tp >> 1) * (int64_t)W * CH;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (pend[tp * 4 + k] != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a + k), (unsigned long long)pend[tp * 4 + k]);
            pend[tp * 4 + k] = 0;
        }
    }
}

__global__ __launch_bounds__(NT) void cvb_grad_kernel(const float* __restrict__ cur, const float* __restrict__ look,
                                                      const float* __restrict__ poses, const float* __restrict__ K,
                                                      const float* __restrict__ invK, const float* __restrict__ bins, int B, int L,
                                                      int Bp, int H, int W, int D, const float* __restrict__ dtotal,
                                                      float* __restrict__ d_current, long long* __restrict__ acc,
                                                      const unsigned* __restrict__ maxword) {
    __shared__ float s_P[MAX_L][12];
    __shared__ int s_skip[MAX_L];

    const int tilesW = (W + TILE - 1) / TILE;
    const int id = blockIdx.x;
    const int tw = id % tilesW, h = (id / tilesW) % H, b = id / (tilesW * H);
    const int w0 = tw * TILE;
    const int grp = threadIdx.x / GL, lane = threadIdx.x & (GL - 1);
    const int HW = H * W;

    if (threadIdx.x < L) {
        const int l = threadIdx.x;
        int skip = 1;
        if (b < Bp) {
            const float* __restrict__ T = poses + ((int64_t)b * L + l) * 16;
            float s = 0.f;
            for (int i = 0; i < 16; ++i) s += T[i];
            skip = s == 0.f;
            float P[12];
            project_matrix(K + (int64_t)b * 16, T, P);
            for (int i = 0; i < 12; ++i) s_P[l][i] = P[i];
        }
        s_skip[l] = skip;
    }
    __syncthreads();

    const double scale = acc ? ldexp(1.0, fixed_shift(*maxword, (long long)HW * D)) : 0.0;
    const float wm1 = (float)(W - 1), hm1 = (float)(H - 1);
    const float* __restrict__ iK = invK + (int64_t)b * 16;

    for (int pp = 0; pp < TILE / (NT / GL); ++pp) {
        const int px = grp + pp * (NT / GL), w = w0 + px;
        if (w >= W) continue;                                           // (uniform over the group)
        const bool interior = h >= 2 && h < H - 2 && w >= 2 && w < W - 2;
        const int64_t pix = (int64_t)h * W + w;
        float4 c4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 gc = make_float4(0.f, 0.f, 0.f, 0.f);
        float cx = 0.f, cy = 0.f, cz = 0.f;
        if (interior) {
            const float* __restrict__ cp = cur + ((int64_t)b * CH + 4 * lane) * HW + pix;
            c4 = make_float4(cp[0], cp[HW], cp[2 * (int64_t)HW], cp[3 * (int64_t)HW]);
            back_project(iK, (float)w, (float)h, cx, cy, cz);
            long long pend[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) pend[i] = 0;
            int64_t pend_o = -1;
            for (int l = 0; l < L; ++l) {
                if (s_skip[l]) continue;
                float P[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) P[i] = s_P[l][i];
                const int64_t lbase = ((int64_t)b * L + l) * HW * CH + 4 * lane;
                for (int d0 = 0; d0 < D; d0 += GL) {
                    const int d = d0 + lane;
                    const float dt = d < D ? dtotal[((int64_t)b * D + d) * HW + pix] : 0.f;
                    int any = dt != 0.f;
#pragma unroll
                    for (int s = GL / 2; s >= 1; s >>= 1) any |= __shfl_xor(any, s, GL);
                    if (!any) continue;                                 // a column without confidence: nothing to do
                    const float depth = d < D ? bins[d] : 1.0f;
                    float ix, iy;
                    sample_pos(P, cx, cy, cz, depth, wm1, hm1, ix, iy);
                    if (d >= D) ix = -1.0f;
#pragma unroll 1
                    for (int j = 0; j < GL; ++j) {
                        const float x = __shfl(ix, j, GL), y = __shfl(iy, j, GL), t = __shfl(dt, j, GL);
                        if (x >= 0.f && t != 0.f) {
                            const float x0f = floorf(x), y0f = floorf(y);
                            const float wx1 = x - x0f, wx0 = (x0f + 1.0f) - x, wy1 = y - y0f, wy0 = (y0f + 1.0f) - y;
                            const float nw = wx0 * wy0, ne = wx1 * wy0, sw = wx0 * wy1, se = wx1 * wy1;
                            const int x0 = min(max((int)x0f, 0), W - 2), y0 = min(max((int)y0f, 0), H - 2);
                            const int64_t o = lbase + ((int64_t)y0 * W + x0) * CH;
                            const float* __restrict__ t0 = look + o;
                            const float4 a = *reinterpret_cast<const float4*>(t0);
                            const float4 e = *reinterpret_cast<const float4*>(t0 + CH);
                            const float4 f = *reinterpret_cast<const float4*>(t0 + (int64_t)W * CH);
                            const float4 q = *reinterpret_cast<const float4*>(t0 + (int64_t)W * CH + CH);
                            const float vx = a.x * nw + e.x * ne + f.x * sw + q.x * se;
                            const float vy = a.y * nw + e.y * ne + f.y * sw + q.y * se;
                            const float vz = a.z * nw + e.z * ne + f.z * sw + q.z * se;
                            const float vw = a.w * nw + e.w * ne + f.w * sw + q.w * se;
                            // t * sgn is +-t or 0, and the division by 64 is exact: the only roundings are the sum's and the weight's
                            const float tx = t * sgn(vx - c4.x), ty = t * sgn(vy - c4.y), tz = t * sgn(vz - c4.z), tw_ = t * sgn(vw - c4.w);
                            gc.x += tx;
                            gc.y += ty;
                            gc.z += tz;
                            gc.w += tw_;
                            if (acc) {
                                if (o != pend_o) {                      // another quad of taps: send what is pending
                                    if (pend_o >= 0) flush_quad(acc, pend_o, W, pend);
                                    pend_o = o;
                                }
                                const float k = 1.0f / CH;
                                const float tt[4] = {tx * k, ty * k, tz * k, tw_ * k}, wq[4] = {nw, ne, sw, se};
#pragma unroll
                                for (int tp = 0; tp < 4; ++tp)
#pragma unroll
                                    for (int c = 0; c < 4; ++c) pend[tp * 4 + c] += __double2ll_rn((double)(tt[c] * wq[tp]) * scale);
                            }
                        }
                    }
                }
            }
            if (acc && pend_o >= 0) flush_quad(acc, pend_o, W, pend);
        }
        if (d_current) {
            float* __restrict__ gp = d_current + ((int64_t)b * CH + 4 * lane) * HW + pix;
            const float k = -1.0f / CH;
            gp[0] = gc.x * k;
            gp[HW] = gc.y * k;
            gp[2 * (int64_t)HW] = gc.z * k;
            gp[3 * (int64_t)HW] = gc.w * k;
        }
    }
}

// accumulators [N][HW][64] (fixed point) -> d_lookup [N][64][HW] (float), 64 x 64 tiles through LDS
__global__ __launch_bounds__(NT) void cvb_finish_kernel(const long long* __restrict__ acc, float* __restrict__ y, int HW, int tiles,
                                                        long long ND, const unsigned* __restrict__ maxword) {
    __shared__ float t[CH][CH + 1];
    const int n = blockIdx.x / tiles, p0 = (blockIdx.x - n * tiles) * 64;
    const long long* __restrict__ src = acc + (int64_t)n * CH * HW;
    float* __restrict__ dst = y + (int64_t)n * CH * HW;
    const int lo = threadIdx.x & 63, hi = threadIdx.x >> 6;
    const double inv = ldexp(1.0, -fixed_shift(*maxword, ND));
#pragma unroll 4
    for (int p = hi; p < 64; p += 4)
        if (p0 + p < HW) t[p][lo] = (float)((double)src[(int64_t)(p0 + p) * CH + lo] * inv);
    __syncthreads();
    if (p0 + lo < HW) {
#pragma unroll 4
        for (int c = hi; c < CH; c += 4) dst[(int64_t)c * HW + p0 + lo] = t[lo][c];
    }
}

}  // namespace

extern "C" {

int dmh_cost_volume_bwd(const float* current, const float* lookup, const float* poses, const float* K, const float* invK,
                        const float* bins, int B, int L, int Bp, int C, int H, int W, int D, const float* g, int64_t g_batch_stride,
                        float* nhwc, float* dtotal, int64_t* acc, float* d_current, float* d_lookup, void* stream) {
    DMH_REQUIRE(current && lookup && poses && K && invK && bins && g && nhwc && dtotal, "null pointer");
    DMH_REQUIRE(d_current || d_lookup, "need d_current or d_lookup");
    DMH_REQUIRE(!d_lookup || acc, "d_lookup needs the accumulator workspace");
    DMH_REQUIRE(B > 0 && L > 0 && L <= MAX_L, "need B > 0 and 1 <= L <= 16");
    DMH_REQUIRE(Bp >= 1 && Bp <= B, "need 1 <= Bp <= B (rows of poses)");
    DMH_REQUIRE(C == CH, "need C = 64 (the layer-1 width of ResNet-18/34)");
    DMH_REQUIRE(D >= 1 && D <= MAX_D, "need 1 <= D <= 128");
    DMH_REQUIRE(H >= 5 && W >= 5, "need H, W >= 5");
    DMH_REQUIRE((int64_t)H * W * CH < (1ll << 31), "need H * W * 64 < 2^31");
    DMH_REQUIRE(g_batch_stride >= (int64_t)D * H * W, "need g_batch_stride >= D * H * W");
    const int64_t tiles = (int64_t)B * H * ((W + TILE - 1) / TILE);
    const int ttiles = (H * W + 63) / 64;
    DMH_REQUIRE(tiles < (1ll << 31) && (int64_t)B * L * ttiles < (1ll << 31), "need fewer than 2^31 tiles");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_acc = (int64_t)B * L * H * W * CH;
    unsigned* maxword = nullptr;
    if (d_lookup) {
        // the accumulators and, behind them, the word that receives max|dtotal|
        if (hipMemsetAsync(acc, 0, (size_t)(n_acc + 1) * sizeof(int64_t), st) != hipSuccess) return check_launch("dmh_cost_volume_bwd");
        maxword = reinterpret_cast<unsigned*>(acc + n_acc);
    }
    hipLaunchKernelGGL(cost_volume_nhwc_kernel, dim3((unsigned)(B * L * ttiles)), dim3(NT), 0, st, lookup, nhwc, H * W, ttiles);
    hipLaunchKernelGGL(cvb_dtotal_kernel, dim3((unsigned)tiles), dim3(NT), 0, st, current, nhwc, poses, K, invK, bins, B, L, Bp, H, W,
                       D, g, g_batch_stride, dtotal, maxword);
    hipLaunchKernelGGL(cvb_grad_kernel, dim3((unsigned)tiles), dim3(NT), 0, st, current, nhwc, poses, K, invK, bins, B, L, Bp, H, W, D,
                       dtotal, d_current, d_lookup ? reinterpret_cast<long long*>(acc) : nullptr, maxword);
    if (d_lookup)
        hipLaunchKernelGGL(cvb_finish_kernel, dim3((unsigned)(B * L * ttiles)), dim3(NT), 0, st, reinterpret_cast<const long long*>(acc),
                           d_lookup, H * W, ttiles, (long long)H * W * D, maxword);
    return check_launch("dmh_cost_volume_bwd");
}

}  // extern "C"
