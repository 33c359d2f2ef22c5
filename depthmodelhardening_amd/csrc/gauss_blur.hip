// K26 -- Gaussian-blur object attack (a search over growing sigmas): scipy.ndimage.gaussian_filter on the device, bit for bit,
// for the one rectangle of the object patch the attack repaints (gfx950).
//
// Replaces torchattacks/attacks/phy_obj_atk_guassian.py:96-103 (a device-to-host copy, gaussian_filter(x0, [0, 0, s, s]) with
// up to 1201 taps per axis over 3 x 260 x 300 on the CPU, np.clip, an upload, the mask blend) for every step of the attack
// at once, before the search starts:
//
//   weights  double [steps][wstride]   row s: p[0 .. lw] of scipy's kernel for sigma s (the left half and the centre; the kernel is
//                                      symmetric), made on the host in float64 as _gaussian_kernel1d makes it, zero padded.
//   radii    int32 [steps]             lw = int(4.0 * sigma + 0.5) per step; clamped to [0, wstride - 1] here.
//   tmp      float [steps][C][rh][W]   pass 1 (axis H) for the rectangle's rows over all columns, rounded to fp32 as scipy's
//                                      float32 output array rounds the intermediate.
//   windows  float [steps][C][rh][rw]  pass 2 (axis W) for the rectangle, then np.clip(., 0, 1).
//
// The order is the contract (scipy's correlate1d, symmetric branch): per output, in double,
//   tmp = a[i] p[lw];  for ll = -lw .. -1: tmp = tmp + (a[r(i + ll)] + a[r(i - ll)]) p[lw + ll]
// every operation rounded on its own (contraction off), one thread per output, a serial tap loop.  r() is mode 'reflect'
// (d c b a | a b c d | d c b a); the radius reaches 2 max(H, W), so the index wraps more than one period: one modulo per
// thread finds the two start positions, then both walk and bounce.  No exp on the device: its last bit differs from libm's.
//
// compose writes the object with window index[0] in the rectangle and the original elsewhere; keep-the-best is K24's commit.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;

// virtual index j of a reflected line of n samples -> (position, direction of the position when j grows by one)
__device__ __forceinline__ void reflect_start(int j, int n, int& pos, int& dir) {
    const int period = 2 * n;
    int m = j % period;
    m = m < 0 ? m + period : m;
    const bool up = m < n;
    pos = up ? m : period - 1 - m;
    dir = up ? 1 : -1;
}

__device__ __forceinline__ void reflect_step(int& pos, int& dir, int n) {
    pos += dir;
    const bool top = pos >= n, bottom = pos < 0;
    pos = top ? n - 1 : (bottom ? 0 : pos);
    dir = top ? -1 : (bottom ? 1 : dir);
}

// one output of correlate1d on the line a[0 .. n) (elements ``stride`` apart) at position i
__device__ __forceinline__ float blur_at(const float* __restrict__ a, int stride, int n, int i, int lw,
                                         const double* __restrict__ p) {
#pragma clang fp contract(off)
    double tmp = (double)a[(int64_t)i * stride] * p[lw];
    int lo, dlo, hi, dhi;
    reflect_start(i - lw, n, lo, dlo);      // i + ll, ll = -lw .. -1: walks towards i
    reflect_start(i + lw, n, hi, dhi);      // i - ll: walks down towards i
    dhi = -dhi;
    for (int k = 0; k < lw; ++k) {
        const double s = (double)a[(int64_t)lo * stride] + (double)a[(int64_t)hi * stride];
        tmp = tmp + s * p[k];
        reflect_step(lo, dlo, n);
        reflect_step(hi, dhi, n);
    }
    return (float)tmp;
}

__device__ __forceinline__ int radius_of(const int32_t* __restrict__ radii, int s, int wstride) {
    return min(max(radii[s], 0), wstride - 1);
}

// Pass 1, axis H.  grid (ceil(W / NT), rh, steps * C): the column is the fastest index, so every tap reads one row segment.
__global__ __launch_bounds__(NT) void gauss_blur_rows_kernel(const float* __restrict__ obj, const double* __restrict__ weights,
                                                             const int32_t* __restrict__ radii, float* __restrict__ tmp,
                                                             int wstride, int C, int H, int W, int r0, int rh) {
    const int x = blockIdx.x * NT + threadIdx.x;
    if (x >= W) return;
    const int y = blockIdx.y, sc = blockIdx.z, s = sc / C, c = sc - s * C;
    const int lw = radius_of(radii, s, wstride);
    const float v = blur_at(obj + (int64_t)c * H * W + x, W, H, r0 + y, lw, weights + (int64_t)s * wstride);
    tmp[((int64_t)sc * rh + y) * W + x] = v;
}

// Pass 2, axis W, and the clip.  grid (ceil(rw / NT), rh, steps * C); the row of tmp a block walks is 4 W bytes: it stays in L1.
__global__ __launch_bounds__(NT) void gauss_blur_cols_kernel(const float* __restrict__ tmp, const double* __restrict__ weights,
                                                             const int32_t* __restrict__ radii, float* __restrict__ windows,
                                                             int wstride, int C, int W, int c0, int rh, int rw) {
    const int x = blockIdx.x * NT + threadIdx.x;
    if (x >= rw) return;
    const int y = blockIdx.y, sc = blockIdx.z, s = sc / C;
    const int lw = radius_of(radii, s, wstride);
    const float v = blur_at(tmp + ((int64_t)sc * rh + y) * W, 1, W, c0 + x, lw, weights + (int64_t)s * wstride);
    windows[((int64_t)sc * rh + y) * rw + x] = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);      // np.clip: a NaN stays
}

__global__ __launch_bounds__(NT) void gauss_blur_compose_kernel(const float* __restrict__ windows, const int32_t* __restrict__ index,
                                                                const float* __restrict__ obj, float* __restrict__ out, int steps,
                                                                int C, int H, int W, int r0, int c0, int rh, int rw) {
    const int q = index[0];
    if (q < 0 || q >= steps) return;        // outside the search: nothing to do, nothing to index
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= C * H * W) return;
    const int c = i / (H * W), rem = i - c * H * W, y = rem / W, x = rem - y * W;
    const int wy = y - r0, wx = x - c0;
    const bool inside = wy >= 0 && wy < rh && wx >= 0 && wx < rw;
    out[i] = inside ? windows[(((int64_t)q * C + c) * rh + wy) * rw + wx] : obj[i];
}

bool region_ok(int H, int W, int r0, int r1, int c0, int c1) { return 0 <= r0 && r0 < r1 && r1 <= H && 0 <= c0 && c0 < c1 && c1 <= W; }

}  // namespace

extern "C" {

int dmh_gauss_blur_windows(const float* obj, const double* weights, const int32_t* radii, float* tmp, float* windows, int steps,
                           int wstride, int C, int H, int W, int r0, int r1, int c0, int c1, void* stream) {
    DMH_REQUIRE(obj && weights && radii && tmp && windows, "null pointer");
    DMH_REQUIRE(steps > 0 && wstride > 0 && C > 0 && H > 0 && W > 0, "need steps, wstride, C, H, W > 0");
    DMH_REQUIRE(region_ok(H, W, r0, r1, c0, c1), "need 0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W");
    DMH_REQUIRE(H < (1 << 20) && W < (1 << 20) && (int64_t)C * H * W < (1 << 28), "need H, W < 2^20 and C * H * W < 2^28");
    DMH_REQUIRE((int64_t)steps * C <= 65535 && (r1 - r0) <= 65535, "need steps * C and the rectangle's rows <= 65535");
    DMH_REQUIRE((int64_t)steps * C * (r1 - r0) * W < (1ll << 31), "need steps * C * rows * W < 2^31");
    DMH_REQUIRE(((uintptr_t)weights & 7) == 0 && ((uintptr_t)radii & 3) == 0, "weights must be 8-byte, radii 4-byte aligned");
    DMH_REQUIRE(tmp != obj && windows != obj && tmp != windows, "obj, tmp and windows must be different buffers");
    const int rh = r1 - r0, rw = c1 - c0;
    hipLaunchKernelGGL(gauss_blur_rows_kernel, dim3((W + NT - 1) / NT, rh, steps * C), dim3(NT), 0, (hipStream_t)stream, obj,
                       weights, radii, tmp, wstride, C, H, W, r0, rh);
    hipLaunchKernelGGL(gauss_blur_cols_kernel, dim3((rw + NT - 1) / NT, rh, steps * C), dim3(NT), 0, (hipStream_t)stream, tmp,
                       weights, radii, windows, wstride, C, W, c0, rh, rw);
    return check_launch("dmh_gauss_blur_windows");
}

int dmh_gauss_blur_compose(const float* windows, const int32_t* index, const float* obj, float* out, int steps, int C, int H,
                           int W, int r0, int r1, int c0, int c1, void* stream) {
    DMH_REQUIRE(windows && index && obj && out, "null pointer");
    DMH_REQUIRE(steps > 0 && C > 0 && H > 0 && W > 0 && (int64_t)C * H * W < (1 << 28), "need steps > 0 and 0 < C * H * W < 2^28");
    DMH_REQUIRE(region_ok(H, W, r0, r1, c0, c1), "need 0 <= r0 < r1 <= H and 0 <= c0 < c1 <= W");
    DMH_REQUIRE((int64_t)steps * C * (r1 - r0) * (c1 - c0) < (1ll << 31), "need steps * C * rows * columns < 2^31");
    DMH_REQUIRE(((uintptr_t)index & 3) == 0, "index must be 4-byte aligned");
    DMH_REQUIRE(out != windows && out != obj, "out must not alias windows or obj");
    const int work = C * H * W;
    hipLaunchKernelGGL(gauss_blur_compose_kernel, dim3((work + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, windows, index, obj,
                       out, steps, C, H, W, r0, c0, r1 - r0, c1 - c0);
    return check_launch("dmh_gauss_blur_compose");
}

}  // extern "C"
