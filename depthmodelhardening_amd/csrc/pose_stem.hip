// K41 -- the pose encoder's first layer on a PAIR of frames, with the channel concatenation and the input normalisation fused:
//     y[p,k,oy,ox] = sum_{c<6,ky,kx} w[k,c,ky,kx] * xn[p,c,2oy-3+ky,2ox-3+kx],   xn = (cat(a, b)[p] - mean) * inv_std inside the
//                                                                                image, 0 in the padding
// i.e. MD2/evaluate_pose.py:94-96 `torch.cat([color_aug 0, color_aug 1], 1)` into MD2/networks/resnet_encoder.py:89-90
// `x = (input_image - 0.45) / 0.225; x = self.encoder.conv1(x)` for num_input_images = 2 (7x7, stride 2, padding 3, 6 -> 64
// channels, no bias).  Forward only: the odometry evaluation runs it under no_grad; training keeps its own path.
//
// It is K14 (stem_conv_fwd.hip: read its header first) swept twice.  K14 keeps a whole 3x7x7 filter in registers, 148 values per
// lane; a 6x7x7 filter does not fit.  So there are two launches of one kernel template on the same stream:
//   sweep 0: w[:, 0:3] (row stride 294, not 147) in registers, a's region staged per tile, y written;
//   sweep 1: w[:, 3:6] in registers, b's region staged per tile, the tile's sum ADDED into y.
// The tile -> workgroup and element -> lane maps are the same in both sweeps, so every y element is written, read back and
// written again by one thread position, the second launch after the first: no atomics, the same bits on every run.  Per output:
// two k-ordered fp32 fma chains of 147 taps (K14's tap order) and one fp32 addition.
// Forms that were compiled and dropped (hipcc, ROCm 7): both sweeps as a loop inside one launch spills 153 registers a lane to
// scratch, and so does starting sweep 1's accumulators from y (62): 148 filter values and 32 accumulators leave no room for 32
// addresses in flight.  The read-add-write after the MFMA loop needs none: 256 registers, no scratch, as K14.
// a and b are two base pointers: each a contiguous [B,3,H,W] block, and they may overlap (frames[:-1] and frames[1:] of one
// [B+1,3,H,W] tensor, which is how the evaluation calls it): neither the concatenation nor a normalised copy ever exists.
//
// The tile geometry, the tap pairing and the operand maps are K14's: a workgroup of 4 waves owns 4 output rows x 32 columns; the
// normalised 13 x 69 x 3 input region is staged in LDS; wave w computes output row w with 74 k-pairs x 2 channel halves of
// v_mfma_f32_32x32x2_f32; the B operand is one ds_read_b32 per pair at an immediate offset from one of three per-lane bases.
#include "common.hpp"

using namespace dmh;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256;
constexpr int TR = 4, TC = 32;                 // output rows (one per wave) x columns per workgroup tile
constexpr int RH = 2 * TR + 5;                 // 13 input rows
constexpr int RW = 2 * TC + 6;                 // 70 input columns (69 used + one finite pad column for the dummy tap)
constexpr int PLANE = RH * RW;                 // 910 floats per channel
constexpr int NPAIR = 74;
constexpr int TAPS = 147;                      // 3 x 7 x 7: one sweep's slice of a filter row
constexpr int WROW = 2 * TAPS;                 // 294: the stride between the filter's output channels

// pair j of a sweep: LDS offset of its first tap, the stride class of the second, the two tap indices (c*49+ky*7+kx, -1: zero)
struct PairDesc { int off; int cls; int k0; int k1; };
__host__ __device__ constexpr PairDesc pair_desc(int j) {
    // 0..62: (c, ky, kx even pairs)   63..71: kx = 6, (ky, ky+1) pairs   72: (c=0,c=1) at (6,6)   73: (c=2, 6, 6) + dummy
    if (j < 63) {
        const int c = j / 21, r = j % 21, ky = r / 3, kx = 2 * (r % 3);
        return {c * PLANE + ky * RW + kx, 0, c * 49 + ky * 7 + kx, c * 49 + ky * 7 + kx + 1};
    }
    if (j < 72) {
        const int q = j - 63, c = q / 3, ky = 2 * (q % 3);
        return {c * PLANE + ky * RW + 6, 1, c * 49 + ky * 7 + 6, c * 49 + (ky + 1) * 7 + 6};
    }
    if (j == 72) return {6 * RW + 6, 2, 0 * 49 + 48, 1 * 49 + 48};
    return {2 * PLANE + 6 * RW + 6, 0, 2 * 49 + 48, -1};
}

struct PArgs {
    const float* x;         // this sweep's frames: a or b
    const float* w;         // this sweep's filter slice: w or w + 147
    float* y;
    int B, H, W, Ho, Wo, gx, gy, ntiles;
    float mean, inv_std;
};

template <int SWEEP>
__global__ __launch_bounds__(NT, 2) void pose_stem_kernel(const PArgs a) {
    __shared__ float tile[3 * PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = lane & 31, h = lane >> 5;

    // ---- this sweep's half of the filter, once: lane supplies A[i = n (+32)][k = h] of every pair
    float wA[NPAIR], wB[NPAIR];
#pragma unroll
    for (int j = 0; j < NPAIR; ++j) {
        const PairDesc d = pair_desc(j);
        const int kk = h ? d.k1 : d.k0;
        wA[j] = kk >= 0 ? a.w[(size_t)n * WROW + kk] : 0.f;
        wB[j] = kk >= 0 ? a.w[(size_t)(n + 32) * WROW + kk] : 0.f;
    }
    // per-lane LDS bases (floats): pixel n of output row wv sits at input row 2*wv, column 2*n of the region
    const int base = (2 * wv) * RW + 2 * n;
    const float* b0 = tile + base + (h ? 1 : 0);
    const float* b1 = tile + base + (h ? RW : 0);
    const float* b2 = tile + base + (h ? PLANE : 0);

    const size_t HW = (size_t)a.H * a.W, HWo = (size_t)a.Ho * a.Wo;
    for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        int q = t;
        const int bxi = q % a.gx;  q /= a.gx;
        const int byi = q % a.gy;
        const int b = q / a.gy;
        const int oy0 = byi * TR, ox0 = bxi * TC;
        const int iy0 = 2 * oy0 - 3, ix0 = 2 * ox0 - 3;
        const float* xb = a.x + (size_t)b * 3 * HW;
        __syncthreads();                              // the previous tile's reads are done
        for (int e = tid; e < 3 * PLANE; e += NT) {
            const int c = e / PLANE, rem = e - c * PLANE, r = rem / RW, cc = rem - r * RW;
            const int iy = iy0 + r, ix = ix0 + cc;
            const bool ok = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            const float v = xb[(size_t)c * HW + (size_t)min(max(iy, 0), a.H - 1) * a.W + min(max(ix, 0), a.W - 1)];
            tile[e] = ok ? (v - a.mean) * a.inv_std : 0.f;
        }
        __syncthreads();
        f32x16 accA, accB;
#pragma unroll
        for (int v = 0; v < 16; ++v) accA[v] = accB[v] = 0.f;
#pragma unroll
        for (int j = 0; j < NPAIR; ++j) {
            const PairDesc d = pair_desc(j);
            const float bv = (d.cls == 0 ? b0 : d.cls == 1 ? b1 : b2)[d.off];
            accA = __builtin_amdgcn_mfma_f32_32x32x2f32(wA[j], bv, accA, 0, 0, 0);
            accB = __builtin_amdgcn_mfma_f32_32x32x2f32(wB[j], bv, accB, 0, 0, 0);
        }
        // D[i][n]: lane holds column n, rows i = 8*(v/4) + 4*h + v%4
        const int oy = oy0 + wv, ox = ox0 + n;
        if (oy < a.Ho && ox < a.Wo) {
            float* yb = a.y + (size_t)b * 64 * HWo + (size_t)oy * a.Wo + ox;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int i = 8 * (v >> 2) + 4 * h + (v & 3);
                if (SWEEP) {                          // on top of what sweep 0 left at this very element
                    yb[(size_t)i * HWo] += accA[v];
                    yb[(size_t)(i + 32) * HWo] += accB[v];
                } else {
                    yb[(size_t)i * HWo] = accA[v];
                    yb[(size_t)(i + 32) * HWo] = accB[v];
                }
            }
        }
    }
}

inline long long pair_tiles(int B, int Ho, int Wo) { return (long long)B * ((Wo + TC - 1) / TC) * ((Ho + TR - 1) / TR); }

}  // namespace

extern "C" {

int dmh_stem_pair_norm_fwd(const float* a, const float* b, const float* w, int B, int H, int W, float mean, float std, float* y,
                           void* stream) {
    DMH_REQUIRE(a && b && w && y, "null pointer");
    DMH_REQUIRE(B > 0 && H >= 2 && W >= 2 && (H & 1) == 0 && (W & 1) == 0, "image height and width must be even");
    DMH_REQUIRE(std > 0.f, "std must be positive");
    DMH_REQUIRE((int64_t)B * 64 * (H / 2) * (W / 2) < ((int64_t)1 << 40), "tensor too large");
    DMH_REQUIRE(((uintptr_t)a & 3) == 0 && ((uintptr_t)b & 3) == 0 && ((uintptr_t)w & 3) == 0 && ((uintptr_t)y & 3) == 0,
                "pointers must be 4-byte aligned");
    DMH_REQUIRE((const void*)y != (const void*)a && (const void*)y != (const void*)b && (const void*)y != (const void*)w,
                "y must not alias an input");
    PArgs p;
    p.x = a;
    p.w = w;
    p.y = y;
    p.B = B;
    p.H = H;
    p.W = W;
    p.Ho = H / 2;
    p.Wo = W / 2;
    p.gx = (p.Wo + TC - 1) / TC;
    p.gy = (p.Ho + TR - 1) / TR;
    const long long tiles = pair_tiles(B, p.Ho, p.Wo);
    if (tiles >= (1ll << 31)) return fail(DMH_EINVAL, "%s: grid too large", "dmh_stem_pair_norm_fwd");
    p.ntiles = (int)tiles;
    p.mean = mean;
    p.inv_std = 1.0f / std;
    const int blocks = (int)(tiles < 512 ? tiles : 512);      // K14's geometry: 2 workgroups per CU, persistent beyond that
    hipLaunchKernelGGL(pose_stem_kernel<0>, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, p);
    p.x = b;
    p.w = w + TAPS;
    hipLaunchKernelGGL(pose_stem_kernel<1>, dim3(blocks), dim3(NT), 0, (hipStream_t)stream, p);
    return check_launch("dmh_stem_pair_norm_fwd");
}

}  // extern "C"
