// K40 -- the odometry protocol's trajectory arithmetic on the device (gfx950): MD2/evaluate_pose.py:23-46 (dump_xyz, compute_ate)
// and :116-125 (the snippet loop, np.mean and np.std of the snippet errors).
//
// The reference copies every batch of predicted poses to the host and then, per snippet, chains up to four 4x4 np.dot products for
// the prediction and four for the ground truth, and aligns the two point lists by one scale factor.  Here the poses stay where
// K29 wrote them and two launches leave ates [N] and stats [2] = (mean, population standard deviation) on the device.
//
// Launch one, one thread per snippet i in [0, N):
//   n = min(track_length - 1, N - i) poses -> n + 1 points: the reference's slices get shorter at the end of the sequence
//   C = I;  p_0 = C[:3, 3];  for k < n: C = C . T[i + k] (C'[r][c] = sum over j ascending of C[r][j] T[j][c]);  p_{k+1} = C[:3, 3]
//   in float64 for the predicted poses (float32, widened exactly, as np.dot widens them) and the ground-truth local poses (float64)
//   offset = gt_0 - pred_0;  pred_k += offset;  scale = sum(gt . pred) / sum(pred^2), points ascending, x y z inside a point
//   ates[i] = sqrt(sum((pred scale - gt)^2)) / (n + 1)          -- the divisor is the point count, as the reference has it
//   sum(pred^2) = 0 gives 0 / 0 = NaN, as numpy does: not guarded.
// Launch two, ONE workgroup: thread t sums ates[t], ates[t + NT], ... in ascending order, a fixed binary tree over LDS joins the NT
// sums; mean = sum / N; the same again over (ates - mean)^2; stats = (mean, sqrt(that / N)) -- np.std's two passes.  No atomics, no
// counters: the same input gives the same bits.
// Products and sums are not contracted into fused multiply-adds, so ops.pose_ate_host can state the same arithmetic in numpy;
// numpy's own 4x4 products go through BLAS and differ from either in the last bit (tests/pose_eval_ref.py has the gate).
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;

// C = C . T in index order; T's element type is the trajectory's own (float for the prediction, double for the ground truth)
template <typename T>
__device__ __forceinline__ void chain(double (&C)[4][4], const T* __restrict__ t) {
#pragma clang fp contract(off)
    double m[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) m[j][c] = (double)t[j * 4 + c];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double row[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double s = C[r][0] * m[0][c];
#pragma unroll
            for (int j = 1; j < 4; ++j) {
                const double p = C[r][j] * m[j][c];
                s = s + p;
            }
            row[c] = s;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) C[r][c] = row[c];
    }
}

__device__ __forceinline__ void identity(double (&C)[4][4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) C[r][c] = r == c ? 1.0 : 0.0;
}

__global__ __launch_bounds__(NT) void pose_ate_kernel(const float* __restrict__ pred, const double* __restrict__ gt, int N, int track_length,
                                                      double* __restrict__ ates) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const int64_t left = (int64_t)N - i;
    const int n = (int)(left < track_length - 1 ? left : track_length - 1);       // poses of this snippet, >= 1
    double P[4][4], G[4][4];
    identity(P);
    identity(G);
    // pass 1: the two sums of the scale.  The first points are both the identity's translation; the reference still subtracts them.
    const double off[3] = {G[0][3] - P[0][3], G[1][3] - P[1][3], G[2][3] - P[2][3]};
    double s_gp = 0.0, s_pp = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p = P[c][3] + off[c], g = G[c][3];
        const double gp = g * p, pp = p * p;
        s_gp = s_gp + gp;
        s_pp = s_pp + pp;
    }
    for (int k = 0; k < n; ++k) {
        chain(P, pred + (i + k) * 16);
        chain(G, gt + (i + k) * 16);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p = P[c][3] + off[c], g = G[c][3];
            const double gp = g * p, pp = p * p;
            s_gp = s_gp + gp;
            s_pp = s_pp + pp;
        }
    }
    const double scale = __ddiv_rn(s_gp, s_pp);
    // pass 2: the same chains again (the same code: the same points), now against the scale
    identity(P);
    identity(G);
    double s_ee = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double p = P[c][3] + off[c];
        const double ps = p * scale;
        const double e = ps - G[c][3];
        const double ee = e * e;
        s_ee = s_ee + ee;
    }
    for (int k = 0; k < n; ++k) {
        chain(P, pred + (i + k) * 16);
        chain(G, gt + (i + k) * 16);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double p = P[c][3] + off[c];
            const double ps = p * scale;
            const double e = ps - G[c][3];
            const double ee = e * e;
            s_ee = s_ee + ee;
        }
    }
    ates[i] = __ddiv_rn(__dsqrt_rn(s_ee), (double)(n + 1));
}

// the fixed tree: after it every thread reads the total from s[0]
__device__ __forceinline__ double tree_sum(double* s, double mine) {
#pragma clang fp contract(off)
    const int t = threadIdx.x;
    s[t] = mine;
    __syncthreads();
#pragma unroll
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (t < o) s[t] = s[t] + s[t + o];
        __syncthreads();
    }
    const double total = s[0];
    __syncthreads();                        // s is written again by the next call
    return total;
}

__global__ __launch_bounds__(NT) void pose_ate_stats_kernel(const double* __restrict__ ates, int N, double* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double s[NT];
    const int t = threadIdx.x;
    double mine = 0.0;
    for (int64_t i = t; i < N; i += NT) mine = mine + ates[i];
    const double mean = __ddiv_rn(tree_sum(s, mine), (double)N);
    mine = 0.0;
    for (int64_t i = t; i < N; i += NT) {
        const double d = ates[i] - mean;
        const double dd = d * d;
        mine = mine + dd;
    }
    const double var = __ddiv_rn(tree_sum(s, mine), (double)N);
    if (t == 0) {
        stats[0] = mean;
        stats[1] = __dsqrt_rn(var);
    }
}

}  // namespace

extern "C" {

int dmh_pose_ate(const float* pred_poses, const double* gt_local, int n, int track_length, double* ates, double* stats, void* stream) {
    DMH_REQUIRE(pred_poses && gt_local && ates && stats, "null pointer");
    DMH_REQUIRE(n > 0 && n <= (1 << 24), "need 0 < n <= 2^24 poses");
    DMH_REQUIRE(track_length >= 2 && track_length <= (1 << 16), "need 2 <= track_length <= 2^16");
    DMH_REQUIRE(((uintptr_t)pred_poses & 3) == 0 && ((uintptr_t)gt_local & 7) == 0 && ((uintptr_t)ates & 7) == 0 && ((uintptr_t)stats & 7) == 0,
                "pred_poses must be 4-byte, gt_local, ates and stats 8-byte aligned");
    DMH_REQUIRE((const void*)ates != (const void*)gt_local && (const void*)stats != (const void*)ates && (const void*)stats != (const void*)gt_local,
                "ates, stats and gt_local must not alias");
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pose_ate_kernel, dim3((n + NT - 1) / NT), dim3(NT), 0, st, pred_poses, gt_local, n, track_length, ates);
    hipLaunchKernelGGL(pose_ate_stats_kernel, dim3(1), dim3(NT), 0, st, (const double*)ates, n, stats);
    return check_launch("dmh_pose_ate");
}

}  // extern "C"
