// K22 -- Auto-PGD (L_inf) on the object patch: the momentum step and the whole step-size controller on the device (gfx950).
//
// Replaces torchattacks/attacks/phy_obj_atk_apgd.py:205-225 (step) and :255-290 (best tracking, loss history, checkpoint,
// step halving, restart from the best point), which in the reference are ~14 element-wise launches and three host reads
// per iteration.  Nothing here is read by the host while the attack runs:
//
//   ctl    float [steps + 1][DMH_APGD_REC]   record i = the controller's state BEFORE iteration i plus what iteration i - 1
//                                            decided.  Iteration i reads record i and writes record i + 1: the slot being
//                                            read is never written, and after the loop the array is the attack's trace.
//   hist   float [steps]                     loss of every iteration, zero until written (check_oscillation :117-122 reads
//                                            row j - k, which at the first checkpoint is row -1 = the LAST row, still zero).
//   cursor int32 [2]                         which iteration is running.  step reads cursor[0] and copies it to cursor[1];
//                                            commit reads cursor[1] and writes cursor[0] = i + 1: no launch reads a word
//                                            that the same launch writes, and a replayed HIP graph advances by itself.
//
// Both kernels are HBM streaming passes over the patch: 16-byte accesses where every pointer is 16-byte aligned, a scalar
// tail, a scalar form otherwise (as K4).  Every block evaluates the scalar decision redundantly from the same words.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int REC = DMH_APGD_REC;

// record fields
enum { R_STEP = 0, R_A, R_BEST, R_BEST_CHK, R_K, R_CNT, R_ITER, R_RED_LAST, R_LOSS, R_CHK, R_RED, R_MOVED, R_ROSE };

__device__ __forceinline__ float sgnf(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// phy_obj_atk_apgd.py:207,213-215 for one texel, every operation rounded on its own as ATen's element-wise kernels do.
// hipcc -O3 runs with -ffp-contract=fast and would fuse (x1 - x) * a + ... and grad2 * (1 - a) + ... into v_fma_f32 (one
// rounding instead of two): the pragma below switches contraction off for this function body, which is what makes the
// result bit-equal to the op-by-op expression.
__device__ __forceinline__ float apgd1(float x, float xo, float x0, float g, float ss, float a, float eps) {
#pragma clang fp contract(off)
    const float lo = x0 - eps, hi = x0 + eps;
    const float grad2 = x - xo;
    float x1 = x + ss * sgnf(g);
    x1 = clampf(fminf(fmaxf(x1, lo), hi), 0.f, 1.f);
    const float d = (x1 - x) * a;
    const float m = grad2 * (1.f - a);
    const float s = x + d;
    const float x2 = s + m;
    return clampf(fminf(fmaxf(x2, lo), hi), 0.f, 1.f);
}

__global__ __launch_bounds__(NT) void apgd_step_kernel(float* x_adv, float* x_old, const float* __restrict__ x0,
                                                       const float* __restrict__ grad, const float* __restrict__ ctl,
                                                       int32_t* cursor, int steps, float eps, int64_t n, int vec_ok) {
    const int it = cursor[0];
    if (it < 0 || it >= steps) return;  // beyond the attack's last iteration: nothing to do, nothing to index
    const float ss = ctl[(int64_t)it * REC + R_STEP], a = ctl[(int64_t)it * REC + R_A];
    if (blockIdx.x == 0 && threadIdx.x == 0) cursor[1] = it;
    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    int64_t tail = i;
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        float4* x4 = reinterpret_cast<float4*>(x_adv);
        float4* o4 = reinterpret_cast<float4*>(x_old);
        const float4* y4 = reinterpret_cast<const float4*>(x0);
        const float4* g4 = reinterpret_cast<const float4*>(grad);
        for (int64_t j = i; j < n4; j += stride) {
            const float4 x = x4[j], o = o4[j], y = y4[j], g = g4[j];
            float4 r;
            r.x = apgd1(x.x, o.x, y.x, g.x, ss, a, eps);
            r.y = apgd1(x.y, o.y, y.y, g.y, ss, a, eps);
            r.z = apgd1(x.z, o.z, y.z, g.z, ss, a, eps);
            r.w = apgd1(x.w, o.w, y.w, g.w, ss, a, eps);
            o4[j] = x;
            x4[j] = r;
        }
        tail = (n4 << 2) + i;
    }
    for (int64_t j = tail; j < n; j += stride) {
        const float x = x_adv[j];
        const float r = apgd1(x, x_old[j], x0[j], grad[j], ss, a, eps);
        x_old[j] = x;
        x_adv[j] = r;
    }
}

struct Decision {
    int moved, chk, reduce;
};

// phy_obj_atk_apgd.py:261-290 on scalars.  Deterministic in its inputs: every thread of every block gets the same answer.
// Thread 0 of block 0 also writes the history row and the next record.
__device__ __forceinline__ Decision apgd_decide(const float* __restrict__ ctl, float* hist, float* ctl_next, int it, int steps,
                                                float loss, int size_decr, int steps_min, double rho, bool writer) {
    const float* r = ctl + (int64_t)it * REC;
    const float ss = r[R_STEP], best = r[R_BEST], best_chk = r[R_BEST_CHK];
    const int k = (int)r[R_K], cnt = (int)r[R_CNT] + 1;
    const bool red_last = r[R_RED_LAST] != 0.f;
    Decision d;
    d.moved = loss > best;                  // strictly (:263)
    const float nbest = d.moved ? loss : best;
    d.chk = cnt == k;
    d.reduce = 0;
    int rose = 0;
    if (d.chk) {
        // check_oscillation(:117-122): rows it - c and it - c - 1 for c < k, negative rows wrapping as numpy's do; row `it`
        // is this iteration's loss (block 0 writes it during this very launch, so nobody reads it from memory)
        for (int c = 0; c < k; ++c) {
            int ja = it - c, jb = it - c - 1;
            ja = ja < 0 ? ja + steps : ja;
            jb = jb < 0 ? jb + steps : jb;
            if (ja < 0 || jb < 0) break;    // k > steps cannot come from a record this library wrote
            const float va = ja == it ? loss : hist[ja], vb = jb == it ? loss : hist[jb];
            rose += va > vb;
        }
        const bool osc = (double)rose <= (double)k * rho;
        const bool no_impr = !red_last && best_chk >= nbest;
        d.reduce = osc || no_impr;
    }
    if (writer) {
        hist[it] = loss;
        int nk = k - size_decr;
        nk = nk < steps_min ? steps_min : nk;
        float4* o = reinterpret_cast<float4*>(ctl_next);    // a record is 64 bytes, the array 16-byte aligned (host check)
        o[0] = make_float4(d.reduce ? ss * 0.5f : ss, 0.75f, nbest, d.chk ? nbest : best_chk);
        o[1] = make_float4((float)(d.chk ? nk : k), (float)(d.chk ? 0 : cnt), (float)(it + 1),
                           d.chk ? (float)d.reduce : (red_last ? 1.f : 0.f));
        o[2] = make_float4(loss, (float)d.chk, (float)d.reduce, (float)d.moved);
        o[3] = make_float4((float)rose, 0.f, 0.f, 0.f);
    }
    return d;
}

__global__ __launch_bounds__(NT) void apgd_commit_kernel(float* x_adv, const float* __restrict__ g_new, float* grad,
                                                         float* x_best, float* grad_best, float* x_ret,
                                                         const float* __restrict__ loss_p, float* ctl, float* hist,
                                                         int32_t* cursor, int steps, int size_decr, int steps_min,
                                                         double rho, int64_t n, int vec_ok) {
    const int it = cursor[1];
    if (it < 0 || it >= steps) return;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    const Decision d = apgd_decide(ctl, hist, ctl + (int64_t)(it + 1) * REC, it, steps, loss_p[0], size_decr, steps_min, rho,
                                   writer);
    if (writer) cursor[0] = it + 1;
    const int64_t stride = (int64_t)gridDim.x * NT;
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    int64_t tail = i;
    if (vec_ok) {
        const int64_t n4 = n >> 2;
        float4* x4 = reinterpret_cast<float4*>(x_adv);
        const float4* gn4 = reinterpret_cast<const float4*>(g_new);
        float4* g4 = reinterpret_cast<float4*>(grad);
        float4* xb4 = reinterpret_cast<float4*>(x_best);
        float4* gb4 = reinterpret_cast<float4*>(grad_best);
        float4* xr4 = reinterpret_cast<float4*>(x_ret);
        for (int64_t j = i; j < n4; j += stride) {
            const float4 x = x4[j], g = gn4[j];
            xr4[j] = x;                         // x_best_adv of :255: the iterate before a possible restart
            if (d.moved) {                      // :265-266
                xb4[j] = x;
                gb4[j] = g;
            }
            if (d.reduce && !d.moved) {         // :286-287 (after a move the best point IS this iterate)
                x4[j] = xb4[j];
                g4[j] = gb4[j];
            } else {
                g4[j] = g;
            }
        }
        tail = (n4 << 2) + i;
    }
    for (int64_t j = tail; j < n; j += stride) {
        const float x = x_adv[j], g = g_new[j];
        x_ret[j] = x;
        if (d.moved) {
            x_best[j] = x;
            grad_best[j] = g;
        }
        if (d.reduce && !d.moved) {
            x_adv[j] = x_best[j];
            grad[j] = grad_best[j];
        } else {
            grad[j] = g;
        }
    }
}

inline int grid_for(int64_t n) {
    const int64_t b = (n + NT - 1) / NT;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

inline bool distinct(const void* const* p, int m) {
    for (int a = 0; a < m; ++a)
        for (int b = a + 1; b < m; ++b)
            if (p[a] == p[b]) return false;
    return true;
}

}  // namespace

extern "C" {

int dmh_apgd_step(float* x_adv, float* x_old, const float* x0, const float* grad, const float* ctl, int32_t* cursor,
                  int steps, float eps, int64_t n, void* stream) {
    DMH_REQUIRE(x_adv && x_old && x0 && grad && ctl && cursor, "null pointer");
    DMH_REQUIRE(n > 0 && steps > 0 && steps < (1 << 24), "need n > 0 and 0 < steps < 2^24");
    DMH_REQUIRE(eps >= 0.f, "eps must not be negative");
    const void* const w[] = {x_adv, x_old, x0, grad};
    DMH_REQUIRE(distinct(w, 4), "x_adv, x_old, x0 and grad must be four different buffers");
    const uintptr_t al = (uintptr_t)x_adv | (uintptr_t)x_old | (uintptr_t)x0 | (uintptr_t)grad;
    const int vec_ok = (al & 15) == 0;
    const int64_t work = vec_ok ? (n + 3) / 4 : n;
    hipLaunchKernelGGL(apgd_step_kernel, dim3(grid_for(work)), dim3(NT), 0, (hipStream_t)stream, x_adv, x_old, x0, grad, ctl,
                       cursor, steps, eps, n, vec_ok);
    return check_launch("dmh_apgd_step");
}

int dmh_apgd_commit(float* x_adv, const float* g_new, float* grad, float* x_best, float* grad_best, float* x_ret,
                    const float* loss, float* ctl, float* hist, int32_t* cursor, int steps, int size_decr, int steps_min,
                    double rho, int64_t n, void* stream) {
    DMH_REQUIRE(x_adv && g_new && grad && x_best && grad_best && x_ret && loss && ctl && hist && cursor, "null pointer");
    DMH_REQUIRE(n > 0 && steps > 0 && steps < (1 << 24), "need n > 0 and 0 < steps < 2^24");
    DMH_REQUIRE(size_decr > 0 && steps_min > 0, "size_decr and steps_min must be positive");
    DMH_REQUIRE(rho > 0.0 && rho <= 1.0, "rho must lie in (0, 1]");
    DMH_REQUIRE(((uintptr_t)ctl & 15) == 0, "the record array must be 16-byte aligned");
    const void* const w[] = {x_adv, g_new, grad, x_best, grad_best, x_ret};
    DMH_REQUIRE(distinct(w, 6), "x_adv, g_new, grad, x_best, grad_best and x_ret must be six different buffers");
    const uintptr_t al = (uintptr_t)x_adv | (uintptr_t)g_new | (uintptr_t)grad | (uintptr_t)x_best | (uintptr_t)grad_best |
                         (uintptr_t)x_ret;
    const int vec_ok = (al & 15) == 0;
    const int64_t work = vec_ok ? (n + 3) / 4 : n;
    hipLaunchKernelGGL(apgd_commit_kernel, dim3(grid_for(work)), dim3(NT), 0, (hipStream_t)stream, x_adv, g_new, grad, x_best,
                       grad_best, x_ret, loss, ctl, hist, cursor, steps, size_decr, steps_min, rho, n, vec_ok);
    return check_launch("dmh_apgd_commit");
}

}  // extern "C"
