// K23 -- the update of one iteration of the L0 object attack in one launch (gfx950).
//
// Covers what iteration i of torchattacks/attacks/phy_obj_atk_l0.py:92-138 does between "the model's gradient has arrived" and
// "the next composed patch exists": the mask-weight selection (:105-111), the gradient's route through the outer clamp and the
// two pattern clamps (K5 l0_compose_bwd), the tanh mask cost's backward (K5 l0_mask_cost_bwd), Adam on both patterns (:138) and
// the compose + L0 count of the next iteration (K5 l0_compose_fwd, :94-99, :43-52).  Every decision is read from device memory:
//
//   count  int32 [2 steps + 1]   count[i] = L0 count of the patch iteration i attacks.  Iteration i reads count[i] and count[0]
//                                and adds (integer atomics, one per wave) into count[i + 1], which the caller zeroed.
//   tab    float [2 steps][2]    (lr / (1 - b1^t), sqrt(1 - b2^t)), t = 1 .. 2 steps: made on the host in double, rounded once.
//   rec    float [2 steps][8]    record i = (l0_i, mw_i, adv_cost_i, mask_cost_i, t, below_i, 0, 0): the attack's trace.
//   cursor int32 [2]             cursor[0] = the iteration that runs; cursor[1] = a ticket counter, zero between launches.
//
// Cursor: a last-block ticket, not K22's two-word cursor with a one-thread second launch.  This kernel exists to shorten a
// chain of short dependent launches, and a second launch per iteration would give one of them back.  Every block reads
// cursor[0] on entry; when all its threads are done (__syncthreads) its thread 0 draws a ticket (atomicAdd); the block that
// draws the last one knows that every other block has read cursor[0], and it alone writes the record, resets the ticket and
// publishes cursor[0] = i + 1.  Nothing else is read and written by one launch: count[i + 1] and rec[i] are written only,
// a texel's patterns and Adam state are read and written by the one thread that owns the texel, and obj, g_adv and adv are
// buffers of their own (host check).
//
// One thread owns all C channels of both patterns at 4 consecutive pixels (16-byte accesses: HW % 4 == 0, all pointers 16-byte
// aligned) or at 1 pixel (scalar form), because the mask cost takes a maximum over channels.  Every block evaluates the scalar
// decision redundantly from the same words.
#include "common.hpp"

using namespace dmh;

namespace {

constexpr int NT = 256;
constexpr int REC = DMH_L0_REC;

struct L0FusedArgs {
    const float* obj;
    float *pos, *neg, *m_pos, *v_pos, *m_neg, *v_neg;
    const float* g_adv;
    float* adv;
    int32_t* count;
    float* rec;
    int32_t* cursor;
    const float* tab;
    const float* adv_cost;
    const float* mask_cost;
    int steps, C, HW;
    float mask_wt, thresh, l0_clip;
};

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

template <int V>
__device__ __forceinline__ void load(const float* p, float (&r)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        r[0] = t.x, r[1] = t.y, r[2] = t.z, r[3] = t.w;
    } else {
        r[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void store(float* p, const float (&r)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
    } else {
        p[0] = r[0];
    }
}

// The selection of phy_obj_atk_l0.py:105-111 as the attack evaluates it on the device: fp32 ratio, correctly rounded quotient.
__device__ __forceinline__ bool l0_below(int32_t c_i, int32_t c_0, float thresh) {
#pragma clang fp contract(off)
    return (float)c_i / (float)c_0 <= thresh;
}

// d mask_cost / d pattern at the maximal channel (l0_mask_bwd_kernel), times the mask weight; up = mw / HW.
__device__ __forceinline__ float mask_grad(float th, float up) {
#pragma clang fp contract(off)
    return up * (1.f - th * th) / 10.f / (float)(2.0 - 1e-7);
}

// torch.optim.Adam(betas=(0.5, 0.9), eps=1e-8) on one element, every product, sum, quotient and root rounded on its own:
// hipcc -O3 contracts a * b + c into one v_fma_f32 by default; the pragma switches that off for this body.  The division and
// the square root stay the correctly rounded expansions.
__device__ __forceinline__ void adam1(float& p, float& m, float& v, float g, float ss, float bc2s) {
#pragma clang fp contract(off)
    m = m * 0.5f + g * 0.5f;
    v = v * 0.9f + (g * g) * (float)(1.0 - 0.9);
    const float den = sqrtf(v) / bc2s + 1e-8f;
    p = p + (-ss) * (m / den);
}

template <int V>
__global__ __launch_bounds__(NT) void l0_fused_kernel(const L0FusedArgs a) {
    const int it = a.cursor[0];
    if (it < 0 || it >= 2 * a.steps) return;    // beyond the attack's last iteration: nothing to do, nothing to index
    const int32_t c_i = a.count[it], c_0 = a.count[0];
    const bool below = l0_below(c_i, c_0, a.thresh);
    const float mw = below ? 0.f : a.mask_wt;
    const float ss = a.tab[2 * it], bc2s = a.tab[2 * it + 1];
    const int HW = a.HW, C = a.C;
    const int px = (blockIdx.x * NT + threadIdx.x) * V;
    bool nz[V];
#pragma unroll
    for (int l = 0; l < V; ++l) nz[l] = false;
    if (px < HW) {
        int bp[V], bq[V];
        float tp[V], tq[V];
#pragma unroll
        for (int l = 0; l < V; ++l) bp[l] = bq[l] = -1, tp[l] = tq[l] = 0.f;
        if (mw != 0.f) {    // torch.max(dim=1) routes the gradient to the first maximal channel
            float vp[V], vq[V];
#pragma unroll
            for (int l = 0; l < V; ++l) vp[l] = vq[l] = -3.0e38f;
            for (int c = 0; c < C; ++c) {
                float p[V], q[V];
                load<V>(a.pos + c * HW + px, p);
                load<V>(a.neg + c * HW + px, q);
#pragma unroll
                for (int l = 0; l < V; ++l) {
                    const float thp = tanhf(p[l] / 10.f), thq = tanhf(q[l] / 10.f);
                    const float fp = thp / (float)(2.0 - 1e-7) + 0.5f, fq = thq / (float)(2.0 - 1e-7) + 0.5f;
                    if (fp > vp[l]) vp[l] = fp, bp[l] = c, tp[l] = thp;
                    if (fq > vq[l]) vq[l] = fq, bq[l] = c, tq[l] = thq;
                }
            }
        }
        const float up = mw / (float)HW;
        float acc[V];
#pragma unroll
        for (int l = 0; l < V; ++l) acc[l] = 0.f;
        for (int c = 0; c < C; ++c) {
            const int o = c * HW + px;
            float ob[V], p[V], q[V], ga[V], mp[V], vp[V], mq[V], vq[V], ad[V];
            load<V>(a.obj + o, ob);
            load<V>(a.pos + o, p);
            load<V>(a.neg + o, q);
            load<V>(a.g_adv + o, ga);
            load<V>(a.m_pos + o, mp);
            load<V>(a.v_pos + o, vp);
            load<V>(a.m_neg + o, mq);
            load<V>(a.v_neg + o, vq);
#pragma unroll
            for (int l = 0; l < V; ++l) {
                // the adversarial cost's gradient through the outer clamp and the pattern clamps (closed intervals)
                const float v = ob[l] + (clampf(p[l], 0.f, 1.f) - clampf(q[l], 0.f, 1.f));
                const float g = (v >= 0.f && v <= 1.f) ? ga[l] : 0.f;
                const float gp = ((p[l] >= 0.f && p[l] <= 1.f) ? g : 0.f) + (c == bp[l] ? mask_grad(tp[l], up) : 0.f);
                const float gn = ((q[l] >= 0.f && q[l] <= 1.f) ? -g : 0.f) + (c == bq[l] ? mask_grad(tq[l], up) : 0.f);
                adam1(p[l], mp[l], vp[l], gp, ss, bc2s);
                adam1(q[l], mq[l], vq[l], gn, ss, bc2s);
                // the next iteration's patch and its thresholded pattern (l0_compose_fwd_kernel)
                const float pp = clampf(p[l], 0.f, 1.f), pn = -clampf(q[l], 0.f, 1.f);
                const float t1 = pp < a.l0_clip ? 0.f : pp, t2 = pn > -a.l0_clip ? 0.f : pn;
                acc[l] += fabsf(t1 + t2);
                ad[l] = clampf(ob[l] + (pp + pn), 0.f, 1.f);
            }
            store<V>(a.pos + o, p);
            store<V>(a.neg + o, q);
            store<V>(a.m_pos + o, mp);
            store<V>(a.v_pos + o, vp);
            store<V>(a.m_neg + o, mq);
            store<V>(a.v_neg + o, vq);
            store<V>(a.adv + o, ad);
        }
#pragma unroll
        for (int l = 0; l < V; ++l) nz[l] = acc[l] != 0.f;
    }
    int32_t n = 0;      // an integer count: independent of the order of the atomics
#pragma unroll
    for (int l = 0; l < V; ++l) n += (int32_t)__popcll(__ballot(nz[l]));
    if ((threadIdx.x & (WAVE - 1)) == 0 && n) atomicAdd(a.count + it + 1, n);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int ticket = atomicAdd(a.cursor + 1, 1);
        if (ticket == (int)gridDim.x - 1) {     // every other block has read cursor[0] and count[it]
            float4* r = reinterpret_cast<float4*>(a.rec + (int64_t)it * REC);   // 32-byte records, 16-byte aligned array
            r[0] = make_float4((float)c_i, mw, a.adv_cost[0], a.mask_cost ? a.mask_cost[0] : 0.f);
            r[1] = make_float4((float)(it + 1), below ? 1.f : 0.f, 0.f, 0.f);
            a.cursor[1] = 0;
            __threadfence();
            a.cursor[0] = it + 1;
        }
    }
}

inline bool distinct(const void* const* p, int m) {
    for (int a = 0; a < m; ++a)
        for (int b = a + 1; b < m; ++b)
            if (p[a] == p[b]) return false;
    return true;
}

}  // namespace

extern "C" {

int dmh_l0_fused_step(const float* obj, float* pos, float* neg, float* m_pos, float* v_pos, float* m_neg, float* v_neg,
                      const float* g_adv, float* adv, int32_t* count, float* rec, int32_t* cursor, const float* tab,
                      const float* adv_cost, const float* mask_cost, int steps, int C, int HW, float mask_wt, float thresh,
                      float l0_clip, void* stream) {
    DMH_REQUIRE(obj && pos && neg && m_pos && v_pos && m_neg && v_neg && g_adv && adv, "null pointer");
    DMH_REQUIRE(count && rec && cursor && tab && adv_cost, "null pointer");
    DMH_REQUIRE(steps > 0 && steps < (1 << 24), "need 0 < steps < 2^24");
    DMH_REQUIRE(C > 0 && HW > 0 && (int64_t)C * HW < (1ll << 31) - 4 * NT, "need C > 0, HW > 0 and C * HW < 2^31");
    DMH_REQUIRE(((uintptr_t)rec & 15) == 0, "the record array must be 16-byte aligned");
    const void* const w[] = {obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv};
    DMH_REQUIRE(distinct(w, 9), "obj, pos, neg, the four Adam state tensors, g_adv and adv must be nine different buffers");
    const L0FusedArgs a = {obj, pos, neg, m_pos, v_pos, m_neg, v_neg, g_adv, adv, count, rec, cursor, tab, adv_cost,
                           mask_cost, steps, C, HW, mask_wt, thresh, l0_clip};
    uintptr_t al = 0;
    for (const void* p : w) al |= (uintptr_t)p;
    if ((al & 15) == 0 && HW % 4 == 0) {
        hipLaunchKernelGGL(l0_fused_kernel<4>, dim3((HW / 4 + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, a);
    } else {
        hipLaunchKernelGGL(l0_fused_kernel<1>, dim3((HW + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, a);
    }
    return check_launch("dmh_l0_fused_step");
}

}  // extern "C"
