/*
 * dmh_hip.h -- C ABI of libdmh_hip.so: the MI355X (gfx950) hot path of the
 * DepthModelHardening adversarial-training loop.
 *
 * The reference (Bob-cheng/DepthModelHardening) is pure Python; its seam for this path
 * is a set of Python call signatures.  Every entry point below
 * replaces one PyTorch op chain of the reference, cited as file:line relative to the
 * reference root (MD2 = DepthNetworks/monodepth2, DH = DepthNetworks/depth-hints).
 * The binding a maintainer would add on the reference side is a ctypes stub -- see
 * INTEGRATION.md.
 *
 * Conventions
 *  - plain C: pointers are DEVICE pointers to fp32, NCHW, contiguous; sizes are ints.
 *    No torch types.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *  - the library allocates nothing, retains nothing, never synchronises; every call only
 *    enqueues kernels on `stream` (safe under hipGraph capture).
 *  - return value: DMH_OK or an error code; dmh_last_error() gives the message of the
 *    calling thread's last failure.  Shape errors are caught on the host BEFORE launch.
 */
#ifndef DMH_HIP_H
#define DMH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMH_OK 0
#define DMH_EINVAL 1  /* bad argument (null pointer, unsupported shape) */
#define DMH_ELAUNCH 2 /* hipLaunch / runtime error                      */

#define DMH_MAX_SCALES 4
#define DMH_MAX_FRAMES 4

#define DMH_VARIANT_MD2 0 /* MD2/trainer.py:647-660  min over {identity, reprojection}, mean over all pixels */
#define DMH_VARIANT_DH 1  /* DH/trainer.py:557-590,700-708  argmin mask, masked sum / mask count            */

#define DMH_NOISE_NONE 0   /* no tie-break term                                                     */
#define DMH_NOISE_TENSOR 1 /* caller passes the already-scaled term (randn*1e-5, MD2/trainer.py:642-645) */
#define DMH_NOISE_PHILOX 2 /* N(0,1)*1e-5 generated in-kernel from (seed, offset): no HBM traffic    */

/* Slots of the `fin` vector written by dmh_loss_finalize (floats). */
#define DMH_FIN_LOSS 0       /* sum_s loss_s / NS                         MD2/trainer.py:670 */
#define DMH_FIN_LOSS_S 1     /* [4] loss/{s}                              MD2/trainer.py:668 */
#define DMH_FIN_REPROJ_S 5   /* [4] mean(to_optimise) | DH reproj_loss/{s}                   */
#define DMH_FIN_COUNT_S 9    /* [4] number of pixels where reprojection was selected         */
#define DMH_FIN_SMOOTH_S 13  /* [4] get_smooth_loss(norm_disp, color)     MD2/trainer.py:664 */
#define DMH_FIN_HINT_S 20    /* [4] depth_hint_loss/{s} (0 without depth hints)   DH/trainer.py:713-725 */
#define DMH_FIN_HINTCOUNT_S 24 /* [4] number of pixels where the depth hint won the argmin */
#define DMH_FIN_SIZE 28

const char* dmh_version(void);
const char* dmh_last_error(void);
/* Diagnostics (tools/rccl_overlap.py): a stand-in with a ring collective's launch geometry -- `channels` persistent workgroups of
 * 256 threads copy n floats src -> dst `rounds` times -- to observe, on ONE GPU, how such a kernel on a side stream is scheduled
 * against the persistent convolution workgroups (a 1-rank RCCL all-reduce launches no device kernel).  Not on any product path. */
int dmh_debug_channel_copy(const float* src, float* dst, int64_t n, int channels, int rounds, void* stream);

/* ------------------------------------------------------------------------------------
 * K1  fused photometric loss: bilinear-upsample(disp_s) -> disp_to_depth -> BackprojectDepth
 *     -> Project3D -> grid_sample(border, align_corners=True) -> SSIM(3x3, reflect) + L1
 *     -> identity term -> per-pixel min / argmin mask -> block partial sums,
 *     for all scales in ONE launch (target/source tiles are read once).
 * Replaces: MD2/trainer.py:472-523 (generate_images_pred), :525-537
 *           (compute_reprojection_loss), :589-660 (compute_losses body),
 *           MD2/layers.py:16-25,139-198,223-253; DH/trainer.py:638-708.
 * ---------------------------------------------------------------------------------- */
typedef struct dmh_photo_args {
    const float* target;                 /* [B,3,H,W] inputs[("color",0,0)]                        */
    const float* source[DMH_MAX_FRAMES]; /* [B,3,H,W] inputs[("color",f,0)], f = frame_ids[1:]     */
    const float* T[DMH_MAX_FRAMES];      /* [B,4,4]   stereo_T or cam_T_cam                        */
    const float* K;                      /* [B,4,4]   inputs[("K",0)]                              */
    const float* inv_K;                  /* [B,4,4]   inputs[("inv_K",0)]                          */
    const float* disp[DMH_MAX_SCALES];   /* [B,1,Hs,Ws] outputs[("disp",s)]                        */
    int Hs[DMH_MAX_SCALES], Ws[DMH_MAX_SCALES];
    int B, H, W;
    int num_frames;                      /* 1..DMH_MAX_FRAMES                                      */
    int num_scales;                      /* 1..DMH_MAX_SCALES                                      */
    float min_depth, max_depth;          /* MD2/options.py:69-76                                   */
    int variant;                         /* DMH_VARIANT_*                                          */
    int automask;                        /* 0 = --disable_automasking                              */
    int no_ssim;                         /* 1 = --no_ssim                                          */
    int noise_mode;                      /* DMH_NOISE_*                                            */
    const float* noise[DMH_MAX_SCALES];  /* TENSOR mode: [B,NF,H,W], NF = num_frames (MD2) or 1 (DH) */
    uint64_t seed, offset;               /* PHILOX mode                                            */
    /* DepthHints --use_depth_hints (DH/trainer.py:510-525,629-636,700-725); both NULL = off.  Needs variant DH,
     * automask and ONE source frame (the reference builds the hint view for the stereo frame only).              */
    const float* depth_hint;             /* [B,1,H,W] inputs["depth_hint"], 0 where there is no hint */
    const float* depth_hint_mask;        /* [B,1,H,W] inputs["depth_hint_mask"]                      */
} dmh_photo_args;

/* number of floats the photometric partial-sum workspace needs */
int64_t dmh_photo_partials_size(int B, int H, int W, int num_scales);   /* 4 floats per (scale, strip) */
/* number of floats of the backward staging workspace (per-strip partial low-resolution gradients) */
int64_t dmh_photo_stage_size(const dmh_photo_args* a);

/* Forward.  sel      : out [B,H,W] uint8, the selection of every scale packed 2 bits per scale: bits [2s, 2s+1] =
 *                      0 identity chosen, 1+f reprojection of source frame f chosen (== outputs["identity_selection/s"]
 *                      for one source frame, MD2/trainer.py:656-658); with depth hints 3 = the hint won (reprojection
 *                      of frame 0 applies as well, DH/trainer.py:583-584).  At most 3 source frames.
 *           to_opt[s]: out [B,H,W] per-pixel selected loss, or NULL
 *           partials : out, dmh_photo_partials_size floats
 * disp[s] must be [B,1,H/f,W/f] with f in {1,2,4,8,16}.                                                     */
int dmh_photo_loss_fwd(const dmh_photo_args* a, uint8_t* sel, float* const to_opt[DMH_MAX_SCALES], float* partials,
                       void* stream);

/* Backward (recompute).  gvec: [DMH_FIN_SIZE] upstream gradient of the fin vector; fin: the finalized forward
 * vector; stage: dmh_photo_stage_size floats of scratch.  g_disp[s]: out [B,1,Hs,Ws] gradient w.r.t. disp[s]
 * (overwritten; the adjoint of the bilinear up-sampling, MD2/trainer.py:481-482, is applied in the kernel).   */
int dmh_photo_loss_bwd(const dmh_photo_args* a, const uint8_t* sel, const float* gvec, const float* fin, float* stage,
                       float* const g_disp[DMH_MAX_SCALES], void* stream);
/* The same + the gradient w.r.t. the camera poses (outputs[("cam_T_cam", 0, f)] of monocular source frames,
 * MD2/trainer.py:276-330,487-519): pose_partials[num_scales][strips][num_frames][12] receives per-strip sums
 *   [ S_i0, S_i1, S_i2, s_i ]  (i = 0, 1, 2)   with   d loss / d P_f[i][j<3] = sum_k inv_K[j][k] S_ik,   d loss / d P_f[i][3] = s_i,
 * P_f = (K T_f)[:3,:] (MD2/layers.py:188); the caller sums over scales and an image's strips (strip index = image-major:
 * strips / B per image) and forms d loss / d T_f = K[:3,:]^T dP_f.  dmh_photo_pose_partials_size(a) floats. */
int64_t dmh_photo_pose_partials_size(const dmh_photo_args* a);
int dmh_photo_loss_bwd_pose(const dmh_photo_args* a, const uint8_t* sel, const float* gvec, const float* fin, float* stage,
                            float* const g_disp[DMH_MAX_SCALES], float* pose_partials, void* stream);

/* out[i] = field `scale` of the packed selection map as float (0 identity, 1+f frame f), n = B*H*W.          */
int dmh_unpack_selection(const uint8_t* sel, int64_t n, int scale, float* out, void* stream);

/* Adjoint of F.interpolate(disp,[H,W],bilinear,align_corners=False) (MD2/trainer.py:481-482):
 * g_disp [B,1,Hs,Ws] (+)= gather(g_up [B,H,W]).  accumulate != 0 adds to g_disp.             */
int dmh_upsample_bilinear_adjoint(const float* g_up, float* g_disp, int B, int H, int W, int Hs, int Ws,
                                  int accumulate, void* stream);

/* Materialise generate_images_pred's tensors for one (scale, frame) (MD2/trainer.py:481-519):
 * depth [B,1,H,W], sample [B,H,W,2], color [B,3,H,W]; any output may be NULL.                */
int dmh_warp_view_fwd(const float* source, const float* disp, const float* K, const float* inv_K,
                      const float* T, int B, int H, int W, int Hs, int Ws, float min_depth,
                      float max_depth, float* depth, float* sample, float* color, void* stream);

/* Backward of dmh_warp_view_fwd w.r.t. the upsampled disparity given grad_color [B,3,H,W]
 * (and optionally grad_depth [B,1,H,W], may be NULL): g_up [B,H,W].                           */
int dmh_warp_view_bwd(const float* source, const float* disp, const float* K, const float* inv_K,
                      const float* T, int B, int H, int W, int Hs, int Ws, float min_depth,
                      float max_depth, const float* grad_color, const float* grad_depth, float* g_up,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * K2  edge-aware smoothness on the mean-normalised disparity, all scales in one launch.
 * Replaces: MD2/trainer.py:662-666 + MD2/layers.py:207-220.
 * ---------------------------------------------------------------------------------- */
typedef struct dmh_smooth_args {
    const float* disp[DMH_MAX_SCALES];  /* [B,1,Hs,Ws] outputs[("disp",s)]   */
    const float* color[DMH_MAX_SCALES]; /* [B,3,Hs,Ws] inputs[("color",0,s)] */
    int Hs[DMH_MAX_SCALES], Ws[DMH_MAX_SCALES];
    int B, num_scales;
} dmh_smooth_args;

int64_t dmh_smooth_partials_size(const dmh_smooth_args* a);
int dmh_smooth_loss_fwd(const dmh_smooth_args* a, float* partials, void* stream);
/* g_disp[s] [B,1,Hs,Ws]; accumulate != 0 adds.  sstats from dmh_loss_finalize. */
int dmh_smooth_loss_bwd(const dmh_smooth_args* a, const float* gvec, const float* sstats,
                        float smooth_wt, float* const g_disp[DMH_MAX_SCALES], int accumulate, void* stream);

/* Deterministic final reduction of K1+K2 partials:  fin[DMH_FIN_SIZE], sstats[NS][B][2] =
 * (mean_disp_b, R_b).  loss_s = reproj_s + smooth_wt * smooth_s / 2^s  (MD2/trainer.py:660-668). */
int dmh_loss_finalize(const float* photo_partials, const float* smooth_partials, int B, int H, int W,
                      const dmh_smooth_args* sm, int variant, float smooth_wt, float* fin, float* sstats,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * K3  EOT paste: Pad -> perspective warp of patch and mask -> composite -> Resize, fused.
 * Replaces: physicalTrans.py:107-166 (padding_img, project) +
 *           torchattacks/attacks/phy_obj_atk.py:87-90 (composite + 2x Resize).
 * coeffs [N,8]: torchvision-0.8.2 perspective coefficients per sample (host computes them from
 * the integer pixel quads, physicalTrans.py:62-81).  scene_bstride = 0 broadcasts one scene.
 * ---------------------------------------------------------------------------------- */
#define DMH_PASTE_COMPOSITE 0 /* adv = resize(scene*(1-m) + obj*m), mask_out = resize(m)   phy_obj_atk.py:88-90 */
#define DMH_PASTE_WARP_ONLY 1 /* adv = resize(obj), mask_out = resize(m); scene ignored    physicalTrans.py:156-165 */

typedef struct dmh_paste_args {
    const float* scene; /* [N or 1,3,SH,SW] */
    int64_t scene_bstride;
    const float* patch; /* [1,3,PH,PW] */
    const float* pmask; /* [1,1,PH,PW] */
    const float* coeffs; /* [N,8] */
    int N, SH, SW, PH, PW, OH, OW;
    int l_pad, t_pad; /* physicalTrans.py:110-113 */
    int mode;         /* DMH_PASTE_COMPOSITE or DMH_PASTE_WARP_ONLY */
    const int32_t* flip; /* [N] or NULL: != 0 mirrors sample n horizontally (do_flip of MD2/datasets/mono_dataset.py:288,
                          :222-225: the loader flips the frame, prep_adv_data flips the projected object and mask; the
                          scene passed here is the UN-flipped frame and the whole composite is written mirrored) */
    const int32_t* scene_index; /* [N] or NULL: sample n reads frame scene_index[n] of `scene` (a pool of frames with batch
                                   stride scene_bstride) instead of frame n -- the loader's index_select / side pick without
                                   a copy of the frames.  Every index must lie inside the pool (checked by the caller). */
} dmh_paste_args;

/* adv [N,3,OH,OW], mask_out [N,1,OH,OW] (either may be NULL) */
int dmh_eot_paste_fwd(const dmh_paste_args* a, float* adv, float* mask_out, void* stream);
/* Host only, no launch: the kernel dmh_eot_paste_fwd takes for these arguments (it decides through this function).
 * 2 = tiled (OW % 4 == 0, both outputs 16-byte aligned, resize ratios the LDS rectangle holds), 1 = four-wide (the same
 * without the ratio limit), 0 = generic, -1 = arguments the forward rejects. */
int dmh_eot_paste_fwd_form(const dmh_paste_args* a, const float* adv, const float* mask_out);
/* g_patch [1,3,PH,PW] is overwritten (gather per patch texel over the inverse homography: no atomics, bitwise
 * reproducible; the caller does not have to zero it). */
int dmh_eot_paste_bwd(const dmh_paste_args* a, const float* g_adv, float* g_patch, void* stream);

/* ------------------------------------------------------------------------------------
 * K4  PGD-L_inf update  x <- clamp(x0 + clamp(x + alpha*sign(g) - x0, -eps, eps), 0, 1)
 * Replaces: phy_obj_atk.py:98-101, pgd_depth.py:76-78.  out may alias x.
 * ---------------------------------------------------------------------------------- */
int dmh_pgd_linf_step(const float* x, const float* x0, const float* g, float alpha, float eps, float* out,
                      int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * K22  Auto-PGD (L_inf) on the object patch: momentum step and step-size controller, both driven from device memory.
 * Replaces: phy_obj_atk_apgd.py:205-225 (step), :255-290 (best point, loss history, checkpoint, halving, restart).
 *   ctl    [steps + 1][DMH_APGD_REC] floats, 16-byte aligned.  Record i is read by iteration i; commit writes record i + 1.
 *          Words: 0 step size, 1 momentum weight a, 2 loss_best, 3 loss_best at the last checkpoint, 4 k, 5 iterations
 *          since the last checkpoint, 6 iteration index, 7 reduced at the last checkpoint (starts 1), and about the
 *          iteration before: 8 its loss, 9 it was a checkpoint, 10 it halved the step and restarted, 11 loss_best moved,
 *          12 how many of the last k losses rose; 13-15 zero.  The caller fills record 0 and zeroes the rest.
 *   hist   [steps] floats, zeroed by the caller: the loss of every iteration.
 *   cursor int32[2], zeroed by the caller: step runs iteration cursor[0] and copies it to cursor[1]; commit finishes
 *          iteration cursor[1] and sets cursor[0] to the next.  A cursor outside [0, steps) makes both a no-op.
 * step:   x_old <- x_adv;  x_adv <- the momentum step of :207-215 with step size and a of record i, every operation
 *         rounded on its own (bit-equal to the element-wise fp32 expression).
 * commit: with loss[0] = the cost at the new x_adv and g_new its gradient: x_ret <- x_adv; if loss > loss_best:
 *         x_best <- x_adv, grad_best <- g_new; hist[i] <- loss; on a checkpoint that reduces: x_adv <- x_best,
 *         grad <- grad_best, else grad <- g_new; record i + 1.  All tensor arguments hold n floats and must not alias.
 * ---------------------------------------------------------------------------------- */
#define DMH_APGD_REC 16
int dmh_apgd_step(float* x_adv, float* x_old, const float* x0, const float* grad, const float* ctl, int32_t* cursor,
                  int steps, float eps, int64_t n, void* stream);
int dmh_apgd_commit(float* x_adv, const float* g_new, float* grad, float* x_best, float* grad_best, float* x_ret,
                    const float* loss, float* ctl, float* hist, int32_t* cursor, int steps, int size_decr, int steps_min,
                    double rho, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------
 * K23  L0 object attack: one iteration's update in one launch, decisions read from device memory.
 * Replaces: phy_obj_atk_l0.py:105-111 (mask-weight selection), the backward of :94-99 and :130-132, Adam's step (:138,
 * betas (0.5, 0.9), eps 1e-8, state m / v in fp32) and the compose + L0 count of the next iteration (:94-99, :43-52).
 *   count  int32 [2 steps + 1]: count[i] = L0 count of the patch iteration i attacks; the caller fills count[0] (K5) and
 *          zeroes the rest.  Iteration i reads count[i], count[0] and adds into count[i + 1].
 *   tab    [2 steps][2] floats: (lr / (1 - b1^t), sqrt(1 - b2^t)), t = 1 .. 2 steps.
 *   rec    [2 steps][DMH_L0_REC] floats, 16-byte aligned.  Record i: 0 l0_i, 1 mask weight used, 2 adv_cost[0], 3 mask_cost[0]
 *          (0 if mask_cost is NULL), 4 t = i + 1, 5 ratio was below the threshold; 6-7 zero.
 *   cursor int32 [2]: cursor[0] = i, advanced by the launch; cursor[1] = its ticket counter, zero between launches.
 *          A cursor outside 0 .. 2 steps - 1 makes the launch a no-op.
 * mw_i = (float)count[i] / (float)count[0] <= thresh ? 0 : mask_wt.  pos, neg, m_*, v_* are updated in place; adv receives
 * clamp(obj + clamp(pos,0,1) - clamp(neg,0,1), 0, 1) of the updated patterns.  All nine tensors hold C * HW floats and must
 * not alias.  16-byte accesses when all nine are 16-byte aligned and HW % 4 == 0, a scalar form otherwise.
 * ---------------------------------------------------------------------------------- */
#define DMH_L0_REC 8
int dmh_l0_fused_step(const float* obj, float* pos, float* neg, float* m_pos, float* v_pos, float* m_neg, float* v_neg,
                      const float* g_adv, float* adv, int32_t* count, float* rec, int32_t* cursor, const float* tab,
                      const float* adv_cost, const float* mask_cost, int steps, int C, int HW, float mask_wt, float thresh,
                      float l0_clip, void* stream);

/* ------------------------------------------------------------------------------------
 * K24  Tube-light object attack (a random search): the lit patch and the "keep the best" step, driven from device memory.
 * Replaces: phy_obj_atk_light.py:130-138 with light_simulation.py:23-28,:124-163 (compose), :165-167 (commit).
 *   table  [n_queries][DMH_LIGHT_REC] doubles, made on the host in float64: 0 k, 1 b, 2 beta, 3 full_end = int(sqrt(beta) + .5),
 *          4 light_end = int(sqrt(20 beta) + .5), 5 sqrt(1 + k k), 6-8 c[i] * alpha (wavelength_to_rgb), 9 zero.
 *   index  int32[>= 1]: compose lights the object with record index[0]; an index outside [0, n_queries) makes it a no-op.
 *   base   uint8 [3][H][W]: the clean object, trunc(obj * 255).   out: float [3][H][W] = uint8 result / 255.
 *   state  int32[2]: 0 the cursor (the caller zeroes it), 1 the best query (the caller sets -1).  best: float[1], 1e10 at start.
 * compose: d = |k x - y + b| / s;  att = d <= full_end ? 1 : d <= light_end ? beta / (d d) : 0;  v = (c att) 255.0, all in
 *          double, every operation rounded on its own; out = trunc(clip((float)base + (float)v, 0, 255)) / 255 in fp32:
 *          bit-equal to the reference's chain.  16-byte stores when W % 4 == 0, base is 4-byte and out 16-byte aligned.
 * commit:  q = state[0]; cost[q] <- cost_in[0]; if cost_in[0] < best[0]: best[0] <- it, state[1] <- q; state[0] <- q + 1.
 *          A cursor outside [0, n_queries) makes it a no-op.
 * ---------------------------------------------------------------------------------- */
#define DMH_LIGHT_REC 10
int dmh_tube_light_compose(const double* table, const int32_t* index, const uint8_t* base, float* out, int n_queries, int H,
                           int W, void* stream);
int dmh_tube_light_commit(const float* cost_in, float* cost, float* best, int32_t* state, int n_queries, void* stream);

/* ------------------------------------------------------------------------------------
 * K26  Gaussian-blur object attack (a search over growing sigmas): scipy.ndimage.gaussian_filter(x, [0, 0, s, s]) (mode
 * 'reflect', truncate 4.0) followed by np.clip(., 0, 1), bit for bit, for the rectangle [r0, r1) x [c0, c1) of the object.
 * Replaces: phy_obj_atk_guassian.py:96-103 (windows, compose); keep-the-best (:121-123) is dmh_tube_light_commit.
 *   obj      float [C][H][W]: the clean object.
 *   weights  double [steps][wstride], made on the host in float64: row s = p[0 .. lw_s] of exp(-0.5 / (s s) x^2), x = -lw .. lw,
 *            divided by its sum (the kernel is symmetric: the left half and the centre), zero padded.
 *   radii    int32 [steps]: lw_s = int(4.0 s + 0.5); the kernels clamp it to [0, wstride - 1].
 *   tmp      float [steps][C][r1 - r0][W]: workspace, pass 1 (axis H) rounded to fp32.
 *   windows  float [steps][C][r1 - r0][c1 - c0]: pass 2 (axis W), clipped.
 * Per output and axis, in double, every operation rounded on its own:
 *   t = a[i] p[lw];  for ll = -lw .. -1: t = t + (a[r(i + ll)] + a[r(i - ll)]) p[lw + ll];  r(j): j mod 2n, 2n - 1 - j if >= n.
 * windows: two launches (one per pass) for all steps.
 * compose: out = obj with windows[index[0]] in the rectangle; an index outside [0, steps) makes it a no-op.
 * ---------------------------------------------------------------------------------- */
int dmh_gauss_blur_windows(const float* obj, const double* weights, const int32_t* radii, float* tmp, float* windows, int steps,
                           int wstride, int C, int H, int W, int r0, int r1, int c0, int c1, void* stream);
int dmh_gauss_blur_compose(const float* windows, const int32_t* index, const float* obj, float* out, int steps, int C, int H,
                           int W, int r0, int r1, int c0, int c1, void* stream);

/* ------------------------------------------------------------------------------------
 * K27  Square attack (L_inf) on the object patch: absorb the previous query's decision and make the next candidate, one launch.
 * Replaces: phy_obj_atk_square.py:259-260 (start stripes), :284-291 (candidate), :312-313 (x_best update); the strict
 * keep-the-best (:298-301) is dmh_tube_light_commit, which also advances the cursor.
 *   x0       float [C][H][W]: the clean object.   x_best, x_new: float [C][H][W], updated in place.  Three different buffers.
 *   table    int32 [n_queries][3 + C]: vh, vw, s, sign_0 .. sign_{C-1} (each -1, 0 or 1) per query; row 0 is not read.
 *   stripes  float [C][W]: +-1, the start point.
 *   state    int32[2] of K24: 0 the cursor q, 1 the best query.  Only read.
 * With accept = (0 < q <= n_queries and state[1] == q - 1), per element:
 *   xb = accept ? x_new : x_best;  x_best <- xb;
 *   q == 0:            x_new <- clamp(x0 + eps stripe, 0, 1)
 *   0 < q < n_queries: x_new <- clamp(min(max(xb + 2 eps sign_c, x0 - eps), x0 + eps), 0, 1) for vh <= y < vh + s and
 *                      vw <= x < vw + s, xb elsewhere
 *   q == n_queries:    x_new stays (the absorb-only call after the last query);  any other q: nothing is written.
 * Every operation is one rounded fp32 operation: bit-equal to the element-wise expression.  16-byte accesses when W % 4 == 0 and
 * x0, x_best, x_new and stripes are 16-byte aligned, a scalar form otherwise.
 * ---------------------------------------------------------------------------------- */
int dmh_square_propose(const float* x0, float* x_best, float* x_new, const int32_t* table, const float* stripes,
                       const int32_t* state, int n_queries, int C, int H, int W, float eps, void* stream);

/* ------------------------------------------------------------------------------------
 * K28  PGD-L2 update on n floats with ONE norm over the whole tensor, two launches, no host read, no atomics:
 *   y = x + alpha g / (||g||_2 + 1e-10);  d = y - x0;  out = clamp(x0 + d min(eps / ||d||_2, 1), 0, 1)
 * Replaces: phy_obj_atk_l2.py:110-120 (shared-patch form).
 *   workspace: dmh_pgd_l2_workspace_size(n) bytes, 8-byte aligned: the per-workgroup double partials of sum(g g),
 *              sum((x - x0) g), sum((x - x0)^2) that launch 1 writes and every workgroup of launch 2 adds in index order.
 *              Written by every call: two calls in flight need two workspaces.
 * ||d||^2 comes from the expansion sum((x-x0)^2) + 2 s sum((x-x0) g) + s^2 sum(g g), s = alpha / (||g|| + 1e-10); eps / 0 gives
 * the factor 1.  Scalars and the element-wise expression are evaluated in double and rounded to fp32 once; the result is bitwise
 * reproducible.  out must not alias x, x0 or g.  16-byte accesses when x, x0, g and out are 16-byte aligned, scalar otherwise.
 * ---------------------------------------------------------------------------------- */
int64_t dmh_pgd_l2_workspace_size(int64_t n);
int dmh_pgd_l2_step(const float* x, const float* x0, const float* g, double alpha, double eps, float* out, int64_t n,
                    void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * K25  Benign depth evaluation (MD2/evaluate_depth.py:351-391): depth at ground-truth resolution, exact medians, eight metrics.
 *   gt       float [gt_len]: the ground-truth maps of a pack, one after the other.
 *   table    int32 [n_images][DMH_EIGEN_REC]: 0 offset into gt, 1 gt_h, 2 gt_w, 3 y0, 4 y1, 5 x0, 6 x1 (crop; the whole map for
 *            splits other than eigen), 7 the image's first work block.  A work block is DMH_EIGEN_CHUNK pixels of one image.
 *   blk_img  int32 [n_blocks]: the image of every work block of the pack.
 *   A call covers the images first .. first + n - 1 (n <= DMH_EIGEN_MAX_BATCH); their work blocks are b0 .. b0 + grid - 1 and
 *   the grid is one workgroup per work block.  px0 = table[first][0]: depth[i - px0] belongs to gt[i].
 *   eigen != 0: valid = 1e-3 < gt < 80 inside the crop; eigen == 0: valid = gt > 0.
 *   ws       uint32 [dmh_eigen_select_ws_size(n)]: histograms and selection state, zeroed by the entry points themselves.
 * gt_stats:   count[n] valid pixels and med[n] = np.median of the valid ground truth (NaN without a valid pixel).
 * pred_depth: depth = factor / resize(disp) at every valid pixel (OpenCV INTER_LINEAR float arithmetic, no antialiasing), the
 *             bit pattern 0xffffffff elsewhere.  flip != NULL: every tap is the blend of batch_post_process_disparity (:102-110)
 *             of pred and the mirrored flip.  ws != NULL: also the first histogram pass of the median (for pred_ratio).
 * pred_ratio: med_pred[n] = np.median of the valid depths, ratio[n] = med_gt[first + i] / med_pred[i]; needs pred_depth's ws.
 * metrics:    errors[n][8] = abs_err, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 of compute_errors' unmasked branch (:61-76) on
 *             clamp(depth * ratio, 1e-3, 80) (ratio == NULL: no scaling); partials: float [dmh_eigen_partials_size(grid)].
 *             fp32 sums per work block, combined in double in a fixed order.  No valid pixel: a row of NaN.
 * ---------------------------------------------------------------------------------- */
#define DMH_EIGEN_REC 8
#define DMH_EIGEN_CHUNK 8192
#define DMH_EIGEN_MAX_BATCH 64
int64_t dmh_eigen_select_ws_size(int n);
int64_t dmh_eigen_partials_size(int grid);
int dmh_eigen_gt_stats(const float* gt, int64_t gt_len, const int32_t* table, const int32_t* blk_img, int n_images, int n_blocks,
                       int first, int n, int b0, int grid, int eigen, uint32_t* ws, float* med, int32_t* count, void* stream);
int dmh_eigen_pred_depth(const float* pred, const float* flip, int h, int w, const float* gt, int64_t gt_len, const int32_t* table,
                         const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int grid, int eigen,
                         float factor, int64_t px0, float* depth, int64_t depth_len, uint32_t* ws, void* stream);
int dmh_eigen_pred_ratio(const float* depth, int64_t depth_len, int64_t px0, int64_t gt_len, const int32_t* table,
                         const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int grid, uint32_t* ws,
                         const float* med_gt, float* med_pred, float* ratio, void* stream);
int dmh_eigen_metrics(const float* gt, int64_t gt_len, const float* depth, int64_t depth_len, int64_t px0, const int32_t* table,
                      const int32_t* blk_img, int n_images, int n_blocks, int first, int n, int b0, int grid, const float* ratio,
                      float* partials, float* errors, void* stream);

/* ------------------------------------------------------------------------------------
 * K5  L0 attack pieces (phy_obj_atk_l0.py).
 * compose (:94-99,:43-52): adv = clamp(obj + clamp(pos,0,1) - clamp(neg,0,1), 0, 1);
 *   l0_count (int32, zeroed by caller) += #pixels whose thresholded pattern is non-zero.
 *   finalize != 0 applies the final thresholding of :143-150 to the composed patch too.
 * ---------------------------------------------------------------------------------- */
int dmh_l0_compose_fwd(const float* obj, const float* pos, const float* neg, int C, int HW, float l0_clip,
                       int finalize, float* adv, int32_t* l0_count, void* stream);
int dmh_l0_compose_bwd(const float* obj, const float* pos, const float* neg, const float* g_adv, int C, int HW,
                       float* g_pos, float* g_neg, int accumulate, void* stream);
/* mask cost (:130-132): mean_hw max_c(tanh(p/10)/(2-1e-7)+0.5) for pos and neg; cost: float[1] out.
 * partials: 2*nblk floats (dmh_l0_mask_partials_size). */
int64_t dmh_l0_mask_partials_size(int HW);
int dmh_l0_mask_cost_fwd(const float* pos, const float* neg, int C, int HW, float* partials, float* cost,
                         void* stream);
/* g_pos/g_neg (+)= gscale[0]*weight[0] * d cost/d p ; gscale, weight: device scalars */
int dmh_l0_mask_cost_bwd(const float* pos, const float* neg, int C, int HW, const float* gscale,
                         const float* weight, float* g_pos, float* g_neg, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------
 * K6  masked squared mean  cost = mean((disp*mask)^2)  (MSELoss against zeros,
 *     phy_obj_atk.py:94, phy_obj_atk_l0.py:127).  mask may be NULL (pgd_depth.py:68).
 * ---------------------------------------------------------------------------------- */
int64_t dmh_sq_mean_partials_size(int64_t n);
int dmh_masked_sq_mean_fwd(const float* disp, const float* mask, int64_t n, float* partials, float* cost,
                           void* stream);
/* g_disp = gscale[0] * 2 * disp * mask^2 / n */
int dmh_masked_sq_mean_bwd(const float* disp, const float* mask, int64_t n, const float* gscale, float* g_disp,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * K6b --gt_depth supervised term (MD2/trainer.py:551-557, options.py:227-229): with
 *     depth(d) = clamp(5.4 / (1/max_depth + (1/min_depth - 1/max_depth) d), 1e-3, 80)   (disp_to_depth, layers.py:16-25)
 *     cost = mean_{b,hw} ( m objdepth[b] + depth(disp_gt) (1 - m) - depth(disp) )^2 ,   m = objmask[b * mask_bstride + hw]
 *     disp, disp_gt: [B,1,H,W]; objmask: channel 0 of inputs[("color_objmask",0,0)] ([B,3,H,W]: mask_bstride = 3 H W);
 *     objdepth: [B] metres.  partials: dmh_sq_mean_partials_size(B*HW) floats; cost: float[1].
 *     bwd: g_disp = gscale[0] * d cost / d disp (0 where depth(disp) sits on a clamp bound, as torch.clamp does).
 * ---------------------------------------------------------------------------------- */
int dmh_gt_depth_mse_fwd(const float* disp, const float* disp_gt, const float* objmask, int64_t mask_bstride,
                         const float* objdepth, int B, int64_t HW, float min_depth, float max_depth, float* partials,
                         float* cost, void* stream);
int dmh_gt_depth_mse_bwd(const float* disp, const float* disp_gt, const float* objmask, int64_t mask_bstride,
                         const float* objdepth, int B, int64_t HW, float min_depth, float max_depth, const float* gscale,
                         float* g_disp, void* stream);

/* ------------------------------------------------------------------------------------
 * K20 weight gradients of the pair of convolutions that opens a down-sampling ResNet block (K15's train-pass counterpart):
 *     dw3[K][C][3][3] of nn.Conv2d(C, K, 3, stride 2, padding 1) and dwd[K][C][1][1] of nn.Conv2d(C, K, 1, stride 2) on the
 *     same x[B,C,H,W], from g3 / gd [B,K,H/2,W/2] (gd and dwd may be NULL: the 3x3 filter only).  Pixel axis on the fp32 MFMA,
 *     one partial block set per workgroup, fixed-order reduction: no atomics, bitwise reproducible (MIOpen's kernels for these
 *     shapes accumulate with float atomics).  C and K multiples of 64, H even, W a multiple of 8.
 *     workspace: dmh_down_wrw_workspace_size(B, C, K, H, W) floats (-1: shape not supported).
 * K21 weight gradient of the encoder's first convolution on the normalised image, nn.Conv2d(3, 64, 7, stride 2, padding 3)
 *     applied to (x - mean) / std (MD2/networks/resnet_encoder.py:89-90): dw[64][3][7][7] from x[B,3,H,W] and g[B,64,H/2,W/2];
 *     the normalisation is applied while the image tile is staged (zero in the padding), as in K14.  Same reduction scheme.
 *     H even, W a multiple of 8.  workspace: dmh_stem_wrw_workspace_size(B, H, W) floats.
 *     The workspaces of K20 and K21 must be 16-byte aligned (their reduce passes read them in 16-byte words).
 * ---------------------------------------------------------------------------------- */
int64_t dmh_down_wrw_workspace_size(int B, int C, int K, int H, int W);
int dmh_down_wrw(const float* x, const float* g3, const float* gd, int B, int C, int K, int H, int W, float* workspace, float* dw3,
                 float* dwd, void* stream);
int64_t dmh_stem_wrw_workspace_size(int B, int H, int W);
int dmh_stem_wrw(const float* x, const float* g, int B, int H, int W, float mean, float std, float* workspace, float* dw,
                 void* stream);

/* ------------------------------------------------------------------------------------
 * Stand-alone forms of the two loss layers of MD2/layers.py (Trainer.compute_losses runs the fused K1 + K2 instead; these
 * serve callers of the reference surface `SSIM()(x, y)` / `get_smooth_loss(disp, img)`):
 *   ssim_map   : out[planes,H,W] = clamp((1 - SSIM(x, y)) / 2, 0, 1), 3x3 means over the ReflectionPad2d(1) planes
 *                (MD2/layers.py:223-253).  bwd: g_x / g_y (either may be NULL); workspace: 5 * planes * H * W floats.
 *   edge_smooth: out = mean(|d_x disp| exp(-mean_c |d_x img|)) + mean(|d_y disp| exp(-mean_c |d_y img|)) for disp[B,1,H,W],
 *                img[B,C,H,W] (MD2/layers.py:207-220).  bwd: g_disp = gscale[0] * d out / d disp.
 * ---------------------------------------------------------------------------------- */
int dmh_ssim_map(const float* x, const float* y, int planes, int H, int W, float* out, void* stream);
int dmh_ssim_map_bwd(const float* x, const float* y, const float* g_out, int planes, int H, int W, float* workspace, float* g_x,
                     float* g_y, void* stream);
/* colour pyramid of the synthesised frame (inputs[("color", f, s)], s = 1..3; the reference's loader resizes per sample on the
 * CPU, MD2/datasets/mono_dataset.py:119-144): out_s[planes, H/2^s, W/2^s] = F.avg_pool2d(x, 2^s) for s = 1, 2, 3 in ONE pass
 * over x[planes, H, W], bit-identical to three ATen avg_pool2d calls.  H, W multiples of 8. */
int dmh_avg_pyramid(const float* x, int planes, int H, int W, float* out1, float* out2, float* out3, void* stream);
int64_t dmh_edge_smooth_partials_size(int B, int H, int W);
int dmh_edge_smooth(const float* disp, const float* img, int B, int C, int H, int W, float* partials, float* out, void* stream);
int dmh_edge_smooth_bwd(const float* disp, const float* img, int B, int C, int H, int W, const float* gscale, float* g_disp,
                        void* stream);

/* ------------------------------------------------------------------------------------
 * K8  attack-evaluation metrics of Trainer.val -> evaluate_attacks (MD2/evaluate_depth.py:57-99,193-197):
 *     depth = clamp(5.4 / (min_disp + (max_disp-min_disp)*|disp|), 1e-3, 80) for both disparities, then the
 *     (mask-weighted) abs_err, abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3 -> out8.  mask may be NULL.
 * ---------------------------------------------------------------------------------- */
int64_t dmh_depth_errors_partials_size(int64_t n);
int dmh_masked_depth_errors(const float* disp_gt, const float* disp_pred, const float* mask, int64_t n,
                            float min_depth, float max_depth, float scale, float clamp_lo, float clamp_hi,
                            float* partials, float* out8, void* stream);

/* ------------------------------------------------------------------------------------
 * Decoder glue (SURVEY.md section 8f direction "fuse around the convolutions"): the element-wise passes between
 * the MIOpen convolutions of the depth decoder, one pass per stage boundary.
 * Replaces MD2/networks/depth_decoder.py:54-60 (ELU, nearest upsample, torch.cat) + the ReflectionPad2d(1) of the
 * following Conv3x3 (MD2/layers.py:133-136).
 *   up_cat_pad: out[B,C1+C2,2h+2,2w+2] = pad1_reflect(cat(up2_nearest(ELU(y[B,C1,h,w])), skip[B,C2,2h,2w]))
 *   elu_pad   : out[B,C,H+2,W+2]       = pad1_reflect(ELU(z[B,C,H,W]))      (apply_elu = 0: pad only)
 * skip / g_skip may be NULL when C2 == 0.
 * ---------------------------------------------------------------------------------- */
int dmh_dec_up_cat_pad_fwd(const float* y, const float* skip, int B, int C1, int C2, int h, int w, float* out,
                           void* stream);
int dmh_dec_up_cat_pad_bwd(const float* y, const float* g_out, int B, int C1, int C2, int h, int w, float* g_y,
                           float* g_skip, void* stream);
int dmh_elu_pad_fwd(const float* z, int B, int C, int H, int W, int apply_elu, float* out, void* stream);
int dmh_elu_pad_bwd(const float* z, const float* g_out, int B, int C, int H, int W, int apply_elu, float* g_z,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * K19 windowed decoder glue + windowed attack cost: the attack evaluated only where its loss lives.
 *     cost = -mean((disp * mask)^2) (torchattacks/attacks/phy_obj_atk.py:88-97, phy_obj_atk_l0.py:118-134) reads the
 *     disparity under the pasted object only, so inside an attack the high-resolution tail of the decoder
 *     (MD2/networks/depth_decoder.py:51-63, upconv(1,0) ... dispconv(0)) runs -- exactly -- on one window per sample
 *     around the object's bounding box: the convolution kernels take compact [B,C,hc+2,wc+2] windows with padding 0,
 *     and this is the pass between them:
 *       out[b, :, i, j] = pad1_reflect(cat(up2_nearest(ELU(y)), skip))  at frame position dst_org[b] + (i, j) - 1
 *     for 0 <= i < hc + 2, 0 <= j < wc + 2: decoder_glue's up_cat_pad / elu_pad restricted to a window of the H x W
 *     destination frame (the reflection is the FRAME's).  y [B,C1,sh,sw] and skip [B,C2,kh,kw] are windows of their own
 *     frames with per-sample origins y_org / skip_org ([B,2] int32: row, column), or whole frames (origin table NULL).
 *     up: y lives at half the destination resolution; elu: ELU is applied to y.  wc must be even.
 *     Every read must fall inside the source windows (the caller's window plan guarantees it; indices are clamped).
 *   bwd: g_y / g_skip over the whole source planes (0 where no window entry reads the element) or, for whole-frame
 *     sources, over a per-sample rectangle (below); g_skip may be NULL.
 *   roi_cost: cost = sum over the windows of (sigmoid(d_pre) * mask)^2 / (B H W); d_pre [B,1,hd,wd] is the disparity
 *     head's output on the window at org[b] of the H x W frame, mask [B,1,H,W] the full-frame K3 mask; sig receives the
 *     sigmoid.  bwd: g_pre = gscale[0] * 2 sig mask^2 / (B H W) * sig (1 - sig).
 * ---------------------------------------------------------------------------------- */
typedef struct dmh_roi_glue_args {
    const float* y;
    const float* skip;      /* NULL when C2 == 0 */
    const int* y_org;       /* [B,2] or NULL (y is the whole frame) */
    const int* skip_org;    /* [B,2] or NULL */
    const int* dst_org;     /* [B,2] window origin in the destination frame (unpadded coordinates) */
    int B, C1, C2;
    int sh, sw;             /* plane size of y */
    int kh, kw;             /* plane size of skip */
    int hc, wc;             /* destination window (unpadded); out is [B, C1 + C2, hc + 2, wc + 2] */
    int H, W;               /* destination frame (unpadded) */
    int up, elu;
} dmh_roi_glue_args;
int dmh_roi_glue_fwd(const dmh_roi_glue_args* a, float* out, void* stream);
/* y_reg_org / skip_reg_org ([B,2] int32 or NULL): for a whole-frame source, write only the y_reg_h x y_reg_w rectangle at
 * that per-sample origin (it must hold everything the window reaches; the caller owns the rest of the plane). */
int dmh_roi_glue_bwd(const dmh_roi_glue_args* a, const float* g_out, float* g_y, float* g_skip, const int* y_reg_org,
                     int y_reg_h, int y_reg_w, const int* skip_reg_org, int skip_reg_h, int skip_reg_w, void* stream);
int64_t dmh_roi_cost_partials_size(int B, int hd, int wd);
int dmh_roi_cost_fwd(const float* d_pre, const float* mask, const int* org, int B, int hd, int wd, int H, int W, float* sig,
                     float* partials, float* cost, void* stream);
int dmh_roi_cost_bwd(const float* sig, const float* mask, const int* org, int B, int hd, int wd, int H, int W,
                     const float* gscale, float* g_pre, void* stream);
/* scale = +1 or -1: the attacks MAXIMISE the cost, i.e. hand autograd -mean(.) (phy_obj_atk.py:95 `cost = -loss(...)`); with
 * scale = -1 the sign is applied here (bit-identical to negating the result and the incoming gradient: two element-wise
 * launches per attack step less). */
int dmh_roi_cost_fwd_scaled(const float* d_pre, const float* mask, const int* org, int B, int hd, int wd, int H, int W,
                            float scale, float* sig, float* partials, float* cost, void* stream);
int dmh_roi_cost_bwd_scaled(const float* sig, const float* mask, const int* org, int B, int hd, int wd, int H, int W,
                            float scale, const float* gscale, float* g_pre, void* stream);

/* K19, encoder side: the backward of conv1 / bn1 / relu / maxpool and layer1 (torchvision ResNet under
 * MD2/networks/resnet_encoder.py:85-98) on one window per scene -- the patch gradient reads d cost / d image under the pasted
 * object only (physicalTrans.py:156-165, phy_obj_atk.py:96).
 *   roi_crop: out[B,C,hc,wc] = src[b, c, org_b + (i, j)] of a whole-frame src[B,C,H,W], times [gate > 0] (gate: whole-frame,
 *             same window; gate_compact != 0: gate is itself a compact [B,C,hc,wc] window at org) when gate is given; or, with g
 *             (compact [B,C,hc,wc]) instead of src, out = g * [gate window > 0].
 *             org [B,2] int32 with even columns, wc and W even.
 *   stem_bn_relu_pool_bwd_win: dmh_stem_bn_relu_pool_bwd on the hs x ws window (even origin org, even sizes) of the H x W
 *             map: g_z[B,C,hs,ws] compact; g_pool is a compact [B,C,hq,wq] window of the H/2 x W/2 map at pool_org (cells
 *             outside it count as 0: it must hold the pooling cells that cover the window); g_feat whole-frame or NULL. */
int dmh_roi_crop(const float* src, const float* gate, const float* g, const int* org, int B, int C, int H, int W, int hc,
                 int wc, int gate_compact, float* out, void* stream);
/* roi_paste: dst[b, c, win_org_b + (i, j)] = src at the same frame position, for the h x w window: src is a compact
 * [B,C,sh,sw] window at frame origin src_org [B,2] that holds it, or (src_org NULL, sh x sw = H x W) a whole-frame tensor.
 * The incremental attack forward writes the part of encoder feature 1 that the pasted object changes into the cached
 * feature of the clean scenes, and puts the clean values back afterwards. */
int dmh_roi_paste(const float* src, const int* src_org, int sh, int sw, const int* win_org, int B, int C, int H, int W, int h,
                  int w, float* dst, void* stream);
int dmh_stem_bn_relu_pool_bwd_win(const float* feat, const unsigned char* argmax, const float* g_feat, const float* g_pool,
                                  const float* scale, const int* org, const int* pool_org, int B, int C, int H, int W, int hs,
                                  int ws, int hq, int wq, float* g_z, void* stream);

/* ------------------------------------------------------------------------------------
 * K9  encoder glue: the element-wise passes between the MIOpen convolutions of the ResNet encoder while the model
 *     is in eval() mode (every attack step: torchattacks/attack.py:165-182 brackets the attack with model.eval()).
 *     Replaces, in MD2/networks/resnet_encoder.py:85-98 / torchvision BasicBlock.forward, the chains
 *     BatchNorm2d(eval) -> [+ identity] -> ReLU and, in the stem, BatchNorm2d(eval) -> ReLU -> MaxPool2d(3, 2, 1).
 *     scale[c] = weight / sqrt(running_var + eps), shift[c] = bias - running_mean * scale (computed by the caller).
 *   bn_act : out[B,C,HW] = act(x * scale[c] + shift[c] (+ residual)),  act = ReLU when relu != 0.  residual may be NULL.
 *            bwd: g_residual = relu ? g_out * [out > 0] : g_out (written when non-NULL);  g_x = g_residual * scale[c].
 *            `out` may be NULL in the backward when relu == 0.
 *   stem   : feat[B,C,H,W] = ReLU(x * scale[c] + shift[c]); pooled[B,C,H/2,W/2] = maxpool3x3/2/1(feat);
 *            argmax[B,C,H/2,W/2] (u8, ky*3+kx, first maximum in scan order as ATen's max_pool2d).  H, W even.
 *            bwd: g_x = scale[c] * [feat > 0] * (g_feat + maxpool_adjoint(g_pooled));  either gradient may be NULL.
 * ---------------------------------------------------------------------------------- */
int dmh_bn_act_fwd(const float* x, const float* scale, const float* shift, const float* residual, int B, int C, int HW,
                   int relu, float* out, void* stream);
int dmh_bn_act_bwd(const float* out, const float* g_out, const float* scale, int B, int C, int HW, int relu, float* g_x,
                   float* g_residual, void* stream);
/* train-mode BatchNorm statistics (model.train(): the training pass of MD2/trainer.py:335-375): per-channel batch mean
 * and biased variance of x[B,C,HW] (two launches, fp32 Welford/Chan combination of shifted sums), from which
 *   scale = weight * invstd, shift = bias - mean * scale      (feed dmh_bn_act_fwd / dmh_stem_bn_relu_pool_fwd)
 *   save_mean, save_invstd                                    (for aten::native_batch_norm_backward)
 * and running_mean / running_var are updated in place with `momentum` (unbiased variance), as nn.BatchNorm2d does.
 * weight / bias / running_* may be NULL.  partials: dmh_bn_stats_partials_size(B, C, HW) floats of scratch. */
int64_t dmh_bn_stats_partials_size(int B, int C, int HW);
/* Also num_batches_tracked[0] += 1 (the module's int64 counter, nn.BatchNorm2d.forward in train mode; may be NULL) in the
 * second launch instead of one more element-wise launch per BatchNorm (20 per train pass of the ResNet-18 encoder). */
int dmh_bn_train_stats_tracked(const float* x, int B, int C, int HW, const float* weight, const float* bias, float momentum,
                               float eps, float* running_mean, float* running_var, long long* num_batches_tracked,
                               float* partials, float* scale, float* shift, float* save_mean, float* save_invstd,
                               void* stream);
/* out[c] = sum over (b, hw) of g[b][c][hw]: the bias gradient of a convolution (aten::convolution_backward's third
 * output, aten::sum(g, (0, 2, 3))).  Two launches, fixed order.  partials: dmh_channel_sum_partials_size(B, C, HW) floats. */
int64_t dmh_channel_sum_partials_size(int B, int C, int HW);
int dmh_channel_sum(const float* g, int B, int C, int HW, float* partials, float* out, void* stream);
/* train-mode BatchNorm backward with the ReLU mask folded in (replaces one dmh_bn_act_bwd pass +
 * aten::miopen_batch_norm_backward in the train pass; torch.nn.BatchNorm2d semantics, torch/nn/functional.py batch_norm
 * as called by torchvision's BasicBlock, MD2/networks/resnet_encoder.py:85-98):
 *   g' = out ? g_out * [out > 0] : g_out;   g_bias = sum g';   g_weight = invstd * sum g' (x - mean);
 *   g_x = weight invstd ( g' - g_bias / N - (x - mean) invstd^2 sum g' (x - mean) / N ),  N = B * HW.
 * out (the saved ReLU output), weight (NULL = 1), g_weight, g_bias, g_pre (receives g', the gradient of a residual branch)
 * may be NULL.  workspace: dmh_bn_train_bwd_workspace_size(B, C, HW) floats, 16-byte aligned.  Three launches, fixed-order
 * sums: bitwise reproducible. */
int64_t dmh_bn_train_bwd_workspace_size(int B, int C, int HW);
int dmh_bn_train_bwd(const float* x, const float* g_out, const float* out, const float* weight, const float* save_mean,
                     const float* save_invstd, int B, int C, int HW, float* workspace, float* g_x, float* g_weight,
                     float* g_bias, float* g_pre, void* stream);
int dmh_stem_bn_relu_pool_fwd(const float* x, const float* scale, const float* shift, int B, int C, int H, int W,
                              float* feat, float* pooled, unsigned char* argmax, void* stream);
int dmh_stem_bn_relu_pool_bwd(const float* feat, const unsigned char* argmax, const float* g_feat, const float* g_pooled,
                              const float* scale, int B, int C, int H, int W, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------
 * K10 3x3 stride-1 convolution, Winograd F(2x2,3x3) on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32).
 *     Replaces the MIOpen call behind nn.Conv2d(.., 3, 1, pad) in torchvision BasicBlock (encoder,
 *     MD2/networks/resnet_encoder.py:85-98) and Conv3x3 (decoder, MD2/layers.py:127-141), forward and backward-data.
 *   weight_transform: U = G w G^T in the chunked layout the kernel streams; `backward` != 0 builds the filter of the
 *                     backward-data pass (flipped, channel roles swapped).  U holds dmh_wino_weight_size(n_out, n_in)
 *                     floats, n_out/n_in = channel roles of that pass; n_in must be a multiple of 8.
 *   conv3x3         : y[B,K,H+2pad-2,W+2pad-2] = corr3x3(zero_pad(x[B,C,H,W], pad), w) (+ bias[K]);  pad in {0,1,2};
 *                     output height and width must be even.  Backward-data of a pad-p convolution is this call on
 *                     g_out with the backward filter and pad = 2 - p.
 * ---------------------------------------------------------------------------------- */
int64_t dmh_wino_weight_size(int n_out, int n_in);
int dmh_wino_weight_transform(const float* w, int K, int C, int backward, float* U, void* stream);
int dmh_wino_conv3x3(const float* x, const float* U, const float* bias, int B, int C, int K, int H, int W, int pad,
                     float* y, void* stream);
/* The same with a caller-owned workspace (device, 16-byte aligned, workspace_floats floats; the library keeps nothing).
 * With whole work items (64 output channels x 64 tiles x ALL input channels) a launch lasts ceil(items / CUs) item times: 288
 * items on 256 CUs take two rounds, 60 items leave 196 CUs idle.  Given a workspace of 2 * CUs * 16,384 floats (32 MB on
 * MI355X) the launch is decomposed stream-K style instead: the (item, 8-channel chunk) units are dealt to the workgroups in
 * equal contiguous ranges, a range that begins or ends inside an item stores that item's partial sums to the workspace,
 * and a second kernel adds an item's pieces in chunk order + bias -- deterministic, no atomics, no zero fill.  Taken only
 * where a cost model says it is faster; NULL / too small a workspace = dmh_wino_conv3x3. */
int dmh_wino_conv3x3_ws(const float* x, const float* U, const float* bias, int B, int C, int K, int H, int W, int pad,
                        float* y, float* workspace, int64_t workspace_floats, void* stream);
/* What a dmh_wino_conv3x3(_act)_ws call of this shape would do, WITHOUT launching: -1 for a shape the kernel does not take, else
 * bit 0: stream-K form, bit 1: two-way channel split, bits 2-3: tile regions (0: 2 x 32 per image, 1: 4 x 16 per image, 2: 4 x 16
 * over the flattened batch), bits 8...: work items.  `epilogue` != 0 asks for the _act form; workspace_floats = the size the
 * caller would pass (0: none).  The caller's dispatch rule (ops._wino_ok) asks this instead of mirroring the decision. */
int dmh_wino_conv3x3_plan(int B, int C, int K, int H, int W, int pad, int epilogue, int64_t workspace_floats);
/* conv -> BatchNorm(eval) -> (+ identity) -> ReLU of a BasicBlock in one launch (torchvision BasicBlock.forward under
 * MD2/networks/resnet_encoder.py:85-98, model in eval()): the per-channel scale is folded into the filter by
 * weight_transform_scaled (backward != 0: into the filter of the backward-data pass, whose input is then the masked
 * output gradient), the shift is `bias`, `residual` (same shape as y, may be NULL) is added before the ReLU.
 *   y = act(corr3x3(zero_pad(x), w * scale[k]) + bias[k] (+ residual)),  act = ReLU when relu & 1.
 * relu & 2: `residual` is not an addend but a saved ReLU output m: y = (corr3x3(...) + bias[k]) * [m > 0] -- the
 * backward-data pass of one convolution of a block, masked for the ReLU in front of it, in the same launch. */
int dmh_wino_weight_transform_scaled(const float* w, int K, int C, int backward, const float* scale, float* U,
                                     void* stream);
int dmh_wino_conv3x3_act(const float* x, const float* U, const float* bias, const float* residual, int relu, int B, int C,
                         int K, int H, int W, int pad, float* y, void* stream);
/* Many filters in one launch: jobs[i] = one dmh_wino_weight_transform_scaled call (scale may be NULL); `jobs` is a HOST array,
 * read before the call returns (its entries travel in the kernel arguments, 32 per launch).  A training step re-transforms
 * every filter twice (forward and backward-data form, once for the attack's frozen weights and once for the train pass): ~76
 * launches of 5-20 us otherwise. */
typedef struct dmh_wino_wt_job {
    const float* w;         /* [K][C][3][3] */
    const float* scale;     /* per-channel factor of the forward OUTPUT (eval-mode BatchNorm), or NULL */
    float* U;               /* dmh_wino_weight_size(n_out, n_in) floats */
    int K, C, backward;
} dmh_wino_wt_job;
int dmh_wino_weight_transform_batch(const dmh_wino_wt_job* jobs, int n, void* stream);
/* The same with a caller-owned stream-K workspace (see dmh_wino_conv3x3_ws).  With the fused epilogue only launches of fewer
 * than 200 tile regions are decomposed (layer4 at the attack batch: 120); the second kernel applies shift / residual / ReLU. */
int dmh_wino_conv3x3_act_ws(const float* x, const float* U, const float* bias, const float* residual, int relu, int B, int C,
                            int K, int H, int W, int pad, float* y, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------
 * K17 the 32-output-channel form of K10 (work item 32 channels x 128 tiles): the decoder layers whose output channel
 *     count is a multiple of 32 but not of 64 -- upconv(1,0) 64 -> 32 and upconv(1,1) 96 -> 32 forward, 32 -> 96
 *     backward-data (MD2/networks/depth_decoder.py:51-63 via MD2/layers.py:127-141 Conv3x3).  Same contract as
 *     dmh_wino_conv3x3; its own filter layout (channel rows padded to 32 instead of 64): weight_size / weight_transform.
 * ---------------------------------------------------------------------------------- */
int64_t dmh_wino32_weight_size(int n_out, int n_in);
int dmh_wino32_weight_transform(const float* w, int K, int C, int backward, float* U, void* stream);
int dmh_wino32_conv3x3(const float* x, const float* U, const float* bias, int B, int C, int K, int H, int W, int pad,
                       float* y, void* stream);
/* The same with a caller-owned stream-K workspace (see dmh_wino_conv3x3_ws): 2 * CUs * 16,384 floats. */
int dmh_wino32_conv3x3_ws(const float* x, const float* U, const float* bias, int B, int C, int K, int H, int W, int pad,
                          float* y, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------------------------
 * K18 weight gradient of a 3x3 stride-1 convolution with C and K multiples of 64, in the Winograd F(2x2,3x3) domain on the
 *     fp32 MFMA: dw[K][C][3][3] = d/dw sum(dy * corr3x3(zero_pad(x, pad), w)) -- what autograd asks
 *     aten.convolution_backward(dy, x, w, ..., [False, True, False]) for in the train pass (MD2/trainer.py:305-309 backward
 *     through torchvision BasicBlock / MD2/layers.py:127-141 Conv3x3).  x [B,C,H,W], dy [B,K,H+2pad-2,W+2pad-2] (even sizes);
 *     workspace: dmh_wino_wrw_workspace_size(...) floats, 16-byte aligned (per-workgroup partial sums, added in a fixed order:
 *     no atomics).
 * ---------------------------------------------------------------------------------- */
int64_t dmh_wino_wrw_workspace_size(int B, int C, int K, int H, int W, int pad);
int dmh_wino_wrw(const float* x, const float* dy, int B, int C, int K, int H, int W, int pad, float* workspace, float* dw,
                 void* stream);

/* ------------------------------------------------------------------------------------
 * K11 3x3 stride-1 convolution with few channels (<=4 -> <=32, 16 -> <=32 or 32 -> <=16) at full resolution, direct implicit
 *     GEMM on v_mfma_f32_16x16x4_f32 with the filter held in registers: the last decoder stage and the disparity heads
 *     (MD2/networks/depth_decoder.py:38-44).  w is the FORWARD filter [Kw][Cw][3][3] in both directions:
 *       backward == 0:  y[B,Kw,H+2pad-2,W+2pad-2] = corr3x3(zero_pad(x[B,Cw,H,W], pad), w) + bias
 *       backward != 0:  y[B,Cw,...]               = corr3x3(zero_pad(x[B,Kw,H,W], pad), flip(w)^T)   (bias ignored if NULL)
 *     so the gradient w.r.t. the input of a pad-p convolution is the backward call on g_out with pad = 2 - p.
 * ---------------------------------------------------------------------------------- */
int dmh_conv3x3_small(const float* x, const float* w, const float* bias, int B, int Kw, int Cw, int H, int W, int pad,
                      int backward, float* y, void* stream);

/* ------------------------------------------------------------------------------------
 * K12 gradient w.r.t. the input image of the encoder's first convolution, nn.Conv2d(Cin, K, 7, stride 2, padding 3)
 *     (torchvision ResNet.conv1, MD2/networks/resnet_encoder.py:88): g_x[B,Cin,H,W] from g_y[B,K,H/2,W/2] and the forward
 *     filter w[K][Cin][7][7].  Direct gather, no atomics.  Cin <= 4, K a multiple of 8, H and W even.
 * ---------------------------------------------------------------------------------- */
int dmh_conv7x7s2_bwd_data(const float* g_y, const float* w, int B, int K, int Cin, int H, int W, float* g_x,
                           void* stream);
/* Launch form of dmh_conv7x7s2_bwd_data for this shape (host only, no launch): 4 = four channel groups per workgroup on a
 * quarter of the rows (fewer than 2048 workgroups of 16 x 64 pixels), 1 = one group per workgroup; -1: bad shape. */
int dmh_conv7x7s2_bwd_data_ksplit(int B, int H, int W);
/* Window form (K19): only the hwin x wwin window of g_x at the per-sample, even pixel origin img_org [B,2] is written (at its
 * place in the whole [B,Cin,H,W] tensor); g_y is a compact [B,K,sh,sw] window of the H/2 x W/2 frame at origin gy_org [B,2]
 * that must hold rows / columns (img_org / 2 - 1) .. ((img_org + hwin) / 2 + 1) of that frame as far as they lie inside it. */
int dmh_conv7x7s2_bwd_data_win(const float* g_y, const float* w, const int* img_org, const int* gy_org, int B, int K, int Cin,
                               int H, int W, int hwin, int wwin, int sh, int sw, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------
 * K13 disparity head: 3x3 stride-1 convolution to ONE output channel (MD2/networks/depth_decoder.py:43-44 dispconv),
 *     forward: y[B,1,H+2pad-2,W+2pad-2] = corr3x3(zero_pad(x[B,C,H,W], pad), w[1][C][3][3]) + bias[0].
 *     pad 0 (the heads on the reflection-padded features): strips of 62 columns x 40 rows per wave, one load per input
 *     row, neighbours by DPP, C a multiple of 4; otherwise vector FMAs on an LDS tile, C a multiple of 16.
 * ---------------------------------------------------------------------------------- */
int dmh_conv3x3_head(const float* x, const float* w, const float* bias, int B, int C, int H, int W, int pad, float* y,
                     void* stream);
/* Which kernel dmh_conv3x3_head launches for this shape (host only, no launch): 1 = strips, 0 = LDS tile, -1 = a shape it
 * rejects. */
int dmh_conv3x3_head_fwd_form(int B, int C, int H, int W, int pad);
/* gradient w.r.t. the input of the same layer at pad 0: g_x[B,C,H,W] from g[B,1,H-2,W-2] (full correlation with the
 * flipped filter); C a multiple of 4.  One gradient plane in registers, C planes streamed out. */
int dmh_conv3x3_head_bwd_data(const float* g, const float* w, int B, int C, int H, int W, float* g_x, void* stream);
/* Waves that share a strip of g_x in dmh_conv3x3_head_bwd_data (channel split; host only): 1 from 2048 strips of 62 x 20
 * pixels on, 4 below; -1: bad shape. */
int dmh_conv3x3_head_bwd_data_nsplit(int B, int C, int H, int W);
/* weight and bias gradient of the same layer (train pass): g_w[1][C][3][3] = sum_{b,y,x} g[b,0,y,x] * zero_pad(x)[b,c,y+ky,x+kx],
 * g_b[0] = sum g (g_b may be NULL).  `partials`: dmh_conv3x3_head_wrw_partials_size(...) floats of workspace (per-strip
 * sums, added in a fixed order: deterministic).  Any C. */
int64_t dmh_conv3x3_head_wrw_partials_size(int B, int C, int H, int W, int pad);
/* Launch form of dmh_conv3x3_head_wrw (host only): strips of 62 x 40 outputs, and the waves per strip that share its
 * channels (doubled while strips x groups < 4096 and the groups divide C); -1: bad shape. */
int64_t dmh_conv3x3_head_wrw_strips(int B, int C, int H, int W, int pad);
int dmh_conv3x3_head_wrw_channel_groups(int B, int C, int H, int W, int pad);
int dmh_conv3x3_head_wrw(const float* x, const float* g, int B, int C, int H, int W, int pad, float* partials, float* g_w,
                         float* g_b, void* stream);

/* ------------------------------------------------------------------------------------
 * K16 weight and bias gradient of the 3x3 stride-1 convolutions with 16 OUTPUT channels and 16 or 32 input channels (the
 *     last decoder stage, MD2/networks/depth_decoder.py:38-41 upconv(0,0) / upconv(0,1); train pass):
 *     g_w[16][C][3][3] = sum_{b,y,x} g[b,k,y,x] * zero_pad(x)[b,c,y+ky,x+kx],  g_b[16] = sum g  (g_b may be NULL).
 *     Pixel axis on the fp32 MFMA; `partials`: dmh_conv3x3_small_wrw_partials_size(C) floats of workspace
 *     (per-workgroup sums, added in a fixed order: deterministic).
 * ---------------------------------------------------------------------------------- */
int64_t dmh_conv3x3_small_wrw_partials_size(int C);
int dmh_conv3x3_small_wrw(const float* x, const float* g, int B, int C, int H, int W, int pad, float* partials, float* g_w,
                          float* g_b, void* stream);

/* ------------------------------------------------------------------------------------
 * K14 the encoder's first layer with its input normalisation fused (MD2/networks/resnet_encoder.py:89-90:
 *     x = (input_image - 0.45) / 0.225;  x = conv1(x),  conv1 = nn.Conv2d(3, 64, 7, stride 2, padding 3, bias=False)):
 *     y[B,64,H/2,W/2] = corr7x7_s2(zero_pad3((x[B,3,H,W] - mean) / std), w[64][3][7][7]) on the exact-fp32 MFMA.
 *     H and W even.  The gradient w.r.t. x is dmh_conv7x7s2_bwd_data(g_y, w) / std.
 * ---------------------------------------------------------------------------------- */
int dmh_stem_conv_norm_fwd(const float* x, const float* w, int B, int H, int W, float mean, float std, float* y,
                           void* stream);
/* Launch geometry of dmh_stem_conv_norm_fwd (host only): tiles of 4 x 32 outputs and the workgroups that run them (at most
 * 512: persistent over the tiles beyond that); -1: bad shape. */
int64_t dmh_stem_conv_norm_fwd_tiles(int B, int H, int W);
int dmh_stem_conv_norm_fwd_workgroups(int B, int H, int W);
/* Window form (K19): only the hw x ww window of the H/2 x W/2 output at the per-sample origin org [B,2] is computed, into a
 * compact y[B,64,hw,ww]; x stays the whole image (zero padding outside it as above). */
int dmh_stem_conv_norm_fwd_win(const float* x, const float* w, const int* org, int B, int H, int W, int hw, int ww, float mean,
                               float std, float* y, void* stream);

/* ------------------------------------------------------------------------------------
 * K15 the two convolutions that open a down-sampling ResNet block (torchvision BasicBlock.conv1 with stride 2 and
 *     BasicBlock.downsample[0], the layers behind MD2/networks/resnet_encoder.py:94-98), one launch per direction:
 *     fwd:  y3[B,Co,H/2,W/2] = corr3x3_s2(zero_pad1(x[B,Ci,H,W]), w3[Co][Ci][3][3]);
 *           yd[B,Co,H/2,W/2] = corr1x1_s2(x, wd[Co][Ci])                      (wd, yd both NULL: 3x3 only)
 *     bwd:  g_x[B,Ci,H,W] = adjoint3x3(g3) + adjoint1x1(gd) with the filters TRANSPOSED: w3t[Ci][Co][3][3],
 *           wdt[Ci][Co]                                                      (gd, wdt both NULL: 3x3 only)
 *     Exact-fp32 MFMA.  H, W even; fwd: Ci % 8 == 0, Co % 64 == 0; bwd: Co % 8 == 0, Ci % 64 == 0.
 * ---------------------------------------------------------------------------------- */
/* fwd with eval-mode BatchNorms folded in (scales already in the filters): y3 = act(corr3x3_s2(x, w3) + shift3[k]),
 * act = ReLU when relu3 != 0; yd = corr1x1_s2(x, wd) + shiftd[k]; shift3 / shiftd may be NULL (both, relu3 = 0: as above). */
int dmh_down_conv_fwd_act(const float* x, const float* w3, const float* wd, const float* shift3, const float* shiftd,
                          int relu3, int B, int Cin, int Cout, int H, int W, float* y3, float* yd, void* stream);
/* bwd with g_add[B, Cin, H, W] (may be NULL) added in the epilogue: the gradient the same tensor receives from its other
 * consumer (the decoder's skip connection), instead of autograd's separate accumulation pass. */
int dmh_down_conv_bwd_data_acc(const float* g3, const float* gd, const float* w3t, const float* wdt, const float* g_add, int B,
                               int Cin, int Cout, int H, int W, float* g_x, void* stream);

/* Round 5: the same two kernels with 16-byte loaders.  The filters are handed over as an IMAGE of the kernels' LDS layout,
 * written once per weight tensor: image[rows / 32][inner / 8][2560] from w3[rows][inner][3][3] and wd[rows][inner] (NULL: zeros)
 * -- forward: rows = Co, inner = Ci (the filters as they are); backward: rows = Ci, inner = Co (the TRANSPOSED filters w3t, wdt).
 * dmh_down_conv_image_size: floats of the image, -1 unless rows % 32 == 0 and inner % 8 == 0.  The *_img entry points take the
 * arguments of dmh_down_conv_fwd_act / dmh_down_conv_bwd_data_acc with the image in place of the filter pair and a flag for the
 * shortcut convolution; they read the tensors in aligned 16-byte words and therefore need W % 4 == 0 (forward) / W % 8 == 0
 * (backward) -- other shapes stay with the entry points above.  Results are bit-identical to theirs. */
int64_t dmh_down_conv_image_size(int rows, int inner);
int dmh_down_conv_weight_image(const float* w3, const float* wd, int rows, int inner, float* image, void* stream);
int dmh_down_conv_fwd_img(const float* x, const float* image, int has_down, const float* shift3, const float* shiftd, int relu3,
                          int B, int Cin, int Cout, int H, int W, float* y3, float* yd, void* stream);
int dmh_down_conv_bwd_data_img(const float* g3, const float* gd, const float* image, const float* g_add, int B, int Cin, int Cout,
                               int H, int W, float* g_x, void* stream);

/* ------------------------------------------------------------------------------------
 * K29 the pose head: the tail of the pose decoder (MD2/networks/pose_decoder.py:47-52: out.mean(3).mean(2), 0.01 *, view, split)
 *     and transformation_from_parameters (MD2/layers.py:28-103), one launch per direction.
 *     fwd:  x[B][6 nf][h][w] -> axisangle[B][nf][1][3], translation[B][nf][1][3] = scale * channel means (scale = 0.01 in the
 *           decoder), T[B][nf][4][4] = Trans(t) Rot(a), or Rot(a)^T Trans(-t) for the frames whose bit of invert_mask is set
 *           (negative frame ids, MD2/trainer.py:408-410).  Fixed-order sums, precise sinf / cosf, the angle + 1e-7 of the axis.
 *     bwd:  g_x[B][6 nf][h][w] = (d / d (scale * mean)) * scale / (h w), broadcast, from g_T and the optional g_axisangle /
 *           g_translation (any may be NULL, not all three) and the forward's axisangle / translation.  At a zero axis-angle the
 *           gradient of the norm is taken as 0 (torch's norm backward); the output is finite.
 *     B <= 65535, nf <= 32, h w < 2^24.  Bitwise reproducible; the invert flags travel as a kernel argument.
 * ---------------------------------------------------------------------------------- */
int dmh_pose_head_fwd(const float* x, int B, int nf, int h, int w, float scale, uint32_t invert_mask, float* axisangle,
                      float* translation, float* T, void* stream);
int dmh_pose_head_bwd(const float* g_T, const float* g_axisangle, const float* g_translation, const float* axisangle,
                      const float* translation, int B, int nf, int h, int w, float scale, uint32_t invert_mask, float* g_x,
                      void* stream);

/* ------------------------------------------------------------------------------------
 * K30 ManyDepth's matching cost volume, forward only (manydepth2/networks/resnet_encoder.py:157-236 match_features, :258-265
 *     compute_confidence_mask, :294-296 the argmin of forward).  The reference computes it under no_grad; the backward is K38.
 *     current[B][C][H][W], lookup[B][L][C][H][W] (layer-1 features), poses[Bp][L][4][4], K / invK[B][4][4], bins[D] (depths).
 *     Per (b, d, h, w, l): the reference's fp32 position arithmetic without contraction, bilinear sample (zero padding,
 *     align_corners), mean over channels of |warped - current| times the edge mask and the current frame's border mask; summed
 *     over the lookups and divided by (count of positive diffs + 1e-7).  Lookup l of sample b is skipped when the 16 entries of
 *     poses[b][l] sum to exactly 0 or b >= Bp: decided on the device, no host read.
 *     cost_volume / missing[B][D][H][W] (missing = cost == 0; with set_missing_to_max those entries take the maximum over the
 *     bins), confidence[B][H][W] (all D bins observed), argmin[B][H][W] (int32; zeros read as 100, first minimum).  cost_volume,
 *     missing and buffer may be NULL; buffer[B][C + D][H][W] receives cost_volume * confidence in channels C .. C + D - 1.
 *     nhwc: workspace of B L C H W floats (the lookup features channels-last).  banded != 0: workgroups that share an XCD take a
 *     contiguous band of tiles (speed only).  C = 64, D <= 128, L <= 16, 1 <= Bp <= B, H, W >= 5, H W C < 2^31.  Two launches,
 *     no atomics: bitwise reproducible.
 * ---------------------------------------------------------------------------------- */
int dmh_cost_volume_fwd(const float* current, const float* lookup, const float* poses, const float* K, const float* invK,
                        const float* bins, int B, int L, int Bp, int C, int H, int W, int D, int set_missing_to_max, int banded,
                        float* nhwc, float* cost_volume, float* missing, float* confidence, int32_t* argmin, float* buffer,
                        void* stream);

/* ------------------------------------------------------------------------------------
 * K38 backward of the matching cost volume (this project's addition: the reference has none).  Differentiates
 *     V[b][d][h][w] = cost_volume[b][d][h][w] * confidence[b][h][w] (what K30 writes into `buffer`) with respect to current and
 *     lookup as torch autograd differentiates the module expression: sample positions, edge / border masks, counts, missing and
 *     confidence are constants, so only confident columns carry gradient and set_missing_to_max plays no part.  With
 *     dtotal[d] = g[d] / (counts[d] + 1e-7) in a confident column:
 *       d_current[b][c][h][w] = -(1/C) sum_{d,l} dtotal[d] edge_l[d] sgn(warped_l[c][d] - current[c]),   sgn(0) = 0;
 *       d_lookup[b][l][c] receives (1/C) dtotal[d] edge_l[d] sgn(...) through the four bilinear weights of the sample.
 *     Inputs and limits as K30 (the positions are K30's own arithmetic; skipped lookups are decided on the device and get exact
 *     zeros).  g: element (b, d, h, w) at g[b * g_batch_stride + (d * H + h) * W + w], so channels C .. C + D - 1 of a
 *     [B][C + D][H][W] gradient are read in place (g + C H W, stride (C + D) H W).  g must be finite.
 *     d_current[B][C][H][W], d_lookup[B][L][C][H][W]: either may be NULL, not both; both are overwritten (no need to zero them).
 *     Workspaces: nhwc (B L C H W floats), dtotal (B D H W floats), acc (B L C H W + 1 int64 words; may be NULL when d_lookup is).
 *     d_current is a gather; d_lookup is accumulated in 64-bit fixed point with integer atomics, the scale taken on the device
 *     from max|dtotal| (csrc/cost_volume_bwd.hip states the bound): no float atomics, bitwise reproducible, no host read.
 * ---------------------------------------------------------------------------------- */
int dmh_cost_volume_bwd(const float* current, const float* lookup, const float* poses, const float* K, const float* invK,
                        const float* bins, int B, int L, int Bp, int C, int H, int W, int D, const float* g, int64_t g_batch_stride,
                        float* nhwc, float* dtotal, int64_t* acc, float* d_current, float* d_lookup, void* stream);

/* ------------------------------------------------------------------------------------
 * K31 Pillow's 8-bit separable resample, Image.resize(size, filter) of mode RGB / L with reducing_gap=None, bit for bit
 *     (MD2/datasets/mono_dataset.py:100-104,119-144: the loader's four-level ANTIALIAS chain).  One launch per level: a
 *     workgroup takes DMH_PIL_TILE_ROWS output rows of one channel of one image, runs the horizontal pass for the source rows
 *     those need into an 8-bit LDS tile (``lds_rows`` rows of W_out bytes), then the vertical pass from the tile.  Integer
 *     arithmetic only: pixel = clip((2^21 + sum(p * k)) >> 22, 0, 255) per pass, Pillow's own 32-bit sums.
 *     tables: int32 words, every axis table laid out as min[out] | count[out] | k[ksize][out] (k has 22 fraction bits; a pass
 *     whose size does not change is the table with ksize 1 and k = 2^22, which reproduces the pixel).  They are made on the
 *     host in float64 (ops.pil_axis_table); dmh_pil_resample_tables_size(in, out, filter) is the word count of one table, -1
 *     for sizes it does not take.  filter: DMH_PIL_BILINEAR (support 1) or DMH_PIL_LANCZOS (support 3).
 *     desc: int32 [N][8] per image = source rows, source columns, word offset and ksize of its horizontal table, word offset and
 *     ksize of its vertical table, 0, 0.  flip (int32 [N], may be NULL): != 0 mirrors the read of the source column, which is
 *     transpose(FLIP_LEFT_RIGHT) before the resize.
 *     src: element (n, c, y, x) at n sn + c sc + y sy + x sx (elements), uint8, or float32 when src_f32 != 0, quantised on read
 *     as ToPILImage does: (uint8)(v * 255.f).  Hs, Ws: the rows and columns the buffer holds per image (every image's own size
 *     is <= them; reads are clamped to them).
 *     out_u8 [N][C][H_out][W_out] and out_f32 = (float)u8 / 255.f (IEEE division) of the same shape; either may be NULL, not both.
 *     N, C <= 65535, every buffer < 2^31 elements, lds_rows W_out <= 65536.  No atomics, no host read; bitwise reproducible.
 * ---------------------------------------------------------------------------------- */
#define DMH_PIL_BILINEAR 2
#define DMH_PIL_LANCZOS 1
#define DMH_PIL_TILE_ROWS 8
int64_t dmh_pil_resample_tables_size(int in_size, int out_size, int filter);
int dmh_pil_resample(const void* src, int src_f32, int64_t sn, int64_t sc, int64_t sy, int64_t sx, int Hs, int Ws,
                     const int32_t* tables, int64_t table_words, const int32_t* desc, const int32_t* flip, int N, int C,
                     int H_out, int W_out, int lds_rows, uint8_t* out_u8, float* out_f32, void* stream);

/* ------------------------------------------------------------------------------------
 * K32 The sparse depth maps of a batch of velodyne scans: MD2/kitti_utils.py:46-98 (generate_depth_map) with the loader's
 *     nearest resize and flip (MD2/datasets/kitti_dataset.py:70-85), float32-equal to the reference.
 *     points: float32 [npts][4] (x forward, y left, z up, reflectance: ignored, the reference overwrites it with 1), the frames
 *     packed one after the other; offsets: int32 [n + 1], frame f owns the points offsets[f] .. offsets[f + 1] - 1 in file order.
 *     proj: float64 [n][12], the row-major 3 x 4 P_velo2im of each frame.  A point is kept if x >= 0; q = P (x, y, z, 1) in float64
 *     as ((P[r][0] x + P[r][1] y) + P[r][2] z) + P[r][3] without contraction; u = rint(q0 / q2) - 1, v = rint(q1 / q2) - 1, kept
 *     if 0 <= u < W and 0 <= v < H; the value is q2, or x when vel_depth != 0, as float32(max(., 0)).  A pixel holds the minimum
 *     over its points, except for the pixel pairs (y, W - 1) / (y + 1, 0) that the reference's sub2ind gives one key: when both
 *     hold points, the one with the earliest point of the pair holds the minimum over both and the other the value of the last
 *     point that fell on it.  A pixel no point reaches is 0.
 *     desc: int32 [n][4] per frame = H, W (W >= 2), the offset of its H W cells in the workspace (and in the native-size output),
 *     the offset of its H rows in the edge table; total_cells = sum H W, total_rows = sum H.  A frame whose descriptor leaves
 *     these bounds is written as zeros.
 *     out_h, out_w > 0: out [n][out_h][out_w], element (oy, ox) reads the map at (((2 oy + 1) H) / (2 out_h),
 *     ((2 ox + 1) W) / (2 out_w)) in integers -- nearest, pixel centres, the identity at equal sizes -- and with flip[f] != 0
 *     (int32 [n], may be NULL) the column out_w - 1 - ox.  out_h = out_w = 0: out [total_cells], every map at its own size at
 *     its cell offset (flip mirrors the columns).  Every element of out is written.
 *     ws: dmh_velo_depth_ws_size(total_cells, total_rows) uint32 words (-1 when they do not fit 2^31), contents ignored.
 *     Three launches (fill, scatter, finalise); 32-bit integer atomics only, no host read: bitwise reproducible.
 * ---------------------------------------------------------------------------------- */
int64_t dmh_velo_depth_ws_size(int64_t total_cells, int64_t total_rows);
int dmh_velo_depth_map(const float* points, int64_t npts, const int32_t* offsets, const double* proj, const int32_t* desc,
                       const int32_t* flip, int n, int vel_depth, int64_t total_cells, int64_t total_rows, int out_h, int out_w,
                       uint32_t* ws, float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * K33 torchvision 0.8.2's ColorJitter on 8-bit PIL images (MD2/datasets/mono_dataset.py:344-348, :133, :144), Pillow's bytes: the
 *     four operations in each item's own order, a byte after every one, for a batch and up to DMH_JITTER_MAX_TENSORS of its keys.
 *     src / out_f32 / out_u8: host arrays of T device pointers, every tensor [B][3][H][W] (planar); out_u8 may be NULL (no byte
 *     output).  out_f32 = (float)byte / 255.f (IEEE division, K31's expression).  Item i of every tensor takes record i; every
 *     image (tensor, item) has its own contrast mean.
 *     rec: int32 [B][8] in device memory per item = the count of operations (0 .. 4; 0: the image is only converted), their codes
 *     in the order they are applied, one per byte, the first in the low byte (0 brightness, 1 contrast, 2 saturation, 3 hue; each
 *     at most once, another code does nothing), the bits of the float32 brightness, contrast and saturation factors, the hue shift
 *     (a byte: ((int)(hue_factor * 255)) mod 256), 0, 0.  It is read on the device only, so a captured graph replays with the
 *     values it holds then.
 *     L = (19595 r + 38470 g + 7471 b + 32768) >> 16.  blend(deg, v, f): t = (float)deg + f * (float)(v - deg) in float32 without
 *     contraction; (int)t for 0 <= f <= 1, else 0 if t <= 0, 255 if t >= 255, (int)t between.  brightness = blend(0, v, f);
 *     saturation = blend(L, v, f); contrast = blend(m, v, f) with m = (int)((double)S / (double)(H W) + 0.5), S the sum of L over
 *     the image as the operations before the contrast left it; hue = Pillow's rgb2hsv (float32 quotients, the hue through double),
 *     H + shift modulo 256, hsv2rgb (double, C's round).
 *     with_contrast != 0: a first pass stores every workgroup's 32-bit sum of L into its slot of ws (uint32,
 *     dmh_color_jitter_ws_size(T, B, H, W) words, -1 for shapes the launcher refuses; contents ignored, nothing to clear) and the
 *     second pass adds the slots of its image; 0 promises that no record holds a contrast step (its mean would read as 0).
 *     1 <= T <= 8, T B <= 65535, H W <= DMH_JITTER_MAX_PIXELS (255 H W fits 32 bits), B 3 H W < 2^31.  Four pixels per thread when
 *     H W is a multiple of 4 and the pointers are aligned (src, out_u8 to 4 bytes, out_f32 to 16), one otherwise.  At most two
 *     launches; integer sums only, no atomics, no host read: bitwise reproducible.
 * ---------------------------------------------------------------------------------- */
#define DMH_JITTER_MAX_TENSORS 8
#define DMH_JITTER_MAX_PIXELS 16843009
int64_t dmh_color_jitter_ws_size(int T, int B, int H, int W);
int dmh_color_jitter(const uint8_t* const* src, float* const* out_f32, uint8_t* const* out_u8, int T, int B, int H, int W,
                     const int32_t* rec, int with_contrast, uint32_t* ws, void* stream);

/* ------------------------------------------------------------------------------------
 * K34 DepthHints' fused hint selection (depth-hints/precompute_depth_hints.py:151,247-252) for a batch of B stereo pairs, and the
 *     loader's side of a stored hint (depth-hints/datasets/mono_dataset.py:382-388).
 *     base, lookup: uint8 [B][3][H][W] (planar; K31's byte output); a value is (float)byte / 255.f.
 *     cand: cand_is_raw = 1: int16 [B][N][H][W], StereoSGBM's output (disparity x 16, -16 = no match),
 *           depth = fx 0.1f / (raw / 16 + 1e-7f) * (raw / 16 > 0), fx = K[b][0][0], float32 operations in that order, IEEE division;
 *           cand_is_raw = 0: float32 [B][N][H][W], the depths.  1 <= N <= DMH_HINT_MAX_CANDIDATES.
 *     K, inv_K, T: float32 [B][4][4].  Per candidate and pixel: BackprojectDepth and Project3D of depth-hints/layers.py
 *     (eps 1e-7, normalised by W - 1 and H - 1), F.grid_sample's defaults with padding_mode='border' (bilinear,
 *     align_corners=False; the coordinate is clamped to [0, size - 1] before it becomes an integer), SSIM over 3 x 3 windows with
 *     reflection padding 1 on both images, loss = 0.85 mean_c SSIM + 0.15 mean_c |base - sample|.
 *     best_depth: float32 [B][1][H][W], the depth of the candidate with the lowest loss, the lowest index among equal losses.
 *     losses: NULL, or float32 [B][N][H][W] that receives every loss (tests, diagnosis).
 *     H, W >= 2; B N H W < 2^31.  One launch, no atomics, no workspace, no host read: bitwise reproducible.
 *
 *     dmh_depth_hint_prepare: src float32 [B][Hs][Ws] -> hint, mask float32 [B][H][W]: np.fliplr where flip[b] != 0 (int32 [B],
 *     may be NULL), then nearest resize through the index tables ytab int32 [H] and xtab int32 [W] (device memory, entries in
 *     [0, Hs - 1] and [0, Ws - 1]; an entry outside is clamped): hint(y, x) = src(ytab[y], flip ? Ws - 1 - xtab[x] : xtab[x]),
 *     mask = hint > 0 as 0 / 1 (a -0.0 is not > 0).  ytab_len, xtab_len: the tables' lengths, which must be H and W.
 * ---------------------------------------------------------------------------------- */
#define DMH_HINT_MAX_CANDIDATES 16
int dmh_depth_hint_fuse(const uint8_t* base, const uint8_t* lookup, const void* cand, int cand_is_raw, const float* K,
                        const float* inv_K, const float* T, int B, int N, int H, int W, float* best_depth, float* losses,
                        void* stream);
int dmh_depth_hint_prepare(const float* src, const int32_t* flip, const int32_t* ytab, const int32_t* xtab, int64_t ytab_len,
                           int64_t xtab_len, int B, int Hs, int Ws, int H, int W, float* hint, float* mask, void* stream);

/* ------------------------------------------------------------------------------------
 * K35 A semi-global stereo matcher in integers for the depth-hint candidates (states the matcher; it is
 *     modelled on the structure of OpenCV's StereoSGBM in its single-pass mode, and nothing is claimed about equality with it).
 *     base, lookup: uint8 [B][3][H][W] (planar; K31's byte output).  reverse: NULL, or int32 [B] in device memory: != 0 matches
 *     the item on the mirrored pair (column W - 1 - x of both views) and stores the result mirrored back.
 *     params: N parameter sets in HOST memory, 1 <= N <= DMH_SGM_MAX_MATCHERS.  num_disparities D: a multiple of 16 in [16, 256];
 *     block_size 1, 2 or 3 (it enters through its radius r = block_size / 2 only); min_disparity 0; P1, P2 >= 0 with
 *     5 ((2r+1)^2 567 + P2) < 32767 (int16 sums stay exact); pre_filter_cap in [1, 63]; uniqueness_ratio in [0, 100];
 *     disp12_max_diff >= 0; speckle_window_size >= 0 (0: no speckle filter); speckle_range in [0, 4096].
 *     out: int16 [B][N][H][W], disparity x 16, -16 where nothing matched (columns x < D always; everything when W <= D): the form
 *     dmh_depth_hint_fuse takes as raw candidates.  Parameter sets that differ in nothing but a block_size of the same radius are
 *     computed once and stored into each of their slots.
 *     Workspace: per item and distinct parameter set two int16 volumes [H][W - D][D] and, with the speckle filter, 8 H W bytes of
 *     labels, each rounded up to 256 bytes.  dmh_sgm_plan returns the bytes to allocate so that the call stays under cap_bytes
 *     (at least 256; -1 with dmh_last_error() for arguments the launcher refuses, or when one parameter set of one item alone is
 *     over the cap) and, through n_chunks (may be NULL), into how many sequences of launches the cap splits the batch.
 *     dmh_sgm_disparity packs as many (item, parameter set) pairs as ws_bytes holds (at most 32) into each sequence of launches
 *     (cost, five path directions, selection, four speckle passes), one sequence after the other on the stream.
 *     phases: DMH_SGM_ALL.  A subset launches only those phases (tools/sgm_bench.py times the prefixes COST, COST | PATHS, ... to
 *     attribute the time); out is defined only after a call whose phases include SELECT (and SPECKLE where a window is set).
 *     W <= DMH_SGM_MAX_WIDTH, H <= 65535, B N H W < 2^31.  Integers only; integer atomics only where the result is unique (the
 *     disp2 tie rule, union-find labels, component sizes); no host read: bitwise reproducible, capturable.
 * ---------------------------------------------------------------------------------- */
#define DMH_SGM_MAX_MATCHERS 16
#define DMH_SGM_MAX_WIDTH 4096
#define DMH_SGM_COST 1
#define DMH_SGM_PATHS 2
#define DMH_SGM_SELECT 4
#define DMH_SGM_SPECKLE 8
#define DMH_SGM_ALL 15
typedef struct dmh_sgm_params {
    int32_t num_disparities, block_size, P1, P2, pre_filter_cap, uniqueness_ratio, disp12_max_diff, speckle_window_size,
        speckle_range, min_disparity;
} dmh_sgm_params;
int64_t dmh_sgm_plan(int B, int H, int W, const dmh_sgm_params* params, int N, int64_t cap_bytes, int* n_chunks);
int dmh_sgm_disparity(const uint8_t* base, const uint8_t* lookup, const int32_t* reverse, int B, int H, int W,
                      const dmh_sgm_params* params, int N, int16_t* out, void* ws, int64_t ws_bytes, int phases, void* stream);

/* ------------------------------------------------------------------------------------
 * K36 ManyDepth's reduce_conv in the degenerate call its trainer and wrapper make (manydepth2/trainer.py:371-385,
 *     depth_model.py:42-58: lookup_images * 0, zero pose -> the D cost-volume channels are exact zeros):
 *       y = relu(corr3x3(zero_pad(x, 1), w[:, :C]) + bias),  w [K][C+D][3][3]  (manydepth2/networks/resnet_encoder.py:124-129,321)
 *     The convolutions are K10 / K18 (or the library's); these are the passes around them.  x [B,C,H,W], y / g / g_pre
 *     [B,K,H,W], HW = H * W.  All refuse null pointers, C % 8, K % 8, K > 65535 and B * max(C, K) * HW >= 2^31 (C is the
 *     node's input channel count everywhere: the element-wise passes check it as part of the node's shape and index by K only).
 *   dmh_reduce_bias_relu : y = relu(z + bias[k]); y may be z.
 *   dmh_reduce_bwd_mask  : g_pre = g * [y > 0]; partials[k][s] = the sum of g_pre over slab s of channel k, all images
 *                          (dmh_reduce_bwd_partials_size floats).  With HW % 4 == 0 the planes must be 16-byte aligned.
 *   dmh_reduce_bwd_finish: g_bias[k] = sum_s partials[k][s] in index order (float64, rounded once);
 *                          g_weight [K][C+D][3][3] = dw [K][C][3][3] in channels < C, exact zeros in the D others.
 *   dmh_reduce_bwd_rounds: the fp32 roundings on the longest path of one g_bias sum (csrc/reduce_node.hip derives it); no launch.
 *     No atomics, no host read, fixed order: two runs give the same bits.
 * ---------------------------------------------------------------------------------- */
int dmh_reduce_bias_relu(const float* z, const float* bias, int B, int C, int K, int HW, float* y, void* stream);
int64_t dmh_reduce_bwd_partials_size(int B, int C, int K, int HW);
int dmh_reduce_bwd_rounds(int B, int C, int K, int HW);
int dmh_reduce_bwd_mask(const float* g, const float* y, int B, int C, int K, int HW, float* g_pre, float* partials, void* stream);
int dmh_reduce_bwd_finish(const float* partials, const float* dw, int B, int C, int K, int D, int HW, float* g_bias,
                          float* g_weight, void* stream);

/* ------------------------------------------------------------------------------------
 * K37 Float maps to magma-coloured bytes (MD2/test_simple.py:136-156, my_utils.py:43-105): source, percentile, limits, colour.
 *   src      float [n_src][h][w]: the maps (finite values).
 *   panels   HOST array [n_panels] (copied into the launches' arguments; n_panels <= DMH_COLORIZE_MAX_PANELS).  Per panel:
 *            a, b    the panel shows src[a] (b = -1) or |src[a] - src[b]|, resized to H x W with the arithmetic of
 *                    F.interpolate(mode="bilinear", align_corners=False) when (H, W) != (h, w) -- the input bits otherwise;
 *            mode    DMH_COLORIZE_MIN_P95: vmin = the panel's minimum, vmax = its percentile;
 *                    DMH_COLORIZE_ZERO_REF: vmin = 0, vmax = the percentile of panel ``ref``;
 *                    DMH_COLORIZE_MIN_MAX: the panel's minimum and maximum;
 *            origin  byte offset of the panel's first pixel in out; pixel (y, x) goes to out + origin + y pitch + 3 x.
 *   lo, hi, g  numpy's virtual index of H W elements: the percentile is lerp(sorted[lo], sorted[hi], g) in float32 as
 *            np.percentile computes it (hi = lo or lo + 1; 0 <= g < 1).
 *   table    uint8 [256][3]: the colour table (device).
 *   map      float [n_panels][H][W]: written with the maps that are coloured.
 *   ws       uint32 [dmh_disp_colorize_ws_size(n_panels)]: histograms and selection state, zeroed by the call.
 *   stats    float [n_panels][DMH_COLORIZE_STATS]: min, max, sorted[lo], sorted[hi], the percentile.
 *   out      uint8 [out_len]: only the panels' bytes are written.  index = 0 where 256 x < 0, 255 where 256 x >= 256, trunc(256 x)
 *            otherwise, x = (a - vmin) / (vmax - vmin), 0 when vmin == vmax.
 * A fixed number of launches, no host read between them, integer atomics only: two runs give the same bits.
 * ---------------------------------------------------------------------------------- */
#define DMH_COLORIZE_MAX_PANELS 32
#define DMH_COLORIZE_STATS 5
#define DMH_COLORIZE_MIN_P95 0
#define DMH_COLORIZE_ZERO_REF 1
#define DMH_COLORIZE_MIN_MAX 2
typedef struct {
    int32_t a, b, mode, ref;
    int64_t origin;
} dmh_colorize_panel;
int64_t dmh_disp_colorize_ws_size(int n_panels);
int dmh_disp_colorize(const float* src, int n_src, int h, int w, const dmh_colorize_panel* panels, int n_panels, int H, int W,
                      int lo, int hi, float g, const uint8_t* table, float* map, uint32_t* ws, float* stats, uint8_t* out,
                      int64_t out_len, int64_t pitch, void* stream);

/* ------------------------------------------------------------------------------------
 * K39 Pseudo-LiDAR: maps of a batch of n frames, each with its own size (H, W) and KITTI-object calibration, to velodyne-frame
 *     clouds: preprocessing/generate_lidar.py:10-33 over kitti_util.Calibration.project_image_to_velo, float32-equal.
 *   form     DMH_LIDAR_DEPTH: src float [src_len], frame f's H W depths at desc[f][2]; every pixel is a candidate, d = (double)src.
 *            DMH_LIDAR_DISP:  the same layout of disparities in pixels; s = src < 0 ? 0 : src, only pixels with s > 0 are
 *                             candidates, d = (f_u * 0.54) / (((double)s + 1.) - 1.).
 *            DMH_LIDAR_NET:   src float [n][h][w], the network's sigmoid output (src_len = n h w); per pixel of (H, W) the taps
 *                             0.01f + 9.99f * src, the bilinear resize with K25's coordinates (OpenCV's INTER_LINEAR), fp32
 *                             unfused, depth = (1.f / disp) * 5.4f clamped to [1e-3, 80], with quantise != 0 then
 *                             (float)(uint16)(depth * 256.f) / 256.f; d = (double)depth.  h = w = quantise = 0 in the other forms.
 *   calib    double [n][DMH_LIDAR_CALIB]: f_u f_v c_u c_v b_x b_y, Ri[9] = inv(R0) row-major, C[12] = C2V row-major.
 *            With u the column and v the row, in float64 without contraction and with IEEE division:
 *            x = ((u - c_u) d) / f_u + b_x, y = ((v - c_v) d) / f_v + b_y, z = d; r_i = (Ri[i][0] x + Ri[i][1] y) + Ri[i][2] z;
 *            o_i = ((C[i][0] r_0 + C[i][1] r_1) + C[i][2] r_2) + C[i][3]; kept if o_0 >= 0 && o_2 < max_high (a NaN is dropped).
 *   desc     int32 [n][4]: H, W (either may be 0: a frame without pixels), the frame's offset in src (ignored by the net form),
 *            its first tile.  A tile is DMH_LIDAR_TILE consecutive pixels of one frame in row-major order; tile_frame int32
 *            [n_tiles] names each tile's frame; the tiles of the frames are consecutive in batch order.  A record that points
 *            outside src yields no point.
 *   ws       int32 [2 n_tiles], contents ignored.
 *   out      float [cap][4], cap = sum H W <= n_tiles DMH_LIDAR_TILE: the kept rows (o_0, o_1, o_2, 1) as float32, frames in batch
 *            order, rows in pixel order; rows from offsets[n] on are not written.  offsets: int64 [n + 1] in device memory.
 *     Three launches (count, one-workgroup scan, write); no atomics, no host read: bitwise reproducible, capturable.
 * ---------------------------------------------------------------------------------- */
#define DMH_LIDAR_DEPTH 0
#define DMH_LIDAR_DISP 1
#define DMH_LIDAR_NET 2
#define DMH_LIDAR_TILE 1024
#define DMH_LIDAR_CALIB 27
int dmh_pseudo_lidar(const float* src, int64_t src_len, int form, int h, int w, int quantise, const double* calib,
                     const int32_t* desc, const int32_t* tile_frame, int n, int n_tiles, double max_high, int32_t* ws,
                     float* out, int64_t cap, int64_t* offsets, void* stream);

/* ------------------------------------------------------------------------------------
 * K40 Trajectory error of the KITTI odometry protocol: MD2/evaluate_pose.py:23-46 (dump_xyz, compute_ate) and :116-125.
 *   pred_poses  float [n][4][4]: the predicted relative poses (K29's T), row-major.
 *   gt_local    double [n][4][4]: the ground truth's local poses, inv(inv(G[i-1]) G[i]) of the global ones.
 *   Snippet i in [0, n) takes the m = min(track_length - 1, n - i) poses from i on (shorter at the end of the sequence, as the
 *   reference's slices are), chains C = C . T from the identity in float64, index order, for both, and collects the m + 1
 *   translations; offset = gt_0 - pred_0, pred += offset, scale = sum(gt pred) / sum(pred^2),
 *   ates[i] = sqrt(sum((pred scale - gt)^2)) / (m + 1).  sum(pred^2) = 0 gives NaN, as numpy's 0 / 0 does.
 *   ates        double [n].   stats  double [2]: mean and population standard deviation (np.std) of ates.
 *     Two launches (one thread per snippet; one workgroup with a fixed-order tree); no atomics, no host read: bitwise
 *     reproducible, capturable.
 * ---------------------------------------------------------------------------------- */
int dmh_pose_ate(const float* pred_poses, const double* gt_local, int n, int track_length, double* ates, double* stats,
                 void* stream);

/* ------------------------------------------------------------------------------------
 * K41 The pose encoder's first layer on a pair of frames: y = conv7x7s2p3((cat(a, b) - mean) / std, w), forward only.
 *   a, b   float [B][3][H][W] each, H and W even; two base pointers that may overlap (frames[:-1] and frames[1:] of one block).
 *   w      float [64][6][7][7];   y  float [B][64][H/2][W/2], not aliasing an input.
 *     Two launches of K14's tile kernel (w[:, :3] over a writes y, then w[:, 3:] over b adds into it, with the same tile and lane
 *     maps); every output is two k-ordered fp32 fma chains of 147 taps and one addition: no atomics, bitwise reproducible,
 *     capturable.
 * ---------------------------------------------------------------------------------- */
int dmh_stem_pair_norm_fwd(const float* a, const float* b, const float* w, int B, int H, int W, float mean, float std, float* y,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMH_HIP_H */
