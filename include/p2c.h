/*
 * p2c.h -- C ABI of libp2c_hip.so: the MI355X (gfx950) pose-sequence hot path of pedestrians-video-2-carla.
 *
 * The reference (wielgosz-info/pedestrians-video-2-carla) is pure Python: there is no FFI to match. These entry
 * points are what a ctypes / cffi binding on the reference side would bind to replace the chains of small PyTorch ops
 * listed below (INTEGRATION.md shows the binding). Paths are relative to src/pedestrians_video_2_carla/ of the reference.
 *
 *   p2c_pose_head_fwd / _bwd   replaces, fused in one launch each:
 *        modules/movements/movements.py:105-118          rotation_6d_to_matrix on the model output
 *        modules/layers/projection.py:52-71              per-clip reference skeleton (O(B) python) -> skel_type index
 *        modules/layers/projection.py:170-195 + walker_control/p3d_pose.py:98-213    cumulative rotations + FK
 *        modules/layers/projection.py:125-136 + transforms/pose/normalization/reference_skeletons_denormalizer.py:67-91
 *        utils/world.py:16-63                            world transform from changes
 *        walker_control/p3d_pose_projection.py:115-152   pinhole projection
 *        transforms/pose/normalization/normalizer.py:20-41 (+ extractors)   dm.transform_callable on the projection
 *        loss/loc_2d.py:69-89, loss/loc_3d.py:12-40, loss/loc_2d_3d.py:6-17
 *   p2c_normalize_fwd / _bwd   transforms/pose/normalization/normalizer.py:20-41 stand-alone (any skeleton)
 *   p2c_loss2d_fwd / _bwd      loss/base_pose_loss.py:36-66 + loss/loc_2d.py:69-89 (autoencoder flow)
 *   p2c_remap_nodes            data/base/base_dataset.py:156-167 (_get_common_tensor, zero-filled joint scatter)
 *   p2c_mlp_fwd / _bwd         modules/movements/linear_ae/linear_ae.py:25-59 (the six nn.Linear + ReLU of LinearAE)
 *
 * Conventions: every pointer is a DEVICE pointer unless named host_*; tensors are dense row-major fp32; `stream` is a
 * hipStream_t passed as void*; nothing is allocated, freed or synchronised inside; no exception crosses the ABI.
 * Return value: 0 = launched, negative = argument error (P2C_E_*), positive = hipError_t of the failed launch.
 */
#ifndef P2C_H
#define P2C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(P2C_BUILD)
#define P2C_API __attribute__((visibility("default")))
#else
#define P2C_API
#endif

#define P2C_JOINTS 26            /* CARLA_SKELETON bones; pose-head tensors are (B, T, 26, k) */
#define P2C_SKELETON_TYPES 4     /* (adult,female) (adult,male) (child,female) (child,male) */

/* kind of the movements-model output handed to the pose head (modules/flow/output_types.py:4-20) */
enum {
  P2C_KIND_POSE_CHANGES_6D = 0,  /* y (B,T,26,6)   6-D rotation *changes*, orthonormalised in-kernel          */
  P2C_KIND_POSE_CHANGES_MAT = 1, /* y (B,T,26,3,3) rotation-matrix changes (the reference's API tensor)        */
  P2C_KIND_RELATIVE_ROT_6D = 2,  /* y (B,T,26,6)   relative rotations (no cumulative product)                  */
  P2C_KIND_RELATIVE_ROT_MAT = 3, /* y (B,T,26,3,3)                                                             */
  P2C_KIND_ABSOLUTE_LOC = 4      /* y (B,T,26,3)   absolute locations, hips-neck re-normalised to the skeleton */
};

/* data-module transform applied to the projection (data/base/base_transforms.py) */
enum { P2C_TRANSFORM_NONE = 0, P2C_TRANSFORM_HIPS_NECK = 1, P2C_TRANSFORM_BBOX = 2, P2C_TRANSFORM_HIPS_NECK_BBOX = 3 };

enum { P2C_E_NULL = -1, P2C_E_SHAPE = -2, P2C_E_ENUM = -3, P2C_E_INDEX = -4 };

typedef struct p2c_pose_head_desc {
  /* ---- shapes / modes ---- */
  int32_t B, T;                 /* clips, frames per clip */
  int32_t kind;                 /* P2C_KIND_* */
  int32_t transform;            /* P2C_TRANSFORM_* */
  int32_t t0, t1;               /* eval_slice [t0, t1) over frames: losses / transformed outputs only there */
  int32_t mask_missing_joints;  /* loc_2d: ignore joints whose gt is exactly (0,0) */
  int32_t hips_lane;            /* predicted joint never masked (tensors.py:33-38), -1 = none */
  int32_t n_hips, n_neck;       /* 1 or 2 joints averaged for the shift / scale points */
  int32_t hips_idx[2], neck_idx[2];
  int32_t gt2d_joints, gt2d_channels;   /* gt2d is (B,T,gt2d_joints,gt2d_channels), channels >= 2 */
  int32_t gt3d_joints;                  /* gt3d is (B,T,gt3d_joints,3) */
  int32_t gmap2d[P2C_JOINTS];   /* per predicted joint: index of its gt joint, -1 = not a common joint */
  int32_t gmap3d[P2C_JOINTS];
  int32_t n_common2d, n_common3d;       /* number of gmap entries >= 0 (loss denominators) */
  int32_t world_absolute;               /* 0: dloc/drot are per-frame changes (utils/world.py:16-63); 1: they are the world
                                           location / rotation of each frame (projection.py:215-226) */
  float cam_f, cam_cx, cam_cy, cam_dist, cam_elev;
  float near_zero;              /* 1e-5 */
  /* ---- inputs ---- */
  const float *y;               /* model output, layout by kind */
  const int32_t *skel_type;     /* (B) in [0,4) */
  const float *ref_rel_loc;     /* (4,26,3)   reference skeleton tables (data/carla/reference.py) */
  const float *ref_rel_rot;     /* (4,26,3,3) */
  const float *ref_hn_shift;    /* (4,3) hips of the reference absolute pose  (absolute_loc kind) */
  const float *ref_hn_scale;    /* (4)   |neck-hips| of the reference absolute pose */
  const float *dloc;            /* (B,T,3)   world location changes (or locations) or NULL (= ZeroTrajectory) */
  const float *drot;            /* (B,T,3,3) world rotation changes or NULL */
  const float *gt2d;            /* targets['projection_2d_transformed'] (or 'projection_2d'); NULL = no loc_2d */
  const float *gt3d;            /* targets['absolute_pose_loc']; NULL = loc_3d unavailable */
  /* ---- outputs ---- */
  float *partials;              /* workspace, p2c_pose_head_workspace_floats(B) floats */
  float *loss_sums;             /* (4): sum_sq_2d, n_unmasked_2d, sum_sq_3d, n_elems_3d */
  float *losses;                /* (3): loc_2d, loc_3d, loc_2d_3d   (NaN when the gt is absent) */
  float *final_rel_rot;         /* (B,26,3,3) last relative rotation, consumed by the backward; pose_changes kinds */
  /* optional materialised tensors (eval / predict); NULL = not written */
  float *out_pose_changes;      /* (B,T,26,3,3) */
  float *out_projection_2d;     /* (B,T,26,3) */
  float *out_projection_2d_transformed; /* (B,T,26,3) frames outside [t0,t1) untouched */
  float *out_shift;             /* (B,T,2) */
  float *out_scale;             /* (B,T) */
  float *out_relative_pose_loc; /* (B,T,26,3) */
  float *out_relative_pose_rot; /* (B,T,26,3,3) */
  float *out_absolute_pose_loc; /* (B,T,26,3) */
  float *out_absolute_pose_rot; /* (B,T,26,3,3) */
  float *out_world_loc;         /* (B,T,3) */
  float *out_world_rot;         /* (B,T,3,3) */
  /* 1 = the caller guarantees that p2c_pose_head_bwd follows with the same desc before anyone reads `losses` / `loss_sums`
   * (a captured train step): for the time-parallel 6-D kernels the forward then skips the one-workgroup finalize launch
   * and the backward kernel finishes the loss reduction itself (same values to fp32 rounding). 2 = same guarantee, and
   * the forward call only counts the unmasked target pairs: the backward kernel, which recomputes the pose head anyway,
   * produces the losses as well as grad_y (+ the finalize launch). Ignored for every other kernel family. */
  int32_t defer_loss_finalize;
  /* ---- rot_3d (loss/rot_3d.py:9-37), 6-D kinds only (P2C_E_ENUM otherwise) ----
   * gt_rot: targets['absolute_pose_rot'] (B,T,gt3d_joints,3,3) or NULL. When set, the forward also sums the squared difference
   * between the absolute joint rotations of the kinematic chain and gt_rot over the joints gmap3d maps and the frames [t0,t1):
   * loss_sums must hold 6 floats ([4] = sum_sq_rot, [5] = n_elems_rot) and losses 4 ([3] = rot_3d = their quotient); nothing
   * else is written (no absolute_pose_rot tensor). The backward adds 2 (A - gt) grad_loss_rot / n as a torque in its
   * tangent-space pass. The joint-lane kernels run (time-parallel or clip-sequential, defer_loss_finalize ignored). */
  const float *gt_rot;
  const float *grad_loss_rot;   /* p2c_pose_head_bwd: device scalar, upstream gradient of rot_3d; NULL = none */
} p2c_pose_head_desc;

/* library / build identification: "p2c-hip <version> gfx950" */
P2C_API const char *p2c_version(void);

/* number of floats `partials` must hold for a batch of B clips */
P2C_API int64_t p2c_pose_head_workspace_floats(int32_t B);

/* Kernel selection for the 6-D kinds with lean outputs: batches of at most `max_b` clips (default 2048, or the
 * environment variable P2C_TP_MAX_B) run the time-parallel kernels (one workgroup per clip, one 32-lane group per frame,
 * T <= 32), larger ones the clip-sequential kernels. Both compute the same function (fp32 rounding order differs in the
 * cumulative rotation product). max_b < 0 only queries. Returns the previous value. */
P2C_API int p2c_pose_head_set_time_parallel_max_batch(int32_t max_b);
/* Experimental, off by default (min_b = 2^30; env P2C_PK_MIN_B): batches of at least `min_b` clips of the same
 * configuration without world motion run the packed-fp32 clip-sequential kernels (two clips per lane, v_pk_fma_f32) --
 * parity-tested, currently slower than the scalar kernels. min_b < 0 only queries. */
P2C_API int p2c_pose_head_set_packed_min_batch(int32_t min_b);
/* Batches of at least `min_b` clips (default 8192, env P2C_CHAIN_MIN_B) that the time-parallel kernels do not take run the
 * chain-lane kernels (csrc/p2c_pose_head_chain.hip: eight clips per wavefront, a lane owns up to four consecutive bones)
 * when the configuration is the training one: 6-D kind, lean outputs, no world motion, no external gradients, targets in
 * the CARLA joint layout with two channels. Otherwise, and below min_b, the joint-lane kernels run. Same function, fp32
 * rounding order differs in the kinematic chain. min_b < 0 only queries. Returns the previous value. */
P2C_API int p2c_pose_head_set_chain_min_batch(int32_t min_b);

/* Forward: fills loss_sums, losses, final_rel_rot and any non-NULL out_* tensor. Two launches on `stream`
 * (pose head + deterministic reduction of the per-wave partial sums); with desc->defer_loss_finalize = 1 / 2 one launch
 * (no reduction / only the per-clip count of unmasked target pairs) -- see the field's comment. */
P2C_API int p2c_pose_head_fwd(const p2c_pose_head_desc *desc, void *stream);
/* Measurement hook (bench.py, rocprofv3 cross-check): the launches of p2c_pose_head_fwd one at a time. which = 1: the
 * pose-head kernel alone, 2: the one-workgroup loss reduction alone, 3: both (= p2c_pose_head_fwd). */
P2C_API int p2c_pose_head_fwd_launch(const p2c_pose_head_desc *desc, int32_t which, void *stream);

/* Backward (recompute): grad_y has the layout of desc->y. `grad_losses` = host array of three device pointers (each
 * NULL = no gradient, or one float): the upstream gradients of (loc_2d, loc_3d, loc_2d_3d) -- for a 3-vector gradient g
 * pass {g, g+1, g+2}; NULL array = all zero. desc->loss_sums and desc->final_rel_rot must hold the forward's values.
 * Optional upstream gradients of materialised outputs (NULL = none): grad_absolute_pose_loc (B,T,26,3),
 * grad_projection_2d_transformed (B,T,26,3) [channel 2 ignored], grad_absolute_pose_rot (B,T,26,3,3) [6-D kinds only:
 * rot_3d-type losses, reference loss/rot_3d.py; P2C_E_ENUM for the matrix kinds]. One launch (two with
 * desc->defer_loss_finalize = 2: the kernel that also sums the losses + their final reduction). */
P2C_API int p2c_pose_head_bwd(const p2c_pose_head_desc *desc, const float *const grad_losses[3],
                      const float *grad_absolute_pose_loc, const float *grad_projection_2d_transformed,
                      const float *grad_absolute_pose_rot, float *grad_y, void *stream);

/* Stand-alone normaliser (Normalizer.__call__, dim = 2 or 3) over N frames of J joints with C channels (C >= dim).
 * out (N,J,C), shift (N,dim), scale (N); shift/scale may be NULL. */
P2C_API int p2c_normalize_fwd(const float *x, float *out, float *shift, float *scale, int64_t N, int32_t J, int32_t C,
                      int32_t dim, int32_t transform, int32_t n_hips, const int32_t *host_hips_idx, int32_t n_neck,
                      const int32_t *host_neck_idx, float near_zero, void *stream);
P2C_API int p2c_normalize_bwd(const float *x, const float *grad_out, float *grad_x, int64_t N, int32_t J, int32_t C,
                      int32_t dim, int32_t transform, int32_t n_hips, const int32_t *host_hips_idx, int32_t n_neck,
                      const int32_t *host_neck_idx, float near_zero, void *stream);

/* Masked 2-D MSE (Loc2DPoseLoss): pred (N,Jp,Cp), gt (N,Jg,Cg); K common joints, host index lists; hips_col = position
 * in the common list that is never masked or -1. loss_sums (2) = sum_sq, n_unmasked; loss (1). */
P2C_API int64_t p2c_loss2d_workspace_floats(int64_t N);
P2C_API int p2c_loss2d_fwd(const float *pred, const float *gt, int64_t N, int32_t Jp, int32_t Cp, int32_t Jg, int32_t Cg,
                   int32_t K, const int32_t *host_pred_idx, const int32_t *host_gt_idx, int32_t hips_col,
                   int32_t mask_missing_joints, float *partials, float *loss_sums, float *loss, void *stream);
P2C_API int p2c_loss2d_bwd(const float *pred, const float *gt, int64_t N, int32_t Jp, int32_t Cp, int32_t Jg, int32_t Cg,
                   int32_t K, const int32_t *host_pred_idx, const int32_t *host_gt_idx, int32_t hips_col,
                   int32_t mask_missing_joints, const float *loss_sums, const float *grad_loss, float *grad_pred,
                   void *stream);

/* Zero-filled joint remap: dst[n, dst_idx[k], :] = src[n, src_idx[k], :], every other dst joint = 0. */
P2C_API int p2c_remap_nodes(const float *src, float *dst, int64_t N, int32_t Jsrc, int32_t Jdst, int32_t C, int32_t K,
                    const int32_t *host_src_idx, const int32_t *host_dst_idx, void *stream);

/* ---- fused small MLP (LinearAE: modules/movements/linear_ae/linear_ae.py:25-59) on fp32 MFMA -------------------------
 * y = W_{L-1} relu( ... relu(W_0 x + b_0) ... ) + b_{L-1} over N rows; dims[l] -> dims[l+1], every width <= 159.
 * Forward: x (N,dims[0]) -> y (N,dims[L]). Backward (activations recomputed): gy (N,dims[L]) -> gW[l] (dims[l+1],dims[l]),
 * gb[l] (dims[l+1]) -- WRITTEN, not accumulated -- through `partials` (p2c_mlp_workspace_floats floats) and a fixed-order
 * reduction (bitwise reproducible). x receives no gradient (the flows feed data). Two or three launches: per-workgroup
 * partial gradient tiles + reduction, or -- around one 16-row tile per CU -- activation / gradient factors + a contraction
 * over all rows + reduction (environment P2C_MLP_WGRAD=fused|split overrides the choice); the workspace size covers both. */
#define P2C_MLP_MAX_LAYERS 8
/* operand precision of the MLP's matrix products (accumulation is always fp32):
 *   F32    v_mfma_f32_16x16x4_f32, bit-for-bit an fmaf chain (default; what every parity claim is made with)
 *   BF16   operands rounded to bf16, v_mfma_f32_16x16x16_bf16: 1/8 of the MFMA cycles, ~2^-9 relative error per product
 *   BF16X3 split-bf16 (hi + lo, three MFMAs): ~fp32-grade products at 3/8 of the cycles
 * The reduced-precision arms exist for the LinearAE shapes with compile-time geometry (BASELINE.json configs[1] names bf16);
 * any other shape with precision != F32 returns P2C_E_ENUM. */
enum { P2C_PREC_F32 = 0, P2C_PREC_BF16 = 1, P2C_PREC_BF16X3 = 2 };
struct p2c_adamw_desc;
typedef struct p2c_mlp_desc {
  int32_t n_layers;
  int32_t dims[P2C_MLP_MAX_LAYERS + 1];
  int64_t N;
  const float *x;
  const float *W[P2C_MLP_MAX_LAYERS];   /* row-major (out, in), as nn.Linear.weight */
  const float *b[P2C_MLP_MAX_LAYERS];
  float *y;                             /* forward output */
  const float *gy;                      /* backward input */
  float *gW[P2C_MLP_MAX_LAYERS];
  float *gb[P2C_MLP_MAX_LAYERS];
  float *partials;                      /* backward workspace, p2c_mlp_workspace_floats floats */
  float *w_image;                       /* p2c_mlp_image_floats floats: packed weights, WRITTEN by p2c_mlp_fwd and
                                           read by p2c_mlp_bwd (same weights: call bwd before the optimizer) */
  /* optional, p2c_mlp_bwd only: apply this optimizer step to the MLP's parameters inside the gradient reduction (single-GPU
   * training, no all-reduce in between): gW/gb must be views of fused_adamw->grad, the MLP must be all of its n parameters;
   * w_image (if set) is refreshed with the new weights; with fused_adamw->zero_grad set, gW / gb are left ZEROED (as
   * p2c_adamw_step leaves them) instead of holding the gradient. Host pointer, read during the call. */
  const struct p2c_adamw_desc *fused_adamw;
  int32_t skip_pack;                    /* 1 = w_image is already current (kept so by p2c_mlp_pack + the optimizer's
                                           scatter, see p2c_adamw_desc): p2c_mlp_fwd does not launch the pack kernel */
  float *saved;                         /* optional, p2c_mlp_saved_floats floats (0 = not worth it at this N: pass NULL): the
                                           forward leaves the hidden activations there and the backward of the SAME call pair
                                           loads them instead of recomputing (bit-identical results) */
  int32_t precision;                    /* P2C_PREC_*: same value for the forward and the backward of a step */
} p2c_mlp_desc;
P2C_API int64_t p2c_mlp_image_floats(const p2c_mlp_desc *desc);
/* writes the packed image from the current weights (what p2c_mlp_fwd does first unless skip_pack) */
P2C_API int p2c_mlp_pack(const p2c_mlp_desc *desc, void *stream);
/* HOST array out: index[i] = float offset inside the image of parameter i, parameters counted in the order
 * W_0 (row-major), b_0, W_1, b_1, ... (n = sum of n_out * (n_in + 1)); returns n, or a negative P2C_E_* code */
P2C_API int64_t p2c_mlp_image_index(const p2c_mlp_desc *desc, int32_t *index, int64_t capacity);
P2C_API int64_t p2c_mlp_workspace_floats(const p2c_mlp_desc *desc);
P2C_API int64_t p2c_mlp_saved_floats(const p2c_mlp_desc *desc);
P2C_API int p2c_mlp_fwd(const p2c_mlp_desc *desc, void *stream);
P2C_API int p2c_mlp_bwd(const p2c_mlp_desc *desc, void *stream);
/* What p2c_mlp_fwd / p2c_mlp_bwd would do for desc->dims, n_layers and N with fp32 operands, from the functions they decide with
 * (the environment overrides included). Geometry only: no pointer of desc is looked at and nothing is launched. Writes
 * P2C_MLP_PLAN_INTS values to the HOST array out; returns 0, or P2C_E_SHAPE for a layer count, width or N outside the ABI. */
enum {
  P2C_MLP_PLAN_PROVIDER = 0,         /* kernels' shape provider: 0 = generic, 1 / 2 / 3 = the LinearAE shapes ending in 156 / 78 / 52 */
  P2C_MLP_PLAN_WAVE_FORWARD = 1,     /* 1 = wave-per-tile forward, 0 = cooperative */
  P2C_MLP_PLAN_SPLIT_WGRAD = 2,      /* 1 = factors + contraction + small reduction, 0 = weight gradient fused into the backward */
  P2C_MLP_PLAN_SAVE_ACTIVATIONS = 3, /* 1 = the forward leaves the hidden activations (given desc->saved), 0 = recomputed */
  P2C_MLP_PLAN_FWD_BLOCKS = 4,       /* workgroups of the forward and of the backward kernel */
  P2C_MLP_PLAN_BWD_BLOCKS = 5,
  P2C_MLP_PLAN_TILES_W = 6,          /* 16x16 tiles of the augmented weight gradients */
  P2C_MLP_PLAN_W_TOTAL = 7,          /* floats of the packed image (p2c_mlp_image_floats) */
  P2C_MLP_PLAN_LDS_FWD = 8,          /* bytes of LDS: cooperative forward, backward, wave-per-tile forward */
  P2C_MLP_PLAN_LDS_BWD = 9,
  P2C_MLP_PLAN_LDS_FWD_WAVE = 10,
  P2C_MLP_PLAN_FWD_OK = 11,          /* 1 = the geometry is one p2c_mlp_fwd / p2c_mlp_bwd accepts, 0 = it returns P2C_E_SHAPE */
  P2C_MLP_PLAN_BWD_OK = 12,
  P2C_MLP_PLAN_INTS = 16
};
P2C_API int p2c_mlp_plan(const p2c_mlp_desc *desc, int32_t *out);

/* ---- K13: the small-batch train step of LitPoseLiftingFlow(LinearAE) in two launches ------------------------------------
 * Replaces, for one optimisation step on a batch of B clips of T <= 16 frames (one clip = one 16-sample MFMA tile):
 *   modules/flow/base.py:397-410 (_step) -> modules/flow/pose_lifting.py:121-144 (_inner_step)
 *     modules/movements/linear_ae/linear_ae.py:50-59 (LinearAE.forward, 6-D rotation output: 52-26-13-6-39-78-156)
 *     everything p2c_pose_head_fwd / _bwd replace (projection layer, transform_callable, loc_2d / loc_3d / loc_2d_3d)
 *   the backward of all of it, and -- with mlp.fused_adamw -- torch.optim.AdamW.step (flow/base_model.py:156-158).
 * Launch 1: one workgroup per clip (LinearAE forward -> pose head forward + backward -> dgrad chain; the model output and
 * its gradient never leave LDS), leaving per-clip loss sums and weight-gradient factors in `mlp.partials`; launch 2: one
 * workgroup per 16x16 weight-gradient tile contracts the factors over all clips in a fixed order, writes gW/gb, applies
 * the optimizer step and refreshes mlp.w_image, and finishes the loss reduction. Same arithmetic, same summation orders
 * as the separate entry points: results are bitwise reproducible, and bit-identical to p2c_mlp_fwd -> p2c_pose_head_* ->
 * p2c_mlp_bwd where that path runs its split weight gradient.
 * head: y / final_rel_rot / out_* unused (out_* must be NULL); kind POSE_CHANGES_6D or RELATIVE_ROT_6D; partials = B*4
 * floats; losses / loss_sums are written by launch 2. mlp: x (B*T, 52), W / b (for p2c_mlp_pack unless skip_pack),
 * w_image, gW / gb (written), partials = p2c_train_step_workspace_floats floats, optional fused_adamw; y / gy / saved unused.
 * pair_counts: (B) floats from p2c_count_target_pairs on the SAME targets (a property of the batch: computed when the batch
 * is staged, not per step). grad_losses: as p2c_pose_head_bwd. */
typedef struct p2c_train_step_desc {
  p2c_pose_head_desc head;
  p2c_mlp_desc mlp;
  const float *pair_counts;
} p2c_train_step_desc;
P2C_API int p2c_train_step_supported(const p2c_train_step_desc *desc);          /* 1 = shapes / kind the kernels cover */
P2C_API int64_t p2c_train_step_workspace_floats(const p2c_train_step_desc *desc);
P2C_API int p2c_train_step(const p2c_train_step_desc *desc, const float *const grad_losses[3], void *stream);
/* Measurement hook: the same call with only some of its launches -- which = 1: the per-clip kernel, 2: the weight-gradient /
 * optimizer / loss kernel (on the factors a previous full call left in the workspace; each launch re-applies the optimizer
 * step), 3: both (= p2c_train_step). bench.py times the launches one by one with it. */
P2C_API int p2c_train_step_launch(const p2c_train_step_desc *desc, const float *const grad_losses[3], int32_t which,
                                  void *stream);
/* The first launch has two forms: one workgroup of eight wavefronts per clip (latency form, up to one clip per CU) and a
 * pair of wavefronts per clip, four pairs sharing a workgroup's weight image (throughput form, csrc/p2c_train_stream.hip), taken
 * from min_b clips on when the descriptor allows it (identity joint maps, CARLA targets, no world motion). Returns the previous threshold;
 * min_b < 0 only queries. Default 257 = more than one clip per CU (env P2C_STREAM_MIN_B). Both leave the same factor blocks for the second launch. */
P2C_API int p2c_train_step_set_stream_min_batch(int32_t min_b);
/* The second launch has two forms as well: a workgroup per dW tile and clip slice with the combine, the optimizer and the loss
 * reduction in the same launch (few hundred clips), and -- from min_b clips on (default 3072, env P2C_WGRAD_STREAM_MIN_B) -- a
 * persistent workgroup per clip slice that reads every factor block once and holds all 79 tiles, followed by a third launch
 * that adds the per-workgroup partials in a fixed order (+ optimizer + losses). Returns the previous threshold. */
P2C_API int p2c_train_step_set_wgrad_stream_min_batch(int32_t min_b);
/* The latency form of the first launch is compiled twice per 6-D kind. One instantiation reads every descriptor field at run
 * time. The other is specialised for ONE descriptor state, the reference's default pose-lifting configuration: transform
 * hips_neck_bbox with n_hips = n_neck = 1, dloc = drot = NULL, identity gmap2d / gmap3d, gt2d and gt3d present, t0 = 0,
 * t1 = T = 16, mask_missing_joints = 1. Same arithmetic, same bits; every other descriptor runs the general one.
 * p2c_train_step_set_specialized(on) switches the specialised instantiation on (default) or off and returns the previous
 * value; on < 0 only queries. p2c_train_step_specialized(desc) = 1 if the descriptor is in that state, else 0. */
P2C_API int p2c_train_step_set_specialized(int32_t on);
P2C_API int p2c_train_step_specialized(const p2c_train_step_desc *desc);
/* counts[b] = number of (frame, joint) pairs of clip b inside [t0, t1) whose 2-D target the loss does not mask
 * (utils/tensors.py:29-40 via loss/base_pose_loss.py:36-66): reads only the target-side fields of desc (gt2d, gmap2d,
 * hips_lane, mask_missing_joints, t0, t1); y / partials / losses may be NULL. One launch. */
P2C_API int p2c_count_target_pairs(const p2c_pose_head_desc *desc, float *counts, void *stream);

/* ---- grouped per-joint embeddings (K7a) --------------------------------------------------------------------------------
 * Replaces the loop over 26 nn.Linear(2, 64) of Seq2SeqEmbeddings._format_input (modules/movements/seq2seq/
 * seq2seq_embeddings.py:53-78): y[(t', b), j, :] = W_j x[b, t, j, :] + b_j with t' = t (or T-1-t when `flip`, the
 * reference's invert_sequence), written sequence-first as the LSTM wants it. x (B,T,J,C), C <= 4; y (T,B,J,E), E % 4 == 0.
 * Joint j's weight (E,C) starts at W + j*w_stride, its bias at b + j*b_stride (floats): stacked tensors and views of a
 * flat parameter buffer are both addressed without a copy. Backward: gW / gb with the same strides (x gets no gradient:
 * it is data); partials = p2c_embed_workspace_floats floats; fixed-order two-stage reduction (bitwise reproducible). */
P2C_API int64_t p2c_embed_workspace_floats(int32_t B, int32_t T, int32_t J, int32_t C, int32_t E);
P2C_API int p2c_embed_fwd(const float *x, const float *W, const float *b, int64_t w_stride, int64_t b_stride, float *y,
                  int32_t B, int32_t T, int32_t J, int32_t C, int32_t E, int32_t flip, void *stream);
P2C_API int p2c_embed_bwd(const float *x, const float *gy, int64_t w_stride, int64_t b_stride, float *gW, float *gb,
                  float *partials, int32_t B, int32_t T, int32_t J, int32_t C, int32_t E, int32_t flip, void *stream);

/* ---- folded input map (K7a') ------------------------------------------------------------------------------------------
 * Seq2SeqEmbeddings feeds concat_j(W_j x_j + b_j) into the encoder LSTM's first input projection (seq2seq_embeddings.py:
 * 53-78 -> seq2seq.py:36-58) with nothing non-linear in between; the train step composes the two linear maps instead of
 * materialising the (T,B,J*E) embedding tensor:
 *   w_eff[g, j*C + c] = sum_e w_ih[g, j*E + e] W_j[e, c]        b_eff[g] = b_ih[g] + b_hh[g] + sum_{j,e} w_ih[g, j*E+e] b_j[e]
 * w_ih (G, J*E); W_j / b_j addressed with strides as in p2c_embed_*; b_ih / b_hh (G) optional. Backward: from g_eff
 * (G, J*C) and g_b (G) it WRITES (accumulate_w = 0) or ADDS TO g_w_ih (G, J*E), ADDS to gW / gb (the strides of W / b)
 * and, when given, ADDS g_b to g_b_ih / g_b_hh. One launch each, fixed summation order. C <= 4. */
P2C_API int p2c_fold_fwd(const float *w_ih, const float *W, const float *b, int64_t w_stride, int64_t b_stride,
                 const float *b_ih, const float *b_hh, float *w_eff, float *b_eff, int32_t G, int32_t J, int32_t E,
                 int32_t C, void *stream);
P2C_API int p2c_fold_bwd(const float *w_ih, const float *W, const float *b, int64_t w_stride, int64_t b_stride,
                 const float *g_eff, const float *g_b, float *g_w_ih, int32_t accumulate_w, float *gW, float *gb,
                 float *g_b_ih, float *g_b_hh, int32_t G, int32_t J, int32_t E, int32_t C, void *stream);

/* ---- LSTM recurrence (K7b) ---------------------------------------------------------------------------------------------
 * The time loop of one torch.nn.LSTM layer (gate order i, f, g, o; reference seq2seq.py:36-58 Encoder / Decoder):
 *   gates[t] = gx[t] + h[t-1] W_hh^T ;  c[t] = f c[t-1] + i g ;  h[t] = o tanh(c[t])
 * with gx[t] = x[t] W_ih^T + b_ih + b_hh computed by the caller (one dense library GEMM for all t). H in {16,32,48,64,96,128}
 * (above 64 the W_hh image is staged through LDS in two chunks),
 * all tensors fp32 row-major, 16-byte aligned. Forward fills out (T,B,H), optional hT/cT (B,H) and the saved activations
 * acts (T,B,4H) / cs (T,B,H). Backward takes g_out / g_hT / g_cT (each optional), acts, cs, c0, w_hh and writes
 * g_gx (T,B,4H) = d gates (from which the caller forms dW_hh = sum_t g_gx[t]^T h[t-1], dW_ih, db with library GEMMs)
 * and optional g_h0 / g_c0. One launch each. B <= 2^20 (per-step rows are addressed through 32-bit buffer offsets); up to
 * B = 4096 the launch tiles 4 sequences per workgroup (v_mfma_f32_4x4x1_16B), above that 16 (v_mfma_f32_16x16x4);
 * P2C_REC_TILE=wide|narrow in the environment forces one.
 * T = 0 (every form of this descriptor, K7b and K18): no step runs and the (T,..) tensors have no rows; forward writes hT = h0 and
 * cT = c0, backward writes g_h0 = g_hT and g_c0 = g_cT -- zeros where the source is NULL, nothing where the destination is. */
typedef struct p2c_lstm_desc {
  int32_t T, B, H;
  const float *gx;              /* (T,B,4H) */
  const float *h0, *c0;         /* (B,H) or NULL = zeros */
  const float *w_hh;            /* (4H,H) */
  float *out;                   /* (T,B,H) */
  float *hT, *cT;               /* (B,H) or NULL */
  float *acts, *cs;             /* (T,B,4H), (T,B,H): written by fwd (may be NULL for inference), read by bwd */
  const float *g_out;           /* (T,B,H) or NULL */
  const float *g_hT, *g_cT;     /* (B,H) or NULL */
  float *g_gx;                  /* (T,B,4H) */
  float *g_h0, *g_c0;           /* (B,H) or NULL */
  /* optional (zero-initialise the struct): */
  const float *bias_a, *bias_b; /* (4H) or NULL: fwd adds them to gx as it reads it (b_ih, b_hh), so the projection GEMM runs bias-free */
  float *g_gx_bt;               /* (B,T,4H) or NULL: bwd writes a second, batch-first copy of g_gx (pairs with a batch-first layer input) */
  int32_t gx_bt;                /* fwd: gx is laid out (B,T,4H) -- the projection of a batch-first input, no permute copy */
  /* nn.LSTM's inter-layer dropout on this layer's output, drawn inside the kernels (drop_state != NULL; the protocol of the four
   * words: p2c_decoder_desc): fwd writes out_drop (T,B,H) = out * mask beside the raw `out` (fwd without out_drop draws nothing),
   * bwd takes g_out as the gradient of out_drop. */
  float *out_drop;
  int32_t *drop_state;
  float drop_p;
  int32_t drop_site;
} p2c_lstm_desc;
P2C_API int p2c_lstm_rec_fwd(const p2c_lstm_desc *desc, void *stream);
P2C_API int p2c_lstm_rec_bwd(const p2c_lstm_desc *desc, void *stream);

/* ---- LSTM recurrence for any hidden size (K18) ------------------------------------------------------------------------------
 * The same layer recurrence as p2c_lstm_rec_fwd / _bwd on the same descriptor, for any 1 <= H <= 1024 (no alignment or multiple
 * of H required), as ONE LAUNCH PER TIME STEP: the launch boundary is the synchronisation between steps. Forward: T launches; it
 * needs acts and cs (cs carries the cell state from one step to the next). Backward: T launches plus one for g_h0 when it is
 * asked for; `workspace` holds p2c_lstm_steps_workspace_floats(B, H) floats (the carried d c; may be NULL when T <= 1), nothing
 * in it is read before the call has written it. B <= 2^20; offsets are 64-bit. gx_bt, g_gx_bt and the dropout fields
 * (out_drop, drop_state) are not implemented here: a descriptor that sets any of them is refused (P2C_E_SHAPE). */
P2C_API int64_t p2c_lstm_steps_workspace_floats(int32_t B, int32_t H);
P2C_API int p2c_lstm_steps_fwd(const p2c_lstm_desc *desc, void *stream);
P2C_API int p2c_lstm_steps_bwd(const p2c_lstm_desc *desc, float *workspace, void *stream);

/* ---- GRU recurrence for any hidden size (K23) -------------------------------------------------------------------------------
 * The time loop of one torch.nn.GRU layer (gate order r, z, n), tiled and launched like K18 (one launch per time step):
 *   r = sigmoid(gx_r + W_hr h + b_hr) ;  z = sigmoid(gx_z + W_hz h + b_hz) ;  n = tanh(gx_n + r (W_hn h + b_hn)) ;
 *   h' = (1 - z) n + z h
 * with gx[t] = x[t] W_ih^T + b_ih computed by the caller. b_hn sits inside the reset gate's product, so bias_hh is the kernel's
 * and the backward writes TWO gradients: g_gx (T,B,3H) = d gx (-> dW_ih, db_ih, dx) and g_gh (T,B,3H) = d (W_hh h + b_hh), which
 * differs from g_gx by the factor r in the n block (-> dW_hh = sum_t g_gh[t]^T h[t-1], db_hh = sum g_gh; the caller's, K12).
 * Any 1 <= H <= 1024, B <= 2^20, 64-bit offsets. h0 = NULL is the zero state: no recurrent product at t = 0. Forward: T
 * launches; fills out (T,B,H), optional hT (B,H) and the saved acts (T,B,4H) = r, z, n, W_hn h + b_hn (NULL: inference).
 * Backward (descending t): g_out and g_hT are each optional; T launches plus one for g_h0 when it is asked for; `workspace` holds
 * p2c_gru_steps_workspace_floats(B, H) floats (the carried z dh; may be NULL when T <= 1 and g_h0 is NULL), nothing in it is read
 * before the call has written it. The fields below `g_h0` are not implemented: a descriptor that sets any of them is refused
 * (P2C_E_SHAPE, nothing launched), as is any other H or B. */
typedef struct p2c_gru_desc {
  int32_t T, B, H;
  const float *gx;              /* (T,B,3H) */
  const float *h0;              /* (B,H) or NULL = zeros */
  const float *w_hh;            /* (3H,H) */
  const float *bias_hh;         /* (3H) or NULL */
  float *out;                   /* (T,B,H) */
  float *hT;                    /* (B,H) or NULL */
  float *acts;                  /* (T,B,4H): written by fwd (may be NULL for inference), read by bwd */
  const float *g_out;           /* (T,B,H) or NULL */
  const float *g_hT;            /* (B,H) or NULL */
  float *g_gx, *g_gh;           /* (T,B,3H) each */
  float *g_h0;                  /* (B,H) or NULL */
  /* the layouts of p2c_lstm_desc that a single-launch GRU would take; must be zero here: */
  int32_t gx_bt;
  float *out_drop;
  int32_t *drop_state;
  float drop_p;
  int32_t drop_site;
} p2c_gru_desc;
P2C_API int64_t p2c_gru_steps_workspace_floats(int32_t B, int32_t H);
P2C_API int p2c_gru_steps_fwd(const p2c_gru_desc *desc, void *stream);
P2C_API int p2c_gru_steps_bwd(const p2c_gru_desc *desc, float *workspace, void *stream);

/* ---- classification head (K24) -------------------------------------------------------------------------------------------
 * One launch: mean cross-entropy of logits (B,C), 2 <= C <= 32, against int64 targets (B) (torch.nn.CrossEntropyLoss; max-
 * subtracted log-sum-exp, fixed summation order: the same bits every run) into loss[0]; g_logits (B,C) = (softmax - onehot) /
 * n_valid (NULL: not wanted); confusion[target][first maximal logit] += 1 in the caller's (C,C) int32 matrix (NULL: not wanted).
 * A row whose target lies outside [0, C) is ignored everywhere (ignore_index = -100 and every other bad label): no loss, a zero
 * gradient row, not in n_valid, not in the matrix. No valid row: loss = NaN. flags: P2C_CLS_BINARY = torch.nn.BCEWithLogitsLoss on
 * logits (B) (C must be 1), targets 0 / 1, prediction logit > 0, a 2 x 2 matrix; P2C_CLS_COUNT_ONLY = the matrix only, loss and
 * g_logits are neither read nor written. P2C_E_SHAPE for any other C, P2C_E_ENUM for any other flag. */
enum { P2C_CLS_BINARY = 1, P2C_CLS_COUNT_ONLY = 2 };
P2C_API int p2c_cls_head(const float *logits, const int64_t *targets, int64_t B, int32_t C, int32_t flags, float *loss,
                         float *g_logits, int32_t *confusion, void *stream);

/* ---- ranking metrics: AUROC, ROC and precision / recall curves (K25) -----------------------------------------------------
 * scores (N,C) float row-major, 1 <= C <= 32, targets (N) int32, N <= 2^24. Class c is ranked one-vs-rest: a row is positive when
 * target == c; with C == 1 the labels are 0 / 1 and a row is positive when target == 1. A row whose target lies outside [0, C)
 * ([0, 2) for C == 1), or that holds a NaN score in any column, is dropped everywhere; n_valid[0] = rows kept. Per class, the kept
 * rows sorted by score, descending; equal scores (-0.0 == +0.0) form one group; for group k, in order: thresholds[c][k] = its
 * score, tps[c][k] / fps[c][k] = positives / negatives with score >= it (scikit-learn's _binary_clf_curve). n_points[c] groups,
 * n_pos[c] = positives kept, auroc[c] = sum_k (fps[k] - fps[k-1]) (tps[k] + tps[k-1]) / (2 P Q) with the sum in 64-bit integers and
 * one fp64 division; NaN when P == 0 or Q == 0. Entries of a row past n_points[c] are not written. All outputs are the caller's.
 * N <= 16384: one launch, one workgroup per class sorting in LDS, no workspace (may be NULL). Larger N, or P2C_RANK_GLOBAL: a radix
 * sort in `workspace` (p2c_rank_workspace_bytes(N, C, flags) bytes, nothing in it is read before the call has written it), 29
 * launches, the same output bits. N == 0: no launch, n_points = n_pos = n_valid = 0, auroc = NaN. P2C_E_SHAPE for any other N or C,
 * P2C_E_ENUM for any other flag (p2c_rank_workspace_bytes returns the same codes), P2C_E_NULL for a missing pointer. */
enum { P2C_RANK_GLOBAL = 1 };
typedef struct p2c_rank_desc {
  int64_t N;
  int32_t C, flags;
  const float *scores;          /* (N,C) */
  const int32_t *targets;       /* (N) */
  float *thresholds;            /* (C,N) */
  int32_t *tps, *fps;           /* (C,N) each */
  int32_t *n_points, *n_pos;    /* (C) each */
  double *auroc;                /* (C) */
  int32_t *n_valid;             /* (1) */
} p2c_rank_desc;
P2C_API int64_t p2c_rank_workspace_bytes(int64_t N, int32_t C, int32_t flags);
P2C_API int p2c_rank_curves(const p2c_rank_desc *desc, void *workspace, void *stream);
/* One launch: logits (B,C) + int64 targets (B) -> fp32 scores and int32 targets at rows [row_offset, row_offset + B) of epoch
 * buffers of `capacity` rows (row_offset + B > capacity: P2C_E_SHAPE). scores = softmax with the maximum subtracted, 2 <= C <= 32;
 * flags = P2C_CLS_BINARY (C must be 1): sigmoid(logit) formed from exp(-|x|) as K24 forms it. A target outside [0, C) ([0, 2)
 * binary) is written as -1. Rows outside the range are not touched. */
P2C_API int p2c_rank_scores(const float *logits, const int64_t *targets, int64_t B, int32_t C, int32_t flags, float *out_scores,
                            int32_t *out_targets, int64_t row_offset, int64_t capacity, void *stream);

/* ---- Seq2Seq decoder loop (K7c) -----------------------------------------------------------------------------------------
 * for t in range(T): out_t = fc(LSTM_2layers(x_t; encoder state)); x_{t+1} = out_t   (reference seq2seq.py:245-349; the
 * decoder state is NOT carried between frames, 272-288). The caller provides the frame-invariant recurrent terms
 * k_l = b_ih_l + b_hh_l + W_hh_l hidden_l (B,4H) and the encoder cell states c_l (B,H). H = 64, 1 <= O <= 160 (anything
 * else: P2C_E_SHAPE, nothing launched). O <= 64 runs on the 16- or the 4-clip tiling (chosen by B, forced by P2C_REC_TILE, see K7b);
 * 64 < O <= 160 has the 16-clip tiling only: P2C_REC_TILE is not read there and both of its values give the same result.
 * Forward writes
 * out (T,B,O) and the saved activations; backward consumes g_out (T,B,O) and writes d gates0 / d gates1 (T,B,4H),
 * d out_total (T,B,O) [= g_out + the gradient that flows back through the fed-back input], and d c_l (B,H): the weight
 * gradients are dense reductions of those over all (t,b) (dW_ih0 = dgates0^T x_prev, dW_ih1 = dgates1^T h0d,
 * dW_fc = dout_total^T h1, dk_l = sum_t dgates_l, db_fc = sum dout_total), left to library GEMMs. One launch each. */
typedef struct p2c_decoder_desc {
  int32_t T, B, H, O;
  const float *k0, *c0, *k1, *c1;
  const float *w_ih0, *w_ih1, *w_fc, *b_fc;   /* (4H,O), (4H,H), (O,H), (O) */
  const float *x0;                /* (B,O) first input, NULL = zeros (<sos>) */
  const float *drop;              /* (T,B,H) multiplicative dropout mask applied to the layer-0 output, or NULL */
  float *out;                     /* (T,B,O) */
  float *acts0, *acts1;           /* (T,B,4H) activated gates, written by fwd, read by bwd */
  float *h0d, *h1;                /* (T,B,H) layer outputs (after dropout for layer 0), written by fwd */
  const float *g_out;             /* (T,B,O) */
  float *g_gates0, *g_gates1;     /* (T,B,4H) */
  float *g_outtot;                /* (T,B,O) */
  float *g_c0, *g_c1;             /* (B,H) */
  /* optional (zero-initialise the struct): the frame-invariant terms formed inside the launch. With hid0 != NULL,
   * k_l = b{l}a + b{l}b + hid_l w_hh{l}^T is computed by the forward itself from the encoder hidden states hid_l (B,H),
   * decoder.rnn.weight_hh_l{l} (4H,H) and the two bias vectors (4H; either may be NULL); k0 / k1 are then ignored and
   * kw0 / kw1 (B,4H) are scratch the 16-clip tiling (B > 4096) writes k_l to. out_bt: a second copy of out laid out
   * (B,T,O), the layout the model returns (saves the permute copy). Backward: g_out_bt != 0 says g_out is laid out (B,T,O);
   * g_k0 / g_k1 (B,4H) receive sum_t d gates_l (= d k_l), g_hid0 / g_hid1 (B,H) receive d hid_l = g_k_l w_hh{l} (both or
   * neither; they need w_hh{l} and, above B = 4096, g_k0 / g_k1). */
  const float *hid0, *hid1, *w_hh0, *w_hh1, *b0a, *b0b, *b1a, *b1b;
  float *kw0, *kw1;
  float *out_bt;
  float *g_k0, *g_k1, *g_hid0, *g_hid1;
  int32_t g_out_bt;
  /* teacher forcing (seq2seq.py:272-288,323-349), both or neither: force (T,B) 0 / 1 and target (T,B,O). Where force[t][b] != 0
   * frame t of clip b -- the stored output AND the next step's input -- is target[t][b]; its rows of d out_total are zero (the
   * reference writes the targets into the output tensor itself: those rows carry neither loss nor gradient). */
  const float *force, *target;
  /* the dropout mask drawn inside the kernels instead of read from `drop` (drop == NULL, drop_state != NULL): keep(e) =
   * hash(seed, step, site, element e of the (T,B,H) mask) >= drop_p 2^32 (csrc/p2c_rec_dev.h: drop_value), mask = keep / (1 - drop_p). drop_state: 4 int32 words
   * on the device {seed_lo, seed_hi, step, next}; fwd reads step and leaves next = step + 1, bwd reads next - 1 and leaves
   * step = next, so the two launches of a step draw the same mask and a replayed graph advances by itself. */
  int32_t *drop_state;
  float drop_p;
  int32_t drop_site;
} p2c_decoder_desc;
P2C_API int p2c_decoder_fwd(const p2c_decoder_desc *desc, void *stream);
P2C_API int p2c_decoder_bwd(const p2c_decoder_desc *desc, void *stream);

/* ---- validation metrics on device -------------------------------------------------------------------------
 * p2c_eval_pose3d: MPJPE (metrics/mpjpe.py:29-45) and MRPE (metrics/mrpe.py:38-76) of one batch, ADDED to `state`
 * (4 doubles, device, zeroed by the caller at reset): state[0] += sum over clips of mean_{t,j} |pred - gt| over the common
 * joints, state[1] += B, state[2] += sum over clips of mean_t |(world_pred + hips_pred) - (world_gt + hips_gt)|,
 * state[3] += B (only when the world locations are given). pred (B,T,26,3); gt (B,T,Jg,3); gmap[26] = gt joint of
 * prediction joint j or -1; world_* = ABSOLUTE world locations (B,T,3) or both NULL. Metres in, metres out (compute() =
 * 1000 * sum / count). partials: p2c_eval_workspace_floats(B) floats.
 * p2c_eval_pck: PCK (metrics/pck.py:66-98): state[0] += correct, state[2] += total. pred (N,Jp,Cp), gt (N,Jg,Cg), N = B*T,
 * Jg <= 64; pmap[Jg] = prediction joint paired with gt joint i or -1; mask_src = targets['projection_2d'] (N,Jg,Cg) or NULL
 * (= gt); hips_joint = gt joint that is never masked or -1; norm_mode 0 = bounding-box diagonal, 1 = |neck - hips| of the
 * gt frame; in norm_mode 1 hips_idx[n_hips] / neck_idx[n_neck] (one or two gt joints each, averaged) must lie in [0, Jg):
 * anything else is refused with P2C_E_INDEX, as the normaliser refuses it. partials: p2c_eval_workspace_floats(N) floats. */
P2C_API int64_t p2c_eval_workspace_floats(int64_t units);
P2C_API int p2c_eval_pose3d(const float *pred, const float *gt, int32_t B, int32_t T, int32_t Jg, const int32_t *gmap,
                    const int32_t *pred_hips, int32_t n_pred_hips, const int32_t *gt_hips, int32_t n_gt_hips,
                    const float *world_pred, const float *world_gt, float *partials, double *state, void *stream);
P2C_API int p2c_eval_pck(const float *pred, const float *gt, const float *mask_src, int64_t N, int32_t Jp, int32_t Cp,
                 int32_t Jg, int32_t Cg, const int32_t *pmap, int32_t mask_missing, int32_t hips_joint, int32_t norm_mode,
                 const int32_t *hips_idx, int32_t n_hips, const int32_t *neck_idx, int32_t n_neck, float threshold,
                 float near_zero, float *partials, double *state, void *stream);
/* p2c_eval_fb (K22): the five FB_* metrics of the pose-lifting flow (the reference package metrics/fb; the functions restated in
 * metrics/extra_metrics.py) of one batch in one launch, ADDED to `state` (10 doubles, device): for each selected metric k,
 * state[2k] += N * (batch mean of metric k), state[2k+1] += N -- what _FBMetric.update accumulates. `which` is a bit mask over
 * k = 0 MPJPE, 1 weighted MPJPE, 2 N-MPJPE, 3 MPJVE (first differences over the FLATTENED frame axis, N - 1 of them), 4 PA-MPJPE
 * (per-frame Procrustes alignment, the 3x3 problem solved in the kernel in fp64); the slots of an unselected metric are left
 * untouched and its work is skipped. pred, gt (N,J,3) contiguous, N = B*T, J <= 64; w = J per-joint weights on the device or
 * NULL (unit weights; then column 1 equals column 0 bit for bit). Metres in, metres out. A frame whose tensor-path value is
 * not finite (all-zero prediction: N-MPJPE; coincident joints: PA-MPJPE) makes that column not finite here as well.
 * P2C_E_SHAPE for J < 1, J > 64, N < 2 with MPJVE selected, `which` empty or above 31; N = 0 returns 0 and launches nothing.
 * partials: p2c_eval_fb_workspace_floats(N) floats. */
P2C_API int64_t p2c_eval_fb_workspace_floats(int64_t N);
P2C_API int p2c_eval_fb(const float *pred, const float *gt, const float *w, int64_t N, int32_t J, int32_t which,
                        float *partials, double *state, void *stream);

/* ---- fused AdamW / Adam over one flat fp32 buffer ------------------------------------------------------------------
 * Replaces torch.optim.AdamW.step() as configured by the reference (modules/flow/base_model.py:156-158) when all
 * trainable parameters live in one flat buffer. Update rule = torch/optim/adamw.py (amsgrad=False, maximize=False):
 *   g *= grad_scale;  p -= lr*wd*p (adamw) | g += wd*p (adam);  m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g^2;
 *   p -= (lr / (1-b1^t)) * m / (sqrt(v)/sqrt(1-b2^t) + eps),  t = *step + 1;  *step = t. One launch, graph-capturable. */
typedef struct p2c_adamw_desc {
  int64_t n;                 /* parameters */
  float *param, *grad, *exp_avg, *exp_avg_sq;   /* device, n floats each, 16-byte aligned */
  float *step;               /* device scalar: steps taken so far; incremented by the call */
  int32_t *ticket;           /* device int, zero-initialised once by the caller (workgroup completion counter) */
  const float *hyper;        /* device, 6 floats: lr, beta1, beta2, eps, weight_decay, grad_scale */
  int32_t adamw;             /* 1 = decoupled weight decay (AdamW), 0 = L2 penalty (Adam) */
  int32_t zero_grad;         /* 1 = leave grad zeroed (replaces the next step's zero_grad memset) */
  /* optional (both or neither): after the update, param[i] is also written to scatter_dst[scatter_idx[i]] where the index
   * is >= 0 -- keeps a consumer's re-laid-out copy of the weights (the fused MLP's LDS image) current without a pack launch */
  const int32_t *scatter_idx;
  float *scatter_dst;
} p2c_adamw_desc;
P2C_API int p2c_adamw_step(const p2c_adamw_desc *desc, void *stream);

/* ---- K29: the same step with the gradient clipped first (csrc/p2c_grad_clip.hip) ----------------------------------------
 * Replaces torch.nn.utils.clip_grad_norm_ / clip_grad_value_ followed by optimizer.step() -- what Lightning does for the
 * reference's --gradient_clip_val / --gradient_clip_algorithm (modeling.py:275, 353) -- on the flat buffer, without a host sync:
 *   NORM:  total_norm = (float)(grad_scale * sqrt(sum of g^2 in double));  coef = min(bound / (total_norm + 1e-6f), 1), NaN kept;
 *          g' = (g * grad_scale) * coef.        Two launches: the squared-norm partials, then the step.
 *   VALUE: g' = clamp(g * grad_scale, -bound, bound), NaN kept.  One launch.
 * followed by the update rule above on g' (grad_scale already applied: average first, then clip, as a data-parallel torch run
 * does). The sum's order depends on n alone: the same data gives the same bits. `bound` is a HOST value: a captured graph
 * bakes it in (re-capture to change it); everything else that varies between steps is read from device memory as above.
 * Same checks as p2c_adamw_step, then P2C_E_ENUM for another mode, P2C_E_SHAPE for a bound that is not finite or not > 0,
 * P2C_E_NULL for missing NORM pointers; n == 0 returns 0 and launches nothing. Graph-capturable. */
enum { P2C_CLIP_NORM = 1, P2C_CLIP_VALUE = 2 };
typedef struct p2c_clip_desc {
  int32_t mode;         /* P2C_CLIP_* */
  float   bound;        /* max_norm (2-norm) or clip_value; finite, > 0 */
  double *partials;     /* NORM: device, p2c_grad_clip_partials(n) doubles; VALUE: NULL */
  float  *total_norm;   /* NORM: device scalar, written by every call; VALUE: NULL */
} p2c_clip_desc;
P2C_API int64_t p2c_grad_clip_partials(int64_t n);
P2C_API int p2c_adamw_step_clipped(const p2c_adamw_desc *desc, const p2c_clip_desc *clip, void *stream);

/* ---- K11: dataset-side input pipeline for a batch of clips, one launch -------------------
 * Replaces, per clip and on the CPU in the reference, BaseDataset.__getitem__ (data/base/base_dataset.py:206-234):
 *   Projection2DMixin.process_projection_2d   data/base/mixins/dataset/projection_2d_mixin.py:209-232
 *     AugmentPose.__call__                     transforms/pose/augmentation/augment_pose.py:43-76
 *       RandomFlip / RandomRotation            .../random_flip.py:39-76, .../random_rotation.py:34-68
 *     apply_deform                             projection_2d_mixin.py:137-171 (noise, per-joint missing mask)
 *     apply_transform x2                       projection_2d_mixin.py:177-189 -> normalizer.py:20-41 + extractors
 *   ConfidenceMixin.process_confidence         data/base/mixins/dataset/confidence_mixin.py:13-20
 *   BaseDataset._map_nodes                     data/base/base_dataset.py:156-190
 * The reference draws its random numbers inside these calls; here every draw is an input tensor so that the kernel is
 * a pure function of its arguments. Device pointers unless marked host; NULL = that step is off / that output is not
 * wanted. Errors mirror the reference's: return_confidence with a 2-channel pose and rotation with boxes derived from
 * a 3-channel pose both raise there (P2C_E_SHAPE here). */
typedef struct p2c_collate_desc {
  int64_t N;                   /* clips */
  int32_t T, Jd, C;            /* frames per clip, joints of the data skeleton (<= 64), channels: 2 (x,y) or 3 (+confidence) */
  const float *raw;            /* (N,T,Jd,C) */
  const uint8_t *is_flipped;   /* (N) 0/1: RandomFlip decision per clip; NULL = no flip augmentation */
  const int32_t *flip_perm;    /* host, Jd: Skeleton.get_flip_mask() of the data skeleton */
  const float *rotation_deg;   /* (N) RandomRotation angle per clip; NULL = no rotation augmentation */
  const float *bboxes;         /* (N,T,2,2) targets['bboxes'] or NULL (boxes of the raw pose, utils/tensors.py:12-26) */
  const float *clip_size;      /* (N,2) meta clip_width / clip_height (0 = unknown) or NULL */
  const float *noise;          /* (N,T,Jd,2) additive noise or NULL */
  const float *miss_u;         /* (N,T,Jd) uniform draws or NULL; joint j is dropped where miss_u < miss_prob[j] */
  const float *miss_prob;      /* host, Jd */
  int32_t transform;           /* P2C_TRANSFORM_* of the data module (NONE: frames = deformed pose) */
  int32_t n_hips, hips_idx[2], n_neck, neck_idx[2];   /* hips / neck points of the DATA skeleton (1 or 2 joints each) */
  float near_zero;             /* 1e-5 in the reference */
  int32_t return_confidence;   /* model needs_confidence: frames keep the confidence channel */
  int32_t Ji, K;               /* joints of the model-input skeleton; common joints (0 = same skeleton, Ji == Jd) */
  const int32_t *src_idx;      /* host, K: data joint ...                    (get_common_indices, skeleton.py:26-56) */
  const int32_t *dst_idx;      /* host, K: ... lands on this model-input joint */
  float *frames;               /* (N,T,Ji,return_confidence ? 3 : 2) model input */
  float *t_projection_2d;      /* (N,T,Ji,2) augmented pose, or NULL */
  float *t_deformed;           /* (N,T,Ji,2) projection_2d_deformed, or NULL */
  float *t_transformed;        /* (N,T,Ji,2) projection_2d_transformed, or NULL */
  float *shift, *scale;        /* (N,T,2), (N,T): projection_2d_shift / _scale, or NULL */
  float *bboxes_out;           /* (N,T,2,2) augmented boxes (needs bboxes), or NULL */
} p2c_collate_desc;
P2C_API int p2c_collate_fwd(const p2c_collate_desc *desc, void *stream);

/* ---- K26: K11 over a batch whose clips come from several data skeletons, one launch -----------------------------------
 * Replaces, in the reference, MixedDataset.__getitem__ (data/mixed/mixed_dataset.py:91-107) handing each index to the
 * dataset it belongs to, i.e. BaseDataset.__getitem__ with that dataset's skeleton, deformation and transform. Clip n of
 * the batch is row[n] of source source[n] and is processed exactly as K11 processes a clip of that source (same device
 * function, same bits). The draws and side tensors are indexed by batch position; noise and miss_u have Jmax = max Jd
 * joints per frame and a source reads its first Jd. A source whose flag is off skips that step and its reads. Clips of a
 * source without boxes use the boxes of the pose, and bboxes_out (optional) receives their augmented pose boxes.
 * Lane grouping as K11 (32 lanes per frame when every Jd and Ji <= 32, else 64). source[n] >= S and row[n] outside
 * [0, n) are clamped in the kernel, never followed. Errors per source as K11's; also P2C_E_SHAPE for S outside
 * [1, P2C_COLLATE_MAX_SOURCES] and P2C_E_NULL without source / row. N == 0 launches nothing. */
#define P2C_COLLATE_MAX_SOURCES 4
typedef struct p2c_collate_source {
  int64_t n;                   /* clips stored in raw */
  const float *raw;            /* (n,T,Jd,C) */
  int32_t Jd, C;               /* joints of this source's skeleton (<= 64), channels 2 or 3 */
  const int32_t *flip_perm;    /* host, Jd (needed when the batch has is_flipped) */
  const float *miss_prob;      /* host, Jd (needed with has_miss) */
  int32_t transform;           /* P2C_TRANSFORM_* */
  int32_t n_hips, hips_idx[2], n_neck, neck_idx[2];
  int32_t K;                   /* common joints with the model-input skeleton (0 = same skeleton, Ji == Jd) */
  const int32_t *src_idx;      /* host, K */
  const int32_t *dst_idx;      /* host, K */
  int32_t has_noise, has_miss, has_bboxes;   /* this source's clips read noise / miss_u / bboxes */
} p2c_collate_source;
typedef struct p2c_collate_mixed_desc {
  int64_t N;                   /* clips in the batch */
  int32_t T, Ji, S;            /* frames per clip, joints of the model-input skeleton, sources */
  int32_t return_confidence;   /* every source must have 3 channels */
  float near_zero;
  p2c_collate_source sources[P2C_COLLATE_MAX_SOURCES];
  const uint8_t *source;       /* (N) source of clip n */
  const int32_t *row;          /* (N) its row in that source's raw */
  const uint8_t *is_flipped;   /* (N) or NULL */
  const float *rotation_deg;   /* (N) or NULL */
  const float *bboxes;         /* (N,T,2,2), read for clips of sources with has_bboxes */
  const float *clip_size;      /* (N,2) or NULL; 0 = unknown */
  const float *noise;          /* (N,T,Jmax,2), Jmax = max Jd over the sources */
  const float *miss_u;         /* (N,T,Jmax) */
  float *frames;               /* (N,T,Ji,return_confidence ? 3 : 2) */
  float *t_projection_2d, *t_deformed, *t_transformed;   /* (N,T,Ji,2) or NULL */
  float *shift, *scale;        /* (N,T,2), (N,T) or NULL */
  float *bboxes_out;           /* (N,T,2,2) or NULL */
} p2c_collate_mixed_desc;
P2C_API int p2c_collate_mixed_fwd(const p2c_collate_mixed_desc *desc, void *stream);

/* ---- C (+)= A^T [B | 1] over K rows (weight + bias gradient of a dense layer) ------------------------------------------------
 * Replaces, in the backward of the Seq2Seq models (modules/movements/seq2seq/seq2seq.py:36-94: the nn.LSTM projections and
 * Decoder.fc_out under autograd), the split-K library GEMM dW = dY^T X and the column reduction db = sum_rows dY.
 * A (K, M) row-major with row pitch lda (= dY), B (K, N) with pitch ldb (= X), C (M, N) with pitch ldc; bias_out (M) or
 * NULL; accumulate: bit 0 = add to C instead of overwriting, bit 1 = the same for bias_out; workspace = p2c_atb_workspace_floats floats (partial
 * tiles of the K slices). Two launches, fixed summation order (bitwise reproducible). */
P2C_API int64_t p2c_atb_workspace_floats(int64_t K, int32_t M, int32_t N, int32_t with_bias);
P2C_API int p2c_atb(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t K, int32_t M, int32_t N, float *C,
                    int64_t ldc, float *bias_out, int32_t accumulate, float *workspace, void *stream);
/* The same with A's row k multiplied by a_scale[k / rows_per_scale] as it is loaded (NULL = p2c_atb): dY of a transformer
 * sub-layer whose output carried a per-sample stochastic-depth factor (PoseTransformer blocks behind
 * modules/movements/pose_former/pose_former.py:62-76), so that no scaled copy of dY is written first. */
P2C_API int p2c_atb_scaled(const float *A, int64_t lda, const float *B, int64_t ldb, int64_t K, int32_t M, int32_t N, float *C,
                    int64_t ldc, float *bias_out, int32_t accumulate, const float *a_scale, int64_t rows_per_scale,
                    float *workspace, void *stream);

/* Grouped form: up to 8 independent problems behind ONE launch pair (the backward of a Seq2Seq layer stack is a row of
 * these contractions). Per problem the fields of p2c_atb; bias_out2 = a second vector that receives the same column sums
 * (bias_ih / bias_hh of an LSTM layer), needs bias_out. flags = the `accumulate` bits of p2c_atb. workspace =
 * p2c_atb_group_workspace_floats floats. Same kernels, same per-problem summation order as p2c_atb (bitwise equal results). */
typedef struct p2c_atb_problem {
  const float *a; int64_t a_stride;   /* (K, M) */
  const float *b; int64_t b_stride;   /* (K, N) */
  int64_t K;
  int32_t M, N;
  float *out; int64_t out_stride;     /* (M, N) */
  float *bias_out, *bias_out2;        /* (M) or NULL */
  int32_t flags;
} p2c_atb_problem;
P2C_API int64_t p2c_atb_group_workspace_floats(const p2c_atb_problem *problems, int32_t n);
P2C_API int p2c_atb_group(const p2c_atb_problem *problems, int32_t n, float *workspace, void *stream);

/* ---- grouped copy (batch staging of a captured step) ------------------------------------------------------------------------
 * dst[i][0:bytes[i]] = src[i][0:bytes[i]] for up to 24 device buffers in ONE launch: a HIP-graph train step reads fixed
 * addresses, so the tensors of every new batch the reference's trainer would hand to `training_step`
 * (modules/flow/base.py:231-246 `_step(batch, ...)`) are copied into the static buffers first. src / dst / bytes are HOST
 * arrays of n entries (device pointers inside). */
P2C_API int p2c_copy_group(const void *const *src, void *const *dst, const int64_t *bytes, int32_t n, void *stream);

/* Inspection: number of nodes / kernel nodes of a hipGraph_t (the trainer replays a captured step by calling its recorded
 * entry point directly when the graph holds nothing but that entry point's launches). */
P2C_API int p2c_graph_node_counts(void *graph, int32_t *n_total, int32_t *n_kernel);

/* ---- multi-head self-attention over short token sequences (K14) --------------------------------------------------------------
 * The attention of the build's PoseTransformer (reference modules/movements/pose_former/pose_former.py:33-76 binds the
 * third-party PoseTransformer: 26 joint tokens x 8 heads of 4 channels in the spatial blocks, 9 frame tokens x 8 heads of
 * 104 in the temporal ones). qkv (S, N, 3, heads, head_dim) = the qkv projection's output viewed; out (S, N, heads*head_dim)
 * = softmax(scale * q k^T) v per head, heads concatenated. Backward: from qkv and g_out (S, N, heads*head_dim) to g_qkv (the
 * layout of qkv); the probabilities are recomputed. One launch each; one workgroup per sequence with everything in LDS:
 * N <= 64, heads*head_dim % 4 == 0 and (N (4 heads head_dim + 8) + 2 heads N^2) floats <= 156 KB -- the backward's image: q, k,
 * v and g_out rows with 4 floats of padding each, scores and their gradients (p2c_attn_small_supported). qkv, out, g_out and
 * g_qkv are read and written 16 bytes at a time: a pointer that is not 16-byte aligned is refused (P2C_E_SHAPE), as K15 does.
 * No attention dropout, no mask. */
P2C_API int p2c_attn_small_supported(int32_t N, int32_t heads, int32_t head_dim);
P2C_API int p2c_attn_small_fwd(const float *qkv, float *out, float scale, int32_t S, int32_t N, int32_t heads, int32_t head_dim,
                       void *stream);
P2C_API int p2c_attn_small_bwd(const float *qkv, const float *g_out, float *g_qkv, float scale, int32_t S, int32_t N,
                       int32_t heads, int32_t head_dim, void *stream);

/* ---- LayerNorm over the last dimension of many short rows (K15) ----------------------------------------------------------------
 * torch.nn.LayerNorm(D) (biased variance, eps inside the root) as the build's PoseTransformer applies it (546 624 rows of 32,
 * 21 024 rows of 832; reference binding: modules/movements/pose_former/pose_former.py:33-76). x, y, gy, gx (rows, D)
 * row-major and 16-byte aligned, D % 4 == 0, D <= 1024; gamma / beta (D), any 4-byte alignment. Forward also writes mean and
 * rstd (rows) for the backward. Backward: gx (+ gx_add (rows, D) when not NULL: the gradient arriving over the residual
 * connection that branches off in front of a pre-norm layer, added in the same pass), and g_gamma / g_beta written
 * (accumulate = 0) or added to; partials = p2c_layernorm_workspace_floats floats; two launches, fixed summation order. */
P2C_API int p2c_layernorm_supported(int32_t D);
P2C_API int64_t p2c_layernorm_workspace_floats(int64_t rows, int32_t D);
P2C_API int p2c_layernorm_fwd(const float *x, const float *gamma, const float *beta, float *y, float *mean, float *rstd,
                      int64_t rows, int32_t D, float eps, void *stream);
P2C_API int p2c_layernorm_bwd(const float *x, const float *gamma, const float *mean, const float *rstd, const float *gy,
                      const float *gx_add, float *gx, float *g_gamma, float *g_beta, int32_t accumulate, float *partials,
                      int64_t rows, int32_t D, void *stream);

/* Learned weighted mean over F frame tokens: out (B, C) = sum_f w[f] x[b, f, c] + bias[0] (bias may be NULL) -- the forward of
 * PoseTransformer's weighted_mean = Conv1d(F, 1, kernel 1), bound at modules/movements/pose_former/pose_former.py:62-76. x (B, F, C)
 * and out (B, C) dense and 16-byte aligned, C % 4 == 0. One launch. */
P2C_API int p2c_frame_mean_fwd(const float *x, const float *w, const float *bias, float *out, int64_t B, int32_t F, int32_t C,
                       void *stream);

/* Testing aid (no counterpart in the reference): fills the LDS of every CU with NaN bit patterns, so that a kernel reading LDS it
 * never wrote fails deterministically instead of by what the previous workgroup left behind. One launch on `stream`. */
P2C_API int p2c_debug_poison_lds(void *stream);

/* ---- dense layers on fp32 MFMA with a fused epilogue (K16, csrc/p2c_gemm.hip) -----------------------------------------------------
 * C (M, N) = epilogue(A (M, K) * op(B)): trans_b = 1: B is (N, K) row-major -- y = x W^T, the forward of torch.nn.Linear as the
 * reference's model plugins use it (PoseTransformer qkv / proj / fc1 / fc2: modules/movements/pose_former/pose_former.py:62-76;
 * the input projections of the Seq2Seq LSTMs: movements/seq2seq/seq2seq.py:36-38,72-73); trans_b = 0: B is (K, N) row-major --
 * dx = dy W, its input gradient (the weight gradient dy^T x is p2c_atb). All row-major with leading dimensions in floats.
 * Epilogue, in this order: v = acc + bias[n] (bias may be NULL); act = 1: aux_out[m][n] = v if aux_out != NULL, then
 * v = gelu(v) (erf form, torch.nn.GELU()); act = 2: v *= gelu'(aux[m][n]) (the backward through that activation, aux = the
 * stored pre-activation); v *= row_scale[m / rows_per_scale] if row_scale != NULL (per-sample stochastic-depth factor);
 * act = 3 / 4: ReLU + dropout and their backward (below); v += residual[m][n] if residual != NULL; C[m][n] = v. C may alias residual. fp32 in, fp32 accumulate (an fmaf chain in k
 * order). 16-byte loads when every base / leading dimension allows, dword loads otherwise. Returns 0 or P2C_E_*. */
typedef struct p2c_gemm_desc {
  int32_t M, N, K, trans_b;
  const float *a; int64_t lda;
  const float *b; int64_t ldb;
  float *c; int64_t ldc;
  const float *bias;
  int32_t act, rows_per_scale;
  const float *aux; float *aux_out; int64_t ldaux;
  const float *row_scale;
  const float *residual; int64_t ldr;
  /* act 3 / 4 (nn.TransformerEncoderLayer's FFN): act 3: v = relu(v) keep(m N + n) / (1 - drop_p) with the hashed mask of site
   * drop_site of drop_state (the 4-word stream of p2c_bnorm_desc: reads `step`, leaves next = step + 1; drop_state NULL: relu
   * alone, which needs drop_p == 0 -- act 4 scales by 1 / (1 - drop_p) with or without a state, so act 3 refuses drop_p > 0
   * without one, P2C_E_SHAPE); act 4: v *= [aux[m][n] > 0] / (1 - drop_p), aux = act 3's output -- relu' and the kept mask in one test, so the
   * backward needs neither the pre-activation nor a mask tensor. 0 <= drop_p < 1; act 3 with drop_state refuses M N >= 2^31
   * (P2C_E_SHAPE, nothing launched). Zero for acts 0..2. */
  void *drop_state;
  float drop_p;
  int32_t drop_site;
} p2c_gemm_desc;
P2C_API int p2c_gemm(const p2c_gemm_desc *desc, void *stream);
/* The weight gradient of a WIDE dense layer, C (M, N) (+)= A^T B with A (K, M) and B (K, N) row-major over K = rows >> M, N
 * (dW = dy^T x; p2c_atb covers layers of up to ~128 features): the same MFMA tiles, K split into slices that each write a slab
 * of `workspace` (p2c_gemm_tn_workspace_floats(M, N, K) floats), added in slice order by a second launch -- bitwise
 * reproducible. accumulate bit 0: add to C; bit 1: add to bias_out. row_scale (NULL = none): A's row k is multiplied by
 * row_scale[k / rows_per_scale] as it is loaded (dy of a layer whose output carried a per-sample stochastic-depth factor).
 * bias_out (M) or NULL: the column sums of the scaled A (= db) from the same pass. */
P2C_API int64_t p2c_gemm_tn_workspace_floats(int32_t M, int32_t N, int32_t K);
/* The tile / slice experiment variables (P2C_GEMM_BN, P2C_GEMM_TN_BN, P2C_GEMM_TN_SLICES) are read once; a tool that changes
 * them inside one process calls this to have them read again. */
P2C_API void p2c_gemm_reload_env(void);
P2C_API int p2c_gemm_tn(const float *a, int64_t lda, const float *b, int64_t ldb, float *c, int64_t ldc, int32_t M, int32_t N,
                int32_t K, int32_t accumulate, const float *row_scale, int32_t rows_per_scale, float *bias_out,
                float *workspace, void *stream);

/* ---- BatchNorm1d + ReLU + dropout (+ residual) over a row-major (N, C) activation (K19) ------------------------------------------
 * Forward: z = act(gamma (y - mean) rstd + beta) * keep(e) / (1 - p) [+ residual], act = ReLU when relu != 0, else identity.
 *   training != 0: mean / rstd (C each) are the batch statistics (biased variance, rstd = 1 / sqrt(var + eps)), computed in a fixed
 *   order (bitwise reproducible) and written for the backward; running_mean / running_var (both or neither) are updated in place
 *   with `momentum` and the unbiased variance, as torch.nn.BatchNorm1d. Needs N >= 2 and `workspace`. Three launches.
 *   training == 0: the running statistics (required), no dropout; mean / rstd receive running_mean and 1 / sqrt(running_var + eps)
 *   for a backward; workspace may be NULL. One launch.
 * Backward: g = g_z keep / (1 - p) [pre > 0]; g_beta = sum_rows g, g_gamma = sum_rows g (y - mean) rstd (stored, or added to when
 *   accumulate != 0); g_y = gamma rstd (g - g_beta / N - (y - mean) rstd g_gamma / N) in training, gamma rstd g in eval (training
 *   as in the forward call). The residual's gradient is g_z itself (the caller's). Same fixed order; three launches.
 * Dropout (training only, drop_state != NULL and drop_p > 0): the hashed masks of the recurrence kernels, site drop_site of the
 *   4-word state {seed_lo, seed_hi, step, next}; the forward reads `step` and leaves next = step + 1, the backward draws the
 *   forward's masks from next - 1 and leaves step = next. No mask tensor.
 * Element indices are 32-bit: N C >= 2^31 is refused (P2C_E_SHAPE) before anything is launched. workspace holds
 * p2c_bnorm_workspace_floats(N, C) floats; nothing in it is read before the call has written it. */
typedef struct p2c_bnorm_desc {
  int64_t N;
  int32_t C, training, relu, accumulate;
  float eps, momentum;
  const float *y, *gamma, *beta, *residual;    /* residual: NULL or (N, C) */
  float *z, *mean, *rstd, *running_mean, *running_var;
  const float *g_z;
  float *g_y, *g_gamma, *g_beta;
  void *drop_state;
  float drop_p;
  int32_t drop_site;
} p2c_bnorm_desc;
P2C_API int64_t p2c_bnorm_workspace_floats(int64_t N, int32_t C);
P2C_API int p2c_bnorm_fwd(const p2c_bnorm_desc *desc, float *workspace, void *stream);
P2C_API int p2c_bnorm_bwd(const p2c_bnorm_desc *desc, float *workspace, void *stream);

/* ---- the post-norm nn.TransformerEncoderLayer of SimpleTransformer (K20, csrc/p2c_encoder.hip) ------------------------------------
 * (reference modules/movements/transformers.py: six layers, d_model = 2 J, ReLU, dropout 0.1 at four places per layer.)
 * K20a  multi-head self-attention with dropout on the probabilities, any head width: qkv (S, N, 3, heads, head_dim) = the
 *   in_proj output viewed, out (S, N, heads head_dim) = concat_h (softmax(scale q k^T) keep / (1 - drop_p)) v. Backward: g_qkv
 *   from qkv and g_out, the probabilities and the mask recomputed. One launch each, one workgroup per (sequence, head).
 *   1 <= N <= 64, heads head_dim <= 256 (p2c_attn_drop_supported). Mask element ((s heads + h) N + i) N + j.
 * K20b  post-norm residual: z = LayerNorm(x + s keep / (1 - drop_p)) over rows of any 2 <= D <= 1024 (gamma / beta (D), biased
 *   variance, eps inside the root); mean / rstd (rows) written (the backward reads rstd and forms the row mean again, in fp64
 *   as the forward does: u - mean survives rows whose elements nearly coincide). Backward: g_x = dz_pre (the residual branch),
 *   g_s = dz_pre keep / (1 - drop_p), g_gamma / g_beta written (accumulate = 0) or added to; workspace =
 *   p2c_postnorm_workspace_floats floats; two launches, fixed summation order. Mask element r D + c.
 * Dropout (drop_state != NULL and drop_p > 0): the hashed stream of p2c_bnorm_desc (forward reads `step`, leaves next = step + 1;
 * backward reads next - 1, leaves step = next), site drop_site. 0 <= drop_p < 1. With a mask, S heads N^2 >= 2^31 (K20a) and
 * rows D >= 2^31 (K20b) are refused (P2C_E_SHAPE) before anything is launched. */
P2C_API int p2c_attn_drop_supported(int32_t N, int32_t heads, int32_t head_dim);
P2C_API int p2c_attn_drop_fwd(const float *qkv, float *out, float scale, int32_t S, int32_t N, int32_t heads, int32_t head_dim,
                              void *drop_state, float drop_p, int32_t drop_site, void *stream);
P2C_API int p2c_attn_drop_bwd(const float *qkv, const float *g_out, float *g_qkv, float scale, int32_t S, int32_t N, int32_t heads,
                              int32_t head_dim, void *drop_state, float drop_p, int32_t drop_site, void *stream);
P2C_API int p2c_postnorm_supported(int32_t D);
P2C_API int64_t p2c_postnorm_workspace_floats(int64_t rows, int32_t D);
P2C_API int p2c_postnorm_fwd(const float *x, const float *s, const float *gamma, const float *beta, float *z, float *mean,
                             float *rstd, int64_t rows, int32_t D, float eps, void *drop_state, float drop_p, int32_t drop_site,
                             void *stream);
P2C_API int p2c_postnorm_bwd(const float *x, const float *s, const float *gamma, const float *mean, const float *rstd,
                             const float *g_z, float *g_x, float *g_s, float *g_gamma, float *g_beta, int32_t accumulate,
                             float *workspace, int64_t rows, int32_t D, void *drop_state, float drop_p, int32_t drop_site,
                             void *stream);

/* ---- fused ReLU stack (K21, csrc/p2c_relu_stack.hip) ---------------------------------------------------------------------------
 * The front end of Seq2SeqFlatEmbeddings (reference modules/movements/seq2seq/seq2seq_flat_embeddings.py:39-44, 62-73):
 * h_0 = x, h_{l+1} = relu(W_l h_l + b_l) for l = 0 .. n_layers - 1 (the ReLU after the last layer included) over the N = B T rows
 * of x (B T, dims[0]); W_l row-major (dims[l+1], dims[l]) as nn.Linear.weight, b_l (dims[l+1]).
 * Forward (one launch): y is written SEQUENCE-FIRST, (T, B, dims[n_layers]): input row b T + t goes to output row t' B + b with
 *   t' = T - 1 - t when flip != 0 (invert_sequence), else t' = t.
 * Backward (two launches): from x, y (the forward's output: the last layer's ReLU mask; the hidden activations are recomputed) and
 *   gy (same layout as y): gW_l / gb_l are written, or added to when accumulate != 0. x is data: no gradient is formed for it.
 *   Per-workgroup partials in `workspace` (p2c_relu_stack_workspace_floats floats, nothing in it is read before it is written)
 *   are added in a fixed order: no float atomics, two runs give the same bits.
 * p2c_relu_stack_supported: 1 when the widths fit -- the zero-padded weight images plus the tile activations of the backward in
 *   160 KiB of LDS and at most 96 16x16 weight-gradient tiles (the exact rule is in the kernel file's header). Unsupported widths
 *   make _fwd / _bwd return P2C_E_SHAPE with nothing launched. Any B >= 0, T >= 1. */
#define P2C_RELU_STACK_MAX_LAYERS 5
typedef struct p2c_relu_stack_desc {
  int32_t n_layers;
  int32_t dims[P2C_RELU_STACK_MAX_LAYERS + 1];
  int32_t B, T, flip;
  const float *x;
  const float *W[P2C_RELU_STACK_MAX_LAYERS], *b[P2C_RELU_STACK_MAX_LAYERS];
  float *y;
  const float *gy;
  float *gW[P2C_RELU_STACK_MAX_LAYERS], *gb[P2C_RELU_STACK_MAX_LAYERS];
  int32_t accumulate;
  float *workspace;
} p2c_relu_stack_desc;
P2C_API int p2c_relu_stack_supported(const p2c_relu_stack_desc *desc);
P2C_API int64_t p2c_relu_stack_workspace_floats(const p2c_relu_stack_desc *desc);
P2C_API int p2c_relu_stack_fwd(const p2c_relu_stack_desc *desc, void *stream);
P2C_API int p2c_relu_stack_bwd(const p2c_relu_stack_desc *desc, void *stream);

/* ---- pose_changes / cum_pose_changes losses (K27, csrc/p2c_pose_change_loss.hip) -------------------------------------------------
 * nn.MSELoss between predicted and target pose changes (reference loss/pose_changes.py:7-28, cumulative = 0: M_t against G_t) or
 * between their running products over the frames (loss/cum_pose_changes.py:9-56, cumulative = 1: C_t = C_{t-1} M_t with
 * C_{-1} = I against the same left-to-right product of the targets), per (clip, joint), in fp32.
 *   pred     (B,T,J,6) raw 6-D rotations (pred_is_6d = 1: orthonormalised in-kernel by the pose head's rot6d_fwd, 8-byte aligned)
 *            or (B,T,J,3,3) matrices (pred_is_6d = 0; they need not be orthonormal);   target (B,T,J,3,3).
 *   mean     1: loss = sum / (B T J 9) -- 9 for 6-D input too, the comparison is over matrices; 0: reduction='sum'.
 *   max_blocks  0: the kernel's own grid cap; > 0 lowers it (a test reaches the grid-stride regime with a handful of chains).
 * _fwd (one launch behind a 16-byte memset node): *loss, and in `workspace` (p2c_pose_change_loss_workspace_floats floats,
 *   16-byte aligned, nothing in it is read before the call has written it) the differences and running products _bwd reads.
 * _bwd (one launch; same desc, the workspace as _fwd left it): grad_pred (layout of pred) = d loss / d pred times *grad_loss
 *   (a device float). No gradient is formed for the target. The running product C_{t-1} is read back, never obtained by
 *   inverting a step.
 * No masking: a NaN anywhere gives a NaN loss. The reduction has a fixed order and uses no float atomics: loss and gradient are
 * bit-identical from run to run. Any T >= 1, J >= 1, B >= 0 (B = 0: nothing is launched, nothing written). Element indices are
 * 32-bit: B T J 9 >= 2^31 is refused (P2C_E_SHAPE). Flags outside {0, 1}: P2C_E_ENUM. Every refusal comes before any launch. */
typedef struct p2c_pose_change_loss_desc {
  int64_t B;
  int32_t T, J;
  int32_t pred_is_6d, cumulative, mean, max_blocks;
  const float *pred, *target;
  float *workspace, *loss;
  const float *grad_loss;
  float *grad_pred;
} p2c_pose_change_loss_desc;
P2C_API int64_t p2c_pose_change_loss_workspace_floats(const p2c_pose_change_loss_desc *desc);
P2C_API int p2c_pose_change_loss_fwd(const p2c_pose_change_loss_desc *desc, void *stream);
P2C_API int p2c_pose_change_loss_bwd(const p2c_pose_change_loss_desc *desc, void *stream);

/* ---- heatmap head of the pose-estimation flow (K28, csrc/p2c_heatmaps.hip) ----------------------------------------------------
 * All fp32, dense row-major tensors, fixed-order reductions, no float atomics: two runs give the same bits.
 *
 * p2c_heatmap_targets_fwd (K28a, one launch): the target maps of N = B T frames, reference VideoMixin._get_heatmap +
 * gaussian_kernel + the flow's avg_pool2d(k, s, p) (count_include_pad), written pooled; the full-resolution maps are not formed.
 *   kp (N,J,2) pixel keypoints, shift (N,2); centre = rint((kp - shift) * (scale_x, scale_y)) in fp32, round-half-even; a
 *   non-finite or |centre| >= 2^30 one has no support.   table[d2], n_table <= 1024 entries: the Gaussian of the integer squared
 *   distance, clamps applied, built by the caller; d2 >= n_table reads as 0.   out (N,J+1,oh,ow): channel 0 = 1 - max_j,
 *   channel j + 1 = joint j; oh = (H + 2p - k) / s + 1 (ow alike) must be what the caller states.   k = 1, s = 1, p = 0 is full
 *   resolution, bit for bit the table's values.   1 <= J <= 63, 1 <= k <= 32, 2p <= k. A cell whose window meets no support is 0.0f.
 * p2c_heatmaps_loss_fwd (K28b, two launches) / _bwd (one): BasePoseLoss's sum_per_frame with nn.MSELoss('mean') over maps.
 *   pred (B,T,Pp,h,w), gt (B,T,Pg,h,w); pair k < K <= 64 compares pred channel pred_channels[k] with gt channel gt_channels[k].
 *   Pair k is selected in (b,t) when mask = 0, or k == forced (-1: none), or every cell of its gt map is != 0.
 *   loss = sum_t S_t / (n_t h w) over the frames with n_t > 0 selected pairs and a non-NaN sum S_t; no such frame: 0.
 *   _fwd writes partials (B,T,K) floats, flags (B,T,K) int32 (the selection), coef (T) floats and *loss; _bwd reads flags and coef
 *   as _fwd left them and writes grad_pred (layout of pred, every element: 0 for unlisted channels and skipped frames) =
 *   d loss / d pred times *grad_loss (a device float). B = 0: loss 0.
 * p2c_heatmap_keypoints_fwd (K28c, one launch): reference _keypoints_from_heatmaps. maps (N,P,h,w), 2 <= P <= 64; out (N,P-1,3) =
 *   (col * sw, row * sh, c) of the maximum c of map p + 1 at its first flat index if c > 0 and the map holds no NaN, else zeros.
 * P2C_E_SHAPE / P2C_E_ENUM / P2C_E_NULL before any launch. */
#define P2C_HEATMAPS_MAX_MAPS 64
#define P2C_HEATMAPS_MAX_TABLE 1024
#define P2C_HEATMAPS_MAX_POOL 32
typedef struct p2c_heatmap_targets_desc {
  int64_t N;
  int32_t J, H, W;
  int32_t k, s, p;
  int32_t oh, ow;
  int32_t n_table;
  float scale_x, scale_y;
  const float *kp, *shift, *table;
  float *out;
} p2c_heatmap_targets_desc;
typedef struct p2c_heatmaps_loss_desc {
  int64_t B;
  int32_t T, Pp, Pg, h, w;
  int32_t K, forced, mask;
  int32_t pred_channels[P2C_HEATMAPS_MAX_MAPS], gt_channels[P2C_HEATMAPS_MAX_MAPS];
  const float *pred, *gt;
  float *partials;
  int32_t *flags;
  float *coef, *loss;
  const float *grad_loss;
  float *grad_pred;
} p2c_heatmaps_loss_desc;
typedef struct p2c_heatmap_keypoints_desc {
  int64_t N;
  int32_t P, h, w;
  float sw, sh;
  const float *maps;
  float *out;
} p2c_heatmap_keypoints_desc;
P2C_API int p2c_heatmap_targets_fwd(const p2c_heatmap_targets_desc *desc, void *stream);
P2C_API int p2c_heatmaps_loss_fwd(const p2c_heatmaps_loss_desc *desc, void *stream);
P2C_API int p2c_heatmaps_loss_bwd(const p2c_heatmaps_loss_desc *desc, void *stream);
P2C_API int p2c_heatmap_keypoints_fwd(const p2c_heatmap_keypoints_desc *desc, void *stream);

/* ---- predicted poses <-> CARLA bone transforms (K30, csrc/p2c_carla_pose.hip) ---------------------------------------------------
 * What the reference does per frame on the host (walker_control/p3d_pose.py:56-96 tensors_to_pose, :34-54 pose_to_tensors,
 * renderers/carla_renderer.py:165-183 for the root), for N = B T frames of J >= 1 bones in one launch each way. fp32.
 * p2c_carla_pose_fwd: rel_loc (N,J,3), rel_rot (N,J,3,3) -> bones (N,J,6); world_loc (N,3), world_rot (N,3,3) -- both null or
 *   both given -- -> root (N,6), written in the same launch and only when they are given. A row is (x, y, -z, pitch, yaw, roll),
 *   locations unscaled, with e = the 'XYZ' Euler angles of R = Rx(e0) Ry(e1) Rz(e2):  e1 = asin(R[0,2] clamped to [-1, 1]),
 *   e0 = atan2(-R[1,2], R[2,2]), e2 = atan2(-R[0,1], R[0,0]);  pitch = -deg(e1), yaw = -deg(e2), roll = -deg(e0).
 * p2c_carla_pose_inv: bones (N,J,6) -> loc (N,J,3) = (x, y, -z), rot (N,J,3,3) = Rx Ry Rz of rad(-roll, -pitch, -yaw).
 * max_blocks  0: the kernels' own grid cap; > 0 lowers it (a test reaches the grid-stride regime with a handful of rows).
 * No masking: a NaN operand gives NaN in the outputs computed from it and nowhere else. Every output element has one writer and
 * nothing is reduced: two runs give the same bits. N = 0: nothing is launched. N < 0, J < 1, max_blocks < 0: P2C_E_SHAPE;
 * a missing tensor, or one world input without the other: P2C_E_NULL; both before any launch. */
P2C_API int p2c_carla_pose_fwd(const float *rel_loc, const float *rel_rot, const float *world_loc, const float *world_rot,
                               float *bones, float *root, int64_t N, int32_t J, int32_t max_blocks, void *stream);
P2C_API int p2c_carla_pose_inv(const float *bones, float *loc, float *rot, int64_t N, int32_t J, int32_t max_blocks,
                               void *stream);

/* ---- K32: keypoint clips -> CARLA bone transforms in one launch (csrc/p2c_lift.hip) -----------------------------------------
 * For B clips of T frames: LinearAE.forward (the 52-26-13-6-39-78-156 model, p2c_mlp_fwd's arithmetic) -> the relative
 * rotations of the materialising pose head (pose_head_rot_fwd<KIND, true>: c = rot6d(y_t), R = c R for pose_changes, R = c for
 * relative_rot, frames in order) -> the rows of p2c_carla_pose_fwd with relative_pose_loc = ref_rel_loc[skel_type]. The model
 * output and the rotations stay in LDS; no forward kinematics, no projection. One workgroup per clip, a clip in tiles of 16
 * frames, any B >= 1 and T >= 1; the same bits as the three separate calls.
 * mlp: x (B*T, 52), N = B*T, dims, w_image and skip_pack as for p2c_mlp_fwd (skip_pack == 0: W / b are read by one
 *   p2c_mlp_pack launch first); precision P2C_PREC_F32; y / gy / gW / gb / partials / saved / fused_adamw unused.
 * kind: P2C_KIND_POSE_CHANGES_6D or P2C_KIND_RELATIVE_ROT_6D (P2C_E_ENUM otherwise).
 * world_loc (B,T,3) / world_rot (B,T,3,3): the world transform of each frame, both or neither; NULL = the identity world.
 * initial_rel_rot (B,26,3,3) or NULL: where the running rotation starts instead of ref_rel_rot[skel_type] (pose_changes; a
 *   video cut into clips hands the previous clip's final_rel_rot here).
 * bones (B,T,26,6); root (B,T,6) or NULL; final_rel_rot (B,26,3,3) or NULL, written for the pose_changes kind only;
 * out_relative_pose_rot (B,T,26,3,3) or NULL. Every output element has one writer, nothing is reduced, no workspace.
 * max_blocks 0: one workgroup per CU at most; > 0 lowers that cap (workgroups stride over the clips).
 * B == 0 or T == 0: nothing is launched. Negative sizes, a geometry p2c_lift_supported refuses: P2C_E_SHAPE; a missing
 * tensor or one world input without the other: P2C_E_NULL; all before any launch. */
typedef struct p2c_lift_desc {
  p2c_mlp_desc mlp;
  int32_t B, T;
  int32_t kind;
  int32_t max_blocks;
  const int32_t *skel_type;        /* (B) in [0,4) */
  const float *ref_rel_loc;        /* (4,26,3) */
  const float *ref_rel_rot;        /* (4,26,3,3) */
  const float *world_loc;
  const float *world_rot;
  const float *initial_rel_rot;
  float *bones;
  float *root;
  float *final_rel_rot;
  float *out_relative_pose_rot;
} p2c_lift_desc;
P2C_API int p2c_lift_supported(const p2c_lift_desc *desc);   /* 1 = the model geometry, kind and precision the kernel covers */
P2C_API int p2c_lift_fwd(const p2c_lift_desc *desc, void *stream);

/* ---- K33: decoded video clips -> the pose-estimation flow's input frames (csrc/p2c_frames.hip) --------------------------------
 * What the reference does per clip on the host (data/base/mixins/dataset/video_mixin.py:143-184 crop_bbox, a paste per frame;
 * transforms/video/video_to_resnet.py:14-56: torchvision equalize per frame and channel, an antialiased bilinear resize per
 * frame, / 255, ImageNet mean / std), for N clips of T frames in two launches behind one memset node.
 *   src      one packed uint8 device buffer of src_bytes bytes; clip i is a dense (T, H_i, W_i, 3) block at clips[i].offset.
 *   clips[i] canvas = 0: the frame itself is the image (vh, vw) = (H, W). canvas > 0: the image is the canvas x canvas zero square
 *            onto which extract_bbox_from_frame pastes the frame around centres[(i T + t)] = (x, y), half = canvas / 2; the
 *            canvas is never formed. (out_h, out_w): the size written; equal to (vh, vw) means no resampling.
 *   centres  (N T, 2) int32 on the device (the host rounds the bboxes; the kernel sees no float bbox); NULL when no clip crops.
 *   workspace p2c_clip_frames_workspace_bytes(N T) bytes, 4-byte aligned: (N T, 3, 256) int32 level counts, zeroed by the call.
 *   out      fp32, clip after clip, each (T, 3, out_h, out_w): ((lut[level] resampled, rounded half-even) / 255 - mean_c) / std_c.
 * Launch A counts the levels of each frame's pasted window (LDS atomics, then int32 global atomics: exact in any order); the zero
 * padding is added to bin 0 analytically. Launch B rebuilds the three look-up tables of its frame per workgroup (step = (pixels -
 * count of the last non-empty bin) / 255; step = 0 leaves the channel unchanged; lut[0] = 0, lut[v] = min((cum[v-1] + step / 2) /
 * step, 255)) and writes one output tile: horizontal taps, LDS, vertical taps. Taps follow torch's antialiased bilinear
 * interpolate (align_corners = False): scale = in / out, support = max(scale, 1), centre = scale (i + 0.5), window
 * [int(centre - support + 0.5), int(centre + support + 0.5)) clipped to the image, triangle weights normalised by their sum; the
 * geometry is formed in fp64, the weights and sums in fp32. Every output element has one writer: two runs give the same bits.
 * 1 <= N <= P2C_FRAMES_MAX_CLIPS, T >= 1, 1 <= H, W, canvas <= 8192, 1 <= out_h, out_w <= 8192: P2C_E_SHAPE otherwise, and for a
 * clip block that does not lie inside src_bytes; P2C_E_NULL for a missing pointer; both before any launch. No host sync. */
#define P2C_FRAMES_MAX_CLIPS 64
#define P2C_FRAMES_MAX_SIDE 8192
typedef struct p2c_clip_frames_clip {
  int64_t offset;
  int32_t H, W;
  int32_t canvas;
  int32_t out_h, out_w;
  int32_t reserved;
} p2c_clip_frames_clip;
typedef struct p2c_clip_frames_desc {
  int32_t N, T;
  int64_t src_bytes;
  const uint8_t *src;
  const int32_t *centres;
  int32_t *workspace;
  float *out;
  p2c_clip_frames_clip clips[P2C_FRAMES_MAX_CLIPS];
} p2c_clip_frames_desc;
P2C_API int64_t p2c_clip_frames_workspace_bytes(int64_t frames);
P2C_API int p2c_clip_frames_fwd(const p2c_clip_frames_desc *desc, void *stream);

/* ---- K34: skeleton clips -> the video logger's uint8 frames (csrc/p2c_render.hip) ---------------------------------------------
 * What the reference's PedestrianWriter does on the host per frame and panel (a PIL canvas, one ellipse per joint, panels
 * concatenated with numpy), for every panel, video and frame in ONE launch with no memset in front of it.
 *   out      uint8 (V, T, rows H, cols W, 3); cell k = panel k sits at rows (k / cols) H.., columns (k % cols) W..; a panel whose
 *            points are NULL and the cells from n_panels on are zero. Every byte is written exactly once.
 *   panel    points fp32 (V, T, J, C >= 2), columns 0 / 1 = x (column) / y (row), further columns ignored; colors uint8 (J, 3);
 *            edges int32 (E, 2) joint indices (an index outside [0, J) draws nothing), NULL when E == 0.
 * All arithmetic behind the rounding is integer. Centre c = rint(x, y) (fp32, half to even); a joint is valid when both
 * coordinates are finite and |c| <= 16383; an invalid joint and its bones draw nothing. Background 0. Bones first, in edge order,
 * only when line_width = L > 0: bone (a, b), d = c_b - c_a, q = p - c_a, s = q.d, n = d.d (int64): s <= 0: 4 |q|^2 <= L^2;
 * s >= n: 4 |p - c_b|^2 <= L^2; else 4 (q x d)^2 <= L^2 n; colour colors[b]. Then joints in index order: |p - c_j|^2 <= radius^2,
 * colour colors[j]. A later primitive overwrites an earlier one.
 * A workgroup owns a 16 x 64 pixel tile of one (cell, video, frame): it rounds the frame's centres, compacts into LDS, in draw
 * order, the primitives whose bounding box grown by radius / ceil(L / 2) meets the tile, and each lane decides four pixels of a
 * row and stores their 12 bytes. Workgroups stride over the tiles; max_blocks 0: the kernel's own grid cap, > 0 lowers it.
 * p2c_render_points_supported: 0 <= n_panels <= min(P2C_RENDER_MAX_PANELS, rows cols), 0 <= J, E <= P2C_RENDER_MAX_PRIMS per panel,
 * C >= 2, 1 <= H, W <= 8192, W % 4 == 0, 0 <= radius, line_width <= P2C_RENDER_MAX_REACH, V, T, rows, cols >= 1.
 * p2c_render_points_fwd: P2C_E_SHAPE for what _supported refuses and for max_blocks < 0; P2C_E_NULL for a missing out, a panel
 * with points but no colors, or E > 0 without edges; both before any launch. No workspace, no host sync: capturable. */
#define P2C_RENDER_MAX_PANELS 8
#define P2C_RENDER_MAX_PRIMS 64
#define P2C_RENDER_MAX_REACH 64
#define P2C_RENDER_MAX_SIDE 8192
#define P2C_RENDER_MAX_COORD 16383
typedef struct p2c_render_panel {
  const float *points;
  const uint8_t *colors;
  const int32_t *edges;
  int32_t J, E, C;
  int32_t reserved;
} p2c_render_panel;
typedef struct p2c_render_points_desc {
  int32_t V, T;
  int32_t H, W;
  int32_t rows, cols;
  int32_t n_panels;
  int32_t radius, line_width;
  int32_t max_blocks;
  uint8_t *out;
  p2c_render_panel panels[P2C_RENDER_MAX_PANELS];
} p2c_render_points_desc;
P2C_API int p2c_render_points_supported(const p2c_render_points_desc *desc);   /* 1 = the shapes the kernel covers */
P2C_API int p2c_render_points_fwd(const p2c_render_points_desc *desc, void *stream);

/* ---- K35: SMPL body poses (AMASS) -> CARLA bone transforms in one launch (csrc/p2c_smpl.hip) ---------------------------------
 * What the reference does per clip on a DataLoader worker (data/smpl/smpl_dataset.py:103-142, convert_smpl_to_carla), for N = B T
 * frames, each independent of every other. fp32.
 *   body_pose (N,66): 22 joints x 3 Euler angles in ORIGINAL SMPL joint order (Pelvis, L_Hip, R_Hip, Spine1, ...).
 *   skel_type (N / frames_per_type) int32 on the device, rows of the reference tables; frame n has type
 *     skel_type[n / frames_per_type] (frames_per_type = T for one type per clip, 1 for one per frame). Not read on the host; a
 *     value outside [0, 4) is clamped in the kernel.
 *   ref_rel_loc (4,26,3), ref_rel_rot (4,26,3,3), ref_abs_rot (4,26,3,3): the reference tables.
 *   world_loc (N,3), world_rot (N,3,3): both NULL or both given; read for `root` only.
 * Per frame: M[s] = Rx Ry Rz of (-p0, p1, p2) of SMPL joint s; C[bone] = M[its joint], C[spine01] = M[Spine3] M[Spine2];
 * L = ref_abs_rot[t][bone] K, K = [[1,0,0],[0,0,-1],[0,1,0]]; relative_pose_rot = (L^T C L) ref_rel_rot[t][bone], and
 * ref_rel_rot[t][bone] itself for the five bones without an SMPL joint; absolute_pose_loc / _rot = forward kinematics of
 * (ref_rel_loc[t], relative_pose_rot) in the row-vector convention; bones = the p2c_carla_pose_fwd row of (ref_rel_loc[t],
 * relative_pose_rot); root = that of (world_loc, world_rot).
 * Outputs, each NULL or given, only the given ones are written: relative_pose_rot (N,26,3,3), absolute_pose_loc (N,26,3),
 * absolute_pose_rot (N,26,3,3), bones (N,26,6), root (N,6). What is written does not depend on which others are asked for.
 * max_blocks  0: the kernel's own grid cap; > 0 lowers it (groups of 32 lanes stride over the frames).
 * No masking: a NaN joint gives NaN in its bone and the bone's descendants, nowhere else. One writer per element, nothing reduced:
 * two runs give the same bits. N = 0: nothing is launched. N < 0, frames_per_type < 1, max_blocks < 0: P2C_E_SHAPE; a missing input,
 * no output at all, one world input without the other, root without world inputs: P2C_E_NULL; all before any launch. */
P2C_API int p2c_smpl_to_carla_fwd(const float *body_pose, const int32_t *skel_type, int64_t frames_per_type,
                                  const float *ref_rel_loc, const float *ref_rel_rot, const float *ref_abs_rot,
                                  const float *world_loc, const float *world_rot, float *relative_pose_rot,
                                  float *absolute_pose_loc, float *absolute_pose_rot, float *bones, float *root, int64_t N,
                                  int32_t max_blocks, void *stream);

/* ---- K36: 3-D joint locations -> CARLA bone rotations (inverse kinematics) in one launch (csrc/p2c_ik.hip) --------------------
 * What lets a movements model with the absolute_loc output drive a CARLA walker; the reference has no such step. Definition:
 * walker_control/inverse_kinematics.py (fit_carla_rotations). N = B T frames, each independent of every other. fp32 in and out,
 * the fit itself in fp64.
 *   loc (N,26,3): joint locations in CARLA_SKELETON order; only differences child - bone are read.
 *   skel_type (N / frames_per_type) int32 on the device, rows of the reference tables; frame n has type
 *     skel_type[n / frames_per_type]. Not read on the host; a value outside [0, 4) is clamped in the kernel.
 *   ref_rel_loc (4,26,3), ref_rel_rot (4,26,3,3): the relative reference tables.
 *   world_loc (N,3), world_rot (N,3,3): both NULL or both given; read for `root` only.
 * Per bone, parents first, A[parent(root)] = I: P = ref_rel_rot[t][j] A[parent]; a child c is usable when neither its reference
 * offset nor loc[c] - loc[j] has length zero; no usable child: A[j] = P and relative_pose_rot[j] = ref_rel_rot[t][j] itself; one
 * child in the tree: A[j] = P S, S the shortest arc from unit(r_c P) to unit(loc[c] - loc[j]) (a half turn about unit(u x e_k), k
 * the smallest |u_k|, when |u + v|^2 <= 2^-40); several children in the tree: A[j] = the proper rotation maximising
 * sum_c d_c . (r_c A) over the usable children's unit vectors; then relative_pose_rot[j] = A[j] A[parent]^T.
 * Outputs, each NULL or given, only the given ones are written: relative_pose_rot (N,26,3,3), absolute_pose_loc (N,26,3) = forward
 * kinematics of (ref_rel_loc[t], A), absolute_pose_rot (N,26,3,3) = A, bones (N,26,6) = the p2c_carla_pose_fwd row of
 * (ref_rel_loc[t], relative_pose_rot), root (N,6) = that of (world_loc, world_rot). What is written does not depend on which
 * others are asked for.
 * max_blocks  0: the kernel's own grid cap; > 0 lowers it (groups of 32 lanes stride over the frames).
 * No masking: a non-finite joint goes wherever the arithmetic takes it. One writer per element, nothing reduced: two runs give
 * the same bits. N = 0: nothing is launched. N < 0, frames_per_type < 1, max_blocks < 0: P2C_E_SHAPE; a missing input, no output at
 * all, one world input without the other, root without world inputs: P2C_E_NULL; all before any launch. */
P2C_API int p2c_loc_to_carla_fwd(const float *loc, const int32_t *skel_type, int64_t frames_per_type, const float *ref_rel_loc,
                                 const float *ref_rel_rot, const float *world_loc, const float *world_rot,
                                 float *relative_pose_rot, float *absolute_pose_loc, float *absolute_pose_rot, float *bones,
                                 float *root, int64_t N, int32_t max_blocks, void *stream);

/* ---- K37: CARLA rows resampled to another frame rate in one launch (csrc/p2c_resample.hip) -----------------------------------
 * What lets rows exported at a source's rate (video 30 / 29.97 fps, mocap 60 / 120 fps) be played at the simulator's tick; the
 * reference has no such step. Definition: walker_control/resample.py. N videos, each row (x, y, z, pitch, yaw, roll).
 *   bones (N,T,J,6), root (N,T,6) or NULL: the source frames with global indices first_frame .. first_frame + T - 1.
 *   carry_bones (N,J,6), carry_root (N,6) or NULL: the source frame with global index first_frame - 1 (a streaming caller's
 *     last frame of the previous chunk).
 *   out_bones (N,K,J,6), out_root (N,K,6) or NULL: output samples with global indices first_output .. first_output + K - 1.
 * Output sample k sits at source position p = fl64(k * ratio), ratio = src_fps / dst_fps: i0 = floor(p), frac = (float)(p - i0).
 * mode P2C_RESAMPLE_SLERP: frac == 0 copies row i0 bit for bit (row i0 + 1 is not read); otherwise locations are
 * a + frac (b - a) and rotations the shortest-arc spherical interpolation of the rows' quaternions (w first, q = qx(e0) qy(e1)
 * qz(e2), (e0, e1, e2) = radians(-roll, -pitch, -yaw); weights (1 - frac, frac) above a dot product of 0.99999), written back
 * through the row arithmetic of p2c_carla_pose_fwd. mode P2C_RESAMPLE_HOLD: row i0, copied. A NaN in a neighbour reaches that
 * output row and nothing else. A source index outside [first_frame - (carry given), first_frame + T - 1] is clamped in the
 * kernel, never followed: the caller checks that the requested outputs lie inside.
 * max_blocks  0: the kernel's own grid cap; > 0 lowers it (lanes stride over the output rows).
 * One lane per output row, one writer per element, nothing reduced; a row's bits depend on its two source rows and frac only.
 * In this order, before anything is launched: P2C_E_SHAPE for negative sizes or indices, J < 1, max_blocks < 0, N K (J + 1) > 2^40,
 * N T (J + 1) > 2^40, first_frame + T or first_output + K > 2^40, ratio not finite or outside [2^-10, 2^10], another mode, outputs
 * asked of no frames (T = 0 with N, K > 0); P2C_E_NULL for a missing bones / out_bones, root without out_root or the reverse,
 * carry_root without carry_bones, carry_bones without carry_root when root is given. Then N = 0 or K = 0: nothing is launched. */
enum { P2C_RESAMPLE_SLERP = 0, P2C_RESAMPLE_HOLD = 1 };
P2C_API int p2c_carla_resample_fwd(const float *bones, const float *root, const float *carry_bones, const float *carry_root,
                                   float *out_bones, float *out_root, int64_t N, int64_t T, int32_t J, int64_t K,
                                   int64_t first_output, int64_t first_frame, double ratio, int32_t mode, int32_t max_blocks,
                                   void *stream);

/* ---- K38: Carla2D3D training batches generated on the device in one launch (csrc/p2c_generate.hip) --------------------------
 * The reference's infinite training set (data/carla/datasets/carla_2d3d_dataset.py:145-210, Carla2D3DIterableDataset.generate_batch)
 * for clips first_clip .. first_clip + B - 1 of (seed, draw_stream). Every random number is a pure function of (seed, draw_stream,
 * clip index, frame, joint, channel): the key schedule and what is made of a word are defined in
 * pedestrians_video_2_carla_amd/data/carla/generator.py, which this entry point equals to the bit. Nothing is read from the device
 * but the reference tables; there is no state.
 *   random_changes_each_frame in [0, 26] joints per frame get Euler angles (2u - 1) max_change_rad; the world's yaw changes by
 *   (2u - 1) max_initial_world_rot_change_rad in frame 0 when that is > 0 and by (2u - 1) max_world_rot_change_rad in later frames
 *   when that is != 0; with both 0 the world is the identity and takes no part in the projection.
 *   transform  P2C_TRANSFORM_*, the data-side normaliser (p2c_collate_fwd's, CARLA hips / neck joints); noise P2C_GENERATE_NOISE_*:
 *   UNIFORM adds u noise_param - noise_param / 2 per channel; miss_prob: NULL or 26 HOST floats, joint j of a frame becomes (0, 0)
 *   where its draw u < miss_prob[j]. camera: 5 HOST floats (f, cx, cy, distance, elevation). ref_rel_loc (4,26,3), ref_rel_rot
 *   (4,26,3,3): the reference tables on the device.
 * Per clip: skeleton type = the top two bits of the clip's word; rel[t] = C[t] rel[t-1] from the type's ref_rel_rot; absolute pose
 * by forward kinematics (row vectors); world_rot[t] = world_rot[t-1] Rz(yaw[t]); projection as p2c_pose_head_fwd; then the tail of
 * p2c_collate_fwd: projection_2d_deformed = projection_2d + noise with missing joints zeroed, frames = normalise(deformed),
 * projection_2d_transformed / _shift / _scale = normalise(projection_2d).
 * Outputs, each NULL or given, only the given ones are written, and what is written does not depend on which others are asked for:
 * frames, projection_2d, projection_2d_deformed, projection_2d_transformed (B,T,26,2); projection_2d_shift (B,T,2);
 * projection_2d_scale (B,T); pose_changes, relative_pose_rot, absolute_pose_rot (B,T,26,3,3); relative_pose_loc, absolute_pose_loc
 * (B,T,26,3); world_loc, world_loc_changes (B,T,3: zeros); world_rot, world_rot_changes (B,T,3,3); skel_type (B) int32.
 * mapping  P2C_GENERATE_SEQUENTIAL: a 32-lane group per clip walks its frames; P2C_GENERATE_FRAME_PARALLEL: a group per (clip,
 *   frame) replays the draws and running products of the frames before its own; P2C_GENERATE_AUTO: the latter up to
 *   P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES frames in the batch. Both give the same bits.
 * max_blocks  0: the kernel's own grid cap; > 0 lowers it (groups stride over clips, or over frames).
 * One writer per element, no atomics, no LDS: two runs give the same bits. In this order, before anything is launched: P2C_E_SHAPE
 * for B < 0, T outside [1, P2C_GENERATE_MAX_T], first_clip < 0, B T > 2^40, random_changes_each_frame outside [0, 26],
 * max_blocks < 0; P2C_E_ENUM for another transform, noise or mapping, or a transformed / shift / scale output with
 * P2C_TRANSFORM_NONE; P2C_E_NULL for a missing camera or table, or no output at all. Then B = 0: nothing is launched. */
enum { P2C_GENERATE_NOISE_ZERO = 0, P2C_GENERATE_NOISE_UNIFORM = 1 };
enum { P2C_GENERATE_AUTO = 0, P2C_GENERATE_SEQUENTIAL = 1, P2C_GENERATE_FRAME_PARALLEL = 2 };
#define P2C_GENERATE_MAX_T 65536
#define P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES 8192
P2C_API int p2c_carla_generate_fwd(int64_t seed, int32_t draw_stream, int64_t first_clip, int64_t B, int32_t T,
                                   int32_t random_changes_each_frame, float max_change_rad, float max_world_rot_change_rad,
                                   float max_initial_world_rot_change_rad, int32_t transform, int32_t noise, float noise_param,
                                   const float *miss_prob, float near_zero, const float *camera, const float *ref_rel_loc,
                                   const float *ref_rel_rot, float *frames, float *projection_2d, float *projection_2d_deformed,
                                   float *projection_2d_transformed, float *projection_2d_shift, float *projection_2d_scale,
                                   float *pose_changes, float *relative_pose_loc, float *relative_pose_rot,
                                   float *absolute_pose_loc, float *absolute_pose_rot, float *world_loc, float *world_rot,
                                   float *world_loc_changes, float *world_rot_changes, int32_t *skel_type, int32_t mapping,
                                   int32_t max_blocks, void *stream);

/* ---- K39: CARLA rows smoothed along time in one launch (csrc/p2c_smooth.hip) ------------------------------------------------
 * What takes the frame-to-frame jitter of per-frame predictions out of an animation before it is played; the reference has no
 * such step. Definition: walker_control/smooth.py. N videos, each row (x, y, z, pitch, yaw, roll); rotations are filtered as the
 * unit quaternions of p2c_carla_resample_fwd and written back through the row arithmetic of p2c_carla_pose_fwd. fp32, no backward.
 *
 * p2c_carla_smooth_gauss_fwd: a zero-phase weighted mean over 2R + 1 frames.
 *   bones (N,S,J,6), root (N,S,6) or NULL: the source frames with global indices first_frame .. first_frame + S - 1.
 *   out_bones (N,K,J,6), out_root (N,K,6) or NULL: output frames with global indices first_output .. first_output + K - 1.
 *   weights (R + 1) on the device: weights[d] for a neighbour d frames away (the host's float32(exp(-d^2 / (2 sigma^2)))); not read
 *     and may be NULL with R = 0.
 *   last_frame: the global index of the video's last frame, or -1 while it is not known.
 * Output frame t combines source frames max(0, t - R) .. min(t + R, last_frame): locations sum(w x) / sum(w), rotations the
 * normalised sum of w q over the neighbours' quaternions, each negated when its dot product with the centre frame's is < 0; every
 * sum in ascending frame order. R = 0 copies the rows bit for bit. A NaN in a source row reaches the outputs of that row within R
 * frames and nothing else. A window is clamped into the given frames in the kernel, never followed outside them, and an output
 * whose own frame is not given is NaN: the caller checks that every window lies inside (with last_frame = -1: up to t + R).
 * A workgroup converts the rows of a tile's F + 2R source frames once into LDS (F <= 32; at most 64 KB) and forms the tile's
 * output rows from there. A row's bits depend on its window's source rows and the table only: not on the tile, the grid, whether
 * the root is asked for, or where a streaming caller cut the video. One writer per element, no atomics.
 *
 * p2c_carla_smooth_euro_fwd: the one-euro filter (Casiez et al.), causal, a lane per (video, row) walking its T frames.
 *   bones (N,T,J,6), root (N,T,6) or NULL -> out_bones, out_root of the same shapes.
 *   state_bones (N,J,12), state_root (N,12): per row (x^ 3, v^ 3, q^ 4 w first, w^ 1, 0). has_state = 1: read before frame 0 (the
 *     frames continue a video); has_state = 0: frame 0 starts the state (x^ = x, q^ = the row's quaternion, v^ = w^ = 0) and its
 *     row is copied bit for bit. Where a state pointer is given the state after frame T - 1 is written there.
 *   With alpha(fc) = 1 / (1 + fps / (2 pi fc)): v = (x - x^) fps, v^ += alpha(d_cutoff) (v - v^), x^ += alpha(min_cutoff +
 *   beta_loc |v^|) (x - x^); q the row's quaternion on q^'s hemisphere, d = min(q^ . q, 1) by comparison, w = 2 acos(d) fps,
 *   w^ += alpha(d_cutoff) (w - w^), q^ = normalised slerp(q^, q, alpha(min_cutoff + beta_rot w^)) with lerp weights above
 *   d = 0.99999. The parameters are used at their fp32 values; alpha(d_cutoff) and fps / 2 pi are formed in fp64 and
 *   rounded once. A NaN row poisons its own chain from that frame on and nothing else. No LDS, no atomics.
 *
 * max_blocks  0: the kernel's own grid cap; > 0 lowers it (workgroups stride over tiles, lanes over chains).
 * In this order, before anything is launched: P2C_E_SHAPE for negative sizes or indices (last_frame < -1), J < 1, max_blocks < 0,
 * R outside [0, P2C_SMOOTH_MAX_RADIUS], N K (J + 1) or N S (J + 1) > 2^40, first_frame + S or first_output + K > 2^40, outputs
 * asked of no frames (S = 0 with N, K > 0), has_state other than 0 / 1, fps, min_cutoff or d_cutoff not finite or not positive
 * (as given or as fp32), a beta that is negative or not finite; P2C_E_NULL for a missing bones / out_bones, root without out_root
 * or the reverse, weights missing with R > 0, a state missing where it is read. Then N = 0 or K = 0 (T = 0): nothing is launched. */
#define P2C_SMOOTH_MAX_RADIUS 32
P2C_API int p2c_carla_smooth_gauss_fwd(const float *bones, const float *root, float *out_bones, float *out_root,
                                       const float *weights, int64_t N, int64_t S, int32_t J, int64_t K, int64_t first_frame,
                                       int64_t first_output, int64_t last_frame, int32_t R, int32_t max_blocks, void *stream);
P2C_API int p2c_carla_smooth_euro_fwd(const float *bones, const float *root, float *state_bones, float *state_root,
                                      float *out_bones, float *out_root, int64_t N, int64_t T, int32_t J, int32_t has_state,
                                      double fps, double min_cutoff, double beta_loc, double beta_rot, double d_cutoff,
                                      int32_t max_blocks, void *stream);

/* ---- K40: root motion of a CARLA animation from its planted feet (csrc/p2c_root_motion.hip) ---------------------------------
 * Every exporter takes the root row from world_loc, which the only trajectory model (ZeroTrajectory) leaves at zero: a played
 * animation walks on the spot. This stage puts the displacement back: the contact joint that is lowest over two neighbouring
 * frames must not move in the world, so the actor moves the other way. Definition: walker_control/root_motion.py. fp32, no backward.
 *   bones (N,T,26,6), root (N,T,6) or NULL (all-zero root rows): frames first_frame .. first_frame + T - 1 of N videos.
 *   Per frame g: (l, R) of every row as p2c_carla_pose_inv forms them, forward kinematics over the 26-bone tree (row vectors), the
 *   actor as one more parent: p_k = x_{C_k} W + r for C = bones (18, 19, 23, 24) (foot R, toe R, foot L, toe L); h_k = -p_k[2].
 *   g >= 1: m_k = max(h_k(g - 1), h_k(g)); s = the smallest k with minimal m_k; d = p_s(g - 1)[0:2] - p_s(g)[0:2];
 *     step(g) = rint(d * 2^10) (half to even) as two int32; contact(g) = s. A non-finite value among the eight heights or the four
 *     coordinates read, or |d * 2^10| >= 2^31: step(g) = (0, 0), contact(g) = -1.
 *   g == 0: step = (0, 0), contact = argmin_k h_k(0), -1 when a height is not finite.
 *   S(g) = S(g - 1) + step(g) in int64, S(-1) = 0: an integer sum, exact and independent of mapping, grid, tiling and cuts.
 *   out_root (N,T,6): x = fp32(fp64(x) + S_x(g) 2^-10), y likewise; z unchanged, or with has_ground = 1 z + (fp32(ground) - min_k
 *     h_k(g)) in fp32 (NaN when a height of the frame is not finite); the three angles bit for bit. The bones are not rewritten.
 *   out_steps (N,T,2) int32, out_contact (N,T) int8: NULL or given; what is written to an output does not depend on the others.
 *   state_in_offset (N,2) int64 + state_in_points (N,4,3): S(first_frame - 1) and the four p_k of frame first_frame - 1, both or
 *     neither; required and read with first_frame > 0, not read with first_frame = 0 (nothing lies before a video's first frame).
 *   state_out_offset + state_out_points: both or neither; S and the p_k of the last frame given.
 *   mapping  P2C_ROOT_MOTION_PER_VIDEO: a workgroup per video walks its tiles of P2C_ROOT_MOTION_TILE frames in order, one launch;
 *     P2C_ROOT_MOTION_FRAME_PARALLEL: a workgroup per (video, tile) in two launches (steps and tile totals to the workspace, then
 *     the rows); P2C_ROOT_MOTION_AUTO: by size. All give the same bits.
 *   workspace  p2c_carla_root_motion_workspace(N, T, mapping) bytes on the device, 16-byte aligned (0: not used, may be NULL);
 *     every word that is read was written by the same call.
 *   max_blocks  0: the kernels' own grid cap; > 0 lowers it (workgroups stride over videos, or over tiles).
 * One writer per element, no atomics. In this order, before anything is launched: P2C_E_SHAPE for negative sizes or first_frame,
 * N, T or first_frame + T > 2^40, N T 27 > 2^40, max_blocks < 0, has_ground other than 0 / 1, a ground that is not finite (as given
 * or as fp32); P2C_E_ENUM for another mapping; P2C_E_NULL for a missing bones / out_root, one half of a state pair, first_frame > 0
 * without state_in, a missing workspace where the mapping uses one. Then N = 0 or T = 0: nothing is launched.
 * p2c_carla_root_motion_tile: P2C_ROOT_MOTION_TILE. p2c_carla_root_motion_workspace: the bytes, or -1 for sizes or a mapping the
 * entry point refuses. */
enum { P2C_ROOT_MOTION_AUTO = 0, P2C_ROOT_MOTION_PER_VIDEO = 1, P2C_ROOT_MOTION_FRAME_PARALLEL = 2 };
#define P2C_ROOT_MOTION_TILE 128
P2C_API int32_t p2c_carla_root_motion_tile(void);
P2C_API int64_t p2c_carla_root_motion_workspace(int64_t N, int64_t T, int32_t mapping);
P2C_API int p2c_carla_root_motion_fwd(const float *bones, const float *root, const int64_t *state_in_offset,
                                      const float *state_in_points, float *out_root, int32_t *out_steps, int8_t *out_contact,
                                      int64_t *state_out_offset, float *state_out_points, int64_t N, int64_t T,
                                      int64_t first_frame, double ground, int32_t has_ground, int32_t mapping,
                                      int32_t max_blocks, void *workspace, void *stream);

/* ---- K41: a CARLA animation as a loop: cycle search and seam blend (csrc/p2c_loop.hip) ---------------------------------------
 * The exported rows are as long as the clip that went in; a scenario needs a walker that keeps walking. Replaying the rows jumps
 * at the seam and, after K40, snaps the root back. This stage finds the cycle that closes best and plays it for any number of
 * frames; the reference has no such step. Definition: walker_control/loop.py. fp32, no backward. q[t, j] is the unit quaternion
 * of bone row (t, j) as p2c_carla_resample_fwd forms it.
 *
 * p2c_carla_loop_find_fwd: the search, per video.
 *   bones (N,T,J,6); weights (J) finite and >= 0 on the device, or NULL for ones. The root is not read.
 *   d(a, b) = sum_j w_j (1 - <q[a,j], q[b,j]>^2), j ascending, the four products of a dot product added from the first to the last.
 *   C(s, e) = sum_{k = -blend .. 0} d(s + k, e + k), k ascending, where blend <= s, s + min_period <= e <= s + max_period and
 *   e <= T - 1 (an admissible pair); +inf elsewhere.
 *   out_loop (N,2) int64, out_loop_cost (N): the admissible pair with the smallest finite cost, ties to the smallest s, then the
 *     smallest e, and its cost; (-1, -1) and NaN when no admissible pair has a finite cost.
 *   out_cost (N,T,T) or NULL: every C(s, e). What is written to an output does not depend on the others.
 *   workspace  p2c_carla_loop_find_workspace(N, T, J, blend) bytes on the device, 8-byte aligned: one 64-bit word a video, set and
 *     read back by the same call (-1: sizes the entry point refuses).
 * A workgroup takes a (video, 32 x 32 tile of (s, e)); a tile off the band min_period <= e - s <= max_period is skipped. The
 * quaternions of the tile's 2 (32 + blend) frames are formed once into LDS, the (32 + blend)^2 tile of d there, and each lane sums
 * its pairs' diagonals in ascending k; at most 64 KB, the bones in chunks when they do not fit. The video's minimum is an integer
 * atomic minimum on an order-preserving 64-bit key (the cost's bits, then s, then e): exact, independent of the order of arrival.
 * No floating-point atomics. C(s, e) is the work of one lane in a fixed order: its bits do not depend on the grid, on max_blocks,
 * on whether out_cost is asked for or on the batch around the video. A NaN row poisons the entries whose window reads it.
 *
 * p2c_carla_loop_play_fwd: the chosen cycles played, one lane per output row.
 *   bones (N,T,J,6), root (N,T,6) or NULL; loop (N,2) int64 on the device; out_bones (N,frames,J,6), out_root (N,frames,6) or NULL:
 *     outputs first_output .. first_output + frames - 1.
 *   Output g of a video with loop (s, e), P = e - s: c = g div P, phi = g mod P, a = s + phi. phi < P - blend: row a copied bit for
 *   bit. Otherwise u = (float)((phi - (P - blend) + 1) / (double)(blend + 1)), b = a - P, and the row is the interpolation of
 *   p2c_carla_resample_fwd of rows a and b at u. Root x and y in fp64: delta = root[e] - root[s]; m = root[a] outside the window,
 *   (1 - u) root[a] + u (root[b] + delta) inside; out = (float)(m + c delta), every product and sum rounded on its own; cycle 0
 *   outside the window is copied. A video whose loop is not blend <= s < e <= T - 1 -- (-1, -1) among them -- plays NaN rows; no
 *   loop is followed outside the video. An output depends on g alone: pieces give the bits of one call. No LDS, no atomics.
 *
 * max_blocks  0: the kernels' own grid cap; > 0 lowers it (workgroups stride over tiles, lanes over rows).
 * In this order, before anything is launched: P2C_E_SHAPE for negative sizes or first_output, max_blocks < 0, J outside
 * [1, P2C_LOOP_MAX_J], blend outside [0, P2C_LOOP_MAX_BLEND], T > P2C_LOOP_MAX_T, N T (J + 1) or N frames (J + 1) >= 2^31,
 * first_output > 2^40; the search: T < 2, min_period < 1, max_period < min_period; the player: T < 2 with outputs asked for;
 * P2C_E_NULL for a missing bones, loop, out_loop, out_loop_cost or out_bones, root without out_root or the reverse, a missing
 * workspace. Then N = 0 or frames = 0: nothing is launched. */
#define P2C_LOOP_MAX_BLEND 32
#define P2C_LOOP_MAX_J 64
#define P2C_LOOP_MAX_T 16384
P2C_API int64_t p2c_carla_loop_find_workspace(int64_t N, int64_t T, int32_t J, int32_t blend);
P2C_API int p2c_carla_loop_find_fwd(const float *bones, const float *weights, int64_t *out_loop, float *out_loop_cost,
                                    float *out_cost, int64_t N, int64_t T, int32_t J, int32_t blend, int64_t min_period,
                                    int64_t max_period, int32_t max_blocks, void *workspace, void *stream);
P2C_API int p2c_carla_loop_play_fwd(const float *bones, const float *root, const int64_t *loop, float *out_bones,
                                    float *out_root, int64_t N, int64_t T, int32_t J, int64_t frames, int64_t first_output,
                                    int32_t blend, int32_t max_blocks, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* P2C_H */
