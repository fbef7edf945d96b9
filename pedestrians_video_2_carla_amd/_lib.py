"""ctypes binding of libp2c_hip.so (C ABI in include/p2c.h).

There is no CPU fallback: if the shared library is missing or an op is given host tensors, the call raises.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('P2C_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libp2c_hip.so')    # (P2C_LIB_PATH: A/B builds, tools only)
P2C_JOINTS = 26

KIND = {'pose_changes_6d': 0, 'pose_changes': 1, 'relative_rot_6d': 2, 'relative_rot': 3, 'absolute_loc': 4}
TRANSFORM = {'none': 0, 'hips_neck': 1, 'bbox': 2, 'hips_neck_bbox': 3}
PRECISION = {'fp32': 0, 'bf16': 1, 'bf16x3': 2}

_f32p = ctypes.c_void_p  # device pointers travel as plain addresses
_i32 = ctypes.c_int32


class PoseHeadDesc(ctypes.Structure):
    """Mirror of ``p2c_pose_head_desc`` (include/p2c.h) -- keep field order in sync."""
    _fields_ = [
        ('B', _i32), ('T', _i32), ('kind', _i32), ('transform', _i32), ('t0', _i32), ('t1', _i32),
        ('mask_missing_joints', _i32), ('hips_lane', _i32), ('n_hips', _i32), ('n_neck', _i32),
        ('hips_idx', _i32 * 2), ('neck_idx', _i32 * 2),
        ('gt2d_joints', _i32), ('gt2d_channels', _i32), ('gt3d_joints', _i32),
        ('gmap2d', _i32 * P2C_JOINTS), ('gmap3d', _i32 * P2C_JOINTS), ('n_common2d', _i32), ('n_common3d', _i32), ('world_absolute', _i32),
        ('cam_f', ctypes.c_float), ('cam_cx', ctypes.c_float), ('cam_cy', ctypes.c_float),
        ('cam_dist', ctypes.c_float), ('cam_elev', ctypes.c_float), ('near_zero', ctypes.c_float),
        ('y', _f32p), ('skel_type', _f32p), ('ref_rel_loc', _f32p), ('ref_rel_rot', _f32p),
        ('ref_hn_shift', _f32p), ('ref_hn_scale', _f32p), ('dloc', _f32p), ('drot', _f32p),
        ('gt2d', _f32p), ('gt3d', _f32p),
        ('partials', _f32p), ('loss_sums', _f32p), ('losses', _f32p), ('final_rel_rot', _f32p),
        ('out_pose_changes', _f32p), ('out_projection_2d', _f32p), ('out_projection_2d_transformed', _f32p),
        ('out_shift', _f32p), ('out_scale', _f32p), ('out_relative_pose_loc', _f32p),
        ('out_relative_pose_rot', _f32p), ('out_absolute_pose_loc', _f32p), ('out_absolute_pose_rot', _f32p),
        ('out_world_loc', _f32p), ('out_world_rot', _f32p), ('defer_loss_finalize', _i32),
        ('gt_rot', _f32p), ('grad_loss_rot', _f32p),
    ]


P2C_MLP_MAX_LAYERS = 8
# what p2c_mlp_plan writes (the P2C_MLP_PLAN_* indices of include/p2c.h, in order) into P2C_MLP_PLAN_INTS values
P2C_MLP_PLAN_FIELDS = ('provider', 'wave_forward', 'split_wgrad', 'save_activations', 'fwd_blocks', 'bwd_blocks', 'tiles',
                       'image_floats', 'lds_fwd', 'lds_bwd', 'lds_fwd_wave', 'fwd_ok', 'bwd_ok')
P2C_MLP_PLAN_INTS = 16


class MlpDesc(ctypes.Structure):
    """Mirror of ``p2c_mlp_desc`` (include/p2c.h)."""
    _fields_ = [
        ('n_layers', _i32), ('dims', _i32 * (P2C_MLP_MAX_LAYERS + 1)), ('N', ctypes.c_int64), ('x', _f32p),
        ('W', _f32p * P2C_MLP_MAX_LAYERS), ('b', _f32p * P2C_MLP_MAX_LAYERS), ('y', _f32p), ('gy', _f32p),
        ('gW', _f32p * P2C_MLP_MAX_LAYERS), ('gb', _f32p * P2C_MLP_MAX_LAYERS), ('partials', _f32p), ('w_image', _f32p),
        ('fused_adamw', _f32p), ('skip_pack', ctypes.c_int32), ('saved', _f32p), ('precision', ctypes.c_int32),
    ]


class TrainStepDesc(ctypes.Structure):
    """Mirror of ``p2c_train_step_desc`` (include/p2c.h)."""
    _fields_ = [('head', PoseHeadDesc), ('mlp', MlpDesc), ('pair_counts', _f32p)]


class LiftDesc(ctypes.Structure):
    """Mirror of ``p2c_lift_desc`` (include/p2c.h)."""
    _fields_ = [('mlp', MlpDesc), ('B', _i32), ('T', _i32), ('kind', _i32), ('max_blocks', _i32), ('skel_type', _f32p),
                ('ref_rel_loc', _f32p), ('ref_rel_rot', _f32p), ('world_loc', _f32p), ('world_rot', _f32p),
                ('initial_rel_rot', _f32p), ('bones', _f32p), ('root', _f32p), ('final_rel_rot', _f32p),
                ('out_relative_pose_rot', _f32p)]


# every symbol include/p2c.h declares: (restype, argtypes)
_vp, _i64, _ip = ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int32)
class AdamWDesc(ctypes.Structure):
    """p2c_adamw_desc (include/p2c.h)."""
    _fields_ = [('n', ctypes.c_int64), ('param', _f32p), ('grad', _f32p), ('exp_avg', _f32p), ('exp_avg_sq', _f32p),
                ('step', _f32p), ('ticket', _f32p), ('hyper', _f32p), ('adamw', ctypes.c_int32),
                ('zero_grad', ctypes.c_int32), ('scatter_idx', _f32p), ('scatter_dst', _f32p)]


P2C_CLIP_NORM, P2C_CLIP_VALUE = 1, 2


class ClipDesc(ctypes.Structure):
    """p2c_clip_desc (include/p2c.h)."""
    _fields_ = [('mode', ctypes.c_int32), ('bound', ctypes.c_float), ('partials', _f32p), ('total_norm', _f32p)]


class GemmDesc(ctypes.Structure):
    """p2c_gemm_desc (include/p2c.h)."""
    _fields_ = [('M', ctypes.c_int32), ('N', ctypes.c_int32), ('K', ctypes.c_int32), ('trans_b', ctypes.c_int32),
                ('a', _f32p), ('lda', ctypes.c_int64), ('b', _f32p), ('ldb', ctypes.c_int64), ('c', _f32p), ('ldc', ctypes.c_int64),
                ('bias', _f32p), ('act', ctypes.c_int32), ('rows_per_scale', ctypes.c_int32), ('aux', _f32p), ('aux_out', _f32p),
                ('ldaux', ctypes.c_int64), ('row_scale', _f32p), ('residual', _f32p), ('ldr', ctypes.c_int64),
                ('drop_state', ctypes.c_void_p), ('drop_p', ctypes.c_float), ('drop_site', ctypes.c_int32)]


class LstmDesc(ctypes.Structure):
    """p2c_lstm_desc (include/p2c.h)."""
    _fields_ = [('T', ctypes.c_int32), ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('gx', _f32p), ('h0', _f32p),
                ('c0', _f32p), ('w_hh', _f32p), ('out', _f32p), ('hT', _f32p), ('cT', _f32p), ('acts', _f32p),
                ('cs', _f32p), ('g_out', _f32p), ('g_hT', _f32p), ('g_cT', _f32p), ('g_gx', _f32p), ('g_h0', _f32p),
                ('g_c0', _f32p), ('bias_a', _f32p), ('bias_b', _f32p), ('g_gx_bt', _f32p), ('gx_bt', ctypes.c_int32),
                ('out_drop', _f32p), ('drop_state', ctypes.c_void_p), ('drop_p', ctypes.c_float), ('drop_site', ctypes.c_int32)]


class GruDesc(ctypes.Structure):
    """p2c_gru_desc (include/p2c.h)."""
    _fields_ = [('T', ctypes.c_int32), ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('gx', _f32p), ('h0', _f32p),
                ('w_hh', _f32p), ('bias_hh', _f32p), ('out', _f32p), ('hT', _f32p), ('acts', _f32p), ('g_out', _f32p),
                ('g_hT', _f32p), ('g_gx', _f32p), ('g_gh', _f32p), ('g_h0', _f32p), ('gx_bt', ctypes.c_int32),
                ('out_drop', _f32p), ('drop_state', ctypes.c_void_p), ('drop_p', ctypes.c_float), ('drop_site', ctypes.c_int32)]


P2C_CLS_BINARY, P2C_CLS_COUNT_ONLY = 1, 2
P2C_RANK_GLOBAL = 1
P2C_RANK_MAX_CLASSES, P2C_RANK_MAX_ROWS, P2C_RANK_LDS_ROWS = 32, 1 << 24, 16384


class RankDesc(ctypes.Structure):
    """p2c_rank_desc (include/p2c.h)."""
    _fields_ = [('N', ctypes.c_int64), ('C', ctypes.c_int32), ('flags', ctypes.c_int32)] + [
        (n, _f32p) for n in ('scores', 'targets', 'thresholds', 'tps', 'fps', 'n_points', 'n_pos', 'auroc', 'n_valid')]


class BnormDesc(ctypes.Structure):
    """p2c_bnorm_desc (include/p2c.h)."""
    _fields_ = [('N', _i64), ('C', _i32), ('training', _i32), ('relu', _i32), ('accumulate', _i32), ('eps', ctypes.c_float),
                ('momentum', ctypes.c_float)] + [(n, _f32p) for n in ('y', 'gamma', 'beta', 'residual', 'z', 'mean', 'rstd',
                                                                     'running_mean', 'running_var', 'g_z', 'g_y', 'g_gamma',
                                                                     'g_beta')] + [
        ('drop_state', ctypes.c_void_p), ('drop_p', ctypes.c_float), ('drop_site', _i32)]


class DecoderDesc(ctypes.Structure):
    """p2c_decoder_desc (include/p2c.h)."""
    _fields_ = [('T', ctypes.c_int32), ('B', ctypes.c_int32), ('H', ctypes.c_int32), ('O', ctypes.c_int32)] + [
        (n, _f32p) for n in ('k0', 'c0', 'k1', 'c1', 'w_ih0', 'w_ih1', 'w_fc', 'b_fc', 'x0', 'drop', 'out', 'acts0', 'acts1',
                             'h0d', 'h1', 'g_out', 'g_gates0', 'g_gates1', 'g_outtot', 'g_c0', 'g_c1',
                             'hid0', 'hid1', 'w_hh0', 'w_hh1', 'b0a', 'b0b', 'b1a', 'b1b', 'kw0', 'kw1', 'out_bt',
                             'g_k0', 'g_k1', 'g_hid0', 'g_hid1')] + [('g_out_bt', ctypes.c_int32), ('force', _f32p), ('target', _f32p),
                                                     ('drop_state', ctypes.c_void_p), ('drop_p', ctypes.c_float), ('drop_site', ctypes.c_int32)]


class AtbProblem(ctypes.Structure):
    """p2c_atb_problem (include/p2c.h)."""
    _fields_ = [('a', _f32p), ('a_stride', _i64), ('b', _f32p), ('b_stride', _i64), ('K', _i64), ('M', _i32), ('N', _i32),
                ('out', _f32p), ('out_stride', _i64), ('bias_out', _f32p), ('bias_out2', _f32p), ('flags', _i32)]


class CollateDesc(ctypes.Structure):
    """p2c_collate_desc (include/p2c.h)."""
    _fields_ = [('N', _i64), ('T', _i32), ('Jd', _i32), ('C', _i32), ('raw', _f32p), ('is_flipped', _vp),
                ('flip_perm', _ip), ('rotation_deg', _f32p), ('bboxes', _f32p), ('clip_size', _f32p), ('noise', _f32p),
                ('miss_u', _f32p), ('miss_prob', ctypes.POINTER(ctypes.c_float)), ('transform', _i32), ('n_hips', _i32),
                ('hips_idx', _i32 * 2), ('n_neck', _i32), ('neck_idx', _i32 * 2), ('near_zero', ctypes.c_float),
                ('return_confidence', _i32), ('Ji', _i32), ('K', _i32), ('src_idx', _ip), ('dst_idx', _ip),
                ('frames', _f32p), ('t_projection_2d', _f32p), ('t_deformed', _f32p), ('t_transformed', _f32p),
                ('shift', _f32p), ('scale', _f32p), ('bboxes_out', _f32p)]


P2C_COLLATE_MAX_SOURCES = 4
_fp = ctypes.POINTER(ctypes.c_float)


class CollateSource(ctypes.Structure):
    """p2c_collate_source (include/p2c.h)."""
    _fields_ = [('n', _i64), ('raw', _f32p), ('Jd', _i32), ('C', _i32), ('flip_perm', _ip), ('miss_prob', _fp),
                ('transform', _i32), ('n_hips', _i32), ('hips_idx', _i32 * 2), ('n_neck', _i32), ('neck_idx', _i32 * 2),
                ('K', _i32), ('src_idx', _ip), ('dst_idx', _ip), ('has_noise', _i32), ('has_miss', _i32),
                ('has_bboxes', _i32)]


class CollateMixedDesc(ctypes.Structure):
    """p2c_collate_mixed_desc (include/p2c.h)."""
    _fields_ = [('N', _i64), ('T', _i32), ('Ji', _i32), ('S', _i32), ('return_confidence', _i32),
                ('near_zero', ctypes.c_float), ('sources', CollateSource * P2C_COLLATE_MAX_SOURCES), ('source', _vp),
                ('row', _vp), ('is_flipped', _vp), ('rotation_deg', _f32p), ('bboxes', _f32p), ('clip_size', _f32p),
                ('noise', _f32p), ('miss_u', _f32p), ('frames', _f32p), ('t_projection_2d', _f32p), ('t_deformed', _f32p),
                ('t_transformed', _f32p), ('shift', _f32p), ('scale', _f32p), ('bboxes_out', _f32p)]


P2C_RELU_STACK_MAX_LAYERS = 5


class ReluStackDesc(ctypes.Structure):
    """p2c_relu_stack_desc (include/p2c.h)."""
    _fields_ = [('n_layers', _i32), ('dims', _i32 * (P2C_RELU_STACK_MAX_LAYERS + 1)), ('B', _i32), ('T', _i32), ('flip', _i32),
                ('x', _f32p), ('W', _f32p * P2C_RELU_STACK_MAX_LAYERS), ('b', _f32p * P2C_RELU_STACK_MAX_LAYERS), ('y', _f32p),
                ('gy', _f32p), ('gW', _f32p * P2C_RELU_STACK_MAX_LAYERS), ('gb', _f32p * P2C_RELU_STACK_MAX_LAYERS),
                ('accumulate', _i32), ('workspace', _f32p)]


class PoseChangeLossDesc(ctypes.Structure):
    """p2c_pose_change_loss_desc (include/p2c.h)."""
    _fields_ = [('B', _i64), ('T', _i32), ('J', _i32), ('pred_is_6d', _i32), ('cumulative', _i32), ('mean', _i32),
                ('max_blocks', _i32), ('pred', _f32p), ('target', _f32p), ('workspace', _f32p), ('loss', _f32p),
                ('grad_loss', _f32p), ('grad_pred', _f32p)]


class HeatmapTargetsDesc(ctypes.Structure):
    """p2c_heatmap_targets_desc (include/p2c.h)."""
    _fields_ = [('N', _i64), ('J', _i32), ('H', _i32), ('W', _i32), ('k', _i32), ('s', _i32), ('p', _i32), ('oh', _i32),
                ('ow', _i32), ('n_table', _i32), ('scale_x', ctypes.c_float), ('scale_y', ctypes.c_float), ('kp', _f32p),
                ('shift', _f32p), ('table', _f32p), ('out', _f32p)]


HEATMAPS_MAX_MAPS, HEATMAPS_MAX_TABLE, HEATMAPS_MAX_POOL = 64, 1024, 32


class HeatmapsLossDesc(ctypes.Structure):
    """p2c_heatmaps_loss_desc (include/p2c.h)."""
    _fields_ = [('B', _i64), ('T', _i32), ('Pp', _i32), ('Pg', _i32), ('h', _i32), ('w', _i32), ('K', _i32), ('forced', _i32),
                ('mask', _i32), ('pred_channels', _i32 * HEATMAPS_MAX_MAPS), ('gt_channels', _i32 * HEATMAPS_MAX_MAPS),
                ('pred', _f32p), ('gt', _f32p), ('partials', _f32p), ('flags', _vp), ('coef', _f32p), ('loss', _f32p),
                ('grad_loss', _f32p), ('grad_pred', _f32p)]


class HeatmapKeypointsDesc(ctypes.Structure):
    """p2c_heatmap_keypoints_desc (include/p2c.h)."""
    _fields_ = [('N', _i64), ('P', _i32), ('h', _i32), ('w', _i32), ('sw', ctypes.c_float), ('sh', ctypes.c_float),
                ('maps', _f32p), ('out', _f32p)]


P2C_FRAMES_MAX_CLIPS, P2C_FRAMES_MAX_SIDE = 64, 8192


class ClipFramesClip(ctypes.Structure):
    """p2c_clip_frames_clip (include/p2c.h)."""
    _fields_ = [('offset', _i64), ('H', _i32), ('W', _i32), ('canvas', _i32), ('out_h', _i32), ('out_w', _i32), ('reserved', _i32)]


class ClipFramesDesc(ctypes.Structure):
    """p2c_clip_frames_desc (include/p2c.h)."""
    _fields_ = [('N', _i32), ('T', _i32), ('src_bytes', _i64), ('src', _vp), ('centres', _vp), ('workspace', _vp), ('out', _f32p),
                ('clips', ClipFramesClip * P2C_FRAMES_MAX_CLIPS)]


P2C_RENDER_MAX_PANELS, P2C_RENDER_MAX_PRIMS, P2C_RENDER_MAX_REACH, P2C_RENDER_MAX_SIDE, P2C_RENDER_MAX_COORD = 8, 64, 64, 8192, 16383


class RenderPanel(ctypes.Structure):
    """p2c_render_panel (include/p2c.h)."""
    _fields_ = [('points', _f32p), ('colors', _vp), ('edges', _vp), ('J', _i32), ('E', _i32), ('C', _i32), ('reserved', _i32)]


class RenderPointsDesc(ctypes.Structure):
    """p2c_render_points_desc (include/p2c.h)."""
    _fields_ = [('V', _i32), ('T', _i32), ('H', _i32), ('W', _i32), ('rows', _i32), ('cols', _i32), ('n_panels', _i32),
                ('radius', _i32), ('line_width', _i32), ('max_blocks', _i32), ('out', _vp),
                ('panels', RenderPanel * P2C_RENDER_MAX_PANELS)]


SYMBOLS = {
    'p2c_version': (ctypes.c_char_p, []),
    'p2c_pose_head_workspace_floats': (_i64, [_i32]),
    'p2c_pose_head_set_time_parallel_max_batch': (ctypes.c_int, [ctypes.c_int32]),
    'p2c_pose_head_set_packed_min_batch': (ctypes.c_int, [ctypes.c_int32]),
    'p2c_pose_head_set_chain_min_batch': (ctypes.c_int, [ctypes.c_int32]),
    'p2c_pose_head_fwd': (ctypes.c_int, [ctypes.POINTER(PoseHeadDesc), _vp]),
    'p2c_pose_head_fwd_launch': (ctypes.c_int, [ctypes.POINTER(PoseHeadDesc), ctypes.c_int32, _vp]),
    'p2c_gemm': (ctypes.c_int, [ctypes.POINTER(GemmDesc), _vp]),
    'p2c_debug_poison_lds': (ctypes.c_int, [_vp]),
    'p2c_frame_mean_fwd': (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    'p2c_gemm_tn_workspace_floats': (_i64, [_i32, _i32, _i32]),
    'p2c_gemm_reload_env': (None, []),
    'p2c_gemm_tn': (ctypes.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    'p2c_pose_head_bwd': (ctypes.c_int, [ctypes.POINTER(PoseHeadDesc), ctypes.POINTER(_vp * 3), _vp, _vp, _vp, _vp, _vp]),
    'p2c_normalize_fwd': (ctypes.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _ip, _i32, _ip,
                                         ctypes.c_float, _vp]),
    'p2c_normalize_bwd': (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _ip, _i32, _ip,
                                         ctypes.c_float, _vp]),
    'p2c_loss2d_workspace_floats': (_i64, [_i64]),
    'p2c_loss2d_fwd': (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _ip, _ip, _i32, _i32, _vp, _vp,
                                      _vp, _vp]),
    'p2c_loss2d_bwd': (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _ip, _ip, _i32, _i32, _vp, _vp,
                                      _vp, _vp]),
    'p2c_remap_nodes': (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _ip, _ip, _vp]),
    'p2c_mlp_workspace_floats': (_i64, [ctypes.POINTER(MlpDesc)]),
    'p2c_mlp_saved_floats': (_i64, [ctypes.POINTER(MlpDesc)]),
    'p2c_mlp_image_floats': (_i64, [ctypes.POINTER(MlpDesc)]),
    'p2c_mlp_pack': (ctypes.c_int, [ctypes.POINTER(MlpDesc), _vp]),
    'p2c_mlp_image_index': (_i64, [ctypes.POINTER(MlpDesc), _ip, _i64]),
    'p2c_adamw_step': (ctypes.c_int, [ctypes.POINTER(AdamWDesc), _vp]),
    'p2c_grad_clip_partials': (_i64, [_i64]),
    'p2c_adamw_step_clipped': (ctypes.c_int, [ctypes.POINTER(AdamWDesc), ctypes.POINTER(ClipDesc), _vp]),
    'p2c_collate_fwd': (ctypes.c_int, [ctypes.POINTER(CollateDesc), _vp]),
    'p2c_collate_mixed_fwd': (ctypes.c_int, [ctypes.POINTER(CollateMixedDesc), _vp]),
    'p2c_lstm_rec_fwd': (ctypes.c_int, [ctypes.POINTER(LstmDesc), _vp]),
    'p2c_lstm_rec_bwd': (ctypes.c_int, [ctypes.POINTER(LstmDesc), _vp]),
    'p2c_lstm_steps_workspace_floats': (_i64, [_i32, _i32]),
    'p2c_lstm_steps_fwd': (ctypes.c_int, [ctypes.POINTER(LstmDesc), _vp]),
    'p2c_lstm_steps_bwd': (ctypes.c_int, [ctypes.POINTER(LstmDesc), _vp, _vp]),
    'p2c_gru_steps_workspace_floats': (_i64, [_i32, _i32]),
    'p2c_gru_steps_fwd': (ctypes.c_int, [ctypes.POINTER(GruDesc), _vp]),
    'p2c_gru_steps_bwd': (ctypes.c_int, [ctypes.POINTER(GruDesc), _vp, _vp]),
    'p2c_cls_head': (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    'p2c_rank_workspace_bytes': (_i64, [_i64, _i32, _i32]),
    'p2c_rank_curves': (ctypes.c_int, [ctypes.POINTER(RankDesc), _vp, _vp]),
    'p2c_rank_scores': (ctypes.c_int, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _i64, _i64, _vp]),
    'p2c_bnorm_workspace_floats': (_i64, [_i64, _i32]),
    'p2c_bnorm_fwd': (ctypes.c_int, [ctypes.POINTER(BnormDesc), _vp, _vp]),
    'p2c_bnorm_bwd': (ctypes.c_int, [ctypes.POINTER(BnormDesc), _vp, _vp]),
    'p2c_decoder_fwd': (ctypes.c_int, [ctypes.POINTER(DecoderDesc), _vp]),
    'p2c_decoder_bwd': (ctypes.c_int, [ctypes.POINTER(DecoderDesc), _vp]),
    'p2c_eval_workspace_floats': (_i64, [_i64]),
    'p2c_eval_pose3d': (ctypes.c_int, [_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _ip, _ip, ctypes.c_int32, _ip,
                                       ctypes.c_int32, _vp, _vp, _vp, _vp, _vp]),
    'p2c_eval_pck': (ctypes.c_int, [_vp, _vp, _vp, _i64] + [ctypes.c_int32] * 4 + [_ip] + [ctypes.c_int32] * 3
                     + [_ip, ctypes.c_int32, _ip, ctypes.c_int32, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp]),
    'p2c_eval_fb_workspace_floats': (_i64, [_i64]),
    'p2c_eval_fb': (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    'p2c_embed_workspace_floats': (_i64, [ctypes.c_int32] * 5),
    'p2c_embed_fwd': (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _vp] + [ctypes.c_int32] * 6 + [_vp]),
    'p2c_embed_bwd': (ctypes.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp] + [ctypes.c_int32] * 6 + [_vp]),
    'p2c_fold_fwd': (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp]),
    'p2c_fold_bwd': (ctypes.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, ctypes.c_int32, _vp, _vp, _vp, _vp] + [ctypes.c_int32] * 4 + [_vp]),
    'p2c_atb_workspace_floats': (_i64, [_i64, _i32, _i32, _i32]),
    'p2c_atb': (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _i32, _vp, _vp]),
    'p2c_atb_scaled': (ctypes.c_int, [_vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i64, _vp, _i32, _vp, _i64, _vp, _vp]),
    'p2c_graph_node_counts': (ctypes.c_int, [_vp, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    'p2c_copy_group': (ctypes.c_int, [_vp, _vp, _vp, _i32, _vp]),
    'p2c_layernorm_supported': (ctypes.c_int, [_i32]),
    'p2c_layernorm_workspace_floats': (_i64, [_i64, _i32]),
    'p2c_layernorm_fwd': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, ctypes.c_float, _vp]),
    'p2c_layernorm_bwd': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp]),
    'p2c_attn_small_supported': (ctypes.c_int, [_i32, _i32, _i32]),
    'p2c_attn_small_fwd': (ctypes.c_int, [_vp, _vp, ctypes.c_float, _i32, _i32, _i32, _i32, _vp]),
    'p2c_attn_small_bwd': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_float, _i32, _i32, _i32, _i32, _vp]),
    'p2c_attn_drop_supported': (ctypes.c_int, [_i32, _i32, _i32]),
    'p2c_attn_drop_fwd': (ctypes.c_int, [_vp, _vp, ctypes.c_float, _i32, _i32, _i32, _i32, _vp, ctypes.c_float, _i32, _vp]),
    'p2c_attn_drop_bwd': (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_float, _i32, _i32, _i32, _i32, _vp, ctypes.c_float, _i32, _vp]),
    'p2c_postnorm_supported': (ctypes.c_int, [_i32]),
    'p2c_postnorm_workspace_floats': (_i64, [_i64, _i32]),
    'p2c_postnorm_fwd': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, ctypes.c_float, _vp, ctypes.c_float, _i32,
                                        _vp]),
    'p2c_postnorm_bwd': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _vp,
                                        ctypes.c_float, _i32, _vp]),
    'p2c_atb_group_workspace_floats': (_i64, [ctypes.POINTER(AtbProblem), _i32]),
    'p2c_atb_group': (ctypes.c_int, [ctypes.POINTER(AtbProblem), _i32, _vp, _vp]),
    'p2c_mlp_fwd': (ctypes.c_int, [ctypes.POINTER(MlpDesc), _vp]),
    'p2c_mlp_bwd': (ctypes.c_int, [ctypes.POINTER(MlpDesc), _vp]),
    'p2c_mlp_plan': (ctypes.c_int, [ctypes.POINTER(MlpDesc), _ip]),
    'p2c_train_step_supported': (ctypes.c_int, [ctypes.POINTER(TrainStepDesc)]),
    'p2c_train_step_workspace_floats': (_i64, [ctypes.POINTER(TrainStepDesc)]),
    'p2c_train_step': (ctypes.c_int, [ctypes.POINTER(TrainStepDesc), ctypes.POINTER(_vp * 3), _vp]),
    'p2c_train_step_launch': (ctypes.c_int, [ctypes.POINTER(TrainStepDesc), ctypes.POINTER(_vp * 3), _i32, _vp]),
    'p2c_count_target_pairs': (ctypes.c_int, [ctypes.POINTER(PoseHeadDesc), _vp, _vp]),
    'p2c_train_step_set_stream_min_batch': (ctypes.c_int, [ctypes.c_int32]),
    'p2c_train_step_set_wgrad_stream_min_batch': (ctypes.c_int, [ctypes.c_int32]),
    'p2c_train_step_set_specialized': (ctypes.c_int, [ctypes.c_int32]),
    'p2c_train_step_specialized': (ctypes.c_int, [ctypes.POINTER(TrainStepDesc)]),
    'p2c_relu_stack_supported': (ctypes.c_int, [ctypes.POINTER(ReluStackDesc)]),
    'p2c_relu_stack_workspace_floats': (_i64, [ctypes.POINTER(ReluStackDesc)]),
    'p2c_relu_stack_fwd': (ctypes.c_int, [ctypes.POINTER(ReluStackDesc), _vp]),
    'p2c_relu_stack_bwd': (ctypes.c_int, [ctypes.POINTER(ReluStackDesc), _vp]),
    'p2c_pose_change_loss_workspace_floats': (_i64, [ctypes.POINTER(PoseChangeLossDesc)]),
    'p2c_pose_change_loss_fwd': (ctypes.c_int, [ctypes.POINTER(PoseChangeLossDesc), _vp]),
    'p2c_pose_change_loss_bwd': (ctypes.c_int, [ctypes.POINTER(PoseChangeLossDesc), _vp]),
    'p2c_heatmap_targets_fwd': (ctypes.c_int, [ctypes.POINTER(HeatmapTargetsDesc), _vp]),
    'p2c_heatmaps_loss_fwd': (ctypes.c_int, [ctypes.POINTER(HeatmapsLossDesc), _vp]),
    'p2c_heatmaps_loss_bwd': (ctypes.c_int, [ctypes.POINTER(HeatmapsLossDesc), _vp]),
    'p2c_heatmap_keypoints_fwd': (ctypes.c_int, [ctypes.POINTER(HeatmapKeypointsDesc), _vp]),
    'p2c_carla_pose_fwd': (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    'p2c_carla_pose_inv': (ctypes.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    'p2c_lift_supported': (ctypes.c_int, [ctypes.POINTER(LiftDesc)]),
    'p2c_lift_fwd': (ctypes.c_int, [ctypes.POINTER(LiftDesc), _vp]),
    'p2c_clip_frames_workspace_bytes': (_i64, [_i64]),
    'p2c_clip_frames_fwd': (ctypes.c_int, [ctypes.POINTER(ClipFramesDesc), _vp]),
    'p2c_render_points_supported': (ctypes.c_int, [ctypes.POINTER(RenderPointsDesc)]),
    'p2c_render_points_fwd': (ctypes.c_int, [ctypes.POINTER(RenderPointsDesc), _vp]),
    'p2c_smpl_to_carla_fwd': (ctypes.c_int, [_vp, _vp, _i64] + [_vp] * 10 + [_i64, _i32, _vp]),
    'p2c_loc_to_carla_fwd': (ctypes.c_int, [_vp, _vp, _i64] + [_vp] * 9 + [_i64, _i32, _vp]),
    'p2c_carla_resample_fwd': (ctypes.c_int, [_vp] * 6 + [_i64, _i64, _i32, _i64, _i64, _i64, ctypes.c_double, _i32, _i32, _vp]),
    'p2c_carla_generate_fwd': (ctypes.c_int, [_i64, _i32, _i64, _i64, _i32, _i32] + [ctypes.c_float] * 3 + [_i32, _i32, ctypes.c_float,
                                              _fp, ctypes.c_float, _fp] + [_vp] * 18 + [_i32, _i32, _vp]),
    'p2c_carla_smooth_gauss_fwd': (ctypes.c_int, [_vp] * 5 + [_i64, _i64, _i32, _i64, _i64, _i64, _i64, _i32, _i32, _vp]),
    'p2c_carla_smooth_euro_fwd': (ctypes.c_int, [_vp] * 6 + [_i64, _i64, _i32, _i32] + [ctypes.c_double] * 5 + [_i32, _vp]),
    'p2c_carla_root_motion_tile': (_i32, []),
    'p2c_carla_root_motion_workspace': (_i64, [_i64, _i64, _i32]),
    'p2c_carla_root_motion_fwd': (ctypes.c_int, [_vp] * 9 + [_i64, _i64, _i64, ctypes.c_double, _i32, _i32, _i32, _vp, _vp]),
    'p2c_carla_loop_find_workspace': (_i64, [_i64, _i64, _i32, _i32]),
    'p2c_carla_loop_find_fwd': (ctypes.c_int, [_vp] * 5 + [_i64, _i64, _i32, _i32, _i64, _i64, _i32, _vp, _vp]),
    'p2c_carla_loop_play_fwd': (ctypes.c_int, [_vp] * 5 + [_i64, _i64, _i32, _i64, _i64, _i32, _i32, _vp]),
}

P2C_ROOT_MOTION_MAPPING = {'auto': 0, 'per_video': 1, 'frame_parallel': 2}

P2C_SMOOTH_MAX_RADIUS = 32
P2C_LOOP_MAX_BLEND, P2C_LOOP_MAX_J, P2C_LOOP_MAX_T = 32, 64, 16384

P2C_GENERATE_NOISE = {'zero': 0, 'uniform': 1}
P2C_GENERATE_MAPPING = {'auto': 0, 'sequential': 1, 'frame_parallel': 2}
P2C_GENERATE_MAX_T, P2C_GENERATE_FRAME_PARALLEL_MAX_FRAMES = 65536, 8192

_lib = None


class P2CError(RuntimeError):
    pass


def grad_loss_pointers(g0=None, g1=None, g2=None, vector=None):
    """The ``grad_losses`` argument of p2c_pose_head_bwd: three nullable device pointers (data_ptr ints or None);
    ``vector`` = data_ptr of a contiguous 3-float gradient."""
    if vector is not None:
        g0, g1, g2 = vector, vector + 4, vector + 8
    return ctypes.byref((_vp * 3)(g0, g1, g2))


def build(verbose: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into csrc/libp2c_hip.so (hipcc cross-compiles without a GPU)."""
    res = subprocess.run(['make', '-j', str(min(os.cpu_count() or 1, 8)), '-C', os.path.join(_HERE, 'csrc')], capture_output=True, text=True)
    if verbose or res.returncode:
        print(res.stdout, res.stderr)
    if res.returncode:
        raise P2CError('building libp2c_hip.so failed:\n' + res.stderr)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    """Load the library once (torch first, so its bundled libamdhip64.so.7 is the HIP runtime both sides use)."""
    global _lib
    if _lib is None:
        import torch  # noqa: F401  (side effect: HIP runtime already mapped)
        if not os.path.exists(LIB_PATH):
            raise P2CError(f'{LIB_PATH} is missing: run `python __graft_entry__.py` (build()) or `make -C '
                           f'{os.path.join(_HERE, "csrc")}`. There is no CPU fallback for the HIP hot path.')
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(handle, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        if os.environ.get('P2C_POISON_LDS') == '1':
            handle = _PoisonedLib(handle)
        _lib = handle
    return _lib


class _PoisonedLib:
    """Test audit (P2C_POISON_LDS=1): every launching entry point -- int result, stream as its last argument -- is preceded by
    p2c_debug_poison_lds on that stream, so a kernel that reads LDS it never wrote returns NaN instead of whatever the previous
    workgroup left behind. Run the GPU suite once under it after touching a kernel's LDS layout."""

    def __init__(self, handle):
        self._h = handle
        self._wrap = {n for n, (res, args) in SYMBOLS.items()
                      if res is ctypes.c_int and args and args[-1] is _vp and not n.startswith('p2c_debug')
                      and n not in ('p2c_graph_node_counts',)}

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        if name not in self._wrap:
            return fn
        poison = self._h.p2c_debug_poison_lds

        def call(*a):
            poison(a[-1])
            return fn(*a)
        return call


def check(rc: int, what: str):
    if rc != 0:
        kind = {-1: 'null pointer', -2: 'bad shape', -3: 'bad enum', -4: 'bad index'}.get(rc, f'hipError_t {rc}')
        raise P2CError(f'{what} failed: {kind} (rc={rc})')
