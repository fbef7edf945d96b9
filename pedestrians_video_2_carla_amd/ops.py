"""Device ops of the hot path: thin ``torch.autograd.Function`` shims over the C ABI (include/p2c.h).

PyTorch is plumbing here (device memory, streams, autograd graph); the arithmetic is in csrc/*.hip.
No CPU path: host tensors raise.
"""
import ctypes
import os
import warnings
import weakref
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from pedestrians_video_2_carla_amd import _lib
from pedestrians_video_2_carla_amd._lib import KIND, TRANSFORM, P2C_JOINTS, PoseHeadDesc
from pedestrians_video_2_carla_amd.data.carla import reference as ref

J = P2C_JOINTS

# names of the optional materialised tensors, in the order PoseHeadFunction returns them
OUTPUT_KEYS = ('pose_changes', 'projection_2d', 'projection_2d_transformed', 'projection_2d_shift',
               'projection_2d_scale', 'relative_pose_loc', 'relative_pose_rot', 'absolute_pose_loc',
               'absolute_pose_rot', 'world_loc', 'world_rot')
_DESC_FIELD = {'pose_changes': 'out_pose_changes', 'projection_2d': 'out_projection_2d',
               'projection_2d_transformed': 'out_projection_2d_transformed', 'projection_2d_shift': 'out_shift',
               'projection_2d_scale': 'out_scale', 'relative_pose_loc': 'out_relative_pose_loc',
               'relative_pose_rot': 'out_relative_pose_rot', 'absolute_pose_loc': 'out_absolute_pose_loc',
               'absolute_pose_rot': 'out_absolute_pose_rot', 'world_loc': 'out_world_loc',
               'world_rot': 'out_world_rot'}


def _require_device(t: Tensor, name: str, dtype=torch.float32) -> Tensor:
    if not t.is_cuda:
        raise _lib.P2CError(f'{name} must live on the GPU: the pose-head hot path has no CPU implementation')
    if t.dtype != dtype:
        t = t.to(dtype)
    return t.contiguous()


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


@dataclass(frozen=True)
class PoseHeadSpec:
    """Static configuration of one flow (everything that does not change from batch to batch)."""
    kind: str = 'pose_changes_6d'                 # key of _lib.KIND
    transform: str = 'hips_neck_bbox'             # key of _lib.TRANSFORM
    mask_missing_joints: bool = True
    hips_idx: Tuple[int, ...] = (1,)              # shift point joints of the normaliser (in the 26-joint output)
    neck_idx: Tuple[int, ...] = (8,)
    gmap2d: Tuple[int, ...] = tuple(range(J))     # predicted joint -> gt joint, -1 = not common
    gmap3d: Tuple[int, ...] = tuple(range(J))
    hips_lane: int = 1                            # predicted joint that is never masked, -1 = none
    eval_slice: Tuple[Optional[int], Optional[int]] = (None, None)
    world_absolute: bool = False                  # trajectory output type loc_rot: dloc/drot are absolute per frame
    near_zero: float = 1e-5
    camera: Tuple[float, float, float, float, float] = (ref.CAMERA['f'], ref.CAMERA['cx'], ref.CAMERA['cy'],
                                                        ref.CAMERA['dist'], ref.CAMERA['elev'])

    def frames(self, T: int) -> Tuple[int, int]:
        t0, t1, _ = slice(*self.eval_slice).indices(T)
        return t0, max(t0, t1)


def joint_maps(out_idx, in_idx, n_gt_joints: int = J) -> Tuple[int, ...]:
    """(output_indices, input_indices) of ``get_common_indices`` -> per-predicted-joint gt index table."""
    if isinstance(out_idx, slice):
        return tuple(j if j < n_gt_joints else -1 for j in range(J))
    table = [-1] * J
    for o, i in zip(out_idx, in_idx):
        table[o] = i
    return tuple(table)


def _fill_desc(spec: PoseHeadSpec, y: Tensor, skel_type: Tensor, dloc, drot, gt2d, gt3d, bufs: Dict[str, Tensor],
               outs: Dict[str, Tensor], gt_rot: Optional[Tensor] = None, grad_rot: Optional[Tensor] = None) -> PoseHeadDesc:
    B, T = y.shape[0], y.shape[1]
    d = PoseHeadDesc()
    d.B, d.T = B, T
    d.kind, d.transform = KIND[spec.kind], TRANSFORM[spec.transform]
    d.t0, d.t1 = spec.frames(T)
    d.mask_missing_joints = int(spec.mask_missing_joints)
    d.hips_lane = spec.hips_lane
    d.n_hips, d.n_neck = len(spec.hips_idx), len(spec.neck_idx)
    for i, v in enumerate(spec.hips_idx):
        d.hips_idx[i] = v
    for i, v in enumerate(spec.neck_idx):
        d.neck_idx[i] = v
    d.gmap2d[:] = spec.gmap2d
    d.gmap3d[:] = spec.gmap3d
    d.n_common2d = sum(1 for v in spec.gmap2d if v >= 0)
    d.n_common3d = sum(1 for v in spec.gmap3d if v >= 0)
    d.world_absolute = int(spec.world_absolute)
    d.cam_f, d.cam_cx, d.cam_cy, d.cam_dist, d.cam_elev = spec.camera
    d.near_zero = spec.near_zero
    dev = y.device
    d.y, d.skel_type = y.data_ptr(), skel_type.data_ptr()
    if spec.kind == 'absolute_loc':
        shift, scale = ref.get_hips_neck_tables(dev)
        d.ref_hn_shift, d.ref_hn_scale = shift.data_ptr(), scale.data_ptr()
    else:
        loc, rot = ref.get_relative_tensors(dev)
        d.ref_rel_loc, d.ref_rel_rot = loc.data_ptr(), rot.data_ptr()
    d.dloc, d.drot = _ptr(dloc), _ptr(drot)
    if gt2d is not None:
        d.gt2d, d.gt2d_joints, d.gt2d_channels = gt2d.data_ptr(), gt2d.shape[-2], gt2d.shape[-1]
    if gt3d is not None:
        d.gt3d, d.gt3d_joints = gt3d.data_ptr(), gt3d.shape[-2]
    if gt_rot is not None:                       # rot_3d fused: the 3-D joint map applies (loss/rot_3d.py:31-35)
        d.gt_rot, d.gt3d_joints = gt_rot.data_ptr(), gt_rot.shape[-3]
        d.grad_loss_rot = _ptr(grad_rot)
    d.partials, d.loss_sums, d.losses = (bufs[k].data_ptr() for k in ('partials', 'loss_sums', 'losses'))
    d.final_rel_rot = _ptr(bufs.get('final_rel_rot'))
    for k, t in outs.items():
        setattr(d, _DESC_FIELD[k], t.data_ptr())
    return d


def _check_shapes(spec: PoseHeadSpec, y, skel_type, dloc, drot, gt2d, gt3d):
    B, T = y.shape[0], y.shape[1]
    want = {'pose_changes_6d': (B, T, J, 6), 'relative_rot_6d': (B, T, J, 6), 'pose_changes': (B, T, J, 3, 3),
            'relative_rot': (B, T, J, 3, 3), 'absolute_loc': (B, T, J, 3)}[spec.kind]
    if tuple(y.shape) != want:
        # same wording as the reference's rank checks (modules/layers/projection.py:90-98)
        raise RuntimeError(f'{spec.kind} input should have shape {want}, got {tuple(y.shape)}')
    if tuple(skel_type.shape) != (B,):
        raise RuntimeError(f'skel_type should have shape ({B},), got {tuple(skel_type.shape)}')
    if dloc is not None and tuple(dloc.shape) != (B, T, 3):
        raise RuntimeError(f'world_loc_change_batch should have shape {(B, T, 3)}, got {tuple(dloc.shape)}')
    if drot is not None and tuple(drot.shape) != (B, T, 3, 3):
        raise RuntimeError(f'world_rot_change_batch should have shape {(B, T, 3, 3)}, got {tuple(drot.shape)}')
    for name, g, c, gm in (('gt2d', gt2d, 2, spec.gmap2d), ('gt3d', gt3d, 3, spec.gmap3d)):
        if g is None:
            continue
        if g.ndim != 4 or g.shape[0] != B or g.shape[1] != T or g.shape[3] < c or (name == 'gt3d' and g.shape[3] != 3):
            raise RuntimeError(f'{name} should have shape ({B}, {T}, joints, {c}), got {tuple(g.shape)}')
        if max(gm) >= g.shape[2]:
            raise RuntimeError(f'{name} has {g.shape[2]} joints but the joint map needs index {max(gm)}')


_OUT_SHAPES = {'pose_changes': (J, 3, 3), 'projection_2d': (J, 3), 'projection_2d_transformed': (J, 3),
               'projection_2d_shift': (2,), 'projection_2d_scale': (), 'relative_pose_loc': (J, 3),
               'relative_pose_rot': (J, 3, 3), 'absolute_pose_loc': (J, 3), 'absolute_pose_rot': (J, 3, 3),
               'world_loc': (3,), 'world_rot': (3, 3)}


def available_outputs(spec: PoseHeadSpec, world: bool) -> Tuple[str, ...]:
    keys = ['projection_2d', 'absolute_pose_loc']
    if spec.transform != 'none':
        keys += ['projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale']
    if spec.kind != 'absolute_loc':
        keys += ['relative_pose_loc', 'relative_pose_rot', 'absolute_pose_rot']
    if spec.kind in ('pose_changes_6d', 'pose_changes'):
        keys += ['pose_changes']
    if world:
        keys += ['world_loc', 'world_rot']
    return tuple(keys)


class PoseLosses:
    """(loc_2d, loc_3d, loc_2d_3d [, rot_3d when ``gt_rot`` was given]) of one fused pose-head call.

    ``losses[i]`` / ``losses.loc_2d_3d`` are 0-dim tensors that are outputs of the autograd node themselves: calling
    ``backward`` on one of them reaches the HIP backward without any select/scatter kernel in between. ``losses.vector``
    is the same three numbers as one (3,) tensor (also differentiable)."""
    names = ('loc_2d', 'loc_3d', 'loc_2d_3d')

    def __init__(self, vector: Tensor, scalars: Sequence[Tensor], rot_3d: Optional[Tensor] = None):
        self.vector = vector
        self.scalars = tuple(scalars)
        self.rot_3d = rot_3d

    def __getitem__(self, i):
        return self.scalars[self.names.index(i)] if isinstance(i, str) else self.scalars[i]

    def __len__(self):
        return 3

    def __iter__(self):
        return iter(self.scalars)

    loc_2d = property(lambda self: self.scalars[0])
    loc_3d = property(lambda self: self.scalars[1])
    loc_2d_3d = property(lambda self: self.scalars[2])


_DEFER_LOSS_FINALIZE = 0


class deferred_loss_finalize:
    """Context manager for a train step whose backward is GUARANTEED to follow the forward before anyone reads the loss
    values (the trainer's step). mode 1: the lean pose-head forward skips its one-workgroup finalize launch and the backward
    kernel finishes the loss reduction. mode 2 (default): the forward call only counts the unmasked target pairs and the
    backward kernel -- which recomputes the pose head anyway -- produces the losses as well as grad_y: the training step
    runs the pose head ONCE (p2c_pose_head_desc.defer_loss_finalize). Outside of the context nothing changes."""

    def __init__(self, mode: int = 2):
        self.mode = mode

    def __enter__(self):
        global _DEFER_LOSS_FINALIZE
        self._prev, _DEFER_LOSS_FINALIZE = _DEFER_LOSS_FINALIZE, self.mode
        return self

    def __exit__(self, *exc):
        global _DEFER_LOSS_FINALIZE
        _DEFER_LOSS_FINALIZE = self._prev
        return False


class PoseHeadFunction(torch.autograd.Function):
    """(losses (3,), loc_2d, loc_3d, loc_2d_3d [, materialised tensors]) = f(model output y)."""

    @staticmethod
    def forward(ctx, y, spec: PoseHeadSpec, skel_type, dloc, drot, gt2d, gt3d, want: Tuple[str, ...], gt_rot=None):
        lib = _lib.lib()
        y = _require_device(y, 'pose_inputs')
        skel_type = _require_device(skel_type, 'skel_type', torch.int32)
        dloc = None if dloc is None else _require_device(dloc, 'world_loc_change_batch')
        drot = None if drot is None else _require_device(drot, 'world_rot_change_batch')
        gt2d = None if gt2d is None else _require_device(gt2d, 'gt2d')
        gt3d = None if gt3d is None else _require_device(gt3d, 'gt3d')
        _check_shapes(spec, y, skel_type, dloc, drot, gt2d, gt3d)
        B, T = y.shape[0], y.shape[1]
        if gt_rot is not None:
            gt_rot = _require_device(gt_rot, 'gt_rot')
            if spec.kind not in ('pose_changes_6d', 'relative_rot_6d'):
                raise RuntimeError('rot_3d is fused for the 6-D kinds only')
            if gt_rot.ndim != 5 or tuple(gt_rot.shape[:2]) != (B, T) or tuple(gt_rot.shape[3:]) != (3, 3) \
                    or max(spec.gmap3d) >= gt_rot.shape[2] or (gt3d is not None and gt3d.shape[2] != gt_rot.shape[2]):
                raise RuntimeError(f'gt_rot should have shape ({B}, {T}, joints, 3, 3), got {tuple(gt_rot.shape)}')
        dev = y.device
        f32 = dict(dtype=torch.float32, device=dev)
        losses4 = torch.empty(4, **f32)             # loc_2d, loc_3d, loc_2d_3d | rot_3d (written when gt_rot is given)
        bufs = {
            'partials': torch.empty(lib.p2c_pose_head_workspace_floats(B), **f32),
            'loss_sums': torch.empty(6, **f32),
            'losses': losses4,
        }
        if spec.kind in ('pose_changes_6d', 'pose_changes'):
            bufs['final_rel_rot'] = torch.empty(B, J, 3, 3, **f32)
        t0, t1 = spec.frames(T)
        outs = {}
        for k in want:
            full = torch.zeros if (k.startswith('projection_2d_') and (t0, t1) != (0, T)) else torch.empty
            outs[k] = full((B, T) + _OUT_SHAPES[k], **f32)
        desc = _fill_desc(spec, y, skel_type, dloc, drot, gt2d, gt3d, bufs, outs, gt_rot)
        # lean training forward inside deferred_loss_finalize(): the backward publishes the loss values
        ctx.deferred = (_DEFER_LOSS_FINALIZE if (not want and ctx.needs_input_grad[0] and gt_rot is None
                                                 and spec.kind in ('pose_changes_6d', 'relative_rot_6d')) else 0)
        desc.defer_loss_finalize = int(ctx.deferred)
        with torch.cuda.device(dev):
            _lib.check(lib.p2c_pose_head_fwd(ctypes.byref(desc), _stream()), 'p2c_pose_head_fwd')
        ctx.spec, ctx.want = spec, want
        ctx.save_for_backward(y, skel_type, dloc, drot, gt2d, gt3d, bufs['loss_sums'], bufs.get('final_rel_rot'), gt_rot)
        ctx.bufs = bufs
        result = [outs[k] for k in want]
        rot_diff = spec.kind in ('pose_changes_6d', 'relative_rot_6d')      # rot_3d-type losses: tangent-space backward
        nondiff = [outs[k] for k in want if k not in ('absolute_pose_loc', 'projection_2d_transformed')
                   and not (k == 'projection_2d' and spec.transform == 'none')
                   and not (k == 'absolute_pose_rot' and rot_diff)]
        ctx.mark_non_differentiable(*nondiff)
        ctx.set_materialize_grads(False)
        vec = losses4[:3]
        return (vec, vec[0], vec[1], vec[2], losses4[3], *result)       # views of one buffer: no device work

    @staticmethod
    def backward(ctx, g_losses, g0, g1, g2, g_rot3d, *g_outs):
        lib = _lib.lib()
        spec = ctx.spec
        y, skel_type, dloc, drot, gt2d, gt3d, loss_sums, final_rel_rot, gt_rot = ctx.saved_tensors
        bufs = dict(ctx.bufs)
        bufs['loss_sums'] = loss_sums
        if final_rel_rot is not None:
            bufs['final_rel_rot'] = final_rel_rot
        g_abs = g_projt = g_rot = None
        for k, g in zip(ctx.want, g_outs):
            if g is None:
                continue
            if k == 'absolute_pose_loc':
                g_abs = _require_device(g, 'grad absolute_pose_loc')
            elif k == 'absolute_pose_rot':
                g_rot = _require_device(g, 'grad absolute_pose_rot')
            elif k == 'projection_2d_transformed' or (k == 'projection_2d' and spec.transform == 'none'):
                g_projt = _require_device(g, 'grad ' + k)
        scalars = [None if g is None else _require_device(g, 'grad loss') for g in (g0, g1, g2)]
        if g_losses is not None:                      # gradient w.r.t. the (3,) vector output
            g_losses = _require_device(g_losses, 'grad losses')
            if any(g is not None for g in scalars):   # both forms used at once (rare): fold the scalars into the vector
                g_losses = g_losses + torch.stack([torch.zeros_like(g_losses[0]) if g is None else g for g in scalars])
            gl = _lib.grad_loss_pointers(vector=g_losses.data_ptr())
        else:
            gl = _lib.grad_loss_pointers(*[_ptr(g) for g in scalars])
        g_rot3d = None if (g_rot3d is None or gt_rot is None) else _require_device(g_rot3d, 'grad rot_3d')
        desc = _fill_desc(spec, y, skel_type, dloc, drot, gt2d, gt3d, bufs, {}, gt_rot, g_rot3d)
        desc.defer_loss_finalize = int(ctx.deferred)
        grad_y = torch.empty_like(y)
        with torch.cuda.device(y.device):
            _lib.check(lib.p2c_pose_head_bwd(ctypes.byref(desc), gl, _ptr(g_abs), _ptr(g_projt), _ptr(g_rot),
                                             grad_y.data_ptr(), _stream()), 'p2c_pose_head_bwd')
        return grad_y, None, None, None, None, None, None, None, None


def pose_head(y: Tensor, spec: PoseHeadSpec, skel_type: Tensor, dloc: Optional[Tensor] = None,
              drot: Optional[Tensor] = None, gt2d: Optional[Tensor] = None, gt3d: Optional[Tensor] = None,
              want: Sequence[str] = (), gt_rot: Optional[Tensor] = None) -> Tuple[Tensor, Dict[str, Tensor]]:
    """Fused pose head. Returns (PoseLosses, {name: materialised tensor for name in want}). ``gt_rot`` =
    targets['absolute_pose_rot']: the rot_3d loss (loss/rot_3d.py:9-37) comes out of the same launches (``losses.rot_3d``) --
    the target rotations are read, no rotation tensor is written (6-D kinds)."""
    want = tuple(want)
    res = PoseHeadFunction.apply(y, spec, skel_type, dloc, drot, gt2d, gt3d, want, gt_rot)
    return PoseLosses(res[0], res[1:4], res[4] if gt_rot is not None else None), dict(zip(want, res[5:]))


# ----------------------------------------------------------------------------------------------------------------------
# stand-alone normaliser (K4), masked 2-D MSE (K3), joint remap (K5)
# ----------------------------------------------------------------------------------------------------------------------
def _iarr(values: Sequence[int]):
    return (ctypes.c_int32 * max(1, len(values)))(*values)


class NormalizeFunction(torch.autograd.Function):
    """Normalizer.__call__ on device: (out, shift, scale) = f(x); only ``out`` carries gradient (as in the reference,
    where shift/scale are read back detached by the dataset, projection_2d_mixin.py:229-230)."""

    @staticmethod
    def forward(ctx, x, transform: str, dim: int, hips_idx, neck_idx, near_zero: float):
        lib = _lib.lib()
        x = _require_device(x, 'sample')
        if x.ndim < 2 or x.shape[-1] < dim:
            raise RuntimeError(f'sample should be (..., joints, >= {dim}), got {tuple(x.shape)}')
        Jn, C = x.shape[-2], x.shape[-1]
        N = x.numel() // (Jn * C)
        out = torch.empty_like(x)
        shift = torch.empty(x.shape[:-2] + (dim,), dtype=torch.float32, device=x.device)
        scale = torch.empty(x.shape[:-2], dtype=torch.float32, device=x.device)
        h, k = _iarr(hips_idx), _iarr(neck_idx)
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_normalize_fwd(x.data_ptr(), out.data_ptr(), shift.data_ptr(), scale.data_ptr(), N, Jn, C,
                                             dim, TRANSFORM[transform], len(hips_idx), h, len(neck_idx), k, near_zero,
                                             _stream()), 'p2c_normalize_fwd')
        ctx.save_for_backward(x)
        ctx.cfg = (transform, dim, tuple(hips_idx), tuple(neck_idx), near_zero)
        ctx.mark_non_differentiable(shift, scale)
        return out, shift, scale

    @staticmethod
    def backward(ctx, g_out, g_shift, g_scale):
        lib = _lib.lib()
        (x,) = ctx.saved_tensors
        transform, dim, hips_idx, neck_idx, near_zero = ctx.cfg
        g_out = _require_device(g_out, 'grad')
        Jn, C = x.shape[-2], x.shape[-1]
        N = x.numel() // (Jn * C)
        gx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_normalize_bwd(x.data_ptr(), g_out.data_ptr(), gx.data_ptr(), N, Jn, C, dim,
                                             TRANSFORM[transform], len(hips_idx), _iarr(hips_idx), len(neck_idx),
                                             _iarr(neck_idx), near_zero, _stream()), 'p2c_normalize_bwd')
        return gx, None, None, None, None, None


def normalize(x: Tensor, transform: str, dim: int = 2, hips_idx: Sequence[int] = (1,), neck_idx: Sequence[int] = (8,),
              near_zero: float = 1e-5) -> Tuple[Tensor, Tensor, Tensor]:
    return NormalizeFunction.apply(x, transform, dim, tuple(hips_idx), tuple(neck_idx), near_zero)


class Loss2DFunction(torch.autograd.Function):
    """Loc2DPoseLoss on device: masked MSE over the common joints of pred (...,Jp,>=2) and gt (...,Jg,>=2)."""

    @staticmethod
    def forward(ctx, pred, gt, pred_idx, gt_idx, hips_col: int, mask_missing_joints: bool):
        lib = _lib.lib()
        pred, gt = _require_device(pred, 'prediction'), _require_device(gt, 'target')
        if pred.shape[:-2] != gt.shape[:-2]:
            raise RuntimeError(f'prediction {tuple(pred.shape)} and target {tuple(gt.shape)} differ in leading dims')
        Jp, Cp, Jg, Cg = pred.shape[-2], pred.shape[-1], gt.shape[-2], gt.shape[-1]
        N = pred.numel() // (Jp * Cp)
        f32 = dict(dtype=torch.float32, device=pred.device)
        partials = torch.empty(lib.p2c_loss2d_workspace_floats(N), **f32)
        sums, loss = torch.empty(2, **f32), torch.empty(1, **f32)
        with torch.cuda.device(pred.device):
            _lib.check(lib.p2c_loss2d_fwd(pred.data_ptr(), gt.data_ptr(), N, Jp, Cp, Jg, Cg, len(pred_idx),
                                          _iarr(pred_idx), _iarr(gt_idx), hips_col, int(mask_missing_joints),
                                          partials.data_ptr(), sums.data_ptr(), loss.data_ptr(), _stream()),
                       'p2c_loss2d_fwd')
        ctx.save_for_backward(pred, gt, sums)
        ctx.cfg = (tuple(pred_idx), tuple(gt_idx), hips_col, bool(mask_missing_joints))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        lib = _lib.lib()
        pred, gt, sums = ctx.saved_tensors
        pred_idx, gt_idx, hips_col, mask = ctx.cfg
        Jp, Cp, Jg, Cg = pred.shape[-2], pred.shape[-1], gt.shape[-2], gt.shape[-1]
        N = pred.numel() // (Jp * Cp)
        g_loss = _require_device(g_loss, 'grad').reshape(1)
        gp = torch.empty_like(pred)
        with torch.cuda.device(pred.device):
            _lib.check(lib.p2c_loss2d_bwd(pred.data_ptr(), gt.data_ptr(), N, Jp, Cp, Jg, Cg, len(pred_idx),
                                          _iarr(pred_idx), _iarr(gt_idx), hips_col, int(mask), sums.data_ptr(),
                                          g_loss.data_ptr(), gp.data_ptr(), _stream()), 'p2c_loss2d_bwd')
        return gp, None, None, None, None, None


def loss_loc_2d(pred: Tensor, gt: Tensor, pred_idx: Sequence[int], gt_idx: Sequence[int], hips_col: int = -1,
                mask_missing_joints: bool = True) -> Tensor:
    return Loss2DFunction.apply(pred, gt, tuple(pred_idx), tuple(gt_idx), hips_col, mask_missing_joints)


def remap_nodes(src: Tensor, n_dst_joints: int, src_idx: Sequence[int], dst_idx: Sequence[int]) -> Tensor:
    """BaseDataset._get_common_tensor on device: (N.., Jsrc, C) -> (N.., Jdst, C), unmapped joints zero."""
    lib = _lib.lib()
    src = _require_device(src, 'data_item')
    Js, C = src.shape[-2], src.shape[-1]
    N = src.numel() // (Js * C)
    dst = torch.empty(src.shape[:-2] + (n_dst_joints, C), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(lib.p2c_remap_nodes(src.data_ptr(), dst.data_ptr(), N, Js, n_dst_joints, C, len(src_idx),
                                       _iarr(src_idx), _iarr(dst_idx), _stream()), 'p2c_remap_nodes')
    return dst


# ----------------------------------------------------------------------------------------------------------------------
# dataset-side input pipeline (K11)
# ----------------------------------------------------------------------------------------------------------------------
def collate(raw: Tensor, *, flip_perm: Optional[Sequence[int]] = None, is_flipped: Optional[Tensor] = None,
            rotation: Optional[Tensor] = None, bboxes: Optional[Tensor] = None, clip_size: Optional[Tensor] = None,
            noise: Optional[Tensor] = None, miss_u: Optional[Tensor] = None,
            miss_prob: Optional[Sequence[float]] = None, transform: str = 'hips_neck_bbox',
            hips_idx: Sequence[int] = (1,), neck_idx: Sequence[int] = (8,), near_zero: float = 1e-5,
            return_confidence: bool = False, src_idx: Optional[Sequence[int]] = None,
            dst_idx: Optional[Sequence[int]] = None, n_input_joints: Optional[int] = None
            ) -> Tuple[Tensor, Dict[str, Tensor]]:
    """``BaseDataset.__getitem__`` for a whole batch in one launch (p2c_collate_fwd): augmentation (flip / rotation with
    the given per-clip draws), deformation (given noise / missing-joint draws), both normalisations, confidence handling
    and the node map. raw (N,T,Jd,2|3) -> (frames (N,T,Ji,2|3), targets) with the reference's target keys
    (projection_2d_mixin.py:209-232, augment_pose.py:62-76)."""
    from pedestrians_video_2_carla_amd._lib import CollateDesc
    lib = _lib.lib()
    raw = _require_device(raw, 'projection_2d')
    if raw.ndim != 4 or raw.shape[-1] not in (2, 3):
        raise RuntimeError(f'projection_2d must be (N,T,J,2|3), got {tuple(raw.shape)}')
    N, T, Jd, C = raw.shape
    if return_confidence and C == 2:      # confidence_mixin.py:17-18 (torch.cat of a 3-D and a 2-D tensor)
        raise RuntimeError('Tensors must have same number of dimensions: got 3 and 2')
    if rotation is not None and bboxes is None and C != 2:   # random_rotation.py:50 (centres of a 3-channel box)
        raise RuntimeError('The size of tensor a (2) must match the size of tensor b (3) at non-singleton dimension 3')
    Ji = n_input_joints if n_input_joints is not None else Jd
    f32 = dict(dtype=torch.float32, device=raw.device)
    d = CollateDesc()
    d.N, d.T, d.Jd, d.C, d.raw = N, T, Jd, C, raw.data_ptr()
    keep = [raw]

    def dev(t, shape, name, dtype=torch.float32):
        t = _require_device(t, name) if dtype == torch.float32 else t.to(device=raw.device, dtype=dtype).contiguous()
        if tuple(t.shape) != shape:
            raise RuntimeError(f'{name} must be {shape}, got {tuple(t.shape)}')
        keep.append(t)
        return t.data_ptr()

    targets: Dict[str, Tensor] = {}
    if is_flipped is not None:
        if flip_perm is None:
            raise RuntimeError('is_flipped needs the flip mask of the data skeleton')
        d.is_flipped = dev(is_flipped, (N,), 'is_flipped', torch.uint8)
        perm = _iarr(flip_perm)
        d.flip_perm = perm
        targets['is_flipped'] = is_flipped
    if rotation is not None:
        d.rotation_deg = dev(rotation, (N,), 'rotation')
        targets['rotation'] = rotation
    augmented = is_flipped is not None or rotation is not None
    if bboxes is not None and augmented:
        d.bboxes = dev(bboxes, (N, T, 2, 2), 'bboxes')
        targets['bboxes'] = torch.empty(N, T, 2, 2, **f32)
        targets['orig_bboxes'] = bboxes
        d.bboxes_out = targets['bboxes'].data_ptr()
    if clip_size is not None and augmented:
        d.clip_size = dev(clip_size, (N, 2), 'clip_size')
    if noise is not None:
        d.noise = dev(noise, (N, T, Jd, 2), 'noise')
    if miss_u is not None:
        d.miss_u = dev(miss_u, (N, T, Jd), 'miss_u')
        probs = (ctypes.c_float * Jd)(*[float(v) for v in miss_prob])
        d.miss_prob = probs
    d.transform = TRANSFORM[transform]
    d.n_hips, d.n_neck = len(hips_idx), len(neck_idx)
    for i, v in enumerate(hips_idx):
        d.hips_idx[i] = v
    for i, v in enumerate(neck_idx):
        d.neck_idx[i] = v
    d.near_zero, d.return_confidence, d.Ji = near_zero, int(return_confidence), Ji
    if src_idx is not None:
        d.K = len(src_idx)
        si, di = _iarr(src_idx), _iarr(dst_idx)
        d.src_idx, d.dst_idx = si, di
    frames = torch.empty(N, T, Ji, C if return_confidence else 2, **f32)
    targets['projection_2d'] = torch.empty(N, T, Ji, 2, **f32)
    d.frames, d.t_projection_2d = frames.data_ptr(), targets['projection_2d'].data_ptr()
    if noise is not None or miss_u is not None:
        targets['projection_2d_deformed'] = torch.empty(N, T, Ji, 2, **f32)
        d.t_deformed = targets['projection_2d_deformed'].data_ptr()
    if transform != 'none':
        targets['projection_2d_transformed'] = torch.empty(N, T, Ji, 2, **f32)
        targets['projection_2d_shift'] = torch.empty(N, T, 2, **f32)
        targets['projection_2d_scale'] = torch.empty(N, T, **f32)
        d.t_transformed, d.shift = targets['projection_2d_transformed'].data_ptr(), targets['projection_2d_shift'].data_ptr()
        d.scale = targets['projection_2d_scale'].data_ptr()
    with torch.cuda.device(raw.device):
        _lib.check(lib.p2c_collate_fwd(ctypes.byref(d), _stream()), 'p2c_collate_fwd')
    return frames, targets


@dataclass
class MixedSource:
    """One source of ``collate_mixed``: its stored clips and what K11 would be told about them."""
    raw: Tensor                                       # (n,T,Jd,2|3) on the device
    flip_perm: Optional[Sequence[int]] = None         # flip mask of the data skeleton (needed with is_flipped)
    miss_prob: Optional[Sequence[float]] = None       # per data joint; clips of this source read miss_u when given
    transform: str = 'hips_neck_bbox'
    hips_idx: Sequence[int] = (1,)
    neck_idx: Sequence[int] = (8,)
    src_idx: Optional[Sequence[int]] = None           # node map onto the model-input skeleton (None: same skeleton)
    dst_idx: Optional[Sequence[int]] = None
    has_noise: bool = False                           # clips of this source add ``noise``
    has_bboxes: bool = False                          # clips of this source take their boxes from ``bboxes``


def check_mixed_index(source, row, counts: Sequence[int]) -> None:
    """Host-side check of a batch's (source, row) pairs, for the code that builds them (numpy arrays or CPU tensors):
    the kernel clamps what is out of range instead of following it, which keeps memory safe but hides the mistake."""
    import numpy as np
    source, row = np.asarray(source), np.asarray(row)
    if source.shape != row.shape or source.ndim != 1:
        raise RuntimeError(f'source and row must be (N,), got {source.shape} and {row.shape}')
    if source.size == 0:
        return
    if source.min() < 0 or source.max() >= len(counts):
        raise RuntimeError(f'source index outside [0, {len(counts)})')
    limit = np.asarray(counts, dtype=np.int64)[source]
    if (row < 0).any() or (row >= limit).any():
        bad = int(np.flatnonzero((row < 0) | (row >= limit))[0])
        raise RuntimeError(f'row {int(row[bad])} of batch clip {bad} is outside source {int(source[bad])} '
                           f'({int(limit[bad])} clips)')


def collate_mixed(sources: Sequence[MixedSource], source: Tensor, row: Tensor, *, is_flipped: Optional[Tensor] = None,
                  rotation: Optional[Tensor] = None, bboxes: Optional[Tensor] = None,
                  clip_size: Optional[Tensor] = None, noise: Optional[Tensor] = None, miss_u: Optional[Tensor] = None,
                  near_zero: float = 1e-5, return_confidence: bool = False, n_input_joints: Optional[int] = None
                  ) -> Tuple[Tensor, Dict[str, Tensor]]:
    """``collate`` for a batch whose clips come from several data skeletons, in one launch (p2c_collate_mixed_fwd): clip n
    is ``sources[source[n]].raw[row[n]]`` and is processed exactly as ``collate`` would process it with that source's
    settings. The draws are indexed by batch position; noise (N,T,Jmax,2) and miss_u (N,T,Jmax) have Jmax = the largest
    source skeleton. ``source`` (uint8) and ``row`` (int32) are device tensors that the caller has checked where it built
    them (``check_mixed_index``); the kernel clamps, it does not report. Returns (frames, targets) with ``collate``'s keys;
    every element of every output is written for every clip."""
    from pedestrians_video_2_carla_amd._lib import CollateMixedDesc, P2C_COLLATE_MAX_SOURCES
    lib = _lib.lib()
    S = len(sources)
    if not 1 <= S <= P2C_COLLATE_MAX_SOURCES:
        raise RuntimeError(f'collate_mixed takes 1..{P2C_COLLATE_MAX_SOURCES} sources, got {S}')
    raws = [_require_device(q.raw, 'projection_2d') for q in sources]
    device = raws[0].device
    for r in raws:
        if r.ndim != 4 or r.shape[-1] not in (2, 3) or r.shape[1] != raws[0].shape[1]:
            raise RuntimeError(f'every source must be (n,T,J,2|3) with one T, got {[tuple(x.shape) for x in raws]}')
    T, Jmax = raws[0].shape[1], max(r.shape[2] for r in raws)
    if return_confidence and any(r.shape[-1] == 2 for r in raws):      # confidence_mixin.py:17-18
        raise RuntimeError('Tensors must have same number of dimensions: got 3 and 2')
    if rotation is not None and any(r.shape[-1] != 2 and not q.has_bboxes for r, q in zip(raws, sources)):
        raise RuntimeError('The size of tensor a (2) must match the size of tensor b (3) at non-singleton dimension 3')
    if not source.is_cuda or not row.is_cuda:
        raise _lib.P2CError('source and row must live on the GPU: check them on the host with check_mixed_index first')
    source = source.to(torch.uint8).contiguous()
    row = row.to(torch.int32).contiguous()
    N = source.shape[0]
    if source.ndim != 1 or tuple(row.shape) != (N,):
        raise RuntimeError(f'source and row must be (N,), got {tuple(source.shape)} and {tuple(row.shape)}')
    Ji = n_input_joints if n_input_joints is not None else raws[0].shape[2]
    f32 = dict(dtype=torch.float32, device=device)
    d = CollateMixedDesc()
    d.N, d.T, d.Ji, d.S, d.return_confidence, d.near_zero = N, T, Ji, S, int(return_confidence), near_zero
    d.source, d.row = source.data_ptr(), row.data_ptr()
    keep = [raws, source, row]

    def dev(t, shape, name, dtype=torch.float32):
        t = _require_device(t, name) if dtype == torch.float32 else t.to(device=device, dtype=dtype).contiguous()
        if tuple(t.shape) != shape:
            raise RuntimeError(f'{name} must be {shape}, got {tuple(t.shape)}')
        keep.append(t)
        return t.data_ptr()

    targets: Dict[str, Tensor] = {}
    if is_flipped is not None:
        if any(q.flip_perm is None for q in sources):
            raise RuntimeError('is_flipped needs the flip mask of every data skeleton')
        d.is_flipped = dev(is_flipped, (N,), 'is_flipped', torch.uint8)
        targets['is_flipped'] = is_flipped
    if rotation is not None:
        d.rotation_deg = dev(rotation, (N,), 'rotation')
        targets['rotation'] = rotation
    augmented = is_flipped is not None or rotation is not None
    with_boxes = bboxes is not None and augmented
    if with_boxes:
        d.bboxes = dev(bboxes, (N, T, 2, 2), 'bboxes')
        targets['bboxes'] = torch.empty(N, T, 2, 2, **f32)
        targets['orig_bboxes'] = bboxes
        d.bboxes_out = targets['bboxes'].data_ptr()
    if clip_size is not None and augmented:
        d.clip_size = dev(clip_size, (N, 2), 'clip_size')
    if noise is not None:
        d.noise = dev(noise, (N, T, Jmax, 2), 'noise')
    if miss_u is not None:
        d.miss_u = dev(miss_u, (N, T, Jmax), 'miss_u')
    for i, (q, r) in enumerate(zip(sources, raws)):
        c = d.sources[i]
        c.n, c.raw, c.Jd, c.C = r.shape[0], r.data_ptr(), r.shape[2], r.shape[3]
        if q.flip_perm is not None and is_flipped is not None:
            perm = _iarr(q.flip_perm)
            c.flip_perm = perm
            keep.append(perm)
        if q.miss_prob is not None and miss_u is not None:
            probs = (ctypes.c_float * r.shape[2])(*[float(v) for v in q.miss_prob])
            c.miss_prob = probs
            c.has_miss = 1
            keep.append(probs)
        c.transform = TRANSFORM[q.transform]
        c.n_hips, c.n_neck = len(q.hips_idx), len(q.neck_idx)
        for k, v in enumerate(q.hips_idx):
            c.hips_idx[k] = v
        for k, v in enumerate(q.neck_idx):
            c.neck_idx[k] = v
        if q.src_idx is not None:
            c.K = len(q.src_idx)
            si, di = _iarr(q.src_idx), _iarr(q.dst_idx)
            c.src_idx, c.dst_idx = si, di
            keep.append((si, di))
        c.has_noise = int(q.has_noise and noise is not None)
        c.has_bboxes = int(q.has_bboxes and with_boxes)
    frames = torch.empty(N, T, Ji, 3 if return_confidence else 2, **f32)
    targets['projection_2d'] = torch.empty(N, T, Ji, 2, **f32)
    d.frames, d.t_projection_2d = frames.data_ptr(), targets['projection_2d'].data_ptr()
    if noise is not None or miss_u is not None:
        targets['projection_2d_deformed'] = torch.empty(N, T, Ji, 2, **f32)
        d.t_deformed = targets['projection_2d_deformed'].data_ptr()
    if any(q.transform != 'none' for q in sources):       # the library refuses a mix of 'none' and a transform
        targets['projection_2d_transformed'] = torch.empty(N, T, Ji, 2, **f32)
        targets['projection_2d_shift'] = torch.empty(N, T, 2, **f32)
        targets['projection_2d_scale'] = torch.empty(N, T, **f32)
        d.t_transformed, d.shift = targets['projection_2d_transformed'].data_ptr(), targets['projection_2d_shift'].data_ptr()
        d.scale = targets['projection_2d_scale'].data_ptr()
    with torch.cuda.device(device):
        _lib.check(lib.p2c_collate_mixed_fwd(ctypes.byref(d), _stream()), 'p2c_collate_mixed_fwd')
    return frames, targets


# ----------------------------------------------------------------------------------------------------------------------
# fused small MLP (LinearAE) on fp32 MFMA
# ----------------------------------------------------------------------------------------------------------------------
def _mlp_desc(x, weights, biases):
    from pedestrians_video_2_carla_amd._lib import MlpDesc, P2C_MLP_MAX_LAYERS
    n = len(weights)
    if not 1 <= n <= P2C_MLP_MAX_LAYERS:
        raise RuntimeError(f'fused MLP supports 1..{P2C_MLP_MAX_LAYERS} layers, got {n}')
    d = MlpDesc()
    d.n_layers = n
    d.dims[0] = weights[0].shape[1]
    for l, (w, b) in enumerate(zip(weights, biases)):
        if w.shape[1] != d.dims[l] or b.shape[0] != w.shape[0]:
            raise RuntimeError('layer shapes do not chain')
        d.dims[l + 1] = w.shape[0]
        d.W[l], d.b[l] = w.data_ptr(), b.data_ptr()
    d.N = x.shape[0]
    d.x = x.data_ptr()
    return d


MLP_LDS_LIMIT = 160 * 1024      # bytes of LDS a workgroup of the fused MLP may ask for (csrc/p2c_mlp.hip)
_MLP_TP, _MLP_FW_WAVES = 17, 4    # TP (p2c_mlp_dev.h), FW_WAVES (p2c_mlp.hip)


def mlp_geometry(dims: Sequence[int]) -> dict:
    """The layout arithmetic of csrc/p2c_mlp.hip (fill(), lds_fwd(), lds_bwd(), lds_fwd_wave()) for the widths ``dims``, in pure
    Python (the callers of ``mlp_supported`` may run before the library is loaded): ``tiles`` (16x16 tiles of the augmented weight
    gradients), ``image_floats`` (the packed weight image) and the bytes of LDS of the cooperative forward, the backward and the
    wave-per-tile forward. tests/test_mlp_cells_gpu.py holds it to ``p2c_mlp_plan``."""
    dims = [int(v) for v in dims]
    nl = len(dims) - 1

    def pad16(n):
        return (n + 15) & ~15

    def ld_of(n_in):                    # pitch of a layer's image: k extent with the bias column, == 2 (mod 4)
        ld = max(((((n_in + 1 + 3) >> 2) + 3) & ~3) * 4, pad16(n_in))
        while ld & 3 != 2:
            ld += 1
        return ld

    def img_rows_of(n_out):
        return (n_out + 16) & ~15

    def act_rows_of(n):
        return pad16(n) + 16

    tiles = sum(((o + 15) // 16) * ((i + 1 + 15) // 16) for i, o in zip(dims[:-1], dims[1:]))
    image = (sum(img_rows_of(o) * ld_of(i) for i, o in zip(dims[:-1], dims[1:])) + 3) & ~3
    h_off = [0]
    for n in dims:
        h_off.append(h_off[-1] + act_rows_of(n))          # h_off[nl + 1] = rows of H_0 .. H_L
    rows_a = max([act_rows_of(n) for n in dims[0:nl:2]], default=0)      # wave forward: H_l lives in buffer l & 1
    rows_b = max([act_rows_of(n) for n in dims[1:nl:2]], default=0)
    return dict(tiles=tiles, image_floats=image,
                lds_fwd=4 * (image + h_off[nl] * _MLP_TP),
                lds_bwd=4 * (image + (h_off[nl] + h_off[nl + 1] - h_off[1]) * _MLP_TP),
                lds_fwd_wave=4 * (image + _MLP_FW_WAVES * (rows_a + rows_b) * _MLP_TP))


def mlp_supported(dims: Sequence[int]) -> bool:
    """Stacks whose forward AND backward the kernel accepts: 1 to 8 layers, every width in 1 .. 159, at most 96 16x16
    weight-gradient tiles, and the LDS of either direction within 160 KB."""
    dims = list(dims)
    if not 1 <= len(dims) - 1 <= 8 or min(dims) < 1 or max(dims) >= 160:
        return False
    g = mlp_geometry(dims)
    return g['tiles'] <= 96 and g['lds_fwd'] <= MLP_LDS_LIMIT and g['lds_bwd'] <= MLP_LDS_LIMIT


def mlp_plan(dims: Sequence[int], rows: int) -> Optional[dict]:
    """What the library would run for a stack of widths ``dims`` on ``rows`` rows in this process (``p2c_mlp_plan``: the kernels'
    shape provider, forward form, weight-gradient form, saved activations, grids, LDS, whether either direction is accepted), as
    a dict keyed by ``_lib.P2C_MLP_PLAN_FIELDS``; None for a layer count or a width outside the ABI. Launches nothing."""
    d = _lib.MlpDesc()
    if not 1 <= len(dims) - 1 <= _lib.P2C_MLP_MAX_LAYERS:
        return None
    d.n_layers, d.N = len(dims) - 1, int(rows)
    for i, v in enumerate(dims):
        d.dims[i] = int(v)
    out = (ctypes.c_int32 * _lib.P2C_MLP_PLAN_INTS)()
    rc = _lib.lib().p2c_mlp_plan(ctypes.byref(d), out)
    if rc == -2:
        return None
    _lib.check(rc, 'p2c_mlp_plan')
    return dict(zip(_lib.P2C_MLP_PLAN_FIELDS, out))


class FusedMLPFunction(torch.autograd.Function):
    """y = Linear_{L-1}(relu(... relu(Linear_0(x)))) in one launch; backward recomputes activations.

    ``sinks``: optional list [gW_0, gb_0, gW_1, ...] of pre-existing gradient tensors (e.g. views of the trainer's flat
    gradient buffer). When given, the backward WRITES the parameter gradients there and returns no gradient tensors --
    no per-parameter accumulate kernels, no zero_grad memset -- valid when this op is the parameters' only use in the
    step (true for the flows here; do not combine with gradient accumulation)."""

    @staticmethod
    def forward(ctx, x, n_layers, sinks, image, skip_pack, fused_opt, precision, *params):
        lib = _lib.lib()
        x = _require_device(x, 'x')
        weights = [_require_device(p, 'weight') for p in params[:n_layers]]
        biases = [_require_device(p, 'bias') for p in params[n_layers:]]
        desc = _mlp_desc(x, weights, biases)
        y = torch.empty(x.shape[0], weights[-1].shape[0], dtype=torch.float32, device=x.device)
        n_image = lib.p2c_mlp_image_floats(ctypes.byref(desc))
        if image is None:        # per-call image, packed by this forward
            image, skip_pack = torch.empty(n_image, dtype=torch.float32, device=x.device), False
        elif image.numel() != n_image or image.device != x.device or image.dtype != torch.float32:
            raise RuntimeError('packed weight image of the wrong size / device')
        desc.y, desc.w_image, desc.skip_pack = y.data_ptr(), image.data_ptr(), int(bool(skip_pack))
        desc.precision = ctx.precision = int(precision)
        # many sample tiles per workgroup: the forward leaves its hidden activations for the backward (0 = recompute)
        saved = None
        if any(ctx.needs_input_grad):           # (grad mode is off inside Function.forward: ask the autograd context)
            n_saved = lib.p2c_mlp_saved_floats(ctypes.byref(desc))
            if n_saved > 0:
                saved = torch.empty(n_saved, dtype=torch.float32, device=x.device)
                desc.saved = saved.data_ptr()
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_mlp_fwd(ctypes.byref(desc), _stream()), 'p2c_mlp_fwd')
        ctx.save_for_backward(x, image, *weights, *biases)
        ctx.saved_acts = saved
        ctx.n_layers, ctx.sinks = n_layers, sinks
        ctx.fused_opt = fused_opt if sinks is not None else None
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.lib()
        n = ctx.n_layers
        x, image, *rest = ctx.saved_tensors
        weights, biases = rest[:n], rest[n:]
        gy = _require_device(gy, 'grad')
        desc = _mlp_desc(x, weights, biases)
        desc.gy, desc.w_image = gy.data_ptr(), image.data_ptr()
        desc.precision = ctx.precision
        if ctx.saved_acts is not None:
            desc.saved = ctx.saved_acts.data_ptr()
        if ctx.sinks is not None:
            gws, gbs = ctx.sinks[0::2], ctx.sinks[1::2]
        else:
            gws = [torch.empty_like(w) for w in weights]
            gbs = [torch.empty_like(b) for b in biases]
        for l in range(n):
            desc.gW[l], desc.gb[l] = gws[l].data_ptr(), gbs[l].data_ptr()
        partials = torch.empty(lib.p2c_mlp_workspace_floats(ctypes.byref(desc)), dtype=torch.float32, device=x.device)
        desc.partials = partials.data_ptr()
        opt_desc = None
        if ctx.fused_opt is not None:       # the optimizer step rides on the gradient reduction (see p2c_mlp_desc.fused_adamw)
            opt_desc = ctx.fused_opt.descriptor_for_fusion()
            desc.fused_adamw = ctypes.addressof(opt_desc)
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_mlp_bwd(ctypes.byref(desc), _stream()), 'p2c_mlp_bwd')
        if ctx.fused_opt is not None:
            ctx.fused_opt.fused_steps_applied += 1       # the trainer checks that its deferred step really happened
        if ctx.sinks is not None:
            return (None,) * 7 + (None,) * (2 * n)
        return (None,) * 7 + (*gws, *gbs)


def fused_mlp(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor],
              sinks: Optional[Sequence[Tensor]] = None, image: Optional[Tensor] = None,
              image_is_current: bool = False, fused_optimizer=None, precision: str = 'fp32') -> Tensor:
    """``image``: optional persistent buffer (``mlp_image_floats`` floats) for the packed weights; with
    ``image_is_current`` the forward trusts it (kept current by ``mlp_pack`` + the optimizer's scatter) and launches no
    pack kernel. ``fused_optimizer`` (a FlatAdamW over exactly these parameters, with ``sinks`` = views of its gradient
    buffer): the backward applies the optimizer step inside its gradient reduction -- the caller must then NOT call
    ``optimizer.step()`` for this backward. ``precision``: 'fp32' (exact fp32 MFMA, default), 'bf16' (operands rounded to bf16)
    or 'bf16x3' (split-bf16, three MFMAs) -- the reduced arms exist for the 52-26-13-6-39-78-156 LinearAE only."""
    return FusedMLPFunction.apply(x, len(weights), None if sinks is None else list(sinks), image, image_is_current,
                                  fused_optimizer, _lib.PRECISION[precision], *weights, *biases)


def mlp_image_layout(dims: Sequence[int]) -> Tuple[int, Tensor]:
    """(floats of the packed image, int32 host tensor: image offset of every parameter in the order W_0, b_0, W_1, ...)."""
    lib = _lib.lib()
    d = _lib.MlpDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = int(v)
    n_params = sum(o * (i + 1) for i, o in zip(dims[:-1], dims[1:]))
    buf = (ctypes.c_int32 * n_params)()
    n = lib.p2c_mlp_image_index(ctypes.byref(d), buf, n_params)
    if n != n_params:
        raise _lib.P2CError(f'p2c_mlp_image_index returned {n}')
    # image size: the same arithmetic as the library, asked through a descriptor with dummy pointers
    x = torch.empty(1, dims[0])
    probe = _lib.MlpDesc()
    probe.n_layers, probe.N, probe.x = d.n_layers, 1, 1
    for i, v in enumerate(dims):
        probe.dims[i] = int(v)
    for l in range(d.n_layers):
        probe.W[l], probe.b[l] = 1, 1
    return int(lib.p2c_mlp_image_floats(ctypes.byref(probe))), torch.tensor(list(buf), dtype=torch.int32)


def mlp_pack(weights: Sequence[Tensor], biases: Sequence[Tensor], image: Tensor):
    """Write the packed image from the current weights (one small launch)."""
    lib = _lib.lib()
    x = weights[0]                       # any device tensor: only the geometry and the weight pointers are used
    desc = _mlp_desc(x.new_empty(1, weights[0].shape[1]), weights, biases)
    desc.w_image = image.data_ptr()
    with torch.cuda.device(image.device):
        _lib.check(lib.p2c_mlp_pack(ctypes.byref(desc), _stream()), 'p2c_mlp_pack')


# ----------------------------------------------------------------------------------------------------------------------
# the whole small-batch train step of LitPoseLiftingFlow(LinearAE) in two launches (K13, csrc/p2c_train.hip)
# ----------------------------------------------------------------------------------------------------------------------
LINEAR_AE_6D_DIMS = (52, 26, 13, 6, 39, 78, 156)
FUSED_TRAIN_MAX_T = 16


class PairCounter:
    """``count_target_pairs`` for one (spec, target shape) with its launch descriptor built once: called for every staged
    batch, so the per-call host work is one ctypes call."""

    def __init__(self, spec: PoseHeadSpec, gt2d: Tensor, out: Optional[Tensor] = None):
        gt2d = _require_device(gt2d, 'gt2d')
        if gt2d.ndim != 4 or gt2d.shape[3] < 2:
            raise RuntimeError(f'gt2d should have shape (B, T, joints, >= 2), got {tuple(gt2d.shape)}')
        B, T = gt2d.shape[0], gt2d.shape[1]
        if max(spec.gmap2d) >= gt2d.shape[2]:
            raise RuntimeError(f'gt2d has {gt2d.shape[2]} joints but the joint map needs index {max(spec.gmap2d)}')
        if out is not None and (tuple(out.shape) != (B,) or out.dtype != torch.float32 or out.device != gt2d.device
                                or not out.is_contiguous()):
            raise RuntimeError(f'out should be a contiguous float32 ({B},) tensor on {gt2d.device}')
        d = PoseHeadDesc()
        d.B, d.T = B, T
        d.kind, d.transform = KIND[spec.kind], TRANSFORM[spec.transform]
        d.t0, d.t1 = spec.frames(T)
        d.mask_missing_joints, d.hips_lane = int(spec.mask_missing_joints), spec.hips_lane
        d.n_hips = d.n_neck = 1
        d.hips_idx[0], d.neck_idx[0] = spec.hips_idx[0], spec.neck_idx[0]
        d.gmap2d[:] = spec.gmap2d
        d.gmap3d[:] = spec.gmap3d
        d.n_common2d = sum(1 for v in spec.gmap2d if v >= 0)
        d.n_common3d = sum(1 for v in spec.gmap3d if v >= 0)
        d.gt2d_joints, d.gt2d_channels = gt2d.shape[2], gt2d.shape[3]
        self.counts = out if out is not None else torch.empty(B, dtype=torch.float32, device=gt2d.device)
        d.skel_type = self.counts.data_ptr()                  # not read by the count kernel; validation wants non-NULL tables
        d.ref_rel_loc = d.ref_rel_rot = d.ref_hn_shift = d.ref_hn_scale = self.counts.data_ptr()
        self.desc, self.shape, self.device, self._lib = d, tuple(gt2d.shape), gt2d.device, _lib.lib()

    def matches(self, spec_shape, device) -> bool:
        return self.shape == tuple(spec_shape) and self.device == device

    def __call__(self, gt2d: Tensor) -> Tensor:
        if tuple(gt2d.shape) != self.shape or gt2d.device != self.device or gt2d.dtype != torch.float32 or not gt2d.is_contiguous():
            raise RuntimeError(f'gt2d should be a contiguous float32 {self.shape} tensor on {self.device}')
        self.desc.gt2d = gt2d.data_ptr()
        _lib.check(self._lib.p2c_count_target_pairs(ctypes.byref(self.desc), self.counts.data_ptr(),
                                                    torch.cuda.current_stream(self.device).cuda_stream), 'p2c_count_target_pairs')
        return self.counts


def count_target_pairs(spec: PoseHeadSpec, gt2d: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """(B,) float: per clip, the (frame, joint) pairs inside the eval slice whose 2-D target the loss does not mask
    (utils/tensors.py:29-40). A property of the targets alone: computed once when a batch is staged. ``out``: write into
    this (B,) buffer (a captured train step keeps reading the SAME address for every later batch)."""
    gt2d = _require_device(gt2d, 'gt2d')
    with torch.cuda.device(gt2d.device):
        return PairCounter(spec, gt2d, out)(gt2d)


TRAIN_STEP_RECORDER: Optional[list] = None      # set by the trainer around a capture: every p2c_train_step call is appended
                                                # (descriptor, gradient pointers, everything they point to)


class FusedTrainStepFunction(torch.autograd.Function):
    """(losses (3,), loc_2d, loc_3d, loc_2d_3d) = step(frames; LinearAE parameters): the forward launches NOTHING, the
    backward runs p2c_train_step (LinearAE forward + pose head forward / backward + dgrad per clip, then weight gradient
    + optional optimizer step + loss reduction) and FILLS the loss tensor. Only valid where the backward is guaranteed to
    follow before anyone reads a loss value: inside ``deferred_loss_finalize(2)`` (the trainer's step).
    ``sinks`` / ``image`` / ``fused_opt``: as FusedMLPFunction."""

    @staticmethod
    def forward(ctx, x, spec: PoseHeadSpec, skel_type, dloc, drot, gt2d, gt3d, counts, sinks, image, skip_pack,
                fused_opt, n_layers, *params):
        lib = _lib.lib()
        x = _require_device(x, 'frames')
        skel_type = _require_device(skel_type, 'skel_type', torch.int32)
        dloc = None if dloc is None else _require_device(dloc, 'world_loc_change_batch')
        drot = None if drot is None else _require_device(drot, 'world_rot_change_batch')
        gt2d = None if gt2d is None else _require_device(gt2d, 'gt2d')
        gt3d = None if gt3d is None else _require_device(gt3d, 'gt3d')
        counts = _require_device(counts, 'pair counts')
        if x.ndim != 4 or x.shape[2] * x.shape[3] != LINEAR_AE_6D_DIMS[0]:
            raise RuntimeError(f'frames should have shape (B, T, 26, 2), got {tuple(x.shape)}')
        B, T = x.shape[0], x.shape[1]
        y_like = x.new_empty((B, T, J, 6), device='meta')
        _check_shapes(spec, y_like, skel_type, dloc, drot, gt2d, gt3d)
        if tuple(counts.shape) != (B,):
            raise RuntimeError(f'pair counts should have shape ({B},), got {tuple(counts.shape)}')
        weights = [_require_device(p, 'weight') for p in params[:n_layers]]
        biases = [_require_device(p, 'bias') for p in params[n_layers:]]
        f32 = dict(dtype=torch.float32, device=x.device)
        ctx.bufs = {'partials': torch.empty(B * 4, **f32), 'loss_sums': torch.empty(4, **f32),
                    'losses': torch.empty(3, **f32)}
        ctx.spec, ctx.n_layers, ctx.sinks = spec, n_layers, sinks
        ctx.image, ctx.skip_pack = image, bool(skip_pack)
        ctx.fused_opt = fused_opt if sinks is not None else None
        ctx.save_for_backward(x, skel_type, dloc, drot, gt2d, gt3d, counts, *weights, *biases)
        ctx.set_materialize_grads(False)
        vec = ctx.bufs['losses']
        return vec, vec[0], vec[1], vec[2]

    @staticmethod
    def backward(ctx, g_losses, g0, g1, g2):
        lib = _lib.lib()
        n = ctx.n_layers
        x, skel_type, dloc, drot, gt2d, gt3d, counts, *rest = ctx.saved_tensors
        weights, biases = rest[:n], rest[n:]
        spec = ctx.spec
        B, T = x.shape[0], x.shape[1]
        scalars = [None if g is None else _require_device(g, 'grad loss') for g in (g0, g1, g2)]
        if g_losses is not None:
            g_losses = _require_device(g_losses, 'grad losses')
            if any(g is not None for g in scalars):
                g_losses = g_losses + torch.stack([torch.zeros_like(g_losses[0]) if g is None else g for g in scalars])
            gl = _lib.grad_loss_pointers(vector=g_losses.data_ptr())
        else:
            gl = _lib.grad_loss_pointers(*[_ptr(g) for g in scalars])
        if ctx.sinks is not None:
            gws, gbs = ctx.sinks[0::2], ctx.sinks[1::2]
        else:
            gws = [torch.empty_like(w) for w in weights]
            gbs = [torch.empty_like(b) for b in biases]
        desc, keep = train_step_desc(x, spec, skel_type, dloc, drot, gt2d, gt3d, counts, weights, biases, gws, gbs, ctx.bufs,
                                     ctx.image, ctx.skip_pack, ctx.fused_opt)
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_train_step(ctypes.byref(desc), gl, _stream()), 'p2c_train_step')
        if ctx.fused_opt is not None:
            ctx.fused_opt.fused_steps_applied += 1
        if TRAIN_STEP_RECORDER is not None:
            TRAIN_STEP_RECORDER.append({'desc': desc, 'gl': gl, 'device': x.device, 'fused_opt': ctx.fused_opt,
                                        'keep': (keep, ctx.bufs, g_losses, scalars, ctx.saved_tensors, gws, gbs, ctx.image)})
        head_none = (None,) * 13
        if ctx.sinks is not None:
            return head_none + (None,) * (2 * n)
        return head_none + (*gws, *gbs)


def train_step_desc(x, spec, skel_type, dloc, drot, gt2d, gt3d, counts, weights, biases, gws, gbs, bufs, image=None,
                    skip_pack=False, fused_opt=None):
    """(p2c_train_step_desc, objects to keep alive while it is used) for one fused train step on device tensors."""
    lib = _lib.lib()
    B, T = x.shape[0], x.shape[1]
    desc = _lib.TrainStepDesc()
    head = _fill_desc(spec, _MetaPtr((B, T, J, 6), x.device), skel_type, dloc, drot, gt2d, gt3d, bufs, {})
    head.y = None
    desc.head = head
    xf = x.reshape(B * T, -1)
    m = _mlp_desc(xf, weights, biases)
    n_image = lib.p2c_mlp_image_floats(ctypes.byref(m))
    if image is None:
        image, skip_pack = torch.empty(n_image, dtype=torch.float32, device=x.device), False
    elif image.numel() != n_image or image.device != x.device or image.dtype != torch.float32:
        raise RuntimeError('packed weight image of the wrong size / device')
    m.w_image, m.skip_pack = image.data_ptr(), int(bool(skip_pack))
    for l in range(len(weights)):
        m.gW[l], m.gb[l] = gws[l].data_ptr(), gbs[l].data_ptr()
    desc.mlp = m
    desc.pair_counts = counts.data_ptr()
    if not lib.p2c_train_step_supported(ctypes.byref(desc)):
        raise _lib.P2CError('p2c_train_step does not cover this shape (LinearAE 52-26-13-6-39-78-156, T <= 16)')
    ws = torch.empty(lib.p2c_train_step_workspace_floats(ctypes.byref(desc)), dtype=torch.float32, device=x.device)
    desc.mlp.partials = ws.data_ptr()
    opt_desc = None
    if fused_opt is not None:       # the optimizer step rides on the gradient reduction (see p2c_mlp_desc.fused_adamw)
        opt_desc = fused_opt.descriptor_for_fusion()
        desc.mlp.fused_adamw = ctypes.addressof(opt_desc)
    return desc, (xf, image, ws, opt_desc, gws, gbs)


class _MetaPtr:
    """Shape carrier for _fill_desc where the model output never exists in memory (fused train step)."""

    def __init__(self, shape, device):
        self.shape, self.device = tuple(shape), device

    def data_ptr(self):
        return 0


def train_step_supported(dims: Sequence[int], T: int) -> bool:
    return tuple(dims) == LINEAR_AE_6D_DIMS and 1 <= T <= FUSED_TRAIN_MAX_T


def fused_train_step(frames: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], spec: PoseHeadSpec,
                     skel_type: Tensor, counts: Tensor, dloc: Optional[Tensor] = None, drot: Optional[Tensor] = None,
                     gt2d: Optional[Tensor] = None, gt3d: Optional[Tensor] = None,
                     sinks: Optional[Sequence[Tensor]] = None, image: Optional[Tensor] = None,
                     image_is_current: bool = False, fused_optimizer=None) -> 'PoseLosses':
    """LinearAE + pose head + losses as ONE autograd node whose backward is the two-launch train step (p2c_train_step).
    Call only inside ``deferred_loss_finalize(2)``: the returned loss tensors are filled by the backward."""
    if _DEFER_LOSS_FINALIZE != 2:
        raise _lib.P2CError('fused_train_step needs the deferred_loss_finalize(2) context: its forward computes nothing')
    res = FusedTrainStepFunction.apply(frames, spec, skel_type, dloc, drot, gt2d, gt3d, counts,
                                       None if sinks is None else list(sinks), image, image_is_current, fused_optimizer,
                                       len(weights), *weights, *biases)
    return PoseLosses(res[0], res[1:4])


# ----------------------------------------------------------------------------------------------------------------------
# grouped per-joint embeddings (K7a, Seq2SeqEmbeddings._format_input)
# ----------------------------------------------------------------------------------------------------------------------
def _uniform_stride(tensors: Sequence[Tensor]) -> Optional[int]:
    """Element stride between consecutive tensors if they are equally spaced views of one buffer (e.g. the trainer's
    flat parameter buffer), else None."""
    if len(tensors) == 1:
        return tensors[0].numel()
    if any(not t.is_contiguous() for t in tensors):
        return None
    step = tensors[1].data_ptr() - tensors[0].data_ptr()
    if step <= 0 or step % 4 or any(tensors[i + 1].data_ptr() - tensors[i].data_ptr() != step
                                    for i in range(len(tensors) - 1)):
        return None
    return step // 4


class JointEmbeddingsFunction(torch.autograd.Function):
    """y (T,B,J,E) = per-joint Linear(C,E) of x (B,T,J,C), sequence-first (time-reversed when ``flip``), one launch.

    ``params`` = (w_0, b_0, w_1, b_1, ...). When the weights (and the biases) are equally spaced views of one buffer they are
    read in place; otherwise they are stacked first. ``sinks`` (optional) = the matching gradient tensors, equally spaced
    too: the backward then writes the gradients there and returns none (same contract as FusedMLPFunction)."""

    @staticmethod
    def forward(ctx, x, flip: bool, sinks, *params):
        lib = _lib.lib()
        x = _require_device(x, 'x')
        if x.ndim != 4:
            raise RuntimeError(f'x should be (B, T, joints, channels), got {tuple(x.shape)}')
        B, T, Jn, C = x.shape
        ws = [_require_device(p, 'weight') for p in params[0::2]]
        bs = [_require_device(p, 'bias') for p in params[1::2]]
        if len(ws) != Jn or any(w.shape != ws[0].shape or w.shape[1] != C for w in ws):
            raise RuntimeError('one (E, C) weight per joint expected')
        E = ws[0].shape[0]
        wst, bst = _uniform_stride(ws), _uniform_stride(bs)
        if wst is None or bst is None:
            W, bb = torch.stack(ws), torch.stack(bs)
            wptr, bptr, wst, bst = W.data_ptr(), bb.data_ptr(), E * C, E
        else:
            wptr, bptr = ws[0].data_ptr(), bs[0].data_ptr()
        y = torch.empty(T, B, Jn, E, dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_embed_fwd(x.data_ptr(), wptr, bptr, wst, bst, y.data_ptr(), B, T, Jn, C, E, int(flip),
                                         _stream()), 'p2c_embed_fwd')
        ctx.save_for_backward(x)
        ctx.cfg = (B, T, Jn, C, E, bool(flip))
        ctx.sinks = sinks
        ctx.n_params = len(params)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.lib()
        (x,) = ctx.saved_tensors
        B, T, Jn, C, E, flip = ctx.cfg
        gy = _require_device(gy, 'grad')
        f32 = dict(dtype=torch.float32, device=x.device)
        part = torch.empty(lib.p2c_embed_workspace_floats(B, T, Jn, C, E), **f32)
        sinks = ctx.sinks
        direct = False
        if sinks is not None:
            gws, gbs = sinks[0::2], sinks[1::2]
            wst, bst = _uniform_stride(gws), _uniform_stride(gbs)
            direct = wst is not None and bst is not None
        if direct:
            gwptr, gbptr = gws[0].data_ptr(), gbs[0].data_ptr()
        else:
            gW, gb = torch.empty(Jn, E, C, **f32), torch.empty(Jn, E, **f32)
            gwptr, gbptr, wst, bst = gW.data_ptr(), gb.data_ptr(), E * C, E
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_embed_bwd(x.data_ptr(), gy.data_ptr(), wst, bst, gwptr, gbptr, part.data_ptr(), B, T, Jn, C, E,
                                         int(flip), _stream()), 'p2c_embed_bwd')
        if direct:
            return (None, None, None) + (None,) * ctx.n_params
        grads = [g for j in range(Jn) for g in (gW[j], gb[j])]
        return (None, None, None, *grads)


def joint_embeddings(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], flip: bool = False,
                     sinks: Optional[Sequence[Tensor]] = None) -> Tensor:
    params = [p for pair in zip(weights, biases) for p in pair]
    return JointEmbeddingsFunction.apply(x, flip, sinks, *params)


# ----------------------------------------------------------------------------------------------------------------------
# dropout masks drawn inside the time-loop kernels (csrc/p2c_rec_dev.h)
# ----------------------------------------------------------------------------------------------------------------------
def dropout_state(device) -> Tensor:
    """Four int32 words {seed_lo, seed_hi, step, next} for the kernels that draw their dropout masks themselves. The seed is ONE
    draw from the framework's default CPU generator (what ``torch.manual_seed`` / ``seed_everything`` seed) mixed with the rank of
    the process: a run repeats under a fixed seed, two modules and two ranks draw different masks, and after this one draw
    nothing comes from the framework's generators (no generator launch, no RNG-state fill in front of a replayed graph)."""
    rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
    draw = int(torch.randint(0, 1 << 62, (1,), dtype=torch.int64).item())
    seed = (draw * 0x9E3779B97F4A7C15 + rank * 0xD1B54A32D192ED03) % (1 << 64)
    lo, hi = seed & 0x7FFFFFFF, (seed >> 32) & 0x7FFFFFFF
    st = torch.tensor([lo, hi, 0, 0], dtype=torch.int32, device=device)
    _DROP_STATES.append(weakref.ref(st))
    return st


_DROP_STATES = []


def dropout_states_snapshot() -> list:
    """(state, copy) of every live in-kernel dropout state: what has to be put back for a step to draw the same masks again
    (the trainer's capture-time replay check compares an eager step with replays of the captured one)."""
    live = [r() for r in _DROP_STATES]
    _DROP_STATES[:] = [weakref.ref(t) for t in live if t is not None]
    return [(t, t.clone()) for t in live if t is not None]


def dropout_states_restore(snapshot: list, rewind_new: bool = False) -> None:
    """Put the snapshot's states back; ``rewind_new``: a state created since the snapshot (by a warm-up step of the trainer)
    goes back to step 0 -- the position it had when its first step drew from it."""
    known = set()
    for t, saved in snapshot:
        t.copy_(saved)
        known.add(id(t))
    if rewind_new:
        for r in _DROP_STATES:
            t = r()
            if t is not None and id(t) not in known:
                t[2:].zero_()


def kernel_dropout_enabled() -> bool:
    """P2C_TORCH_DROPOUT=1: the framework's dropout (one generator launch per site + RNG-state fills per replay) instead."""
    return os.environ.get('P2C_TORCH_DROPOUT', '0') != '1'


# ----------------------------------------------------------------------------------------------------------------------
# LSTM layer: library GEMM for the input projection + one HIP launch for the recurrence (K7b), or one launch per time step
# for any other hidden size up to 1024 (K18)
# ----------------------------------------------------------------------------------------------------------------------
def lstm_supported(hidden_size: int) -> bool:
    """The widths of the single-launch recurrence (K7b). Gates Seq2Seq's encoder stack and decoder loop."""
    return hidden_size in (16, 32, 48, 64, 96, 128)


REC_STEPS_MAX_HIDDEN = 1024      # the widest layer of the one-launch-per-step recurrences (K18, K23: csrc/p2c_rec_step_dev.h)


def lstm_steps_supported(hidden_size: int) -> bool:
    """The widths of the one-launch-per-step recurrence (K18, p2c_lstm_steps_*): any 1 <= H <= REC_STEPS_MAX_HIDDEN.
    ``lstm_layer`` takes it for every width outside ``lstm_supported``."""
    return 1 <= hidden_size <= REC_STEPS_MAX_HIDDEN


def _dense_grad(g: Optional[Tensor], name: str) -> Optional[Tensor]:
    """An optional incoming gradient, dense on the device. Keep it in a local: a strided one is a copy the launch has to outlive."""
    return None if g is None else _require_device(g, name)


def _recurrent_weight_grad(g: Tensor, out: Tensor, h0: Tensor, w_hh: Tensor, zero_state: bool) -> Optional[Tensor]:
    """dW_hh = sum_t g[t]^T h[t-1] over all (t, b) (K12), g (T,B,G) the gradient of the recurrent pre-activations. None: it was
    added into w_hh.grad (the gradient sink)."""
    sink = _sink(w_hh)
    g_w, acc = sink, sink is not None
    if out.shape[0] > 1:
        g_w, acc = atb(g[1:].reshape(-1, g.shape[2]), out[:-1].reshape(-1, out.shape[2]), out=g_w, accumulate=acc)[0], True
    if not zero_state:                # the t = 0 term meets the initial state (zero state: no contribution)
        g_w = atb(g[0], h0, out=g_w, accumulate=acc)[0]
    if sink is not None:
        return None
    return torch.zeros_like(w_hh) if g_w is None else g_w


class LSTMRecurrenceFunction(torch.autograd.Function):
    """(out (T,B,H), hT, cT) = recurrence(gx (T,B,4H), h0, c0, W_hh (4H,H)); gate order i, f, g, o (torch.nn.LSTM)."""

    @staticmethod
    def forward(ctx, gx, h0, c0, w_hh):
        lib = _lib.lib()
        ctx.set_materialize_grads(False)                      # an unused output (out of the last layer, hT / cT) stays None:
        gx, w_hh = _require_device(gx, 'gx'), _require_device(w_hh, 'weight_hh')   # the kernel reads nothing for it
        ctx.zero_state = h0 is None and c0 is None           # nn.LSTM's default initial state: nothing to read or to return
        T, B, G = gx.shape
        H = w_hh.shape[1]
        if ctx.zero_state:
            h0 = c0 = gx.new_empty(0)
        else:
            h0, c0 = _require_device(h0, 'h0'), _require_device(c0, 'c0')
        if G != 4 * H or w_hh.shape[0] != 4 * H or (not ctx.zero_state and (h0.shape != (B, H) or c0.shape != (B, H))):
            raise RuntimeError(f'inconsistent LSTM shapes: gx {tuple(gx.shape)}, w_hh {tuple(w_hh.shape)}, h0 {tuple(h0.shape)}')
        ctx.steps = not lstm_supported(H)                     # K18 for the widths K7b does not cover
        if ctx.steps and not lstm_steps_supported(H):
            raise RuntimeError(f'hidden size {H} is not supported by the HIP recurrence (16, 32, 48, 64, 96, 128 in one launch, '
                               f'any other 1 ... {REC_STEPS_MAX_HIDDEN} one launch per step)')
        f32 = dict(dtype=torch.float32, device=gx.device)
        out, hT, cT = torch.empty(T, B, H, **f32), torch.empty(B, H, **f32), torch.empty(B, H, **f32)
        acts, cs = torch.empty(T, B, 4 * H, **f32), torch.empty(T, B, H, **f32)
        d = _lib.LstmDesc()
        d.T, d.B, d.H = T, B, H
        d.gx, d.w_hh = gx.data_ptr(), w_hh.data_ptr()
        if not ctx.zero_state:
            d.h0, d.c0 = h0.data_ptr(), c0.data_ptr()
        d.out, d.hT, d.cT, d.acts, d.cs = out.data_ptr(), hT.data_ptr(), cT.data_ptr(), acts.data_ptr(), cs.data_ptr()
        with torch.cuda.device(gx.device):
            if ctx.steps:
                _lib.check(lib.p2c_lstm_steps_fwd(ctypes.byref(d), _stream()), 'p2c_lstm_steps_fwd')
            else:
                _lib.check(lib.p2c_lstm_rec_fwd(ctypes.byref(d), _stream()), 'p2c_lstm_rec_fwd')
        ctx.save_for_backward(h0, c0, w_hh, out, acts, cs)
        return out, hT, cT

    @staticmethod
    def backward(ctx, g_out, g_hT, g_cT):
        lib = _lib.lib()
        h0, c0, w_hh, out, acts, cs = ctx.saved_tensors
        T, B, H = out.shape
        f32 = dict(dtype=torch.float32, device=out.device)
        zero = ctx.zero_state
        g_gx = torch.empty(T, B, 4 * H, **f32)
        g_h0 = g_c0 = None
        d = _lib.LstmDesc()
        d.T, d.B, d.H = T, B, H
        d.w_hh, d.acts, d.cs = w_hh.data_ptr(), acts.data_ptr(), cs.data_ptr()
        if not zero:
            g_h0, g_c0 = torch.empty(B, H, **f32), torch.empty(B, H, **f32)
            d.c0, d.g_h0, d.g_c0 = c0.data_ptr(), g_h0.data_ptr(), g_c0.data_ptr()
        g_out, g_hT, g_cT = _dense_grad(g_out, 'grad out'), _dense_grad(g_hT, 'grad hT'), _dense_grad(g_cT, 'grad cT')
        d.g_out, d.g_hT, d.g_cT = _ptr(g_out), _ptr(g_hT), _ptr(g_cT)
        d.g_gx = g_gx.data_ptr()
        with torch.cuda.device(out.device):
            if ctx.steps:
                ws = torch.empty(lib.p2c_lstm_steps_workspace_floats(B, H), **f32)
                _lib.check(lib.p2c_lstm_steps_bwd(ctypes.byref(d), ws.data_ptr(), _stream()), 'p2c_lstm_steps_bwd')
            else:
                _lib.check(lib.p2c_lstm_rec_bwd(ctypes.byref(d), _stream()), 'p2c_lstm_rec_bwd')
        g_w = _recurrent_weight_grad(g_gx, out, h0, w_hh, zero) if ctx.needs_input_grad[3] else None
        return g_gx, g_h0, g_c0, g_w


_BLAS_CHOSEN = False


def _prefer_rocblas_once():
    """The projections around the recurrence are small dense GEMMs (e.g. 512 x 52 x 256 per decoder step). Measured on
    MI355X (cfg3, B = 512): hipBLASLt's pick for them runs 33.7 us per call, rocBLAS's 7.9 us (step 5.7 -> 3.5 ms), so the
    first fused LSTM call switches torch's preferred BLAS library to rocBLAS. ``P2C_KEEP_BLAS=1`` leaves torch's choice."""
    global _BLAS_CHOSEN
    if _BLAS_CHOSEN:
        return
    _BLAS_CHOSEN = True
    import os
    if os.environ.get('P2C_KEEP_BLAS', '0') != '1':
        try:
            torch.backends.cuda.preferred_blas_library('cublas')      # = rocBLAS on ROCm
        except Exception:                                              # older torch: keep the default
            pass


def lstm_layer(x: Tensor, h0: Optional[Tensor], c0: Optional[Tensor], w_ih: Tensor, w_hh: Tensor, b_ih: Optional[Tensor],
               b_hh: Optional[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """One unidirectional torch.nn.LSTM layer: x (T,B,I) -> (out (T,B,H), hT (B,H), cT (B,H)). The input projection for
    all time steps is one dense GEMM (library); the time loop is one HIP launch (p2c_lstm_rec_fwd) for the widths of
    ``lstm_supported`` and one launch per time step (p2c_lstm_steps_fwd) for any other width up to 1024."""
    _prefer_rocblas_once()
    T, B, I = x.shape
    bias = None if b_ih is None else (b_ih + b_hh if b_hh is not None else b_ih)
    gx = dense(x.reshape(T * B, I), w_ih, bias).view(T, B, -1)
    return LSTMRecurrenceFunction.apply(gx, h0, c0, w_hh)


# ----------------------------------------------------------------------------------------------------------------------
# GRU layer: library GEMM for the input projection + one HIP launch per time step for the recurrence (K23)
# ----------------------------------------------------------------------------------------------------------------------
def gru_steps_supported(hidden_size: int) -> bool:
    """The widths of the GRU recurrence (K23, p2c_gru_steps_*): any 1 <= H <= REC_STEPS_MAX_HIDDEN."""
    return 1 <= hidden_size <= REC_STEPS_MAX_HIDDEN


class GRURecurrenceFunction(torch.autograd.Function):
    """(out (T,B,H), hT) = recurrence(gx (T,B,3H), h0, W_hh (3H,H), b_hh (3H)); gate order r, z, n (torch.nn.GRU). b_hh is the
    recurrence's own: b_hn sits inside the reset gate's product."""

    @staticmethod
    def forward(ctx, gx, h0, w_hh, b_hh):
        lib = _lib.lib()
        ctx.set_materialize_grads(False)                      # an unused output (out of the last layer, hT) stays None
        gx, w_hh = _require_device(gx, 'gx'), _require_device(w_hh, 'weight_hh')
        ctx.zero_state = h0 is None                           # nn.GRU's default initial state: nothing to read or to return
        ctx.has_bias, ctx.bias_param = b_hh is not None, b_hh     # (the parameter itself: its .grad may be a gradient sink)
        T, B, G = gx.shape
        H = w_hh.shape[1]
        h0 = gx.new_empty(0) if ctx.zero_state else _require_device(h0, 'h0')
        b_hh = gx.new_empty(0) if b_hh is None else _require_device(b_hh, 'bias_hh')
        if G != 3 * H or w_hh.shape[0] != 3 * H or (not ctx.zero_state and h0.shape != (B, H)) or (ctx.has_bias and b_hh.shape != (3 * H,)):
            raise RuntimeError(f'inconsistent GRU shapes: gx {tuple(gx.shape)}, w_hh {tuple(w_hh.shape)}, h0 {tuple(h0.shape)}')
        if not gru_steps_supported(H):
            raise RuntimeError(f'hidden size {H} is not supported by the HIP GRU recurrence (any 1 ... {REC_STEPS_MAX_HIDDEN})')
        f32 = dict(dtype=torch.float32, device=gx.device)
        out, hT, acts = torch.empty(T, B, H, **f32), torch.empty(B, H, **f32), torch.empty(T, B, 4 * H, **f32)
        d = _lib.GruDesc()
        d.T, d.B, d.H = T, B, H
        d.gx, d.w_hh = gx.data_ptr(), w_hh.data_ptr()
        if not ctx.zero_state:
            d.h0 = h0.data_ptr()
        if ctx.has_bias:
            d.bias_hh = b_hh.data_ptr()
        d.out, d.hT, d.acts = out.data_ptr(), hT.data_ptr(), acts.data_ptr()
        with torch.cuda.device(gx.device):
            _lib.check(lib.p2c_gru_steps_fwd(ctypes.byref(d), _stream()), 'p2c_gru_steps_fwd')
        ctx.save_for_backward(h0, w_hh, out, acts)
        return out, hT

    @staticmethod
    def backward(ctx, g_out, g_hT):
        lib = _lib.lib()
        h0, w_hh, out, acts = ctx.saved_tensors
        T, B, H = out.shape
        f32 = dict(dtype=torch.float32, device=out.device)
        zero = ctx.zero_state
        g_gx, g_gh = torch.empty(T, B, 3 * H, **f32), torch.empty(T, B, 3 * H, **f32)
        g_h0 = None
        d = _lib.GruDesc()
        d.T, d.B, d.H = T, B, H
        d.w_hh, d.acts, d.out = w_hh.data_ptr(), acts.data_ptr(), out.data_ptr()
        if not zero:
            g_h0 = torch.empty(B, H, **f32)
            d.h0, d.g_h0 = h0.data_ptr(), g_h0.data_ptr()
        g_out, g_hT = _dense_grad(g_out, 'grad out'), _dense_grad(g_hT, 'grad hT')
        d.g_out, d.g_hT = _ptr(g_out), _ptr(g_hT)
        d.g_gx, d.g_gh = g_gx.data_ptr(), g_gh.data_ptr()
        with torch.cuda.device(out.device):
            ws = torch.empty(lib.p2c_gru_steps_workspace_floats(B, H), **f32)
            _lib.check(lib.p2c_gru_steps_bwd(ctypes.byref(d), ws.data_ptr(), _stream()), 'p2c_gru_steps_bwd')
        g_w = _recurrent_weight_grad(g_gh, out, h0, w_hh, zero) if ctx.needs_input_grad[2] else None
        g_b = None
        if ctx.has_bias and ctx.needs_input_grad[3]:      # db_hh = sum over all (t, b) of g_gh, t = 0 included
            g_b = column_sums(g_gh.view(-1, 3 * H))
            sink = _sink(ctx.bias_param)
            if sink is not None:
                sink.view(-1).add_(g_b)
                g_b = None
        return g_gx, g_h0, g_w, g_b


def gru_layer(x: Tensor, h0: Optional[Tensor], w_ih: Tensor, w_hh: Tensor, b_ih: Optional[Tensor],
              b_hh: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """One unidirectional torch.nn.GRU layer: x (T,B,I) -> (out (T,B,H), hT (B,H)). The input projection x W_ih^T + b_ih for
    all time steps is one dense GEMM; the time loop is one HIP launch per step (p2c_gru_steps_fwd, any H up to 1024), which
    takes b_hh itself."""
    _prefer_rocblas_once()
    T, B, I = x.shape
    gx = dense(x.reshape(T * B, I), w_ih, b_ih).view(T, B, -1)
    return GRURecurrenceFunction.apply(gx, h0, w_hh, b_hh)


# ----------------------------------------------------------------------------------------------------------------------
# classification head: loss, d logits, predicted class and confusion counts in one launch (K24)
# ----------------------------------------------------------------------------------------------------------------------
CLS_MAX_CLASSES = 32


def cls_framework() -> bool:
    """P2C_CLS_FRAMEWORK=1: the classification models run the framework RNN and the flow the torch criterion on the device (the
    comparison arm of tools/bench_gru_classifier.py)."""
    return os.environ.get('P2C_CLS_FRAMEWORK', '0') == '1'


def _cls_head_ok(logits: Tensor, targets: Tensor, confusion: Optional[Tensor], binary: bool) -> bool:
    C = 2 if binary else logits.shape[-1]
    return (logits.is_cuda and logits.dtype == torch.float32 and targets.is_cuda and targets.dtype == torch.int64
            and 2 <= C <= CLS_MAX_CLASSES and not cls_framework() and not torch.is_autocast_enabled()
            and (confusion is None or (confusion.is_cuda and confusion.dtype == torch.int32 and confusion.is_contiguous()
                                       and confusion.shape == (C, C))))


def _count_confusion(logits: Tensor, targets: Tensor, confusion: Tensor, binary: bool) -> None:
    """The tensor-op confusion count (host tensors, C > 32, other dtypes): same rule as K24."""
    C = confusion.shape[0]
    with torch.no_grad():
        pred = (logits.reshape(-1) > 0).long() if binary else logits.argmax(dim=-1)
        t = targets.reshape(-1).long()
        ok = (t >= 0) & (t < C)
        counts = torch.bincount(t[ok] * C + pred[ok], minlength=C * C).view(C, C)
        confusion += counts.to(confusion.dtype)


class ClassificationHeadFunction(torch.autograd.Function):
    """loss = K24(logits, targets); the launch leaves d loss / d logits, the backward multiplies it by the incoming gradient."""

    @staticmethod
    def forward(ctx, logits, targets, confusion, binary: bool):
        lib = _lib.lib()
        x = logits.contiguous()
        B = targets.numel()
        C = 1 if binary else x.shape[-1]
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        g = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_cls_head(x.data_ptr(), targets.data_ptr(), B, C, _lib.P2C_CLS_BINARY if binary else 0,
                                        loss.data_ptr(), _ptr(g), _ptr(confusion), _stream()), 'p2c_cls_head')
        ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        g, = ctx.saved_tensors
        return (None if g is None else g * g_loss), None, None, None


def classification_loss(logits: Tensor, targets: Tensor, confusion: Optional[Tensor] = None, binary: bool = False) -> Tensor:
    """Mean ``CrossEntropyLoss`` of logits (B, C) against int64 targets (B) -- ``binary``: ``BCEWithLogitsLoss`` of logits (B) or
    (B, 1) against targets 0 / 1 -- and, when ``confusion`` ((C, C) int32, the caller's) is given,
    ``confusion[target, predicted] += 1`` for every row, in one launch (K24). Rows whose target lies outside [0, C) are ignored.
    C > 32, host tensors and other dtypes take the torch criterion plus a tensor-op count."""
    if binary and logits.ndim == 2 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    targets = targets.reshape(-1)
    if logits.shape[0] != targets.shape[0] or logits.ndim != (1 if binary else 2):
        raise RuntimeError(f'classification_loss: logits {tuple(logits.shape)} against targets {tuple(targets.shape)}')
    if _cls_head_ok(logits, targets, confusion, binary):
        return ClassificationHeadFunction.apply(logits, targets.contiguous(), confusion, binary)
    if binary:
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, targets.to(logits.dtype))
    else:
        loss = torch.nn.functional.cross_entropy(logits, targets.long())
    if confusion is not None:
        _count_confusion(logits, targets, confusion, binary)
    return loss


def classification_count(logits: Tensor, targets: Tensor, confusion: Tensor, binary: bool = False) -> None:
    """``confusion[target, predicted] += 1`` alone (K24's count-only mode: no loss, no gradient)."""
    if binary and logits.ndim == 2 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    targets = targets.reshape(-1)
    if _cls_head_ok(logits, targets, confusion, binary):
        x, t = logits.detach().contiguous(), targets.contiguous()
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().p2c_cls_head(x.data_ptr(), t.data_ptr(), t.numel(), 1 if binary else x.shape[-1],
                                               _lib.P2C_CLS_COUNT_ONLY | (_lib.P2C_CLS_BINARY if binary else 0), None, None,
                                               confusion.data_ptr(), _stream()), 'p2c_cls_head')
    else:
        _count_confusion(logits, targets, confusion, binary)


# ----------------------------------------------------------------------------------------------------------------------
# ranking metrics: per-class sorted curve counts and AUROC of an epoch's scores (K25)
# ----------------------------------------------------------------------------------------------------------------------
def rank_framework() -> bool:
    """P2C_RANK_FRAMEWORK=1: the ranking runs as tensor ops on the device (the comparison arm of tools/bench_rank_metrics.py)."""
    return os.environ.get('P2C_RANK_FRAMEWORK', '0') == '1'


def _rank_curves_tensor_ops(scores: Tensor, targets: Tensor) -> dict:
    """K25's outputs from ``torch.sort``, a cumulative sum and the differences of the sorted values: the same integers."""
    N, C = scores.shape
    K = 2 if C == 1 else C
    t = targets.long()
    keep = (t >= 0) & (t < K) & ~torch.isnan(scores).any(dim=1)
    s, t = scores[keep] + 0.0, t[keep]                                  # (-0.0 + 0.0 = +0.0: one group with +0.0)
    n_valid = int(s.shape[0])
    out = {'thresholds': [], 'tps': [], 'fps': [], 'n_points': [], 'n_pos': [], 'n_valid': n_valid}
    auroc = []
    for c in range(C):
        v, order = torch.sort(s[:, c], descending=True)
        pos = (t == (1 if C == 1 else c))[order]
        ends = torch.ones(n_valid, dtype=torch.bool, device=s.device)
        if n_valid > 1:
            ends[:-1] = v[1:] != v[:-1]
        idx = torch.nonzero(ends).reshape(-1)
        tps = torch.cumsum(pos.long(), 0)[idx]
        fps = idx + 1 - tps
        P = int(tps[-1]) if n_valid else 0
        Q = n_valid - P
        zero = torch.zeros(1, dtype=torch.int64, device=s.device)
        num = ((fps - torch.cat([zero, fps])[:-1]) * (tps + torch.cat([zero, tps])[:-1])).sum()
        # the one division on the host, in Python integers: a device fp64 division of the framework need not round correctly
        auroc.append(int(num) / (2 * P * Q) if P > 0 and Q > 0 else float('nan'))
        out['thresholds'].append(v[idx])
        out['tps'].append(tps.int())
        out['fps'].append(fps.int())
        out['n_points'].append(int(idx.numel()))
        out['n_pos'].append(P)
    out['auroc'] = torch.tensor(auroc, dtype=torch.float64, device=s.device)
    return out


def rank_curves(scores: Tensor, targets: Tensor, force_global: bool = False) -> dict:
    """The ranking behind AUROC / ROC / precision-recall of scores (N, C) -- or (N), the binary form: one column, positive when
    target == 1 -- against integer targets (N). Class c one-vs-rest; rows with a target outside the label range or a NaN score are
    dropped. Returns ``thresholds`` / ``tps`` / ``fps``: per class, one tensor per list entry, the distinct scores in descending
    order and the positives / negatives ranked at or above each (int32); ``n_points``, ``n_pos``: per-class ints; ``auroc``: (C)
    float64 tensor, NaN for a class without positives or without negatives; ``n_valid``: rows kept. Device float32 scores with
    C <= 32 and N <= 2^24 run K25 (one launch up to N = 16384, a radix sort beyond, or with ``force_global``), one host sync for
    the sizes; host tensors, other shapes and P2C_RANK_FRAMEWORK=1 take the tensor-op restatement."""
    if scores.ndim == 1:
        scores = scores[:, None]
    targets = targets.reshape(-1)
    if scores.ndim != 2 or scores.shape[0] != targets.shape[0] or scores.shape[1] < 1:
        raise RuntimeError(f'rank_curves: scores {tuple(scores.shape)} against targets {tuple(targets.shape)}')
    N, C = scores.shape
    if not (scores.is_cuda and targets.is_cuda and scores.dtype == torch.float32 and C <= _lib.P2C_RANK_MAX_CLASSES
            and N <= _lib.P2C_RANK_MAX_ROWS and not rank_framework()):
        with torch.no_grad():
            return _rank_curves_tensor_ops(scores.detach().float(), targets)
    lib = _lib.lib()
    dev = scores.device
    s, t = scores.detach().contiguous(), targets.to(torch.int32).contiguous()
    flags = _lib.P2C_RANK_GLOBAL if force_global else 0
    rows = max(N, 1)
    thresholds = torch.empty(C, rows, dtype=torch.float32, device=dev)
    counts = torch.empty(2, C, rows, dtype=torch.int32, device=dev)      # tps, fps
    sizes = torch.empty(2 * C + 1, dtype=torch.int32, device=dev)        # n_points (C), n_pos (C), n_valid
    auroc = torch.empty(C, dtype=torch.float64, device=dev)
    ws_bytes = lib.p2c_rank_workspace_bytes(N, C, flags)
    if ws_bytes < 0:
        _lib.check(int(ws_bytes), 'p2c_rank_workspace_bytes')
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if ws_bytes else None
    d = _lib.RankDesc()
    d.N, d.C, d.flags = N, C, flags
    d.scores, d.targets, d.thresholds = s.data_ptr(), t.data_ptr(), thresholds.data_ptr()
    d.tps, d.fps = counts[0].data_ptr(), counts[1].data_ptr()
    d.n_points, d.n_pos, d.n_valid = sizes.data_ptr(), sizes[C:].data_ptr(), sizes[2 * C:].data_ptr()
    d.auroc = auroc.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(lib.p2c_rank_curves(ctypes.byref(d), _ptr(ws), _stream()), 'p2c_rank_curves')
    host = sizes.cpu().tolist()                                          # the one host sync
    n_points, n_pos = host[:C], host[C:2 * C]
    return {'thresholds': [thresholds[c, :n_points[c]] for c in range(C)],
            'tps': [counts[0, c, :n_points[c]] for c in range(C)], 'fps': [counts[1, c, :n_points[c]] for c in range(C)],
            'n_points': n_points, 'n_pos': n_pos, 'auroc': auroc, 'n_valid': host[2 * C]}


def rank_scores(logits: Tensor, targets: Tensor, out_scores: Tensor, out_targets: Tensor, offset: int, binary: bool = False) -> None:
    """Rows [offset, offset + B) of the epoch buffers ``out_scores`` ((capacity, C) float32; (capacity, 1) binary) and
    ``out_targets`` ((capacity) int32) from a batch's logits (B, C) -- binary: (B) or (B, 1) -- and integer targets (B): fp32
    softmax with the maximum subtracted, or sigmoid; a target outside the label range arrives as -1. One launch on the device
    (K25's ``p2c_rank_scores``, on both arms of P2C_RANK_FRAMEWORK: the switch is about the ranking); host tensors, other dtypes
    and C > 32 take the tensor ops."""
    if binary and logits.ndim == 2 and logits.shape[1] == 1:
        logits = logits.squeeze(1)
    targets = targets.reshape(-1)
    B = targets.shape[0]
    C = 1 if binary else logits.shape[-1]
    if logits.shape[0] != B or logits.ndim != (1 if binary else 2):
        raise RuntimeError(f'rank_scores: logits {tuple(logits.shape)} against targets {tuple(targets.shape)}')
    cap = out_targets.shape[0]
    if (out_scores.shape != (cap, C) or out_scores.dtype != torch.float32 or out_targets.dtype != torch.int32 or offset < 0
            or offset + B > cap or not out_scores.is_contiguous() or not out_targets.is_contiguous()):
        raise RuntimeError(f'rank_scores: rows [{offset}, {offset + B}) of buffers {tuple(out_scores.shape)} / {tuple(out_targets.shape)}')
    if (logits.is_cuda and targets.is_cuda and out_scores.is_cuda and out_targets.is_cuda and logits.dtype == torch.float32
            and targets.dtype == torch.int64 and (binary or 2 <= C <= _lib.P2C_RANK_MAX_CLASSES)):
        x, t = logits.detach().contiguous(), targets.contiguous()
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().p2c_rank_scores(x.data_ptr(), t.data_ptr(), B, C, _lib.P2C_CLS_BINARY if binary else 0,
                                                  out_scores.data_ptr(), out_targets.data_ptr(), offset, cap, _stream()),
                       'p2c_rank_scores')
        return
    with torch.no_grad():
        x, t = logits.detach().float(), targets.long()
        out_scores[offset:offset + B] = torch.sigmoid(x)[:, None] if binary else torch.softmax(x, dim=-1)
        K = 2 if binary else C
        out_targets[offset:offset + B] = torch.where((t >= 0) & (t < K), t, torch.full_like(t, -1)).to(torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# weight / bias gradient of a dense layer over many rows (K12)
# ----------------------------------------------------------------------------------------------------------------------
GRAD_SINKS = False      # inside ``grad_sinks(True)`` (the flat trainer's step): weight gradients may be ADDED straight into an
                        # existing ``param.grad``


class grad_sinks:
    """Context of one trainer's step: while it is active ``DenseFunction`` / the LSTM ops add their weight gradients
    straight into ``param.grad`` (views of the trainer's flat gradient buffer) and return none to autograd. Outside of it
    -- other models in the process, ``torch.autograd.grad``, parameter hooks -- autograd receives the gradients as usual."""

    def __init__(self, on: bool = True):
        self.on = bool(on)

    def __enter__(self):
        global GRAD_SINKS
        self._prev, GRAD_SINKS = GRAD_SINKS, self.on
        return self

    def __exit__(self, *exc):
        global GRAD_SINKS
        GRAD_SINKS = self._prev
        return False



def _sink(p: Tensor) -> Optional[Tensor]:
    """``p.grad`` if gradients may be accumulated into it directly (same result as returning the gradient to autograd, minus
    the temporary and the per-parameter accumulate launch; parameter hooks do not fire)."""
    g = p.grad if (GRAD_SINKS and p.is_leaf) else None
    return g if (g is not None and g.is_cuda and g.dtype == torch.float32 and g.stride(-1) == 1) else None


def _group_sinks(*params: Optional[Tensor]) -> List[Optional[Tensor]]:
    """The sinks of parameters whose gradients leave through one launch, i.e. under one accumulate flag (``None``: a parameter
    the layer does not have). Either every parameter of the group has a sink or none is used: all ``None`` then."""
    sinks = [None if p is None else _sink(p) for p in params]
    if any(s is None for p, s in zip(params, sinks) if p is not None):
        sinks = [None] * len(params)
    return sinks


def _grad_target(sink: Optional[Tensor], param: Tensor) -> Tuple[Tensor, Optional[Tensor]]:
    """(the tensor a backward kernel writes the gradient of ``param`` to, what goes back to autograd): the sink, added into, and
    ``None``; or a fresh tensor, both times."""
    if sink is not None:
        return sink, None
    g = torch.empty_like(param)
    return g, g


def _atb_no_rows(M: int, N: int, device, bias: bool, out: Optional[Tensor], bias_out: Optional[Tensor],
                 bias_out2: Optional[Tensor], accumulate: bool) -> Tuple[Tensor, Optional[Tensor]]:
    """What p2c_atb leaves for K = 0, without a launch (a tensor without elements has no address to hand over): an empty sum
    is zero, so an output that is overwritten becomes zeros and one that is added into stays as it is. The flags are those of
    ``atb``: ``out`` is added into under ``accumulate``, the bias vectors only if ``bias_out`` was given as well."""
    if out is None:
        out = torch.zeros(M, N, dtype=torch.float32, device=device)
    elif not accumulate:
        out.zero_()
    if not bias:
        return out, None
    keep_bias = accumulate and bias_out is not None
    if bias_out is None:
        bias_out = torch.zeros(M, dtype=torch.float32, device=device)
    elif not keep_bias:
        bias_out.zero_()
    if bias_out2 is not None and not keep_bias:
        bias_out2.zero_()
    return out, bias_out


def atb(a: Tensor, b: Tensor, bias: bool = False, out: Optional[Tensor] = None, bias_out: Optional[Tensor] = None,
        accumulate: bool = False, a_scale: Optional[Tensor] = None, rows_per_scale: int = 1) -> Tuple[Tensor, Optional[Tensor]]:
    """(a^T b, column sums of a) for a (K, M), b (K, N) -- the dW / db of ``y = x W^T + b`` from dY = a and X = b -- in one
    launch (p2c_atb). Rows may be strided views (row pitch = stride(0), unit column stride). ``a_scale``: row k of a is
    multiplied by ``a_scale[k // rows_per_scale]`` as it is read. K = 0 is answered on the host (``_atb_no_rows``)."""
    lib = _lib.lib()
    a, b = (t if (t.is_cuda and t.dtype == torch.float32 and t.stride(-1) == 1) else _require_device(t, 'operand') for t in (a, b))
    K, M, N = a.shape[0], a.shape[1], b.shape[1]
    if b.shape[0] != K:
        raise RuntimeError('atb: row counts differ')
    a_scale = None if a_scale is None else _require_device(a_scale, 'a_scale')       # the kernel reads it with unit stride
    if K == 0:
        return _atb_no_rows(M, N, a.device, bias, out, bias_out, None, accumulate)
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    flags = (1 if accumulate else 0) | (2 if (accumulate and bias_out is not None) else 0)   # a fresh bias vector is overwritten
    if bias and bias_out is None:
        bias_out = torch.empty(M, dtype=torch.float32, device=a.device)
    ws = torch.empty(lib.p2c_atb_workspace_floats(K, M, N, int(bias)), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.p2c_atb_scaled(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), K, M, N, out.data_ptr(), out.stride(0),
                                      _ptr(bias_out) if bias else None, flags, _ptr(a_scale), int(rows_per_scale),
                                      ws.data_ptr(), _stream()), 'p2c_atb')
    return out, (bias_out if bias else None)


def atb_group(problems: Sequence[dict]) -> list:
    """Up to 8 ``atb`` problems behind one launch pair (p2c_atb_group). Each problem: dict(a=(K,M), b=(K,N), out=None,
    accumulate=False, bias=False, bias_out=None, bias_out2=None); returns [(out, bias_out), ...] like ``atb``. ``bias_out2``
    receives the same column sums as ``bias_out`` (the two bias vectors of an LSTM layer)."""
    lib = _lib.lib()
    n = len(problems)
    if n == 0:
        return []
    if n > 8:
        return atb_group(problems[:8]) + atb_group(problems[8:])
    if any(pr['a'].shape[0] == 0 for pr in problems):           # no rows: zeros (or an untouched accumulator), no launch
        live = [pr for pr in problems if pr['a'].shape[0] > 0]
        done = iter(atb_group(live))
        results = []
        for pr in problems:
            if pr['a'].shape[0] > 0:
                results.append(next(done))
                continue
            if pr['b'].shape[0] != 0:
                raise RuntimeError('atb_group: row counts differ')
            out = pr.get('out')
            results.append(_atb_no_rows(pr['a'].shape[1], pr['b'].shape[1], pr['a'].device, bool(pr.get('bias', False)), out,
                                        pr.get('bias_out'), pr.get('bias_out2'),
                                        bool(pr.get('accumulate', False)) and out is not None))
        return results
    arr = (_lib.AtbProblem * n)()
    keep, results = [], []
    for q, pr in zip(arr, problems):
        a, b = (t if (t.is_cuda and t.dtype == torch.float32 and t.stride(-1) == 1) else _require_device(t, 'operand')
                for t in (pr['a'], pr['b']))
        K, M, N = a.shape[0], a.shape[1], b.shape[1]
        if b.shape[0] != K:
            raise RuntimeError('atb_group: row counts differ')
        out, acc = pr.get('out'), bool(pr.get('accumulate', False))
        if out is None:
            out, acc = torch.empty(M, N, dtype=torch.float32, device=a.device), False
        bias, bias_out, bias_out2 = bool(pr.get('bias', False)), pr.get('bias_out'), pr.get('bias_out2')
        flags = (1 if acc else 0) | (2 if (acc and bias_out is not None) else 0)
        if bias and bias_out is None:
            bias_out = torch.empty(M, dtype=torch.float32, device=a.device)
        q.a, q.a_stride, q.b, q.b_stride, q.K, q.M, q.N = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), K, M, N
        q.out, q.out_stride, q.flags = out.data_ptr(), out.stride(0), flags
        q.bias_out = _ptr(bias_out) if bias else None
        q.bias_out2 = _ptr(bias_out2) if (bias and bias_out2 is not None) else None
        keep.append((a, b, out, bias_out, bias_out2))
        results.append((out, bias_out if bias else None))
    dev = keep[0][0].device
    ws = torch.empty(max(1, lib.p2c_atb_group_workspace_floats(arr, n)), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.p2c_atb_group(arr, n, ws.data_ptr(), _stream()), 'p2c_atb_group')
    return results


def _check_out(t: Tensor, shape: tuple, device, what: str) -> None:
    """An output the kernel writes in place: the given shape, float32 on the operands' device, unit inner stride (a 1-D output
    dense) -- anything else would be written past or beside the tensor."""
    if (tuple(t.shape) != shape or t.dtype != torch.float32 or t.device != device or t.stride(-1) != 1
            or (t.ndim == 2 and t.stride(0) < shape[1])):
        raise RuntimeError(f'{what} should be a float32 {shape} tensor on {device} with unit inner stride, got {tuple(t.shape)} '
                           f'{t.dtype} on {t.device} with strides {t.stride()}')


def gemm(a: Tensor, b: Tensor, trans_b: bool, bias: Optional[Tensor] = None, act: int = 0, aux: Optional[Tensor] = None,
         aux_out: Optional[Tensor] = None, row_scale: Optional[Tensor] = None, rows_per_scale: int = 1,
         residual: Optional[Tensor] = None, out: Optional[Tensor] = None, drop_state: Optional[Tensor] = None,
         drop_p: float = 0.0, drop_site: int = 0) -> Tensor:
    """K16 (csrc/p2c_gemm.hip): ``out = epilogue(a @ (b.T if trans_b else b))`` on fp32 MFMA, 2-D row-major operands with unit
    inner stride. Epilogue order: + bias, act (1: GELU, storing the pre-activation in ``aux_out``; 2: times gelu'(``aux``);
    3: ReLU times the hashed dropout mask of site ``drop_site`` of ``drop_state`` / (1 - ``drop_p``); 4: times
    [``aux`` > 0] / (1 - ``drop_p``), aux = act 3's output), times ``row_scale[row // rows_per_scale]``, + ``residual``."""
    a, b = _require_device(a, 'a'), _require_device(b, 'b')
    if a.ndim != 2 or b.ndim != 2 or a.stride(1) != 1 or b.stride(1) != 1:
        raise RuntimeError('gemm: 2-D operands with unit inner stride expected')
    M, K = a.shape
    N = b.shape[0] if trans_b else b.shape[1]
    if (b.shape[1] if trans_b else b.shape[0]) != K:
        raise RuntimeError(f'gemm: inner dimensions differ: {tuple(a.shape)} x {tuple(b.shape)} (trans_b={trans_b})')
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    _check_out(out, (M, N), a.device, 'gemm: out')
    if bias is not None:
        bias = _require_device(bias, 'bias')
        if tuple(bias.shape) != (N,):
            raise RuntimeError(f'gemm: bias should hold {N} floats, got {tuple(bias.shape)}')
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.trans_b = M, N, K, int(bool(trans_b))
    d.a, d.lda, d.b, d.ldb, d.c, d.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0)
    d.bias = _ptr(bias)
    d.act, d.rows_per_scale = int(act), int(rows_per_scale)
    for t, name in ((aux, 'aux'), (aux_out, 'aux_out')):
        if t is not None and (tuple(t.shape) != (M, N) or t.stride(1) != 1):
            raise RuntimeError(f'gemm: {name} should be ({M}, {N}) with unit inner stride')
    d.aux, d.aux_out = _ptr(aux), _ptr(aux_out)
    d.ldaux = (aux if aux is not None else aux_out).stride(0) if (aux is not None or aux_out is not None) else 0
    if row_scale is not None and row_scale.numel() * rows_per_scale < M:
        raise RuntimeError('gemm: row_scale is too short')
    row_scale = None if row_scale is None else _require_device(row_scale, 'row_scale')       # (a local: a copy outlives the launch)
    d.row_scale = _ptr(row_scale)
    if residual is not None and (tuple(residual.shape) != (M, N) or residual.stride(1) != 1):
        raise RuntimeError(f'gemm: residual should be ({M}, {N}) with unit inner stride')
    d.residual, d.ldr = _ptr(residual), (residual.stride(0) if residual is not None else 0)
    d.drop_state, d.drop_p, d.drop_site = _ptr(drop_state), float(drop_p), int(drop_site)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().p2c_gemm(ctypes.byref(d), _stream()), 'p2c_gemm')
    return out


def gemm_tn(a: Tensor, b: Tensor, out: Optional[Tensor] = None, accumulate: bool = False, bias: bool = False,
            bias_out: Optional[Tensor] = None, a_scale: Optional[Tensor] = None, rows_per_scale: int = 1):
    """K16, TN form (p2c_gemm_tn): ``out (+)= a^T b`` for a (K, M), b (K, N) with K = rows >> M, N -- the weight gradient of a
    wide layer; K is split over workgroups and the slabs are added in a fixed order (bitwise reproducible). ``a_scale``: row k
    of a times ``a_scale[k // rows_per_scale]``; ``bias``: also the column sums of the scaled a (written to / added into
    ``bias_out``). Returns out, or (out, bias_out) with ``bias``."""
    a, b = _require_device(a, 'a'), _require_device(b, 'b')
    if a.ndim != 2 or b.ndim != 2 or a.stride(1) != 1 or b.stride(1) != 1 or a.shape[0] != b.shape[0]:
        raise RuntimeError('gemm_tn: (K, M) and (K, N) operands with unit inner stride expected')
    K, M, N = a.shape[0], a.shape[1], b.shape[1]
    a_scale = None if a_scale is None else _require_device(a_scale, 'a_scale')       # the kernel reads it with unit stride
    if out is None:
        out, accumulate = torch.empty(M, N, dtype=torch.float32, device=a.device), False
    _check_out(out, (M, N), a.device, 'gemm_tn: out')
    flags = (1 if accumulate else 0) | (2 if (bias and bias_out is not None and accumulate) else 0)
    if bias and bias_out is None:
        bias_out = torch.empty(M, dtype=torch.float32, device=a.device)
    if bias:
        _check_out(bias_out, (M,), a.device, 'gemm_tn: bias_out')
    lib = _lib.lib()
    ws = torch.empty(max(1, lib.p2c_gemm_tn_workspace_floats(M, N, K)), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(lib.p2c_gemm_tn(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), M, N, K,
                                   flags, _ptr(a_scale), int(rows_per_scale), _ptr(bias_out) if bias else None,
                                   ws.data_ptr(), _stream()), 'p2c_gemm_tn')
    return (out, bias_out) if bias else out


WIDE_LAYER = 128      # layers with both feature counts above this take the MFMA TN GEMM (K16) for dW ...
LONG_ROWS = 65536     # ... and so do layers with >= 64 outputs over this many rows (PoseTransformer's spatial blocks: 96 x 32 from
                      # 546 624 rows: 189 -> 68 us, 64 x 32: 117 -> 65; K12's extra column of ones doubles its tiles when the
                      # input width is a multiple of 32). 32 x 32 and 32 x 64 stay with K12 (68 / 81 us against 64 / 95)


def weight_grad(gy: Tensor, x: Tensor, w: Tensor, b: Optional[Tensor], scale: Optional[Tensor] = None, rows_per_scale: int = 1):
    """(dW, db) of y = (x W^T + b) * scale[row // rows_per_scale] from dY (rows, out) and X (rows, in): the factor is applied
    to dY's rows as they are read, db comes out of the same pass. Inside ``grad_sinks`` both are ADDED straight into
    ``w.grad`` / ``b.grad`` and (None, None) is returned to autograd."""
    sw, sb = _group_sinks(w, b)                    # one accumulate flag for both
    fn = gemm_tn if (gy.shape[0] > 0 and ((gy.shape[1] > WIDE_LAYER and x.shape[1] > WIDE_LAYER) or (gy.shape[0] >= LONG_ROWS and gy.shape[1] >= 64))) else atb
    res = fn(gy, x, bias=b is not None, out=sw, bias_out=sb, accumulate=sw is not None, a_scale=scale,
             rows_per_scale=rows_per_scale)
    gw, gb = res if isinstance(res, tuple) else (res, None)
    return (None if sw is not None else gw), (None if (b is None or sb is not None) else gb)


class DenseFunction(torch.autograd.Function):
    """y = (x W^T + b) * scale[row // rows_per_scale] + residual over (rows, in): K16 forward and input gradient (the scale --
    a per-sample stochastic-depth factor -- and the residual ride in the GEMM epilogues), K12 (p2c_atb) for the weight + bias
    gradient."""

    @staticmethod
    def forward(ctx, x, w, b, scale, rows_per_scale, residual):
        ctx.save_for_backward(x, w, scale)
        ctx.bias, ctx.rows_per_scale, ctx.has_residual = b, rows_per_scale, residual is not None
        return gemm(x, w, True, bias=b, row_scale=scale, rows_per_scale=rows_per_scale, residual=residual)

    @staticmethod
    def backward(ctx, gy):
        x, w, scale = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gemm(gy, w, False, row_scale=scale, rows_per_scale=ctx.rows_per_scale) if ctx.needs_input_grad[0] else None
        gw, gb = weight_grad(gy, x, w, ctx.bias, scale, ctx.rows_per_scale)
        return gx, gw, gb, None, None, (gy if ctx.has_residual else None)


def dense(x: Tensor, w: Tensor, b: Optional[Tensor], scale: Optional[Tensor] = None, rows_per_scale: int = 1,
          residual: Optional[Tensor] = None) -> Tensor:
    """``torch.nn.functional.linear`` for 2-D x on the device (K16 + K12), optionally followed by a per-sample factor and a
    residual add in the same launch; host tensors / other dtypes take the framework ops."""
    if (x.is_cuda and x.dtype == torch.float32 and x.ndim == 2 and x.stride(1) == 1 and w.is_cuda and w.dtype == torch.float32
            and w.stride(1) == 1 and not torch.is_autocast_enabled()):
        return DenseFunction.apply(x, w, b, scale, rows_per_scale, None if residual is None else residual.contiguous())
    y = torch.nn.functional.linear(x, w, b)
    if scale is not None:
        y = (y.view(scale.numel(), -1) * scale.view(-1, 1)).view_as(y)
    return y if residual is None else y + residual


class MlpFunction(torch.autograd.Function):
    """y = (gelu(x W1^T + b1) W2^T + b2) * scale[row // rows_per_scale] + residual -- the feed-forward half of a transformer block
    as two K16 launches forward (the first stores the pre-activation z beside gelu(z)) and two backward: d z comes out of the
    second layer's input-gradient GEMM with gelu'(z) and the scale applied in its epilogue; weight gradients through K12."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, scale, rows_per_scale, residual):
        z = torch.empty(x.shape[0], w1.shape[0], dtype=torch.float32, device=x.device)
        a = gemm(x, w1, True, bias=b1, act=1, aux_out=z)
        y = gemm(a, w2, True, bias=b2, row_scale=scale, rows_per_scale=rows_per_scale, residual=residual)
        ctx.save_for_backward(x, w1, w2, z, a, scale)
        ctx.rows_per_scale, ctx.has_residual, ctx.b1, ctx.b2 = rows_per_scale, residual is not None, b1, b2
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w1, w2, z, a, scale = ctx.saved_tensors
        gy = gy.contiguous()
        dz = gemm(gy, w2, False, act=2, aux=z, row_scale=scale, rows_per_scale=ctx.rows_per_scale)
        gw2, gb2 = weight_grad(gy, a, w2, ctx.b2, scale, ctx.rows_per_scale)
        gw1, gb1 = weight_grad(dz, x, w1, ctx.b1)
        gx = gemm(dz, w1, False) if ctx.needs_input_grad[0] else None
        return gx, gw1, gb1, gw2, gb2, None, None, (gy if ctx.has_residual else None)


def mlp_gelu(x: Tensor, w1: Tensor, b1: Tensor, w2: Tensor, b2: Tensor, scale: Optional[Tensor] = None,
             rows_per_scale: int = 1, residual: Optional[Tensor] = None) -> Tensor:
    return MlpFunction.apply(x, w1, b1, w2, b2, scale, rows_per_scale, None if residual is None else residual.contiguous())


# ----------------------------------------------------------------------------------------------------------------------
# Seq2Seq decoder loop (K7c)
# ----------------------------------------------------------------------------------------------------------------------
DECODER_LOOP_MAX_O = 160      # K7c: O <= 64 on both tilings, 64 < O <= 160 on the 16-clip tiling (csrc/p2c_s2s_wide.h)


def decoder_loop_supported(hidden_size: int, num_layers: int, output_size: int) -> bool:
    """The shapes of the single-launch decoder loop (K7c): hidden size 64, two layers, 1 <= O <= 160 (pose_2d 52, absolute_loc 78,
    pose_changes / relative_rot 156). ``hidden_size = 128`` and O > 160 (absolute_loc_rot: 234) are not built: those decoders take
    the per-step path. 64 < O <= 160 is opt-in: ``P2C_DECODER_WIDE=1`` (read at every call) takes the fused loop, unset or ``0`` keeps
    the per-step path -- no timing of the two arms on an MI355X is recorded yet (tools/bench_decoder_wide.py alternates them), and
    the default moves only with such a table in DESIGN.md."""
    if hidden_size != 64 or num_layers != 2 or not 1 <= output_size <= DECODER_LOOP_MAX_O:
        return False
    if output_size > 64:
        return os.environ.get('P2C_DECODER_WIDE', '0') == '1'
    return True


class DecoderLoopFunction(torch.autograd.Function):
    """out (T,B,O): T applications of fc(LSTM_2layers(x; frozen encoder state)) to its own output, one launch.

    k0, k1 (B,4H) = b_ih_l + b_hh_l + hidden_l W_hh_l^T; c0, c1 (B,H) = encoder cell states; drop = (T,B,H) dropout mask
    (already divided by the keep probability) or None."""

    @staticmethod
    def forward(ctx, k0, c0, k1, c1, w_ih0, w_ih1, w_fc, b_fc, drop, T: int):
        lib = _lib.lib()
        k0, c0, k1, c1, w_ih0, w_ih1, w_fc, b_fc = (_require_device(t, n) for t, n in (
            (k0, 'k0'), (c0, 'c0'), (k1, 'k1'), (c1, 'c1'), (w_ih0, 'weight_ih_l0'), (w_ih1, 'weight_ih_l1'),
            (w_fc, 'fc_out.weight'), (b_fc, 'fc_out.bias')))
        drop = None if drop is None else _require_device(drop, 'dropout mask')
        B, H = c0.shape
        O = w_fc.shape[0]
        if not decoder_loop_supported(H, 2, O) or w_ih0.shape != (4 * H, O) or w_ih1.shape != (4 * H, H) \
                or w_fc.shape != (O, H) or k0.shape != (B, 4 * H) or k1.shape != (B, 4 * H) or c1.shape != (B, H):
            raise RuntimeError('decoder loop: unsupported or inconsistent shapes')
        f32 = dict(dtype=torch.float32, device=c0.device)
        out = torch.empty(T, B, O, **f32)
        acts0, acts1 = torch.empty(T, B, 4 * H, **f32), torch.empty(T, B, 4 * H, **f32)
        h0d, h1 = torch.empty(T, B, H, **f32), torch.empty(T, B, H, **f32)
        d = _lib.DecoderDesc()
        d.T, d.B, d.H, d.O = T, B, H, O
        d.k0, d.c0, d.k1, d.c1 = k0.data_ptr(), c0.data_ptr(), k1.data_ptr(), c1.data_ptr()
        d.w_ih0, d.w_ih1, d.w_fc, d.b_fc = w_ih0.data_ptr(), w_ih1.data_ptr(), w_fc.data_ptr(), b_fc.data_ptr()
        d.drop = _ptr(drop)
        d.out, d.acts0, d.acts1, d.h0d, d.h1 = (t.data_ptr() for t in (out, acts0, acts1, h0d, h1))
        with torch.cuda.device(c0.device):
            _lib.check(lib.p2c_decoder_fwd(ctypes.byref(d), _stream()), 'p2c_decoder_fwd')
        ctx.save_for_backward(k0, c0, k1, c1, w_ih0, w_ih1, w_fc, b_fc, drop, out, acts0, acts1, h0d, h1)
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.lib()
        k0, c0, k1, c1, w_ih0, w_ih1, w_fc, b_fc, drop, out, acts0, acts1, h0d, h1 = ctx.saved_tensors
        T, B, O = out.shape
        H = c0.shape[1]
        g_out = _require_device(g_out, 'grad out')
        f32 = dict(dtype=torch.float32, device=out.device)
        gg0, gg1 = torch.empty(T, B, 4 * H, **f32), torch.empty(T, B, 4 * H, **f32)
        gtot, gc0, gc1 = torch.empty(T, B, O, **f32), torch.empty(B, H, **f32), torch.empty(B, H, **f32)
        d = _lib.DecoderDesc()
        d.T, d.B, d.H, d.O = T, B, H, O
        d.k0, d.c0, d.k1, d.c1 = k0.data_ptr(), c0.data_ptr(), k1.data_ptr(), c1.data_ptr()
        d.w_ih0, d.w_ih1, d.w_fc, d.b_fc = w_ih0.data_ptr(), w_ih1.data_ptr(), w_fc.data_ptr(), b_fc.data_ptr()
        d.drop = _ptr(drop)
        d.acts0, d.acts1, d.h0d, d.h1 = acts0.data_ptr(), acts1.data_ptr(), h0d.data_ptr(), h1.data_ptr()
        d.g_out, d.g_gates0, d.g_gates1, d.g_outtot = g_out.data_ptr(), gg0.data_ptr(), gg1.data_ptr(), gtot.data_ptr()
        d.g_c0, d.g_c1 = gc0.data_ptr(), gc1.data_ptr()
        with torch.cuda.device(out.device):
            _lib.check(lib.p2c_decoder_bwd(ctypes.byref(d), _stream()), 'p2c_decoder_bwd')
        # weight gradients: dense reductions over all (t, b) at once -- library GEMMs
        g0 = gg0.view(T * B, 4 * H)
        s0, s1 = _sink(w_ih0), _sink(w_ih1)
        sf, sb = _group_sinks(w_fc, b_fc)     # weight and bias of fc_out leave through one launch
        g_w_ih0 = (atb(g0[B:], out[:-1].reshape(-1, O), out=s0, accumulate=s0 is not None)[0] if T > 1
                   else torch.zeros_like(w_ih0))                                            # x_0 = <sos> = 0
        g_w_ih1 = atb(gg1.view(T * B, 4 * H), h0d.view(T * B, H), out=s1, accumulate=s1 is not None)[0]
        g_w_fc, g_b_fc = atb(gtot.view(T * B, O), h1.view(T * B, H), bias=True, out=sf, bias_out=sb, accumulate=sf is not None)
        return (gg0.sum(0), gc0, gg1.sum(0), gc1, None if (s0 is not None and T > 1) else g_w_ih0,
                None if s1 is not None else g_w_ih1, None if sf is not None else g_w_fc, None if sb is not None else g_b_fc,
                None, None)


def decoder_loop(k0: Tensor, c0: Tensor, k1: Tensor, c1: Tensor, w_ih0: Tensor, w_ih1: Tensor, w_fc: Tensor, b_fc: Tensor,
                 T: int, drop: Optional[Tensor] = None) -> Tensor:
    _prefer_rocblas_once()
    return DecoderLoopFunction.apply(k0, c0, k1, c1, w_ih0, w_ih1, w_fc, b_fc, drop, T)


class DecoderStackFunction(torch.autograd.Function):
    """The whole decoder of Seq2Seq for one clip batch, frame-invariant terms included: from the encoder state
    (hidden, cell (2,B,H)) and the decoder parameters to the model output (B,T,O) in ONE launch, and back in one launch plus
    one grouped weight-gradient launch pair. Compared with ``decoder_loop`` behind framework ops this drops, per step, the
    two k_l GEMMs + bias adds forward and their five-launch backwards, the select / stack copies around the state tensors,
    the two sum_t reductions and the two permute copies of the output and its gradient (cfg3: ~30 launches)."""

    @staticmethod
    def forward(ctx, hidden, cell, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, w_fc, b_fc, drop, T: int,
                force=None, target=None):
        lib = _lib.lib()
        names = ('hidden', 'cell', 'weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0', 'weight_ih_l1', 'weight_hh_l1',
                 'bias_ih_l1', 'bias_hh_l1', 'fc_out.weight', 'fc_out.bias')
        hidden, cell, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, w_fc, b_fc = (
            _require_device(t, n) for t, n in zip((hidden, cell, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, w_fc, b_fc), names))
        hashed = drop if isinstance(drop, tuple) else None         # (state, p, site): the mask is drawn inside the kernels
        drop = None if (drop is None or hashed is not None) else _require_device(drop, 'dropout mask')
        L, B, H = hidden.shape
        O = w_fc.shape[0]
        G = 4 * H
        if L != 2 or cell.shape != hidden.shape or not decoder_loop_supported(H, 2, O) or w_ih0.shape != (G, O) \
                or w_ih1.shape != (G, H) or w_hh0.shape != (G, H) or w_hh1.shape != (G, H) or w_fc.shape != (O, H):
            raise RuntimeError('decoder stack: unsupported or inconsistent shapes')
        f32 = dict(dtype=torch.float32, device=hidden.device)
        out, out_bt = torch.empty(T, B, O, **f32), torch.empty(B, T, O, **f32)
        acts0, acts1 = torch.empty(T, B, G, **f32), torch.empty(T, B, G, **f32)
        h0d, h1 = torch.empty(T, B, H, **f32), torch.empty(T, B, H, **f32)
        kw = torch.empty(2, B, G, **f32)                                 # scratch of the 16-clip tiling (B > 4096)
        d = _lib.DecoderDesc()
        d.T, d.B, d.H, d.O = T, B, H, O
        d.hid0, d.hid1, d.c0, d.c1 = hidden[0].data_ptr(), hidden[1].data_ptr(), cell[0].data_ptr(), cell[1].data_ptr()
        d.w_ih0, d.w_ih1, d.w_fc, d.b_fc = w_ih0.data_ptr(), w_ih1.data_ptr(), w_fc.data_ptr(), b_fc.data_ptr()
        d.w_hh0, d.w_hh1, d.b0a, d.b0b, d.b1a, d.b1b = (t.data_ptr() for t in (w_hh0, w_hh1, b_ih0, b_hh0, b_ih1, b_hh1))
        if kw is not None:
            d.kw0, d.kw1 = kw[0].data_ptr(), kw[1].data_ptr()
        d.drop = _ptr(drop)
        if hashed is not None:
            d.drop_state, d.drop_p, d.drop_site = hashed[0].data_ptr(), float(hashed[1]), int(hashed[2])
        ctx.hashed = hashed
        if force is not None:            # teacher forcing: (T,B) 0 / 1 flags and the (T,B,O) target frames
            force = _require_device(force, 'force flags').contiguous()
            target = _require_device(target, 'forced targets').contiguous()
            if tuple(force.shape) != (T, B) or tuple(target.shape) != (T, B, O):
                raise RuntimeError(f'decoder stack: force should be ({T}, {B}) and target ({T}, {B}, {O})')
            d.force, d.target = force.data_ptr(), target.data_ptr()
        d.out, d.out_bt, d.acts0, d.acts1, d.h0d, d.h1 = (t.data_ptr() for t in (out, out_bt, acts0, acts1, h0d, h1))
        with torch.cuda.device(hidden.device):
            _lib.check(lib.p2c_decoder_fwd(ctypes.byref(d), _stream()), 'p2c_decoder_fwd')
        ctx.save_for_backward(hidden, cell, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, w_fc, b_fc, drop,
                              out, acts0, acts1, h0d, h1, force, target)
        return out_bt

    @staticmethod
    def backward(ctx, g_out_bt):
        lib = _lib.lib()
        (hidden, cell, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, w_fc, b_fc, drop,
         out, acts0, acts1, h0d, h1, force, target) = ctx.saved_tensors
        T, B, O = out.shape
        H = hidden.shape[2]
        G = 4 * H
        g_out_bt = _require_device(g_out_bt, 'grad out')
        f32 = dict(dtype=torch.float32, device=out.device)
        gg0, gg1, gtot = torch.empty(T, B, G, **f32), torch.empty(T, B, G, **f32), torch.empty(T, B, O, **f32)
        g_hidden, g_cell, g_k = torch.empty(2, B, H, **f32), torch.empty(2, B, H, **f32), torch.empty(2, B, G, **f32)
        d = _lib.DecoderDesc()
        d.T, d.B, d.H, d.O = T, B, H, O
        d.hid0, d.hid1, d.c0, d.c1 = hidden[0].data_ptr(), hidden[1].data_ptr(), cell[0].data_ptr(), cell[1].data_ptr()
        d.w_ih0, d.w_ih1, d.w_fc, d.b_fc = w_ih0.data_ptr(), w_ih1.data_ptr(), w_fc.data_ptr(), b_fc.data_ptr()
        d.w_hh0, d.w_hh1 = w_hh0.data_ptr(), w_hh1.data_ptr()
        d.drop = _ptr(drop)
        if ctx.hashed is not None:
            d.drop_state, d.drop_p, d.drop_site = ctx.hashed[0].data_ptr(), float(ctx.hashed[1]), int(ctx.hashed[2])
        d.acts0, d.acts1, d.h0d, d.h1 = acts0.data_ptr(), acts1.data_ptr(), h0d.data_ptr(), h1.data_ptr()
        d.g_out, d.g_out_bt = g_out_bt.data_ptr(), 1
        if force is not None:
            d.force, d.target = force.data_ptr(), target.data_ptr()
        d.g_gates0, d.g_gates1, d.g_outtot = gg0.data_ptr(), gg1.data_ptr(), gtot.data_ptr()
        d.g_c0, d.g_c1, d.g_hid0, d.g_hid1 = g_cell[0].data_ptr(), g_cell[1].data_ptr(), g_hidden[0].data_ptr(), g_hidden[1].data_ptr()
        d.g_k0, d.g_k1 = g_k[0].data_ptr(), g_k[1].data_ptr()
        with torch.cuda.device(out.device):
            _lib.check(lib.p2c_decoder_bwd(ctypes.byref(d), _stream()), 'p2c_decoder_bwd')
        # all weight / bias gradients: five contractions over rows, one grouped launch pair
        params = dict(w_ih0=w_ih0, w_hh0=w_hh0, b_ih0=b_ih0, b_hh0=b_hh0, w_ih1=w_ih1, w_hh1=w_hh1, b_ih1=b_ih1, b_hh1=b_hh1,
                      w_fc=w_fc, b_fc=b_fc)
        sinks = {}
        for group in (('w_ih0',), ('w_ih1',), ('w_hh0', 'b_ih0', 'b_hh0'), ('w_hh1', 'b_ih1', 'b_hh1'), ('w_fc', 'b_fc')):
            sinks.update(zip(group, _group_sinks(*(params[n] for n in group))))   # a weight and its biases leave through one problem

        def prob(a, b, w, bias=None, bias2=None, with_bias=False):
            return dict(a=a, b=b, out=sinks[w], accumulate=sinks[w] is not None, bias=with_bias,
                        bias_out=sinks[bias] if bias else None, bias_out2=sinks[bias2] if bias2 else None)
        problems, order = [], []
        if T > 1:                                            # x_0 = <sos> = 0: the first frame adds nothing to dW_ih0
            problems.append(prob(gg0.view(T * B, G)[B:], out[:-1].reshape(-1, O), 'w_ih0')), order.append('w_ih0')
        problems.append(prob(gg1.view(T * B, G), h0d.view(T * B, H), 'w_ih1')), order.append('w_ih1')
        problems.append(prob(gtot.view(T * B, O), h1.view(T * B, H), 'w_fc', 'b_fc', None, True)), order.append('w_fc')
        problems.append(prob(g_k[0], hidden[0], 'w_hh0', 'b_ih0', 'b_hh0', True)), order.append('w_hh0')
        problems.append(prob(g_k[1], hidden[1], 'w_hh1', 'b_ih1', 'b_hh1', True)), order.append('w_hh1')
        res = dict(zip(order, atb_group(problems)))
        ret = {n: None for n in sinks}                       # what autograd still has to accumulate itself
        for w, biases in (('w_ih0', ()), ('w_ih1', ()), ('w_fc', ('b_fc',)), ('w_hh0', ('b_ih0', 'b_hh0')), ('w_hh1', ('b_ih1', 'b_hh1'))):
            if sinks[w] is None:
                ret[w] = res[w][0] if w in res else torch.zeros_like(w_ih0)
                for bn in biases:
                    ret[bn] = res[w][1]
        return (g_hidden, g_cell, ret['w_ih0'], ret['w_hh0'], ret['b_ih0'], ret['b_hh0'], ret['w_ih1'], ret['w_hh1'],
                ret['b_ih1'], ret['b_hh1'], ret['w_fc'], ret['b_fc'], None, None, None, None)


def decoder_stack(hidden: Tensor, cell: Tensor, rnn, fc, T: int, drop: Optional[Tensor] = None, force: Optional[Tensor] = None,
                  target: Optional[Tensor] = None) -> Tensor:
    """Seq2Seq's decoder (2-layer ``nn.LSTM`` ``rnn`` with biases + ``nn.Linear`` ``fc``) unrolled over T frames from the
    encoder state; returns the frames batch-first, (B,T,O). Teacher forcing: where ``force`` (T,B) is non-zero the frame IS
    ``target`` (T,B,O) -- output and next input -- and passes no gradient (reference seq2seq.py:283-288)."""
    _prefer_rocblas_once()
    return DecoderStackFunction.apply(hidden, cell, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0,
                                      rnn.weight_ih_l1, rnn.weight_hh_l1, rnn.bias_ih_l1, rnn.bias_hh_l1, fc.weight, fc.bias,
                                      drop, T, None if force is None else force.to(torch.float32),
                                      None if force is None else target.detach())


def encoder_stack_supported(rnn, x: Tensor, flip: bool = False) -> bool:
    return (rnn.num_layers == 2 and rnn.bias and not rnn.bidirectional and rnn.proj_size == 0 and lstm_supported(rnn.hidden_size)
            and not flip and x.is_cuda and x.dtype == torch.float32 and not x.requires_grad      # (x is data: no d x is formed)
            and x.shape[0] <= 2 ** 20 and x.shape[0] * x.shape[1] * 4 * rnn.hidden_size * 4 < 2 ** 31)


class EncoderStackFunction(torch.autograd.Function):
    """Seq2Seq's encoder -- a 2-layer ``nn.LSTM`` from the zero state over a BATCH-FIRST input -- as an explicit launch
    sequence: (hidden, cell) (2,B,H) from x (B,T,I), layer 0's input map (w_in (4H,I), up to two bias vectors) and the other
    LSTM parameters. Forward: projection GEMM of the batch-first rows (no permute copy; the recurrence reads gx batch-first
    and adds the biases itself), recurrence, inter-layer dropout, projection GEMM, recurrence; the final states are written
    straight into the stacked (2,B,H) tensors. Backward: two recurrence launches around one input-gradient GEMM and the
    dropout backward, then ALL weight / bias gradients in one grouped launch pair. Compared with the same layers as separate
    autograd nodes: no stack / select copies, no bias adds and their backwards, no zero-filled placeholder gradients, four
    weight-gradient launch pairs less."""

    @staticmethod
    def forward(ctx, x, w_in, b_in_a, b_in_b, w_hh0, w_ih1, w_hh1, b_ih1, b_hh1, p_drop: float, train: bool, drop_state=None):
        lib = _lib.lib()
        ctx.set_materialize_grads(False)
        x = _require_device(x, 'x')
        w_in, w_hh0, w_ih1, w_hh1, b_ih1, b_hh1 = (_require_device(t, n) for t, n in (
            (w_in, 'layer-0 input map'), (w_hh0, 'weight_hh_l0'), (w_ih1, 'weight_ih_l1'), (w_hh1, 'weight_hh_l1'),
            (b_ih1, 'bias_ih_l1'), (b_hh1, 'bias_hh_l1')))
        b_in_a = None if b_in_a is None else _require_device(b_in_a, 'layer-0 bias')
        b_in_b = None if b_in_b is None else _require_device(b_in_b, 'layer-0 bias')
        B, T, I = x.shape
        H = w_hh0.shape[1]
        G = 4 * H
        if w_in.shape != (G, I) or w_hh0.shape != (G, H) or w_ih1.shape != (G, H) or w_hh1.shape != (G, H) or not lstm_supported(H):
            raise RuntimeError('encoder stack: unsupported or inconsistent shapes')
        f32 = dict(dtype=torch.float32, device=x.device)
        hidden, cell = torch.empty(2, B, H, **f32), torch.empty(2, B, H, **f32)
        out0, out1 = torch.empty(T, B, H, **f32), torch.empty(T, B, H, **f32)
        acts0, acts1 = torch.empty(T, B, G, **f32), torch.empty(T, B, G, **f32)
        cs0, cs1 = torch.empty(T, B, H, **f32), torch.empty(T, B, H, **f32)

        hashed = bool(train and p_drop > 0 and drop_state is not None)      # the inter-layer mask is drawn inside the recurrence

        def rec(gx, gx_bt, ba, bb, w_hh, out, acts, cs, k, out_drop=None):
            d = _lib.LstmDesc()
            d.T, d.B, d.H, d.gx_bt = T, B, H, int(gx_bt)
            d.gx, d.w_hh, d.bias_a, d.bias_b = gx.data_ptr(), w_hh.data_ptr(), _ptr(ba), _ptr(bb)
            d.out, d.hT, d.cT, d.acts, d.cs = out.data_ptr(), hidden[k].data_ptr(), cell[k].data_ptr(), acts.data_ptr(), cs.data_ptr()
            if out_drop is not None:
                d.out_drop, d.drop_state, d.drop_p, d.drop_site = out_drop.data_ptr(), drop_state.data_ptr(), float(p_drop), 0
            _lib.check(lib.p2c_lstm_rec_fwd(ctypes.byref(d), _stream()), 'p2c_lstm_rec_fwd')

        with torch.cuda.device(x.device):
            gx0 = gemm(x.view(B * T, I), w_in, True)                       # (B,T,4H) rows, bias-free (K16)
            mask = None
            x1 = out0
            if hashed:
                x1 = torch.empty(T, B, H, **f32)
            rec(gx0, True, b_in_a, b_in_b, w_hh0, out0, acts0, cs0, 0, x1 if hashed else None)
            if train and p_drop > 0 and not hashed:
                x1, mask = torch.native_dropout(out0, p_drop, True)
            gx1 = gemm(x1.view(T * B, H), w_ih1, True)
            rec(gx1, False, b_ih1, b_hh1, w_hh1, out1, acts1, cs1, 1)
        ctx.save_for_backward(x, w_in, b_in_a, b_in_b, w_hh0, w_ih1, w_hh1, b_ih1, b_hh1, out0, x1, mask, out1, acts0, cs0, acts1, cs1)
        ctx.p_drop = p_drop
        ctx.drop_state = drop_state if hashed else None
        return hidden, cell

    @staticmethod
    def backward(ctx, g_hidden, g_cell):
        lib = _lib.lib()
        x, w_in, b_in_a, b_in_b, w_hh0, w_ih1, w_hh1, b_ih1, b_hh1, out0, x1, mask, out1, acts0, cs0, acts1, cs1 = ctx.saved_tensors
        B, T, I = x.shape
        H = w_hh0.shape[1]
        G = 4 * H
        f32 = dict(dtype=torch.float32, device=x.device)
        g_hidden = None if g_hidden is None else _require_device(g_hidden, 'grad hidden')
        g_cell = None if g_cell is None else _require_device(g_cell, 'grad cell')
        g_gx1, g_gx0, g_gx0_bt = torch.empty(T, B, G, **f32), torch.empty(T, B, G, **f32), torch.empty(B, T, G, **f32)

        def rec(w_hh, acts, cs, g_out, k, g_gx, g_gx_bt=None):
            d = _lib.LstmDesc()
            d.T, d.B, d.H = T, B, H
            d.w_hh, d.acts, d.cs = w_hh.data_ptr(), acts.data_ptr(), cs.data_ptr()
            d.g_out = _ptr(g_out)
            if k == 0 and ctx.drop_state is not None:                     # g_out is the gradient of the DROPPED output
                d.drop_state, d.drop_p, d.drop_site = ctx.drop_state.data_ptr(), float(ctx.p_drop), 0
            d.g_hT = None if g_hidden is None else g_hidden[k].data_ptr()
            d.g_cT = None if g_cell is None else g_cell[k].data_ptr()
            d.g_gx, d.g_gx_bt = g_gx.data_ptr(), _ptr(g_gx_bt)
            _lib.check(lib.p2c_lstm_rec_bwd(ctypes.byref(d), _stream()), 'p2c_lstm_rec_bwd')

        with torch.cuda.device(x.device):
            rec(w_hh1, acts1, cs1, None, 1, g_gx1)
            g_x1 = gemm(g_gx1.view(T * B, G), w_ih1, False).view(T, B, H)
            if mask is not None:
                g_x1 = torch.ops.aten.native_dropout_backward(g_x1, mask, 1.0 / (1.0 - ctx.p_drop))
            rec(w_hh0, acts0, cs0, g_x1, 0, g_gx0, g_gx0_bt)
        names = ('w_in', 'b_in_a', 'b_in_b', 'w_hh0', 'w_ih1', 'w_hh1', 'b_ih1', 'b_hh1')
        params = dict(zip(names, (w_in, b_in_a, b_in_b, w_hh0, w_ih1, w_hh1, b_ih1, b_hh1)))
        sinks = {}
        for group in (('w_in', 'b_in_a', 'b_in_b'), ('w_hh0',), ('w_ih1', 'b_ih1', 'b_hh1'), ('w_hh1',)):
            sinks.update(zip(group, _group_sinks(*(params[n] for n in group))))

        def prob(a, b, w, bias=None, bias2=None):
            return dict(a=a, b=b, out=sinks[w], accumulate=sinks[w] is not None, bias=bias is not None,
                        bias_out=sinks[bias] if bias else None, bias_out2=sinks[bias2] if bias2 else None)
        res = atb_group([
            prob(g_gx1[1:].reshape(-1, G), out1[:-1].reshape(-1, H), 'w_hh1'),
            prob(g_gx1.view(T * B, G), x1.reshape(T * B, H), 'w_ih1', 'b_ih1', 'b_hh1'),
            prob(g_gx0[1:].reshape(-1, G), out0[:-1].reshape(-1, H), 'w_hh0'),
            prob(g_gx0_bt.view(B * T, G), x.view(B * T, I), 'w_in', 'b_in_a' if b_in_a is not None else None,
                 'b_in_b' if (b_in_a is not None and b_in_b is not None) else None)])
        g = {n: None for n in names}
        if sinks['w_hh1'] is None:
            g['w_hh1'] = res[0][0]
        if sinks['w_ih1'] is None:
            g['w_ih1'], g['b_ih1'], g['b_hh1'] = res[1][0], res[1][1], res[1][1]
        if sinks['w_hh0'] is None:
            g['w_hh0'] = res[2][0]
        if sinks['w_in'] is None:
            g['w_in'] = res[3][0]
            g['b_in_a'] = res[3][1] if b_in_a is not None else None
            g['b_in_b'] = res[3][1] if (b_in_a is not None and b_in_b is not None) else None
        return (None, g['w_in'], g['b_in_a'], g['b_in_b'], g['w_hh0'], g['w_ih1'], g['w_hh1'], g['b_ih1'], g['b_hh1'], None, None, None)


def encoder_stack(x: Tensor, rnn, input_map=None, drop_state: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(hidden, cell) (2,B,H) of the 2-layer ``nn.LSTM`` ``rnn`` run from the zero state over the batch-first x (B,T,I).
    ``input_map`` = (weight (4H,I), bias (4H)) replaces layer 0's (weight_ih_l0, bias_ih_l0 + bias_hh_l0). ``drop_state``
    (``dropout_state``): the inter-layer dropout mask is drawn inside the recurrence kernels (site 0 of that state)."""
    _prefer_rocblas_once()
    if input_map is not None:
        w_in, b_a, b_b = input_map[0], input_map[1], None
    else:
        w_in, b_a, b_b = rnn.weight_ih_l0, rnn.bias_ih_l0, rnn.bias_hh_l0
    return EncoderStackFunction.apply(x, w_in, b_a, b_b, rnn.weight_hh_l0, rnn.weight_ih_l1, rnn.weight_hh_l1,
                                      rnn.bias_ih_l1, rnn.bias_hh_l1, float(rnn.dropout), bool(rnn.training), drop_state)


# ----------------------------------------------------------------------------------------------------------------------
# multi-head self-attention over short token sequences (K14, csrc/p2c_attn.hip)
# ----------------------------------------------------------------------------------------------------------------------
def small_attention_supported(N: int, heads: int, head_dim: int) -> bool:
    return bool(_lib.lib().p2c_attn_small_supported(int(N), int(heads), int(head_dim)))


def _aligned16(t: Tensor) -> Tensor:
    """K14 and K15 move 16 bytes at a time and refuse other pointers: a dense view that starts inside a larger buffer (``buf[1:]``
    passes ``contiguous()`` unchanged) is copied into an allocation of its own."""
    return t if t.data_ptr() % 16 == 0 else t.clone()


class SmallAttentionFunction(torch.autograd.Function):
    """out (S,N,heads*head_dim) = concat_h softmax(scale q_h k_h^T) v_h from qkv (S,N,3,heads,head_dim): one launch forward, one
    backward (probabilities recomputed), one workgroup per sequence."""

    @staticmethod
    def forward(ctx, qkv, scale: float):
        lib = _lib.lib()
        qkv = _aligned16(_require_device(qkv, 'qkv'))
        S, N, three, Hh, D = qkv.shape
        if three != 3 or not small_attention_supported(N, Hh, D):
            raise RuntimeError(f'small attention: unsupported shape {tuple(qkv.shape)}')
        out = torch.empty(S, N, Hh * D, dtype=torch.float32, device=qkv.device)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.p2c_attn_small_fwd(qkv.data_ptr(), out.data_ptr(), float(scale), S, N, Hh, D, _stream()), 'p2c_attn_small_fwd')
        ctx.save_for_backward(qkv)
        ctx.scale = float(scale)
        return out

    @staticmethod
    def backward(ctx, g_out):
        lib = _lib.lib()
        (qkv,) = ctx.saved_tensors
        S, N, _, Hh, D = qkv.shape
        g_out = _aligned16(_require_device(g_out, 'grad out'))
        g_qkv = torch.empty_like(qkv)
        with torch.cuda.device(qkv.device):
            _lib.check(lib.p2c_attn_small_bwd(qkv.data_ptr(), g_out.data_ptr(), g_qkv.data_ptr(), ctx.scale, S, N, Hh, D, _stream()),
                       'p2c_attn_small_bwd')
        return g_qkv, None


def small_attention(qkv: Tensor, scale: float) -> Tensor:
    return SmallAttentionFunction.apply(qkv, scale)


# ----------------------------------------------------------------------------------------------------------------------
# LayerNorm over many short rows (K15, csrc/p2c_norm.hip)
# ----------------------------------------------------------------------------------------------------------------------
def layer_norm_supported(x: Tensor, D: int) -> bool:
    return bool(x.is_cuda and x.dtype == torch.float32 and x.shape[-1] == D and _lib.lib().p2c_layernorm_supported(int(D)))


class LayerNormFunction(torch.autograd.Function):
    """torch.nn.functional.layer_norm over the last dimension, one launch forward, two backward (p2c_layernorm_*). Inside the
    trainer's ``grad_sinks`` context the gamma / beta gradients are added straight into their ``.grad``."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps: float):
        x, weight, bias = _aligned16(_require_device(x, 'x')), _require_device(weight, 'weight'), _require_device(bias, 'bias')
        D = x.shape[-1]
        with torch.cuda.device(x.device):
            y, stats = _ln_fwd(x.view(x.numel() // D, D), weight, bias, eps)
        ctx.save_for_backward(x, weight, bias, stats)
        return y.view_as(x)

    @staticmethod
    def backward(ctx, gy):
        x, weight, bias, stats = ctx.saved_tensors
        D = x.shape[-1]
        gy = _aligned16(_require_device(gy, 'grad'))
        with torch.cuda.device(x.device):
            gx, gw, gb = _ln_bwd(x.view(x.numel() // D, D), weight, bias, stats, gy, None)
        return gx.view_as(x), gw, gb, None


def layer_norm(x: Tensor, weight: Tensor, bias: Tensor, eps: float) -> Tensor:
    return LayerNormFunction.apply(x, weight, bias, eps)


# ----------------------------------------------------------------------------------------------------------------------
# BatchNorm1d + ReLU + dropout (+ residual) over (N, C) rows (K19, csrc/p2c_bnorm.hip)
# ----------------------------------------------------------------------------------------------------------------------
BNORM_MAX_ELEMENTS = 1 << 31        # the hashed dropout stream indexes elements with 32 bits
_BN_WARNED = set()


class BatchNormActFunction(torch.autograd.Function):
    """z = relu(batch_norm(y)) * mask / (1 - p) [+ residual] for y (N, C): three launches forward in training (slab statistics,
    their fixed-order combine + the running-statistics update, the element-wise pass), one in eval; three backward. Saved: y,
    mean and rstd only -- the ReLU gate and the dropout mask (hashed, site ``site`` of ``drop_state``) are recomputed. Inside the
    trainer's ``grad_sinks`` context the gamma / beta gradients are added straight into their ``.grad``."""

    @staticmethod
    def forward(ctx, y, weight, bias, residual, running_mean, running_var, training: bool, momentum: float, eps: float,
                p: float, drop_state, site: int, relu: bool):
        lib = _lib.lib()
        N, C = y.shape
        f32 = dict(dtype=torch.float32, device=y.device)
        z, mean, rstd = torch.empty_like(y), torch.empty(C, **f32), torch.empty(C, **f32)
        ws = torch.empty(max(1, lib.p2c_bnorm_workspace_floats(N, C)), **f32)
        d = _lib.BnormDesc()
        d.N, d.C, d.training, d.relu, d.eps, d.momentum = N, C, int(training), int(relu), float(eps), float(momentum)
        d.y, d.gamma, d.beta, d.residual = y.data_ptr(), weight.data_ptr(), bias.data_ptr(), _ptr(residual)
        d.z, d.mean, d.rstd = z.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        d.running_mean, d.running_var = _ptr(running_mean), _ptr(running_var)
        use_drop = training and p > 0 and drop_state is not None
        d.drop_state, d.drop_p, d.drop_site = (drop_state.data_ptr() if use_drop else None), float(p if use_drop else 0.), int(site)
        with torch.cuda.device(y.device):
            _lib.check(lib.p2c_bnorm_fwd(ctypes.byref(d), ws.data_ptr(), _stream()), 'p2c_bnorm_fwd')
        ctx.save_for_backward(y, weight, bias, mean, rstd)
        ctx.drop_state, ctx.cfg = (drop_state if use_drop else None), (bool(training), float(p if use_drop else 0.), int(site),
                                                                         bool(relu), residual is not None)
        return z

    @staticmethod
    def backward(ctx, gz):
        lib = _lib.lib()
        y, weight, bias, mean, rstd = ctx.saved_tensors
        training, p, site, relu, has_residual = ctx.cfg
        N, C = y.shape
        gz = _require_device(gz, 'grad')
        gy = torch.empty_like(y)
        sw, sb = _group_sinks(weight, bias)
        (gw, ret_w), (gb, ret_b) = _grad_target(sw, weight), _grad_target(sb, bias)
        ws = torch.empty(max(1, lib.p2c_bnorm_workspace_floats(N, C)), dtype=torch.float32, device=y.device)
        d = _lib.BnormDesc()
        d.N, d.C, d.training, d.relu, d.accumulate = N, C, int(training), int(relu), int(sw is not None)
        d.y, d.gamma, d.beta, d.mean, d.rstd = y.data_ptr(), weight.data_ptr(), bias.data_ptr(), mean.data_ptr(), rstd.data_ptr()
        d.g_z, d.g_y, d.g_gamma, d.g_beta = gz.data_ptr(), gy.data_ptr(), gw.data_ptr(), gb.data_ptr()
        d.drop_state, d.drop_p, d.drop_site = _ptr(ctx.drop_state), p, site
        with torch.cuda.device(y.device):
            _lib.check(lib.p2c_bnorm_bwd(ctypes.byref(d), ws.data_ptr(), _stream()), 'p2c_bnorm_bwd')
        return (gy, ret_w, ret_b, gz if has_residual else None,
                None, None, None, None, None, None, None, None, None)


def batch_norm_act_supported(y: Tensor, bn: torch.nn.BatchNorm1d) -> bool:
    """The inputs K19 covers: a contiguous fp32 (N, C) device tensor outside autocast, an affine BatchNorm1d that tracks running
    statistics with a float momentum, and N C < 2^31 (N C beyond that takes the framework ops, with a warning)."""
    if not (y.is_cuda and y.dtype == torch.float32 and y.ndim == 2 and y.is_contiguous() and not torch.is_autocast_enabled()
            and isinstance(bn.momentum, float) and bn.track_running_stats and bn.affine and bn.weight.is_cuda
            and bn.weight.dtype == torch.float32 and bn.running_mean is not None and y.shape[1] == bn.num_features):
        return False
    if y.shape[0] * y.shape[1] >= BNORM_MAX_ELEMENTS:
        key = tuple(y.shape)
        if key not in _BN_WARNED:
            _BN_WARNED.add(key)
            warnings.warn(f'batch_norm_act: {tuple(y.shape)} has 2^31 elements or more (the fused kernel indexes them with 32 bits): '
                          f'this layer runs on the framework ops', RuntimeWarning, stacklevel=3)
        return False
    return True


def batch_norm_act(y: Tensor, bn: torch.nn.BatchNorm1d, p: float, drop_state: Optional[Tensor], site: int,
                   residual: Optional[Tensor] = None, relu: bool = True) -> Tensor:
    """``dropout(relu(bn(y)), p) [+ residual]`` for 2-D y, with the BatchNorm1d module's own parameters and buffers (running
    statistics and ``num_batches_tracked`` advance as in ``bn(y)``). On the device this is K19, whose dropout mask is drawn from
    ``drop_state`` (``dropout_state``; ``site`` tells the layers that share it apart); ``drop_state=None`` with p > 0 -- the
    framework's dropout asked for (P2C_TORCH_DROPOUT=1) -- and every input K19 does not cover take the framework ops."""
    training = bn.training
    kernel_drop = not (training and p > 0) or drop_state is not None
    if kernel_drop and batch_norm_act_supported(y, bn):
        if training and y.shape[0] < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size(y.shape)}')
        if residual is not None:
            residual = residual.contiguous()
        z = BatchNormActFunction.apply(y, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var, training,
                                       bn.momentum, bn.eps, float(p), drop_state, int(site), bool(relu))
        if training:
            bn.num_batches_tracked.add_(1)
        return z
    z = bn(y)
    if relu:
        z = torch.relu(z)
    if training and p > 0:
        z = torch.nn.functional.dropout(z, p, True)
    return z if residual is None else z + residual


# ----------------------------------------------------------------------------------------------------------------------
# broadcast parameters without framework reductions in the backward
# ----------------------------------------------------------------------------------------------------------------------
# Why these exist: on this stack (PyTorch 2.10 / ROCm 7.0) a captured step whose backward holds one of ATen's multi-block
# reductions -- the gradient of any parameter that is broadcast over the batch: position embeddings, a frame-mean weight, a bias
# added outside a GEMM -- replays WRONG once the allocator has handed out other memory in between: the reduction's scratch
# buffers come from the raw allocator API and do not stay with the graph's private pool (tools/graph_reduce_repro.py: pure
# torch, errors of 1e3..1e7 from the second replay on; found because the NaN-filled-torch.empty audit of tests/conftest.py made
# cfg5's replayed step diverge from the eager one). Inside a trainer's captured step every reduction over rows therefore runs
# through the build's own kernels (K12: fixed-order column sums).
def column_sums(a: Tensor) -> Tensor:
    """Sum of the rows of a 2-D device tensor (K12's bias column: fixed summation order, no framework reduction)."""
    a = _require_device(a, 'rows')
    return atb(a, a[:, :1], bias=True)[1]


class AddRowParameterFunction(torch.autograd.Function):
    """x (rows..., F) + p (broadcast over the leading dimensions, F = p.numel()): the gradient of p is the column sum of the
    upstream gradient through K12, added straight into p.grad inside ``grad_sinks``."""

    @staticmethod
    def forward(ctx, x, p):                 # x (rows, F), p (F)
        ctx.p = p
        return x + p

    @staticmethod
    def backward(ctx, g):
        p = ctx.p
        g = g.contiguous()
        gp = None
        if ctx.needs_input_grad[1]:
            sums = column_sums(g)
            sink = _sink(p)
            if sink is not None:
                sink.view(-1).add_(sums)
            else:
                gp = sums.view_as(p)
        return (g if ctx.needs_input_grad[0] else None), gp


def add_row_parameter(x: Tensor, p: Tensor) -> Tensor:
    """``x + p`` for a learned p of shape (1, ...) that spans the trailing dimensions of x (position embeddings, a bias outside
    a GEMM)."""
    tail = tuple(p.shape[1:]) if (p.ndim > 1 and p.shape[0] == 1) else tuple(p.shape)
    if (x.is_cuda and x.dtype == torch.float32 and p.dtype == torch.float32 and x.numel() > 0 and len(tail) >= 1
            and x.ndim > len(tail) and tuple(x.shape[x.ndim - len(tail):]) == tail):
        F = p.numel()
        return AddRowParameterFunction.apply(x.reshape(-1, F), p.view(F)).view_as(x)
    return x + p


class FrameMeanFunction(torch.autograd.Function):
    """out (B, C) = sum_f w[f] x[b, f, c] + bias: the learned weighted mean over the F frame tokens (PoseTransformer's
    ``weighted_mean`` = Conv1d(F, 1, kernel 1)). Backward: d x = g (x) w element-wise; d w[f] = <g, x[:, f, :]> and d bias = sum g as
    K12 contractions over the B * C (row, channel) pairs."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.b = b
        B, F, C = x.shape
        if C % 4 == 0 and x.data_ptr() % 16 == 0:
            out = torch.empty(B, C, dtype=torch.float32, device=x.device)
            wc, bc = w.contiguous(), b.contiguous()                          # (locals: a copy outlives the launch)
            with torch.cuda.device(x.device):
                _lib.check(_lib.lib().p2c_frame_mean_fwd(x.data_ptr(), wc.data_ptr(), bc.data_ptr(),
                                                         out.data_ptr(), B, F, C, _stream()), 'p2c_frame_mean_fwd')
            return out
        return (x * w.view(1, -1, 1)).sum(1) + b.view(1, 1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        b = ctx.b
        g = g.contiguous()
        B, F, C = x.shape
        gx = g.unsqueeze(1) * w.view(1, -1, 1) if ctx.needs_input_grad[0] else None
        rows = x.permute(0, 2, 1).reshape(B * C, F)                       # (b, c) pairs x frames
        gcol = g.reshape(B * C, 1)
        gw, _ = atb(rows, gcol)                                            # (F, 1)
        gb = column_sums(gcol)                                             # (1,)
        out_w, out_b = gw.view_as(w), gb.view_as(b)
        sw, sb = _group_sinks(w, b)
        if sw is not None:
            sw.view(-1).add_(gw.view(-1)), sb.view(-1).add_(gb.view(-1))
            out_w = out_b = None
        return gx, out_w, out_b


def frame_mean(x: Tensor, w: Tensor, b: Tensor) -> Tensor:
    if x.is_cuda and x.dtype == torch.float32 and x.ndim == 3 and w.numel() == x.shape[1] and b.numel() == 1:
        return FrameMeanFunction.apply(x.contiguous(), w.reshape(-1), b.reshape(-1))
    return (x * w.view(1, -1, 1)).sum(1) + b


# ----------------------------------------------------------------------------------------------------------------------
# one pre-norm transformer block as ONE autograd node (K15 + K16 + K14 + K12 launches only)
# ----------------------------------------------------------------------------------------------------------------------
def _ln_fwd(x2d: Tensor, w: Tensor, b: Tensor, eps: float):
    lib = _lib.lib()
    rows, D = x2d.shape
    y = torch.empty_like(x2d)
    stats = torch.empty(2, rows, dtype=torch.float32, device=x2d.device)
    _lib.check(lib.p2c_layernorm_fwd(x2d.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), stats[0].data_ptr(),
                                     stats[1].data_ptr(), rows, D, float(eps), _stream()), 'p2c_layernorm_fwd')
    return y, stats


def _ln_bwd(x2d: Tensor, w: Tensor, b: Tensor, stats: Tensor, gy: Tensor, gx_add: Optional[Tensor]):
    """(gx [+ gx_add], g_gamma, g_beta); the parameter gradients go straight into their sinks when both exist (-> None)."""
    lib = _lib.lib()
    rows, D = x2d.shape
    gx = torch.empty_like(x2d)
    sw, sb = _group_sinks(w, b)
    (gw, ret_w), (gb, ret_b) = _grad_target(sw, w), _grad_target(sb, b)
    ws = torch.empty(max(1, lib.p2c_layernorm_workspace_floats(rows, D)), dtype=torch.float32, device=x2d.device)
    _lib.check(lib.p2c_layernorm_bwd(x2d.data_ptr(), w.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), gy.data_ptr(),
                                     _ptr(gx_add), gx.data_ptr(), gw.data_ptr(), gb.data_ptr(), int(sw is not None),
                                     ws.data_ptr(), rows, D, _stream()), 'p2c_layernorm_bwd')
    return gx, ret_w, ret_b


def transformer_block_supported(x: Tensor, heads: int) -> bool:
    if not (x.is_cuda and x.dtype == torch.float32 and x.ndim == 3 and not torch.is_autocast_enabled()):
        return False
    S, N, C = x.shape
    return (C % heads == 0 and layer_norm_supported(x, C) and small_attention_supported(N, heads, C // heads)
            and x.numel() * 4 < 2 ** 40)


class TransformerBlockFunction(torch.autograd.Function):
    """One pre-norm transformer block (PoseTransformer's ``Block``: x1 = x + f1 * proj(attention(norm1(x))),
    x2 = x1 + f2 * fc2(gelu(fc1(norm2(x1)))), f1 / f2 per-sample stochastic-depth factors or None) over x (S, N, C) as a single
    autograd node: 7 launches forward (2 LayerNorm, 4 GEMMs with bias / GELU / factor / residual in their epilogues, attention),
    and backward 4 input-gradient GEMMs (gelu' and the factors in the epilogues), 4 weight + bias gradient launch pairs (the
    factor applied to dY as it is read, results added straight into the parameter sinks inside ``grad_sinks``), attention, and
    2 LayerNorm backward pairs that also ADD the gradient arriving over the residual connection. As separate autograd nodes the
    same block cost one framework ``add`` per residual fan-in, one ``mul`` per factor, one ``sum`` per wide bias gradient and
    one accumulate per parameter on top of these."""

    @staticmethod
    def forward(ctx, x, f1, f2, heads, scale, eps1, eps2, n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2):
        x = _aligned16(_require_device(x, 'x'))
        S, N, C = x.shape
        rows = S * N
        x2 = x.view(rows, C)
        with torch.cuda.device(x.device):
            h1, st1 = _ln_fwd(x2, n1w, n1b, eps1)
            qkv = gemm(h1, wqkv, True, bias=bqkv)
            att = torch.empty(rows, C, dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().p2c_attn_small_fwd(qkv.data_ptr(), att.data_ptr(), float(scale), S, N, heads, C // heads,
                                                     _stream()), 'p2c_attn_small_fwd')
            x1 = gemm(att, wproj, True, bias=bproj, row_scale=f1, rows_per_scale=N, residual=x2)
            h2, st2 = _ln_fwd(x1, n2w, n2b, eps2)
            z = torch.empty(rows, w1.shape[0], dtype=torch.float32, device=x.device)
            a = gemm(h2, w1, True, bias=b1, act=1, aux_out=z)
            out = gemm(a, w2, True, bias=b2, row_scale=f2, rows_per_scale=N, residual=x1)
        ctx.save_for_backward(x2, h1, st1, qkv, att, x1, h2, st2, z, a, f1, f2)
        ctx.params = (n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2)
        ctx.geom = (S, N, C, heads, float(scale))
        return out.view(S, N, C)

    @staticmethod
    def backward(ctx, g):
        x2, h1, st1, qkv, att, x1, h2, st2, z, a, f1, f2 = ctx.saved_tensors
        n1w, n1b, wqkv, bqkv, wproj, bproj, n2w, n2b, w1, b1, w2, b2 = ctx.params
        S, N, C, heads, scale = ctx.geom
        g = _aligned16(_require_device(g, 'grad')).view(S * N, C)
        with torch.cuda.device(g.device):
            dz = gemm(g, w2, False, act=2, aux=z, row_scale=f2, rows_per_scale=N)
            gw2, gb2 = weight_grad(g, a, w2, b2, f2, N)
            gw1, gb1 = weight_grad(dz, h2, w1, b1)
            dh2 = gemm(dz, w1, False)
            g1, gn2w, gn2b = _ln_bwd(x1, n2w, n2b, st2, dh2, g)                 # + the gradient over the second residual
            datt = gemm(g1, wproj, False, row_scale=f1, rows_per_scale=N)
            gwp, gbp = weight_grad(g1, att, wproj, bproj, f1, N)
            dqkv = torch.empty_like(qkv)
            _lib.check(_lib.lib().p2c_attn_small_bwd(qkv.data_ptr(), datt.data_ptr(), dqkv.data_ptr(), scale, S, N, heads,
                                                     C // heads, _stream()), 'p2c_attn_small_bwd')
            gwq, gbq = weight_grad(dqkv, h1, wqkv, bqkv)
            gx = None
            if ctx.needs_input_grad[0]:
                dh1 = gemm(dqkv, wqkv, False)
                gx, gn1w, gn1b = _ln_bwd(x2, n1w, n1b, st1, dh1, g1)             # + the gradient over the first residual
                gx = gx.view(S, N, C)
            else:                                                                # (x is data: only the LayerNorm parameters)
                dh1 = gemm(dqkv, wqkv, False)
                _, gn1w, gn1b = _ln_bwd(x2, n1w, n1b, st1, dh1, None)
        return (gx, None, None, None, None, None, None, gn1w, gn1b, gwq, gbq, gwp, gbp, gn2w, gn2b, gw1, gb1, gw2, gb2)


def transformer_block(x, f1, f2, heads, scale, norm1, qkv, proj, norm2, fc1, fc2) -> Tensor:
    """``TransformerBlockFunction`` from the block's nn modules (LayerNorm / Linear with biases)."""
    return TransformerBlockFunction.apply(x, f1, f2, int(heads), float(scale), float(norm1.eps), float(norm2.eps), norm1.weight,
                                          norm1.bias, qkv.weight, qkv.bias, proj.weight, proj.bias, norm2.weight, norm2.bias,
                                          fc1.weight, fc1.bias, fc2.weight, fc2.bias)


# ----------------------------------------------------------------------------------------------------------------------
# grouped copy: a new batch into the static buffers of a captured step (one launch)
# ----------------------------------------------------------------------------------------------------------------------
class GroupCopy:
    """``dst[i].copy_(src[i])`` for a FIXED list of contiguous destination tensors in one launch (p2c_copy_group). The
    destination table is built once; a call costs one pointer per source and one ctypes call. Sources must be contiguous
    device tensors of the destinations' shapes and dtypes (the caller checks shapes; non-contiguous sources are made so)."""
    MAX = 24

    def __init__(self, dst: Sequence[Tensor]):
        self.dst = list(dst)
        if not self.dst or any((not t.is_cuda) or (not t.is_contiguous()) for t in self.dst):
            raise RuntimeError('GroupCopy: destinations must be contiguous device tensors')
        self.device = self.dst[0].device
        self.chunks = [range(i, min(i + self.MAX, len(self.dst))) for i in range(0, len(self.dst), self.MAX)]
        self._tables = []
        for ch in self.chunks:
            n = len(ch)
            d = (ctypes.c_void_p * n)(*[self.dst[i].data_ptr() for i in ch])
            b = (ctypes.c_int64 * n)(*[self.dst[i].numel() * self.dst[i].element_size() for i in ch])
            self._tables.append((d, b, (ctypes.c_void_p * n)()))

    def __call__(self, src: Sequence[Tensor]):
        lib = _lib.lib()
        stream = _stream()
        keep = []
        with torch.cuda.device(self.device):
            for ch, (d, b, s) in zip(self.chunks, self._tables):
                for k, i in enumerate(ch):
                    t = src[i]
                    if not t.is_contiguous():
                        t = t.contiguous()
                        keep.append(t)
                    s[k] = t.data_ptr()
                _lib.check(lib.p2c_copy_group(s, d, b, len(ch), stream), 'p2c_copy_group')


# ----------------------------------------------------------------------------------------------------------------------
# one post-norm nn.TransformerEncoderLayer as ONE autograd node (K16 + K20 + K12 launches only)
# ----------------------------------------------------------------------------------------------------------------------
ENCODER_MAX_TOKENS = 64             # K20a keeps a sequence's N x N probabilities in LDS
ENCODER_MAX_ELEMENTS = 1 << 31      # the hashed dropout stream indexes elements with 32 bits
_ENC_WARNED = set()


def post_norm_encoder_layer_module_ok(layer) -> bool:
    """``layer`` is the layer K20 restates: a batch-first, post-norm ``nn.TransformerEncoderLayer`` with ReLU, biases everywhere,
    one packed in_proj and affine LayerNorms."""
    if not isinstance(layer, torch.nn.TransformerEncoderLayer):
        return False
    sa = layer.self_attn
    return bool(not layer.norm_first and getattr(layer, 'activation_relu_or_gelu', 0) == 1 and sa.batch_first
                and sa._qkv_same_embed_dim and sa.in_proj_bias is not None and sa.bias_k is None and not sa.add_zero_attn
                and sa.out_proj.bias is not None and layer.linear1.bias is not None and layer.linear2.bias is not None
                and all(n.weight is not None and n.bias is not None for n in (layer.norm1, layer.norm2))
                and all(t.is_cuda and t.dtype == torch.float32 for t in layer.parameters()))


def post_norm_encoder_layer_supported(B: int, T: int, d: int, heads: int, training: bool, dim_ff: int = 2048) -> bool:
    """The shapes K20 covers: T <= 64 tokens, heads (d / heads) = d <= 256, 2 <= d; with dropout (training) also every mask index
    below 2^31 -- (B T) x dim_ff for the FFN's. (B T) x dim_ff >= 2^31 in training warns once and returns False: the caller runs the
    framework layer."""
    lib = _lib.lib()
    if not (d % heads == 0 and lib.p2c_attn_drop_supported(int(T), int(heads), int(d // heads)) and lib.p2c_postnorm_supported(int(d))):
        return False
    if training and B * T * max(dim_ff, d) >= ENCODER_MAX_ELEMENTS or training and B * heads * T * T >= ENCODER_MAX_ELEMENTS:
        key = (B, T, d, heads, dim_ff)
        if key not in _ENC_WARNED:
            _ENC_WARNED.add(key)
            warnings.warn(f'post_norm_encoder_layer: {B * T} rows x {dim_ff} has 2^31 elements or more (the dropout masks are indexed '
                          f'with 32 bits): this layer runs on the framework ops', RuntimeWarning, stacklevel=3)
        return False
    return True


def _postnorm_fwd(x2d: Tensor, s2d: Tensor, w: Tensor, b: Tensor, eps: float, drop_state, p: float, site: int):
    rows, D = x2d.shape
    z = torch.empty_like(x2d)
    stats = torch.empty(2, rows, dtype=torch.float32, device=x2d.device)
    _lib.check(_lib.lib().p2c_postnorm_fwd(x2d.data_ptr(), s2d.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(),
                                           stats[0].data_ptr(), stats[1].data_ptr(), rows, D, float(eps), _ptr(drop_state),
                                           float(p), int(site), _stream()), 'p2c_postnorm_fwd')
    return z, stats


def _postnorm_bwd(x2d: Tensor, s2d: Tensor, w: Tensor, b: Tensor, stats: Tensor, gz: Tensor, drop_state, p: float, site: int):
    """(g_x, g_s, g_gamma, g_beta); the parameter gradients go straight into their sinks when both exist (-> None)."""
    lib = _lib.lib()
    rows, D = x2d.shape
    gx, gs = torch.empty_like(x2d), torch.empty_like(x2d)
    sw, sb = _group_sinks(w, b)
    (gw, ret_w), (gb, ret_b) = _grad_target(sw, w), _grad_target(sb, b)
    ws = torch.empty(max(1, lib.p2c_postnorm_workspace_floats(rows, D)), dtype=torch.float32, device=x2d.device)
    _lib.check(lib.p2c_postnorm_bwd(x2d.data_ptr(), s2d.data_ptr(), w.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(),
                                    gz.data_ptr(), gx.data_ptr(), gs.data_ptr(), gw.data_ptr(), gb.data_ptr(), int(sw is not None),
                                    ws.data_ptr(), rows, D, _ptr(drop_state), float(p), int(site), _stream()), 'p2c_postnorm_bwd')
    return gx, gs, ret_w, ret_b


def _wide_weight_grad(gy: Tensor, x: Tensor, w: Tensor, b: Tensor):
    """``weight_grad`` on the TN GEMM whatever the widths (the FFN's 2048-wide side is past what K12 tiles)."""
    sw, sb = _group_sinks(w, b)
    gw, gb = gemm_tn(gy, x, out=sw, accumulate=sw is not None, bias=True, bias_out=sb)
    return (None if sw is not None else gw), (None if sb is not None else gb)


class PostNormEncoderLayerFunction(torch.autograd.Function):
    """One post-norm ``nn.TransformerEncoderLayer`` (ReLU, training-mode dropout at four sites) over x (B, T, d) as a single
    autograd node. Forward, 7 launches: in_proj (K16), attention with dropout on the probabilities (K20a), out_proj (K16),
    x1 = LayerNorm1(x + drop(sa)) (K20b), h = drop(relu(linear1(x1))) (K16, act 3), linear2 (K16),
    z = LayerNorm2(x1 + drop(ff)) (K20b). Saved: x, qkv, the attention output, the two pre-residual branch outputs, x1, h and the
    LayerNorm statistics; no mask (the hashed stream redraws them; h > 0 is the FFN's ReLU gate and mask at once). The
    parameter gradients go straight into the trainer's sinks inside ``grad_sinks``."""

    @staticmethod
    def forward(ctx, x, heads, eps1, eps2, probs, drop_state, site, wqkv, bqkv, wo, bo, n1w, n1b, w1, b1, w2, b2, n2w, n2b):
        x = _require_device(x, 'x').contiguous()
        B, T, d = x.shape
        rows, hd = B * T, d // heads
        p_att, p1, p_ff, p2 = probs
        st = lambda p: drop_state if (drop_state is not None and p > 0) else None      # noqa: E731
        x2 = x.view(rows, d)
        scale = 1.0 / float(hd) ** 0.5
        with torch.cuda.device(x.device):
            qkv = gemm(x2, wqkv, True, bias=bqkv)
            att = torch.empty(rows, d, dtype=torch.float32, device=x.device)
            _lib.check(_lib.lib().p2c_attn_drop_fwd(qkv.data_ptr(), att.data_ptr(), scale, B, T, heads, hd, _ptr(st(p_att)),
                                                    float(p_att), int(site), _stream()), 'p2c_attn_drop_fwd')
            s1 = gemm(att, wo, True, bias=bo)
            x1, st1 = _postnorm_fwd(x2, s1, n1w, n1b, eps1, st(p1), p1, site + 1)
            h = gemm(x1, w1, True, bias=b1, act=3, drop_state=st(p_ff), drop_p=p_ff, drop_site=site + 2)
            s2 = gemm(h, w2, True, bias=b2)
            out, st2 = _postnorm_fwd(x1, s2, n2w, n2b, eps2, st(p2), p2, site + 3)
        ctx.save_for_backward(x2, qkv, att, s1, x1, st1, h, s2, st2)
        ctx.params = (wqkv, bqkv, wo, bo, n1w, n1b, w1, b1, w2, b2, n2w, n2b)
        ctx.cfg = (B, T, d, heads, scale, probs, drop_state, site)
        return out.view(B, T, d)

    @staticmethod
    def backward(ctx, g):
        x2, qkv, att, s1, x1, st1, h, s2, st2 = ctx.saved_tensors
        wqkv, bqkv, wo, bo, n1w, n1b, w1, b1, w2, b2, n2w, n2b = ctx.params
        B, T, d, heads, scale, (p_att, p1, p_ff, p2), drop_state, site = ctx.cfg
        st = lambda p: drop_state if (drop_state is not None and p > 0) else None      # noqa: E731
        g = _require_device(g, 'grad').contiguous().view(B * T, d)
        with torch.cuda.device(g.device):
            gx1, gs2, gn2w, gn2b = _postnorm_bwd(x1, s2, n2w, n2b, st2, g, st(p2), p2, site + 3)
            dpre = gemm(gs2, w2, False, act=4, aux=h, drop_p=p_ff)                     # relu' and the FFN mask from h > 0
            gw2, gb2 = _wide_weight_grad(gs2, h, w2, b2)
            gw1, gb1 = _wide_weight_grad(dpre, x1, w1, b1)
            gx1 = gemm(dpre, w1, False, residual=gx1)                                 # + the gradient over the second residual
            gx, gs1, gn1w, gn1b = _postnorm_bwd(x2, s1, n1w, n1b, st1, gx1, st(p1), p1, site + 1)
            gatt = gemm(gs1, wo, False)
            gwo, gbo = weight_grad(gs1, att, wo, bo)
            gqkv = torch.empty_like(qkv)
            _lib.check(_lib.lib().p2c_attn_drop_bwd(qkv.data_ptr(), gatt.data_ptr(), gqkv.data_ptr(), scale, B, T, heads, d // heads,
                                                    _ptr(st(p_att)), float(p_att), int(site), _stream()), 'p2c_attn_drop_bwd')
            gwq, gbq = weight_grad(gqkv, x2, wqkv, bqkv)
            gx = gemm(gqkv, wqkv, False, residual=gx).view(B, T, d) if ctx.needs_input_grad[0] else None
        return (gx, None, None, None, None, None, None, gwq, gbq, gwo, gbo, gn1w, gn1b, gw1, gb1, gw2, gb2, gn2w, gn2b)


def post_norm_encoder_layer(x: Tensor, layer, heads: int, drop_state: Optional[Tensor], site: int) -> Tensor:
    """``layer(x)`` for a post-norm ``nn.TransformerEncoderLayer`` (``post_norm_encoder_layer_module_ok``) over x (B, T, d) on
    the device: ``PostNormEncoderLayerFunction``. In training the four dropout masks come from ``drop_state`` (sites ``site`` ...
    ``site + 3``: attention probabilities, after out_proj, after the ReLU, after linear2); ``drop_state=None`` draws none."""
    sa = layer.self_attn
    training = layer.training
    probs = tuple(float(p) if training else 0.0 for p in (sa.dropout, layer.dropout1.p, layer.dropout.p, layer.dropout2.p))
    if any(p > 0 for p in probs) and drop_state is None:
        raise RuntimeError('post_norm_encoder_layer: dropout is live but no drop_state was given')
    return PostNormEncoderLayerFunction.apply(
        x, int(heads), float(layer.norm1.eps), float(layer.norm2.eps), probs, drop_state, int(site), sa.in_proj_weight,
        sa.in_proj_bias, sa.out_proj.weight, sa.out_proj.bias, layer.norm1.weight, layer.norm1.bias, layer.linear1.weight,
        layer.linear1.bias, layer.linear2.weight, layer.linear2.bias, layer.norm2.weight, layer.norm2.bias)


# ----------------------------------------------------------------------------------------------------------------------
# fused ReLU stack (K21, csrc/p2c_relu_stack.hip): the front end of Seq2SeqFlatEmbeddings
# ----------------------------------------------------------------------------------------------------------------------
def _relu_stack_desc(dims: Sequence[int], B: int = 1, T: int = 1, flip: bool = False):
    d = _lib.ReluStackDesc()
    d.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.dims[i] = int(v)
    d.B, d.T, d.flip = int(B), int(T), int(bool(flip))
    return d


def relu_stack_supported(dims: Sequence[int]) -> bool:
    """Widths K21 covers: 1..5 layers whose zero-padded weight images and tile activations fit the 160 KiB of LDS and whose
    weight gradient is at most 96 16x16 tiles (p2c_relu_stack_supported; the exact rule is in csrc/p2c_relu_stack.hip)."""
    if not 2 <= len(dims) <= _lib.P2C_RELU_STACK_MAX_LAYERS + 1:
        return False
    return bool(_lib.lib().p2c_relu_stack_supported(ctypes.byref(_relu_stack_desc(dims))))


class ReluStackFunction(torch.autograd.Function):
    """y (T,B,dims[L]) = relu(W_{L-1} ... relu(W_0 x + b_0) ... + b_{L-1}) of the batch-first frames x (B,T,dims[0]), written
    sequence-first and time-reversed with ``flip`` -- one launch forward, two backward (K21). The backward recomputes the hidden
    activations and takes the last ReLU's mask from y. x is data: no gradient is formed for it. Inside ``grad_sinks`` the weight
    and bias gradients are ADDED straight into ``param.grad`` (all parameters or none) and None is returned to autograd."""

    @staticmethod
    def forward(ctx, x, flip: bool, n_layers: int, *params):
        lib = _lib.lib()
        x = _require_device(x, 'x')
        weights = [_require_device(p, 'weight') for p in params[:n_layers]]
        biases = [_require_device(p, 'bias') for p in params[n_layers:]]
        if x.ndim != 3:
            raise RuntimeError('relu_stack: x should be (B, T, features)')
        B, T, n0 = x.shape
        dims = [n0] + [w.shape[0] for w in weights]
        for l, (w, b) in enumerate(zip(weights, biases)):
            if tuple(w.shape) != (dims[l + 1], dims[l]) or tuple(b.shape) != (dims[l + 1],):
                raise RuntimeError('relu_stack: layer shapes do not chain')
        desc = _relu_stack_desc(dims, B, T, flip)
        if not lib.p2c_relu_stack_supported(ctypes.byref(desc)):
            raise _lib.P2CError(f'relu_stack: widths {dims} are outside the fused kernel (ops.relu_stack_supported)')
        y = torch.empty(T, B, dims[-1], dtype=torch.float32, device=x.device)
        desc.x, desc.y = x.data_ptr(), y.data_ptr()
        for l in range(n_layers):
            desc.W[l], desc.b[l] = weights[l].data_ptr(), biases[l].data_ptr()
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_relu_stack_fwd(ctypes.byref(desc), _stream()), 'p2c_relu_stack_fwd')
        ctx.save_for_backward(x, y, *weights, *biases)
        ctx.params = params
        ctx.dims, ctx.flip, ctx.n_layers = dims, bool(flip), n_layers
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.lib()
        n = ctx.n_layers
        x, y, *rest = ctx.saved_tensors
        weights, biases = rest[:n], rest[n:]
        gy = _require_device(gy, 'grad')
        B, T = x.shape[:2]
        desc = _relu_stack_desc(ctx.dims, B, T, ctx.flip)
        sinks = _group_sinks(*ctx.params)
        if any(s is None or not s.is_contiguous() for s in sinks):
            sinks = None
        if sinks is not None:
            gws, gbs = sinks[:n], sinks[n:]
        else:
            gws, gbs = [torch.empty_like(w) for w in weights], [torch.empty_like(b) for b in biases]
        desc.x, desc.y, desc.gy, desc.accumulate = x.data_ptr(), y.data_ptr(), gy.data_ptr(), int(sinks is not None)
        for l in range(n):
            desc.W[l], desc.b[l] = weights[l].data_ptr(), biases[l].data_ptr()
            desc.gW[l], desc.gb[l] = gws[l].data_ptr(), gbs[l].data_ptr()
        ws = torch.empty(max(1, lib.p2c_relu_stack_workspace_floats(ctypes.byref(desc))), dtype=torch.float32, device=x.device)
        desc.workspace = ws.data_ptr()
        with torch.cuda.device(x.device):
            _lib.check(lib.p2c_relu_stack_bwd(ctypes.byref(desc), _stream()), 'p2c_relu_stack_bwd')
        if sinks is not None:
            return (None,) * (3 + 2 * n)
        return (None, None, None, *gws, *gbs)


def relu_stack(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], flip: bool = False) -> Tensor:
    """K21: ``relu(Linear_{L-1}(... relu(Linear_0(x))))`` of the batch-first x (B,T,F) as the SEQUENCE-FIRST (T,B,E) tensor an
    LSTM encoder reads, time-reversed with ``flip``. Raises for widths outside ``relu_stack_supported`` -- the caller composes
    those from ``dense_chain``; there is no framework fallback here."""
    if x.requires_grad:
        raise RuntimeError('relu_stack: x is treated as data (no input gradient is formed); use dense_chain for a differentiable input')
    return ReluStackFunction.apply(x, bool(flip), len(weights), *weights, *biases)


class DenseChainFunction(torch.autograd.Function):
    """h_{l+1} = act_l(h_l W_l^T + b_l) over 2-D rows with act_l = ReLU where ``relus[l]``, as K16 launches: forward one GEMM per
    layer with the ReLU in its epilogue (act 3 without a dropout state); backward one input-gradient GEMM per layer with the
    previous layer's ReLU mask in ITS epilogue (act 4, aux = that layer's output) and K12 / K16-TN for the weight and bias
    gradients (``weight_grad``: inside ``grad_sinks`` added straight into ``param.grad``). The layers K8 / K21 do not cover."""

    @staticmethod
    def forward(ctx, x, relus: Tuple[bool, ...], *params):
        n = len(relus)
        weights, biases = params[:n], params[n:]
        hs = [x]
        for l in range(n):
            hs.append(gemm(hs[-1], weights[l], True, bias=biases[l], act=3 if relus[l] else 0))
        ctx.save_for_backward(*hs)
        ctx.params, ctx.relus = params, tuple(bool(r) for r in relus)
        return hs[-1]

    @staticmethod
    def backward(ctx, gy):
        hs, relus = ctx.saved_tensors, ctx.relus
        n = len(relus)
        weights, biases = ctx.params[:n], ctx.params[n:]
        g = gy = _require_device(gy, 'grad')     # (gy keeps a copy alive to the end: no launch below may find one of its operands freed)
        if relus[-1]:                                # no GEMM behind the last layer whose epilogue could carry its mask
            g = torch.ops.aten.threshold_backward(gy, hs[-1], 0.0)
        gws, gbs, gx = [None] * n, [None] * n, None
        for l in range(n - 1, -1, -1):
            gws[l], gbs[l] = weight_grad(g, hs[l], weights[l], biases[l])
            if l > 0:
                g = gemm(g, weights[l], False, act=4 if relus[l - 1] else 0, aux=hs[l] if relus[l - 1] else None)
            elif ctx.needs_input_grad[0]:
                gx = gemm(g, weights[0], False)
        return (gx, None, *gws, *gbs)


def dense_chain(x: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], relus: Sequence[bool]) -> Tensor:
    """A stack of Linear layers over the rows of the 2-D x, layer l followed by ReLU where ``relus[l]`` (K16 + K12, see
    ``DenseChainFunction``). fp32 device tensors only: there is no framework fallback."""
    x = _require_device(x, 'x')
    if x.ndim != 2 or len(weights) != len(biases) or len(weights) != len(relus):
        raise RuntimeError('dense_chain: 2-D x and one weight, bias and ReLU flag per layer expected')
    return DenseChainFunction.apply(x, tuple(relus), *[_require_device(w, 'weight') for w in weights],
                                    *[_require_device(b, 'bias') for b in biases])


# ----------------------------------------------------------------------------------------------------------------------
# pose_changes / cum_pose_changes losses (K27, csrc/p2c_pose_change_loss.hip)
# ----------------------------------------------------------------------------------------------------------------------
def pcl_framework() -> bool:
    """P2C_PCL_FRAMEWORK=1: the two pose-change losses run as tensor ops on the device (the comparison arm of
    tools/bench_pose_change_loss.py)."""
    return os.environ.get('P2C_PCL_FRAMEWORK', '0') == '1'


def _pcl_layout_ok(pred: Tensor, target: Tensor) -> bool:
    if target.ndim != 5 or tuple(target.shape[-2:]) != (3, 3):
        return False
    if pred.ndim == 4 and pred.shape[-1] == 6:
        return pred.shape[:3] == target.shape[:3]
    return pred.ndim == 5 and pred.shape == target.shape


def pose_change_loss_supported(pred: Tensor, target: Tensor, criterion) -> bool:
    """What K27 covers: fp32 device tensors, ``pred`` (B,T,J,6) or (B,T,J,3,3) against ``target`` (B,T,J,3,3), ``nn.MSELoss``
    with reduction 'mean' or 'sum', at least one element and fewer than 2^31 (the kernel indexes with 32 bits). Everything
    else -- host tensors, fp64, other criteria -- and ``P2C_PCL_FRAMEWORK=1`` is the losses' tensor code."""
    return (type(criterion) is torch.nn.MSELoss and criterion.reduction in ('mean', 'sum')
            and isinstance(pred, Tensor) and isinstance(target, Tensor)
            and pred.is_cuda and target.is_cuda and pred.device == target.device
            and pred.dtype == torch.float32 and target.dtype == torch.float32 and _pcl_layout_ok(pred, target)
            and 0 < target.numel() < 2 ** 31 and not pcl_framework() and not torch.is_autocast_enabled())


def _pcl_desc(pred: Tensor, target: Tensor, cumulative: bool, mean: bool, max_blocks: int = 0):
    d = _lib.PoseChangeLossDesc()
    d.B, d.T, d.J = target.shape[0], target.shape[1], target.shape[2]
    d.pred_is_6d, d.cumulative, d.mean, d.max_blocks = int(pred.ndim == 4), int(bool(cumulative)), int(bool(mean)), int(max_blocks)
    d.pred, d.target = pred.data_ptr(), target.data_ptr()
    return d


class PoseChangeLossFunction(torch.autograd.Function):
    """loss = K27(pred, target): one launch forward, one backward. The forward leaves the differences and the running products
    in a workspace the backward reads; the gradient goes to the prediction only."""

    @staticmethod
    def forward(ctx, pred, target, cumulative: bool, mean: bool, max_blocks: int):
        lib = _lib.lib()
        pred, target = _aligned16(_require_device(pred, 'pose changes')), _require_device(target, 'target pose changes')
        if not _pcl_layout_ok(pred, target):
            raise RuntimeError(f'pose_change_loss: prediction {tuple(pred.shape)} against target {tuple(target.shape)}; '
                               '(B,T,J,6) or (B,T,J,3,3) against (B,T,J,3,3) expected')
        desc = _pcl_desc(pred, target, cumulative, mean, max_blocks)
        n_ws = lib.p2c_pose_change_loss_workspace_floats(ctypes.byref(desc))
        _lib.check(min(n_ws, 0), 'p2c_pose_change_loss_workspace_floats')
        f32 = dict(dtype=torch.float32, device=pred.device)
        ws, loss = torch.empty(n_ws, **f32), torch.zeros(1, **f32)
        desc.workspace, desc.loss = ws.data_ptr(), loss.data_ptr()
        with torch.cuda.device(pred.device):
            _lib.check(lib.p2c_pose_change_loss_fwd(ctypes.byref(desc), _stream()), 'p2c_pose_change_loss_fwd')
        ctx.save_for_backward(pred, target, ws)
        ctx.cfg = (bool(cumulative), bool(mean), int(max_blocks))
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g_loss):
        lib = _lib.lib()
        pred, target, ws = ctx.saved_tensors
        g_loss = _require_device(g_loss, 'grad').reshape(1)       # (a local: an expanded scalar is copied, the copy outlives the launch)
        gp = torch.empty_like(pred)
        desc = _pcl_desc(pred, target, *ctx.cfg)
        desc.workspace, desc.grad_loss, desc.grad_pred = ws.data_ptr(), g_loss.data_ptr(), gp.data_ptr()
        with torch.cuda.device(pred.device):
            _lib.check(lib.p2c_pose_change_loss_bwd(ctypes.byref(desc), _stream()), 'p2c_pose_change_loss_bwd')
        return gp, None, None, None, None


def pose_change_loss(pred: Tensor, target: Tensor, cumulative: bool, reduction: str = 'mean', max_blocks: int = 0) -> Tensor:
    """K27: ``MSELoss(reduction)`` between the pose changes ``pred`` -- (B,T,J,6) raw 6-D rotations or (B,T,J,3,3) matrices -- and
    ``target`` (B,T,J,3,3) directly (``cumulative=False``, the reference's pose_changes) or between their running products
    over the frames (``cumulative=True``, cum_pose_changes). The mean divides by B T J 9 for either layout. fp32 device
    tensors; views are copied (``pose_change_loss_supported`` says what is covered: there is no framework fallback here).
    ``max_blocks`` lowers the kernel's grid cap (tests)."""
    if reduction not in ('mean', 'sum'):
        raise RuntimeError(f"pose_change_loss: reduction '{reduction}' (mean or sum expected)")
    return PoseChangeLossFunction.apply(pred, target, bool(cumulative), reduction == 'mean', int(max_blocks))


# ----------------------------------------------------------------------------------------------------------------------
# heatmap head of the pose-estimation flow (K28, csrc/p2c_heatmaps.hip)
# ----------------------------------------------------------------------------------------------------------------------
HEATMAPS_POOL = (9, 8, 1)            # the flow's target resize: avg_pool2d(kernel 9, stride 8, padding 1)
_HM_FAR = 2 ** 30                    # a centre no window reaches: where non-finite or huge keypoints land (kernel: kFar)


def heatmaps_framework() -> bool:
    """P2C_HEATMAPS_FRAMEWORK=1: the three heatmap ops run their tensor restatements on the device (the comparison arm of
    tools/bench_heatmaps.py)."""
    return os.environ.get('P2C_HEATMAPS_FRAMEWORK', '0') == '1'


def _hm_kernel_ok(*tensors: Tensor) -> bool:
    return (all(isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.device == tensors[0].device for t in tensors)
            and not heatmaps_framework() and not torch.is_autocast_enabled())


_gaussian_tables: Dict[tuple, Tensor] = {}


def gaussian_table(sigma, device=None) -> Tensor:
    """g[d2] = float32(exp(-d2 / 2 / sigma / sigma)) for the integer squared distances d2 = 0, 1, ..., formed in fp64 with both
    clamps of the reference's gaussian_kernel (> 1 -> 1, < 0.0099 -> 0) before the cast, up to and including the first zero
    (11 entries for sigma = 1, 85 for sigma = 3); every later entry is zero. Cached per (sigma, device)."""
    import numpy as np
    key = (float(sigma), str(device))
    if key not in _gaussian_tables:
        if not sigma > 0:
            raise ValueError(f'gaussian_table: sigma {sigma}')
        n = int(-2.0 * float(sigma) ** 2 * np.log(0.0099)) + 3          # past the cut, whatever the rounding
        g = np.exp(-np.arange(n) / 2.0 / sigma / sigma)
        g[g > 1] = 1
        g[g < 0.0099] = 0
        first_zero = int(np.argmin(g > 0))
        assert g[first_zero] == 0 and first_zero > 0
        _gaussian_tables[key] = torch.from_numpy(g[:first_zero + 1]).float().to(device or 'cpu')
    return _gaussian_tables[key]


def _pool_out(size: int, k: int, s: int, p: int) -> int:
    return (size + 2 * p - k) // s + 1


def heatmap_centres(projection_2d: Tensor, shift: Tensor, scale) -> Tensor:
    """``((kp - shift) * scale).round()`` in the keypoints' own precision, as int64; non-finite and huge values go to a far
    corner whose Gaussian reaches no frame (the reference's ``.int()`` is undefined there)."""
    scale = torch.as_tensor(scale, dtype=torch.float32).to(device=projection_2d.device, dtype=projection_2d.dtype)
    c = ((projection_2d - shift.to(projection_2d.dtype)[..., None, :]) * scale).round()
    c = torch.where((c > -_HM_FAR) & (c < _HM_FAR), c, torch.full_like(c, -_HM_FAR))
    return c.long()


def _heatmap_targets_tensor(projection_2d: Tensor, shift: Tensor, scale, size, sigma, pool) -> Tensor:
    H, W = int(size[0]), int(size[1])
    dev = projection_2d.device
    table = gaussian_table(sigma, dev)
    n = table.numel()
    table = torch.cat((table, table.new_zeros(1))).to(projection_2d.dtype)
    c = heatmap_centres(projection_2d[..., :2], shift, scale)                            # (B,T,J,2)
    dx = torch.arange(W, device=dev) - c[..., 0, None]                                    # (B,T,J,W)
    dy = torch.arange(H, device=dev) - c[..., 1, None]
    d2 = (dy * dy)[..., :, None] + (dx * dx)[..., None, :]                                # (B,T,J,H,W)
    g = table[d2.clamp_(max=n)]
    out = torch.cat((1 - g.max(dim=2, keepdim=True).values, g), dim=2)
    if pool is not None:
        k, s, p = pool
        out = torch.nn.functional.avg_pool2d(out.flatten(0, 1), kernel_size=k, stride=s, padding=p).unflatten(0, out.shape[:2])
    return out


def heatmap_targets_supported(projection_2d: Tensor, shift: Tensor, sigma, pool) -> bool:
    """What K28a covers: fp32 device keypoints outside autocast, at most 63 joints (64 maps), a Gaussian table of at most 1 024
    entries and a pooling window of at most 32; everything else, and ``P2C_HEATMAPS_FRAMEWORK=1``, is the tensor path."""
    k, s, p = pool if pool is not None else (1, 1, 0)
    return (_hm_kernel_ok(projection_2d, shift) and projection_2d.ndim == 4 and 1 <= projection_2d.shape[2] < _lib.HEATMAPS_MAX_MAPS
            and gaussian_table(sigma).numel() <= _lib.HEATMAPS_MAX_TABLE and 1 <= k <= _lib.HEATMAPS_MAX_POOL and 2 * p <= k)


def heatmap_targets(projection_2d: Tensor, shift: Tensor, scale, size, sigma=1, pool=HEATMAPS_POOL) -> Tensor:
    """Target maps (B,T,J+1,oh,ow) of the pose-estimation flow straight from the keypoints: the reference's ``_get_heatmap``
    (Gaussians of ``sigma`` around ``rint((kp - shift) * scale)`` on a ``size`` = (H, W) frame, background first) and the flow's
    ``avg_pool2d(*pool)`` in one launch (K28a); ``pool=None`` gives the full-resolution maps, bit for bit the reference's.
    ``projection_2d`` (B,T,J,>=2) pixels, ``shift`` (B,T,2), ``scale`` = (clip_w / original_w, clip_h / original_h)."""
    if projection_2d.ndim != 4 or projection_2d.shape[-1] < 2 or tuple(shift.shape) != (*projection_2d.shape[:2], 2):
        raise RuntimeError(f'heatmap_targets: keypoints {tuple(projection_2d.shape)} with shifts {tuple(shift.shape)}; '
                           '(B,T,J,>=2) with (B,T,2) expected')
    if pool is not None:
        pool = tuple(int(v) for v in pool)
    if not heatmap_targets_supported(projection_2d, shift, sigma, pool):
        return _heatmap_targets_tensor(projection_2d, shift, scale, size, sigma, pool)
    lib = _lib.lib()
    kp, shift = projection_2d[..., :2].contiguous(), shift.contiguous()
    table = gaussian_table(sigma, kp.device)
    B, T, Jn = kp.shape[:3]
    k, s, p = pool if pool is not None else (1, 1, 0)
    sx, sy = (float(v) for v in torch.as_tensor(scale, dtype=torch.float32).reshape(2))
    d = _lib.HeatmapTargetsDesc()
    d.N, d.J, d.H, d.W, d.k, d.s, d.p = B * T, Jn, int(size[0]), int(size[1]), k, s, p
    d.oh, d.ow, d.n_table, d.scale_x, d.scale_y = _pool_out(d.H, k, s, p), _pool_out(d.W, k, s, p), table.numel(), sx, sy
    out = torch.empty(B, T, Jn + 1, max(d.oh, 0), max(d.ow, 0), dtype=torch.float32, device=kp.device)
    d.kp, d.shift, d.table, d.out = kp.data_ptr(), shift.data_ptr(), table.data_ptr(), out.data_ptr()
    with torch.cuda.device(kp.device):
        _lib.check(lib.p2c_heatmap_targets_fwd(ctypes.byref(d), _stream()), 'p2c_heatmap_targets_fwd')
    return out


def grouped_loss_tensor(pred: Tensor, gt: Tensor, mask: Optional[Tensor], criterion, group_dim: int):
    """``BasePoseLoss``'s ``sum_per_frame`` (``group_dim=1``) / ``sum_per_joint`` (``group_dim=-2``) without boolean gathers:
    ``pred`` and ``gt`` (B,T,K,D), ``mask`` (B,T,K) or None; per group the criterion over the selected (.., D) rows, groups whose
    value is NaN (nothing selected under 'mean', or a NaN inside) skipped with zero gradient, the rest summed. Where the
    reference raises on an empty ``torch.stack`` (every group skipped) the result is 0."""
    import copy
    each = copy.copy(criterion)
    each.reduction = 'none'
    mean = getattr(criterion, 'reduction', 'mean') == 'mean'
    group_dim = group_dim % pred.ndim
    others = [d for d in range(pred.ndim - 1) if d != group_dim]
    sel = torch.ones(pred.shape[:-1], dtype=torch.bool, device=pred.device) if mask is None else mask.bool()
    count = sel.sum(others).to(pred.dtype) * pred.shape[-1]

    def per_group(w, count):
        p = torch.where(w[..., None], pred, gt.detach())          # an unselected row never meets the criterion's backward
        e = torch.where(w[..., None], each(p, gt), torch.zeros((), dtype=pred.dtype, device=pred.device))
        s = e.sum(-1).sum(others)
        return s / count if mean else s
    with torch.no_grad():
        use = ~torch.isnan(per_group(sel, count))               # 0 / 0 where nothing is selected under 'mean'
    shape = [1] * (pred.ndim - 1)
    shape[group_dim] = -1
    w = sel & use.reshape(shape)
    terms = per_group(w, count.clamp(min=1))
    return torch.where(use, terms, torch.zeros_like(terms)).sum(), sel


def _hm_channels(pred: Tensor, gt: Tensor, pred_channels, gt_channels, forced: int):
    pc, gc = [int(c) for c in pred_channels], [int(c) for c in gt_channels]
    if pred.ndim != 5 or gt.ndim != 5 or pred.shape[:2] != gt.shape[:2] or pred.shape[3:] != gt.shape[3:]:
        raise RuntimeError(f'heatmaps_loss: prediction {tuple(pred.shape)} against target {tuple(gt.shape)}; (B,T,P,h,w) maps '
                           'of one resolution expected')
    if (len(pc) != len(gc) or not pc or any(not 0 <= c < pred.shape[2] for c in pc) or any(not 0 <= c < gt.shape[2] for c in gc)
            or not -1 <= int(forced) < len(pc)):
        raise RuntimeError(f'heatmaps_loss: channel lists {pc} / {gc} (forced {forced}) for {pred.shape[2]} / {gt.shape[2]} maps')
    return pc, gc


def _heatmaps_loss_tensor(pred: Tensor, gt: Tensor, pc, gc, forced: int, mask: bool):
    cp, cg = pred[:, :, pc].flatten(3), gt[:, :, gc].flatten(3).to(pred.dtype)
    sel = None
    if mask:
        sel = (cg != 0).all(-1)
        if forced >= 0:
            sel[..., forced] = True
    return grouped_loss_tensor(cp, cg, sel, torch.nn.MSELoss(reduction='mean'), 1)


def heatmaps_loss_supported(pred: Tensor, gt: Tensor, n_pairs: int) -> bool:
    """What K28b covers: fp32 device maps outside autocast, at most 64 maps a frame on either side and at most 64 pairs."""
    return (_hm_kernel_ok(pred, gt) and pred.ndim == 5 and gt.ndim == 5 and max(pred.shape[2], gt.shape[2], n_pairs) <= _lib.HEATMAPS_MAX_MAPS
            and pred.numel() > 0)


def _hm_loss_desc(pred, gt, pc, gc, forced, mask):
    d = _lib.HeatmapsLossDesc()
    d.B, d.T, d.Pp, d.Pg, d.h, d.w = pred.shape[0], pred.shape[1], pred.shape[2], gt.shape[2], pred.shape[3], pred.shape[4]
    d.K, d.forced, d.mask = len(pc), int(forced), int(bool(mask))
    for i, (a, b) in enumerate(zip(pc, gc)):
        d.pred_channels[i], d.gt_channels[i] = a, b
    d.pred, d.gt = pred.data_ptr(), gt.data_ptr()
    return d


class HeatmapsLossFunction(torch.autograd.Function):
    """(loss, selection flags) = K28b(pred, gt): two launches forward (per-pair sums and flags, then the fixed-order finish),
    one backward that reads the saved per-frame coefficients and flags. The gradient goes to the prediction only."""

    @staticmethod
    def forward(ctx, pred, gt, pc, gc, forced: int, mask: bool):
        lib = _lib.lib()
        pred, gt = _require_device(pred, 'heatmaps'), _require_device(gt, 'target heatmaps')   # views are copied dense
        B, T = pred.shape[:2]
        f32 = dict(dtype=torch.float32, device=pred.device)
        partials, coef, loss = torch.empty(B, T, len(pc), **f32), torch.empty(T, **f32), torch.empty(1, **f32)
        flags = torch.empty(B, T, len(pc), dtype=torch.int32, device=pred.device)
        d = _hm_loss_desc(pred, gt, pc, gc, forced, mask)
        d.partials, d.flags, d.coef, d.loss = partials.data_ptr(), flags.data_ptr(), coef.data_ptr(), loss.data_ptr()
        with torch.cuda.device(pred.device):
            _lib.check(lib.p2c_heatmaps_loss_fwd(ctypes.byref(d), _stream()), 'p2c_heatmaps_loss_fwd')
        ctx.save_for_backward(pred, gt, partials, flags, coef)
        ctx.cfg = (pc, gc, forced, mask)
        ctx.mark_non_differentiable(flags)
        return loss.reshape(()), flags

    @staticmethod
    def backward(ctx, g_loss, _g_flags):
        lib = _lib.lib()
        pred, gt, partials, flags, coef = ctx.saved_tensors
        g_loss = _require_device(g_loss, 'grad').reshape(1)       # (a local: an expanded scalar is copied, the copy outlives the launch)
        gp = torch.empty_like(pred)
        d = _hm_loss_desc(pred, gt, *ctx.cfg)
        d.partials, d.flags, d.coef = partials.data_ptr(), flags.data_ptr(), coef.data_ptr()
        d.grad_loss, d.grad_pred = g_loss.data_ptr(), gp.data_ptr()
        with torch.cuda.device(pred.device):
            _lib.check(lib.p2c_heatmaps_loss_bwd(ctypes.byref(d), _stream()), 'p2c_heatmaps_loss_bwd')
        return gp, None, None, None, None, None


def heatmaps_loss(pred: Tensor, gt: Tensor, pred_channels: Sequence[int], gt_channels: Sequence[int], forced: int = -1,
                  mask: bool = True, with_flags: bool = False):
    """``HeatmapsLoss`` = ``BasePoseLoss``'s ``sum_per_frame`` with ``MSELoss('mean')`` over heatmaps: pair k compares the stored
    channel ``pred_channels[k]`` of ``pred`` (B,T,Pp,h,w) with ``gt_channels[k]`` of ``gt`` (B,T,Pg,h,w); it is selected in (b,t)
    when ``mask`` is off, when every cell of its target map is != 0, or when ``k == forced``; loss = sum over the frames of
    S_t / (n_t h w), frames with nothing selected or a NaN sum skipped (zero gradient there). K28b on fp32 device tensors, the
    tensor restatement otherwise. ``with_flags`` also returns the (B,T,K) selection."""
    pc, gc = _hm_channels(pred, gt, pred_channels, gt_channels, forced)
    if heatmaps_loss_supported(pred, gt, len(pc)):
        loss, flags = HeatmapsLossFunction.apply(pred, gt, tuple(pc), tuple(gc), int(forced), bool(mask))
        flags = flags.bool()
    else:
        loss, flags = _heatmaps_loss_tensor(pred, gt, pc, gc, int(forced), bool(mask))
    return (loss, flags) if with_flags else loss


def _heatmap_keypoints_tensor(heatmaps: Tensor, frame_size) -> Tensor:
    B, T, P, h, w = heatmaps.shape
    sw, sh = frame_size[0] / w, frame_size[1] / h
    m = heatmaps[:, :, 1:].flatten(3)
    c = m.max(-1).values                                            # NaN if the map holds one: c > 0 is false then
    cells = torch.arange(h * w, device=m.device)
    first = torch.where(m == c[..., None], cells, torch.full_like(cells, h * w)).min(-1).values.clamp_(max=h * w - 1)
    row, col = torch.div(first, w, rounding_mode='floor'), first % w
    out = torch.stack((col.float() * sw, row.float() * sh, c.float()), -1)
    return torch.where((c > 0)[..., None], out, torch.zeros_like(out))


def heatmap_keypoints(heatmaps: Tensor, frame_size) -> Tensor:
    """The reference's ``_keypoints_from_heatmaps``: (B,T,P-1,3) = (col * sw, row * sh, c) of the maximum c of every map of
    channels 1..P-1 at its first flat index when c > 0, zeros otherwise (a map with a NaN too), fp32. ``frame_size`` is
    ``frames.shape[-2:]`` and is read as the reference reads it, (bbox_width, bbox_height): sw = frame_size[0] / w,
    sh = frame_size[1] / h -- swapped for non-square frames, kept for parity. K28c (one launch, no host sync) on fp32 device
    tensors with at most 64 maps, the tensor restatement otherwise."""
    if heatmaps.ndim != 5 or heatmaps.shape[2] < 2 or heatmaps.shape[3] * heatmaps.shape[4] < 1:
        raise RuntimeError(f'heatmap_keypoints: (B,T,P>=2,h,w) expected, got {tuple(heatmaps.shape)}')
    B, T, P, h, w = heatmaps.shape
    if not (_hm_kernel_ok(heatmaps) and P <= _lib.HEATMAPS_MAX_MAPS):
        return _heatmap_keypoints_tensor(heatmaps, frame_size)
    lib = _lib.lib()
    maps = heatmaps.detach().contiguous()
    out = torch.empty(B, T, P - 1, 3, dtype=torch.float32, device=maps.device)
    d = _lib.HeatmapKeypointsDesc()
    d.N, d.P, d.h, d.w, d.sw, d.sh = B * T, P, h, w, frame_size[0] / w, frame_size[1] / h
    d.maps, d.out = maps.data_ptr(), out.data_ptr()
    with torch.cuda.device(maps.device):
        _lib.check(lib.p2c_heatmap_keypoints_fwd(ctypes.byref(d), _stream()), 'p2c_heatmap_keypoints_fwd')
    return out


# ----------------------------------------------------------------------------------------------------------------------
# predicted poses <-> CARLA bone transforms (K30, csrc/p2c_carla_pose.hip)
# ----------------------------------------------------------------------------------------------------------------------
def carla_framework() -> bool:
    """P2C_CARLA_FRAMEWORK=1: ``carla_pose_export`` / ``carla_pose_import`` run their tensor definitions on the device (the
    comparison arm of tools/bench_carla_pose.py)."""
    return os.environ.get('P2C_CARLA_FRAMEWORK', '0') == '1'


def _carla_kernel_ok(*tensors: Tensor) -> bool:
    return (all(t.is_cuda and t.dtype == torch.float32 and t.device == tensors[0].device for t in tensors)
            and not carla_framework() and not torch.is_autocast_enabled())


def _carla_row(loc: Tensor, rot: Tensor) -> Tensor:
    """(..., 3), (..., 3, 3) -> (..., 6) = (x, y, -z, pitch, yaw, roll): the tensor definition of K30's forward."""
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import matrix_to_euler_angles
    deg = -torch.rad2deg(matrix_to_euler_angles(rot, 'XYZ'))
    return torch.stack((loc[..., 0], loc[..., 1], -loc[..., 2], deg[..., 1], deg[..., 2], deg[..., 0]), -1)


def _carla_check_export(rel_loc, rel_rot, world_loc, world_rot):
    if (rel_loc.ndim < 2 or rel_loc.shape[-1] != 3 or rel_rot.ndim != rel_loc.ndim + 1
            or tuple(rel_rot.shape) != tuple(rel_loc.shape) + (3,) or rel_loc.shape[-2] < 1):
        raise RuntimeError(f'carla_pose_export: locations {tuple(rel_loc.shape)} with rotations {tuple(rel_rot.shape)}; '
                           '(...,J,3) with (...,J,3,3) expected')
    if (world_loc is None) != (world_rot is None):
        raise RuntimeError('carla_pose_export: world_loc and world_rot come together or not at all')
    if world_loc is not None:
        lead = tuple(rel_loc.shape[:-2])
        if tuple(world_loc.shape) != lead + (3,) or tuple(world_rot.shape) != lead + (3, 3):
            raise RuntimeError(f'carla_pose_export: world tensors {tuple(world_loc.shape)}, {tuple(world_rot.shape)} for poses '
                               f'{tuple(rel_loc.shape)}; {lead + (3,)} and {lead + (3, 3)} expected')


@torch.no_grad()
def carla_pose_export(rel_loc: Tensor, rel_rot: Tensor, world_loc: Optional[Tensor] = None,
                      world_rot: Optional[Tensor] = None, max_blocks: int = 0) -> Tuple[Tensor, Optional[Tensor]]:
    """What a CARLA walker consumes, from what ``flow.predict_step`` leaves: ``rel_loc`` (...,J,3) and ``rel_rot`` (...,J,3,3)
    -> ``bones`` (...,J,6), and ``world_loc`` (...,3) with ``world_rot`` (...,3,3) -> ``root`` (...,6) (None without them). A row is
    (x, y, -z, pitch, yaw, roll) with (roll, pitch, yaw) = -degrees of ``matrix_to_euler_angles(R, 'XYZ')[(0, 1, 2)]`` --
    the reference's ``P3dPose.tensors_to_pose`` and the root conversion of ``CarlaRenderer.render_frame``; locations are not
    scaled. Any leading dimensions, any J >= 1; views are made contiguous. A predict-time operation: nothing is recorded for
    autograd. fp32 device tensors outside autocast take K30 (one launch for bones and root); host tensors, fp64, other dtypes
    and ``P2C_CARLA_FRAMEWORK=1`` take the tensor definition. ``max_blocks`` lowers the kernel's grid cap (tests)."""
    _carla_check_export(rel_loc, rel_rot, world_loc, world_rot)
    given = [t for t in (rel_loc, rel_rot, world_loc, world_rot) if t is not None]
    if not _carla_kernel_ok(*given):
        return _carla_row(rel_loc, rel_rot), (_carla_row(world_loc, world_rot) if world_loc is not None else None)
    lib = _lib.lib()
    loc, rot = rel_loc.detach().contiguous(), rel_rot.detach().contiguous()
    wl = world_loc.detach().contiguous() if world_loc is not None else None
    wr = world_rot.detach().contiguous() if world_rot is not None else None
    n_joints = loc.shape[-2]
    n = loc.numel() // (3 * n_joints)
    bones = torch.empty(tuple(loc.shape[:-1]) + (6,), dtype=torch.float32, device=loc.device)
    root = torch.empty(tuple(wl.shape[:-1]) + (6,), dtype=torch.float32, device=loc.device) if wl is not None else None
    with torch.cuda.device(loc.device):
        _lib.check(lib.p2c_carla_pose_fwd(loc.data_ptr(), rot.data_ptr(), _ptr(wl), _ptr(wr), bones.data_ptr(), _ptr(root),
                                          n, n_joints, int(max_blocks), _stream()), 'p2c_carla_pose_fwd')
    return bones, root


@torch.no_grad()
def carla_pose_import(bones: Tensor, max_blocks: int = 0) -> Tuple[Tensor, Tensor]:
    """The inverse of ``carla_pose_export`` (the reference's ``P3dPose.pose_to_tensors``): ``bones`` (...,J,6) rows of
    (x, y, z, pitch, yaw, roll) -> ``loc`` (...,J,3) = (x, y, -z) and ``rot`` (...,J,3,3) = ``euler_angles_to_matrix`` of
    radians(-roll, -pitch, -yaw), 'XYZ'. Dispatch as ``carla_pose_export``."""
    if bones.ndim < 2 or bones.shape[-1] != 6 or bones.shape[-2] < 1:
        raise RuntimeError(f'carla_pose_import: (...,J,6) expected, got {tuple(bones.shape)}')
    if not _carla_kernel_ok(bones):
        from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix
        angles = torch.deg2rad(torch.stack((-bones[..., 5], -bones[..., 3], -bones[..., 4]), -1))
        return (torch.stack((bones[..., 0], bones[..., 1], -bones[..., 2]), -1), euler_angles_to_matrix(angles, 'XYZ'))
    lib = _lib.lib()
    rows = bones.detach().contiguous()
    n_joints = rows.shape[-2]
    n = rows.numel() // (6 * n_joints)
    loc = torch.empty(tuple(rows.shape[:-1]) + (3,), dtype=torch.float32, device=rows.device)
    rot = torch.empty(tuple(rows.shape[:-1]) + (3, 3), dtype=torch.float32, device=rows.device)
    with torch.cuda.device(rows.device):
        _lib.check(lib.p2c_carla_pose_inv(rows.data_ptr(), loc.data_ptr(), rot.data_ptr(), n, n_joints, int(max_blocks),
                                          _stream()), 'p2c_carla_pose_inv')
    return loc, rot


# ----------------------------------------------------------------------------------------------------------------------
# keypoint clips -> CARLA bone transforms in one launch (K32, csrc/p2c_lift.hip)
# ----------------------------------------------------------------------------------------------------------------------
LIFT_KINDS = ('pose_changes_6d', 'relative_rot_6d')


def lift_framework() -> bool:
    """P2C_LIFT_FRAMEWORK=1: ``lift_to_carla`` runs the three separate calls (``fused_mlp`` -> ``pose_head`` ->
    ``carla_pose_export``) on the device: the comparison arm of tools/bench_lift.py."""
    return os.environ.get('P2C_LIFT_FRAMEWORK', '0') == '1'


def lift_supported(dims: Sequence[int]) -> bool:
    """The model geometry K32 is compiled for: the LinearAE 52-26-13-6-39-78-156 (fp32, the two 6-D kinds)."""
    dims = [int(v) for v in dims]
    if not 2 <= len(dims) <= _lib.P2C_MLP_MAX_LAYERS + 1:
        return False
    d = _lib.LiftDesc()
    d.mlp.n_layers = len(dims) - 1
    for i, v in enumerate(dims):
        d.mlp.dims[i] = v
    d.kind = KIND['pose_changes_6d']
    return bool(_lib.lib().p2c_lift_supported(ctypes.byref(d)))


def _fma32(a: Tensor, b: Tensor, c: Tensor) -> Tensor:
    """fmaf(a, b, c) on fp32 tensors, bit for bit, from fp64 tensor ops: the product of two fp32 values is exact in fp64; the
    sum is rounded to odd (TwoSum gives the rounding error of the nearest-even sum; where it is non-zero and the sum's last
    bit is even, the neighbour on the error's side is the odd one), and a value rounded to odd with 29 spare bits rounds to
    fp32 as the exact sum does."""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)
    even = (s.view(torch.int64) & 1) == 0
    side = torch.where(err > 0, torch.full_like(s, float('inf')), torch.full_like(s, float('-inf')))
    return torch.where((err != 0) & even & torch.isfinite(s), torch.nextafter(s, side), s).float()


def _mul3_fma(a: Tensor, b: Tensor) -> Tensor:
    """a @ b for (...,3,3) fp32 in the order of the kernels' ``mul``: fmaf(a_i0, b_0k, fmaf(a_i1, b_1k, a_i2 * b_2k))."""
    a0, a1, a2 = (a[..., :, k, None] for k in range(3))          # (...,3,1) columns of a
    b0, b1, b2 = (b[..., None, k, :] for k in range(3))          # (...,1,3) rows of b
    return _fma32(a0, b0, _fma32(a1, b1, a2 * b2))


def _lift_chain(changes: Tensor, start: Tensor, exact_fma: bool) -> Tensor:
    """R_t = c_t @ R_{t-1} over the frames (reference projection.py:190-193), R_{-1} = ``start`` (B,J,3,3)."""
    prev, rel = start, []
    for t in range(changes.shape[1]):
        prev = _mul3_fma(changes[:, t], prev) if exact_fma else changes[:, t] @ prev
        rel.append(prev)
    return torch.stack(rel, 1)


@torch.no_grad()
def pose_to_carla_rows(y: Tensor, skel_type: Tensor, kind: str, world_loc: Optional[Tensor] = None,
                       world_rot: Optional[Tensor] = None, initial_rel_rot: Optional[Tensor] = None, want_rot: bool = False,
                       max_blocks: int = 0, tensor_ops: bool = False):
    """A movements model's rotation output -> ``(bones, root, final_rel_rot, relative_pose_rot | None)`` as ``lift_to_carla``
    returns them: the two calls behind the model in the composed path. ``kind``: 'pose_changes_6d' / 'relative_rot_6d' with
    ``y`` (B,T,26,6), 'pose_changes' / 'relative_rot' with (B,T,26,3,3). fp32 device tensors take the materialising pose head and
    K30; the pose head starts every clip from the reference pose, so with ``initial_rel_rot`` its pose changes are multiplied up
    again from there in the order of its own 3x3 product (``_mul3_fma``). Host tensors, other dtypes and ``tensor_ops`` take the
    definition on tensor ops (reference projection.py:144-195 and ``carla_pose_export``'s)."""
    B, T = y.shape[:2]
    scan = kind.startswith('pose_changes')
    wl, wr = (world_loc, world_rot) if world_loc is not None else identity_world((B, T), y)
    if not tensor_ops and y.is_cuda and y.dtype == torch.float32 and not torch.is_autocast_enabled():
        carry = scan and initial_rel_rot is not None
        want = ('relative_pose_loc', 'relative_pose_rot') + (('pose_changes',) if carry else ())
        _, outs = pose_head(y, PoseHeadSpec(kind=kind, transform='none'), skel_type, want=want)
        rot = _lift_chain(outs['pose_changes'], initial_rel_rot, exact_fma=True) if carry else outs['relative_pose_rot']
        bones, root = carla_pose_export(outs['relative_pose_loc'], rot, wl, wr, max_blocks=max_blocks)
    else:
        from pedestrians_video_2_carla_amd.transforms.rotation_conversions import rotation_6d_to_matrix
        m = rotation_6d_to_matrix(y) if kind.endswith('6d') else y
        ref_loc, ref_rot = ref.get_relative_tensors(y.device, dtype=y.dtype)
        st = skel_type.long()
        rot = _lift_chain(m, initial_rel_rot if initial_rel_rot is not None else ref_rot[st], exact_fma=False) if scan else m
        bones, root = _carla_row(ref_loc[st][:, None].expand(B, T, J, 3), rot), _carla_row(wl, wr)
    return bones, root, (rot[:, -1].clone() if scan else None), (rot.contiguous() if want_rot else None)


def _linear_stack(x2d: Tensor, weights, biases) -> Tensor:
    h = x2d
    for l, (w, b) in enumerate(zip(weights, biases)):
        h = torch.nn.functional.linear(h, w, b)
        if l < len(weights) - 1:
            h = torch.relu(h)
    return h


@torch.no_grad()
def lift_to_carla(frames: Tensor, weights: Sequence[Tensor], biases: Sequence[Tensor], skel_type: Tensor,
                  kind: str = 'pose_changes_6d', image: Optional[Tensor] = None, image_is_current: bool = False,
                  world_loc: Optional[Tensor] = None, world_rot: Optional[Tensor] = None,
                  initial_rel_rot: Optional[Tensor] = None, want_rot: bool = False,
                  max_blocks: int = 0) -> Tuple[Tensor, Tensor, Optional[Tensor], Optional[Tensor]]:
    """2-D keypoint clips -> the rows a CARLA walker consumes. ``frames`` (B,T,26,2) or (B,T,52), the LinearAE's ``weights`` /
    ``biases`` (as ``fused_mlp`` takes them), ``skel_type`` (B) -> ``bones`` (B,T,26,6), ``root`` (B,T,6) (the identity world's
    row without ``world_loc`` (B,T,3) / ``world_rot`` (B,T,3,3), which come together), ``final_rel_rot`` (B,26,3,3) (the last
    relative rotation, pose_changes kind; None otherwise) and, with ``want_rot``, ``relative_pose_rot`` (B,T,26,3,3).
    ``initial_rel_rot`` (B,26,3,3): where the running rotation of the pose_changes kind starts instead of the reference pose --
    hand a clip the previous clip's ``final_rel_rot`` and a cut video yields the rows of the uncut one.
    fp32 device tensors of the 52-26-13-6-39-78-156 model take K32: one launch (two when ``image`` -- ``mlp_image_layout``
    floats -- is not given or not ``image_is_current``: the weights are packed first), with the bits of the three separate calls.
    ``P2C_LIFT_FRAMEWORK=1`` runs those calls; host tensors, fp64 and other geometries the same composition on tensor ops.
    A predict-time operation: nothing is recorded for autograd. ``max_blocks`` lowers the grid cap (tests)."""
    if kind not in LIFT_KINDS:
        raise RuntimeError(f'lift_to_carla: kind {kind!r}; one of {LIFT_KINDS} expected')
    if frames.ndim not in (3, 4) or len(weights) != len(biases) or not weights:
        raise RuntimeError(f'lift_to_carla: frames (B,T,26,2) or (B,T,52) expected, got {tuple(frames.shape)}')
    B, T = frames.shape[:2]
    x = frames.reshape(B, T, -1)
    dims = [weights[0].shape[1]] + [w.shape[0] for w in weights]
    if x.shape[-1] != dims[0] or dims[-1] != J * 6:
        raise RuntimeError(f'lift_to_carla: frames of {x.shape[-1]} values for a model {dims[0]} -> {dims[-1]}; '
                           f'{dims[0]} -> {J * 6} expected')
    if tuple(skel_type.shape) != (B,):
        raise RuntimeError(f'skel_type should have shape ({B},), got {tuple(skel_type.shape)}')
    if (world_loc is None) != (world_rot is None):
        raise RuntimeError('lift_to_carla: world_loc and world_rot come together or not at all')
    if world_loc is not None and (tuple(world_loc.shape) != (B, T, 3) or tuple(world_rot.shape) != (B, T, 3, 3)):
        raise RuntimeError(f'lift_to_carla: world tensors {tuple(world_loc.shape)}, {tuple(world_rot.shape)}; '
                           f'{(B, T, 3)} and {(B, T, 3, 3)} expected')
    if initial_rel_rot is not None and tuple(initial_rel_rot.shape) != (B, J, 3, 3):
        raise RuntimeError(f'initial_rel_rot should have shape {(B, J, 3, 3)}, got {tuple(initial_rel_rot.shape)}')
    floats = [x, *weights, *biases] + [t for t in (world_loc, world_rot, initial_rel_rot) if t is not None]
    if B == 0 or T == 0:
        e = dict(dtype=x.dtype, device=x.device)
        return (torch.empty(B, T, J, 6, **e), torch.empty(B, T, 6, **e),
                torch.empty(B, J, 3, 3, **e) if kind == 'pose_changes_6d' else None,
                torch.empty(B, T, J, 3, 3, **e) if want_rot else None)
    on_device = (all(t.is_cuda and t.dtype == torch.float32 and t.device == x.device for t in floats)
                 and skel_type.device == x.device and not torch.is_autocast_enabled())
    if not (on_device and lift_supported(dims)):
        y = _linear_stack(x.reshape(B * T, -1), weights, biases).view(B, T, J, 6)
        return pose_to_carla_rows(y, skel_type, kind, world_loc, world_rot, initial_rel_rot, want_rot, tensor_ops=True)
    x = x.detach().contiguous()
    weights, biases = [w.detach().contiguous() for w in weights], [b.detach().contiguous() for b in biases]
    skel_type = _require_device(skel_type, 'skel_type', torch.int32)
    wl = world_loc.detach().contiguous() if world_loc is not None else None
    wr = world_rot.detach().contiguous() if world_rot is not None else None
    init = initial_rel_rot.detach().contiguous() if initial_rel_rot is not None else None
    if lift_framework():
        y = fused_mlp(x.view(B * T, -1), weights, biases, image=image, image_is_current=image_is_current).view(B, T, J, 6)
        return pose_to_carla_rows(y, skel_type, kind, wl, wr, init, want_rot, max_blocks)
    lib = _lib.lib()
    n_image = lib.p2c_mlp_image_floats(ctypes.byref(_mlp_desc(x.view(B * T, -1), weights, biases)))
    if image is None:
        image, image_is_current = torch.empty(n_image, dtype=torch.float32, device=x.device), False
    elif image.numel() != n_image or image.device != x.device or image.dtype != torch.float32:
        raise RuntimeError('packed weight image of the wrong size / device')
    f32 = dict(dtype=torch.float32, device=x.device)
    bones, root = torch.empty(B, T, J, 6, **f32), torch.empty(B, T, 6, **f32)
    final = torch.empty(B, J, 3, 3, **f32) if kind == 'pose_changes_6d' else None
    rot = torch.empty(B, T, J, 3, 3, **f32) if want_rot else None
    d = _lift_desc(x, weights, biases, skel_type, kind, image, image_is_current, wl, wr, init, bones, root, final, rot, max_blocks)
    with torch.cuda.device(x.device):
        _lib.check(lib.p2c_lift_fwd(ctypes.byref(d), _stream()), 'p2c_lift_fwd')
    return bones, root, final, rot


def _lift_desc(x, weights, biases, skel_type, kind, image, image_is_current, world_loc, world_rot, initial_rel_rot, bones, root,
               final_rel_rot, rot, max_blocks=0):
    """``p2c_lift_desc`` over contiguous fp32 device tensors (x (B,T,52), skel_type int32)."""
    B, T = x.shape[:2]
    d = _lib.LiftDesc()
    d.mlp = _mlp_desc(x.view(B * T, -1), weights, biases)
    d.mlp.w_image, d.mlp.skip_pack = image.data_ptr(), int(bool(image_is_current))
    d.B, d.T, d.kind, d.max_blocks = B, T, KIND[kind], int(max_blocks)
    ref_loc, ref_rot = ref.get_relative_tensors(x.device)
    d.skel_type, d.ref_rel_loc, d.ref_rel_rot = skel_type.data_ptr(), ref_loc.data_ptr(), ref_rot.data_ptr()
    d.world_loc, d.world_rot, d.initial_rel_rot = _ptr(world_loc), _ptr(world_rot), _ptr(initial_rel_rot)
    d.bones, d.root, d.final_rel_rot, d.out_relative_pose_rot = bones.data_ptr(), _ptr(root), _ptr(final_rel_rot), _ptr(rot)
    return d


# ---- K35, K36: per-frame converters to CARLA poses, one launch each (csrc/p2c_smpl.hip, csrc/p2c_ik.hip) -------------------------
SMPL_CARLA_OUTPUTS = IK_CARLA_OUTPUTS = ('relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot', 'bones', 'root')
_CARLA_TAIL = {'relative_pose_rot': (J, 3, 3), 'absolute_pose_loc': (J, 3), 'absolute_pose_rot': (J, 3, 3), 'bones': (J, 6),
               'root': (6,)}


def identity_world(lead, like: Tensor) -> Tuple[Tensor, Tensor]:
    """``world_loc`` (*lead,3) of zeros and ``world_rot`` (*lead,3,3) of identities, dtype and device of ``like``."""
    lead = tuple(lead)
    return (torch.zeros(lead + (3,), dtype=like.dtype, device=like.device),
            torch.eye(3, dtype=like.dtype, device=like.device).expand(lead + (3, 3)).contiguous())


def _frames_to_carla(symbol: str, definition, framework: bool, x: Tensor, width: int, lead, skel_type: Tensor, world_loc, world_rot,
                     want, max_blocks: int, abs_table: bool) -> Dict[str, Tensor]:
    """What ``smpl_to_carla`` and ``locations_to_carla`` do behind their shape checks: ``x``, ``width`` values in each of its
    ``lead`` frames, goes to the C-ABI ``symbol`` with the relative reference tables (and the absolute rotations with
    ``abs_table``) when everything is fp32 on one device outside autocast and ``framework`` is off, else to ``definition``."""
    floats = [t for t in (x, world_loc, world_rot) if t is not None]
    if not _carla_kernel_ok(*floats) or framework:
        return definition(x, skel_type, world_loc, world_rot, want)
    device = x.device
    x = x.detach().reshape(lead + (width,)).contiguous()
    n = x.numel() // width
    st = skel_type.detach().to(device=device, dtype=torch.int32).contiguous()
    wl = world_loc.detach().contiguous() if world_loc is not None else None
    wr = world_rot.detach().contiguous() if world_rot is not None else None
    frames_per_type = max(n // max(st.numel(), 1), 1)
    result = {k: torch.empty(lead + _CARLA_TAIL[k], dtype=torch.float32, device=device) for k in SMPL_CARLA_OUTPUTS if k in want}
    if n == 0:
        return result
    tables = [t.data_ptr() for t in ref.get_relative_tensors(device)]
    if abs_table:
        tables.append(ref.get_absolute_tensors(device)[1].data_ptr())
    with torch.cuda.device(device):
        _lib.check(getattr(_lib.lib(), symbol)(x.data_ptr(), st.data_ptr(), frames_per_type, *tables, _ptr(wl), _ptr(wr),
                                               *(_ptr(result.get(k)) for k in SMPL_CARLA_OUTPUTS), n, int(max_blocks), _stream()),
                   symbol)
    return result


def smpl_framework() -> bool:
    """P2C_SMPL_FRAMEWORK=1: ``smpl_to_carla`` runs its tensor definition on the device (the comparison arm of
    tools/bench_smpl_retarget.py)."""
    return os.environ.get('P2C_SMPL_FRAMEWORK', '0') == '1'


@torch.no_grad()
def smpl_to_carla(body_pose: Tensor, skel_type: Tensor, world_loc: Optional[Tensor] = None, world_rot: Optional[Tensor] = None,
                  want: Sequence[str] = ('relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot'),
                  max_blocks: int = 0) -> Dict[str, Tensor]:
    """SMPL body poses as AMASS stores them -> CARLA poses (the reference's ``SMPLDataset.convert_smpl_to_carla``; definition:
    ``data/smpl/retarget.py``). ``body_pose`` (...,66) or (...,22,3) in original SMPL joint order; ``skel_type`` integer, its shape
    a prefix of the leading dimensions ((B,) for (B,T,66), (N,) for (N,66)). Returns a dict of the ``want``-ed among
    ``relative_pose_rot`` (...,26,3,3), ``absolute_pose_loc`` (...,26,3), ``absolute_pose_rot`` (...,26,3,3) and the rows of
    ``carla_pose_export``: ``bones`` (...,26,6) of (reference locations, ``relative_pose_rot``) and ``root`` (...,6) of
    ``world_loc`` (...,3) / ``world_rot`` (...,3,3), which come together. A predict / data-time operation: nothing is recorded
    for autograd. fp32 device tensors outside autocast take K35, one launch whatever is wanted; host tensors, fp64, other
    dtypes and ``P2C_SMPL_FRAMEWORK=1`` take the tensor definition. ``max_blocks`` lowers the kernel's grid cap (tests)."""
    from pedestrians_video_2_carla_amd.data.smpl import retarget
    want = tuple(want)
    lead = retarget.check_shapes(body_pose, skel_type, world_loc, world_rot, want)
    return _frames_to_carla('p2c_smpl_to_carla_fwd', retarget.convert_smpl_to_carla, smpl_framework(), body_pose, 66, lead,
                            skel_type, world_loc, world_rot, want, max_blocks, abs_table=True)


def ik_framework() -> bool:
    """P2C_IK_FRAMEWORK=1: ``locations_to_carla`` runs its tensor definition on the device (the comparison arm of
    tools/bench_ik.py)."""
    return os.environ.get('P2C_IK_FRAMEWORK', '0') == '1'


@torch.no_grad()
def locations_to_carla(loc: Tensor, skel_type: Tensor, world_loc: Optional[Tensor] = None, world_rot: Optional[Tensor] = None,
                       want: Sequence[str] = ('relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot'),
                       max_blocks: int = 0) -> Dict[str, Tensor]:
    """3-D joint locations -> the CARLA pose whose bones point along them (inverse kinematics over the 26-bone tree; definition:
    ``walker_control/inverse_kinematics.py``). ``loc`` (...,26,3) in ``CARLA_SKELETON`` order; ``skel_type`` integer, its shape a
    prefix of the leading dimensions ((B,) for (B,T,26,3), (N,) for (N,26,3)). Returns a dict of the ``want``-ed among
    ``relative_pose_rot`` (...,26,3,3), ``absolute_pose_loc`` (...,26,3) (the pose re-targeted to the reference bone lengths),
    ``absolute_pose_rot`` (...,26,3,3) and the rows of ``carla_pose_export``: ``bones`` (...,26,6) of (reference locations,
    ``relative_pose_rot``) and ``root`` (...,6) of ``world_loc`` (...,3) / ``world_rot`` (...,3,3), which come together. A predict-time
    operation: nothing is recorded for autograd. fp32 device tensors outside autocast take K36, one launch whatever is wanted;
    host tensors, fp64, other dtypes and ``P2C_IK_FRAMEWORK=1`` take the tensor definition on the tensor's device.
    ``max_blocks`` lowers the kernel's grid cap (tests)."""
    from pedestrians_video_2_carla_amd.walker_control import inverse_kinematics as ik
    want = tuple(want)
    lead = ik.check_shapes(loc, skel_type, world_loc, world_rot, want)
    return _frames_to_carla('p2c_loc_to_carla_fwd', ik.fit_carla_rotations, ik_framework(), loc, J * 3, lead, skel_type,
                            world_loc, world_rot, want, max_blocks, abs_table=False)


# ---- K37: CARLA rows resampled to another frame rate (csrc/p2c_resample.hip) ---------------------------------------------------
def resample_framework() -> bool:
    """P2C_RESAMPLE_FRAMEWORK=1: ``resample_carla_rows`` runs its tensor definition on the device (the comparison arm of
    tools/bench_resample.py)."""
    return os.environ.get('P2C_RESAMPLE_FRAMEWORK', '0') == '1'


@torch.no_grad()
def resample_carla_rows(bones: Tensor, root: Optional[Tensor] = None, *, src_fps, dst_fps, mode: str = 'slerp', carry=None,
                        first_frame: int = 0, first_output: int = 0, count: Optional[int] = None,
                        max_blocks: int = 0) -> Tuple[Tensor, Optional[Tensor]]:
    """Exported rows at the rate of a simulator's tick (definition: ``walker_control/resample.py``). ``bones`` (N,T,J,6) and
    ``root`` (N,T,6) or None, rows of (x, y, z, pitch, yaw, roll) at ``src_fps`` -> ``(bones (N,K,J,6), root (N,K,6) or None)`` at
    ``dst_fps``: output ``k`` sits at source position ``fl64(k * (src_fps / dst_fps))``; where that is a whole number the source
    row is copied bit for bit, elsewhere ``mode='slerp'`` interpolates locations linearly and rotations along the shortest arc
    and ``mode='hold'`` copies the row before. ``bones[:, 0]`` is global source frame ``first_frame``, ``out[:, 0]`` global output
    ``first_output``; ``count`` outputs are returned (None: all up to the last frame given); ``carry`` = ``(bones (N,J,6),
    root (N,6) or None)`` is source frame ``first_frame - 1`` (``CarlaResampler.push`` keeps it). Outputs that read a frame that
    is not given raise. Any J >= 1; views are made contiguous; nothing is recorded for autograd. fp32 device tensors outside
    autocast take K37 (one launch for bones and root); host tensors, fp64, other dtypes and ``P2C_RESAMPLE_FRAMEWORK=1`` take the
    tensor definition. ``max_blocks`` lowers the kernel's grid cap (tests)."""
    from pedestrians_video_2_carla_amd.walker_control import resample as rs
    ratio = rs.rate_ratio(src_fps, dst_fps)
    mode_id = rs.check_mode(mode)
    first_frame, first_output = int(first_frame), int(first_output)
    cb, cr = rs.check_rows(bones, root, carry)
    N, T, n_joints, _ = bones.shape
    if count is None:
        count = max(rs.output_count(first_frame + T - 1, ratio) - first_output, 0)
    count = int(count)
    if first_frame == 0:                       # nothing lies before the first frame of a video
        cb = cr = None
    rs.check_span(first_output, count, ratio, first_frame, T, cb is not None, 'resample_carla_rows')
    given = [t for t in (bones, root, cb, cr) if t is not None]
    if not _carla_kernel_ok(*given) or resample_framework():
        return rs.resample_rows(bones, root, cb, cr, ratio, mode_id == rs.MODES['hold'], first_frame, first_output, count)
    src_b, src_r, cb, cr = (t.detach().contiguous() if t is not None else None for t in (bones, root, cb, cr))
    out_b = torch.empty((N, count, n_joints, 6), dtype=torch.float32, device=bones.device)
    out_r = torch.empty((N, count, 6), dtype=torch.float32, device=bones.device) if root is not None else None
    if N == 0 or count == 0:
        return out_b, out_r
    with torch.cuda.device(bones.device):
        _lib.check(_lib.lib().p2c_carla_resample_fwd(src_b.data_ptr(), _ptr(src_r), _ptr(cb), _ptr(cr), out_b.data_ptr(), _ptr(out_r),
                                                     N, T, n_joints, count, first_output, first_frame, ratio, mode_id,
                                                     int(max_blocks), _stream()), 'p2c_carla_resample_fwd')
    return out_b, out_r


# ---- K39: CARLA rows smoothed along time (csrc/p2c_smooth.hip) -----------------------------------------------------------------
def smooth_framework() -> bool:
    """P2C_SMOOTH_FRAMEWORK=1: ``smooth_carla_rows`` runs its tensor definition on the device (the comparison arm of
    tools/bench_smooth.py)."""
    return os.environ.get('P2C_SMOOTH_FRAMEWORK', '0') == '1'


_SMOOTH_TABLES: Dict[Tuple, Tensor] = {}


def _smooth_table(sigma: float, R: int, device) -> Tensor:
    """The gaussian weight table of (sigma, R) on ``device``, formed once."""
    from pedestrians_video_2_carla_amd.walker_control import smooth as sm
    key = (sigma, R, str(device))
    if key not in _SMOOTH_TABLES:
        if len(_SMOOTH_TABLES) >= 64:
            _SMOOTH_TABLES.clear()
        _SMOOTH_TABLES[key] = sm.gauss_table(sigma, R).to(device)
    return _SMOOTH_TABLES[key]


@torch.no_grad()
def smooth_carla_rows(bones: Tensor, root: Optional[Tensor] = None, *, mode: str, sigma=None, radius=None, fps=None,
                      min_cutoff=1.0, beta_loc=0.0, beta_rot=0.0, d_cutoff=1.0, state=None, first_frame: int = 0,
                      first_output: int = 0, count: Optional[int] = None, last_frame: Optional[int] = None,
                      max_blocks: int = 0) -> Tuple[Tensor, Optional[Tensor], Optional[Tuple]]:
    """Exported rows smoothed along time (definition: ``walker_control/smooth.py``). ``bones`` (N,T,J,6) and ``root`` (N,T,6) or
    None, rows of (x, y, z, pitch, yaw, roll) -> ``(bones, root or None, state or None)``; rotations are filtered as quaternions.
    ``mode='gaussian'`` (``sigma`` in frames, ``radius`` R <= 32, default ``ceil(3 sigma)``): output frame t is the weighted mean
    of source frames ``max(0, t - R) .. min(t + R, last_frame)``. ``bones[:, 0]`` is global source frame ``first_frame``,
    ``out[:, 0]`` global output ``first_output``; ``last_frame`` is the video's last global index (None: the last frame given;
    -1: not known yet, every window must then lie inside the given frames); ``count`` outputs are returned (None: all that can
    be formed). A window that reads a frame that is not given raises. R = 0 or sigma = 0 copies the rows; the state is None.
    ``mode='one_euro'`` (``fps``, ``min_cutoff``, ``beta_loc``, ``beta_rot``, ``d_cutoff``): the causal one-euro filter over the T
    frames; ``state`` = ``(bones (N,J,12), root (N,12) or None)`` continues a video (None: frame 0 starts one and is copied),
    and the state after the last frame is returned; the given one is left as it was. Any J >= 1; views are made contiguous;
    nothing is recorded for autograd. fp32 device tensors outside autocast take K39 (one launch for bones and root); host
    tensors, fp64, other dtypes and ``P2C_SMOOTH_FRAMEWORK=1`` take the tensor definition. ``max_blocks`` lowers the kernel's
    grid cap (tests)."""
    from pedestrians_video_2_carla_amd.walker_control import resample as rs, smooth as sm
    sm.check_mode(mode)
    rs.check_rows(bones, root, None, 'smooth_carla_rows')
    N, T, n_joints, _ = bones.shape
    f32 = dict(dtype=torch.float32, device=bones.device)
    if mode == 'one_euro':
        params = sm.euro_params(fps, min_cutoff, beta_loc, beta_rot, d_cutoff)
        sb, sr = sm.check_state(bones, root, state)
        if T == 0:
            return bones.detach().clone(), (root.detach().clone() if root is not None else None), state
        given = [t for t in (bones, root, sb, sr) if t is not None]
        if not _carla_kernel_ok(*given) or smooth_framework():
            return sm.euro_rows(bones, root, sb, sr, params)
        src_b, src_r = (t.detach().contiguous() if t is not None else None for t in (bones, root))
        new_b = sb.detach().clone().contiguous() if sb is not None else torch.empty((N, n_joints, sm.STATE), **f32)
        new_r = None
        if root is not None:
            new_r = sr.detach().clone().contiguous() if sr is not None else torch.empty((N, sm.STATE), **f32)
        out_b = torch.empty((N, T, n_joints, 6), **f32)
        out_r = torch.empty((N, T, 6), **f32) if root is not None else None
        if N > 0:
            with torch.cuda.device(bones.device):
                _lib.check(_lib.lib().p2c_carla_smooth_euro_fwd(
                    src_b.data_ptr(), _ptr(src_r), new_b.data_ptr(), _ptr(new_r), out_b.data_ptr(), _ptr(out_r), N, T, n_joints,
                    int(sb is not None), params['fps'], params['min_cutoff'], params['beta_loc'], params['beta_rot'],
                    params['d_cutoff'], int(max_blocks), _stream()), 'p2c_carla_smooth_euro_fwd')
        return out_b, out_r, (new_b, new_r)
    sigma, R = sm.gauss_params(sigma, radius)
    first_frame, first_output = int(first_frame), int(first_output)
    last_frame = first_frame + T - 1 if last_frame is None else int(last_frame)
    if count is None:
        count = max((last_frame if last_frame >= 0 else first_frame + T - 1 - R) - first_output + 1, 0)
    count = int(count)
    sm.check_gauss_span(first_output, count, R, first_frame, T, last_frame, 'smooth_carla_rows')
    given = [t for t in (bones, root) if t is not None]
    if not _carla_kernel_ok(*given) or smooth_framework():
        return (*sm.gauss_rows(bones, root, _smooth_table(sigma, R, bones.device), R, first_frame, first_output, count, last_frame), None)
    src_b, src_r = (t.detach().contiguous() if t is not None else None for t in (bones, root))
    out_b = torch.empty((N, count, n_joints, 6), **f32)
    out_r = torch.empty((N, count, 6), **f32) if root is not None else None
    if N == 0 or count == 0:
        return out_b, out_r, None
    table = _smooth_table(sigma, R, bones.device)
    with torch.cuda.device(bones.device):
        _lib.check(_lib.lib().p2c_carla_smooth_gauss_fwd(src_b.data_ptr(), _ptr(src_r), out_b.data_ptr(), _ptr(out_r),
                                                         table.data_ptr(), N, T, n_joints, count, first_frame, first_output,
                                                         last_frame, R, int(max_blocks), _stream()),
                   'p2c_carla_smooth_gauss_fwd')
    return out_b, out_r, None


# ---- K40: root motion of CARLA rows from their planted feet (csrc/p2c_root_motion.hip) -----------------------------------------
def root_motion_framework() -> bool:
    """P2C_ROOT_MOTION_FRAMEWORK=1: ``root_motion_carla_rows`` runs its tensor definition on the device (the comparison arm of
    tools/bench_root_motion.py)."""
    return os.environ.get('P2C_ROOT_MOTION_FRAMEWORK', '0') == '1'


def root_motion_tile() -> int:
    """Frames of a tile of K40: the length at which a video takes more than one pass of the scan."""
    return int(_lib.lib().p2c_carla_root_motion_tile())


@torch.no_grad()
def root_motion_carla_rows(bones: Tensor, root: Optional[Tensor] = None, *, ground=None, state=None, first_frame: int = 0,
                           want: Sequence[str] = ('root',), mapping=None, max_blocks: int = 0) -> Dict[str, object]:
    """Root rows that keep the supporting foot planted (definition: ``walker_control/root_motion.py``). ``bones`` (N,T,26,6) and
    ``root`` (N,T,6) or None (all-zero root rows), rows of (x, y, z, pitch, yaw, roll) -> a dict with the ``want``-ed among
    ``root`` (N,T,6: x and y moved by the running sum of the steps, z put on ``ground`` when that is given, the angles bit for
    bit), ``steps`` (N,T,2) int32 in quanta of 2^-10 of the length unit and ``contact`` (N,T) int8 (0..3 = foot R, toe R, foot L,
    toe L; -1 where a frame pair had a non-finite value), and always ``state`` = ``(S (N,2) int64, points (N,4,3))`` after the
    last frame. ``bones[:, 0]`` is global frame ``first_frame``; ``first_frame > 0`` continues a video and needs the ``state`` the
    call before returned (``CarlaRootMotion.push`` keeps it; with ``first_frame = 0`` a state is not read). Each clip is a video
    of its own. The CARLA skeleton is the only tree: another J raises. Views are made contiguous; nothing is recorded for
    autograd. fp32 device tensors outside autocast take K40; host tensors, fp64, other dtypes and
    ``P2C_ROOT_MOTION_FRAMEWORK=1`` take the tensor definition. ``mapping``: None / 'auto' chooses by size between 'per_video' (1:
    a workgroup per video, one launch) and 'frame_parallel' (2: two launches over (video, tile)); all give the same bits.
    ``max_blocks`` lowers the kernels' grid cap (tests)."""
    from pedestrians_video_2_carla_amd.walker_control import root_motion as rm
    rm.check_bones(bones, root)
    want, mapping_id, z0, first_frame = rm.check_want(want), rm.check_mapping(mapping), rm.check_ground(ground), int(first_frame)
    state = rm.check_state(bones, state, first_frame)
    N, T = bones.shape[:2]
    given = [t for t in (bones, root, state[1] if state is not None else None) if t is not None]   # the int64 offset is on their device
    if T == 0 or not _carla_kernel_ok(*given) or root_motion_framework():
        full = rm.root_motion_rows(bones, root, z0, state, first_frame)
        return {**{k: full[k] for k in want}, 'state': full['state']}
    lib = _lib.lib()
    src_b, src_r = (t.detach().contiguous() if t is not None else None for t in (bones, root))
    in_s, in_p = (t.detach().contiguous() for t in state) if state is not None and first_frame > 0 else (None, None)
    dev = bones.device
    out_root = torch.empty((N, T, 6), dtype=torch.float32, device=dev)
    steps = torch.empty((N, T, 2), dtype=torch.int32, device=dev) if 'steps' in want else None
    contact = torch.empty((N, T), dtype=torch.int8, device=dev) if 'contact' in want else None
    new_s, new_p = torch.empty((N, 2), dtype=torch.int64, device=dev), torch.empty((N, 4, 3), dtype=torch.float32, device=dev)
    if N > 0:
        ws_bytes = int(lib.p2c_carla_root_motion_workspace(N, T, mapping_id))
        if ws_bytes < 0:
            raise _lib.P2CError(f'root_motion_carla_rows: {N} videos of {T} frames are more than K40 takes')
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev) if ws_bytes else None
        with torch.cuda.device(dev):
            _lib.check(lib.p2c_carla_root_motion_fwd(src_b.data_ptr(), _ptr(src_r), _ptr(in_s), _ptr(in_p), out_root.data_ptr(),
                                                     _ptr(steps), _ptr(contact), new_s.data_ptr(), new_p.data_ptr(), N, T,
                                                     first_frame, 0.0 if z0 is None else z0, int(z0 is not None), mapping_id,
                                                     int(max_blocks), _ptr(ws), _stream()), 'p2c_carla_root_motion_fwd')
    out = {'root': out_root, 'steps': steps, 'contact': contact}
    return {**{k: out[k] for k in want}, 'state': (new_s, new_p)}


# ---- K41: CARLA rows as a loop: cycle search and seam blend (csrc/p2c_loop.hip) ------------------------------------------------
def loop_framework() -> bool:
    """P2C_LOOP_FRAMEWORK=1: ``find_carla_loop`` and ``loop_carla_rows`` run their tensor definitions on the device (the
    comparison arm of tools/bench_loop.py)."""
    return os.environ.get('P2C_LOOP_FRAMEWORK', '0') == '1'


def _loop_kernel_ok(bones: Tensor, frames: int, *more: Optional[Tensor]) -> bool:
    """K41's domain: fp32 on the device outside autocast, 1 <= J <= 64, 2 <= T <= 16 384, row counts under 2^31."""
    from pedestrians_video_2_carla_amd.walker_control import loop as lp
    N, T, n_joints, _ = bones.shape
    return (_carla_kernel_ok(bones, *(t for t in more if t is not None)) and not loop_framework()
            and 1 <= n_joints <= lp.MAX_J and 2 <= T <= lp.MAX_T
            and N * max(T, frames) * (n_joints + 1) < 2 ** 31)


@torch.no_grad()
def find_carla_loop(bones: Tensor, *, blend, min_period, max_period=None, weights=None, want: Sequence[str] = ('loop',),
                    max_blocks: int = 0) -> Dict[str, Tensor]:
    """The cycle of every video that closes best (definition: ``walker_control/loop.py``). ``bones`` (N,T,J,6), rows of (x, y, z,
    pitch, yaw, roll) -> a dict with ``loop`` (N,2) int64, the pair ``(s, e)``: frames ``s .. e - 1`` and then ``s`` again, and
    ``loop_cost`` (N), its cost; with ``'cost'`` in ``want`` also ``cost`` (N,T,T), every pair's. The cost of a pair compares the
    ``blend`` frames that lead into ``s`` and ``s`` itself with those that lead into ``e`` and ``e``, bone by bone, as
    ``weights[j] sin^2`` of half the angle between the two rotations (``weights`` (J) finite and >= 0, default ones); pairs with
    ``blend <= s``, ``s + min_period <= e <= s + max_period`` (default T) and ``e <= T - 1`` are admissible, the others cost
    ``+inf``. The smallest finite cost wins, ties to the smallest ``s``, then the smallest ``e``; a video without one gets ``(-1,
    -1)`` and NaN. What is returned for a key does not depend on what else is asked for. Views are made contiguous; nothing is
    recorded for autograd. fp32 device tensors outside autocast with J <= 64 and 2 <= T <= 16 384 take K41; host tensors, fp64,
    other dtypes and sizes and ``P2C_LOOP_FRAMEWORK=1`` take the tensor definition. ``max_blocks`` lowers the kernel's grid cap
    (tests)."""
    from pedestrians_video_2_carla_amd.walker_control import loop as lp, resample as rs
    blend = lp.check_blend(blend)
    min_period, max_period = lp.check_periods(min_period, max_period)
    want = lp.check_want(want)
    rs.check_rows(bones, None, None, 'find_carla_loop')
    w = lp.check_weights(weights, bones)
    N, T, n_joints, _ = bones.shape
    if not _loop_kernel_ok(bones, 0, w):
        full = lp.find_loop(bones, blend, min_period, max_period, w)
        return {k: full[k] for k in ('loop', 'loop_cost') + (('cost',) if 'cost' in want else ())}
    lib = _lib.lib()
    dev = bones.device
    src, w = bones.detach().contiguous(), (w.contiguous() if w is not None else None)
    loop = torch.empty((N, 2), dtype=torch.int64, device=dev)
    loop_cost = torch.empty((N,), dtype=torch.float32, device=dev)
    cost = torch.empty((N, T, T), dtype=torch.float32, device=dev) if 'cost' in want else None
    if N > 0:
        ws_bytes = int(lib.p2c_carla_loop_find_workspace(N, T, n_joints, blend))
        if ws_bytes < 0:
            raise _lib.P2CError(f'find_carla_loop: {N} videos of {T} frames are more than K41 takes')
        ws = torch.empty((ws_bytes // 8,), dtype=torch.int64, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.p2c_carla_loop_find_fwd(src.data_ptr(), _ptr(w), loop.data_ptr(), loop_cost.data_ptr(), _ptr(cost), N, T,
                                                   n_joints, blend, min(min_period, lp.INT_MAX),
                                                   lp.INT_MAX if max_period is None else min(max_period, lp.INT_MAX),
                                                   int(max_blocks), ws.data_ptr(), _stream()), 'p2c_carla_loop_find_fwd')
    out = {'loop': loop, 'loop_cost': loop_cost}
    if cost is not None:
        out['cost'] = cost
    return out


@torch.no_grad()
def loop_carla_rows(bones: Tensor, root: Optional[Tensor] = None, *, loop, blend, frames, first_output: int = 0,
                    max_blocks: int = 0) -> Tuple[Tensor, Optional[Tensor]]:
    """The cycles ``find_carla_loop`` chose, played (definition: ``walker_control/loop.py``). ``bones`` (N,T,J,6) and ``root``
    (N,T,6) or None, ``loop`` (N,2) whole numbers -> ``(bones (N,frames,J,6), root (N,frames,6) or None)``: outputs
    ``first_output .. first_output + frames - 1`` of an animation that plays frames ``s .. e - 1`` over and over. Outside the last
    ``blend`` frames of a cycle the source rows are copied bit for bit; inside them they are blended (K37's interpolation)
    towards the frames that lead into ``s``, so that the cycle closes. Root x and y advance by ``root[e] - root[s]`` a cycle, as
    a product formed in fp64: an output depends on its index alone and pieces give the bits of one call. A video with ``loop =
    (-1, -1)`` plays NaN rows; another pair that is not ``blend <= s < e <= T - 1`` raises. Views are made contiguous; nothing
    is recorded for autograd. fp32 device tensors outside autocast with J <= 64 and 2 <= T <= 16 384 take K41 (one launch for
    bones and root); host tensors, fp64, other dtypes and sizes and ``P2C_LOOP_FRAMEWORK=1`` take the tensor definition.
    ``max_blocks`` lowers the kernel's grid cap (tests)."""
    from pedestrians_video_2_carla_amd.walker_control import loop as lp, resample as rs
    blend, frames = lp.check_blend(blend), lp.check_frames(frames)
    first_output = int(first_output)
    if first_output < 0:
        raise ValueError(f'loop_carla_rows: first_output = {first_output}; not negative expected')
    rs.check_rows(bones, root, None, 'loop_carla_rows')
    pairs = lp.check_loop(loop, bones, blend)
    N, T, n_joints, _ = bones.shape
    if N == 0 or frames == 0 or first_output + frames > 2 ** 40 or not _loop_kernel_ok(bones, frames, root):
        return lp.play_rows(bones, root, pairs, blend, frames, first_output)
    src_b, src_r = (t.detach().contiguous() if t is not None else None for t in (bones, root))
    out_b = torch.empty((N, frames, n_joints, 6), dtype=torch.float32, device=bones.device)
    out_r = torch.empty((N, frames, 6), dtype=torch.float32, device=bones.device) if root is not None else None
    with torch.cuda.device(bones.device):
        _lib.check(_lib.lib().p2c_carla_loop_play_fwd(src_b.data_ptr(), _ptr(src_r), pairs.contiguous().data_ptr(), out_b.data_ptr(),
                                                      _ptr(out_r), N, T, n_joints, frames, first_output, blend, int(max_blocks),
                                                      _stream()), 'p2c_carla_loop_play_fwd')
    return out_b, out_r


# ---- K33: decoded video clips -> the pose-estimation flow's input frames (csrc/p2c_frames.hip) ---------------------------------
FRAMES_MAX_TARGET = 1024             # the largest target size K33 is dispatched for


def frames_framework() -> bool:
    """P2C_FRAMES_FRAMEWORK=1: ``clip_frames`` runs the tensor definition (data/base/video.py) on the clips' device (the comparison
    arm of tools/bench_frames.py)."""
    return os.environ.get('P2C_FRAMES_FRAMEWORK', '0') == '1'


@dataclass
class PackedClips:
    """N decoded clips in one uint8 buffer: clip i is the dense (T, H_i, W_i, 3) block at ``offsets[i]`` (bytes)."""
    buffer: Tensor
    offsets: Tuple[int, ...]
    shapes: Tuple[Tuple[int, int, int], ...]

    def __len__(self):
        return len(self.shapes)

    def clip(self, i: int) -> Tensor:
        T, H, W = self.shapes[i]
        return self.buffer[self.offsets[i]:self.offsets[i] + T * H * W * 3].view(T, H, W, 3)


def pack_clips(clips: Sequence[Tensor]) -> PackedClips:
    """One buffer from a list of uint8 (T, H_i, W_i, 3) tensors on one device (a single clip that is already dense is not copied)."""
    shapes, offsets, at = [], [], 0
    for c in clips:
        if c.ndim != 4 or c.shape[3] != 3 or c.dtype != torch.uint8:
            raise RuntimeError(f'clip_frames: a clip is uint8 (T,H,W,3), got {c.dtype} {tuple(c.shape)}')
        shapes.append(tuple(int(v) for v in c.shape[:3]))
        offsets.append(at)
        at += c.numel()
    buffer = clips[0].contiguous().view(-1) if len(clips) == 1 else torch.cat([c.reshape(-1) for c in clips])
    return PackedClips(buffer, tuple(offsets), tuple(shapes))


def _frames_sizes(packed: PackedClips, target_size: int, canvas):
    """Per clip: the (height, width) that is resized -- the canvas under the crop -- and the size written."""
    from pedestrians_video_2_carla_amd.data.base.video import resized_size
    src = [(int(canvas[i]),) * 2 if canvas is not None else (H, W) for i, (_, H, W) in enumerate(packed.shapes)]
    return src, [resized_size(h, w, target_size) for h, w in src]


def clip_frames_supported(clips, target_size: int, canvas=None) -> bool:
    """What K33 covers: uint8 clips on the device, frame and canvas sides up to 8 192 (int32 level counts), a target size in
    [1, 1024]; everything else, and ``P2C_FRAMES_FRAMEWORK=1``, is the tensor path."""
    packed = clips if isinstance(clips, PackedClips) else None
    tensors = [packed.buffer] if packed is not None else list(clips)
    if frames_framework() or not all(isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.device == tensors[0].device
                                     for t in tensors):
        return False
    shapes = packed.shapes if packed is not None else [tuple(t.shape[:3]) for t in tensors]
    side = max(max(s[1], s[2]) for s in shapes)
    if canvas is not None:
        side = max(side, max(int(c) for c in canvas))
    return 1 <= int(target_size) <= FRAMES_MAX_TARGET and side <= _lib.P2C_FRAMES_MAX_SIDE


def _clip_frames_tensor(packed: PackedClips, target_size: int, centres, canvas) -> Tensor:
    """The definition: per clip the reference's paste (around the given integer centres), then ``VideoToResNet``."""
    from pedestrians_video_2_carla_amd.data.base.video import VideoToResNet, extract_bbox_from_frame
    to_resnet, out = VideoToResNet(target_size), []
    if isinstance(centres, Tensor):
        T = packed.shapes[0][0]
        centres = centres.detach().cpu().numpy().reshape(len(packed), T, 2)
    for i in range(len(packed)):
        clip = packed.clip(i)
        if canvas is not None:
            c, (T, H, W) = int(canvas[i]), packed.shapes[i]
            pasted = clip.new_zeros((T, c, c, 3))
            for t in range(T):
                extract_bbox_from_frame(pasted[t], clip[t], (c // 2, c // 2), centres[i][t], (W, H))
            clip = pasted
        out.append(to_resnet(clip))
    return torch.stack(out)


def clip_frames(clips, target_size: int, centres=None, canvas=None) -> Tensor:
    """Decoded clips -> the pose-estimation flow's frames (N,T,3,h,w) fp32: the reference's ``crop_bbox`` paste (when ``canvas`` is
    given), ``equalize`` per frame and channel, the antialiased bilinear resize of ``VideoToResNet`` and the ImageNet
    normalisation -- K33, two launches for the whole batch; the canvas, the equalized clip and the float image are never formed.

    ``clips``: a list of uint8 (T, H_i, W_i, 3) tensors or a ``PackedClips``. ``canvas``: per clip the canvas size of
    ``data.base.video.crop_geometry`` (None: no crop); ``centres``: with it, per clip the (T,2) integer (x, y) centres -- a list
    of host arrays (one small upload) or an int32 device tensor (N,T,2) (nothing is copied: capturable). All clips must have the
    same T and resize to the same (h, w). Host clips, sizes ``clip_frames_supported`` refuses and ``P2C_FRAMES_FRAMEWORK=1`` run
    the tensor definition on the clips' device."""
    import numpy as np
    packed = clips if isinstance(clips, PackedClips) else pack_clips(list(clips))
    N = len(packed)
    if N == 0:
        raise RuntimeError('clip_frames: no clips')
    if (canvas is None) != (centres is None) or (canvas is not None and len(canvas) != N):
        raise RuntimeError('clip_frames: canvas and centres come together, one entry per clip')
    T = packed.shapes[0][0]
    if T < 1 or any(s[0] != T for s in packed.shapes):
        raise RuntimeError(f'clip_frames: every clip needs the same T >= 1, got {[s[0] for s in packed.shapes]}')
    _, sizes = _frames_sizes(packed, target_size, canvas)
    if len(set(sizes)) != 1:
        raise RuntimeError(f'clip_frames: the clips resize to different sizes {sorted(set(sizes))}')
    if not clip_frames_supported(packed, target_size, canvas):
        return _clip_frames_tensor(packed, target_size, centres, canvas)
    lib = _lib.lib()
    dev = packed.buffer.device
    if canvas is None:
        centres_dev = None
    elif isinstance(centres, Tensor):
        if not centres.is_cuda or centres.dtype != torch.int32 or centres.numel() != N * T * 2:
            raise RuntimeError('clip_frames: a tensor of centres is int32 (N,T,2) on the device')
        centres_dev = centres.contiguous()
    else:
        host = np.ascontiguousarray(np.stack([np.asarray(c) for c in centres]).reshape(N, T, 2).clip(-2 ** 30, 2 ** 30), dtype=np.int32)
        centres_dev = torch.from_numpy(host).to(dev)
    h, w = sizes[0]
    out = torch.empty(N, T, 3, h, w, dtype=torch.float32, device=dev)
    workspace = torch.empty(lib.p2c_clip_frames_workspace_bytes(min(N, _lib.P2C_FRAMES_MAX_CLIPS) * T) // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        for i0 in range(0, N, _lib.P2C_FRAMES_MAX_CLIPS):              # the per-clip table travels in the kernel arguments
            n = min(_lib.P2C_FRAMES_MAX_CLIPS, N - i0)
            d = _lib.ClipFramesDesc()
            d.N, d.T, d.src_bytes, d.src = n, T, packed.buffer.numel(), packed.buffer.data_ptr()
            d.centres = None if centres_dev is None else centres_dev.data_ptr() + i0 * T * 2 * 4
            d.workspace, d.out = workspace.data_ptr(), out[i0].data_ptr()
            for k in range(n):
                _, H, W = packed.shapes[i0 + k]
                clip = d.clips[k]
                clip.offset, clip.H, clip.W, clip.out_h, clip.out_w = packed.offsets[i0 + k], H, W, h, w
                clip.canvas = 0 if canvas is None else int(canvas[i0 + k])
            _lib.check(lib.p2c_clip_frames_fwd(ctypes.byref(d), _stream()), 'p2c_clip_frames_fwd')
    return out


# ---- K34: skeleton clips -> the video logger's uint8 frames (csrc/p2c_render.hip) ---------------------------------------------
RENDER_MAX_COORD = _lib.P2C_RENDER_MAX_COORD
_RENDER_CHUNK = 1 << 23               # elements of one (frames, primitives, H, W) mask block of the tensor definition


def render_framework() -> bool:
    """P2C_RENDER_FRAMEWORK=1: ``render_points`` runs its tensor definition on the points' device (the comparison arm of
    tools/bench_render.py)."""
    return os.environ.get('P2C_RENDER_FRAMEWORK', '0') == '1'


def _render_panels(panels):
    """Checked panels: None or (points (V,T,J,C>=2) float, colors (J,3) uint8, edges (E,2) int64), all on the points' device."""
    out, lead = [], None
    for k, panel in enumerate(panels):
        if panel is None:
            out.append(None)
            continue
        points, colors, edges = panel
        if not (isinstance(points, Tensor) and points.ndim == 4 and points.shape[-1] >= 2 and points.is_floating_point()):
            raise RuntimeError(f'render_points: panel {k}: points are float (V,T,J,C>=2), got {getattr(points, "shape", None)}')
        J, dev = points.shape[2], points.device
        if lead is None:
            lead = points
        elif tuple(points.shape[:2]) != tuple(lead.shape[:2]) or dev != lead.device:
            raise RuntimeError(f'render_points: panel {k} has (V,T) {tuple(points.shape[:2])} on {dev}; '
                               f'{tuple(lead.shape[:2])} on {lead.device} expected')
        colors = torch.as_tensor(colors)
        if tuple(colors.shape) != (J, 3) or colors.dtype != torch.uint8:
            raise RuntimeError(f'render_points: panel {k}: colors are uint8 ({J},3), got {colors.dtype} {tuple(colors.shape)}')
        edges = torch.as_tensor(edges if edges is not None else [], dtype=torch.int64).reshape(-1, 2)
        if edges.numel() and bool(((edges < 0) | (edges >= J)).any()):
            raise RuntimeError(f'render_points: panel {k}: an edge names a joint outside [0, {J})')
        out.append((points.detach(), colors.to(dev), edges.to(dev)))
    if lead is None:
        raise RuntimeError('render_points: at least one panel needs points (they carry V and T)')
    return out, lead


def _render_last_cover(best: Tensor, mask: Tensor, first: int) -> None:
    """best (n,H,W) <- max(best, index + 1 of the last primitive of ``mask`` (n,P,H,W) that covers the pixel), indices from ``first``."""
    index = torch.arange(first + 1, first + 1 + mask.shape[1], device=mask.device).view(1, -1, 1, 1)
    torch.maximum(best, (index * mask).amax(1), out=best)


def _render_panel_tensor(points: Tensor, colors: Tensor, edges: Tensor, H: int, W: int, radius: int, line_width: int) -> Tensor:
    """One panel, (V,T,H,W,3) uint8: masks over (frames, primitive, H, W) -- bones in edge order, then joints in index order -- the
    last covering primitive by ``amax`` of (index + 1) * mask, then the colour gathered. int64 throughout (include/p2c.h, K34)."""
    V, T, J = points.shape[:3]
    dev, N = points.device, V * T
    xy = torch.round(points[..., :2].to(torch.float32)).reshape(N, J, 2)
    valid = (torch.isfinite(xy) & (xy.abs() <= RENDER_MAX_COORD)).all(-1)                       # (N,J)
    c = torch.where(valid[..., None], xy, torch.zeros_like(xy)).to(torch.int64)
    E = edges.shape[0] if line_width > 0 else 0
    table = torch.cat([colors.new_zeros(1, 3), colors[edges[:E, 1]], colors])                   # 0: background
    px = torch.arange(W, device=dev, dtype=torch.int64).view(1, 1, 1, W)
    py = torch.arange(H, device=dev, dtype=torch.int64).view(1, 1, H, 1)
    out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    L2, r2 = int(line_width) ** 2, int(radius) ** 2
    per = max(1, _RENDER_CHUNK // (H * W))                   # (frame, primitive) pairs per block
    n_step = max(1, per // max(1, max(E, J)))
    p_step = max(1, per // n_step)
    for n0 in range(0, N, n_step):
        cn, vn = c[n0:n0 + n_step], valid[n0:n0 + n_step]
        best = torch.zeros(cn.shape[0], H, W, dtype=torch.int64, device=dev)
        for e0 in range(0, E, p_step):
            a, b = edges[e0:e0 + p_step, 0], edges[e0:e0 + p_step, 1]
            ca, cb = cn[:, a], cn[:, b]                                                          # (n,P,2)
            ok = (vn[:, a] & vn[:, b])[..., None, None]
            ax, ay, bx, by = (t[..., None, None] for t in (ca[..., 0], ca[..., 1], cb[..., 0], cb[..., 1]))
            dx, dy, qx, qy = bx - ax, by - ay, px - ax, py - ay
            s, n = qx * dx + qy * dy, dx * dx + dy * dy
            near_a = 4 * (qx * qx + qy * qy) <= L2
            near_b = 4 * ((px - bx) ** 2 + (py - by) ** 2) <= L2
            cross = qx * dy - qy * dx
            between = 4 * cross * cross <= L2 * n
            mask = torch.where(s <= 0, near_a, torch.where(s >= n, near_b, between)) & ok
            _render_last_cover(best, mask, e0)
        for j0 in range(0, J, p_step):
            cj = cn[:, j0:j0 + p_step]
            ex, ey = px - cj[..., 0, None, None], py - cj[..., 1, None, None]
            mask = (ex * ex + ey * ey <= r2) & vn[:, j0:j0 + p_step, None, None]
            _render_last_cover(best, mask, E + j0)
        out[n0:n0 + n_step] = table[best]
    return out.view(V, T, H, W, 3)


def _render_points_tensor(panels, size, layout, radius: int = 2, line_width: int = 0) -> Tensor:
    """The definition of ``render_points`` on tensor ops (and its fallback): checked ``panels`` as ``_render_panels`` returns them."""
    (H, W), (rows, cols) = size, layout
    lead = next(p[0] for p in panels if p is not None)
    V, T = lead.shape[:2]
    out = torch.zeros(V, T, rows * H, cols * W, 3, dtype=torch.uint8, device=lead.device)
    for k, panel in enumerate(panels):
        if panel is not None:
            r, c = divmod(k, cols)
            out[:, :, r * H:(r + 1) * H, c * W:(c + 1) * W] = _render_panel_tensor(*panel, H, W, radius, line_width)
    return out


def _render_desc(panels, V, T, H, W, rows, cols, radius, line_width, max_blocks=0):
    """``p2c_render_points_desc`` without pointers: the shapes ``p2c_render_points_supported`` judges. More panels than the
    descriptor holds are counted, not described."""
    d = _lib.RenderPointsDesc()
    d.V, d.T, d.H, d.W, d.rows, d.cols, d.n_panels = V, T, H, W, rows, cols, len(panels)
    d.radius, d.line_width, d.max_blocks = int(radius), int(line_width), int(max_blocks)
    for k, panel in enumerate(panels[:_lib.P2C_RENDER_MAX_PANELS]):
        if panel is not None:
            points, _colors, edges = panel
            d.panels[k].J, d.panels[k].E, d.panels[k].C = points.shape[2], edges.shape[0], points.shape[3]
    return d


def render_points_supported(panels, size, layout, radius: int = 2, line_width: int = 0) -> bool:
    """What K34 covers, asked of the library (``p2c_render_points_supported``): at most 8 panels, J and E up to 64 per panel, H and W
    up to 8192 with W a multiple of 4, radius and line width up to 64 -- for fp32 points on the device and without
    ``P2C_RENDER_FRAMEWORK=1``."""
    return _render_supported(*_render_panels(panels), size, layout, radius, line_width)


def _render_supported(checked, lead, size, layout, radius, line_width) -> bool:
    if render_framework() or not all(p is None or (p[0].is_cuda and p[0].dtype == torch.float32) for p in checked):
        return False
    d = _render_desc(checked, lead.shape[0], lead.shape[1], int(size[0]), int(size[1]), int(layout[0]), int(layout[1]), radius, line_width)
    for k, panel in enumerate(checked[:_lib.P2C_RENDER_MAX_PANELS]):
        if panel is not None:
            d.panels[k].points = 1        # "this panel draws": the answer does not read through the pointer
    return bool(_lib.lib().p2c_render_points_supported(ctypes.byref(d)))


def render_points(panels, size=(800, 600), layout=(1, 1), radius: int = 2, line_width: int = 0, max_blocks: int = 0) -> Tensor:
    """Skeleton clips -> merged uint8 frames (V, T, rows*H, cols*W, 3), the video logger's pixels. ``panels``: a sequence of None
    or ``(points (V,T,J,C>=2) float, colors (J,3) uint8, edges (E,2) joint indices)``; panel k fills cell (k // cols, k % cols) of
    ``layout = (rows, cols)``, each cell ``size = (H, W)``; None panels and unused cells are zero. Rules (include/p2c.h, K34): centre
    = rint(x, y) in fp32, x the column; non-finite or |c| > 16383 draws nothing; bones (only with ``line_width`` > 0) in edge order
    in the colour of their second joint, then joints as discs of ``radius`` in index order, later over earlier.
    fp32 device points inside ``render_points_supported`` take K34: ONE launch for every panel, video and frame, no memset. Host
    tensors, other float types, refused shapes and ``P2C_RENDER_FRAMEWORK=1`` take the tensor definition, which gives the same
    bytes. ``max_blocks`` lowers the grid cap (tests)."""
    (H, W), (rows, cols) = (int(v) for v in size), (int(v) for v in layout)
    radius, line_width = int(radius), int(line_width)
    if H < 1 or W < 1 or rows < 1 or cols < 1 or radius < 0 or line_width < 0:
        raise RuntimeError(f'render_points: size {size}, layout {layout}, radius {radius}, line_width {line_width}')
    checked, lead = _render_panels(panels)
    if len(checked) > rows * cols:
        raise RuntimeError(f'render_points: {len(checked)} panels for a layout of {rows} x {cols} cells')
    V, T = lead.shape[:2]
    if V == 0 or T == 0:
        return torch.zeros(V, T, rows * H, cols * W, 3, dtype=torch.uint8, device=lead.device)
    if not _render_supported(checked, lead, (H, W), (rows, cols), radius, line_width):
        return _render_points_tensor(checked, (H, W), (rows, cols), radius, line_width)
    dev = lead.device
    keep = []               # contiguous operands stay alive until the launch is issued
    d = _render_desc(checked, V, T, H, W, rows, cols, radius, line_width, max_blocks)
    for k, panel in enumerate(checked):
        if panel is None or panel[0].shape[2] == 0:
            continue
        points, colors, edges = panel
        points, colors, edges = points.contiguous(), colors.contiguous(), edges.to(torch.int32).contiguous()
        keep += [points, colors, edges]
        d.panels[k].points, d.panels[k].colors = points.data_ptr(), colors.data_ptr()
        d.panels[k].edges = edges.data_ptr() if edges.numel() else None
    out = torch.empty(V, T, rows * H, cols * W, 3, dtype=torch.uint8, device=dev)
    d.out = out.data_ptr()
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().p2c_render_points_fwd(ctypes.byref(d), _stream()), 'p2c_render_points_fwd')
    return out


# ---- K38: Carla2D3D training batches generated on the device (csrc/p2c_generate.hip) ---------------------------------------------
GENERATE_OUTPUTS = ('frames', 'projection_2d', 'projection_2d_deformed', 'projection_2d_transformed', 'projection_2d_shift',
                    'projection_2d_scale', 'pose_changes', 'relative_pose_loc', 'relative_pose_rot', 'absolute_pose_loc',
                    'absolute_pose_rot', 'world_loc', 'world_rot', 'world_loc_changes', 'world_rot_changes', 'skel_type')
_GENERATE_TAIL = {'frames': (J, 2), 'projection_2d': (J, 2), 'projection_2d_deformed': (J, 2), 'projection_2d_transformed': (J, 2),
                  'projection_2d_shift': (2,), 'projection_2d_scale': (), 'pose_changes': (J, 3, 3), 'relative_pose_loc': (J, 3),
                  'relative_pose_rot': (J, 3, 3), 'absolute_pose_loc': (J, 3), 'absolute_pose_rot': (J, 3, 3), 'world_loc': (3,),
                  'world_rot': (3, 3), 'world_loc_changes': (3,), 'world_rot_changes': (3, 3)}
_GENERATE_NEEDS_TRANSFORM = ('projection_2d_transformed', 'projection_2d_shift', 'projection_2d_scale')


def generate_framework() -> bool:
    """P2C_GENERATE_FRAMEWORK=1: ``generate_carla_batch`` runs the composed device path -- the definition's draws moved to the device,
    ``euler_angles_to_matrix``, ``pose_head``, ``collate`` -- (the comparison arm of tools/bench_generate.py)."""
    return os.environ.get('P2C_GENERATE_FRAMEWORK', '0') == '1'


def generate_miss_prob(miss_prob) -> Optional[Tuple[float, ...]]:
    """None / () -> None (no joint goes missing); one value -> 26 of it; 26 values."""
    if miss_prob is None:
        return None
    probs = [float(miss_prob)] if isinstance(miss_prob, (int, float)) else [float(p) for p in miss_prob]
    if len(probs) == 0:
        return None
    if len(probs) == 1:
        probs = probs * J
    if len(probs) != J:
        raise ValueError(f'Missing joint probabilities must have length 1 or {J}, got {len(probs)}.')
    return tuple(probs)


def _generate_composed(B, T, draws_kwargs, transform, miss_prob, want, device) -> Dict[str, Tensor]:
    from pedestrians_video_2_carla_amd.data.carla import generator
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix
    d = generator.draws(B=B, T=T, **draws_kwargs)
    st = d['skel_type'].to(device)
    changes = euler_angles_to_matrix(d['angles'].to(device), 'XYZ')
    world_on = draws_kwargs['max_world_rot_change_in_deg'] != 0 or draws_kwargs['max_initial_world_rot_change_in_deg'] != 0
    f32 = dict(dtype=torch.float32, device=device)
    world_loc, world_rot = identity_world((B, T), changes)
    out = {'skel_type': st, 'world_loc_changes': world_loc.clone(), 'world_rot_changes': world_rot.clone(), 'world_loc': world_loc,
           'world_rot': world_rot}
    drot = None
    if world_on:
        yaw = torch.zeros(B, T, 3)
        yaw[..., 2] = d['world_yaw']
        drot = euler_angles_to_matrix(yaw.to(device), 'XYZ')
        out['world_rot_changes'] = drot
    keys = ('projection_2d', 'absolute_pose_loc', 'absolute_pose_rot', 'relative_pose_loc', 'relative_pose_rot') + \
        (('world_rot',) if world_on else ())
    _, o = pose_head(changes, PoseHeadSpec(kind='pose_changes', transform='none'), st, None, drot, want=keys)
    out.update({k: v for k, v in o.items() if k != 'projection_2d'})
    out['pose_changes'] = changes
    raw = o['projection_2d'][..., :2].contiguous()
    frames, targets = collate(raw, noise=d['noise'].to(device) if d['noise'] is not None else None,
                              miss_u=d['miss_u'].to(device) if miss_prob is not None else None, miss_prob=miss_prob,
                              transform=transform)
    out['frames'] = frames
    out.update(targets)
    out.setdefault('projection_2d_deformed', targets['projection_2d'].clone())
    return {k: out[k] for k in GENERATE_OUTPUTS if k in want}


@torch.no_grad()
def generate_carla_batch(B: int, T: int, *, seed: int, stream: int = 0, first_clip: int = 0, random_changes_each_frame: int = 3,
                         max_change_in_deg: float = 5.0, max_world_rot_change_in_deg: float = 0.0,
                         max_initial_world_rot_change_in_deg: float = 0.0, transform: str = 'hips_neck_bbox', noise: str = 'zero',
                         noise_param: float = 1.0, miss_prob=None, want: Optional[Sequence[str]] = None, device,
                         max_blocks: int = 0, mapping: str = 'auto') -> Dict[str, Tensor]:
    """Clips ``first_clip .. first_clip + B - 1`` of ``(seed, stream)`` of the reference's infinite Carla2D3D training set
    (``Carla2D3DIterableDataset.generate_batch``), T frames each, made on ``device`` by K38 in ONE launch: draws, Euler matrices, the
    running product of the pose changes, forward kinematics, world yaw, projection, deformation and both normalisations. The random
    part is the pure function ``data/carla/generator.py`` defines -- clip n of a stream is the same clip in whatever batch --; no
    host synchronisation, no host-to-device copy, nothing recorded for autograd. Returns the ``want``-ed of ``GENERATE_OUTPUTS``
    (default: all the transform allows). ``miss_prob``: None, one probability or 26; ``noise``: 'zero' | 'uniform'.
    ``mapping``: 'auto' | 'sequential' | 'frame_parallel' (same bits; include/p2c.h); ``max_blocks`` lowers the grid cap (tests).
    ``P2C_GENERATE_FRAMEWORK=1`` runs the composed path instead: the definition's draws, ``pose_head`` and ``collate``."""
    import math
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.P2CError('generate_carla_batch makes its batches on the GPU: there is no CPU implementation')
    if transform not in TRANSFORM:
        raise ValueError(f'unknown transform {transform!r}')
    if noise is None:
        noise = 'zero'
    if noise not in _lib.P2C_GENERATE_NOISE:
        raise ValueError(f"generate_carla_batch draws noise 'zero' or 'uniform', got {noise!r}")
    if mapping not in _lib.P2C_GENERATE_MAPPING:
        raise ValueError(f'unknown mapping {mapping!r}')
    B, T, k = int(B), int(T), int(random_changes_each_frame)
    if B < 0 or not 1 <= T <= _lib.P2C_GENERATE_MAX_T or not 0 <= k <= J or first_clip < 0:
        raise ValueError(f'generate_carla_batch: B {B}, T {T}, random_changes_each_frame {k}, first_clip {first_clip}')
    available = tuple(o for o in GENERATE_OUTPUTS if transform != 'none' or o not in _GENERATE_NEEDS_TRANSFORM)
    want = available if want is None else tuple(want)
    unknown = [o for o in want if o not in available]
    if unknown or not want:
        raise RuntimeError(f'generate_carla_batch: want {want}; a non-empty choice of {available} expected')
    probs = generate_miss_prob(miss_prob)
    if generate_framework():
        kwargs = dict(seed=seed, stream=stream, first_clip=first_clip, random_changes_each_frame=k,
                      max_change_in_deg=max_change_in_deg, max_world_rot_change_in_deg=max_world_rot_change_in_deg,
                      max_initial_world_rot_change_in_deg=max_initial_world_rot_change_in_deg, noise=noise, noise_param=noise_param)
        return _generate_composed(B, T, kwargs, transform, probs, want, device)
    result = {o: torch.empty((B, T) + _GENERATE_TAIL[o], dtype=torch.float32, device=device) for o in want if o != 'skel_type'}
    if 'skel_type' in want:
        result['skel_type'] = torch.empty(B, dtype=torch.int32, device=device)
    if B == 0:
        return result
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    seed = seed - (1 << 64) if seed >= (1 << 63) else seed
    stream = int(stream) & 0xFFFFFFFF
    stream = stream - (1 << 32) if stream >= (1 << 31) else stream
    camera = (ctypes.c_float * 5)(*PoseHeadSpec().camera)
    probs_c = (ctypes.c_float * J)(*probs) if probs is not None else None
    tables = [t.data_ptr() for t in ref.get_relative_tensors(device)]
    with torch.cuda.device(device):
        _lib.check(_lib.lib().p2c_carla_generate_fwd(
            seed, stream, int(first_clip), B, T, k, math.radians(max_change_in_deg), math.radians(max_world_rot_change_in_deg),
            math.radians(max_initial_world_rot_change_in_deg), TRANSFORM[transform], _lib.P2C_GENERATE_NOISE[noise],
            float(noise_param), probs_c, PoseHeadSpec().near_zero, camera, *tables, *(_ptr(result.get(o)) for o in GENERATE_OUTPUTS),
            _lib.P2C_GENERATE_MAPPING[mapping], int(max_blocks), _stream()), 'p2c_carla_generate_fwd')
    return result
