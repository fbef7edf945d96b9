"""The heatmap head of the pose-estimation flow on the host: the tensor paths of ops.heatmap_targets / heatmaps_loss /
heatmap_keypoints against tests/golden/heatmaps.npz (the reference's own gaussian_kernel, VideoMixin._get_heatmap, HeatmapsLoss and
_keypoints_from_heatmaps, see make_golden_heatmaps.py), the registry, the sum_per_joint / sum_per_frame reductions of
BasePoseLoss against a written-out loop, and the C ABI of K28 (csrc/p2c_heatmaps.hip)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.loss import LossModes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K28_SYMBOLS = ('p2c_heatmap_targets_fwd', 'p2c_heatmaps_loss_fwd', 'p2c_heatmaps_loss_bwd', 'p2c_heatmap_keypoints_fwd')
POOL = (9, 8, 1)


def _scale(g, tag):
    (ch, cw), (oh, ow) = g[f'tgt_{tag}_clip'].tolist(), g[f'tgt_{tag}_original'].tolist()
    return (cw / ow, ch / oh), (ch, cw)


def test_gaussian_table_is_the_reference_kernel(golden):
    g = golden('heatmaps')
    assert ops.gaussian_table(1).numel() == 11 and ops.gaussian_table(3).numel() == 85
    for sigma, name, (cx, cy) in ((1, 'gk_s1', (7, 6)), (3, 'gk_s3', (20, 18))):
        ref, table = g[name], ops.gaussian_table(sigma)
        H, W = ref.shape
        d2 = (torch.arange(H)[:, None] - cy) ** 2 + (torch.arange(W)[None, :] - cx) ** 2
        mine = torch.cat((table, table.new_zeros(1)))[d2.clamp(max=table.numel())]
        assert torch.equal(mine, ref)                          # bit for bit, the cut to zero included
        assert table[0] == 1 and table[-1] == 0 and (table[:-1] >= 0.0099).all()


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_targets_tensor_path_against_the_reference(golden, tag):
    g = golden('heatmaps')
    scale, clip = _scale(g, tag)
    kp, shift, sigma = g[f'tgt_{tag}_kp'][None], g[f'tgt_{tag}_shift'][None], int(g[f'tgt_{tag}_sigma'])
    full = ops.heatmap_targets(kp, shift, scale, clip, sigma, pool=None)[0]
    assert full.dtype == torch.float32 and torch.equal(full, g[f'tgt_{tag}_full'])      # full resolution: bit-exact
    pooled = ops.heatmap_targets(kp, shift, scale, clip, sigma, pool=POOL)[0]
    ref = g[f'tgt_{tag}_pooled']
    assert pooled.shape == ref.shape and torch.equal(pooled == 0, ref == 0)
    torch.testing.assert_close(pooled, ref, rtol=0, atol=81 * 2.0 ** -24)               # at most k k addends in [0, 1], any order
    # the loader-side callable is the same thing
    from pedestrians_video_2_carla_amd.data.base.heatmaps import HeatmapTargets
    made = HeatmapTargets(sigma=sigma, clip_size=clip, pool=POOL)(kp, shift, g[f'tgt_{tag}_original'].tolist())[0]
    assert torch.equal(made, pooled)


def test_targets_have_exact_zeros_and_a_background(golden):
    g = golden('heatmaps')
    full = g['tgt_a_full']
    assert (full[:, 1:] == 0).float().mean() > 0.9             # almost all of a joint's map is the literal zero
    assert torch.equal(full[:, 0], 1 - full[:, 1:].max(1).values)
    # a joint outside the frame: a zero map, at full resolution and pooled
    scale, clip = _scale(g, 'a')
    pooled = ops.heatmap_targets(g['tgt_a_kp'][None], g['tgt_a_shift'][None], scale, clip, 1)[0]
    assert (pooled[0, 5] == 0).all() and (full[0, 5] == 0).all()


def _loss_class(pair, mask):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    cls, crit = LossModes.heatmaps.value
    return cls(criterion=crit, input_nodes=CARLA_SKELETON if pair == 'cc' else BODY_25_SKELETON, output_nodes=CARLA_SKELETON,
               mask_missing_joints=mask)


@pytest.mark.parametrize('pair', ['cc', 'bc'])
@pytest.mark.parametrize('mask', ['on', 'off'])
def test_loss_tensor_path_against_the_reference_class(golden, pair, mask):
    g = golden('heatmaps')
    fn = _loss_class(pair, mask == 'on')
    pred, gt = g[f'loss_pred_{pair}'], g[f'loss_gt_{pair}']
    assert pred.dtype == torch.float64
    p = pred.clone().requires_grad_(True)
    loss = fn(heatmaps=p, targets={'heatmaps': gt})
    torch.testing.assert_close(loss, g[f'loss_{pair}_{mask}'], rtol=1e-12, atol=0)
    loss.backward()
    torch.testing.assert_close(p.grad, g[f'grad_{pair}_{mask}'], rtol=1e-12, atol=1e-15)
    assert (p.grad[:, 1] == 0).all() and p.grad.isfinite().all()                          # the NaN frame is skipped
    # the op with the class's three index arguments is the same value; another criterion takes the grouped tensor path
    pc, gc, forced = fn.channels(pred.shape[2], gt.shape[2])
    value, flags = ops.heatmaps_loss(pred, gt, pc, gc, forced, mask == 'on', with_flags=True)
    torch.testing.assert_close(value, g[f'loss_{pair}_{mask}'], rtol=1e-12, atol=0)
    assert flags.shape == (2, 3, len(pc)) and (flags[..., forced].all() if forced >= 0 else True)
    if mask == 'off':
        assert flags.all()
    else:
        assert not flags.all() and flags[1, 2].sum() == (1 if forced >= 0 else 0)


def test_loss_channel_lists_address_stored_channels():
    fn = _loss_class('bc', True)
    pc, gc, forced = fn.channels(27, 26)
    assert pc[-1] == 25 and gc[-1] == 24 and pc.count(25) == 2 and len(pc) == len(gc) == 22     # a repeated prediction channel
    assert gc[forced] == 8                                                                       # BODY_25's MidHip index
    pc, gc, forced = _loss_class('cc', True).channels(27, 27)
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    assert pc == gc == list(range(27)) and forced == CARLA_SKELETON.get_hips_point().value     # a stored channel: the joint before


def test_loss_with_every_frame_skipped_is_zero():
    pred = torch.randn(1, 2, 3, 2, 2, dtype=torch.float64, requires_grad=True)
    gt = torch.zeros(1, 2, 3, 2, 2, dtype=torch.float64)
    loss = ops.heatmaps_loss(pred, gt, [0, 1, 2], [0, 1, 2], -1, True)
    assert float(loss.detach()) == 0
    loss.backward()
    assert (pred.grad == 0).all()


def test_decode_tensor_path_against_the_reference(golden):
    g = golden('heatmaps')
    maps, frame = g['dec_maps'], tuple(g['dec_frame'].tolist())
    out = ops.heatmap_keypoints(maps, frame)
    ref = g['dec_out']
    assert out.dtype == torch.float32 and out.shape == ref.shape == (2, 3, 3, 3)
    assert torch.equal(out[..., 2], ref[..., 2])
    torch.testing.assert_close(out[..., :2], ref[..., :2], rtol=1e-6, atol=0)
    assert (out[1, 0, 2] == 0).all() and (out[1, 1, 0] == 0).all() and (out[1, 2, 1] == 0).all()   # non-positive, zero, NaN maps
    assert out[0, 0, 0, 2] == 2 and out[0, 1, 1, 2] == 3
    # the tie went to the first index (row 1, column 2); (sw, sh) = (40 / 7, 56 / 5): the reference's assignment
    torch.testing.assert_close(out[0, 0, 0, :2], torch.tensor([2 * 40 / 7, 1 * 56 / 5]), rtol=1e-6, atol=0)


def test_registry():
    from pedestrians_video_2_carla_amd.modules.flow.pose_estimation import LitPoseEstimationFlow
    from pedestrians_video_2_carla_amd.modules.pose_estimation import Linear, PoseEstimationModel
    from pedestrians_video_2_carla_amd.modules.flow.output_types import PoseEstimationModelOutputType
    assert list(LitPoseEstimationFlow.get_available_models()['movements']) == ['Linear']
    assert LitPoseEstimationFlow.get_default_models() == {'movements': Linear}
    assert list(LossModes.__members__)[-1] == 'heatmaps'
    cls, crit = LossModes.heatmaps.value
    assert cls.__name__ == 'HeatmapsLoss' and type(crit) is torch.nn.MSELoss and crit.reduction == 'mean'
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    model = Linear(input_nodes=CARLA_SKELETON)
    assert isinstance(model, PoseEstimationModel) and model.needs_heatmaps
    assert model.output_type == PoseEstimationModelOutputType.heatmaps
    assert model(torch.zeros(2, 3, 3, 40, 56)).shape == (2, 3, 27, 5, 7)
    flow = LitPoseEstimationFlow(movements_model=model, loss_modes=['heatmaps'])
    assert flow.needs_heatmaps and flow.get_initial_metrics() == {}
    import argparse
    args = LitPoseEstimationFlow.add_model_specific_args(argparse.ArgumentParser()).parse_args([])
    assert args.heatmaps_sigma == 1


def _flow_and_batch(supplied, dtype=torch.float64):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_estimation import LitPoseEstimationFlow
    from pedestrians_video_2_carla_amd.modules.pose_estimation import Linear
    torch.manual_seed(5)
    flow = LitPoseEstimationFlow(movements_model=Linear(input_nodes=CARLA_SKELETON), loss_modes=['heatmaps'], transform='none').to(dtype)
    gen = torch.Generator().manual_seed(6)
    frames = torch.randn(2, 3, 3, 40, 56, generator=gen, dtype=dtype)
    kp = torch.rand(2, 3, 26, 2, generator=gen, dtype=dtype) * torch.tensor([112.0, 80.0], dtype=dtype)
    kp[0, 0, 3] = 0
    shift = torch.tensor([2.0, -1.0], dtype=dtype).expand(2, 3, 2).contiguous()
    targets = {'projection_2d': kp, 'heatmaps_shift': shift}
    if supplied:
        targets['heatmaps'] = ops.heatmap_targets(kp, shift, (0.5, 0.5), (40, 56), 1, pool=None)
    return flow, (frames, targets, {'original_size': (80, 112)})


def test_flow_step_builds_or_pools_its_targets():
    values = []
    for supplied in (False, True):
        flow, batch = _flow_and_batch(supplied)
        out = flow.training_step(batch, 0)
        assert out['targets']['heatmaps'].shape == (2, 3, 27, 5, 7) and out['preds']['projection_2d'] is None    # lean: no decode
        out['loss'].backward()
        assert all(p.grad is not None and p.grad.isfinite().all() for p in flow.parameters())
        values.append(out['loss'].detach())
        flow.eval()
        val = flow._step(batch, 0, 'val')
        assert val['preds']['projection_2d'].shape == (2, 3, 26, 2)
    torch.testing.assert_close(values[0], values[1], rtol=1e-6, atol=0)          # K28a's restatement = avg_pool2d of the full maps
    # a target already at the output's resolution is used as supplied
    flow, (frames, targets, meta) = _flow_and_batch(True)
    small = torch.nn.functional.avg_pool2d(targets['heatmaps'].flatten(0, 1), 9, 8, 1).unflatten(0, (2, 3))
    out = flow.training_step((frames, {**targets, 'heatmaps': small}, meta), 0)
    assert out['targets']['heatmaps'].data_ptr() == small.data_ptr() and torch.equal(out['targets']['heatmaps'], small)


def _reference_loop(pred, gt, mask, criterion, per_joint):
    """BasePoseLoss's grouped reductions, written out: the criterion on the selected rows of every frame (or joint), NaN groups
    skipped, the rest summed."""
    losses = []
    n = pred.shape[-2] if per_joint else pred.shape[1]
    for i in range(n):
        p, g = (pred[..., i, :], gt[..., i, :]) if per_joint else (pred[:, i], gt[:, i])
        if mask is not None:
            m = mask[..., i] if per_joint else mask[:, i]
            p, g = p[m], g[m]
        value = criterion(p, g)
        if not torch.isnan(value):
            losses.append(value)
    return torch.stack(losses).sum()


@pytest.mark.parametrize('per_joint', [True, False])
@pytest.mark.parametrize('mask', [True, False])
def test_loc_2d_grouped_sums_against_the_loop(per_joint, mask):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.loss.loc_2d import Loc2DPoseLoss
    gen = torch.Generator().manual_seed(9)
    pred = torch.randn(3, 4, 26, 2, generator=gen, dtype=torch.float64)
    gt = torch.randn(3, 4, 26, 2, generator=gen, dtype=torch.float64)
    gt[0, :, 5] = 0
    gt[:, 2, 1:] = 0                    # frame 2: only the hips survive the mask
    gt[:, :, 7] = 0                     # joint 7: nothing selected -> that group is skipped under the mask
    for crit in (torch.nn.MSELoss(reduction='mean'), torch.nn.L1Loss(reduction='mean'), torch.nn.MSELoss(reduction='sum')):
        fn = Loc2DPoseLoss(criterion=crit, input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, mask_missing_joints=mask,
                           sum_per_joint=per_joint, sum_per_frame=not per_joint)
        p = pred.clone().requires_grad_(True)
        got = fn(projection_2d=p, targets={'projection_2d': gt})
        m = None
        if mask:
            m = (gt != 0).all(-1)
            m[..., CARLA_SKELETON.get_hips_point().value] = True
        q = pred.clone().requires_grad_(True)
        want = _reference_loop(q, gt, m, crit, per_joint)
        torch.testing.assert_close(got, want, rtol=1e-12, atol=0)
        got.backward(), want.backward()
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-12, atol=1e-15)


def _lib_loaded():
    from pedestrians_video_2_carla_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_k28_symbols_are_declared_bound_and_exported():
    _lib, lib = _lib_loaded()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    for name in K28_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p      # the stream goes last: the LDS-poisoning audit covers them
    for name in ('heatmap_targets', 'heatmaps_loss', 'heatmap_keypoints'):
        assert callable(getattr(ops, name))
    assert (_lib.HEATMAPS_MAX_MAPS, _lib.HEATMAPS_MAX_TABLE, _lib.HEATMAPS_MAX_POOL) == tuple(
        int(re.search(rf'#define {n}\s+(\d+)', header).group(1))
        for n in ('P2C_HEATMAPS_MAX_MAPS', 'P2C_HEATMAPS_MAX_TABLE', 'P2C_HEATMAPS_MAX_POOL'))


def test_k28_descriptor_layouts_match_the_header(tmp_path):
    from pedestrians_video_2_carla_amd import _lib
    descs = (('p2c_heatmap_targets_desc', _lib.HeatmapTargetsDesc), ('p2c_heatmaps_loss_desc', _lib.HeatmapsLossDesc),
             ('p2c_heatmap_keypoints_desc', _lib.HeatmapKeypointsDesc))
    body = ''
    for cname, cls in descs:
        body += f'  printf("{cname}.sizeof %zu\\n", sizeof({cname}));\n'
        body += ''.join(f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));\n' for f in cls._fields_)
    src, exe = tmp_path / 'hm.c', tmp_path / 'hm'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n' + body + '  return 0;\n}\n')
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    for cname, cls in descs:
        assert int(out[f'{cname}.sizeof']) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(out[f'{cname}.{f[0]}']) == getattr(cls, f[0]).offset, (cname, f[0])


def test_k28_refuses_bad_arguments_without_a_device():
    """Every refusal is answered on the host, before anything could be launched: these run on a machine without a GPU."""
    _lib, lib = _lib_loaded()

    def targets(**kw):
        d = _lib.HeatmapTargetsDesc()
        v = dict(N=2, J=5, H=40, W=56, k=9, s=8, p=1, oh=5, ow=7, n_table=11, scale_x=1.0, scale_y=1.0, kp=64, shift=64, table=64, out=64)
        v.update(kw)
        for name, value in v.items():
            setattr(d, name, value)
        return ctypes.byref(d)
    fn = lib.p2c_heatmap_targets_fwd
    assert fn(None, None) == -1 and fn(targets(N=0), None) == 0
    for bad in (dict(J=0), dict(J=64), dict(H=0), dict(k=33), dict(k=0), dict(s=0), dict(p=5), dict(oh=6), dict(ow=6), dict(n_table=0),
                dict(n_table=1025), dict(N=-1), dict(H=4, oh=0)):
        assert fn(targets(**bad), None) == -2, bad
    for ptr in ('kp', 'shift', 'table', 'out'):
        assert fn(targets(**{ptr: None}), None) == -1, ptr

    def loss(pc=(0, 1, 1), gc=(1, 0, 2), **kw):
        d = _lib.HeatmapsLossDesc()
        v = dict(B=2, T=3, Pp=2, Pg=3, h=5, w=7, K=len(pc), forced=0, mask=1, pred=64, gt=64, partials=64, flags=64, coef=64, loss=64,
                 grad_loss=64, grad_pred=64)
        v.update(kw)
        for name, value in v.items():
            setattr(d, name, value)
        for i, (a, b) in enumerate(zip(pc, gc)):
            d.pred_channels[i], d.gt_channels[i] = a, b
        return ctypes.byref(d)
    for fn in (lib.p2c_heatmaps_loss_fwd, lib.p2c_heatmaps_loss_bwd):
        assert fn(None, None) == -1
        for bad in (dict(T=0), dict(Pp=65), dict(Pg=0), dict(h=0), dict(K=0), dict(K=65), dict(forced=3), dict(forced=-2), dict(B=-1),
                    dict(pc=(0, 2, 1)), dict(gc=(1, 3, 2)), dict(pc=(0, -1, 1))):
            assert fn(loss(**bad), None) == -2, bad
        assert fn(loss(mask=2), None) == -3
        for ptr in ('pred', 'gt', 'partials', 'flags', 'coef'):
            assert fn(loss(**{ptr: None}), None) == -1, ptr
    assert lib.p2c_heatmaps_loss_fwd(loss(loss=None), None) == -1
    assert lib.p2c_heatmaps_loss_bwd(loss(grad_pred=None), None) == -1 and lib.p2c_heatmaps_loss_bwd(loss(grad_loss=None), None) == -1
    assert lib.p2c_heatmaps_loss_bwd(loss(B=0), None) == 0

    def decode(**kw):
        d = _lib.HeatmapKeypointsDesc()
        v = dict(N=2, P=4, h=5, w=7, sw=1.0, sh=1.0, maps=64, out=64)
        v.update(kw)
        for name, value in v.items():
            setattr(d, name, value)
        return ctypes.byref(d)
    fn = lib.p2c_heatmap_keypoints_fwd
    assert fn(None, None) == -1 and fn(decode(N=0), None) == 0
    for bad in (dict(P=1), dict(P=65), dict(h=0), dict(w=0), dict(N=-1)):
        assert fn(decode(**bad), None) == -2, bad
    assert fn(decode(maps=None), None) == -1 and fn(decode(out=None), None) == -1
