#!/usr/bin/env python3
"""Generate tests/golden/heatmaps.npz by RUNNING THE REFERENCE's own heatmap code (build container only).

The reference imports under the third-party stand-ins of make_golden.py (``install_standins``) plus three of this file's own:
``pims`` (video_mixin.py imports it; nothing here decodes a video), ``torchvision`` where it is absent (VideoToResNet is imported,
never called), and for the flow module, of which only ``_keypoints_from_heatmaps`` is called: the three pose-estimation models
that need third-party sources, ``torchmetrics`` and the autoencoder flow it derives from (a bare base class). What runs unmodified:

  utils/gaussian_kernel.py                          ``gk_s1`` (13, 15) around (7, 6), ``gk_s3`` (37, 41) around (20, 18)
  VideoMixin._get_heatmap                           on a two-attribute object (num_input_joints, sigma): ``tgt_a_*`` J = 5,
                                                    (40, 56) clip of an (80, 84) original, sigma = 1, T = 3; ``tgt_b_*`` J = 4,
                                                    (33, 47) clip of itself, sigma = 3, T = 2. ``*_full`` is what it returns,
                                                    ``*_pooled`` the flow's avg_pool2d(9, 8, 1) of it. The keypoints hold centres
                                                    outside the frame, on its border, a coincident pair, the (0, 0) of a missing
                                                    joint and scaled values ending in .5
  loss/heatmaps_loss.py (HeatmapsLoss, fp64)        ``loss_<pair>_<mask>`` and the gradient ``grad_<pair>_<mask>`` of
                                                    ``loss_pred_<pair>`` for pair in (cc: CARLA -> CARLA, bc: BODY_25 input ->
                                                    CARLA output), mask in (on, off); B = 2, T = 3, (5, 7) maps; frame 1 of the
                                                    prediction holds a NaN in a selected map (the reference skips the frame)
  LitPoseEstimationFlow._keypoints_from_heatmaps    ``dec_maps`` (2, 3, 4, 5, 7) with ties, a maximum at the last cell, an
                                                    all-non-positive map and a NaN map, frames of (40, 56) -> ``dec_out``
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_SRC, install_standins, npz  # noqa: E402


def _standin(name, **attrs):
    if name in sys.modules:
        return
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition('.')
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)


def keypoints_a():
    # pixels of the (80, 84) original, shift (3, -2), scale (56 / 84, 40 / 80): centre = rint((kp - shift) * scale)
    kp = torch.tensor([
        [[45.0, 38.0], [3.0, -2.0], [87.0, 78.0], [45.0, 38.0], [-30.0, 500.0]],    # inside, corner (0,0), far corner, coincident, outside
        [[0.0, 0.0], [6.75, 1.0], [3.75, 3.0], [86.25, 76.0], [60.0, -3.0]],       # missing joint; x*2/3 = 2.5, 0.5 (ties); border; just outside
        [[44.3, 17.9], [20.0, 20.0], [20.0, 21.0], [84.0, 39.0], [5.0, 77.0]],
    ])
    return kp, torch.tensor([[3.0, -2.0]] * 3), (40, 56), (80, 84)


def keypoints_b():
    kp = torch.tensor([
        [[23.0, 16.0], [0.0, 0.0], [46.0, 32.0], [-2.0, 10.0]],
        [[10.5, 11.5], [10.0, 12.0], [49.0, 35.0], [23.4, -1.6]],                   # .5 under unit scale; a coincident pair after rounding
    ])
    return kp, torch.zeros(2, 2), (33, 47), (33, 47)


def main():
    if not os.path.isdir(REF_SRC):
        sys.exit('reference tree not present: the committed .npz files are the artefact to use')
    install_standins()
    _standin('pims')
    try:
        import torchvision  # noqa: F401
    except ImportError:
        _standin('torchvision')
        _standin('torchvision.transforms')
        _standin('torchvision.transforms.functional', equalize=None, normalize=None, resize=None)
    sys.path.insert(0, REF_SRC)
    pe = 'pedestrians_video_2_carla.modules.pose_estimation.'
    import pedestrians_video_2_carla.modules.pose_estimation  # noqa: F401
    for pkg in ('unipose', 'transformers', 'regular'):
        _standin(pe + pkg)
    _standin(pe + 'unipose.unipose_lstm', UniPoseLSTM=type('UniPoseLSTM', (), {}))
    _standin(pe + 'transformers.avpedestrian_pose_transformer', AvPedestrianPoseTransformer=type('AvPedestrianPoseTransformer', (), {}))
    _standin(pe + 'regular.p0', P0=type('P0', (), {}))
    # the flow module is imported for one method that touches neither its base class nor a metric
    _standin('torchmetrics', Metric=object)
    _standin('pedestrians_video_2_carla.modules.flow.autoencoder', LitAutoencoderFlow=object)
    from pedestrians_video_2_carla.data.base.mixins.dataset.video_mixin import VideoMixin
    from pedestrians_video_2_carla.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla.loss.heatmaps_loss import HeatmapsLoss
    from pedestrians_video_2_carla.modules.flow.pose_estimation import LitPoseEstimationFlow
    from pedestrians_video_2_carla.utils.gaussian_kernel import gaussian_kernel

    out = dict(gk_s1=gaussian_kernel(15, 13, 7, 6, 1)[0], gk_s3=gaussian_kernel(41, 37, 20, 18, 3)[0])

    for tag, (kp, shift, clip, original), sigma in (('a', keypoints_a(), 1), ('b', keypoints_b(), 3)):
        holder = types.SimpleNamespace(num_input_joints=kp.shape[1], sigma=sigma)
        full = torch.stack([VideoMixin._get_heatmap(holder, kp[t], clip, original, shift[t]) for t in range(len(kp))])
        pooled = torch.nn.functional.avg_pool2d(full, kernel_size=9, stride=8, padding=1)      # the flow's resize
        out.update({f'tgt_{tag}_kp': kp, f'tgt_{tag}_shift': shift, f'tgt_{tag}_clip': torch.tensor(clip),
                    f'tgt_{tag}_original': torch.tensor(original), f'tgt_{tag}_sigma': sigma,
                    f'tgt_{tag}_full': full, f'tgt_{tag}_pooled': pooled})

    g = torch.Generator().manual_seed(28)
    for pair, nodes_in, nodes_out in (('cc', CARLA_SKELETON, CARLA_SKELETON), ('bc', BODY_25_SKELETON, CARLA_SKELETON)):
        B, T, h, w = 2, 3, 5, 7
        gt = torch.rand(B, T, len(nodes_in) + 1, h, w, generator=g, dtype=torch.float64) + 0.01
        gt[:, :, ::3, 1, 2] = 0                      # every third target map has an exact zero: dropped under the mask
        gt[1, 2, :, 0, 0] = 0                        # clip 1, frame 2: nothing but the forced entry survives the mask
        pred = torch.randn(B, T, len(nodes_out) + 1, h, w, generator=g, dtype=torch.float64)
        pred[0, 1, 1, 2, 3] = float('nan')           # stored channel 1 is compared in both pairs: frame 1 is skipped
        out.update({f'loss_gt_{pair}': gt, f'loss_pred_{pair}': pred})
        for mask in (True, False):
            p = pred.clone().requires_grad_(True)
            loss = HeatmapsLoss(criterion=torch.nn.MSELoss(reduction='mean'), input_nodes=nodes_in, output_nodes=nodes_out,
                                mask_missing_joints=mask)(heatmaps=p, targets={'heatmaps': gt})
            loss.backward()
            name = f'{pair}_{"on" if mask else "off"}'
            out.update({f'loss_{name}': loss, f'grad_{name}': p.grad})

    maps = torch.rand(2, 3, 4, 5, 7, generator=g)
    maps[0, 0, 1, 1, 2] = maps[0, 0, 1, 3, 4] = 2.0  # a tie: the first index wins
    maps[0, 1, 2, 4, 6] = 3.0                        # the maximum at the last cell
    maps[1, 0, 3] = -maps[1, 0, 3]                   # nothing positive
    maps[1, 1, 1] = 0.0                              # all zero
    maps[1, 2, 2, 2, 2] = float('nan')               # a NaN map
    maps[:, :, 0] = 5.0                              # the background is never decoded
    out.update(dec_maps=maps, dec_frame=torch.tensor((40, 56)),
               dec_out=LitPoseEstimationFlow._keypoints_from_heatmaps(None, maps, (40, 56)))
    npz('heatmaps', **out)


if __name__ == '__main__':
    main()
