#!/usr/bin/env python3
"""Generate tests/golden/frames.npz by RUNNING THE REFERENCE's own static ``VideoMixin.crop_bbox`` (build container only).

The reference imports under the third-party stand-ins of make_golden.py (``install_standins``) plus the two of
make_golden_heatmaps.py that video_mixin.py needs: ``pims`` (imported, nothing here decodes a video) and ``torchvision`` where it
is absent (``VideoToResNet`` is imported, never called). What runs unmodified is ``crop_bbox`` with ``extract_bbox_from_frame``
(data/base/mixins/dataset/video_mixin.py:143-184) on one random uint8 clip ``frames`` (3, 48, 64, 3), of which a case takes the
first T frames. Per case ``<tag>_bboxes`` (T,2,2), ``<tag>_margin``, ``<tag>_target`` -> ``<tag>_canvas`` (T,c,c,3) and
``<tag>_shifts`` (T,2):

  centred   a 20 x 16 bbox in the middle of the frame, canvas 28; centres ending in .5 before the rounding (ties go to even)
  borders   T = 3: the canvas hangs over the left, the top and the right border
  corner    T = 2: over the bottom border; over the top-left corner with a centre outside the frame
  odd       the largest bbox side is 25: canvas int(25 * 1.4) = 35, half 17 -- the last row and column stay zero
  small     a 6 x 5 bbox: int(6 * 1.4) = 8 < target 24, canvas_size == target_size
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF_SRC, install_standins, npz  # noqa: E402
from make_golden_heatmaps import _standin  # noqa: E402


def box(cx, cy, w, h):
    return [[cx - w / 2.0, cy - h / 2.0], [cx + w / 2.0, cy + h / 2.0]]


def cases():
    """tag -> (bboxes (T,2,2) float64, margin, target_size)"""
    return {
        'centred': (np.array([box(32.0, 24.0, 20, 16), box(31.5, 23.5, 20, 16), box(33.0, 22.25, 18, 16)]), 0.2, 24),
        'borders': (np.array([box(5.0, 24.0, 20, 20), box(30.0, 3.0, 20, 20), box(61.0, 20.0, 20, 20)]), 0.2, 24),
        'corner': (np.array([box(40.0, 46.0, 20, 20), box(-2.0, 1.0, 20, 20)]), 0.2, 24),
        'odd': (np.array([box(30.0, 20.0, 25, 11), box(8.0, 40.0, 13, 25)]), 0.2, 24),
        'small': (np.array([box(20.0, 20.0, 6, 5), box(60.0, 44.0, 4, 6)]), 0.2, 24),
    }


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
    from pedestrians_video_2_carla.data.base.mixins.dataset.video_mixin import VideoMixin

    frames = np.random.default_rng(33).integers(0, 256, size=(3, 48, 64, 3), dtype=np.uint8)
    out = dict(frames=frames)
    for tag, (bboxes, margin, target) in cases().items():
        canvas, shifts = VideoMixin.crop_bbox(frames[:len(bboxes)], bboxes, bbox_margin=margin, target_size=target)
        out.update({f'{tag}_bboxes': bboxes, f'{tag}_margin': margin, f'{tag}_target': target, f'{tag}_canvas': canvas,
                    f'{tag}_shifts': shifts})
        print(tag, canvas.shape, shifts.tolist())
    npz('frames', **out)


if __name__ == '__main__':
    main()
