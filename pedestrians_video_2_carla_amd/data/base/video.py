"""Video clips for the pose-estimation flow (reference data/base/mixins/dataset/video_mixin.py:88-184, ``VideoMixin.__getitem__`` /
``_get_clip_frames`` / ``crop_bbox`` / ``extract_bbox_from_frame``, and transforms/video/video_to_resnet.py:14-56, ``VideoToResNet``).

The reference prepares every clip on a DataLoader worker: a bbox-centred square crop pasted onto a zero canvas frame by frame,
torchvision ``equalize`` per frame and channel, an antialiased bilinear ``resize`` per frame, ``/ 255``, the ImageNet mean and
standard deviation, a stack to (T, 3, S, S). This module restates that as tensor code -- the definition, on whatever device the
clip lives -- and ``ClipFramesPipeline`` is the batched replacement a loader calls once per batch: on the device it is K33
(``ops.clip_frames``, csrc/p2c_frames.hip), which never forms the canvas, the equalized clip or the float image.

Decoding (``pims`` in the reference) is out of scope: a clip is a uint8 (T, H, W, 3) array or tensor, however it was decoded.

What is pinned and what is not: ``crop_bbox`` reproduces the reference's own function byte for byte (tests/golden/frames.npz);
``equalize`` equals ``PIL.ImageOps.equalize``, the integer formula torchvision's ``_scale_channel`` restates; the resize rule is
torchvision 0.10.1's (the version the reference's environment pins) and the resampling is ``torch.nn.functional.interpolate(...,
mode='bilinear', antialias=True)``, which is what torchvision's tensor ``resize`` calls. torchvision itself is not a dependency
and parity with it is not tested.
"""
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from pedestrians_video_2_carla_amd.data.base.heatmaps import HeatmapTargets

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- crop (video_mixin.py:143-184) --------------------------------------------------------------------------------------------
def canvas_size_of(bboxes: np.ndarray, bbox_margin: float = 0.2, target_size: int = 368) -> int:
    """``max(int((bboxes[:, 1] - bboxes[:, 0]).max() * (1 + 2 margin)), target_size)`` (video_mixin.py:149-151); bboxes (T,2,2)."""
    bboxes = np.asarray(bboxes)
    return max(int(((bboxes[:, 1] - bboxes[:, 0]).max() * (1 + 2 * bbox_margin)).astype(int)), int(target_size))


def bbox_centres(bboxes: np.ndarray) -> np.ndarray:
    """``(bboxes.mean(-2) + 0.5).round().astype(int)``: numpy's round half to even (video_mixin.py:155); (T,2) = (x, y)."""
    return (np.asarray(bboxes).mean(axis=-2) + 0.5).round().astype(int)


def paste_window(half_size: Tuple[int, int], bbox_center: Tuple[int, int], clip_size: Tuple[int, int]):
    """The integers of ``extract_bbox_from_frame`` (video_mixin.py:168-184): (frame_x_min, frame_y_min, width, height,
    canvas_x_shift, canvas_y_shift). A centre so far outside the frame that the copied width or height would be negative gives
    an empty window (width = height = 0): the reference is undefined there (numpy slices with a negative extent)."""
    (half_width, half_height), (x_center, y_center), (clip_width, clip_height) = half_size, bbox_center, clip_size
    x_center, y_center = int(x_center), int(y_center)
    frame_x_min = int(max(0, x_center - half_width))
    frame_x_max = int(min(clip_width, x_center + half_width))
    frame_y_min = int(max(0, y_center - half_height))
    frame_y_max = int(min(clip_height, y_center + half_height))
    frame_width, frame_height = max(frame_x_max - frame_x_min, 0), max(frame_y_max - frame_y_min, 0)
    if frame_width == 0 or frame_height == 0:
        frame_width = frame_height = 0
    return frame_x_min, frame_y_min, frame_width, frame_height, max(0, half_width - x_center), max(0, half_height - y_center)


def extract_bbox_from_frame(canvas, frame, half_size: Tuple[int, int], bbox_center: Tuple[int, int], clip_size: Tuple[int, int]):
    """Paste the part of ``frame`` around ``bbox_center`` into ``canvas`` (both (h, w, 3), arrays or tensors); returns the shift
    (x, y) that takes canvas coordinates to frame coordinates (video_mixin.py:168-184)."""
    x0, y0, w, h, cx, cy = paste_window(half_size, bbox_center, clip_size)
    if w and h:
        canvas[cy:cy + h, cx:cx + w] = frame[y0:y0 + h, x0:x0 + w]
    return x0 - cx, y0 - cy


def crop_geometry(bboxes, clip_hw: Tuple[int, int], bbox_margin: float = 0.2, target_size: int = 368):
    """Everything ``crop_bbox`` derives from the bboxes alone: (canvas_size, centres (T,2) int, shifts (T,2) int)."""
    bboxes = np.asarray(bboxes)
    canvas_size = canvas_size_of(bboxes, bbox_margin, target_size)
    half = canvas_size // 2
    centres = bbox_centres(bboxes)
    shifts = np.zeros((len(centres), 2), dtype=int)
    for t, centre in enumerate(centres):
        x0, y0, _, _, cx, cy = paste_window((half, half), centre, (clip_hw[1], clip_hw[0]))
        shifts[t] = (x0 - cx, y0 - cy)
    return canvas_size, centres, shifts


def crop_bbox(clip_frames, bboxes, bbox_margin: float = 0.2, target_size: int = 368):
    """``VideoMixin.crop_bbox`` (video_mixin.py:143-165): ``clip_frames`` uint8 (T,H,W,3), array or tensor (the canvas comes back as
    the same kind, on the same device), ``bboxes`` (T,2,2) on the host -> (canvas (T,c,c,3), shifts (T,2) int array). Integer
    arithmetic, exactly the reference's; an odd canvas size leaves its last row and column zero (half = c // 2). Where a centre
    lies so far outside the frame that the copied width or height would be negative, it is clamped to 0 and that frame's canvas
    is all zero -- the reference is undefined in that case."""
    bboxes = np.asarray(bboxes.cpu() if isinstance(bboxes, Tensor) else bboxes)
    clip_length, clip_height, clip_width, _ = clip_frames.shape
    canvas_size = canvas_size_of(bboxes, bbox_margin, target_size)
    half = canvas_size // 2
    if isinstance(clip_frames, Tensor):
        canvas = clip_frames.new_zeros((clip_length, canvas_size, canvas_size, 3))
    else:
        canvas = np.zeros((clip_length, canvas_size, canvas_size, 3), dtype=np.uint8)
    centres = bbox_centres(bboxes)
    shifts = np.zeros((clip_length, 2), dtype=int)
    for idx in range(clip_length):
        shifts[idx] = extract_bbox_from_frame(canvas[idx], clip_frames[idx], (half, half), centres[idx], (clip_width, clip_height))
    return canvas, shifts


# ---- VideoToResNet (video_to_resnet.py:14-56) ---------------------------------------------------------------------------------
def equalize(clip: Tensor) -> Tensor:
    """torchvision's ``equalize`` on a uint8 (..., H, W) tensor, every leading index an image of its own (``_scale_channel``): a
    256-bin histogram; step = (sum of the non-zero bins except the last non-zero one) // 255; step == 0 leaves the image
    unchanged; otherwise lut = (cumsum(hist) + step // 2) // step, shifted right by one with a leading 0, clamped to [0, 255]."""
    if clip.dtype != torch.uint8:
        raise TypeError(f'equalize: uint8 expected, got {clip.dtype}')
    if clip.numel() == 0:
        return clip
    flat = clip.reshape(-1, clip.shape[-2] * clip.shape[-1])
    n = flat.shape[0]
    rows = torch.arange(n, device=clip.device)
    hist = torch.zeros(n * 256, dtype=torch.int64, device=clip.device)
    hist.scatter_add_(0, (flat.long() + rows[:, None] * 256).reshape(-1), torch.ones(flat.numel(), dtype=torch.int64, device=clip.device))
    hist = hist.view(n, 256)
    bins = torch.arange(256, device=clip.device)
    last = torch.where(hist != 0, bins, bins.new_full((), -1)).max(dim=1).values
    step = (hist.sum(1) - hist[rows, last]) // 255
    safe = step.clamp(min=1)[:, None]
    lut = (hist.cumsum(1) + (step // 2)[:, None]) // safe
    lut = torch.cat((lut.new_zeros(n, 1), lut[:, :-1]), 1).clamp(0, 255)
    lut = torch.where(step[:, None] == 0, bins[None, :], lut).to(torch.uint8)
    return lut.gather(1, flat.long()).view(clip.shape)


def resized_size(height: int, width: int, target_size: int) -> Tuple[int, int]:
    """``VideoToResNet``'s output size: untouched unless ``height > S or width > S``; then torchvision 0.10.1's ``resize(img, S)``:
    the short side goes to S, the long side to ``int(S * long / short)``, unchanged if the short side already equals S."""
    S = int(target_size)
    if not (height > S or width > S):
        return height, width
    short, long = (width, height) if width <= height else (height, width)
    if short == S:
        return height, width
    new_short, new_long = S, int(S * long / short)
    return (new_long, new_short) if width <= height else (new_short, new_long)


def resize_levels(clip: Tensor, size: Tuple[int, int], dtype=torch.float32) -> Tensor:
    """(T,3,H,W) levels -> (T,3,h,w) levels: antialiased bilinear interpolation in ``dtype``, unrounded."""
    return torch.nn.functional.interpolate(clip.to(dtype), size=tuple(size), mode='bilinear', antialias=True, align_corners=False)


def normalize_levels(levels: Tensor) -> Tensor:
    """``(level / 255.0 - mean_c) / std_c`` in fp32 with true divisions (tensor divisors: a Python-scalar divisor may be turned
    into a product with its reciprocal on the device); ``levels`` (T,3,h,w)."""
    dev = levels.device
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32, device=dev)[:, None, None]
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32, device=dev)[:, None, None]
    return (levels.float() / torch.full((1,), 255.0, dtype=torch.float32, device=dev) - mean) / std


class VideoToResNet:
    """transforms/video/video_to_resnet.py:7-56: uint8 (T,H,W,3) -> fp32 (T,3,h,w). Permute, ``equalize`` per (frame, channel),
    resize only if ``H > S or W > S`` (``resized_size``; ``interpolate(x.float(), size, mode='bilinear', antialias=True,
    align_corners=False)``, then ``torch.round`` back to levels, as torchvision does for uint8 tensors), ``(level / 255.0 -
    mean_c) / std_c``. torchvision is not installed where this was written: parity with torchvision's own ``resize`` is unpinned."""

    def __init__(self, target_size: int = 368, **kwargs):
        self._target_size = int(target_size)

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(target_size={self._target_size})'

    def __call__(self, clip) -> Tensor:
        if not isinstance(clip, Tensor):
            clip = torch.from_numpy(np.ascontiguousarray(clip))
        clip = equalize(clip.permute((0, 3, 1, 2)))
        size = resized_size(clip.shape[2], clip.shape[3], self._target_size)
        if size != tuple(clip.shape[2:]):
            clip = torch.round(resize_levels(clip, size))
        return normalize_levels(clip)


# ---- the batched pipeline -----------------------------------------------------------------------------------------------------
class ClipFramesPipeline:
    """``VideoMixin.__getitem__`` (video_mixin.py:88-141) for a whole batch: called with the decoded clips (a list of uint8
    (T, H_i, W_i, 3) arrays or tensors), the batch's ``targets`` and ``meta``; returns ``(frames (N,T,3,h,w) fp32, targets, meta)``.

      targets['heatmaps_shift']  (N,T,2) fp32 holding the integer shifts of ``crop_bbox`` (zeros without the crop)
      meta['original_size']      the (height, width) that was resized -- the canvas under the crop, which is what the reference
                                 hands to ``_add_heatmaps_to_targets``: one tuple when every clip has the same, otherwise a list
                                 of N tuples (the flow's own target builder takes the single tuple only)
      targets['heatmaps']        when ``heatmaps`` (a ``HeatmapTargets``) is given: the maps at the resolution its pool gives for
                                 the frames written here, by ONE ``ops.heatmap_targets`` call on centres pre-scaled per clip in
                                 fp32 -- ``(kp - shift) * scale_i``, then shift 0 and scale (1, 1) -- so clips with different
                                 canvas sizes share a batch.

    With ``bbox_crop`` the bboxes come from ``targets['bboxes']`` (N,T,2,2) and are read on the host (centres, canvas sizes and
    shifts are a few integers per frame); without it all clips must share (H, W), else ``ValueError``. Frames on the device go
    through K33 (``ops.clip_frames``); host clips, and ``P2C_FRAMES_FRAMEWORK=1``, through the tensor code of this module.
    Like the reference, it refuses ``augment_*`` arguments."""

    def __init__(self, target_size: int = 368, bbox_crop: bool = False, bbox_margin: float = 0.2,
                 heatmaps: Optional[HeatmapTargets] = None, device=None, **kwargs):
        if any(v for k, v in kwargs.items() if k.startswith('augment_')):
            raise ValueError('VideoMixin does not support augment_* args.')
        self.target_size, self.bbox_crop, self.bbox_margin = int(target_size), bool(bbox_crop), float(bbox_margin)
        self.heatmaps, self.device = heatmaps, device

    @staticmethod
    def add_cli_args(parser):
        """reference video_mixin.py:62-85 (``--heatmaps_sigma`` belongs to ``HeatmapTargets.add_cli_args``)."""
        from pedestrians_video_2_carla_amd.modules.movements.linear import boolean
        parser.add_argument('--frames_target_size', type=int, default=368, help='Size of the image inserted into the network.')
        parser.add_argument('--frames_bbox_crop', type=boolean, default=False,
                            help='Should image be cropped to square centered on bbox?')
        parser.add_argument('--frames_bbox_margin', type=float, default=0.2, help='Margin around bbox to crop.')
        return parser

    def geometry(self, clips: Sequence, targets: Dict[str, Any]):
        """Host side: per clip (canvas or None, centres or None, shifts (T,2) int array, resized-from (h, w), output (h, w))."""
        out = []
        if self.bbox_crop:
            bboxes = targets['bboxes']
            bboxes = np.asarray(bboxes.detach().cpu() if isinstance(bboxes, Tensor) else bboxes)
        for i, clip in enumerate(clips):
            T, H, W = (int(v) for v in clip.shape[:3])
            if self.bbox_crop:
                canvas, centres, shifts = crop_geometry(bboxes[i], (H, W), self.bbox_margin, self.target_size)
                size = (canvas, canvas)
            else:
                canvas, centres, shifts, size = None, None, np.zeros((T, 2), dtype=int), (H, W)
            out.append((canvas, centres, shifts, size, resized_size(size[0], size[1], self.target_size)))
        return out

    def __call__(self, clips: Sequence, targets: Dict[str, Any], meta: Dict[str, Any]):
        from pedestrians_video_2_carla_amd import ops
        if len(clips) == 0:
            raise ValueError('ClipFramesPipeline: an empty batch')
        if not self.bbox_crop and len({tuple(c.shape[1:3]) for c in clips}) != 1:
            raise ValueError('ClipFramesPipeline: without frames_bbox_crop all clips of a batch must share (H, W), got '
                             f'{sorted({tuple(int(v) for v in c.shape[1:3]) for c in clips})}')
        geo = self.geometry(clips, targets)
        if len({g[4] for g in geo}) != 1:
            raise ValueError(f'ClipFramesPipeline: the clips resize to different sizes {sorted({g[4] for g in geo})}')
        device = self.device
        if device is None:
            device = clips[0].device if isinstance(clips[0], Tensor) else torch.device('cpu')
        clips = [(c if isinstance(c, Tensor) else torch.from_numpy(np.ascontiguousarray(c))).to(device) for c in clips]
        frames = ops.clip_frames(clips, self.target_size, centres=[g[1] for g in geo] if self.bbox_crop else None,
                                 canvas=[g[0] for g in geo] if self.bbox_crop else None)
        shifts = torch.from_numpy(np.stack([g[2] for g in geo])).to(device=frames.device, dtype=torch.float32)
        targets['heatmaps_shift'] = shifts
        sizes = [g[3] for g in geo]
        meta['original_size'] = sizes[0] if len(set(sizes)) == 1 else sizes
        if self.heatmaps is not None:
            h, w = frames.shape[-2:]
            kp = targets['projection_2d'][..., :2].to(device=frames.device, dtype=torch.float32)
            scale = torch.tensor([[w / float(ow), h / float(oh)] for oh, ow in sizes], dtype=torch.float64).float()
            scaled = (kp - shifts[:, :, None, :]) * scale.to(frames.device)[:, None, None, :]
            targets['heatmaps'] = ops.heatmap_targets(scaled, torch.zeros_like(shifts), (1.0, 1.0), (h, w), self.heatmaps.sigma,
                                                      self.heatmaps.pool)
        return frames, targets, meta
