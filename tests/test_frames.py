"""K33 (csrc/p2c_frames.hip, ``ops.clip_frames``, ``data.base.video``) -- what runs without a GPU: the crop against the reference's
own ``crop_bbox`` (tests/golden/frames.npz), ``equalize`` against PIL, the resize rule, the pipeline's targets against a per-clip
loop, and the C-ABI surface."""
import argparse
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.base import video as V
from pedestrians_video_2_carla_amd.data.base.heatmaps import HeatmapTargets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ('centred', 'borders', 'corner', 'odd', 'small')
POOL = (9, 8, 1)


# ---- crop -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('as_tensor', [False, True], ids=['array', 'tensor'])
@pytest.mark.parametrize('tag', CASES)
def test_crop_bbox_reproduces_the_reference(golden, tag, as_tensor):
    g = golden('frames')
    bboxes, margin, target = g[f'{tag}_bboxes'].numpy(), float(g[f'{tag}_margin']), int(g[f'{tag}_target'])
    frames = g['frames'][:len(bboxes)]
    canvas, shifts = V.crop_bbox(frames if as_tensor else frames.numpy(), bboxes, bbox_margin=margin, target_size=target)
    assert isinstance(canvas, torch.Tensor if as_tensor else np.ndarray)
    canvas = canvas if as_tensor else torch.from_numpy(canvas)
    assert canvas.dtype == torch.uint8 and torch.equal(canvas, g[f'{tag}_canvas'])
    assert np.array_equal(shifts, g[f'{tag}_shifts'].numpy())
    size, centres, shifts2 = V.crop_geometry(bboxes, frames.shape[1:3], margin, target)
    assert size == canvas.shape[1] == canvas.shape[2] and np.array_equal(shifts2, shifts) and centres.shape == (len(bboxes), 2)


def test_the_fixture_holds_the_cases_it_names(golden):
    g = golden('frames')
    assert g['odd_canvas'].shape[1] % 2 == 1 and not g['odd_canvas'][:, -1].any() and not g['odd_canvas'][:, :, -1].any()
    assert g['small_canvas'].shape[1] == int(g['small_target'])
    s = g['borders_shifts']
    assert s[0, 0] < 0 and s[1, 1] < 0 and s[2, 0] + g['borders_canvas'].shape[1] > 64          # left, top, right
    assert g['corner_shifts'][0, 1] + g['corner_canvas'].shape[1] > 48 and (g['corner_shifts'][1] < 0).all()


def test_a_centre_far_outside_gives_a_zero_canvas():
    frames = torch.full((1, 48, 64, 3), 7, dtype=torch.uint8)
    canvas, _ = V.crop_bbox(frames, np.array([[[500.0, 20.0], [520.0, 40.0]]]), target_size=24)
    assert canvas.shape == (1, 28, 28, 3) and not canvas.any()


# ---- equalize -------------------------------------------------------------------------------------------------------------------
def equalize_images():
    g = torch.Generator().manual_seed(33)
    rnd = lambda *s, lo=0, hi=256: torch.randint(lo, hi, s, generator=g, dtype=torch.uint8)       # noqa: E731
    half = rnd(31, 45)
    half[:, :22] = 0
    skew = (torch.rand(40, 40, generator=g) ** 4 * 255).to(torch.uint8)
    return {'random': rnd(37, 53), 'random_small': rnd(16, 17), 'narrow': rnd(33, 29, lo=100, hi=110), 'two_levels': rnd(20, 20, lo=7, hi=9),
            'constant': torch.full((19, 23), 77, dtype=torch.uint8), 'zeros': torch.zeros(12, 12, dtype=torch.uint8),
            'half_zero': half, 'skewed': skew, 'few_pixels': rnd(14, 18), 'tiny': rnd(3, 5)}


@pytest.mark.parametrize('name', list(equalize_images()))
def test_equalize_equals_pil(name):
    ImageOps = pytest.importorskip('PIL.ImageOps')
    from PIL import Image
    img = equalize_images()[name]
    want = torch.from_numpy(np.array(ImageOps.equalize(Image.fromarray(img.numpy(), mode='L'))))
    got = V.equalize(img)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    hist = torch.bincount(img.flatten().long(), minlength=256)
    step = int(hist[hist != 0][:-1].sum()) // 255
    # step == 0: a single level, fewer than 255 pixels, or fewer than 255 pixels below the last level -- left unchanged
    assert (step == 0) == (name in ('constant', 'zeros', 'few_pixels', 'tiny', 'two_levels'))
    assert torch.equal(got, img) == (step == 0)


def test_equalize_treats_every_frame_and_channel_alone():
    imgs = equalize_images()
    stack = torch.stack([imgs['random'][:30, :40], imgs['skewed'][:30, :40], imgs['narrow'][:30, :29].repeat(1, 2)[:, :40],
                         torch.full((30, 40), 9, dtype=torch.uint8)]).view(2, 2, 30, 40)
    got = V.equalize(stack)
    for f in range(2):
        for c in range(2):
            assert torch.equal(got[f, c], V.equalize(stack[f, c]))
    with pytest.raises(TypeError):
        V.equalize(stack.float())


# ---- sizes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw, S, want', [
    ((1080, 1920), 368, (368, 654)),      # landscape: int(368 * 1920 / 1080) = 654
    ((64, 48), 24, (32, 24)),             # portrait
    ((49, 49), 48, (48, 48)),             # square
    ((16, 24), 16, (16, 24)),             # the short side already equals S: unchanged though the long side exceeds it
    ((20, 24), 24, (20, 24)), ((9, 7), 24, (9, 7)),      # both sides <= S: untouched
    ((500, 300), 368, (613, 368)),        # only the long side exceeds S: the short one still goes to S (up)
    ((200, 300), 32, (32, 48)), ((9, 9), 8, (8, 8)),
])
def test_resized_size_follows_the_rule(hw, S, want):
    assert V.resized_size(*hw, S) == want
    clip = torch.randint(0, 256, (1, *hw, 3), dtype=torch.uint8) if hw[0] * hw[1] < 10000 else None
    if clip is not None:
        out = V.VideoToResNet(S)(clip)
        assert out.shape == (1, 3, *want) and out.dtype == torch.float32
        assert torch.equal(out, V.VideoToResNet(S)(clip.numpy()))


def test_video_to_resnet_without_resize_is_lut_and_normalisation():
    clip = torch.randint(0, 256, (2, 16, 24, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
    out = V.VideoToResNet(16)(clip)
    eq = V.equalize(clip.permute(0, 3, 1, 2)).float()
    for c in range(3):
        want = (eq[:, c] / 255.0 - V.IMAGENET_MEAN[c]) / V.IMAGENET_STD[c]
        torch.testing.assert_close(out[:, c], want, rtol=0, atol=4e-7)       # two fp32 divisions either way, |value| < 2.7
    levels = torch.round(torch.clamp((out * torch.tensor(V.IMAGENET_STD)[:, None, None] + torch.tensor(V.IMAGENET_MEAN)[:, None, None]) * 255, 0, 255))
    assert torch.equal(levels, eq)


# ---- pipeline -------------------------------------------------------------------------------------------------------------------
def pipeline_batch(golden):
    g = golden('frames')
    clips = [g['frames'][:2].numpy(), g['frames'][:2].flip(0).contiguous()]           # an array and a tensor
    bboxes = torch.stack([g['centred_bboxes'][:2], g['odd_bboxes']])                    # fp64; canvases 28 and 35
    gen = torch.Generator().manual_seed(4)
    centre = bboxes.mean(-2).float()                                                    # (2,2,2)
    kp = centre[:, :, None, :] + (torch.rand(2, 2, 5, 2, generator=gen) - 0.5) * 30
    kp[0, 0, 1] = 0                                                                     # a missing joint, as stored
    return clips, {'bboxes': bboxes, 'projection_2d': kp}


def test_pipeline_targets_equal_a_per_clip_loop(golden):
    clips, targets = pipeline_batch(golden)
    hm = HeatmapTargets(sigma=1, clip_size=(24, 24), pool=POOL)
    pipe = V.ClipFramesPipeline(target_size=24, bbox_crop=True, bbox_margin=0.2, heatmaps=hm)
    frames, out, meta = pipe(clips, dict(targets), {})
    assert frames.shape == (2, 2, 3, 24, 24) and frames.dtype == torch.float32
    assert meta['original_size'] == [(28, 28), (35, 35)]
    assert out['heatmaps_shift'].shape == (2, 2, 2) and out['heatmaps_shift'].dtype == torch.float32
    assert out['heatmaps'].shape == (2, 2, 6, 3, 3)
    for i, clip in enumerate(clips):
        canvas, shifts = V.crop_bbox(clip, targets['bboxes'][i].numpy(), 0.2, 24)
        assert torch.equal(out['heatmaps_shift'][i], torch.from_numpy(shifts).float())
        assert meta['original_size'][i] == tuple(canvas.shape[1:3])
        assert torch.equal(frames[i], V.VideoToResNet(24)(canvas))
        oh, ow = canvas.shape[1:3]
        # the reference's _get_heatmap (K28a at full resolution restates it bit for bit, tests/test_heatmaps.py), then the flow's pool
        full = ops.heatmap_targets(targets['projection_2d'][i:i + 1], torch.from_numpy(shifts).float()[None], (24 / ow, 24 / oh),
                                   (24, 24), 1, pool=None)
        want = torch.nn.functional.avg_pool2d(full[0], kernel_size=9, stride=8, padding=1)
        got = out['heatmaps'][i]
        assert (want[:, 1:] > 0).any() and torch.equal(got == 0, want == 0)
        torch.testing.assert_close(got, want, rtol=0, atol=81 * 2.0 ** -24)          # tests/test_heatmaps.py's bound for pooled maps


def test_pipeline_without_crop(golden):
    g = golden('frames')
    clips = [g['frames'][:2], g['frames'][1:3]]
    frames, targets, meta = V.ClipFramesPipeline(target_size=24)(clips, {}, {})
    assert frames.shape == (2, 2, 3, 24, 32) and meta['original_size'] == (48, 64)
    assert targets['heatmaps_shift'].shape == (2, 2, 2) and not targets['heatmaps_shift'].any()
    assert torch.equal(frames[1], V.VideoToResNet(24)(clips[1]))
    with pytest.raises(ValueError, match='share'):
        V.ClipFramesPipeline(target_size=24)([clips[0], clips[1][:, :40]], {}, {})
    with pytest.raises(ValueError, match='augment'):
        V.ClipFramesPipeline(target_size=24, augment_rotation=True)
    V.ClipFramesPipeline(target_size=24, augment_rotation=False)


def test_cli_args():
    args = V.ClipFramesPipeline.add_cli_args(argparse.ArgumentParser()).parse_args([])
    assert (args.frames_target_size, args.frames_bbox_crop, args.frames_bbox_margin) == (368, False, 0.2)
    args = V.ClipFramesPipeline.add_cli_args(argparse.ArgumentParser()).parse_args(
        ['--frames_target_size', '184', '--frames_bbox_crop', 'true', '--frames_bbox_margin', '0.3'])
    assert (args.frames_target_size, args.frames_bbox_crop, args.frames_bbox_margin) == (184, True, 0.3)


def test_op_on_host_clips_is_the_definition(golden, monkeypatch):
    g = golden('frames')
    clips = [g['frames'][:2]]
    size, centres, _ = V.crop_geometry(g['odd_bboxes'].numpy(), (48, 64), 0.2, 24)
    assert not ops.clip_frames_supported(clips, 24, [size])
    got = ops.clip_frames(clips, 24, centres=[centres], canvas=[size])
    assert torch.equal(got[0], V.VideoToResNet(24)(g['odd_canvas']))
    packed = ops.pack_clips([g['frames'][:2], g['frames'][:2, :40, :50].contiguous()])
    assert packed.offsets == (0, 2 * 48 * 64 * 3) and torch.equal(packed.clip(1), g['frames'][:2, :40, :50])
    with pytest.raises(RuntimeError, match='different sizes'):
        ops.clip_frames(packed, 24)
    with pytest.raises(RuntimeError, match='together'):
        ops.clip_frames(clips, 24, canvas=[size])
    monkeypatch.setenv('P2C_FRAMES_FRAMEWORK', '1')
    assert ops.frames_framework()


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_frames_symbols_are_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    lib = getattr(_lib.lib(), '_h', _lib.lib())                         # the plain handle, also under the LDS audit
    for name in ('p2c_clip_frames_workspace_bytes', 'p2c_clip_frames_fwd'):
        assert name in declared and name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    res, args = _lib.SYMBOLS['p2c_clip_frames_fwd']
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p          # the stream goes last: the LDS-poison audit wraps the call
    wrapped = _lib._PoisonedLib(lib)._wrap
    assert 'p2c_clip_frames_fwd' in wrapped and 'p2c_clip_frames_workspace_bytes' not in wrapped
    assert int(re.search(r'#define P2C_FRAMES_MAX_CLIPS (\d+)', header).group(1)) == _lib.P2C_FRAMES_MAX_CLIPS
    assert int(re.search(r'#define P2C_FRAMES_MAX_SIDE (\d+)', header).group(1)) == _lib.P2C_FRAMES_MAX_SIDE
    # the workspace is a function of the frame count: 3 x 256 int32 counts per frame
    for frames in (0, 1, 16, 64 * 16):
        assert lib.p2c_clip_frames_workspace_bytes(frames) == frames * 3 * 256 * 4
    assert lib.p2c_clip_frames_workspace_bytes(-1) < 0
    # refusals come before any launch (no GPU is touched): a null descriptor, a bad clip count
    assert lib.p2c_clip_frames_fwd(None, None) == -1
    d = _lib.ClipFramesDesc()
    d.N, d.T = _lib.P2C_FRAMES_MAX_CLIPS + 1, 1
    assert lib.p2c_clip_frames_fwd(ctypes.byref(d), None) == -2
    d.N, d.src_bytes = 1, 10
    d.clips[0].H, d.clips[0].W, d.clips[0].out_h, d.clips[0].out_w = 2, 2, 2, 2       # 12 bytes > src_bytes
    assert lib.p2c_clip_frames_fwd(ctypes.byref(d), None) == -2
    d.src_bytes = 12
    assert lib.p2c_clip_frames_fwd(ctypes.byref(d), None) == -1                        # no pointers


def test_frames_descriptor_layout_matches_the_header(tmp_path):
    lines = ['  printf("sizeof %zu\\n", sizeof(p2c_clip_frames_desc));', '  printf("sizeof_clip %zu\\n", sizeof(p2c_clip_frames_clip));']
    lines += [f'  printf("{f} %zu\\n", offsetof(p2c_clip_frames_desc, {f}));' for f, _ in _lib.ClipFramesDesc._fields_]
    lines += [f'  printf("clip_{f} %zu\\n", offsetof(p2c_clip_frames_clip, {f}));' for f, _ in _lib.ClipFramesClip._fields_]
    src = tmp_path / 'frames_desc.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n' + '\n'.join(lines) + '\n  return 0;\n}\n')
    exe = tmp_path / 'frames_desc'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(out['sizeof']) == ctypes.sizeof(_lib.ClipFramesDesc) < 4096             # the table stays in the kernel arguments
    assert int(out['sizeof_clip']) == ctypes.sizeof(_lib.ClipFramesClip)
    for f, _ in _lib.ClipFramesDesc._fields_:
        assert int(out[f]) == getattr(_lib.ClipFramesDesc, f).offset, f
    for f, _ in _lib.ClipFramesClip._fields_:
        assert int(out['clip_' + f]) == getattr(_lib.ClipFramesClip, f).offset, f
