"""GPU: K33 (csrc/p2c_frames.hip, ``ops.clip_frames``) against the tensor definition of data/base/video.py on the CPU.

Without resampling the kernel is integer look-ups and two IEEE divisions: equal bits. With resampling it forms its tap geometry in
fp64 and its weights and sums in fp32, in another order than ATen's separable fp32 kernel, so the unrounded level differs in the
last bits and the rounded level can differ where the exact value sits on a rounding tie. The bound: every output within one level
of the fp32 tensor path, and equal bits wherever the fp64 tensor definition's unrounded level is farther than delta from k + 0.5;
delta = 4 x the largest difference between the fp32 and the fp64 tensor definitions on the case's own input (measured on the CPU,
below), the 4 x for a kernel that places its fp32 roundings elsewhere; at most 2 % of the outputs may be left out that way.

Measured on the CPU for the inputs of this file (max |fp32 - fp64| of the unrounded levels -> delta, share left out by delta):
  one_block  9 -> 8           3.4e-5 -> 1.3e-4, 0.52 %     borders    28, 35 -> 24          3.5e-4 -> 1.4e-3, 0.14 %
  three_taps 49 -> 48         8.6e-4 -> 3.4e-3, 0.58 %     many_taps  200 x 300 -> 32 x 48  4.1e-5 -> 1.6e-4, 0 %
  mixed      28, 35 -> 24     3.6e-4 -> 1.5e-3, 0.28 %     degenerate 40 -> 24              1.7e-4 -> 6.7e-4, 0.23 %
  constant   20 x 30 -> 16 x 24   3.1e-5 -> 1.2e-4, 1.39 % (scale 1.25 and a two-level channel: exact ties, not near ones)
(the test prints the figures of its own run). A CPU emulation of the kernel's arithmetic (fp64 tap geometry, fp32 weights, fused
multiply-adds in tap order) differed from the fp32 tensor path in 0 to 5 outputs per clip, every one of them inside delta."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.base import video as V
from pedestrians_video_2_carla_amd.data.base.heatmaps import HeatmapTargets

pytestmark = pytest.mark.gpu

MAX_LEFT_OUT = 0.02


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def box(cx, cy, w, h):
    return [[cx - w / 2.0, cy - h / 2.0], [cx + w / 2.0, cy + h / 2.0]]


def frames_of(g, T, H, W):
    """uint8 (T,H,W,3): channel 0 uniform, channel 1 in a narrow band, channel 2 skewed towards dark -- three different tables."""
    c0 = torch.randint(0, 256, (T, H, W), generator=g)
    c1 = torch.randint(90, 140, (T, H, W), generator=g)
    c2 = (torch.rand(T, H, W, generator=g) ** 3 * 255).long()
    return torch.stack((c0, c1, c2), -1).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(clips, bboxes or None, target size). The bboxes are (T,2,2) fp64 arrays per clip. Never modified."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    if name == 'one_block':                      # one workgroup, scale 1.125
        # 9 -> 8 has normalised weights in multiples of 1/20 per axis: the exact level is a multiple of 1/400 and lands on k + 0.5
        # for 1 - 2 % of random inputs (measured over twelve seeds: 1 to 7 of the 192 outputs). Four such outputs would already
        # exceed the 2 % cap on their own, so this case takes a seed of its own, one with a single exact tie.
        return [frames_of(torch.Generator().manual_seed(7), 1, 9, 9)], None, 8
    if name == 'no_resize':                      # the short side equals S: look-up and normalisation only
        return [frames_of(g, 2, 16, 24)], None, 16
    if name == 'borders':                        # the canvas over each border; clip 1's canvas is odd (35), clip 0's is 28
        b0 = np.array([box(5.0, 24.0, 20, 20), box(30.0, 3.0, 20, 20), box(61.0, 20.0, 20, 20)])
        b1 = np.array([box(40.0, 46.0, 25, 20), box(-2.0, 1.0, 20, 25), box(31.5, 23.5, 25, 25)])
        return [frames_of(g, 3, 48, 64), frames_of(g, 3, 48, 64)], [b0, b1], 24
    if name == 'three_taps':                     # canvas int(35 * 1.4) = 49 -> 48: scale ~ 1.02
        b = [np.array([box(24.0, 25.0, 35, 30), box(20.5, 30.0, 30, 35)]), np.array([box(40.0, 10.0, 35, 35), box(25.0, 24.0, 35, 20)])]
        return [frames_of(g, 2, 49, 49), frames_of(g, 2, 49, 49)], b, 48
    if name == 'many_taps':                      # scale 6.25: 13-14 taps, 32 x 48 outputs = 4 tiles
        return [frames_of(g, 1, 200, 300)], None, 32
    if name == 'mixed':                          # three frame sizes, canvases 28, 35 and 24 (= S: that clip is not resampled)
        b = [np.array([box(30.0, 20.0, 20, 16), box(3.0, 40.0, 20, 20)]), np.array([box(25.0, 20.0, 25, 11), box(48.0, 2.0, 13, 25)]),
             np.array([box(10.0, 10.0, 6, 5), box(69.0, 32.0, 4, 6)])]
        return [frames_of(g, 2, 48, 64), frames_of(g, 2, 40, 50), frames_of(g, 2, 33, 70)], b, 24
    if name == 'degenerate':                     # a 10 x 12 frame on a 40 x 40 canvas (1 480 of 1 600 pixels are padding), green constant
        clip = frames_of(g, 2, 10, 12)
        clip[..., 1] = 50
        clip[1, ..., 2] = 0                      # frame 1: blue is zero like the padding -- one level in the whole image
        return [clip], [np.array([box(6.0, 5.0, 29, 20), box(2.0, 9.0, 29, 29)])], 24
    if name == 'constant':                       # no crop: a constant channel and a two-level channel (step 0: unchanged)
        clip = frames_of(g, 1, 20, 30)
        clip[..., 0] = 200
        clip[..., 2] = (clip[..., 2] > 40).to(torch.uint8) * 9 + 3
        return [clip], None, 16
    raise KeyError(name)


CASES = ('one_block', 'no_resize', 'borders', 'three_taps', 'many_taps', 'mixed', 'degenerate', 'constant')


@functools.lru_cache(maxsize=None)
def geometry(name):
    clips, bboxes, S = problem(name)
    if bboxes is None:
        return None, None, [np.zeros((c.shape[0], 2), dtype=int) for c in clips], [tuple(c.shape[1:3]) for c in clips]
    geo = [V.crop_geometry(b, tuple(c.shape[1:3]), 0.2, S) for c, b in zip(clips, bboxes)]
    return [g[0] for g in geo], [g[1] for g in geo], [g[2] for g in geo], [(g[0], g[0]) for g in geo]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The tensor definition on the CPU, computed once: (frames fp32, per clip the exact-comparison mask or None, delta, left out)."""
    clips, bboxes, S = problem(name)
    canvas, centres, _, _ = geometry(name)
    want = ops.clip_frames(clips, S, centres=centres, canvas=canvas)                 # host tensors: the tensor path
    masks, delta, left_out, total = [], 0.0, 0, 0
    for i, clip in enumerate(clips):
        image = clip if bboxes is None else V.crop_bbox(clip, bboxes[i], 0.2, S)[0]
        assert torch.equal(want[i], V.VideoToResNet(S)(image))                        # the op's paste = crop_bbox
        eq = V.equalize(image.permute(0, 3, 1, 2))
        size = V.resized_size(*eq.shape[2:], S)
        if size == tuple(eq.shape[2:]):
            masks.append(None)
            continue
        u64, u32 = V.resize_levels(eq, size, torch.float64), V.resize_levels(eq, size, torch.float32)
        masks.append((u64, (u32.double() - u64).abs().max().item()))
    diffs = [m[1] for m in masks if m is not None]
    if diffs:
        delta = 4 * max(diffs)
        for k, m in enumerate(masks):
            if m is not None:
                exact = ((m[0] - torch.floor(m[0])) - 0.5).abs() > delta
                masks[k] = exact
                left_out += int((~exact).sum())
                total += exact.numel()
    return want, masks, delta, (left_out / total if total else 0.0)


def levels_of(frames):
    mean, std = (torch.tensor(v, dtype=torch.float64)[:, None, None] for v in (V.IMAGENET_MEAN, V.IMAGENET_STD))
    return torch.round((frames.double() * std + mean) * 255)


def run(name, packed=False):
    clips, _, S = problem(name)
    canvas, centres, _, _ = geometry(name)
    on = [c.to(dev()) for c in clips]
    assert ops.clip_frames_supported(on, S, canvas)
    return ops.clip_frames(ops.pack_clips(on) if packed else on, S, centres=centres, canvas=canvas)


def compare(name, got):
    want, masks, delta, left_out = reference(name)
    assert got.shape == want.shape and got.dtype == torch.float32
    got = got.cpu()
    assert torch.isfinite(got).all()
    print(f'{name}: delta {delta:.2e}, left out of the exact comparison {100 * left_out:.3f} %')
    assert left_out <= MAX_LEFT_OUT
    for i, mask in enumerate(masks):
        if mask is None:
            assert torch.equal(got[i], want[i]), f'{name}: clip {i} is not resampled -- equal bits expected'
            continue
        off = (levels_of(got[i]) - levels_of(want[i])).abs()
        differing = int((got[i] != want[i]).sum())
        print(f'  clip {i}: {differing} of {got[i].numel()} outputs differ from the fp32 tensor path, largest {int(off.max())} level(s), '
              f'{int((got[i] != want[i])[mask].sum())} of them away from a tie')
        assert off.max() <= 1                                               # one level = (1 / 255) / std_c in the output
        assert torch.equal(got[i][mask], want[i][mask])


@pytest.mark.parametrize('name', CASES)
def test_clip_frames(name):
    got = run(name)
    compare(name, got)
    assert torch.equal(run(name, packed=True), got)                         # two runs, a list or a packed buffer: the same bits
    if name in ('degenerate', 'constant'):
        clips, _, _ = problem(name)
        want = reference(name)[0]
        if name == 'constant':                                              # step == 0: red and blue keep their levels
            assert torch.equal(levels_of(got.cpu())[0, 0, 0], torch.full((16, 24), 200.0, dtype=torch.float64))
        else:                                                               # frame 1, blue: nothing but zeros in the image
            assert torch.equal(got.cpu()[0, 1, 2], want[0, 1, 2]) and levels_of(want)[0, 1, 2].abs().max() == 0


def test_shifts_and_sizes_are_the_reference_integers():
    clips, bboxes, S = problem('borders')
    on = [c.to(dev()) for c in clips]
    targets = {'bboxes': torch.from_numpy(np.stack(bboxes))}
    frames, targets, meta = V.ClipFramesPipeline(target_size=S, bbox_crop=True)(on, targets, {})
    assert frames.is_cuda and targets['heatmaps_shift'].is_cuda and meta['original_size'] == [(28, 28), (35, 35)]
    for i, clip in enumerate(clips):
        canvas, shifts = V.crop_bbox(clip.numpy(), bboxes[i], 0.2, S)
        assert torch.equal(targets['heatmaps_shift'][i].cpu().long(), torch.from_numpy(shifts))
        assert meta['original_size'][i] == canvas.shape[1:3]
    compare('borders', frames)
    # without the crop: zeros and the frame's own size
    clips, _, S = problem('many_taps')
    frames, targets, meta = V.ClipFramesPipeline(target_size=S)([c.to(dev()) for c in clips], {}, {})
    assert meta['original_size'] == (200, 300) and not targets['heatmaps_shift'].any() and frames.shape == (1, 1, 3, 32, 48)
    compare('many_taps', frames)


def test_direct_abi_call_gives_the_same_output():
    clips, _, S = problem('mixed')
    canvas, centres, _, _ = geometry('mixed')
    want = run('mixed')
    lib = _lib.lib()
    T = clips[0].shape[0]
    # the three clips behind 5 bytes of padding, each at an odd offset: every alignment of the row loads
    parts, offsets, at = [torch.zeros(5, dtype=torch.uint8)], [], 5
    for c in clips:
        offsets.append(at)
        parts += [c.reshape(-1), torch.zeros(3, dtype=torch.uint8)]
        at += c.numel() + 3
    src = torch.cat(parts).to(dev())
    cent = torch.from_numpy(np.stack(centres).astype(np.int32)).to(dev())
    out = torch.empty(3, T, 3, S, S, device=dev())
    work = torch.empty(lib.p2c_clip_frames_workspace_bytes(3 * T) // 4, dtype=torch.int32, device=dev())
    d = _lib.ClipFramesDesc()
    d.N, d.T, d.src_bytes, d.src, d.centres, d.workspace, d.out = 3, T, src.numel(), src.data_ptr(), cent.data_ptr(), work.data_ptr(), out.data_ptr()
    for k, c in enumerate(clips):
        d.clips[k].offset, d.clips[k].H, d.clips[k].W, d.clips[k].canvas = offsets[k], c.shape[1], c.shape[2], canvas[k]
        d.clips[k].out_h = d.clips[k].out_w = S
    _lib.check(lib.p2c_clip_frames_fwd(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), 'p2c_clip_frames_fwd')
    assert torch.equal(out, want)
    # the workspace holds the level counts of the pasted windows: per frame and channel, the window's pixel count
    counts = work.view(3, T, 3, 256).sum(-1).cpu()
    for i, c in enumerate(clips):
        for t in range(T):
            _, _, w, h, _, _ = V.paste_window((canvas[i] // 2,) * 2, centres[i][t], (c.shape[2], c.shape[1]))
            assert counts[i, t].tolist() == [w * h] * 3
    # refusals: a clip block that leaves the buffer, a misaligned workspace, crops without centres
    d.src_bytes = src.numel() - 4
    assert lib.p2c_clip_frames_fwd(ctypes.byref(d), None) == -2
    d.src_bytes, d.centres = src.numel(), None
    assert lib.p2c_clip_frames_fwd(ctypes.byref(d), None) == -1


def test_framework_switch_takes_the_tensor_path(monkeypatch):
    def refuse(*a):
        raise AssertionError('p2c_clip_frames_fwd was called')
    for name in ('no_resize', 'borders'):
        clips, _, S = problem(name)
        canvas, centres, _, _ = geometry(name)
        on = [c.to(dev()) for c in clips]
        with monkeypatch.context() as m:
            m.setattr(_lib.lib(), 'p2c_clip_frames_fwd', refuse, raising=False)
            with pytest.raises(AssertionError, match='p2c_clip_frames_fwd was called'):
                ops.clip_frames(on, S, centres=centres, canvas=canvas)
            m.setenv('P2C_FRAMES_FRAMEWORK', '1')
            assert ops.frames_framework() and not ops.clip_frames_supported(on, S, canvas)
            got = ops.clip_frames(on, S, centres=centres, canvas=canvas)
        assert got.is_cuda and torch.equal(got, ops._clip_frames_tensor(ops.pack_clips(on), S, centres, canvas))
        if name == 'no_resize':
            assert torch.equal(got.cpu(), reference(name)[0])               # no resampling: the CPU's bits
        else:
            assert (levels_of(got.cpu()) - levels_of(reference(name)[0])).abs().max() <= 1


def test_poison_audits(monkeypatch):
    """Every case again with every LDS byte NaN before each launch (``P2C_POISON_LDS=1``) and NaN- / INT_MAX-filled ``torch.empty``
    (``P2C_POISON_EMPTY=1``): an output element or a workspace count read before it was written would show."""
    clean = {name: run(name) for name in CASES}
    monkeypatch.setenv('P2C_POISON_LDS', '1')
    monkeypatch.setenv('P2C_POISON_EMPTY', '1')
    monkeypatch.setattr(_lib, '_lib', None)                  # the next lib() wraps every launch with the LDS poisoning
    deterministic, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    monkeypatch.setattr(torch.utils.deterministic, 'fill_uninitialized_memory', True)
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert isinstance(_lib.lib(), _lib._PoisonedLib) and bool(torch.isnan(torch.empty(8, device=dev())).all())
        assert bool((torch.empty(8, dtype=torch.int32, device=dev()) != 0).all())
        got = {name: run(name) for name in CASES}
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(deterministic, warn_only=warn_only)
    for name in CASES:
        assert torch.isfinite(got[name]).all() and torch.equal(got[name], clean[name]), name


def test_captured_call_replays_on_a_second_batch():
    clips, bboxes, S = problem('borders')
    canvas, centres, _, _ = geometry('borders')
    # a second batch of the same structure: other pixels, the two clips' bboxes swapped between frames (same canvas sizes)
    g = torch.Generator().manual_seed(99)
    clips2 = [frames_of(g, 3, 48, 64), frames_of(g, 3, 48, 64)]
    bboxes2 = [bboxes[0][::-1].copy(), bboxes[1][::-1].copy()]
    geo2 = [V.crop_geometry(b, (48, 64), 0.2, S) for b in bboxes2]
    assert [q[0] for q in geo2] == canvas
    centres2 = [q[1] for q in geo2]
    eager1 = ops.clip_frames([c.to(dev()) for c in clips], S, centres=centres, canvas=canvas)
    eager2 = ops.clip_frames([c.to(dev()) for c in clips2], S, centres=centres2, canvas=canvas)
    assert not torch.equal(eager1, eager2)
    packed = ops.pack_clips([c.to(dev()) for c in clips])
    cent = torch.from_numpy(np.stack(centres).astype(np.int32)).to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.clip_frames(packed, S, centres=cent, canvas=canvas)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.clip_frames(packed, S, centres=cent, canvas=canvas)
    graph.replay()
    assert torch.equal(out, eager1)
    packed.buffer.copy_(ops.pack_clips([c.to(dev()) for c in clips2]).buffer)
    cent.copy_(torch.from_numpy(np.stack(centres2).astype(np.int32)))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager2)


def test_flow_training_step_from_the_pipeline():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_estimation import LitPoseEstimationFlow
    from pedestrians_video_2_carla_amd.modules.pose_estimation import Linear
    clips, bboxes, S = problem('borders')
    g = torch.Generator().manual_seed(7)
    centre = torch.from_numpy(np.stack(bboxes)).mean(-2).float()                       # (2,3,2)
    kp = centre[:, :, None, :] + (torch.rand(2, 3, 26, 2, generator=g) - 0.5) * 24
    kp[1, 0, 3] = 0

    def flow():
        torch.manual_seed(5)
        return LitPoseEstimationFlow(movements_model=Linear(input_nodes=CARLA_SKELETON), loss_modes=['heatmaps'],
                                     transform='none').to(dev()).train()

    pipe = V.ClipFramesPipeline(target_size=S, bbox_crop=True, heatmaps=HeatmapTargets(sigma=1, clip_size=(S, S)))
    frames, targets, meta = pipe([c.to(dev()) for c in clips], {'bboxes': torch.from_numpy(np.stack(bboxes)), 'projection_2d': kp.to(dev())}, {})
    assert targets['heatmaps'].shape == (2, 3, 27, 3, 3) and targets['heatmaps'].is_cuda
    out = flow().training_step((frames, targets, meta), 0)
    loss = out['loss'].detach()
    assert torch.isfinite(loss) and float(loss) > 0
    # the same flow handed the frames and maps made by hand: K28a per clip with the clip's own shift and scale
    shift = targets['heatmaps_shift']
    made = torch.cat([ops.heatmap_targets(kp[i:i + 1].to(dev()), shift[i:i + 1], (S / float(ow), S / float(oh)), (S, S), 1, ops.HEATMAPS_POOL)
                      for i, (oh, ow) in enumerate(meta['original_size'])])
    assert torch.equal(made, targets['heatmaps'])
    by_hand = flow().training_step((frames, {'projection_2d': kp.to(dev()), 'heatmaps': made}, {}), 0)['loss'].detach()
    assert torch.equal(by_hand, loss)
