"""K33 (ops.clip_frames) against the tensor definition of data/base/video.py on the device (P2C_FRAMES_FRAMEWORK=1).

    python tools/bench_frames.py [N ...]        # clips per batch, default 2

Per batch size: N decoded clips of T = 16 frames at 1920 x 1080 (uint8, already on the device in one packed buffer), target size
368, with and without the bbox crop (bboxes around 300 px wandering over the frame, some hanging over a border; canvas 420):
  crop      420 x 420 canvas -> 368 x 368   (the tensor arm pastes the canvas frame by frame, equalizes, interpolates, normalises)
  full      1080 x 1920 -> 368 x 654
Both arms get the same packed buffer and integer centres (host arrays: one small upload per call in the K33 arm, as a loader
would issue it) and their results are compared before timing (levels that differ, largest difference). Times are device events
around windows of ``REPS`` calls (launch gaps and the host's share included: time per call, not kernel time), the two arms
alternating window by window; the median window of each arm is reported with its spread. One JSON line.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.data.base import video as V

T, H, W, S, BOX, REPS, ROUNDS = 16, 1080, 1920, 368, 300, 3, 7
ARMS = (('k33', '0'), ('framework', '1'))


def window(fn, reps=REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def alternate(fn):
    def armed(env):
        def run():
            os.environ['P2C_FRAMES_FRAMEWORK'] = env
            return fn()
        return run
    calls = {name: armed(env) for name, env in ARMS}
    for call in calls.values():
        window(call, 1)
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call))
    res = {name: {'us_per_call': round(statistics.median(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1)}
           for name, v in times.items()}
    res['ratio'] = round(res['framework']['us_per_call'] / res['k33']['us_per_call'], 2)
    os.environ['P2C_FRAMES_FRAMEWORK'] = '0'
    return res


def both(fn):
    got = {}
    for name, env in ARMS:
        os.environ['P2C_FRAMES_FRAMEWORK'] = env
        got[name] = fn()
    os.environ['P2C_FRAMES_FRAMEWORK'] = '0'
    return got['k33'], got['framework']


def levels(frames):
    mean, std = (torch.tensor(v, device=frames.device)[:, None, None] for v in (V.IMAGENET_MEAN, V.IMAGENET_STD))
    return torch.round((frames * std + mean) * 255)


def case(N, device):
    g = torch.Generator(device=device).manual_seed(33)
    # smooth-ish content: a random low-resolution field blown up, plus noise -- a histogram that is neither flat nor a spike
    clips = []
    for _ in range(N):
        base = torch.rand(T, 3, H // 40, W // 40, generator=g, device=device)
        img = torch.nn.functional.interpolate(base, size=(H, W), mode='bilinear') * 200 + torch.rand(T, 3, H, W, generator=g, device=device) * 55
        clips.append(img.permute(0, 2, 3, 1).to(torch.uint8).contiguous())
    packed = ops.pack_clips(clips)
    del clips
    rng = np.random.default_rng(33)
    bboxes = []
    for _ in range(N):
        cx = np.linspace(rng.uniform(-50, W / 2), rng.uniform(W / 2, W + 50), T)
        cy = np.linspace(rng.uniform(100, H - 100), rng.uniform(100, H - 100), T)
        bboxes.append(np.stack([np.stack([cx - BOX / 2, cy - BOX / 2], -1), np.stack([cx + BOX / 2, cy + BOX / 2], -1)], 1))
    geo = [V.crop_geometry(b, (H, W), 0.2, S) for b in bboxes]
    canvas, centres = [q[0] for q in geo], [q[1] for q in geo]
    out = {'N': N, 'canvas': canvas[0], 'source_MB_per_call': round(packed.buffer.numel() / 1e6, 1)}
    for name, kw in (('crop', dict(centres=centres, canvas=canvas)), ('full', {})):
        def call():
            return ops.clip_frames(packed, S, **kw)
        a, b = both(call)
        diff = (levels(a) - levels(b)).abs()
        out[name] = {**alternate(call), 'out_shape': list(a.shape), 'levels_differing': int((diff > 0).sum()),
                     'largest_level_difference': int(diff.max())}
        del a, b, diff
    return out


def main():
    device = torch.device('cuda:0')
    out = {'tool': 'bench_frames', 'T': T, 'frame': (H, W), 'target_size': S, 'bbox_px': BOX, 'reps_per_window': REPS, 'windows': ROUNDS,
           'timing': 'device events around windows of calls (launch gaps included)', 'cases': []}
    for N in [int(a) for a in sys.argv[1:]] or [2]:
        out['cases'].append(case(N, device))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
