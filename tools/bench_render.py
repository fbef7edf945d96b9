"""K34 (ops.render_points) against the two renderers it can be measured against: its tensor definition on the device
(P2C_RENDER_FRAMEWORK=1) and the same definition on the host, where the reference draws, plus the copy of its points.

    python tools/bench_render.py [--host_videos N]

V = 10 videos of T = 30 frames, 800 x 600 panels of the CARLA skeleton (J = 26), the logger's defaults (radius 2, no bones), two
panels side by side and four in a square: what ``PedestrianWriter`` renders per logged batch. The arms get the same points and
their bytes are compared before timing. Device arms: device events around windows of ``REPS`` calls (launch gaps and the host's
share included), alternating window by window, median window with its spread; ``k34_to_host`` adds the copy of the frames to the
host (wall clock, what a logged batch costs the training loop). Host arm: wall clock of one call on the first ``--host_videos``
videos (default: all), reported per video. One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.renderers import PointsRenderer

V, T, W, H, REPS, ROUNDS = 10, 30, 800, 600, 3, 5
LAYOUTS = {2: (1, 2), 4: (2, 2)}
ARMS = (('k34', '0'), ('framework', '1'))


def window(fn, reps=REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def case(n_panels, device, host_videos):
    g = torch.Generator().manual_seed(34)
    renderer = PointsRenderer(CARLA_SKELETON, image_size=(W, H))
    # a pedestrian-sized cloud walking across the canvas
    centre = torch.stack([torch.linspace(200, 600, T), torch.full((T,), 300.0)], -1)
    host_points = [centre[None, :, None, :] + torch.randn(V, T, 26, 2, generator=g) * torch.tensor([40.0, 90.0]) for _ in range(n_panels)]
    panels = [renderer.render(p.to(device)) for p in host_points]
    kw = dict(size=(H, W), layout=LAYOUTS[n_panels], radius=renderer.radius, line_width=renderer.line_width)

    def call(env):
        def run():
            os.environ['P2C_RENDER_FRAMEWORK'] = env
            return ops.render_points(panels, **kw)
        return run
    calls = {name: call(env) for name, env in ARMS}
    got = {name: fn() for name, fn in calls.items()}
    out = {'panels': n_panels, 'out_shape': list(got['k34'].shape), 'out_MB': round(got['k34'].numel() / 1e6, 1),
           'device_arms_equal': bool(torch.equal(got['k34'], got['framework']))}
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            times[name].append(window(fn))
    for name, v in times.items():
        out[name] = {'us_per_call': round(statistics.median(v), 1), 'min': round(min(v), 1), 'max': round(max(v), 1)}
    out['framework_over_k34'] = round(out['framework']['us_per_call'] / out['k34']['us_per_call'], 1)
    os.environ['P2C_RENDER_FRAMEWORK'] = '0'
    walls = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        calls['k34']().cpu()
        walls.append((time.perf_counter() - t0) * 1e3)
    out['k34_to_host_ms'] = round(statistics.median(walls), 2)
    n = min(host_videos, V)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = ops.render_points([renderer.render(p[0][:n].cpu()) for p in panels], **kw)
    out['host'] = {'videos': n, 'ms_per_video': round((time.perf_counter() - t0) * 1e3 / n, 1),
                   'equal': bool(torch.equal(host, got['k34'][:n].cpu()))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--host_videos', type=int, default=V)
    args = ap.parse_args()
    device = torch.device('cuda:0')
    out = {'tool': 'bench_render', 'V': V, 'T': T, 'panel': (H, W), 'J': 26, 'reps_per_window': REPS, 'windows': ROUNDS,
           'timing': 'device events around windows of calls (launch gaps included); wall clock for *_ms', 'cases': []}
    for n_panels in LAYOUTS:
        out['cases'].append(case(n_panels, device, args.host_videos))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
