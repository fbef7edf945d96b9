"""K41 (ops.find_carla_loop, ops.loop_carla_rows) against its tensor definition on the device (P2C_LOOP_FRAMEWORK=1).

    python tools/bench_loop.py [N:T ...]        # default 1:81 64:81 1:1024 64:1024

bones (N,T,26,6) and root (N,T,6) of a seeded gait: per bone a base orientation times a swing about a fixed axis with a period of
24 to 40 frames and half a degree of jitter, a root that drifts. Both arms get the same device tensors. The search is asked for
the loop alone, as the writers ask (blend 8, periods 12 to 60); the player plays 30 seconds at 30 fps of the loop the kernel found.
The results are compared before timing: the period found and the largest cost difference (the start of a cycle is not well
posed: DESIGN K41), the played rows by the largest difference of a matrix entry (``carla_pose_import``) and of a location (row
angles are no measure: a pitch near 90 degrees magnifies them). Times are device events around windows of calls as an export loop
would issue them (launch gaps, the workspace allocation and the host's argument checks, which read the loop back, included: time
per call, not kernel time), the arms alternating window by window; a window is sized to about a quarter of a second from a first
timed pass. The median window of each arm is reported with its spread. One JSON line per (N, T).
"""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops

J, ROUNDS, WINDOW_US = 26, 7, 250e3
SHAPES = ((1, 81), (64, 81), (1, 1024), (64, 1024))
ARMS = (('kernel', '0'), ('framework', '1'))
ENV = 'P2C_LOOP_FRAMEWORK'
BLEND, MIN_PERIOD, MAX_PERIOD, FRAMES = 8, 12, 60, 900


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def armed(fn, env):
    def run():
        os.environ[ENV] = env
        return fn()
    return run


def alternate(fn):
    calls = {name: armed(fn, env) for name, env in ARMS}
    reps = {}
    for name, call in calls.items():                           # warm-up, and the window's size
        window(call, 1)
        reps[name] = max(1, min(2000, int(WINDOW_US / max(window(call, 3), 1.0))))
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call, reps[name]))
    os.environ[ENV] = '0'
    return {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2),
                   'calls_per_window': reps[name]} for name, v in times.items()}


def problem(N, T, device):
    g = torch.Generator().manual_seed(41)
    spread = torch.tensor([50.0, 180.0, 180.0], dtype=torch.float64)                 # the pitch stays off the poles
    base = (torch.rand(N, 1, J, 3, generator=g, dtype=torch.float64) * 2 - 1) * spread
    axis = torch.randn(N, 1, J, 3, generator=g, dtype=torch.float64)
    axis = 25.0 * axis / axis.norm(dim=-1, keepdim=True) * (0.3 + 0.7 * torch.rand(N, 1, J, 1, generator=g, dtype=torch.float64))
    period = 24.0 + 16.0 * torch.rand(N, 1, 1, 1, generator=g, dtype=torch.float64)
    t = torch.arange(T, dtype=torch.float64).reshape(1, T, 1, 1)
    swing = torch.sin(2 * math.pi * (t / period + torch.rand(N, 1, J, 1, generator=g, dtype=torch.float64)))
    bones = torch.zeros(N, T, J, 6, dtype=torch.float64)
    bones[..., :3] = torch.randn(N, 1, J, 3, generator=g, dtype=torch.float64)
    bones[..., 3:] = base + axis * swing + 0.5 * torch.randn(N, T, J, 3, generator=g, dtype=torch.float64)
    root = torch.zeros(N, T, 6, dtype=torch.float64)
    root[..., :3] = torch.randn(N, 1, 3, generator=g, dtype=torch.float64) + t[..., 0] * torch.tensor([0.05, 0.01, 0.0], dtype=torch.float64)
    root[..., 4] = (torch.rand(N, 1, generator=g, dtype=torch.float64) * 2 - 1) * 180.0
    return bones.float().to(device), root.float().to(device)


def matrix_difference(a, b):
    as4 = lambda r: r if r.ndim == 4 else r.unsqueeze(-2)      # noqa: E731
    return float((ops.carla_pose_import(as4(a))[1] - ops.carla_pose_import(as4(b))[1]).abs().max())


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_loop.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    shapes = [tuple(int(v) for v in a.split(':')) for a in sys.argv[1:]] or SHAPES
    for N, T in shapes:
        bones, root = problem(N, T, device)
        find = lambda want=('loop',): ops.find_carla_loop(bones, blend=BLEND, min_period=MIN_PERIOD, max_period=MAX_PERIOD, want=want)   # noqa: E731
        got = {name: armed(lambda: find(('loop', 'cost')), env)() for name, env in ARMS}
        os.environ[ENV] = '0'
        k, f = got['kernel'], got['framework']
        finite = torch.isfinite(f['cost'])
        loop = k['loop']
        play = lambda: ops.loop_carla_rows(bones, root, loop=loop, blend=BLEND, frames=FRAMES)   # noqa: E731
        rows = {name: armed(play, env)() for name, env in ARMS}
        os.environ[ENV] = '0'
        res = {'N': N, 'T': T, 'J': J, 'blend': BLEND, 'frames_played': FRAMES,
               'same_inf_pattern': bool(torch.equal(torch.isfinite(k['cost']), finite)),
               'largest_cost_difference': float((k['cost'][finite] - f['cost'][finite]).abs().max()),
               'videos_with_the_same_period': int((k['loop'][:, 1] - k['loop'][:, 0] == f['loop'][:, 1] - f['loop'][:, 0]).sum()),
               'videos_with_the_same_pair': int((k['loop'] == f['loop']).all(1).sum()),
               'largest_played_matrix_entry_difference': max(matrix_difference(a, b) for a, b in zip(rows['kernel'], rows['framework'])),
               'largest_played_location_difference': float(max((a[..., :3] - b[..., :3]).abs().max()
                                                               for a, b in zip(rows['kernel'], rows['framework']))),
               'intermediate_bytes_of_the_tensor_form': N * T * T * J * 4,
               'find': alternate(find), 'play': alternate(play)}
        for what in ('find', 'play'):
            res[what]['framework_over_kernel'] = round(res[what]['framework']['us_per_call'] / res[what]['kernel']['us_per_call'], 1)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
