"""K40 (ops.root_motion_carla_rows) with each mapping forced, against its tensor definition on the device
(P2C_ROOT_MOTION_FRAMEWORK=1).

    python tools/bench_root_motion.py [N:T ...]        # default 256:16 4096:16 16:1024 1:16384

bones (N,T,26,6) and root (N,T,6) of a seeded walk on the reference pose (thighs and knees swing, a little noise on every angle,
a root within +-100 with a random yaw). All arms get the same device tensors and ask for the root rows alone, as the writers do;
their results are compared before timing: the two mappings bit for bit, the definition by the steps (at most one quantum apart
where the stance choice agrees) and the share of frames whose contact differs. Times are device events around windows of calls as
an export loop would issue them (launch gaps, the workspace allocation and the host's argument checks included: time per call,
not kernel time), the arms alternating window by window; a window is sized to about a quarter of a second from a first timed pass.
The median window of each arm is reported with its spread, the bytes a call has to read (24 per bone and root row, once) and
write (24 per root row) with the rate the faster mapping's median makes of their sum, and which mapping ``mapping=None`` takes.
One JSON line per (N, T).
"""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla import reference

J, ROUNDS, WINDOW_US = 26, 7, 250e3
SHAPES = ((256, 16), (4096, 16), (16, 1024), (1, 16384))
ARMS = (('per_video', '0', 1), ('frame_parallel', '0', 2), ('framework', '1', None))
ENV = 'P2C_ROOT_MOTION_FRAMEWORK'
ALL = ('root', 'steps', 'contact')


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def armed(fn, env, mapping):
    def run(**kw):
        os.environ[ENV] = env
        return fn(mapping=mapping, **kw)
    return run


def alternate(fn):
    calls = {name: armed(fn, env, mapping) for name, env, mapping in ARMS}
    reps = {}
    for name, call in calls.items():                           # warm-up of every shape the windows use, and the window's size
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
    g = torch.Generator().manual_seed(7)
    loc, rot = reference.get_relative_tensors(dtype=torch.float64)
    rows = ops.carla_pose_export(loc, rot)[0]
    bones = rows[torch.randint(0, 4, (N,), generator=g)].unsqueeze(1).repeat(1, T, 1, 1)
    period = 16.0 + 24.0 * torch.rand(N, 1, generator=g, dtype=torch.float64)
    phase = 2 * math.pi * (torch.arange(T, dtype=torch.float64).unsqueeze(0) / period + torch.rand(N, 1, generator=g, dtype=torch.float64))
    for thigh, leg, off in ((16, 17, 0.0), (21, 22, math.pi)):     # the fore-and-aft angle of these rows is the third one
        bones[:, :, thigh, 5] += 25.0 * torch.sin(phase + off)
        bones[:, :, leg, 5] -= 30.0 * (1.0 - torch.cos(phase + off)) / 2
    bones[..., 3:] += 0.2 * torch.randn(N, T, J, 3, generator=g, dtype=torch.float64)
    root = torch.zeros(N, T, 6, dtype=torch.float64)
    root[..., :3] = (torch.rand(N, 1, 3, generator=g, dtype=torch.float64) * 2 - 1) * 100.0
    root[..., 4] = (torch.rand(N, 1, generator=g, dtype=torch.float64) * 2 - 1) * 180.0
    return bones.float().to(device), root.float().to(device)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_root_motion.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    shapes = [tuple(int(v) for v in a.split(':')) for a in sys.argv[1:]] or SHAPES
    for N, T in shapes:
        bones, root = problem(N, T, device)
        call = lambda mapping=None, want=('root',): ops.root_motion_carla_rows(bones, root, want=want, mapping=mapping)   # noqa: E731
        got = {name: armed(call, env, mapping)(want=ALL) for name, env, mapping in ARMS}
        os.environ[ENV] = '0'
        a, b, f = got['per_video'], got['frame_parallel'], got['framework']
        agree = a['contact'] == f['contact']
        res = {'N': N, 'T': T, 'frames': N * T,
               'mappings_same_bits': all(torch.equal(a[k], b[k]) for k in ALL) and all(torch.equal(x, y) for x, y in zip(a['state'], b['state'])),
               'contact_differs_from_framework': round(float((~agree).double().mean()), 5),
               'largest_step_difference_where_contact_agrees': int((a['steps'].long() - f['steps'].long()).abs()[agree].max()),
               'auto_takes': 'per_video' if _lib.lib().p2c_carla_root_motion_workspace(N, T, 0) == 0 else 'frame_parallel'}
        moved = N * T * ((J + 1) * 24 + 24)
        res.update(bytes_read_once_and_written=moved, **alternate(call))
        best = min(res['per_video']['us_per_call'], res['frame_parallel']['us_per_call'])
        res['faster_mapping'] = 'per_video' if best == res['per_video']['us_per_call'] else 'frame_parallel'
        res['faster_mapping_GB_per_s'] = round(moved / best / 1e3, 1)
        res['framework_over_faster_mapping'] = round(res['framework']['us_per_call'] / best, 1)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
