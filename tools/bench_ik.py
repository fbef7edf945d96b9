"""K36 (ops.locations_to_carla: one launch) against its tensor definition on the device (P2C_IK_FRAMEWORK=1).

    python tools/bench_ik.py [B ...]      # clips per batch, default 1, 256 and 4096

T = 16: loc (B,T,26,3), skel_type (B) -> the three pose tensors (2.8 KB per frame), and, as a second case, bones + root alone
(648 B per frame) with a world per frame. Both arms get the same device tensors and their results are compared before timing.
Times are device events around windows of calls as a predict loop would issue them (launch gaps included: time per call, not
kernel time), the two arms alternating window by window; a window holds as many calls as fill 0.3 s (3 to 200, from a pilot
window per arm and case); the median window of each arm is reported with its spread, and the bytes a call has to move. One
JSON line per B.
"""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.data.carla import reference as ref
from pedestrians_video_2_carla_amd.data.carla.skeleton import PARENTS
from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix

T, ROUNDS, WINDOW_US = 16, 7, 3e5
ARMS = (('k36', '0'), ('framework', '1'))
POSES = ('relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot')
ROWS = ('bones', 'root')


def window(fn, reps):
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
            os.environ['P2C_IK_FRAMEWORK'] = env
            fn()
        return run
    calls = {name: armed(env) for name, env in ARMS}
    reps = {}
    for name, call in calls.items():                           # warm-up of every shape the windows use, and the pilot
        window(call, 3)
        reps[name] = max(3, min(200, math.ceil(WINDOW_US / window(call, 3))))
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call, reps[name]))
    os.environ['P2C_IK_FRAMEWORK'] = '0'
    return {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2),
                   'calls_per_window': reps[name]} for name, v in times.items()}


def results(fn):
    out = {}
    for name, env in ARMS:
        os.environ['P2C_IK_FRAMEWORK'] = env
        out[name] = {k: v.double().cpu() for k, v in fn().items()}
    os.environ['P2C_IK_FRAMEWORK'] = '0'
    return out


def poses(B, g):
    """(B,T,26,3) locations: the forward kinematics of random rotations (angles ~ N(0, 0.6^2)) on top of the reference pose."""
    skel_type = torch.randint(0, 4, (B,), generator=g)
    rel_loc, rel_rot = (t[skel_type][:, None].expand(B, T, *t.shape[1:]) for t in ref.get_relative_tensors(dtype=torch.float64))
    w = torch.randn(B, T, 26, 3, generator=g, dtype=torch.float64) * 0.6
    rot = euler_angles_to_matrix(w, 'XYZ') @ rel_rot
    loc, abs_rot = [None] * 26, [None] * 26
    for j, p in enumerate(PARENTS):
        if p < 0:
            loc[j], abs_rot[j] = rel_loc[..., j, :], rot[..., j, :, :]
        else:
            loc[j] = (rel_loc[..., j, None, :] @ abs_rot[p])[..., 0, :] + loc[p]
            abs_rot[j] = rot[..., j, :, :] @ abs_rot[p]
    return torch.stack(loc, -2).float(), skel_type.to(torch.int32)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_ik.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    for B in [int(a) for a in sys.argv[1:]] or [1, 256, 4096]:
        g = torch.Generator().manual_seed(36)
        loc, skel_type = (t.to(device) for t in poses(B, g))
        world_loc = torch.randn(B, T, 3, generator=g).to(device)
        world_rot = euler_angles_to_matrix((torch.rand(B, T, 3, generator=g) * 2 - 1) * 1.2, 'XYZ').to(device)
        pose_call = lambda: ops.locations_to_carla(loc, skel_type, want=POSES)                              # noqa: E731
        row_call = lambda: ops.locations_to_carla(loc, skel_type, world_loc, world_rot, want=ROWS)         # noqa: E731
        rp, rr = results(pose_call), results(row_call)
        wrap = lambda d: (d + 180.0) % 360.0 - 180.0                                                       # noqa: E731
        agree = {'poses': max(float((rp['k36'][k] - rp['framework'][k]).abs().max()) for k in POSES),
                 'rows_angles_deg': max(float(wrap(rr['k36'][k][..., 3:] - rr['framework'][k][..., 3:]).abs().max()) for k in ROWS),
                 'rows_locations': max(float((rr['k36'][k][..., :3] - rr['framework'][k][..., :3]).abs().max()) for k in ROWS)}
        n = B * T
        res = {'B': B, 'T': T, 'frames': n, 'arms_differ_by': agree,
               'poses': alternate(pose_call), 'poses_bytes': n * (312 + 26 * 84),
               'rows': alternate(row_call), 'rows_bytes': n * (312 + 48 + 26 * 24 + 24)}
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
