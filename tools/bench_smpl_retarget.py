"""K35 (ops.smpl_to_carla: one launch) against its tensor definition on the device (P2C_SMPL_FRAMEWORK=1).

    python tools/bench_smpl_retarget.py [B ...]      # clips per batch, default 256 and 4096

T = 16: body_pose (B,T,66), skel_type (B) -> the three pose tensors (2.8 KB per frame), and, as a second case, bones + root
alone (648 B per frame) with a world rotation per frame. Both arms get the same device tensors and their results are compared
before timing. Times are device events around windows of ``REPS`` calls as a data loop would issue them (launch gaps included:
time per call, not kernel time), the two arms alternating window by window; the median window of each arm is reported with its
spread, and the bytes a call has to move. One JSON line per B.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix

T, REPS, ROUNDS = 16, 200, 7
ARMS = (('k35', '0'), ('framework', '1'))
POSES = ('relative_pose_rot', 'absolute_pose_loc', 'absolute_pose_rot')
ROWS = ('bones', 'root')


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
            os.environ['P2C_SMPL_FRAMEWORK'] = env
            fn()
        return run
    calls = {name: armed(env) for name, env in ARMS}
    for call in calls.values():                                # warm-up of every shape the windows use
        window(call, 20)
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call))
    os.environ['P2C_SMPL_FRAMEWORK'] = '0'
    return {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}
            for name, v in times.items()}


def results(fn):
    out = {}
    for name, env in ARMS:
        os.environ['P2C_SMPL_FRAMEWORK'] = env
        out[name] = {k: v.double().cpu() for k, v in fn().items()}
    os.environ['P2C_SMPL_FRAMEWORK'] = '0'
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_smpl_retarget.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    for B in [int(a) for a in sys.argv[1:]] or [256, 4096]:
        g = torch.Generator().manual_seed(35)
        body = ((torch.rand(B, T, 66, generator=g) * 2 - 1) * 1.5).to(device)
        skel_type = torch.randint(0, 4, (B,), generator=g).to(torch.int32).to(device)
        world_loc = torch.zeros(B, T, 3, device=device)
        world_rot = euler_angles_to_matrix((torch.rand(B, T, 3, generator=g) * 2 - 1) * 1.2, 'XYZ').to(device)
        poses = lambda: ops.smpl_to_carla(body, skel_type, want=POSES)                            # noqa: E731
        rows = lambda: ops.smpl_to_carla(body, skel_type, world_loc, world_rot, want=ROWS)        # noqa: E731
        rp, rr = results(poses), results(rows)
        wrap = lambda d: (d + 180.0) % 360.0 - 180.0                                              # noqa: E731
        agree = {'poses': max(float((rp['k35'][k] - rp['framework'][k]).abs().max()) for k in POSES),
                 'rows_angles_deg': max(float(wrap(rr['k35'][k][..., 3:] - rr['framework'][k][..., 3:]).abs().max()) for k in ROWS),
                 'rows_locations': max(float((rr['k35'][k][..., :3] - rr['framework'][k][..., :3]).abs().max()) for k in ROWS)}
        n = B * T
        res = {'B': B, 'T': T, 'frames': n, 'arms_differ_by': agree,
               'poses': alternate(poses), 'poses_bytes': n * (264 + 26 * 84),
               'rows': alternate(rows), 'rows_bytes': n * (264 + 48 + 26 * 24 + 24)}
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
