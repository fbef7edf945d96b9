"""K30 (ops.carla_pose_export / carla_pose_import: one launch each) against their tensor definitions on the device
(P2C_CARLA_FRAMEWORK=1).

    python tools/bench_carla_pose.py [B ...]      # clips per batch, default 256

T = 16, J = 26: rel_loc (B,T,J,3), rel_rot (B,T,J,3,3), world_loc (B,T,3), world_rot (B,T,3,3) -> bones (B,T,J,6), root (B,T,6),
and the inverse on the bones. Both arms get the same device tensors, and their results are compared before timing (angles as
rotations, modulo 360 degrees). Times are device events around windows of ``REPS`` calls as a predict loop would issue them
(launch gaps included: time per call, not kernel time), the two arms alternating window by window; the median window of each
arm is reported with its spread, and the bytes each call has to move (48 in, 24 out per element). One JSON line per B.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix

T, J, REPS, ROUNDS = 16, 26, 2000, 9
ARMS = (('k30', '0'), ('framework', '1'))


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
            os.environ['P2C_CARLA_FRAMEWORK'] = env
            fn()
        return run
    calls = {name: armed(env) for name, env in ARMS}
    for call in calls.values():                                # warm-up of every shape the windows use
        window(call)
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call))
    os.environ['P2C_CARLA_FRAMEWORK'] = '0'
    return {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}
            for name, v in times.items()}


def results(fn):
    out = {}
    for name, env in ARMS:
        os.environ['P2C_CARLA_FRAMEWORK'] = env
        out[name] = [t.double().cpu() for t in fn()]
    os.environ['P2C_CARLA_FRAMEWORK'] = '0'
    return out


def problem(B, device):
    g = torch.Generator().manual_seed(5)
    n = B * T * J + B * T
    angles = (torch.rand(n, 3, generator=g, dtype=torch.float64) * 2 - 1) * torch.tensor([3.14, 1.4, 3.14], dtype=torch.float64)
    rot = euler_angles_to_matrix(angles, 'XYZ').float()
    loc = torch.randn(n, 3, generator=g)
    k = B * T * J
    return (loc[:k].reshape(B, T, J, 3).to(device), rot[:k].reshape(B, T, J, 3, 3).to(device),
            loc[k:].reshape(B, T, 3).to(device), rot[k:].reshape(B, T, 3, 3).to(device))


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_carla_pose.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    for B in [int(a) for a in sys.argv[1:]] or [256]:
        loc, rot, wloc, wrot = problem(B, device)
        bones, _ = ops.carla_pose_export(loc, rot, wloc, wrot)
        export = lambda: ops.carla_pose_export(loc, rot, wloc, wrot)          # noqa: E731
        inverse = lambda: ops.carla_pose_import(bones)                        # noqa: E731
        ex, iv = results(export), results(inverse)
        wrap = lambda d: (d + 180.0) % 360.0 - 180.0                          # noqa: E731
        agree = {'export_angles_deg': max(float(wrap(a[..., 3:] - b[..., 3:]).abs().max()) for a, b in zip(ex['k30'], ex['framework'])),
                 'export_locations': max(float((a[..., :3] - b[..., :3]).abs().max()) for a, b in zip(ex['k30'], ex['framework'])),
                 'import': max(float((a - b).abs().max()) for a, b in zip(iv['k30'], iv['framework']))}
        elements = B * T * J + B * T
        res = {'B': B, 'T': T, 'J': J, 'arms_differ_by': agree,
               'export': alternate(export), 'export_bytes': elements * 72,
               'import': alternate(inverse), 'import_bytes': B * T * J * 72}
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
