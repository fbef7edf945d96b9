"""K32 (ops.lift_to_carla: keypoint clips -> CARLA rows in one launch) against the composed path it replaces
(P2C_LIFT_FRAMEWORK=1: ops.fused_mlp -> the materialising pose head -> ops.carla_pose_export).

    python tools/bench_lift.py [B ...]      # clips per batch, default 1 16 256 4096

T = 16, the pose_changes kind, a trained-size LinearAE (52-26-13-6-39-78-156) with its packed weight image current in both arms
(no pack launch in either), world transforms given, ``final_rel_rot`` produced: what ``CarlaLifter.push`` issues per clip. Both
arms get the same device tensors and their results are compared bit for bit before timing. Times are device events around
windows of calls as a player loop would issue them (launch gaps and the host's share included: time per call, not kernel time),
the two arms alternating window by window; the median window of each arm is reported with its spread. One JSON line per B.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.transforms.rotation_conversions import rotation_6d_to_matrix

T, ROUNDS = 16, 9
ARMS = (('k32', '0'), ('composed', '1'))


def reps_for(B):
    """Windows of about a tenth of a second or more in the slower arm."""
    return 3000 if B <= 64 else (1500 if B <= 1024 else 300)


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def alternate(fn, reps):
    def armed(env):
        def run():
            os.environ['P2C_LIFT_FRAMEWORK'] = env
            fn()
        return run
    calls = {name: armed(env) for name, env in ARMS}
    for call in calls.values():                                # warm-up of every shape the windows use
        window(call, max(reps // 10, 20))
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call, reps))
    os.environ['P2C_LIFT_FRAMEWORK'] = '0'
    return {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}
            for name, v in times.items()}


def problem(B, device):
    g = torch.Generator().manual_seed(7)
    dims = ops.LINEAR_AE_6D_DIMS
    weights = [(torch.randn(o, i, generator=g) / i ** 0.5).to(device) for i, o in zip(dims[:-1], dims[1:])]
    biases = [(0.1 * torch.randn(o, generator=g)).to(device) for o in dims[1:]]
    frames = torch.randn(B, T, 26, 2, generator=g).to(device)
    skel_type = (torch.arange(B, dtype=torch.int32) % 4).to(device)
    world_loc = torch.randn(B, T, 3, generator=g).to(device)
    world_rot = rotation_6d_to_matrix(torch.randn(B, T, 6, generator=g)).to(device)
    image = torch.empty(ops.mlp_image_layout(dims)[0], device=device)
    ops.mlp_pack(weights, biases, image)
    return frames, weights, biases, skel_type, world_loc, world_rot, image


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_lift.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    for B in [int(a) for a in sys.argv[1:]] or [1, 16, 256, 4096]:
        frames, weights, biases, skel_type, world_loc, world_rot, image = problem(B, device)
        lift = lambda: ops.lift_to_carla(frames, weights, biases, skel_type, 'pose_changes_6d', image=image,     # noqa: E731
                                         image_is_current=True, world_loc=world_loc, world_rot=world_rot)
        out = {}
        for name, env in ARMS:
            os.environ['P2C_LIFT_FRAMEWORK'] = env
            out[name] = lift()
        os.environ['P2C_LIFT_FRAMEWORK'] = '0'
        same = all(torch.equal(a, b) for a, b in zip(out['k32'][:3], out['composed'][:3]))
        res = {'B': B, 'T': T, 'same_bits': same, 'reps_per_window': reps_for(B), 'windows_per_arm': ROUNDS}
        res.update(alternate(lift, reps_for(B)))
        res['k32_over_composed'] = round(res['k32']['us_per_call'] / res['composed']['us_per_call'], 3)
        print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
