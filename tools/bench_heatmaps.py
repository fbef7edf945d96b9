"""K28 (ops.heatmap_targets / heatmaps_loss / heatmap_keypoints) against the tensor restatements on the device
(P2C_HEATMAPS_FRAMEWORK=1).

    python tools/bench_heatmaps.py [B ...]      # clips per batch, default 8

Per batch size, T = 16, CARLA's 26 joints + background, 368 x 368 crops pooled 9/8/1 to 46 x 46:
  targets    ops.heatmap_targets from the keypoints (sigma = 1); the tensor arm forms the full-resolution maps and pools them
  loss       ops.heatmaps_loss forward + backward on (B, T, 27, 46, 46) maps, mask on, the hips pair forced
  keypoints  ops.heatmap_keypoints of the same maps
Both arms get the same device tensors and their results are compared before timing. Times are device events around windows of
``REPS`` calls as a training loop would issue them (launch gaps included: time per call, not kernel time), the two arms
alternating window by window; the median window of each arm is reported with its spread. One JSON line.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops

T, J, SIZE, SIGMA, REPS, ROUNDS = 16, 26, (368, 368), 1, 10, 9
ARMS = (('k28', '0'), ('framework', '1'))


def window(fn, reps=REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def alternate(fn):
    """-> arm -> {us_per_call, min, max} for ``fn`` under either setting of the switch, windows alternating."""
    def armed(env):
        def run():
            os.environ['P2C_HEATMAPS_FRAMEWORK'] = env
            return fn()
        return run
    calls = {name: armed(env) for name, env in ARMS}
    for call in calls.values():                                # warm-up of every shape the windows use
        window(call, 2)
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call))
    res = {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}
           for name, v in times.items()}
    res['ratio'] = round(res['framework']['us_per_call'] / res['k28']['us_per_call'], 2)
    os.environ['P2C_HEATMAPS_FRAMEWORK'] = '0'
    return res


def both(fn):
    got = {}
    for name, env in ARMS:
        os.environ['P2C_HEATMAPS_FRAMEWORK'] = env
        got[name] = fn()
    os.environ['P2C_HEATMAPS_FRAMEWORK'] = '0'
    return got['k28'], got['framework']


def case(B, device):
    g = torch.Generator().manual_seed(5)
    kp = (torch.rand(B, T, J, 2, generator=g) * 1.2 - 0.1) * torch.tensor([float(SIZE[1]), float(SIZE[0])])
    kp, shift = kp.to(device), torch.zeros(B, T, 2, device=device)

    def targets():
        return ops.heatmap_targets(kp, shift, (1.0, 1.0), SIZE, SIGMA, ops.HEATMAPS_POOL)
    a, b = both(targets)
    out = {'B': B, 'targets': {**alternate(targets), 'max_abs_diff': float((a - b).abs().max())}}

    gt = a.clone()
    gt[:, :, 1::2] += 0.01                                     # every other joint's map has no exact zero: selected under the mask
    pred = torch.randn(a.shape, generator=g).to(device).requires_grad_(True)
    channels = list(range(J + 1))

    def loss():
        pred.grad = None
        value = ops.heatmaps_loss(pred, gt, channels, channels, 1, True)
        value.backward()
        return value.detach().double(), pred.grad.double().clone()
    (la, ga), (lb, gb) = both(loss)
    out['loss'] = {**alternate(loss), 'loss_rel_diff': float((la - lb).abs() / lb.abs()),
                   'grad_rel_diff': float((ga - gb).abs().max() / gb.abs().max())}

    maps = pred.detach()

    def keypoints():
        return ops.heatmap_keypoints(maps, SIZE)
    a, b = both(keypoints)
    out['keypoints'] = {**alternate(keypoints), 'max_abs_diff': float((a - b).abs().max())}
    return out


def main():
    device = torch.device('cuda:0')
    out = {'tool': 'bench_heatmaps', 'T': T, 'J': J, 'size': SIZE, 'sigma': SIGMA, 'reps_per_window': REPS, 'windows': ROUNDS,
           'timing': 'device events around windows of calls (launch gaps included)', 'cases': []}
    for B in [int(a) for a in sys.argv[1:]] or [8]:
        out['cases'].append(case(B, device))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
