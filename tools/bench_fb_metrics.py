"""The five FB_* validation metrics of one batch: K22 (csrc/p2c_eval_fb.hip, one launch for all five through FBMetricSet) against
the tensor restatement in metrics/extra_metrics.py (``P2C_FB_FRAMEWORK=1``), in the same process, alternating.

One "batch" is what ``flow._update_metrics`` does with the FB metrics of a validation batch: ``update`` on each of the five members
of one set, on resident GPU tensors of the headline shape (B = 256, T = 16, J = 26). Both paths are warmed up, then timed for ROUNDS
windows of STEPS batches each with device events, taking turns window by window; the figure is the median window. Launch counts
come last, from capturing one batch of each path into a HIP graph and counting its kernel nodes; a path that cannot be captured
(the tensor path's library SVD checks its status on the host) reports null.

  python tools/bench_fb_metrics.py [--steps 200] [--rounds 5] [--warmup 10] [--shape B,T,J] [--out f.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pedestrians_video_2_carla_amd.metrics import (FB_MPJPE, FB_MPJVE, FB_N_MPJPE, FB_PA_MPJPE, FB_WeightedMPJPE,  # noqa: E402
                                                   FBMetricSet)
from pedestrians_video_2_carla_amd.trainer import Trainer  # noqa: E402

KEY = 'absolute_pose_loc'


def make_path(framework, pred, gt):
    fb = FBMetricSet()
    members = [FB_MPJPE(fb), FB_WeightedMPJPE(None, fb), FB_PA_MPJPE(fb), FB_N_MPJPE(fb), FB_MPJVE(fb)]   # the flow's order
    preds, targets = {KEY: pred}, {KEY: gt}

    def batch():
        os.environ['P2C_FB_FRAMEWORK'] = '1' if framework else '0'
        for m in members:
            m.update(preds, targets)
    return dict(batch=batch, set=fb, members=members)


def timed(run, steps, d):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        run['batch']()
    end.record()
    torch.cuda.synchronize(d)
    return start.elapsed_time(end) / steps


def count_launches(run, d):
    """Kernel nodes of one captured batch, or None where the path does not capture."""
    try:
        g = torch.cuda.CUDAGraph(keep_graph=True)
    except TypeError:
        return None
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    try:
        with torch.cuda.graph(g, stream=side):
            run['batch']()
        nodes = Trainer._count_nodes(g)
    except Exception:                           # noqa: BLE001 -- a host-synchronising op inside the path
        nodes = None
    torch.cuda.synchronize(d)
    return nodes[1] if nodes else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--shape', default='256,16,26', help='B,T,J of the validation batch')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_fb_metrics.py times GPU paths: no GPU here, nothing measured')
    d = torch.device('cuda:0')
    B, T, J = (int(v) for v in a.shape.split(','))
    gen = torch.Generator(device=d).manual_seed(22742)
    gt = 0.4 * torch.randn(B, T, J, 3, device=d, generator=gen) + torch.tensor([0.0, 1.0, 0.0], device=d)
    pred = gt + 0.05 * torch.randn(B, T, J, 3, device=d, generator=gen)
    runs = {'hip': make_path(False, pred, gt), 'framework': make_path(True, pred, gt)}
    for r in runs.values():
        timed(r, a.warmup, d)
    ms = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, r in runs.items():
            ms[k].append(timed(r, a.steps, d))
    rec = dict(B=B, T=T, J=J, steps=a.steps, rounds=a.rounds,
               hip_us=round(1e3 * statistics.median(ms['hip']), 2), framework_us=round(1e3 * statistics.median(ms['framework']), 2))
    rec['speedup'] = round(rec['framework_us'] / rec['hip_us'], 2)
    rec['hip_entry_calls_per_batch'] = runs['hip']['set'].launches / (a.warmup + a.rounds * a.steps)
    rec['framework_entry_calls'] = runs['framework']['set'].launches
    rec['values_mm'] = {k: [round(float(m.compute()), 4) for m in r['members']] for k, r in runs.items()}
    rec['rounds_us'] = {k: [round(1e3 * v, 2) for v in vs] for k, vs in ms.items()}
    print(json.dumps(rec), flush=True)                     # the times are out before anything is captured
    rec['hip_launches'] = count_launches(runs['hip'], d)
    rec['framework_launches'] = count_launches(runs['framework'], d)
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
