"""The ranking behind AUROC / ROCCurve / PRCurve of one evaluation epoch: K25 (csrc/p2c_rank.hip through ``ops.rank_curves``)
against the tensor restatement (``P2C_RANK_FRAMEWORK=1``: torch.sort, cumsum, differences), in the same process, alternating.

One call ranks resident device scores (N, C) and ends with the host sync that brings the curve sizes back, on both arms, so a call
is timed on the host clock between two device synchronisations. Both arms are warmed up, then timed for ROUNDS windows of STEPS
calls each, taking turns window by window; the figure is the median window. N <= 16384 is K25's one-launch LDS regime, larger N
its radix sort. Prints one JSON line.

  python tools/bench_rank_metrics.py [--steps 20] [--rounds 5] [--warmup 3] [--out f.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pedestrians_video_2_carla_amd import ops  # noqa: E402

SHAPES = [(N, C) for N in (2048, 16384, 131072) for C in (1, 2, 5)]


def timed(scores, targets, framework, steps, d):
    os.environ['P2C_RANK_FRAMEWORK'] = '1' if framework else '0'
    torch.cuda.synchronize(d)
    t0 = time.perf_counter()
    for _ in range(steps):
        out = ops.rank_curves(scores, targets)
    torch.cuda.synchronize(d)
    return (time.perf_counter() - t0) / steps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_rank_metrics.py times GPU paths: no GPU here, nothing measured')
    d = torch.device('cuda:0')
    gen = torch.Generator(device=d).manual_seed(22742)
    rows = []
    for N, C in SHAPES:
        logits = torch.randn(N, C, device=d, generator=gen)
        scores = torch.sigmoid(logits) if C == 1 else torch.softmax(logits, dim=-1)
        targets = torch.randint(0, 2 if C == 1 else C, (N,), device=d, generator=gen).to(torch.int32)
        outs = {}
        for fw in (False, True):
            _, outs[fw] = timed(scores, targets, fw, a.warmup, d)
        agree = (outs[False]['n_points'] == outs[True]['n_points'] and torch.equal(outs[False]['auroc'], outs[True]['auroc'])
                 and all(torch.equal(x, y) for k in ('thresholds', 'tps', 'fps') for x, y in zip(outs[False][k], outs[True][k])))
        ms = {False: [], True: []}
        for _ in range(a.rounds):
            for fw in (False, True):
                ms[fw].append(timed(scores, targets, fw, a.steps, d)[0])
        hip, fw = 1e6 * statistics.median(ms[False]), 1e6 * statistics.median(ms[True])
        rows.append(dict(N=N, C=C, regime='lds' if N <= 16384 else 'global', hip_us=round(hip, 1), framework_us=round(fw, 1),
                         speedup=round(fw / hip, 2), same_output=bool(agree),
                         hip_rounds_us=[round(1e6 * v, 1) for v in ms[False]], framework_rounds_us=[round(1e6 * v, 1) for v in ms[True]]))
    os.environ['P2C_RANK_FRAMEWORK'] = '0'
    line = json.dumps(dict(steps=a.steps, rounds=a.rounds, warmup=a.warmup, shapes=rows))
    print(line, flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
