"""Train-step timing of Baseline3DPose(Rot): HIP path (K16 dense layers + K19 BatchNorm / ReLU / dropout) against the framework
path (nn.Linear + nn.BatchNorm1d + nn.ReLU + nn.Dropout), in the same process, alternating.

Each shape builds one LitPoseLiftingFlow + Trainer per path from the same weights and batch (loc_2d_3d, p_dropout 0.5), warms
both up (the trainer captures its graph at the first step and checks the replay), then times ROUNDS x STEPS train steps per path
with device events, the two paths taking turns round by round; the per-step figure is the median over rounds. The framework path
is selected here only (the inner model's ``_device_path`` is replaced on that instance); if its step cannot be captured it is
timed eagerly and says so.

  python tools/bench_baseline3d.py [--steps 20] [--rounds 5] [--warmup 3] [--shape model,B,linear_size] [--hip-only] [--out file.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule  # noqa: E402
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON  # noqa: E402
from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow  # noqa: E402
from pedestrians_video_2_carla_amd.modules.movements import baseline_3d_pose  # noqa: E402
from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything  # noqa: E402

SHAPES = [dict(model=m, B=B, T=16, linear_size=s, num_stage=2) for m in ('Baseline3DPose', 'Baseline3DPoseRot')
          for s in (1024, 256) for B in (256, 1024, 4096)]


def build(shape, framework):
    seed_everything(22742)
    dm = SyntheticCarlaRecordedDataModule(clip_length=shape['T'], batch_size=shape['B'], missing_joint_probabilities=0.1)
    model = getattr(baseline_3d_pose, shape['model'])(input_nodes=CARLA_SKELETON, linear_size=shape['linear_size'],
                                                       num_stage=shape['num_stage'], p_dropout=0.5)
    if framework:
        model.baseline._device_path = lambda x: False        # the nn modules on the device
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    return flow, dm


def make(shape, framework, d):
    for graph in (True, False):
        flow, dm = build(shape, framework)
        batch = dm.generate_batch(d)
        try:
            trainer = Trainer(device=d, use_graph=graph).setup(flow, dm)
            loss = trainer.train_step(flow, batch, 0)
            torch.cuda.synchronize(d)
            return dict(trainer=trainer, flow=flow, batch=batch, graph=bool(trainer.use_graph), first_loss=float(loss))
        except Exception as e:  # noqa: BLE001 -- the framework path may refuse capture: time it eagerly
            if not graph:
                raise
            print(f'[bench_baseline3d] {shape} framework={framework}: graph capture failed ({type(e).__name__}: {e}); eager steps',
                  file=sys.stderr, flush=True)
            torch.cuda.synchronize(d)


def timed(run, steps, d):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(steps):
        run['trainer'].train_step(run['flow'], run['batch'], i)
    end.record()
    torch.cuda.synchronize(d)
    return start.elapsed_time(end) / steps


def gemm_flop(shape):
    """fp32 GEMM FLOP of one train step: forward 2 N (I L + 2 S L^2 + L O); backward twice that minus the first layer's dX."""
    N, L, S = shape['B'] * shape['T'], shape['linear_size'], shape['num_stage']
    I, O = 52, 26 * (3 if shape['model'] == 'Baseline3DPose' else 9)
    fwd = 2 * N * (I * L + 2 * S * L * L + L * O)
    return fwd + 2 * fwd - 2 * N * I * L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shape', default=None, help='model,B,linear_size: one shape only (e.g. for a kernel-trace run)')
    ap.add_argument('--hip-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    d = torch.device('cuda:0')
    shapes = SHAPES
    if a.shape:
        m, B, s = a.shape.split(',')
        shapes = [dict(model=m, B=int(B), T=16, linear_size=int(s), num_stage=2)]
    out = open(a.out, 'w') if a.out else None
    for shape in shapes:
        runs = {'hip': make(shape, False, d)}
        if not a.hip_only:
            runs['framework'] = make(shape, True, d)
        for r in runs.values():
            timed(r, a.warmup, d)
        ms = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, r in runs.items():
                ms[k].append(timed(r, a.steps, d))
        rec = dict(shape, hip_ms=round(statistics.median(ms['hip']), 4), hip_graph=runs['hip']['graph'],
                   gemm_gflop=round(gemm_flop(shape) / 1e9, 2))
        if 'framework' in runs:
            rec.update(framework_ms=round(statistics.median(ms['framework']), 4), framework_graph=runs['framework']['graph'])
            rec['speedup'] = round(rec['framework_ms'] / rec['hip_ms'], 2)
        rec['rounds_ms'] = {k: [round(v, 4) for v in vs] for k, vs in ms.items()}
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()
        del runs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
