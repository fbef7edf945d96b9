"""Train-step timing of the LSTM movements model: HIP path (dense kernels + K7b / K18 recurrences) against the framework RNN
path (nn.Linear + nn.LSTM, i.e. MIOpen), in the same process, alternating.

Each shape builds one flow + Trainer per path from the same weights and batch, warms both up (the trainer captures its graph
at the first step and checks the replay), then times ROUNDS x STEPS train steps per path with device events, the two paths
taking turns round by round; the per-step figure is the median over rounds. The framework path is selected here only (the
model's ``_hip_path`` is replaced on that instance); if its step cannot be captured it is timed eagerly and says so.

  python tools/bench_lstm_model.py [--steps 20] [--rounds 5] [--warmup 3] [--only pose|ae] [--shape T,H,L] [--out file.jsonl]
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
from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow  # noqa: E402
from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT  # noqa: E402
from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow  # noqa: E402
from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM  # noqa: E402
from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything  # noqa: E402

POSE = [dict(flow='pose_lifting', B=256, T=16, H=64, L=2)]
AE = [dict(flow='autoencoder', B=256, T=T, H=H, L=L) for T in (4, 15) for H in (100, 191, 256, 512) for L in (1, 2, 4)]


def build(shape, framework):
    seed_everything(22742)
    dm = SyntheticCarlaRecordedDataModule(clip_length=shape['T'], batch_size=shape['B'], missing_joint_probabilities=0.1)
    if shape['flow'] == 'pose_lifting':
        model = LSTM(input_nodes=CARLA_SKELETON, hidden_size=shape['H'], num_layers=shape['L'])
        flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    else:
        model = LSTM(input_nodes=CARLA_SKELETON, hidden_size=shape['H'], num_layers=shape['L'], movements_output_type=MT.pose_2d)
        flow = LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox')
    if framework:
        model._hip_path = lambda x: False          # nn.Linear + nn.LSTM on the device
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
        except Exception as e:  # noqa: BLE001 -- the framework RNN may refuse capture: time it eagerly
            if not graph:
                raise
            print(f'[bench_lstm_model] {shape} framework={framework}: graph capture failed ({type(e).__name__}: {e}); eager steps',
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=['pose', 'ae'], default=None)
    ap.add_argument('--shape', default=None, help='T,H,L: one autoencoder shape only (e.g. for a kernel-trace run)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    d = torch.device('cuda:0')
    shapes = (POSE if a.only != 'ae' else []) + (AE if a.only != 'pose' else [])
    if a.shape:
        T, H, L = (int(v) for v in a.shape.split(','))
        shapes = [dict(flow='autoencoder', B=256, T=T, H=H, L=L)]
    out = open(a.out, 'w') if a.out else None
    for shape in shapes:
        runs = {'hip': make(shape, False, d), 'framework': make(shape, True, d)}
        for r in runs.values():
            timed(r, a.warmup, d)
        ms = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, r in runs.items():
                ms[k].append(timed(r, a.steps, d))
        rec = dict(shape, hip_ms=round(statistics.median(ms['hip']), 4), framework_ms=round(statistics.median(ms['framework']), 4),
                   hip_graph=runs['hip']['graph'], framework_graph=runs['framework']['graph'],
                   rounds_ms={k: [round(v, 4) for v in vs] for k, vs in ms.items()})
        rec['speedup'] = round(rec['framework_ms'] / rec['hip_ms'], 2)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()
        del runs
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
