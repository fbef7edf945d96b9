"""Autoencoder train-step timing of Seq2SeqFlatEmbeddings, LinearAE2D and Linear: HIP path (K21 front end / K16 composition /
K16 dense) against the same model with those layers as framework ops (``hip_path = False`` on that instance: nn.Linear, ReLU,
permute and flip kernels), in the same process, alternating. The sweep's shape: B = 256, T = 15
(configs/sweep/carla-recorded_seq2seq-flat-embeddings.yaml of the reference).

Each model builds one flow + Trainer per path from the same weights and batch, warms both up (the trainer captures its graph at
the first step and checks the replay), then times ROUNDS x STEPS train steps per path with device events, the two paths taking
turns round by round; the per-step figure is the median over rounds.

  python tools/bench_flat_models.py [--steps 20] [--rounds 5] [--warmup 3] [--only NAME] [--batch 256] [--clip 15] [--out file.jsonl]
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
from pedestrians_video_2_carla_amd.modules.movements import Linear  # noqa: E402
from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE2D  # noqa: E402
from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqFlatEmbeddings  # noqa: E402
from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything  # noqa: E402

MODELS = {
    'Seq2SeqFlatEmbeddings': lambda: Seq2SeqFlatEmbeddings(input_nodes=CARLA_SKELETON, movements_output_type=MT.pose_2d),
    'Seq2SeqFlatEmbeddings-inverted': lambda: Seq2SeqFlatEmbeddings(input_nodes=CARLA_SKELETON, movements_output_type=MT.pose_2d,
                                                                    invert_sequence=True),
    'Seq2SeqFlatEmbeddings-512-256': lambda: Seq2SeqFlatEmbeddings(input_nodes=CARLA_SKELETON, movements_output_type=MT.pose_2d,
                                                                   embeddings_size=[512, 256]),
    'LinearAE2D': lambda: LinearAE2D(input_nodes=CARLA_SKELETON),
    'LinearAE2D-f1': lambda: LinearAE2D(input_nodes=CARLA_SKELETON, model_scaling_factor=1),
    'Linear': lambda: Linear(input_nodes=CARLA_SKELETON, movements_output_type=MT.pose_2d),
}


def make(name, B, T, framework, d):
    for graph in (True, False):
        seed_everything(22742)
        dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
        model = MODELS[name]()
        model.hip_path = not framework
        flow = LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox')
        batch = dm.generate_batch(d)
        try:
            trainer = Trainer(device=d, use_graph=graph).setup(flow, dm)
            loss = trainer.train_step(flow, batch, 0)
            torch.cuda.synchronize(d)
            return dict(trainer=trainer, flow=flow, batch=batch, graph=bool(trainer.use_graph), first_loss=float(loss))
        except Exception as e:  # noqa: BLE001 -- a path that refuses capture is timed eagerly
            if not graph:
                raise
            print(f'[bench_flat_models] {name} framework={framework}: graph capture failed ({type(e).__name__}: {e}); eager steps',
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
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--clip', type=int, default=15)
    ap.add_argument('--only', choices=sorted(MODELS), default=None)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    d = torch.device('cuda:0')
    out = open(a.out, 'w') if a.out else None
    for name in ([a.only] if a.only else list(MODELS)):
        runs = {'hip': make(name, a.batch, a.clip, False, d), 'framework': make(name, a.batch, a.clip, True, d)}
        for r in runs.values():
            timed(r, a.warmup, d)
        ms = {k: [] for k in runs}
        for _ in range(a.rounds):
            for k, r in runs.items():
                ms[k].append(timed(r, a.steps, d))
        rec = dict(model=name, B=a.batch, T=a.clip, hip_ms=round(statistics.median(ms['hip']), 4),
                   framework_ms=round(statistics.median(ms['framework']), 4), hip_graph=runs['hip']['graph'],
                   framework_graph=runs['framework']['graph'], first_loss={k: r['first_loss'] for k, r in runs.items()},
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
