"""Train-step timing of the classification flow: HIP arm (dense kernels + K7b / K23 recurrences + K24 loss) against the framework
arm (``P2C_CLS_FRAMEWORK=1``: nn.LSTM / nn.GRU, i.e. MIOpen, and the torch criterion), in the same process, alternating.

One train step of LitClassificationFlow at B = 256, T = 16, CARLA input, H = 64, L = 2, for both models. Each arm builds its flow +
Trainer (eager steps, flat parameters, fused AdamW) from the same weights and batch, warms up, then times ROUNDS x STEPS train
steps with device events, the two arms taking turns round by round; the per-step figure is the median over rounds. The switch is
read at every forward, so it is set around each arm's steps.

  python tools/bench_gru_classifier.py [--steps 20] [--rounds 5] [--warmup 3] [--only GRU|LSTM] [--out profiles/classification/bench_gru_classifier.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON  # noqa: E402
from pedestrians_video_2_carla_amd.modules import classification  # noqa: E402
from pedestrians_video_2_carla_amd.modules.flow.classification import LitClassificationFlow  # noqa: E402
from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [dict(model=m, B=256, T=16, H=64, L=2, num_classes=2) for m in ('LSTM', 'GRU')]


class arm:
    """The environment switch of one arm, set while its steps are issued."""

    def __init__(self, framework: bool):
        self.value = '1' if framework else '0'

    def __enter__(self):
        self.prev = os.environ.get('P2C_CLS_FRAMEWORK')
        os.environ['P2C_CLS_FRAMEWORK'] = self.value

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop('P2C_CLS_FRAMEWORK', None)
        else:
            os.environ['P2C_CLS_FRAMEWORK'] = self.prev
        return False


def make(shape, framework, d):
    seed_everything(22742)
    model = getattr(classification, shape['model'])(input_nodes=CARLA_SKELETON, hidden_size=shape['H'], num_layers=shape['L'],
                                                    num_classes=shape['num_classes'])
    flow = LitClassificationFlow(classification_model=model, classification_targets_key='cross', num_classes=shape['num_classes'])
    g = torch.Generator().manual_seed(31)
    batch = (torch.randn(shape['B'], shape['T'], len(CARLA_SKELETON), 2, generator=g).to(d),
             {'cross': torch.randint(0, shape['num_classes'], (shape['B'], 1), generator=g).to(d)}, {})
    trainer = Trainer(device=d, use_graph=False).setup(flow, None)
    with arm(framework):
        loss = trainer.train_step(flow, batch, 0)
    torch.cuda.synchronize(d)
    return dict(trainer=trainer, flow=flow, batch=batch, framework=framework, first_loss=float(loss))


def timed(run, steps, d):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with arm(run['framework']):
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
    ap.add_argument('--only', choices=['GRU', 'LSTM'], default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'classification', 'bench_gru_classifier.jsonl'))
    a = ap.parse_args()
    d = torch.device('cuda:0')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as out:
        for shape in SHAPES:
            if a.only and shape['model'] != a.only:
                continue
            runs = {'hip': make(shape, False, d), 'framework': make(shape, True, d)}
            for r in runs.values():
                timed(r, a.warmup, d)
            ms = {k: [] for k in runs}
            for _ in range(a.rounds):
                for k, r in runs.items():
                    ms[k].append(timed(r, a.steps, d))
            rec = dict(shape, hip_ms=round(statistics.median(ms['hip']), 4), framework_ms=round(statistics.median(ms['framework']), 4),
                       first_loss={k: r['first_loss'] for k, r in runs.items()},
                       rounds_ms={k: [round(v, 4) for v in vs] for k, vs in ms.items()})
            rec['speedup'] = round(rec['framework_ms'] / rec['hip_ms'], 2)
            line = json.dumps(rec)
            print(line, flush=True)
            out.write(line + '\n')
            out.flush()
            del runs
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
