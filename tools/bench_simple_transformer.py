"""Train-step timing of SimpleTransformer in the autoencoder flow: HIP path (K16 GEMMs with the ReLU + dropout epilogues, K20
attention and post-norm residual LayerNorm) against the framework path (nn.TransformerEncoder), in the same process, alternating.

Each shape builds one LitAutoencoderFlow + Trainer per path from the same weights and batch (loc_2d, dropout 0.1), warms both up
(the trainer captures its graph at the first step and checks the replay; a path whose replay check fails runs eagerly and the
record says so), then times ROUNDS x STEPS train steps per path with device events, the two paths taking turns round by round;
the per-step figure is the median over rounds. The framework path is selected per instance here (P2C_ENCODER_FRAMEWORK=1 selects
it for a whole process). GEMM TFLOP/s is the step's fp32 GEMM work over the HIP step time against the 157.3 TFLOP/s fp32-MFMA
peak; launches per step come from the captured graph's kernel nodes where the trainer counted them.

  python tools/bench_simple_transformer.py [--steps 20] [--rounds 5] [--warmup 3] [--shape skel,heads,T,B] [--hip-only] [--out f.jsonl]
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
from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON  # noqa: E402
from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow  # noqa: E402
from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer  # noqa: E402
from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything  # noqa: E402

SKELETONS = {'CARLA': CARLA_SKELETON, 'BODY_25': BODY_25_SKELETON}
SHAPES = [dict(skel='CARLA', heads=4, T=16, B=B) for B in (64, 512, 2048)] + [dict(skel='BODY_25', heads=5, T=30, B=512)]
PEAK_TFLOPS = 157.3


def build(shape, framework):
    seed_everything(22742)
    nodes = SKELETONS[shape['skel']]
    dm = SyntheticCarlaRecordedDataModule(clip_length=shape['T'], batch_size=shape['B'], missing_joint_probabilities=0.1,
                                          **({} if nodes is CARLA_SKELETON else dict(input_nodes=nodes)))
    model = SimpleTransformer(input_nodes=nodes, n_heads=shape['heads'], movements_output_type='pose_2d')
    if framework:
        model._device_path = lambda x: False                  # the nn modules on the device
    flow = LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox')
    return flow, dm


def make_model_step(shape, framework, d):
    """BODY_25: the synthetic data module yields CARLA frames only, so the step is the model's own -- forward, MSE against a fixed
    target, backward, AdamW (the flow's optimizer settings) -- eagerly, with the same two paths."""
    seed_everything(22742)
    nodes = SKELETONS[shape['skel']]
    model = SimpleTransformer(input_nodes=nodes, n_heads=shape['heads'], movements_output_type='pose_2d').to(d).train()
    if framework:
        model._device_path = lambda x: False
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2)
    g = torch.Generator(device=d).manual_seed(1)
    x = torch.randn(shape['B'], shape['T'], len(nodes), 2, device=d, generator=g)
    y = torch.randn(x.shape, device=d, generator=g)

    def step(i):
        opt.zero_grad(set_to_none=True)
        loss = (model(x) - y).pow(2).mean()
        loss.backward()
        opt.step()
        return loss
    loss = step(0)
    torch.cuda.synchronize(d)
    return dict(step=step, graph=False, first_loss=float(loss), launches=None, kind='model step (eager)')


def make(shape, framework, d):
    if shape['skel'] != 'CARLA':
        return make_model_step(shape, framework, d)
    flow, dm = build(shape, framework)
    batch = dm.generate_batch(d)
    trainer = Trainer(device=d, use_graph=True).setup(flow, dm)
    loss = trainer.train_step(flow, batch, 0)
    torch.cuda.synchronize(d)
    nodes = trainer._graph_nodes
    return dict(step=lambda i: trainer.train_step(flow, batch, i), graph=bool(trainer.use_graph), first_loss=float(loss),
                launches=(nodes[1] if nodes else None), kind='autoencoder flow step')


def timed(run, steps, d):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(steps):
        run['step'](i)
    end.record()
    torch.cuda.synchronize(d)
    return start.elapsed_time(end) / steps


def gemm_flop(shape, d_ff=2048):
    """fp32 GEMM FLOP of one train step over six layers: forward 2 R (4 d^2 + 2 d d_ff) per layer (in_proj 3 d^2, out_proj d^2,
    the FFN), backward twice that (input and weight gradients). The attention itself (4 R T d) is not counted."""
    R, dm = shape['B'] * shape['T'], 2 * len(SKELETONS[shape['skel']])
    return 6 * 3 * 2 * R * (4 * dm * dm + 2 * dm * d_ff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shape', default=None, help='skel,heads,T,B: one shape only (e.g. for a kernel-trace run)')
    ap.add_argument('--hip-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    d = torch.device('cuda:0')
    shapes = SHAPES
    if a.shape:
        sk, h, T, B = a.shape.split(',')
        shapes = [dict(skel=sk, heads=int(h), T=int(T), B=int(B))]
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
        hip = statistics.median(ms['hip'])
        flop = gemm_flop(shape)
        rec = dict(shape, d=2 * len(SKELETONS[shape['skel']]), step=runs['hip']['kind'], hip_ms=round(hip, 4), hip_graph=runs['hip']['graph'],
                   hip_launches=runs['hip']['launches'], gemm_gflop=round(flop / 1e9, 2),
                   gemm_tflops=round(flop / hip / 1e9, 2), peak_fraction=round(flop / hip / 1e9 / PEAK_TFLOPS, 3))
        if 'framework' in runs:
            rec.update(framework_ms=round(statistics.median(ms['framework']), 4), framework_graph=runs['framework']['graph'],
                       framework_launches=runs['framework']['launches'])
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
