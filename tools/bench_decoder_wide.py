"""K7c at 64 < O <= 160: decoder forward + backward through ops.decoder_stack (10 launches: forward = 2 decoder_k + the loop,
backward = the loop + 2 decoder_gk + 2 decoder_ghid, then the grouped weight-gradient pair) against the per-step path of Seq2Seq.forward (per frame: K7b layer launches, K16 projections, torch.where / stack; selected
with P2C_DECODER_WIDE=0, which is read at every call), both arms in ONE process, alternated.

usage: bench_decoder_wide.py [--rounds 3] [--iters 100] [--warmup 20] [--shapes 512x78,512x156,...] [--arms fused,steps]
Per shape (B, O), T = 16, H = 64, dropout off: `rounds` alternations of (fused, per-step); each visit = warm-up iterations, then
`iters` timed ones between two events on the live stream. Prints one JSON line per shape: the median of each arm's visits, the
min..max spread over the visits, and the launches of one forward + backward counted with the profiler (kernel events).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON  # noqa: E402
from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT  # noqa: E402
from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2Seq  # noqa: E402

OTYPE = {78: MT.absolute_loc, 156: MT.pose_changes}
T = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--shapes', default='512x78,512x156,4096x78,4096x156,8192x78,8192x156')
    ap.add_argument('--arms', default='fused,steps')
    args = ap.parse_args()
    d = torch.device('cuda:0')
    arms = args.arms.split(',')
    for shape in args.shapes.split(','):
        B, O = (int(v) for v in shape.split('x'))
        torch.manual_seed(B + O)
        model = Seq2Seq(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=OTYPE[O], p_dropout=0.0,
                        hidden_size=64).to(d).train()
        model.rotation_output_format = 'rotation_6d'
        assert model.decoder.output_size == O
        hidden, cell = torch.randn(2, B, 64, device=d) * 0.3, torch.randn(2, B, 64, device=d) * 0.3
        up = torch.randn(B, T, O, device=d)
        x = torch.empty(B, T, 26, 2, device=d)
        params = list(model.decoder.parameters())

        def step(arm):
            """the decoder half of Seq2Seq.forward + its backward, from the encoder state"""
            os.environ['P2C_DECODER_WIDE'] = '1' if arm == 'fused' else '0'
            h, c = hidden.clone().requires_grad_(True), cell.clone().requires_grad_(True)
            if model._decoder_loop_fusable(x):
                out = model._fused_decoder(h, c, T)
            else:
                assert arm == 'steps'
                step_in, outs = torch.zeros(B, O, device=d), []
                for _ in range(T):
                    step_in, o = model._decode_frame(h, c, step_in, False, None, None)
                    outs.append(o)
                out = torch.stack(outs, 0).permute(1, 0, 2)
            torch.autograd.backward((out * up).sum(), inputs=[h, c] + params)
            for p in params:
                p.grad = None

        def launches(arm):
            step(arm)
            torch.cuda.synchronize()
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                step(arm)
                torch.cuda.synchronize()
            return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)

        times = {a: [] for a in arms}
        for _ in range(args.rounds):
            for arm in arms:
                for _ in range(args.warmup):
                    step(arm)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    step(arm)
                e1.record()
                e1.synchronize()
                times[arm].append(e0.elapsed_time(e1) / args.iters * 1e3)
        row = {'B': B, 'O': O, 'T': T, 'iters': args.iters, 'rounds': args.rounds}
        for arm in arms:
            v = sorted(times[arm])
            row[arm + '_us'] = round(v[len(v) // 2], 1)
            row[arm + '_us_visits'] = [round(t, 1) for t in times[arm]]
            try:
                row[arm + '_launches'] = launches(arm)
            except Exception as e:      # the profiler is a convenience here, not the measurement
                row[arm + '_launches'] = f'n/a ({type(e).__name__})'
        if len(arms) == 2:
            row['steps_over_fused'] = round(row['steps_us'] / row['fused_us'], 2)
        print(json.dumps(row), flush=True)


if __name__ == '__main__':
    main()
