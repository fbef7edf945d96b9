"""K29 (gradient clipping inside the optimizer launch, csrc/p2c_grad_clip.hip) against the unclipped step and against the
tensor path, on flat buffers of the sizes two models really have.

    python tools/bench_grad_clip.py

Arms, all on the same flat buffers (FlatAdamW with zero_grad_in_step=False, so the gradient stays what it was):
  unclipped   p2c_adamw_step                                               1 launch
  k29_norm    p2c_adamw_step_clipped, P2C_CLIP_NORM (squared-norm partials + step)   2 launches
  k29_value   p2c_adamw_step_clipped, P2C_CLIP_VALUE                       1 launch
  torch_norm  torch.nn.utils.clip_grad_norm_ on the flat tensor, then p2c_adamw_step
The flat sizes are counted from LinearAE and PoseFormer as the trainer would flatten them (trainable parameters that take
part in forward) and printed. Times are device events around windows of REPS calls issued as a training loop would (launch
gaps included: time per call, not kernel time); the arms alternate window by window, one warm-up window each, then ROUNDS
windows each (REPS * ROUNDS = 450 timed calls per arm); the median window is reported with its spread. One JSON line.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

REPS, ROUNDS = 50, 9
CLIP = 0.5


def flat_sizes():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.modules.movements.pose_former import PoseFormer
    models = {'LinearAE': LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
              'PoseFormer': PoseFormer(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, clip_length=81)}
    return {name: sum(p.numel() for p in m.parameters() if p.requires_grad and not getattr(p, 'p2c_unused', False))
            for name, m in models.items()}


def window(fn, reps=REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def case(n, device):
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    g = torch.Generator(device=device).manual_seed(n)
    p0 = torch.randn(n, device=device, generator=g)
    grad = torch.randn(n, device=device, generator=g) * 3
    arms = {}
    for name, clip in (('unclipped', None), ('k29_norm', 'norm'), ('k29_value', 'value'), ('torch_norm', None)):
        p = torch.nn.Parameter(p0.clone())
        p.grad = grad.clone()
        o = FlatAdamW([p], zero_grad_in_step=False)
        if clip:
            o.set_clip(CLIP, clip)
        if name == 'torch_norm':
            def fn(o=o, p=p):
                # (scales the gradient in place: from the second call on its norm IS the bound and the coefficient clamps to 1,
                # but clip_grad_norm_ multiplies whatever the coefficient is -- no host sync -- so every call does the same work)
                torch.nn.utils.clip_grad_norm_([p], CLIP)
                o.step()
        else:
            fn = o.step
        arms[name] = fn
    for fn in arms.values():
        window(fn)
    times = {name: [] for name in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            times[name].append(window(fn))
    res = {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}
           for name, v in times.items()}
    res['n'] = n
    return res


def main():
    device = torch.device('cuda:0')
    sizes = flat_sizes()
    print('flat sizes:', sizes, file=sys.stderr, flush=True)
    out = {'tool': 'bench_grad_clip', 'reps_per_window': REPS, 'windows': ROUNDS, 'clip': CLIP,
           'timing': 'device events around windows of calls (launch gaps included)',
           'flat_sizes': sizes, 'cases': {name: case(n, device) for name, n in sizes.items()}}
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
