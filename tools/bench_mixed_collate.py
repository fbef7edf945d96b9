"""K26 (one launch for a mixed batch) against the path K11 alone would need: gather + one K11 launch per source + index_copy.

    python tools/bench_mixed_collate.py [B ...]      # clips per batch, default 256 1024 8192

The batch is the reference's three-source mixture at its default proportions (JAADCarlaRecAMASS: 0.1 BODY_25 with
confidence, boxes and clip sizes / 0.4 CARLA / 0.5 SMPL), T = 16, shuffled so that the sources interleave clip by clip,
with flip + rotation for all, gaussian noise and missing joints for the two synthetic sources, hips_neck_bbox.
Both arms start from the same per-source device arrays and the same batch-ordered draws and end with the same batch-ordered
tensors (checked bit for bit before timing). Times are device events around windows of ``REPS`` calls as a training loop
would issue them (descriptor building and launch gaps included: it is the time per batch, not kernel time), the two arms
alternating window by window; the median window of each arm is reported, with the spread. One JSON line.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops
from pedestrians_video_2_carla_amd.data.base.skeleton import get_common_indices
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
from pedestrians_video_2_carla_amd.data.smpl.skeleton import SMPL_SKELETON

T, REPS, ROUNDS = 16, 50, 9
MIX = ((BODY_25_SKELETON, 0.1, 3), (CARLA_SKELETON, 0.4, 2), (SMPL_SKELETON, 0.5, 2))


def _points(p):
    return tuple(q.value for q in (p if isinstance(p, (list, tuple)) else (p,)))


def case(B, device, seed=3):
    g = torch.Generator().manual_seed(seed)
    counts = [int(B * f) for _, f, _ in MIX]
    counts[-1] = B - sum(counts[:-1])
    source = torch.cat([torch.full((n,), k, dtype=torch.uint8) for k, n in enumerate(counts)])
    row = torch.cat([torch.arange(n, dtype=torch.int32) for n in counts])
    order = torch.randperm(B, generator=g)
    source, row = source[order], row[order]
    specs, settings = [], []
    bboxes, clip_size = torch.full((B, T, 2, 2), float('nan')), torch.zeros(B, 2)
    for k, ((nodes, _, C), n) in enumerate(zip(MIX, counts)):
        J = len(nodes)
        raw = torch.rand(n, T, J, 2, generator=g) * torch.tensor([600., 400.]) + torch.tensor([100., 50.])
        if C == 3:
            raw = torch.cat((raw, torch.rand(n, T, J, 1, generator=g) * 0.9 + 0.05), -1)
        raw[torch.rand(n, T, J, generator=g) < 0.05] = 0.0
        kw = dict(flip_perm=nodes.get_flip_mask(), transform='hips_neck_bbox', hips_idx=_points(nodes.get_hips_point()),
                  neck_idx=_points(nodes.get_neck_point()), miss_prob=[0.1] * J if k else None)
        if nodes is not CARLA_SKELETON:
            dst, src = get_common_indices(input_nodes=nodes, output_nodes=CARLA_SKELETON)
            kw.update(src_idx=list(src), dst_idx=list(dst))
        if k == 0:
            mine = source == 0
            bboxes[mine] = torch.stack((raw[..., :2].amin(-2) - 4, raw[..., :2].amax(-2) + 4), -2)[row[mine].long()]
            clip_size[mine] = torch.tensor([1920., 1080.])
        specs.append(ops.MixedSource(raw=raw.to(device), has_noise=k > 0, has_bboxes=k == 0, **kw))
        settings.append(kw)
    draws = dict(is_flipped=(torch.rand(B, generator=g) < 0.5).to(torch.uint8), rotation=(torch.rand(B, generator=g) * 2 - 1) * 10,
                 noise=torch.randn(B, T, 26, 2, generator=g), miss_u=torch.rand(B, T, 26, generator=g), bboxes=bboxes,
                 clip_size=clip_size)
    return specs, settings, source.to(device), row.to(device), {k: v.to(device) for k, v in draws.items()}


def mixed(specs, source, row, draws):
    return ops.collate_mixed(specs, source, row, n_input_joints=26, **draws)


class PerSource:
    """The other arm: what a loader would do per batch with K11 only. The index tensors are per batch, so building them
    (one nonzero per source, a device-to-host size each) belongs to the arm; the output buffers are reused."""

    def __init__(self, specs, settings, B, device):
        self.specs, self.settings = specs, settings
        f32 = dict(dtype=torch.float32, device=device)
        self.frames = torch.empty(B, T, 26, 2, **f32)
        self.targets = {k: torch.empty(B, T, 26, 2, **f32) for k in ('projection_2d', 'projection_2d_deformed', 'projection_2d_transformed')}
        self.targets.update(projection_2d_shift=torch.empty(B, T, 2, **f32), projection_2d_scale=torch.empty(B, T, **f32),
                            bboxes=torch.empty(B, T, 2, 2, **f32))

    def __call__(self, source, row, draws):
        for k, (spec, kw) in enumerate(zip(self.specs, self.settings)):
            idx = torch.nonzero(source == k).flatten()
            J = spec.raw.shape[2]
            one = dict(is_flipped=draws['is_flipped'][idx], rotation=draws['rotation'][idx])
            if k == 0:
                one.update(bboxes=draws['bboxes'][idx], clip_size=draws['clip_size'][idx])
            else:
                one.update(noise=draws['noise'][idx][:, :, :J].contiguous(), miss_u=draws['miss_u'][idx][:, :, :J].contiguous())
            frames, targets = ops.collate(spec.raw[row[idx].long()], n_input_joints=26, **kw, **one)
            self.frames.index_copy_(0, idx, frames)
            for name, buf in self.targets.items():
                if name in targets:
                    buf.index_copy_(0, idx, targets[name])
                elif name == 'projection_2d_deformed':
                    buf.index_copy_(0, idx, targets['projection_2d'])
        return self.frames, self.targets


def window(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(REPS):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / REPS


def main():
    device = torch.device('cuda:0')
    out = {'tool': 'bench_mixed_collate', 'T': T, 'mix': [f for _, f, _ in MIX], 'reps_per_window': REPS, 'windows': ROUNDS,
           'timing': 'device events around windows of calls (launch gaps included)', 'batches': []}
    for B in [int(a) for a in sys.argv[1:]] or [256, 1024, 8192]:
        specs, settings, source, row, draws = case(B, device)
        other = PerSource(specs, settings, B, device)
        arms = {'k26_one_launch': lambda: mixed(specs, source, row, draws), 'k11_per_source': lambda: other(source, row, draws)}
        f_a, t_a = arms['k26_one_launch']()
        f_b, t_b = arms['k11_per_source']()
        same = torch.equal(f_a, f_b) and all(
            torch.equal(torch.nan_to_num(t_a[k][source == 0] if k == 'bboxes' else t_a[k]),
                        torch.nan_to_num(v[source == 0] if k == 'bboxes' else v)) for k, v in t_b.items())
        for fn in arms.values():                     # warm-up of every shape the windows use
            window(fn)
        times = {name: [] for name in arms}
        for _ in range(ROUNDS):
            for name, fn in arms.items():
                times[name].append(window(fn))
        res = {'B': B, 'outputs_equal': bool(same)}
        for name, v in times.items():
            res[name] = {'us_per_batch': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2)}
        res['ratio'] = round(res['k11_per_source']['us_per_batch'] / res['k26_one_launch']['us_per_batch'], 2)
        out['batches'].append(res)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
