"""K27 (ops.pose_change_loss: one launch each way) against the tensor path on the device (P2C_PCL_FRAMEWORK=1: what ran before K27).

    python tools/bench_pose_change_loss.py [B ...]      # clips per batch, default 256 8192

Part 1, the loss alone: cum_pose_changes and pose_changes, forward + backward, T = 16, J = 26, on the raw 6-D output and on
matrices; both arms get the same device tensors, and their losses and gradients are compared before timing.
Part 2, the whole ``training_step`` + backward of a LinearAE LitPoseLiftingFlow with ``loss_modes=['cum_pose_changes']``: with K27
the lean step is model + K27; the other arm is the step as it was (materialising pose head in front of the tensor-op loss).
Times are device events around windows of ``REPS`` calls as a training loop would issue them (launch gaps included: time per
call, not kernel time), the two arms alternating window by window; the median window of each arm is reported with its
spread. Kernel launches per call are counted with the profiler where it is available. One JSON line.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd.loss import LossModes

T, J, REPS, ROUNDS = 16, 26, 20, 9
ARMS = (('k27', '0'), ('framework', '1'))


def window(fn, reps=REPS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def launches(fn):
    """Kernel launches of one call (None where the profiler cannot trace the device)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, 'device_type', None) is not None and 'cuda' in str(e.device_type).lower()
                and 'memcpy' not in e.name.lower() and 'memset' not in e.name.lower())
        return n or None
    except Exception:                                          # noqa: BLE001  (a count is a nicety; the times are the result)
        return None


def alternate(fns):
    """fns: arm -> callable (the switch is set around every call of that arm). -> arm -> {us, min, max}, plus launch counts."""
    def armed(name, env):
        def run():
            os.environ['P2C_PCL_FRAMEWORK'] = env
            fns[name]()
        return run
    calls = {name: armed(name, env) for name, env in ARMS}
    for fn in calls.values():                                  # warm-up of every shape the windows use
        window(fn)
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, fn in calls.items():
            times[name].append(window(fn))
    res = {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2),
                  'launches': launches(calls[name])} for name, v in times.items()}
    res['ratio'] = round(res['framework']['us_per_call'] / res['k27']['us_per_call'], 2)
    os.environ['P2C_PCL_FRAMEWORK'] = '0'
    return res


def loss_case(mode, B, six_d, device):
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import rotation_6d_to_matrix
    g = torch.Generator().manual_seed(5)
    fn, crit = LossModes[mode].value
    tgt = rotation_6d_to_matrix(torch.randn(B, T, J, 6, generator=g)).to(device)
    pred = torch.randn(B, T, J, 6, generator=g)
    pred = (pred if six_d else rotation_6d_to_matrix(pred)).to(device).requires_grad_(True)

    def step():
        pred.grad = None
        fn(criterion=crit, pose_inputs=pred, targets={'pose_changes': tgt}).backward()
    got = {}
    for name, env in ARMS:
        os.environ['P2C_PCL_FRAMEWORK'] = env
        pred.grad = None
        loss = fn(criterion=crit, pose_inputs=pred, targets={'pose_changes': tgt})
        loss.backward()
        got[name] = (loss.detach().double(), pred.grad.double().clone())
    (la, ga), (lb, gb) = got['k27'], got['framework']
    res = alternate({'k27': step, 'framework': step})
    res.update(mode=mode, B=B, layout='6d' if six_d else 'matrix', loss_rel_diff=float((la - lb).abs() / lb.abs()),
               grad_rel_diff=float((ga - gb).abs().max() / gb.abs().max()))
    return res


def flow_case(B, device):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix
    seed_everything(22742)
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
    flow = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
                              loss_modes=['cum_pose_changes'], transform=dm.transform.name)
    flow.attach_datamodule(dm)
    flow.to(device).train()
    batch = dm.generate_batch(device)
    g = torch.Generator().manual_seed(3)
    batch[1]['pose_changes'] = euler_angles_to_matrix((torch.rand(B, T, J, 3, generator=g) * 2 - 1) * 0.1).to(device)

    def step():
        flow.zero_grad(set_to_none=True)
        flow.on_train_batch_start(batch, 0)
        flow.training_step(batch, 0)['loss'].backward()
    res = alternate({'k27': step, 'framework': step})
    res.update(B=B, what='training_step + backward, LinearAE, loss_modes=[cum_pose_changes]')
    return res


def main():
    device = torch.device('cuda:0')
    out = {'tool': 'bench_pose_change_loss', 'T': T, 'J': J, 'reps_per_window': REPS, 'windows': ROUNDS,
           'timing': 'device events around windows of calls (launch gaps included)', 'loss': [], 'training_step': []}
    for B in [int(a) for a in sys.argv[1:]] or [256, 8192]:
        for mode in ('cum_pose_changes', 'pose_changes'):
            for six_d in (True, False):
                out['loss'].append(loss_case(mode, B, six_d, device))
        out['training_step'].append(flow_case(B, device))
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
