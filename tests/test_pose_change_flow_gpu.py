"""GPU: ``--loss_modes pose_changes`` / ``cum_pose_changes`` through LitPoseLiftingFlow. training_step + backward against LinearAE
in fp64 on the CPU with the losses written out (tolerances of tests/test_losses_extra.py::test_extra_modes_train_through_the_flow),
which launches the step makes (one K27 call, no pose head when these are the only modes; the lean pose-head launches untouched
next to loc_2d_3d), validation still materialising, and the P2C_PCL_FRAMEWORK=1 arm."""
import copy

import pytest
import torch

from oracle import pose_head as O
from tests.test_flow_gpu import close, make

pytestmark = pytest.mark.gpu

B, T = 6, 16
# the issue's three, and the mixed pair the other way round: the first requested loss that can be calculated is the step's
# loss (base.py:464-465), so only there does K27 run next to the lean pose-head launches
MODES = [('pose_changes',), ('cum_pose_changes',), ('loc_2d_3d', 'cum_pose_changes'), ('cum_pose_changes', 'loc_2d_3d')]


def setup(modes, lean=True):
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import euler_angles_to_matrix
    d = torch.device('cuda:0')
    flow, dm = make(loss_modes=modes, B=B, T=T, missing=0.1, lean=lean)
    flow.attach_datamodule(dm)
    flow.to(d).train()
    batch = dm.generate_batch(d)
    g = torch.Generator().manual_seed(3)
    batch[1]['pose_changes'] = euler_angles_to_matrix((torch.rand(B, T, 26, 3, generator=g) * 2 - 1) * 0.1).to(d)
    return flow, dm, batch


def cpu_reference(flow, batch, primary):
    """LinearAE in fp64 on the CPU and the primary loss written out; returns (loss, model with .grad)."""
    from pedestrians_video_2_carla_amd.loss.cum_pose_changes import _accumulate
    frames, targets, meta = batch
    cpu_model = copy.deepcopy(flow.movements_model).cpu().double()
    cpu_model.rotation_output_format = 'rotation_6d'
    y = cpu_model(frames.double().cpu())
    gt = targets['pose_changes'].double().cpu()
    if primary == 'cum_pose_changes':
        ref = torch.nn.functional.mse_loss(_accumulate(O.rotation_6d_to_matrix(y)), _accumulate(gt))
    elif primary == 'pose_changes':
        ref = ((O.rotation_6d_to_matrix(y) - gt) ** 2).sum()
    else:
        ref = O.pose_head(y, 'pose_changes_6d', meta['skel_type'].cpu(), gt2d=targets['projection_2d_transformed'].double().cpu(),
                          gt3d=targets['absolute_pose_loc'].double().cpu())['loc_2d_3d']
    ref.backward()
    return ref.detach(), cpu_model


class Calls:
    """Counts what a step calls: the K27 op, the pose head behind the projection module, and the module's two entries."""

    def __init__(self, monkeypatch):
        from pedestrians_video_2_carla_amd import ops
        from pedestrians_video_2_carla_amd.modules.layers.projection import ProjectionModule
        self.n = dict(k27=0, pose_head=0, forward=0, fused_losses=0)
        for owner, name, key in ((ops, 'pose_change_loss', 'k27'), (ops, 'pose_head', 'pose_head'),
                                 (ProjectionModule, 'forward', 'forward'), (ProjectionModule, 'fused_losses', 'fused_losses')):
            monkeypatch.setattr(owner, name, self.wrap(getattr(owner, name), key))

    def wrap(self, fn, key):
        def counted(*a, **k):
            self.n[key] += 1
            return fn(*a, **k)
        return counted


@pytest.mark.parametrize('modes', MODES, ids=['+'.join(m) for m in MODES])
def test_training_step_matches_the_cpu_pipeline_and_takes_the_lean_launches(modes, monkeypatch):
    flow, dm, batch = setup(modes)
    calls = Calls(monkeypatch)
    flow.on_train_batch_start(batch, 0)
    out = flow.training_step(batch, 0)
    out['loss'].backward()
    ref, cpu_model = cpu_reference(flow, batch, modes[0])
    print(modes, 'loss', float(out['loss']), 'reference', float(ref), 'calls', calls.n)
    close(out['loss'], ref, f'{modes} loss')
    close(flow.logged['train_loss/primary'], ref, f'{modes} primary')
    for (n, pg), (_, pc) in zip(flow.movements_model.named_parameters(), cpu_model.named_parameters()):
        close(pg.grad, pc.grad, f'{modes} grad {n}', rtol=2e-4)
    if len(modes) == 1:                  # model + K27 forward + K27 backward: nobody reads what the pose head computes
        assert calls.n == dict(k27=1, pose_head=0, forward=0, fused_losses=0)
        assert out['preds']['projection_2d_transformed'] is None and out['preds']['absolute_pose_loc'] is None
    else:                                # the lean pose-head launches stay; the materialising forward is not taken
        assert calls.n['fused_losses'] == 1 and calls.n['pose_head'] == 1 and calls.n['forward'] == 0
        assert calls.n['k27'] == (1 if modes[0] == 'cum_pose_changes' else 0)
        assert out['preds']['absolute_pose_loc'] is None          # lean train outputs


@pytest.mark.parametrize('modes', MODES[:3], ids=['+'.join(m) for m in MODES[:3]])
def test_validation_and_full_outputs_still_materialise(modes):
    flow, dm, batch = setup(modes)
    frames, targets, meta = batch
    flow.eval()
    flow.on_validation_batch_start(batch, 0)
    with torch.no_grad():
        val = flow.validation_step(batch, 0)
        y = flow.movements_model(frames)
    o = O.pose_head(y.double().cpu(), 'pose_changes_6d', meta['skel_type'].cpu(),
                    gt2d=targets['projection_2d_transformed'].double().cpu(), gt3d=targets['absolute_pose_loc'].double().cpu())
    assert val['preds']['projection_2d_transformed'] is not None
    close(val['preds']['projection_2d_transformed'][..., :2], o['projection_2d_transformed'][..., :2], f'{modes} val projection')
    close(val['preds']['absolute_pose_loc'], o['absolute_pose_loc'], f'{modes} val abs loc')
    ref, _ = cpu_reference(flow, batch, modes[0])
    close(val['loss'], ref, f'{modes} val loss')
    # lean_train_outputs=False: the train step materialises too
    full, dm2, batch2 = setup(modes, lean=False)
    full.on_train_batch_start(batch2, 0)
    out = full.training_step(batch2, 0)
    assert out['preds']['projection_2d_transformed'] is not None and out['preds']['absolute_pose_loc'] is not None
    close(out['loss'], cpu_reference(full, batch2, modes[0])[0], f'{modes} full-output loss')


@pytest.mark.parametrize('modes', MODES[:3], ids=['+'.join(m) for m in MODES[:3]])
def test_framework_arm_gives_the_same_loss(modes, monkeypatch):
    flow, dm, batch = setup(modes)
    ref, _ = cpu_reference(flow, batch, modes[0])
    monkeypatch.setenv('P2C_PCL_FRAMEWORK', '1')
    calls = Calls(monkeypatch)
    flow.on_train_batch_start(batch, 0)
    out = flow.training_step(batch, 0)
    out['loss'].backward()
    assert calls.n['k27'] == 0
    close(out['loss'], ref, f'{modes} framework loss')
