"""GPU: K30 (csrc/p2c_carla_pose.hip, ``ops.carla_pose_export`` / ``carla_pose_import``) against the fp64 tensor definitions
evaluated on the host on the same fp32 inputs.

Tolerance, per case: the error of the fp32 tensor restatement on the device (the ``P2C_CARLA_FRAMEWORK=1`` path) against fp64 is
measured on the same inputs, and K30 is allowed four times that for the libm differences of atan2f / asinf / sincosf, with a
floor of 1e-4 degree on angles. Locations must be exact (a copy and a sign). The inverse writes matrix entries, each a sum of
products of sines and cosines whose derivative with respect to any one of the three angles is at most 1 in magnitude, so an
angle error at the floor moves an entry by at most 3 * radians(1e-4): that is the floor on matrices. Measured values: DESIGN
section 5.13."""
import functools
import math

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import ops
from test_carla_pose import host_flow, problem

pytestmark = pytest.mark.gpu

ANGLE_FLOOR_DEG = 1e-4
MATRIX_FLOOR = 3 * math.radians(ANGLE_FLOOR_DEG)
# what rounding exact rotations to fp32 costs a fwd -> inv round trip: entries move by up to 2^-25, asin by that / cos(80 deg),
# each atan2 by sqrt(2) times that / cos(80 deg), and every angle error reaches an entry with a factor of at most 1
INPUT_ROUNDING = (1 + 2 * math.sqrt(2.0)) * 2.0 ** -25 / math.cos(math.radians(80.0)) + 2.0 ** -25
# (N, J, max_blocks): one lane; under one wavefront; across a wavefront with a partial last one; several workgroups with a partial
# last one (1040 bone rows: the root rows start inside the fifth workgroup); another J; two workgroups striding over 1040 (+ 40) rows
SHAPES = [(1, 1, 0), (1, 26, 0), (5, 26, 0), (40, 26, 0), (3, 5, 0), (40, 26, 2)]


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def reference(N, J):
    """fp64 on the host, on the fp32 inputs of ``problem``: (bones, root), and the inverse of the fp32-rounded bones."""
    loc, rot, wloc, wrot = problem(N, J)
    bones, root = ops.carla_pose_export(loc.double(), rot.double(), wloc.double(), wrot.double())
    rows32 = bones.float()
    inv_loc, inv_rot = ops.carla_pose_import(rows32.double())
    return bones, root, rows32, inv_loc, inv_rot


def angle_tolerance(framework_rows, want_rows, what):
    err = float((framework_rows.double().cpu()[..., 3:] - want_rows[..., 3:]).abs().max())
    tol = max(4 * err, ANGLE_FLOOR_DEG)
    print(f'{what}: fp32 tensor restatement on the device is {err:.3e} degree from fp64 -> K30 is allowed {tol:.3e}')
    return tol


def check_rows(got, want, tol, what):
    got = got.double().cpu()
    assert got.shape == want.shape, what
    assert torch.equal(got[..., :3], want[..., :3]), f'{what}: locations are a copy and a sign, they must be exact'
    err = float((got[..., 3:] - want[..., 3:]).abs().max())
    print(f'{what}: K30 is {err:.3e} degree from fp64 (allowed {tol:.3e})')
    assert math.isfinite(err) and err <= tol, what


@pytest.mark.parametrize('world', [False, True])
@pytest.mark.parametrize('N,J,max_blocks', SHAPES)
def test_export_matches_the_fp64_definition(N, J, max_blocks, world):
    loc, rot, wloc, wrot = (t.to(dev()) for t in problem(N, J))
    want_bones, want_root, *_ = reference(N, J)
    tol = angle_tolerance(ops._carla_row(loc, rot), want_bones, f'({N},{J}) bones')
    bones, root = ops.carla_pose_export(loc, rot, wloc if world else None, wrot if world else None, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert bones.dtype == torch.float32 and bones.is_cuda and bones.shape == (N, J, 6)
    check_rows(bones, want_bones, tol, f'({N},{J}) cap {max_blocks} bones')
    if world:
        # the root rows are the elements behind the last bone row, in the same workgroups: compared on their own, against values
        # no bone row holds
        tol_root = angle_tolerance(ops._carla_row(wloc, wrot), want_root, f'({N},{J}) root')
        assert root.shape == (N, 6) and root.dtype == torch.float32
        check_rows(root, want_root, tol_root, f'({N},{J}) cap {max_blocks} root')
        alone, _ = ops.carla_pose_export(loc, rot, max_blocks=max_blocks)
        assert torch.equal(alone, bones)                               # the bone rows do not depend on the root rows being there
    else:
        assert root is None
    again, _ = ops.carla_pose_export(loc, rot, max_blocks=max_blocks)
    assert torch.equal(again, bones)                                   # one writer per element, nothing reduced
    if max_blocks:
        full, full_root = ops.carla_pose_export(loc, rot, wloc if world else None, wrot if world else None)
        assert torch.equal(full, bones) and (not world or torch.equal(full_root, root))     # the grid does not change a bit


@pytest.mark.parametrize('N,J,max_blocks', SHAPES)
def test_import_matches_the_fp64_definition(N, J, max_blocks, monkeypatch):
    _, _, rows32, want_loc, want_rot = reference(N, J)
    rows = rows32.to(dev())
    with monkeypatch.context() as m:
        m.setenv('P2C_CARLA_FRAMEWORK', '1')
        fw_loc, fw_rot = ops.carla_pose_import(rows)
    err_fw = float((fw_rot.double().cpu() - want_rot).abs().max())
    tol = max(4 * err_fw, MATRIX_FLOOR)
    loc, rot = ops.carla_pose_import(rows, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert loc.shape == (N, J, 3) and rot.shape == (N, J, 3, 3) and rot.dtype == torch.float32
    err = float((rot.double().cpu() - want_rot).abs().max())
    print(f'({N},{J}) cap {max_blocks} inverse: tensor restatement {err_fw:.3e}, K30 {err:.3e} from fp64 (allowed {tol:.3e})')
    assert torch.equal(loc.double().cpu(), want_loc) and torch.equal(fw_loc.double().cpu(), want_loc)
    assert math.isfinite(err) and err <= tol
    assert torch.equal(ops.carla_pose_import(rows)[1], rot)


@pytest.mark.parametrize('N,J,max_blocks', SHAPES)
def test_import_of_export_gives_the_matrices_back(N, J, max_blocks):
    loc, rot, _, _ = (t.to(dev()) for t in problem(N, J))
    want_bones, *_ = reference(N, J)
    bones, _ = ops.carla_pose_export(loc, rot, max_blocks=max_blocks)
    loc2, rot2 = ops.carla_pose_import(bones, max_blocks=max_blocks)
    # forward angle error (as allowed above) carried into the entries, the inverse's own allowance, and the fp32 rounding of the inputs
    tol_deg = angle_tolerance(ops._carla_row(loc, rot), want_bones, f'({N},{J})')
    tol = 3 * math.radians(tol_deg) + MATRIX_FLOOR + INPUT_ROUNDING
    err = float((rot2 - rot).abs().max())
    print(f'({N},{J}) inv(fwd(R)) - R: {err:.3e} (allowed {tol:.3e})')
    assert torch.equal(loc2, loc) and math.isfinite(err) and err <= tol


def test_views_give_the_bits_of_their_contiguous_copies():
    N, J = 6, 27
    loc, rot, wloc, wrot = (t.to(dev()) for t in problem(N, J))
    vloc, vrot = loc[:, 1:], rot[:, 1:]                                        # the flow's eval_slice views look like this
    assert not vloc.is_contiguous() and not vrot.is_contiguous()
    wl, wr = wloc.reshape(2, 3, 3)[:, 1:], wrot.reshape(2, 3, 3, 3)[:, 1:]
    lead_loc, lead_rot = loc.reshape(2, 3, J, 3)[:, 1:], rot.reshape(2, 3, J, 3, 3)[:, 1:]
    assert not wl.is_contiguous() and not lead_rot.is_contiguous()
    bones, _ = ops.carla_pose_export(vloc, vrot)
    want, _ = ops.carla_pose_export(vloc.contiguous(), vrot.contiguous())
    assert bones.shape == (N, J - 1, 6) and torch.equal(bones, want)
    b2, r2 = ops.carla_pose_export(lead_loc, lead_rot, wl, wr)
    w2, wr2 = ops.carla_pose_export(lead_loc.contiguous(), lead_rot.contiguous(), wl.contiguous(), wr.contiguous())
    assert b2.shape == (2, 2, J, 6) and r2.shape == (2, 2, 6) and torch.equal(b2, w2) and torch.equal(r2, wr2)
    rows = want.reshape(N, J - 1, 6)
    il, ir = ops.carla_pose_import(rows[:, 1:])
    cl, cr = ops.carla_pose_import(rows[:, 1:].contiguous())
    assert torch.equal(il, cl) and torch.equal(ir, cr)


def test_nan_rows_stay_nan_and_touch_nothing_else():
    N, J = 5, 26
    loc, rot, wloc, wrot = (t.to(dev()).clone() for t in problem(N, J))
    clean, clean_root = ops.carla_pose_export(loc, rot, wloc, wrot)
    holes = [(0, 0), (1, 25), (2, 12), (4, 25)]                                # the 64th element is (2, 12): a wavefront's first lane
    for n, j in holes:
        loc[n, j] = float('nan')
        rot[n, j] = float('nan')
    wloc[3] = float('nan')
    wrot[3] = float('nan')
    bones, root = ops.carla_pose_export(loc, rot, wloc, wrot)
    mask = torch.zeros(N, J, dtype=torch.bool, device=dev())
    for n, j in holes:
        mask[n, j] = True
    assert torch.isnan(bones[mask]).all() and torch.equal(bones[~mask], clean[~mask])
    assert torch.isnan(root[3]).all() and torch.equal(root[[0, 1, 2, 4]], clean_root[[0, 1, 2, 4]])
    back_loc, back_rot = ops.carla_pose_import(bones)
    clean_loc, clean_rot = ops.carla_pose_import(clean)
    assert torch.isnan(back_loc[mask]).all() and torch.isnan(back_rot[mask]).all()
    assert torch.equal(back_loc[~mask], clean_loc[~mask]) and torch.equal(back_rot[~mask], clean_rot[~mask])


def test_clamp_one_ulp_outside():
    rot = torch.eye(3).repeat(3, 1, 1)
    for row, sign in ((1, 1.0), (2, -1.0)):
        rot[row] = torch.tensor([[0.0, 0.0, sign * (1.0 + 2.0 ** -23)], [0.0, 1.0, 0.0], [-sign, 0.0, 0.0]])
    assert float(rot[1, 0, 2]) > 1.0 and float(rot[2, 0, 2]) < -1.0
    bones, _ = ops.carla_pose_export(torch.zeros(3, 3, device=dev()), rot.to(dev()))
    bones = bones.cpu()
    assert torch.isfinite(bones).all()
    assert abs(float(bones[1, 3]) + 90.0) <= ANGLE_FLOOR_DEG and abs(float(bones[2, 3]) - 90.0) <= ANGLE_FLOOR_DEG
    assert float(bones[0, 3:].abs().max()) == 0.0


def test_framework_switch_takes_the_tensor_path(monkeypatch):
    N, J = 5, 26
    loc, rot, wloc, wrot = (t.to(dev()) for t in problem(N, J))
    want_bones, want_root, *_ = reference(N, J)
    monkeypatch.setenv('P2C_CARLA_FRAMEWORK', '1')
    assert ops.carla_framework()
    bones, root = ops.carla_pose_export(loc, rot, wloc, wrot)
    assert bones.is_cuda and torch.equal(bones, ops._carla_row(loc, rot)) and torch.equal(root, ops._carla_row(wloc, wrot))
    monkeypatch.setenv('P2C_CARLA_FRAMEWORK', '0')
    kernel, kernel_root = ops.carla_pose_export(loc, rot, wloc, wrot)
    tol = angle_tolerance(bones, want_bones, 'framework switch')
    check_rows(kernel, want_bones, tol, 'K30')
    check_rows(bones, want_bones, tol, 'tensor path')
    check_rows(kernel_root, want_root, angle_tolerance(root, want_root, 'framework switch, root'), 'K30 root')
    # fp64 and autocast stay on the tensor path whatever the switch says
    d64, _ = ops.carla_pose_export(loc.double(), rot.double())
    assert d64.dtype == torch.float64 and d64.is_cuda and float((d64.cpu() - want_bones).abs().max()) <= 1e-9


def test_abi_refusals_come_before_any_launch():
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    loc, rot, wloc, wrot = (t.to(dev()) for t in problem(3, 5))
    bones, root = torch.zeros(3, 5, 6, device=dev()), torch.zeros(3, 6, device=dev())
    p = lambda t: t.data_ptr()                                                  # noqa: E731
    fwd, inv = lib.p2c_carla_pose_fwd, lib.p2c_carla_pose_inv
    assert fwd(p(loc), p(rot), None, None, p(bones), None, -1, 5, 0, None) == -2
    assert fwd(p(loc), p(rot), None, None, p(bones), None, 3, 0, 0, None) == -2
    assert fwd(p(loc), p(rot), None, None, p(bones), None, 3, 5, -1, None) == -2
    assert fwd(None, p(rot), None, None, p(bones), None, 3, 5, 0, None) == -1
    assert fwd(p(loc), p(rot), p(wloc), None, p(bones), p(root), 3, 5, 0, None) == -1      # one world input without the other
    assert fwd(p(loc), p(rot), None, p(wrot), p(bones), p(root), 3, 5, 0, None) == -1
    assert fwd(p(loc), p(rot), p(wloc), p(wrot), p(bones), None, 3, 5, 0, None) == -1
    assert inv(p(bones), None, p(rot), 3, 5, 0, None) == -1 and inv(p(bones), p(loc), p(rot), 3, -2, 0, None) == -2
    assert fwd(p(loc), p(rot), None, None, p(bones), None, 0, 5, 0, None) == 0 and inv(p(bones), p(loc), p(rot), 0, 5, 0, None) == 0
    torch.cuda.synchronize()
    assert float(bones.abs().sum()) == 0.0 and float(root.abs().sum()) == 0.0
    # without world inputs the root buffer is not written even when one is passed
    assert fwd(p(loc), p(rot), None, None, p(bones), p(root), 3, 5, 0, None) == 0
    torch.cuda.synchronize()
    assert float(root.abs().sum()) == 0.0 and float(bones.abs().sum()) > 0.0


def wrapped(a, b):
    """Difference of angles in degrees as rotations: 179.99 and -179.99 are 0.02 apart."""
    return (a - b + 180.0) % 360.0 - 180.0


def test_device_flow_to_animation_file_end_to_end(tmp_path, monkeypatch):
    """LitPoseLiftingFlow(LinearAE) on the device, B = 4, T = 4 -> Trainer.predict -> save_carla_animation, against the host run of
    the same parameters (the host flow of tests/test_carla_pose.py). The tolerance is formed as everywhere in this file: the
    run with the fp32 tensor restatement of the export on the device (P2C_CARLA_FRAMEWORK=1) is measured against the host run,
    and the K30 run is allowed four times that, floor 1e-4 degree (here the measured part holds what the fp32 model and pose
    head on the device differ from the host's, which both device runs share). Angles are compared as rotations (modulo 360)."""
    from pedestrians_video_2_carla_amd.data.carla.animation import load_carla_animation, save_carla_animation
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    seed_everything(11)
    B, T = 4, 4
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B)
    flow = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
                              loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    trainer = Trainer(max_steps=1, device=dev()).setup(flow, dm)
    batch = dm.generate_batch(dev())
    frames, targets, meta = batch

    host_model = LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON)
    host_model.load_state_dict({k: v.detach().cpu().clone() for k, v in flow.movements_model.state_dict().items()})
    host = host_flow(host_model)
    host_meta = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in meta.items()}
    host_batch = (frames.cpu(), {k: v.cpu() for k, v in targets.items()}, host_meta)
    want = load_carla_animation(save_carla_animation(str(tmp_path / 'host'), Trainer().predict(host, [host_batch])))

    outputs = trainer.predict(flow, [batch])
    assert flow.training
    sliced = outputs[0][0]
    assert sliced['relative_pose_rot'].is_cuda and sliced['relative_pose_rot'].shape == (B, T, 26, 3, 3)
    got = load_carla_animation(save_carla_animation(str(tmp_path / 'device'), outputs, fps=30.0))
    with monkeypatch.context() as m:
        m.setenv('P2C_CARLA_FRAMEWORK', '1')
        fw = load_carla_animation(save_carla_animation(str(tmp_path / 'framework'), trainer.predict(flow, [batch])))
    assert got['bones'].shape == (B, T, 26, 6) and got['root'].shape == (B, T, 6)
    assert got['bone_names'] == want['bone_names'] and got['age'] == want['age'] and got['gender'] == want['gender']
    for key in ('bones', 'root'):
        g, f, w = (np.asarray(x[key], dtype=np.float64) for x in (got, fw, want))
        err_fw = float(np.abs(wrapped(f[..., 3:], w[..., 3:])).max())
        err = float(np.abs(wrapped(g[..., 3:], w[..., 3:])).max())
        tol = max(4 * err_fw, ANGLE_FLOOR_DEG)
        loc_fw = float(np.abs(f[..., :3] - w[..., :3]).max())
        loc_err = float(np.abs(g[..., :3] - w[..., :3]).max())
        loc_tol = max(4 * loc_fw, 1e-6 * float(np.abs(w[..., :3]).max()))
        print(f'{key}: tensor-path run {err_fw:.3e} degree / {loc_fw:.3e} m from the host run; K30 run {err:.3e} (allowed {tol:.3e}) / '
              f'{loc_err:.3e} (allowed {loc_tol:.3e})')
        assert math.isfinite(err) and err <= tol and loc_err <= loc_tol, key
        assert np.array_equal(g[..., :3], f[..., :3])                           # same device outputs, exact copy either way
    # and K30 itself: the file against the fp64 definition on the very tensors the predict step left on the device
    b64, r64 = ops.carla_pose_export(sliced['relative_pose_loc'].double().cpu(), sliced['relative_pose_rot'].double().cpu(),
                                     sliced['world_loc'].double().cpu(), sliced['world_rot'].double().cpu())
    fb, fr = ops._carla_row(sliced['relative_pose_loc'], sliced['relative_pose_rot']), ops._carla_row(sliced['world_loc'], sliced['world_rot'])
    for name, g, f, w in (('bones', got['bones'], fb, b64), ('root', got['root'], fr, r64)):
        err_fw = float(wrapped(f.double().cpu()[..., 3:], w[..., 3:]).abs().max())
        err = float(wrapped(torch.from_numpy(g).double()[..., 3:], w[..., 3:]).abs().max())
        tol = max(4 * err_fw, ANGLE_FLOOR_DEG)
        print(f'{name} of the device outputs: tensor restatement {err_fw:.3e}, K30 {err:.3e} degree from fp64 (allowed {tol:.3e})')
        assert err <= tol and np.array_equal(g[..., :3], w[..., :3].numpy().astype(np.float32))
