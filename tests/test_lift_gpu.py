"""GPU: K32 (csrc/p2c_lift.hip, ``ops.lift_to_carla``) against the composed path it replaces -- ``ops.fused_mlp`` (K8) -> the
materialising pose head -> ``ops.carla_pose_export`` (K30), which ``P2C_LIFT_FRAMEWORK=1`` runs -- on the same device tensors.

The criterion is bit equality, as for K13 (tests/test_train_fused_gpu.py): the kernel runs the same device functions on the same
operands in the same order (fp32 MFMA chains in k order per frame column, ``rot6d_fwd``, the sequential 3x3 product, the row
arithmetic of K30), so nothing may differ. With ``initial_rel_rot`` the composed path cannot use the pose head's own product (it
starts every clip from the reference pose): it multiplies the pose head's ``pose_changes`` up again with ``ops._mul3_fma``, the
fp32 restatement of that product's fmaf order (pinned on the host in tests/test_lift.py)."""
import copy
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
from pedestrians_video_2_carla_amd.walker_control.carla_lifter import CarlaLifter

pytestmark = pytest.mark.gpu

KINDS = {'pose_changes_6d': 'pose_changes', 'relative_rot_6d': 'relative_rot'}
# (B, T, max_blocks): one frame; a partial tile; a full tile; a carry across a tile boundary with a 1-frame tail; three tiles;
# two workgroups striding over five clips, uneven; more clips than frames
SHAPES = [(1, 1, 0), (1, 5, 0), (1, 16, 0), (1, 17, 0), (3, 33, 0), (5, 16, 2), (40, 4, 0)]


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def trained_model(kind):
    """LinearAE after ``seed_everything`` and a few AdamW steps towards random 6-D targets: rotations far from the identity."""
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(17)
    model = LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=KINDS[kind]).to(dev())
    model.rotation_output_format = 'rotation_6d'
    opt = torch.optim.AdamW(model.parameters(), lr=3e-2)
    x, target = torch.randn(8, 16, 26, 2, device=dev()), torch.randn(8, 16, 26, 6, device=dev())
    for _ in range(5):
        opt.zero_grad()
        ((model(x) - target) ** 2).mean().backward()
        opt.step()
    return model.eval()


def params_of(model):
    layers = model._linears()
    return [m.weight.detach() for m in layers], [m.bias.detach() for m in layers]


@functools.lru_cache(maxsize=None)
def problem(B, T):
    """frames, skeleton types (all four from B = 4 on, mixed below), world transforms, a random proper rotation per joint."""
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import rotation_6d_to_matrix
    g = torch.Generator().manual_seed(1000 * B + T)
    frames = torch.randn(B, T, 26, 2, generator=g)
    skel_type = torch.tensor([(3 * b + 2) % 4 for b in range(B)], dtype=torch.int32)
    world_loc = torch.randn(B, T, 3, generator=g)
    world_rot = rotation_6d_to_matrix(torch.randn(B, T, 6, generator=g))
    initial = rotation_6d_to_matrix(torch.randn(B, 26, 6, generator=g))
    assert float((torch.linalg.det(initial) - 1).abs().max()) < 1e-5
    return tuple(t.to(dev()) for t in (frames, skel_type, world_loc, world_rot, initial))


def run(kind, B, T, max_blocks=0, world=False, init=False, framework=False, **kw):
    frames, skel_type, world_loc, world_rot, initial = problem(B, T)
    weights, biases = params_of(trained_model(kind))
    before = os.environ.get('P2C_LIFT_FRAMEWORK')
    os.environ['P2C_LIFT_FRAMEWORK'] = '1' if framework else '0'
    try:
        return ops.lift_to_carla(frames, weights, biases, skel_type, kind, world_loc=world_loc if world else None,
                                 world_rot=world_rot if world else None, initial_rel_rot=initial if init else None,
                                 want_rot=True, max_blocks=max_blocks, **kw)
    finally:
        if before is None:
            del os.environ['P2C_LIFT_FRAMEWORK']
        else:
            os.environ['P2C_LIFT_FRAMEWORK'] = before


@functools.lru_cache(maxsize=None)
def composed(kind, B, T, max_blocks, world, init):
    """The three separate calls, once per case."""
    return run(kind, B, T, max_blocks, world, init, framework=True)


def same_bits(a, b):
    """torch.equal that also holds for equal NaNs."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('init', [False, True], ids=['reference-start', 'initial'])
@pytest.mark.parametrize('world', [False, True], ids=['identity-world', 'world'])
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('B,T,max_blocks', SHAPES)
def test_one_launch_carries_the_bits_of_the_three_calls(B, T, max_blocks, kind, world, init):
    want_bones, want_root, want_final, want_rot = composed(kind, B, T, max_blocks, world, init)
    bones, root, final, rot = run(kind, B, T, max_blocks, world, init)
    torch.cuda.synchronize()
    assert bones.shape == (B, T, 26, 6) and root.shape == (B, T, 6) and rot.shape == (B, T, 26, 3, 3)
    assert torch.isfinite(bones).all() and torch.isfinite(rot).all()
    if B >= 4:
        assert sorted(set(problem(B, T)[1].tolist())) == [0, 1, 2, 3]
    assert torch.equal(rot, want_rot), 'out_relative_pose_rot'
    if not init or kind == 'relative_rot_6d':              # the pose head's own tensor
        frames, skel_type, *_ = problem(B, T)
        weights, biases = params_of(trained_model(kind))
        y = ops.fused_mlp(frames.view(B * T, 52), weights, biases).view(B, T, 26, 6)
        _, outs = ops.pose_head(y, ops.PoseHeadSpec(kind=kind, transform='none'), skel_type, want=('relative_pose_rot',))
        assert torch.equal(rot, outs['relative_pose_rot']), 'relative_pose_rot of the pose head'
    assert torch.equal(bones, want_bones), 'bones'
    assert torch.equal(root, want_root), 'root'
    if kind == 'pose_changes_6d':
        assert torch.equal(final, want_final) and torch.equal(final, rot[:, -1]), 'final_rel_rot'
    else:
        assert final is None and want_final is None
    # one writer per element, nothing reduced: a second run and another grid give the same bits
    again = run(kind, B, T, 1 if B > 1 else 0, world, init)
    assert torch.equal(again[0], bones) and torch.equal(again[1], root) and torch.equal(again[3], rot)
    # the rotations are rotations, and differ from the reference pose
    eye = torch.eye(3, device=dev())
    assert float((rot @ rot.transpose(-1, -2) - eye).abs().max()) < 1e-4


def test_carry_over_two_halves_is_the_uncut_clip():
    """T = 16 as 8 + 8, ``final_rel_rot`` handed to ``initial_rel_rot``: the bits of the composed path on the uncut clip."""
    kind, B, T = 'pose_changes_6d', 5, 16
    frames, skel_type, world_loc, world_rot, _ = problem(B, T)
    weights, biases = params_of(trained_model(kind))
    want_bones, want_root, want_final, want_rot = composed(kind, B, T, 0, True, False)
    first = ops.lift_to_carla(frames[:, :8], weights, biases, skel_type, kind, world_loc=world_loc[:, :8],
                              world_rot=world_rot[:, :8], want_rot=True)
    second = ops.lift_to_carla(frames[:, 8:], weights, biases, skel_type, kind, world_loc=world_loc[:, 8:],
                               world_rot=world_rot[:, 8:], initial_rel_rot=first[2], want_rot=True)
    assert torch.equal(torch.cat((first[0], second[0]), 1), want_bones)
    assert torch.equal(torch.cat((first[1], second[1]), 1), want_root)
    assert torch.equal(torch.cat((first[3], second[3]), 1), want_rot) and torch.equal(second[2], want_final)
    # and the lifter's push does the same
    lifter = CarlaLifter(trained_model(kind))
    a = lifter.push(frames[:, :8], skel_type, world_loc[:, :8], world_rot[:, :8])
    b = lifter.push(frames[:, 8:], skel_type, world_loc[:, 8:], world_rot[:, 8:])
    assert torch.equal(torch.cat((a[0], b[0]), 1), want_bones) and torch.equal(torch.cat((a[1], b[1]), 1), want_root)
    lifter.reset()
    assert torch.equal(lifter.push(frames[:, :8], skel_type)[0], want_bones[:, :8])
    lifter.close()


def test_prepacked_image_and_repacking_after_a_weight_change():
    kind, B, T = 'pose_changes_6d', 3, 33
    frames, skel_type, *_ = problem(B, T)
    want = composed(kind, B, T, 0, False, False)
    model = copy.deepcopy(trained_model(kind))
    weights, biases = params_of(model)
    image = torch.empty(ops.mlp_image_layout(ops.LINEAR_AE_6D_DIMS)[0], device=dev())
    ops.mlp_pack(weights, biases, image)
    got = ops.lift_to_carla(frames, weights, biases, skel_type, kind, image=image, image_is_current=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    stale = torch.zeros_like(image)                          # not current: packed inside the call
    got = ops.lift_to_carla(frames, weights, biases, skel_type, kind, image=stale, image_is_current=False)
    assert torch.equal(got[0], want[0]) and torch.equal(stale, image)
    with pytest.raises(RuntimeError):
        ops.lift_to_carla(frames, weights, biases, skel_type, kind, image=image[:-4], image_is_current=True)
    # the lifter: one pack, none for the next clip, one more after an in-place change
    lifter = CarlaLifter(model)
    bones, _ = lifter.lift(frames, skel_type)
    assert torch.equal(bones, want[0]) and lifter.packs == 1
    assert torch.equal(lifter.lift(frames, skel_type)[0], want[0]) and lifter.packs == 1
    with torch.no_grad():
        model._linears()[-1].weight.mul_(0.5)
        model._linears()[0].bias.add_(0.25)
    changed, _ = lifter.lift(frames, skel_type)
    assert lifter.packs == 2 and not torch.equal(changed, want[0])
    os.environ['P2C_LIFT_FRAMEWORK'] = '1'
    try:
        new_want = ops.lift_to_carla(frames, *params_of(model), skel_type, kind)
    finally:
        del os.environ['P2C_LIFT_FRAMEWORK']
    assert torch.equal(changed, new_want[0])
    model.load_state_dict(trained_model(kind).state_dict())
    assert torch.equal(lifter.lift(frames, skel_type)[0], want[0]) and lifter.packs == 3
    lifter.close()


@pytest.mark.parametrize('kind', list(KINDS))
def test_a_nan_frame_stays_in_its_clip_and_padding_never_shows(kind, monkeypatch):
    """B = 3 clips of 21 frames (a full tile and a partial one with eleven padding columns), a NaN in the input of clip 1, frame
    4. The kernel runs under the two audit modes -- every LDS byte NaN before the launch (``P2C_POISON_LDS=1``) and NaN-filled
    ``torch.empty`` (``P2C_POISON_EMPTY=1``) -- so a padding column, an unwritten LDS row or an unwritten output element would
    show as NaN. Expected: the rows of the other clips and of clip 1 before frame 4 carry the bits of the clean run; for
    pose_changes frame 4 and every later frame of clip 1 differ from it (the running product passes through frame 4), for
    relative_rot frame 4 alone; and everything carries the bits of the composed path on the same input. (Whether the NaN arrives
    as a NaN is the model's business: the layers' ReLU is fmaxf(v, 0), which answers 0 for a NaN, as in K8.)"""
    B, T, b0, t0 = 3, 21, 1, 4
    frames, skel_type, world_loc, world_rot, _ = problem(B, T)
    weights, biases = params_of(trained_model(kind))
    clean = run(kind, B, T, 0, True, False)
    bad = frames.clone()
    bad[b0, t0, 7, 1] = float('nan')
    monkeypatch.setenv('P2C_LIFT_FRAMEWORK', '1')
    want = ops.lift_to_carla(bad, weights, biases, skel_type, kind, world_loc=world_loc, world_rot=world_rot, want_rot=True)
    monkeypatch.setenv('P2C_LIFT_FRAMEWORK', '0')
    monkeypatch.setenv('P2C_POISON_LDS', '1')
    monkeypatch.setenv('P2C_POISON_EMPTY', '1')
    monkeypatch.setattr(_lib, '_lib', None)                  # the next lib() wraps every launch with the LDS poisoning
    deterministic, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    monkeypatch.setattr(torch.utils.deterministic, 'fill_uninitialized_memory', True)
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert isinstance(_lib.lib(), _lib._PoisonedLib) and bool(torch.isnan(torch.empty(8, device=dev())).all())
        got = ops.lift_to_carla(bad, weights, biases, skel_type, kind, world_loc=world_loc, world_rot=world_rot, want_rot=True)
        got_clean = ops.lift_to_carla(frames, weights, biases, skel_type, kind, world_loc=world_loc, world_rot=world_rot,
                                      want_rot=True)
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(deterministic, warn_only=warn_only)
    for i in (0, 1, 3):
        assert same_bits(got_clean[i], clean[i]) and torch.isfinite(got_clean[i]).all()
        assert same_bits(got[i], want[i]), ('bones', 'root', 'final', 'rot')[i]
    touched = torch.zeros(B, T, dtype=torch.bool, device=dev())
    touched[b0, t0:] = True
    if kind == 'relative_rot_6d':
        touched[b0, t0 + 1:] = False
    differs = (got[0].view(torch.int32) != clean[0].view(torch.int32)).flatten(2).any(-1)
    assert torch.equal(differs, touched), differs.nonzero().tolist()
    rot_differs = (got[3].view(torch.int32) != clean[3].view(torch.int32)).flatten(2).any(-1)
    assert torch.equal(rot_differs, touched)
    assert same_bits(got[1], clean[1])                       # the root rows never meet the model
    if kind == 'pose_changes_6d':
        assert same_bits(got[2], want[2])
        assert same_bits(got[2][[0, 2]], clean[2][[0, 2]]) and not same_bits(got[2][b0], clean[2][b0])
    # a NaN in the world transform of one frame reaches that frame's root row and nothing else
    wl = world_loc.clone()
    wl[2, 20, 0] = float('nan')
    got = ops.lift_to_carla(frames, weights, biases, skel_type, kind, world_loc=wl, world_rot=world_rot)
    assert torch.equal(got[0], clean[0]) and bool(torch.isnan(got[1][2, 20, 0]))
    ok = torch.ones(B, T, dtype=torch.bool, device=dev())
    ok[2, 20] = False
    assert torch.equal(got[1][ok], clean[1][ok]) and torch.equal(got[1][2, 20, 1:], clean[1][2, 20, 1:])


def test_framework_switch_takes_the_composed_path(monkeypatch):
    kind, B, T = 'pose_changes_6d', 5, 16
    frames, skel_type, *_ = problem(B, T)
    weights, biases = params_of(trained_model(kind))
    want = composed(kind, B, T, 0, False, False)

    def refuse(*a):
        raise AssertionError('p2c_lift_fwd was called')
    monkeypatch.setattr(_lib.lib(), 'p2c_lift_fwd', refuse, raising=False)
    with pytest.raises(AssertionError, match='p2c_lift_fwd was called'):
        ops.lift_to_carla(frames, weights, biases, skel_type, kind)
    monkeypatch.setenv('P2C_LIFT_FRAMEWORK', '1')
    assert ops.lift_framework()
    got = ops.lift_to_carla(frames, weights, biases, skel_type, kind, want_rot=True)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # fp64 on the device: the tensor definition, whatever the switch says
    monkeypatch.setenv('P2C_LIFT_FRAMEWORK', '0')
    d64 = ops.lift_to_carla(frames.double(), [w.double() for w in weights], [b.double() for b in biases], skel_type, kind)
    assert d64[0].dtype == torch.float64 and d64[0].is_cuda
    assert torch.equal(d64[0][..., :3].float(), want[0][..., :3])


def test_abi_refusals_come_before_any_launch():
    kind, B, T = 'pose_changes_6d', 3, 5
    lib = _lib.lib()
    frames, skel_type, world_loc, world_rot, initial = problem(B, T)
    weights, biases = params_of(trained_model(kind))
    image = torch.zeros(ops.mlp_image_layout(ops.LINEAR_AE_6D_DIMS)[0], device=dev())
    bones, root = torch.zeros(B, T, 26, 6, device=dev()), torch.zeros(B, T, 6, device=dev())
    final, rot = torch.zeros(B, 26, 3, 3, device=dev()), torch.zeros(B, T, 26, 3, 3, device=dev())

    def desc(**changes):
        d = ops._lift_desc(frames.view(B, T, 52), weights, biases, skel_type, kind, image, False, world_loc, world_rot, initial,
                           bones, root, final, rot)
        for k, v in changes.items():
            if k.startswith('mlp_'):
                setattr(d.mlp, k[4:], v)
            else:
                setattr(d, k, v)
        return d

    def call(**changes):
        return lib.p2c_lift_fwd(ctypes.byref(desc(**changes)), None)

    assert lib.p2c_lift_fwd(None, None) == -1
    for field in ('skel_type', 'ref_rel_loc', 'ref_rel_rot', 'bones', 'mlp_x', 'mlp_w_image'):
        assert call(**{field: None}) == -1, field
    assert call(world_loc=None) == -1 and call(world_rot=None) == -1          # a world pair given by half
    assert call(root=None) == -1                                              # world inputs with nowhere to put their rows
    d = desc()
    d.mlp.W[3] = None
    assert lib.p2c_lift_fwd(ctypes.byref(d), None) == -1                      # weights are read by the pack launch
    for k in (1, 3, 4, 7, -1):
        assert call(kind=k) == -3, k
    assert call(mlp_precision=1) == -3
    assert call(B=-1) == -2 and call(T=-1) == -2 and call(max_blocks=-1) == -2 and call(mlp_N=B * T + 1) == -2
    d = desc()
    d.mlp.dims[0] = 50
    assert lib.p2c_lift_fwd(ctypes.byref(d), None) == -2 and lib.p2c_lift_supported(ctypes.byref(d)) == 0
    assert lib.p2c_lift_supported(ctypes.byref(desc())) == 1 and lib.p2c_lift_supported(ctypes.byref(desc(kind=4))) == 0
    assert call(B=0, mlp_N=0) == 0 and call(T=0, mlp_N=0) == 0
    torch.cuda.synchronize()
    for t in (image, bones, root, final, rot):                                # nothing ran: not even the pack launch
        assert float(t.abs().sum()) == 0.0
    assert call() == 0
    torch.cuda.synchronize()
    assert float(bones.abs().sum()) > 0.0 and float(image.abs().sum()) > 0.0
    # without world inputs a root buffer gets the identity world's rows; without a root buffer nothing is written there
    root.fill_(7.0)
    assert call(world_loc=None, world_rot=None) == 0
    torch.cuda.synchronize()
    assert float(root.abs().max()) == 0.0
    assert call(world_loc=None, world_rot=None, root=None, final_rel_rot=None, out_relative_pose_rot=None) == 0
    torch.cuda.synchronize()


def test_animation_file_end_to_end(tmp_path, monkeypatch):
    """LitPoseLiftingFlow(LinearAE) on the device, B = 4, T = 4: ``lift_carla_animation`` writes the arrays of
    ``save_carla_animation(trainer.predict(...))``. Against the host run of the same parameters the tolerance is formed as in
    test_device_flow_to_animation_file_end_to_end: what the composed device run is from the host run is measured, and K32,
    which must carry the composed run's bits, gets that value."""
    from pedestrians_video_2_carla_amd.data.carla.animation import lift_carla_animation, load_carla_animation, save_carla_animation
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    from test_carla_pose import host_flow
    from test_carla_pose_gpu import wrapped
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

    composed_run = load_carla_animation(save_carla_animation(str(tmp_path / 'composed'), trainer.predict(flow, [batch]), fps=30.0))

    def refuse(*a):
        raise AssertionError('the composed path ran')
    with monkeypatch.context() as m:
        m.setattr(ops, 'pose_head', refuse)
        m.setattr(ops, 'carla_pose_export', refuse)
        got = load_carla_animation(lift_carla_animation(str(tmp_path / 'lift'), flow, [batch], fps=30.0))
    assert flow.training
    assert got['bones'].shape == (B, T, 26, 6) and got['root'].shape == (B, T, 6)
    assert np.array_equal(got['bones'], composed_run['bones']) and np.array_equal(got['root'], composed_run['root'])
    for key in ('bone_names', 'age', 'gender', 'fps'):
        assert got[key] == composed_run[key] == want[key], key
    for key in ('bones', 'root'):
        g, c, w = (np.asarray(x[key], dtype=np.float64) for x in (got, composed_run, want))
        tol = float(np.abs(wrapped(c[..., 3:], w[..., 3:])).max())
        err = float(np.abs(wrapped(g[..., 3:], w[..., 3:])).max())
        loc_tol, loc_err = float(np.abs(c[..., :3] - w[..., :3]).max()), float(np.abs(g[..., :3] - w[..., :3]).max())
        print(f'{key}: composed device run {tol:.3e} degree / {loc_tol:.3e} m from the host run; K32 run {err:.3e} / {loc_err:.3e}')
        assert np.isfinite(err) and err <= tol and loc_err <= loc_tol, key
    out = trainer.predict_carla(flow, [batch])
    assert len(out) == 1 and out[0][0].is_cuda and out[0][2] is meta and flow.training
