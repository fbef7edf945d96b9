"""K32 (csrc/p2c_lift.hip, ``ops.lift_to_carla``, ``CarlaLifter``) -- what runs without a GPU: the C-ABI surface, the definition on
host tensors against the oracle's pose head, the carry between clips and the fall-back for models the kernel does not cover."""
import ctypes
import os
import re
import subprocess
import warnings

import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
from pedestrians_video_2_carla_amd.walker_control.carla_lifter import CarlaLifter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {'pose_changes_6d': 'pose_changes', 'relative_rot_6d': 'relative_rot'}


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_lift_symbols_are_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    lib = _lib.lib()
    for name in ('p2c_lift_supported', 'p2c_lift_fwd'):
        assert name in declared and name in _lib.SYMBOLS
        assert getattr(lib, name) is not None
    res, args = _lib.SYMBOLS['p2c_lift_fwd']
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p          # the stream goes last: the LDS-poison audit wraps the call
    assert 'p2c_lift_fwd' in _lib._PoisonedLib(lib)._wrap and 'p2c_lift_supported' not in _lib._PoisonedLib(lib)._wrap
    assert ops.lift_supported(ops.LINEAR_AE_6D_DIMS)
    for dims in ((50, 25, 12, 6, 39, 78, 156), (52, 26, 13, 6, 19, 39, 78), (52, 26, 156), (52,)):
        assert not ops.lift_supported(dims), dims


def test_lift_descriptor_layout_matches_the_header(tmp_path):
    """``LiftDesc`` against ``p2c_lift_desc``: same size, same offset for every field (the embedded ``p2c_mlp_desc`` has its own
    check in test_host_logic.py)."""
    fields = [f[0] for f in _lib.LiftDesc._fields_]
    body = '\n'.join(f'  printf("{f} %zu\\n", offsetof(p2c_lift_desc, {f}));' for f in fields)
    src = tmp_path / 'lift_desc.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(p2c_lift_desc));\n' + body + '\n  return 0;\n}\n')
    exe = tmp_path / 'lift_desc'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.strip().splitlines())
    assert int(out['sizeof']) == ctypes.sizeof(_lib.LiftDesc)
    for f in fields:
        assert int(out[f]) == getattr(_lib.LiftDesc, f).offset, f
    assert _lib.LiftDesc.mlp.size == ctypes.sizeof(_lib.MlpDesc)


# ------------------------------------------------------------------------------------------------- host definition
def host_model(kind, dtype, seed=0, input_nodes=CARLA_SKELETON):
    torch.manual_seed(seed)
    model = LinearAE(input_nodes=input_nodes, output_nodes=CARLA_SKELETON, movements_output_type=KINDS[kind]).to(dtype)
    with torch.no_grad():                                   # away from the near-identity rotations of the default init
        for p in model.parameters():
            p.add_(0.3 * torch.randn(p.shape, dtype=dtype))
    return model


def params_of(model):
    layers = model._linears()
    return [m.weight for m in layers], [m.bias for m in layers]


def host_problem(B, T, dtype, seed=1, joints=26):
    g = torch.Generator().manual_seed(seed)
    frames = torch.randn(B, T, joints, 2, generator=g, dtype=dtype)
    skel_type = torch.tensor([(3 * b + 1) % 4 for b in range(B)], dtype=torch.int32)
    world_loc = torch.randn(B, T, 3, generator=g, dtype=dtype)
    world_rot = ops.carla_pose_import(torch.cat((torch.zeros(B, T, 1, 3, dtype=dtype),
                                                 160 * torch.rand(B, T, 1, 3, generator=g, dtype=dtype) - 80), -1))[1][:, :, 0]
    return frames, skel_type, world_loc, world_rot


def identity_world(B, T, dtype):
    return torch.zeros(B, T, 3, dtype=dtype), torch.eye(3, dtype=dtype).expand(B, T, 3, 3).contiguous()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('kind', list(KINDS))
def test_host_lift_is_linear_ae_then_oracle_pose_head_then_export(kind, dtype):
    """B = 3, T = 5, skeleton types 1, 0, 3: ``ops.lift_to_carla`` on host tensors against the host LinearAE, the oracle's pose
    head and ``ops.carla_pose_export`` on host tensors. Both sides run the same tensor ops: equal bits wherever they start from
    the same values (see the note on the reference tables below)."""
    from oracle import pose_head as O
    B, T = 3, 5
    model = host_model(kind, dtype)
    model.rotation_output_format = 'rotation_6d'            # the raw network output, as the flows ask for it
    weights, biases = params_of(model)
    frames, skel_type, world_loc, world_rot = host_problem(B, T, dtype)
    assert sorted(skel_type.tolist()) == [0, 1, 3]
    with torch.no_grad():
        y = model(frames)
    assert y.shape == (B, T, 26, 6) and y.dtype == dtype
    o = O.pose_head(y, kind, skel_type, transform='none')
    # The oracle builds its reference rotations with torch's sin / cos, the package with numpy's: in fp64 one entry in a few is an
    # ulp apart (2^-53; in fp32 both round to the same value). So in fp64 the clip is started from the ORACLE's rows, handed over
    # as initial_rel_rot -- then both sides run the same tensor ops on the same values and the bits must agree -- and the start
    # from the package's own table is held to what a 2^-53 difference in R_0 can do to R_t = C R_0 with C a product of rotations:
    # each entry is a sum of three products with factors of magnitude <= 1, so 3 * 2^-53 on R_0 gives at most 9 * 2^-53 (1e-15).
    oracle_start = O.relative_tensors(dtype)[1][skel_type.long()]
    starts = [None] if dtype == torch.float32 else [oracle_start, None]
    for start in starts:
        exact = start is not None or dtype == torch.float32
        for wl, wr in ((world_loc, world_rot), (None, None)):
            want_bones, want_root = ops.carla_pose_export(o['relative_pose_loc'], o['relative_pose_rot'],
                                                          *((wl, wr) if wl is not None else identity_world(B, T, dtype)))
            bones, root, final, rot = ops.lift_to_carla(frames, weights, biases, skel_type, kind, world_loc=wl, world_rot=wr,
                                                        initial_rel_rot=start, want_rot=True)
            assert bones.dtype == dtype and bones.shape == (B, T, 26, 6) and root.shape == (B, T, 6)
            assert torch.equal(root, want_root)
            if exact or kind == 'relative_rot_6d':
                assert torch.equal(rot, o['relative_pose_rot'])
                assert torch.equal(bones, want_bones)
            else:
                err = float((rot - o['relative_pose_rot']).abs().max())
                print(f'fp64, package table against oracle table: relative rotations differ by {err:.3e} (allowed 1e-15)')
                assert err <= 1e-15
                assert torch.equal(bones[..., :3], want_bones[..., :3])
            if kind == 'pose_changes_6d':
                assert torch.equal(final, rot[:, -1])
            else:
                assert final is None
    assert ops.lift_to_carla(frames, weights, biases, skel_type, kind)[3] is None
    with pytest.raises(RuntimeError):
        ops.lift_to_carla(frames, weights, biases, skel_type, kind, world_loc=world_loc)
    with pytest.raises(RuntimeError):
        ops.lift_to_carla(frames, weights, biases, skel_type, 'absolute_loc')


def test_fmaf_restatement_is_exact():
    """``ops._fma32`` (the composed path's carry uses it to multiply in the kernels' order) against fp64-exact arithmetic on
    cases where rounding the fp64 sum to fp32 in two steps goes wrong: a product that ends exactly on an fp32 midpoint plus a
    summand far below it. Exact result by integer arithmetic on the scaled operands."""
    from fractions import Fraction
    import struct

    def f32(v):
        return struct.unpack('f', struct.pack('f', v))[0]

    def round_f32(q: Fraction) -> float:                    # nearest-even rounding of an exact rational to fp32 (normal range)
        lo = f32(float(q))
        cands = sorted({lo, f32(float(torch.nextafter(torch.tensor(lo), torch.tensor(float('inf'))))),
                        f32(float(torch.nextafter(torch.tensor(lo), torch.tensor(float('-inf')))))})
        best = min(cands, key=lambda c: (abs(Fraction(c) - q), struct.unpack('I', struct.pack('f', c))[0] & 1))
        return best

    cases = [(1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12, 2.0 ** -60), (1.0 + 2.0 ** -12, 1.0 + 2.0 ** -12, -2.0 ** -60),
             (3.0, 1.0 + 2.0 ** -23, 2.0 ** -70), (0.1, 0.2, 0.3), (-1.5, 2.0 ** -20, 1.0), (1e-3, -7.0, 7e-3)]
    g = torch.Generator().manual_seed(3)
    cases += [tuple(torch.randn(3, generator=g).tolist()) for _ in range(64)]
    a, b, c = (torch.tensor([f32(v[i]) for v in cases], dtype=torch.float32) for i in range(3))
    got = ops._fma32(a, b, c)
    for i in range(len(cases)):
        want = round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
        assert float(got[i]) == want, (cases[i], float(got[i]), want)
    m, r = torch.randn(4, 26, 3, 3, generator=g), torch.randn(4, 26, 3, 3, generator=g)
    assert float((ops._mul3_fma(m, r).double() - m.double() @ r.double()).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------------ the lifter
ANGLE_ULPS_DEG = 4 * 2.0 ** -45      # four ulps of an fp64 angle in [128, 256) degrees


def same_rows(got, want):
    """Locations are copies: equal. Angles within four ulps of 180 degrees in fp64, modulo 360: the host's asin / atan2 run a
    vector loop with a scalar tail, so the same operand may come out an ulp apart at another position of another shape."""
    if got.shape != want.shape or not torch.equal(got[..., :3], want[..., :3]):
        return False
    d = (got[..., 3:] - want[..., 3:]).abs()
    return bool((torch.minimum(d, 360.0 - d) <= ANGLE_ULPS_DEG).all())


@pytest.mark.parametrize('kind', list(KINDS))
def test_carry_over_a_cut_video_is_exact_given_the_model_output(kind):
    """The carry alone, bit for bit: 17 frames of one model output as 7 + 9 + 1 with ``final_rel_rot`` handed to
    ``initial_rel_rot`` give the relative rotations of the uncut clip -- the product over the frames is sequential, the same
    operations on the same operands in the same order either way."""
    B, T = 2, 17
    g = torch.Generator().manual_seed(9)
    y = torch.randn(B, T, 26, 6, generator=g)
    _, skel_type, world_loc, world_rot = host_problem(B, T, torch.float32, seed=6)
    _, _, whole_final, whole_rot = ops.pose_to_carla_rows(y, skel_type, kind, want_rot=True)
    carry, rots = None, []
    for a, b in ((0, 7), (7, 16), (16, 17)):
        _, _, carry, rot = ops.pose_to_carla_rows(y[:, a:b], skel_type, kind, initial_rel_rot=carry, want_rot=True)
        rots.append(rot)
    assert torch.equal(torch.cat(rots, 1), whole_rot)
    if kind == 'pose_changes_6d':
        assert torch.equal(carry, whole_final) and torch.equal(whole_final, whole_rot[:, -1])
        assert not torch.equal(ops.pose_to_carla_rows(y[:, 7:16], skel_type, kind, want_rot=True)[3], whole_rot[:, 7:16])
    else:
        assert carry is None and whole_final is None


@pytest.mark.parametrize('kind', list(KINDS))
def test_push_over_a_cut_video_equals_lift_of_the_whole(kind):
    """``CarlaLifter.push`` over 17 frames cut as 7 + 9 + 1 against the uncut pose head. fp64. The host's matrix products round
    differently for 14-, 18-, 2- and 34-row inputs, so the rows expected of the pushes are those of the UNCUT pose head on the
    model outputs of the three pieces put end to end: what is left between the two is the carry. ``lift`` of the whole clip is
    that on the whole clip's model output. ``reset`` puts the reference start back; a relative_rot model carries nothing."""
    B, T = 2, 17
    model = host_model(kind, torch.float64, seed=4)
    frames, skel_type, world_loc, world_rot = host_problem(B, T, torch.float64, seed=6)
    cuts = [(0, 7), (7, 16), (16, 17)]
    weights, biases = params_of(model)
    with torch.no_grad():
        y_cut = torch.cat([ops._linear_stack(frames[:, a:b].reshape(-1, 52), weights, biases).view(B, b - a, 26, 6) for a, b in cuts], 1)
    cut_bones, cut_root, _, _ = ops.pose_to_carla_rows(y_cut, skel_type, kind, world_loc, world_rot)
    lifter = CarlaLifter(model)
    assert lifter.supported and lifter.kind == KINDS[kind]
    whole_bones, whole_root = lifter.lift(frames, skel_type, world_loc, world_rot)
    want = ops.lift_to_carla(frames, weights, biases, skel_type, kind, world_loc=world_loc, world_rot=world_rot)
    assert whole_bones.shape == (B, T, 26, 6) and torch.equal(whole_bones, want[0]) and torch.equal(whole_root, want[1])
    parts = [lifter.push(frames[:, a:b], skel_type, world_loc[:, a:b], world_rot[:, a:b]) for a, b in cuts]
    assert same_rows(torch.cat([p[0] for p in parts], 1), cut_bones)
    assert same_rows(torch.cat([p[1] for p in parts], 1), cut_root)
    # without reset the next push continues the video; after it, the first clip comes out as at the start
    again = lifter.push(frames[:, :7], skel_type)[0]
    assert same_rows(again, cut_bones[:, :7]) == (kind == 'relative_rot_6d')
    lifter.reset()
    assert same_rows(lifter.push(frames[:, :7], skel_type)[0], cut_bones[:, :7])
    # lift is stateless: it neither reads nor moves the carry
    assert torch.equal(lifter.lift(frames[:, 7:16], skel_type)[0], CarlaLifter(model).lift(frames[:, 7:16], skel_type)[0])
    assert same_rows(lifter.push(frames[:, 7:16], skel_type)[0], cut_bones[:, 7:16])
    # meta instead of the index tensor
    types = ('adult', 'female'), ('adult', 'male'), ('child', 'female'), ('child', 'male')
    meta = {'age': [types[s][0] for s in skel_type.tolist()], 'gender': [types[s][1] for s in skel_type.tolist()]}
    assert torch.equal(lifter.lift(frames, meta, world_loc, world_rot)[0], whole_bones)
    if kind == 'pose_changes_6d':                          # another number of clips cannot continue this video
        with pytest.raises(RuntimeError):
            lifter.push(frames[:1, :3], skel_type[:1])


def test_lifter_falls_back_for_models_the_kernel_does_not_cover():
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    frames, skel_type, _, _ = host_problem(2, 3, torch.float32)
    # absolute locations: nothing to export, as for export_clips
    lifter = CarlaLifter(LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type='absolute_loc'))
    assert not lifter.supported and lifter.kind is None
    with pytest.warns(UserWarning, match='one-launch path'):
        with pytest.raises(KeyError):
            lifter.lift(frames, skel_type)
    with warnings.catch_warnings():
        warnings.simplefilter('error')                      # one warning per lifter
        with pytest.raises(KeyError):
            lifter.lift(frames, skel_type)
    # 25 input joints: 50 values per frame, not 52 -- the composed path, the rows of the model's own forward
    model = host_model('pose_changes_6d', torch.float32, seed=2, input_nodes=BODY_25_SKELETON)
    lifter = CarlaLifter(model)
    assert not lifter.supported and not ops.lift_supported([50, 25, 12, 6, 39, 78, 156])
    frames25 = host_problem(2, 3, torch.float32, joints=25)[0]
    with pytest.warns(UserWarning, match='one-launch path'):
        bones, root = lifter.lift(frames25, skel_type)
    weights, biases = params_of(model)
    want = ops.lift_to_carla(frames25, weights, biases, skel_type, 'pose_changes_6d')
    assert bones.shape == (2, 3, 26, 6) and torch.equal(bones, want[0]) and torch.equal(root, want[1])


def test_predict_carla_and_the_animation_file_on_the_host(tmp_path):
    """``Trainer.predict_carla`` / ``lift_carla_animation`` against ``Trainer.predict`` / ``save_carla_animation`` with the host
    flow of tests/test_carla_pose.py: the same arrays, and the flow's mode is put back."""
    import numpy as np
    from pedestrians_video_2_carla_amd.data.carla.animation import lift_carla_animation, load_carla_animation, save_carla_animation
    from pedestrians_video_2_carla_amd.trainer import Trainer
    from pedestrians_video_2_carla_amd.walker_control.carla_pose import export_clips
    from test_carla_pose import host_batches, host_flow
    flow = host_flow(host_model('pose_changes_6d', torch.float32, seed=8))
    batches = host_batches(2, 3, 4)
    flow.train()
    got = Trainer().predict_carla(flow, batches)
    assert flow.training and len(got) == 2
    for (bones, root, meta), batch in zip(got, batches):
        want_bones, want_root = export_clips(flow.predict_step(batch, 0))
        assert meta is batch[2] and np.array_equal(bones.numpy(), want_bones) and np.array_equal(root.numpy(), want_root)
    a = load_carla_animation(lift_carla_animation(str(tmp_path / 'lift'), flow, batches, fps=25.0))
    b = load_carla_animation(save_carla_animation(str(tmp_path / 'save'), Trainer().predict(flow, batches), fps=25.0))
    assert np.array_equal(a['bones'], b['bones']) and np.array_equal(a['root'], b['root'])
    assert a['age'] == b['age'] and a['gender'] == b['gender'] and a['bone_names'] == b['bone_names'] and a['fps'] == b['fps']
