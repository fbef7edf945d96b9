"""GPU: the two instantiations of train_clip_kernel (csrc/p2c_train.hip). CFG_DEFAULT is compiled for ONE descriptor
state -- hips_neck_bbox with one hips and one neck joint, no world motion, identity joint maps, both targets, the whole clip of
T = 16 frames in the slice, masked missing joints -- with the fields that state fixes as compile-time constants; CFG_GENERIC reads
them at run time and serves every other descriptor. Both run the same arithmetic in the same order, so everything the step leaves
is compared BIT FOR BIT (int32 views: a NaN loss of an absent target compares as the bits it is), with the switch
p2c_train_step_set_specialized on against off, on the same tensors, in the latency form:

  * losses, loss sums, the flat gradient and the raw factor block of launch 1;
  * which descriptors take CFG_DEFAULT (p2c_train_step_specialized): the benchmark's does, every near miss -- one field off at a
    time -- does not, and runs the general form's bits with the switch on;
  * the bounding-box fallback INSIDE CFG_DEFAULT, which is the one branch of the normaliser that the configuration leaves to the data."""
import ctypes
import dataclasses
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_gpu import dev, make  # noqa: E402
from test_clip_tail_gpu import F_ROWS, _inputs  # noqa: E402
from test_step_prologue_gpu import latency_form  # noqa: E402,F401

FORMS = ['vector', 'loc_2d_3d', 'loc_2d', 'loc_3d']     # the upstream gradient: all three pointers, or one and two nulls
_CACHE = {}


def _cached_inputs(B, T, otype='pose_changes', transform='hips_neck_bbox'):
    """The seeded inputs of tests/test_clip_tail_gpu.py (2-D mask at 0.3), made once per shape and left unchanged."""
    key = (B, T, otype, transform)
    if key not in _CACHE:
        _CACHE[key] = _inputs(B, T, transform=transform, otype=otype, mask2d=0.3)
    return _CACHE[key]


@pytest.fixture
def switch():
    """The library's switch, restored afterwards."""
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    prev = lib.p2c_train_step_set_specialized(-1)
    yield lib
    lib.p2c_train_step_set_specialized(prev)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().clone()


def _step(lib, inp, on, form='vector', gt2d=True, gt3d=True, dloc=None, drot=None, **spec_kw):
    """Both launches, one after the other, with the switch at `on`: (is the descriptor CFG_DEFAULT's, {name: bits})."""
    from pedestrians_video_2_carla_amd import _lib, ops
    spec = ops.PoseHeadSpec(kind=inp['kind'], transform=inp['transform'], **spec_kw)
    B = inp['frames'].shape[0]
    n = len(inp['params']) // 2
    weights, biases = inp['params'][:n], inp['params'][n:]
    f32 = dict(dtype=torch.float32, device=dev())
    bufs = {'partials': torch.zeros(B * 4, **f32), 'loss_sums': torch.zeros(4, **f32), 'losses': torch.zeros(3, **f32)}
    gws, gbs = [torch.zeros_like(w) for w in weights], [torch.zeros_like(b) for b in biases]
    g2, g3 = (inp['gt2d'] if gt2d else None), (inp['gt3d'] if gt3d else None)
    counts = ops.count_target_pairs(spec, g2) if g2 is not None else torch.zeros(B, **f32)
    desc, keep = ops.train_step_desc(inp['frames'], spec, inp['st'], dloc, drot, g2, g3, counts, weights, biases, gws, gbs, bufs)
    ws = keep[2]
    ws.zero_()
    up = {'vector': torch.tensor([0.7, 1.3, 0.5], **f32), 'loc_2d_3d': torch.tensor([1.0], **f32),
          'loc_2d': torch.tensor([1.0], **f32), 'loc_3d': torch.tensor([1.0], **f32)}[form]
    slot = {'loc_2d': 0, 'loc_3d': 1, 'loc_2d_3d': 2}
    glp = (_lib.grad_loss_pointers(vector=up.data_ptr()) if form == 'vector'
           else _lib.grad_loss_pointers(*[up.data_ptr() if i == slot[form] else None for i in range(3)]))
    lib.p2c_train_step_set_specialized(1 if on else 0)
    assert lib.p2c_train_step_set_specialized(-1) == (1 if on else 0)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.p2c_train_step_launch(ctypes.byref(desc), glp, 1, stream), 'first launch')
    torch.cuda.synchronize()
    out = {'factor block': _bits(ws[:B * F_ROWS * 16]), 'partials': _bits(bufs['partials'])}
    _lib.check(lib.p2c_train_step_launch(ctypes.byref(desc), glp, 2, stream), 'second launch')
    torch.cuda.synchronize()
    out['losses'], out['loss_sums'] = _bits(bufs['losses']), _bits(bufs['loss_sums'])
    out['flat gradient'] = _bits(torch.cat([g.reshape(-1) for g in gws] + [g.reshape(-1) for g in gbs]))
    flat = out['flat gradient'].view(torch.float32)
    assert torch.isfinite(flat).all() and flat.abs().max() > 0, 'the case compares nothing: no finite non-zero gradient'
    return int(lib.p2c_train_step_specialized(ctypes.byref(desc))), out


def _same_bits(a, b, what):
    for k in a:
        differ = int((a[k] != b[k]).sum())
        print(f'{what} {k}: {differ} of {a[k].numel()} words differ')
    for k in a:
        assert torch.equal(a[k], b[k]), f'{what}: {k} differs in {int((a[k] != b[k]).sum())} of {a[k].numel()} words'


# ---- specialised against generic ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('otype', ['pose_changes', 'relative_rot'])
@pytest.mark.parametrize('B', [1, 2, 3, 257])
def test_specialised_gives_the_bits_of_generic(latency_form, switch, B, otype, form):
    """T = 16, the default descriptor, both 6-D kinds, every form of the upstream gradient, 30 % of the 2-D targets masked. B = 1:
    one workgroup; 2 and 3: wave 1's pair-count sum over few clips; 257: workgroup 0 runs the NON-FIRST clip body too (its own
    copy of the pose phase in the code). A constant folded to the wrong value, a field of PoseConstsDefault that the kernel should
    still read, or a select that `has2 = has3 = active` simplifies wrongly changes losses or gradient by far more than a bit."""
    inp = _cached_inputs(B, 16, otype)
    is_def, gen = _step(switch, inp, False, form)
    is_def2, spe = _step(switch, inp, True, form)
    assert is_def == 1 and is_def2 == 1, 'the descriptor of this case does not take CFG_DEFAULT: the case compares generic with itself'
    _same_bits(spe, gen, f'B={B} {otype} {form}')


# ---- dispatch -----------------------------------------------------------------------------------------------------------------
def test_the_benchmarks_descriptor_takes_the_specialised_form(monkeypatch, switch):
    """bench.py's flow (B = 256, T = 16, LinearAE pose_changes, loc_2d_3d, hips_neck_bbox, the data module's defaults) through the
    trainer's captured step: the recorded p2c_train_step descriptor, the one every timed step replays, is CFG_DEFAULT's and the
    switch is on by default."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    monkeypatch.setenv('P2C_DIRECT_REPLAY', '1')
    monkeypatch.delenv('P2C_FUSED_TRAIN', raising=False)
    monkeypatch.delenv('P2C_FUSED_UPDATE', raising=False)
    assert switch.p2c_train_step_set_specialized(-1) == 1, 'the switch is not on by default'
    flow, dm = make(B=256, T=16, missing=0.1)
    trainer = Trainer(device=dev(), use_graph=True).setup(flow, dm)
    batch = dm.generate_batch(dev())
    for i in range(2):
        trainer.train_step(flow, batch, i)
    torch.cuda.synchronize()
    assert trainer._direct is not None, 'the trainer did not keep a recorded two-launch step: nothing to look at'
    assert switch.p2c_train_step_specialized(trainer._direct['desc_ref']) == 1
    assert switch.p2c_train_step_specialized(None) == 0


def _world(B, T):
    return torch.zeros(B, T, 3, device=dev()), torch.eye(3, device=dev()).expand(B, T, 3, 3).contiguous()


def _swapped_map():
    m = list(range(26))
    m[3], m[4] = m[4], m[3]
    return tuple(m)


NEAR_MISSES = {          # one field off the default descriptor at a time: (T, transform, keyword arguments of _step)
    'T=15': (15, 'hips_neck_bbox', {}),
    'transform none': (16, 'none', {}),
    'transform bbox': (16, 'bbox', {}),
    'transform hips_neck': (16, 'hips_neck', {}),
    'two hips joints': (16, 'hips_neck_bbox', {'hips_idx': (16, 21)}),
    'world motion': (16, 'hips_neck_bbox', {'world': True}),
    'no gt3d': (16, 'hips_neck_bbox', {'gt3d': False, 'form': 'loc_2d'}),
    'no gt2d': (16, 'hips_neck_bbox', {'gt2d': False, 'form': 'loc_3d'}),
    'joint map': (16, 'hips_neck_bbox', {'gmap2d': _swapped_map()}),
    't0=1': (16, 'hips_neck_bbox', {'eval_slice': (1, None)}),
    'mask_missing_joints=0': (16, 'hips_neck_bbox', {'mask_missing_joints': False}),
}


@pytest.mark.parametrize('miss', list(NEAR_MISSES))
def test_a_near_miss_runs_generic(latency_form, switch, miss):
    """Every field the configuration fixes, moved alone: the descriptor is not CFG_DEFAULT's, and the step with the switch on leaves
    the bits of the switch off (a predicate that forgot the field would run constants that do not hold: another transform, a second
    hips joint dropped, world motion ignored, a target pointer read that is null, frame 0 counted, unmasked pairs masked)."""
    T, transform, kw = NEAR_MISSES[miss]
    kw = dict(kw)
    B = 3
    inp = _cached_inputs(B, T, 'pose_changes', transform)
    if kw.pop('world', False):
        kw['dloc'], kw['drot'] = _world(B, T)
    is_def, gen = _step(switch, inp, False, **kw)
    is_def2, spe = _step(switch, inp, True, **kw)
    assert is_def == 0 and is_def2 == 0, f'{miss}: the descriptor is reported as CFG_DEFAULT\'s'
    _same_bits(spe, gen, miss)
    ref_def, _ = _step(switch, _cached_inputs(B, 16), True)
    assert ref_def == 1, 'the same recipe with no field moved is not CFG_DEFAULT\'s: the near miss shows nothing'


# ---- the bounding-box fallback inside CFG_DEFAULT -------------------------------------------------------------------------------
def test_bbox_fallback_inside_the_specialised_form(latency_form, switch):
    """The fallback of hips_neck_bbox (hips or neck at u, v < near_zero -> the bounding-box scale) is the one normaliser branch
    CFG_DEFAULT leaves to the data. tests/test_clip_tail_gpu.py::test_bbox_fallback_of_one_clip moves one clip's hips with world
    motion, which selects CFG_GENERIC now. Without world motion the hips are the skeleton's root: they project to the image
    centre whatever the frames or the weights are (the model output rotates the joints about it), so no frame or weight puts them
    below near_zero alone. Here the camera's centre (cam_cx, cam_cy: run-time fields of CFG_DEFAULT) is moved so that the hips
    land one pixel outside the image corner while the joints below and right of them stay inside. Checked on the materialised
    projection: the frames whose hips are below near_zero (__any(need_bb) is true for them; the root being where it is, that is
    every frame) keep at least two joints in view each, so their bounding box is finite. Then CFG_DEFAULT against CFG_GENERIC, bit
    for bit, and against the camera where it was: the fallback did change the gradient."""
    from pedestrians_video_2_carla_amd import ops
    B, T = 3, 16
    inp = _cached_inputs(B, T)
    n = len(inp['params']) // 2
    spec0 = ops.PoseHeadSpec(kind=inp['kind'], transform='none')
    with torch.no_grad():
        y = ops.fused_mlp(inp['frames'].reshape(B * T, -1), inp['params'][:n], inp['params'][n:]).view(B, T, 26, 6)
        _, o = ops.pose_head(y, spec0, inp['st'], want=('projection_2d',))
        u0, v0 = o['projection_2d'][0, 0, 1, :2].tolist()
        f, cx, cy, dist, elev = spec0.camera
        camera = (f, cx - u0 - 1.0, cy - v0 - 1.0, dist, elev)
        _, o = ops.pose_head(y, dataclasses.replace(spec0, camera=camera), inp['st'], want=('projection_2d',))
        p = o['projection_2d'][..., :2].cpu()
    hips_out = (p[:, :, 1] < spec0.near_zero).all(-1)                    # (B, T): hips below near_zero in u AND v
    in_view = (p > spec0.near_zero).any(-1).sum(-1)                      # (B, T): joints the bounding box keeps
    print(f'frames that take the fallback: {int(hips_out.sum())} of {B * T}; joints in view there: {in_view[hips_out].tolist()}')
    assert hips_out[0, 0] and (in_view[hips_out] >= 2).all(), 'no frame takes the bounding-box fallback with a finite box: the case shows nothing'
    is_def, gen = _step(switch, inp, False, camera=camera)
    is_def2, spe = _step(switch, inp, True, camera=camera)
    assert is_def == 1 and is_def2 == 1
    _same_bits(spe, gen, 'bbox fallback')
    _, plain = _step(switch, inp, True)
    assert not torch.equal(plain['flat gradient'], spe['flat gradient']), 'the moved camera changed nothing'
