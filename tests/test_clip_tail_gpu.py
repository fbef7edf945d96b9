"""GPU: train_clip_kernel (csrc/p2c_train.hip) past its forward, after the dependent round trips were taken out of the pose phase
and the tail -- the factor block leaves LDS as one batch of reads followed by one batch of stores over a flat index, wave 0 reads
the 24 per-wave loss sums in the same LDS trip, the loss coefficients are worked out once per workgroup by wave 1 during forward
layers 1 -> 2 (upstream gradients loaded in the prologue, the loc_3d denominator handed over by the host) and wave_sum moves its
partners with v_permlane*_swap / DPP instead of ds_bpermute. No arithmetic on data and no summation order moved, so the rule of
tests/test_step_prologue_gpu.py holds against the separate kernels (P2C_FUSED_TRAIN=0 / mlp_fwd + pose head + mlp_bwd): the
losses are the same BITS; the flat gradient is the same bits at B = 256, T = 16 and within 1e-4 of its scale elsewhere (the two
paths cut the frames into other sample tiles there). Each case names what the rearrangement could break."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_gpu import close, dev, make  # noqa: E402
from test_step_prologue_gpu import _same_as_separate, latency_form  # noqa: E402,F401

F_ROWS = 532                                   # rows of a clip's factor block: H_0 .. H_5 (214) | G_1 .. G_6 (318), 16 samples each
SLICE_FLOATS, TICKET_FLOATS = 256 * 79 * 256, 128
SEGMENTS = [0, 52, 78, 91, 97, 136, 214, 240, 253, 259, 298, 376, 532]      # first rows of H_0 .. H_5, G_1 .. G_6, end


def test_headline_shape_is_bit_identical(monkeypatch):
    """B = 256, T = 16, one clip per workgroup (what bench.py measures): losses and the whole flat gradient, bit for bit."""
    _same_as_separate(monkeypatch, B=256, T=16, missing=0.3, otype='pose_changes')


# ---- the two paths on the same tensors, below the flow ------------------------------------------------------------------------
def _inputs(B, T, transform='hips_neck_bbox', otype='pose_changes', mask2d=0.3):
    """Frames, targets, skeleton types and LinearAE parameters of the flow's own recipe; a share of the 2-D targets zeroed
    (= masked, utils/tensors.py:29-40) so that the clips' pair counts differ."""
    from pedestrians_video_2_carla_amd.data.base.base_transforms import BaseTransforms
    flow, dm = make(B=B, T=T, missing=0.3, otype=otype, transform=BaseTransforms[transform])
    frames, targets, meta = dm.generate_batch(dev())
    layers = flow.movements_model.to(dev())._linears()
    params = [l.weight.detach().clone() for l in layers] + [l.bias.detach().clone() for l in layers]
    gt2d = targets['projection_2d_transformed' if transform != 'none' else 'projection_2d'].clone()
    if mask2d:
        g = torch.Generator().manual_seed(11)
        gt2d[(torch.rand(B, T, 26, generator=g) < mask2d).to(dev())] = 0.0
    kind = {'pose_changes': 'pose_changes_6d', 'relative_rot': 'relative_rot_6d'}[otype]
    return dict(frames=frames.contiguous(), gt2d=gt2d.contiguous(), gt3d=targets['absolute_pose_loc'].contiguous(),
                st=meta['skel_type'], params=params, kind=kind, transform=transform)


def _backward(losses, form):
    if form == 'vector':
        (losses.vector * torch.tensor([0.7, 1.3, 0.5], device=dev())).sum().backward()
    else:
        losses[form].backward()


def _both_paths(inp, form='loc_2d_3d', gt2d=True, gt3d=True, hips_lane=1, dloc=None, drot=None):
    """One step of the separate kernels and one of the two-launch step on the same tensors, the upstream gradient arriving
    in the given form. Returns ((loss vector, flat gradient) of the separate kernels, the same of the fused step)."""
    from pedestrians_video_2_carla_amd import ops
    spec = ops.PoseHeadSpec(kind=inp['kind'], transform=inp['transform'], hips_lane=hips_lane)
    frames, st = inp['frames'], inp['st']
    g2, g3 = (inp['gt2d'] if gt2d else None), (inp['gt3d'] if gt3d else None)
    B, T = frames.shape[:2]
    n = len(inp['params']) // 2
    out = []
    for fused in (False, True):
        params = [p.clone().requires_grad_(True) for p in inp['params']]
        with ops.deferred_loss_finalize(2):
            if fused:
                counts = ops.count_target_pairs(spec, g2) if g2 is not None else torch.zeros(B, device=dev())
                losses = ops.fused_train_step(frames, params[:n], params[n:], spec, st, counts, dloc=dloc, drot=drot, gt2d=g2, gt3d=g3)
            else:
                y = ops.fused_mlp(frames.reshape(B * T, -1), params[:n], params[n:]).view(B, T, 26, 6)
                losses, _ = ops.pose_head(y, spec, st, dloc, drot, g2, g3)
            _backward(losses, form)
        torch.cuda.synchronize()
        out.append((losses.vector.detach().cpu().clone(), torch.cat([p.grad.reshape(-1) for p in params]).cpu()))
    return out


def _check(sep, fus, what, nonzero=True):
    print(f'{what}: losses {fus[0].tolist()} (separate {sep[0].tolist()}), flat gradient max |diff| '
          f'{(sep[1] - fus[1]).abs().max().item():.3e} at scale {sep[1].abs().max().item():.3e}')
    assert torch.equal(torch.isnan(sep[0]), torch.isnan(fus[0])), f'{what}: losses {fus[0].tolist()} vs {sep[0].tolist()}'
    assert torch.equal(torch.nan_to_num(sep[0], nan=-7.0), torch.nan_to_num(fus[0], nan=-7.0)), \
        f'{what}: losses {fus[0].tolist()} vs {sep[0].tolist()}'
    assert torch.isfinite(sep[1]).all() and torch.isfinite(fus[1]).all(), f'{what}: non-finite gradient'
    if nonzero:
        assert sep[1].abs().max() > 0
    close(fus[1], sep[1], f'{what}: flat gradient', rtol=1e-4)


# ---- factor block -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 5, 16])
@pytest.mark.parametrize('B', [1, 2, 257])
def test_factor_block_is_written_completely_and_only_where_it_belongs(latency_form, B, T):
    """The first launch alone (p2c_train_step_launch, which = 1) into a workspace full of NaN: a flat index that maps a factor
    row to the wrong LDS row, drops the partial fifth round or runs past it shows as a NaN left inside [0, B 532 16), a sample
    column >= T that does not hold what belongs there (below), or a clobbered float behind the last clip's block. At B = 257
    workgroup 0 stores two clips (the second one's reads must not overtake the barrier in front of them). The second launch
    alone (which = 2) on that block then gives the separate kernels' gradient."""
    from pedestrians_video_2_carla_amd import _lib, ops
    lib = _lib.lib()
    inp = _inputs(B, T)
    spec = ops.PoseHeadSpec(kind=inp['kind'], transform=inp['transform'])
    n = len(inp['params']) // 2
    weights, biases = inp['params'][:n], inp['params'][n:]
    f32 = dict(dtype=torch.float32, device=dev())
    bufs = {'partials': torch.empty(B * 4, **f32), 'loss_sums': torch.empty(4, **f32), 'losses': torch.empty(3, **f32)}
    gws, gbs = [torch.full_like(w, float('nan')) for w in weights], [torch.full_like(b, float('nan')) for b in biases]
    counts = ops.count_target_pairs(spec, inp['gt2d'])
    desc, keep = ops.train_step_desc(inp['frames'], spec, inp['st'], None, None, inp['gt2d'], inp['gt3d'], counts, weights, biases,
                                     gws, gbs, bufs)
    ws = keep[2]
    assert ws.numel() == B * F_ROWS * 16 + SLICE_FLOATS + TICKET_FLOATS
    ws.fill_(float('nan'))
    gl = torch.tensor([0.0, 0.0, 1.0], **f32)
    glp = _lib.grad_loss_pointers(vector=gl.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.p2c_train_step_launch(ctypes.byref(desc), glp, 1, stream), 'first launch')
    torch.cuda.synchronize()
    block = ws[:B * F_ROWS * 16].view(B, F_ROWS, 16).cpu()
    assert not torch.isnan(block).any(), f'{int(torch.isnan(block).sum())} floats of the factor block were not written'
    assert torch.isfinite(block).all()
    # Columns >= T. The issue asked for exact zeros in every row; that holds for H_0 (the x tile reads rows beyond the clip as
    # zero) and for G_1 .. G_6 (grad_y is zero there and the dgrad of zero is zero), which is what keeps those samples out of dW.
    # H_1 .. H_5 hold the forward of an all-zero frame there, relu(b_l + W_l h_{l-1}) from h_0 = 0 (the bias enters through the
    # ones row of every sample), measured 0.119 / 0.206 / 0.181 / 0.459 / 0.415 at most, on the parent build as well. Checked
    # instead: the same bits in every such column of every clip, and the host's fp32 forward of the zero frame to 1e-5 of its
    # scale (dot products of at most 52 fp32 terms: rounding of the order of 1e-6 relative).
    print(f'B={B} T={T} max |columns >= T| per segment:',
          [float(block[:, a:b, T:].abs().max()) if T < 16 else 0.0 for a, b in zip(SEGMENTS[:-1], SEGMENTS[1:])])
    assert (block[:, :52, T:] == 0).all() and (block[:, 214:, T:] == 0).all(), 'H_0 / G_l: sample columns beyond the clip are not zero'
    if T < 16:
        pad = block[:, 52:214, T:]
        assert (pad == pad[:1, :, :1]).all(), 'H_1 .. H_5: the columns beyond the clip differ from one another'
        h, want = torch.zeros(52), []
        for l, (w, b) in enumerate(zip(weights, biases)):
            h = torch.relu(w.cpu() @ h + b.cpu()) if l < n - 1 else w.cpu() @ h + b.cpu()
            want.append(h)
        close(pad[0, :, 0], torch.cat(want[:-1]), 'H_1 .. H_5 of the zero frame', rtol=1e-5)
    assert block[:, :52, :T].abs().max() > 0 and block[:, 376:, :T].abs().max() > 0          # H_0 = x^T, G_6 = grad_y^T
    assert torch.isnan(ws[B * F_ROWS * 16:B * F_ROWS * 16 + 4].cpu()).all(), 'the float behind the last block was written'
    _lib.check(lib.p2c_train_step_launch(ctypes.byref(desc), glp, 2, stream), 'second launch')
    torch.cuda.synchronize()
    flat = torch.cat([g.reshape(-1) for g in gws] + [g.reshape(-1) for g in gbs]).cpu()
    sep, _ = _both_paths(inp)
    _check(sep, (bufs['losses'].cpu(), flat), f'B={B} T={T}')


# ---- loss coefficients ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('form', ['vector', 'loc_2d_3d', 'loc_2d', 'loc_3d'])
def test_coefficients_for_every_form_of_the_upstream_gradient(latency_form, form, B):
    """The upstream gradient as a 3-vector (all three pointers set), as the one loc_2d_3d scalar, as loc_2d only and as loc_3d
    only (the other pointers null: loaded from a stand-in address and dropped): a coefficient formed from the wrong scalar, a
    stand-in value that leaks in, or coefficients read before wave 1 published them change the gradient by a factor."""
    sep, fus = _both_paths(_inputs(B, 16), form)
    _check(sep, fus, f'{form} B={B}')


def test_coefficients_with_every_2d_target_masked(latency_form):
    """Pair count 0 (all 2-D targets zero, no never-masked joint): coef2 is 0, not g / 0; loc_2d is 0 / 0 = NaN on both paths and
    the gradient, which comes from loc_3d alone, is finite."""
    inp = _inputs(3, 16)
    inp['gt2d'].zero_()
    sep, fus = _both_paths(inp, 'vector', hips_lane=-1)
    assert torch.isnan(sep[0][0]) and torch.isfinite(sep[0][1])
    _check(sep, fus, 'all masked')


def test_coefficients_without_3d_targets(latency_form):
    """No 3-D targets: coef3 stays 0 whatever the loc_3d denominator says; loc_2d alone drives the gradient."""
    sep, fus = _both_paths(_inputs(3, 16), 'loc_2d', gt3d=False)
    _check(sep, fus, 'no gt3d')


def test_pair_count_beyond_two_entries_per_thread(latency_form):
    """B = 1 025 in the latency form: thread 0 adds a third pair count in the loop behind the two prologue loads, and the
    workgroups are persistent (four or five clips each): the coefficients of the first clip serve the later ones."""
    sep, fus = _both_paths(_inputs(1025, 16), 'vector')
    _check(sep, fus, 'B=1025')


# ---- descriptor fields of the pose phase --------------------------------------------------------------------------------------
@pytest.mark.parametrize('otype', ['pose_changes', 'relative_rot'])
@pytest.mark.parametrize('transform', ['none', 'bbox', 'hips_neck', 'hips_neck_bbox'])
def test_every_transform_and_both_kinds(monkeypatch, latency_form, transform, otype):
    """B = 2, T = 5 through the flow: the transform, the hips / neck indices, near_zero, the camera constants and the slice bounds
    reach frame_head in every branch of the normaliser, for both 6-D kinds."""
    from pedestrians_video_2_carla_amd.data.base.base_transforms import BaseTransforms
    _same_as_separate(monkeypatch, B=2, T=5, missing=0.3, otype=otype, transform=BaseTransforms[transform])


def test_bbox_fallback_of_one_clip(latency_form):
    """hips_neck_bbox with a world shift that puts clip 0's hips one pixel outside the image corner (u, v < near_zero) while other
    joints of the clip stay inside: that clip takes the bounding-box scale, clip 1 keeps hips-neck (both checked on the
    materialised projection). Also the one case here with world motion: the world pointers' null-ness and the world loads."""
    from pedestrians_video_2_carla_amd import ops
    B, T = 2, 5
    inp = _inputs(B, T)
    spec0 = ops.PoseHeadSpec(kind=inp['kind'], transform='none')
    n = len(inp['params']) // 2
    with torch.no_grad():
        y = ops.fused_mlp(inp['frames'].reshape(B * T, -1), inp['params'][:n], inp['params'][n:]).view(B, T, 26, 6)
        _, o = ops.pose_head(y, spec0, inp['st'], want=('projection_2d',))
        u0, v0, inv_z = o['projection_2d'][0, 0, 1].tolist()           # hips = joint 1: the root, the same in every frame
        f = spec0.camera[0]
        dloc = torch.zeros(B, T, 3, device=dev())
        dloc[0, 0, 1], dloc[0, 0, 2] = (u0 + 1.0) / (f * inv_z), -(v0 + 1.0) / (f * inv_z)     # changes: frame 0's shift stays
        drot = torch.eye(3, device=dev()).expand(B, T, 3, 3).contiguous()
        _, o = ops.pose_head(y, spec0, inp['st'], dloc, drot, want=('projection_2d',))
        p = o['projection_2d'][..., :2].cpu()
    assert (p[0, :, 1] < spec0.near_zero).all(), p[0, :, 1]
    assert (p[1, :, 1] > spec0.near_zero).all() and (p[0] > spec0.near_zero).any(-1).sum() > 10 * T
    sep, fus = _both_paths(inp, 'loc_2d_3d', dloc=dloc, drot=drot)
    _check(sep, fus, 'bbox fallback')


# ---- loss sums --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 15, 16])
def test_loss_sums_with_partly_idle_waves(monkeypatch, latency_form, T):
    """T = 1 (seven of eight waves hold no frame), 15 (wave 7 half idle), 16: every wave reaches wave_sum and writes its three
    sums, wave 0 adds the 24 values in wave order; the losses are the separate kernels' bits."""
    _same_as_separate(monkeypatch, B=3, T=T, missing=0.3, otype='pose_changes')
