"""The streaming kernels -- K4 normaliser, K3 masked 2-D MSE, K5 joint remap (csrc/p2c_aux.hip) and the device metrics
(csrc/p2c_eval.hip) -- on every lane grouping (32 and 64 lanes per frame), in the one-pass and the grid-stride regime of
their launch grids, with every option of their C ABI, against the fp64 oracle (oracle/pose_head.py, oracle/metrics.py;
gradients by fp64 autograd of the same functions). K5 is compared with an index assignment written out here.

Errors are max |got - ref| / max |ref| per tensor. Bounds: values 1e-5, input gradients 5e-5 (the project's bounds for the
shuffle-reduction kernels K14 / K15, tests/test_pose_former_gpu.py); counts, remap outputs and structural zeros exactly.

``near_zero`` is given to kernel and oracle as the SAME number: the fp32 value nearest 1e-5 (the C ABI takes a float). With
the double 1e-5 on the oracle side a confidence of exactly near_zero -- a case below -- would compare differently on the two
sides for a reason that lies in the test, not in the kernel.

The input builders at the top are deterministic and run on the host; ``test_input_conditions`` (not gpu-marked) asserts with
the oracle alone what the GPU comparisons rely on.
"""
import ctypes
import itertools

import pytest
import torch

from oracle import metrics as OM
from oracle import pose_head as O

NZ = float(torch.tensor(1e-5, dtype=torch.float32))
TOL_VALUE, TOL_GRAD = 1e-5, 5e-5
E_NULL, E_SHAPE, E_ENUM, E_INDEX = -1, -2, -3, -4
STREAM_ONE_PASS = 2048 * 256                 # items one launch of stream_grid covers without striding


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _iarr(values):
    return (ctypes.c_int32 * max(1, len(values)))(*values)


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double()
    den = float(ref.abs().max())
    return float((got - ref).abs().max()) / (den if den > 0 else 1.0)


# ======================================================================================================================
# input builders (host)
# ======================================================================================================================
# ---- K4 ----------------------------------------------------------------------------------------------------------------
NORM_TRANSFORMS = (('hips_neck', 2), ('hips_neck', 3), ('bbox', 2), ('hips_neck_bbox', 2))
NORM_JOINTS = (5, 25, 26, 32, 33, 48, 64)
NORM_ARITY = ((1, 1), (1, 2), (2, 1), (2, 2))
# frames 2k, 2k+1 share a wavefront at 32 lanes per frame: (no, no), (no, fallback), (fallback, no), (fallback, fallback)
FALLBACK_PATTERN = (False, False, False, True, True, False, True, True)


def _pick_points(J, nh, nk, variant, seed):
    """hips / neck joint lists: 'last' puts J - 1 among them, 'high' takes every index >= 32 it can, 'any' neither."""
    perm = torch.randperm(J, generator=_gen(seed)).tolist()
    if variant == 'high':
        order = [j for j in perm if j >= 32] + [j for j in perm if j < 32]
    elif variant == 'last':
        order = [J - 1] + [j for j in perm if j != J - 1]
    else:
        order = perm
    pts = order[:nh + nk]
    if seed % 2:                                   # the forced index lands in hips for even seeds, in neck for odd ones
        pts = pts[::-1]
    return tuple(pts[:nh]), tuple(pts[nh:])


def norm_cases():
    cases, i = [], 0
    for tr, dim in NORM_TRANSFORMS:
        sizes = (8, 9, 37, 16, 9) if tr == 'hips_neck_bbox' else (1, 7, 8, 9, 37)   # the fallback mix needs four frame pairs
        for J in NORM_JOINTS:
            for v in range(2):
                nh, nk = NORM_ARITY[i % 4]
                variant = 'last' if v == 0 else ('high' if J > 32 else 'any')
                hips, neck = _pick_points(J, nh, nk, variant, 1000 + i)
                cases.append(dict(tr=tr, dim=dim, J=J, N=sizes[i % 5], C=dim + (i + i // 4) % 4, hips=hips, neck=neck, seed=i))
                i += 1
    # the long runs: 12 501 workgroups at 32 lanes, 25 001 at 64
    cases.append(dict(tr='hips_neck_bbox', dim=2, J=26, N=100003, C=3, hips=(1,), neck=(8,), seed=900))
    cases.append(dict(tr='bbox', dim=2, J=33, N=100003, C=2, hips=(32,), neck=(0,), seed=901))
    cases.append(dict(tr='hips_neck', dim=3, J=5, N=100003, C=4, hips=(4, 0), neck=(2,), seed=902))
    for c in cases:
        c['id'] = '{tr}{dim}-J{J}-N{N}-C{C}-h{h}-k{k}'.format(h='_'.join(map(str, c['hips'])), k='_'.join(map(str, c['neck'])), **c)
    return cases


NORM_CASES = norm_cases()


def norm_input(c):
    """x (N, J, C) fp32. hips_neck: unit-scale-free coordinates around 200. bbox transforms: image-like coordinates, ~15 % of the
    joints at (0, 0) and ~3 % negative (both count as missing). Confidence channel (dim 2, C > 2): 25 % zero, 5 % exactly
    near_zero, the rest in [0.1, 1). Degenerate frames (scale 0 or not finite) on every 40th frame from frame 20."""
    g = _gen(7000 + c['seed'])
    N, J, C, dim, tr = c['N'], c['J'], c['C'], c['dim'], c['tr']
    hips, neck = list(c['hips']), list(c['neck'])
    x, present = torch.zeros(N, J, C), None
    if tr == 'hips_neck':
        x[..., :dim] = torch.randn(N, J, dim, generator=g) * 30 + 200
    else:
        # a random rank per frame and coordinate plus jitter below one rank: no two joints of a frame share a coordinate, so no
        # bounding-box extremum is tied (the kernel credits the first lane there, autograd splits the gradient)
        rank = torch.rand(N, J, 2, generator=g).argsort(1).argsort(1)
        xy = (rank + 0.5 * torch.rand(N, J, 2, generator=g)) * (300.0 / J) + 50
        present = xy.clone()
        u = torch.rand(N, J, generator=g)
        xy[u < 0.15] = 0
        xy[(u >= 0.15) & (u < 0.18)] *= -1
        xy[0, 0] = 0                                                                 # (both kinds in the smallest case too)
        xy[0, 1] = -xy[0, 1].abs() - 1
        x[..., :2] = xy
    if C > dim:
        x[..., dim:] = torch.randn(N, J, C - dim, generator=g)
        if dim == 2:
            conf = torch.rand(N, J, generator=g) * 0.9 + 0.1
            v = torch.rand(N, J, generator=g)
            conf[v < 0.25] = 0
            conf[(v >= 0.25) & (v < 0.30)] = NZ
            conf[0, 0], conf[0, 1], conf[0, 2] = 0.0, NZ, 0.5
            x[..., 2] = conf
    frames = torch.arange(N)
    if tr == 'hips_neck_bbox':
        pts = torch.tensor(hips + neck)
        x[:, pts, :2] = present[:, pts]                                             # hips and neck present ...
        fb = torch.tensor(FALLBACK_PATTERN)[frames % 8]
        for idx, w in ((hips, 0), (neck, 1)):                                       # ... but for the fallback frames
            rows = torch.nonzero(fb & ((frames // 4) % 2 == w)).flatten()
            x[rows[:, None], torch.tensor(idx)[None, :], 0:2] = 0
    for k, n in enumerate(range(20, N, 40)):
        if tr == 'hips_neck' or (tr == 'hips_neck_bbox' and k % 3 == 2):
            n = n + 1 if tr == 'hips_neck_bbox' else n                              # (a frame without the fallback)
            x[n, hips + neck, :dim] = x[n, hips[0], :dim].clone()                         # hips = neck: scale 0
        elif k % 3 == 0:
            x[n, :, :2] = 0                                                         # every joint missing: scale NaN
        elif k % 3 == 1:
            keep = x[n, n % J, :2].abs() + 1
            x[n, :, :2] = 0
            x[n, n % J, :2] = keep                                                  # one present joint: scale 0
        else:
            x[n, :, :2] = -x[n, :, :2].abs() - 1                                    # missing because negative
    return x


def norm_reference(x64, c):
    """The oracle where the reference defines the operation. For dim 2 with C > 3 the reference normaliser is undefined
    (normalizer.py:23-28 leaves the channels past the confidence unwritten); the kernel copies them through nan_to_zero, so
    the expected result there is the oracle on the first three channels and the input itself on the rest."""
    kw = dict(dim=c['dim'], hips=c['hips'], neck=c['neck'], near_zero=NZ)
    if c['dim'] == 2 and x64.shape[-1] > 3:
        out, shift, scale = O.normalize(x64[..., :3], c['tr'], **kw)
        return torch.cat((out, O.nan_to_zero(x64[..., 3:])), -1), shift, scale
    return O.normalize(x64, c['tr'], **kw)


def norm_fallback_frames(x64, c):
    s, k = O._points(x64[..., :2], c['hips']), O._points(x64[..., :2], c['neck'])
    return torch.all(s < NZ, dim=-1) | torch.all(k < NZ, dim=-1)


def norm_degenerate(scale64):
    return ~torch.isfinite(scale64) | (scale64 == 0)


# ---- K3 ----------------------------------------------------------------------------------------------------------------
def _loss_case(N, Jp, Cp, Jg, Cg, K, mask, hips, seed):
    g = _gen(seed)
    pidx = torch.randperm(Jp, generator=g)[:K].tolist()          # partial and permuted
    gidx = torch.randperm(Jg, generator=g)[:K].tolist()
    hips_col = {'none': -1, 'first': 0, 'last': K - 1}[hips]
    return dict(N=N, Jp=Jp, Cp=Cp, Jg=Jg, Cg=Cg, K=K, mask=mask, hips_col=hips_col, pidx=pidx, gidx=gidx, seed=seed,
                id=f'N{N}-Jp{Jp}c{Cp}-Jg{Jg}c{Cg}-K{K}-mask{int(mask)}-hips{hips_col}')


LOSS_CASES = [
    _loss_case(1, 3, 2, 4, 3, 1, False, 'none', 1),              # N K = 1
    _loss_case(9, 26, 3, 25, 2, 7, True, 'first', 2),            # 63
    _loss_case(1, 64, 2, 70, 4, 64, True, 'last', 3),            # 64: one full wavefront, K at its bound
    _loss_case(5, 20, 4, 13, 2, 13, True, 'none', 4),            # 65
    _loss_case(400, 26, 3, 25, 3, 25, True, 'first', 5),         # 10 000
    _loss_case(400, 26, 2, 25, 4, 25, False, 'last', 6),         # mask off, hips_col given all the same
    _loss_case(37, 200, 3, 30, 2, 10, True, 'last', 7),          # few common joints of a wide prediction
    _loss_case(21000, 26, 2, 25, 2, 25, True, 'last', 8),        # N K = 525 000 and N Jp = 546 000: both grids stride
    _loss_case(8200, 80, 3, 64, 3, 64, False, 'none', 9),        # 524 800 / 656 000, mask off
]


def loss_input(c):
    """pred, gt fp32. With the mask on: 20 % of gt joints at zero, 5 % with ONE zero coordinate (masked all the same), and the hips
    joint zeroed on a third of the frames (counted all the same)."""
    g = _gen(5000 + c['seed'])
    pred = torch.randn(c['N'], c['Jp'], c['Cp'], generator=g)
    gt = torch.randn(c['N'], c['Jg'], c['Cg'], generator=g)
    if c['mask'] and c['N'] * c['K'] > 1:
        u = torch.rand(c['N'], c['Jg'], generator=g)
        gt[u < 0.2] = 0
        gt[..., 0][(u >= 0.2) & (u < 0.225)] = 0
        gt[..., 1][(u >= 0.225) & (u < 0.25)] = 0
        if c['N'] * c['K'] > 16:                                  # (make sure both kinds occur in the small cases too)
            gt[0, c['gidx'][-1 if c['hips_col'] == 0 else 0], :2] = 0
            gt[-1, c['gidx'][-1 if c['hips_col'] == 0 else 0], :2] = 0.5
        if c['hips_col'] >= 0:
            gt[::3, c['gidx'][c['hips_col']]] = 0
    return pred, gt


def loss_reference(p64, g64, c):
    return O.loss_loc_2d(p64, g64, c['pidx'], c['gidx'], None if c['hips_col'] < 0 else c['hips_col'], c['mask'])


def loss_mask(g64, c):
    g = g64[..., c['gidx'], 0:2]
    if not c['mask']:
        return torch.ones(g.shape[:-1], dtype=torch.bool)
    m = torch.all(g != 0, dim=-1)
    if c['hips_col'] >= 0:
        m[..., c['hips_col']] = True
    return m


# ---- K5 ----------------------------------------------------------------------------------------------------------------
def _remap_case(name, N, Js, Jd, C, src, dst):
    return dict(id=name, N=N, Js=Js, Jd=Jd, C=C, src=list(src), dst=list(dst))


def remap_cases():
    g = _gen(11)
    perm26 = torch.randperm(26, generator=g).tolist()
    p64 = torch.randperm(64, generator=g).tolist()
    return [
        _remap_case('K0', 5, 7, 9, 3, [], []),
        _remap_case('identity', 9, 26, 26, 2, range(26), range(26)),
        _remap_case('permutation', 35, 26, 26, 3, range(26), perm26),
        _remap_case('partial', 35, 25, 26, 4, perm26[:11], [(3 * j + 1) % 26 for j in range(11)]),
        _remap_case('Jdst64', 7, 70, 64, 1, [(j * 7) % 70 for j in range(40)], p64[:40]),
        _remap_case('N1', 1, 5, 3, 2, [4, 0], [0, 2]),
        _remap_case('stride', 2731, 25, 64, 3, perm26[:20], p64[:20]),      # 2731 * 64 * 3 = 524 352 > 524 288
        _remap_case('stride-C4', 5100, 30, 26, 4, perm26, range(26)),        # 530 400
    ]


REMAP_CASES = remap_cases()


def remap_input(c):
    return torch.randn(c['N'], c['Js'], c['C'], generator=_gen(600 + c['N'] + c['Jd']))


def remap_expected(src, c):
    dst = torch.zeros(c['N'], c['Jd'], c['C'], dtype=src.dtype)
    for s, d in zip(c['src'], c['dst']):
        dst[:, d, :] = src[:, s, :]
    return dst


# ---- MPJPE / MRPE ----------------------------------------------------------------------------------------------------------
def _gmap(kind):
    if kind == 'carla26':
        return 26, list(range(26))
    if kind == 'body25':
        from pedestrians_video_2_carla_amd.data.base.skeleton import get_common_indices
        from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
        from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
        out_idx, in_idx = get_common_indices(input_nodes=BODY_25_SKELETON, output_nodes=CARLA_SKELETON)
        gmap = [-1] * 26
        for o, i in zip(out_idx, in_idx):
            gmap[o] = i
        return 25, gmap
    return 40, [-1 if j % 3 == 2 else (3 * j + 1) % 40 for j in range(26)]       # sparse: 18 of 26 joints, scattered over 40


def _pose3d_case(B, T, kind, nph, ngh, world, seed):
    Jg, gmap = _gmap(kind)
    return dict(B=B, T=T, kind=kind, Jg=Jg, gmap=gmap, pred_hips=[1, 17][:nph], gt_hips=[Jg - 1, 3][:ngh], world=world, seed=seed,
                id=f'B{B}-T{T}-{kind}-ph{nph}-gh{ngh}-world{int(world)}')


POSE3D_CASES = [
    _pose3d_case(1, 1, 'carla26', 1, 1, True, 1),
    _pose3d_case(2, 16, 'body25', 1, 2, True, 2),
    _pose3d_case(3, 81, 'sparse40', 2, 1, True, 3),
    _pose3d_case(8, 300, 'carla26', 2, 2, False, 4),
    _pose3d_case(9, 16, 'sparse40', 1, 2, True, 5),
    _pose3d_case(513, 16, 'body25', 2, 2, True, 6),              # 257 wavefronts -> 260 partials: accumulate strides
    _pose3d_case(4099, 1, 'carla26', 1, 1, False, 7),
    _pose3d_case(4099, 16, 'sparse40', 2, 2, True, 8),
]


def pose3d_input(c, B=None):
    g = _gen(3000 + c['seed'] + (B or 0))
    B = B or c['B']
    pred, gt = torch.randn(B, c['T'], 26, 3, generator=g), torch.randn(B, c['T'], c['Jg'], 3, generator=g)
    wp, wg = torch.randn(B, c['T'], 3, generator=g) * 0.3, torch.randn(B, c['T'], 3, generator=g) * 0.3
    return pred, gt, wp, wg


def pose3d_reference(pred, gt, wp, wg, c):
    out_idx = [j for j in range(26) if c['gmap'][j] >= 0]
    s0, n0 = OM.mpjpe_update(pred.double(), gt.double(), out_idx, [c['gmap'][j] for j in out_idx])
    s1, n1 = OM.mrpe_update(pred.double(), gt.double(), wp.double(), wg.double(), c['pred_hips'], c['gt_hips'])
    return float(s0), n0, float(s1), n1


# ---- PCK ---------------------------------------------------------------------------------------------------------------
def _pck_case(Jg, Jp, Cp, Cg, N, mode, nh, nk, mask, own_src, hips, seed):
    g = _gen(seed)
    gperm = torch.randperm(Jg, generator=g).tolist()
    n_common = max(2, min(Jp, Jg) * 4 // 5)
    ins = sorted(gperm[:n_common])                                # gt joints that have a partner ...
    outs = torch.randperm(Jp, generator=g)[:n_common].tolist()    # ... and the partner
    pmap = [-1] * Jg
    for i, o in zip(ins, outs):
        pmap[i] = o
    variant = 'high' if (Jg > 32 and seed % 2) else 'last'
    hips_idx, neck_idx = _pick_points(Jg, nh, nk, variant, 40 + seed)
    hips_joint = ins[len(ins) // 2] if hips else -1
    return dict(Jg=Jg, Jp=Jp, Cp=Cp, Cg=Cg, N=N, mode=mode, hips_idx=hips_idx, neck_idx=neck_idx, mask=mask, own_src=own_src,
                hips_joint=hips_joint, pmap=pmap, ins=ins, outs=outs, threshold=0.2 if mode else 0.05, seed=seed,
                id=f'Jg{Jg}c{Cg}-Jp{Jp}c{Cp}-N{N}-mode{mode}-h{nh}k{nk}-mask{int(mask)}-src{int(own_src)}-hj{hips_joint}')


PCK_CASES = [
    _pck_case(5, 7, 2, 2, 1, 0, 1, 1, True, False, True, 1),
    _pck_case(5, 4, 3, 2, 9, 1, 2, 2, True, True, False, 2),
    _pck_case(25, 26, 2, 3, 2, 1, 1, 1, True, True, True, 3),
    _pck_case(25, 26, 3, 3, 513, 0, 1, 1, False, False, True, 4),
    _pck_case(26, 26, 2, 2, 7, 1, 1, 2, True, False, True, 5),
    _pck_case(26, 20, 2, 2, 20001, 0, 1, 1, True, True, True, 6),     # 10 001 wavefronts: accumulate strides
    _pck_case(32, 40, 3, 2, 8, 1, 2, 1, True, True, False, 7),
    _pck_case(32, 26, 2, 3, 9, 0, 1, 1, True, False, False, 8),
    _pck_case(33, 26, 2, 2, 7, 1, 1, 1, True, True, True, 9),         # 64 lanes per frame from here
    _pck_case(33, 40, 3, 3, 513, 0, 1, 1, True, True, True, 10),
    _pck_case(64, 64, 2, 2, 8, 1, 2, 2, True, False, True, 11),
    _pck_case(64, 26, 2, 3, 9, 1, 2, 1, False, False, False, 12),
    _pck_case(64, 70, 3, 2, 20001, 1, 1, 2, True, True, True, 13),
    _pck_case(48, 26, 2, 2, 2, 0, 1, 1, True, True, False, 14),
    _pck_case(64, 64, 2, 2, 1, 0, 1, 1, False, False, True, 15),
]


def pck_terms(pred, gt, src, c, threshold=None):
    """fp64 normalised distance (N, K) of every common joint, the mask of the counted ones and the frame normaliser, step by
    step as oracle.metrics.pck_update takes them (test_input_conditions holds the two together)."""
    g, p, m = gt.double()[..., :2], pred.double()[..., :2], src.double()[..., :2]
    if c['mask']:
        mask = torch.all(m[:, c['ins']] != 0, dim=-1)
        if c['hips_joint'] >= 0:
            mask[:, c['ins'].index(c['hips_joint'])] = True
    else:
        mask = torch.ones(g.shape[0], len(c['ins']), dtype=torch.bool)
    if c['mode'] == 0:
        boxes = O.get_bboxes(g, NZ)
        norm = torch.linalg.norm(boxes[..., 1, :] - boxes[..., 0, :], dim=-1)
    else:
        norm = torch.linalg.norm(O._points(g, c['neck_idx']) - O._points(g, c['hips_idx']), dim=-1)
    mask = mask & ~(norm < NZ)[:, None]
    norm = torch.where(norm < NZ, torch.ones_like(norm), norm)
    dist = torch.linalg.norm((p[:, c['outs']] - g[:, c['ins']]) / norm[:, None, None], dim=-1)
    return dist, mask, norm


def pck_input(c):
    """pred, gt, mask_src fp32. gt image-like with ~15 % of the joints at (0, 0); predictions of the common joints = gt + noise of
    about the threshold; mask_src (when it is a tensor of its own) with its own zeros, some in one coordinate only. From N = 7 up:
    frame 2 has every joint missing, frame 5 a normaliser below near_zero. Last, any counted joint whose fp64 normalised distance
    lies within a relative 1e-4 of the threshold gets a prediction at half the threshold instead."""
    g = _gen(9000 + c['seed'])
    N, Jg, Jp = c['N'], c['Jg'], c['Jp']
    gt = torch.rand(N, Jg, c['Cg'], generator=g) * 300 + 50
    gt[torch.rand(N, Jg, generator=g) < 0.15] = 0
    if N >= 7:
        gt[2] = 0
        if c['mode'] == 0:
            one = gt[5, 3].abs() + 60
            gt[5] = 0
            gt[5, 3] = one                                             # one present joint: bounding-box diagonal 0
        else:
            gt[5, list(c['hips_idx']) + list(c['neck_idx'])] = gt[5, c['hips_idx'][0]].abs() + 60      # |neck - hips| = 0
    pred = torch.rand(N, Jp, c['Cp'], generator=g) * 300 + 50
    sigma = 12.0 if c['mode'] == 0 else 25.0
    pred[:, c['outs'], :2] = gt[:, c['ins'], :2] + torch.randn(N, len(c['ins']), 2, generator=g) * sigma
    if c['own_src']:
        src = torch.rand(N, Jg, c['Cg'], generator=g) * 300 + 50
        u = torch.rand(N, Jg, generator=g)
        src[u < 0.2] = 0
        src[..., 0][(u >= 0.2) & (u < 0.24)] = 0
        src[..., 1][(u >= 0.24) & (u < 0.28)] = 0
    else:
        src = gt
    dist, mask, norm = pck_terms(pred, gt, src, c)
    near = torch.nonzero(mask & ((dist / c['threshold'] - 1).abs() < 1e-4))
    for n, k in near.tolist():
        pred[n, c['outs'][k], 0] = gt[n, c['ins'][k], 0] + 0.5 * c['threshold'] * float(norm[n])
        pred[n, c['outs'][k], 1] = gt[n, c['ins'][k], 1]
    return pred, gt, src


def pck_reference(pred, gt, src, c, threshold=None):
    """OM.pck_update in fp64 on the two channels the C ABI reads (its bounding box would take a third channel into the diagonal)."""
    hips_col = c['ins'].index(c['hips_joint']) if c['hips_joint'] >= 0 else None
    correct, total = OM.pck_update(pred.double()[None, ..., :2], gt.double()[None, ..., :2], c['outs'], c['ins'], hips_col,
                                   c['mask'], src.double()[None, ..., :2], 'bbox' if c['mode'] == 0 else 'hn', c['hips_idx'],
                                   c['neck_idx'], c['threshold'] if threshold is None else threshold, NZ)
    return int(correct), int(total)


def pck_band_is_empty(pred, gt, src, c):
    lo = pck_reference(pred, gt, src, c, c['threshold'] * (1 - 1e-4))
    hi = pck_reference(pred, gt, src, c, c['threshold'] * (1 + 1e-4))
    return lo == hi


# ======================================================================================================================
# the conditions the GPU comparisons rely on, from the oracle alone (runs without a GPU)
# ======================================================================================================================
def test_input_conditions():
    for c in NORM_CASES:
        x64 = norm_input(c).double()
        _, _, scale = norm_reference(x64, c)
        deg = norm_degenerate(scale)
        assert int(deg.sum()) * 20 <= c['N'], (c['id'], int(deg.sum()))                     # at most 5 % degenerate frames
        if c['N'] >= 37:
            assert int(deg.sum()) >= 1, c['id']
        if c['tr'] != 'hips_neck':
            # the kernel credits the first lane at a bounding-box extremum, autograd splits the gradient between equals
            missing = torch.all(x64[..., :2] < NZ, dim=-1)
            boxes = O.get_bboxes(x64[..., :2], NZ)
            for b in (0, 1):
                hits = ((x64[..., :2] == boxes[:, b, None, :]) & ~missing[..., None]).sum(1)
                assert bool((hits[~deg] == 1).all()), (c['id'], 'tie at a bounding-box extremum')
            assert bool(missing.any()) and (bool((x64[..., :2] < 0).any()) or c['N'] * c['J'] < 200), c['id']
        if c['tr'] == 'hips_neck_bbox':
            fb = norm_fallback_frames(x64, c)
            pairs = {(bool(fb[2 * k]), bool(fb[2 * k + 1])) for k in range(c['N'] // 2)}
            assert pairs == set(itertools.product((False, True), repeat=2)), (c['id'], pairs)
        if c['dim'] == 2 and c['C'] > 2:
            conf = x64[..., 2]
            assert bool((conf == 0).any()) and bool((conf == NZ).any()) and bool((conf >= 0.1).any()), c['id']
    lanes = {(c['J'] > 32, len(c['hips']), len(c['neck'])) for c in NORM_CASES if c['tr'] != 'bbox'}
    assert len(lanes) == 8                                                                   # every arity on both lane groupings
    assert any(min(c['hips'] + c['neck']) >= 32 for c in NORM_CASES) and all(
        any(c['J'] == J and J - 1 in c['hips'] + c['neck'] for c in NORM_CASES) for J in NORM_JOINTS)

    for c in LOSS_CASES:
        pred, gt = loss_input(c)
        m = loss_mask(gt.double(), c)
        if c['mask']:
            assert bool(m.any()) and not bool(m.all()), c['id']                              # masked and unmasked joints
            g = gt[..., c['gidx'], 0:2]
            assert bool((((g[..., 0] == 0) != (g[..., 1] == 0)) & ~m).any()) or c['N'] * c['K'] < 100, c['id']
            if c['hips_col'] >= 0:
                assert bool(torch.all(g[:, c['hips_col']] == 0, -1).any()), c['id']          # a zero hips joint, counted
        assert int(m.sum()) == int(loss_reference(pred.double(), gt.double(), c)[2]), c['id']
    assert any(c['N'] * c['K'] > STREAM_ONE_PASS and c['N'] * c['Jp'] > STREAM_ONE_PASS for c in LOSS_CASES)
    assert {c['N'] * c['K'] for c in LOSS_CASES} >= {1, 63, 64, 65, 10000}

    assert any(c['N'] * c['Jd'] * c['C'] > STREAM_ONE_PASS for c in REMAP_CASES)

    for c in PCK_CASES:
        pred, gt, src = pck_input(c)
        dist, mask, _ = pck_terms(pred, gt, src, c)
        assert not bool((mask & ((dist / c['threshold'] - 1).abs() < 1e-4)).any()), c['id']  # nobody inside the band
        assert pck_band_is_empty(pred, gt, src, c), c['id']
        correct, total = pck_reference(pred, gt, src, c)
        assert (int((dist[mask] < c['threshold']).sum()), int(mask.sum())) == (correct, total), c['id']
        if c['N'] >= 7:
            assert 0 < correct < total, (c['id'], correct, total)
            assert not bool(mask[5].any()), c['id']                                          # the frame below near_zero
        if c['mask'] and c['N'] >= 7:
            assert not bool(mask.all()), c['id']


# ======================================================================================================================
# GPU
# ======================================================================================================================
def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _same_nonfinite(got, ref, what):
    got = got.detach().double().cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), what
    inf = torch.isinf(ref)
    assert torch.equal(torch.isinf(got), inf) and torch.equal(got[inf], ref[inf]), what
    fin = torch.isfinite(ref)
    return _rel(got[fin], ref[fin]) if bool(fin.any()) else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('c', NORM_CASES, ids=[c['id'] for c in NORM_CASES])
def test_normaliser_against_fp64(c):
    """K4 forward (out, shift, scale) and backward (x.grad for a random upstream gradient) through ops.normalize.

    Degenerate frames (scale 0 or not finite) stay in the forward comparison; in the backward one the kernel's gradient only has
    to be finite there (autograd through nan_to_num gives NaN). Exact zeros: the output coordinates of a joint whose confidence
    is below near_zero, and its gradient wherever autograd's is zero too (a hips / neck / bounding-box-extremum joint still gets
    the gradient of shift and scale).

    Worst ratios observed on an MI355X (the test prints every case's before it asserts): out 4.5e-6 (hips_neck 3-D, J 5, N 100 003:
    one frame of 100 003 with a small hips-neck distance), shift 5.9e-8, scale 4.2e-7, gradient 7.8e-6 (hips_neck_bbox, J 5, N 37).
    All inside the starting bounds, so no case has a bound of its own."""
    from pedestrians_video_2_carla_amd import ops
    d = _dev()
    x = norm_input(c)
    w = torch.randn(x.shape, generator=_gen(c['seed'] + 1))
    x64 = x.double().requires_grad_(True)
    ref_out, ref_shift, ref_scale = norm_reference(x64, c)
    (ref_out * w.double()).sum().backward()
    deg = norm_degenerate(ref_scale.detach())

    xd = x.to(d).requires_grad_(True)
    out, shift, scale = ops.normalize(xd, c['tr'], c['dim'], c['hips'], c['neck'], NZ)
    (out * w.to(d)).sum().backward()
    torch.cuda.synchronize()
    out, grad = out.detach().cpu(), xd.grad.cpu()

    e_out = _rel(out, ref_out)
    e_shift = _same_nonfinite(shift, ref_shift.detach(), 'shift')
    e_scale = _same_nonfinite(scale, ref_scale.detach(), 'scale')
    assert bool(torch.isfinite(grad).all()), 'the gradient of a degenerate frame must be finite'
    e_grad = _rel(grad[~deg], x64.grad[~deg]) if bool((~deg).any()) else 0.0
    print(f'K4 {c["id"]}: out {e_out:.2e} shift {e_shift:.2e} scale {e_scale:.2e} grad {e_grad:.2e}')
    if c['dim'] == 2 and c['C'] > 2:
        dropped = x[..., 2] < NZ
        assert bool(dropped.any()) and bool((out[..., :2][dropped] == 0).all())
        quiet = (dropped & ~deg[:, None])[..., None] & (x64.grad[..., :2] == 0)
        assert bool(quiet.any()) and bool((grad[..., :2][quiet] == 0).all())
        assert torch.equal(out[..., 2:], O.nan_to_zero(x[..., 2:]))                  # confidence and further channels: copies
        assert torch.equal(grad[..., 2:], w[..., 2:])
    assert e_out <= TOL_VALUE and e_shift <= TOL_VALUE and e_scale <= TOL_VALUE, (e_out, e_shift, e_scale)
    assert e_grad <= TOL_GRAD, e_grad


def _loss2d_fwd_abi(pred, gt, c):
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    f32 = dict(dtype=torch.float32, device=pred.device)
    partials = torch.empty(lib.p2c_loss2d_workspace_floats(c['N']), **f32)
    sums, loss = torch.empty(2, **f32), torch.empty(1, **f32)
    _lib.check(lib.p2c_loss2d_fwd(pred.data_ptr(), gt.data_ptr(), c['N'], c['Jp'], c['Cp'], c['Jg'], c['Cg'], c['K'], _iarr(c['pidx']),
                                  _iarr(c['gidx']), c['hips_col'], int(c['mask']), partials.data_ptr(), sums.data_ptr(),
                                  loss.data_ptr(), torch.cuda.current_stream().cuda_stream), 'p2c_loss2d_fwd')
    torch.cuda.synchronize()
    return loss.cpu(), sums.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('c', LOSS_CASES, ids=[c['id'] for c in LOSS_CASES])
def test_loss2d_against_fp64(c):
    """K3: loss and pred.grad (of 1.7 * loss, so grad_loss != 1) through ops.loss_loc_2d, sum_sq and n_unmasked through the C ABI.
    Exact: n_unmasked, and the zeros of the gradient on prediction joints outside the common list, on masked joints and on
    channels >= 2.

    Worst ratios observed on an MI355X: loss 1.0e-7, sum_sq 5.1e-8, gradient 1.1e-7."""
    from pedestrians_video_2_carla_amd import ops
    d = _dev()
    pred, gt = loss_input(c)
    p64 = pred.double().requires_grad_(True)
    ref_loss, ref_sum, ref_n = loss_reference(p64, gt.double(), c)
    (1.7 * ref_loss).backward()

    pd, gd = pred.to(d).requires_grad_(True), gt.to(d)
    loss = ops.loss_loc_2d(pd, gd, c['pidx'], c['gidx'], c['hips_col'], c['mask'])
    (1.7 * loss).backward()
    loss_abi, sums = _loss2d_fwd_abi(pd.detach(), gd, c)
    grad = pd.grad.cpu()
    e_loss, e_sum, e_grad = _rel(loss, ref_loss), _rel(sums[0], ref_sum), _rel(grad, p64.grad)
    print(f'K3 {c["id"]}: loss {e_loss:.2e} sum_sq {e_sum:.2e} grad {e_grad:.2e}')
    assert float(sums[1]) == float(ref_n)
    assert float(loss_abi) == float(loss.detach())
    outside = torch.ones(c['Jp'], dtype=torch.bool)
    outside[c['pidx']] = False
    assert bool((grad[:, outside] == 0).all()) and bool((grad[..., 2:] == 0).all())
    masked = ~loss_mask(gt.double(), c)
    assert bool((grad[:, c['pidx'], :2][masked] == 0).all())
    assert bool((grad[:, c['pidx'], :2][~masked] != 0).any())
    assert e_loss <= TOL_VALUE and e_sum <= TOL_VALUE, (e_loss, e_sum)
    assert e_grad <= TOL_GRAD, e_grad


@pytest.mark.gpu
def test_loss2d_all_masked():
    """Mask on, no hips column, gt all zero: nothing is counted, and the kernel's coef = 0 rule gives an all-zero gradient (autograd
    would give 0 / 0 there, so it is not consulted)."""
    from pedestrians_video_2_carla_amd import ops
    d = _dev()
    c = _loss_case(40, 26, 3, 25, 2, 25, True, 'none', 77)
    pred = torch.randn(40, 26, 3, generator=_gen(77))
    gt = torch.zeros(40, 25, 2)
    pd = pred.to(d).requires_grad_(True)
    loss = ops.loss_loc_2d(pd, gt.to(d), c['pidx'], c['gidx'], -1, True)
    (1.7 * loss).backward()
    _, sums = _loss2d_fwd_abi(pd.detach(), gt.to(d), c)
    assert int(loss_reference(pred.double(), gt.double(), c)[2]) == 0
    assert float(sums[1]) == 0.0 and float(sums[0]) == 0.0
    assert bool((pd.grad == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize('c', REMAP_CASES, ids=[c['id'] for c in REMAP_CASES])
def test_remap_is_the_index_assignment(c):
    """K5: dst[:, dst_idx[k]] = src[:, src_idx[k]], every other destination joint zero; bit-exact."""
    from pedestrians_video_2_carla_amd import ops
    src = remap_input(c)
    got = ops.remap_nodes(src.to(_dev()), c['Jd'], c['src'], c['dst']).cpu()
    assert torch.equal(got, remap_expected(src, c))


def _pose3d_abi(pred, gt, wp, wg, c, state):
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    B = pred.shape[0]
    part = torch.empty(lib.p2c_eval_workspace_floats(B), dtype=torch.float32, device=pred.device)
    _lib.check(lib.p2c_eval_pose3d(pred.data_ptr(), gt.data_ptr(), B, c['T'], c['Jg'], _iarr(c['gmap']), _iarr(c['pred_hips']),
                                   len(c['pred_hips']), _iarr(c['gt_hips']), len(c['gt_hips']),
                                   None if wp is None else wp.data_ptr(), None if wg is None else wg.data_ptr(), part.data_ptr(),
                                   state.data_ptr(), torch.cuda.current_stream().cuda_stream), 'p2c_eval_pose3d')
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize('c', POSE3D_CASES, ids=[c['id'] for c in POSE3D_CASES])
def test_pose3d_against_fp64(c):
    """p2c_eval_pose3d through the C ABI (two-point hips on either side and a sparse 40-joint map have no skeleton class): the four
    state slots against mpjpe_update / mrpe_update, counts exactly. Without world locations slots 2 and 3 keep what was there.

    Worst ratios observed on an MI355X: MPJPE sum 6.9e-8, MRPE sum 4.8e-8."""
    d = _dev()
    pred, gt, wp, wg = pose3d_input(c)
    s0, n0, s1, n1 = pose3d_reference(pred, gt, wp, wg, c)
    start = torch.tensor([0.5, 3.0, -7.25, 11.0], dtype=torch.float64)
    state = start.to(d)
    world = (wp.to(d), wg.to(d)) if c['world'] else (None, None)
    _pose3d_abi(pred.to(d), gt.to(d), world[0], world[1], c, state)
    got = state.cpu() - start
    e0 = abs(float(got[0]) - s0) / s0
    e1 = abs(float(got[2]) - s1) / s1 if c['world'] else 0.0
    print(f'pose3d {c["id"]}: mpjpe {e0:.2e} mrpe {e1:.2e}')
    assert float(got[1]) == n0 == c['B']
    if c['world']:
        assert float(got[3]) == n1 == c['B']
    else:
        assert float(state[2]) == -7.25 and float(state[3]) == 11.0
    assert e0 <= TOL_VALUE and e1 <= TOL_VALUE, (e0, e1)


@pytest.mark.gpu
def test_metric_classes_accumulate_over_updates():
    """MPJPE (CARLA and BODY_25 targets) and MRPE through their classes: three updates of different batch sizes add their sums
    into one state, the counts are exact, compute() is within 1e-5 relative."""
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla_amd.metrics import MPJPE, MRPE
    d = _dev()
    for kind, metric in (('carla26', MPJPE()), ('body25', MPJPE(input_nodes=BODY_25_SKELETON, output_nodes=CARLA_SKELETON)),
                         ('carla26', MRPE())):
        c = _pose3d_case(0, 16, kind, 1, 1, True, 31)
        c['pred_hips'] = c['gt_hips'] = [O.HIPS]
        tot, cnt = 0.0, 0
        for B in (3, 513, 9):
            pred, gt, wp, wg = pose3d_input(c, B)
            dp, dg = torch.randn(B, 16, 3, generator=_gen(B)) * 0.05, torch.randn(B, 16, 3, generator=_gen(B + 1)) * 0.05
            metric.update({'absolute_pose_loc': pred.to(d), 'world_loc_changes': dp.to(d)},
                          {'absolute_pose_loc': gt.to(d), 'world_loc_changes': dg.to(d)})
            ref = pose3d_reference(pred, gt, OM.world_loc_from_changes(dp.double()), OM.world_loc_from_changes(dg.double()), c)
            s, n = ref[2:] if isinstance(metric, MRPE) else ref[:2]
            tot, cnt = tot + s, cnt + n
        state = metric._state.cpu()
        k = 2 if isinstance(metric, MRPE) else 0
        print(f'classes {type(metric).__name__} {kind}: sum {abs(float(state[k]) - tot) / tot:.2e}')
        assert float(state[k + 1]) == cnt == 525
        assert abs(float(state[k]) - tot) <= TOL_VALUE * tot
        assert abs(float(metric.compute()) - 1000 * tot / cnt) <= 1e-5 * 1000 * tot / cnt
        if not isinstance(metric, MRPE):
            assert float(state[2]) == 0.0 and float(state[3]) == 0.0


def _pck_abi(pred, gt, src, c, state, hips_idx=None, neck_idx=None):
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    N = pred.shape[0]
    part = torch.empty(lib.p2c_eval_workspace_floats(N), dtype=torch.float32, device=pred.device)
    hips_idx, neck_idx = hips_idx or c['hips_idx'], neck_idx or c['neck_idx']
    rc = lib.p2c_eval_pck(pred.data_ptr(), gt.data_ptr(), None if src is None else src.data_ptr(), N, c['Jp'], c['Cp'], c['Jg'],
                          c['Cg'], _iarr(c['pmap']), int(c['mask']), c['hips_joint'], c['mode'], _iarr(hips_idx), len(hips_idx),
                          _iarr(neck_idx), len(neck_idx), c['threshold'], NZ, part.data_ptr(), state.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.gpu
@pytest.mark.parametrize('c', PCK_CASES, ids=[c['id'] for c in PCK_CASES])
def test_pck_counts_equal_fp64(c):
    """p2c_eval_pck: correct and total equal to OM.pck_update in fp64, exactly; state[1] and state[3] untouched. The kernel decides
    dist < threshold in fp32: the builder has moved every counted joint within a relative 1e-4 of the threshold away from it (fp32
    rounding over these few operations is of order 1e-6), and the fp64 counts at threshold (1 +- 1e-4) are asserted equal first --
    a condition on the inputs, not a tolerance on the kernel."""
    d = _dev()
    pred, gt, src = pck_input(c)
    assert pck_band_is_empty(pred, gt, src, c)
    correct, total = pck_reference(pred, gt, src, c)
    start = torch.tensor([2.0, -3.5, 5.0, 9.25], dtype=torch.float64)
    state = start.to(d)
    gd = gt.to(d)
    rc = _pck_abi(pred.to(d), gd, src.to(d) if c['own_src'] else None, c, state)
    assert rc == 0
    got = state.cpu()
    print(f'pck {c["id"]}: correct {int(got[0] - 2)} / {correct}, total {int(got[2] - 5)} / {total}')
    assert float(got[1]) == -3.5 and float(got[3]) == 9.25
    assert (float(got[0]) - 2.0, float(got[2]) - 5.0) == (float(correct), float(total))


# ---- refusals: the documented code, and nothing written ---------------------------------------------------------------------------
SENTINEL = -12345.5


def _refusals(fn_name, base, outputs, cases):
    """base: ordered {argument: value} of a valid call (device tensors stand for their pointers); cases: (label, {argument: value},
    code). Every case must come back with its code and leave each tensor of ``outputs`` at the sentinel."""
    from pedestrians_video_2_carla_amd import _lib
    fn = getattr(_lib.lib(), fn_name)
    seen = []
    for label, change, code in cases:
        assert set(change) <= set(base), (fn_name, label)
        args = dict(base, **change)
        rc = fn(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args.values()])
        torch.cuda.synchronize()
        seen.append((label, rc, code))
        for name in outputs:
            t = base[name]
            assert bool((t == SENTINEL).all()), (fn_name, label, name, 'written by a refused call')
    wrong = [s for s in seen if s[1] != s[2]]
    assert not wrong, (fn_name, wrong)


def _buf(n, d, dtype=torch.float32):
    return torch.full((n,), SENTINEL, dtype=dtype, device=d)


@pytest.mark.gpu
def test_aux_entry_points_refuse_bad_arguments():
    """p2c_normalize_fwd / _bwd, p2c_loss2d_fwd / _bwd, p2c_remap_nodes: every NULL, shape, enum and index check. (The normaliser
    answers a hips / neck COUNT outside 1..2 with P2C_E_INDEX: the count belongs to the index list.)"""
    d = _dev()
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.randn(4 * 26 * 3, device=d)
    norm_tail = dict(N=4, J=26, C=3, dim=2, transform=3, n_hips=1, hips=_iarr([1]), n_neck=1, neck=_iarr([8]), near_zero=NZ,
                     stream=stream)
    norm_cases_ = [
        ('x NULL', dict(x=None), E_NULL),
        ('N < 0', dict(N=-1), E_SHAPE), ('J = 0', dict(J=0), E_SHAPE), ('J = 65', dict(J=65), E_SHAPE),
        ('dim = 4', dict(dim=4, C=4), E_SHAPE), ('dim = 1', dict(dim=1), E_SHAPE), ('C < dim', dict(C=1), E_SHAPE),
        ('C < dim 3', dict(dim=3, transform=1, C=2), E_SHAPE),
        ('transform none', dict(transform=0), E_ENUM), ('transform 4', dict(transform=4), E_ENUM),
        ('dim 3 bbox', dict(dim=3, transform=2), E_ENUM), ('dim 3 hips_neck_bbox', dict(dim=3, transform=3), E_ENUM),
        ('hips NULL', dict(hips=None), E_INDEX), ('neck NULL', dict(neck=None), E_INDEX),
        ('n_hips 0', dict(n_hips=0), E_INDEX), ('n_hips 3', dict(n_hips=3, hips=_iarr([1, 2, 3])), E_INDEX),
        ('n_neck 0', dict(n_neck=0), E_INDEX), ('n_neck 3', dict(n_neck=3, neck=_iarr([1, 2, 3])), E_INDEX),
        ('hips -1', dict(hips=_iarr([-1])), E_INDEX), ('hips J', dict(hips=_iarr([26])), E_INDEX),
        ('second hips J', dict(n_hips=2, hips=_iarr([1, 26])), E_INDEX),
        ('neck -1', dict(neck=_iarr([-1])), E_INDEX), ('neck J', dict(neck=_iarr([26])), E_INDEX),
        ('second neck -1', dict(n_neck=2, neck=_iarr([8, -1])), E_INDEX),
        ('hips_neck with a bad neck', dict(transform=1, neck=_iarr([64])), E_INDEX),
    ]
    fwd = dict(x=x, out=_buf(x.numel(), d), shift=_buf(8, d), scale=_buf(4, d), **norm_tail)
    _refusals('p2c_normalize_fwd', fwd, ('out', 'shift', 'scale'), norm_cases_ + [('out NULL', dict(out=None), E_NULL)])
    bwd = dict(x=x, grad_out=x.clone(), grad_x=_buf(x.numel(), d), **norm_tail)
    _refusals('p2c_normalize_bwd', bwd, ('grad_x',), norm_cases_ + [('grad_out NULL', dict(grad_out=None), E_NULL),
                                                                     ('grad_x NULL', dict(grad_x=None), E_NULL)])

    pred, gt = torch.randn(3 * 26 * 3, device=d), torch.randn(3 * 25 * 2, device=d)
    big = _iarr(list(range(65)))
    loss_head = dict(pred=pred, gt=gt, N=3, Jp=26, Cp=3, Jg=25, Cg=2, K=4, pidx=_iarr([0, 5, 7, 25]), gidx=_iarr([1, 2, 24, 3]),
                     hips_col=1, mask=1)
    loss_cases_ = [
        ('pred NULL', dict(pred=None), E_NULL), ('gt NULL', dict(gt=None), E_NULL), ('pidx NULL', dict(pidx=None), E_NULL),
        ('gidx NULL', dict(gidx=None), E_NULL),
        ('N < 0', dict(N=-1), E_SHAPE), ('Jp = 0', dict(Jp=0), E_SHAPE), ('Jg = 0', dict(Jg=0), E_SHAPE),
        ('Cp = 1', dict(Cp=1), E_SHAPE), ('Cg = 1', dict(Cg=1), E_SHAPE), ('K = 0', dict(K=0), E_SHAPE),
        ('K = 65', dict(K=65, pidx=big, gidx=big), E_SHAPE), ('Jp = 257', dict(Jp=257), E_SHAPE),
        ('hips_col -2', dict(hips_col=-2), E_INDEX), ('hips_col K', dict(hips_col=4), E_INDEX),
        ('pidx -1', dict(pidx=_iarr([0, 5, -1, 25])), E_INDEX), ('pidx Jp', dict(pidx=_iarr([0, 5, 7, 26])), E_INDEX),
        ('gidx -1', dict(gidx=_iarr([-1, 2, 24, 3])), E_INDEX), ('gidx Jg', dict(gidx=_iarr([1, 2, 25, 3])), E_INDEX),
    ]
    fwd = dict(loss_head, partials=_buf(16384, d), loss_sums=_buf(2, d), loss=_buf(1, d), stream=stream)
    _refusals('p2c_loss2d_fwd', fwd, ('partials', 'loss_sums', 'loss'), loss_cases_ + [
        ('partials NULL', dict(partials=None), E_NULL), ('loss_sums NULL', dict(loss_sums=None), E_NULL),
        ('loss NULL', dict(loss=None), E_NULL)])
    bwd = dict(loss_head, loss_sums=torch.ones(2, device=d), grad_loss=torch.ones(1, device=d), grad_pred=_buf(pred.numel(), d),
               stream=stream)
    _refusals('p2c_loss2d_bwd', bwd, ('grad_pred',), loss_cases_ + [
        ('loss_sums NULL', dict(loss_sums=None), E_NULL), ('grad_loss NULL', dict(grad_loss=None), E_NULL),
        ('grad_pred NULL', dict(grad_pred=None), E_NULL)])

    remap = dict(src=torch.randn(3 * 25 * 2, device=d), dst=_buf(3 * 26 * 2, d), N=3, Jsrc=25, Jdst=26, C=2, K=3,
                 src_idx=_iarr([0, 24, 7]), dst_idx=_iarr([25, 0, 3]), stream=stream)
    _refusals('p2c_remap_nodes', remap, ('dst',), [
        ('src NULL', dict(src=None), E_NULL), ('dst NULL', dict(dst=None), E_NULL), ('src_idx NULL', dict(src_idx=None), E_NULL),
        ('dst_idx NULL', dict(dst_idx=None), E_NULL),
        ('N < 0', dict(N=-1), E_SHAPE), ('Jsrc = 0', dict(Jsrc=0), E_SHAPE), ('Jdst = 0', dict(Jdst=0), E_SHAPE),
        ('Jdst = 65', dict(Jdst=65), E_SHAPE), ('C = 0', dict(C=0), E_SHAPE), ('K < 0', dict(K=-1), E_SHAPE),
        ('K = 65', dict(K=65, src_idx=big, dst_idx=big), E_SHAPE),
        ('src_idx -1', dict(src_idx=_iarr([0, -1, 7])), E_INDEX), ('src_idx Jsrc', dict(src_idx=_iarr([0, 25, 7])), E_INDEX),
        ('dst_idx -1', dict(dst_idx=_iarr([-1, 0, 3])), E_INDEX), ('dst_idx Jdst', dict(dst_idx=_iarr([25, 0, 26])), E_INDEX)])


@pytest.mark.gpu
def test_eval_entry_points_refuse_bad_arguments():
    """p2c_eval_pose3d and p2c_eval_pck: every NULL, shape and index check, among them the hips / neck joints of PCK's norm_mode 1
    outside [0, Jg) -- once copied unchecked, so that the kernel's shuffle read a lane of the neighbouring frame or an inactive one
    and the call returned 0."""
    d = _dev()
    stream = torch.cuda.current_stream().cuda_stream
    gmap = [j if j < 25 else -1 for j in range(26)]
    pose = dict(pred=torch.randn(3 * 4 * 26 * 3, device=d), gt=torch.randn(3 * 4 * 25 * 3, device=d), B=3, T=4, Jg=25, gmap=_iarr(gmap),
                pred_hips=_iarr([1]), n_pred_hips=1, gt_hips=_iarr([8]), n_gt_hips=1, world_pred=torch.randn(36, device=d),
                world_gt=torch.randn(36, device=d), partials=_buf(64, d), state=_buf(4, d, torch.float64), stream=stream)
    _refusals('p2c_eval_pose3d', pose, ('partials', 'state'), [
        ('pred NULL', dict(pred=None), E_NULL), ('gt NULL', dict(gt=None), E_NULL), ('gmap NULL', dict(gmap=None), E_NULL),
        ('partials NULL', dict(partials=None), E_NULL), ('state NULL', dict(state=None), E_NULL),
        ('world_pred alone', dict(world_gt=None), E_NULL), ('world_gt alone', dict(world_pred=None), E_NULL),
        ('B < 0', dict(B=-1), E_SHAPE), ('T = 0', dict(T=0), E_SHAPE), ('Jg = 0', dict(Jg=0), E_SHAPE),
        ('n_pred_hips 0', dict(n_pred_hips=0), E_SHAPE), ('n_pred_hips 3', dict(n_pred_hips=3, pred_hips=_iarr([1, 2, 3])), E_SHAPE),
        ('n_gt_hips 0', dict(n_gt_hips=0), E_SHAPE), ('n_gt_hips 3', dict(n_gt_hips=3, gt_hips=_iarr([1, 2, 3])), E_SHAPE),
        ('no common joint', dict(gmap=_iarr([-1] * 26)), E_SHAPE),
        ('gmap -2', dict(gmap=_iarr([-2] + gmap[1:])), E_INDEX), ('gmap Jg', dict(gmap=_iarr(gmap[:25] + [25])), E_INDEX),
        ('pred_hips -1', dict(pred_hips=_iarr([-1])), E_INDEX), ('pred_hips 26', dict(pred_hips=_iarr([26])), E_INDEX),
        ('second pred_hips 26', dict(n_pred_hips=2, pred_hips=_iarr([1, 26])), E_INDEX),
        ('gt_hips -1', dict(gt_hips=_iarr([-1])), E_INDEX), ('gt_hips Jg', dict(gt_hips=_iarr([25])), E_INDEX),
        ('second gt_hips Jg', dict(n_gt_hips=2, gt_hips=_iarr([8, 25])), E_INDEX)])

    pck = dict(pred=torch.randn(5 * 26 * 2, device=d), gt=torch.randn(5 * 25 * 2, device=d), mask_src=None, N=5, Jp=26, Cp=2, Jg=25, Cg=2,
               pmap=_iarr(list(range(25))), mask_missing=1, hips_joint=8, norm_mode=1, hips_idx=_iarr([8]), n_hips=1,
               neck_idx=_iarr([1]), n_neck=1, threshold=0.05, near_zero=NZ, partials=_buf(64, d), state=_buf(4, d, torch.float64),
               stream=stream)
    _refusals('p2c_eval_pck', pck, ('partials', 'state'), [
        ('pred NULL', dict(pred=None), E_NULL), ('gt NULL', dict(gt=None), E_NULL), ('pmap NULL', dict(pmap=None), E_NULL),
        ('partials NULL', dict(partials=None), E_NULL), ('state NULL', dict(state=None), E_NULL),
        ('N < 0', dict(N=-1), E_SHAPE), ('Jp = 0', dict(Jp=0), E_SHAPE), ('Jg = 0', dict(Jg=0), E_SHAPE),
        ('Jg = 65', dict(Jg=65, pmap=_iarr([-1] * 65)), E_SHAPE), ('Cp = 1', dict(Cp=1), E_SHAPE), ('Cg = 1', dict(Cg=1), E_SHAPE),
        ('norm_mode 2', dict(norm_mode=2), E_SHAPE), ('norm_mode -1', dict(norm_mode=-1), E_SHAPE),
        ('pmap -2', dict(pmap=_iarr([-2] + list(range(1, 25)))), E_INDEX), ('pmap Jp', dict(pmap=_iarr(list(range(24)) + [26])), E_INDEX),
        ('hips_idx NULL', dict(hips_idx=None), E_INDEX), ('neck_idx NULL', dict(neck_idx=None), E_INDEX),
        ('n_hips 0', dict(n_hips=0), E_INDEX), ('n_hips 3', dict(n_hips=3, hips_idx=_iarr([1, 2, 3])), E_INDEX),
        ('n_neck 0', dict(n_neck=0), E_INDEX), ('n_neck 3', dict(n_neck=3, neck_idx=_iarr([1, 2, 3])), E_INDEX),
        ('hips_idx -1', dict(hips_idx=_iarr([-1])), E_INDEX), ('hips_idx Jg', dict(hips_idx=_iarr([25])), E_INDEX),
        ('hips_idx 40, a lane of the next frame', dict(hips_idx=_iarr([40])), E_INDEX),
        ('second hips_idx Jg', dict(n_hips=2, hips_idx=_iarr([8, 25])), E_INDEX),
        ('neck_idx -1', dict(neck_idx=_iarr([-1])), E_INDEX), ('neck_idx Jg', dict(neck_idx=_iarr([25])), E_INDEX),
        ('second neck_idx -1', dict(n_neck=2, neck_idx=_iarr([1, -1])), E_INDEX)])
