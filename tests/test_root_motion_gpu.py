"""K40 (csrc/p2c_root_motion.hip) on the device: against the fp64 definition, the exactness of the integer sum (the formula of
the output row on the kernel's own steps, the two mappings, grids, requests, cuts of the video), streaming, the dispatch, the
edge cases and the two audit modes.

Inputs, shapes and the margin condition come from tests/test_root_motion.py: ``walk_rows(N, T, seed=N)`` rounded to fp32, N in
{1, 3, 5} and T in {1, 2, F - 1, F, F + 1, 2 F + 3} with F the tile length the library reports. Frames whose best and second-best
``m_k`` are closer than ``MARGIN`` in the fp64 definition are excluded from the comparison of contact and steps (at most 5 % of
a shape's frames, asserted there on the host); everything else holds on every frame.

Allowance. Coordinates stay below about 400 units (here: root locations within 100, a skeleton of about one unit), where an fp32
value carries an error of at most 2^-16; the difference of two ``p_k`` is then off by far less than one quantum (2^-10), and two
values less than one apart round to integers at most 1 apart: steps within +-1 quantum.
"""
import functools

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.walker_control import root_motion as rm
from pedestrians_video_2_carla_amd.walker_control.root_motion import CarlaRootMotion
from test_root_motion import GPU_N, GPU_T, MARGIN, Q, TILE, walk_rows

pytestmark = pytest.mark.gpu

SHAPES = [(N, T) for N in GPU_N for T in GPU_T]
ALL = ('root', 'steps', 'contact')


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def problem(N, T):
    """fp32 rows on the host, rounded from the fp64 recipe."""
    bones, root = walk_rows(N, T, seed=N)
    return bones.float(), root.float()


@functools.lru_cache(maxsize=None)
def reference(N, T, ground=None):
    """The fp64 definition on the fp32 inputs, on the host, once per shape: its outputs, the contact points and the margins."""
    bones, root = (t.double() for t in problem(N, T))
    out = ops.root_motion_carla_rows(bones, root, want=ALL, ground=ground)
    points = rm.contact_points(bones, root)
    out['points'], out['margin'] = points, rm.frame_steps(points, None)[3]
    return out


def run(N, T, root=True, **kw):
    bones, rows = (t.to(dev()) for t in problem(N, T))
    kw.setdefault('want', ALL)
    return ops.root_motion_carla_rows(bones, rows if root else None, **kw)


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a if k != 'state') and all(torch.equal(x, y) for x, y in zip(a['state'], b['state']))


def test_the_tile_length_and_the_workspace_query():
    lib = _lib.lib()
    assert ops.root_motion_tile() == TILE                                       # the shapes of this file and of the margin condition
    assert lib.p2c_carla_root_motion_workspace(5, TILE, 0) == 0 and lib.p2c_carla_root_motion_workspace(5, 3 * TILE, 1) == 0
    frames, up = 5 * (2 * TILE + 3), lambda v: (v + 15) // 16 * 16                # three tiles a video; every part 16-byte aligned
    assert lib.p2c_carla_root_motion_workspace(5, 2 * TILE + 3, 2) == up(5 * 3 * 16) + up(frames * 8) + up(frames * 4) + up(frames)
    assert lib.p2c_carla_root_motion_workspace(-1, 4, 0) == -1 and lib.p2c_carla_root_motion_workspace(1, 4, 3) == -1
    # the default: a workgroup per video where a video is one tile or the videos fill the chip, frame-parallel below that
    assert lib.p2c_carla_root_motion_workspace(1024, 2 * TILE, 0) == 0 and lib.p2c_carla_root_motion_workspace(2, 2 * TILE, 0) > 0
    assert lib.p2c_carla_root_motion_workspace(1023, 2 * TILE, 0) == lib.p2c_carla_root_motion_workspace(1023, 2 * TILE, 2) > 0


# --------------------------------------------------------------------------------------------------- against the fp64 definition
@pytest.mark.parametrize('N,T', SHAPES)
def test_against_the_fp64_definition(N, T):
    ref, got = reference(N, T), run(N, T)
    root_in = problem(N, T)[1]
    fair = ref['margin'] >= MARGIN
    contact, steps = got['contact'].cpu(), got['steps'].cpu()
    assert contact.dtype == torch.int8 and steps.dtype == torch.int32 and got['root'].dtype == torch.float32
    step_error = (steps.long() - ref['steps'].long()).abs()
    point_error = float((got['state'][1].cpu().double() - ref['points'][:, -1]).abs().max()) / Q
    print(f'N {N} T {T}: {int((~fair).sum())} frames excluded; contact differs on {int((contact[fair] != ref["contact"][fair]).sum())}, '
          f'largest step difference {int(step_error[fair].max()) if fair.any() else 0} quanta on fair frames, '
          f'{int(step_error.max())} on all; steps that differ {float((step_error[fair] > 0).double().mean()):.4f}; '
          f'last frame p_k off by {point_error:.4f} quanta')
    assert torch.equal(contact[fair], ref['contact'][fair])
    assert int(step_error[fair].max()) <= 1
    assert torch.equal(got['root'].cpu()[..., 2:].view(torch.int32), root_in[..., 2:].view(torch.int32))    # bit for bit
    assert point_error < 1.0


# ------------------------------------------------------------------------------------------------------- exactness, bit for bit
@pytest.mark.parametrize('N,T', SHAPES)
def test_the_row_is_the_formula_on_the_kernels_own_steps_in_every_mapping_and_grid(N, T):
    got = run(N, T)
    root_in = problem(N, T)[1]
    S = torch.cumsum(got['steps'].cpu().long(), 1)
    want_xy = (root_in[..., :2].double() + S.double() * Q).float()
    assert torch.equal(got['root'].cpu()[..., :2], want_xy) and torch.equal(got['state'][0].cpu(), S[:, -1])
    assert int(S.abs().max()) > 0 or T == 1
    for kw in (dict(mapping=1), dict(mapping=2), dict(mapping='per_video'), dict(mapping='frame_parallel'), dict(max_blocks=1),
               dict(mapping=1, max_blocks=1), dict(mapping=2, max_blocks=1), dict(mapping=2, max_blocks=2)):
        assert same(run(N, T, **kw), got), kw
    for mapping in (None, 1, 2):
        only = run(N, T, want=('root',), mapping=mapping)
        assert set(only) == {'root', 'state'} and torch.equal(only['root'], got['root'])
        pair = run(N, T, want=('contact', 'steps'), mapping=mapping)
        assert set(pair) == {'contact', 'steps', 'state'} and torch.equal(pair['steps'], got['steps']) and torch.equal(pair['contact'], got['contact'])


@pytest.mark.parametrize('mapping', [1, 2])
def test_a_static_video_keeps_its_root(mapping):
    T = TILE + 1
    bones, root = (t[:, :1].repeat(1, T, *([1] * (t.ndim - 2))).to(dev()) for t in problem(3, 2))
    out = ops.root_motion_carla_rows(bones, root, want=ALL, mapping=mapping)
    assert torch.equal(out['root'].view(torch.int32), root.view(torch.int32)) and int(out['steps'].abs().max()) == 0
    assert int(out['contact'].min()) >= 0 and int(out['state'][0].abs().max()) == 0


@pytest.mark.parametrize('mapping', [1, 2])
@pytest.mark.parametrize('cut', [1, TILE, TILE + 1])
def test_the_state_continues_a_cut_video(cut, mapping):
    N, T = 3, 2 * TILE + 3
    whole = run(N, T)
    bones, root = (t.to(dev()) for t in problem(N, T))
    head = ops.root_motion_carla_rows(bones[:, :cut], root[:, :cut], want=ALL, mapping=mapping)
    tail = ops.root_motion_carla_rows(bones[:, cut:], root[:, cut:], want=ALL, mapping=mapping, state=head['state'], first_frame=cut)
    for k in ALL:
        assert torch.equal(head[k], whole[k][:, :cut]) and torch.equal(tail[k], whole[k][:, cut:]), k
    assert all(torch.equal(a, b) for a, b in zip(tail['state'], whole['state']))
    other = ops.root_motion_carla_rows(bones[:, cut:], root[:, cut:], want=ALL, mapping=3 - mapping, state=head['state'], first_frame=cut)
    assert same(other, tail)


# ------------------------------------------------------------------------------------------------------- streaming and dispatch
@pytest.mark.parametrize('ground', [None, 2.5])
def test_pushed_chunks_give_the_bits_of_the_uncut_video(ground):
    N, T = 3, 2 * TILE + 3
    bones, root = (t.to(dev()) for t in problem(N, T))
    mover = CarlaRootMotion(ground=ground)
    want = mover.apply(bones, root)[1]
    for chunk in (TILE - 1, 100):
        mover.reset()
        got = torch.cat([mover.push(bones[:, t:t + chunk], root[:, t:t + chunk])[1] for t in range(0, T, chunk)], 1)
        assert torch.equal(got, want) and mover.frames == T


def test_the_framework_switch_and_host_tensors_take_the_definition(monkeypatch):
    N, T = 3, TILE + 1
    ref, got = reference(N, T), run(N, T)
    fair = ref['margin'] >= MARGIN

    def refuse(*a):
        raise AssertionError('the kernel entry point was called')
    monkeypatch.setattr(_lib.lib(), 'p2c_carla_root_motion_fwd', refuse)
    with pytest.raises(AssertionError):
        run(N, T)                                                               # the patch is where the device path goes
    with pytest.raises(AssertionError):
        run(N, T, state=got['state'], first_frame=T)                            # and a call that continues a video
    monkeypatch.setenv('P2C_ROOT_MOTION_FRAMEWORK', '1')
    on_device = run(N, T)
    monkeypatch.delenv('P2C_ROOT_MOTION_FRAMEWORK')
    bones, root = problem(N, T)
    on_host = ops.root_motion_carla_rows(bones, root, want=ALL)
    f64 = ops.root_motion_carla_rows(*(t.double().to(dev()) for t in problem(N, T)), want=ALL)
    for out, where in ((on_device, 'cuda'), (on_host, 'cpu'), (f64, 'cuda')):
        assert out['root'].device.type == where and out['state'][1].dtype == out['root'].dtype
        assert torch.equal(out['contact'].cpu()[fair], ref['contact'][fair])
        assert int((out['steps'].cpu().long() - ref['steps'].long()).abs()[fair].max()) <= 1
    monkeypatch.undo()
    assert same(run(N, T), got)


# -------------------------------------------------------------------------------------------------------------------- edge cases
@pytest.mark.parametrize('mapping', [1, 2])
def test_without_a_root_and_on_views(mapping):
    N, T = 3, TILE + 1
    bones, root = (t.to(dev()) for t in problem(N, T))
    alone = ops.root_motion_carla_rows(bones, None, want=ALL, mapping=mapping)
    zeros = ops.root_motion_carla_rows(bones, torch.zeros_like(root), want=ALL, mapping=mapping)
    assert same(alone, zeros) and int(alone['steps'].abs().max()) > 0
    wide_b = torch.full((N, 2 * T, 26, 7), float('nan'), device=dev())
    wide_r = torch.full((N, 2 * T, 7), float('nan'), device=dev())
    wide_b[:, ::2, :, :6], wide_r[:, ::2, :6] = bones, root
    view_b, view_r = wide_b[:, ::2, :, :6], wide_r[:, ::2, :6]
    assert not view_b.is_contiguous() and not view_r.is_contiguous()
    assert same(ops.root_motion_carla_rows(view_b, view_r, want=ALL, mapping=mapping), run(N, T))
    empty = ops.root_motion_carla_rows(bones[:0], root[:0], want=ALL, mapping=mapping)
    assert empty['root'].shape == (0, T, 6) and empty['steps'].shape == (0, T, 2) and empty['root'].is_cuda
    with pytest.raises((ValueError, RuntimeError)):
        ops.root_motion_carla_rows(bones[:, :, :25], root)


@pytest.mark.parametrize('mapping', [1, 2])
@pytest.mark.parametrize('z0', [0.0, -41.5])
def test_the_ground_plane(z0, mapping):
    N, T = 5, TILE + 1
    ref, got, plain = reference(N, T, z0), run(N, T, ground=z0, mapping=mapping), run(N, T)
    root_in = problem(N, T)[1]
    low = (-ref['points'][..., 2]).min(-1).values
    size = torch.stack((root_in[..., 2].double().abs(), low.abs(), (z0 - low).abs(), ref['root'][..., 2].abs(),
                        torch.full_like(low, abs(z0)))).max(0).values
    ulp = torch.from_numpy(np.spacing(size.float().numpy())).double()
    off = (got['root'].cpu()[..., 2].double() - ref['root'][..., 2]).abs() / ulp
    print(f'ground {z0} mapping {mapping}: z off by at most {float(off.max()):.3f} fp32 ulp of the magnitudes involved')
    assert float(off.max()) <= 2.0
    for k in ('steps', 'contact'):
        assert torch.equal(got[k], plain[k])
    assert torch.equal(got['root'][..., :2], plain['root'][..., :2]) and torch.equal(got['root'][..., 3:], plain['root'][..., 3:])


def test_a_nan_row_on_the_device():
    N, T = 3, TILE + 1
    bones, root = (t.to(dev()) for t in problem(N, T))
    clean = run(N, T)
    bad = bones.clone()
    bad[1, TILE - 1, 21] = float('nan')                                        # the pair that spans two tiles is dropped too
    for mapping in (1, 2):
        out = ops.root_motion_carla_rows(bad, root, want=ALL, mapping=mapping, ground=0.0)
        assert out['contact'][1, TILE - 1] == -1 and out['contact'][1, TILE] == -1 and int(out['steps'][1, TILE - 1:].abs().max()) == 0
        assert torch.equal(out['steps'][1, :TILE - 1], clean['steps'][1, :TILE - 1])
        assert bool(torch.isnan(out['root'][1, TILE - 1, 2])) and bool(torch.isfinite(out['root'][1, :TILE - 1]).all())
        assert bool(torch.isfinite(out['root'][..., :2]).all())
        for k in ('steps', 'contact'):
            assert torch.equal(out[k][[0, 2]], clean[k][[0, 2]])


def test_the_abi_refuses_before_it_launches():
    lib = _lib.lib()
    bones, root = (t.to(dev()) for t in problem(1, 2))
    out = torch.zeros(1, 2, 6, device=dev())
    S, P = torch.zeros(1, 2, dtype=torch.int64, device=dev()), torch.zeros(1, 4, 3, device=dev())
    b, r, o, s, p = bones.data_ptr(), root.data_ptr(), out.data_ptr(), S.data_ptr(), P.data_ptr()

    def call(bones=b, root=r, s_in=None, p_in=None, out_root=o, s_out=None, p_out=None, N=1, T=2, first=0, ground=0.0, has=0, mapping=0,
             max_blocks=0, ws=None):
        return lib.p2c_carla_root_motion_fwd(bones, root, s_in, p_in, out_root, None, None, s_out, p_out, N, T, first, ground, has,
                                             mapping, max_blocks, ws, None)
    SHAPE, NULL, ENUM = -2, -1, -3
    assert call() == 0 and call(root=None) == 0 and call(N=0, bones=None, out_root=None) == NULL
    for kw in (dict(N=-1), dict(T=-1), dict(first=-1), dict(max_blocks=-1), dict(has=2), dict(has=1, ground=float('nan')),
               dict(has=1, ground=1e39), dict(N=1 << 41), dict(N=1 << 30, T=1 << 30)):
        assert call(**kw) == SHAPE, kw
    assert call(mapping=3) == ENUM and call(mapping=-1) == ENUM
    for kw in (dict(bones=None), dict(out_root=None), dict(s_in=s), dict(p_in=p), dict(s_out=s), dict(p_out=p), dict(first=1),
               dict(mapping=2, T=2)):
        assert call(**kw) == NULL, kw
    assert call(N=0) == 0 and call(T=0) == 0 and call(T=0, mapping=2) == 0 and call(first=1, s_in=s, p_in=p) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the audits
def test_under_the_two_audit_modes_the_bits_stay(monkeypatch):
    """Every LDS byte NaN before each launch (``P2C_POISON_LDS=1``) and NaN- / INT_MAX-filled ``torch.empty``
    (``P2C_POISON_EMPTY=1``): an image slot or a total read before it was written, a workspace word of mapping B read before
    launch 1 wrote it, or an output element that was not written would change the bits."""
    N, T, cut = 3, 2 * TILE + 3, TILE + 1
    want = {m: run(N, T, mapping=m, ground=1.0) for m in (1, 2)}
    bones, root = (t.to(dev()) for t in problem(N, T))
    monkeypatch.setenv('P2C_POISON_LDS', '1')
    monkeypatch.setenv('P2C_POISON_EMPTY', '1')
    monkeypatch.setattr(_lib, '_lib', None)                  # the next lib() wraps every launch with the LDS poisoning
    deterministic, warn_only = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    monkeypatch.setattr(torch.utils.deterministic, 'fill_uninitialized_memory', True)
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        assert isinstance(_lib.lib(), _lib._PoisonedLib) and bool(torch.isnan(torch.empty(8, device=dev())).all())
        got = {m: run(N, T, mapping=m, ground=1.0) for m in (1, 2)}
        cuts = {}
        for m in (1, 2):
            head = ops.root_motion_carla_rows(bones[:, :cut], root[:, :cut], want=ALL, mapping=m, ground=1.0)
            cuts[m] = ops.root_motion_carla_rows(bones[:, cut:], root[:, cut:], want=ALL, mapping=m, ground=1.0, state=head['state'],
                                                 first_frame=cut)
        torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(deterministic, warn_only=warn_only)
    for m in (1, 2):
        assert same(got[m], want[m]) and bool(torch.isfinite(got[m]['root']).all())
        assert all(torch.equal(cuts[m][k], want[m][k][:, cut:]) for k in ALL)
