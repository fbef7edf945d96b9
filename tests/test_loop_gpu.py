"""K41 (csrc/p2c_loop.hip) on the device: the search against the fp64 definition, the choice as the first minimal entry of the
kernel's own costs, the planted period, bit stability across grids, requests, views and batches, NaN videos and rows; the player's
copies, its blended rows in matrix space, pieces against the whole; the dispatch, the C ABI's refusals and
``Trainer.predict_carla`` with a looper.

The allowance for a cost is the project's rule (tests/test_smooth_gpu.py): what the fp32 tensor restatement of the definition,
run on the device (``P2C_LOOP_FRAMEWORK=1``), is from fp64 on the same fp32 inputs is measured, and the kernel gets four times
that, with the floor ``J (blend + 1) 2^-21``. The floor is derived, not measured: an fp32 unit quaternion carries 2^-24 per
component, a four-term dot product four of those, ``1 - dot^2`` doubles it: 8 * 2^-24 a term, times the number of terms. Played
rows follow the rule of tests/test_resample_gpu.py: matrices through ``carla_pose_import``, ``MATRIX_FLOOR``, ``1e-6 max|loc|``,
four times the restatement's error.

Inputs are the planted-period paths of ``test_loop.gait_paths``. The period is well posed -- every case asserts on its fp64
reference that the cheapest pair at another period costs at least 10 times the best -- and the start ``s`` is not: the runner-up
at the same period can be within the floor of the best. So ``e - s`` is compared with the planted period, the pair itself only
with the kernel's own costs, and its fp64 cost with the fp64 optimum.
"""
import functools
import math

import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.walker_control import loop as lp
from pedestrians_video_2_carla_amd.walker_control.loop import CarlaLooper
from test_carla_pose_gpu import MATRIX_FLOOR
from test_loop import CASES, gait_paths, other_period_ratio

pytestmark = pytest.mark.gpu

# (case, max_blocks): the cases of test_loop.py -- one tile a side; no blend and a partial tile; several tiles, some off the band;
# one bone -- and the first again with two workgroups striding over the tiles
RUNS = [(0, 0), (0, 2), (1, 0), (2, 0), (3, 0)]
LOC_FLOOR = 1e-6
WELL_POSED = 10.0


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def problem(case):
    """fp32 rows on the host, rounded from the fp64 paths."""
    N, T, J, period = CASES[case][:4]
    bones, root = gait_paths(N, T, J, period)
    return bones.float(), root.float()


@functools.lru_cache(maxsize=None)
def reference(case):
    """The fp64 definition on the host, on the fp32 inputs of ``problem``."""
    blend, min_period, max_period = CASES[case][4:]
    return ops.find_carla_loop(problem(case)[0].double(), blend=blend, min_period=min_period, max_period=max_period,
                               want=('loop', 'cost'))


def floor_of(case):
    J, blend = CASES[case][2], CASES[case][4]
    return J * (blend + 1) * 2.0 ** -21


def search(bones, case, want=('loop', 'cost'), **kw):
    blend, min_period, max_period = CASES[case][4:]
    out = ops.find_carla_loop(bones, blend=blend, min_period=min_period, max_period=max_period, want=want, **kw)
    torch.cuda.synchronize()
    return out


def no_library():
    raise AssertionError('the library was asked for: a launch where none belongs')


def framework(monkeypatch, fn, *args, **kw):
    with monkeypatch.context() as m:
        m.setenv('P2C_LOOP_FRAMEWORK', '1')
        m.setattr(_lib, 'lib', no_library)
        out = fn(*args, **kw)
        torch.cuda.synchronize()
        return out


def cost_error(cost, want):
    cost = cost.double().cpu()
    assert torch.equal(torch.isinf(cost) & (cost > 0), torch.isinf(want))       # the +inf pattern
    finite = torch.isfinite(want)
    return float((cost[finite] - want[finite]).abs().max()) if bool(finite.any()) else 0.0


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


@pytest.mark.parametrize('case,max_blocks', RUNS)
def test_the_search_against_fp64_and_bit_stability(case, max_blocks, monkeypatch):
    N, T, J, period, blend, min_period, max_period = CASES[case]
    bones = problem(case)[0].to(dev())
    ref = reference(case)
    ratio = other_period_ratio(ref['cost'], ref['loop'], period)
    print(f'{CASES[case]}: fp64 best pairs {ref["loop"].tolist()} cost {ref["loop_cost"].tolist()}; another period costs {ratio:.1f} x')
    assert ratio >= WELL_POSED and bool((ref['loop'][:, 1] - ref['loop'][:, 0] == period).all())
    got = search(bones, case, max_blocks=max_blocks)
    cost, loop, loop_cost = got['cost'], got['loop'], got['loop_cost']
    assert cost.shape == (N, T, T) and cost.dtype == torch.float32 and cost.is_cuda
    assert loop.shape == (N, 2) and loop.dtype == torch.int64 and loop_cost.shape == (N,) and loop_cost.dtype == torch.float32
    fw = framework(monkeypatch, search, bones, case)
    fw_err, err = cost_error(fw['cost'], ref['cost']), cost_error(cost, ref['cost'])
    tol = max(4 * fw_err, floor_of(case))
    print(f'{CASES[case]} cap {max_blocks}: tensor restatement {fw_err:.3e}, K41 {err:.3e} from fp64 (allowed {tol:.3e}, floor '
          f'{floor_of(case):.3e})')
    assert math.isfinite(err) and err <= tol                              # 1
    host_cost = cost.cpu()
    for n in range(N):                                                     # 2: the first minimal entry of the kernel's own costs
        best = host_cost[n][torch.isfinite(host_cost[n])].min()
        first = (host_cost[n] == best).nonzero()[0].tolist()
        assert loop[n].tolist() == first
        chosen = host_cost[n, first[0], first[1]:first[1] + 1]
        assert loop_cost[n:n + 1].cpu().view(torch.int32).item() == chosen.clone().view(torch.int32).item()     # its bits
        s, e = first
        assert e - s == period                                             # 3
        optimum = float(ref['loop_cost'][n])
        print(f'  video {n}: K41 {first} fp64 cost {float(ref["cost"][n, s, e]):.4e}, fp64 optimum {optimum:.4e}')
        assert float(ref['cost'][n, s, e]) - optimum <= 2 * tol            # 4
    # 5: a repeat, the other grid, without the matrix, strided views of wider buffers, a video alone
    assert same(search(bones, case, max_blocks=max_blocks), got)
    assert same(search(bones, case, max_blocks=0 if max_blocks else 2), got)
    few = search(bones, case, want=('loop',), max_blocks=max_blocks)
    assert set(few) == {'loop', 'loop_cost'} and torch.equal(few['loop'], loop) and torch.equal(few['loop_cost'], loop_cost)
    wide = torch.zeros(N, 2 * T, J, 8, device=dev())
    wide[:, ::2, :, 1:7] = bones
    assert same(search(wide[:, ::2, :, 1:7], case, max_blocks=max_blocks), got)
    for n in range(N):
        alone = search(bones[n:n + 1], case)
        assert all(torch.equal(alone[k], got[k][n:n + 1]) for k in got)
    ones = search(bones, case, weights=torch.ones(J), max_blocks=max_blocks)
    assert same(ones, got)


def test_nan_videos_and_rows_go_where_the_windows_read_them():
    case = 0
    N, T, J, period, blend, min_period, max_period = CASES[case]
    bones = torch.cat((problem(case)[0], problem(case)[0][:1]), 0).to(dev())          # three videos
    clean = search(bones, case)
    nan = bones.clone()
    nan[1] = float('nan')
    got = search(nan, case)
    assert got['loop'][1].tolist() == [-1, -1] and math.isnan(float(got['loop_cost'][1]))      # 6
    admissible = lp.admissible(T, blend, min_period, max_period, dev())
    assert bool(torch.isnan(got['cost'][1][admissible]).all()) and bool(torch.isinf(got['cost'][1][~admissible]).all())
    for n in (0, 2):
        assert all(torch.equal(got[k][n], clean[k][n]) for k in got)
    one = bones.clone()                                                    # 7: one row, next to a tile's edge
    t0 = 31
    one[0, t0, 7] = float('nan')
    got = search(one, case)
    s_idx, e_idx = torch.arange(T, device=dev()).unsqueeze(1), torch.arange(T, device=dev()).unsqueeze(0)
    reads = torch.zeros(T, T, dtype=torch.bool, device=dev())
    for k in range(-blend, 1):
        reads |= (s_idx + k == t0) | (e_idx + k == t0)
    poisoned = reads & admissible
    assert torch.equal(torch.isnan(got['cost'][0]), poisoned) and bool(poisoned.any())
    assert torch.equal(got['cost'][0][~poisoned], clean['cost'][0][~poisoned])
    assert torch.equal(got['cost'][1:], clean['cost'][1:]) and torch.equal(got['loop'][1:], clean['loop'][1:])
    s, e = got['loop'][0].tolist()
    assert not bool(poisoned[s, e]) and e - s == period
    # 8: too short for any admissible pair, with and without the matrix; the shortest video that has one
    for T_short in (2, blend + min_period):
        short = search(bones[:, :T_short].contiguous(), case)
        assert short['loop'].tolist() == [[-1, -1]] * 3 and bool(torch.isnan(short['loop_cost']).all())
        assert bool((torch.isinf(short['cost']) & (short['cost'] > 0)).all())
        assert search(bones[:, :T_short], case, want=('loop',))['loop'].tolist() == [[-1, -1]] * 3
    assert search(bones[:, :blend + min_period + 1], case)['loop'].tolist() == [[blend, blend + min_period]] * 3


def test_more_bones_than_an_image_and_the_widest_blend(monkeypatch):
    """blend = 32 makes 64 frames a side and an image of 23 bones: J = 26 takes two chunks. The costs are those of the definition
    and a bone's share is what it is in a call of its own."""
    N, T, J, period, blend = 1, 70, 26, 16, 32
    bones = gait_paths(N, T, J, period, seed=3)[0].float()
    kw = dict(blend=blend, min_period=8, max_period=30, want=('loop', 'cost'))
    ref = ops.find_carla_loop(bones.double(), **kw)
    got = ops.find_carla_loop(bones.to(dev()), **kw)
    torch.cuda.synchronize()
    fw_err = cost_error(framework(monkeypatch, ops.find_carla_loop, bones.to(dev()), **kw)['cost'], ref['cost'])
    err, tol = cost_error(got['cost'], ref['cost']), max(4 * fw_err, J * (blend + 1) * 2.0 ** -21)
    print(f'blend 32, J 26: tensor restatement {fw_err:.3e}, K41 {err:.3e} from fp64 (allowed {tol:.3e})')
    assert err <= tol and int(got['loop'][0, 1] - got['loop'][0, 0]) == period and int(got['loop'][0, 0]) >= blend
    w = torch.zeros(J)
    w[24] = 1.0                                                            # a bone of the second chunk
    tail = ops.find_carla_loop(bones.to(dev()), weights=w, **kw)
    alone = ops.find_carla_loop(bones[:, :, 24:25].to(dev()), **kw)
    assert torch.equal(tail['cost'], alone['cost']) and torch.equal(tail['loop'], alone['loop'])


# -------------------------------------------------------------------------------------------------------------- the player
def errors(rows, want_rows):
    """(largest matrix entry difference, largest location difference) of device rows against fp64 rows."""
    rows = rows.double().cpu()
    assert rows.shape == want_rows.shape
    as4 = lambda r: r if r.ndim == 4 else r.unsqueeze(-2)                  # noqa: E731
    rot, want_rot = ops.carla_pose_import(as4(rows))[1], ops.carla_pose_import(as4(want_rows))[1]
    return float((rot - want_rot).abs().max()), float((rows[..., :3] - want_rows[..., :3]).abs().max())


def play(bones, root, loop, case, frames, **kw):
    out = ops.loop_carla_rows(bones, root, loop=loop, blend=CASES[case][4], frames=frames, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('case,max_blocks', RUNS)
def test_the_player_against_fp64_copies_and_pieces(case, max_blocks, monkeypatch):
    N, T, J, period, blend = CASES[case][:5]
    bones, root = (t.to(dev()) for t in problem(case))
    loop = search(bones, case, want=('loop',))['loop']
    P, frames = period, 3 * period + 5
    assert bool((loop[:, 1] - loop[:, 0] == P).all())
    got_b, got_r = play(bones, root, loop, case, frames, max_blocks=max_blocks)
    assert got_b.shape == (N, frames, J, 6) and got_r.shape == (N, frames, 6) and got_b.dtype == torch.float32 and got_b.is_cuda
    g = torch.arange(frames, device=dev())
    outside = g % P < P - blend
    at = loop[:, :1] + g % P                                               # (N, frames)
    src_b = torch.stack([bones[n, at[n]] for n in range(N)])
    src_r = torch.stack([root[n, at[n]] for n in range(N)])
    assert torch.equal(got_b[:, outside], src_b[:, outside]) and torch.equal(got_r[:, outside][..., 2:], src_r[:, outside][..., 2:])
    first = outside & (g < P)
    assert torch.equal(got_r[:, first], src_r[:, first])                   # cycle 0 outside the window
    if blend == 0:
        assert bool(outside.all()) and torch.equal(got_b, src_b)          # a pure gather
    else:
        assert not bool((got_b[:, ~outside] == src_b[:, ~outside]).all(-1).all(-1).any())
    want_b, want_r = ops.loop_carla_rows(bones.double().cpu(), root.double().cpu(), loop=loop.cpu(), blend=blend, frames=frames)
    fw_b, fw_r = framework(monkeypatch, play, bones, root, loop, case, frames)
    scale = float(want_r[..., :3].abs().max().clamp(min=float(want_b[..., :3].abs().max())))
    for what, got, fw, want in (('bones', got_b, fw_b, want_b), ('root', got_r, fw_r, want_r)):
        (fw_rot, fw_loc), (rot, loc) = errors(fw, want), errors(got, want)
        rot_tol, loc_tol = max(4 * fw_rot, MATRIX_FLOOR), max(4 * fw_loc, LOC_FLOOR * scale)
        print(f'{CASES[case]} cap {max_blocks} {what}: tensor restatement {fw_rot:.3e} / {fw_loc:.3e}, K41 {rot:.3e} / {loc:.3e} from '
              f'fp64 (matrix entries / locations; allowed {rot_tol:.3e} / {loc_tol:.3e})')
        assert math.isfinite(rot) and rot <= rot_tol, what
        assert math.isfinite(loc) and loc <= loc_tol, what
    # pieces, the other grid, without the root, strided inputs, a video without a loop
    pieces = [play(bones, root, loop, case, k, first_output=f0, max_blocks=max_blocks) for f0, k in ((0, 7), (7, P), (7 + P, frames - 7 - P))]
    assert torch.equal(torch.cat([p[0] for p in pieces], 1), got_b) and torch.equal(torch.cat([p[1] for p in pieces], 1), got_r)
    other_b, other_r = play(bones, root, loop, case, frames, max_blocks=0 if max_blocks else 2)
    assert torch.equal(other_b, got_b) and torch.equal(other_r, got_r)
    alone_b, none = play(bones, None, loop, case, frames, max_blocks=max_blocks)
    assert none is None and torch.equal(alone_b, got_b)
    wide_b, wide_r = torch.zeros(N, T, J, 8, device=dev()), torch.zeros(N, 2 * T, 6, device=dev())
    wide_b[..., 1:7], wide_r[:, ::2] = bones, root
    view_b, view_r = play(wide_b[..., 1:7], wide_r[:, ::2], loop, case, frames, max_blocks=max_blocks)
    assert torch.equal(view_b, got_b) and torch.equal(view_r, got_r)
    none = loop.clone()
    none[0] = -1
    nan_b, nan_r = play(bones, root, none, case, frames, max_blocks=max_blocks)
    assert bool(torch.isnan(nan_b[0]).all()) and bool(torch.isnan(nan_r[0]).all())
    assert torch.equal(nan_b[1:], got_b[1:]) and torch.equal(nan_r[1:], got_r[1:])


# ---------------------------------------------------------------------------------------------------------------- dispatch
def test_dispatch(monkeypatch):
    case = 0
    N, T, J, period, blend = CASES[case][:5]
    bones, root = (t.to(dev()) for t in problem(case))
    ref = reference(case)
    fw = framework(monkeypatch, search, bones, case)                      # the library is not asked for
    assert fw['cost'].dtype == torch.float32 and fw['cost'].is_cuda
    tol = max(4 * cost_error(fw['cost'], ref['cost']), floor_of(case))
    frames = 2 * period
    want_b, want_r = ops.loop_carla_rows(bones.double().cpu(), root.double().cpu(), loop=ref['loop'], blend=blend, frames=frames)
    with monkeypatch.context() as m:
        m.setattr(_lib, 'lib', no_library)
        d = search(bones.double(), case)
        h = ops.find_carla_loop(bones.cpu(), blend=blend, min_period=CASES[case][5], max_period=CASES[case][6], want=('loop', 'cost'))
        with torch.autocast('cuda', dtype=torch.bfloat16):
            ac = search(bones, case)
            ac_b, _ = play(bones, root, ref['loop'], case, frames)
        d_b, d_r = play(bones.double(), root.double(), ref['loop'], case, frames)
        h_b, h_r = ops.loop_carla_rows(bones.cpu(), root.cpu(), loop=ref['loop'], blend=blend, frames=frames)
    assert d['cost'].dtype == torch.float64 and d['cost'].is_cuda and d['loop_cost'].dtype == torch.float64
    assert h['cost'].dtype == torch.float32 and not h['cost'].is_cuda and not h['loop'].is_cuda
    assert ac['cost'].dtype == torch.float32 and ac['cost'].is_cuda
    for what, out in (('fp64 on the device', d), ('the host', h), ('autocast', ac), ('the kernel', search(bones, case))):
        err = cost_error(out['cost'], ref['cost'])
        print(f'{what}: {err:.3e} from fp64 (allowed {tol:.3e})')
        assert err <= tol and bool((out['loop'][:, 1] - out['loop'][:, 0] == period).all())
    assert torch.equal(d['loop'].cpu(), ref['loop'])
    assert d_b.dtype == torch.float64 and d_b.is_cuda and d_r.dtype == torch.float64
    assert h_b.dtype == torch.float32 and not h_b.is_cuda and not h_r.is_cuda and ac_b.dtype == torch.float32 and ac_b.is_cuda
    fw_b, fw_r = framework(monkeypatch, play, bones, root, ref['loop'], case, frames)
    rot_tol = max(4 * errors(fw_b, want_b)[0], MATRIX_FLOOR)
    for out in (d_b, h_b, ac_b, fw_b, play(bones, root, ref['loop'], case, frames)[0]):
        assert errors(out, want_b)[0] <= rot_tol
    assert errors(d_r, want_r)[0] <= rot_tol and errors(h_r, want_r)[0] <= rot_tol


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_find_abi_refusals_come_before_any_launch():
    lib = _lib.lib()
    N, T, J, blend = 2, 12, 3, 2
    bones = torch.zeros(N, T, J, 6, device=dev())
    weights = torch.ones(J, device=dev())
    loop, loop_cost = torch.zeros(N, 2, dtype=torch.int64, device=dev()), torch.zeros(N, device=dev())
    cost, ws = torch.zeros(N, T, T, device=dev()), torch.zeros(N, dtype=torch.int64, device=dev())
    assert lib.p2c_carla_loop_find_workspace(N, T, J, blend) == 8 * N and lib.p2c_carla_loop_find_workspace(0, T, J, blend) == 0
    for args in ((-1, T, J, blend), (N, 1, J, blend), (N, 16385, J, blend), (N, T, 0, blend), (N, T, 65, blend), (N, T, J, -1),
                 (N, T, J, 33), (2 ** 20, 2 ** 10, 26, 2)):
        assert lib.p2c_carla_loop_find_workspace(*args) == -1, args
    base = dict(bones=bones.data_ptr(), weights=weights.data_ptr(), out_loop=loop.data_ptr(), out_loop_cost=loop_cost.data_ptr(),
                out_cost=cost.data_ptr(), N=N, T=T, J=J, blend=blend, min_period=3, max_period=8, max_blocks=0, workspace=ws.data_ptr())

    def call(**changes):
        a = {**base, **changes}
        return lib.p2c_carla_loop_find_fwd(*a.values(), None)

    for changes in (dict(N=-1), dict(T=-1), dict(T=0), dict(T=1), dict(T=16385), dict(J=0), dict(J=65), dict(blend=-1), dict(blend=33),
                    dict(min_period=0), dict(min_period=-1), dict(max_period=2), dict(max_blocks=-1), dict(N=2 ** 20, T=2 ** 10, J=26),
                    dict(N=2 ** 31)):
        assert call(**changes) == -2, changes
    assert call(N=-1, bones=None) == -2 and call(blend=33, workspace=None) == -2           # shapes are looked at first
    for changes in (dict(bones=None), dict(out_loop=None), dict(out_loop_cost=None), dict(workspace=None)):
        assert call(**changes) == -1, changes
    assert call(N=0) == 0 and call(N=0, workspace=None) == 0
    torch.cuda.synchronize()
    for t in (loop, loop_cost, cost, ws):
        assert float(t.abs().sum()) == 0.0                                 # nothing ran
    # a video that stands still: every admissible pair costs 0, the first one wins; without weights and without the matrix
    assert call() == 0
    torch.cuda.synchronize()
    assert loop.tolist() == [[2, 5]] * N and loop_cost.tolist() == [0.0] * N
    admissible = lp.admissible(T, blend, 3, 8, dev())
    assert bool((cost[:, admissible] == 0).all()) and bool(torch.isinf(cost[:, ~admissible]).all())
    loop.zero_(), loop_cost.fill_(7.0)
    assert call(weights=None, out_cost=None, max_period=2 ** 40) == 0
    torch.cuda.synchronize()
    assert loop.tolist() == [[2, 5]] * N and loop_cost.tolist() == [0.0] * N


def test_play_abi_refusals_come_before_any_launch():
    lib = _lib.lib()
    N, T, J, K, blend = 2, 12, 3, 9, 2
    bones, root = torch.zeros(N, T, J, 6, device=dev()), torch.zeros(N, T, 6, device=dev())
    out_b, out_r = torch.zeros(N, K, J, 6, device=dev()), torch.zeros(N, K, 6, device=dev())
    loop = torch.tensor([[2, 6], [3, 11]], device=dev())
    base = dict(bones=bones.data_ptr(), root=root.data_ptr(), loop=loop.data_ptr(), out_bones=out_b.data_ptr(),
                out_root=out_r.data_ptr(), N=N, T=T, J=J, frames=K, first_output=0, blend=blend, max_blocks=0)

    def call(**changes):
        a = {**base, **changes}
        return lib.p2c_carla_loop_play_fwd(*a.values(), None)

    for changes in (dict(N=-1), dict(T=-1), dict(frames=-1), dict(first_output=-1), dict(max_blocks=-1), dict(J=0), dict(J=65),
                    dict(blend=-1), dict(blend=33), dict(T=16385), dict(T=1), dict(T=0), dict(N=2 ** 20, frames=2 ** 10),
                    dict(N=2 ** 20, T=2 ** 10, frames=0), dict(first_output=2 ** 41), dict(N=2 ** 31)):
        assert call(**changes) == -2, changes
    assert call(N=-1, bones=None) == -2 and call(blend=33, loop=None) == -2                # shapes are looked at first
    for changes in (dict(bones=None), dict(loop=None), dict(out_bones=None), dict(out_root=None), dict(root=None)):
        assert call(**changes) == -1, changes
    assert call(N=0) == 0 and call(frames=0) == 0 and call(frames=0, T=0) == 0
    torch.cuda.synchronize()
    assert float(out_b.abs().sum()) == 0.0 and float(out_r.abs().sum()) == 0.0   # nothing ran
    # the frame index as x: which source frame an output came from; the root moves by e - s = 4 a cycle in video 0
    frame = torch.arange(T, device=dev(), dtype=torch.float32)
    bones[..., 0], root[..., 0] = frame[None, :, None], frame[None, :]
    assert call() == 0
    torch.cuda.synchronize()
    # P = 4, blend = 2: outputs 0, 1 copy frames 2, 3; outputs 2, 3 blend frames 4, 5 towards frames 0, 1 at u = 1/3, 2/3
    want = torch.tensor([2.0, 3.0, 4 - 4 / 3, 5 - 8 / 3, 2.0, 3.0, 4 - 4 / 3, 5 - 8 / 3, 2.0], device=dev())
    assert float((out_b[0, :, 0, 0] - want).abs().max()) <= 1e-6 and float(out_b[0, 0, 0, 0]) == 2.0
    moved = want + 4.0 * (torch.arange(K, device=dev()) // 4) + torch.tensor([0, 0, 4 / 3, 8 / 3] * 2 + [0], device=dev())
    assert float((out_r[0, :, 0] - moved).abs().max()) <= 1e-6             # inside the window the root keeps walking
    assert float(out_b[..., 3:].abs().max()) <= 1e-4 and float(out_b[1, 8, 0, 0]) == 3.0 and float(out_r[1, 8, 0]) == 11.0
    # a loop that cannot be followed is never followed: NaN rows, no fault
    loop[0] = torch.tensor([1, 6], device=dev())                           # s < blend
    loop[1] = torch.tensor([3, 12], device=dev())                          # e > T - 1
    assert call(root=None, out_root=None) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(out_b).all())


# ------------------------------------------------------------------------------------------------------------- end to end
def test_predict_carla_with_a_looper():
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    from pedestrians_video_2_carla_amd.walker_control.root_motion import CarlaRootMotion
    seed_everything(11)
    B, T = 2, 8
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B)
    flow = LitPoseLiftingFlow(movements_model=LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON),
                              loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    trainer = Trainer(max_steps=1, device=dev()).setup(flow, dm)
    batches = [dm.generate_batch(dev()), dm.generate_batch(dev())]
    kw = dict(blend=2, min_period=3, frames=20)
    plain = trainer.predict_carla(flow, batches)
    same_rows = trainer.predict_carla(flow, batches, loop=None)
    looped = trainer.predict_carla(flow, batches, root_motion=True, loop=kw)
    again = trainer.predict_carla(flow, batches, root_motion=CarlaRootMotion(), loop=CarlaLooper(**kw))
    torch.cuda.synchronize()
    for (b, r, meta), (nb, nr, _), (lb, lr, lmeta), (ab, ar, _) in zip(plain, same_rows, looped, again):
        assert torch.equal(nb, b) and torch.equal(nr, r)
        mb, mr = CarlaRootMotion().apply(b, r)
        looper = CarlaLooper(blend=2, min_period=3)
        found = looper.find(mb)['loop']
        wb, wr = looper.play(mb, mr, 20, found)
        assert lb.is_cuda and lb.shape == (B, 20, 26, 6) and lr.shape == (B, 20, 6) and lmeta is meta
        assert bool((found[:, 0] >= 2).all()) and bool(torch.isfinite(lb).all()) and bool(torch.isfinite(lr).all())
        assert torch.equal(lb, wb) and torch.equal(lr, wr) and torch.equal(ab, wb) and torch.equal(ar, wr)
