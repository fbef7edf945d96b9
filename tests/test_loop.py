"""K41 on the host: the definition of the loop search and the looping player (walker_control/loop.py), in fp64 and fp32."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.walker_control import loop as lp
from pedestrians_video_2_carla_amd.walker_control.loop import CarlaLooper
from test_smooth import geodesic, matrices, random_rotations, rodrigues, rows_of, unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
REFUSED = (ValueError,)
# (N, T, J, period, blend, min_period, max_period); max_period < 2 period on purpose: twice the period is as good a loop
CASES = [(2, 40, 26, 12, 3, 6, 20), (1, 33, 5, 10, 0, 4, 16), (2, 70, 26, 16, 8, 8, 30), (1, 40, 1, 12, 3, 6, 20)]


# ------------------------------------------------------------------------------------------------------------------ inputs
def gait_paths(N, T, J, period, seed=0, jitter_deg=0.5):
    """fp64 rows ``(bones (N,T,J,6), root (N,T,6))`` with a planted period: per bone a random base orientation times a rotation
    about a fixed random axis by ``amp sin(2 pi t / period + phase)``, ``amp`` 0.3 to 1.0 of 25 degrees, ``jitter_deg`` (s.d.) of
    jitter about random axes on top; constant bone locations; a root of constant orientation that drifts (0.05, 0.01, 0) a frame."""
    g = torch.Generator().manual_seed(4100 + 1000 * N + 10 * T + J + 97 * period + seed)
    base = random_rotations(g, N, 1, J)
    axis = unit(torch.randn(N, 1, J, 3, generator=g, dtype=F64)).expand(N, T, J, 3)
    amp = math.radians(25.0) * (0.3 + 0.7 * torch.rand(N, 1, J, generator=g, dtype=F64))
    phase = 2 * math.pi * torch.rand(N, 1, J, generator=g, dtype=F64)
    t = torch.arange(T, dtype=F64).reshape(1, T, 1)
    rot = base @ rodrigues(axis, amp * torch.sin(2 * math.pi * t / period + phase))
    if jitter_deg:
        rot = rot @ rodrigues(unit(torch.randn(N, T, J, 3, generator=g, dtype=F64)),
                              torch.randn(N, T, J, generator=g, dtype=F64) * math.radians(jitter_deg))
    loc = torch.randn(N, 1, J, 3, generator=g, dtype=F64).expand(N, T, J, 3)
    root_loc = torch.randn(N, 1, 3, generator=g, dtype=F64) + t * torch.tensor([0.05, 0.01, 0.0], dtype=F64)
    root_rot = random_rotations(g, N, 1).expand(N, T, 3, 3)
    return rows_of(loc, rot), rows_of(root_loc, root_rot)


def find(bones, blend, min_period, max_period=None, **kw):
    return ops.find_carla_loop(bones, blend=blend, min_period=min_period, max_period=max_period, want=('loop', 'cost'), **kw)


def other_period_ratio(cost, loop, period):
    """The cheapest finite entry at another period over the best entry, per video, the smallest of them."""
    T = cost.shape[-1]
    diff = torch.arange(T).unsqueeze(0) - torch.arange(T).unsqueeze(1)
    ratios = []
    for n in range(cost.shape[0]):
        others = cost[n][(diff != period) & torch.isfinite(cost[n])]
        ratios.append(float(others.min() / cost[n, loop[n, 0], loop[n, 1]]))
    return min(ratios)


def step_angles(rows_a, rows_b):
    return geodesic(matrices(rows_a.double()), matrices(rows_b.double()))


# -------------------------------------------------------------------------------------------------------------- the search
@pytest.mark.parametrize('dtype', [torch.float32, F64])
@pytest.mark.parametrize('N,T,J,period,blend,min_period,max_period', CASES)
def test_the_search_is_the_definition_spelled_out(N, T, J, period, blend, min_period, max_period, dtype):
    """Every entry against loops over (s, e, k, j) in fp64, the +inf pattern, and the choice as the first minimal entry."""
    bones = gait_paths(N, T, J, period)[0].to(dtype)
    got = find(bones, blend, min_period, max_period)
    cost, loop, loop_cost = got['cost'], got['loop'], got['loop_cost']
    assert cost.shape == (N, T, T) and cost.dtype == dtype and loop.dtype == torch.int64 and loop_cost.dtype == dtype
    q = lp._row_quat(bones.double())
    want = torch.full((N, T, T), float('inf'), dtype=F64)
    for s in range(blend, T):
        for e in range(s + min_period, min(s + max_period, T - 1) + 1):
            ks = torch.arange(-blend, 1)
            dots = (q[:, s + ks] * q[:, e + ks]).sum(-1)                     # (N, blend + 1, J)
            want[:, s, e] = (1 - dots * dots).sum((-1, -2))
    assert torch.equal(torch.isinf(cost), torch.isinf(want))
    finite = torch.isfinite(want)
    tol = 1e-12 if dtype == F64 else J * (blend + 1) * 2.0 ** -19
    assert float((cost.double()[finite] - want[finite]).abs().max()) <= tol
    for n in range(N):
        best = cost[n][torch.isfinite(cost[n])].min()
        first = (cost[n] == best).nonzero()[0]
        assert loop[n].tolist() == first.tolist() and loop_cost[n] == best
        assert int(loop[n, 1] - loop[n, 0]) == period
    assert other_period_ratio(want, loop, period) >= 10.0
    # what is returned for a key does not depend on what else is asked for
    alone = ops.find_carla_loop(bones, blend=blend, min_period=min_period, max_period=max_period)
    assert set(alone) == {'loop', 'loop_cost'} and torch.equal(alone['loop'], loop) and torch.equal(alone['loop_cost'], loop_cost)


@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_a_path_without_jitter_closes_at_its_period_and_ties_go_to_the_first_pair(dtype):
    N, T, J, period, blend = 2, 40, 5, 12, 3
    bones = gait_paths(N, T, J, period, jitter_deg=0.0)[0].to(dtype)
    got = find(bones, blend, 6, 20)
    diagonal = torch.stack([got['cost'][:, s, s + period] for s in range(blend, T - period)], 1)
    print(f'{dtype}: the largest C(s, s + period) without jitter is {float(diagonal.max()):.3e}')
    assert float(diagonal.abs().max()) <= (1e-12 if dtype == F64 else J * (blend + 1) * 2.0 ** -21)
    assert bool((got['loop'][:, 1] - got['loop'][:, 0] == period).all())
    # costs that are equal to the bit: a video that stands still. Every admissible pair costs the same, and the first one in
    # row-major order is (blend, blend + min_period). (On the periodic path the costs of the pairs one period apart are rounding
    # noise around zero, not equal: which of them is smallest is not a property of the definition.)
    still = bones[:, :1].expand(N, T, J, 6)
    tied = find(still, blend, 6, 20)
    for n in range(N):
        assert bool((tied['cost'][n][torch.isfinite(tied['cost'][n])] == tied['cost'][n, blend, blend + 6]).all())
    assert tied['loop'].tolist() == [[blend, blend + 6]] * N and torch.equal(tied['loop_cost'], tied['cost'][:, blend, blend + 6])


def test_weights_of_zero_for_all_bones_but_one_are_that_bone_alone():
    N, T, J, period, blend = 2, 40, 5, 12, 3
    bones = gait_paths(N, T, J, period)[0]
    for dtype in (torch.float32, F64):
        b = bones.to(dtype)
        for j in (0, 3):
            w = torch.zeros(J)
            w[j] = 1.0
            weighted, alone = find(b, blend, 6, 20, weights=w), find(b[:, :, j:j + 1], blend, 6, 20)
            assert all(torch.equal(weighted[k], alone[k]) for k in ('cost', 'loop', 'loop_cost'))
        doubled, plain = find(b, blend, 6, 20, weights=[2.0] * J), find(b, blend, 6, 20)
        assert torch.equal(doubled['cost'], 2 * plain['cost']) and torch.equal(doubled['loop'], plain['loop'])


def test_non_finite_costs_are_never_chosen():
    N, T, J, period, blend = 3, 40, 5, 12, 3
    bones = gait_paths(N, T, J, period)[0].clone()
    clean = find(bones, blend, 6, 20)
    bones[1] = float('nan')
    s, e = clean['loop'][2].tolist()
    bones[2, s, 1] = float('nan')                                          # the best pair of video 2 reads this row
    got = find(bones, blend, 6, 20)
    assert got['loop'][1].tolist() == [-1, -1] and math.isnan(float(got['loop_cost'][1]))
    assert torch.equal(got['loop'][0], clean['loop'][0]) and torch.equal(got['cost'][0], clean['cost'][0])
    s_idx, e_idx = torch.arange(T).unsqueeze(1), torch.arange(T).unsqueeze(0)
    reads = torch.zeros(T, T, dtype=torch.bool)
    for k in range(-blend, 1):
        reads |= (s_idx + k == s) | (e_idx + k == s)
    poisoned = reads & torch.isfinite(clean['cost'][2])
    assert torch.equal(torch.isnan(got['cost'][2]), poisoned) and bool(poisoned[s, e])
    assert torch.equal(got['cost'][2][~poisoned], clean['cost'][2][~poisoned])
    ns, ne = got['loop'][2].tolist()
    assert [ns, ne] != [s, e] and not bool(poisoned[ns, ne]) and float(got['loop_cost'][2]) == float(got['cost'][2, ns, ne])
    # a video too short for any admissible pair
    short = find(bones[:1, :9], blend, 6, 20)
    assert short['loop'].tolist() == [[-1, -1]] and bool(torch.isinf(short['cost']).all())
    assert find(bones[:1, :10], blend, 6, 20)['loop'].tolist() == [[3, 9]]
    empty = find(bones[:0], blend, 6, 20)
    assert empty['loop'].shape == (0, 2) and empty['cost'].shape == (0, T, T)


# -------------------------------------------------------------------------------------------------------------- the player
def played(dtype, case=CASES[0], **kw):
    N, T, J, period, blend, min_period, max_period = case
    bones, root = (t.to(dtype) for t in gait_paths(N, T, J, period))
    looper = CarlaLooper(blend, min_period, max_period)
    loop = looper.find(bones)['loop']
    return bones, root, looper, loop, period


@pytest.mark.parametrize('dtype', [torch.float32, F64])
@pytest.mark.parametrize('case', [CASES[0], CASES[1]], ids=['blend-3', 'blend-0'])
def test_copies_are_copies_and_pieces_equal_the_whole(case, dtype):
    bones, root, looper, loop, P = played(dtype, case)
    blend, frames = looper.blend, 3 * P + 5
    out_b, out_r = looper.play(bones, root, frames, loop)
    assert out_b.shape == (bones.shape[0], frames, bones.shape[2], 6) and out_r.shape == (bones.shape[0], frames, 6)
    assert out_b.dtype == dtype and bool(torch.isfinite(out_b).all()) and bool(torch.isfinite(out_r).all())
    for n, (s, e) in enumerate(loop.tolist()):
        assert e - s == P
        for g in range(frames):
            c, phi = divmod(g, P)
            if phi < P - blend:
                assert torch.equal(out_b[n, g], bones[n, s + phi]) and torch.equal(out_r[n, g, 2:], root[n, s + phi, 2:])
                if c == 0:
                    assert torch.equal(out_r[n, g], root[n, s + phi])
            else:
                assert not torch.equal(out_b[n, g], bones[n, s + phi])
    pieces = [looper.play(bones, root, k, loop, first_output=first) for first, k in ((0, 7), (7, P), (7 + P, frames - 7 - P))]
    assert torch.equal(torch.cat([p[0] for p in pieces], 1), out_b) and torch.equal(torch.cat([p[1] for p in pieces], 1), out_r)
    alone_b, none = looper.play(bones, None, frames, loop)
    assert none is None and torch.equal(alone_b, out_b)
    both_b, both_r = looper.loop(bones, root, frames)
    assert torch.equal(both_b, out_b) and torch.equal(both_r, out_r)
    if blend == 0:                                                         # a pure gather
        at = torch.stack([s + torch.arange(frames) % P for s, _ in loop.tolist()])
        assert torch.equal(out_b, torch.stack([bones[n, at[n]] for n in range(len(at))]))


@pytest.mark.parametrize('dtype', [torch.float32, F64])
def test_the_root_advances_by_exactly_delta_a_cycle(dtype):
    bones, root, looper, loop, P = played(dtype)
    frames = 4 * P + 3
    _, out_r = looper.play(bones, root, frames, loop)
    eps = torch.finfo(dtype).eps
    for n, (s, e) in enumerate(loop.tolist()):
        delta = root[n, e, :2].double() - root[n, s, :2].double()
        step = out_r[n, P:, :2].double() - out_r[n, :-P, :2].double()
        # each of the two outputs is m + c delta, formed in fp64 and rounded once: half a unit in the last place each
        # (fp64 rows: the products and sums before it round as well)
        bound = eps * float(out_r[n, :, :2].abs().max()) * (1.001 if dtype == torch.float32 else 4.0)
        print(f'{dtype} video {n}: delta {delta.tolist()}, largest departure {float((step - delta).abs().max()):.3e} (allowed {bound:.3e})')
        assert float((step - delta).abs().max()) <= bound
        assert torch.equal(out_r[n, P:, 2:], out_r[n, :-P, 2:])            # z and the angles repeat
    if dtype == torch.float32:
        # before the rounding: the same rows in fp64 advance by delta up to fp64's own rounding
        _, out64 = looper.play(bones.double(), root.double(), frames, loop)
        for n, (s, e) in enumerate(loop.tolist()):
            delta = root[n, e, :2].double() - root[n, s, :2].double()
            step = out64[n, P:, :2] - out64[n, :-P, :2]
            assert float((step - delta).abs().max()) <= 4 * 2.0 ** -52 * float(out64[n, :, :2].abs().max())
            # and outside the blend window, where no u is used, the fp32 rows are those values rounded once
            outside = torch.arange(frames) % P < P - looper.blend
            assert torch.equal(out64[n, outside, :2].float(), out_r[n, outside, :2])


@pytest.mark.parametrize('dtype', [torch.float32, F64])
@pytest.mark.parametrize('case', [CASES[0], CASES[1], CASES[2]], ids=['blend-3', 'blend-0', 'blend-8'])
def test_the_seam_is_no_rougher_than_the_cycle_plus_its_share_of_the_mismatch(case, dtype):
    """out[P - 1] is the slerp of src[e - 1] (or src[e - 1] itself at blend 0) towards src[s - 1] at u = blend / (blend + 1): it is
    ``mismatch / (blend + 1)`` from src[s - 1] (from src[e] at blend 0: then out[P - 1] = src[e - 1] is one source step from src[e],
    which is ``mismatch`` from src[s]), and out[P] = src[s] is one source step further. So per bone
    ``angle(out[P - 1], out[P]) <= largest step among frames s - blend .. e + largest mismatch over the window / (blend + 1)``,
    plus what the lerp arm (below half a degree) and the rows' rounding add: 1e-6 rad in fp64, 1e-4 rad in fp32."""
    bones, root, looper, loop, P = played(dtype, case)
    blend = looper.blend
    out_b, _ = looper.play(bones, None, P + 1, loop)
    slack = 1e-6 if dtype == F64 else 1e-4
    for n, (s, e) in enumerate(loop.tolist()):
        seam = step_angles(out_b[n, P - 1], out_b[n, P])
        steps = step_angles(bones[n, s - blend:e], bones[n, s - blend + 1:e + 1]).max(0).values
        mismatch = step_angles(bones[n, s - blend:s + 1], bones[n, e - blend:e + 1]).max(0).values
        bound = steps + mismatch / (blend + 1) + slack
        raw = step_angles(bones[n, e - 1], bones[n, s])                   # the seam of a replay without the blend
        print(f'{dtype} blend {blend} video {n}: seam {float(seam.max()):.4f} rad, bound {float(bound.max()):.4f}, unblended '
              f'{float(raw.max()):.4f}')
        assert bool((seam <= bound).all())


def test_a_video_without_a_loop_plays_nan_and_touches_nothing_else():
    bones, root, looper, loop, P = played(F64)
    frames = 2 * P
    want_b, want_r = looper.play(bones, root, frames, loop)
    none = loop.clone()
    none[0] = -1
    out_b, out_r = looper.play(bones, root, frames, none)
    assert bool(torch.isnan(out_b[0]).all()) and bool(torch.isnan(out_r[0]).all())
    assert torch.equal(out_b[1], want_b[1]) and torch.equal(out_r[1], want_r[1])
    assert looper.play(bones, root, 0, loop)[0].shape == (2, 0, 26, 6)
    assert not looper.play(bones.clone().requires_grad_(), root, 3, loop)[0].requires_grad
    wide = torch.zeros(2, 40, 26, 8, dtype=F64)
    wide[..., 1:7] = bones
    assert torch.equal(looper.play(wide[..., 1:7], root, frames, loop)[0], want_b)
    assert torch.equal(looper.play(bones, root, frames, loop.tolist())[0], want_b)     # a list of pairs


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    bones, root = gait_paths(2, 20, 3, 6)
    for kw in (dict(blend=-1, min_period=3), dict(blend=33, min_period=3), dict(blend=1.5, min_period=3), dict(blend=2, min_period=0),
               dict(blend=2, min_period=-4), dict(blend=2, min_period=5, max_period=4), dict(blend=2, min_period=3, max_period=2.5)):
        with pytest.raises(REFUSED):
            ops.find_carla_loop(bones, **kw)
        with pytest.raises(REFUSED):
            CarlaLooper(**kw)
    for kw in (dict(weights=torch.ones(4)), dict(weights=[1.0, -1.0, 1.0]), dict(weights=[1.0, float('nan'), 1.0]),
               dict(weights=[1.0, float('inf'), 1.0]), dict(want=('loop', 'period'))):
        with pytest.raises(REFUSED):
            ops.find_carla_loop(bones, blend=2, min_period=3, **kw)
    for b in (bones[..., :5], bones[0]):
        with pytest.raises(REFUSED):
            ops.find_carla_loop(b, blend=2, min_period=3)
    assert ops.find_carla_loop(bones, blend=32, min_period=1, max_period=10 ** 12)['loop'].tolist() == [[-1, -1]] * 2
    good = torch.tensor([[2, 9], [-1, -1]])
    play = lambda **kw: ops.loop_carla_rows(bones, root, **{**dict(loop=good, blend=2, frames=5), **kw})     # noqa: E731
    assert play()[0].shape == (2, 5, 3, 6)
    for kw in (dict(blend=-1), dict(blend=33), dict(frames=-1), dict(frames=2.5), dict(first_output=-1),
               dict(loop=torch.tensor([[1, 9], [-1, -1]])),                 # s < blend
               dict(loop=torch.tensor([[2, 20], [-1, -1]])),                # e > T - 1
               dict(loop=torch.tensor([[9, 9], [-1, -1]])), dict(loop=torch.tensor([[9, 2], [-1, -1]])),
               dict(loop=torch.tensor([[-1, 5], [-1, -1]])), dict(loop=torch.tensor([[2, 9]])),
               dict(loop=torch.tensor([[2.0, 9.0], [-1.0, -1.0]]))):
        with pytest.raises(REFUSED):
            play(**kw)
    for b, r in ((bones, root[:1]), (bones, root[:, :3]), (bones, root.float())):
        with pytest.raises(REFUSED):
            ops.loop_carla_rows(b, r, loop=good, blend=2, frames=5)
    with pytest.raises(REFUSED):
        CarlaLooper(2, 3).loop(bones, root)                                # no frames, here or there
    with pytest.raises(REFUSED):
        lp.as_looper(dict(blend=2, min_period=3))
    with pytest.raises(REFUSED):
        lp.as_looper(dict(blend=2, min_period=3, frames=5, sigma=1.0))     # not an argument
    with pytest.raises(REFUSED):
        lp.as_looper(True)


# ---------------------------------------------------------------------------------------------------- files and the writers
def test_the_file_rewriter_round_trips(tmp_path):
    from pedestrians_video_2_carla_amd.data.carla import animation
    N, T, J, period, blend, min_period, max_period = CASES[0]
    bones, root = (t.float() for t in gait_paths(N, T, J, period))
    src = animation._write(str(tmp_path / 'src'), [(bones.numpy(), root.numpy(), {'age': ['adult', 'child'], 'gender': ['male', 'female']})], 25.0)
    before = animation.load_carla_animation(src)
    assert 'loop_start' not in before and set(before) == {'bones', 'root', 'bone_names', 'age', 'gender', 'fps'}
    looper = CarlaLooper(blend, min_period, max_period)
    found = looper.find(bones, want=('loop', 'loop_cost'))
    want_b, want_r = looper.play(bones, root, 50, found['loop'])
    got = animation.load_carla_animation(animation.loop_carla_animation(src, str(tmp_path / 'dst'), frames=50, blend=blend,
                                                                        min_period=min_period, max_period=max_period))
    assert np.array_equal(got['bones'], want_b.numpy()) and np.array_equal(got['root'], want_r.numpy())
    assert got['bones'].shape == (N, 50, J, 6) and got['bones'].dtype == np.float32
    assert got['loop_start'].dtype == np.int64 and np.array_equal(got['loop_start'], found['loop'][:, 0].numpy())
    assert np.array_equal(got['loop_end'], found['loop'][:, 1].numpy()) and np.array_equal(got['loop_cost'], found['loop_cost'].numpy())
    assert got['fps'] == 25.0 and all(got[k] == before[k] for k in ('age', 'gender', 'bone_names'))
    with pytest.raises(REFUSED):
        animation.loop_carla_animation(src, str(tmp_path / 'bad'), frames=-1, blend=blend, min_period=min_period)


def test_the_writers_take_a_loop_after_the_root_motion_and_before_the_resampling(tmp_path):
    from pedestrians_video_2_carla_amd.data.carla import animation
    from pedestrians_video_2_carla_amd.trainer import Trainer
    from pedestrians_video_2_carla_amd.walker_control.resample import CarlaResampler
    from pedestrians_video_2_carla_amd.walker_control.root_motion import CarlaRootMotion
    from test_resample import animation_batches, linear_flow
    flow, batches = linear_flow(), animation_batches()
    outputs = Trainer().predict(flow, batches)
    kw = dict(blend=2, min_period=3, frames=20)
    plain = animation.save_carla_animation(str(tmp_path / 'a'), outputs, fps=30.0)
    explicit = animation.save_carla_animation(str(tmp_path / 'b'), outputs, fps=30.0, loop=None)
    assert open(plain, 'rb').read() == open(explicit, 'rb').read()         # None: the bytes of the call without it
    lifted = animation.lift_carla_animation(str(tmp_path / 'c'), flow, batches, fps=30.0)
    lifted_none = animation.lift_carla_animation(str(tmp_path / 'd'), flow, batches, fps=30.0, loop=None)
    assert open(lifted, 'rb').read() == open(lifted_none, 'rb').read()
    src = animation.load_carla_animation(plain)
    src_b, src_r = torch.from_numpy(src['bones']), torch.from_numpy(src['root'])
    moved_b, moved_r = CarlaRootMotion().apply(src_b, src_r)
    want_b, want_r = CarlaLooper(**kw).loop(moved_b, moved_r)
    assert want_b.shape[1] == 20 and bool(torch.isfinite(want_b).all())
    rate_b, rate_r = CarlaResampler(30.0, 20.0).resample(want_b, want_r)
    for looper in (kw, CarlaLooper(**kw)):
        for path in (animation.save_carla_animation(str(tmp_path / 'e'), outputs, fps=30.0, root_motion=True, loop=looper),
                     animation.lift_carla_animation(str(tmp_path / 'f'), flow, batches, fps=30.0, root_motion=True, loop=looper)):
            got = animation.load_carla_animation(path)
            assert np.array_equal(got['bones'], want_b.numpy()) and np.array_equal(got['root'], want_r.numpy())
        got = animation.load_carla_animation(animation.save_carla_animation(str(tmp_path / 'g'), outputs, fps=30.0, out_fps=20.0,
                                                                            root_motion=True, loop=looper))
        assert got['fps'] == 20.0 and np.array_equal(got['bones'], rate_b.numpy()) and np.array_equal(got['root'], rate_r.numpy())
    rows = Trainer().predict_carla(flow, batches)
    same = Trainer().predict_carla(flow, batches, loop=None)
    looped = Trainer().predict_carla(flow, batches, root_motion=True, loop=kw)
    for (b, r, meta), (nb, nr, _), (lb, lr, lmeta) in zip(rows, same, looped):
        assert torch.equal(nb, b) and torch.equal(nr, r)
        wb, wr = CarlaLooper(**kw).loop(*CarlaRootMotion().apply(b, r))
        assert torch.equal(lb, wb) and torch.equal(lr, wr) and lmeta is meta and lb.shape[1] == 20
    with pytest.raises(REFUSED):
        animation.save_carla_animation(str(tmp_path / 'z'), outputs, loop=dict(blend=2, min_period=3))     # no frames


# --------------------------------------------------------------------------------------------------------------------- ABI
def test_k41_symbols_are_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    ctype = {'const float *': ctypes.c_void_p, 'float *': ctypes.c_void_p, 'void *': ctypes.c_void_p, 'int64_t *': ctypes.c_void_p,
             'const int64_t *': ctypes.c_void_p, 'int64_t ': ctypes.c_int64, 'int32_t ': ctypes.c_int32}
    names = {'p2c_carla_loop_find_workspace': ['N', 'T', 'J', 'blend'],
             'p2c_carla_loop_find_fwd': ['bones', 'weights', 'out_loop', 'out_loop_cost', 'out_cost', 'N', 'T', 'J', 'blend', 'min_period',
                                         'max_period', 'max_blocks', 'workspace', 'stream'],
             'p2c_carla_loop_play_fwd': ['bones', 'root', 'loop', 'out_bones', 'out_root', 'N', 'T', 'J', 'frames', 'first_output',
                                         'blend', 'max_blocks', 'stream']}
    for name, want in names.items():
        assert name in declared and name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None
        res, args = _lib.SYMBOLS[name]
        launches = name.endswith('_fwd')
        assert res is (ctypes.c_int if launches else ctypes.c_int64)
        assert (name in _lib._PoisonedLib(_lib.lib())._wrap) == launches
        decl = re.search(rf'P2C_API \w+ {name}\((.*?)\);', header, re.S).group(1)
        params = [' '.join(p.split()) for p in decl.split(',')]
        assert [ctype[re.match(r'(.*?)(\w+)$', p).group(1)] for p in params] == list(args)
        assert [re.match(r'(.*?)(\w+)$', p).group(2) for p in params] == want
    for macro, value in (('P2C_LOOP_MAX_BLEND', lp.MAX_BLEND), ('P2C_LOOP_MAX_J', lp.MAX_J), ('P2C_LOOP_MAX_T', lp.MAX_T)):
        assert int(re.search(rf'#define {macro} (\d+)', header).group(1)) == value == getattr(_lib, macro)
    # the kernel file shares the row arithmetic (not a copy of it), and the only atomic is the integer minimum
    source = open(os.path.join(ROOT, 'pedestrians_video_2_carla_amd', 'csrc', 'p2c_loop.hip')).read()
    assert '#include "p2c_carla_dev.h"' in source and 'row_quat(' in source and 'carla_row(' in source and 'sincosf(' not in source
    assert 'p2c_host::grid_for(' in source and 'asm' not in source.replace('__launch_bounds__', '')
    assert re.findall(r'\batomic\w+\(', source) == ['atomicMin('] and 'fminf' not in source and 'fmaxf' not in source
