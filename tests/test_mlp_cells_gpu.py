"""GPU: the fused MLP (K8: csrc/p2c_mlp.hip, csrc/p2c_mlp_dev.h, ops.fused_mlp) in every dispatch cell, on inputs where every
result is an exact integer.

K8 chooses between static (LinearAE156/78/52) and generic (DynShape) kernels, a cooperative and a wave-per-tile forward (with an
LDS guard that falls back to the cooperative one), recomputed and saved activations, a fused and a split weight gradient, vector
and scalar tile loads, one staging round or several for the weight image (`stage_rest`, images above 96 KB), and one or many
sample tiles per workgroup. Which of them runs is decided by the row count against P2C_MLP_MAX_BLOCKS and by environment
overrides that are read once per process, so the cases run in child processes (this file as a script, one child per
configuration) with P2C_MLP_MAX_BLOCKS=2: ten sample tiles are then five per workgroup, and 150 rows reach every regime that the
default 256 workgroups reach only at 131 072 rows.

Oracle: the integer construction of tests/test_mlp_weave_gpu.py (`_case`). Inputs, weights, biases and upstream gradients are in
{-1, 0, 1}; the test asserts on the host, in fp64, that the largest sum of ABSOLUTE products anywhere is < 2^24 (it is 135 282 over
the whole table, 0.8 % of 2^24); then every partial sum in any order is exact in fp32, and y, every gW and every gb must be
torch.equal to the fp64 result cast to fp32. No tolerance, no ReLU kink; split and fused weight gradient, wave and cooperative
forward, saved and recomputed activations must all give these bits whatever their summation order.

Every child records `p2c_mlp_plan` -- the library's own dispatch functions, asked without a launch -- for each case, and the
parent asserts that the plan is the cell the case is named for: a test that claims a cell proves the cell ran."""
import functools
import os
import random
import subprocess
import sys
import tempfile
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (this file also runs as a script)
from test_mlp_weave_gpu import LIMIT, _case  # noqa: E402

LDS_LIMIT = 160 * 1024
STATIC = ((52, 26, 13, 6, 39, 78, 156), (52, 26, 13, 6, 19, 39, 78), (52, 26, 13, 6, 13, 26, 52))      # providers 1, 2, 3
STACKS = STATIC + (
    (50, 25, 12, 6, 39, 78, 156),           # generic, near-static widths
    (1, 1),                                 # narrowest; one layer
    (4, 8),                                 # one layer; vector x and y
    (15, 16, 17, 1),                        # ones row at 15 and at 16 (a new k-group); unit row in a second tile
    (3, 159),                               # widest output; scalar y
    (159, 4),                               # widest input; 40 x floats per lane in the wave kernel (FW_XU)
    (20, 9, 33, 4, 17, 5, 31, 2, 12),       # 8 layers
    (60, 112, 128),                         # 92 tiles, image 108 672 B -> stage_rest; lds_fwd_wave 165 248 B: never the wave forward
    (96, 95, 143),                          # exactly 96 tiles, image 100 224 B; lds_fwd_wave 161 152 B fits: wave forward, big image
)
ROWS = (1, 16, 17, 48, 49, 100, 113, 150)   # 1, 1, 2, 3, 4, 7, 8, 10 sample tiles
# x and gy as contiguous views whose data pointer is 4 bytes off a 16-byte boundary: the scalar vec_x / vec_gy path at widths
# divisible by 4 (a static and a generic kernel)
MISALIGNED = ((52, 26, 13, 6, 39, 78, 156), (4, 8))
# The draws of `_case` whose results would be vacuous: (1,1) draws W = b = 0 (y == 0) at these rows, (15,16,17,1) at 16 rows a
# zero gradient for one parameter tensor. Another draw of the same distribution each (the smallest salt that passes
# `_nonvacuous`, found on the host); every other case keeps salt 0.
SALTS = {((1, 1), 17): 1, ((1, 1), 48): 1, ((1, 1), 49): 1, ((1, 1), 150): 1, ((15, 16, 17, 1), 16): 1}
# the figures the stack table above quotes, held to ops.mlp_geometry (and that to p2c_mlp_plan) below
QUOTED = {(60, 112, 128): dict(tiles=92, image_floats=108672 // 4, lds_fwd_wave=165248, lds_bwd=141312),
          (96, 95, 143): dict(tiles=96, image_floats=100224 // 4, lds_fwd_wave=161152)}
# pass ops.mlp_supported's tile and width limits, but the backward's LDS does not fit (166 336 B and 165 376 B of 163 840 B)
LDS_REFUSED = ((96, 48, 24, 12, 33, 66, 132), (82, 54, 25, 78, 77, 50, 27))
TOO_MANY_TILES = (127, 96, 127)             # 104 weight-gradient tiles: the forward runs, the backward is refused

MAX_BLOCKS = 2
CONFIGS = {
    'C0': dict(env={}, stacks=STACKS, doc='the default rules'),
    'C1': dict(env={'P2C_MLP_GENERIC': '1'}, stacks=STATIC, doc='the generic kernels at the LinearAE shapes'),
    'C2': dict(env={'P2C_MLP_SAVE': '0', 'P2C_MLP_FWD': 'coop', 'P2C_MLP_WGRAD': 'fused'}, stacks=STACKS, doc='the plain cell'),
    'C3': dict(env={'P2C_MLP_WGRAD': 'split', 'P2C_MLP_FWD': 'wave'}, stacks=STACKS, doc='split everywhere, wave where LDS allows'),
}
OVERRIDES = ('P2C_MLP_GENERIC', 'P2C_MLP_SAVE', 'P2C_MLP_FWD', 'P2C_MLP_WGRAD', 'P2C_MLP_MAX_BLOCKS')


def _name(dims, rows, misaligned=False):
    return '-'.join(map(str, dims)) + f'/{rows}' + ('/off4' if misaligned else '')


def _cases(config):
    """(dims, rows, misaligned) of one child, in the order it runs them."""
    cases = [(dims, rows, False) for dims in CONFIGS[config]['stacks'] for rows in ROWS]
    if config == 'C0':
        cases += [(dims, rows, True) for dims in MISALIGNED for rows in ROWS]
    return cases


@functools.lru_cache(maxsize=None)
def _reference(dims, rows):
    """`_case` of one (stack, rows), computed once per process and shared by every configuration; nobody writes to it."""
    return _case(list(dims), rows, SALTS.get((dims, rows), 0))


def _nonvacuous(ref):
    _, _, _, _, y_ref, gW_ref, gb_ref, _ = ref
    return bool((y_ref != 0).any()) and all(bool((g != 0).any()) for g in gW_ref) and all(bool((g != 0).any()) for g in gb_ref)


def _expected_cell(config, dims, rows):
    """The cell a case is named for, by sample-tile count at two workgroups (the rules as DESIGN.md states them):
    one tile: fused, recompute, cooperative, one workgroup; 2 - 3 tiles: split, two workgroups; 4 - 7 tiles: fused and saved;
    8 tiles and more: wave forward where its LDS fits. The overrides of the configuration on top."""
    tiles, layers = (rows + 15) // 16, len(dims) - 1
    wave_fits = dims != (60, 112, 128)                       # (held to mlp_geometry in the host test below)
    blocks = min(tiles, MAX_BLOCKS)
    split = 2 <= tiles <= 3
    wave = wave_fits and tiles >= 4 * MAX_BLOCKS
    if config == 'C2':
        split, wave, save = False, False, False
    else:
        if config == 'C3':
            split, wave = True, wave_fits
        save = layers >= 2 and not split and tiles >= 2 * blocks
    provider = STATIC.index(dims) + 1 if dims in STATIC and config != 'C1' else 0
    return dict(provider=provider, wave_forward=int(wave), split_wgrad=int(split), save_activations=int(save),
                fwd_blocks=min((tiles + 3) // 4, MAX_BLOCKS) if wave else blocks, bwd_blocks=blocks, fwd_ok=1, bwd_ok=1)


# ---------------------------------------------------------------------------------------------------------------- host
def test_case_table_holds_its_preconditions_on_the_host():
    """No GPU: for the whole case table the 2^24 precondition of exactness, the non-vacuity of every case of 16 rows and more (a
    non-zero entry in y and in every gW and gb), the salt table being minimal, the geometry figures the stack table quotes, and
    that the expected cells cover every regime the file claims."""
    from pedestrians_video_2_carla_amd import ops
    worst_all = 0.0
    for dims in STACKS:
        for rows in ROWS:
            ref = _reference(dims, rows)
            worst_all = max(worst_all, ref[-1])
            assert ref[-1] < LIMIT, f'precondition of the test violated at {_name(dims, rows)}: {ref[-1]} >= 2^24'
            if rows >= 16:
                assert _nonvacuous(ref), f'{_name(dims, rows)}: y or a gradient of the reference is all zero -- pick another salt'
    for (dims, rows), salt in SALTS.items():
        assert all(not _nonvacuous(_case(list(dims), rows, s)) for s in range(salt)), f'{_name(dims, rows)}: a smaller salt would do'
    print(f'largest sum of absolute products over the table: {worst_all:.0f} = {100 * worst_all / LIMIT:.2f} % of 2^24')
    assert worst_all < LIMIT / 100          # (135 282 with the generator of torch 2.x: two orders of magnitude of room)
    for dims, quoted in QUOTED.items():
        geo = ops.mlp_geometry(dims)
        assert {k: geo[k] for k in quoted} == quoted, (dims, geo)
    one_round = 12 * 512 * 16               # STAGE_U float4 of NTH threads: what one staging round holds
    assert 4 * ops.mlp_geometry((60, 112, 128))['image_floats'] > one_round and 4 * ops.mlp_geometry((96, 95, 143))['image_floats'] > one_round
    assert max(4 * ops.mlp_geometry(d)['image_floats'] for d in STACKS[:-2]) <= one_round
    for dims in STACKS:
        geo = ops.mlp_geometry(dims)
        assert ops.mlp_supported(dims) and geo['lds_fwd'] <= LDS_LIMIT and geo['lds_bwd'] <= LDS_LIMIT and geo['tiles'] <= 96
        assert (geo['lds_fwd_wave'] <= LDS_LIMIT) == (dims != (60, 112, 128)), (dims, geo)
    for dims in LDS_REFUSED:
        geo = ops.mlp_geometry(dims)
        assert geo['tiles'] <= 96 and geo['lds_fwd'] <= LDS_LIMIT < geo['lds_bwd'] and not ops.mlp_supported(dims), (dims, geo)
    assert ops.mlp_geometry(TOO_MANY_TILES)['tiles'] == 104 and not ops.mlp_supported(TOO_MANY_TILES)
    assert not ops.mlp_supported((0, 5)) and not ops.mlp_supported((5, -3, 2)) and not ops.mlp_supported((5, 160))
    assert not ops.mlp_supported((5,)) and not ops.mlp_supported((4,) * 10) and ops.mlp_supported((4,) * 9)
    # every regime is visited: (wave, split, saved) of the expected cells, and several tiles per workgroup in each of them
    def regimes(cfg, stacks=None):
        return {(c['wave_forward'], c['split_wgrad'], c['save_activations'])
                for c in (_expected_cell(cfg, d, r) for d, r, _ in _cases(cfg) if stacks is None or d in stacks)}
    assert regimes('C1') == {(0, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1)}
    assert regimes('C0') == regimes('C1') | {(1, 0, 0)}                  # (one layer saves nothing)
    assert regimes('C0', STACKS[3:]) == regimes('C0') and regimes('C0', STATIC) == regimes('C1')     # generic and static kernels
    assert regimes('C0', ((60, 112, 128),)) == {(0, 0, 0), (0, 1, 0), (0, 0, 1)}                      # never the wave forward
    assert regimes('C2') == {(0, 0, 0)} and regimes('C3') == {(1, 1, 0), (0, 1, 0)}
    assert regimes('C3', ((60, 112, 128),)) == {(0, 1, 0)}


# ------------------------------------------------------------------------------------------------------------ children
def _run_case(dims, rows, misaligned):
    """One case on the device (child process): y, gW, gb on the host and the library's plan for it."""
    from pedestrians_video_2_carla_amd import ops
    Ws, bs, x, gy, _, _, _, _ = _reference(dims, rows)
    d = torch.device('cuda:0')

    def rows_of(t):
        if not misaligned:
            return t.float().to(d)
        buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=d)         # (allocations are 16-byte aligned)
        off = 1 + (-buf.data_ptr() // 4) % 4                                    # floats up to 4 bytes past a 16-byte boundary
        view = buf[off:off + t.numel()].view(t.shape)
        view.copy_(t)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view

    Wd = [w.float().to(d).requires_grad_(True) for w in Ws]
    bd = [b.float().to(d).requires_grad_(True) for b in bs]
    y = ops.fused_mlp(rows_of(x), Wd, bd)
    y.backward(rows_of(gy))
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), gW=[w.grad.cpu() for w in Wd], gb=[b.grad.cpu() for b in bd], plan=ops.mlp_plan(dims, rows))


def _child_main(config, out):
    assert os.environ.get('P2C_MLP_MAX_BLOCKS') == str(MAX_BLOCKS), 'run by the `cells` fixture'
    t0 = time.perf_counter()
    results = {_name(*case): _run_case(*case) for case in _cases(config)}
    results['seconds_on_cases'] = time.perf_counter() - t0
    torch.save(results, out)


_child_failed = None        # the first child that ended with a non-zero status: no further child is started in this session
_results = {}
_seconds = {}


def _child(config):
    """The results of one configuration's child, run once per session. Children run one at a time; after one has failed (or run
    into its time limit) no other is started."""
    global _child_failed
    if config in _results:
        return _results[config]
    if _child_failed is not None:
        pytest.fail(f'child {_child_failed} failed earlier in this session: child {config} is not started', pytrace=False)
    env = {k: v for k, v in os.environ.items() if k not in OVERRIDES}
    env.update(CONFIGS[config]['env'], P2C_MLP_MAX_BLOCKS=str(MAX_BLOCKS))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, f'{config}.pt')
        t0 = time.perf_counter()
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), config, out], env=env, capture_output=True, text=True,
                                 timeout=300)
        except subprocess.TimeoutExpired as e:
            _child_failed = config
            pytest.fail(f'child {config} ran into its time limit: {str(e.stdout)[-3000:]} {str(e.stderr)[-3000:]}', pytrace=False)
        _seconds[config] = time.perf_counter() - t0
        if res.returncode != 0:
            _child_failed = config
            pytest.fail(f'child {config} ended with status {res.returncode}:\n{res.stdout[-3000:]}\n{res.stderr[-3000:]}', pytrace=False)
        _results[config] = torch.load(out)
    print(f'child {config} ({CONFIGS[config]["doc"]}): {len(_results[config]) - 1} cases, wall time {_seconds[config]:.1f} s, '
          f'of which {_results[config]["seconds_on_cases"]:.1f} s on the cases')
    return _results[config]


@pytest.fixture(scope='module')
def cells():
    return _child


ALL_CASES = [(config,) + case for config in CONFIGS for case in _cases(config)]


@pytest.mark.gpu
@pytest.mark.parametrize('config,dims,rows,misaligned', ALL_CASES, ids=[f'{c[0]}-{_name(*c[1:])}' for c in ALL_CASES])
def test_cell_runs_as_planned_and_equals_fp64(cells, config, dims, rows, misaligned):
    """One case of one child: the library planned the cell the case is named for, and y, every gW and every gb are the fp64
    results, bit for bit."""
    got = cells(config)[_name(dims, rows, misaligned)]
    ref = _reference(dims, rows)
    _, _, _, _, y_ref, gW_ref, gb_ref, worst = ref
    assert worst < LIMIT, f'precondition of the test violated: {worst} >= 2^24 -- choose other inputs'
    if rows >= 16:
        assert _nonvacuous(ref)
    plan, want = got['plan'], _expected_cell(config, dims, rows)
    assert {k: plan[k] for k in want} == want, f'planned {plan}, the case is named for {want}'
    assert got['y'].shape == y_ref.shape and torch.equal(got['y'], y_ref.float()), \
        f'y: max |diff| {(got["y"].double() - y_ref).abs().max().item()}, {int((got["y"].double() != y_ref).sum())} entries'
    for l in range(len(dims) - 1):
        assert torch.equal(got['gW'][l], gW_ref[l].float()), \
            f'gW[{l}]: max |diff| {(got["gW"][l].double() - gW_ref[l]).abs().max().item()}, {int((got["gW"][l].double() != gW_ref[l]).sum())} entries'
        assert torch.equal(got['gb'][l], gb_ref[l].float()), \
            f'gb[{l}]: max |diff| {(got["gb"][l].double() - gb_ref[l]).abs().max().item()}, {int((got["gb"][l].double() != gb_ref[l]).sum())} entries'


@pytest.mark.gpu
def test_split_and_fused_weight_gradient_give_the_same_bits_in_every_cell(cells):
    """C2 (fused, cooperative, recomputed) against C3 (split, wave) and against the default rules, case by case: the summation
    orders differ (per-workgroup accumulators and a 16-group reduction; eight K-split partials of eight waves each), the values
    must not in any bit (torch.equal on fp32: only the sign of a zero is free, see fwd_ksteps in p2c_mlp_dev.h)."""
    plain, split, default = cells('C2'), cells('C3'), cells('C0')
    flat = lambda r: torch.cat([t.reshape(-1) for t in [r['y']] + r['gW'] + r['gb']])     # noqa: E731
    n = 0
    for dims, rows, _ in _cases('C2'):
        key = _name(dims, rows)
        assert plain[key]['plan']['split_wgrad'] == 0 and split[key]['plan']['split_wgrad'] == 1
        a, b, c = flat(plain[key]), flat(split[key]), flat(default[key])
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c), \
            f'{key}: {int((a != b).sum())} values differ split / fused, {int((a != c).sum())} default / fused'
        n += 1
    assert n == len(STACKS) * len(ROWS)


# ------------------------------------------------------------------------------------------ in process, 256 workgroups
def _params(dims, device):
    gen = torch.Generator().manual_seed(sum(dims))
    Ws = [torch.randint(-1, 2, (o, i), generator=gen).float().to(device).requires_grad_(True) for i, o in zip(dims[:-1], dims[1:])]
    bs = [torch.randint(-1, 2, (o,), generator=gen).float().to(device).requires_grad_(True) for o in dims[1:]]
    return Ws, bs


@pytest.mark.gpu
@pytest.mark.parametrize('dims', [(52, 26, 13, 6, 39, 78, 156), (15, 16, 17, 1), (4, 8)], ids=lambda d: '-'.join(map(str, d)))
def test_empty_batch_gives_an_empty_output_and_zero_gradients(dims):
    """N = 0: y has shape (0, n_L); after backward every gradient is exactly zero (the backward's workgroup sees no sample tile
    and writes a zero partial: the gradients are WRITTEN, so whatever the buffers held before is gone)."""
    from pedestrians_video_2_carla_amd import ops
    d = torch.device('cuda:0')
    Ws, bs = _params(dims, d)
    y = ops.fused_mlp(torch.empty(0, dims[0], device=d), Ws, bs)
    assert y.shape == (0, dims[-1])
    y.backward(torch.empty(0, dims[-1], device=d))
    torch.cuda.synchronize()
    for p in Ws + bs:
        assert p.grad is not None and p.grad.shape == p.shape and not p.grad.any(), 'a gradient of an empty batch is not zero'


@pytest.mark.gpu
def test_more_than_96_weight_gradient_tiles_run_forward_and_refuse_the_backward():
    """(127,96,127) has 104 tiles of dW: the forward holds no tile table and runs (checked against fp64 on integer inputs), the
    backward raises, and ops.mlp_supported says so beforehand."""
    from pedestrians_video_2_carla_amd import _lib, ops
    dims, rows = TOO_MANY_TILES, 37
    assert not ops.mlp_supported(dims)
    plan = ops.mlp_plan(dims, rows)
    assert plan['tiles'] == 104 and plan['fwd_ok'] == 1 and plan['bwd_ok'] == 0
    Ws, bs, x, gy, y_ref, _, _, worst = _case(list(dims), rows)
    assert worst < LIMIT and (y_ref != 0).any()
    d = torch.device('cuda:0')
    Wd = [w.float().to(d).requires_grad_(True) for w in Ws]
    bd = [b.float().to(d).requires_grad_(True) for b in bs]
    y = ops.fused_mlp(x.float().to(d), Wd, bd)
    assert torch.equal(y.detach().cpu(), y_ref.float())
    with pytest.raises(_lib.P2CError):
        y.backward(gy.float().to(d))


# ------------------------------------------------------------------------------------- the predicate and the library
def _agree(ops, dims, rows=100):
    """ops.mlp_geometry and ops.mlp_supported against p2c_mlp_plan for one stack; returns whether it is supported."""
    plan, geo = ops.mlp_plan(dims, rows), ops.mlp_geometry(dims)
    assert plan is not None, dims
    assert {k: plan[k] for k in geo} == geo, f'{dims}: library {plan}, ops.mlp_geometry {geo}'
    assert ops.mlp_supported(dims) == bool(plan['fwd_ok'] and plan['bwd_ok']), f'{dims}: mlp_supported {ops.mlp_supported(dims)}, {plan}'
    assert plan['fwd_ok'] == (plan['lds_fwd'] <= LDS_LIMIT) and plan['bwd_ok'] == (plan['lds_bwd'] <= LDS_LIMIT and plan['tiles'] <= 96)
    return ops.mlp_supported(dims)


@pytest.mark.gpu
def test_mlp_supported_and_mlp_geometry_equal_the_library_plan():
    """Launches nothing. The pure-Python predicate (it is asked where the library may not be loaded) against the functions the
    launch code decides with: every stack of the table, the two stacks whose backward does not fit the LDS, 104 tiles, and 2 000
    seeded random stacks of 1 - 8 layers and widths 1 - 159; widths and layer counts outside the ABI are refused by both."""
    from pedestrians_video_2_carla_amd import ops
    for dims in STACKS:
        assert _agree(ops, dims)
    for dims in LDS_REFUSED + (TOO_MANY_TILES,):
        assert not _agree(ops, dims)
        assert ops.mlp_plan(dims, 100)['fwd_ok'] == 1 and ops.mlp_plan(dims, 100)['bwd_ok'] == 0
    rnd = random.Random(20260)
    supported = sum(_agree(ops, tuple(rnd.randint(1, 159) for _ in range(rnd.randint(1, 8) + 1)), rnd.randint(0, 5000))
                    for _ in range(2000))
    print(f'{supported} of 2000 random stacks are supported')
    assert 200 < supported < 1800            # both answers are exercised
    for dims in ((0, 5), (5, 160), (5, -1, 5), (4,) * 10, (5,)):
        assert ops.mlp_plan(dims, 16) is None and not ops.mlp_supported(dims), dims


@pytest.mark.gpu
def test_linear_ae_whose_backward_does_not_fit_the_lds_takes_the_aten_path():
    """LinearAE over 48 input joints and 22 output nodes in 6-D is (96,48,24,12,33,66,132): 94 tiles, so the tile limit passes,
    but its backward needs 166 336 B of LDS. The module must not hand it to the fused kernel (whose forward would run and whose
    backward would raise): forward + backward run on the device through the plain layers and match them in fp64."""
    import copy
    from pedestrians_video_2_carla_amd.data.base.skeleton import Skeleton
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    d = torch.device('cuda:0')
    torch.manual_seed(48)
    model = LinearAE(input_nodes=Skeleton('Joints48', [(f'j{i}', i) for i in range(48)]),
                     output_nodes=Skeleton('Nodes22', [(f'n{i}', i) for i in range(22)])).to(d)
    model.rotation_output_format = 'rotation_6d'
    assert model.fused_mlp
    fa_dims = [96] + [m.out_features for m in model._linears()]
    assert tuple(fa_dims) == LDS_REFUSED[0] and model.fused_args(d) is None
    ref = copy.deepcopy(model).double()
    ref.fused_mlp = False
    x, w = torch.randn(3, 5, 48, 2, device=d), torch.randn(3, 5, 22, 6, device=d)
    y = model(x)
    (y * w).sum().backward()
    torch.cuda.synchronize()
    yr = ref(x.double())
    (yr * w.double()).sum().backward()
    assert y.shape == (3, 5, 22, 6) and torch.isfinite(y).all()
    assert (y.double() - yr).abs().max() <= 2e-5 * yr.abs().max()
    for (n, p), q in zip(model.named_parameters(), ref.parameters()):
        assert p.grad is not None and (p.grad.double() - q.grad).abs().max() <= 2e-5 * q.grad.abs().max() + 1e-30, n


if __name__ == '__main__':      # a child of `cells`: every case of configuration sys.argv[1] -> sys.argv[2]
    _child_main(sys.argv[1], sys.argv[2])
