"""GPU: K21, the fused ReLU stack (csrc/p2c_relu_stack.hip, ops.relu_stack) against an fp64 CPU evaluation of the same stack:
y and every gW / gb within 1e-4 x scale for the widths Seq2SeqFlatEmbeddings uses, single rows, exact and ragged 16-row tiles,
T = 1 and a grid-stride case; the sequence-first / time-reversed row mapping exactly; accumulation into existing gradients;
bitwise reproducibility; the coverage rule."""
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-4
DIMS = [(52, 128, 64), (50, 128, 64), (52, 64), (78, 128, 64), (52, 37, 96, 17, 64, 33)]
SHAPES = [(1, 1), (1, 16), (4, 15), (17, 1), (33, 15)]
KINK_MARGIN = 1e-4      # |pre-activation| every test frame keeps, in fp64 (see problem())
MAX_BLOCKS = 256         # workgroups the launch code starts at most (p2c_relu_stack.hip: MAX_BLOCKS), one 16-row tile at a time


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def close(a, b, what, rtol=RTOL):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err == err and err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


def problem(dims, B, T, seed=0):
    g = torch.Generator().manual_seed(1000 * len(dims) + 10 * B + T + seed)
    x = torch.randn(B * T, dims[0], generator=g)
    ws = [torch.randn(o, i, generator=g) / i ** 0.5 for i, o in zip(dims[:-1], dims[1:])]
    bs = [torch.randn(o, generator=g) * 0.5 for o in dims[1:]]
    up = torch.randn(T, B, dims[-1], generator=g)
    # The gradient of a ReLU jumps at 0: a frame with a pre-activation inside the rounding of an fp32 dot product (at most
    # 160 terms of magnitude ~1: below 1e-5) has no fp32 answer to compare with fp64 -- either side of the kink is right and they
    # differ by a whole rank-one term. Such frames (about 1 % at this margin) are drawn again, on the host, in fp64.
    while True:
        h, bad = x.double(), torch.zeros(B * T, dtype=torch.bool)
        for w, b in zip(ws, bs):
            pre = h @ w.double().T + b.double()
            bad |= (pre.abs() < KINK_MARGIN).any(1)
            h = torch.relu(pre)
        if not bad.any():
            break
        x[bad] = torch.randn(int(bad.sum()), dims[0], generator=g)
    return x.view(B, T, dims[0]), ws, bs, up


def reference(x, ws, bs, up, flip):
    """fp64 on the host: batch-first evaluation, then permute(1,0,2) / flip(0)."""
    ws = [w.double().requires_grad_(True) for w in ws]
    bs = [b.double().requires_grad_(True) for b in bs]
    h = x.double()
    for w, b in zip(ws, bs):
        h = torch.relu(h @ w.T + b)
    y = h.permute(1, 0, 2)
    if flip:
        y = y.flip(0)
    (y * up.double()).sum().backward()
    return y.detach(), [w.grad for w in ws], [b.grad for b in bs]


def run(x, ws, bs, up, flip, d):
    from pedestrians_video_2_carla_amd import ops
    wd = [w.to(d).requires_grad_(True) for w in ws]
    bd = [b.to(d).requires_grad_(True) for b in bs]
    y = ops.relu_stack(x.to(d), wd, bd, flip=flip)
    (y * up.to(d)).sum().backward()
    return y.detach(), [w.grad for w in wd], [b.grad for b in bd]


@pytest.mark.parametrize('flip', [False, True])
@pytest.mark.parametrize('B,T', SHAPES)
@pytest.mark.parametrize('dims', DIMS, ids=lambda v: '-'.join(map(str, v)))
def test_matches_fp64(dims, B, T, flip):
    d = dev()
    x, ws, bs, up = problem(dims, B, T)
    y_r, gw_r, gb_r = reference(x, ws, bs, up, flip)
    y, gw, gb = run(x, ws, bs, up, flip, d)
    assert y.shape == (T, B, dims[-1]) and y.is_contiguous()
    close(y, y_r, 'y')
    for l in range(len(ws)):
        close(gw[l], gw_r[l], f'gW{l}'), close(gb[l], gb_r[l], f'gb{l}')


@pytest.mark.parametrize('B,T', [(4, 15), (33, 15), (17, 1)])
def test_row_mapping_is_exact(B, T):
    """Row b T + t of the batch-first evaluation (the same kernel over one clip of B T frames: output row = input row) is row
    t B + b of the sequence-first output, and row (T - 1 - t) B + b with flip -- bit for bit."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    dims = (52, 128, 64)
    x, ws, bs, _ = problem(dims, B, T)
    wd, bd = [w.to(d) for w in ws], [b.to(d) for b in bs]
    rows = ops.relu_stack(x.to(d).view(1, B * T, dims[0]), wd, bd).view(B, T, dims[-1])      # batch first
    plain = ops.relu_stack(x.to(d), wd, bd, flip=False)
    flipped = ops.relu_stack(x.to(d), wd, bd, flip=True)
    assert (rows != 0).any()
    assert torch.equal(plain, rows.permute(1, 0, 2))
    assert torch.equal(flipped, rows.permute(1, 0, 2).flip(0))


def test_grid_stride_many_row_tiles():
    """More 16-row tiles than workgroups: 2 x 256 tiles, three more and a ragged tail of 5 rows (B T = 1649 x 5 = 8245). y on 64
    sampled rows plus the first and the last (rows are independent), the gradients -- sums over all rows -- in full."""
    d = dev()
    dims, B, T = (52, 128, 64), 1649, 5
    assert B * T == (2 * MAX_BLOCKS + 3) * 16 + 5
    x, ws, bs, up = problem(dims, B, T)
    y, gw, gb = run(x, ws, bs, up, True, d)
    y_r, gw_r, gb_r = reference(x, ws, bs, up, True)
    n = B * T
    idx = torch.cat([torch.randperm(n - 2, generator=torch.Generator().manual_seed(5))[:64] + 1, torch.tensor([0, n - 1])])
    close(y.view(n, -1)[idx.to(d)], y_r.reshape(n, -1)[idx], 'y')
    for l in range(len(ws)):
        close(gw[l], gw_r[l], f'gW{l}'), close(gb[l], gb_r[l], f'gb{l}')


@pytest.mark.parametrize('dims', [(52, 128, 64), (52, 37, 96, 17, 64, 33)], ids=lambda v: '-'.join(map(str, v)))
def test_accumulate_adds_into_existing_gradients(dims):
    """Inside ops.grad_sinks the backward ADDS into param.grad (accumulate = 1): prefilled buffers end as prefill + gradient."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    B, T = 33, 15
    x, ws, bs, up = problem(dims, B, T)
    _, gw, gb = run(x, ws, bs, up, False, d)
    wd = [w.to(d).requires_grad_(True) for w in ws]
    bd = [b.to(d).requires_grad_(True) for b in bs]
    g = torch.Generator().manual_seed(9)
    pre = [torch.randn(p.shape, generator=g).to(d) for p in wd + bd]
    for p, q in zip(wd + bd, pre):
        p.grad = q.clone()
    with ops.grad_sinks(True):
        y = ops.relu_stack(x.to(d), wd, bd)
        (y * up.to(d)).sum().backward()
    for p, q, gr in zip(wd + bd, pre, gw + gb):
        assert torch.equal(p.grad, q + gr)


@pytest.mark.parametrize('dims,B,T', [((52, 128, 64), 33, 15), ((78, 128, 64), 300, 15)], ids=['small', 'grid-stride'])
def test_two_runs_are_bitwise_equal(dims, B, T):
    d = dev()
    x, ws, bs, up = problem(dims, B, T)
    a, b = run(x, ws, bs, up, True, d), run(x, ws, bs, up, True, d)
    assert torch.equal(a[0], b[0])
    for p, q in zip(a[1] + a[2], b[1] + b[2]):
        assert torch.equal(p, q)


def test_coverage_rule():
    from pedestrians_video_2_carla_amd import _lib, ops
    d = dev()
    for dims in DIMS:
        assert ops.relu_stack_supported(dims), dims
    assert not ops.relu_stack_supported((52, 512, 256))          # 660 KB of weight images
    assert not ops.relu_stack_supported((52, 8, 8, 8, 8, 8, 8))  # six layers
    x, ws, bs, _ = problem((52, 512, 256), 2, 3)
    with pytest.raises(_lib.P2CError, match='outside the fused kernel'):
        ops.relu_stack(x.to(d), [w.to(d) for w in ws], [b.to(d) for b in bs])
