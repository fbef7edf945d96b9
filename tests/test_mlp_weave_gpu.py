"""GPU: the k-loops of the fused MLP (csrc/p2c_mlp_dev.h: layer_forward_nt, layer_dgrad and the weight gradient behind them) on
inputs where every result is an exact integer. A k-loop goes wrong by pairing an operand with the wrong step, by dropping or
doubling a step at a group boundary or in a tail, or by reading past the layer; a tolerance against fp64 can hide one wrong
k-step among dozens, so nothing here has a tolerance.

Inputs, weights, biases and upstream gradients are small integers. The test first asserts ITS OWN precondition on the host in
fp64: at every layer, forward and backward, and for every weight and bias gradient, the sum of the ABSOLUTE products that feed
one output is below 2^24. Then every partial sum, in any order and grouping, is an integer of magnitude < 2^24 and so exact in
fp32: the kernel's result must be torch.equal to the fp64 result cast to fp32. The precondition is a property of the inputs
(seed and value distribution below), not of the kernel."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LIMIT = float(2 ** 24)
ROWS = (1, 16, 17, 37)   # one partial sample tile, one full tile, a tile boundary crossed (twice)
# The static LinearAE widths: forward 14 / 7 / 4 / 2 / 10 / 20 k-steps, dgrad 39 / 20 / 10 / 2 / 4 (tails of 0, 2 and 3 steps,
# 0, 1, 2, 3, 5 and 9 whole groups of four). The generic stacks put n_in + 1 and n_out on one, two, three and ten whole groups
# (16, 32, 48, 160 rows) and just past them.
STACKS = ([52, 26, 13, 6, 39, 78, 156], [3, 5], [15, 16, 17], [31, 33, 47, 6], [52, 159], [159, 49, 32])


def _ints(gen, shape, p_nonzero):
    """Integers from {-1, 0, 1}: non-zero with probability p_nonzero, either sign equally likely."""
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1
    keep = torch.rand(shape, generator=gen, dtype=torch.float64) < p_nonzero
    return (sign * keep).double()


def _case(dims, rows, salt=0):
    """Inputs and the fp64 results of one case, with the largest sum of absolute products met anywhere. `salt` picks another draw
    of the same distribution (tests/test_mlp_cells_gpu.py: a draw whose results are not all zero)."""
    gen = torch.Generator().manual_seed(1000 * len(dims) + 10 * dims[-1] + rows + 1000003 * salt)
    Ws = [_ints(gen, (o, i), 0.5) for i, o in zip(dims[:-1], dims[1:])]
    bs = [_ints(gen, (o,), 0.5) for o in dims[1:]]
    x, gy = _ints(gen, (rows, dims[0]), 0.75), _ints(gen, (rows, dims[-1]), 0.75)
    L, worst = len(Ws), 0.0
    hs = [x]
    for l in range(L):
        z = hs[l] @ Ws[l].T + bs[l]
        worst = max(worst, (hs[l].abs() @ Ws[l].abs().T + bs[l].abs()).max().item())
        hs.append(z if l == L - 1 else z.clamp_min(0.0))
    g, gWs, gbs = gy, [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        gWs[l], gbs[l] = g.T @ hs[l], g.sum(0)
        worst = max(worst, (g.abs().T @ hs[l].abs()).max().item(), g.abs().sum(0).max().item())
        if l > 0:
            worst = max(worst, (g.abs() @ Ws[l].abs()).max().item())
            g = (g @ Ws[l]) * (hs[l] > 0)
    return Ws, bs, x, gy, hs[-1], gWs, gbs, worst


@pytest.mark.parametrize('rows', ROWS)
@pytest.mark.parametrize('dims', STACKS, ids=lambda d: '-'.join(map(str, d)))
def test_integer_inputs_give_the_exact_result(dims, rows):
    from pedestrians_video_2_carla_amd import ops
    assert ops.mlp_supported(dims)
    Ws, bs, x, gy, y_ref, gW_ref, gb_ref, worst = _case(dims, rows)
    print(f'{dims} rows {rows}: largest sum of absolute products {worst:.0f} (limit {LIMIT:.0f})')
    assert worst < LIMIT, f'precondition of the test violated: {worst} >= 2^24 -- choose other inputs'
    d = torch.device('cuda:0')
    Wd = [w.float().to(d).requires_grad_(True) for w in Ws]
    bd = [b.float().to(d).requires_grad_(True) for b in bs]
    y = ops.fused_mlp(x.float().to(d), Wd, bd)
    y.backward(gy.float().to(d))
    assert torch.equal(y.detach().cpu(), y_ref.float()), f'y: {(y.detach().cpu().double() - y_ref).abs().max().item()}'
    for l in range(len(Ws)):
        assert torch.equal(Wd[l].grad.cpu(), gW_ref[l].float()), \
            f'gW[{l}]: {(Wd[l].grad.cpu().double() - gW_ref[l]).abs().max().item()}'
        assert torch.equal(bd[l].grad.cpu(), gb_ref[l].float()), \
            f'gb[{l}]: {(bd[l].grad.cpu().double() - gb_ref[l]).abs().max().item()}'


@pytest.mark.parametrize('B,T', [(1, 1), (3, 5)])
def test_fused_step_losses_equal_the_separate_kernels_at_tiny_batches(monkeypatch, B, T):
    """One clip of one frame, three clips of five frames: the clip kernel's MLP chains with one and five live sample columns
    of sixteen. The rule of test_fused_gradient_against_the_separate_kernels for the losses: the same bits."""
    from test_clip_chain_gpu import _one_step
    monkeypatch.setenv('P2C_FUSED_UPDATE', '0')
    sep = _one_step(monkeypatch, '0', B=B, T=T, missing=0.3, otype='pose_changes')
    fus = _one_step(monkeypatch, '1', B=B, T=T, missing=0.3, otype='pose_changes')
    for a, b, what in zip(sep[:3], fus[:3], ('loss', 'loc_2d', 'loc_3d')):
        print(f'B={B} T={T} {what}: separate {a.item():.9g} fused {b.item():.9g}')
        assert torch.isfinite(a).all() and torch.equal(a, b), f'{what}: max |diff| {(a - b).abs().max().item():.3e}'
