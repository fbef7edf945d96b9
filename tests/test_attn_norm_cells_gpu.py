"""The transformer kernels -- K14 small attention (csrc/p2c_attn.hip), K15 LayerNorm (csrc/p2c_norm.hip), K20a attention with
dropout and K20b post-norm residual (csrc/p2c_encoder.hip) -- in every cell of their dispatch (template instantiation picked
from the shape) and in both regimes of their launch grids (one pass; workgroups striding over sequences or rows), through the
C ABI, against the written-out formula in fp64 (gradients by fp64 autograd of the same formula).

The host functions at the top MIRROR the dispatch code (family / row width / LDS bytes / grid of K14; lanes per row, vectors
per lane, rows per workgroup and workgroup count of K15 and K20b); ``test_dispatch_mirrors_and_case_coverage`` (not
gpu-marked) checks them against hand-computed cells and asserts that every reachable cell has a one-pass and a striding case.
``test_input_conditions`` (not gpu-marked) asserts on the fp64 reference alone what the GPU comparisons rely on.

Two criteria per output tensor:
  * the project's per-tensor bounds, max |got - ref| / max |ref| (tests/test_pose_former_gpu.py, tests/test_simple_transformer_gpu.py):
    K14 1e-5 on out and g_qkv; K20a 1e-4; K15 2e-5 on y, 5e-5 on gx, 5e-5 sqrt(rows) on the parameter gradients; K20b 1e-4 with
    the cancellation floor 1e-3 max(rstd |gz gamma|) under dx and ds;
  * per row -- a (sequence, token) row of the attentions, a row of the norms -- max |got - ref| over the row / max |ref| over
    the SAME row (for the LayerNorm input gradients: the larger of that and the cancellation floor above), so that one wrong
    row of small magnitude cannot hide behind the tensor's largest element. Its bound is ROW_BOUND below: four times the worst
    such ratio of the same formula evaluated in fp32 on the host (torch CPU) on the same inputs, per kernel family. The factor
    covers the kernels' different but fixed summation order, __expf / rsqrtf in place of the correctly rounded functions and the
    backward's recomputed probabilities.

Everything is unit-scale but for the ``maxrow`` inputs: scores that span more than 90 in every row with the row maximum in the last
valid column -- exponentiating them without subtracting the row maximum overflows. Their q and k are small dyadic numbers and their
scale a power of two, so every score is exact in fp32 in any summation order: what is compared is the softmax, not the rounding
of a score of size 300.
"""
import ctypes
import math

import pytest
import torch

E_NULL, E_SHAPE = -1, -2
LDS_BOUND = 156 * 1024
SENTINEL = 123.25


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(v):
    """the fp32 number the C ABI receives for a float argument: both sides of a comparison get the same scale / eps"""
    return float(torch.tensor(v, dtype=torch.float32))


# ======================================================================================================================
# dispatch mirrors (host)
# ======================================================================================================================
def k14_family(N, D):
    """family() of p2c_attn.hip; the generic instantiation holds a vector (D % 4 == 0) and a scalar path."""
    if D == 4:
        return 'narrow-4'
    if D == 8:
        return 'narrow-8'
    if D % 4 == 0 and D > 8 and N <= 16:
        return 'wide'
    return 'generic-vector' if D % 4 == 0 else 'generic-scalar'


def k14_nb(N):
    return 16 if N <= 16 else 32 if N <= 32 else 64


def k14_cell(N, D):
    return k14_family(N, D), k14_nb(N)


def k14_lds(N, heads, D, bwd):
    E, NN = heads * D, N * N
    return 4 * (N * (4 * E + 8) + 2 * heads * NN if bwd else N * (3 * E + 4) + heads * NN)


def k14_supported(N, heads, D, bwd=True):
    return 1 <= N <= 64 and heads >= 1 and D >= 1 and (heads * D) % 4 == 0 and k14_lds(N, heads, D, bwd) <= LDS_BOUND


def k14_grid(S, N, heads, D, bwd):
    per_cu = max(1, LDS_BOUND // k14_lds(N, heads, D, bwd))
    return min(256 * min(per_cu, 8) * 4, S)


K14_CELLS = ([('narrow-4', nb) for nb in (16, 32, 64)] + [('narrow-8', nb) for nb in (16, 32, 64)] + [('wide', 16)] +
             [('generic-vector', nb) for nb in (32, 64)] + [('generic-scalar', nb) for nb in (16, 32, 64)])


def k15_cell(D):
    """(G lanes per row, KV float4 per lane) of P2C_LN_DISPATCH"""
    return (8, 1) if D <= 32 else (16, 1) if D <= 64 else (32, 1) if D <= 128 else (64, 1) if D <= 256 else (64, 2) if D <= 512 else (64, 4)


def k20b_cell(D):
    """(G lanes per row, KV columns per lane) of P2C_PN_DISPATCH"""
    return (8, 4) if D <= 32 else (16, 4) if D <= 64 else (32, 4) if D <= 128 else (64, 4) if D <= 256 else (64, 8) if D <= 512 else (64, 16)


def norm_rpb(D):
    """rows per workgroup pass: 256 threads / G lanes per row (both norms)"""
    return 32 if D <= 32 else 16 if D <= 64 else 8 if D <= 128 else 4


def norm_blocks(rows, D):
    return max(1, min(1024, -(-rows // norm_rpb(D))))


def norm_strides(rows, D):
    return rows > 1024 * norm_rpb(D)


K15_CELLS = [(8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 4)]
K20B_CELLS = [(8, 4), (16, 4), (32, 4), (64, 4), (64, 8), (64, 16)]


# ======================================================================================================================
# case tables
# ======================================================================================================================
# K14: (N, heads, head_dim). Remainders in every loop: N % 4 != 0 (4-unrolled tails), head widths 12 / 20 / 36 / 104 (the 8-step
# blocks and the tail of head_dots_mfma), 24 / 136 (two / nine column tiles of contract_mfma), N at 1, at the row-width edges
# 16 | 17, 32 | 33, 64 and in between, more than four heads (the wave-dealt loops go round twice), heads * N > 256 (the
# row-owner loops go round twice). N = 64 leaves room for four narrow-4 / three narrow-8 heads under the LDS bound of the backward.
K14_ONE_PASS = {
    'narrow-4': [(5, 1, 4), (16, 8, 4), (26, 8, 4), (33, 9, 4), (64, 4, 4)],
    'narrow-8': [(12, 4, 8), (17, 3, 8), (32, 9, 8), (64, 3, 8)],
    'wide': [(1, 1, 12), (9, 8, 104), (16, 2, 16), (15, 5, 20), (7, 6, 136), (13, 3, 36), (9, 2, 24)],
    'generic-vector': [(17, 3, 12), (33, 2, 12), (64, 1, 20), (64, 1, 120)],        # (64, 1, 120): 157 696 of 159 744 bytes of LDS
    'generic-scalar': [(7, 4, 3), (16, 4, 13), (17, 4, 5), (40, 4, 7), (64, 2, 6)],
}
K14_OTHER_SCALE = {(26, 8, 4), (17, 3, 8), (15, 5, 20), (33, 2, 12), (16, 4, 13)}      # scale 0.37 instead of head_dim ** -0.5
# small LDS images: the grid is the capped 8192 (or a little less at NB = 64); S = grid + 3: some workgroups take two sequences,
# most take one; 'stride2': S = 2 grid + 1
K14_STRIDE = [((5, 1, 4), 'stride2'), ((17, 1, 4), 'stride'), ((33, 1, 4), 'stride'),
              ((12, 4, 8), 'stride'), ((17, 1, 8), 'stride'), ((33, 1, 8), 'stride'),
              ((9, 1, 12), 'stride2'),
              ((17, 1, 12), 'stride'), ((33, 1, 12), 'stride'),
              ((7, 4, 3), 'stride'), ((17, 4, 5), 'stride'), ((33, 2, 6), 'stride')]
K14_MAXROW = [(26, 8, 4), (17, 3, 8), (9, 8, 104), (33, 2, 12), (17, 4, 5)]
K20A_MAXROW = (33, 2, 5)


def k14_cases():
    cases = []
    for fam, shapes in K14_ONE_PASS.items():
        for shp in shapes:
            cases.append(dict(shape=shp, regime='one', kind='randn', scale=0.37 if shp in K14_OTHER_SCALE else shp[2] ** -0.5))
    for shp, regime in K14_STRIDE:
        cases.append(dict(shape=shp, regime=regime, kind='randn', scale=shp[2] ** -0.5))
    for shp in K14_MAXROW:
        cases.append(dict(shape=shp, regime='one', kind='maxrow', scale=maxrow_scale(shp[2])))
    for i, c in enumerate(cases):
        N, H, D = c['shape']
        grid = 256 * min(max(1, LDS_BOUND // k14_lds(N, H, D, False)), 8) * 4      # the forward's grid: the larger of the two
        c['S'] = {'one': 3, 'stride': grid + 3, 'stride2': 2 * grid + 1}[c['regime']]
        c['scale'] = _f32(c['scale'])
        c['seed'] = 100 + i
        c['family'] = k14_family(N, D)
        c['id'] = 'N{}-h{}-d{}-S{}-{}{}'.format(N, H, D, c['S'], c['kind'], '' if c['scale'] == _f32(D ** -0.5) else '-scale')
    return cases


def maxrow_scale(D):
    return 2.0 ** -int(math.floor(math.log2(D)))


def randn_qkv(S, N, H, D, seed):
    g = _gen(seed)
    return torch.randn(S, N, 3, H, D, generator=g), torch.randn(S, N, H * D, generator=g)


def maxrow_qkv(S, N, H, D, seed):
    """q = 1 + {-1/4, 0, 1/4} per channel, k_j = t_j in every channel with t_(N-1) = 128, t_(N-2) = 127.5 and the others spread
    over [0, 120] in steps of 1/2; with scale = 2^-floor(log2 D) a row's scores are a_i t_j, 0.75 <= a_i < 2.5: they span 96 a_i
    > 90, the maximum sits in the last valid column and the runner-up 0.5 a_i below it. All products and sums are multiples of
    1/8 below 2^17: exact in fp32."""
    assert N >= 3
    g = _gen(seed)
    qkv, go = randn_qkv(S, N, H, D, seed)
    qkv[:, :, 0] = 1 + 0.25 * torch.randint(-1, 2, (S, N, H, D), generator=g).float()
    t = torch.empty(N)
    t[N - 1], t[N - 2] = 128.0, 127.5
    for j in range(N - 2):
        t[j] = 0.5 * round(2 * 120.0 * j / max(N - 3, 1))
    qkv[:, :, 1] = t.view(1, N, 1, 1)
    return qkv, go


def k14_input(c):
    N, H, D = c['shape']
    return (maxrow_qkv if c['kind'] == 'maxrow' else randn_qkv)(c['S'], N, H, D, c['seed'])


# ---- K15 / K20b ---------------------------------------------------------------------------------------------------------
K15_D = (4, 8, 32, 36, 64, 68, 128, 132, 200, 256, 260, 512, 516, 832, 1024)          # first and last width of every cell
K20B_D = (2, 3, 31, 32, 33, 64, 65, 100, 128, 129, 256, 257, 400, 512, 513, 1023, 1024)
N_BLOCKS = (1, 8, 9, 56, 57, 64, 65, 121)        # through the finish kernels' loops (1024, capped: the striding cases)
K15_STRIDE_D = (32, 64, 128, 256, 512, 1024)
K20B_STRIDE_D = (31, 52, 100, 200, 400, 1023)


def norm_cases(widths, blocks_D, stride_widths):
    cases = []
    for D in widths:
        rpb = norm_rpb(D)
        for rows in (rpb - 1, rpb + 1, 2 * rpb + rpb // 2 + 1):
            cases.append(dict(rows=rows, D=D, regime='one'))
    for b in N_BLOCKS:
        rows = norm_rpb(blocks_D) * (b - 1) + 5
        if not any(c['rows'] == rows and c['D'] == blocks_D for c in cases):
            cases.append(dict(rows=rows, D=blocks_D, regime='one'))
    for D in stride_widths:
        cases.append(dict(rows=1024 * norm_rpb(D) + norm_rpb(D) + 1, D=D, regime='stride'))
    for i, c in enumerate(cases):
        c['seed'] = 500 + i
        c['offset'] = (1, 2, 3, 0)[i % 4]           # gamma / beta start this many floats into a 16-byte aligned buffer
        c['id'] = 'rows{}-D{}-off{}'.format(c['rows'], c['D'], 4 * c['offset'])
    return cases


K15_CASES = norm_cases(K15_D, 8, K15_STRIDE_D)
K20B_CASES = norm_cases(K20B_D, 7, K20B_STRIDE_D)
K14_CASES = k14_cases()


def norm_input(c, residual):
    """x (and the branch output s of K20b) 2 randn + 0.5, gamma / beta randn (K15) or 1 + 0.1 randn / 0.1 randn (K20b, as
    tests/test_simple_transformer_gpu.py), upstream gradient, the gradient over the residual connection, parameter-gradient seeds"""
    g = _gen(c['seed'])
    rows, D = c['rows'], c['D']
    t = dict(x=torch.randn(rows, D, generator=g) * 2 + 0.5, gy=torch.randn(rows, D, generator=g))
    if residual:
        t['s'] = torch.randn(rows, D, generator=g)
        t['gamma'], t['beta'] = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    else:
        t['gx_add'] = torch.randn(rows, D, generator=g)
        t['gamma'], t['beta'] = torch.randn(D, generator=g), torch.randn(D, generator=g)
    t['seed_gamma'], t['seed_beta'] = torch.randn(D, generator=g), torch.randn(D, generator=g)
    return t


# ======================================================================================================================
# the formulas (any dtype: fp64 is the reference, fp32 on the host sets the per-row bound)
# ======================================================================================================================
def attn_formula(qkv, go, scale, dtype, mask=None, chunk=1024):
    """out = concat_h (softmax(scale q k^T) [* mask]) v and the gradient of qkv for the upstream gradient go; qkv (S, N, 3, heads,
    head_dim), mask (S, heads, N, N) holding 0 or 1 / (1 - p). Returned as doubles."""
    outs, grads = [], []
    for s0 in range(0, qkv.shape[0], chunk):
        x = qkv[s0:s0 + chunk].to(dtype).clone().requires_grad_(True)
        q, k, v = x.permute(2, 0, 3, 1, 4)
        p = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
        if mask is not None:
            p = p * mask[s0:s0 + chunk].to(dtype)
        o = (p @ v).transpose(1, 2).reshape(x.shape[0], x.shape[1], -1)
        o.backward(go[s0:s0 + chunk].to(dtype))
        outs.append(o.detach().double()), grads.append(x.grad.double())
    return torch.cat(outs), torch.cat(grads)


def norm_formula(t, eps, dtype, keep=None):
    """z = LayerNorm(x [+ s keep]) gamma + beta and the gradients of x, s, gamma, beta for the upstream gradient gy (doubles)."""
    x, w, b = (t[n].to(dtype).clone().requires_grad_(True) for n in ('x', 'gamma', 'beta'))
    s = t['s'].to(dtype).clone().requires_grad_(True) if 's' in t else None
    u = x if s is None else x + (s if keep is None else s * keep.to(dtype))
    z = torch.nn.functional.layer_norm(u, (x.shape[1],), w, b, eps)
    z.backward(t['gy'].to(dtype))
    r = dict(z=z.detach().double(), gx=x.grad.double(), g_gamma=w.grad.double(), g_beta=b.grad.double())
    if s is not None:
        r['gs'] = s.grad.double()
    return r


def cancellation_floor(t, eps, keep=None):
    """1e-3 max(rstd |gy gamma|): the three terms of the LayerNorm input gradient are of that size and cancel"""
    u = t['x'].double() if 's' not in t else t['x'].double() + t['s'].double() * (1.0 if keep is None else keep)
    if u.shape[0] == 0:
        return 0.0
    rstd = 1 / (u.var(-1, unbiased=False) + eps).sqrt()
    return 1e-3 * float((rstd.view(-1, 1) * (t['gy'].double() * t['gamma'].double()).abs()).max())


def tensor_ratio(got, ref, floor=0.0):
    """max |got - ref| / max(max |ref|, floor)"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    err, den = float((got - ref).abs().max()), max(float(ref.abs().max()), floor)
    return float('inf') if err != err else (err / den if den > 0 else (0.0 if err == 0 else float('inf')))


def row_ratio(got, ref, floor=0.0):
    """worst row of max_row |got - ref| / max(max_row |ref|, floor); rows = all but the last dimension"""
    got, ref = got.detach().double().cpu(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    err, den = (got - ref).abs().amax(1), ref.abs().amax(1).clamp_min(floor)
    if bool(torch.isnan(err).any()):
        return float('inf')
    ratio = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    return float(ratio.max())


# Per-row criterion: the worst per-row ratio of the formulas evaluated in fp32 on the host against fp64 over ALL cases of the
# family (host_fp32_row_ratios() below), (values, input gradients); the bound is four times it. test_input_conditions measures
# the one-pass cases again and asserts that they stay under half the bound (another host's vector width changes the summation
# order of its fp32 products, not the size of the figure).
ROW_HOST_FP32 = {                                           # worst GPU ratio measured (values, gradients)
    'narrow-4': (3.153e-06, 4.037e-06),                     # 5.04e-06, 3.42e-06
    'narrow-8': (2.065e-06, 2.670e-06),                     # 1.75e-06, 2.67e-06
    'wide': (9.601e-07, 1.800e-06),                         # 1.09e-06, 1.47e-06
    'generic-vector': (1.225e-06, 1.184e-06),               # 9.11e-07, 2.30e-06
    'generic-scalar': (1.151e-06, 2.413e-06),               # 1.33e-06, 2.91e-06
    'narrow-4/maxrow': (1.325e-07, 1.942e-04),              # 8.72e-08, 1.94e-04
    'narrow-8/maxrow': (9.119e-08, 1.196e-04),              # 9.54e-08, 9.30e-05
    'wide/maxrow': (1.129e-07, 6.673e-05),                  # 1.14e-07, 1.26e-04
    'generic-vector/maxrow': (1.011e-07, 2.831e-04),        # 1.05e-07, 2.97e-04
    'generic-scalar/maxrow': (1.208e-07, 1.803e-04),        # 1.72e-07, 1.49e-04
    'k20a': (5.256e-07, 5.258e-07),                         # 4.52e-07, 6.09e-07
    'k20a/maxrow': (1.130e-07, 2.472e-04),                  # 1.17e-07, 2.47e-04
    'k20a/dropout': (7.833e-07, 1.148e-06),                 # 6.98e-07, 1.09e-06
    'k15': (5.530e-07, 2.408e-06),                          # 5.28e-07, 1.09e-06
    'k20b': (3.177e-07, 1.464e-06),                         # 2.62e-07, 8.74e-07
    'k20b/D<4': (2.372e-05, 2.471e-03),                     # 1.53e-07, 1.15e-05
    'k20b/dropout': (3.015e-07, 3.309e-07),                 # 2.28e-07, 2.68e-07
}
ROW_BOUND = {k: (4 * v, 4 * g) for k, (v, g) in ROW_HOST_FP32.items()}


def bound_key(fam, c):
    """the unit-scale cases are not judged by the figure of the row-maximum inputs (whose gradient rows cancel to 1e-4 of their
    terms in fp32 as well), nor the post-norm widths >= 4 by that of D = 2 and 3 (where the normalised row is +-1 and the input
    gradient cancels almost completely)"""
    if c.get('kind') == 'maxrow':
        return fam + '/maxrow'
    return fam + '/D<4' if fam == 'k20b' and c['D'] < 4 else fam


def host_fp32_row_ratios(regimes=('one', 'stride', 'stride2')):
    """{family: [worst value ratio, worst gradient ratio]} of the formulas evaluated in fp32 on the host against fp64"""
    worst = {}

    def note(fam, v, g):
        w = worst.setdefault(fam, [0.0, 0.0])
        w[0], w[1] = max(w[0], v), max(w[1], g)
    for c in K14_CASES:
        if c['regime'] in regimes:
            qkv, go = k14_input(c)
            (o64, g64), (o32, g32) = (attn_formula(qkv, go, c['scale'], dt) for dt in (torch.float64, torch.float32))
            note(bound_key(c['family'], c), row_ratio(o32, o64), row_ratio(g32.flatten(2), g64.flatten(2)))
    for c in K20A_CASES:
        qkv, go = k20a_input(c)
        scale = _f32(c['scale'])
        (o64, g64), (o32, g32) = (attn_formula(qkv, go, scale, dt) for dt in (torch.float64, torch.float32))
        note(bound_key('k20a', c), row_ratio(o32, o64), row_ratio(g32.flatten(2), g64.flatten(2)))
    for fam, cases, residual, eps in (('k15', K15_CASES, False, EPS15), ('k20b', K20B_CASES, True, EPS20)):
        for c in cases:
            if c['regime'] in regimes and c['rows'] > 0:
                t = norm_input(c, residual)
                r64, r32 = norm_formula(t, eps, torch.float64), norm_formula(t, eps, torch.float32)
                floor = cancellation_floor(t, eps)
                note(bound_key(fam, c), row_ratio(r32['z'], r64['z']), max(row_ratio(r32[n], r64[n], floor) for n in ('gx', 'gs') if n in r64))
    for p in (0.1, 0.5):           # dropout: host-drawn Bernoulli masks of the same rate stand in for the kernels' (same shapes)
        for S, N, H, D in K20A_DROP:
            qkv, go = randn_qkv(S, N, H, D, 940 + N)
            mask = (torch.rand(S, H, N, N, generator=_gen(N), dtype=torch.float64) >= p).double() / (1 - p)
            (o64, g64), (o32, g32) = (attn_formula(qkv, go, _f32(D ** -0.5), dt, mask=mask) for dt in (torch.float64, torch.float32))
            note('k20a/dropout', row_ratio(o32, o64), row_ratio(g32.flatten(2), g64.flatten(2)))
        for rows, D in K20B_DROP:
            if rows * D < 10 ** 5 or 'stride' in regimes:
                t = norm_input(dict(rows=rows, D=D, seed=960 + D), residual=True)
                keep = (torch.rand(rows, D, generator=_gen(D), dtype=torch.float64) >= p).double() / (1 - p)
                r64, r32 = norm_formula(t, EPS20, torch.float64, keep), norm_formula(t, EPS20, torch.float32, keep)
                floor = cancellation_floor(t, EPS20, keep)
                note('k20b/dropout', row_ratio(r32['z'], r64['z']), max(row_ratio(r32[n], r64[n], floor) for n in ('gx', 'gs')))
    return worst


EPS15, EPS20 = _f32(1e-6), _f32(1e-5)

# ---- K20a: no striding (one workgroup per (sequence, head)); head widths that are no multiple of 4, every N edge ---------------
K20A_CASES = [dict(S=3, N=K20A_MAXROW[0], heads=K20A_MAXROW[1], hd=K20A_MAXROW[2], kind='maxrow', scale=maxrow_scale(K20A_MAXROW[2]), seed=900),
              dict(S=3, N=17, heads=3, hd=7, kind='randn', scale=0.37, seed=901),
              dict(S=700, N=5, heads=4, hd=13, kind='randn', scale=13 ** -0.5, seed=902)]
for _c in K20A_CASES:
    _c['id'] = 'N{N}-h{heads}-d{hd}-S{S}-{kind}'.format(**_c)


def k20a_input(c):
    return (maxrow_qkv if c['kind'] == 'maxrow' else randn_qkv)(c['S'], c['N'], c['heads'], c['hd'], c['seed'])


# K20 with dropout: (S, N, heads, head_dim >= N) -- v = the first N columns of an identity returns P' itself
K20A_DROP = [(3, 7, 2, 8), (600, 16, 4, 16), (2, 64, 2, 64), (3, 33, 3, 40)]
K20B_DROP = [(37, 33), (1024 * 16 + 16 + 1, 52)]                 # (rows, D): one pass; striding


# ======================================================================================================================
# refusal tables: entry point -> argument order of the C ABI, a small valid call, which pointers may not be NULL
# ======================================================================================================================
ENTRY = {
    'p2c_attn_small_fwd': dict(args=('qkv', 'out', 'scale', 'S', 'N', 'heads', 'hd'), need=('qkv', 'out'), align=('qkv', 'out'),
                               base=dict(scale=0.5, S=2, N=5, heads=1, hd=4)),
    'p2c_attn_small_bwd': dict(args=('qkv', 'g_out', 'g_qkv', 'scale', 'S', 'N', 'heads', 'hd'), need=('qkv', 'g_out', 'g_qkv'),
                               align=('qkv', 'g_out', 'g_qkv'), base=dict(scale=0.5, S=2, N=5, heads=1, hd=4)),
    'p2c_layernorm_fwd': dict(args=('x', 'gamma', 'beta', 'y', 'mean', 'rstd', 'rows', 'D', 'eps'),
                              need=('x', 'gamma', 'beta', 'y', 'mean', 'rstd'), align=('x', 'y'), base=dict(rows=5, D=8, eps=1e-6)),
    'p2c_layernorm_bwd': dict(args=('x', 'gamma', 'mean', 'rstd', 'gy', 'gx_add', 'gx', 'g_gamma', 'g_beta', 'accumulate', 'partials',
                                    'rows', 'D'),
                              need=('x', 'gamma', 'mean', 'rstd', 'gy', 'gx', 'g_gamma', 'g_beta', 'partials'),
                              align=('x', 'gy', 'gx', 'gx_add'), base=dict(accumulate=0, rows=5, D=8)),
    'p2c_attn_drop_fwd': dict(args=('qkv', 'out', 'scale', 'S', 'N', 'heads', 'hd', 'drop_state', 'drop_p', 'drop_site'),
                              need=('qkv', 'out'), align=(), base=dict(scale=0.5, S=2, N=5, heads=2, hd=3, drop_p=0.0, drop_site=0)),
    'p2c_attn_drop_bwd': dict(args=('qkv', 'g_out', 'g_qkv', 'scale', 'S', 'N', 'heads', 'hd', 'drop_state', 'drop_p', 'drop_site'),
                              need=('qkv', 'g_out', 'g_qkv'), align=(),
                              base=dict(scale=0.5, S=2, N=5, heads=2, hd=3, drop_p=0.0, drop_site=0)),
    'p2c_postnorm_fwd': dict(args=('x', 's', 'gamma', 'beta', 'z', 'mean', 'rstd', 'rows', 'D', 'eps', 'drop_state', 'drop_p', 'drop_site'),
                             need=('x', 's', 'gamma', 'beta', 'z', 'mean', 'rstd'), align=(),
                             base=dict(rows=5, D=7, eps=1e-5, drop_p=0.0, drop_site=0)),
    'p2c_postnorm_bwd': dict(args=('x', 's', 'gamma', 'mean', 'rstd', 'g_z', 'g_x', 'g_s', 'g_gamma', 'g_beta', 'accumulate', 'workspace',
                                   'rows', 'D', 'drop_state', 'drop_p', 'drop_site'),
                             need=('x', 's', 'gamma', 'mean', 'rstd', 'g_z', 'g_x', 'g_s', 'g_gamma', 'g_beta', 'workspace'), align=(),
                             base=dict(accumulate=0, rows=5, D=7, drop_p=0.0, drop_site=0)),
}
POINTERS = {'qkv', 'out', 'g_out', 'g_qkv', 'x', 's', 'gamma', 'beta', 'y', 'z', 'mean', 'rstd', 'gy', 'g_z', 'gx_add', 'gx', 'g_x', 'g_s',
            'g_gamma', 'g_beta', 'partials', 'workspace', 'drop_state'}
K14_OVER_FWD, K14_OVER_BWD, K14_UNDER = (64, 1, 188), (64, 1, 124), (64, 1, 120)      # LDS bytes: 161 792 | 161 792 | 157 696 (bwd)
_K14_SHAPES = [('S<0', dict(S=-1)), ('N=0', dict(N=0)), ('N=65', dict(N=65)), ('heads=0', dict(heads=0)), ('hd=0', dict(hd=0)),
               ('heads*hd%4', dict(heads=3, hd=3))]
_K20A_SHAPES = [('N=0', dict(N=0)), ('N=65', dict(N=65)), ('heads*hd=257', dict(heads=1, hd=257)), ('S<0', dict(S=-1)),
                ('S*heads>2^31-1', dict(S=1 << 30, heads=4, hd=4))]
_DROP_P = [('p<0', dict(drop_p=-0.1, drop_state='drop_state')), ('p=1', dict(drop_p=1.0, drop_state='drop_state')),
           ('p=nan', dict(drop_p=float('nan'), drop_state='drop_state')), ('p=nan,no state', dict(drop_p=float('nan')))]
SHAPE_REFUSALS = {
    'p2c_attn_small_fwd': _K14_SHAPES + [('lds', dict(zip(('N', 'heads', 'hd'), K14_OVER_FWD)))],
    'p2c_attn_small_bwd': _K14_SHAPES + [('lds', dict(zip(('N', 'heads', 'hd'), K14_OVER_BWD)))],
    'p2c_layernorm_fwd': [('D=%d' % D, dict(D=D)) for D in (0, 2, 6, 1028)] + [('rows<0', dict(rows=-1))],
    'p2c_layernorm_bwd': [('D=%d' % D, dict(D=D)) for D in (0, 2, 6, 1028)] + [('rows<0', dict(rows=-1))],
    'p2c_attn_drop_fwd': _K20A_SHAPES + _DROP_P,
    'p2c_attn_drop_bwd': _K20A_SHAPES + _DROP_P,
    'p2c_postnorm_fwd': [('D=1', dict(D=1)), ('D=1025', dict(D=1025)), ('rows<0', dict(rows=-1))] + _DROP_P,
    'p2c_postnorm_bwd': [('D=1', dict(D=1)), ('D=1025', dict(D=1025)), ('rows<0', dict(rows=-1))] + _DROP_P,
}


def refusals(name):
    """[(label, overrides, expected code)]: NULL for each required pointer, every refused shape, each 16-byte-aligned pointer
    4 bytes off ('+4': the arena's address plus 4)"""
    e = ENTRY[name]
    table = [('NULL ' + p, {p: None}, E_NULL) for p in e['need']]
    table += [(label, over, E_SHAPE) for label, over in SHAPE_REFUSALS[name]]
    table += [('misaligned ' + p, {p: '+4'}, E_SHAPE) for p in e['align']]
    return table


# ======================================================================================================================
# what the GPU tests rely on, without a GPU
# ======================================================================================================================
def test_dispatch_mirrors_and_case_coverage():
    # the mirrors against cells computed by hand from the dispatch code
    assert k14_cell(26, 4) == ('narrow-4', 32) and k14_cell(9, 104) == ('wide', 16) and k14_cell(17, 104) == ('generic-vector', 32)
    assert k14_cell(16, 8) == ('narrow-8', 16) and k14_cell(16, 13) == ('generic-scalar', 16) and k14_cell(33, 6) == ('generic-scalar', 64)
    assert k14_cell(16, 12) == ('wide', 16) and k14_cell(17, 12) == ('generic-vector', 32) and k14_cell(64, 4) == ('narrow-4', 64)
    assert (k14_lds(26, 8, 4, False), k14_lds(26, 8, 4, True)) == (32032, 57408)          # 4 (26 * 100 + 8 * 676) | 4 (26 * 136 + 2 * 8 * 676)
    assert (k14_grid(10 ** 6, 26, 8, 4, False), k14_grid(10 ** 6, 26, 8, 4, True)) == (4096, 2048)
    assert (k14_lds(9, 8, 104, False), k14_lds(9, 8, 104, True)) == (92592, 125280)
    assert k14_grid(21024, 9, 8, 104, False) == k14_grid(21024, 9, 8, 104, True) == 1024 and k14_grid(7, 9, 8, 104, True) == 7
    assert k14_grid(10 ** 6, 5, 1, 4, True) == 8192                                       # per_cu capped at 8
    assert k14_supported(*K14_UNDER) and not k14_supported(*K14_OVER_BWD) and k14_supported(*K14_OVER_BWD, bwd=False)
    assert not k14_supported(*K14_OVER_FWD, bwd=False) and not k14_supported(64, 5, 4) and k14_supported(64, 4, 4)
    assert k14_lds(*K14_UNDER, True) == 157696 and k14_lds(*K14_OVER_BWD, True) == 161792 and k14_lds(*K14_OVER_FWD, False) == 161792
    assert [k15_cell(D) for D in (4, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024)] == [c for c in K15_CELLS for _ in (0, 1)]
    assert [k20b_cell(D) for D in (2, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024)] == [c for c in K20B_CELLS for _ in (0, 1)]
    assert [norm_rpb(D) for D in (2, 32, 33, 64, 65, 128, 129, 1024)] == [32, 32, 16, 16, 8, 8, 4, 4]
    assert norm_blocks(0, 8) == 1 and norm_blocks(32, 8) == 1 and norm_blocks(33, 8) == 2 and norm_blocks(4101, 1024) == 1024
    assert not norm_strides(4096, 1024) and norm_strides(4097, 1024) and not norm_strides(32768, 32) and norm_strides(32769, 32)

    # K14: every reachable cell one-pass and striding; striding means S above BOTH grids
    assert len(set(K14_CELLS)) == 12
    ids = [c['id'] for c in K14_CASES]
    assert len(set(ids)) == len(ids), 'duplicate K14 case'
    for c in K14_CASES:
        N, H, D = c['shape']
        assert k14_supported(N, H, D), c['id']
        fwd, bwd = k14_grid(c['S'], N, H, D, False), k14_grid(c['S'], N, H, D, True)
        if c['regime'] == 'one':
            assert fwd == bwd == c['S'], c['id']
        else:
            assert c['S'] > fwd >= bwd and c['S'] < (2 if c['regime'] == 'stride' else 3) * fwd, c['id']
    for fam, shapes in K14_ONE_PASS.items():
        assert all(k14_family(N, D) == fam for N, _, D in shapes), fam
    for cell in K14_CELLS:
        here = [c for c in K14_CASES if k14_cell(c['shape'][0], c['shape'][2]) == cell]
        assert any(c['regime'] == 'one' for c in here) and any(c['regime'] != 'one' for c in here), cell
    for fam in K14_ONE_PASS:
        here = [c for c in K14_CASES if c['family'] == fam]
        assert any(c['kind'] == 'maxrow' for c in here), fam
        assert any(c['kind'] == 'randn' and c['scale'] != _f32(c['shape'][2] ** -0.5) for c in here), fam
        assert any(c['regime'] != 'one' for c in here), fam
    assert sum(c['regime'] == 'stride2' for c in K14_CASES) == 2
    assert any(c['shape'][1] > 4 for c in K14_CASES if c['family'] == 'wide')                    # heads dealt to four waves twice
    assert all(any(c['shape'][0] * c['shape'][1] > 256 for c in K14_CASES if c['family'] == f) for f in ('narrow-4', 'narrow-8'))
    assert {c['shape'][0] for c in K14_CASES} >= {1, 16, 17, 32, 33, 64}
    assert {c['shape'][2] for c in K14_CASES if c['family'] == 'wide'} >= {12, 20, 24, 36, 104, 136}

    # the norms: every cell at its first and last width, rows around rows-per-workgroup, every finish-loop count, a striding case
    for cases, cell_of, cells, widths in ((K15_CASES, k15_cell, K15_CELLS, K15_D), (K20B_CASES, k20b_cell, K20B_CELLS, K20B_D)):
        ids = [c['id'].rsplit('-', 1)[0] for c in cases]
        assert len(set(ids)) == len(ids), 'duplicate norm case'
        assert {c['D'] for c in cases} >= set(widths)
        for cell in cells:
            here = [c for c in cases if cell_of(c['D']) == cell]
            assert any(c['regime'] == 'one' for c in here) and any(c['regime'] == 'stride' for c in here), cell
            assert {c['offset'] for c in here} == {0, 1, 2, 3}, cell
            for c in here:
                assert norm_strides(c['rows'], c['D']) == (c['regime'] == 'stride'), c['id']
                if c['regime'] == 'stride':
                    assert norm_blocks(c['rows'], c['D']) == 1024 and c['rows'] % norm_rpb(c['D']) == 1, c['id']
        for D in widths:
            rpb = norm_rpb(D)
            rows = {c['rows'] for c in cases if c['D'] == D}
            assert rpb - 1 in rows and rpb + 1 in rows and any(r % rpb and r > rpb + 1 for r in rows), D
        assert {norm_blocks(c['rows'], c['D']) for c in cases} >= set(N_BLOCKS) | {1024}
    assert max(c['rows'] * c['D'] for c in K15_CASES) == 4101 * 1024

    # K20 with dropout, and the refusal tables
    assert all(hd >= N and heads * hd <= 256 for _, N, heads, hd in K20A_DROP) and {N for _, N, _, _ in K20A_DROP} >= {33, 64}
    assert [norm_strides(r, D) for r, D in K20B_DROP] == [False, True]
    for name, e in ENTRY.items():
        table = refusals(name)
        assert {o for _, over, _ in table for o in over} <= set(e['args']), name
        assert [lab for lab, _, _ in table if lab.startswith('NULL')] == ['NULL ' + p for p in e['need']], name
        assert set(e['need']) | set(e['align']) <= POINTERS and len({lab for lab, _, _ in table}) == len(table), name
    assert {p for p in ENTRY['p2c_attn_small_fwd']['align']} == {'qkv', 'out'}
    assert {p for p in ENTRY['p2c_attn_small_bwd']['align']} == {'qkv', 'g_out', 'g_qkv'}


def test_input_conditions():
    # the row-maximum inputs: exact in fp32, span > 90 in every row, maximum in the last valid column, finite, not one-hot
    for c in [c for c in K14_CASES if c['kind'] == 'maxrow'] + [dict(shape=(c['N'], c['heads'], c['hd']), **c) for c in K20A_CASES
                                                                 if c['kind'] == 'maxrow']:
        N, H, D = c['shape']
        qkv, go = maxrow_qkv(c['S'], N, H, D, c['seed'])
        scale = _f32(c['scale'])
        assert scale == c['scale'] and math.log2(scale) == int(math.log2(scale)), c['id']
        q, k = qkv[:, :, 0].permute(0, 2, 1, 3), qkv[:, :, 1].permute(0, 2, 1, 3)
        s64 = q.double() @ k.double().transpose(-1, -2) * scale
        assert torch.equal((q @ k.transpose(-1, -2) * scale).double(), s64), c['id']          # fp32 scores are exact
        assert float((s64.amax(-1) - s64.amin(-1)).min()) > 90 and float(s64.max()) > 89, c['id']   # exp(max) overflows fp32
        assert bool((s64.argmax(-1) == N - 1).all()), c['id']
        p = torch.softmax(s64, -1)
        assert bool(((p > 1e-3).sum(-1) >= 2).all()) and float(p.amax(-1).max()) < 0.8, c['id']    # argmax alone does not pass
        out, grad = attn_formula(qkv, go, scale, torch.float64)
        assert bool(torch.isfinite(p).all() and torch.isfinite(out).all() and torch.isfinite(grad).all()), c['id']
        # a one-hot output would differ from the reference by far more than the bound
        onehot = qkv[:, N - 1:N, 2].double().reshape(c['S'], 1, H * D).expand(-1, N, -1)
        assert tensor_ratio(onehot, out) > 0.05, c['id']
    # unit scale everywhere else
    for c in K14_CASES:
        if c['kind'] == 'randn' and c['regime'] == 'one':
            qkv, _ = k14_input(c)
            assert float(qkv.abs().max()) < 6, c['id']
    # every bound is four times a measured host figure; the one-pass cases measured again here stay under half of it
    worst = host_fp32_row_ratios(regimes=('one',))
    assert set(worst) == set(ROW_BOUND)
    for fam, (bv, bg) in ROW_BOUND.items():
        assert worst[fam][0] <= bv / 2 and worst[fam][1] <= bg / 2, (fam, worst[fam], (bv, bg))


# ======================================================================================================================
# GPU
# ======================================================================================================================
def _dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _lib():
    from pedestrians_video_2_carla_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _report(what, figures):
    print(what, ' '.join('{}={:.3e}'.format(k, v) for k, v in figures.items()))


def k14_call(qkv, go, scale, S, N, H, D):
    out, gq = torch.empty(S, N, H * D, device=qkv.device), torch.empty_like(qkv)
    assert _lib().p2c_attn_small_fwd(qkv.data_ptr(), out.data_ptr(), scale, S, N, H, D, _stream()) == 0
    assert _lib().p2c_attn_small_bwd(qkv.data_ptr(), go.data_ptr(), gq.data_ptr(), scale, S, N, H, D, _stream()) == 0
    return out, gq


def k20a_call(qkv, go, scale, S, N, H, D, st=None, p=0.0, site=0, backward=True):
    out, gq = torch.empty(S, N, H * D, device=qkv.device), torch.empty_like(qkv)
    assert _lib().p2c_attn_drop_fwd(qkv.data_ptr(), out.data_ptr(), scale, S, N, H, D, _ptr(st), p, site, _stream()) == 0
    if backward:
        assert _lib().p2c_attn_drop_bwd(qkv.data_ptr(), go.data_ptr(), gq.data_ptr(), scale, S, N, H, D, _ptr(st), p, site, _stream()) == 0
    return out, gq


def _check_attention(fam, c, out, gq, ref_out, ref_grad, tensor_bound):
    what, fam = c['id'], bound_key(fam, c)
    figs = dict(out=tensor_ratio(out, ref_out), grad=tensor_ratio(gq, ref_grad), out_row=row_ratio(out, ref_out),
                grad_row=row_ratio(gq.flatten(2), ref_grad.flatten(2)))
    _report('{} {}'.format(fam, what), figs)
    assert figs['out'] <= tensor_bound and figs['grad'] <= tensor_bound, (what, figs)
    assert figs['out_row'] <= ROW_BOUND[fam][0] and figs['grad_row'] <= ROW_BOUND[fam][1], (what, figs, ROW_BOUND[fam])


@pytest.mark.gpu
@pytest.mark.parametrize('c', K14_CASES, ids=[c['id'] for c in K14_CASES])
def test_k14_every_cell_matches_fp64(c):
    """p2c_attn_small_fwd/_bwd in all twelve (family, row width) cells, one pass and striding over sequences (S = grid + 3 and
    2 grid + 1), unit-scale and row-maximum inputs, head_dim ** -0.5 and another scale: out and g_qkv within 1e-5 of the fp64 formula
    per tensor and within ROW_BOUND per (sequence, token) row; two calls give the same bits."""
    d = _dev()
    (N, H, D), S = c['shape'], c['S']
    assert bool(_lib().p2c_attn_small_supported(N, H, D))
    qkv, go = k14_input(c)
    ref_out, ref_grad = attn_formula(qkv, go, c['scale'], torch.float64)
    q, g = qkv.to(d), go.to(d)
    out, gq = k14_call(q, g, c['scale'], S, N, H, D)
    out2, gq2 = k14_call(q, g, c['scale'], S, N, H, D)
    assert torch.equal(out, out2) and torch.equal(gq, gq2), 'repeated calls differ'
    _check_attention(c['family'], c, out, gq, ref_out, ref_grad, 1e-5)


@pytest.mark.gpu
@pytest.mark.parametrize('c', K20A_CASES, ids=[c['id'] for c in K20A_CASES])
def test_k20a_without_dropout_matches_fp64(c):
    """p2c_attn_drop_fwd/_bwd with drop_p = 0: the row-maximum input, a scale other than head_dim ** -0.5, 2 800 workgroups."""
    d = _dev()
    S, N, H, D, scale = c['S'], c['N'], c['heads'], c['hd'], _f32(c['scale'])
    qkv, go = k20a_input(c)
    ref_out, ref_grad = attn_formula(qkv, go, scale, torch.float64)
    q, g = qkv.to(d), go.to(d)
    out, gq = k20a_call(q, g, scale, S, N, H, D)
    out2, gq2 = k20a_call(q, g, scale, S, N, H, D)
    assert torch.equal(out, out2) and torch.equal(gq, gq2), 'repeated calls differ'
    _check_attention('k20a', c, out, gq, ref_out, ref_grad, 1e-4)


# ---- the norms ----------------------------------------------------------------------------------------------------------------
def _params(t, offset, d):
    """gamma | beta as views `offset` floats into one 16-byte aligned buffer, as the flat parameter buffer hands them out"""
    D = t['gamma'].numel()
    flat = torch.zeros(2 * D + 4, device=d)
    gamma, beta = flat[offset:offset + D], flat[offset + D:offset + 2 * D]
    gamma.copy_(t['gamma']), beta.copy_(t['beta'])
    assert flat.data_ptr() % 16 == 0 and gamma.data_ptr() % 16 == (4 * offset) % 16
    return flat, gamma, beta


def _check_norm(fam, c, got, ref, floor, bounds, seeded):
    key = c.get('bound') or bound_key(fam, c)
    figs, limit = {}, {}
    for name, bound in bounds.items():
        want = ref[name] + seeded.get(name, 0.0)
        fl = floor if name in ('gx', 'gs') else 0.0
        figs[name], limit[name] = tensor_ratio(got[name], want, fl if fam == 'k20b' else 0.0), bound
        if name in ('z', 'gx', 'gs'):
            figs[name + '_row'], limit[name + '_row'] = row_ratio(got[name], want, fl), ROW_BOUND[key][0 if name == 'z' else 1]
    _report('{} {}'.format(fam, c['id']), figs)
    for name in figs:
        assert figs[name] <= limit[name], (c['id'], name, figs[name], limit[name])


def k15_run(c, t, dv, gamma, beta, accumulate, with_add):
    lib, rows, D = _lib(), c['rows'], c['D']
    d = dv['x'].device
    y, mean, rstd, gx = torch.empty_like(dv['x']), torch.empty(rows, device=d), torch.empty(rows, device=d), torch.empty_like(dv['x'])
    assert lib.p2c_layernorm_fwd(dv['x'].data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                 rows, D, EPS15, _stream()) == 0
    gg, gb = (dv['seed_gamma'].clone(), dv['seed_beta'].clone()) if accumulate else (torch.empty(D, device=d), torch.empty(D, device=d))
    floats = lib.p2c_layernorm_workspace_floats(rows, D)
    assert floats == norm_blocks(rows, D) * 2 * D
    ws = torch.empty(floats, device=d)
    assert lib.p2c_layernorm_bwd(dv['x'].data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dv['gy'].data_ptr(),
                                 _ptr(dv['gx_add'] if with_add else None), gx.data_ptr(), gg.data_ptr(), gb.data_ptr(), accumulate,
                                 ws.data_ptr(), rows, D, _stream()) == 0
    return dict(z=y, gx=gx, g_gamma=gg, g_beta=gb)


@pytest.mark.gpu
@pytest.mark.parametrize('c', K15_CASES, ids=[c['id'] for c in K15_CASES])
def test_k15_every_cell_matches_fp64(c):
    """p2c_layernorm_fwd/_bwd at the first and last width of every (G, KV) instantiation, rows around rows-per-workgroup, every
    workgroup count the finish kernel's loops distinguish, striding over rows, gamma / beta 0, 4, 8 and 12 bytes off 16-byte
    alignment; backward written (accumulate 0, no gx_add) and added into seeds with the residual gradient (accumulate 1, gx_add)."""
    d = _dev()
    t = norm_input(c, residual=False)
    ref = norm_formula(t, EPS15, torch.float64)
    floor = cancellation_floor(t, EPS15)
    dv = {k: v.to(d) for k, v in t.items()}
    _, gamma, beta = _params(t, c['offset'], d)
    sq = max(1.0, c['rows'] ** 0.5)
    bounds = dict(z=2e-5, gx=5e-5, g_gamma=5e-5 * sq, g_beta=5e-5 * sq)
    for accumulate, with_add in ((0, False), (1, True)):
        got = k15_run(c, t, dv, gamma, beta, accumulate, with_add)
        again = k15_run(c, t, dv, gamma, beta, accumulate, with_add)
        assert all(torch.equal(got[k], again[k]) for k in got), 'repeated calls differ'
        seeded = {}
        if accumulate:
            seeded = dict(g_gamma=t['seed_gamma'].double(), g_beta=t['seed_beta'].double())
        if with_add:
            seeded['gx'] = t['gx_add'].double()
        _check_norm('k15', c, got, ref, floor, bounds, seeded)


def k20b_run(c, dv, gamma, beta, accumulate, st=None, p=0.0, site=1):
    lib, rows, D = _lib(), c['rows'], c['D']
    d = dv['x'].device
    z, mean, rstd = torch.empty_like(dv['x']), torch.empty(rows, device=d), torch.empty(rows, device=d)
    assert lib.p2c_postnorm_fwd(dv['x'].data_ptr(), dv['s'].data_ptr(), gamma.data_ptr(), beta.data_ptr(), z.data_ptr(), mean.data_ptr(),
                                rstd.data_ptr(), rows, D, EPS20, _ptr(st), p, site, _stream()) == 0
    gx, gs = torch.empty_like(z), torch.empty_like(z)
    gg, gb = (dv['seed_gamma'].clone(), dv['seed_beta'].clone()) if accumulate else (torch.empty(D, device=d), torch.empty(D, device=d))
    floats = lib.p2c_postnorm_workspace_floats(rows, D)
    assert floats == norm_blocks(rows, D) * 2 * D
    ws = torch.empty(floats, device=d)
    assert lib.p2c_postnorm_bwd(dv['x'].data_ptr(), dv['s'].data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                dv['gy'].data_ptr(), gx.data_ptr(), gs.data_ptr(), gg.data_ptr(), gb.data_ptr(), accumulate, ws.data_ptr(),
                                rows, D, _ptr(st), p, site, _stream()) == 0
    return dict(z=z, gx=gx, gs=gs, g_gamma=gg, g_beta=gb)


K20B_BOUNDS = dict(z=1e-4, gx=1e-4, gs=1e-4, g_gamma=1e-4, g_beta=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize('c', K20B_CASES, ids=[c['id'] for c in K20B_CASES])
def test_k20b_every_cell_matches_fp64(c):
    """p2c_postnorm_fwd/_bwd with drop_p = 0 at the first and last width of every (G, KV) instantiation (odd widths too), rows
    around rows-per-workgroup, the finish kernel's workgroup counts, striding over rows; accumulate 0 and 1.

    D = 2 is where u - mean cancels: rows81-D2 holds a row with x1 + s1 within 5e-3 of x2 + s2, which a kernel that rounds u
    and the row mean to fp32 gets wrong by 3e-4 of the cancellation floor in dx / ds (bound 1e-4) and by 2e-5 in z."""
    d = _dev()
    t = norm_input(c, residual=True)
    ref = norm_formula(t, EPS20, torch.float64)
    floor = cancellation_floor(t, EPS20)
    dv = {k: v.to(d) for k, v in t.items()}
    _, gamma, beta = _params(t, c['offset'], d)
    for accumulate in (0, 1):
        got = k20b_run(c, dv, gamma, beta, accumulate)
        again = k20b_run(c, dv, gamma, beta, accumulate)
        assert all(torch.equal(got[k], again[k]) for k in got), 'repeated calls differ'
        seeded = dict(g_gamma=t['seed_gamma'].double(), g_beta=t['seed_beta'].double()) if accumulate else {}
        _check_norm('k20b', c, got, ref, floor, K20B_BOUNDS, seeded)


@pytest.mark.gpu
@pytest.mark.parametrize('kernel,D', [('k15', 8), ('k15', 260), ('k20b', 7), ('k20b', 300)])
def test_norms_with_no_rows(kernel, D):
    """rows = 0: the forward writes nothing; the backward writes zero parameter gradients (accumulate 0) or leaves the seeds
    (accumulate 1), and nothing else."""
    d = _dev()
    lib = _lib()
    buf = {n: torch.full((4 * D,), SENTINEL, device=d) for n in ('x', 's', 'gamma', 'beta', 'y', 'mean', 'rstd', 'gy', 'gx', 'gs', 'ws')}
    p = {n: b.data_ptr() for n, b in buf.items()}
    if kernel == 'k15':
        assert lib.p2c_layernorm_workspace_floats(0, D) == 2 * D
        assert lib.p2c_layernorm_fwd(p['x'], p['gamma'], p['beta'], p['y'], p['mean'], p['rstd'], 0, D, EPS15, _stream()) == 0
    else:
        assert lib.p2c_postnorm_workspace_floats(0, D) == 2 * D
        assert lib.p2c_postnorm_fwd(p['x'], p['s'], p['gamma'], p['beta'], p['y'], p['mean'], p['rstd'], 0, D, EPS20, None, 0.0, 0, _stream()) == 0
    for accumulate in (0, 1):
        gg, gb = torch.full((D + 3,), 2.5, device=d), torch.full((D + 3,), -1.5, device=d)
        if kernel == 'k15':
            rc = lib.p2c_layernorm_bwd(p['x'], p['gamma'], p['mean'], p['rstd'], p['gy'], None, p['gx'], gg.data_ptr(), gb.data_ptr(),
                                       accumulate, p['ws'], 0, D, _stream())
        else:
            rc = lib.p2c_postnorm_bwd(p['x'], p['s'], p['gamma'], p['mean'], p['rstd'], p['gy'], p['gx'], p['gs'], gg.data_ptr(),
                                      gb.data_ptr(), accumulate, p['ws'], 0, D, None, 0.0, 0, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        want_g, want_b = (2.5, -1.5) if accumulate else (0.0, 0.0)
        assert bool((gg[:D] == want_g).all() and (gb[:D] == want_b).all()), (accumulate, gg, gb)
        assert bool((gg[D:] == 2.5).all() and (gb[D:] == -1.5).all())
    assert all(bool((b == SENTINEL).all()) for n, b in buf.items() if n != 'ws'), 'a call without rows wrote something'


# ---- K20 with dropout ---------------------------------------------------------------------------------------------------------
def _snap_mask(values, p, what):
    """recovered keep factors: nothing but 0 and 1 / (1 - p) (to 1e-4); returned snapped to those two numbers, in fp64"""
    values = values.double().cpu()
    kept = values > 0.5
    assert bool(((values[kept] * (1 - p) - 1).abs() < 1e-4).all()) and bool((values[~kept].abs() < 1e-6).all()), what
    return kept.double() * float(1 / (1 - torch.tensor(p, dtype=torch.float32)))           # (the kernels' fp32 1 / (1 - p))


def _keep_fraction_ok(mask, p):
    """|kept fraction - (1 - p)| < 0.01 (tests/test_simple_transformer_gpu.py), or five standard deviations where the mask is too
    small for that"""
    n = mask.numel()
    return abs(float((mask != 0).double().mean()) - (1 - p)) < max(0.01, 5 * math.sqrt(p * (1 - p) / n))


def _k20a_read_mask(st, S, N, H, D, p, site):
    """(S, heads, N, N) keep factors of the stream position in ``st``, read off a forward: q = k = 0 gives P = 1 / N, v = the
    first N columns of an identity returns P' itself. The state is put back."""
    snap = st.clone()
    qkv = torch.zeros(S, N, 3, H, D, device=st.device)
    qkv[:, :, 2] = torch.eye(N, D, device=st.device).view(1, N, 1, D)
    out, _ = k20a_call(qkv, None, 1.0, S, N, H, D, st, p, site, backward=False)
    st.copy_(snap)
    return (out.view(S, N, H, D)[..., :N].permute(0, 2, 1, 3) * N)          # [s][h][i][j]


@pytest.mark.gpu
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('S,N,H,D', K20A_DROP, ids=['S{}-N{}-h{}-d{}'.format(*s) for s in K20A_DROP])
def test_k20a_dropout_matches_fp64_with_the_kernels_own_mask(S, N, H, D, p):
    """The mask read off the kernel's forward holds only 0 and 1 / (1 - p) at the expected rate; with it in the fp64 formula the
    forward AND the backward that follows it agree (the backward used the forward's mask); the next forward draws another."""
    from pedestrians_video_2_carla_amd import ops
    d = _dev()
    torch.manual_seed(31)
    st = ops.dropout_state(d)
    site, scale = 4, _f32(D ** -0.5)
    mask = _snap_mask(_k20a_read_mask(st, S, N, H, D, p, site), p, 'attention mask')
    assert _keep_fraction_ok(mask, p), float((mask != 0).double().mean())
    qkv, go = randn_qkv(S, N, H, D, 940 + N)
    ref_out, ref_grad = attn_formula(qkv, go, scale, torch.float64, mask=mask)
    before = st.clone()
    out, gq = k20a_call(qkv.to(d), go.to(d), scale, S, N, H, D, st, p, site)
    assert int(st[2]) == int(st[3]) == int(before[2]) + 1                      # forward: next = step + 1; backward: step = next
    figs = dict(out=tensor_ratio(out, ref_out), grad=tensor_ratio(gq, ref_grad), out_row=row_ratio(out, ref_out),
                grad_row=row_ratio(gq.flatten(2), ref_grad.flatten(2)))
    _report('k20a dropout p={} N={}'.format(p, N), figs)
    assert figs['out'] <= 1e-4 and figs['grad'] <= 1e-4, figs
    assert figs['out_row'] <= ROW_BOUND['k20a/dropout'][0] and figs['grad_row'] <= ROW_BOUND['k20a/dropout'][1], figs
    nxt = _snap_mask(_k20a_read_mask(st, S, N, H, D, p, site), p, 'next attention mask')
    assert not torch.equal(nxt, mask)
    other_site = _snap_mask(_k20a_read_mask(before.clone(), S, N, H, D, p, site + 1), p, 'other site')
    assert not torch.equal(other_site, mask)


@pytest.mark.gpu
@pytest.mark.parametrize('p', [0.1, 0.5])
@pytest.mark.parametrize('rows,D', K20B_DROP, ids=['rows{}-D{}'.format(*s) for s in K20B_DROP])
def test_k20b_dropout_matches_fp64_with_the_kernels_own_mask(rows, D, p):
    """keep = g_s / g_x off the backward holds only 0 and 1 / (1 - p); with it in the fp64 formula z of the FORWARD before it and
    all four gradients agree; the next forward / backward pair draws another mask."""
    from pedestrians_video_2_carla_amd import ops
    d = _dev()
    torch.manual_seed(32)
    st = ops.dropout_state(d)
    c = dict(rows=rows, D=D, seed=960 + D, id='rows{}-D{}-p{}'.format(rows, D, p), bound='k20b/dropout')
    t = norm_input(c, residual=True)
    dv = {k: v.to(d) for k, v in t.items()}
    _, gamma, beta = _params(t, 0, d)
    before = st.clone()
    got = k20b_run(c, dv, gamma, beta, 0, st, p, 3)
    assert int(st[2]) == int(st[3]) == int(before[2]) + 1
    live = got['gx'] != 0
    assert bool(live.all())                                                   # (fixed inputs: no input gradient is exactly zero)
    keep = _snap_mask(got['gs'] / got['gx'], p, 'post-norm mask')
    assert _keep_fraction_ok(keep, p), float((keep != 0).double().mean())
    ref = norm_formula(t, EPS20, torch.float64, keep=keep)
    _check_norm('k20b', c, got, ref, cancellation_floor(t, EPS20, keep), K20B_BOUNDS, {})
    nxt = k20b_run(c, dv, gamma, beta, 0, st, p, 3)
    assert int(st[2]) == int(before[2]) + 2 and not torch.equal(nxt['gs'] != 0, got['gs'] != 0)
    other_site = k20b_run(c, dv, gamma, beta, 0, before.clone(), p, 1)
    assert not torch.equal(other_site['gs'] != 0, got['gs'] != 0)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
_ARENA_FLOATS = 1 << 16


def _refusal_call(name, over, arenas, state):
    e = ENTRY[name]
    values = dict(e['base'])
    values.update(over)
    argv = []
    for a in e['args']:
        if a in POINTERS:
            v = values.get(a, a if a != 'drop_state' and a != 'gx_add' else None)
            if v is None:
                argv.append(None)
            elif v == '+4':
                argv.append(arenas[a].data_ptr() + 4)
            elif a == 'drop_state':
                argv.append(state.data_ptr())
            else:
                argv.append(arenas[a].data_ptr())
        else:
            argv.append(values[a])
    return getattr(_lib(), name)(*argv, _stream())


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(ENTRY))
def test_refused_calls_return_their_code_and_write_nothing(name):
    """Every documented refusal of the entry point: NULL for each pointer in turn, every shape outside its range, the dropout
    probabilities outside [0, 1), the 16-byte alignment K14 and K15 ask for. Every buffer the call was given (outputs, workspaces,
    the dropout state) holds its sentinel afterwards. S = 0 / rows = 0 are no refusals: 0 is returned (and the forward entry points
    write nothing)."""
    d = _dev()
    e = ENTRY[name]
    arenas = {a: torch.full((_ARENA_FLOATS,), SENTINEL, device=d) for a in e['args'] if a in POINTERS and a != 'drop_state'}
    state = torch.tensor([11, 22, 5, 5], dtype=torch.int32, device=d)
    state0 = state.clone()
    for label, over, code in refusals(name):
        rc = _refusal_call(name, over, arenas, state)
        assert rc == code, (name, label, rc)
    empty = {'S': 0} if 'S' in e['args'] else {'rows': 0}
    if 'fwd' in name or 'attn' in name:
        assert _refusal_call(name, empty, arenas, state) == 0, (name, 'empty')
    torch.cuda.synchronize()
    assert torch.equal(state, state0), name
    for a, buf in arenas.items():
        assert bool((buf == SENTINEL).all()), (name, a, 'written by a refused call')


@pytest.mark.gpu
def test_supported_and_workspace_answers():
    lib = _lib()
    assert lib.p2c_attn_small_supported(*K14_UNDER) == 1 and lib.p2c_attn_small_supported(*K14_OVER_BWD) == 0
    for N, H, D in [(0, 1, 4), (65, 1, 4), (5, 0, 4), (5, 1, 0), (5, 3, 3), (64, 5, 4), (64, 4, 8)]:
        assert lib.p2c_attn_small_supported(N, H, D) == 0 and not k14_supported(N, H, D), (N, H, D)
    for c in K14_CASES:
        assert lib.p2c_attn_small_supported(*c['shape']) == 1
    assert [lib.p2c_layernorm_supported(D) for D in (0, 2, 4, 6, 1024, 1028)] == [0, 0, 1, 0, 1, 0]
    assert [lib.p2c_postnorm_supported(D) for D in (1, 2, 3, 1024, 1025)] == [0, 1, 1, 1, 0]
    assert [lib.p2c_attn_drop_supported(*s) for s in ((0, 1, 4), (65, 1, 4), (64, 1, 256), (64, 1, 257), (5, 0, 4), (5, 4, 0))] == [0, 0, 1, 0, 0, 0]
    assert lib.p2c_layernorm_workspace_floats(-1, 8) == 0 and lib.p2c_layernorm_workspace_floats(5, 6) == 0
    assert lib.p2c_postnorm_workspace_floats(-1, 7) == 0 and lib.p2c_postnorm_workspace_floats(5, 1025) == 0


@pytest.mark.gpu
def test_ops_small_attention_refuses_shapes_and_copies_misaligned_views():
    """ops.small_attention raises on a shape the kernel does not take; a dense view that starts 4 bytes into a buffer (it passes
    ``contiguous()`` unchanged, and the kernel would refuse its pointer) gives the bits of the aligned call, gradients included."""
    from pedestrians_video_2_carla_amd import ops
    d = _dev()
    for shape in ((2, 65, 3, 1, 4), (2, 5, 3, 3, 3), (2, 64, 3, 5, 4), (2, 5, 2, 1, 4)):
        x = torch.full(shape, SENTINEL, device=d, requires_grad=True)
        with pytest.raises(RuntimeError):
            ops.small_attention(x, 0.5)
        assert x.grad is None and bool((x == SENTINEL).all())
    S, N, H, D = 3, 9, 2, 12
    qkv, go = randn_qkv(S, N, H, D, 77)
    a = qkv.to(d).requires_grad_(True)
    out = ops.small_attention(a, 0.3)
    out.backward(go.to(d))
    flat = torch.zeros(qkv.numel() + 1, device=d)
    flat[1:] = qkv.flatten().to(d)
    gflat = torch.zeros(go.numel() + 1, device=d)
    gflat[1:] = go.flatten().to(d)
    b = flat[1:].view(S, N, 3, H, D).requires_grad_(True)
    assert b.data_ptr() % 16 == 4 and b.is_contiguous()
    out_b = ops.small_attention(b, 0.3)
    out_b.backward(gflat[1:].view(S, N, H * D))
    assert torch.equal(out_b, out) and torch.equal(b.grad, a.grad)
