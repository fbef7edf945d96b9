"""K12 -- C (+)= A^T [B | 1] of csrc/p2c_atb.hip (``p2c_atb``, ``p2c_atb_scaled``, ``p2c_atb_group``; ``ops.atb``,
``ops.atb_group``) -- in every block, K-tail, slice, scale, flag and group cell, through the C ABI with ctypes.

Launch plan, MIRRORED here from the rule in DESIGN.md / include/p2c.h (``plan``): 32 x 32 blocks of [C | bias column],
    blocks = ceil(M / 32) * ceil((N + bias) / 32),   ks = clamp(min(1024 // blocks, ceil(K / 256)), 1, 256),
    workspace = ks * blocks * 1024 floats,
and every call asserts ``p2c_atb_workspace_floats`` against it, so a change of the rule cannot move a shape out of its cell
unnoticed. A slice is cut into eight equal wave chunks of a multiple of 4 rows (``row_split``, from the header comment of
the kernel file; used to NAME the cell a case is in, never to compute an expected value).

Cell tables (``test_input_conditions`` shows without a GPU that the case tables below reach each of them):
  block cells, K = 37 (BLOCK_M x BLOCK_N x bias off / on)
    whole                 a block inside both matrices with even pitches and 8-byte aligned bases: 8-byte pair loads
    edge-M, edge-N        a block that crosses the last row / column of C: per-lane choice of pair or scalar loads
    straddle-M, -N        M / N odd: the last pair holds one real column (and, for N with a bias, the ones column)
    ones-first            N even, N % 32 != 0: the ones column opens a pair
    ones-second           N odd: the ones column is the second element of the last pair
    ones-last             N % 32 == 31: the ones column is the last column of its block
    bias-in-block         N % 32 == 0: virtual column block, the extra accumulators of column block 0, waves 4 and 5 publish
    bias-in-block ragged  the same with M % 32 != 0
    N=1, M=1
  load cells (ALIGN_SHAPES x LAYOUTS for A x LAYOUTS for B, K = 300, bias on), reached in blocks that are otherwise whole
    pair                  even pitch, base 8-byte aligned (dense, or wider than the matrix and 8 bytes in)
    scalar/base           even pitch, base 4 bytes off
    scalar/pitch          odd pitch
    column-of-A           B = A[:, :1] with ldb = lda (the column sums of ``ops``)
  K cells (K_TABLE on K_SHAPES)
    K=0, K<4, K%4         no row, fewer rows than one MFMA step, a last step with idle row lanes
    past-K                waves (and whole slices) whose chunk starts behind the last row
    chunk<16, =16, >16    below, at and above one unrolled step of 16 rows; tail = unrolled steps followed by a guarded one
  slice regimes (SLICE_CASES): ks=1 | padded (1 < ks < 8: workgroups return on slice >= ks) | ks=8 | ragged (ks > 8, no
    multiple of 8) | cap (256) | tile-limited (1024 // blocks < ceil(K / 256)) | >1024 blocks
  scale cells (SCALE_RPS x SCALE_K x SCALE_SHAPES): every rows_per_scale; K % rows_per_scale != 0 with ``a_scale`` of
    exactly ceil(K / rows_per_scale) entries between NaNs; wave and slice starts inside a group, also for rows_per_scale < 4
  flag cells: accumulate 0..3 x bias NULL / given
  group cells: n = 1, n = 8 (K = 0 member, bias-in-block member, accumulate = 3, two bias_out2), n = 0 / 9 refused,
    ``ops.atb_group`` splitting 11 problems, K = 0 through ``ops``

Exactness (every test but the fp64 one compares with ``torch.equal``): A and B hold integers in [-3, 3], ``a_scale`` values
from {0, 1, 2}, the initial C and bias integers in [-8, 8]. Every partial sum, in any order, is an integer of magnitude
<= 18 K + 8 < 2^24, fp32 arithmetic on those is exact, so the device result must EQUAL the int64 result of the CPU whatever
the summation order. A dropped, doubled or mis-indexed row, a wrong scale index, tile or flag, a stale workspace word: each
changes an integer.

Buffers of every ABI call: C sits at ldc = N + 3 inside a sentinel-filled allocation, bias vectors between sentinel words, the
workspace (NaN-filled: a partial tile that is added without having been written shows) between sentinel words with one whole
slice of them behind it; all sentinels are asserted untouched after every call. Inputs are windows of NaN-filled allocations.

fp64 comparison (``test_randn_against_fp64``): bound of tests/test_gemm_gpu.py for this kernel,
max |got - ref| <= (2e-6 sqrt(K) + 1e-7) max |ref|; ``test_input_conditions`` shows that a sequential fp32 sum of the same
inputs stays within half of it. Each case prints error / bound (``pytest -s``); the largest seen is in DESIGN.md.
"""
import functools
import itertools
import math
import zlib

import pytest
import torch

E_NULL, E_SHAPE = -1, -2
SENT = -777.5
GUARD = 64                                        # floats; even, and a multiple of 4: the workspace stays 16-byte aligned
NAN = float('nan')


# ======================================================================================================================
# the launch plan, mirrored
# ======================================================================================================================
def plan(K, M, N, bias):
    """(blocks, ks, workspace floats)"""
    blocks = -(-M // 32) * -(-(N + (1 if bias else 0)) // 32)
    ks = max(1, min(256, min(1024 // blocks, -(-K // 256))))
    return blocks, ks, ks * blocks * 1024


def row_split(K, ks):
    """(rows per slice, rows per wave): equal slices, each eight equal wave chunks of a multiple of 4 rows"""
    per_slice = -(-K // (ks * 32)) * 32
    return per_slice, per_slice // 8


def regime(K, M, N, bias):
    blocks, ks, _ = plan(K, M, N, bias)
    want = -(-K // 256)
    if blocks > 1024:
        return '>1024 blocks'
    if ks == 256 and want > 256 and 1024 // blocks >= 256:
        return 'cap'
    if ks == 1024 // blocks and ks < want:
        return 'tile-limited'
    if ks == 1:
        return 'ks=1'
    if ks < 8:
        return 'padded'
    return 'ks=8' if ks == 8 else ('ragged' if ks % 8 else 'multiple of 8')


def layout(name, width):
    """(row pitch, floats the base lies behind an 8-byte aligned address)"""
    return {'dense': (width, 0), 'off1': (width + (width & 1), 1), 'w3': (width + 3, 0), 'w4off2': (width + 4, 2)}[name]


def load_cell(name, width):
    pitch, off = layout(name, width)
    return 'scalar/pitch' if pitch & 1 else ('scalar/base' if off & 1 else 'pair')


def block_cells(M, N, bias, la='dense', lb='dense'):
    cells = set()
    pairs_ok = load_cell(la, M) == 'pair' and load_cell(lb, N) == 'pair'
    virtual = bool(bias) and N % 32 == 0
    for mb in range(-(-M // 32)):
        for nb in range(-(-(N + (1 if bias else 0)) // 32) - (1 if virtual else 0)):
            inside_m, inside_n = mb * 32 + 32 <= M, nb * 32 + 32 <= N
            if inside_m and inside_n:
                cells.add('whole' if pairs_ok else 'scalar in a full block')
            if not inside_m:
                cells.add('edge-M')
            if not inside_n:
                cells.add('edge-N')
    if M & 1:
        cells.add('straddle-M')
    if N & 1:
        cells.add('straddle-N')
    if bias:
        if virtual:
            cells.add('bias-in-block')
            if M % 32:
                cells.add('bias-in-block ragged')
        else:
            cells.add('ones-second' if N & 1 else 'ones-first')
            if N % 32 == 31:
                cells.add('ones-last')
    if N == 1:
        cells.add('N=1')
    if M == 1:
        cells.add('M=1')
    return cells


def k_cells(K, M, N, bias):
    _, ks, _ = plan(K, M, N, bias)
    per_slice, chunk = row_split(K, ks)
    cells = set()
    if K == 0:
        cells.add('K=0')
    elif K < 4:
        cells.add('K<4')
    if K % 4:
        cells.add('K%4')
    for s in range(ks):
        for w in range(8):
            k0 = s * per_slice + w * chunk
            rows = min(K, k0 + chunk) - k0
            if rows <= 0:
                if K:
                    cells.add('past-K')
                continue
            cells.add('chunk<16' if rows < 16 else ('chunk=16' if rows == 16 else 'chunk>16'))
            if rows > 16 and rows % 16:
                cells.add('tail')
    return cells


def scale_cells(rps, K, M, N, bias):
    _, ks, _ = plan(K, M, N, bias)
    per_slice, chunk = row_split(K, ks)
    cells = {'rps=%d' % rps}
    small = ' (rps<4)' if rps < 4 else ''
    if K % rps:
        cells.add('K%rps')
    if ks > 1:
        cells.add('slices')
    for s in range(ks):
        for w in range(8):
            k0 = s * per_slice + w * chunk
            if k0 < K and k0 % rps:
                cells.add(('slice' if w == 0 else 'wave') + ' start inside a group' + small)
            if k0 < K and any((k0 + kk) % rps for kk in range(4) if k0 + kk < K):
                cells.add('lane start inside a group' + small)
    return cells


# ======================================================================================================================
# case tables
# ======================================================================================================================
BLOCK_K = 37
BLOCK_M, BLOCK_N = (1, 2, 31, 32, 33, 64, 65), (1, 2, 31, 32, 33, 63, 64, 96)
BLOCK_CASES = list(itertools.product(BLOCK_M, BLOCK_N, (0, 1)))
BLOCK_CELLS = ('whole', 'edge-M', 'edge-N', 'straddle-M', 'straddle-N', 'N=1', 'M=1')
BIAS_CELLS = ('ones-first', 'ones-second', 'ones-last', 'bias-in-block', 'bias-in-block ragged')

LAYOUTS = ('dense', 'off1', 'w3', 'w4off2')
ALIGN_SHAPES, ALIGN_K = ((64, 64), (33, 31), (65, 33)), 300   # the last: whole blocks next to straddling pairs (even pitches)
LOAD_CELLS = ('pair', 'scalar/base', 'scalar/pitch')

K_TABLE = (0, 1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 255, 256, 257, 700, 1000)
K_SHAPES = ((40, 24), (32, 32))                  # with bias: ones column inside the block | bias-in-block
K_CELLS = ('K=0', 'K<4', 'K%4', 'past-K', 'chunk<16', 'chunk=16', 'chunk>16', 'tail')

# regime -> (K, M, N, bias, ks)
SLICE_CASES = {'ks=1': (37, 40, 40, 1, 1), 'padded': (700, 40, 40, 1, 3), 'ks=8': (2048, 40, 40, 1, 8), 'ragged': (3100, 40, 40, 1, 13),
               'cap': (65537, 5, 3, 1, 256), 'tile-limited': (15360, 256, 64, 1, 42), '>1024 blocks': (40, 1056, 993, 1, 1)}
# the 4-block regimes once more on a problem with the virtual bias block (2 x (1 real + 1 virtual) blocks)
SLICE_CASES_VIRTUAL = {'padded': (700, 64, 32, 1, 3), 'ks=8': (2048, 64, 32, 1, 8), 'ragged': (3100, 64, 32, 1, 13)}

SCALE_RPS, SCALE_K, SCALE_SHAPES = (1, 2, 3, 4, 5, 7, 26), (37, 257, 3100, 3101), ((33, 31), (64, 64))
SCALE_CASES = list(itertools.product(SCALE_RPS, SCALE_K, SCALE_SHAPES))

FLAG_SHAPES, FLAG_K = ((33, 32), (32, 31)), 300

# n = 8 group: (K, M, N, bias, bias2, flags, layout of A, layout of B)
GROUP8 = ((0, 40, 24, 1, 0, 0, 'dense', 'dense'),          # no rows: zeros
          (300, 33, 32, 1, 0, 0, 'dense', 'dense'),        # bias-in-block, ragged M
          (700, 40, 40, 1, 0, 3, 'w3', 'dense'),           # accumulate = 3, padded grid
          (37, 65, 63, 1, 1, 0, 'dense', 'w4off2'),        # bias_out2
          (2048, 64, 32, 1, 1, 2, 'dense', 'dense'),       # bias_out2 added into, C overwritten; bias-in-block, ks = 8
          (257, 1, 1, 0, 0, 1, 'dense', 'off1'),
          (3100, 33, 31, 0, 0, 0, 'off1', 'w4off2'),       # ragged slice count
          (1000, 32, 96, 0, 0, 0, 'dense', 'dense'))

# fp64 comparison: (name, K, M, N, bias, layout of A, layout of B, rows_per_scale of the run with a row factor)
ACC_CASES = (('ks=1 whole', 200, 64, 64, 0, 'dense', 'dense', 3),
             ('ks=1 edge', 129, 33, 31, 1, 'dense', 'dense', 3),
             ('scalar in a full block', 300, 64, 64, 1, 'w3', 'off1', 3),
             ('bias-in-block ragged', 255, 40, 32, 1, 'dense', 'dense', 3),
             ('padded', 700, 40, 40, 1, 'dense', 'dense', 3),
             ('ks=8', 2048, 64, 32, 1, 'dense', 'dense', 5),
             ('ragged', 3100, 40, 40, 1, 'dense', 'dense', 3),
             ('cap', 65537, 5, 3, 1, 'dense', 'dense', 7),
             ('tile-limited', 15360, 256, 64, 1, 'dense', 'dense', 26),
             ('>1024 blocks', 40, 1056, 993, 1, 'dense', 'dense', 3))


MAGNITUDE_CASES = ((700, 40, 40), (300, 64, 64), (129, 33, 31))


def bound(K):
    return 2e-6 * math.sqrt(K) + 1e-7            # tests/test_gemm_gpu.py


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def exact_case(K, M, N, rps=0, seed=0):
    """Integer operands and the int64 results: prod = (f A)^T B, colsum = column sums of f A."""
    g = _gen('exact', K, M, N, rps, seed)
    c = Case()
    c.K, c.M, c.N, c.rps = K, M, N, rps
    c.a = torch.randint(-3, 4, (K, M), generator=g)
    c.b = torch.randint(-3, 4, (K, N), generator=g)
    c.c0 = torch.randint(-8, 9, (M, N), generator=g)
    c.bias0 = torch.randint(-8, 9, (M,), generator=g)
    c.bias20 = torch.randint(-8, 9, (M,), generator=g)
    af = c.a
    c.f = None
    if rps:
        groups = -(-K // rps)
        steps = torch.randint(1, 3, (groups,), generator=g)           # neighbouring groups differ: each factor is the last + 1 or + 2 mod 3
        c.f = (torch.cumsum(steps, 0) + int(torch.randint(0, 3, (1,), generator=g))) % 3
        af = c.a * c.f.repeat_interleave(rps)[:K, None]
    c.prod, c.colsum = af.t() @ c.b, af.sum(0)
    return c


def expected(c, flags, with_bias):
    C = (c.c0 if flags & 1 else 0) + c.prod
    if not with_bias:
        return C.float(), None, None
    return C.float(), ((c.bias0 if flags & 2 else 0) + c.colsum).float(), ((c.bias20 if flags & 2 else 0) + c.colsum).float()


@functools.lru_cache(maxsize=None)
def randn_case(K, M, N, rps):
    g = _gen('randn', K, M, N, rps)
    c = Case()
    c.a, c.b = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    c.f = None
    af = c.a.double()
    if rps:
        c.f = (torch.rand(-(-K // rps), generator=g) > 0.3).float() / 0.7
        af = af * c.f.double().repeat_interleave(rps)[:K, None]
    c.ref, c.refb = af.t() @ c.b.double(), af.sum(0)
    return c


def sequential_fp32(c, rps):
    """row after row in fp32, as the plainest CPU loop would"""
    a = c.a if c.f is None else c.a * c.f.repeat_interleave(rps)[:len(c.a), None]
    acc, accb = torch.zeros(a.shape[1], c.b.shape[1]), torch.zeros(a.shape[1])
    for k in range(a.shape[0]):
        acc += a[k, :, None] * c.b[k, None, :]
        accb += a[k]
    return acc, accb


def all_exact_K():
    ks = {BLOCK_K, ALIGN_K, FLAG_K} | set(K_TABLE) | set(SCALE_K) | {g[0] for g in GROUP8}
    return ks | {v[0] for v in SLICE_CASES.values()} | {v[0] for v in SLICE_CASES_VIRTUAL.values()}


# ======================================================================================================================
# host-only: the tables reach their cells, the numeric preconditions hold
# ======================================================================================================================
def test_input_conditions():
    # ---- the mirror against hand-computed plans
    assert plan(37, 64, 64, 0) == (4, 1, 4096) and plan(37, 64, 64, 1) == (6, 1, 6144) and plan(0, 5, 3, 1) == (1, 1, 1024)
    assert plan(8192, 256, 64, 0) == (16, 32, 32 * 16 * 1024) and plan(546624, 96, 32, 1) == (6, 170, 170 * 6 * 1024)
    assert row_split(257, 2) == (160, 20) and row_split(37, 1) == (64, 8) and row_split(0, 1) == (0, 0)
    # ---- (a) block cells, in both bias states where they apply
    for bias in (0, 1):
        reached = set().union(*(block_cells(M, N, b) for M, N, b in BLOCK_CASES if b == bias))
        assert reached >= set(BLOCK_CELLS), (bias, set(BLOCK_CELLS) - reached)
        assert (reached >= set(BIAS_CELLS)) if bias else not (reached & set(BIAS_CELLS))
    assert all(plan(BLOCK_K, M, N, b)[1] == 1 for M, N, b in BLOCK_CASES)
    assert k_cells(BLOCK_K, 64, 64, 0) == {'K%4', 'past-K', 'chunk<16'}          # one slice, every wave on the guarded step or empty
    # straddling pairs in a problem that also has whole blocks: odd M and N under even pitches (a dense odd width is an odd pitch)
    assert block_cells(65, 33, 1, 'w3', 'w3') >= {'whole', 'straddle-M', 'straddle-N'} and 'whole' not in block_cells(65, 33, 1)
    # ---- load cells: each for A and for B, in full blocks (64 x 64), in edge blocks (33 x 31) and in both (65 x 33)
    for M, N in ALIGN_SHAPES:
        assert {load_cell(l, M) for l in LAYOUTS} == set(LOAD_CELLS) == {load_cell(l, N) for l in LAYOUTS}, (M, N)
        for l in LAYOUTS:
            for w in (M, N):
                assert layout(l, w)[0] >= w
    assert layout('off1', 64) == (64, 1) and layout('w3', 64) == (67, 0) and layout('w4off2', 64) == (68, 2)
    assert block_cells(64, 64, 1, 'dense', 'dense') >= {'whole', 'bias-in-block'}
    assert 'scalar in a full block' in block_cells(64, 64, 1, 'off1', 'dense') & block_cells(64, 64, 1, 'dense', 'w3')
    assert all(plan(ALIGN_K, M, N, 1)[1] == 2 for M, N in ALIGN_SHAPES)
    # ---- K cells on both shapes
    for M, N in K_SHAPES:
        reached = set().union(*(k_cells(K, M, N, 1) for K in K_TABLE))
        assert reached >= set(K_CELLS), (M, N, set(K_CELLS) - reached)
    assert 'bias-in-block' in block_cells(32, 32, 1) and 'ones-first' in block_cells(40, 24, 1)
    # ---- slice regimes
    assert set(SLICE_CASES) == {'ks=1', 'padded', 'ks=8', 'ragged', 'cap', 'tile-limited', '>1024 blocks'}
    for table in (SLICE_CASES, SLICE_CASES_VIRTUAL):
        for name, (K, M, N, bias, ks) in table.items():
            assert regime(K, M, N, bias) == name and plan(K, M, N, bias)[1] == ks, (name, regime(K, M, N, bias), plan(K, M, N, bias))
    assert all(plan(*v[:4])[0] == 4 for k, v in SLICE_CASES.items() if k in ('padded', 'ks=8', 'ragged'))
    assert all('bias-in-block' in block_cells(v[1], v[2], 1) for v in SLICE_CASES_VIRTUAL.values())
    assert plan(*SLICE_CASES['>1024 blocks'][:4])[0] == 1056 and plan(*SLICE_CASES['tile-limited'][:4])[0] == 24
    assert max(plan(*v[:4])[2] for v in SLICE_CASES.values()) == 1056 * 1024      # the largest workspace of the file: 4.3 MB
    # ---- scale cells
    reached = set().union(*(scale_cells(r, K, M, N, 1) for r, K, (M, N) in SCALE_CASES))
    need = {'rps=%d' % r for r in SCALE_RPS} | {'K%rps', 'slices'}
    for what in ('slice', 'wave', 'lane'):
        need |= {what + ' start inside a group', what + ' start inside a group (rps<4)'}
    assert reached >= need, need - reached
    for r in SCALE_RPS[1:]:
        assert 'K%rps' in scale_cells(r, 37, 33, 31, 1)
        c = exact_case(257, 33, 31, r)
        assert len(c.f) == -(-257 // r) and bool((c.f[1:] != c.f[:-1]).all()) and set(c.f.tolist()) <= {0, 1, 2}
    assert {'bias-in-block', 'whole'} <= block_cells(64, 64, 1) and {'edge-M', 'ones-second'} <= block_cells(33, 31, 1)
    # ---- flags and group
    assert 'bias-in-block ragged' in block_cells(*FLAG_SHAPES[0], 1) and 'ones-last' in block_cells(*FLAG_SHAPES[1], 1)
    assert len(GROUP8) == 8 and len(set(GROUP8)) == 8
    assert any(g[0] == 0 for g in GROUP8) and any(g[5] == 3 for g in GROUP8) and sum(g[4] for g in GROUP8) == 2
    assert any('bias-in-block' in block_cells(g[1], g[2], g[3]) for g in GROUP8)
    assert {regime(*g[:4]) for g in GROUP8} >= {'ks=1', 'padded', 'ks=8', 'ragged'}
    # ---- (b) exactness: every partial sum is an integer below 2^24
    for K in all_exact_K():
        assert 18 * K + 8 < 2 ** 24, K
    c = exact_case(257, 33, 31, 3)
    assert c.a.abs().max() <= 3 and c.b.abs().max() <= 3 and c.c0.abs().max() <= 8 and c.bias0.abs().max() <= 8
    assert c.prod.dtype == torch.int64 and int((c.a.abs().t() @ c.b.abs()).max()) * 2 + 8 <= 18 * 257 + 8
    # ---- (b) fp64 comparison: the cases cover every slice regime and block path, and a sequential fp32 sum of each stays
    # within half of the bound
    assert {regime(K, M, N, b) for _, K, M, N, b, _, _, _ in ACC_CASES} >= set(SLICE_CASES)
    paths = set().union(*(block_cells(M, N, b, la, lb) for _, K, M, N, b, la, lb, _ in ACC_CASES))
    assert paths >= {'whole', 'edge-M', 'edge-N', 'scalar in a full block', 'bias-in-block', 'bias-in-block ragged', 'ones-second',
                     'ones-first'}
    for name, K, M, N, bias, la, lb, rps in ACC_CASES:
        for r in (0, rps):
            c = randn_case(K, M, N, r)
            acc, accb = sequential_fp32(c, r)
            e = float((acc.double() - c.ref).abs().max() / c.ref.abs().max()) / bound(K)
            eb = float((accb.double() - c.refb).abs().max() / c.refb.abs().max()) / bound(K)
            assert e <= 0.5 and eb <= 0.5, (name, r, e, eb)
    # ---- magnitude cases: nothing under- or overflows (|value| in {0} or [2^-12, 8], factors 2^-10 .. 2^10 per side)
    for K, M, N in MAGNITUDE_CASES:
        a, b, s, r = magnitude_case(K, M, N)
        for t in (a, b):
            nz = t[t != 0].abs()
            assert float(nz.min()) >= 2.0 ** -12 and float(nz.max()) <= 8.0
        assert float(s.min()) >= 2.0 ** -10 and float(s.max()) <= 2.0 ** 10 and bool((torch.log2(s) % 1 == 0).all())
        assert K * 64.0 * 2.0 ** 20 < 3e38 and 2.0 ** -24 * 2.0 ** -20 > 2.0 ** -126


# ======================================================================================================================
# device side
# ======================================================================================================================
def lib():
    from pedestrians_video_2_carla_amd import _lib
    return _lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Span:
    """A (rows, cols) window with row pitch ``pitch``, ``front`` floats into a flat device allocation filled with ``fill``,
    with ``back`` floats behind it. The address is computed (a tensor without elements has none)."""

    def __init__(self, rows, cols, pitch, fill, init=None, front=GUARD, back=GUARD):
        self.rows, self.cols, self.pitch, self.fill, self.front = rows, cols, pitch, fill, front
        body = (rows - 1) * pitch + cols if rows else 0
        self.buf = torch.full((front + body + back,), fill, dtype=torch.float32, device='cuda')
        assert self.buf.data_ptr() % 16 == 0
        if init is not None:
            self.view.copy_(init.reshape(rows, cols))

    @property
    def view(self):
        return self.buf.as_strided((self.rows, self.cols), (self.pitch, 1), self.front)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.front

    def host(self):
        return self.view.cpu()

    def untouched_outside(self):
        c = self.buf.clone()
        c.as_strided((self.rows, self.cols), (self.pitch, 1), self.front).fill_(self.fill)
        return bool((c == self.fill).all())


def operand(t, name):
    """the CPU matrix as a window of a NaN-filled allocation, in layout ``name``"""
    pitch, off = layout(name, t.shape[1])
    s = Span(t.shape[0], t.shape[1], pitch, NAN, t.float(), front=GUARD + off)
    assert s.ptr % 8 == 4 * (off & 1)
    return s


def vector(t, fill=SENT):
    return Span(len(t), 1, 1, fill, t.float())


def workspace(floats, behind):
    ws = Span(1, floats, floats, SENT, back=behind)
    ws.view.fill_(NAN)
    assert ws.ptr % 16 == 0
    return ws


class Run:
    pass


def abi_run(a, b, c0, bias0=None, flags=0, f=None, rps=1, la='dense', lb='dense', b_column_of_a=False):
    """One p2c_atb / p2c_atb_scaled call on guarded buffers; CPU tensors in, the outputs on the CPU back. ``bias0``: the initial
    bias vector, None = NULL bias_out."""
    L = lib()
    K, M = a.shape
    A = operand(a, la)
    if b_column_of_a:
        N, b_ptr, ldb = 1, A.ptr, A.pitch
    else:
        Bm = operand(b, lb)
        N, b_ptr, ldb = b.shape[1], Bm.ptr, Bm.pitch
    with_bias = bias0 is not None
    blocks, ks, floats = plan(K, M, N, with_bias)
    assert L.p2c_atb_workspace_floats(K, M, N, int(with_bias)) == floats, (K, M, N, with_bias)
    C, ws = Span(M, N, N + 3, SENT, c0.float()), workspace(floats, blocks * 1024)
    bias = vector(bias0) if with_bias else None
    if f is None:
        rc = L.p2c_atb(A.ptr, A.pitch, b_ptr, ldb, K, M, N, C.ptr, C.pitch, bias.ptr if with_bias else None, flags, ws.ptr, stream())
    else:
        assert len(f) == -(-K // rps)
        F = vector(f, NAN)
        rc = L.p2c_atb_scaled(A.ptr, A.pitch, b_ptr, ldb, K, M, N, C.ptr, C.pitch, bias.ptr if with_bias else None, flags, F.ptr,
                              rps, ws.ptr, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert C.untouched_outside(), 'written outside C'
    assert ws.untouched_outside(), 'written outside the workspace'
    assert bias is None or bias.untouched_outside(), 'written outside bias_out'
    r = Run()
    r.C, r.bias = C.host(), (bias.host().flatten() if with_bias else None)
    return r


def run_exact(c, with_bias, flags=0, **kw):
    """the exact case on the device, compared with the int64 result"""
    r = abi_run(c.a, c.b, c.c0, c.bias0 if with_bias else None, flags, f=c.f, rps=c.rps or 1, **kw)
    C, bias, _ = expected(c, flags, with_bias)
    assert torch.equal(r.C, C), 'C: %d wrong elements' % int((r.C != C).sum())
    assert (not with_bias) or torch.equal(r.bias, bias), 'bias'
    return r


@pytest.mark.gpu
@pytest.mark.parametrize('M,N,bias', BLOCK_CASES)
def test_block_cells_exact(M, N, bias):
    run_exact(exact_case(BLOCK_K, M, N), bool(bias))


@pytest.mark.gpu
@pytest.mark.parametrize('M,N', K_SHAPES)
@pytest.mark.parametrize('K', K_TABLE)
def test_k_tails_exact(K, M, N):
    """every K of the table, overwriting and under both accumulate bits (K = 0: zeros, resp. C and bias as they were)"""
    c = exact_case(K, M, N)
    r = run_exact(c, True, 0)
    run_exact(c, True, 3)
    if K == 0:
        assert not r.C.any() and not r.bias.any()
        r = run_exact(c, True, 3)
        assert torch.equal(r.C, c.c0.float()) and torch.equal(r.bias, c.bias0.float())
        run_exact(c, False, 0), run_exact(c, False, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('table,name', [('real', k) for k in SLICE_CASES] + [('virtual', k) for k in SLICE_CASES_VIRTUAL])
def test_slice_regimes_exact(table, name):
    K, M, N, bias, ks = (SLICE_CASES if table == 'real' else SLICE_CASES_VIRTUAL)[name]
    assert lib().p2c_atb_workspace_floats(K, M, N, bias) == ks * plan(K, M, N, bias)[0] * 1024
    c = exact_case(K, M, N)
    run_exact(c, bool(bias), 0)
    run_exact(c, bool(bias), 3)


@pytest.mark.gpu
@pytest.mark.parametrize('M,N', ALIGN_SHAPES)
def test_load_forms_give_the_same_bits(M, N):
    """4 x 4 layouts of A and B: the loaded values and the summation order do not depend on the load width. And B as the first
    column of A (ldb = lda)."""
    c = exact_case(ALIGN_K, M, N)
    dense = run_exact(c, True, 0)
    for la, lb in itertools.product(LAYOUTS, LAYOUTS):
        r = run_exact(c, True, 0, la=la, lb=lb)
        assert torch.equal(r.C, dense.C) and torch.equal(r.bias, dense.bias), (la, lb)
    col = Case()
    col.a, col.b, col.c0, col.bias0, col.bias20, col.f, col.rps = c.a, c.a[:, :1], c.c0[:, :1], c.bias0, c.bias20, None, 0
    col.prod, col.colsum = c.a.t() @ c.a[:, :1], c.colsum
    for la in LAYOUTS:
        for flags in (0, 3):
            run_exact(col, True, flags, la=la, b_column_of_a=True)
        run_exact(col, False, 0, la=la, b_column_of_a=True)


@pytest.mark.gpu
@pytest.mark.parametrize('rps,K,shape', SCALE_CASES)
def test_row_factor_exact(rps, K, shape):
    c = exact_case(K, shape[0], shape[1], rps)
    run_exact(c, True, 0)
    run_exact(c, False, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('M,N', FLAG_SHAPES)
def test_accumulate_bits_are_independent(M, N):
    c = exact_case(FLAG_K, M, N)
    for flags in (0, 1, 2, 3):
        r = run_exact(c, True, flags)
        # written out once more: bit 0 adds to C only, bit 1 to the bias only
        assert torch.equal(r.C, ((c.c0 if flags & 1 else 0) + c.prod).float())
        assert torch.equal(r.bias, ((c.bias0 if flags & 2 else 0) + c.colsum).float())
        run_exact(c, False, flags)                        # NULL bias: nothing but C changes (the guards say so)


# ---- group ---------------------------------------------------------------------------------------------------------------
def group_run(members, n=None, call=True):
    """members: (case, with_bias, with_bias2, flags, la, lb). One p2c_atb_group call on guarded buffers."""
    from pedestrians_video_2_carla_amd import _lib
    L = lib()
    arr = (_lib.AtbProblem * max(1, len(members)))()
    boxes, total, behind = [], 0, 0
    for q, (c, wb, wb2, flags, la, lb) in zip(arr, members):
        A, Bm = operand(c.a, la), operand(c.b, lb)
        C = Span(c.M, c.N, c.N + 3, SENT, c.c0.float())
        bias, bias2 = (vector(c.bias0) if wb else None), (vector(c.bias20) if wb2 else None)
        q.a, q.a_stride, q.b, q.b_stride, q.K, q.M, q.N = A.ptr, A.pitch, Bm.ptr, Bm.pitch, c.K, c.M, c.N
        q.out, q.out_stride, q.flags = C.ptr, C.pitch, flags
        q.bias_out, q.bias_out2 = (bias.ptr if wb else None), (bias2.ptr if wb2 else None)
        blocks, _, floats = plan(c.K, c.M, c.N, wb)
        total, behind = total + floats, max(behind, blocks * 1024)
        boxes.append((A, Bm, C, bias, bias2))
    n = len(members) if n is None else n
    assert L.p2c_atb_group_workspace_floats(arr, n) == total
    ws = workspace(total, behind)
    rc = L.p2c_atb_group(arr, n, ws.ptr, stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert ws.untouched_outside(), 'written outside the workspace'
    out = []
    for A, Bm, C, bias, bias2 in boxes:
        assert C.untouched_outside() and (bias is None or bias.untouched_outside()) and (bias2 is None or bias2.untouched_outside())
        out.append((C.host(), None if bias is None else bias.host().flatten(), None if bias2 is None else bias2.host().flatten()))
    return out


def check_group(members):
    got = group_run(members)
    for i, ((c, wb, wb2, flags, la, lb), (C, bias, bias2)) in enumerate(zip(members, got)):
        single = abi_run(c.a, c.b, c.c0, c.bias0 if wb else None, flags, la=la, lb=lb)
        wC, wbias, wbias2 = expected(c, flags, wb)
        assert torch.equal(C, single.C) and torch.equal(C, wC), i
        if wb:
            assert torch.equal(bias, single.bias) and torch.equal(bias, wbias), i
        if wb2:
            assert torch.equal(bias2, wbias2), i
            if not flags & 2:
                assert torch.equal(bias2, single.bias), i
    return got


def group8():
    return [(exact_case(K, M, N, seed=i), bool(b), bool(b2), flags, la, lb) for i, (K, M, N, b, b2, flags, la, lb) in enumerate(GROUP8)]


@pytest.mark.gpu
def test_group_of_one_and_of_eight_equal_the_single_launches():
    members = group8()
    for m in members:
        check_group([m])
    got = check_group(members)
    assert not got[0][0].any() and not got[0][1].any()                    # the K = 0 member wrote zeros
    again = group_run(members)
    for g, h in zip(got, again):
        assert all(torch.equal(x, y) for x, y in zip(g, h) if x is not None)


@pytest.mark.gpu
def test_ops_group_of_eleven_equals_ops_atb_one_by_one():
    """``ops.atb_group`` splits 11 problems into 8 + 3; members without rows write zeros (or leave an accumulator alone) exactly
    as ``ops.atb`` does."""
    from pedestrians_video_2_carla_amd import ops
    d = torch.device('cuda')
    shapes = [g[:3] for g in GROUP8] + [(129, 31, 2), (0, 7, 5), (5, 64, 64)]
    cases = [exact_case(K, M, N, seed=20 + i) for i, (K, M, N) in enumerate(shapes)]
    # (bias, outputs given, accumulate, second bias vector)
    modes = [(True, True, False, True), (True, False, False, False), (True, True, True, False), (False, False, False, False),
             (True, True, False, True), (False, True, True, False), (True, True, True, True), (False, True, False, False),
             (True, False, False, False), (True, True, True, True), (True, True, True, False)]
    assert shapes[0][0] == 0 and modes[0][:3] == (True, True, False) and shapes[9][0] == 0 and modes[9][2]

    def build(group):
        problems = []
        for c, (bias, given, acc, second) in zip(cases, modes):
            wide = torch.full((c.K, c.M + 4), NAN, device=d)
            a, b = wide[:, 2:2 + c.M], c.b.float().to(d)
            a.copy_(c.a.float())
            pr = dict(a=a, b=b, bias=bias, accumulate=acc)
            if given:
                pr['out'] = c.c0.float().to(d)
                if bias:
                    pr['bias_out'] = c.bias0.float().to(d)
            if second and group:
                pr['bias_out2'] = c.bias20.float().to(d)
            problems.append(pr)
        return problems

    grouped = build(True)
    res = ops.atb_group(grouped)
    singles = build(False)
    for i, (c, pr, one, (bias, given, acc, second)) in enumerate(zip(cases, grouped, singles, modes)):
        out, bo = ops.atb(one['a'], one['b'], bias=bias, out=one.get('out'), bias_out=one.get('bias_out'), accumulate=acc)
        flags = (1 if (acc and given) else 0) | (2 if (acc and given and bias) else 0)
        wC, wbias, wbias2 = expected(c, flags, bias)
        assert torch.equal(res[i][0], out) and torch.equal(out.cpu(), wC), i
        if given:
            assert res[i][0] is pr['out'] and out is one['out']
        if bias:
            assert torch.equal(res[i][1], bo) and torch.equal(bo.cpu(), wbias), i
            if second:
                assert torch.equal(pr['bias_out2'].cpu(), wbias2), i
        else:
            assert res[i][1] is None and bo is None
    # a fresh operand without rows (no address at all), every output fresh
    e = ops.atb(torch.empty(0, 7, device=d), torch.empty(0, 5, device=d), bias=True)
    assert e[0].shape == (7, 5) and not e[0].any() and e[1].shape == (7,) and not e[1].any()
    (g0, gb), = ops.atb_group([dict(a=torch.empty(0, 7, device=d), b=torch.empty(0, 5, device=d), bias=True)])
    assert torch.equal(g0, e[0]) and torch.equal(gb, e[1])


# ---- error paths ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_entry_points_refuse_bad_arguments():
    """status only: nothing is written, sentinels and outputs as they were"""
    L = lib()
    K, M, N = 40, 5, 3
    c = exact_case(K, M, N)
    A, Bm = operand(c.a, 'dense'), operand(c.b, 'dense')
    C, bias, F = Span(M, N, N + 3, SENT, c.c0.float()), vector(c.bias0), vector(torch.ones(K))
    ws = workspace(plan(K, M, N, 1)[2], 1024)
    ok = dict(A=A.ptr, lda=M, B=Bm.ptr, ldb=N, K=K, M=M, N=N, C=C.ptr, ldc=N + 3, bias=bias.ptr, acc=0, ws=ws.ptr)

    def call(scaled=False, a_scale=None, rps=1, **kw):
        p = dict(ok, **kw)
        head = (p['A'], p['lda'], p['B'], p['ldb'], p['K'], p['M'], p['N'], p['C'], p['ldc'], p['bias'], p['acc'])
        if scaled:
            return L.p2c_atb_scaled(*head, a_scale, rps, p['ws'], stream())
        return L.p2c_atb(*head, p['ws'], stream())

    for scaled in (False, True):
        for name in ('A', 'B', 'C', 'ws'):
            assert call(scaled, **{name: None}) == E_NULL, name
        for kw in (dict(K=-1), dict(M=0), dict(N=0), dict(M=-3), dict(lda=M - 1), dict(ldb=N - 1), dict(ldc=N - 1)):
            assert call(scaled, **kw) == E_SHAPE, kw
    assert call(True, a_scale=F.ptr, rps=0) == E_SHAPE and call(True, a_scale=F.ptr, rps=-2) == E_SHAPE
    assert L.p2c_atb_workspace_floats(-1, M, N, 1) == 0 and L.p2c_atb_workspace_floats(K, 0, N, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(C.host(), c.c0.float()) and torch.equal(bias.host().flatten(), c.bias0.float())
    assert C.untouched_outside() and bias.untouched_outside() and ws.untouched_outside() and bool(ws.view.isnan().all())
    assert call(True, a_scale=None, rps=0) == 0 and call(False) == 0            # no a_scale: rows_per_scale is not looked at
    torch.cuda.synchronize()
    assert torch.equal(C.host(), c.prod.float())


@pytest.mark.gpu
def test_group_refuses_bad_arguments():
    from pedestrians_video_2_carla_amd import _lib
    L = lib()
    c = exact_case(40, 5, 3)
    A, Bm = operand(c.a, 'dense'), operand(c.b, 'dense')
    C, bias, bias2 = Span(5, 3, 6, SENT, c.c0.float()), vector(c.bias0), vector(c.bias20)
    ws = workspace(9 * 1024, 1024)

    def problems(n, **kw):
        arr = (_lib.AtbProblem * n)()
        for q in arr:
            q.a, q.a_stride, q.b, q.b_stride, q.K, q.M, q.N = A.ptr, 5, Bm.ptr, 3, 40, 5, 3
            q.out, q.out_stride, q.flags, q.bias_out, q.bias_out2 = C.ptr, 6, 0, bias.ptr, bias2.ptr
        for k, v in kw.items():
            setattr(arr[n - 1], k, v)
        return arr

    assert L.p2c_atb_group(problems(9), 9, ws.ptr, stream()) == E_SHAPE and L.p2c_atb_group(problems(1), 0, ws.ptr, stream()) == E_SHAPE
    assert L.p2c_atb_group_workspace_floats(problems(9), 9) == 0 and L.p2c_atb_group_workspace_floats(problems(1), 0) == 0
    assert L.p2c_atb_group(None, 1, ws.ptr, stream()) == E_NULL and L.p2c_atb_group_workspace_floats(None, 1) == 0
    assert L.p2c_atb_group(problems(2), 2, None, stream()) == E_NULL
    for kw in (dict(out=None), dict(a=None), dict(b=None), dict(bias_out=None)):          # the last: bias_out2 without bias_out
        assert L.p2c_atb_group(problems(2, **kw), 2, ws.ptr, stream()) == E_NULL, kw
    for kw in (dict(K=-1), dict(M=0), dict(N=0), dict(a_stride=4), dict(b_stride=2), dict(out_stride=2)):
        assert L.p2c_atb_group(problems(3, **kw), 3, ws.ptr, stream()) == E_SHAPE, kw
    torch.cuda.synchronize()
    assert torch.equal(C.host(), c.c0.float()) and torch.equal(bias.host().flatten(), c.bias0.float())
    assert torch.equal(bias2.host().flatten(), c.bias20.float())
    assert C.untouched_outside() and bias.untouched_outside() and bias2.untouched_outside()
    assert ws.untouched_outside() and bool(ws.view.isnan().all())
    assert L.p2c_atb_group_workspace_floats(problems(8), 8) == 8 * 1024


# ---- fp64, magnitudes, repeat calls ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('case', ACC_CASES, ids=[c[0] for c in ACC_CASES])
def test_randn_against_fp64(case):
    name, K, M, N, bias, la, lb, rps = case
    for r in (0, rps):
        c = randn_case(K, M, N, r)
        got = abi_run(c.a, c.b, torch.zeros(M, N), torch.zeros(M) if bias else None, 0, f=c.f, rps=r or 1, la=la, lb=lb)
        e = float((got.C.double() - c.ref).abs().max() / c.ref.abs().max()) / bound(K)
        eb = float((got.bias.double() - c.refb).abs().max() / c.refb.abs().max()) / bound(K) if bias else 0.0
        print('atb error / bound: %-24s rows_per_scale %2d  C %.4f  bias %.4f' % (name, r, e, eb))
        assert e <= 1.0 and eb <= 1.0, (name, r, e, eb)
        again = abi_run(c.a, c.b, torch.zeros(M, N), torch.zeros(M) if bias else None, 0, f=c.f, rps=r or 1, la=la, lb=lb)
        assert torch.equal(got.C, again.C) and (not bias or torch.equal(got.bias, again.bias))       # two calls, the same bits


@functools.lru_cache(maxsize=None)
def magnitude_case(K, M, N):
    g = _gen('magnitude', K, M, N)
    q = lambda t: torch.round(t.clamp(-8, 8) * 4096) / 4096   # noqa: E731  (multiples of 2^-12: no product near the subnormals)
    a, b = q(torch.randn(K, M, generator=g)), q(torch.randn(K, N, generator=g))
    s = 2.0 ** torch.randint(-10, 11, (M,), generator=g).float()
    r = 2.0 ** torch.randint(-10, 11, (N,), generator=g).float()
    return a, b, s, r


@pytest.mark.gpu
@pytest.mark.parametrize('K,M,N', MAGNITUDE_CASES)
def test_column_magnitudes_do_not_leak(K, M, N):
    """Column i of A times s_i, column j of B times r_j (powers of two): C[i, j] is s_i r_j times what it was and the bias s_i
    times, bit for bit -- each output element depends on its own two columns only."""
    a, b, s, r = magnitude_case(K, M, N)
    f = (torch.rand(-(-K // 3), generator=_gen('mf', K)) > 0.3).float() * 2
    for fac in (None, f):
        one = abi_run(a, b, torch.zeros(M, N), torch.zeros(M), 0, f=fac, rps=3)
        two = abi_run(a * s, b * r, torch.zeros(M, N), torch.zeros(M), 0, f=fac, rps=3)
        assert torch.equal(two.C, one.C * s[:, None] * r[None, :])
        assert torch.equal(two.bias, one.bias * s)
        assert bool(one.C.isfinite().all()) and bool(two.C.isfinite().all())
