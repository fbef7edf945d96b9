"""K19 -- the fused BatchNorm1d + ReLU + dropout (+ residual) kernels of csrc/p2c_bnorm.hip (``ops.batch_norm_act``) -- in every
cell of their host-side dispatch, through the C ABI (``_lib.BnormDesc``), against fp64 ``nn.BatchNorm1d`` -> ReLU -> + residual
on the CPU (gradients by fp64 autograd of the same module).

The host code picks two things per call, and the tables below walk both.

Row plan (``slab_rows_for`` is MIRRORED here; every case asserts its slab count through ``p2c_bnorm_workspace_floats``, so a
change of TARGET_BLOCKS cannot move a shape out of its cell unnoticed):
  N = 2, 5      one slab, fewer rows than the four waves of a workgroup
  N = 32        one full slab
  N = 33        2 slabs, the last of 1 row        (fewer slabs than the four waves of the two finalize kernels: empty waves)
  N = 96        3 full slabs                      (one empty wave)
  N = 97        4 slabs, the last of 1 row
  N = 195       7 slabs, the last of 3 rows       (slab count no multiple of 4)
  (16421, 8)    slab_rows = 33, 498 slabs, the last of 20 rows
  (8200, 260)   two 256-column tiles: 256 slabs wanted, slab_rows = 33, 249 slabs, the last of 16 rows
Column form: C = 1, 3, 63, 65 take VEC = 1 by their width (64 columns per tile: the edges 63 | 65; C = 64 itself is a multiple of
4 and fills a VEC = 1 tile exactly only in the misaligned cells below); C = 4, 64, 252, 256, 260 take VEC = 4 (256 columns per
tile: 252 | 256 | 260; the finalize kernels always take 64 columns per workgroup, C = 260 leaves one with four live lanes). For
C = 4, 64 and 260 the row tensors are ALSO placed 4 bytes into a larger allocation -- what a contiguous
view at an odd offset is -- in the four alignment cells
  aligned            forward VEC = 4, backward VEC = 4
  y                  y off: both passes VEC = 1
  residual           only the residual off: forward VEC = 1, backward VEC = 4
  g_z                only the upstream gradient off: forward VEC = 4, backward VEC = 1
  all                every row tensor off (the cross-form checks)
and ``data_ptr() % 16`` of every row tensor is asserted in front of each call.

Bound: the project's 1e-4, PER COLUMN: max_r |got - ref| <= 1e-4 max_r |ref[:, c]| for z, dy and d residual, so that a wrong column
of small values cannot hide behind the largest column; the columns' standard deviations are log-uniform in [1e-2, 1e2], their means
up to 10 standard deviations either side, gamma in [0.5, 1.5]. The per-column vectors (d gamma, d beta, mean, rstd, the running
statistics) are judged per element against 1e-4 |ref|. An absolute floor is used ONLY where the reference element is itself a
cancellation -- a sum of terms of both signs: d gamma = sum g xh, d beta = sum g, a batch mean next to 0, the momentum blend of
the running mean -- namely 1e-4 of 1 % of the sum of the terms' magnitudes (an element smaller than that has lost two digits to
the cancellation in ANY fp32 evaluation); rstd and the running variance are sums of positive terms and get none. For N <= 3,
dy = gamma rstd (g - mean g - xh mean(g xh)) cancels to ~0 (N = 2: exactly) and is judged against 1 % of gamma rstd max |g| of its
column, as in tests/test_baseline_3d_pose_gpu.py. Where the fp64 pre-activation lies within 1e-5 of its maximum of 0 the ReLU
gate of an fp32 kernel is a coin toss: the upstream gradient is zero there (same file).
Every case also evaluates fp32 ``torch.nn.functional.batch_norm`` on the CPU against the fp64 twin and asserts that it stays under
1e-5 by the same per-column measure: a failure is then the kernel's and not the case's (``test_cases_are_well_conditioned``
does that for every case without a GPU). Where dropout is on, the reference uses the kernel's own keep mask, read off a forward
with a large beta.

Cross-form checks (no tolerance): the aligned and the all-misaligned run give bitwise equal z, mean, rstd and running statistics,
with p = 0.5 the same keep pattern; in eval mode the backward's recomputed ReLU gate is the forward's in both mixed cells.
Flags: relu = 0; eval-mode backward with a residual; accumulate = 1 (ABI and ``ops.grad_sinks``); parameters and statistics at
unaligned offsets of one flat buffer with guard words; p = 1 and p = 0 with a state; two training calls on one module; a
zero-variance column; a column of magnitude 4e19 with empty finalize waves.

Each GPU test prints the worst per-column ratio of every tensor it compares (``pytest -s``); the largest seen are in DESIGN.md.
"""
import ctypes
import functools

import pytest
import torch

BOUND, GUARD = 1e-4, 1e-5
EPS, MOMENTUM = 1e-5, 0.1
TARGET_BLOCKS, MIN_SLAB_ROWS = 512, 32          # p2c_bnorm.hip
GUARD_WORD = 123.25
ROW_TENSORS = ('y', 'z', 'residual', 'g_z', 'g_y')


# ======================================================================================================================
# the dispatch, mirrored
# ======================================================================================================================
def slab_rows_for(N, C):
    want = max(TARGET_BLOCKS // -(-C // 256), 1)
    return max(MIN_SLAB_ROWS, -(-N // want))


def row_plan(N, C):
    """(slab_rows, slabs, rows of the last slab)"""
    rows = slab_rows_for(N, C)
    slabs = -(-N // rows)
    return rows, slabs, N - (slabs - 1) * rows


def workspace_floats(N, C):
    return 2 * row_plan(N, C)[1] * C + 2 * C


# the cell table: N -> (slab_rows, slabs, rows of the last slab) for any C of the column table ...
ROW_CELLS = {2: (32, 1, 2), 5: (32, 1, 5), 32: (32, 1, 32), 33: (32, 2, 1), 96: (32, 3, 32), 97: (32, 4, 1), 195: (32, 7, 3)}
# ... and the two shapes with slab_rows > 32 and a ragged last slab
BIG_CELLS = {(16421, 8): (33, 498, 20), (8200, 260): (33, 249, 16)}
VEC1_C, VEC4_C = (1, 3, 63, 65), (4, 64, 252, 256, 260)
# every N and every C at least once; VEC = 1 and VEC = 4 at every N
CELLS = [(2, 63), (2, 256), (5, 65), (5, 4), (32, 1), (32, 252), (33, 64), (33, 65), (96, 3), (96, 256), (97, 65), (97, 4),
         (195, 63), (195, 260), (16421, 8), (8200, 260)]
ALIGN_C = (4, 64, 260)
ALIGN_N = 97
# alignment cell -> (row tensors placed 4 bytes off, forward VEC, backward VEC) for C % 4 == 0
ALIGN_CELLS = {'aligned': ((), 4, 4), 'y': (('y',), 1, 1), 'residual': (('residual',), 1, 4), 'g_z': (('g_z',), 4, 1),
               'all': (ROW_TENSORS, 1, 1)}


def expected_plan(N, C):
    return BIG_CELLS[(N, C)] if (N, C) in BIG_CELLS else ROW_CELLS[N]


def test_row_plan_mirror_and_cell_coverage():
    for (N, C) in CELLS + [(ALIGN_N, c) for c in ALIGN_C]:
        assert row_plan(N, C) == expected_plan(N, C), (N, C, row_plan(N, C))
        assert N * C <= 2_200_000
    assert {n for n, _ in CELLS} >= set(ROW_CELLS) and set(BIG_CELLS) <= set(CELLS)
    assert {c for _, c in CELLS} >= set(VEC1_C) | set(VEC4_C)
    assert all(c % 4 for c in VEC1_C) and not any(c % 4 for c in VEC4_C + ALIGN_C)
    for n in ROW_CELLS:                                   # both column forms at every row plan
        assert {c % 4 == 0 for m, c in CELLS if m == n} == {True, False}, n
    # hand-computed: the reference shape of the existing suite, and the first N that leaves 32-row slabs at one column tile
    assert row_plan(65536, 1024) == (512, 128, 512) and row_plan(16384, 8) == (32, 512, 32) and row_plan(16385, 8)[0] == 33


# ======================================================================================================================
# cases (CPU, fp64 holding fp32-representable numbers) and their references
# ======================================================================================================================
class Case:
    pass


@functools.lru_cache(maxsize=None)
def make_case(N, C, seed=0, beta_scale=0.5, residual=True, const_col=None, zero_residual=False, dense_g=False):
    g = torch.Generator().manual_seed(1000 * seed + 7 * N + C)
    f = lambda t: t.float().double()   # noqa: E731  (inputs rounded to fp32 first: the twin sees exactly what the kernel sees)
    c = Case()
    c.N, c.C = N, C
    c.std = 10.0 ** (torch.rand(C, generator=g, dtype=torch.float64) * 4 - 2)
    # means up to 10 standard deviations either side; up to 1 for N <= 3, where dy is judged against 1 % of its terms: an fp32
    # rounding of xh at mean / std = 10 is 6e-7 of the terms, 6e-5 by that measure, and the fp32 framework misses the guard
    cap = 10.0 if N > 3 else 1.0
    c.mu = (torch.rand(C, generator=g, dtype=torch.float64) * 2 - 1) * cap * c.std
    # (the draws standardised per column: mean and standard deviation are the BATCH's -- at N = 2 two draws 0.1 apart around a
    # mean of 10 would be a column of mean / std = 200, which the fp32 framework itself misses by 1e-4)
    xi = torch.randn(N, C, generator=g, dtype=torch.float64)
    xi = (xi - xi.mean(0)) / xi.std(0, unbiased=False)
    c.y = f(c.mu + c.std * xi)
    c.gamma = f(torch.rand(C, generator=g, dtype=torch.float64) + 0.5)
    c.beta = f(torch.randn(C, generator=g, dtype=torch.float64) * beta_scale)
    if N <= 3:          # xh is +-1 (N = 2): with beta next to -gamma the whole column of z is a cancellation; beta >= 0 keeps it O(1)
        c.beta = c.beta.abs()
    # running statistics near the columns' own (an eval forward stays O(1) per column)
    c.rm = f(c.mu + 0.3 * c.std * torch.randn(C, generator=g, dtype=torch.float64))
    c.rv = f(c.std ** 2 * (torch.rand(C, generator=g, dtype=torch.float64) + 0.5))
    c.residual = f(torch.randn(N, C, generator=g, dtype=torch.float64)) if residual else None
    if zero_residual:
        c.residual = torch.zeros(N, C, dtype=torch.float64)
    c.g_z = f(torch.randn(N, C, generator=g, dtype=torch.float64))
    if dense_g:                                          # no element near 0: dy != 0 wherever the gate is open
        c.g_z = f(torch.where(c.g_z < 0, c.g_z - 0.5, c.g_z + 0.5))
    if const_col is not None:
        c.y[:, const_col] = 3.0
        c.beta[const_col] = c.beta[const_col].abs() + 0.125          # relu(beta) > 0: the column's bound is not vacuous
    return c


def _twin(c, training, relu, keep, p, dtype, g_z=None, calls=1):
    """BatchNorm1d -> ReLU -> dropout with the given keep mask -> + residual on the CPU in ``dtype``; fp64 through the module,
    fp32 through torch.nn.functional.batch_norm. ``calls``: that many forwards on the same module (running statistics)."""
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)   # noqa: E731  (the case's own tensors stay as they are)
    y = leaf(c.y)
    res = None if c.residual is None else leaf(c.residual)
    if dtype == torch.float64:
        bn = torch.nn.BatchNorm1d(c.C, eps=EPS, momentum=MOMENTUM).double()
        with torch.no_grad():
            bn.weight.copy_(c.gamma), bn.bias.copy_(c.beta), bn.running_mean.copy_(c.rm), bn.running_var.copy_(c.rv)
        bn.train(training)
        w, b, rm, rv = bn.weight, bn.bias, bn.running_mean, bn.running_var
        for _ in range(calls):
            pre = bn(y)
        nbt = int(bn.num_batches_tracked)
    else:
        w, b = leaf(c.gamma), leaf(c.beta)
        rm, rv, nbt = c.rm.to(dtype).clone(), c.rv.to(dtype).clone(), calls if training else 0
        for _ in range(calls):
            pre = torch.nn.functional.batch_norm(y, rm, rv, w, b, training, MOMENTUM, EPS)
    act = torch.relu(pre) if relu else pre
    if keep is not None:
        act = act * keep.to(dtype) * (0.0 if p >= 1 else 1.0 / (1.0 - p))
    z = act if res is None else act + res
    if g_z is None:
        g_z = c.g_z.clone()
        if relu:
            pd = pre.detach()
            g_z[pd.abs() < 1e-5 * pd.abs().max()] = 0.0
    z.backward(g_z.to(dtype))
    o = Case()
    o.z, o.dy, o.dgamma, o.dbeta, o.g_z = z.detach(), y.grad, w.grad, b.grad, g_z
    o.dres = None if res is None else res.grad
    o.rm, o.rv, o.nbt, o.pre = rm.detach().clone(), rv.detach().clone(), nbt, pre.detach()
    return o


def col_ratio(got, ref, floor=None):
    """worst over the columns of max_r |got - ref| / max(max_r |ref[:, c]|, floor[c]); a column whose reference (and floor) is
    all zero must match exactly."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), 'not finite'
    err, scale = (got - ref).abs().amax(0), ref.abs().amax(0)
    if floor is not None:
        scale = torch.maximum(scale, floor)
    ratio = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float('inf')), err))
    return float(ratio.max())


def vec_ratio(got, ref, terms=None):
    """worst over the elements of |got - ref| / max(|ref|, 1e-2 terms): ``terms`` is the sum of the magnitudes of the signed
    terms the reference element is the sum of (None: a sum of positive terms, no floor)."""
    return col_ratio(got.reshape(1, -1), ref.reshape(1, -1), None if terms is None else 1e-2 * terms.reshape(-1))


def reference(c, training, relu=True, keep=None, p=0.0, calls=1, check_guard=True, z_guard_without=None):
    """The fp64 twin of one case with everything the comparisons need, and the guard: the fp32 framework on the same inputs stays
    within GUARD of it by the per-column measure (z, dy)."""
    r = _twin(c, training, relu, keep, p, torch.float64, calls=calls)
    y, N = c.y, c.N
    if training:
        r.mean, var = y.mean(0), y.var(0, unbiased=False)
    else:
        r.mean, var = c.rm.clone(), c.rv.clone()
    r.rstd = (var + EPS).rsqrt()
    xh = (y - r.mean) * r.rstd
    g = r.g_z.clone()
    if keep is not None:
        g = g * keep.double() * (0.0 if p >= 1 else 1.0 / (1.0 - p))
    if relu:
        g = g * (r.pre > 0)
    # sums of the magnitudes of the signed terms (the cancellation floors of vec_ratio)
    r.t_dgamma, r.t_dbeta, r.t_mean = (g * xh).abs().sum(0), g.abs().sum(0), y.abs().mean(0)
    r.t_rm = (1 - MOMENTUM) * c.rm.abs() + MOMENTUM * y.abs().mean(0)
    # N <= 3: dy is a cancellation of terms of size gamma rstd |g|
    r.dy_floor = None
    if training and N <= 3:                 # the floor of tests/test_baseline_3d_pose_gpu.py as it stands there: one number
        r.dy_floor = torch.full((c.C,), 1e-2 * float((c.gamma * r.rstd).max()) * float(r.g_z.abs().max()), dtype=torch.float64)
    if not training:
        # eval statistics are constants: dy = gamma rstd g (the written-out formula next to autograd's)
        assert col_ratio(c.gamma * r.rstd * g, r.dy) <= 1e-12
    if check_guard:
        f = _twin(c, training, relu, keep, p, torch.float32, g_z=r.g_z, calls=calls)
        cols = [k for k in range(c.C) if k != z_guard_without]       # (test_zero_variance_column says why one may be left out)
        r.guard = dict(z=col_ratio(f.z[:, cols], r.z[:, cols]), dy=col_ratio(f.dy, r.dy, r.dy_floor))
        assert max(r.guard.values()) <= GUARD, ('the case is ill-conditioned for fp32', c.N, c.C, training, r.guard)
    return r


@functools.lru_cache(maxsize=None)
def cell_reference(N, C, training, residual):
    """the reference of a table cell, computed once and shared (never modified) by the tests that run the cell"""
    c = make_case(N, C, residual=residual)
    return c, reference(c, training)


def _has_residual(N, C):
    return (N + C) % 2 == 1 or (N, C) in BIG_CELLS


def test_cases_are_well_conditioned():
    """Without a GPU: the fp32 framework BatchNorm stays within 1e-5 (per column) of the fp64 twin for every case of the tables
    (``reference`` asserts it), in training and in eval mode."""
    worst = dict(z=0.0, dy=0.0)
    for training in (True, False):
        for (N, C) in CELLS:
            _, r = cell_reference(N, C, training, _has_residual(N, C))
            worst = {k: max(worst[k], r.guard[k]) for k in worst}
        for C in ALIGN_C:
            _, r = cell_reference(ALIGN_N, C, training, True)
            worst = {k: max(worst[k], r.guard[k]) for k in worst}
    print('fp32 framework vs fp64 twin, worst per-column ratio:', worst)


# ======================================================================================================================
# GPU: the C ABI
# ======================================================================================================================
def _dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def _lib():
    from pedestrians_video_2_carla_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Placed:
    """A contiguous fp32 device tensor inside a larger allocation filled with guard words, 16-byte aligned or 4 bytes past."""

    def __init__(self, shape, off, fill=None, pad=8):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + pad,), GUARD_WORD, device=_dev())
        assert self.buf.data_ptr() % 16 == 0
        self.off, self.n = off, n
        self.t = self.buf[off:off + n].view(*shape)
        if torch.is_tensor(fill):
            self.t.copy_(fill.float())
        elif fill is not None:
            self.t.fill_(float(fill))
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 4 * off

    def guards_intact(self):
        return bool((self.buf[:self.off] == GUARD_WORD).all()) and bool((self.buf[self.off + self.n:] == GUARD_WORD).all())


def _flat(vectors, offsets_odd=True):
    """The vectors as views of ONE flat buffer, each at an offset that is a multiple of 4 bytes but not of 16, one guard word
    at least between neighbours."""
    sizes = [v.numel() for v in vectors]
    offs, o = [], 1
    for s in sizes:
        while o % 4 == 0:
            o += 1
        offs.append(o)
        o += s + 1
    buf = torch.full((o + 4,), GUARD_WORD, device=_dev())
    assert buf.data_ptr() % 16 == 0
    views = []
    for v, a in zip(vectors, offs):
        t = buf[a:a + v.numel()]
        t.copy_(v.float())
        assert t.data_ptr() % 16 != 0 and t.data_ptr() % 4 == 0
        views.append(t)
    mask = torch.ones_like(buf, dtype=torch.bool)
    for a, s in zip(offs, sizes):
        mask[a:a + s] = False
    return buf, views, mask


def run_abi(c, training, relu=True, mis=(), p=0.0, state=None, site=0, accumulate=False, g_z=None, grads0=None,
            flat_params=False, backward=True, expect_vec=None, residual=True):
    """One p2c_bnorm_fwd (+ p2c_bnorm_bwd) on the case: the row tensors named in ``mis`` start 4 bytes into their allocation.
    Everything that is written starts as NaN (mean, rstd, the workspace) or between guard words (z, g_y)."""
    lib, d = _lib(), _dev()
    N, C = c.N, c.C
    assert lib.p2c_bnorm_workspace_floats(N, C) == workspace_floats(N, C) == 2 * expected_plan(N, C)[1] * C + 2 * C
    off = {k: int(k in mis) for k in ROW_TENSORS}
    has_res = residual and c.residual is not None
    y, z = Placed((N, C), off['y'], c.y), Placed((N, C), off['z'], float('nan'))
    res = Placed((N, C), off['residual'], c.residual) if has_res else None
    gz = Placed((N, C), off['g_z'], c.g_z if g_z is None else g_z)
    gy = Placed((N, C), off['g_y'], float('nan'))
    # what the host code will pick (asserted, so that a cell is the cell its name says)
    fwd_vec = 4 if (C % 4 == 0 and not (off['y'] or off['z'] or (has_res and off['residual']))) else 1
    bwd_vec = 4 if (C % 4 == 0 and not (off['y'] or off['g_z'] or off['g_y'])) else 1
    for t, k in ((y, 'y'), (z, 'z'), (res, 'residual'), (gz, 'g_z'), (gy, 'g_y')):
        assert t is None or t.t.data_ptr() % 16 == 4 * off[k]
    if expect_vec is not None:
        assert (fwd_vec, bwd_vec) == tuple(expect_vec), (fwd_vec, bwd_vec, expect_vec)
    g0 = [torch.zeros(C, dtype=torch.float64)] * 2 if grads0 is None else grads0
    if flat_params:
        pbuf, (gamma, beta, rm, rv), pmask = _flat([c.gamma, c.beta, c.rm, c.rv])
        nan = torch.full((C,), float('nan'))
        sbuf, (mean, rstd, gg, gb), smask = _flat([nan, nan, g0[0], g0[1]])
    else:
        gamma, beta, rm, rv = (t.float().to(d) for t in (c.gamma, c.beta, c.rm, c.rv))
        mean, rstd = torch.full((C,), float('nan'), device=d), torch.full((C,), float('nan'), device=d)
        gg, gb = g0[0].float().to(d), g0[1].float().to(d)
    ds = _lib_desc()
    ds.N, ds.C, ds.training, ds.relu, ds.accumulate, ds.eps, ds.momentum = N, C, int(training), int(relu), int(accumulate), EPS, MOMENTUM
    ds.y, ds.gamma, ds.beta, ds.residual = y.t.data_ptr(), gamma.data_ptr(), beta.data_ptr(), (res.t.data_ptr() if has_res else None)
    ds.z, ds.mean, ds.rstd, ds.running_mean, ds.running_var = z.t.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rm.data_ptr(), rv.data_ptr()
    ds.g_z, ds.g_y, ds.g_gamma, ds.g_beta = gz.t.data_ptr(), gy.t.data_ptr(), gg.data_ptr(), gb.data_ptr()
    ds.drop_state, ds.drop_p, ds.drop_site = (None if state is None else state.data_ptr()), float(p), int(site)
    ws = torch.full((workspace_floats(N, C),), float('nan'), device=d)
    assert lib.p2c_bnorm_fwd(ctypes.byref(ds), ws.data_ptr(), _stream()) == 0
    if backward:
        ws2 = torch.full((workspace_floats(N, C),), float('nan'), device=d)      # (ops allocates a fresh one too)
        assert lib.p2c_bnorm_bwd(ctypes.byref(ds), ws2.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    o = Case()
    o.z, o.mean, o.rstd, o.rm, o.rv = z.t.clone(), mean.clone(), rstd.clone(), rm.clone(), rv.clone()
    o.dy, o.dgamma, o.dbeta = gy.t.clone(), gg.clone(), gb.clone()
    assert all(t.guards_intact() for t in (y, z, gz, gy) + ((res,) if has_res else ())), 'a write outside a row tensor'
    assert torch.equal(y.t.cpu().double(), c.y) and (not has_res or torch.equal(res.t.cpu().double(), c.residual)), 'an input was written'
    if flat_params:
        assert bool((pbuf[pmask] == GUARD_WORD).all()) and bool((sbuf[smask] == GUARD_WORD).all()), 'a write between the flat views'
        assert torch.equal(gamma.cpu().double(), c.gamma) and torch.equal(beta.cpu().double(), c.beta)
    return o


def _lib_desc():
    from pedestrians_video_2_carla_amd import _lib as L
    return L.BnormDesc()


def compare(what, c, r, o, training, backward=True, grads0=None, stats=True):
    """Every output of one run against the reference: per column for the (N, C) tensors, per element for the vectors. Prints the
    ratios (1.0 = at the bound of 1e-4) and asserts them."""
    figs = dict(z=col_ratio(o.z, r.z))
    if stats:
        figs['mean'] = vec_ratio(o.mean, r.mean, r.t_mean if training else None)
        figs['rstd'] = vec_ratio(o.rstd, r.rstd)
        figs['running_mean'] = vec_ratio(o.rm, r.rm, r.t_rm if training else None)
        figs['running_var'] = vec_ratio(o.rv, r.rv)
    if backward:
        a0, b0 = (torch.zeros(c.C, dtype=torch.float64),) * 2 if grads0 is None else grads0
        figs['dy'] = col_ratio(o.dy, r.dy, r.dy_floor)
        figs['dgamma'] = vec_ratio(o.dgamma, r.dgamma + a0, r.t_dgamma + a0.abs())
        figs['dbeta'] = vec_ratio(o.dbeta, r.dbeta + b0, r.t_dbeta + b0.abs())
    print(what, ' '.join('{}={:.3e}'.format(k, v) for k, v in figs.items()))
    bad = {k: v for k, v in figs.items() if not v <= BOUND}
    assert not bad, (what, 'beyond 1e-4 per column / element', bad, figs)
    if not training and stats:
        assert torch.equal(o.mean.cpu().double(), c.rm), 'eval: mean must hold the running mean, every column'
        assert torch.equal(o.rm.cpu().double(), c.rm) and torch.equal(o.rv.cpu().double(), c.rv), 'eval changed the running statistics'
    return figs


def _mode(training):
    return 'train' if training else 'eval'


@pytest.mark.gpu
@pytest.mark.parametrize('training', [True, False], ids=_mode)
@pytest.mark.parametrize('N,C', CELLS, ids=['{}x{}'.format(*s) for s in CELLS])
def test_every_row_plan_and_column_form_matches_fp64(N, C, training):
    """Every row of the cell table, aligned tensors, with a residual in about half of them: z, mean, rstd, the running
    statistics, dy, d gamma and d beta (d residual is the upstream gradient itself) within 1e-4 per column / element."""
    c, r = cell_reference(N, C, training, _has_residual(N, C))
    vec = 4 if C % 4 == 0 else 1
    o = run_abi(c, training, g_z=r.g_z, expect_vec=(vec, vec))
    compare('cell {}x{} {}'.format(N, C, _mode(training)), c, r, o, training)


@pytest.mark.gpu
@pytest.mark.parametrize('training', [True, False], ids=_mode)
@pytest.mark.parametrize('cell', ['aligned', 'y', 'residual', 'g_z'])
@pytest.mark.parametrize('C', ALIGN_C)
def test_every_alignment_cell_matches_fp64(C, cell, training):
    """C % 4 == 0 with row tensors 4 bytes into a larger allocation: the VEC = 1 branch taken for the pointer alone, and the
    two mixed cells where forward and backward run different instantiations."""
    c, r = cell_reference(ALIGN_N, C, training, True)
    mis, fv, bv = ALIGN_CELLS[cell]
    o = run_abi(c, training, g_z=r.g_z, mis=mis, expect_vec=(fv, bv))
    compare('align {} C={} {}'.format(cell, C, _mode(training)), c, r, o, training)


def _ops_run(c, training, mis, g_z, relu=True, p=0.0, state=None, site=0, sinks=False, grads0=None):
    """the case through ops.batch_norm_act on a BatchNorm1d module; the tensors named in ``mis`` are views at an odd offset"""
    from pedestrians_video_2_carla_amd import ops
    d = _dev()
    bn = torch.nn.BatchNorm1d(c.C, eps=EPS, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(c.gamma), bn.bias.copy_(c.beta), bn.running_mean.copy_(c.rm), bn.running_var.copy_(c.rv)
    bn = bn.to(d).train(training)
    y = Placed((c.N, c.C), int('y' in mis), c.y).t.requires_grad_(True)
    res = None if c.residual is None else Placed((c.N, c.C), int('residual' in mis), c.residual).t.requires_grad_(True)
    gz = Placed((c.N, c.C), int('g_z' in mis), g_z).t
    if grads0 is not None:
        bn.weight.grad, bn.bias.grad = grads0[0].float().to(d), grads0[1].float().to(d)
    with ops.grad_sinks(sinks):
        z = ops.batch_norm_act(y, bn, p, state, site, residual=res, relu=relu)
        z.backward(gz)
    torch.cuda.synchronize()
    o = Case()
    o.z, o.dy, o.dgamma, o.dbeta = z.detach(), y.grad, bn.weight.grad, bn.bias.grad
    o.dres = None if res is None else res.grad
    o.rm, o.rv, o.nbt, o.bn = bn.running_mean, bn.running_var, int(bn.num_batches_tracked), bn
    return o


@pytest.mark.gpu
@pytest.mark.parametrize('cell', ['aligned', 'y', 'residual', 'g_z'])
def test_alignment_cells_through_ops(cell):
    """One run of each alignment cell through ops.batch_norm_act (C = 260, training): views at an odd offset as y, as the
    residual and as the gradient autograd hands over."""
    c, r = cell_reference(ALIGN_N, 260, True, True)
    o = _ops_run(c, True, ALIGN_CELLS[cell][0], r.g_z)
    figs = compare('ops align {}'.format(cell), c, r, o, True, stats=False)
    figs.update(running_mean=vec_ratio(o.rm, r.rm, r.t_rm), running_var=vec_ratio(o.rv, r.rv), dres=col_ratio(o.dres, r.dres))
    assert max(figs.values()) <= BOUND and o.nbt == 1, figs


# ======================================================================================================================
# cross-form checks
# ======================================================================================================================
def _state(seed=11):
    from pedestrians_video_2_carla_amd import ops
    torch.manual_seed(seed)
    return ops.dropout_state(_dev())


def kernel_keep_mask(N, C, p, state, site):
    """The keep mask the next training forward of (N, C) draws at ``site``: a forward with beta = 1000 (|xh| <= sqrt(N - 1) < 129:
    the ReLU is the identity, z == 0 exactly where an element was dropped); the state is put back."""
    snap = state.clone()
    probe = Case()
    probe.N, probe.C = N, C
    g = torch.Generator().manual_seed(N + C)
    probe.y = torch.randn(N, C, generator=g).double()
    probe.gamma, probe.beta = torch.ones(C, dtype=torch.float64), torch.full((C,), 1000.0, dtype=torch.float64)
    probe.rm, probe.rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    probe.residual, probe.g_z = None, torch.zeros(N, C, dtype=torch.float64)
    z = run_abi(probe, True, p=p, state=state, site=site, backward=False).z
    state.copy_(snap)
    return (z != 0).cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('p', [0.0, 0.5])
@pytest.mark.parametrize('N,C', [(ALIGN_N, 4), (195, 64), (ALIGN_N, 260)])
def test_aligned_and_misaligned_forms_agree_bitwise(N, C, p):
    """Same data, same dropout state: the VEC = 4 run and the VEC = 1 run (every row tensor 4 bytes off) give the same bits in
    z, mean, rstd and the running statistics -- explicit fma, one summation order per column whatever the form -- and with
    p = 0.5 the same keep pattern (element index r C + c in both forms)."""
    c = make_case(N, C)
    state = _state() if p else None
    keep = kernel_keep_mask(N, C, p, state, 2).to(_dev()) if p else None
    assert keep is None or 0.4 < float(keep.float().mean()) < 0.6
    snap = None if state is None else state.clone()
    runs = []
    for cell in ('aligned', 'all'):
        if state is not None:
            state.copy_(snap)
        mis, fv, bv = ALIGN_CELLS[cell]
        runs.append(run_abi(c, True, mis=mis, p=p, state=state, site=2, expect_vec=(fv, bv)))
    a, b = runs
    for k in ('z', 'mean', 'rstd', 'rm', 'rv'):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    if p:
        # the pattern itself, in both forms, against the mask of a probe forward: a dropped element is the residual exactly, a
        # kept one differs from it wherever the ReLU is open (more than half of the kept ones)
        res = c.residual.float().to(_dev())
        for o in runs:
            changed = o.z != res
            assert not bool((changed & ~keep).any()) and float(changed[keep].float().mean()) > 0.3


@pytest.mark.gpu
@pytest.mark.parametrize('cell', ['residual', 'g_z'])
@pytest.mark.parametrize('C', ALIGN_C)
def test_mixed_forms_recompute_the_forward_gate_in_eval(C, cell):
    """Eval mode, both mixed cells: (dy != 0) == (z - residual > 0) element for element -- the backward's recomputed gate is the
    forward's across the two instantiations. beta near 0: about half the gates are closed; the residual is all zeros (z - residual
    is then z exactly; it still travels as a misaligned pointer) and no upstream gradient is near 0."""
    c = make_case(ALIGN_N, C, seed=3, beta_scale=0.1, zero_residual=True, dense_g=True)
    mis, fv, bv = ALIGN_CELLS[cell]
    o = run_abi(c, False, mis=mis, expect_vec=(fv, bv))
    gate_f, gate_b = o.z > 0, o.dy != 0
    assert 0.3 < float(gate_f.float().mean()) < 0.7
    assert torch.equal(gate_f, gate_b), int((gate_f != gate_b).sum())


@pytest.mark.gpu
@pytest.mark.parametrize('cell', ['residual', 'g_z'])
@pytest.mark.parametrize('C', ALIGN_C)
def test_mixed_forms_use_the_forward_mask_in_training(C, cell):
    """Training with p = 0.5, both mixed cells: z, dy, d gamma and d beta match the fp64 twin under the forward's keep mask."""
    c = make_case(ALIGN_N, C, seed=4)
    state = _state(12)
    keep = kernel_keep_mask(c.N, C, 0.5, state, 5)
    assert 0.4 < float(keep.float().mean()) < 0.6
    r = reference(c, True, keep=keep, p=0.5)
    mis, fv, bv = ALIGN_CELLS[cell]
    o = run_abi(c, True, mis=mis, p=0.5, state=state, site=5, g_z=r.g_z, expect_vec=(fv, bv))
    compare('mixed {} C={} p=0.5'.format(cell, C), c, r, o, True)


# ======================================================================================================================
# flags
# ======================================================================================================================
FLAG_SHAPES = [(195, 63), (ALIGN_N, 260)]         # a ragged VEC = 1 shape and a VEC = 4 shape with a second column tile


@pytest.mark.gpu
@pytest.mark.parametrize('residual', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('training', [True, False], ids=_mode)
@pytest.mark.parametrize('N,C', FLAG_SHAPES)
def test_relu_off_matches_fp64(N, C, training, residual):
    c = make_case(N, C, seed=5, residual=residual)
    r = reference(c, training, relu=False)
    o = run_abi(c, training, relu=False, g_z=r.g_z)
    compare('relu=0 {}x{} {} res={}'.format(N, C, _mode(training), residual), c, r, o, training)


@pytest.mark.gpu
@pytest.mark.parametrize('N,C', FLAG_SHAPES + [(33, 65)])
def test_eval_backward_with_a_residual(N, C):
    """Eval mode with a residual: dy = gamma rstd g (``reference`` checks autograd against that formula), d gamma and d beta
    against autograd of the fp64 eval module, d residual through ops; mean / rstd hold the running statistics in EVERY column
    after the eval forward (only slab 0's tiles write them; they start as NaN here)."""
    c = make_case(N, C, seed=6)
    r = reference(c, False)
    o = run_abi(c, False, g_z=r.g_z)
    compare('eval backward {}x{}'.format(N, C), c, r, o, False)
    o2 = _ops_run(c, False, (), r.g_z)
    figs = dict(dy=col_ratio(o2.dy, r.dy), dres=col_ratio(o2.dres, r.dres), dgamma=vec_ratio(o2.dgamma, r.dgamma, r.t_dgamma),
                dbeta=vec_ratio(o2.dbeta, r.dbeta, r.t_dbeta))
    assert max(figs.values()) <= BOUND and o2.nbt == 0, figs


@pytest.mark.gpu
@pytest.mark.parametrize('training', [True, False], ids=_mode)
@pytest.mark.parametrize('N,C', FLAG_SHAPES)
def test_accumulate_adds_to_existing_gradients(N, C, training):
    """accumulate = 1: g_gamma / g_beta end as what they held + the gradient (through the ABI, and through ops inside
    ``grad_sinks`` with .grad set); accumulate = 0 overwrites what they held."""
    c = make_case(N, C, seed=7)
    r = reference(c, training)
    g = torch.Generator().manual_seed(N)
    grads0 = [(torch.randn(C, generator=g) * 3).double(), (torch.randn(C, generator=g) * 3).double()]
    o = run_abi(c, training, g_z=r.g_z, accumulate=True, grads0=grads0)
    compare('accumulate abi {}x{} {}'.format(N, C, _mode(training)), c, r, o, training, grads0=grads0)
    o = run_abi(c, training, g_z=r.g_z, accumulate=False, grads0=grads0)
    compare('overwrite abi {}x{} {}'.format(N, C, _mode(training)), c, r, o, training)
    o = _ops_run(c, training, (), r.g_z, sinks=True, grads0=grads0)
    compare('accumulate sinks {}x{} {}'.format(N, C, _mode(training)), c, r, o, training, grads0=grads0, stats=False)


@pytest.mark.gpu
@pytest.mark.parametrize('training', [True, False], ids=_mode)
@pytest.mark.parametrize('N,C', FLAG_SHAPES + [(33, 4)])
def test_parameters_at_unaligned_offsets_of_a_flat_buffer(N, C, training):
    """gamma, beta, the running statistics (and mean, rstd, g_gamma, g_beta) as views at 4-byte offsets that are no multiple of
    16 inside one flat buffer each: same results, and the words between the views are untouched (``run_abi`` asserts both)."""
    c = make_case(N, C, seed=8)
    r = reference(c, training)
    o = run_abi(c, training, g_z=r.g_z, flat_params=True)
    compare('flat parameters {}x{} {}'.format(N, C, _mode(training)), c, r, o, training)


@pytest.mark.gpu
@pytest.mark.parametrize('residual', [True, False], ids=['res', 'nores'])
@pytest.mark.parametrize('N,C', FLAG_SHAPES)
def test_dropout_p_one_and_p_zero(N, C, residual):
    """p = 1: z is the residual (or 0) and dy, d gamma, d beta are exactly zero, like nn.Dropout(1.0); the statistics are the
    batch's all the same. p = 0 with a state given: nothing is dropped -- the bits of the run without a state."""
    c = make_case(N, C, seed=9, residual=residual)
    r = reference(c, True)
    state = _state(13)
    o = run_abi(c, True, p=1.0, state=state, site=1, g_z=r.g_z)
    want = c.residual.float() if residual else torch.zeros(N, C)
    assert torch.equal(o.z.cpu(), want)
    assert not bool(o.dy.any()) and not bool(o.dgamma.any()) and not bool(o.dbeta.any())
    figs = dict(mean=vec_ratio(o.mean, r.mean, r.t_mean), rstd=vec_ratio(o.rstd, r.rstd), running_var=vec_ratio(o.rv, r.rv))
    assert max(figs.values()) <= BOUND, figs
    plain = run_abi(c, True, g_z=r.g_z)
    snap = state.clone()
    o = run_abi(c, True, p=0.0, state=state, site=1, g_z=r.g_z)
    for k in ('z', 'dy', 'dgamma', 'dbeta', 'mean', 'rstd', 'rm', 'rv'):
        assert torch.equal(getattr(o, k), getattr(plain, k)), k
    assert torch.equal(state, snap)
    compare('p=0 with a state {}x{}'.format(N, C), c, r, o, True)


@pytest.mark.gpu
@pytest.mark.parametrize('N,C', FLAG_SHAPES)
def test_two_training_calls_on_one_module(N, C):
    """Two consecutive training forwards through ops.batch_norm_act: the running statistics after the second match the fp64
    twin's and num_batches_tracked == 2."""
    from pedestrians_video_2_carla_amd import ops
    c = make_case(N, C, seed=10)
    r = reference(c, True, calls=2)
    d = _dev()
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(c.gamma), bn.bias.copy_(c.beta), bn.running_mean.copy_(c.rm), bn.running_var.copy_(c.rv)
    bn = bn.to(d).train()
    y, res = c.y.float().to(d), c.residual.float().to(d)
    for _ in range(2):
        z = ops.batch_norm_act(y, bn, 0.0, None, 0, residual=res)
    t_rm2 = (1 - MOMENTUM) * r.t_rm + MOMENTUM * c.y.abs().mean(0)
    figs = dict(z=col_ratio(z, r.z), running_mean=vec_ratio(bn.running_mean, r.rm, t_rm2), running_var=vec_ratio(bn.running_var, r.rv))
    print('two calls {}x{}'.format(N, C), figs)
    assert max(figs.values()) <= BOUND and int(bn.num_batches_tracked) == r.nbt == 2, figs


@pytest.mark.gpu
@pytest.mark.parametrize('residual', [False, True], ids=['nores', 'res'])
@pytest.mark.parametrize('training', [True, False], ids=_mode)
@pytest.mark.parametrize('N,C,col', [(195, 63, 17), (195, 256, 130)], ids=['195x63', '195x256'])
def test_zero_variance_column(N, C, col, training, residual):
    """One column of y constant at 3.0 among ordinary ones: fp64 gives z = relu(beta) = beta (+ residual) and, in training,
    rstd = 1 / sqrt(eps) for it. K19 forms the pre-activation as fma(y, a, fma(-mean, a, beta)), which rounds at the size of
    y gamma / sqrt(eps) ~ 1e3 (up to 6e-5 absolute), not at the size of beta; with the column's beta of 0.56 / 0.46 that is
    4e-5 of the column by an fp32 emulation on the host, inside the bound. The fp32 framework folds the mean into the offset the
    same way and is 2e-5 ... 4e-5 off the fp64 twin in this column when no residual lifts the column's scale: without a residual
    the guard on z leaves this one column out (the kernel is still held to 1e-4 there); with a residual it covers every column."""
    c = make_case(N, C, seed=11, residual=residual, const_col=col)
    if not training:                                         # (eval: the running statistics of the column are its own, 3 and 0)
        c = _with_column(c, col, c.y[:, col])
    r = reference(c, training, z_guard_without=None if residual else col)
    if training:
        assert float(r.rstd[col]) == pytest.approx(EPS ** -0.5, rel=1e-12)
    rest = r.z[:, col] - (c.residual[:, col] if residual else 0.0)
    assert float(c.beta[col]) > 0 and float((rest - c.beta[col]).abs().max()) < 1e-12
    o = run_abi(c, training, g_z=r.g_z)
    compare('zero variance {}x{} {} res={}'.format(N, C, _mode(training), residual), c, r, o, training)


@pytest.mark.gpu
@pytest.mark.parametrize('N,C', [(5, 3), (33, 65), (96, 4)])
def test_empty_finalize_waves_with_a_column_of_magnitude_4e19(N, C):
    """Fewer slabs than the four waves of K19b: an empty wave holds (n, mean, M2) = (0, 0, 0) and must be SKIPPED, not combined --
    combining it forms (0 - mean)^2 n_b / n, which is inf * 0 once mean^2 leaves fp32 (|mean| > 1.8e19). The same holds for a wave's
    FIRST slab, which meets the wave's own empty start: K19b combined it and returned rstd = NaN for this column at every shape
    until it took the first slab as it is (this test found that). Column 0 has mean 4e19
    and standard deviation 1e18 (squares of deviations stay below 3.4e38; mean / std = 40 is past the cap of the tables, so only
    the forward and the statistics are compared, at the usual bound, and the fp32 framework is not asked)."""
    c = make_case(N, C, seed=12, residual=False)
    g = torch.Generator().manual_seed(N)
    c = _with_column(c, 0, (4e19 + 1e18 * torch.randn(N, generator=g, dtype=torch.float64)).float().double())
    r = reference(c, True, check_guard=False)
    o = run_abi(c, True, g_z=r.g_z, backward=False)
    compare('4e19 column {}x{}'.format(N, C), c, r, o, True, backward=False)


def _with_column(c, col, values):
    """a copy of the case (the cached one is shared) with one column of y replaced"""
    n = Case()
    n.__dict__.update(c.__dict__)
    n.y = c.y.clone()
    n.y[:, col] = values
    n.rm, n.rv = c.rm.clone(), c.rv.clone()
    n.rm[col], n.rv[col] = values.mean().float().double(), values.var(unbiased=False).float().double()
    return n
