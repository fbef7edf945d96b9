"""GPU: every form of K16 (csrc/p2c_gemm.hip) through the C ABI, against fp64 and against each other.

The host picks one of the forward instantiations gemm_kernel<BN, TRANS_B, VEC, FAST> from the shape, the alignment and the
tile count, and one of gemm_tn_kernel<BN, VEC, FAST> plus a finish kernel for p2c_gemm_tn. The tests here fill the descriptor
themselves (``c_gemm`` / ``c_gemm_tn``), so real leading dimensions and offset bases reach the kernel, force the tile width
(P2C_GEMM_BN, P2C_GEMM_TN_BN) and the slice count (P2C_GEMM_TN_SLICES) in-process, and name the form each case runs in with a
mirror of the host dispatch (``fwd_form``, ``tn_form``, ``tn_finish``). ``test_the_case_tables_cover_every_cell`` fails when a
cell loses its cases. Cells and the tests that cover them:

  forward {BN 32, 64, 128} x {NT, NN} x {FAST, VEC, dword}   test_product_matches_fp64_in_every_form[bnB-TRANS-FORM-...]
                                                            test_epilogue_matches_fp64_in_every_form[bnB-actA-FORM]
                                                            test_act3_mask_is_the_same_in_every_form
                                                            test_every_tile_and_load_form_gives_the_same_bits
  TN {BN 32, 64, 128} x {FAST, VEC, dword} x {vec, vec8, scalar finish}
                                                            test_tn_every_tile_finish_and_load_form_gives_the_same_bits
BN = 128 is reached only through the variables (the production dispatch picks 32 or 64). The VEC forms at K % 32 == 0 (in
place of FAST) are checked by test_every_form_also_passes_with_the_fast_loads_off, which reruns this file with
P2C_GEMM_NO_FAST=1 (read once per process).

Tolerances are those of test_gemm_gpu.py: products 2e-6 sqrt(K) + 1e-7 relative to the max, epilogues 2e-5."""
import contextlib
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_ENUM = -1, -2, -3
BM, BK, OOB_OFF = 128, 32, 0x7fffff00
SENT = 0x5A5A5A5A                       # sentinel bits of untouched memory (a finite float: torch.equal holds for it)
NO_FAST = int(os.environ.get('P2C_GEMM_NO_FAST', '0') or 0) != 0


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def lib():
    from pedestrians_video_2_carla_amd import _lib
    return _lib.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def prod_tol(K):
    return 2e-6 * math.sqrt(K) + 1e-7


def gelu64(z):
    return 0.5 * z * (1 + torch.erf(z / math.sqrt(2.0)))


def gelu_grad64(z):
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


# ---------------------------------------------------------------------------------------------------------- placement / C ABI
def place(x, ld=None, off=0):
    """x (rows, cols) copied into a fresh buffer that holds the sentinel elsewhere: leading dimension ``ld`` (>= cols) and the
    first element ``off`` floats past a 512-byte aligned allocation (off 1 / 2: 4 / 8 bytes off 16-byte alignment). The result
    is a view with unit inner stride; ``untouched_outside`` checks the rest of its buffer."""
    rows, cols = x.shape
    ld = cols if ld is None else ld
    assert ld >= cols
    buf = torch.empty(off + (rows - 1) * ld + cols + 64, dtype=torch.float32, device=dev())
    buf.view(torch.int32).fill_(SENT)
    v = buf.as_strided((rows, cols), (ld, 1), off)
    v.copy_(x)
    return v


def untouched_outside(v):
    whole = v._base.clone()
    whole.as_strided(v.shape, v.stride(), v.storage_offset()).view(torch.int32).fill_(SENT)
    return bool((whole.view(torch.int32) == SENT).all())


def gemm_desc(a, b, trans_b, c, bias=None, act=0, aux=None, aux_out=None, row_scale=None, rows_per_scale=1, residual=None,
              drop_state=None, drop_p=0.0, drop_site=0):
    """p2c_gemm_desc from tensor views as they are: their strides are the leading dimensions, their data pointers the bases."""
    from pedestrians_video_2_carla_amd import _lib
    M, K = a.shape
    N = b.shape[0] if trans_b else b.shape[1]
    d = _lib.GemmDesc()
    d.M, d.N, d.K, d.trans_b = M, N, K, int(bool(trans_b))
    d.a, d.lda, d.b, d.ldb, d.c, d.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0)
    d.bias = None if bias is None else bias.data_ptr()
    d.act, d.rows_per_scale = act, rows_per_scale
    assert aux is None or aux_out is None or aux.stride(0) == aux_out.stride(0)
    d.aux, d.aux_out = (None if aux is None else aux.data_ptr()), (None if aux_out is None else aux_out.data_ptr())
    d.ldaux = aux.stride(0) if aux is not None else (aux_out.stride(0) if aux_out is not None else 0)
    d.row_scale = None if row_scale is None else row_scale.data_ptr()
    d.residual, d.ldr = (None, 0) if residual is None else (residual.data_ptr(), residual.stride(0))
    d.drop_state = None if drop_state is None else drop_state.data_ptr()
    d.drop_p, d.drop_site = drop_p, drop_site
    return d


def c_gemm(a, b, trans_b, c, over=None, **kw):
    """One p2c_gemm launch on views (``over``: descriptor fields set after the tensors', for the refusals); returns its code."""
    d = gemm_desc(a, b, trans_b, c, **kw)
    for k, v in (over or {}).items():
        setattr(d, k, v)
    return lib().p2c_gemm(ctypes.byref(d), _stream())


def c_gemm_tn(a, b, c, accumulate=0, row_scale=None, rows_per_scale=1, bias_out=None, ws=True, over=None):
    """One p2c_gemm_tn launch on views a (K, M), b (K, N), c (M, N) with a fresh workspace sized under the current variables."""
    K, M = a.shape
    N = b.shape[1]
    arg = dict(a=a.data_ptr(), lda=a.stride(0), b=b.data_ptr(), ldb=b.stride(0), c=c.data_ptr(), ldc=c.stride(0), M=M, N=N, K=K)
    arg.update(over or {})
    w = torch.empty(max(1, lib().p2c_gemm_tn_workspace_floats(arg['M'], arg['N'], arg['K'])), dtype=torch.float32, device=dev())
    return lib().p2c_gemm_tn(arg['a'], arg['lda'], arg['b'], arg['ldb'], arg['c'], arg['ldc'], arg['M'], arg['N'], arg['K'],
                             accumulate, None if row_scale is None else row_scale.data_ptr(), rows_per_scale,
                             None if bias_out is None else bias_out.data_ptr(), w.data_ptr() if ws else None, _stream())


@contextlib.contextmanager
def gemm_env(**values):
    """Set the tile / slice variables (None: unset) and have the library read them again; both are restored on exit."""
    saved = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        lib().p2c_gemm_reload_env()
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        lib().p2c_gemm_reload_env()


@pytest.fixture(params=[32, 64, 128], ids=lambda v: f'bn{v}')
def bn(request):
    with gemm_env(P2C_GEMM_BN=request.param):
        yield request.param


# --------------------------------------------------------------------------------------- mirror of the host dispatch (p2c_gemm.hip)
def fwd_bn(M, N, K, trans_b, env_bn=0):
    """Tile width of p2c_gemm (the bn choice in front of the launch)."""
    bn = 64 if N > 32 else 32
    if not trans_b and 256 <= K < 2048:
        bn = 32
    row_tiles = (M + BM - 1) // BM
    while bn > 32 and row_tiles * ((N + bn - 1) // bn) < 512:
        bn >>= 1
    if K <= 128:
        cand = bn >> 1
        while cand >= 32:
            if (N + cand - 1) // cand * cand < (N + bn - 1) // bn * bn:
                bn = cand
            cand >>= 1
    return env_bn if env_bn in (32, 64, 128) else bn


def fwd_form(M, N, K, trans_b, a_ptr, lda, b_ptr, ldb, no_fast=None):
    """Load form of gemm_kernel: 'FAST' (buffer loads), 'VEC' (16-byte loads) or 'dword'."""
    no_fast = NO_FAST if no_fast is None else no_fast
    vec = a_ptr % 16 == 0 and b_ptr % 16 == 0 and lda % 4 == 0 and ldb % 4 == 0 and K % 4 == 0 and (trans_b or N % 4 == 0)
    a_bytes = ((M - 1) * lda + K) * 4
    b_bytes = (((N - 1) * ldb + K) if trans_b else ((K - 1) * ldb + N)) * 4
    if vec and not no_fast and K % BK == 0 and a_bytes < OOB_OFF and b_bytes < OOB_OFF:
        return 'FAST'
    return 'VEC' if vec else 'dword'


def tn_bn(N, env_bn=0):
    return env_bn if env_bn in (32, 64, 128) else (64 if N > 32 else 32)


def tn_slices(M, N, K, env_bn=0, env_slices=0):
    bn = tn_bn(N, env_bn)
    tiles = ((M + BM - 1) // BM) * ((N + bn - 1) // bn)
    max_s = min(max(K // (16 * BK), 1), 1024)
    if env_slices >= 1:
        return min(env_slices, max_s)
    if tiles < 64:
        return min(max(1024 // tiles, 1), max_s)
    max_s = min(max_s, 64)
    step_cost = [0.0, 5.7e3, 5.7e3, 7.2e3, 9.4e3, 11.6e3]
    finish = 8.0 * M * N / 4.0e12 * 2.35e9
    best, best_cost = 1, 1e300
    for s in range(1, max_s + 1):
        n_max = (tiles * s + 255) // 256
        kt = float((K + s * BK - 1) // (s * BK))
        cost = kt * ((n_max // 5) * step_cost[5] + step_cost[n_max % 5]) + finish * s
        if cost < best_cost:
            best_cost, best = cost, s
    return best


def tn_form(M, N, K, a_ptr, lda, b_ptr, ldb, no_fast=None):
    no_fast = NO_FAST if no_fast is None else no_fast
    vec = a_ptr % 16 == 0 and b_ptr % 16 == 0 and lda % 4 == 0 and ldb % 4 == 0 and M % 4 == 0 and N % 4 == 0
    fast = vec and not no_fast and K % BK == 0 and ((K - 1) * lda + M) * 4 < OOB_OFF and ((K - 1) * ldb + N) * 4 < OOB_OFF
    return 'FAST' if fast else ('VEC' if vec else 'dword')


def tn_finish(N, ldc, c_ptr, slices):
    if N % 4 == 0 and ldc % 4 == 0 and c_ptr % 16 == 0:      # (the workspace is a fresh allocation: aligned)
        return 'vec' if slices <= 8 else 'vec8'
    return 'scalar'


# ---------------------------------------------------------------------------------------------------- the hashed dropout mask
def _mix32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def host_keep(state, site, p, M, N):
    """keep(m N + n) of act 3 (p2c_rec_dev.h drop_keys_only / drop_value) for the forward step of ``state``, on the host."""
    s = state.cpu().numpy().astype(np.int64).astype(np.uint32)
    u = lambda v: np.array([v & 0xFFFFFFFF], dtype=np.uint32)            # noqa: E731
    with np.errstate(over='ignore'):
        step, site1 = u(int(s[2])), u(site + 1)
        k0 = _mix32(u(int(s[0])) ^ (step * np.uint32(0x9E3779B9)) ^ (site1 * np.uint32(0x632BE59B)))
        k1 = _mix32(u(int(s[1])) + step + np.uint32(0x85EBCA6B) * site1)
        e = np.arange(M * N, dtype=np.uint32)
        h = _mix32(e * np.uint32(0x9E3779B1) + k0) ^ k1
    thresh = np.uint32(int(float(np.float32(p)) * 4294967296.0))     # ((double) of the fp32 drop_p, as the kernel forms it)
    return torch.from_numpy((h >= thresh).reshape(M, N))


def drop_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def new_state(step=5):
    return torch.tensor([0x1234567, 0x3456789, step, 0], dtype=torch.int32, device=dev())


# =========================================================================================== 2. the forward form matrix (NT, NN)
# (M, N, K, layout) per (trans_b, form); layout: lda / ldb / ldc = width + pad, a / b / c bases `off` floats past alignment.
_M = (1, 127, 128, 129, 257)


def _lay(la=0, lb=0, lc=0, ao=0, bo=0, co=0):
    return dict(la=la, lb=lb, lc=lc, ao=ao, bo=bo, co=co)


_NT_N = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
_NN_N4 = (4, 32, 36, 60, 64, 68, 124, 128, 132, 32)       # NN with 16-byte loads needs N % 4 == 0
_NN_ODD = (1, 31, 33, 63, 65, 127, 129, 64, 128, 32)
FORM_CASES = []
for i in range(10):
    m, lay_fast = _M[i % 5], _lay(la=(0, 4, 8)[i % 3], lb=(0, 4)[i % 2], lc=(0, 1, 3)[i % 3], co=i % 2)
    lay_vec = _lay(la=(4, 0)[i % 2], lb=(0, 8)[i % 2], lc=(2, 0, 1)[i % 3], co=(i + 1) % 2)
    # dword: K % 4 != 0, or an operand 4 / 8 bytes off alignment, or an odd leading dimension
    lay_dw = [_lay(), _lay(lc=1), _lay(), _lay(ao=1), _lay(bo=2, lc=2), _lay(la=1), _lay(lb=3, co=1), _lay(), _lay(la=5, lb=1),
              _lay(ao=2, bo=1, lc=1)][i]
    FORM_CASES += [
        (True, 'FAST', m, _NT_N[i], (32, 64, 96)[i % 3], lay_fast),
        (True, 'VEC', m, _NT_N[i], (4, 36, 60, 100)[i % 4], lay_vec),
        (True, 'dword', m, _NT_N[i], (1, 31, 33, 32, 64, 32, 64, 1, 33, 96)[i], lay_dw),
        (False, 'FAST', m, _NN_N4[i], (32, 64, 96)[i % 3], lay_fast),
        (False, 'VEC', m, _NN_N4[i], (4, 36, 60, 100)[i % 4], lay_vec),
        (False, 'dword', m, _NN_ODD[i] if i < 7 else _NN_N4[i], (1, 31, 33, 32, 64, 32, 64, 1, 33, 96)[i], lay_dw),
    ]


def _form_id(c):
    t, f, M, N, K, _ = c
    return f'{"NT" if t else "NN"}-{f}-{M}x{N}x{K}'


def _operands(trans_b, M, N, K, lay, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    A = torch.randn(M, K, generator=g)
    B = torch.randn(N, K, generator=g) if trans_b else torch.randn(K, N, generator=g)
    a = place(A.to(dev()), K + lay['la'], lay['ao'])
    b = place(B.to(dev()), B.shape[1] + lay['lb'], lay['bo'])
    return a, b


@pytest.mark.parametrize('case', FORM_CASES, ids=[_form_id(c) for c in FORM_CASES])
def test_product_matches_fp64_in_every_form(bn, case):
    trans_b, form, M, N, K, lay = case
    a, b = _operands(trans_b, M, N, K, lay, M * 7919 + N * 31 + K)
    assert fwd_form(M, N, K, trans_b, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)) == form
    c = place(torch.zeros(M, N, device=dev()), N + lay['lc'], lay['co'])
    assert c_gemm(a, b, trans_b, c) == 0
    want = a.double() @ (b.double().t() if trans_b else b.double())
    torch.cuda.synchronize()
    assert rel(c, want) < prod_tol(K)
    assert untouched_outside(c)


# ================================================================================================================ 3. epilogues
EPI_SHAPES = {'full': (256, 128), 'partial': (199, 77)}
EPI_K = {('FAST', 'full'): (64, _lay()), ('FAST', 'partial'): (96, _lay(la=4, lb=4)),
         ('VEC', 'full'): (36, _lay()), ('VEC', 'partial'): (100, _lay(la=4)),
         ('dword', 'full'): (64, _lay(ao=1)), ('dword', 'partial'): (33, _lay())}
# (bias, rows_per_scale or None, residual: None / 'sep' (ldr > N) / 'alias' (residual is c), act 1: aux_out, act 3: drop state)
EPI_COMBOS = [(False, None, None, False), (True, None, None, True), (True, 1, None, True), (False, None, 'sep', False),
              (True, 7, 'alias', True), (False, 26, 'sep', False)]


@pytest.mark.parametrize('form', ['FAST', 'VEC', 'dword'])
@pytest.mark.parametrize('act', [0, 1, 2, 3, 4])
def test_epilogue_matches_fp64_in_every_form(bn, act, form):
    """Every act with and without bias, row scale (1 / 7 / 26 rows per factor) and residual (separate with ldr > N, or aliased
    with c), in a full and a partial tile, both trans_b; act 1 stores the pre-activation (ldaux > N), acts 2 / 4 read theirs
    with ldaux > N; act 3 draws the hashed mask (checked against the host's hash) or, without a state, is ReLU alone."""
    d = dev()
    for trans_b in (True, False):
        for shape, (M, N) in EPI_SHAPES.items():
            K, lay = EPI_K[(form, shape)]
            if not trans_b and form != 'dword' and N % 4:
                N += 4 - N % 4                           # (NN 16-byte loads need N % 4 == 0)
            for ci, (use_bias, per, res_kind, extra) in enumerate(EPI_COMBOS):
                seed = act * 1000 + ci * 10 + M + (0 if trans_b else 5)
                a, b = _operands(trans_b, M, N, K, lay, seed)
                assert fwd_form(M, N, K, trans_b, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)) == form
                g = torch.Generator(device='cpu').manual_seed(seed + 1)
                v64 = a.double() @ (b.double().t() if trans_b else b.double())
                kw = {}
                if use_bias:
                    bias = torch.randn(N, generator=g).to(d)
                    kw['bias'] = bias
                    v64 = v64 + bias.double()
                c = place(torch.randn(M, N, generator=g).to(d), N + 3, 1)
                s64 = 1.0
                if per is not None:
                    f = (torch.rand((M + per - 1) // per, generator=g) > 0.3).float() / 0.7 + 0.25
                    kw['row_scale'], kw['rows_per_scale'] = f.to(d), per
                    s64 = f.double().to(d).repeat_interleave(per)[:M].view(-1, 1)
                r64 = 0.0
                if res_kind == 'sep':
                    kw['residual'] = place(torch.randn(M, N, generator=g).to(d), N + 5)
                    r64 = kw['residual'].double()
                elif res_kind == 'alias':
                    kw['residual'] = c
                    r64 = c.double()
                p, aux_out = 0.0, None
                if act == 0:
                    y64 = v64
                elif act == 1:
                    y64 = gelu64(v64)
                    if extra:
                        aux_out = kw['aux_out'] = place(torch.zeros(M, N, device=d), N + 2)
                elif act == 2:
                    kw['aux'] = place(torch.randn(M, N, generator=g).to(d), N + 7, 2)
                    y64 = v64 * gelu_grad64(kw['aux'].double())
                elif act == 3:
                    if extra:
                        p = 0.3
                        st = new_state(ci)
                        kw.update(drop_state=st, drop_p=p, drop_site=ci)
                        keep = host_keep(st, ci, p, M, N).to(d)
                        y64 = v64.clamp(min=0) * keep.double() * drop_scale(p)
                    else:
                        y64 = v64.clamp(min=0)
                else:
                    p = 0.3 if extra else 0.0
                    kw['drop_p'] = p
                    kw['aux'] = place(torch.randn(M, N, generator=g).to(d), N + 1)
                    y64 = v64 * (kw['aux'].double() > 0).double() * drop_scale(p)
                want = y64 * s64 + r64
                assert c_gemm(a, b, trans_b, c, act=act, **kw) == 0
                torch.cuda.synchronize()
                what = (trans_b, shape, ci)
                assert rel(c, want) < 2e-5, what
                assert untouched_outside(c), what
                if aux_out is not None:
                    assert rel(aux_out, v64) < 2e-5 and untouched_outside(aux_out), what
                if act == 3 and extra:
                    assert int(st[3]) == int(st[2]) + 1, what


def test_act3_mask_is_the_same_in_every_form():
    """Positive operands and bias: v > 0 everywhere, so the kept entries are exactly C != 0. In every tile width and load form
    (and at three K: the mask depends on m N + n only) the mask equals the host's hash bit for bit, and the kept entries equal
    v / (1 - p) in fp64."""
    d = dev()
    M, N, p, site = 199, 77, 0.35, 3
    st = new_state(11)
    keep = host_keep(st, site, p, M, N).to(d)
    seen = set()
    for bnv in (0, 32, 64, 128):
        with gemm_env(P2C_GEMM_BN=bnv or None):
            for trans_b in (True, False):
                for K, lay in ((64, _lay()), (36, _lay()), (64, _lay(ao=1)), (33, _lay())):
                    a, b = _operands(trans_b, M, N, K, lay, K)
                    a.abs_(), b.abs_()
                    seen.add((bnv, trans_b, fwd_form(M, N, K, trans_b, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0))))
                    bias = torch.full((N,), 0.5, device=d)
                    c = place(torch.zeros(M, N, device=d), N)
                    assert c_gemm(a, b, trans_b, c, bias=bias, act=3, drop_state=st, drop_p=p, drop_site=site) == 0
                    torch.cuda.synchronize()
                    assert torch.equal(c != 0, keep), (bnv, trans_b, K, lay)
                    want = ((a.double() @ (b.double().t() if trans_b else b.double())) + 0.5) * drop_scale(p)
                    assert rel(c * keep, want * keep.double()) < 2e-5
    assert abs(float(keep.float().mean()) - (1 - p)) < 0.02
    assert len({f for _, _, f in seen}) == (2 if NO_FAST else 3)


def test_act3_and_act4_chain_to_the_fp64_derivative():
    """act 3 (forward) then act 4 (backward, aux = act 3's output): d/dv [relu(v) keep / (1 - p)] = [v > 0] keep / (1 - p), for
    p = 0 and 0.3, with and without a state. Without a state act 3 is ReLU alone, so p > 0 is refused there (act 4 always
    scales by 1 / (1 - p)); act 4 stays legal without a state (the encoder layer's backward calls it so)."""
    d = dev()
    M, N, K, site = 150, 70, 40, 2
    torch.manual_seed(4)
    x, w = torch.randn(M, K, device=d), torch.randn(N, K, device=d)
    gy, w2 = torch.randn(M, 24, device=d), torch.randn(24, N, device=d)   # the gradient arriving at h: gy w2 (NN)
    v64 = x.double() @ w.double().t()
    g64 = gy.double() @ w2.double()
    for p in (0.0, 0.3):
        for with_state in (True, False):
            st = new_state(7) if with_state else None
            h = place(torch.zeros(M, N, device=d), N + 3, 1)
            rc = c_gemm(x, w, True, h, act=3, drop_state=st, drop_p=p, drop_site=site)
            if p > 0 and not with_state:
                assert rc == E_SHAPE
                torch.cuda.synchronize()
                assert bool((h.view(torch.int32) == 0).all())
                continue
            assert rc == 0
            keep = host_keep(st, site, p, M, N).to(d).double() if with_state else torch.ones(M, N, dtype=torch.float64, device=d)
            dv = place(torch.zeros(M, N, device=d), N + 1)
            assert c_gemm(gy, w2, False, dv, act=4, aux=h, drop_p=p) == 0
            torch.cuda.synchronize()
            clear = (v64.abs() > 1e-3).double()          # (where the fp32 product's sign could differ from fp64's: none expected)
            want = g64 * (v64 > 0).double() * keep * drop_scale(p)
            assert rel(dv * clear, want * clear) < 2e-5, (p, with_state)
            assert rel(h, v64.clamp(min=0) * keep * drop_scale(p)) < 2e-5
    # act 4 without a state at p > 0: legal
    h = torch.rand(M, N, device=d) - 0.5
    dv = torch.zeros(M, N, device=d)
    assert c_gemm(gy, w2, False, dv, act=4, aux=h, drop_p=0.3) == 0
    torch.cuda.synchronize()
    assert rel(dv, g64 * (h > 0).double() * drop_scale(0.3)) < 2e-5


# ======================================================================================================= 4. bitwise invariants
@pytest.mark.parametrize('trans_b', [True, False], ids=['NT', 'NN'])
def test_every_tile_and_load_form_gives_the_same_bits(trans_b):
    """Every form runs the same v_mfma_f32_32x32x2_f32 sequence in k order: at one K every tile width and load form gives the
    same bits, plain and with the full epilogue (bias, GELU, row scale, residual). K = 64 (FAST / VEC against dword) and
    K = 36 (VEC against dword: the same zero padding of the last k-tile)."""
    d = dev()
    M, N = 257, 132 if not trans_b else 129
    forms = set()
    for K in (64, 36):
        for act in (0, 1):
            outs = []
            g = torch.Generator(device='cpu').manual_seed(K + act)
            A = torch.randn(M, K, generator=g).to(d)
            B = (torch.randn(N, K, generator=g) if trans_b else torch.randn(K, N, generator=g)).to(d)
            bias, res = torch.randn(N, generator=g).to(d), torch.randn(M, N, generator=g).to(d)
            f = torch.rand(M // 7 + 1, generator=g).to(d)
            for bnv in (0, 32, 64, 128):
                with gemm_env(P2C_GEMM_BN=bnv or None):
                    for lay in (_lay(), _lay(ao=1), _lay(la=1, lb=3), _lay(bo=2, lc=5, co=1)):
                        a, b = place(A, K + lay['la'], lay['ao']), place(B, B.shape[1] + lay['lb'], lay['bo'])
                        forms.add(fwd_form(M, N, K, trans_b, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)))
                        c = place(torch.zeros(M, N, device=d), N + lay['lc'], lay['co'])
                        kw = dict(bias=bias, act=1, row_scale=f, rows_per_scale=7, residual=res) if act else {}
                        assert c_gemm(a, b, trans_b, c, **kw) == 0
                        outs.append(c.clone())
            for i, o in enumerate(outs[1:]):
                assert torch.equal(o, outs[0]), (K, act, i + 1)
    assert forms == ({'VEC', 'dword'} if NO_FAST else {'FAST', 'VEC', 'dword'})


@pytest.mark.parametrize('act', [0, 1, 2, 4])
def test_a_block_equals_the_same_block_of_a_larger_product(bn, act):
    """An (M, N) product (+ epilogue) equals the matching block of the same product computed on a superset -- more rows of A,
    more columns of C -- bit for bit: edge tiles compute what interior tiles do. (Act 3 is left out: its mask index is m N + n.)
    The subset's operands are views into the superset's (leading dimensions > width)."""
    d = dev()
    for trans_b in (True, False):
        for (M, N), (Ms, Ns), K in (((129, 33), (257, 129), 64), ((1, 1), (128, 64), 32), ((127, 65), (300, 200), 36),
                                    ((128, 100), (131, 132), 33)):
            g = torch.Generator(device='cpu').manual_seed(M * N + act)
            A = torch.randn(Ms, K, generator=g).to(d)
            B = (torch.randn(Ns, K, generator=g) if trans_b else torch.randn(K, Ns, generator=g)).to(d)
            bias, res, aux = (torch.randn(Ns, generator=g).to(d), torch.randn(Ms, Ns, generator=g).to(d),
                              torch.randn(Ms, Ns, generator=g).to(d))
            f = torch.rand(Ms // 3 + 1, generator=g).to(d)
            big, small = torch.zeros(Ms, Ns, device=d), torch.zeros(M, N, device=d)

            def kw(m, n):
                k = dict(bias=bias[:n], act=act, row_scale=f, rows_per_scale=3, residual=res[:m, :n])
                if act in (2, 4):
                    k['aux'] = aux[:m, :n]
                if act == 4:
                    k['drop_p'] = 0.2
                return k
            assert c_gemm(A, B, trans_b, big, **kw(Ms, Ns)) == 0
            assert c_gemm(A[:M], B[:N] if trans_b else B[:, :N], trans_b, small, **kw(M, N)) == 0
            torch.cuda.synchronize()
            assert torch.equal(small, big[:M, :N]), (trans_b, M, N)


TN_SLICES = (1, 3, 8, 9, 64)
# (TN_BN, a / b / c layout): the load form follows from K and the a / b bases, the finish kernel from c and the slice count
TN_VARIANTS = [(bnv, lay) for bnv in (32, 64, 128)
               for lay in (_lay(), _lay(ao=1, lc=4), _lay(co=1), _lay(lc=1, bo=2), _lay(la=4, lb=4))]
TN_K = (32768, 32764)          # K % 32 == 0 (FAST / dword) and not (VEC / dword); max_s = K / 512 allows 64 (63) slices


def _tn_cell(bnv, lay, K, slices, M, N, no_fast=False):
    a_ptr, b_ptr, c_ptr = 4 * lay['ao'], 4 * lay['bo'], 4 * lay['co']
    s = tn_slices(M, N, K, bnv, slices)
    return (bnv, tn_form(M, N, K, a_ptr, M + lay['la'], b_ptr, N + lay['lb'], no_fast),
            tn_finish(N, N + lay['lc'], c_ptr, s))


@pytest.mark.parametrize('slices', TN_SLICES)
def test_tn_every_tile_finish_and_load_form_gives_the_same_bits(slices):
    """p2c_gemm_tn at a fixed slice count: every P2C_GEMM_TN_BN, load form and finish kernel (vec for <= 8 slices, vec8 above,
    the scalar one for a c 4 bytes off alignment or an odd ldc) gives the same bits for C and for the bias column sums (the
    slabs are added in slice order by each), with a row factor; and both match fp64."""
    d = dev()
    M, N, per = 132, 100, 9
    for K in TN_K:
        g = torch.Generator(device='cpu').manual_seed(K + slices)
        A, B = torch.randn(K, M, generator=g).to(d), torch.randn(K, N, generator=g).to(d)
        f = torch.rand((K + per - 1) // per, generator=g).to(d) + 0.5
        a64 = A.double() * f.double().repeat_interleave(per)[:K].view(-1, 1)
        want, want_b = a64.t() @ B.double(), a64.sum(0)
        outs = []
        for bnv, lay in TN_VARIANTS:
            with gemm_env(P2C_GEMM_TN_BN=bnv, P2C_GEMM_TN_SLICES=slices):
                a, b = place(A, M + lay['la'], lay['ao']), place(B, N + lay['lb'], lay['bo'])
                c, bo = place(torch.zeros(M, N, device=d), N + lay['lc'], lay['co']), place(torch.zeros(1, M, device=d), M, 3)
                s = tn_slices(M, N, K, bnv, slices)
                cell = (bnv, tn_form(M, N, K, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)),
                        tn_finish(N, c.stride(0), c.data_ptr(), s))
                assert cell == _tn_cell(bnv, lay, K, slices, M, N, NO_FAST)
                assert c_gemm_tn(a, b, c, 0, f, per, bo) == 0
                torch.cuda.synchronize()
                assert untouched_outside(c) and untouched_outside(bo)
                outs.append((cell, c.clone(), bo.clone()))
        assert rel(outs[0][1], want) < prod_tol(K) and rel(outs[0][2][0], want_b) < prod_tol(K)
        for cell, c, bo in outs[1:]:
            assert torch.equal(c, outs[0][1]) and torch.equal(bo, outs[0][2]), (K, cell, outs[0][0])


# ============================================================================================================ 5. TN flag matrix
@pytest.mark.parametrize('K,M,N', [(26 * 9 * 20, 260, 136), (2000, 132, 100), (4001, 130, 33)])
def test_tn_flags_bias_and_row_factor_match_fp64(K, M, N):
    """accumulate bit 0: add to C, bit 1: add to bias_out (flag 1 -- C accumulates, the bias is written fresh -- is what
    ops.gemm_tn produces inside the gradient sinks); with and without bias_out and a row factor per 1 / 9 / 26 rows; c dense
    or with an odd ldc (the vec / vec8 finish kernels at the first two shapes, the scalar one)."""
    d = dev()
    g = torch.Generator(device='cpu').manual_seed(K + M)
    A, B = torch.randn(K, M, generator=g).to(d), torch.randn(K, N, generator=g).to(d)
    c0, b0 = torch.randn(M, N, generator=g).to(d), torch.randn(1, M, generator=g).to(d)
    for per in (None, 1, 9, 26):
        f, a64 = None, A.double()
        if per is not None:
            f = (torch.rand((K + per - 1) // per, generator=g) > 0.3).float().to(d) / 0.7
            a64 = a64 * f.double().repeat_interleave(per)[:K].view(-1, 1)
        for flags in (0, 1, 2, 3):
            for with_bias in (False, True):
                c, bo = place(c0, N + 3 * (flags & 1 ^ with_bias)), place(b0, M, 1)
                assert c_gemm_tn(A, B, c, flags, f, per or 1, bo if with_bias else None) == 0
                torch.cuda.synchronize()
                want = a64.t() @ B.double() + (c0.double() if flags & 1 else 0.0)
                assert rel(c, want) < prod_tol(K), (per, flags, with_bias)
                if with_bias:
                    want_b = a64.sum(0) + (b0[0].double() if flags & 2 else 0.0)
                    assert rel(bo[0], want_b) < prod_tol(K), (per, flags)
                else:
                    assert torch.equal(bo, b0)
                assert untouched_outside(c) and untouched_outside(bo)


@pytest.mark.parametrize('K', [(1 << 21) - 3, (1 << 21) + 5])
def test_tn_row_factor_index_is_exact_near_2_pow_21(K):
    """The row-factor index floor((k + 0.5) / rows_per_scale) in fp32 (K <= 2^21; an integer division above). Small integers
    throughout -- every partial sum is an integer below 2^24, exact in fp32 -- so a single row given its neighbour sample's
    factor changes the result: it must equal fp64 exactly."""
    d = dev()
    M, N = 8, 4
    g = torch.Generator(device='cpu').manual_seed(K)
    A = torch.randint(-1, 2, (K, M), generator=g).float().to(d)
    B = torch.randint(-1, 2, (K, N), generator=g).float().to(d)
    for per in (7, 26, 61):        # (61: 1 / 61 rounds down in fp32 -- without the + 0.5, 30 587 rows below 2^21 get the wrong factor)
        f = torch.randint(0, 4, ((K + per - 1) // per,), generator=g).float().to(d)
        a64 = A.double() * f.double().repeat_interleave(per)[:K].view(-1, 1)
        c, bo = torch.zeros(M, N, device=d), torch.zeros(M, device=d)
        assert c_gemm_tn(A, B, c, 0, f, per, bo) == 0
        torch.cuda.synchronize()
        assert torch.equal(c.double(), a64.t() @ B.double()), per
        assert torch.equal(bo.double(), a64.sum(0)), per


# ================================================================================================================= 6. refusals
@pytest.mark.parametrize('trans_b', [1, 0], ids=['NT', 'NN'])
def test_gemm_refusals_launch_nothing(trans_b):
    d = dev()
    M, N, K = 8, 12, 8
    a, c = torch.randn(M, K, device=d), torch.empty(M, N, device=d)
    b = torch.randn(N, K, device=d) if trans_b else torch.randn(K, N, device=d)
    aux, f, st = torch.randn(M, N, device=d), torch.ones(M, device=d), new_state(3)
    cases = [
        ('lda < K', {}, {'lda': K - 1}, E_SHAPE),
        ('ldb below its minimum', {}, {'ldb': (K if trans_b else N) - 1}, E_SHAPE),
        ('ldc < N', {}, {'ldc': N - 1}, E_SHAPE),
        ('ldr < N', {'residual': aux}, {'ldr': N - 1}, E_SHAPE),
        ('ldaux < N (act 2)', {'act': 2, 'aux': aux}, {'ldaux': N - 1}, E_ENUM),
        ('ldaux < N (act 1 aux_out)', {'act': 1, 'aux_out': aux}, {'ldaux': N - 1}, E_ENUM),
        ('ldaux < N (act 4)', {'act': 4, 'aux': aux}, {'ldaux': N - 1}, E_ENUM),
        ('act -1', {'act': -1}, {}, E_ENUM),
        ('act 5', {'act': 5}, {}, E_ENUM),
        ('act 2 without aux', {'act': 2}, {}, E_ENUM),
        ('act 4 without aux', {'act': 4}, {}, E_ENUM),
        ('act 3 drop_p 1', {'act': 3, 'drop_state': st, 'drop_p': 1.0}, {}, E_SHAPE),
        ('act 3 drop_p < 0', {'act': 3, 'drop_state': st, 'drop_p': -0.1}, {}, E_SHAPE),
        ('act 3 drop_p NaN', {'act': 3, 'drop_state': st, 'drop_p': float('nan')}, {}, E_SHAPE),
        ('act 3 drop_p > 0 without a state', {'act': 3, 'drop_p': 0.3}, {}, E_SHAPE),
        ('act 4 drop_p 1', {'act': 4, 'aux': aux, 'drop_p': 1.0}, {}, E_SHAPE),
        ('act 4 drop_p < 0', {'act': 4, 'aux': aux, 'drop_p': -0.5}, {}, E_SHAPE),
        ('rows_per_scale 0', {'row_scale': f, 'rows_per_scale': 0}, {}, E_SHAPE),
        ('rows_per_scale -1', {'row_scale': f, 'rows_per_scale': -1}, {}, E_SHAPE),
        ('M 0', {}, {'M': 0}, E_SHAPE), ('N 0', {}, {'N': 0}, E_SHAPE), ('K 0', {}, {'K': 0}, E_SHAPE),
        ('M -1', {}, {'M': -1}, E_SHAPE), ('N -5', {}, {'N': -5}, E_SHAPE), ('K -1', {}, {'K': -1}, E_SHAPE),
        ('a NULL', {}, {'a': None}, E_NULL), ('b NULL', {}, {'b': None}, E_NULL), ('c NULL', {}, {'c': None}, E_NULL),
    ]
    c.view(torch.int32).fill_(SENT)
    st0 = st.clone()
    for name, kw, over, rc in cases:
        assert c_gemm(a, b, trans_b, c, over=over, **kw) == rc, name
    assert lib().p2c_gemm(None, _stream()) == E_NULL
    torch.cuda.synchronize()
    assert bool((c.view(torch.int32) == SENT).all())
    assert torch.equal(st, st0)
    assert c_gemm(a, b, trans_b, c) == 0             # (the same descriptor without the fault launches)


def test_gemm_tn_refusals_launch_nothing():
    d = dev()
    K, M, N = 64, 8, 12
    a, b, c, bo = torch.randn(K, M, device=d), torch.randn(K, N, device=d), torch.empty(M, N, device=d), torch.empty(M, device=d)
    f = torch.ones(K, device=d)
    cases = [
        ('a NULL', {'a': None}, {}, E_NULL), ('b NULL', {'b': None}, {}, E_NULL), ('c NULL', {'c': None}, {}, E_NULL),
        ('workspace NULL', {}, {'ws': False}, E_NULL),
        ('M 0', {'M': 0}, {}, E_SHAPE), ('N 0', {'N': 0}, {}, E_SHAPE), ('K 0', {'K': 0}, {}, E_SHAPE),
        ('M -1', {'M': -1}, {}, E_SHAPE), ('K -3', {'K': -3}, {}, E_SHAPE),
        ('lda < M', {'lda': M - 1}, {}, E_SHAPE), ('ldb < N', {'ldb': N - 1}, {}, E_SHAPE), ('ldc < N', {'ldc': N - 1}, {}, E_SHAPE),
        ('rows_per_scale 0', {}, {'row_scale': f, 'rows_per_scale': 0}, E_SHAPE),
        ('rows_per_scale -2', {}, {'row_scale': f, 'rows_per_scale': -2}, E_SHAPE),
    ]
    c.view(torch.int32).fill_(SENT)
    bo.view(torch.int32).fill_(SENT)
    for name, over, kw, rc in cases:
        assert c_gemm_tn(a, b, c, 3, bias_out=bo, over=over, **kw) == rc, name
    torch.cuda.synchronize()
    assert bool((c.view(torch.int32) == SENT).all()) and bool((bo.view(torch.int32) == SENT).all())


# ===================================================================================================== 7. host-side argument checks
def test_ops_gemm_rejects_a_wrong_out_or_bias():
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    M, N, K = 20, 12, 8
    a, w = torch.randn(M, K, device=d), torch.randn(N, K, device=d)
    bad_outs = {'shape': torch.zeros(M, N + 1, device=d), 'rows': torch.zeros(M + 1, N, device=d),
                'dtype': torch.zeros(M, N, device=d, dtype=torch.float64), 'host': torch.zeros(M, N),
                'inner stride': torch.zeros(N, M, device=d).t(), 'overlapping rows': torch.zeros(1, N, device=d).expand(M, N)}
    for name, out in bad_outs.items():
        keep = out.clone()
        with pytest.raises(RuntimeError, match='out'):
            ops.gemm(a, w, True, out=out)
        assert torch.equal(out, keep), name
    for bias in (torch.randn(N - 1, device=d), torch.randn(N + 1, device=d), torch.randn(2, N, device=d)):
        with pytest.raises(RuntimeError, match='bias'):
            ops.gemm(a, w, True, bias=bias)
    out = torch.empty(M, N + 4, device=d)[:, 2:N + 2]                # a strided but legal out
    ops.gemm(a, w, True, bias=torch.zeros(N, device=d), out=out)
    assert rel(out, a.double() @ w.double().t()) < prod_tol(K)


def test_ops_gemm_tn_rejects_a_wrong_out_or_bias_out():
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    K, M, N = 300, 16, 12
    a, b = torch.randn(K, M, device=d), torch.randn(K, N, device=d)
    for name, out in {'shape': torch.empty(M, N - 1, device=d), 'transposed': torch.empty(N, M, device=d),
                      'dtype': torch.empty(M, N, device=d, dtype=torch.float16), 'host': torch.empty(M, N),
                      'inner stride': torch.empty(N, M, device=d).t()}.items():
        with pytest.raises(RuntimeError, match='out'):
            ops.gemm_tn(a, b, out=out, accumulate=True)
    for name, bo in {'short': torch.empty(M - 1, device=d), 'long': torch.empty(M + 1, device=d),
                     'strided': torch.empty(2 * M, device=d)[::2], 'dtype': torch.empty(M, device=d, dtype=torch.float64),
                     '2-D': torch.empty(1, M, device=d)}.items():
        with pytest.raises(RuntimeError, match='bias_out'):
            ops.gemm_tn(a, b, bias=True, bias_out=bo)
    c, db = ops.gemm_tn(a, b, bias=True, bias_out=torch.empty(M, device=d))
    assert rel(c, a.double().t() @ b.double()) < prod_tol(K) and rel(db, a.double().sum(0)) < prod_tol(K)


# ====================================================================================================== coverage and the child run
def test_the_case_tables_cover_every_cell():
    """Every forward cell {BN} x {NT, NN} x {FAST, VEC, dword} and every TN cell {BN} x {FAST, VEC, dword} x {vec, vec8, scalar}
    has cases, by the mirror of the host dispatch (a change of the dispatch that moves cases out of a cell fails here)."""
    fwd = set()
    for trans_b, form, M, N, K, lay in FORM_CASES:
        got = fwd_form(M, N, K, trans_b, 4 * lay['ao'], K + lay['la'], 4 * lay['bo'], (K if trans_b else N) + lay['lb'],
                       no_fast=False)
        assert got == form, (trans_b, form, M, N, K, lay)
        fwd.add((trans_b, form))
    assert fwd == {(t, f) for t in (True, False) for f in ('FAST', 'VEC', 'dword')}
    tn = {_tn_cell(bnv, lay, K, s, 132, 100) for s in TN_SLICES for K in TN_K for bnv, lay in TN_VARIANTS}
    assert tn == {(b, f, k) for b in (32, 64, 128) for f in ('FAST', 'VEC', 'dword') for k in ('vec', 'vec8', 'scalar')}
    # the epilogue table: every act in every form, full and partial tiles (the bn fixture crosses all of it with 32 / 64 / 128)
    assert {f for f, _ in EPI_K} == {'FAST', 'VEC', 'dword'} and {s for _, s in EPI_K} == set(EPI_SHAPES)
    for (form, shape), (K, lay) in EPI_K.items():
        M, N = EPI_SHAPES[shape]
        for trans_b in (True, False):
            n = N if (trans_b or form == 'dword' or N % 4 == 0) else N + 4 - N % 4
            assert fwd_form(M, n, K, trans_b, 4 * lay['ao'], K + lay['la'], 4 * lay['bo'], (K if trans_b else n) + lay['lb'],
                            no_fast=False) == form
    # the production dispatch never picks BN = 128 (reachable only through P2C_GEMM_BN)
    assert {fwd_bn(M, N, K, t) for M in (1, 8192, 21024, 546624) for N in (32, 96, 832, 2496) for K in (32, 52, 832, 1664)
            for t in (True, False)} == {32, 64}


def test_every_form_also_passes_with_the_fast_loads_off():
    """P2C_GEMM_NO_FAST=1 (read once per process, so a child pytest): the cases that ran in a FAST form run in the VEC form at
    K % 32 == 0; every case that expects FAST by name is left out."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, P2C_GEMM_NO_FAST='1')
    res = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider',
                          '-k', 'not FAST'], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
