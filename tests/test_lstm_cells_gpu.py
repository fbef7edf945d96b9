"""The LSTM recurrence behind p2c_lstm_desc in every descriptor cell: K7b on the 16-sequence tiling (``wide``), K7b on the
4-sequence tiling (``narrow``) and K18 (``steps``, one launch per time step), each driven through the C ABI with a hand-filled
``_lib.LstmDesc`` and compared with the layer written out step by step in fp64 on the CPU (``reference``; not nn.LSTM).

Cells (``CASES``, checked by ``test_coverage_rule``, which needs no GPU). For every (form, H) -- K7b: H in 16, 32, 48, 64, 96, 128;
K18: H in 16, 48, 63, 64, 65, 128, 129 -- four value cases and one T = 0 case which together meet
  * every B edge of the form's tile (narrow 1, 3, 4, 5; wide 15, 16, 17, 33; K18 31, 32, 33, 65) and T = 0, 1, 2, 5;
  * every option off and on: h0, c0, hT, cT, g_out, g_hT, g_cT (at least one of the three), g_h0, g_c0 each on its own; bias_a only,
    bias_b only, both, none; and on K7b acts / cs = NULL in the forward, gx_bt, g_gx_bt, out_drop + drop_state (p = 0.2, site 3).
    On K18 the last four are refusals (``STEPS_REFUSALS``): P2C_E_SHAPE, or P2C_E_NULL for acts / cs, and nothing written.
One saturated case per form (pre-activations up to +-200: ``__expf`` overflows inside the activations) and one
sequence-independence case per form at a B that is no multiple of the tile.

Value bounds, for every produced tensor (acts and cs included):
  * whole tensor: max|got - ref| / max|ref| <= 1e-4, the bound tests/test_lstm_gpu.py holds these kernels to;
  * the same ratio per time-step slice [t], and per gate block of a slice for g_gx and acts: <= max(1e-4, 4 e_ref), e_ref = the
    ratio of the same step-by-step formula evaluated in fp32 on the CPU against fp64 for that slice. The factor 4 is the "within
    four e_ref" margin of tests/test_ik_gpu.py and tests/test_smpl_retarget_gpu.py; it covers v_exp_f32 / v_rcp_f32 against libm
    and the different summation orders of the three forms. A slice whose reference is all zero must be all zero.
Exact (bit for bit, within one form): hT == out[T-1], cT == cs[T-1]; g_gx_bt == g_gx^T; gx_bt == the (T,B) run; biases == the
bias-free run fed gx + (bias_a + bias_b); a NULL g_out / g_hT / g_cT / h0 / c0 == zeros in its place; out without acts / cs == out
with them; out_drop == out * mask; a second run repeats its bits; a sequence in a batch == that sequence alone; a NaN sequence
leaves every other row's bits alone. T = 0 (include/p2c.h): hT = h0, cT = c0, g_h0 = g_hT, g_c0 = g_cT, zeros for NULL.
Every tensor of a run lives in one pool with 256 sentinel floats between neighbours: the guards, the inputs and every tensor
whose pointer was not passed are compared with what they held before the launch.

Largest per-slice ratio max|got - ref| / max|ref| measured on the MI355X over all of the above (every test prints its own and the
running maximum of its form; the fp32 CPU evaluation's own largest slice error is 1.8e-6, so no slice's bound left 1e-4):
  wide   1.564e-06  (acts[0], H = 96, B = 17, T = 5)
  narrow 1.060e-06  (g_gx[3] gate o, H = 96, B = 1, T = 5)
  steps  1.813e-06  (acts[0], H = 129, B = 65, T = 1)
The saturated cases: 1.441e-06, 1.003e-06, 1.189e-06.
"""
import collections
import ctypes
import functools

import pytest
import torch

gpu = pytest.mark.gpu

FORMS = ('wide', 'narrow', 'steps')
WIDTHS = {'wide': (16, 32, 48, 64, 96, 128), 'narrow': (16, 32, 48, 64, 96, 128), 'steps': (16, 48, 63, 64, 65, 128, 129)}
B_EDGES = {'narrow': (1, 3, 4, 5), 'wide': (15, 16, 17, 33), 'steps': (31, 32, 33, 65)}
T_VALUES = (0, 1, 2, 5)
BIASES = ('none', 'a', 'b', 'ab')
FLAGS = ('h0', 'c0', 'hT', 'cT', 'g_out', 'g_hT', 'g_cT', 'g_h0', 'g_c0')        # every form: pointer passed or NULL
REC_FLAGS = ('saved', 'gx_bt', 'g_gx_bt', 'drop')                                # K7b only (saved: acts / cs passed to the forward)
STEPS_REFUSED = {'gx_bt': -2, 'g_gx_bt': -2, 'out_drop': -2, 'drop_state': -2, 'acts': -1, 'cs': -1}   # P2C_E_SHAPE / P2C_E_NULL
RTOL, MARGIN = 1e-4, 4.0
GUARD, SENTINEL, SENTINEL_INT = 256, -7777.25, 0x5A5A5A5A
DROP_P, DROP_SITE, DROP_STATE = 0.2, 3, (0x2545F491, 0x1B873593, 7, 0)

Case = collections.namedtuple('Case', 'form H B T h0 c0 hT cT g_out g_hT g_cT g_h0 g_c0 bias saved gx_bt g_gx_bt drop sat')

# option groups: row k of a group is what value case k takes, rotated per width so that the widths do not all see the same
# combinations; every column of every group holds both values, the gradient group never drops all three
_GROUPS = [(('h0', 'c0'), ((1, 1), (1, 0), (0, 1), (0, 0))),
           (('hT', 'cT'), ((1, 0), (0, 1), (1, 1), (0, 0))),
           (('g_out', 'g_hT', 'g_cT'), ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1))),
           (('g_h0', 'g_c0'), ((1, 1), (0, 1), (1, 0), (0, 0))),
           (('bias',), (('ab',), ('a',), ('b',), ('none',))),
           (('saved',), ((1,), (1,), (0,), (1,))),
           (('gx_bt', 'g_gx_bt'), ((1, 0), (0, 1), (1, 1), (0, 0))),
           (('drop',), ((1,), (0,), (0,), (1,)))]
_VALUE_T = (5, 1, 2, 5)


def _cases():
    out = []
    for form in FORMS:
        rec = form != 'steps'
        for j, H in enumerate(WIDTHS[form]):
            for k in range(4):
                o = {}
                for gi, (names, rows) in enumerate(_GROUPS):
                    o.update(zip(names, rows[(k + j * (gi + 1)) % 4]))
                if not rec:
                    o.update(saved=1, gx_bt=0, g_gx_bt=0, drop=0)
                out.append(Case(form=form, H=H, B=B_EDGES[form][(k + 2 * j) % 4], T=_VALUE_T[(k + j) % 4], sat=False,
                                **{n: (v if n == 'bias' else bool(v)) for n, v in o.items()}))
            # T = 0: one or both initial states / incoming state gradients, every destination
            out.append(Case(form=form, H=H, B=B_EDGES[form][j % 4], T=0, h0=j % 2 == 0, c0=(j // 2) % 2 == 0, hT=True, cT=True,
                            g_out=False, g_hT=j % 2 == 1, g_cT=j % 2 == 0 or j % 4 == 3, g_h0=True, g_c0=True, bias='ab', saved=True,
                            gx_bt=rec and j % 2 == 0, g_gx_bt=rec and j % 2 == 1, drop=False, sat=False))
    return out


CASES = _cases()
STEPS_REFUSALS = [(H, what) for H in WIDTHS['steps'] for what in STEPS_REFUSED]
SATURATED = {form: Case(form=form, H=129 if form == 'steps' else 96, B=B_EDGES[form][3], T=5, h0=True, c0=True, hT=True, cT=True, g_out=True,
                        g_hT=True, g_cT=True, g_h0=True, g_c0=True, bias='ab', saved=True, gx_bt=False, g_gx_bt=False,
                        drop=form != 'steps', sat=True) for form in FORMS}
INDEPENDENT = {form: Case(form=form, H=65 if form == 'steps' else 96, B={'narrow': 5, 'wide': 17, 'steps': 33}[form], T=5, h0=True, c0=True,
                          hT=True, cT=True, g_out=True, g_hT=True, g_cT=True, g_h0=True, g_c0=True, bias='ab', saved=True,
                          gx_bt=form != 'steps', g_gx_bt=form != 'steps', drop=False, sat=False) for form in FORMS}
WORST = {form: (0.0, '') for form in FORMS}        # largest per-slice ratio seen so far, per form


def case_id(c):
    on = [n for n in FLAGS + REC_FLAGS if getattr(c, n)]
    return f'{c.form}-H{c.H}-B{c.B}-T{c.T}-bias_{c.bias}-' + '.'.join(on) + ('-sat' if c.sat else '')


def test_coverage_rule():
    """Walks CASES and STEPS_REFUSALS: every (form, H) meets every option value, every B edge of its tile and every T; a table
    with an entry taken out fails here, on any machine."""
    by = collections.defaultdict(list)
    for c in CASES:
        assert c.T <= 5 and c.B <= 65 and c.H <= 129
        assert c.T in T_VALUES and c.B in B_EDGES[c.form] and not c.sat, c
        assert c.g_out or c.g_hT or c.g_cT, c                  # a backward with no incoming gradient checks nothing
        if c.form == 'steps':
            assert c.saved and not (c.gx_bt or c.g_gx_bt or c.drop), c
        by[c.form, c.H].append(c)
    assert sorted(by) == sorted((f, H) for f in FORMS for H in WIDTHS[f])
    for (form, H), cs in by.items():
        assert {c.T for c in cs} == set(T_VALUES), (form, H)
        assert {c.B for c in cs} == set(B_EDGES[form]), (form, H)
        value = [c for c in cs if c.T > 0]                     # an option met only where no step runs has not been met
        for name in FLAGS + (REC_FLAGS if form != 'steps' else ()):
            assert {getattr(c, name) for c in value} == {False, True}, (form, H, name)
        assert {c.bias for c in value} == set(BIASES), (form, H)
        assert any(c.h0 != c.c0 for c in value) and any(c.hT != c.cT for c in value) and any(c.g_h0 != c.g_c0 for c in value), (form, H)
        zero = [c for c in cs if c.T == 0]
        assert zero and all(c.hT and c.cT and c.g_h0 and c.g_c0 for c in zero), (form, H)
    for form in FORMS:                                          # (the stated minimum, implied by the above: each B edge at one width
        for B in B_EDGES[form]:                                 # on either side of the two-chunk threshold)
            assert any(c.B == B and c.H <= 64 for c in CASES if c.form == form) and any(c.B == B and c.H > 64 for c in CASES if c.form == form)
    assert sorted(STEPS_REFUSALS) == sorted((H, what) for H in WIDTHS['steps'] for what in STEPS_REFUSED)
    for form in FORMS:
        assert SATURATED[form].sat and SATURATED[form].form == form
        assert INDEPENDENT[form].form == form and INDEPENDENT[form].B % {'narrow': 4, 'wide': 16, 'steps': 32}[form] != 0


# ---- inputs and the fp64 / fp32 reference (CPU, computed once per case, read-only) ------------------------------------------------
@functools.lru_cache(maxsize=None)
def problem(H, B, T, sat):
    """The project's scale: gx ~ 0.5 randn, W_hh ~ 0.2 randn, states and incoming gradients ~ randn. All of it is drawn whatever the
    options; a case reads what its flags select. ``sat``: gx rescaled so that its largest pre-activation is +-200."""
    g = torch.Generator().manual_seed(100003 * H + 1009 * B + 17 * T + int(sat))
    rnd = lambda *s: torch.randn(*s, generator=g)
    P = {'gx': rnd(T, B, 4 * H) * 0.5, 'w_hh': rnd(4 * H, H) * 0.2, 'h0': rnd(B, H), 'c0': rnd(B, H), 'bias_a': rnd(4 * H) * 0.3,
         'bias_b': rnd(4 * H) * 0.3, 'g_out': rnd(T, B, H), 'g_hT': rnd(B, H), 'g_cT': rnd(B, H)}
    if sat:
        P['gx'] = P['gx'] * (200.0 / P['gx'].abs().max())
    return P


def hash_mask(shape):
    from test_lstm_gpu import _hash_mask
    return _hash_mask(list(DROP_STATE), DROP_SITE, DROP_P, shape)


def bias_sum(c, P):
    """bias_a + bias_b as every form adds it, in the dtype of P (None: no bias)."""
    if c.bias == 'none':
        return None
    return P['bias_a'] + P['bias_b'] if c.bias == 'ab' else P['bias_' + c.bias]


def layer(c, P, dtype):
    """The layer step by step in ``dtype``: gates = gx[t] + (bias_a + bias_b) + h W_hh^T (i, f, g, o), c' = f c + i g, h' = o tanh c',
    the optional mask on out; the gradients by autograd of sum(out . g_out) + hT . g_hT + cT . g_cT (g_out: of out_drop with dropout)."""
    T, B, H = c.T, c.B, c.H
    Q = {k: v.to(dtype) for k, v in P.items()}
    gx = Q['gx'].clone().requires_grad_(True)
    # (a NULL initial state is a zero state: its gradient is as defined as any other's)
    h0 = (Q['h0'].clone() if c.h0 else torch.zeros(B, H, dtype=dtype)).requires_grad_(True)
    c0 = (Q['c0'].clone() if c.c0 else torch.zeros(B, H, dtype=dtype)).requires_grad_(True)
    h, cell = h0, c0
    bias, w = bias_sum(c, Q), Q['w_hh']
    outs, acts, cs = [], [], []
    for t in range(T):
        pre = gx[t] + bias if bias is not None else gx[t]
        pre = pre + h @ w.t()
        i, f, gg, o = pre.chunk(4, -1)
        i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        cell = f * cell + i * gg
        h = o * torch.tanh(cell)
        outs.append(h), acts.append(torch.cat([i, f, gg, o], -1)), cs.append(cell)
    stack = lambda xs, w_: torch.stack(xs) if xs else torch.zeros(0, B, w_, dtype=dtype)
    R = {'out': stack(outs, H), 'acts': stack(acts, 4 * H), 'cs': stack(cs, H), 'hT': h, 'cT': cell}
    seen = R['out']
    if c.drop:
        R['out_drop'] = seen = R['out'] * hash_mask((T, B, H)).to(dtype)
    loss = torch.zeros((), dtype=dtype)
    if c.g_out:
        loss = loss + (seen * Q['g_out']).sum()
    if c.g_hT:
        loss = loss + (h * Q['g_hT']).sum()
    if c.g_cT:
        loss = loss + (cell * Q['g_cT']).sum()
    grads = torch.autograd.grad(loss, [gx, h0, c0], allow_unused=True) if loss.requires_grad else (None, None, None)
    for name, g_, like in zip(('g_gx', 'g_h0', 'g_c0'), grads, (gx, h0, c0)):
        R[name] = torch.zeros_like(like) if g_ is None else g_
    return {k: v.detach() for k, v in R.items()}


@functools.lru_cache(maxsize=None)
def reference(c):
    """(fp64, fp32) evaluations of the case; the options that change no value (hT, cT, g_h0, g_c0, saved, the layouts) are
    stripped from the cache key."""
    key = c._replace(form='', hT=True, cT=True, g_h0=True, g_c0=True, saved=True, gx_bt=False, g_gx_bt=False)
    return _reference(key)


@functools.lru_cache(maxsize=None)
def _reference(c):
    P = problem(c.H, c.B, c.T, c.sat)
    return layer(c, P, torch.float64), layer(c, P, torch.float32)


# ---- the harness -----------------------------------------------------------------------------------------------------------------
class Pool:
    """Every tensor of one run inside one device allocation filled with SENTINEL, GUARD floats in front of, between and behind them
    (starts 16-byte aligned). ``snapshot`` brings the whole pool to the host once; the checks run there."""

    def __init__(self, device):
        self.device, self.at, self.size = device, {}, GUARD

    def add(self, name, shape):
        n = 1
        for s in shape:
            n *= s
        self.at[name] = (self.size, n, tuple(shape))
        self.size += (n + 3) // 4 * 4 + GUARD

    def commit(self, inputs):
        host = torch.full((self.size,), SENTINEL)
        for name, t in inputs.items():
            o, n, shape = self.at[name]
            assert tuple(t.shape) == shape, (name, t.shape, shape)
            host[o:o + n] = t.reshape(-1)
        self.before, self.inputs = host, tuple(inputs)
        self.dev = host.to(self.device)

    def ptr(self, name):
        return self.dev.data_ptr() + 4 * self.at[name][0]

    def snapshot(self, written):
        """Host copy after the run: everything outside the tensors in ``written`` -- guards, inputs, tensors behind a pointer that
        was not passed -- must hold what it held before. Returns the written tensors."""
        after = self.dev.cpu()
        keep = torch.ones(self.size, dtype=torch.bool)
        for name in written:
            o, n, _ = self.at[name]
            keep[o:o + n] = False
        same = (after.view(torch.int32) == self.before.view(torch.int32)) | ~keep          # (bits: a NaN input stays a NaN)
        if not bool(same.all()):
            first = int((~same).nonzero()[0])
            owner = [name for name, (o, n, _) in self.at.items() if o - GUARD <= first < o + n + GUARD]
            raise AssertionError(f'float {first} of the pool changed (at or next to {owner}): {float(self.before[first])} -> {float(after[first])}')
        return {name: after[self.at[name][0]:self.at[name][0] + self.at[name][1]].view(self.at[name][2]).clone() for name in written}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def launch(c, monkeypatch, P=None, tweak=None, expect=0):
    """One forward (+ one backward when acts / cs were saved) of case ``c`` on inputs ``P`` (default: the case's own). ``tweak``
    edits the descriptor before the calls; ``expect``: the code both calls must return (not 0: nothing may be written). Returns
    the written tensors on the host, plus 'state' (the four dropout words after the run) with dropout."""
    from pedestrians_video_2_carla_amd import _lib, ops
    d, lib = dev(), _lib.lib()
    T, B, H = c.T, c.B, c.H
    P = problem(H, B, T, c.sat) if P is None else P
    steps = c.form == 'steps'
    if not steps:
        monkeypatch.setenv('P2C_REC_TILE', c.form)
    pool = Pool(d)
    gx = P['gx'].transpose(0, 1).contiguous() if c.gx_bt else P['gx']
    inputs = {'gx': gx, 'w_hh': P['w_hh'], 'h0': P['h0'], 'c0': P['c0'], 'bias_a': P['bias_a'], 'bias_b': P['bias_b'], 'g_out': P['g_out'],
              'g_hT': P['g_hT'], 'g_cT': P['g_cT']}
    for name, t in inputs.items():
        pool.add(name, t.shape)
    shapes = {'out': (T, B, H), 'hT': (B, H), 'cT': (B, H), 'acts': (T, B, 4 * H), 'cs': (T, B, H), 'out_drop': (T, B, H), 'g_gx': (T, B, 4 * H),
              'g_h0': (B, H), 'g_c0': (B, H), 'g_gx_bt': (B, T, 4 * H), 'ws': (B, H)}
    for name, shape in shapes.items():
        pool.add(name, shape)
    pool.commit(inputs)
    state = torch.tensor(DROP_STATE + (SENTINEL_INT,) * 4, dtype=torch.int32, device=d)

    q = _lib.LstmDesc()
    q.T, q.B, q.H, q.gx_bt = T, B, H, int(c.gx_bt)
    q.gx, q.w_hh, q.out, q.g_gx = pool.ptr('gx'), pool.ptr('w_hh'), pool.ptr('out'), pool.ptr('g_gx')
    passed = [n for n in FLAGS if getattr(c, n)]
    passed += ['bias_a'] * (c.bias in ('a', 'ab')) + ['bias_b'] * (c.bias in ('b', 'ab')) + ['acts', 'cs'] * c.saved + ['g_gx_bt'] * c.g_gx_bt
    for name in passed:
        setattr(q, name, pool.ptr(name))
    if c.drop:
        q.out_drop, q.drop_state, q.drop_p, q.drop_site = pool.ptr('out_drop'), state.data_ptr(), DROP_P, DROP_SITE
    if tweak is not None:
        tweak(q, pool, state)
    stream = ops._stream()
    with torch.cuda.device(d):
        rc_f = (lib.p2c_lstm_steps_fwd if steps else lib.p2c_lstm_rec_fwd)(ctypes.byref(q), stream)
        rc_b = None
        if c.saved or expect:
            if steps:
                rc_b = lib.p2c_lstm_steps_bwd(ctypes.byref(q), pool.ptr('ws') if T > 1 else None, stream)     # (NULL allowed at T <= 1)
            else:
                rc_b = lib.p2c_lstm_rec_bwd(ctypes.byref(q), stream)
    torch.cuda.synchronize()
    assert rc_f == expect and rc_b in (None, expect), (case_id(c), rc_f, rc_b, expect)
    words = state.cpu().tolist()
    assert words[4:] == [SENTINEL_INT] * 4
    if expect:
        pool.snapshot([])
        assert words[:4] == list(DROP_STATE)
        return {}
    written = ['out'] + [n for n in ('hT', 'cT') if getattr(c, n)] + ['acts', 'cs'] * c.saved + ['out_drop'] * c.drop
    if c.saved:
        written += ['g_gx'] + [n for n in ('g_h0', 'g_c0', 'g_gx_bt') if getattr(c, n)] + ['ws'] * (steps and T > 1)
    got = pool.snapshot(written)
    got.pop('ws', None)
    if c.drop:          # forward: next = step + 1; backward: step = next
        assert words[:4] == list(DROP_STATE[:2]) + ([8, 8] if c.saved else [7, 8]), words
        got['state'] = words[:4]
    else:
        assert words[:4] == list(DROP_STATE)
    return got



def same_bits(a, b, what, names=None):
    for name in (names if names is not None else sorted(set(a) | set(b))):
        assert name in a and name in b, (what, name)
        if name == 'state':
            assert a[name] == b[name], (what, name)
            continue
        x, y = a[name], b[name]
        assert x.shape == y.shape, (what, name, x.shape, y.shape)
        # bit for bit: compared as integers, so that NaN equals NaN and -0 does not equal +0
        diff = x.contiguous().view(torch.int32) != y.contiguous().view(torch.int32)
        assert not bool(diff.any()), f'{what}: {name} differs in {int(diff.sum())} of {diff.numel()} elements, first at {diff.nonzero()[0].tolist()}'


def _ratio(got, ref):
    if ref.numel() == 0:
        return 0.0, 0.0
    err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
    if err != err:
        return float('inf'), scale
    if scale == 0.0:
        return (0.0 if err == 0.0 else float('inf')), scale
    return err / scale, scale


def check_values(c, got):
    """Every produced tensor against fp64: whole tensor within RTOL; every time-step slice (and gate block of g_gx / acts) within
    max(RTOL, MARGIN * e_ref). Returns the largest per-slice ratio."""
    ref64, ref32 = reference(c)
    worst, where, fails = 0.0, '', []
    for name, x in got.items():
        if name in ('state', 'g_gx_bt'):                      # (g_gx_bt: bit-equal to g_gx^T, which is checked)
            continue
        r, r32 = ref64[name], ref32[name]
        assert x.shape == r.shape, (name, x.shape, r.shape)
        assert bool(torch.isfinite(x).all()), f'{case_id(c)}: {name} is not finite'
        whole, scale = _ratio(x, r)
        if not whole <= RTOL:
            fails.append(f'{name}: {whole:.3e} of max {scale:.3e} (bound {RTOL:.1e})')
        if x.dim() != 3:
            continue
        blocks = [slice(None)] + ([slice(q * c.H, (q + 1) * c.H) for q in range(4)] if name in ('g_gx', 'acts') else [])
        for t in range(c.T):
            for bi, blk in enumerate(blocks):
                ratio, scale = _ratio(x[t][:, blk], r[t][:, blk])
                e_ref, _ = _ratio(r32[t][:, blk], r[t][:, blk])
                bound = max(RTOL, MARGIN * e_ref)
                label = f'{name}[{t}]' + (f' gate {bi - 1}' if bi else '')
                if ratio > worst:
                    worst, where = ratio, f'{label} of {case_id(c)}'
                if not ratio <= bound:
                    fails.append(f'{label}: {ratio:.3e} of max {scale:.3e} (bound {bound:.3e}, e_ref {e_ref:.3e})')
    if worst > WORST[c.form][0]:
        WORST[c.form] = (worst, where)
    print(f'per-slice ratio: this case {worst:.3e} ({where}); largest so far on {c.form}: {WORST[c.form][0]:.3e} ({WORST[c.form][1]})')
    assert not fails, f'{case_id(c)}: ' + '; '.join(fails)
    return worst


# ---- the cells -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('c', CASES, ids=case_id)
def test_cell(c, monkeypatch):
    P = problem(c.H, c.B, c.T, c.sat)
    got = launch(c, monkeypatch)
    if not c.saved:   # the forward for inference (acts = cs = NULL): the same out / hT / cT / out_drop as the run that saves them; that
        check_values(c, got)                                  # run then stands for the cell in everything below, its backward included
        c = c._replace(saved=True)
        full = launch(c, monkeypatch)
        same_bits({k: full[k] for k in got if k != 'state'}, {k: v for k, v in got.items() if k != 'state'}, 'acts / cs = NULL vs passed')
        got = full
    check_values(c, got)
    same_bits(launch(c, monkeypatch), got, 'second run')
    zeros = {k: torch.zeros_like(v) for k, v in P.items()}
    if c.T == 0:      # include/p2c.h: the states pass through
        same_bits(got, {'hT': P['h0'] if c.h0 else zeros['h0'], 'cT': P['c0'] if c.c0 else zeros['c0'],
                        'g_h0': P['g_hT'] if c.g_hT else zeros['g_hT'], 'g_c0': P['g_cT'] if c.g_cT else zeros['g_cT']}, 'T = 0',
                  names=['hT', 'cT', 'g_h0', 'g_c0'])
        return
    if c.hT:
        same_bits({'hT': got['hT']}, {'hT': got['out'][c.T - 1]}, 'hT == out[T-1]')
    if c.cT:
        same_bits({'cT': got['cT']}, {'cT': got['cs'][c.T - 1]}, 'cT == cs[T-1]')
    if c.g_gx_bt:
        same_bits({'g': got['g_gx_bt']}, {'g': got['g_gx'].transpose(0, 1)}, 'g_gx_bt == g_gx^T')
    if c.drop:
        same_bits({'o': got['out_drop']}, {'o': got['out'] * hash_mask((c.T, c.B, c.H))}, 'out_drop == out * mask')
    if c.gx_bt:
        same_bits(launch(c._replace(gx_bt=False), monkeypatch), got, 'gx_bt vs the (T,B) run')
    if c.bias != 'none':
        folded = dict(P, gx=P['gx'] + bias_sum(c, P))
        same_bits(launch(c._replace(bias='none'), monkeypatch, P=folded), got, 'biases vs gx + (bias_a + bias_b)')
    if not (c.g_out and c.g_hT and c.g_cT):
        filled = dict(P, **{n: (P[n] if getattr(c, n) else zeros[n]) for n in ('g_out', 'g_hT', 'g_cT')})
        same_bits(launch(c._replace(g_out=True, g_hT=True, g_cT=True), monkeypatch, P=filled), got, 'NULL incoming gradients vs zeros')
    if not (c.h0 and c.c0):
        filled = dict(P, **{n: (P[n] if getattr(c, n) else zeros[n]) for n in ('h0', 'c0')})
        same_bits(launch(c._replace(h0=True, c0=True), monkeypatch, P=filled), got, 'NULL initial states vs zeros')


@gpu
@pytest.mark.parametrize('form', FORMS)
def test_saturated_gates_stay_finite_and_within_the_bounds(form, monkeypatch):
    """gx scaled so that pre-activations reach +-200: exp overflows to inf inside sigmoid / tanh, the reciprocal takes it to 0 --
    every output finite (check_values asserts it) and inside the same bounds."""
    c = SATURATED[form]
    assert problem(c.H, c.B, c.T, True)['gx'].abs().max().item() == pytest.approx(200.0)
    got = launch(c, monkeypatch)
    check_values(c, got)
    sat = got['acts'][:, :, :c.H]
    assert bool((sat == 0).any()) and bool((sat == 1).any())         # the input gate did saturate both ways in fp32


@gpu
@pytest.mark.parametrize('form', FORMS)
def test_sequences_are_independent(form, monkeypatch):
    """A batch that is no multiple of the tile: every sequence's rows equal, bit for bit, the run of that sequence alone (B = 1);
    with one sequence's gx set to NaN its own rows are NaN and every other row keeps its bits."""
    c = INDEPENDENT[form]
    P = problem(c.H, c.B, c.T, False)
    got = launch(c, monkeypatch)
    check_values(c, got)
    seq = {'gx': 1, 'h0': 0, 'c0': 0, 'g_out': 1, 'g_hT': 0, 'g_cT': 0}                       # input -> its sequence axis
    axis = {'out': 1, 'acts': 1, 'cs': 1, 'g_gx': 1, 'hT': 0, 'cT': 0, 'g_h0': 0, 'g_c0': 0, 'g_gx_bt': 0}
    for b in range(c.B):
        alone = launch(c._replace(B=1), monkeypatch, P={k: (v.narrow(seq[k], b, 1).contiguous() if k in seq else v) for k, v in P.items()})
        same_bits(alone, {k: v.narrow(axis[k], b, 1) for k, v in got.items()}, f'sequence {b} alone')
    bad = 1
    poisoned = dict(P, gx=P['gx'].clone())
    poisoned['gx'][:, bad] = float('nan')
    nan = launch(c, monkeypatch, P=poisoned)
    others = [b for b in range(c.B) if b != bad]
    for name, x in nan.items():
        assert bool(torch.isnan(x.narrow(axis[name], bad, 1)).all()), f'{name}: the NaN sequence has a row that is not NaN'
        same_bits({name: x.index_select(axis[name], torch.tensor(others))}, {name: got[name].index_select(axis[name], torch.tensor(others))},
                  'next to a NaN sequence')


@gpu
@pytest.mark.parametrize('H', WIDTHS['steps'])
def test_steps_refuses_what_it_does_not_implement(H, monkeypatch):
    """K18: gx_bt, g_gx_bt, out_drop, drop_state -> P2C_E_SHAPE; acts or cs = NULL -> P2C_E_NULL; from the forward and from the
    backward, with nothing written (launch compares the whole pool and the dropout words)."""
    c = Case(form='steps', H=H, B=31, T=2, h0=True, c0=True, hT=True, cT=True, g_out=True, g_hT=True, g_cT=True, g_h0=True, g_c0=True, bias='ab',
             saved=True, gx_bt=False, g_gx_bt=False, drop=False, sat=False)
    tweaks = {'gx_bt': lambda q, pool, state: setattr(q, 'gx_bt', 1),
              'g_gx_bt': lambda q, pool, state: setattr(q, 'g_gx_bt', pool.ptr('g_gx_bt')),
              'out_drop': lambda q, pool, state: setattr(q, 'out_drop', pool.ptr('out_drop')),
              'drop_state': lambda q, pool, state: (setattr(q, 'drop_state', state.data_ptr()), setattr(q, 'drop_p', DROP_P)),
              'acts': lambda q, pool, state: setattr(q, 'acts', None),
              'cs': lambda q, pool, state: setattr(q, 'cs', None)}
    for h, what in STEPS_REFUSALS:
        if h == H:
            assert launch(c, monkeypatch, tweak=tweaks[what], expect=STEPS_REFUSED[what]) == {}
    check_values(c, launch(c, monkeypatch))                  # the same descriptor without the refused field runs
