"""GPU: the autograd Functions of ops.py with the gradients and inputs a real graph hands them, not only the contiguous ones of
``(y * up).sum()``.

Every case drives one public wrapper and sends its output through a graph construct that decides the layout of the gradient
its ``backward`` receives: ``(y * up).sum()`` (contiguous, the control), ``torch.cat`` with a random neighbour (a narrowed view,
with a storage offset for the right half -- what ``_run_stack`` of seq2seq.py does to every bidirectional LSTM layer),
``.transpose(0, 1)`` (a permuted view), ``y.sum()`` (all strides 0) and ``y.backward(buf[1:].view_as(y))`` (dense, 4 bytes into
a buffer). A tensor hook on the output records the layout that really arrived and the case asserts it. Where the wrapper takes
activation tensors they are also passed as transposed / narrowed / strided views of the same values.

Three assertions per case:
1. outputs and every gradient against the fp64 CPU reference of the op's own test file (torch.nn.LSTM / GRU, the written-out
   formulas, the oracle), within that file's tolerance -- imported from it where it is a module-level helper, repeated by
   number where it sits inside a test;
2. ``torch.equal`` with a second run that is fed ``gradient.contiguous()`` and contiguous inputs: a layout changes no bit;
3. pointer lifetime (fixture ``lifetimes``): every tensor ``ops._require_device`` or a ``.contiguous()`` call inside ops.py had
   to create is still alive at the next ``p2c_*`` call -- the launch that reads its pointer. Deterministic: it asks Python
   whether the object exists, not the allocator what it did with the memory. The same fixture asserts that a contiguous
   fp32 device tensor comes back from ``_require_device`` as the same object (no copy and no launch on the hot path).
"""
import copy
import functools
import os
import sys
import types
import weakref

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import pose_head as O  # noqa: E402
from test_baseline_3d_pose_gpu import close as bn_close  # noqa: E402
from test_decoder_wide_gpu import _cell  # noqa: E402
from test_embed_gpu import close as embed_close, reference as embed_reference  # noqa: E402
from test_flow_gpu import close as flow_close  # noqa: E402
from test_gemm_gpu import gelu64, rel  # noqa: E402
from test_gru_gpu import close as gru_close  # noqa: E402
from test_lstm_gpu import close as lstm_close  # noqa: E402
from test_lstm_model_gpu import close as lstm_steps_close  # noqa: E402
from test_mlp_gpu import close as mlp_close  # noqa: E402
from test_pose_head_gpu import _random_case, close as pose_close  # noqa: E402
from test_relu_stack_gpu import close as relu_close, problem as relu_problem  # noqa: E402
from test_simple_transformer_gpu import close as encoder_close  # noqa: E402

pytestmark = pytest.mark.gpu

LAYOUTS = ('contiguous', 'cat_left', 'cat_right', 'transposed', 'expanded', 'offset')
NARROW = 3          # floats in front of a narrowed input view: 12 bytes, so the view is not 16-byte aligned either

# A copy that may die before the next p2c_* call: label of the site -> why that is right. (None so far.)
MAY_DIE = {}


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


# ----------------------------------------------------------------------------------------------------------------------
# assertion 3: pointer lifetime
# ----------------------------------------------------------------------------------------------------------------------
_QUERIES = ('workspace', 'supported', '_floats', '_bytes', 'image_index', 'version', '_set_')


class Lifetimes:
    """Weak references to the tensors ops.py had to create to get a dense fp32 device operand, checked at every p2c_* call."""

    def __init__(self):
        self.pending, self.faults, self.same_object, self.calls = [], [], 0, 0

    def note(self, t, label):
        self.pending.append((weakref.ref(t), label))

    def at_call(self, name):
        self.calls += 1
        for r, label in self.pending:
            if r() is None and not any(k in label for k in MAY_DIE):
                self.faults.append(f'lifetime: the copy made by {label} was freed before {name}')
        if not any(q in name for q in _QUERIES):      # a launch: what it reads was alive when it was issued
            self.pending = []
        else:                                         # a host-side question: report each dead copy once, keep the live ones
            self.pending = [(r, label) for r, label in self.pending if r() is not None]

    def drain(self):
        faults, self.faults = self.faults, []
        return faults


class _Watching:
    """The library handle with every p2c_* entry point announced to ``Lifetimes`` first (as ``Counting`` of test_cls_head_gpu.py)."""

    def __init__(self, handle, watch):
        self._h, self._watch = handle, watch

    def __getattr__(self, name):
        fn = getattr(self._h, name)
        if not name.startswith('p2c_'):
            return fn

        def call(*args):
            self._watch.at_call(name)
            return fn(*args)
        return call


@pytest.fixture(autouse=True)
def lifetimes(monkeypatch):
    from pedestrians_video_2_carla_amd import _lib, ops
    watch = Lifetimes()
    require, contiguous, ops_file = ops._require_device, torch.Tensor.contiguous, ops.__file__

    def watched_require(t, name, dtype=torch.float32):
        r = require(t, name, dtype)
        if t.is_cuda and t.dtype == dtype and t.is_contiguous():
            assert r is t, f'_require_device({name!r}) copied a contiguous {dtype} device tensor'
            watch.same_object += 1
        if r is not t:
            watch.note(r, f'_require_device({name!r})')
        return r

    def watched_contiguous(self, *args, **kwargs):
        r = contiguous(self, *args, **kwargs)
        frame = sys._getframe(1)
        if r is not self and frame.f_code.co_filename == ops_file and frame.f_code.co_name != '_require_device':
            watch.note(r, f'.contiguous() in ops.{frame.f_code.co_name}')
        return r

    monkeypatch.setattr(ops, '_require_device', watched_require)
    monkeypatch.setattr(torch.Tensor, 'contiguous', watched_contiguous)
    monkeypatch.setattr(_lib, '_lib', _Watching(_lib.lib(), watch))
    yield watch
    assert not watch.faults, '\n'.join(watch.faults)


# ----------------------------------------------------------------------------------------------------------------------
# one op = one Problem; the runner below is the same for all of them
# ----------------------------------------------------------------------------------------------------------------------
class Problem:
    """acts / params: name -> fp64 CPU tensor (an act may be None: the optional input is absent). ``dev_fn(A, P)`` calls the
    wrapper on fp32 device tensors, ``ref_fn(A, P)`` the reference on the fp64 ones; both return a tuple of outputs.
    ``check(kind, name, got, want)``: the op's own tolerance, kind 'out' or 'grad'. ``views``: act -> how it is passed when the
    case asks for input views. ``data``: acts without a gradient. ``aux``: outputs that ride along through a transposed
    construct (hT, cT). ``scalars``: 0-dim outputs (a layout means nothing for them but the offset). ``nondiff``: outputs that are
    compared and never used in a loss."""

    def __init__(self, acts, params, dev_fn, ref_fn, check, views=None, data=(), aux=(), scalars=(), nondiff=(), n_out=1):
        self.acts, self.params, self.dev_fn, self.ref_fn, self.check = acts, params, dev_fn, ref_fn, check
        self.views, self.data, self.aux, self.scalars, self.nondiff, self.n_out = views or {}, set(data), set(aux), set(scalars), set(nondiff), n_out

    def layouts(self, layout, used=None):
        out = []
        for i in range(self.n_out):
            if i in self.nondiff or (used is not None and i not in used):
                out.append(None)
            elif i in self.scalars:
                out.append('offset' if layout == 'offset' else 'contiguous')
            elif i in self.aux and layout not in ('contiguous', 'offset'):
                out.append('transposed')
            else:
                out.append(layout)
        return out

    def applicable(self, layout):
        return layout in ('contiguous', 'offset') or self.n_out > len(self.scalars | self.nondiff)


def _as_view(val, kind):
    """(leaf, leaf -> the tensor handed to the op, gradient of the leaf -> gradient of the value)."""
    junk = lambda *shape: torch.full(shape, 7.0, device=val.device)      # noqa: E731
    if kind is None:
        return val.clone(), (lambda l: l), (lambda g: g)
    if kind == 'transposed':
        return val.transpose(0, 1).contiguous(), (lambda l: l.transpose(0, 1)), (lambda g: g.transpose(0, 1))
    if kind == 'narrowed':
        return torch.cat([junk(*val.shape[:-1], NARROW), val], -1), (lambda l: l[..., NARROW:]), (lambda g: g[..., NARROW:])
    if kind == 'strided':
        return torch.stack([val, junk(*val.shape)], -1), (lambda l: l[..., 0]), (lambda g: g[..., 0])
    raise KeyError(kind)


def _dense_strides(shape):
    st, n = [], 1
    for s in reversed(shape):
        st.append(n)
        n *= s
    return tuple(reversed(st))


def layout_fault(layout, rec, shape):
    """None if the gradient that reached the op has the layout the construct promises."""
    contig, stride, offset, ptr16 = rec
    if layout == 'contiguous':
        ok = contig and offset == 0
    elif layout in ('cat_left', 'cat_right'):
        wide = _dense_strides(tuple(shape[:-1]) + (2 * shape[-1],))
        ok = not contig and stride == wide and offset == (shape[-1] if layout == 'cat_right' else 0)
    elif layout == 'transposed':
        t = _dense_strides((shape[1], shape[0]) + tuple(shape[2:]))
        ok = not contig and stride == (t[1], t[0]) + t[2:] and offset == 0
    elif layout == 'expanded':
        ok = not contig and all(s == 0 for s in stride)
    else:
        ok = contig and offset == 1 and ptr16 % 16 == 4
    return None if ok else f'layout: {layout} delivered contiguous={contig} stride={stride} offset={offset} ptr%16={ptr16} for shape {tuple(shape)}'


def run(prob, layouts, views, feed=None, seed=0):
    """One forward + backward on the device. ``feed``: output index -> gradient handed over as it is."""
    d = dev()
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(tuple(shape), generator=gen).to(d)      # noqa: E731
    P = {n: v.float().to(d).requires_grad_(True) for n, v in prob.params.items()}
    A, leaves = {}, {}
    for n, v in prob.acts.items():
        if v is None:
            A[n] = None
            continue
        leaf, view, unview = _as_view(v.float().to(d), prob.views.get(n) if views else None)
        leaf.requires_grad_(n not in prob.data)
        A[n], leaves[n] = view(leaf), (leaf, unview)
        if views and n in prob.views and v.numel() > 1:
            assert not A[n].is_contiguous(), n
    outs = prob.dev_fn(A, P)
    outs = outs if isinstance(outs, tuple) else (outs,)
    assert len(outs) == prob.n_out
    rec, G, keep = {}, {}, []

    def hook(i):
        def fn(g):
            rec[i] = (g.is_contiguous(), tuple(g.stride()), g.storage_offset(), g.data_ptr() % 16)
            G[i] = g.clone(memory_format=torch.contiguous_format)
        return fn
    tensors, grads = [], []
    for i, (y, layout) in enumerate(zip(outs, layouts)):
        if layout is None:
            continue
        y.register_hook(hook(i))
        if feed is not None:
            tensors.append(y), grads.append(feed[i])
        elif layout == 'contiguous':
            tensors.append((y * rnd(*y.shape)).sum()), grads.append(None)
        elif layout in ('cat_left', 'cat_right'):
            other = rnd(*y.shape)
            both = torch.cat([y, other] if layout == 'cat_left' else [other, y], -1)
            tensors.append((both * rnd(*both.shape)).sum()), grads.append(None)
        elif layout == 'transposed':
            yt = y.transpose(0, 1)
            tensors.append((yt * rnd(*yt.shape)).sum()), grads.append(None)
        elif layout == 'expanded':
            tensors.append(y.sum()), grads.append(None)
        else:
            buf = rnd(y.numel() + 1)
            keep.append(buf)
            tensors.append(y), grads.append(buf[1:].view_as(y))
    torch.autograd.backward(tensors, grads)
    torch.cuda.synchronize() if d.type == 'cuda' else None
    agrad = {n: (None if leaf.grad is None else unview(leaf.grad)) for n, (leaf, unview) in leaves.items() if n not in prob.data}
    return types.SimpleNamespace(outs=[o.detach() for o in outs], rec=rec, G=G, agrad=agrad, pgrad={n: p.grad for n, p in P.items()},
                                 keep=(keep, A, P, leaves, outs))


def reference(prob, G):
    A = {n: (None if v is None else v.clone().requires_grad_(n not in prob.data)) for n, v in prob.acts.items()}
    P = {n: v.clone().requires_grad_(True) for n, v in prob.params.items()}
    outs = prob.ref_fn(A, P)
    outs = outs if isinstance(outs, tuple) else (outs,)
    names = [('a', n) for n, v in A.items() if v is not None and n not in prob.data] + [('p', n) for n in P]
    wrt = [A[n] if k == 'a' else P[n] for k, n in names]
    used = sorted(G)
    grads = torch.autograd.grad([outs[i] for i in used], wrt, [G[i].double().cpu() for i in used], allow_unused=True)
    return [o.detach() for o in outs], {kn: g for kn, g in zip(names, grads)}


def check_case(prob, layout, views, watch, used=None):
    assert prob.applicable(layout), 'an op with only 0-dim outputs has no such layout: cases() leaves it out'
    layouts = prob.layouts(layout, used)
    a = run(prob, layouts, views)
    faults = watch.drain()
    for i, want in enumerate(layouts):
        if want is None:
            continue
        if i not in a.rec:
            faults.append(f'layout: no gradient reached output {i}')
            continue
        fault = layout_fault(want, a.rec[i], a.outs[i].shape)
        if fault:
            faults.append(fault)
    # 1. against fp64
    ref_outs, ref_grads = reference(prob, a.G)

    def judge(kind, name, got, want):
        try:
            if want is None:
                assert got is None or not bool(got.any()), f'{name}: the reference has no gradient here'
            else:
                assert got is not None, f'{name}: no gradient'
                prob.check(kind, name, got, want)
        except AssertionError as e:
            faults.append(f'fp64: {e}')
    for i, (got, want) in enumerate(zip(a.outs, ref_outs)):
        judge('out', f'output {i}', got, want)
    for (k, n), want in ref_grads.items():
        judge('grad', f'grad {n}', a.agrad[n] if k == 'a' else a.pgrad[n], want)
    # 2. the same bits from contiguous gradients and inputs
    b = run(prob, layouts, False, feed=a.G)
    faults += watch.drain()
    pairs = [(f'output {i}', x, y) for i, (x, y) in enumerate(zip(a.outs, b.outs))]
    pairs += [(f'grad {n}', a.agrad[n], b.agrad[n]) for n in a.agrad] + [(f'grad {n}', a.pgrad[n], b.pgrad[n]) for n in a.pgrad]
    for name, x, y in pairs:
        if (x is None) != (y is None) or (x is not None and not torch.equal(x, y)):
            faults.append(f'bits: {name} differs from the run on contiguous tensors'
                          + ('' if x is None or y is None else f' by {float((x - y).abs().max()):.3e}'))
    assert watch.calls > 0, 'no p2c_* call was seen: the wrapper did not reach the library'
    assert not faults, '\n'.join(faults)


def _within(a, b, what, rtol):
    """max |a - b| <= rtol max |b|: the bound the tests of test_pose_former_gpu.py state inline."""
    err = rel(a, b)
    assert err == err and err <= rtol, f'{what}: {err:.3e} of the scale (bound {rtol:.1e})'


def _checker(close, out, grad):
    def check(kind, name, got, want):
        close(got, want, name, out if kind == 'out' else (grad(name) if callable(grad) else grad))
    return check


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _bind(module, P):
    """``module`` with its parameters replaced by the leaves of P (the wrappers read attributes, they never call forward)."""
    for name, t in P.items():
        *path, leaf = name.split('.')
        m = module
        for part in path:
            m = getattr(m, part)
        m._parameters[leaf] = t
    return module


# ------------------------------------------------------------------------------------------------------------ recurrences
@functools.lru_cache(maxsize=None)
def lstm_problem(H, with_state):
    """K7b for H = 16, K18 for H = 20: T, B, I = 3, 5, 7 against torch.nn.LSTM in fp64 (test_lstm_gpu.py / test_lstm_model_gpu.py)."""
    T, B, I = 3, 5, 7
    torch.manual_seed(T * 100 + B + H)
    ref = torch.nn.LSTM(I, H).double()
    g = _g(H)
    acts = {'x': _randn(g, T, B, I), 'h0': _randn(g, B, H) if with_state else None, 'c0': _randn(g, B, H) if with_state else None}
    params = {n: p.detach().clone() for n, p in ref.named_parameters()}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        assert ops.lstm_supported(H) == (H == 16)
        return ops.lstm_layer(A['x'], A['h0'], A['c0'], P['weight_ih_l0'], P['weight_hh_l0'], P['bias_ih_l0'], P['bias_hh_l0'])

    def ref_fn(A, P):
        state = None if A['h0'] is None else (A['h0'][None], A['c0'][None])
        out, (h, c) = torch.func.functional_call(ref, P, (A['x'], state))
        return out, h[0], c[0]
    close = lstm_close if H == 16 else lstm_steps_close
    return Problem(acts, params, dev_fn, ref_fn, _checker(close, 1e-4, 1e-4), views={'x': 'transposed', 'h0': 'transposed', 'c0': 'transposed'},
                   aux=(1, 2), n_out=3)


@functools.lru_cache(maxsize=None)
def gru_problem(with_state):
    """K23: T, B, I, H = 3, 5, 7, 20 against torch.nn.GRU in fp64 (test_gru_gpu.py)."""
    T, B, I, H = 3, 5, 7, 20
    torch.manual_seed(T * 1000 + B + H)
    ref = torch.nn.GRU(I, H).double()
    g = _g(23)
    acts = {'x': _randn(g, T, B, I), 'h0': _randn(g, B, H) if with_state else None}
    params = {n: p.detach().clone() for n, p in ref.named_parameters()}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.gru_layer(A['x'], A['h0'], P['weight_ih_l0'], P['weight_hh_l0'], P['bias_ih_l0'], P['bias_hh_l0'])

    def ref_fn(A, P):
        out, h = torch.func.functional_call(ref, P, (A['x'],) if A['h0'] is None else (A['x'], A['h0'][None]))
        return out, h[0]
    return Problem(acts, params, dev_fn, ref_fn, _checker(gru_close, 1e-4, 1e-4), views={'x': 'transposed', 'h0': 'transposed'},
                   aux=(1,), n_out=2)


@functools.lru_cache(maxsize=None)
def encoder_stack_problem():
    """B, T, I, H = 5, 3, 5, 16 against torch.nn.LSTM(num_layers=2) in fp64; outputs 1e-4, gradients 2e-4 (test_lstm_gpu.py)."""
    B, T, I, H = 5, 3, 5, 16
    torch.manual_seed(T * 3 + B)
    ref = torch.nn.LSTM(I, H, num_layers=2).double()
    acts = {'x': _randn(_g(1), B, T, I)}
    params = {n: p.detach().clone() for n, p in ref.named_parameters()}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.encoder_stack(A['x'], types.SimpleNamespace(dropout=0.0, training=False, **P))

    def ref_fn(A, P):
        _, (h, c) = torch.func.functional_call(ref, P, (A['x'].transpose(0, 1),))
        return h, c
    return Problem(acts, params, dev_fn, ref_fn, _checker(lstm_close, 1e-4, 2e-4), views={'x': 'transposed'}, data=('x',), n_out=2)


def _decoder_formula(T, k0, c0, k1, c1, w_ih0, w_ih1, w_fc, b_fc):
    x, outs = torch.zeros(k0.shape[0], w_fc.shape[0], dtype=k0.dtype), []
    for _ in range(T):
        h0 = _cell(x @ w_ih0.t() + k0, c0)
        h1 = _cell(h0 @ w_ih1.t() + k1, c1)
        x = h1 @ w_fc.t() + b_fc
        outs.append(x)
    return outs


@functools.lru_cache(maxsize=None)
def decoder_loop_problem():
    """K7c: T, B, O = 3, 5, 12 at its only hidden size, 64, against the per-step formula in fp64; output 1e-4, gradients 2e-4."""
    T, B, O, H = 3, 5, 12, 64
    g = _g(T * 7 + B)
    acts = {'k0': _randn(g, B, 4 * H, scale=0.3), 'c0': _randn(g, B, H, scale=0.3), 'k1': _randn(g, B, 4 * H, scale=0.3),
            'c1': _randn(g, B, H, scale=0.3)}
    params = {'w_ih0': _randn(g, 4 * H, O, scale=0.3), 'w_ih1': _randn(g, 4 * H, H, scale=0.3), 'w_fc': _randn(g, O, H, scale=0.3),
              'b_fc': _randn(g, O, scale=0.3)}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.decoder_loop(A['k0'], A['c0'], A['k1'], A['c1'], P['w_ih0'], P['w_ih1'], P['w_fc'], P['b_fc'], T)

    def ref_fn(A, P):
        return torch.stack(_decoder_formula(T, A['k0'], A['c0'], A['k1'], A['c1'], P['w_ih0'], P['w_ih1'], P['w_fc'], P['b_fc']))
    return Problem(acts, params, dev_fn, ref_fn, _checker(lstm_close, 1e-4, 2e-4), views={n: 'transposed' for n in acts})


@functools.lru_cache(maxsize=None)
def decoder_stack_problem():
    """The decoder from the encoder state: T, B, O = 3, 5, 12, H = 64, output batch-first; output 1e-4, gradients 2e-4."""
    T, B, O, H = 3, 5, 12, 64
    g = _g(T * 11 + B)
    torch.manual_seed(T * 11 + B)
    rnn, fc = torch.nn.LSTM(O, H, num_layers=2).double(), torch.nn.Linear(H, O).double()
    acts = {'hidden': _randn(g, 2, B, H, scale=0.3), 'cell': _randn(g, 2, B, H, scale=0.3)}
    params = {'rnn.' + n: p.detach().clone() for n, p in rnn.named_parameters()}
    params.update({'fc.' + n: p.detach().clone() for n, p in fc.named_parameters()})

    def split(P):
        return ({n[4:]: p for n, p in P.items() if n.startswith('rnn.')}, {n[3:]: p for n, p in P.items() if n.startswith('fc.')})

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        r, f = split(P)
        return ops.decoder_stack(A['hidden'], A['cell'], types.SimpleNamespace(**r), types.SimpleNamespace(**f), T)

    def ref_fn(A, P):
        r, f = split(P)
        k0 = A['hidden'][0] @ r['weight_hh_l0'].t() + r['bias_ih_l0'] + r['bias_hh_l0']
        k1 = A['hidden'][1] @ r['weight_hh_l1'].t() + r['bias_ih_l1'] + r['bias_hh_l1']
        return torch.stack(_decoder_formula(T, k0, A['cell'][0], k1, A['cell'][1], r['weight_ih_l0'], r['weight_ih_l1'], f['weight'],
                                            f['bias']), 1)
    return Problem(acts, params, dev_fn, ref_fn, _checker(lstm_close, 1e-4, 2e-4), views={'hidden': 'transposed', 'cell': 'transposed'})


# ------------------------------------------------------------------------------------------------------------ front ends
@functools.lru_cache(maxsize=None)
def joint_embeddings_problem():
    """K7a: B, T, J, C, E = 3, 4, 5, 2, 8 against test_embed_gpu.reference."""
    B, T, J, C, E = 3, 4, 5, 2, 8
    g = _g(B * 131 + T)
    acts = {'x': _randn(g, B, T, J, C)}
    params = {f'w{j}': _randn(g, E, C, scale=0.3) for j in range(J)}
    params.update({f'b{j}': _randn(g, E, scale=0.3) for j in range(J)})
    lists = lambda P: ([P[f'w{j}'] for j in range(J)], [P[f'b{j}'] for j in range(J)])      # noqa: E731

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.joint_embeddings(A['x'], *lists(P), flip=True)
    return Problem(acts, params, dev_fn, lambda A, P: embed_reference(A['x'], *lists(P), True), _checker(embed_close, 1e-4, 1e-4),
                   views={'x': 'transposed'}, data=('x',))


def _relu_layers(P, n):
    return [P[f'w{l}'] for l in range(n)], [P[f'b{l}'] for l in range(n)]


@functools.lru_cache(maxsize=None)
def relu_stack_problem():
    """K21: dims (7, 9, 5), B, T = 3, 4, on the kink-free frames of test_relu_stack_gpu.problem."""
    x, ws, bs, _ = relu_problem((7, 9, 5), 3, 4)
    params = {f'w{l}': w.double() for l, w in enumerate(ws)}
    params.update({f'b{l}': b.double() for l, b in enumerate(bs)})

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.relu_stack(A['x'], *_relu_layers(P, 2), flip=True)

    def ref_fn(A, P):
        h = A['x']
        for w, b in zip(*_relu_layers(P, 2)):
            h = torch.relu(h @ w.T + b)
        return h.permute(1, 0, 2).flip(0)
    return Problem({'x': x.double()}, params, dev_fn, ref_fn, _checker(relu_close, 1e-4, 1e-4), views={'x': 'transposed'}, data=('x',))


@functools.lru_cache(maxsize=None)
def dense_chain_problem():
    """K16 + K12 composition: the same kink-free frames as 12 rows through 7 -> 9 -> 5 with both ReLUs (test_flat_models_gpu.py: 1e-4)."""
    x, ws, bs, _ = relu_problem((7, 9, 5), 3, 4)
    params = {f'w{l}': w.double() for l, w in enumerate(ws)}
    params.update({f'b{l}': b.double() for l, b in enumerate(bs)})

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.dense_chain(A['x'], *_relu_layers(P, 2), (True, True))

    def ref_fn(A, P):
        h = A['x']
        for w, b in zip(*_relu_layers(P, 2)):
            h = torch.relu(h @ w.T + b)
        return h
    return Problem({'x': x.double().reshape(12, 7)}, params, dev_fn, ref_fn, _checker(relu_close, 1e-4, 1e-4), views={'x': 'transposed'})


@functools.lru_cache(maxsize=None)
def fused_mlp_problem():
    """K8 at the odd stack 7 -> 33 -> 5 of test_mlp_gpu.py over 37 rows; 2e-5."""
    dims, rows = (7, 33, 5), 37
    g = _g(0)
    params = {f'w{l}': _randn(g, o, i, scale=i ** -0.5) for l, (i, o) in enumerate(zip(dims[:-1], dims[1:]))}
    params.update({f'b{l}': _randn(g, o, scale=0.3) for l, o in enumerate(dims[1:])})

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        assert ops.mlp_supported(dims)
        return ops.fused_mlp(A['x'], *_relu_layers(P, 2))

    def ref_fn(A, P):
        (w0, w1), (b0, b1) = _relu_layers(P, 2)
        return torch.relu(A['x'] @ w0.T + b0) @ w1.T + b1
    return Problem({'x': _randn(g, rows, dims[0])}, params, dev_fn, ref_fn, _checker(mlp_close, 2e-5, 2e-5), views={'x': 'narrowed'},
                   data=('x',))


def _dense_acts(g, rows, din, dout, per):
    return {'x': _randn(g, rows, din, scale=0.5), 'residual': _randn(g, rows, dout),
            'scale': (torch.rand(rows // per, generator=g) > 0.25).double() / 0.75}


def _gemm_check(kind, name, got, want):
    _within(got, want, name, 2e-5 if kind == 'out' else 5e-5)      # test_gemm_gpu.py: test_fused_dense_and_mlp_gradients_match_autograd_fp64


@functools.lru_cache(maxsize=None)
def dense_problem():
    """ops.dense with the per-sample factor and the residual: 36 rows, 12 -> 20, three rows per factor."""
    rows, din, dout, per = 36, 12, 20, 3
    g = _g(rows)
    params = {'w': _randn(g, dout, din, scale=din ** -0.5), 'b': _randn(g, dout, scale=0.1)}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.dense(A['x'], P['w'], P['b'], A['scale'], per, A['residual'])

    def ref_fn(A, P):
        return (A['x'] @ P['w'].t() + P['b']) * A['scale'].repeat_interleave(per).view(-1, 1) + A['residual']
    return Problem(_dense_acts(g, rows, din, dout, per), params, dev_fn, ref_fn, _gemm_check,
                   views={'x': 'narrowed', 'residual': 'transposed', 'scale': 'strided'}, data=('scale',))


@functools.lru_cache(maxsize=None)
def mlp_gelu_problem():
    """ops.mlp_gelu: 36 rows, 12 -> 20 -> 12, three rows per factor."""
    rows, din, dhid, per = 36, 12, 20, 3
    g = _g(rows + 1)
    params = {'w1': _randn(g, dhid, din, scale=din ** -0.5), 'b1': _randn(g, dhid, scale=0.1),
              'w2': _randn(g, din, dhid, scale=dhid ** -0.5), 'b2': _randn(g, din, scale=0.1)}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.mlp_gelu(A['x'], P['w1'], P['b1'], P['w2'], P['b2'], A['scale'], per, A['residual'])

    def ref_fn(A, P):
        return ((gelu64(A['x'] @ P['w1'].t() + P['b1']) @ P['w2'].t() + P['b2']) * A['scale'].repeat_interleave(per).view(-1, 1)
                + A['residual'])
    return Problem(_dense_acts(g, rows, din, din, per), params, dev_fn, ref_fn, _gemm_check,
                   views={'x': 'narrowed', 'residual': 'transposed', 'scale': 'strided'}, data=('scale',))


# ------------------------------------------------------------------------------------------------------------ norms
@functools.lru_cache(maxsize=None)
def layer_norm_problem():
    """K15: 37 rows x 20 against torch.nn.functional.layer_norm in fp64; test_pose_former_gpu.py: y 2e-5, d x 5e-5, d gamma / d beta
    5e-5 sqrt(rows)."""
    rows, D = 37, 20
    g = _g(rows + D)
    params = {'weight': _randn(g, D), 'bias': _randn(g, D)}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        assert ops.layer_norm_supported(A['x'], D)
        return ops.layer_norm(A['x'], P['weight'], P['bias'], 1e-6)

    def check(kind, name, got, want):
        _within(got, want, name, 2e-5 if kind == 'out' else (5e-5 if name == 'grad x' else 5e-5 * rows ** 0.5))
    return Problem({'x': _randn(g, rows, D, scale=2.0) + 0.5}, params, dev_fn,
                   lambda A, P: torch.nn.functional.layer_norm(A['x'], (D,), P['weight'], P['bias'], 1e-6), check, views={'x': 'transposed'})


@functools.lru_cache(maxsize=None)
def batch_norm_act_problem():
    """K19 in training with the residual: 37 rows x 7 against relu(batch_norm) + residual in fp64 (test_baseline_3d_pose_gpu.py: 1e-4).
    y itself stays contiguous: a strided y is outside ``batch_norm_act_supported`` and belongs to the framework ops."""
    N, C = 37, 7
    g = _g(N * 7 + C)
    acts = {'y': _randn(g, N, C, scale=2.0) + 1.0, 'residual': _randn(g, N, C)}
    params = {'weight': torch.rand(C, generator=g, dtype=torch.float64) + 0.5, 'bias': _randn(g, C, scale=0.5)}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        d = A['y'].device
        bn = types.SimpleNamespace(training=True, momentum=0.1, eps=1e-5, track_running_stats=True, affine=True, num_features=C,
                                   weight=P['weight'], bias=P['bias'], running_mean=torch.zeros(C, device=d),
                                   running_var=torch.ones(C, device=d), num_batches_tracked=torch.zeros((), dtype=torch.long, device=d))
        assert ops.batch_norm_act_supported(A['y'], bn)
        return ops.batch_norm_act(A['y'], bn, 0.0, None, 0, residual=A['residual'])

    def ref_fn(A, P):
        return torch.relu(torch.nn.functional.batch_norm(A['y'], None, None, P['weight'], P['bias'], True, 0.1, 1e-5)) + A['residual']
    return Problem(acts, params, dev_fn, ref_fn, _checker(bn_close, 1e-4, 1e-4), views={'residual': 'transposed'})


def _pose_former_check(kind, name, got, want):
    _within(got, want, name, 1e-5 if kind == 'out' else 5e-5)      # test_frame_mean_and_row_parameter_ops_match_fp64


@functools.lru_cache(maxsize=None)
def add_row_parameter_problem():
    B, F, C = 5, 3, 8
    g = _g(B + F)

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.add_row_parameter(A['x'], P['p'])
    return Problem({'x': _randn(g, B, F, C)}, {'p': _randn(g, 1, F, C)}, dev_fn, lambda A, P: A['x'] + P['p'], _pose_former_check,
                   views={'x': 'transposed'})


@functools.lru_cache(maxsize=None)
def frame_mean_problem():
    """p2c_frame_mean_fwd + K12 behind it: B, F, C = 5, 3, 8; w a stride-2 view in the input-view cases (b holds one float: any view
    of it is dense, it is passed 4 bytes into a buffer)."""
    B, F, C = 5, 3, 8
    g = _g(B + F + 1)
    acts = {'x': _randn(g, B, F, C), 'w': _randn(g, F), 'b': _randn(g, 1)}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.frame_mean(A['x'], A['w'], A['b'])
    return Problem(acts, {}, dev_fn, lambda A, P: (A['x'] * A['w'].view(1, F, 1)).sum(1) + A['b'], _pose_former_check,
                   views={'x': 'transposed', 'w': 'strided', 'b': 'narrowed'})


@functools.lru_cache(maxsize=None)
def normalize_problem():
    """K4: 20 frames of 26 joints x 2 against the oracle's Normalizer (test_flow_gpu.py: 1e-4); shift and scale carry no gradient."""
    g = _g(1)

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.normalize(A['x'], 'hips_neck_bbox')
    return Problem({'x': _randn(g, 4, 5, 26, 2, scale=30.0) + 200.0}, {}, dev_fn, lambda A, P: O.normalize(A['x'], 'hips_neck_bbox'),
                   _checker(flow_close, 1e-4, 1e-4), views={'x': 'transposed'}, nondiff=(1, 2), n_out=3)


@functools.lru_cache(maxsize=None)
def loss_loc_2d_problem():
    """K3: 35 frames, BODY_25 targets against CARLA predictions (test_flow_gpu.py: 1e-4). The output is 0-dim."""
    from pedestrians_video_2_carla_amd.data.base.skeleton import get_common_indices
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    g = _g(3)
    out_idx, in_idx = get_common_indices(input_nodes=BODY_25_SKELETON, output_nodes=CARLA_SKELETON)
    hips_col = in_idx.index(BODY_25_SKELETON.MidHip.value)
    pred, gt = _randn(g, 7, 5, 26, 3), _randn(g, 7, 5, 25, 2)
    gt[torch.rand(7, 5, 25, generator=g) < 0.2] = 0

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        return ops.loss_loc_2d(A['pred'], A['gt'], out_idx, in_idx, hips_col, True)
    return Problem({'pred': pred, 'gt': gt}, {}, dev_fn, lambda A, P: O.loss_loc_2d(A['pred'], A['gt'], out_idx, in_idx, hips_col, True)[0],
                   _checker(flow_close, 1e-4, 1e-4), views={'pred': 'transposed', 'gt': 'transposed'}, data=('gt',), scalars=(0,))


# ------------------------------------------------------------------------------------------------------------ transformers
def _attention64(qkv, scale):
    S, N, _, heads, hd = qkv.shape
    q, k, v = qkv.permute(2, 0, 3, 1, 4)
    return (torch.softmax(q @ k.transpose(-1, -2) * scale, -1) @ v).transpose(1, 2).reshape(S, N, heads * hd)


@functools.lru_cache(maxsize=None)
def small_attention_problem():
    """K14: S, N, heads, head_dim = 3, 2, 1, 4 -- two tokens, one head of the narrowest row -- against softmax(q k^T) v in fp64; 1e-5
    (test_pose_former_gpu.py)."""
    S, N, heads, hd = 3, 2, 1, 4

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        assert ops.small_attention_supported(N, heads, hd)
        return ops.small_attention(A['qkv'], hd ** -0.5)
    return Problem({'qkv': _randn(_g(S * 31 + N), S, N, 3, heads, hd)}, {}, dev_fn, lambda A, P: _attention64(A['qkv'], hd ** -0.5),
                   lambda kind, name, got, want: _within(got, want, name, 1e-5), views={'qkv': 'transposed'})


@functools.lru_cache(maxsize=None)
def transformer_block_problem():
    """One pre-norm block as one node: S, N, C = 3, 2, 4 with one head and both stochastic-depth factors, against the written-out
    formula in fp64; y 2e-5, gradients 1e-4 (test_pose_former_gpu.py)."""
    S, N, C, heads, hid = 3, 2, 4, 1, 8
    torch.manual_seed(S + C)
    ref = torch.nn.ModuleDict({'norm1': torch.nn.LayerNorm(C, eps=1e-6), 'qkv': torch.nn.Linear(C, 3 * C), 'proj': torch.nn.Linear(C, C),
                               'norm2': torch.nn.LayerNorm(C, eps=1e-6), 'fc1': torch.nn.Linear(C, hid), 'fc2': torch.nn.Linear(hid, C)}).double()
    g = _g(S + C)
    params = {n: p.detach().clone() + _randn(g, *p.shape, scale=0.05) for n, p in ref.named_parameters()}
    acts = {'x': _randn(g, S, N, C), 'f1': torch.tensor([1.25, 0.0, 1.25], dtype=torch.float64), 'f2': torch.tensor([0.0, 1.25, 1.25], dtype=torch.float64)}
    scale = (C // heads) ** -0.5

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        assert ops.transformer_block_supported(A['x'], heads)
        m = _bind(copy.deepcopy(ref).float(), P)
        return ops.transformer_block(A['x'], A['f1'], A['f2'], heads, scale, m['norm1'], m['qkv'], m['proj'], m['norm2'], m['fc1'], m['fc2'])

    def ref_fn(A, P):
        F = torch.nn.functional
        x = A['x']
        h1 = F.layer_norm(x, (C,), P['norm1.weight'], P['norm1.bias'], 1e-6)
        att = _attention64(F.linear(h1, P['qkv.weight'], P['qkv.bias']).reshape(S, N, 3, heads, C // heads), scale)
        x1 = x + F.linear(att, P['proj.weight'], P['proj.bias']) * A['f1'].view(-1, 1, 1)
        h2 = F.layer_norm(x1, (C,), P['norm2.weight'], P['norm2.bias'], 1e-6)
        return x1 + F.linear(gelu64(F.linear(h2, P['fc1.weight'], P['fc1.bias'])), P['fc2.weight'], P['fc2.bias']) * A['f2'].view(-1, 1, 1)
    return Problem(acts, params, dev_fn, ref_fn, lambda kind, name, got, want: _within(got, want, name, 2e-5 if kind == 'out' else 1e-4),
                   views={'x': 'transposed', 'f1': 'strided', 'f2': 'strided'}, data=('f1', 'f2'))


@functools.lru_cache(maxsize=None)
def post_norm_encoder_layer_problem():
    """K20: one post-norm nn.TransformerEncoderLayer without dropout, B, T, d = 3, 2, 4 with two heads and an 8-wide feed-forward,
    against the layer's formula in fp64; 1e-4 (test_simple_transformer_gpu.py). (The predicate accepts d = 2 as well, but a
    LayerNorm over two elements returns +-1 whatever it is given: every gradient behind it cancels to rounding.)"""
    B, T, d, heads, ff = 3, 2, 4, 2, 8
    torch.manual_seed(9)
    ref = torch.nn.TransformerEncoderLayer(d, heads, dim_feedforward=ff, dropout=0.0, batch_first=True).double().train()
    g = _g(9)
    params = {n: p.detach().clone() + _randn(g, *p.shape, scale=0.05) for n, p in ref.named_parameters()}

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        assert ops.post_norm_encoder_layer_supported(B, T, d, heads, True, ff)
        return ops.post_norm_encoder_layer(A['x'], _bind(copy.deepcopy(ref).float(), P), heads, None, 0)

    def ref_fn(A, P):
        F = torch.nn.functional
        x = A['x']
        qkv = F.linear(x, P['self_attn.in_proj_weight'], P['self_attn.in_proj_bias']).view(B, T, 3, heads, d // heads)
        att = _attention64(qkv, (d // heads) ** -0.5)
        x1 = F.layer_norm(x + F.linear(att, P['self_attn.out_proj.weight'], P['self_attn.out_proj.bias']), (d,), P['norm1.weight'],
                          P['norm1.bias'], ref.norm1.eps)
        hh = torch.relu(F.linear(x1, P['linear1.weight'], P['linear1.bias']))
        return F.layer_norm(x1 + F.linear(hh, P['linear2.weight'], P['linear2.bias']), (d,), P['norm2.weight'], P['norm2.bias'], ref.norm2.eps)
    return Problem({'x': _randn(g, B, T, d)}, params, dev_fn, ref_fn, _checker(encoder_close, 1e-4, 1e-4), views={'x': 'transposed'})


# ------------------------------------------------------------------------------------------------------------ pose head
@functools.lru_cache(maxsize=None)
def pose_head_problem():
    """The pose head with a materialised output, B, T = 3, 5: absolute_pose_loc through the construct and loc_2d_3d (0-dim) beside
    it, against the oracle (test_pose_head_gpu.py: 1e-4)."""
    y, st, gt2, gt3, _ = _random_case(3, 5, seed=305)

    def dev_fn(A, P):
        from pedestrians_video_2_carla_amd import ops
        d = A['y'].device
        losses, outs = ops.pose_head(A['y'], ops.PoseHeadSpec(kind='pose_changes_6d'), st.to(d).int(), gt2d=gt2.to(d), gt3d=gt3.to(d),
                                     want=('absolute_pose_loc',))
        return outs['absolute_pose_loc'], losses[2]

    def ref_fn(A, P):
        o = O.pose_head(A['y'], 'pose_changes_6d', st, gt2d=gt2.double(), gt3d=gt3.double())
        return o['absolute_pose_loc'], o['loc_2d_3d']
    return Problem({'y': y.double()}, {}, dev_fn, ref_fn, _checker(pose_close, 1e-4, 1e-4), views={'y': 'transposed'}, scalars=(1,), n_out=2)


# ----------------------------------------------------------------------------------------------------------------------
# the cases
# ----------------------------------------------------------------------------------------------------------------------
OPS = {
    'lstm_k7b': lambda: lstm_problem(16, True), 'lstm_k7b_zero_state': lambda: lstm_problem(16, False),
    'lstm_k18': lambda: lstm_problem(20, True), 'lstm_k18_zero_state': lambda: lstm_problem(20, False),
    'gru': lambda: gru_problem(True), 'gru_zero_state': lambda: gru_problem(False),
    'encoder_stack': encoder_stack_problem, 'decoder_loop': decoder_loop_problem, 'decoder_stack': decoder_stack_problem,
    'joint_embeddings': joint_embeddings_problem, 'relu_stack': relu_stack_problem, 'fused_mlp': fused_mlp_problem,
    'dense': dense_problem, 'mlp_gelu': mlp_gelu_problem, 'dense_chain': dense_chain_problem, 'layer_norm': layer_norm_problem,
    'batch_norm_act': batch_norm_act_problem, 'add_row_parameter': add_row_parameter_problem, 'frame_mean': frame_mean_problem,
    'normalize': normalize_problem, 'loss_loc_2d': loss_loc_2d_problem, 'small_attention': small_attention_problem,
    'transformer_block': transformer_block_problem, 'post_norm_encoder_layer': post_norm_encoder_layer_problem,
    'pose_head': pose_head_problem,
}
SCALAR_ONLY = ('loss_loc_2d',)          # a 0-dim output: contiguous and offset are all the layouts there are
TILED = ('lstm_k7b', 'lstm_k7b_zero_state', 'encoder_stack', 'decoder_loop', 'decoder_stack')      # kernels that read P2C_REC_TILE


def cases():
    out = []
    for name in OPS:
        for layout in LAYOUTS:
            if name in SCALAR_ONLY and layout not in ('contiguous', 'offset'):
                continue
            out.append((name, layout, False))
        out.append((name, 'contiguous', True))
        if name not in SCALAR_ONLY:
            out.append((name, 'transposed', True))
    return out


def _id(v):
    return {True: 'views', False: 'plain'}.get(v, v) if isinstance(v, bool) else str(v)


@pytest.fixture(params=['narrow', 'wide'])
def rec_tile(request, monkeypatch):
    """Both tilings of the time-loop kernels (P2C_REC_TILE, read by the library at each call)."""
    monkeypatch.setenv('P2C_REC_TILE', request.param)
    return request.param


@pytest.mark.parametrize('name,layout,views', [c for c in cases() if c[0] not in TILED], ids=_id)
def test_op_with_the_layouts_a_graph_delivers(name, layout, views, lifetimes):
    check_case(OPS[name](), layout, views, lifetimes)


@pytest.mark.parametrize('name,layout,views', [c for c in cases() if c[0] in TILED], ids=_id)
def test_time_loop_op_with_the_layouts_a_graph_delivers(name, layout, views, rec_tile, lifetimes):
    check_case(OPS[name](), layout, views, lifetimes)


@pytest.mark.parametrize('layout', LAYOUTS)
@pytest.mark.parametrize('name', ['lstm_k7b', 'lstm_k18', 'gru'])
def test_recurrence_with_only_hT_used(name, layout, rec_tile, lifetimes):
    """The classifier's backward: ``out`` (and cT) unused, g_out is None, hT's gradient arrives in every layout."""
    prob = OPS[name]()
    layouts = [None, layout] + [None] * (prob.n_out - 2)
    a = run(prob, layouts, False)
    assert a.rec.keys() == {1}
    fault = layout_fault(layout, a.rec[1], a.outs[1].shape)
    faults = lifetimes.drain() + ([fault] if fault else [])
    ref_outs, ref_grads = reference(prob, a.G)
    for (k, n), want in ref_grads.items():
        try:
            prob.check('grad', f'grad {n}', a.agrad[n] if k == 'a' else a.pgrad[n], want)
        except AssertionError as e:
            faults.append(f'fp64: {e}')
    b = run(prob, layouts, False, feed=a.G)
    faults += lifetimes.drain()
    for n in a.agrad:
        if not torch.equal(a.agrad[n], b.agrad[n]):
            faults.append(f'bits: grad {n}')
    for n in a.pgrad:
        if not torch.equal(a.pgrad[n], b.pgrad[n]):
            faults.append(f'bits: grad {n}')
    assert not faults, '\n'.join(faults)


def test_gemm_row_scale_view(lifetimes):
    """K16 called directly with a stride-2 ``row_scale``: the copy ``gemm`` makes of it lives until the launch, and the result is
    the fp64 product (2e-5, test_gemm_gpu.py) and bit for bit that of the dense factor."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    g = _g(5)
    a, b, s = _randn(g, 36, 12), _randn(g, 20, 12), _randn(g, 12)
    pair = torch.stack([s.float(), torch.full((12,), 7.0)], -1).to(d)
    view = pair[:, 0]
    assert not view.is_contiguous()
    out = ops.gemm(a.float().to(d), b.float().to(d), True, row_scale=view, rows_per_scale=3)
    faults = lifetimes.drain()
    same = ops.gemm(a.float().to(d), b.float().to(d), True, row_scale=s.float().to(d), rows_per_scale=3)
    torch.cuda.synchronize()
    assert not faults, '\n'.join(faults)
    assert rel(out, (a @ b.t()) * s.repeat_interleave(3).view(-1, 1)) < 2e-5
    assert torch.equal(out, same)


def test_contiguous_operands_come_back_as_the_same_object(lifetimes):
    """What stands in place of a timing claim: on the hot path -- dense fp32 device tensors -- ``_require_device`` returns its
    argument, so keeping its result alive adds no copy and no launch. (The fixture asserts it at every call of every case; this
    one counts the calls of a step with contiguous tensors only and sees that nothing was copied.)"""
    prob = OPS['lstm_k18']()
    run(prob, prob.layouts('contiguous'), False)
    assert lifetimes.same_object >= 6 and not lifetimes.pending and not lifetimes.drain()


# ----------------------------------------------------------------------------------------------------------------------
# grad sinks with a mixed group: one parameter of a layer has a prefilled .grad, the other has none
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sink_problem(op):
    """(call, x, weight, bias, upstream gradient, gradient of weight, gradient of bias) on the device; the two gradients come from
    one call outside ``grad_sinks``. layer_norm: 37 rows leave a partly filled workgroup pass and D = 12 leaves five of a row's
    eight lanes without a column; dense: 5 rows, 12 -> 7."""
    from pedestrians_video_2_carla_amd import ops
    d, g = dev(), _g(37)
    if op == 'layer_norm':
        x, w, b, up = _randn(g, 37, 12), 1 + _randn(g, 12, scale=0.1), _randn(g, 12, scale=0.1), _randn(g, 37, 12)
        call = lambda x, w, b: ops.layer_norm(x, w, b, 1e-5)      # noqa: E731
    else:
        x, w, b, up = _randn(g, 5, 12), _randn(g, 7, 12), _randn(g, 7), _randn(g, 5, 7)
        call = ops.dense
    x, w, b, up = (t.float().to(d) for t in (x, w, b, up))
    pw, pb = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    (call(x, pw, pb) * up).sum().backward()
    return call, x, w, b, up, pw.grad.clone(), pb.grad.clone()


@pytest.mark.parametrize('prefilled', ['weight', 'bias', 'both'])
@pytest.mark.parametrize('op', ['layer_norm', 'dense'])
def test_grad_sinks_with_a_mixed_group(op, prefilled):
    """Inside ``grad_sinks`` a layer whose weight has a ``.grad`` and whose bias has none (or the reverse) must leave what
    autograd leaves: prefill + gradient where a ``.grad`` stood, the gradient where none did. Either way the last operation is
    one fp32 add of the same two numbers, so the bits are equal."""
    from pedestrians_video_2_carla_amd import ops
    call, x, w, b, up, gw, gb = _sink_problem(op)
    pw, pb = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    fill_w, fill_b = torch.full_like(w, 0.375) + w, torch.full_like(b, -1.25) + b
    if prefilled in ('weight', 'both'):
        pw.grad = fill_w.clone()
    if prefilled in ('bias', 'both'):
        pb.grad = fill_b.clone()
    with ops.grad_sinks(True):
        (call(x, pw, pb) * up).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(pw.grad, fill_w + gw if prefilled in ('weight', 'both') else gw)
    assert torch.equal(pb.grad, fill_b + gb if prefilled in ('bias', 'both') else gb)
