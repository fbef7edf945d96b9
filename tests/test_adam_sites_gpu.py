"""GPU: the AdamW / Adam update at each of the five kernels that apply it (csrc/p2c_adam_math.h), against the textbook formula
evaluated in fp64, element by element, and against each other bit for bit.

  site 1  adamw_kernel                     p2c_optim.hip   FlatAdamW.step()
  site 2  mlp_reduce_kernel<true>          p2c_mlp.hip     fused MLP backward, fused weight gradient
  site 3  mlp_reduce_small_kernel<true, 8> p2c_mlp.hip     fused MLP backward, split weight gradient
  site 4  train_wgrad_kernel<true>         p2c_train.hip   two-launch train step below wgrad_stream_min_b clips
  site 5  wgrad_reduce_kernel<true>        p2c_train.hip   two-launch train step from wgrad_stream_min_b clips

Every driver starts from a GIVEN state (parameters, both moments, step count, hyper-parameters, mode, zero_grad, grad_scale), runs
one step at its site and hands back what the site saw and left. The gradient G a fused site applied is read from the site itself:
with zero_grad off every site stores the reduced gradient next to the update, which separates the optimizer from the gradient
arithmetic (covered by test_mlp_gpu.py / test_train_fused_gpu.py).

The tolerance (``adam_bound``) is a derivation from the rounding count of an fp32 evaluation, u = 2^-24, not a measurement:
  G     = |g gs| + (0 if decoupled else wd |p|)          the gradient's size before the L2 term can cancel it
  tol_m = 8u (|m| + G)
  tol_v = 8u (v + G^2)
  tol_p = 8u (|p| + |upd|) + step_size tol_m / denom + |upd| (tol_v / (2 sqrt(v') sqrt(bc2))) / denom      (last term 0 at v' = 0)
A numpy-fp32 transcription of the kernel's update stays below 0.38 of each bound over 400 random hyper-parameter sets x 20 000
elements spanning 1e-6 .. 1e3, both modes, steps 1 .. 2^24 - 1 (checked on the CPU). Every element is compared; none is left out.
"""
import contextlib
import functools
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

U = 2.0 ** -24
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-8
# the parameter lists every test below crosses (and test_the_case_tables_cover_every_cell reads)
MODES = [(True, 0.0), (True, 0.05), (False, 0.0), (False, 0.05)]                # (decoupled, weight_decay): AdamW / Adam (L2)
GRAD_SCALES = (1.0, 0.25)
START_STEPS = (0, 1, 9, 999, 99999, 2 ** 24 - 2)
ZERO_GRAD = (False, True)
MODE_IDS = [f'{"adamw" if d else "adam"}-wd{w}' for d, w in MODES]

SITE1_SIZES = (1, 3, 4, 5, 1023, 70001, 2 * 1024 * 1024 + 1027)    # vector body, scalar tail, grid cap (2048 x 256 x 4) with n % 4 = 3
SITE1_CASES = [(n, s) for n in SITE1_SIZES for s in (False, True)]               # (n, with set_scatter)
LINEAR_AE = (52, 26, 13, 6, 39, 78, 156)
# n_in = 16 / 32 / 48: the bias column opens a tile of its own (first and only live column); n_in = 15 / 31: it is a tile's last
# column; a single output row at the end
TILE_EDGES = (16, 32, 15, 48, 31, 1)
# rows on both sides of split_wgrad() (p2c_mlp.hip): split for (192, 384] sample tiles of 16 rows, i.e. 3073 .. 6144 rows
MLP_CASES = [(LINEAR_AE, 3), (LINEAR_AE, 777), (LINEAR_AE, 3072), (LINEAR_AE, 3073), (LINEAR_AE, 4096), (LINEAR_AE, 6144),
             (LINEAR_AE, 6145), (LINEAR_AE, 70000), (TILE_EDGES, 5), (TILE_EDGES, 777), (TILE_EDGES, 3333), (TILE_EDGES, 4096),
             (TILE_EDGES, 70000)]
# (site, clips, first-launch form, output type). form None: the library's own thresholds (B = 8192: streamed weight gradient, its
# reduction adds 256 partials in the eight-deep loop); site 5 at 64 clips adds 8 partials (tail loop only), at 300 clips 32
TRAIN_CASES = [(4, 1, 'latency', 'pose_changes'), (4, 1, 'stream', 'relative_rot'), (4, 256, 'latency', 'pose_changes'),
               (4, 256, 'stream', 'relative_rot'), (4, 1030, 'stream', 'pose_changes'), (4, 1030, 'latency', 'relative_rot'),
               (5, 64, 'latency', 'pose_changes'), (5, 64, 'stream', 'relative_rot'), (5, 300, 'stream', 'pose_changes'),
               (5, 300, 'latency', 'relative_rot'), (5, 8192, None, 'pose_changes'), (5, 8192, None, 'relative_rot')]
WORST = {}           # (site, tensor) -> largest error / bound seen in this process (printed by the last test)


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _f32(x):
    return float(np.float32(x))


def hyper_of(wd, gs, lr=LR):
    return (lr, BETAS[0], BETAS[1], EPS, wd, gs)


# ====================================================================================================== references
def _coefs64(step, hyper):
    lr, b1, b2, eps, wd, gs = (_f32(x) for x in hyper)          # what sits in device memory
    return lr, b1, b2, eps, wd, gs, 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)


def adam_ref64(p, g, m, v, step, hyper, decoupled):
    """torch's _single_tensor_adam in fp64 on the fp32 inputs; ``step`` is the integer AFTER the increment."""
    lr, b1, b2, eps, wd, gs, bc1, bc2 = _coefs64(step, hyper)
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    g = g * gs
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v


def adam_bound(p, g, m, v, step, hyper, decoupled):
    """(tol_p, tol_m, tol_v) per element: see the module docstring."""
    lr, b1, b2, eps, wd, gs, bc1, bc2 = _coefs64(step, hyper)
    _, m1, v1 = adam_ref64(p, g, m, v, step, hyper, decoupled)
    p, g, m, v = (t.detach().double().cpu() for t in (p, g, m, v))
    G = (g * gs).abs() + (0.0 if decoupled else wd * p.abs())
    tol_m = 8 * U * (m.abs() + G)
    tol_v = 8 * U * (v + G * G)
    step_size = lr / bc1
    denom = v1.sqrt() / math.sqrt(bc2) + eps
    upd = (step_size * m1 / denom).abs()
    d_sqrt = torch.where(v1 > 0, tol_v / (2.0 * v1.sqrt().clamp_min(1e-300) * math.sqrt(bc2)), torch.zeros_like(v1))
    tol_p = 8 * U * (p.abs() + upd) + step_size * tol_m / denom + upd * d_sqrt / denom
    return tol_p, tol_m, tol_v


def _ipow(b, n):
    r = 1.0
    while n:
        if n & 1:
            r *= b
        b *= b
        n >>= 1
    return r


def adam_mirror32(p, g, m, v, step, hyper, decoupled):
    """numpy-fp32 transcription of p2c_optim::coefs / update: same operation order, no FMA, coefficients in Python doubles."""
    f = np.float32
    lr, b1, b2, eps, wd, gs = (f(x) for x in hyper)
    bc1, bc2 = 1.0 - _ipow(float(b1), int(step)), 1.0 - _ipow(float(b2), int(step))
    lr_wd, omb1, omb2 = f(lr * wd), f(f(1) - b1), f(f(1) - b2)
    step_size, inv_bc2_sqrt = f(float(lr) / bc1), f(1.0 / math.sqrt(bc2))
    p, g, m, v = (t.detach().cpu().numpy().astype(f) for t in (p, g, m, v))
    with np.errstate(all='ignore'):
        g = g * gs
        if decoupled:
            p = p - lr_wd * p
        else:
            g = g + wd * p
        m = m + omb1 * (g - m)
        v = b2 * v + omb2 * g * g
        denom = np.sqrt(v) * inv_bc2_sqrt + eps
        p = p - step_size * m / denom
    assert p.dtype == m.dtype == v.dtype == f
    return torch.from_numpy(p), torch.from_numpy(m), torch.from_numpy(v)


def check_update(out, state, step, hyper, decoupled, what, site):
    """(a): p', m', v' of ``out`` within adam_bound of adam_ref64 applied to the gradient the site reported, at EVERY element."""
    p0, m0, v0 = state[:3]
    ref = adam_ref64(p0, out['G'], m0, v0, step, hyper, decoupled)
    tol = adam_bound(p0, out['G'], m0, v0, step, hyper, decoupled)
    assert torch.isfinite(out['G']).all(), f'{what}: the site reported a non-finite gradient'
    for name, key, r, t in (('param', 'p', ref[0], tol[0]), ('exp_avg', 'm', ref[1], tol[1]), ('exp_avg_sq', 'v', ref[2], tol[2])):
        a = out[key].double().cpu()
        assert a.shape == r.shape and torch.isfinite(a).all(), f'{what}: {name} not finite'
        err = (a - r).abs()
        live = t > 0
        if live.any():
            k = (site, name)
            WORST[k] = max(WORST.get(k, 0.0), float((err[live] / t[live]).max()))
        bad = err > t                         # t == 0 (no gradient, zero moments, no decay): the result must be exact
        if bad.any():
            i = int(torch.nonzero(bad)[0])
            raise AssertionError(
                f'{what}: {name} outside the bound at {int(bad.sum())} of {bad.numel()} elements; first at {i}: got {float(a[i])!r} '
                f'want {float(r[i])!r} err {float(err[i]):.3e} bound {float(t[i]):.3e} (p {float(p0[i])!r} g {float(out["G"][i])!r} '
                f'm {float(m0[i])!r} v {float(v0[i])!r} step {step} hyper {hyper} decoupled {decoupled})')


@functools.lru_cache(maxsize=32)
def _draws(n, seed, lo, hi):
    g = torch.Generator().manual_seed(seed)

    def draw():
        mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo)
        return (torch.randn(n, generator=g, dtype=torch.float64) * mag).float()
    return draw(), draw(), draw().square()


def make_state(n, step0, seed, decades, zero_at=None):
    """(p, m, v, step0) on the device: magnitudes drawn per element over ``decades`` (log10 range), moments zero at step 0 and
    wherever ``zero_at`` says (parameters that never received a gradient)."""
    p, m, v = (t.clone() for t in _draws(n, seed, decades[0], decades[1]))
    if step0 == 0:
        m.zero_(), v.zero_()
    if zero_at is not None:
        m[zero_at.cpu()] = 0.0
        v[zero_at.cpu()] = 0.0
    return p.to(dev()), m.to(dev()), v.to(dev()), step0


@functools.lru_cache(maxsize=32)
def _grad_draw(n, seed, zero_share):
    g = torch.Generator().manual_seed(seed + 7919)
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 9.0 - 6.0)
    G = (torch.randn(n, generator=g, dtype=torch.float64) * mag).float()
    zero = torch.rand(n, generator=g) < zero_share
    G[zero] = 0.0
    return G, zero


def make_grad(n, seed, zero_share=0.05):
    """A gradient over nine decades with a share of exact zeros (and where they are)."""
    G, zero = _grad_draw(n, seed, zero_share)
    return G.to(dev()), zero


# ====================================================================================================== drivers
class Rig:
    """One site on one shape. ``run`` puts the given state in place, takes one step and returns what the site saw and left."""
    site = 0
    n = 0
    has_image = False

    def _opt_and_flat(self):
        raise NotImplementedError

    def _set(self, state, hyper, decoupled, zero_grad):
        opt, flat = self._opt_and_flat()
        p0, m0, v0, step0 = state
        st = opt.state[flat]
        with torch.no_grad():
            flat.data.copy_(p0)
            st['exp_avg'].copy_(m0), st['exp_avg_sq'].copy_(v0), st['step'].fill_(float(step0))
        assert float(st['step']) == float(step0)                  # representable in the fp32 counter
        grp = opt.param_groups[0]
        grp['lr'], grp['betas'], grp['eps'], grp['weight_decay'] = hyper[0], (hyper[1], hyper[2]), hyper[3], hyper[4]
        opt.grad_scale, opt.decoupled, opt.zero_grad_in_step = hyper[5], bool(decoupled), bool(zero_grad)

    def _read(self, G=None):
        opt, flat = self._opt_and_flat()
        torch.cuda.synchronize()
        st = opt.state[flat]
        out = {'p': flat.detach().clone(), 'm': st['exp_avg'].clone(), 'v': st['exp_avg_sq'].clone(), 'step': float(st['step']),
               'ticket': int(opt._ticket), 'grad_after': flat.grad.clone()}
        out['G'] = G.clone() if G is not None else out['grad_after']       # zero_grad off: the site left the gradient it applied
        return out


class OptimRig(Rig):
    """Site 1: FlatAdamW.step() on a chosen gradient."""
    site = 1

    def __init__(self, n, scatter=False):
        from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
        self.n = n
        self.flat = torch.nn.Parameter(torch.zeros(n, device=dev()))
        self.flat.grad = torch.zeros_like(self.flat)
        self.opt = FlatAdamW([self.flat], lr=LR, betas=BETAS, eps=EPS)
        self.scatter = None
        if scatter:
            g = torch.Generator().manual_seed(n)
            index = torch.randperm(n + 7, generator=g)[:n].to(torch.int32)
            index[torch.rand(n, generator=g) < 0.25] = -1
            if n > 1:
                index[n // 2] = -1
            self.scatter = (index.to(dev()), torch.empty(n + 7, device=dev()))
            self.opt.set_scatter(*self.scatter)

    def _opt_and_flat(self):
        return self.opt, self.flat

    def run(self, state, hyper, decoupled, zero_grad, G):
        self._set(state, hyper, decoupled, zero_grad)
        self.flat.grad.copy_(G)
        if self.scatter is not None:
            self.scatter[1].fill_(7.5)
        self.opt.step()
        out = self._read(G)
        if self.scatter is not None:
            out['scatter_dst'] = self.scatter[1].clone()
        return out

    def step_again(self):
        G = self.flat.grad.clone()
        self.opt.step()
        return self._read(G)

    def check_scatter(self, out, what):
        """The scattered copy equals the new parameter bitwise; destinations no index names stay as they were."""
        if self.scatter is None:
            return
        index, dst = self.scatter[0].long(), out['scatter_dst']
        live = index >= 0
        want = torch.full_like(dst, 7.5)
        want[index[live]] = out['p'][live]
        assert torch.equal(dst, want), f'{what}: scattered copy'


def mlp_site(rows, mode=None):
    """Mirror of split_wgrad() (p2c_mlp.hip): which reduction applies the optimizer at this row count (``mode``: the forced
    form, by default what P2C_MLP_WGRAD says)."""
    mode = (os.environ.get('P2C_MLP_WGRAD', '') if mode is None else mode)[:1]
    n_stiles = (rows + 15) // 16
    cus = int(os.environ.get('P2C_MLP_MAX_BLOCKS', '256'))
    split = mode == 's' or (mode != 'f' and 4 * n_stiles > 3 * cus and 2 * n_stiles <= 3 * cus)
    return 3 if split else 2


class MlpRig(Rig):
    """Sites 2 / 3: ops.fused_mlp(..., fused_optimizer=opt), built as test_mlp_gpu.py builds it."""
    has_image = True

    def __init__(self, dims, rows):
        from pedestrians_video_2_carla_amd import ops
        from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
        d = dev()
        self.dims, self.rows, self.site = list(dims), rows, mlp_site(rows)
        self.n = sum(o * (i + 1) for i, o in zip(dims[:-1], dims[1:]))
        g = torch.Generator().manual_seed(rows)
        self.x = torch.randn(rows, dims[0], generator=g).to(d)
        self.gy = torch.randn(rows, dims[-1], generator=g).to(d)
        self.flat = torch.nn.Parameter(torch.zeros(self.n, device=d))
        self.flat.grad = torch.zeros_like(self.flat)
        self.ws, self.bs, self.sinks, off = [], [], [], 0
        for i, o in zip(dims[:-1], dims[1:]):
            self.ws.append(self.flat.data[off:off + o * i].view(o, i).requires_grad_(True))
            self.sinks.append(self.flat.grad[off:off + o * i].view(o, i))
            off += o * i
            self.bs.append(self.flat.data[off:off + o].requires_grad_(True))
            self.sinks.append(self.flat.grad[off:off + o])
            off += o
        self.opt = FlatAdamW([self.flat], lr=LR, betas=BETAS, eps=EPS)
        n_image, index = ops.mlp_image_layout(self.dims)
        self.image = torch.zeros(n_image, device=d)
        self.opt.set_scatter(index.to(d), self.image)                 # flat order == (W_0, b_0, W_1, ...) here

    def _opt_and_flat(self):
        return self.opt, self.flat

    def _step(self):
        from pedestrians_video_2_carla_amd import ops
        before = self.opt.fused_steps_applied
        ops.fused_mlp(self.x, self.ws, self.bs, self.sinks, image=self.image, image_is_current=True,
                      fused_optimizer=self.opt).backward(self.gy)
        assert self.opt.fused_steps_applied == before + 1
        out = self._read()
        out['image'] = self.image.clone()
        out['fresh'] = torch.zeros_like(self.image)
        ops.mlp_pack(self.ws, self.bs, out['fresh'])
        torch.cuda.synchronize()
        return out

    def run(self, state, hyper, decoupled, zero_grad, G=None):
        from pedestrians_video_2_carla_amd import ops
        self._set(state, hyper, decoupled, zero_grad)
        ops.mlp_pack(self.ws, self.bs, self.image)
        self.flat.grad.fill_(123.0)               # every entry is WRITTEN by the reduction (the gradient, or zero)
        return self._step()

    def step_again(self):
        return self._step()


@contextlib.contextmanager
def train_thresholds(site, form):
    """Which kernels the two-launch step takes: first launch 'latency' / 'stream', streamed weight gradient (site 5) or not; ``form``
    None leaves the library's own thresholds. They are restored."""
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    if form is None:
        yield lib.p2c_train_step_set_wgrad_stream_min_batch(-1)
        return
    prev = lib.p2c_train_step_set_stream_min_batch(1 if form == 'stream' else (1 << 30))
    prev_w = lib.p2c_train_step_set_wgrad_stream_min_batch(1 if site == 5 else (1 << 30))
    try:
        yield 1 if site == 5 else (1 << 30)
    finally:
        lib.p2c_train_step_set_stream_min_batch(prev)
        lib.p2c_train_step_set_wgrad_stream_min_batch(prev_w)


class TrainRig(Rig):
    """Sites 4 / 5: the two-launch step through the flow and the trainer, the optimizer inside."""
    has_image = True

    def __init__(self, site, B, form, otype, use_graph=False):
        from test_flow_gpu import make
        from pedestrians_video_2_carla_amd.trainer import Trainer
        self.site, self.B, self.form = site, B, form
        self.flow, dm = make(B=B, otype=otype)
        self.trainer = Trainer(device=dev(), use_graph=use_graph).setup(self.flow, dm)
        assert self.trainer._opt_in_backward
        self.batch = dm.generate_batch(dev())
        self.opt = self.trainer.optimizers[0]
        self.flat = self.trainer.flat.flat_param
        self.n = self.flat.numel()
        self.model = self.flow.movements_model
        self.calls = 0

    def _opt_and_flat(self):
        return self.opt, self.flat

    def _set(self, state, hyper, decoupled, zero_grad):
        super()._set(state, hyper, decoupled, zero_grad)
        for m in self.trainer._packed:            # the parameters were rewritten behind the optimizer's back
            m.repack()

    def _step(self):
        from pedestrians_video_2_carla_amd import ops
        before = self.opt.fused_steps_applied
        with train_thresholds(self.site, self.form) as min_b:
            assert (5 if self.B >= min_b else 4) == self.site       # mirror of the dispatch in p2c_train_step_launch
            self.trainer.train_step(self.flow, self.batch, self.calls)
            torch.cuda.synchronize()
        self.calls += 1
        assert self.flow._pair_counts is not None, 'the batch did not take the two-launch step'
        if not self.trainer.use_graph:
            assert self.opt.fused_steps_applied == before + 1, 'the optimizer did not ride on the backward'
        out = self._read()
        out['image'] = self.model._image.clone()
        layers = self.model._linears()
        out['fresh'] = torch.zeros_like(self.model._image)
        ops.mlp_pack([m.weight for m in layers], [m.bias for m in layers], out['fresh'])
        torch.cuda.synchronize()
        return out

    def run(self, state, hyper, decoupled, zero_grad, G=None):
        self._set(state, hyper, decoupled, zero_grad)
        self.flat.grad.fill_(0.0 if not zero_grad else 123.0)     # zero_grad on: the trainer clears nothing, the step writes every entry
        return self._step()

    def step_again(self):
        return self._step()


_RIGS = {}


def rig_for(kind, *key):
    """Rigs are built once per shape and reused by every mode (a trainer over 8192 clips is the expensive part, not its steps)."""
    k = (kind,) + key
    if k not in _RIGS:
        _RIGS[k] = {'optim': OptimRig, 'mlp': MlpRig, 'train': TrainRig}[kind](*key)
    return _RIGS[k]


# ====================================================================================================== the shared assertions
def exercise(rig, decoupled, wd, what):
    """(a) - (e, one step) for one mode at one rig, over GRAD_SCALES x START_STEPS x ZERO_GRAD."""
    fused = rig.site != 1
    twin = rig_for('optim', rig.n, False) if fused else None
    decades = (-4, 0) if fused else (-6, 3)
    for gs, step0 in itertools.product(GRAD_SCALES, START_STEPS):
        tag = f'{what} decoupled={decoupled} wd={wd} gs={gs} step0={step0}'
        hyper = hyper_of(wd, gs)
        seed = (rig.n * 31 + step0 * 7 + int(gs * 100)) % (2 ** 31)
        if fused:
            # the gradient is a function of parameters and batch alone: one look at it (moments zero) says which parameters get
            # none; half of those start with zero moments, as a parameter that never received a gradient does
            p0 = make_state(rig.n, step0, seed, decades)[0]
            zeros = torch.zeros_like(p0)
            probe = rig.run((p0, zeros, zeros, step0), hyper, decoupled, False)['G']
            none = (probe == 0) & (torch.rand(rig.n, generator=torch.Generator().manual_seed(seed)) < 0.5).to(dev())
            state = make_state(rig.n, step0, seed, decades, zero_at=none)
            G = None
        else:
            G, none = make_grad(rig.n, seed)
            state = make_state(rig.n, step0, seed, decades, zero_at=none)
        kept = rig.run(state, hyper, decoupled, False, G)
        check_update(kept, state, step0 + 1, hyper, decoupled, tag, rig.site)                                        # (a)
        assert kept['step'] == float(step0 + 1) and kept['ticket'] == 0, (tag, kept['step'], kept['ticket'])         # (e)
        if fused:
            assert torch.equal(kept['G'], probe), f'{tag}: the gradient depends on the moments?'
            one = twin.run(state, hyper, decoupled, False, kept['G'])                                                # (b)
            for k in ('p', 'm', 'v'):
                assert torch.equal(kept[k], one[k]), \
                    f'{tag}: {k} differs from site 1 at {int((kept[k] != one[k]).sum())} elements, first {int(torch.nonzero(kept[k] != one[k])[0])}'
        else:
            assert torch.equal(kept['grad_after'], G), f'{tag}: zero_grad off must leave the gradient'
            rig.check_scatter(kept, tag)
        cleared = rig.run(state, hyper, decoupled, True, kept['G'])                                                  # (c)
        for k in ('p', 'm', 'v') + (('image',) if rig.has_image else ()):
            assert torch.equal(kept[k], cleared[k]), f'{tag}: {k} differs between zero_grad off and on'
        assert cleared['step'] == float(step0 + 1) and cleared['ticket'] == 0, tag
        assert int(torch.count_nonzero(cleared['grad_after'])) == 0, f'{tag}: zero_grad on left a gradient behind'
        if not fused:
            rig.check_scatter(cleared, tag)
        if rig.has_image:                                                                                            # (d)
            # pack writes the whole image (padding zero, one unit entry per layer), so live image == fresh pack everywhere
            for o in (kept, cleared):
                assert torch.equal(o['image'], o['fresh']), \
                    f'{tag}: weight image differs from a fresh pack at {int((o["image"] != o["fresh"]).sum())} entries'


def three_steps(rig, what):
    """(e): three consecutive steps without anybody touching the state in between (the ticket re-arms itself), each within the
    bound of the reference applied to the state read back before it."""
    decoupled, wd, gs, step0 = True, 0.05, 1.0, 9
    hyper = hyper_of(wd, gs)
    state = make_state(rig.n, step0, 4242, (-4, 0) if rig.site != 1 else (-6, 3))
    G = make_grad(rig.n, 4242)[0] if rig.site == 1 else None
    out = rig.run(state, hyper, decoupled, False, G)
    for k in range(3):
        check_update(out, state, step0 + 1 + k, hyper, decoupled, f'{what} step {k + 1} of 3', rig.site)
        assert out['step'] == float(step0 + 1 + k) and out['ticket'] == 0, (what, k, out['step'], out['ticket'])
        if rig.has_image:
            assert torch.equal(out['image'], out['fresh']), f'{what} step {k + 1}: weight image'
        state = (out['p'], out['m'], out['v'], step0 + 1 + k)
        if k < 2:
            out = rig.step_again()


# ====================================================================================================== site 1
@pytest.mark.parametrize('decoupled,wd', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('n,scatter', SITE1_CASES)
def test_site_1_update(n, scatter, decoupled, wd):
    exercise(rig_for('optim', n, scatter), decoupled, wd, f'site 1 n={n} scatter={scatter}')


@pytest.mark.parametrize('n', [5, 70001])
def test_site_1_three_steps(n):
    three_steps(rig_for('optim', n, True), f'site 1 n={n}')


@pytest.mark.parametrize('decoupled,wd', MODES, ids=MODE_IDS)
def test_site_1_equals_the_fp32_host_mirror(decoupled, wd):
    """With contraction off and no fast-math flag the kernel evaluates exactly what a numpy-fp32 transcription of update() does:
    correctly rounded sqrt and divide, denormals kept. Bit for bit, at every start step and grad scale (measured on an MI355X
    before this was made an assertion: no element of 70 001 differs in any of the 48 combinations)."""
    n = 70001
    rig = rig_for('optim', n, False)
    for gs, step0 in itertools.product(GRAD_SCALES, START_STEPS):
        hyper = hyper_of(wd, gs)
        G, none = make_grad(n, step0)
        state = make_state(n, step0, step0 + 1, (-6, 3), zero_at=none)
        out = rig.run(state, hyper, decoupled, False, G)
        want = adam_mirror32(state[0], G, state[1], state[2], step0 + 1, hyper, decoupled)
        for k, w in zip(('p', 'm', 'v'), want):
            got = out[k].cpu()
            diff = got != w
            if diff.any():
                i = int(torch.nonzero(diff)[0])
                ulps = (got.view(torch.int32).long() - w.view(torch.int32).long()).abs()
                raise AssertionError(f'{k} (decoupled={decoupled} wd={wd} gs={gs} step0={step0}): {int(diff.sum())} of {n} elements '
                                     f'differ, up to {int(ulps.max())} ulp; first at {i}: kernel {float(got[i])!r} mirror {float(w[i])!r}')


def test_site_1_counter_stops_at_2_to_24():
    """The step counter is an fp32 number: 16 777 216 + 1 == 16 777 216, so from 2^24 on it no longer counts and the bias
    corrections stay those of step 2^24. torch's own fp32 step tensor does exactly the same; this pins the behaviour, it does not
    endorse it. From 2^24 - 1, two steps stay finite and within the bound of the reference at n = 2^24; the counter reads 2^24."""
    n, top = 1023, 2 ** 24
    rig = rig_for('optim', n, False)
    hyper = hyper_of(0.05, 1.0)
    G = make_grad(n, 5)[0]
    state = make_state(n, top - 1, 5, (-6, 3))
    out = rig.run(state, hyper, True, False, G)
    for k in range(2):
        check_update(out, state, top, hyper, True, f'step {k + 1} from 2^24 - 1', 1)
        assert out['step'] == float(top) and out['ticket'] == 0
        state = (out['p'], out['m'], out['v'], top)
        if k == 0:
            out = rig.step_again()
    ref = torch.zeros((), dtype=torch.float32) + float(top)
    assert float(ref + 1) == float(top)                       # the same saturation in torch's arithmetic


def test_site_1_graph_replays_follow_a_learning_rate_change():
    """(e): three replays of a captured step, the learning rate changed between the first and the second: every replay within the
    bound of the fp64 reference evaluated with the learning rate in force, the counter and the ticket right after each."""
    n, step0 = 4099, 9
    rig = rig_for('optim', n, True)
    G = make_grad(n, 77)[0]
    state = make_state(n, step0, 77, (-6, 3))
    rig._set(state, hyper_of(0.05, 0.25), True, False)
    rig.flat.grad.copy_(G)
    rig.opt.sync_hyper()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rig.opt.step()
    torch.cuda.current_stream().wait_stream(side)
    for k in range(3):
        lr = LR if k == 0 else LR * 0.1
        rig.opt.param_groups[0]['lr'] = lr
        rig.opt.sync_hyper()
        graph.replay()
        out = rig._read(G)
        check_update(out, state, step0 + 1 + k, hyper_of(0.05, 0.25, lr), True, f'replay {k + 1}', 1)
        assert out['step'] == float(step0 + 1 + k) and out['ticket'] == 0
        state = (out['p'], out['m'], out['v'], step0 + 1 + k)


# ====================================================================================================== sites 2 / 3
MLP_IDS = [f'{"ae" if dims == LINEAR_AE else "edges"}-{rows}' for dims, rows in MLP_CASES]


@pytest.mark.parametrize('decoupled,wd', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('dims,rows', MLP_CASES, ids=MLP_IDS)
def test_mlp_sites_update(dims, rows, decoupled, wd):
    rig = rig_for('mlp', dims, rows)
    exercise(rig, decoupled, wd, f'site {rig.site} dims={"-".join(map(str, dims))} rows={rows}')


@pytest.mark.parametrize('dims,rows', MLP_CASES, ids=MLP_IDS)
def test_mlp_sites_three_steps(dims, rows):
    rig = rig_for('mlp', dims, rows)
    three_steps(rig, f'site {rig.site} dims={"-".join(map(str, dims))} rows={rows}')


@pytest.mark.parametrize('form', ['split', 'fused'])
def test_every_mlp_site_case_also_passes_with_the_weight_gradient_form_forced(form):
    """P2C_MLP_WGRAD (read once per process, so a child pytest) sends EVERY row count through site 3 (split) or site 2 (fused): the
    one-tile batches and the ragged ones through the small reduction, 4096 rows through the wide one."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, P2C_MLP_WGRAD=form)
    res = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-p', 'no:cacheprovider',
                          '-k', 'test_mlp_sites'], env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]


# ====================================================================================================== sites 4 / 5
TRAIN_IDS = [f'site{s}-B{B}-{form or "default"}-{otype}' for s, B, form, otype in TRAIN_CASES]


@pytest.mark.parametrize('decoupled,wd', MODES, ids=MODE_IDS)
@pytest.mark.parametrize('site,B,form,otype', TRAIN_CASES, ids=TRAIN_IDS)
def test_train_sites_update(site, B, form, otype, decoupled, wd):
    exercise(rig_for('train', site, B, form, otype), decoupled, wd, f'site {site} B={B} {form} {otype}')


@pytest.mark.parametrize('site,B,form,otype', TRAIN_CASES, ids=TRAIN_IDS)
def test_train_sites_three_steps(site, B, form, otype):
    three_steps(rig_for('train', site, B, form, otype), f'site {site} B={B} {form} {otype}')


@pytest.mark.parametrize('site,B,form,otype', [(4, 256, 'latency', 'pose_changes'), (5, 300, 'stream', 'relative_rot')])
def test_train_sites_graph_replays_follow_a_learning_rate_change(site, B, form, otype):
    """(e) for the captured two-launch step: three replays from a given state, the learning rate changed between the first and the
    second. With zero_grad off every replay leaves the gradient it applied: each replay is held against the fp64 reference with the
    learning rate in force. With zero_grad on (the trainer's default; the capture is then replayed as its one recorded call) the
    same three replays must give the same bits and leave the gradient buffer zero."""
    step0, wd, gs = 9, 0.05, 1.0
    runs = {}
    for zero_grad in ZERO_GRAD:
        rig = TrainRig(site, B, form, otype, use_graph=True)
        rig.opt.decoupled, rig.opt.zero_grad_in_step = True, zero_grad     # part of the captured launch: set before the capture
        with train_thresholds(site, form):
            rig.trainer.train_step(rig.flow, rig.batch, 0)            # captures (warm-up steps, state restored) and replays once
        assert rig.trainer.use_graph, 'the captured step failed its replay check'
        state = make_state(rig.n, step0, 99, (-4, 0))
        rig._set(state, hyper_of(wd, gs), True, zero_grad)
        outs = []
        for k in range(3):
            lr = LR if k == 0 else LR * 0.1
            rig.opt.param_groups[0]['lr'] = lr
            if zero_grad and k == 0:
                rig.flat.grad.fill_(123.0)            # the step writes every entry of the gradient buffer
            outs.append(rig.step_again())
            assert outs[-1]['step'] == float(step0 + 1 + k) and outs[-1]['ticket'] == 0, (zero_grad, k, outs[-1]['step'])
            assert torch.equal(outs[-1]['image'], outs[-1]['fresh']), f'replay {k + 1}: weight image'
        runs[zero_grad] = outs
    prev = make_state(rig.n, step0, 99, (-4, 0))
    for k, (kept, cleared) in enumerate(zip(runs[False], runs[True])):
        lr = LR if k == 0 else LR * 0.1
        check_update(kept, prev, step0 + 1 + k, hyper_of(wd, gs, lr), True, f'site {site} replay {k + 1}', site)
        for key in ('p', 'm', 'v', 'image'):
            assert torch.equal(kept[key], cleared[key]), f'replay {k + 1}: {key} differs between zero_grad off and on'
        assert int(torch.count_nonzero(cleared['grad_after'])) == 0
        prev = (kept['p'], kept['m'], kept['v'], step0 + 1 + k)


# ====================================================================================================== load_state_dict
def _loaded_sources(flat0, grads):
    """Three optimizer states after two steps on ``grads`` whose tensors do not sit where the kernel needs them."""
    import io
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    kw = dict(lr=LR, betas=BETAS, eps=EPS, weight_decay=0.05)
    ours = torch.nn.Parameter(flat0.clone())
    o = FlatAdamW([ours], zero_grad_in_step=False, **kw)
    theirs = torch.nn.Parameter(flat0.clone())
    t = torch.optim.AdamW([theirs], **kw)
    for g in grads:
        ours.grad = g.clone()
        theirs.grad = g.clone()
        o.step(), t.step()
    torch.cuda.synchronize()
    sd = o.state_dict()
    to_cpu = {'state': {k: {n: (v.cpu() if isinstance(v, torch.Tensor) else v) for n, v in s.items()} for k, s in sd['state'].items()},
              'param_groups': sd['param_groups']}
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return {'own state moved to the host': (to_cpu, ours.detach().clone()),
            'torch.optim.AdamW': (t.state_dict(), theirs.detach().clone()),
            'torch.load map_location=cpu': (torch.load(buf, map_location='cpu'), ours.detach().clone())}


@pytest.mark.parametrize('source', ['own state moved to the host', 'torch.optim.AdamW', 'torch.load map_location=cpu'])
def test_load_state_dict_brings_the_state_to_the_device(source):
    """Whatever the loaded dict held (host tensor, int64, Python number), the kernel's three state tensors must sit on the
    parameter's device, the step counter as a 0-dim fp32 tensor. Decided on the HOST -- device, dtype and the addresses in the launch
    descriptor -- before any launch; only then one step, compared with the reference continuing from the loaded step."""
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    d, n = dev(), 1023
    g = torch.Generator().manual_seed(11)
    flat0 = torch.randn(n, generator=g).to(d)
    grads = [torch.randn(n, generator=g).to(d) for _ in range(3)]
    sd, params = _loaded_sources(flat0, grads[:2])[source]
    step_in = sd['state'][0]['step']
    assert not (isinstance(step_in, torch.Tensor) and step_in.is_cuda), 'the case is about a counter that does not sit on the device'
    for as_int in (False, True):
        if as_int:                                    # the same dict with an integer counter (int64 tensor / Python number)
            sd = {'state': {0: dict(sd['state'][0])}, 'param_groups': sd['param_groups']}
            sd['state'][0]['step'] = torch.tensor(2) if source != 'torch.optim.AdamW' else 2.0
        p = torch.nn.Parameter(params.clone())
        p.grad = grads[2].clone()
        o = FlatAdamW([p], zero_grad_in_step=False)
        o.load_state_dict(sd)
        st = o.state[p]
        assert set(st) >= {'step', 'exp_avg', 'exp_avg_sq'}
        assert st['step'].device == p.device and st['step'].dtype == torch.float32 and st['step'].ndim == 0
        for k in ('exp_avg', 'exp_avg_sq'):
            assert st[k].device == p.device and st[k].dtype == torch.float32 and st[k].shape == p.shape and st[k].is_contiguous()
        desc = o._descriptor(p)
        assert desc.step == st['step'].data_ptr() and desc.exp_avg == st['exp_avg'].data_ptr() \
            and desc.exp_avg_sq == st['exp_avg_sq'].data_ptr() and desc.param == p.data_ptr()
        assert st['step'].is_cuda and st['step'].get_device() == p.get_device()
        assert float(st['step']) == 2.0
        state = (p.detach().clone(), st['exp_avg'].clone(), st['exp_avg_sq'].clone(), 2)
        # ---- only now a launch ----
        o.step()
        torch.cuda.synchronize()
        out = {'p': p.detach().clone(), 'm': st['exp_avg'].clone(), 'v': st['exp_avg_sq'].clone(), 'G': grads[2]}
        g0 = o.param_groups[0]
        hyper = (g0['lr'], g0['betas'][0], g0['betas'][1], g0['eps'], g0['weight_decay'], 1.0)
        assert hyper[:5] == (LR, BETAS[0], BETAS[1], EPS, 0.05)
        check_update(out, state, 3, hyper, True, f'{source} (integer counter: {as_int})', 1)
        assert float(o.state[p]['step']) == 3.0 and int(o._ticket) == 0


# ====================================================================================================== coverage
def test_the_case_tables_cover_every_cell():
    """{site 1 .. 5} x {AdamW, Adam} x {zero_grad off, on} x {grad_scale 1, 0.25}: every cell has a case, read from the very lists
    the tests above are parametrised with (exercise() crosses MODES x GRAD_SCALES x ZERO_GRAD at every rig)."""
    site_of = lambda rows: mlp_site(rows, mode='')          # noqa: E731 -- the library's own rule, whatever this process forces
    sites = {1: len(SITE1_CASES)}
    for dims, rows in MLP_CASES:
        s = site_of(rows)
        sites[s] = sites.get(s, 0) + 1
    for s, B, form, otype in TRAIN_CASES:
        sites[s] = sites.get(s, 0) + 1
    cells = {(s, d, z, gs) for s in sites for d, _wd in MODES for z in ZERO_GRAD for gs in GRAD_SCALES}
    assert cells == {(s, d, z, gs) for s in (1, 2, 3, 4, 5) for d in (True, False) for z in (False, True) for gs in (1.0, 0.25)}
    assert {wd for _d, wd in MODES} == {0.0, 0.05} and set(START_STEPS) == {0, 1, 9, 999, 99999, 2 ** 24 - 2}
    # the shapes the sites are known to go wrong at
    assert {site_of(rows) for dims, rows in MLP_CASES if dims == TILE_EDGES} == {2, 3}
    assert {site_of(rows) for dims, rows in MLP_CASES if dims == LINEAR_AE} == {2, 3}
    assert [site_of(r) for r in (3072, 3073, 6144, 6145)] == [2, 3, 3, 2]
    n_ins = TILE_EDGES[:-1]
    assert any(i % 16 == 0 for i in n_ins) and any(i % 16 == 15 for i in n_ins) and TILE_EDGES[-1] == 1
    assert {B for s, B, _f, _o in TRAIN_CASES if s == 4} == {1, 256, 1030} and {B for s, B, _f, _o in TRAIN_CASES if s == 5} == {64, 300, 8192}
    for s in (4, 5):
        assert {o for t, _B, _f, o in TRAIN_CASES if t == s} == {'pose_changes', 'relative_rot'}
        assert {f for t, B, f, _o in TRAIN_CASES if t == s and B < 8192} == {'latency', 'stream'}
    assert any(n > 2048 * 256 * 4 and n % 4 for n in SITE1_SIZES) and {1, 3, 4, 5, 1023} <= set(SITE1_SIZES)
    print('largest error / bound per (site, tensor) in this process:', {k: round(v, 3) for k, v in sorted(WORST.items())})
