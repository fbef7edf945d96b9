"""K29 on the GPU: gradient clipping inside the optimizer launch (csrc/p2c_grad_clip.hip, FlatAdamW.set_clip,
Trainer(gradient_clip_val=...)).

  1. the norm the kernels report against fp64, to 1 fp32 ulp, and the same bits on a second call;
  2. the clipped step BIT FOR BIT against the unclipped kernel (p2c_adamw_step, untouched by K29) fed with the gradient clipped
     by tensor ops -- norm and value mode, clipping and not clipping, zeroed gradient and scatter destination included;
  3. 25 steps against torch.nn.utils.clip_grad_* + torch.optim.AdamW / Adam, TOL of tests/test_optim_gpu.py; NaN pattern;
  4. the clipped step captured in a graph and replayed across an LR change;
  5. the Trainer: eager, captured, and in the two-stage graph of a data-parallel run (child process, one-rank RCCL group).
Sizes: 1, 3 scalar tail only; 7 float4 body + tail; 1021 one partial workgroup; 4099 a few workgroups; 70001 many, ragged end;
2 200 003 past the 2048 x 256 float4 cap of the step grid and the 1024-workgroup cap of the norm grid (grid-stride in both)."""
import ctypes
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 5e-6                       # tests/test_optim_gpu.py
SIZES = [1, 3, 7, 1021, 4099, 70001, 2200003]
OK = 'P2C_CLIP_CASE_OK'
HYPER = (3e-3, 0.9, 0.99, 1e-8, 0.05)         # lr, beta1, beta2, eps, weight_decay


def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


class State:
    """Everything one optimizer launch reads and writes, for the C ABI called directly."""

    def __init__(self, n, seed=0):
        d = dev()
        g = torch.Generator(device=d).manual_seed(1000 + n + seed)
        self.n = n
        self.param = torch.randn(n, device=d, generator=g)
        self.grad = torch.randn(n, device=d, generator=g) * 3
        self.exp_avg = torch.randn(n, device=d, generator=g) * 0.1
        self.exp_avg_sq = torch.rand(n, device=d, generator=g) * 0.01
        self.step = torch.full((), 3.0, device=d)
        self.ticket = torch.zeros(1, dtype=torch.int32, device=d)
        idx = torch.full((n,), -1, dtype=torch.int32, device=d)
        picked = torch.arange(0, n, 3, device=d)
        idx[picked] = torch.arange(len(picked), dtype=torch.int32, device=d).flip(0)
        self.scatter_idx, self.scatter_dst = idx, torch.full((len(picked),), -7.0, device=d)

    def clone(self):
        other = object.__new__(State)
        other.n = self.n
        for k, v in self.__dict__.items():
            if isinstance(v, torch.Tensor):
                setattr(other, k, v.clone())
        return other

    def launch(self, grad_scale, decoupled, zero_grad, clip=None):
        """clip = None: p2c_adamw_step; (mode, bound): p2c_adamw_step_clipped. Returns the device total norm (norm mode)."""
        from pedestrians_video_2_carla_amd import _lib
        lib = _lib.lib()
        hyper = torch.tensor(HYPER + (grad_scale,), dtype=torch.float32, device=self.param.device)
        d = _lib.AdamWDesc()
        d.n = self.n
        for f in ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'step', 'ticket', 'scatter_idx', 'scatter_dst'):
            setattr(d, f, getattr(self, f).data_ptr())
        d.hyper, d.adamw, d.zero_grad = hyper.data_ptr(), int(decoupled), int(zero_grad)
        stream = torch.cuda.current_stream().cuda_stream
        total = None
        if clip is None:
            _lib.check(lib.p2c_adamw_step(ctypes.byref(d), stream), 'p2c_adamw_step')
        else:
            c = _lib.ClipDesc()
            c.mode, c.bound = {'norm': _lib.P2C_CLIP_NORM, 'value': _lib.P2C_CLIP_VALUE}[clip[0]], clip[1]
            if clip[0] == 'norm':
                # (torch.empty: under P2C_POISON_EMPTY the workspace starts as NaN -- every slot read must have been written)
                partials = torch.empty(lib.p2c_grad_clip_partials(self.n), dtype=torch.float64, device=self.param.device)
                total = torch.full((), -1.0, device=self.param.device)
                c.partials, c.total_norm = partials.data_ptr(), total.data_ptr()
            _lib.check(lib.p2c_adamw_step_clipped(ctypes.byref(d), ctypes.byref(c), stream), 'p2c_adamw_step_clipped')
        torch.cuda.synchronize()
        return total

    def same_bits(self, other, what):
        for k in ('param', 'exp_avg', 'exp_avg_sq', 'step', 'grad', 'scatter_dst', 'ticket'):
            a, b = getattr(self, k), getattr(other, k)
            assert torch.equal(a, b), f'{what}: {k} differs, max |diff| {float((a - b).abs().max()):.3e}'


_STATES = {}


def state(n):
    """One seeded state per size, shared by the tests and never written: every launch runs on a clone."""
    if n not in _STATES:
        _STATES[n] = State(n)
    return _STATES[n]


def f32(x):
    return float(np.float32(x))


# ---- 1: the norm -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad_scale', [1.0, 0.25])
@pytest.mark.parametrize('n', SIZES)
def test_norm_is_the_fp64_norm_to_one_ulp_and_reproducible(n, grad_scale):
    s0 = state(n)
    want = float(grad_scale * s0.grad.double().pow(2).sum().sqrt())
    runs = []
    for _ in range(2):
        s = s0.clone()
        total = s.launch(grad_scale, True, True, clip=('norm', 1.0))
        runs.append((total.clone(), s))
    got = float(runs[0][0])
    ulp = float(np.spacing(np.float32(want)))
    print(f'n={n} grad_scale={grad_scale}: total_norm {got!r}, fp64 {want!r}, diff {abs(got - want):.3e}, ulp {ulp:.3e}')
    assert abs(got - want) <= ulp
    assert torch.equal(runs[0][0], runs[1][0])
    runs[0][1].same_bits(runs[1][1], 'second call on the same data')


# ---- 2: bit for bit against the unclipped kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize('grad_scale', [1.0, 0.25])
@pytest.mark.parametrize('n', SIZES)
def test_clipped_step_is_the_unclipped_kernel_on_the_clipped_gradient(n, grad_scale):
    s0 = state(n)
    d = s0.param.device
    norm64 = float(grad_scale * s0.grad.double().pow(2).sum().sqrt())
    top = float((s0.grad * grad_scale).abs().max())
    for decoupled in (True, False):
        for zero_grad in (True, False):
            tag = f'n={n} gs={grad_scale} decoupled={decoupled} zero_grad={zero_grad}'
            # norm mode: a bound at half the norm clips, one at twice the norm does not
            for bound, clips in ((f32(0.5 * norm64), True), (f32(2.0 * norm64), False)):
                ours = s0.clone()
                total = ours.launch(grad_scale, decoupled, zero_grad, clip=('norm', bound))
                assert (float(total) > bound) == clips, (tag, float(total), bound)
                coef = torch.tensor(bound, dtype=torch.float32, device=d) / (total + 1e-6)
                coef = torch.clamp(coef, max=1.0)
                assert (float(coef) < 1.0) == clips
                ref = s0.clone()
                ref.grad = (s0.grad * grad_scale) * coef
                ref.launch(1.0, decoupled, zero_grad)
                if not zero_grad:
                    assert torch.equal(ours.grad, s0.grad)       # the clipped call does not write the gradient back
                    ref.grad = s0.grad.clone()
                ours.same_bits(ref, f'{tag} norm bound={bound}')
            # value mode: half the largest |g * grad_scale| clips at least that element, twice it clips nothing
            for bound, clips in ((f32(0.5 * top), True), (f32(2.0 * top), False)):
                ours = s0.clone()
                assert ours.launch(grad_scale, decoupled, zero_grad, clip=('value', bound)) is None
                g2 = torch.clamp(s0.grad * grad_scale, -bound, bound)
                assert bool((g2 != s0.grad * grad_scale).any()) == clips, tag
                ref = s0.clone()
                ref.grad = g2
                ref.launch(1.0, decoupled, zero_grad)
                if not zero_grad:
                    assert torch.equal(ours.grad, s0.grad)
                    ref.grad = s0.grad.clone()
                ours.same_bits(ref, f'{tag} value bound={bound}')
            # a bound that never clips: the unclipped step on the ORIGINAL gradient and grad_scale
            plain = s0.clone()
            plain.launch(grad_scale, decoupled, zero_grad)
            for mode in ('norm', 'value'):
                ours = s0.clone()
                ours.launch(grad_scale, decoupled, zero_grad, clip=(mode, 1e30))
                ours.same_bits(plain, f'{tag} {mode} bound=1e30')
            assert float(plain.step) == 4.0 and int(plain.ticket) == 0
            assert not torch.equal(plain.param, s0.param)


# ---- 3: against torch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('algorithm', ['norm', 'value'])
@pytest.mark.parametrize('decoupled', [True, False])
@pytest.mark.parametrize('n', [7, 4099, 70001])
def test_25_steps_match_torch_clip_and_adamw(n, decoupled, algorithm):
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    d = dev()
    g = torch.Generator(device=d).manual_seed(n)
    p0 = torch.randn(n, device=d, generator=g)
    ours, ref = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    kw = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    o = FlatAdamW([ours], decoupled=decoupled, zero_grad_in_step=True, **kw)
    o.set_clip(0.5, algorithm)
    r = (torch.optim.AdamW if decoupled else torch.optim.Adam)([ref], **kw)
    ours.grad = torch.zeros_like(ours)
    clipped = 0
    for step in range(25):
        grad = torch.randn(n, device=d, generator=g) * (1.0 + step)
        ours.grad.add_(grad)
        ref.grad = grad.clone()
        o.step()
        if algorithm == 'norm':
            norm = torch.nn.utils.clip_grad_norm_([ref], 0.5)
            clipped += int(float(norm) > 0.5)
            assert abs(float(o.last_grad_norm) - float(norm)) <= 2e-6 * float(norm)
        else:
            clipped += int(float(grad.abs().max()) > 0.5)
            torch.nn.utils.clip_grad_value_([ref], 0.5)
            assert o.last_grad_norm is None
        r.step()
        assert float(ours.grad.abs().max()) == 0.0
    assert clipped >= 20                                   # (randn * (1 + step): nearly every step is over the bound)
    st, rt = o.state[ours], r.state[ref]
    errs = (rel(ours.data, ref.data), rel(st['exp_avg'], rt['exp_avg']), rel(st['exp_avg_sq'], rt['exp_avg_sq']))
    print(f'n={n} decoupled={decoupled} {algorithm}: rel err param / exp_avg / exp_avg_sq {errs}')
    assert float(st['step']) == 25.0 == float(rt['step'])
    assert max(errs) < TOL


@pytest.mark.parametrize('algorithm', ['norm', 'value'])
def test_nan_gradient_element_spreads_as_in_torch(algorithm):
    """A NaN norm stays NaN through the clamp (every parameter becomes NaN, as after clip_grad_norm_); clamping by value keeps
    the one NaN where it is."""
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    d = dev()
    n = 4099
    g = torch.Generator(device=d).manual_seed(9)
    p0 = torch.randn(n, device=d, generator=g)
    grad = torch.randn(n, device=d, generator=g) * 3
    grad[1234] = float('nan')
    ours, ref = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    o = FlatAdamW([ours], lr=1e-2, zero_grad_in_step=False)
    o.set_clip(0.5, algorithm)
    r = torch.optim.AdamW([ref], lr=1e-2)
    ours.grad, ref.grad = grad.clone(), grad.clone()
    o.step()
    (torch.nn.utils.clip_grad_norm_ if algorithm == 'norm' else torch.nn.utils.clip_grad_value_)([ref], 0.5)
    r.step()
    want = torch.isnan(ref.data)
    assert int(want.sum()) == (n if algorithm == 'norm' else 1)
    assert torch.equal(torch.isnan(ours.data), want)
    if algorithm == 'norm':
        assert bool(torch.isnan(o.last_grad_norm))
    else:
        assert rel(ours.data[~want], ref.data[~want]) < TOL


def test_fused_descriptor_is_refused_and_clip_can_be_switched_off():
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    d = dev()
    p = torch.nn.Parameter(torch.randn(64, device=d))
    p.grad = torch.randn(64, device=d)
    o = FlatAdamW([p])
    with pytest.raises(ValueError):
        o.set_clip(1.0, 'l1')
    o.set_clip(1.0)
    assert o.last_grad_norm is not None and o.last_grad_norm.is_cuda
    with pytest.raises(RuntimeError, match='clip'):
        o.descriptor_for_fusion()
    o.set_clip(None)
    assert o.last_grad_norm is None
    o.descriptor_for_fusion()
    o.set_clip(0)
    o.descriptor_for_fusion()


# ---- 4: graph ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('algorithm', ['norm', 'value'])
def test_clipped_step_in_a_graph_follows_lr_changes(algorithm):
    """The shape of test_grad_scale_lr_change_and_graph_replay (tests/test_optim_gpu.py) with a clip: both K29 launches are
    captured; the gradient is averaged (grad_scale = 1/4) BEFORE it is clipped, as torch clips the averaged gradient."""
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    d = dev()
    g = torch.Generator(device=d).manual_seed(3)
    n = 4099
    p0 = torch.randn(n, device=d, generator=g)
    ours, ref = torch.nn.Parameter(p0.clone()), torch.nn.Parameter(p0.clone())
    o = FlatAdamW([ours], lr=1e-2, weight_decay=0.01, zero_grad_in_step=False)
    o.grad_scale = 0.25
    o.set_clip(0.5, algorithm)
    r = torch.optim.AdamW([ref], lr=1e-2, weight_decay=0.01)
    grads = [torch.randn(n, device=d, generator=g) for _ in range(6)]
    ours.grad = torch.zeros_like(ours)
    static = ours.grad
    o.sync_hyper()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            o.step()
    torch.cuda.current_stream().wait_stream(side)
    for i, gr in enumerate(grads):
        if i == 3:
            o.param_groups[0]['lr'] = r.param_groups[0]['lr'] = 2e-3
            o.sync_hyper()
        static.copy_(gr * 4.0)
        graph.replay()
        ref.grad = gr.clone()
        if algorithm == 'norm':
            norm = torch.nn.utils.clip_grad_norm_([ref], 0.5)
            assert float(norm) > 0.5 and abs(float(o.last_grad_norm) - float(norm)) <= 2e-6 * float(norm)
        else:
            torch.nn.utils.clip_grad_value_([ref], 0.5)
        r.step()
    torch.cuda.synchronize()
    assert float(o.state[ours]['step']) == 6.0
    err = rel(ours.data, ref.data)
    print(f'graph {algorithm}: rel err {err:.3e}')
    assert err < TOL


# ---- 5: trainer ----------------------------------------------------------------------------------------------------------------
def _make():
    """The smallest LinearAE pose-lifting configuration of tests/test_train_fused_gpu.py: one clip of one frame, no missing
    joints, no transform (its (1, 1, 0.0, 'none', 'pose_changes') case)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_flow_gpu import make
    from pedestrians_video_2_carla_amd.data.base.base_transforms import BaseTransforms
    return make(B=1, T=1, missing=0.0, transform=BaseTransforms['none'], otype='pose_changes')


def _first_unclipped_gradient(monkeypatch):
    """(2-norm, largest magnitude) of the first step's gradient, from a second, unclipped trainer whose optimizer is kept out of
    the backward so that the gradient survives it; and the batch every trainer of the test then steps on."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    monkeypatch.setenv('P2C_FUSED_UPDATE', '0')
    flow, dm = _make()
    t = Trainer(device=dev()).setup(flow, dm)
    t.optimizers[0].zero_grad_in_step = False
    batch = dm.generate_batch(dev())
    t._forward_backward(flow, batch, 0)
    monkeypatch.delenv('P2C_FUSED_UPDATE')
    return float(t.flat.flat_grad.double().norm()), float(t.flat.flat_grad.abs().max()), batch


def _run_trainer(c, batch, steps=3, **kw):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    flow, dm = _make()
    t = Trainer(device=dev(), gradient_clip_val=c, **kw).setup(flow, dm)
    norms = []
    for i in range(steps):
        t.train_step(flow, batch, i)
        norms.append(float(t.last_grad_norm))
    torch.cuda.synchronize()
    return t, norms


def test_trainer_clips_in_the_optimizer_launch_eager_and_captured(monkeypatch):
    """Trainer(gradient_clip_val=c), c = half the first step's unclipped norm, 3 steps on one batch: every step clips; the
    parameters are within TOL of the P2C_FUSED_UPDATE=0 trainer with clip_grad_norm_ on the flat parameter between backward and
    optimizer; the captured trainer gives the eager one's bits. Measured on an MI355X at this configuration: 9.1e-9 against
    torch's clip, 0 between captured and eager. (The distance to torch's clip is torch's own fp32 norm, an ulp off the fp64
    one from step 2 on, amplified by the model: at make(B=8) it grows to 1.1e-4 after step 3 while the kernel path stays
    bit-identical to a tensor-op clip with an fp64-derived norm -- DESIGN section 4, K29.)"""
    from pedestrians_video_2_carla_amd.parallel.optim import FlatAdamW
    from pedestrians_video_2_carla_amd.trainer import Trainer
    first, _, batch = _first_unclipped_gradient(monkeypatch)
    c = 0.5 * first
    monkeypatch.setenv('P2C_FUSED_UPDATE', '0')
    # reference: the route P2C_FUSED_UPDATE=0 takes, with torch's clip on the flat parameter between backward and optimizer
    flow_r, dm = _make()
    tr = Trainer(device=dev()).setup(flow_r, dm)
    assert isinstance(tr.optimizers[0], FlatAdamW) and not tr._opt_in_backward
    ref_norms = []
    for i in range(3):
        tr._forward_backward(flow_r, batch, i)
        ref_norms.append(float(torch.nn.utils.clip_grad_norm_([tr.flat.flat_param], c)))
        tr._optimizer_step()
    monkeypatch.delenv('P2C_FUSED_UPDATE')                 # the clip itself must keep the optimizer out of the backward
    te, norms = _run_trainer(c, batch)
    print(f'first unclipped norm {first!r}, c {c!r}, norms {norms} (torch: {ref_norms})')
    assert te._clip_in_kernel and not te._opt_in_backward and te._direct is None
    assert te.last_grad_norm is te.optimizers[0].last_grad_norm and te.last_grad_norm.is_cuda
    assert abs(norms[0] - first) <= 2e-6 * first
    assert all(x > c for x in norms), (norms, c)
    err = rel(te.flat.flat_param.data, tr.flat.flat_param.data)
    print(f'eager clipped trainer vs torch clip: rel err {err:.3e}')
    assert err < TOL
    assert float(te.optimizers[0].state[te.flat.flat_param]['step']) == 3.0
    # captured: the same launches in the same order -> the same bits
    tg, gnorms = _run_trainer(c, batch, use_graph=True)
    assert tg.use_graph and tg._graphs is not None, 'the captured step was kept'
    assert tg._clip_in_kernel and not tg._opt_in_backward and tg._direct is None and tg._graphs[1] is None
    assert all(x > c for x in gnorms), (gnorms, c)
    diff = float((tg.flat.flat_param.data - te.flat.flat_param.data).abs().max())
    print(f'captured vs eager clipped trainer: max |diff| {diff:.3e}')
    assert torch.equal(tg.flat.flat_param.data, te.flat.flat_param.data)
    assert gnorms == norms


def test_trainer_value_clip_and_framework_switch(monkeypatch):
    """'value' through the trainer, and P2C_CLIP_FRAMEWORK=1 (the tensor path on the device) against the kernel path."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    first, top, batch = _first_unclipped_gradient(monkeypatch)
    c = 0.5 * first
    tk, norms = _run_trainer(c, batch)
    monkeypatch.setenv('P2C_CLIP_FRAMEWORK', '1')
    tf, fnorms = _run_trainer(c, batch)
    monkeypatch.delenv('P2C_CLIP_FRAMEWORK')
    assert not tf._clip_in_kernel and not tf._opt_in_backward and tk._clip_in_kernel
    assert all(abs(a - b) <= 2e-6 * b for a, b in zip(norms, fnorms)), (norms, fnorms)
    assert rel(tk.flat.flat_param.data, tf.flat.flat_param.data) < TOL
    assert top > 0.0                                       # half the largest element: the first step clips at least that one
    results = []
    for framework in ('0', '1'):
        monkeypatch.setenv('P2C_CLIP_FRAMEWORK', framework)
        flow, dm = _make()
        t = Trainer(device=dev(), gradient_clip_val=0.5 * top, gradient_clip_algorithm='value').setup(flow, dm)
        for i in range(3):
            t.train_step(flow, batch, i)
        assert t.last_grad_norm is None and not t._opt_in_backward
        results.append(t.flat.flat_param.data.clone())
    assert rel(results[0], results[1]) < TOL


def test_clipped_optimizer_in_the_two_stage_graph():
    """One-rank RCCL group with the exchange forced on and the collective kept out of the graph (P2C_GRAPH_ALLREDUCE=0): stage B
    is a captured graph holding both K29 launches. Child process, as in tests/test_ddp_gpu.py."""
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT='29541', P2C_FORCE_EXCHANGE='1', P2C_GRAPH_ALLREDUCE='0',
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, 'tests')]
                                          + [p for p in os.environ.get('PYTHONPATH', '').split(os.pathsep) if p]))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), 'two_stage'], env=env, cwd=ROOT, capture_output=True,
                         text=True, timeout=300)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and OK in res.stdout, f'rc={res.returncode}\n{res.stdout[-4000:]}\n{res.stderr[-4000:]}'


def _case_two_stage():
    import torch.distributed as dist
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = torch.device('cuda:0')
    torch.cuda.set_device(d)
    os.environ['P2C_FUSED_UPDATE'] = '0'                    # an unclipped trainer that keeps its gradient: half its norm is the clip
    flow_u, dm = _make()
    tu = Trainer(device=d).setup(flow_u, dm)
    tu.optimizers[0].zero_grad_in_step = False
    batch = dm.generate_batch(d)
    tu._forward_backward(flow_u, batch, 0)
    c = 0.5 * float(tu.flat.flat_grad.double().norm())
    os.environ.pop('P2C_FUSED_UPDATE')

    def run(trainer, flow):
        norms = []
        for i in range(3):
            trainer.train_step(flow, batch, i)
            norms.append(float(trainer.last_grad_norm))
        return norms
    flow_a, _ = _make()
    ta = Trainer(device=d, use_graph=True, gradient_clip_val=c).setup(flow_a, dm)
    single = run(ta, flow_a)
    dist.init_process_group(backend='nccl', rank=0, world_size=1)
    flow_b, _ = _make()
    tb = Trainer(device=d, use_graph=True, gradient_clip_val=c).setup(flow_b, dm)
    assert tb.exchange.enabled and not tb.exchange.average_here and tb._clip_in_kernel and not tb._opt_in_backward
    multi = run(tb, flow_b)
    assert isinstance(tb._graphs[1], torch.cuda.CUDAGraph), 'stage B (clip + optimizer) is a captured graph'
    print('norms', single, multi, 'c', c)
    dist.barrier()
    assert all(x > c for x in multi), (multi, c)
    pa, pb = ta.flat.flat_param.data, tb.flat.flat_param.data
    err = float((pa - pb).abs().max() / pb.abs().max())
    print(f'two-stage vs single graph: rel err {err:.3e}')
    assert err < TOL
    assert float(tb.optimizers[0].state[tb.flat.flat_param]['step']) == 3.0


if __name__ == '__main__':
    code = 1
    try:
        {'two_stage': _case_two_stage}[sys.argv[1]]()
        torch.cuda.synchronize()
        print(OK, flush=True)
        code = 0
    except BaseException:                                   # noqa: BLE001 -- the verdict has to reach the parent
        traceback.print_exc()
    sys.stdout.flush()
    sys.stderr.flush()
    os._exit(code)                                          # (no interpreter / RCCL teardown: see tests/test_ddp_gpu.py)
