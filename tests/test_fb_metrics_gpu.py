"""GPU: K22 (csrc/p2c_eval_fb.hip), the five FB_* metrics in one launch, through the FB_* classes and through the raw C ABI.

Truth = the tensor functions of metrics/extra_metrics.py (mpjpe, weighted_mpjpe, n_mpjpe, mean_velocity_error, p_mpjpe) on the
CPU, on ``.double()`` copies of the same fp32 inputs, scaled as ``_FBMetric`` scales them (millimetres). Bound for every
comparison: |got - want| <= 1e-5 |want| + 32 * 2^-24 * S, with 1e-5 the project's bound for device metrics (tests/test_metrics.py)
and S the mean distance of the target joints from the origin in millimetres (fp32 input rounding through a few dozen operations;
it decides only where ``want`` is near zero or the skeleton is far from the origin)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
KEY = 'absolute_pose_loc'
NAMES = ('FB_MPJPE', 'FB_WeightedMPJPE', 'FB_N_MPJPE', 'FB_MPJVE', 'FB_PA_MPJPE')         # slot k = bit k of `which`
E_SHAPE = -2

SHAPES = [(1, 2, 26), (2, 1, 26), (3, 5, 26), (130, 5, 26), (2, 3, 17), (2, 3, 32), (2, 3, 33), (2, 3, 64)]
KINDS = ['randn', 'similarity', 'mirrored', 'planar', 'equal', 'offset', 'zero frame']
CASES = [(s, 'randn') for s in SHAPES] + [(s, k) for s in ((3, 5, 26), (2, 3, 33)) for k in KINDS[1:]]


def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def inputs(shape, kind, seed=0):
    """(pred, gt) fp32 on the CPU."""
    B, T, J = shape
    gen = torch.Generator().manual_seed(1000 * seed + 100 * B + 10 * T + J + 7 * KINDS.index(kind))
    gt = torch.randn(B, T, J, 3, generator=gen)
    noise = torch.randn(B, T, J, 3, generator=gen)
    if kind == 'randn':
        pred = noise
    elif kind == 'similarity':               # as tests/test_metrics.py: Procrustes alignment must remove all but the noise
        c, s = math.cos(0.7), math.sin(0.7)
        R = torch.tensor([[c, -s, 0.], [s, c, 0.], [0., 0., 1.]])
        pred = 1.7 * (gt @ R) + torch.tensor([0.3, -0.2, 0.5]) + 0.01 * noise
    elif kind == 'mirrored':                 # the best orthogonal map is a reflection: the det < 0 branch of p_mpjpe
        pred = gt * torch.tensor([-1., 1., 1.]) + 0.01 * noise
    elif kind == 'planar':                   # rank-2 cross-covariance
        pred = gt + 0.1 * noise
        pred[..., 2], gt[..., 2] = 0.0, 0.0
    elif kind == 'equal':
        pred = gt.clone()
    elif kind == 'offset':                   # a 0.5 m skeleton 60 m from the origin: cancellation in the centring
        gt = 0.5 * (torch.rand(B, T, J, 3, generator=gen) - 0.5) + torch.tensor([50., -30., 20.])
        pred = gt + 0.01 * noise
    elif kind == 'zero frame':               # 0/0 in N-MPJPE and in the normalisation of PA-MPJPE
        pred = noise
        pred[0, T // 2] = 0.0
    return pred.contiguous(), gt.contiguous()


def truth_sums(pred, gt, w=None):
    """What one ``_FBMetric.update`` adds: (N * metric_k for the five metrics, N), in fp64 on the CPU."""
    from pedestrians_video_2_carla_amd.metrics import extra_metrics as E
    p, g = pred.double().cpu(), gt.double().cpu()
    J = p.shape[-2]
    fp, fg = p.reshape(-1, J, 3), g.reshape(-1, J, 3)
    N = fp.shape[0]
    ww = torch.ones(1, 1, J, dtype=torch.float64) if w is None else w.double().cpu().reshape(1, 1, J)
    try:
        pa = E.p_mpjpe(fp, fg)
    except torch.linalg.LinAlgError:         # the host's LAPACK refuses the NaN matrix of a 0/0 frame: no finite value either way
        pa = torch.tensor(float('nan'), dtype=torch.float64)
    vals = [E.mpjpe(fp, fg), E.weighted_mpjpe(p, g, ww.repeat(*p.shape[:2], 1)), E.n_mpjpe(p, g),
            E.mean_velocity_error(fp, fg), pa]
    return [N * float(v) for v in vals], N


@functools.lru_cache(maxsize=None)
def truth(shape, kind):
    pred, gt = inputs(shape, kind)
    sums, N = truth_sums(pred, gt)
    return [1000.0 * s / N for s in sums], 1000.0 * float(gt.double().norm(dim=-1).mean())


def within(got, want, S, what):
    if math.isnan(want):
        print(f'{what}: got {got} want nan')
        assert math.isnan(got), what
        return
    err, bound = abs(got - want), 1e-5 * abs(want) + 32 * 2.0 ** -24 * S
    print(f'{what}: got {got:.9g} want {want:.9g} err {err:.3e} bound {bound:.3e}')
    assert err <= bound, f'{what}: |{got} - {want}| = {err:.3e} > {bound:.3e}'


def five(metric_set=None, w=None):
    from pedestrians_video_2_carla_amd.metrics import FB_MPJPE, FB_MPJVE, FB_N_MPJPE, FB_PA_MPJPE, FB_WeightedMPJPE
    kw = {} if metric_set is None else {'metric_set': metric_set}
    return {'FB_MPJPE': FB_MPJPE(**kw), 'FB_WeightedMPJPE': FB_WeightedMPJPE(w, **kw), 'FB_N_MPJPE': FB_N_MPJPE(**kw),
            'FB_MPJVE': FB_MPJVE(**kw), 'FB_PA_MPJPE': FB_PA_MPJPE(**kw)}


def abi(pred, gt, w=None, which=31, state=None, N=None, J=None):
    """p2c_eval_fb on device tensors: (rc, state, partials)."""
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    N = pred.shape[0] * pred.shape[1] if N is None else N
    J = pred.shape[2] if J is None else J
    part = torch.empty(max(1, lib.p2c_eval_fb_workspace_floats(N)), dtype=torch.float32, device=pred.device)
    if state is None:
        state = torch.zeros(10, dtype=torch.float64, device=pred.device)
    rc = lib.p2c_eval_fb(pred.data_ptr(), gt.data_ptr(), None if w is None else w.data_ptr(), N, J, which, part.data_ptr(),
                         state.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, state, part


@pytest.mark.parametrize('shape,kind', CASES, ids=[f'{s[0]}x{s[1]}x{s[2]}-{k}' for s, k in CASES])
def test_kernel_matches_the_fp64_tensor_functions(shape, kind):
    from pedestrians_video_2_carla_amd.metrics import FBMetricSet
    d = dev()
    pred, gt = (t.to(d) for t in inputs(shape, kind))
    want, S = truth(shape, kind)
    N = shape[0] * shape[1]
    # the classes, sharing one launch
    fb = FBMetricSet()
    ms = five(fb)
    for m in ms.values():
        m.update({KEY: pred}, {KEY: gt})
    assert fb.launches == 1
    got = {name: float(ms[name].compute()) for name in NAMES}
    for k, name in enumerate(NAMES):
        within(got[name], want[k], S, f'{name} (class) {shape} {kind}')
        assert float(ms[name]._state[1]) == N
    # the raw C ABI
    rc, state, _ = abi(pred, gt)
    assert rc == 0
    st = state.cpu()
    for k, name in enumerate(NAMES):
        within(1000.0 * float(st[2 * k]) / float(st[2 * k + 1]), want[k], S, f'{name} (ABI) {shape} {kind}')
        assert float(st[2 * k + 1]) == N
    assert torch.equal(st, fb._state.cpu()) or kind == 'zero frame'        # one kernel, one reduction order
    assert torch.equal(st[2:4], st[0:2]) and (float(st[0]) > 0 or kind == 'equal')   # unit weights: FB_MPJPE bit for bit
    if kind == 'similarity':
        assert got['FB_PA_MPJPE'] < 0.05 * got['FB_MPJPE']                # the similarity transform is gone
    if kind == 'zero frame':
        assert math.isnan(want[2]) and math.isnan(want[4]) and math.isnan(got['FB_N_MPJPE']) and math.isnan(got['FB_PA_MPJPE'])
        assert math.isfinite(want[0]) and math.isfinite(got['FB_MPJPE']) and math.isfinite(got['FB_MPJVE'])


@pytest.mark.parametrize('shape', [(3, 5, 26), (2, 3, 33)], ids=str)
def test_weights_per_joint(shape):
    from pedestrians_video_2_carla_amd.metrics import FB_WeightedMPJPE
    d = dev()
    pred, gt = (t.to(d) for t in inputs(shape, 'randn'))
    J = shape[2]
    w = torch.rand(1, 1, J, generator=torch.Generator().manual_seed(J)) + 0.5
    sums, N = truth_sums(pred, gt, w)
    want, S = 1000.0 * sums[1] / N, truth(shape, 'randn')[1]
    m = FB_WeightedMPJPE(w)
    m.update({KEY: pred}, {KEY: gt})
    assert m._set.launches == 1
    within(float(m.compute()), want, S, f'weighted (class) {shape}')
    rc, state, _ = abi(pred, gt, w=w.reshape(J).to(d).contiguous(), which=2)
    assert rc == 0
    within(1000.0 * float(state[2]) / float(state[3]), want, S, f'weighted (ABI) {shape}')
    ones = torch.ones(J, device=d)                                         # unit weights given as a tensor: still bit for bit
    rc, state, _ = abi(pred, gt, w=ones, which=3)
    assert rc == 0 and torch.equal(state[2:4], state[0:2]) and float(state[0]) > 0


def test_accumulation_over_batches_reset_and_fixed_order():
    from pedestrians_video_2_carla_amd.metrics import FBMetricSet
    d = dev()
    batches = [inputs((2, 5, 26), 'similarity'), inputs((3, 5, 26), 'randn')]
    sums, frames = [0.0] * 5, 0
    for pred, gt in batches:
        s, n = truth_sums(pred, gt)
        sums, frames = [a + b for a, b in zip(sums, s)], frames + n
    S = 1000.0 * float(torch.cat([gt.reshape(-1, 3) for _, gt in batches]).double().norm(dim=-1).mean())
    states = []
    for _ in range(2):
        fb = FBMetricSet()
        ms = five(fb)
        for pred, gt in batches:
            pred, gt = pred.to(d), gt.to(d)
            for m in ms.values():
                m.update({KEY: pred}, {KEY: gt})
        assert fb.launches == 2
        states.append(fb._state.clone())
    assert torch.equal(states[0], states[1])                               # the reduction order is fixed
    for k, name in enumerate(NAMES):
        within(float(ms[name].compute()), 1000.0 * sums[k] / frames, S, f'{name} over two batches')
        assert float(ms[name]._state[1]) == frames
    for m in ms.values():
        m.reset()
    assert float(fb._state.abs().sum()) == 0.0


def test_one_launch_serves_the_set_round_robin():
    from pedestrians_video_2_carla_amd.metrics import FB_PA_MPJPE, FBMetricSet
    d = dev()
    batches = [tuple(t.to(d) for t in inputs((3, 5, 26), 'mirrored')), tuple(t.to(d) for t in inputs((2, 3, 26), 'randn'))]
    fb = FBMetricSet()
    shared, alone = five(fb), five()
    for pred, gt in batches:
        for group in (shared, alone):
            for m in group.values():
                m.update({KEY: pred}, {KEY: gt})
    assert fb.launches == 2
    for name in NAMES:
        assert alone[name]._set.launches == 2
        assert float(shared[name].compute()) == float(alone[name].compute()), name
        assert torch.equal(shared[name]._state, alone[name]._state)
    pa = FB_PA_MPJPE()
    pa.update({KEY: batches[0][0]}, {KEY: batches[0][1]})
    st = pa._set._state.cpu()
    assert float(st[:8].abs().sum()) == 0.0 and float(st[8]) > 0 and float(st[9]) == 15.0
    # a member that comes round before the others took their turn starts the next launch
    fb2 = FBMetricSet()
    ms = five(fb2)
    pred, gt = batches[0]
    ms['FB_MPJPE'].update({KEY: pred}, {KEY: gt})
    ms['FB_MPJPE'].update({KEY: pred}, {KEY: gt})
    assert fb2.launches == 2 and float(fb2._state[9]) == 30.0


def test_refusals_come_before_any_launch():
    from pedestrians_video_2_carla_amd import _lib
    d, lib = dev(), _lib.lib()
    pred = torch.randn(1, 2, 65, 3, device=d)
    gt = torch.randn(1, 2, 65, 3, device=d)
    for kw in (dict(J=65), dict(N=1, J=26, which=8), dict(N=1, J=26, which=31), dict(J=0), dict(J=26, which=0),
               dict(J=26, which=32)):
        part = torch.full((4096,), 7.0, dtype=torch.float32, device=d)
        state = torch.zeros(10, dtype=torch.float64, device=d)
        rc = lib.p2c_eval_fb(pred.data_ptr(), gt.data_ptr(), None, kw.get('N', 2), kw['J'], kw.get('which', 31), part.data_ptr(),
                             state.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == E_SHAPE, (kw, rc)
        assert float(state.abs().sum()) == 0.0 and bool((part == 7.0).all()), kw
    rc, state, _ = abi(pred, gt, N=1, J=26, which=31 - 8)                  # a single frame is fine without the velocity
    assert rc == 0 and float(state[1]) == 1.0 and float(state[7]) == 0.0
    rc, state, _ = abi(pred, gt, N=0, J=26)
    assert rc == 0 and float(state.abs().sum()) == 0.0


def make_flow(B=6, T=16):
    """As tests/test_flow_gpu.py builds it: LinearAE in the pose-lifting flow on the synthetic CARLA data module."""
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(22742)
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.0)
    model = LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=MT['pose_changes'])
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], lean_train_outputs=False,
                              transform=dm.transform.name)
    return flow, dm


@pytest.mark.parametrize('framework', [False, True], ids=['kernel', 'P2C_FB_FRAMEWORK=1'])
def test_trainer_validate_feeds_the_flow_metrics(framework, monkeypatch):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    if framework:
        monkeypatch.setenv('P2C_FB_FRAMEWORK', '1')
    else:
        monkeypatch.delenv('P2C_FB_FRAMEWORK', raising=False)
    d = dev()
    flow, dm = make_flow()
    flow.attach_datamodule(dm)
    flow.to(d).train()
    batches = [dm.generate_batch(d), dm.generate_batch(d)]
    outs, step = [], flow.validation_step

    def recording_step(batch, i):
        out = step(batch, i)
        outs.append((out['preds'][KEY].detach().clone(), out['targets'][KEY].detach().clone()))
        return out
    monkeypatch.setattr(flow, 'validation_step', recording_step)
    vals = Trainer().validate(flow, batches)
    assert flow.training                                                   # back in the mode it came in
    assert len(outs) == 2 and set(vals) >= set(NAMES) | {'MPJPE'}
    fb = flow.metrics['FB_MPJPE']._set
    assert fb.launches == (0 if framework else 2)
    sums, frames = [0.0] * 5, 0
    for pred, gt in outs:
        s, n = truth_sums(pred, gt)
        sums, frames = [a + b for a, b in zip(sums, s)], frames + n
    S = 1000.0 * float(torch.cat([gt.reshape(-1, 3) for _, gt in outs]).double().norm(dim=-1).mean())
    for k, name in enumerate(NAMES):
        within(vals[name], 1000.0 * sums[k] / frames, S, f'{name} through Trainer.validate')
    assert flow.compute_metrics(sync=False) == {}                          # reset
    flow.eval()
    Trainer().validate(flow, batches[:1])
    assert not flow.training
