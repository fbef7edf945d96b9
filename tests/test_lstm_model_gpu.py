"""GPU: the LSTM movements model and K18, the recurrence for any hidden size (csrc/p2c_lstm_step.hip, p2c_lstm_steps_*).

(a) ops.lstm_layer for widths outside K7b against fp64 torch.nn.LSTM on the CPU: out, hT, cT and every gradient within 1e-4;
(b) the reference fixtures model_lstm_*.npz on the device; (c) one training step of each flow against its fp64 CPU twin;
(d) graph replay; (e) no framework RNN up to H = 1024; (f) H = 1025 falls back with a warning; (g) the K7b widths keep K7b."""
import copy
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def close(a, b, what, rtol=RTOL):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err == err and err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


# every H in {1, 20, 65, 100, 191, 256, 512, 1024}, every T in {1, 4, 15}, every B in {1, 33, 256, 1030} at least once
CASES = [(1, 1, 5, 1), (4, 33, 52, 20), (15, 256, 52, 65), (4, 1030, 32, 100), (15, 33, 52, 191), (4, 256, 52, 256),
         (1, 256, 64, 512), (15, 33, 100, 512), (4, 3, 16, 1024), (15, 1, 8, 1024)]


@pytest.mark.parametrize('T,B,I,H', CASES)
@pytest.mark.parametrize('with_state', [False, True])
def test_layer_any_width_matches_torch_lstm(T, B, I, H, with_state):
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    torch.manual_seed(T * 1000 + B + H)
    ref = torch.nn.LSTM(I, H).double()
    x = torch.randn(T, B, I, dtype=torch.float64)
    h0, c0 = torch.randn(B, H, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64)
    up, uh, uc = torch.randn(T, B, H, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64)
    xr, hr, cr = x.clone().requires_grad_(True), h0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
    out_r, (hT_r, cT_r) = ref(xr, (hr[None], cr[None])) if with_state else ref(xr)
    ((out_r * up).sum() + (hT_r[0] * uh).sum() + (cT_r[0] * uc).sum()).backward()

    p = {n: v.detach().float().to(d).requires_grad_(True) for n, v in ref.named_parameters()}
    xd, hd, cd = (t.float().to(d).requires_grad_(True) for t in (x, h0, c0))
    out, hT, cT = ops.lstm_layer(xd, hd if with_state else None, cd if with_state else None, p['weight_ih_l0'], p['weight_hh_l0'],
                                 p['bias_ih_l0'], p['bias_hh_l0'])
    ((out * up.float().to(d)).sum() + (hT * uh.float().to(d)).sum() + (cT * uc.float().to(d)).sum()).backward()
    close(out, out_r, 'out'), close(hT, hT_r[0], 'hT'), close(cT, cT_r[0], 'cT')
    close(xd.grad, xr.grad, 'grad x')
    if with_state:
        close(hd.grad, hr.grad, 'grad h0'), close(cd.grad, cr.grad, 'grad c0')
    for n, v in ref.named_parameters():
        close(p[n].grad, v.grad, 'grad ' + n)


def test_layer_many_row_tiles_sampled_sequences():
    """B = 16 384, H = 512: 512 row tiles per step and 64-bit offsets into the (T,B,4H) tensors. Sequences are independent,
    so out, hT, cT and g_x of 64 sampled sequences equal an fp64 CPU run of those sequences alone."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    T, B, I, H = 4, 16384, 52, 512
    torch.manual_seed(11)
    ref = torch.nn.LSTM(I, H).double()
    x, up = torch.randn(T, B, I), torch.randn(T, B, H)
    h0, c0, uh, uc = (torch.randn(B, H) for _ in range(4))
    p = {n: v.detach().float().to(d) for n, v in ref.named_parameters()}
    xd = x.to(d).requires_grad_(True)
    out, hT, cT = ops.lstm_layer(xd, h0.to(d), c0.to(d), p['weight_ih_l0'], p['weight_hh_l0'], p['bias_ih_l0'], p['bias_hh_l0'])
    ((out * up.to(d)).sum() + (hT * uh.to(d)).sum() + (cT * uc.to(d)).sum()).backward()
    idx = torch.cat([torch.randperm(B - 2, generator=torch.Generator().manual_seed(5))[:62] + 1, torch.tensor([0, B - 1])])
    xr = x[:, idx].double().requires_grad_(True)
    out_r, (hT_r, cT_r) = ref(xr, (h0[idx].double()[None], c0[idx].double()[None]))
    ((out_r * up[:, idx].double()).sum() + (hT_r[0] * uh[idx].double()).sum() + (cT_r[0] * uc[idx].double()).sum()).backward()
    idx_d = idx.to(d)
    close(out[:, idx_d], out_r, 'out'), close(hT[idx_d], hT_r[0], 'hT'), close(cT[idx_d], cT_r[0], 'cT')
    close(xd.grad[:, idx_d], xr.grad, 'grad x')


@pytest.mark.parametrize('name', ['model_lstm_pose_changes', 'model_lstm_h191_pose_2d', 'model_lstm_body25_emb'])
def test_reference_fixture_on_the_device(name):
    from test_lstm_model import build_model, load_fixture
    d = dev()
    g = load_fixture(name)
    model = build_model(name, g).train().to(d)
    out = model(g['frames'].to(d))
    close(out, g['out'], 'out')
    (out * g['g_out'].to(d)).sum().backward()
    for n, p in model.named_parameters():
        close(p.grad, g['grad__' + n], 'grad ' + n)


def _pose_lifting(B, T):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(22742)
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
    flow = LitPoseLiftingFlow(movements_model=LSTM(input_nodes=CARLA_SKELETON), loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    return flow, dm


def _autoencoder(B, T, H=191):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(22742)
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
    model = LSTM(input_nodes=CARLA_SKELETON, hidden_size=H, movements_output_type=MT.pose_2d)
    flow = LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox')
    return flow, dm


def _check_against_twins(flow, batch, loss_fn):
    """loss and every parameter gradient of flow.training_step against the fp64 CPU twin, with the tolerance rule of
    test_cfg3_batch_size_parity_with_the_cpu_twin: max(1e-4, 2 x what fp32 on the CPU loses against fp64)."""
    frames = batch[0]
    twins = {torch.float64: copy.deepcopy(flow.movements_model).cpu().double(),
             torch.float32: copy.deepcopy(flow.movements_model).cpu().float()}
    flow.on_train_batch_start(batch, 0)
    out = flow.training_step(batch, 0)
    out['loss'].backward()
    ref = {}
    for dt, twin in twins.items():
        twin.train()
        loss = loss_fn(twin(frames.to('cpu', dt)), dt)
        loss.backward()
        ref[dt] = (loss.detach(), [p.grad for p in twin.parameters()])
    (l64, g64), (l32, g32) = ref[torch.float64], ref[torch.float32]
    close(out['loss'], l64, 'loss', rtol=max(1e-4, 2 * abs(float(l32) - float(l64)) / abs(float(l64))))
    for (n, p), q, q32 in zip(flow.movements_model.named_parameters(), g64, g32):
        ref_err = (q32.double() - q).abs().max().item() / (q.abs().max().item() + 1e-30)
        close(p.grad, q, 'grad ' + n, rtol=max(1e-4, 2 * ref_err))


def test_pose_lifting_training_step_matches_the_cpu_twin():
    """LitPoseLiftingFlow(LSTM()) with loc_2d_3d, B = 256, T = 16: the 6-D output feeds the fused pose head."""
    from oracle import pose_head as O
    d = dev()
    flow, dm = _pose_lifting(256, 16)
    flow.to(d).train()
    flow.attach_datamodule(dm)
    assert flow.movements_model.rotation_output_format == 'rotation_6d'
    batch = dm.generate_batch(d)
    _, targets, meta = batch

    def loss_fn(pred, dt):
        return O.pose_head(pred, 'pose_changes_6d', meta['skel_type'].cpu(), gt2d=targets['projection_2d_transformed'].to('cpu', dt),
                           gt3d=targets['absolute_pose_loc'].to('cpu', dt))['loc_2d_3d']
    _check_against_twins(flow, batch, loss_fn)


def test_autoencoder_training_step_h191_matches_the_cpu_twin():
    """LitAutoencoderFlow(LSTM(hidden_size=191, pose_2d)) with loc_2d, B = 256, T = 15: the recurrence is K18."""
    from oracle import pose_head as O
    d = dev()
    flow, dm = _autoencoder(256, 15)
    flow.to(d).train()
    batch = dm.generate_batch(d)
    targets = batch[1]
    _check_against_twins(flow, batch, lambda pred, dt: O.loss_loc_2d(pred, targets['projection_2d_transformed'].to('cpu', dt))[0])


def test_graph_replay_h191():
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _autoencoder(64, 15)
    trainer = Trainer(device=d, use_graph=True).setup(flow, dm)
    trainer.train_step(flow, dm.generate_batch(d), 0)
    diff, scale = trainer._replay_check
    assert trainer.use_graph and scale > 0 and diff == 0.0, (diff, scale)


@pytest.mark.parametrize('H', [64, 100, 1024])
def test_no_framework_rnn_up_to_1024(H, monkeypatch):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM

    def framework_rnn(*a, **k):
        raise AssertionError('the framework RNN ran')
    monkeypatch.setattr(torch.nn.LSTM, 'forward', framework_rnn)
    d = dev()
    torch.manual_seed(1)
    model = LSTM(input_nodes=CARLA_SKELETON, hidden_size=H, num_layers=2, embeddings_size=40).to(d)
    x = torch.randn(8, 5, 26, 2, device=d)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = model(x)
        out.sum().backward()
    assert out.shape == (8, 5, 26, 3, 3) and torch.isfinite(out).all()


def test_h1025_falls_back_with_a_warning_and_matches_the_cpu(monkeypatch):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import seq2seq as s2s
    monkeypatch.setattr(s2s, '_WARNED', set())
    d = dev()
    torch.manual_seed(2)
    model = LSTM(input_nodes=CARLA_SKELETON, hidden_size=1025, num_layers=1, movements_output_type=MT.pose_2d)
    cpu = copy.deepcopy(model).double()
    x = torch.randn(4, 3, 26, 2)
    with pytest.warns(RuntimeWarning, match='LSTM: nn.LSTM\\(hidden_size=1025'):
        out = model.to(d)(x.to(d))
    close(out, cpu(x.double()), 'out')


def test_k7b_widths_keep_k7b(monkeypatch):
    from pedestrians_video_2_carla_amd import _lib
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM
    counts = {}

    class Counting:
        def __init__(self, h):
            self._h = h

        def __getattr__(self, name):
            fn = getattr(self._h, name)
            if name not in ('p2c_lstm_rec_fwd', 'p2c_lstm_rec_bwd', 'p2c_lstm_steps_fwd', 'p2c_lstm_steps_bwd'):
                return fn

            def call(*a):
                counts[name] = counts.get(name, 0) + 1
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, '_lib', Counting(_lib.lib()))
    d = dev()
    x = torch.randn(8, 5, 26, 2, device=d)
    for H in (16, 32, 48, 64, 96, 128, 100):
        counts.clear()
        model = LSTM(input_nodes=CARLA_SKELETON, hidden_size=H, num_layers=2).to(d)
        model(x).sum().backward()
        if H == 100:
            assert counts == {'p2c_lstm_steps_fwd': 2, 'p2c_lstm_steps_bwd': 2}, counts
        else:
            assert counts == {'p2c_lstm_rec_fwd': 2, 'p2c_lstm_rec_bwd': 2}, (H, counts)
