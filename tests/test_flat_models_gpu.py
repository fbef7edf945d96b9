"""GPU: Seq2SeqFlatEmbeddings (K21 front end), LinearAE2D and Linear on the device: (a) the reference fixtures; (b) one training
step of each flow against its fp64 CPU twin; (c) no framework linear / RNN on the device; (d) the K16 composition for widths
outside K21; (e) graph replay."""
import copy
import os
import sys

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


def _fixture_names():
    from test_flat_models import FIXTURES
    return sorted(FIXTURES)


@pytest.mark.parametrize('name', _fixture_names())
def test_reference_fixture_on_the_device(name):
    from test_flat_models import build_model, load_fixture
    d = dev()
    g = load_fixture(name)
    model = build_model(name, g).train().to(d)
    out = model(g['frames'].to(d))
    close(out, g['out'], 'out')
    (out * g['g_out'].to(d)).sum().backward()
    for n, p in model.named_parameters():
        close(p.grad, g['grad__' + n], 'grad ' + n)


def _model(kind, **kw):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements import Linear
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE2D
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqFlatEmbeddings
    if kind == 'flat':
        return Seq2SeqFlatEmbeddings(input_nodes=CARLA_SKELETON, movements_output_type=MT.pose_2d, **kw)
    if kind == 'ae2d':
        return LinearAE2D(input_nodes=CARLA_SKELETON, **kw)
    return Linear(input_nodes=CARLA_SKELETON, **kw)


def _autoencoder(model, B=33, T=15):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
    return LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox'), dm


def _seeded(kind, **kw):
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(22742)
    return _model(kind, **kw)


def _check_against_twins(flow, batch, loss_fn):
    """loss and every parameter gradient of flow.training_step against the fp64 CPU twin: max(1e-4, 2 x what fp32 on the CPU loses
    against fp64) (the rule of test_lstm_model_gpu._check_against_twins)."""
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
        assert p.grad is not None, n
        ref_err = (q32.double() - q).abs().max().item() / (q.abs().max().item() + 1e-30)
        close(p.grad, q, 'grad ' + n, rtol=max(1e-4, 2 * ref_err))


def _autoencoder_step_matches(model):
    from oracle import pose_head as O
    d = dev()
    flow, dm = _autoencoder(model)
    flow.to(d).train()
    batch = dm.generate_batch(d)
    targets = batch[1]
    _check_against_twins(flow, batch, lambda pred, dt: O.loss_loc_2d(pred, targets['projection_2d_transformed'].to('cpu', dt))[0])


@pytest.mark.parametrize('kind,kw', [('flat', dict(p_dropout=0.0, hidden_size=64)), ('ae2d', {})], ids=['Seq2SeqFlatEmbeddings', 'LinearAE2D'])
def test_autoencoder_training_step_matches_the_cpu_twin(kind, kw):
    _autoencoder_step_matches(_seeded(kind, **kw))


@pytest.mark.parametrize('kind,kw', [('flat', dict(p_dropout=0.0, hidden_size=64, embeddings_size=[512, 256])),
                                     ('flat', dict(p_dropout=0.0, hidden_size=64, embeddings_size=[512, 256], invert_sequence=True)),
                                     ('ae2d', dict(model_scaling_factor=4))], ids=['flat-512-256', 'flat-512-256-inverted', 'ae2d-f4'])
def test_widths_outside_the_fused_kernels_take_the_k16_composition(kind, kw, monkeypatch):
    from pedestrians_video_2_carla_amd import ops
    if kind == 'flat':
        assert not ops.relu_stack_supported([52, 512, 256])
    calls = []
    real = ops.dense_chain
    monkeypatch.setattr(ops, 'dense_chain', lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    _autoencoder_step_matches(_seeded(kind, **kw))
    assert calls


def test_linear_pose_lifting_training_step_matches_the_cpu_twin():
    from oracle import pose_head as O
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    d = dev()
    model = _seeded('linear')
    dm = SyntheticCarlaRecordedDataModule(clip_length=15, batch_size=33, missing_joint_probabilities=0.1)
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')
    flow.to(d).train()
    flow.attach_datamodule(dm)
    assert model.rotation_output_format == 'rotation_6d'
    batch = dm.generate_batch(d)
    _, targets, meta = batch

    def loss_fn(pred, dt):
        return O.pose_head(pred, 'pose_changes_6d', meta['skel_type'].cpu(), gt2d=targets['projection_2d_transformed'].to('cpu', dt),
                           gt3d=targets['absolute_pose_loc'].to('cpu', dt))['loc_2d_3d']
    _check_against_twins(flow, batch, loss_fn)


@pytest.mark.parametrize('kind', ['flat', 'ae2d'])
def test_no_framework_linear_or_rnn_on_the_device(kind, monkeypatch):
    from pedestrians_video_2_carla_amd import _lib

    def framework_op(*a, **k):
        raise AssertionError('a framework linear / RNN ran on the device')
    monkeypatch.setattr(torch.nn.functional, 'linear', framework_op)
    monkeypatch.setattr(torch.nn.LSTM, 'forward', framework_op)
    counts = {}

    class Counting:
        def __init__(self, h):
            self._h = h

        def __getattr__(self, name):
            fn = getattr(self._h, name)
            if not name.startswith('p2c_relu_stack_') or name.endswith('supported') or name.endswith('floats'):
                return fn

            def call(*a):
                counts[name] = counts.get(name, 0) + 1
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, '_lib', Counting(_lib.lib()))
    d = dev()
    flow, dm = _autoencoder(_seeded(kind))                       # defaults (dropout 0.2 in the recurrent stacks)
    flow.to(d).train()
    batch = dm.generate_batch(d)
    flow.on_train_batch_start(batch, 0)
    out = flow.training_step(batch, 0)
    out['loss'].backward()
    assert torch.isfinite(out['loss'])
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in flow.movements_model.parameters())
    assert counts == ({'p2c_relu_stack_fwd': 1, 'p2c_relu_stack_bwd': 1} if kind == 'flat' else {}), counts


def test_graph_replay_flat_embeddings():
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _autoencoder(_seeded('flat', p_dropout=0.0), B=64)
    trainer = Trainer(device=d, use_graph=True).setup(flow, dm)
    trainer.train_step(flow, dm.generate_batch(d), 0)
    diff, scale = trainer._replay_check
    assert trainer.use_graph and scale > 0 and diff == 0.0, (diff, scale)
