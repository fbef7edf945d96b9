"""GPU: the LSTM / GRU classifiers and LitClassificationFlow on the device. (a) the reference fixtures model_cls_*.npz, outputs and
gradients; (b) one Trainer.fit step per model against an fp64 CPU twin; (c) three steps stay finite under check_finite;
(d) Trainer.validate over two batches returns the metrics of the summed matrix; (e) no framework RNN up to H = 1024;
(f) P2C_CLS_FRAMEWORK=1 gives the same numbers through the framework arm. Bound: 1e-4 of the reference tensor's max magnitude."""
import copy
import os
import sys
import warnings

import numpy as np
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
    print(f'{what}: err {err:.3e} scale {scale:.3e}')
    assert err == err and err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


@pytest.mark.parametrize('name', ['model_cls_gru_default', 'model_cls_gru_body25_emb', 'model_cls_gru_h191', 'model_cls_lstm_default'])
def test_reference_fixture_on_the_device(name):
    from test_classification import build_model, load_fixture
    d = dev()
    g = load_fixture(name)
    model = build_model(name, g).train().to(d)
    out = model(g['frames'].to(d))
    close(out, g['out'], 'out')
    (out * g['g_out'].to(d)).sum().backward()
    for n, p in model.named_parameters():
        close(p.grad, g['grad__' + n], 'grad ' + n)


def _flow(model_name, num_classes=3, H=64, L=2, **kw):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules import classification
    from pedestrians_video_2_carla_amd.modules.flow.classification import LitClassificationFlow
    torch.manual_seed(7)
    model = getattr(classification, model_name)(input_nodes=CARLA_SKELETON, hidden_size=H, num_layers=L, num_classes=num_classes,
                                                classification_lr=1e-3)
    return LitClassificationFlow(classification_model=model, classification_targets_key='cross', num_classes=num_classes, **kw)


def _batches(n, B=33, T=6, C=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, T, 26, 2, generator=g), {'cross': torch.randint(0, C, (B, 1), generator=g)}, {}) for _ in range(n)]


def _to(batch, d):
    return batch[0].to(d), {k: v.to(d) for k, v in batch[1].items()}, batch[2]


def _twin_step(flow, batch):
    """One AdamW step of an fp64 CPU copy of the model on the same batch: (loss, updated parameters)."""
    twin = copy.deepcopy(flow.classification_model).cpu().double()
    opt = torch.optim.AdamW(twin.parameters(), lr=twin.learning_rate, weight_decay=twin.lr_weight_decay)
    loss = torch.nn.CrossEntropyLoss()(twin(batch[0].double()), batch[1]['cross'][:, 0])
    loss.backward()
    opt.step()
    return loss.detach(), twin


@pytest.mark.parametrize('model_name,H', [('GRU', 64), ('LSTM', 64), ('GRU', 100), ('LSTM', 100)])
def test_one_fit_step_matches_the_cpu_twin(model_name, H):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow = _flow(model_name, H=H)
    (batch,) = _batches(1)
    want_loss, twin = _twin_step(flow, batch)
    before = [p.detach().clone() for p in flow.classification_model.parameters()]
    trainer = Trainer(max_steps=1, device=d, use_graph=False)
    (loss,) = trainer.fit(flow, None, batches=[_to(batch, d)])
    close(loss, want_loss, 'loss')
    lr = twin.learning_rate
    for (n, p), q, p0 in zip(flow.classification_model.named_parameters(), twin.parameters(), before):
        # Adam's first step is lr * g / (|g| + eps): where |g| is far below the gradient's own fp32 error the step's size is decided
        # by that error, on either side. The updated parameters are compared (1e-4 of max |parameter|) where the reference gradient
        # is at least 1e-3 of its tensor's largest -- a relative gradient error of 1e-6 moves the step by 1e-3 lr = 1e-6 there, and
        # a wrong step (lr = 1e-3) is 80 tolerances away; everywhere else the step is bounded by lr.
        new, ref, scale = p.detach().cpu().double(), q.detach(), q.detach().abs().max().item()
        sure = q.grad.abs() >= 1e-3 * q.grad.abs().max()
        err = ((new - ref).abs() * sure).max().item()
        print(f'updated {n}: err {err:.3e} scale {scale:.3e} ({int(sure.sum())} of {sure.numel()} elements)')
        assert sure.float().mean() > 0.5 and err <= RTOL * scale, f'updated {n}: {err:.3e} vs scale {scale:.3e}'
        assert float((new - p0.double()).abs().max()) <= lr * 1.001 + 1e-7 * scale
    assert int(flow.confusion.sum()) == 33
    flow.check_finite('train')


@pytest.mark.parametrize('model_name', ['GRU', 'LSTM'])
def test_three_steps_stay_finite(model_name):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow = _flow(model_name)
    trainer = Trainer(max_steps=3, device=d, use_graph=False, log_every_n_steps=1)
    losses = trainer.fit(flow, None, batches=[_to(b, d) for b in _batches(3)])
    assert len(losses) == 3 and all(bool(torch.isfinite(v)) for v in losses)
    assert all(bool(torch.isfinite(p).all()) for p in flow.parameters())


def test_validate_returns_the_metrics_of_the_summed_matrix():
    from pedestrians_video_2_carla_amd.modules.flow.classification import classification_metrics
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow = _flow('GRU', classification_average='macro')
    trainer = Trainer(device=d, use_graph=False).setup(flow, None)
    batches = _batches(2, seed=3)
    got = trainer.validate(flow, [_to(b, d) for b in batches])
    twin = copy.deepcopy(flow.classification_model).cpu().double().eval()
    m = np.zeros((3, 3), dtype=np.int64)
    with torch.no_grad():
        for frames, targets, _ in batches:
            logits = twin(frames.double())
            assert float((logits.topk(2).values[:, 0] - logits.topk(2).values[:, 1]).min()) > 1e-4      # no near ties to flip
            for t, p in zip(targets['cross'][:, 0].tolist(), logits.argmax(-1).tolist()):
                m[t, p] += 1
    assert got['ConfusionMatrix'] == m.tolist() and m.sum() == 66
    for k, v in classification_metrics(m, flow._average).items():
        assert got[k] == v
    assert flow.training and int(flow.confusion.sum()) == 0 and 'val_loss/primary' in flow.logged


@pytest.mark.parametrize('model_name', ['GRU', 'LSTM'])
@pytest.mark.parametrize('H', [64, 100, 1024])
def test_no_framework_rnn_up_to_1024(model_name, H, monkeypatch):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules import classification

    def framework_rnn(*a, **k):
        raise AssertionError('the framework RNN ran')
    monkeypatch.setattr(torch.nn.GRU, 'forward', framework_rnn)
    monkeypatch.setattr(torch.nn.LSTM, 'forward', framework_rnn)
    d = dev()
    torch.manual_seed(1)
    model = getattr(classification, model_name)(input_nodes=CARLA_SKELETON, hidden_size=H, num_layers=2, embeddings_size=40,
                                                num_classes=4).to(d)
    x = torch.randn(8, 5, 26, 2, device=d)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = model(x)
        out.sum().backward()
    assert out.shape == (8, 4) and torch.isfinite(out).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_h1025_falls_back_with_a_warning(monkeypatch):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.classification import GRU
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import seq2seq as s2s
    monkeypatch.setattr(s2s, '_WARNED', set())
    d = dev()
    torch.manual_seed(2)
    model = GRU(input_nodes=CARLA_SKELETON, hidden_size=1025, num_layers=1)
    cpu = copy.deepcopy(model).double()
    x = torch.randn(4, 3, 26, 2)
    with pytest.warns(RuntimeWarning, match='classification GRU: nn.GRU\\(hidden_size=1025'):
        out = model.to(d)(x.to(d))
    close(out, cpu(x.double()), 'out')


@pytest.mark.parametrize('model_name', ['GRU', 'LSTM'])
def test_framework_arm_gives_the_same_numbers(model_name, monkeypatch):
    from pedestrians_video_2_carla_amd import _lib
    d = dev()
    (batch,) = _batches(1, seed=9)
    batch = _to(batch, d)
    results = {}
    for arm in ('hip', 'framework'):
        monkeypatch.setenv('P2C_CLS_FRAMEWORK', '1' if arm == 'framework' else '0')
        calls = []

        class Counting:
            def __init__(self, h):
                self._h = h

            def __getattr__(self, name):
                if name in ('p2c_gru_steps_fwd', 'p2c_lstm_rec_fwd', 'p2c_lstm_steps_fwd', 'p2c_cls_head'):
                    calls.append(name)
                return getattr(self._h, name)
        real = _lib.lib()
        monkeypatch.setattr(_lib, '_lib', Counting(real))
        flow = _flow(model_name).to(d)
        out = flow.training_step(batch, 0)
        out['loss'].backward()
        monkeypatch.setattr(_lib, '_lib', real)
        assert bool(calls) == (arm == 'hip'), (arm, calls)
        results[arm] = (out['loss'].detach(), [p.grad.clone() for p in flow.parameters()], flow.confusion.clone())
    close(results['hip'][0], results['framework'][0], 'loss')
    for a, b in zip(results['hip'][1], results['framework'][1]):
        close(a, b, 'grad')
    assert torch.equal(results['hip'][2], results['framework'][2])
