"""GPU: K24, the classification head in one launch (csrc/p2c_cls_head.hip) through ops.classification_loss against fp64
CrossEntropyLoss / BCEWithLogitsLoss on the CPU. Bound: 1e-5 of the reference tensor's max magnitude -- a handful of fp32
roundings per row (exp, log, at most 32 adds) plus a log2 B-deep fixed tree, about 2.5e-6; the confusion matrix is exact."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
RTOL = 1e-5


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def close(a, b, what, rtol=RTOL):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    print(f'{what}: err {err:.3e} scale {scale:.3e}')
    assert err == err and err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


def confusion_of(pred, target, C):
    m = np.zeros((C, C), dtype=np.int64)
    for t, p in zip(target.tolist(), pred.tolist()):
        if 0 <= t < C:
            m[t, p] += 1
    return m


def case(B, C, scale=1.0, seed=0):
    """Logits with tied maxima in some rows, targets with some -100 and some C (ignored) rows when the batch is large enough."""
    g = torch.Generator().manual_seed(B * 100 + C + seed)
    x = torch.randn(B, C, generator=g) * scale
    for b in range(0, B, 5):                         # ties: two or more equal maxima, the first index must win
        x[b, torch.randperm(C, generator=g)[:2]] = x[b].max() + 1.0
    t = torch.randint(0, C, (B,), generator=g)
    if B >= 7:
        t[3], t[B - 1] = -100, C
    return x, t


def run_device(x, t, confusion=None, binary=False, weight=1.0):
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    xd = x.to(d).requires_grad_(True)
    loss = ops.classification_loss(xd, t.to(d), confusion=confusion, binary=binary)
    (loss * weight).backward()
    return loss, xd.grad


@pytest.mark.parametrize('B', [1, 7, 64, 257, 5000])
@pytest.mark.parametrize('C', [2, 3, 5, 32])
@pytest.mark.parametrize('scale', [1.0, 50.0])
def test_cross_entropy_gradient_and_counts(B, C, scale):
    x, t = case(B, C, scale)
    ref_t = torch.where((t >= 0) & (t < C), t, torch.full_like(t, -100))
    xr = x.double().requires_grad_(True)
    want = torch.nn.CrossEntropyLoss()(xr, ref_t)
    (want * 3.0).backward()
    cm = torch.zeros(C, C, dtype=torch.int32, device=dev())
    loss, grad = run_device(x, t, cm, weight=3.0)
    close(loss, want, 'loss'), close(grad, xr.grad, 'd logits')
    assert loss.shape == () and np.array_equal(cm.cpu().numpy(), confusion_of(x.argmax(-1), t, C))
    # two calls accumulate into one matrix; two runs give the same bits
    loss2, grad2 = run_device(x, t, cm, weight=3.0)
    assert np.array_equal(cm.cpu().numpy(), 2 * confusion_of(x.argmax(-1), t, C))
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


def test_tied_maxima_go_to_the_first_index():
    d = dev()
    from pedestrians_video_2_carla_amd import ops
    x = torch.tensor([[1.0, 4.0, 4.0, 0.0], [2.0, 2.0, 2.0, 2.0], [0.0, -1.0, 3.0, 3.0], [5.0, 0.0, 5.0, 5.0]])
    t = torch.tensor([3, 3, 3, 3])
    cm = torch.zeros(4, 4, dtype=torch.int32, device=d)
    ops.classification_loss(x.to(d), t.to(d), confusion=cm)
    assert cm.cpu().tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [2, 1, 1, 0]]
    assert torch.equal(x.argmax(-1), torch.tensor([1, 0, 2, 0]))


def test_all_rows_ignored_gives_nan_and_counts_nothing():
    d = dev()
    x = torch.randn(9, 3, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([-100, 3, -1, -100, 7, 3, -100, 2 ** 40, -2 ** 40])
    cm = torch.zeros(3, 3, dtype=torch.int32, device=d)
    loss, grad = run_device(x, t, cm)
    assert torch.isnan(loss) and int(cm.sum()) == 0 and bool((grad == 0).all())
    assert torch.isnan(torch.nn.CrossEntropyLoss()(x, torch.full((9,), -100)))


@pytest.mark.parametrize('B', [1, 7, 257, 5000])
@pytest.mark.parametrize('column', [False, True])
def test_binary_mode(B, column):
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, generator=g) * 20.0
    t = torch.randint(0, 2, (B,), generator=g)
    xr = x.double().requires_grad_(True)
    want = torch.nn.BCEWithLogitsLoss()(xr, t.double())
    want.backward()
    cm = torch.zeros(2, 2, dtype=torch.int32, device=dev())
    loss, grad = run_device(x[:, None] if column else x, t, cm, binary=True)
    close(loss, want, 'loss'), close(grad.reshape(-1), xr.grad, 'd logits')
    assert grad.shape == ((B, 1) if column else (B,))
    assert np.array_equal(cm.cpu().numpy(), confusion_of((x > 0).long(), t, 2))


def test_count_only_leaves_loss_and_gradient_unwritten():
    from pedestrians_video_2_carla_amd import _lib, ops
    d = dev()
    x, t = case(257, 5)
    xd, td = x.to(d), t.to(d)
    loss, grad = torch.full((1,), 7.0, device=d), torch.full((257, 5), 7.0, device=d)
    cm = torch.zeros(5, 5, dtype=torch.int32, device=d)
    rc = _lib.lib().p2c_cls_head(xd.data_ptr(), td.data_ptr(), 257, 5, _lib.P2C_CLS_COUNT_ONLY, loss.data_ptr(), grad.data_ptr(),
                                 cm.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((loss == 7.0).all()) and bool((grad == 7.0).all())
    assert np.array_equal(cm.cpu().numpy(), confusion_of(x.argmax(-1), t, 5))
    ops.classification_count(xd, td, cm)
    assert np.array_equal(cm.cpu().numpy(), 2 * confusion_of(x.argmax(-1), t, 5))
    cb = torch.zeros(2, 2, dtype=torch.int32, device=d)
    ops.classification_count(xd[:, :1], (td % 2), cb, binary=True)
    assert np.array_equal(cb.cpu().numpy(), confusion_of((x[:, 0] > 0).long(), t % 2, 2))


def test_more_than_32_classes_take_the_tensor_path(monkeypatch):
    from pedestrians_video_2_carla_amd import _lib
    C, B = 33, 64
    x, t = case(B, C)
    calls = []

    class Counting:
        def __init__(self, h):
            self._h = h

        def __getattr__(self, name):
            if name == 'p2c_cls_head':
                calls.append(name)
            return getattr(self._h, name)
    monkeypatch.setattr(_lib, '_lib', Counting(_lib.lib()))
    xr = x.double().requires_grad_(True)
    ref_t = torch.where((t >= 0) & (t < C), t, torch.full_like(t, -100))
    want = torch.nn.CrossEntropyLoss()(xr, ref_t)
    want.backward()
    cm = torch.zeros(C, C, dtype=torch.int32, device=dev())
    loss, grad = run_device(x, ref_t, cm)
    assert not calls
    close(loss, want, 'loss', 1e-5), close(grad, xr.grad, 'd logits', 1e-5)
    assert np.array_equal(cm.cpu().numpy(), confusion_of(x.argmax(-1), ref_t, C))
    # and 32 classes do take the kernel
    x32, t32 = case(B, 32)
    run_device(x32, t32)
    assert calls
