"""GPU: K23, the GRU layer recurrence for any hidden size (csrc/p2c_gru_step.hip, p2c_gru_steps_*), through ops.gru_layer
against fp64 torch.nn.GRU on the CPU: out, hT, g_x, g_h0 and every parameter gradient within 1e-4 of the reference tensor's
max magnitude (the bound of tests/test_lstm_model_gpu.py). nn.GRU's default init keeps all four biases non-zero."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
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


# H below one unit tile and not a multiple of 4 or 16 (1, 20), one past the 64-wide K chunk (65), the width limit (1024);
# B below (1, 3), one past (33) and several times (70, 256) the 32-row tile; T = 1, where the zero state gives no recurrent product
CASES = [(1, 1, 5, 1), (4, 33, 52, 20), (15, 33, 52, 65), (4, 70, 32, 100), (15, 33, 52, 191), (2, 256, 52, 256), (4, 3, 16, 1024),
         (15, 1, 8, 1024)]


def _reference(T, B, I, H, with_state, use_out=True, use_hT=True):
    torch.manual_seed(T * 1000 + B + H)
    ref = torch.nn.GRU(I, H).double()
    x, h0 = torch.randn(T, B, I, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64)
    up, uh = torch.randn(T, B, H, dtype=torch.float64), torch.randn(B, H, dtype=torch.float64)
    xr, hr = x.clone().requires_grad_(True), h0.clone().requires_grad_(True)
    out_r, hT_r = ref(xr, hr[None]) if with_state else ref(xr)
    ((out_r * up).sum() * float(use_out) + (hT_r[0] * uh).sum() * float(use_hT)).backward()
    return ref, (x, h0, up, uh), (out_r, hT_r[0], xr.grad, hr.grad)


def _device(ref, tensors, with_state, use_out=True, use_hT=True):
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    x, h0, up, uh = tensors
    p = {n: v.detach().float().to(d).requires_grad_(True) for n, v in ref.named_parameters()}
    xd, hd = x.float().to(d).requires_grad_(True), h0.float().to(d).requires_grad_(True)
    out, hT = ops.gru_layer(xd, hd if with_state else None, p['weight_ih_l0'], p['weight_hh_l0'], p['bias_ih_l0'], p['bias_hh_l0'])
    loss = 0
    if use_out:
        loss = loss + (out * up.float().to(d)).sum()
    if use_hT:
        loss = loss + (hT * uh.float().to(d)).sum()
    loss.backward()
    return p, (out, hT, xd.grad, hd.grad)


def _compare(ref, p, got, want, with_state):
    for name, a, b in zip(('out', 'hT', 'grad x'), got, want):
        close(a, b, name)
    if with_state:
        close(got[3], want[3], 'grad h0')
    else:
        assert got[3] is None
    for n, v in ref.named_parameters():
        assert float(v.detach().abs().max()) > 0, n          # (the biases too: b_hn inside the reset product is exercised)
        close(p[n].grad, v.grad, 'grad ' + n)


@pytest.mark.parametrize('T,B,I,H', CASES)
@pytest.mark.parametrize('with_state', [False, True])
def test_layer_matches_torch_gru(T, B, I, H, with_state):
    ref, tensors, want = _reference(T, B, I, H, with_state)
    p, got = _device(ref, tensors, with_state)
    _compare(ref, p, got, want, with_state)


@pytest.mark.parametrize('with_state', [False, True])
@pytest.mark.parametrize('use_out,use_hT', [(False, True), (True, False)])
def test_one_output_unused(use_out, use_hT, with_state):
    """Only hT used (g_out is None: the classifier's backward) / only out used (g_hT is None)."""
    ref, tensors, want = _reference(5, 33, 12, 65, with_state, use_out, use_hT)
    p, got = _device(ref, tensors, with_state, use_out, use_hT)
    _compare(ref, p, got, want, with_state)


def test_width_above_the_limit_is_refused_with_nothing_written():
    from pedestrians_video_2_carla_amd import _lib
    d = dev()
    T, B, H = 2, 3, 1025
    f = dict(device=d, dtype=torch.float32)
    gx, w, out, acts = torch.zeros(T, B, 3 * H, **f), torch.zeros(3 * H, H, **f), torch.full((T, B, H), 7.0, **f), torch.full((T, B, 4 * H), 7.0, **f)
    g_gx, g_gh, ws = torch.full((T, B, 3 * H), 7.0, **f), torch.full((T, B, 3 * H), 7.0, **f), torch.full((B, H), 7.0, **f)
    desc = _lib.GruDesc()
    desc.T, desc.B, desc.H = T, B, H
    desc.gx, desc.w_hh, desc.out, desc.acts, desc.g_gx, desc.g_gh = (t.data_ptr() for t in (gx, w, out, acts, g_gx, g_gh))
    stream = torch.cuda.current_stream().cuda_stream
    assert _lib.lib().p2c_gru_steps_fwd(ctypes.byref(desc), stream) == -2
    assert _lib.lib().p2c_gru_steps_bwd(ctypes.byref(desc), ws.data_ptr(), stream) == -2
    torch.cuda.synchronize()
    for t in (out, acts, g_gx, g_gh, ws):
        assert bool((t == 7.0).all())
    from pedestrians_video_2_carla_amd import ops
    assert ops.gru_steps_supported(1024) and not ops.gru_steps_supported(1025) and not ops.gru_steps_supported(0)
    with pytest.raises(RuntimeError, match='1025'):
        ops.gru_layer(torch.zeros(T, B, 4, **f), None, torch.zeros(3 * H, 4, **f), w, None, None)


def test_layer_many_row_tiles_sampled_sequences():
    """B = 16 384, H = 512, T = 2: 512 row tiles per step and 64-bit offsets into the (T,B,3H) / (T,B,4H) tensors. Sequences are
    independent, so out, hT and g_x of 64 sampled sequences equal an fp64 CPU run of those sequences alone."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    T, B, I, H = 2, 16384, 52, 512
    torch.manual_seed(11)
    ref = torch.nn.GRU(I, H).double()
    x, up = torch.randn(T, B, I), torch.randn(T, B, H)
    h0, uh = torch.randn(B, H), torch.randn(B, H)
    p = {n: v.detach().float().to(d) for n, v in ref.named_parameters()}
    xd, hd = x.to(d).requires_grad_(True), h0.to(d).requires_grad_(True)
    out, hT = ops.gru_layer(xd, hd, p['weight_ih_l0'], p['weight_hh_l0'], p['bias_ih_l0'], p['bias_hh_l0'])
    ((out * up.to(d)).sum() + (hT * uh.to(d)).sum()).backward()
    idx = torch.cat([torch.randperm(B - 2, generator=torch.Generator().manual_seed(5))[:62] + 1, torch.tensor([0, B - 1])])
    xr, hr = x[:, idx].double().requires_grad_(True), h0[idx].double().requires_grad_(True)
    out_r, hT_r = ref(xr, hr[None])
    ((out_r * up[:, idx].double()).sum() + (hT_r[0] * uh[idx].double()).sum()).backward()
    idx_d = idx.to(d)
    close(out[:, idx_d], out_r, 'out'), close(hT[idx_d], hT_r[0], 'hT')
    close(xd.grad[:, idx_d], xr.grad, 'grad x'), close(hd.grad[idx_d], hr.grad, 'grad h0')
