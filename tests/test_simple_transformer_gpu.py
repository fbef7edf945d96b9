"""GPU: K20 (csrc/p2c_encoder.hip: attention with dropout for any head width, the post-norm residual LayerNorm for any width),
K16's ReLU + dropout epilogues (act 3 / 4), ``ops.post_norm_encoder_layer`` and the SimpleTransformer model on them.

(a) each kernel against fp64 framework ops with dropout 0 (d in {8, 50, 52, 256}, N in {1, 7, 16, 64}, odd row counts); bitwise
repeats; (b) the hashed dropout: keep fraction per site, distinct sites / steps, the backward's masks are the forward's; 2^31
refused without a launch; (c) the reference fixtures on the device; (d) training steps against the fp64 CPU twin, both trainers;
(e) graph capture with dropout 0.1; (f) no framework attention / dropout / LayerNorm / ReLU in the device step; (g) the fallback
above 64 tokens."""
import copy
import ctypes
import os
import sys

import pytest
import torch

from oracle import pose_head as O

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def close(a, b, what, rtol=RTOL, floor=0.0):
    """max |a - b| <= rtol * max(max |b|, floor)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), max(b.abs().max().item(), floor)
    assert err == err and err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


def _lib():
    from pedestrians_video_2_carla_amd import _lib as L
    return L.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------ (a) kernels
def attn_fwd(qkv, S, N, heads, hd, st=None, p=0.0, site=0):
    out = torch.empty(S * N, heads * hd, device=qkv.device)
    rc = _lib().p2c_attn_drop_fwd(qkv.data_ptr(), out.data_ptr(), 1.0 / hd ** 0.5, S, N, heads, hd, _ptr(st), p, site, _stream())
    assert rc == 0, rc
    return out


def attn_bwd(qkv, g, S, N, heads, hd, st=None, p=0.0, site=0):
    gq = torch.empty_like(qkv)
    rc = _lib().p2c_attn_drop_bwd(qkv.data_ptr(), g.data_ptr(), gq.data_ptr(), 1.0 / hd ** 0.5, S, N, heads, hd, _ptr(st), p, site,
                                  _stream())
    assert rc == 0, rc
    return gq


def attn_ref(qkv, S, N, heads, hd):
    q, k, v = qkv.view(S, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    a = torch.softmax(q @ k.transpose(-1, -2) / hd ** 0.5, -1)
    return (a @ v).permute(0, 2, 1, 3).reshape(S * N, heads * hd)


@pytest.mark.parametrize('d,heads,N,S', [(8, 2, 1, 3), (8, 2, 7, 5), (50, 5, 7, 9), (50, 25, 16, 3), (52, 4, 16, 33),
                                         (256, 4, 64, 3), (256, 1, 64, 2), (2, 1, 64, 5)])
def test_attention_matches_fp64(d, heads, N, S):
    g = torch.Generator().manual_seed(d + N)
    qkv = torch.randn(S * N, 3 * d, generator=g, dtype=torch.float64)
    go = torch.randn(S * N, d, generator=g, dtype=torch.float64)
    hd = d // heads
    q = qkv.float().to(dev())
    out = attn_fwd(q, S, N, heads, hd)
    gq = attn_bwd(q, go.float().to(dev()), S, N, heads, hd)
    r = qkv.clone().requires_grad_(True)
    ref = attn_ref(r, S, N, heads, hd)
    ref.backward(go)
    close(out, ref, 'out'), close(gq, r.grad, 'g_qkv')
    assert torch.equal(out, attn_fwd(q, S, N, heads, hd)) and torch.equal(gq, attn_bwd(q, go.float().to(dev()), S, N, heads, hd))


def postnorm(x, s, w, b, gz, st=None, p=0.0, site=0, eps=1e-5):
    lib = _lib()
    rows, D = x.shape
    z, stats = torch.empty_like(x), torch.empty(2, rows, device=x.device)
    assert lib.p2c_postnorm_fwd(x.data_ptr(), s.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), stats[0].data_ptr(),
                                stats[1].data_ptr(), rows, D, eps, _ptr(st), p, site, _stream()) == 0
    gx, gs, gw, gb = torch.empty_like(x), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    ws = torch.empty(max(1, lib.p2c_postnorm_workspace_floats(rows, D)), device=x.device)
    assert lib.p2c_postnorm_bwd(x.data_ptr(), s.data_ptr(), w.data_ptr(), stats[0].data_ptr(), stats[1].data_ptr(), gz.data_ptr(),
                                gx.data_ptr(), gs.data_ptr(), gw.data_ptr(), gb.data_ptr(), 0, ws.data_ptr(), rows, D, _ptr(st), p,
                                site, _stream()) == 0
    return z, gx, gs, gw, gb


@pytest.mark.parametrize('rows,D', [(1, 2), (37, 8), (1001, 50), (513, 52), (77, 256), (4099, 52), (33, 1000), (5, 1024)])
def test_postnorm_matches_fp64(rows, D):
    g = torch.Generator().manual_seed(rows + D)
    x, s, gz = (torch.randn(rows, D, generator=g, dtype=torch.float64) for _ in range(3))
    w, b = 1 + 0.1 * torch.randn(D, generator=g, dtype=torch.float64), 0.1 * torch.randn(D, generator=g, dtype=torch.float64)
    dv = lambda t: t.float().to(dev())      # noqa: E731
    res = postnorm(dv(x), dv(s), dv(w), dv(b), dv(gz))
    xr, sr, wr, br = (t.clone().requires_grad_(True) for t in (x, s, w, b))
    zr = torch.nn.functional.layer_norm(xr + sr, (D,), wr, br, 1e-5)
    zr.backward(gz)
    # (dx / ds: the three terms of the LayerNorm backward are of size rstd |gz gamma| and cancel -- for D = 2 almost completely)
    rstd = 1 / ((xr + sr).detach().var(-1, unbiased=False) + 1e-5).sqrt()
    floor = 1e-3 * float((rstd.view(-1, 1) * (gz * w).abs()).max())
    for got, want, what in zip(res, (zr, xr.grad, sr.grad, wr.grad, br.grad), ('z', 'dx', 'ds', 'dgamma', 'dbeta')):
        close(got, want, what, floor=floor if what in ('dx', 'ds') else 0.0)
    again = postnorm(dv(x), dv(s), dv(w), dv(b), dv(gz))
    assert all(torch.equal(a, b) for a, b in zip(res, again))


@pytest.mark.parametrize('M,N,K', [(37, 2048, 52), (1001, 2048, 50), (512, 64, 8)])
def test_gemm_relu_epilogues_match_fp64(M, N, K):
    from pedestrians_video_2_carla_amd import ops
    g = torch.Generator().manual_seed(M)
    x, w, bias = (torch.randn(M, K, generator=g, dtype=torch.float64), torch.randn(N, K, generator=g, dtype=torch.float64),
                  torch.randn(N, generator=g, dtype=torch.float64))
    gh = torch.randn(M, N, generator=g, dtype=torch.float64)
    h = ops.gemm(x.float().to(dev()), w.float().to(dev()), True, bias=bias.float().to(dev()), act=3)
    ref = torch.relu(x @ w.T + bias)
    close(h, ref, 'relu(xW^T + b)')
    w2 = torch.randn(K, N, generator=g, dtype=torch.float64)
    gs = torch.randn(M, K, generator=g, dtype=torch.float64)
    da = ops.gemm(gs.float().to(dev()), w2.float().to(dev()), False, act=4, aux=h)
    close(da, (gs @ w2) * (ref > 0), 'backward through relu')
    del gh


# ------------------------------------------------------------------------------------------------------------ (b) dropout
def _ffn_mask(st, p, site, M=999, N=2048):
    from pedestrians_video_2_carla_amd import ops
    ones = torch.ones(M, 4, device=dev())
    h = ops.gemm(ones, torch.full((N, 4), 0.25, device=dev()), True, act=3, drop_state=st, drop_p=p, drop_site=site)
    return h != 0


@pytest.mark.parametrize('p', [0.1, 0.5])
def test_dropout_keep_fraction_sites_and_steps(p):
    from pedestrians_video_2_carla_amd import ops
    torch.manual_seed(4)
    st = ops.dropout_state(dev())
    # FFN epilogue
    m0, m1 = _ffn_mask(st, p, 2), _ffn_mask(st, p, 6)
    for m in (m0, m1):
        assert abs(m.float().mean().item() - (1 - p)) < 0.01
    assert not torch.equal(m0, m1)
    # the post-norm residual: ds = dx keep / (1 - p)
    rows, D = 4001, 52
    x, s, gz = (torch.randn(rows, D, device=dev()) for _ in range(3))
    w, b = torch.ones(D, device=dev()), torch.zeros(D, device=dev())
    _, gx, gs, _, _ = postnorm(x, s, w, b, gz, st, p, 1)
    keep = (gs != 0)
    assert abs(keep.float().mean().item() - (1 - p)) < 0.01
    close(gs[keep], gx[keep] / (1 - p), 'kept ds')
    # attention probabilities: the next step draws other masks
    S, N, heads, hd = 64, 16, 4, 13
    qkv = torch.randn(S * N, 3 * heads * hd, device=dev())
    o1 = attn_fwd(qkv, S, N, heads, hd, st, p, 0)
    st_fwd = st.clone()
    attn_bwd(qkv, torch.randn(S * N, heads * hd, device=dev()), S, N, heads, hd, st, p, 0)
    assert int(st[2]) == int(st_fwd[3]) == int(st_fwd[2]) + 1
    o2 = attn_fwd(qkv, S, N, heads, hd, st, p, 0)
    assert not torch.equal(o1, o2)
    m2 = _ffn_mask(st, p, 2)
    assert not torch.equal(m0, m2)


def test_dropout_backward_uses_the_forward_mask():
    """One encoder layer with dropout 0.5 at all four sites: the forward's masks, read off its outputs, applied to an fp64 twin,
    give the layer's gradients."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    torch.manual_seed(9)
    layer = torch.nn.TransformerEncoderLayer(52, 4, dim_feedforward=64, dropout=0.5, batch_first=True).to(d).train()
    st = ops.dropout_state(d)
    B, T = 6, 16
    x = torch.randn(B, T, 52, device=d, requires_grad=True)
    snap = st.clone()
    z = ops.post_norm_encoder_layer(x, layer, 4, st, 0)
    gz = torch.randn_like(z)
    z.backward(gz)
    # masks of the four sites, redrawn by single kernel calls from the same stream position
    st2 = snap.clone()
    rows = B * T
    m_ff = _ffn_mask(st2, 0.5, 2, rows, 64).double().cpu() / 0.5
    zero, one, rnd = torch.zeros(rows, 52, device=d), torch.ones(52, device=d), torch.randn(rows, 52, device=d)
    _, _, gs1, _, _ = postnorm(zero, rnd, one, zero[0], rnd, st2, 0.5, 1)
    st2.copy_(snap)
    _, _, gs3, _, _ = postnorm(zero, rnd, one, zero[0], rnd, st2, 0.5, 3)
    st2.copy_(snap)
    m1 = (gs1 != 0).double().cpu() / 0.5
    m3 = (gs3 != 0).double().cpu() / 0.5
    S, N = B, T
    lr = copy.deepcopy(layer).cpu().double()
    xr = x.detach().cpu().double().requires_grad_(True)
    sa = lr.self_attn
    st2.copy_(snap)
    ma = _attn_masks(st2, S, N, 4, 13, 0.5)
    q, k, v = torch.nn.functional.linear(xr, sa.in_proj_weight, sa.in_proj_bias).view(B, T, 3, 4, 13).permute(2, 0, 3, 1, 4)
    a = torch.softmax(q @ k.transpose(-1, -2) / 13 ** 0.5, -1) * ma
    att = (a @ v).permute(0, 2, 1, 3).reshape(B, T, 52)
    x1 = lr.norm1(xr + sa.out_proj(att) * m1.view(B, T, 52))
    hh = torch.relu(lr.linear1(x1)) * m_ff.view(B, T, 64)
    zr = lr.norm2(x1 + lr.linear2(hh) * m3.view(B, T, 52))
    zr.backward(gz.cpu().double())
    close(z, zr, 'z', 1e-4), close(x.grad, xr.grad, 'dx', 1e-4)
    for (n, p), (_, pr) in zip(layer.named_parameters(), lr.named_parameters()):
        close(p.grad, pr.grad, n, 1e-4)


def _attn_masks(st, S, N, heads, hd, p):
    """The (S, heads, N, N) attention mask of the stream position in ``st``, read off the forward: q = k = 0 gives P = 1/N, and
    v = one-hot rows (hd >= N) or one pass per key block."""
    d = heads * hd
    out = torch.empty(S, heads, N, N, dtype=torch.float64)
    snap = st.clone()
    for j0 in range(0, N, hd):
        st.copy_(snap)
        qkv = torch.zeros(S, N, 3, heads, hd, device=st.device)
        for j in range(j0, min(N, j0 + hd)):
            qkv[:, j, 2, :, j - j0] = 1.0
        o = attn_fwd(qkv.view(S * N, 3 * d), S, N, heads, hd, st, p, 0).view(S, N, heads, hd)
        for j in range(j0, min(N, j0 + hd)):
            out[:, :, :, j] = (o[:, :, :, j - j0].permute(0, 2, 1) * N).double().cpu()
    st.copy_(snap)
    return out.round(decimals=3)


def test_2_pow_31_is_refused_without_a_launch():
    from pedestrians_video_2_carla_amd import _lib as L
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    st = ops.dropout_state(d)
    a, b = torch.zeros(1, 4, device=d), torch.zeros(4, 4, device=d)
    desc = L.GemmDesc()
    desc.M, desc.N, desc.K, desc.trans_b = 1 << 20, 2048, 4, 1
    desc.a, desc.lda, desc.b, desc.ldb, desc.c, desc.ldc = a.data_ptr(), 4, b.data_ptr(), 4, a.data_ptr(), 2048
    desc.act, desc.drop_state, desc.drop_p, desc.drop_site = 3, st.data_ptr(), 0.1, 0
    before = st.clone()
    assert _lib().p2c_gemm(ctypes.byref(desc), _stream()) == -2
    assert _lib().p2c_postnorm_fwd(a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr(),
                                   1 << 26, 32, 1e-5, st.data_ptr(), 0.1, 0, _stream()) == -2
    assert _lib().p2c_attn_drop_fwd(a.data_ptr(), a.data_ptr(), 1.0, 1 << 20, 64, 1, 4, st.data_ptr(), 0.1, 0, _stream()) == -2
    torch.cuda.synchronize()
    assert torch.equal(st, before)
    with pytest.warns(RuntimeWarning, match='2\\^31'):
        assert not ops.post_norm_encoder_layer_supported(1 << 16, 16, 52, 4, True)
    assert ops.post_norm_encoder_layer_supported(1 << 16, 16, 52, 4, False)


# ------------------------------------------------------------------------------------------------------------ (c) fixtures
def test_fixtures_on_the_device():
    from test_simple_transformer import load, nodes_of, tiny_model
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    d = dev()
    g = load('model_simple_transformer_tiny_0', 'model_simple_transformer_tiny_1', 'model_simple_transformer_tiny_grads')
    model = tiny_model(g).to(d).eval()
    out = model(g['frames'].to(d))
    close(out, g['out'], 'tiny out')
    (out * g['g_out'].to(d)).sum().backward()
    for n, p in model.named_parameters():
        if n.startswith('encoder_layer.'):
            assert p.grad is None
        else:
            close(p.grad, g['grad__' + n], 'tiny grad ' + n, 5e-4)
    for name in ('carla', 'body25'):
        g = load('model_simple_transformer_' + name)
        nodes, heads, seed = nodes_of(name)
        torch.manual_seed(seed)
        model = SimpleTransformer(input_nodes=nodes, n_heads=heads, movements_output_type='pose_2d').to(d).eval()
        out = model(g['frames'].to(d))
        close(out, g['out'], name + ' out')
        (out * g['g_out'].to(d)).sum().backward()
        for n, p in model.named_parameters():
            if p.grad is not None:
                assert abs(float(p.grad.double().norm()) - float(g['gnorm__' + n])) <= 5e-4 * float(g['gnorm__' + n]) + 1e-6, n


# ------------------------------------------------------------------------------------------------------------ (d)-(g) models
def _no_dropout(model):
    for layer in list(model.encoder.layers) + [model.encoder_layer]:
        layer.dropout.p = layer.dropout1.p = layer.dropout2.p = 0.0
        layer.self_attn.dropout = 0.0
    return model


def _flow(B=32, T=16, dropout=True):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(8)
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
    model = SimpleTransformer(input_nodes=CARLA_SKELETON, movements_output_type='pose_2d')
    if not dropout:
        _no_dropout(model)
    return LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox'), dm


def _check_grads(model, twins):
    cpu64, cpu32 = twins[torch.float64], twins[torch.float32]
    top = max(float(pc.grad.abs().max()) for pc in cpu64.parameters() if pc.grad is not None)
    for (n, pg), pc, pc32 in zip(model.named_parameters(), cpu64.parameters(), cpu32.parameters()):
        if pc.grad is None:
            assert pg.grad is None or float(pg.grad.abs().max()) == 0.0, n
            continue
        scale = max(float(pc.grad.abs().max()), 1e-3 * top)
        ref_err = float((pc32.grad.double() - pc.grad).abs().max()) / scale
        err = float((pg.grad.double().cpu() - pc.grad).abs().max())
        assert err <= max(5e-4, 2 * ref_err) * scale, (n, err, scale, ref_err)


@pytest.mark.parametrize('flatten', [False, True])
def test_flow_training_step_matches_the_cpu_twin_d52(flatten):
    from pedestrians_video_2_carla_amd import ops
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _flow(dropout=False)
    model = flow.movements_model
    twins = {dt: copy.deepcopy(model).to(dt).train() for dt in (torch.float64, torch.float32)}
    trainer = Trainer(device=d, flatten=flatten).setup(flow, dm)
    batch = dm.generate_batch(d)
    frames, targets, _ = batch
    flow.train()
    with ops.grad_sinks(trainer._grad_sinks):
        flow.on_train_batch_start(batch, 0)
        loss = flow.training_step(batch, 0)['loss']
        loss.backward()
    ref = {}
    for dt, twin in twins.items():
        r, _, _ = O.loss_loc_2d(twin(frames.to('cpu', dt)), targets['projection_2d_transformed'].to('cpu', dt))
        r.backward()
        ref[dt] = r.detach()
    l64, l32 = float(ref[torch.float64]), float(ref[torch.float32])
    close(loss, ref[torch.float64], 'loss', rtol=max(1e-4, 2 * abs(l32 - l64) / abs(l64)))
    _check_grads(model, twins)


@pytest.mark.parametrize('flatten', [False, True])
def test_model_training_step_matches_the_cpu_twin_d50(flatten):
    """BODY_25 (d = 50, 5 heads, T = 30): one step of the model under both gradient routes (autograd / the flat buffer's sinks).
    A pre-activation of the FFN within fp32 rounding of zero flips its ReLU gate against the fp64 twin and moves that layer's
    linear1 gradient by one row's contribution (seen: 2 % of the largest element with 16 clips): the shape and seed here are
    chosen so that none is within 1e-6 of zero in the fp64 twin, which the test checks first; then the flow rule holds."""
    from pedestrians_video_2_carla_amd import ops
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    from pedestrians_video_2_carla_amd.parallel.flat import FlatParameters
    d = dev()
    torch.manual_seed(17)
    model = _no_dropout(SimpleTransformer(input_nodes=BODY_25_SKELETON, n_heads=5, movements_output_type='pose_2d')).train()
    twins = {dt: copy.deepcopy(model).to(dt).train() for dt in (torch.float64, torch.float32)}
    model.to(d)
    if flatten:
        FlatParameters(model.parameters())
    g = torch.Generator().manual_seed(2)
    frames, tgt = torch.randn(4, 30, 25, 2, generator=g), torch.randn(4, 30, 25, 2, generator=g)
    gates = []
    for layer in twins[torch.float64].encoder.layers:
        layer.linear1.register_forward_hook(lambda mod, i, o: gates.append(float(o.detach().abs().min())))
    with ops.grad_sinks(flatten):
        loss = (model(frames.to(d)) - tgt.to(d)).pow(2).mean()
        loss.backward()
    for dt, twin in twins.items():
        ((twin(frames.to(dt)) - tgt.to(dt)).pow(2).mean()).backward()
    assert len(gates) == 6 and min(gates) > 1e-6, gates           # no ReLU gate at the edge of fp32 rounding
    _check_grads(model, twins)


def test_graph_capture_with_dropout():
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _flow(B=64, T=16, dropout=True)
    model = flow.movements_model
    tpl = [p.detach().clone() for p in model.encoder_layer.parameters()]
    trainer = Trainer(device=d, use_graph=True).setup(flow, dm)
    batch = dm.generate_batch(d)
    losses = [float(trainer.train_step(flow, batch, 0))]
    diff, scale = trainer._replay_check
    assert trainer.use_graph and scale > 0 and diff == 0.0, (diff, scale)
    for i in range(1, 50):
        losses.append(float(trainer.train_step(flow, batch, i)))
    torch.cuda.synchronize()
    assert all(l == l and abs(l) < float('inf') for l in losses), losses
    assert sum(losses[-5:]) < sum(losses[:5]), losses
    assert all(torch.equal(a.to(d), b.detach()) for a, b in zip(tpl, model.encoder_layer.parameters()))


@pytest.mark.parametrize('flatten', [False, True])
def test_template_unchanged_by_device_training(flatten):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _flow(B=16, T=16, dropout=True)
    model = flow.movements_model
    tpl = [p.detach().clone() for p in model.encoder_layer.parameters()]
    l0 = model.encoder.layers[0].linear1.weight.detach().clone()
    trainer = Trainer(device=d, flatten=flatten).setup(flow, dm)
    batch = dm.generate_batch(d)
    for i in range(3):
        trainer.train_step(flow, batch, i)
    torch.cuda.synchronize()
    assert all(torch.equal(a.to(d), b.detach()) for a, b in zip(tpl, model.encoder_layer.parameters()))
    assert not torch.equal(l0.to(d), model.encoder.layers[0].linear1.weight)


def test_no_framework_attention_dropout_layer_norm_or_relu_in_the_device_step(monkeypatch):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _flow(B=16, T=16, dropout=True)
    trainer = Trainer(device=d).setup(flow, dm)
    batch = dm.generate_batch(d)

    def framework(*a, **k):
        raise AssertionError('a framework attention / dropout / LayerNorm / ReLU ran')
    for owner, name in ((torch.nn.functional, 'multi_head_attention_forward'), (torch.nn.functional, 'dropout'),
                        (torch.nn.functional, 'layer_norm'), (torch.nn.functional, 'relu'), (torch, 'relu'),
                        (torch.nn.TransformerEncoderLayer, 'forward'), (torch.nn.TransformerEncoder, 'forward')):
        monkeypatch.setattr(owner, name, framework)
    loss = trainer.train_step(flow, batch, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(loss)


def test_fallback_above_64_tokens_warns_and_matches_the_framework():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    d = dev()
    torch.manual_seed(1)
    model = SimpleTransformer(input_nodes=CARLA_SKELETON, movements_output_type='pose_2d').to(d).eval()
    x = torch.randn(2, 65, 26, 2, device=d)
    with pytest.warns(RuntimeWarning, match='framework layers'):
        out = model(x)
    close(out, model.encoder(x.view(2, 65, 52)).view_as(x), 'fallback')
