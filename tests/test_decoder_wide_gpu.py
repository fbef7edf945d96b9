"""K7c for 64 < O <= 160 (csrc/p2c_s2s_wide.h): the decoder loop of Seq2Seq in one launch each way at the widths of the
absolute_loc (78) and pose_changes / relative_rot (156) outputs -- kernel level against the per-step formula in fp64 (tolerances of
tests/test_lstm_gpu.py: output 1e-4, gradients 2e-4, relative to the tensor's max), model, fixture and flow level on top.
The one test without the ``gpu`` mark loads the reference fixture into the module on the CPU."""
import functools

import pytest
import torch

gpu = pytest.mark.gpu
H = 64


@pytest.fixture(params=['narrow', 'wide'])
def rec_tile(request, monkeypatch):
    """Both values of the tiling switch: only the 16-clip tiling exists for O > 64, so the switch must change nothing."""
    monkeypatch.setenv('P2C_REC_TILE', request.param)
    return request.param


@pytest.fixture(autouse=True)
def wide_on(monkeypatch):
    """The fused loop at 64 < O <= 160 is opt-in (ops.decoder_loop_supported): every test here runs with it switched on."""
    monkeypatch.setenv('P2C_DECODER_WIDE', '1')


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def close(a, b, what, rtol=1e-4):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    print(f'{what}: err {err:.3e} scale {scale:.3e} rel {err / (scale + 1e-30):.3e} (bound {rtol:.1e})')
    assert err == err and err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


def _cell(gates, c_enc):
    i, f, gg, o = gates.chunk(4, -1)
    return torch.sigmoid(o) * torch.tanh(torch.sigmoid(f) * c_enc + torch.sigmoid(i) * torch.tanh(gg))


@functools.lru_cache(maxsize=None)
def _loop_reference(T, B, O, with_drop):
    """The per-step formula in fp64 (computed once per shape, shared by the two tiling runs; read-only)."""
    g = torch.Generator().manual_seed(T * 7 + B)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.3
    P = {'k0': rnd(B, 4 * H), 'c0': rnd(B, H), 'k1': rnd(B, 4 * H), 'c1': rnd(B, H), 'w_ih0': rnd(4 * H, O),
         'w_ih1': rnd(4 * H, H), 'w_fc': rnd(O, H), 'b_fc': rnd(O)}
    drop = (torch.rand(T, B, H, generator=g) < 0.8).double() / 0.8 if with_drop else None
    up = torch.randn(T, B, O, generator=g, dtype=torch.float64)
    R = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    x, outs = torch.zeros(B, O, dtype=torch.float64), []
    for t in range(T):
        h0 = _cell(x @ R['w_ih0'].t() + R['k0'], R['c0'])
        if drop is not None:
            h0 = h0 * drop[t]
        h1 = _cell(h0 @ R['w_ih1'].t() + R['k1'], R['c1'])
        x = h1 @ R['w_fc'].t() + R['b_fc']
        outs.append(x)
    ref = torch.stack(outs)
    (ref * up).sum().backward()
    return P, drop, up, ref.detach(), {k: v.grad for k, v in R.items()}


@gpu
@pytest.mark.parametrize('T,B,O,with_drop', [(1, 1, 65, False), (16, 37, 156, True), (5, 16, 160, False), (16, 130, 78, True),
                                             (3, 5, 97, False)] + [
    (T, B, O, with_drop) for T, O in ((3, 66), (5, 79), (4, 80), (5, 81), (2, 159)) for B, with_drop in ((5, False), (17, True))])
def test_wide_decoder_loop_matches_the_per_step_formula(T, B, O, with_drop, rec_tile):
    """K7c against the reference loop written out in fp64: out_t = fc(cell1(cell0(x_t))) with the frozen encoder state; output and
    all eight gradients. 65: first width past the 64-feature kernels; 97: one feature into a new 16-block; 156: a multiple of 4, not
    of 16; 160: full. B = 1, 5, 37, 130 leave a ragged clip tile, 16 is an exact one. 79, 80, 81: either side of the O <= 80 dispatch
    boundary; 66 and 159: next to 65 and 160 from the inside; each with and without the mask at B = 5 and 17."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    P, drop, up, ref, grads = _loop_reference(T, B, O, with_drop)
    D = {k: v.float().to(d).requires_grad_(True) for k, v in P.items()}
    out = ops.decoder_loop(D['k0'], D['c0'], D['k1'], D['c1'], D['w_ih0'], D['w_ih1'], D['w_fc'], D['b_fc'], T,
                           None if drop is None else drop.float().to(d))
    (out * up.float().to(d)).sum().backward()
    close(out, ref, 'out')
    for k in P:
        close(D[k].grad, grads[k], 'grad ' + k, rtol=2e-4)


@functools.lru_cache(maxsize=None)
def _stack_reference(T, B, O, with_drop):
    g = torch.Generator().manual_seed(T * 11 + B)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.3
    torch.manual_seed(T * 13 + O)
    dec64 = torch.nn.LSTM(O, H, num_layers=2).double()
    fc64 = torch.nn.Linear(H, O).double()
    hidden64, cell64 = rnd(2, B, H).requires_grad_(True), rnd(2, B, H).requires_grad_(True)
    drop = (torch.rand(T, B, H, generator=g) < 0.8).double() / 0.8 if with_drop else None
    up = torch.randn(B, T, O, generator=g, dtype=torch.float64)
    k0 = hidden64[0] @ dec64.weight_hh_l0.t() + dec64.bias_ih_l0 + dec64.bias_hh_l0
    k1 = hidden64[1] @ dec64.weight_hh_l1.t() + dec64.bias_ih_l1 + dec64.bias_hh_l1
    x, outs = torch.zeros(B, O, dtype=torch.float64), []
    for t in range(T):
        h0 = _cell(x @ dec64.weight_ih_l0.t() + k0, cell64[0])
        if drop is not None:
            h0 = h0 * drop[t]
        h1 = _cell(h0 @ dec64.weight_ih_l1.t() + k1, cell64[1])
        x = fc64(h1)
        outs.append(x)
    ref = torch.stack(outs, 1)                                        # (B,T,O)
    (ref * up).sum().backward()
    return dec64, fc64, hidden64, cell64, drop, up, ref.detach()


@gpu
@pytest.mark.parametrize('T,B,O,with_drop,sinks', [(1, 1, 156, False, False), (16, 37, 156, True, True), (5, 16, 78, False, False),
                                                    (16, 130, 65, True, False)])
def test_wide_decoder_stack_from_the_encoder_state(T, B, O, with_drop, sinks, rec_tile):
    """The decoder in one launch each way WITH its frame-invariant terms (k_l formed by the library, d k_l / d hidden_l in the
    backward, output and its gradient batch-first) against the per-frame formula in fp64: output, d hidden, d cell and all ten
    parameter gradients -- returned to autograd, or added into existing .grad tensors (= ones) inside ``grad_sinks``."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    dec64, fc64, hidden64, cell64, drop, up, ref = _stack_reference(T, B, O, with_drop)
    dec = torch.nn.LSTM(O, H, num_layers=2).to(d)
    fc = torch.nn.Linear(H, O).to(d)
    dec.load_state_dict({k: v.float() for k, v in dec64.state_dict().items()})
    fc.load_state_dict({k: v.float() for k, v in fc64.state_dict().items()})
    if sinks:
        for p_ in list(dec.parameters()) + list(fc.parameters()):
            p_.grad = torch.ones_like(p_)
    hidden, cellg = hidden64.detach().float().to(d).requires_grad_(True), cell64.detach().float().to(d).requires_grad_(True)
    with ops.grad_sinks(sinks):
        out = ops.decoder_stack(hidden, cellg, dec, fc, T, None if drop is None else drop.float().to(d))
        (out * up.float().to(d)).sum().backward()
    assert out.shape == (B, T, O)
    close(out, ref, 'out')
    close(hidden.grad, hidden64.grad, 'grad hidden', rtol=2e-4), close(cellg.grad, cell64.grad, 'grad cell', rtol=2e-4)
    for (name, p_), q in zip(list(dec.named_parameters()) + list(fc.named_parameters()), list(dec64.parameters()) + list(fc64.parameters())):
        close(p_.grad, q.grad + 1 if sinks else q.grad, 'grad ' + name, rtol=2e-4)


@gpu
@pytest.mark.parametrize('mode', ['frames_force', 'clip_force'])
def test_teacher_forcing_inside_the_wide_decoder_launch(mode, rec_tile, monkeypatch):
    """Teacher forcing at O = 156 (pose_changes): forced frames are replaced by their targets inside the one launch (output AND next
    input, no gradient through them). Against the per-step path of a twin (``_decoder_loop_fusable`` patched to False) with the same
    draws: output 2e-5, every parameter gradient 2e-4."""
    import copy
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2Seq
    from pedestrians_video_2_carla_amd.transforms.rotation_conversions import matrix_to_rotation_6d, rotation_6d_to_matrix
    d = dev()
    torch.manual_seed(17)
    model = Seq2Seq(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=MT.pose_changes, p_dropout=0.0,
                    teacher_mode=mode, teacher_force_ratio=0.4).to(d).train()
    model.rotation_output_format = 'rotation_6d'              # the raw (B,T,26,6) frames: forced ones equal their targets bit for bit
    twin = copy.deepcopy(model)
    B, T = 21, 12
    x, up = torch.randn(B, T, 26, 2, device=d), torch.randn(B, T, 26, 6, device=d)
    targets = {'pose_changes': rotation_6d_to_matrix(torch.randn(B, T, 26, 6, device=d))}
    assert model.decoder.output_size == 156 and model._decoder_loop_fusable(x)
    torch.manual_seed(5)
    y = model(x, targets)
    (y * up).sum().backward()
    monkeypatch.setattr(type(twin), '_decoder_loop_fusable', lambda self, x: False)
    torch.manual_seed(5)
    y_ref = twin(x, targets)
    (y_ref * up).sum().backward()
    monkeypatch.undo()
    forced = (y == matrix_to_rotation_6d(targets['pose_changes'])).all(-1).all(-1)           # (B,T) frames that are their targets
    assert 0.2 < float(forced.float().mean()) < 0.6
    if mode == 'clip_force':
        assert bool((forced.all(1) | (~forced).all(1)).all())
    close(y, y_ref, 'forced decoder output', rtol=2e-5)
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        close(p.grad, q.grad, 'grad ' + n, rtol=2e-4)


def _hash_mask(state, site, p, shape):
    """numpy restatement of csrc/p2c_rec_dev.h (drop_begin / drop_value) for the FORWARD of the step `state` is at."""
    import numpy as np
    M = 0xFFFFFFFF

    def mix(x):
        x = x.astype(np.uint64)
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7feb352d)) & np.uint64(M)
        x ^= x >> np.uint64(15)
        x = (x * np.uint64(0x846ca68b)) & np.uint64(M)
        x ^= x >> np.uint64(16)
        return x
    s0, s1, step = (int(v) & M for v in state[:3])
    k0 = int(mix(np.array([s0 ^ ((step * 0x9E3779B9) & M) ^ (((site + 1) * 0x632BE59B) & M)], dtype=np.uint64))[0])
    k1 = int(mix(np.array([(s1 + step + 0x85EBCA6B * (site + 1)) & M], dtype=np.uint64))[0])
    n = 1
    for v in shape:
        n *= v
    e = np.arange(n, dtype=np.uint64)
    h = mix((e * np.uint64(0x9E3779B1) + np.uint64(k0)) & np.uint64(M)) ^ np.uint64(k1)
    keep = h >= np.uint64(int(p * 4294967296.0))
    return torch.from_numpy((keep.astype(np.float32) * np.float32(1.0 / (1.0 - p))).reshape(shape))


@gpu
def test_wide_decoder_dropout_drawn_inside_the_kernels(rec_tile):
    """ops.decoder_stack at (T, B, O) = (16, 37, 156) with drop = (state, p, site): output and every gradient equal, bit for bit, the
    run that READS the same mask as a tensor (the numpy restatement of the hash); the state words advance {.., 0, 0} -> {.., 1, 1}
    and the next step draws another mask."""
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    T, B, O, p, site = 16, 37, 156, 0.2, 1
    torch.manual_seed(T * 3 + B)
    dec, fc = torch.nn.LSTM(O, H, num_layers=2).to(d), torch.nn.Linear(H, O).to(d)
    hidden0, cell0 = torch.randn(2, B, H, device=d) * 0.3, torch.randn(2, B, H, device=d) * 0.3
    up = torch.randn(B, T, O, device=d)
    state = ops.dropout_state(d)
    start = state.cpu().tolist()

    def run(drop):
        for q in list(dec.parameters()) + list(fc.parameters()):
            q.grad = None
        hidden, cell = hidden0.clone().requires_grad_(True), cell0.clone().requires_grad_(True)
        out = ops.decoder_stack(hidden, cell, dec, fc, T, drop)
        (out * up).sum().backward()
        return [out.detach().clone(), hidden.grad.clone(), cell.grad.clone()] + [q.grad.clone() for q in list(dec.parameters()) + list(fc.parameters())]
    got = run((state, p, site))
    torch.cuda.synchronize()
    assert state.cpu().tolist() == start[:2] + [1, 1]
    want = run(_hash_mask(start, site, p, (T, B, H)).to(d))
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), i
    again = run((state, p, site))                          # the next step of the stream: another mask
    assert not torch.equal(again[0], got[0])
    want2 = run(_hash_mask(start[:2] + [1, 1], site, p, (T, B, H)).to(d))
    assert torch.equal(again[0], want2[0])


@gpu
@pytest.mark.parametrize('O', [161, 0])
def test_widths_outside_the_wide_decoder_are_refused_with_nothing_launched(O, rec_tile):
    """p2c_decoder_fwd / p2c_decoder_bwd through the C ABI: O = 161 and O = 0 return P2C_E_SHAPE and the pre-filled outputs keep
    their values."""
    import ctypes
    from pedestrians_video_2_carla_amd import _lib, ops
    d = dev()
    lib = _lib.lib()
    T, B, Oa, E_SHAPE = 3, 5, max(O, 1), -2            # (include/p2c.h: P2C_E_SHAPE)
    f = dict(dtype=torch.float32, device=d)
    k0, k1, c0, c1 = torch.zeros(B, 4 * H, **f), torch.zeros(B, 4 * H, **f), torch.zeros(B, H, **f), torch.zeros(B, H, **f)
    w_ih0, w_ih1, w_fc, b_fc = torch.zeros(4 * H, Oa, **f), torch.zeros(4 * H, H, **f), torch.zeros(Oa, H, **f), torch.zeros(Oa, **f)
    out, gtot = torch.full((T, B, Oa), 7.0, **f), torch.full((T, B, Oa), 7.0, **f)
    acts0, acts1, gg0, gg1 = (torch.full((T, B, 4 * H), 7.0, **f) for _ in range(4))
    h0d, h1 = torch.full((T, B, H), 7.0, **f), torch.full((T, B, H), 7.0, **f)
    gc0, gc1, g_out = torch.full((B, H), 7.0, **f), torch.full((B, H), 7.0, **f), torch.zeros(T, B, Oa, **f)
    q = _lib.DecoderDesc()
    q.T, q.B, q.H, q.O = T, B, H, O
    q.k0, q.c0, q.k1, q.c1 = k0.data_ptr(), c0.data_ptr(), k1.data_ptr(), c1.data_ptr()
    q.w_ih0, q.w_ih1, q.w_fc, q.b_fc = w_ih0.data_ptr(), w_ih1.data_ptr(), w_fc.data_ptr(), b_fc.data_ptr()
    q.out, q.acts0, q.acts1, q.h0d, q.h1 = (t.data_ptr() for t in (out, acts0, acts1, h0d, h1))
    q.g_out, q.g_gates0, q.g_gates1, q.g_outtot = g_out.data_ptr(), gg0.data_ptr(), gg1.data_ptr(), gtot.data_ptr()
    q.g_c0, q.g_c1 = gc0.data_ptr(), gc1.data_ptr()
    with torch.cuda.device(d):
        assert lib.p2c_decoder_fwd(ctypes.byref(q), ops._stream()) == E_SHAPE
        assert lib.p2c_decoder_bwd(ctypes.byref(q), ops._stream()) == E_SHAPE
    torch.cuda.synchronize()
    for t in (out, gtot, acts0, acts1, gg0, gg1, h0d, h1, gc0, gc1):
        assert bool((t == 7.0).all())


@gpu
@pytest.mark.parametrize('T,B,O', [(3, 5, 156), (2, 21, 78)])
def test_wide_decoder_starts_from_a_given_first_input(T, B, O, rec_tile):
    """``p2c_decoder_desc.x0`` (B,O) through the C ABI: the first step reads x0 instead of <sos> = 0 (ops never sets it, so no other
    test reaches it at these widths). Output against the per-step formula in fp64 started from the same x0, 1e-4 of its max; and the
    run differs from the one that starts from zeros."""
    import ctypes
    from pedestrians_video_2_carla_amd import _lib, ops
    d = dev()
    lib = _lib.lib()
    g = torch.Generator().manual_seed(T * 5 + B)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.3
    P = {'k0': rnd(B, 4 * H), 'c0': rnd(B, H), 'k1': rnd(B, 4 * H), 'c1': rnd(B, H), 'w_ih0': rnd(4 * H, O), 'w_ih1': rnd(4 * H, H),
         'w_fc': rnd(O, H), 'b_fc': rnd(O), 'x0': rnd(B, O)}
    x, outs = P['x0'], []
    for t in range(T):
        h1 = _cell(_cell(x @ P['w_ih0'].t() + P['k0'], P['c0']) @ P['w_ih1'].t() + P['k1'], P['c1'])
        x = h1 @ P['w_fc'].t() + P['b_fc']
        outs.append(x)
    ref = torch.stack(outs)
    D = {k: v.float().to(d).contiguous() for k, v in P.items()}
    f = dict(dtype=torch.float32, device=d)
    got = {}
    for with_x0 in (True, False):
        out, acts0, acts1 = torch.empty(T, B, O, **f), torch.empty(T, B, 4 * H, **f), torch.empty(T, B, 4 * H, **f)
        h0d, h1d = torch.empty(T, B, H, **f), torch.empty(T, B, H, **f)
        q = _lib.DecoderDesc()
        q.T, q.B, q.H, q.O = T, B, H, O
        for n in ('k0', 'c0', 'k1', 'c1', 'w_ih0', 'w_ih1', 'w_fc', 'b_fc'):
            setattr(q, n, D[n].data_ptr())
        if with_x0:
            q.x0 = D['x0'].data_ptr()
        q.out, q.acts0, q.acts1, q.h0d, q.h1 = (t.data_ptr() for t in (out, acts0, acts1, h0d, h1d))
        with torch.cuda.device(d):
            assert lib.p2c_decoder_fwd(ctypes.byref(q), ops._stream()) == 0
        torch.cuda.synchronize()
        got[with_x0] = out
    close(got[True], ref, 'out from x0')
    assert not torch.equal(got[True][0], got[False][0])


def test_decoder_loop_supported_bounds_and_the_switch(monkeypatch):
    """Host logic: the widths the fused loop takes with P2C_DECODER_WIDE=1; hidden_size 128 stays out; P2C_DECODER_WIDE=0, or no
    setting, keeps O > 64 (only) on the per-step path."""
    from pedestrians_video_2_carla_amd import ops
    monkeypatch.delenv('P2C_DECODER_WIDE', raising=False)
    assert not ops.decoder_loop_supported(64, 2, 156) and ops.decoder_loop_supported(64, 2, 64)
    monkeypatch.setenv('P2C_DECODER_WIDE', '1')
    assert all(ops.decoder_loop_supported(64, 2, O) for O in (1, 52, 64, 65, 78, 156, 160))
    assert not any(ops.decoder_loop_supported(64, 2, O) for O in (0, 161, 234))
    assert not ops.decoder_loop_supported(128, 2, 156) and not ops.decoder_loop_supported(64, 3, 156)
    monkeypatch.setenv('P2C_DECODER_WIDE', '0')
    assert not ops.decoder_loop_supported(64, 2, 156) and not ops.decoder_loop_supported(64, 2, 65)
    assert ops.decoder_loop_supported(64, 2, 64) and ops.decoder_loop_supported(64, 2, 52)


def _counted(monkeypatch):
    """Count the entries of ops.decoder_stack and record the (T, B, I) of every ops.lstm_layer call."""
    from pedestrians_video_2_carla_amd import ops
    calls = {'decoder_stack': 0, 'lstm_layer': []}
    stack, layer = ops.decoder_stack, ops.lstm_layer

    def counted_stack(*a, **k):
        calls['decoder_stack'] += 1
        return stack(*a, **k)

    def counted_layer(x, *a, **k):
        calls['lstm_layer'].append(tuple(x.shape))
        return layer(x, *a, **k)
    monkeypatch.setattr(ops, 'decoder_stack', counted_stack)
    monkeypatch.setattr(ops, 'lstm_layer', counted_layer)
    return calls


def _bound(a32, a64):      # max(1e-4, 2 x the error fp32 on the CPU makes against fp64): tests/test_lstm_gpu.py's rule
    return max(1e-4, 2.0 * (a32.double() - a64).abs().max().item() / (a64.abs().max().item() + 1e-30))


@gpu
@pytest.mark.parametrize('cls,otype', [('Seq2SeqEmbeddings', 'pose_changes'), ('Seq2Seq', 'absolute_loc')])
def test_models_with_wide_outputs_take_the_fused_decoder_and_match_cpu(cls, otype, monkeypatch):
    """Seq2SeqEmbeddings(pose_changes: O = 156) and Seq2Seq(absolute_loc: O = 78), hidden_size 64, train mode, B = 5, T = 16, against
    the same module in fp64 on the CPU. The decoder is ONE ops.decoder_stack call per forward, no per-frame ops.lstm_layer call is
    made, nn.LSTM.forward is refused and no fall-back warning is raised."""
    import copy
    import warnings
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements import seq2seq
    d = dev()
    torch.manual_seed(5)
    model = getattr(seq2seq, cls)(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=MT[otype],
                                  p_dropout=0.0, hidden_size=64).train()
    cpu = copy.deepcopy(model).double()
    cpu32 = copy.deepcopy(model)
    x = torch.randn(5, 16, 26, 2)
    yr = cpu(x.double())
    up = torch.randn(*yr.shape)
    (yr * up.double()).sum().backward()
    y32 = cpu32(x)
    (y32 * up).sum().backward()
    gpu_model = model.to(d)
    calls = _counted(monkeypatch)

    def refuse(*a, **k):
        raise AssertionError('nn.LSTM.forward entered: the stack left the HIP path')
    monkeypatch.setattr(torch.nn.LSTM, 'forward', refuse)
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        y = gpu_model(x.to(d))
        (y * up.to(d)).sum().backward()
    monkeypatch.undo()
    assert calls['decoder_stack'] == 1, calls
    assert not [s for s in calls['lstm_layer'] if s[0] == 1], calls          # (a decoder frame is a T = 1 layer call)
    close(y, yr, 'model output', rtol=_bound(y32, yr))
    for (n, pg), (_, pc), (_, p32) in zip(gpu_model.named_parameters(), cpu.named_parameters(), cpu32.named_parameters()):
        assert pg.grad is not None, n
        close(pg.grad, pc.grad, 'grad ' + n, rtol=_bound(p32.grad, pc.grad))


FIXTURE = 'model_seq2seq_embeddings_h64_pose_changes'


def _fixture_models(golden, device):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqEmbeddings
    g, gg = golden(FIXTURE), golden(FIXTURE + '_grads')
    sd = {k[4:]: v for k, v in g.items() if k.startswith('sd__')}
    kw = dict(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=MT.pose_changes, hidden_size=64,
              single_joint_embeddings_size=8)
    ev, tr = Seq2SeqEmbeddings(**kw).eval(), Seq2SeqEmbeddings(p_dropout=0.0, **kw).train()
    ev.load_state_dict(sd), tr.load_state_dict(sd)
    assert sum(p.numel() for p in ev.parameters()) == int(g['n_params'])
    return g, gg, ev.to(device), tr.to(device)


def _check_fixture(g, gg, ev, tr, device):
    with torch.no_grad():
        out = ev(g['frames'].to(device))
    close(out, g['out'].double(), 'reference output', rtol=1e-4)
    (tr(g['frames'].to(device)) * gg['g_out'].to(device)).sum().backward()
    for n, p in tr.named_parameters():
        close(p.grad, gg['grad__' + n].double(), 'reference grad ' + n, rtol=2e-4)


def test_reference_fixture_of_the_hidden_64_pose_changes_model_on_the_cpu(golden):
    """tests/golden/model_seq2seq_embeddings_h64_pose_changes{,_grads}.npz = the REFERENCE's Seq2SeqEmbeddings(hidden_size=64,
    single_joint_embeddings_size=8, pose_changes) run by tests/golden/make_golden_decoder_wide.py: its state_dict in the module on the
    CPU, its frames in; output within 1e-4 and parameter gradients within 2e-4 (checks the fixture and the host code)."""
    _check_fixture(*_fixture_models(golden, torch.device('cpu')), torch.device('cpu'))


@gpu
def test_reference_run_of_the_hidden_64_pose_changes_model_on_the_fused_decoder(golden, monkeypatch):
    """The same fixture on the device: output within 1e-4, gradients within 2e-4, each forward's decoder ONE ops.decoder_stack call."""
    d = dev()
    g, gg, ev, tr = _fixture_models(golden, d)
    calls = _counted(monkeypatch)

    def refuse(*a, **k):
        raise AssertionError('nn.LSTM.forward entered: the stack left the HIP path')
    monkeypatch.setattr(torch.nn.LSTM, 'forward', refuse)
    _check_fixture(g, gg, ev, tr, d)
    monkeypatch.undo()
    assert calls['decoder_stack'] == 2 and not [s for s in calls['lstm_layer'] if s[0] == 1], calls


def _lifting_flow(B, T=16):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqEmbeddings
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(22742)
    dm = SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B, missing_joint_probabilities=0.1)
    model = Seq2SeqEmbeddings(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=MT.pose_changes,
                              p_dropout=0.0)
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform=dm.transform.name)
    return flow, dm


@gpu
def test_pose_lifting_step_with_the_wide_decoder_matches_the_cpu_twin(monkeypatch):
    """LitPoseLiftingFlow + Seq2SeqEmbeddings(pose_changes) + loc_2d_3d, B = 6, T = 16, under the flat trainer: loss and every
    parameter gradient (views of the flat gradient buffer) of one train step vs the model in fp64 on the CPU + the oracle pose head;
    tolerance max(1e-4, 2 x what fp32 on the CPU loses), the rule of test_cfg3_batch_size_parity_with_the_cpu_twin."""
    import copy
    from oracle import pose_head as O
    from pedestrians_video_2_carla_amd import ops
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow, dm = _lifting_flow(6)
    twins = {torch.float64: copy.deepcopy(flow.movements_model).double(), torch.float32: copy.deepcopy(flow.movements_model)}
    trainer = Trainer(device=d, use_graph=False).setup(flow, dm)
    calls = _counted(monkeypatch)
    batch = dm.generate_batch(d)
    frames, targets, meta = batch
    flow.train()
    with ops.grad_sinks(trainer._grad_sinks):
        flow.on_train_batch_start(batch, 0)
        out = flow.training_step(batch, 0)
        out['loss'].backward()
    monkeypatch.undo()
    assert calls['decoder_stack'] == 1, calls
    ref = {}
    for dt, twin in twins.items():
        twin.train()
        o = O.pose_head(twin(frames.to('cpu', dt)), 'pose_changes_6d', meta['skel_type'].cpu(),
                        gt2d=targets['projection_2d_transformed'].to('cpu', dt), gt3d=targets['absolute_pose_loc'].to('cpu', dt))
        o['loc_2d_3d'].backward()
        ref[dt] = (o['loc_2d_3d'].detach(), [p.grad for p in twin.parameters()])
    l64, g64 = ref[torch.float64]
    l32, g32 = ref[torch.float32]
    close(out['loss'], l64, 'loss', rtol=max(1e-4, 2 * abs(float(l32) - float(l64)) / abs(float(l64))))
    flat = trainer.flat.flat_grad
    for (n, p), q, q32 in zip(flow.movements_model.named_parameters(), g64, g32):
        lo = flat.data_ptr()
        assert lo <= p.grad.data_ptr() < lo + flat.numel() * 4, n          # the gradient IS a block of the flat buffer
        ref_err = (q32.double() - q).abs().max().item() / (q.abs().max().item() + 1e-30)
        close(p.grad, q, 'grad ' + n, rtol=max(1e-4, 2 * ref_err))


@gpu
def test_pose_lifting_steps_with_the_wide_decoder_replay_as_a_graph():
    """Three train steps of the same flow through Trainer(use_graph=True): the capture is kept (no fall-back to eager steps) and its
    losses equal three eager steps from the same start within 1e-6 relative."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    losses = {}
    for graph in (False, True):
        flow, dm = _lifting_flow(6)
        trainer = Trainer(device=d, use_graph=graph).setup(flow, dm)
        batch = dm.generate_batch(d)
        losses[graph] = torch.stack([trainer.train_step(flow, batch, i).detach().clone() for i in range(3)]).double().cpu()
        assert trainer.use_graph == graph, 'the captured step was dropped for eager steps'
    print('eager', losses[False].tolist(), 'graph', losses[True].tolist())
    assert bool(((losses[True] - losses[False]).abs() <= 1e-6 * losses[False].abs()).all()), (losses[False], losses[True])
