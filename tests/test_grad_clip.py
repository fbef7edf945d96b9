"""Gradient clipping (K29), host side: the Trainer's gradient_clip_val / gradient_clip_algorithm arguments, the tensor path a
trainer on the host takes, the C ABI of p2c_clip_desc and the argument checks of p2c_adamw_step_clipped (which fail before
any launch). CPU only; the kernels themselves are tested in tests/test_grad_clip_gpu.py."""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TinyFlow(torch.nn.Module):
    """The smallest thing Trainer.setup / train_step accept: one plugin, one optimizer, a loss whose gradient norm is far above
    the clips used below."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.net = torch.nn.Sequential(torch.nn.Linear(6, 9), torch.nn.Tanh(), torch.nn.Linear(9, 3))

    def configure_optimizers(self):
        return [{'optimizer': torch.optim.AdamW(self.parameters(), lr=1e-2, weight_decay=0.05)}]

    def on_train_batch_start(self, batch, batch_idx):
        pass

    def training_step(self, batch, batch_idx):
        x, y, _ = batch
        return {'loss': 40.0 * (self.net(x) - y).pow(2).mean()}


def _batches(n=4):
    g = torch.Generator().manual_seed(11)
    return [(torch.randn(16, 6, generator=g), torch.randn(16, 3, generator=g), {}) for _ in range(n)]


# ---- 6: host logic ---------------------------------------------------------------------------------------------------------
def test_bad_algorithm_and_bad_value_raise_in_the_constructor():
    from pedestrians_video_2_carla_amd.trainer import Trainer
    with pytest.raises(ValueError):
        Trainer(gradient_clip_val=1.0, gradient_clip_algorithm='l1')
    with pytest.raises(ValueError):
        Trainer(gradient_clip_algorithm='Norm')                  # also without a value: a typo does not wait for the day it matters
    with pytest.raises(ValueError):
        Trainer(gradient_clip_val=-1.0)
    t = Trainer(gradient_clip_val=0.5)
    assert t.gradient_clip_val == 0.5 and t.gradient_clip_algorithm == 'norm'        # Lightning's default algorithm
    assert Trainer(gradient_clip_val=2, gradient_clip_algorithm='value').gradient_clip_algorithm == 'value'


@pytest.mark.parametrize('off', [None, 0, 0.0])
def test_none_and_zero_mean_off(off):
    """No clip: set_clip is never called on the optimizer, nothing is clipped on the tensor path either, and the step is the
    unclipped step."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    calls = []

    class Opt(torch.optim.AdamW):
        def set_clip(self, *a, **k):
            calls.append((a, k))

    class Flow(TinyFlow):
        def configure_optimizers(self):
            return [{'optimizer': Opt(self.parameters(), lr=1e-2, weight_decay=0.05)}]

    flow, plain = Flow(), Flow()
    t = Trainer(gradient_clip_val=off).setup(flow, None)
    p = Trainer().setup(plain, None)
    assert t.gradient_clip_val is None and not t._clip_in_kernel
    for i, b in enumerate(_batches(2)):
        t.train_step(flow, b, i), p.train_step(plain, b, i)
    assert calls == [] and t.last_grad_norm is None
    assert torch.equal(t.flat.flat_param.data, p.flat.flat_param.data)
    # ... and with a clip, an optimizer that can clip in its own launch is told to (P2C_CLIP_FRAMEWORK unset)
    Trainer(gradient_clip_val=0.25, gradient_clip_algorithm='value').setup(Flow(), None)
    assert calls == [((0.25, 'value'), {})]


def test_clip_framework_switch_keeps_the_tensor_path(monkeypatch):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    calls = []

    class Opt(torch.optim.AdamW):
        def set_clip(self, *a, **k):
            calls.append(a)

    class Flow(TinyFlow):
        def configure_optimizers(self):
            return [{'optimizer': Opt(self.parameters(), lr=1e-2)}]

    monkeypatch.setenv('P2C_CLIP_FRAMEWORK', '1')
    t = Trainer(gradient_clip_val=0.5).setup(Flow(), None)
    assert calls == [] and not t._clip_in_kernel


# ---- 7: the trainer on the host takes the tensor path and equals a hand-written torch loop ---------------------------------------
@pytest.mark.parametrize('flatten', [True, False])
@pytest.mark.parametrize('algorithm,clip', [('norm', 0.5), ('value', 0.01)])
def test_cpu_trainer_equals_a_hand_written_loop(flatten, algorithm, clip):
    from pedestrians_video_2_carla_amd.parallel.flat import FlatParameters
    from pedestrians_video_2_carla_amd.trainer import Trainer
    flow, hand = TinyFlow(), TinyFlow()
    assert all(torch.equal(a, b) for a, b in zip(flow.parameters(), hand.parameters()))
    trainer = Trainer(gradient_clip_val=clip, gradient_clip_algorithm=algorithm, flatten=flatten).setup(flow, None)
    assert not trainer._clip_in_kernel and not trainer._opt_in_backward
    if flatten:                                   # the trainer's optimizer steps ONE flat tensor: so does the loop
        flat = FlatParameters(hand.parameters())
        params = [flat.flat_param]
    else:
        params = list(hand.parameters())
    opt = torch.optim.AdamW(params, lr=1e-2, weight_decay=0.05)
    for i, batch in enumerate(_batches()):
        trainer.train_step(flow, batch, i)
        if flatten:
            flat.zero_grad()
        else:
            opt.zero_grad(set_to_none=True)
        hand.training_step(batch, i)['loss'].backward()
        if algorithm == 'norm':
            norm = torch.nn.utils.clip_grad_norm_(params, clip)
            assert float(norm) > clip                                              # it really clipped
            assert torch.equal(trainer.last_grad_norm, norm)
        else:
            assert max(float(p.grad.abs().max()) for p in params) > clip
            torch.nn.utils.clip_grad_value_(params, clip)
            assert trainer.last_grad_norm is None
        opt.step()
    for a, b in zip(flow.parameters(), hand.parameters()):
        assert torch.equal(a, b)
    unclipped = TinyFlow()                        # and the clip changed the run
    tu = Trainer(flatten=flatten).setup(unclipped, None)
    for i, batch in enumerate(_batches()):
        tu.train_step(unclipped, batch, i)
    assert not all(torch.equal(a, b) for a, b in zip(flow.parameters(), unclipped.parameters()))


# ---- 8: ABI --------------------------------------------------------------------------------------------------------------
def test_clip_descriptor_layout_matches_the_header(tmp_path):
    """ctypes mirror vs the C struct (the method of tests/test_host_logic.py): same size, same offsets, same enum values."""
    from pedestrians_video_2_carla_amd import _lib
    fields = [f[0] for f in _lib.ClipDesc._fields_]
    src = tmp_path / 'clip.c'
    body = '\n'.join(f'  printf("{f} %zu\\n", offsetof(p2c_clip_desc, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(p2c_clip_desc));\n'
                   '  printf("NORM %d\\n  VALUE %d\\n", (int)P2C_CLIP_NORM, (int)P2C_CLIP_VALUE);\n' + body + '\n  return 0;\n}\n')
    exe = tmp_path / 'clip'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.strip().splitlines())
    assert int(out['sizeof']) == ctypes.sizeof(_lib.ClipDesc)
    for f in fields:
        assert int(out[f]) == getattr(_lib.ClipDesc, f).offset, f
    assert (int(out['NORM']), int(out['VALUE'])) == (_lib.P2C_CLIP_NORM, _lib.P2C_CLIP_VALUE) == (1, 2)


def _lib_handle():
    from pedestrians_video_2_carla_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_both_symbols_are_in_the_built_library_and_the_partials_count_is_a_function_of_n():
    _lib, lib = _lib_handle()
    assert {'p2c_grad_clip_partials', 'p2c_adamw_step_clipped'} <= set(_lib.SYMBOLS)
    assert lib.p2c_adamw_step_clipped is not None
    f = lib.p2c_grad_clip_partials
    assert [f(n) for n in (-1, 0, 1, 3, 4, 1024, 1025, 4099, 70001)] == [0, 0, 1, 1, 1, 1, 2, 5, 69]
    assert f(1024 * 1024) == 1024 == f(1 << 40) and f(1024 * 1023 + 1) == 1024 and f(1024 * 1023) == 1023     # capped at 1024


# ---- 9: error codes (all of them returned before any launch: no device needed, the pointers are never followed) -------------------
def _descs(_lib, n=64):
    d = _lib.AdamWDesc()
    d.n = n
    for i, f in enumerate(('param', 'grad', 'exp_avg', 'exp_avg_sq', 'step', 'ticket', 'hyper')):
        setattr(d, f, 0x10000 * (i + 1))
    d.adamw = 1
    c = _lib.ClipDesc()
    c.mode, c.bound, c.partials, c.total_norm = _lib.P2C_CLIP_NORM, 1.0, 0x100000, 0x200000
    return d, c


def test_clipped_step_returns_its_documented_error_codes():
    _lib, lib = _lib_handle()
    E_NULL, E_SHAPE, E_ENUM = -1, -2, -3
    call = lambda d, c: lib.p2c_adamw_step_clipped(ctypes.byref(d), ctypes.byref(c), None)   # noqa: E731
    d, c = _descs(_lib)
    assert lib.p2c_adamw_step_clipped(None, ctypes.byref(c), None) == E_NULL
    assert lib.p2c_adamw_step_clipped(ctypes.byref(d), None, None) == E_NULL
    for mode in (0, 3, -1):
        d, c = _descs(_lib)
        c.mode = mode
        assert call(d, c) == E_ENUM, mode
    for bound in (0.0, -1.0, float('inf'), float('-inf'), float('nan')):
        for mode in (_lib.P2C_CLIP_NORM, _lib.P2C_CLIP_VALUE):
            d, c = _descs(_lib)
            c.mode, c.bound = mode, bound
            assert call(d, c) == E_SHAPE, (mode, bound)
    for missing in ('partials', 'total_norm'):
        d, c = _descs(_lib)
        setattr(c, missing, None)
        assert call(d, c) == E_NULL, missing
    # the checks of p2c_adamw_step come first and are the same
    for f in ('param', 'grad', 'exp_avg', 'exp_avg_sq', 'step', 'ticket', 'hyper'):
        d, c = _descs(_lib)
        setattr(d, f, None)
        assert call(d, c) == E_NULL, f
    d, c = _descs(_lib)
    d.scatter_idx = 0x300000                      # an index without a destination
    assert call(d, c) == E_NULL
    d, c = _descs(_lib, n=-1)
    assert call(d, c) == E_SHAPE
    d, c = _descs(_lib)
    d.grad = 0x20004                              # flat buffers are 16-byte aligned
    assert call(d, c) == E_SHAPE
    # n == 0: nothing to do, nothing launched -- in both modes, VALUE without the NORM pointers
    d, c = _descs(_lib, n=0)
    assert call(d, c) == 0
    c.mode, c.partials, c.total_norm = _lib.P2C_CLIP_VALUE, None, None
    assert call(d, c) == 0
    d, c = _descs(_lib, n=0)
    c.mode = 7                                    # ... but a bad descriptor is still a bad descriptor
    assert call(d, c) == E_ENUM
