"""The SimpleTransformer movements model (modules/movements/transformers.py) on the host against the reference's own model:
fixtures model_simple_transformer_*.npz (tests/golden/make_golden_simple_transformer.py) hold a full state_dict with output and
gradients for a tiny 4-joint skeleton, and the seeded initial template layer, output and gradient sums for CARLA and BODY_25;
registry, CLI defaults and hparams as in the reference; the unused ``encoder_layer`` template stays out of the flat trainer's
buffers and unchanged through its steps."""
import argparse
import enum
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class TINY_SKELETON(enum.Enum):          # the fixture generator's 4-joint skeleton (d = 8)
    hips = 0
    neck = 1
    head = 2
    foot = 3


def load(*names):
    out = {}
    for f in names:
        d = np.load(os.path.join(ROOT, 'tests', 'golden', f + '.npz'))
        out.update({k: torch.from_numpy(d[k]) if d[k].dtype != object and d[k].dtype.kind != 'U' else d[k] for k in d.files})
    return out


def close(a, b, what, rtol):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


def nodes_of(name):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    return {'carla': (CARLA_SKELETON, 4, 22742), 'body25': (BODY_25_SKELETON, 5, 1234)}[name]


def tiny_model(g):
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    model = SimpleTransformer(input_nodes=TINY_SKELETON, n_heads=2, movements_output_type='pose_2d')
    sd = {k[4:]: v for k, v in g.items() if k.startswith('sd__')}
    assert set(model.state_dict().keys()) == set(sd.keys())
    model.load_state_dict(sd)
    assert sum(p.numel() for p in model.parameters()) == int(g['n_params'])
    return model


def test_registered_in_the_autoencoder_flow_only_and_not_the_default():
    from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqEmbeddings
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    assert LitAutoencoderFlow.get_available_models()['movements']['SimpleTransformer'] is SimpleTransformer
    assert 'SimpleTransformer' not in LitPoseLiftingFlow.get_available_models()['movements']
    assert LitAutoencoderFlow.get_default_models()['movements'] is Seq2SeqEmbeddings


def test_tiny_fixture_on_the_host():
    g = load('model_simple_transformer_tiny_0', 'model_simple_transformer_tiny_1', 'model_simple_transformer_tiny_grads')
    model = tiny_model(g).eval()
    out = model(g['frames'])
    close(out, g['out'], 'out', 1e-5)
    (out * g['g_out']).sum().backward()
    names = [n for n, _ in model.named_parameters()]
    for n, p in model.named_parameters():
        if n.startswith('encoder_layer.'):
            assert p.grad is None, n                      # the template is never in forward
        else:
            close(p.grad, g['grad__' + n], 'grad ' + n, 1e-5)
    assert {k[6:] for k in g if k.startswith('grad__')} == {n for n in names if not n.startswith('encoder_layer.')}
    # the six layers really differ (a layer-indexing bug could not pass)
    w = [model.encoder.layers[i].linear1.weight for i in range(6)]
    assert all(not torch.equal(w[0], w[i]) for i in range(1, 6))


@pytest.mark.parametrize('name', ['carla', 'body25'])
def test_seeded_initial_parameters_keys_and_fixture(name):
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    g = load('model_simple_transformer_' + name)
    nodes, heads, seed = nodes_of(name)
    torch.manual_seed(seed)
    model = SimpleTransformer(input_nodes=nodes, n_heads=heads, movements_output_type='pose_2d').eval()
    assert model.input_size == 2 * len(nodes)
    assert sorted(model.state_dict().keys()) == [str(k) for k in g['keys']]
    assert sum(p.numel() for p in model.parameters()) == int(g['n_params'])
    tpl = {k[5:]: v for k, v in g.items() if k.startswith('tpl__')}
    assert set(tpl) == set(model.encoder_layer.state_dict().keys())
    for k, v in tpl.items():
        assert torch.equal(model.encoder_layer.state_dict()[k], v), k
        for i in range(6):
            assert torch.equal(model.encoder.layers[i].state_dict()[k], v), (i, k)
    out = model(g['frames'])
    close(out, g['out'], 'out', 1e-5)
    (out * g['g_out']).sum().backward()
    for n, p in model.named_parameters():
        if p.grad is None:
            assert n.startswith('encoder_layer.') and ('gsum__' + n) not in g, n
            continue
        s, nrm = float(p.grad.double().sum()), float(p.grad.double().norm())
        assert abs(s - float(g['gsum__' + n])) <= 1e-4 * float(g['gnorm__' + n]) * p.numel() ** 0.5 + 1e-6, (n, s)
        assert abs(nrm - float(g['gnorm__' + n])) <= 1e-4 * float(g['gnorm__' + n]) + 1e-6, (n, nrm)


def test_n_heads_assert_kept():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    with pytest.raises(AssertionError, match='divisible by n_heads'):
        SimpleTransformer(input_nodes=CARLA_SKELETON, n_heads=5, movements_output_type='pose_2d')      # 52 % 5


def test_cli_defaults_and_hparams():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    parser = SimpleTransformer.add_model_specific_args(argparse.ArgumentParser())
    args = parser.parse_args([])
    assert args.n_heads == 4
    assert args.movements_output_type == MovementsModelOutputType.pose_2d
    assert args.movements_lr == 1e-3 and args.movements_weight_decay == 1e-2
    assert args.movements_scheduler_type == 'CosineAnnealingWarmRestarts'
    assert args.movements_enable_lr_scheduler is True and args.movements_scheduler_step_size == 30
    assert parser.parse_args(['--n_heads', '2']).n_heads == 2
    model = SimpleTransformer(input_nodes=CARLA_SKELETON, movements_output_type='pose_2d')
    assert model.output_type == MovementsModelOutputType.pose_2d
    assert 'n_heads' not in model.hparams                  # the reference adds no model-specific hparams


def _template(model):
    return [p.detach().clone() for p in model.encoder_layer.parameters()]


def _flat_steps(model, flat, opt, exchange=None, steps=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        flat.zero_grad()
        x = torch.randn(4, 5, 4, 2, generator=g)
        loss = (model(x) - x).pow(2).mean()
        loss.backward()
        if exchange is not None:
            exchange.all_reduce_gradients()
        opt.step()


def test_template_stays_out_of_the_flat_buffer_and_unchanged():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    from pedestrians_video_2_carla_amd.parallel.flat import FlatParameters
    torch.manual_seed(3)
    model = SimpleTransformer(input_nodes=TINY_SKELETON, n_heads=2, movements_output_type='pose_2d').train()
    before, layer0 = _template(model), model.encoder.layers[0].linear1.weight.detach().clone()
    flat = FlatParameters(model.parameters())
    n_tpl = sum(p.numel() for p in model.encoder_layer.parameters())
    assert flat.numel == sum(p.numel() for p in model.parameters()) - n_tpl
    assert len(flat.unused) == len(list(model.encoder_layer.parameters()))
    opt = flat.rebuild_optimizer(torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2))
    _flat_steps(model, flat, opt)
    assert all(torch.equal(a, b) for a, b in zip(before, _template(model)))
    assert not torch.equal(layer0, model.encoder.layers[0].linear1.weight)
    # every other model's flat buffer holds all of its trainable parameters, as before
    other = LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON)
    f2 = FlatParameters(other.parameters())
    assert f2.numel == sum(p.numel() for p in other.parameters()) and f2.unused == []


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _gloo_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    from pedestrians_video_2_carla_amd.modules.movements.transformers import SimpleTransformer
    from pedestrians_video_2_carla_amd.parallel.flat import FlatParameters, GradientExchange
    from pedestrians_video_2_carla_amd.trainer import init_distributed
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    init_distributed('gloo')
    torch.manual_seed(3)
    model = SimpleTransformer(input_nodes=TINY_SKELETON, n_heads=2, movements_output_type='pose_2d').train()
    if rank == 1:                       # different initial weights on purpose: the rank-0 broadcast must win, template included
        with torch.no_grad():
            for p in model.parameters():
                p.add_(1.0)
    flat = FlatParameters(model.parameters())
    exchange = GradientExchange(flat)
    exchange.broadcast_parameters(0)
    before = _template(model)
    opt = flat.rebuild_optimizer(torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-2))
    _flat_steps(model, flat, opt, exchange, seed=10 + rank)
    torch.save({'before': before, 'after': _template(model), 'flat': flat.flat_param.detach().clone()},
               os.path.join(out_dir, f'rank{rank}.pt'))
    dist.destroy_process_group()


def test_template_unchanged_under_two_rank_gloo(tmp_path):
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f'rank{r}.pt')) for r in (0, 1))
    for r in (r0, r1):
        assert all(torch.equal(a, b) for a, b in zip(r['before'], r['after']))
    assert all(torch.equal(a, b) for a, b in zip(r0['after'], r1['after']))
    assert torch.equal(r0['flat'], r1['flat'])


def test_gemm_descriptor_layout_matches_the_header(tmp_path):
    """``_lib.GemmDesc`` (ctypes) against ``p2c_gemm_desc`` compiled from include/p2c.h: same size, same offset for every field
    (the act 3 / 4 dropout fields appended last)."""
    import ctypes
    import subprocess
    from pedestrians_video_2_carla_amd._lib import GemmDesc
    fields = [f[0] for f in GemmDesc._fields_]
    assert fields[-3:] == ['drop_state', 'drop_p', 'drop_site']
    src = tmp_path / 'gemm_desc.c'
    body = '\n'.join(f'  printf("{f} %zu\\n", offsetof(p2c_gemm_desc, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(p2c_gemm_desc));\n' + body + '\n  return 0;\n}\n')
    exe = tmp_path / 'gemm_desc'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(out['sizeof']) == ctypes.sizeof(GemmDesc)
    for f in fields:
        assert int(out[f]) == getattr(GemmDesc, f).offset, f
