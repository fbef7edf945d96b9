"""The LSTM movements model (modules/movements/lstm.py) on the host against the reference's own model: fixtures
model_lstm_*.npz (tests/golden/make_golden_lstm.py) hold its state_dict, output and parameter gradients; registry and CLI
defaults as in the reference."""
import argparse
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {
    'model_lstm_pose_changes': dict(nodes='CARLA_SKELETON', kw={}),
    'model_lstm_h191_pose_2d': dict(nodes='CARLA_SKELETON', kw=dict(hidden_size=191, num_layers=1, movements_output_type='pose_2d')),
    'model_lstm_body25_emb': dict(nodes='BODY_25_SKELETON', kw=dict(hidden_size=100, num_layers=3, embeddings_size=32,
                                                                   movements_output_type='pose_2d')),
}


def load_fixture(name):
    out = {}
    for f in (name, name + '_grads'):
        d = np.load(os.path.join(ROOT, 'tests', 'golden', f + '.npz'))
        out.update({k: torch.from_numpy(d[k]) for k in d.files})
    return out


def build_model(name, g):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.data.openpose.skeleton import BODY_25_SKELETON
    from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM
    spec = FIXTURES[name]
    nodes = {'CARLA_SKELETON': CARLA_SKELETON, 'BODY_25_SKELETON': BODY_25_SKELETON}[spec['nodes']]
    model = LSTM(input_nodes=nodes, **spec['kw'])
    sd = {k[4:]: v for k, v in g.items() if k.startswith('sd__')}
    assert set(model.state_dict().keys()) == set(sd.keys())
    model.load_state_dict(sd)
    assert sum(p.numel() for p in model.parameters()) == int(g['n_params'])
    return model


def close(a, b, what, rtol):
    a, b = a.detach().double(), b.detach().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= rtol * scale + 1e-30, f'{what}: {err:.3e} vs scale {scale:.3e}'


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_reference_fixture_on_the_host(name):
    g = load_fixture(name)
    model = build_model(name, g).train()
    out = model(g['frames'])
    close(out, g['out'], 'out', 1e-5)
    (out * g['g_out']).sum().backward()
    for n, p in model.named_parameters():
        close(p.grad, g['grad__' + n], 'grad ' + n, 1e-5)


def test_registered_in_both_flows_but_not_the_default():
    from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements import LSTM
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqEmbeddings
    assert LitPoseLiftingFlow.get_available_models()['movements']['LSTM'] is LSTM
    assert LitAutoencoderFlow.get_available_models()['movements']['LSTM'] is LSTM
    assert LitPoseLiftingFlow.get_default_models()['movements'] is LinearAE
    assert LitAutoencoderFlow.get_default_models()['movements'] is Seq2SeqEmbeddings


def test_cli_defaults_and_hparams_match_the_reference():
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements.lstm import LSTM
    args = LSTM.add_model_specific_args(argparse.ArgumentParser()).parse_args([])
    assert args.hidden_size == 64 and args.num_layers == 2 and args.embeddings_size is None
    assert args.movements_output_type == MT.pose_changes
    args = LSTM.add_model_specific_args(argparse.ArgumentParser()).parse_args(
        ['--hidden_size', '191', '--num_layers', '4', '--embeddings_size', '32', '--movements_output_type', 'pose_2d'])
    assert (args.hidden_size, args.num_layers, args.embeddings_size, args.movements_output_type) == (191, 4, 32, MT.pose_2d)
    m = LSTM(input_nodes=CARLA_SKELETON, hidden_size=191, num_layers=4, embeddings_size=32)
    assert {k: m._hparams[k] for k in ('hidden_size', 'num_layers', 'embeddings_size')} == dict(hidden_size=191, num_layers=4,
                                                                                                 embeddings_size=32)
    assert isinstance(LSTM(input_nodes=CARLA_SKELETON).linear_1, torch.nn.Identity)
    assert m.lstm_1.batch_first and m.lstm_1.dropout == 0 and not m.lstm_1.bidirectional
