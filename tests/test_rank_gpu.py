"""GPU: K25 (``ops.rank_curves`` / ``ops.rank_scores``) and the classification flow's AUROC / ROCCurve / PRCurve on the device.
Every output of the ranking -- thresholds, tps, fps, sizes and the AUROC quotient -- is compared for EQUALITY with the numpy
restatement of tests/test_rank_metrics.py, in the LDS regime, in the radix-sort regime, and between the two. The one tolerance is
``p2c_rank_scores``' softmax / sigmoid: 1e-5 of the column's largest value, K24's bound for the same exp-sum-divide chain, plus
fp32's smallest normal number 2^-126 for columns that lie below fp32's range altogether."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_rank_metrics import KINDS, check_against_definitions, check_flow_metrics, make_scores, np_curves, same  # noqa: E402

REGIMES = ['lds', 'global']


def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


def rank(scores, targets, regime='auto'):
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    return ops.rank_curves(torch.as_tensor(scores).to(d), torch.as_tensor(targets).to(d), force_global=regime == 'global')


def assert_same_bits(a, b):
    assert a['n_points'] == b['n_points'] and a['n_pos'] == b['n_pos'] and a['n_valid'] == b['n_valid']
    assert torch.equal(a['auroc'].view(torch.int64), b['auroc'].view(torch.int64))
    for k in ('thresholds', 'tps', 'fps'):
        for x, y in zip(a[k], b[k]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k


# ------------------------------------------------------------------------------------------------------------- the regimes
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C', [1, 3, 32])
@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 257, 1000, 16384])
def test_lds_regime_against_the_definitions(N, C, kind):
    scores, targets = make_scores(N, C, kind, seed=7000 + 40 * N + C)
    check_against_definitions(rank(scores, targets), scores, targets)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C', [1, 3, 32])
@pytest.mark.parametrize('N', [1, 257, 4097, 16384])
def test_global_regime_gives_the_lds_regimes_bits(N, C, kind):
    scores, targets = make_scores(N, C, kind, seed=9000 + 40 * N + C)
    forced = rank(scores, targets, 'global')
    check_against_definitions(forced, scores, targets)
    assert_same_bits(forced, rank(scores, targets))


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('N', [16385, 70001])
def test_global_regime_unforced_above_the_lds_capacity(N, kind):
    scores, targets = make_scores(N, 2, kind, seed=N)
    check_against_definitions(rank(scores, targets), scores, targets)


# ----------------------------------------------------------------------------------------------------------------- hazards
@pytest.mark.parametrize('regime', REGIMES)
def test_all_scores_equal_is_one_point(regime):
    scores, targets = np.full((300, 3), 0.25, dtype=np.float32), np.arange(300) % 3
    got = rank(scores, targets, regime)
    check_against_definitions(got, scores, targets)
    assert got['n_points'] == [1, 1, 1] and got['tps'][0].tolist() == [100] and got['fps'][0].tolist() == [200]
    assert got['auroc'].tolist() == [0.5, 0.5, 0.5]


@pytest.mark.parametrize('regime', REGIMES)
def test_signed_zeros_form_one_group(regime):
    g = np.random.default_rng(5)
    scores = g.choice(np.array([-0.0, 0.0, 0.5, -0.5], dtype=np.float32), size=(500, 2))
    targets = g.integers(0, 2, 500)
    got = rank(scores, targets, regime)
    check_against_definitions(got, scores, targets)
    assert got['n_points'] == [3, 3] and got['thresholds'][0].tolist() == [0.5, 0.0, -0.5]
    assert not np.signbit(got['thresholds'][0].cpu().numpy()[1])


@pytest.mark.parametrize('regime', REGIMES)
def test_infinities_and_denormals_are_ordinary_values_next_to_the_padding(regime):
    """N = 1000 pads to 1024 in the LDS regime: kept -inf rows sort right in front of the padding and must not merge with it."""
    g = np.random.default_rng(6)
    pool = np.array([-np.inf, np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 0.0, 1.0, -1.0, 3.4e38, -3.4e38], dtype=np.float32)
    scores = g.choice(pool, size=(1000, 3))
    targets = g.integers(0, 3, 1000)
    got = rank(scores, targets, regime)
    check_against_definitions(got, scores, targets)
    assert got['n_valid'] == 1000 and got['n_points'] == [11, 11, 11]
    assert got['thresholds'][1][0].item() == math.inf and got['thresholds'][1][-1].item() == -math.inf
    assert (got['tps'][1][-1] + got['fps'][1][-1]).item() == 1000


@pytest.mark.parametrize('regime', REGIMES)
def test_nan_rows_and_bad_targets_are_dropped_everywhere(regime):
    scores, targets = make_scores(1000, 3, 'score_ties', seed=77)
    clean = rank(scores, targets, regime)
    g = np.random.default_rng(8)
    extra_s, extra_t = make_scores(200, 3, 'score_ties', seed=78)
    extra_s[60:100] = -np.inf                                        # dropped rows whose other scores are ordinary values
    extra_s[np.arange(80), g.integers(0, 3, 80)] = np.nan            # NaN in one column: dropped in every class
    extra_t[80:140], extra_t[140:] = -100, 3
    s, t = np.concatenate([scores, extra_s]), np.concatenate([targets, extra_t])
    perm = g.permutation(len(t))
    got = rank(s[perm], t[perm], regime)
    check_against_definitions(got, s[perm], t[perm])
    assert got['n_valid'] == 1000
    assert_same_bits(got, clean)                                     # no group's counts changed


@pytest.mark.parametrize('regime', REGIMES)
def test_a_class_without_positives(regime):
    scores, targets = make_scores(400, 3, 'continuous', seed=9)
    targets[targets == 2] = 0
    got = rank(scores, targets, regime)
    check_against_definitions(got, scores, targets)
    au = got['auroc'].tolist()
    assert math.isnan(au[2]) and not math.isnan(au[0]) and got['n_pos'][2] == 0 and int(got['tps'][2].abs().sum()) == 0
    assert got['n_points'][2] > 0


@pytest.mark.parametrize('regime', REGIMES)
def test_all_rows_dropped(regime):
    scores, targets = make_scores(100, 3, 'continuous', seed=10)
    scores[::2, 1] = np.nan
    targets[1::2] = -100
    got = rank(scores, targets, regime)
    assert got['n_valid'] == 0 and got['n_points'] == [0, 0, 0] and got['n_pos'] == [0, 0, 0]
    assert all(math.isnan(v) for v in got['auroc'].tolist()) and all(len(v) == 0 for v in got['thresholds'])


def test_no_rows_at_all():
    got = rank(np.zeros((0, 3), dtype=np.float32), np.zeros(0, dtype=np.int64))
    assert got['n_valid'] == 0 and got['n_points'] == [0, 0, 0] and all(math.isnan(v) for v in got['auroc'].tolist())


# ------------------------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize('regime,N', [('lds', 3000), ('global', 3000), ('auto', 20000)])
def test_two_runs_and_a_row_permutation_give_the_same_bits(regime, N):
    scores, targets = make_scores(N, 3, 'score_ties', seed=12)
    a, b = rank(scores, targets, regime), rank(scores, targets, regime)
    assert_same_bits(a, b)
    perm = np.random.default_rng(13).permutation(N)
    assert_same_bits(a, rank(scores[perm], targets[perm], regime))


# ---------------------------------------------------------------------------------------------------------- p2c_rank_scores
@pytest.mark.parametrize('scale', [1.0, 50.0])
@pytest.mark.parametrize('C', [2, 5, 32, 'binary'])
@pytest.mark.parametrize('B', [1, 7, 257])
def test_rank_scores_against_fp64(B, C, scale):
    from pedestrians_video_2_carla_amd import ops
    d = dev()
    binary = C == 'binary'
    cols = 1 if binary else C
    g = torch.Generator().manual_seed(B * 100 + cols)
    logits = torch.randn(B, cols, generator=g) * scale
    targets = torch.randint(0, 2 if binary else C, (B,), generator=g)
    targets[::3] = torch.tensor([-100, 2 if binary else C, -1])[torch.arange(len(targets[::3])) % 3]     # out of range
    cap, offset = B + 11, 5
    out_s = torch.full((cap, cols), -7.0, device=d)
    out_t = torch.full((cap,), -9, dtype=torch.int32, device=d)
    ops.rank_scores(logits.to(d), targets.to(d), out_s, out_t, offset, binary=binary)
    want = torch.sigmoid(logits.double()) if binary else torch.softmax(logits.double(), -1)
    got = out_s[offset:offset + B].cpu().double()
    err = (got - want).abs().max(dim=0).values
    print(f'rank_scores B={B} C={C} scale={scale}: max err {float(err.max()):.3e}')
    # 2^-126, fp32's smallest normal number: at scale 50 whole columns of a small batch lie below it (down to 1e-90), where fp32
    # holds at best a denormal and no relative bound can be met; K24's own test allows 1e-30 there
    assert bool((err <= 1e-5 * want.max(dim=0).values + 2.0 ** -126).all())
    K = 2 if binary else C
    assert out_t[offset:offset + B].cpu().tolist() == [t if 0 <= t < K else -1 for t in targets.tolist()]
    # rows outside [offset, offset + B) are untouched
    assert bool((out_s[:offset] == -7).all()) and bool((out_s[offset + B:] == -7).all())
    assert bool((out_t[:offset] == -9).all()) and bool((out_t[offset + B:] == -9).all())


# ------------------------------------------------------------------------------------------------------------------ the flow
def _flow(num_classes=3, **kw):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules import classification
    from pedestrians_video_2_carla_amd.modules.flow.classification import LitClassificationFlow
    torch.manual_seed(7)
    model = classification.GRU(input_nodes=CARLA_SKELETON, hidden_size=64, num_layers=2, num_classes=num_classes)
    return LitClassificationFlow(classification_model=model, classification_targets_key='cross', num_classes=num_classes, **kw)


def _validate():
    """Trainer.validate over three batches of unequal size, the epoch buffer started at 8 rows; the buffer's own fp32 scores are
    read back (by a wrapped compute_metrics, before the reset) for the restatement."""
    from pedestrians_video_2_carla_amd.trainer import Trainer
    d = dev()
    flow = _flow()
    flow.rank_initial_capacity = 8
    g = torch.Generator().manual_seed(4)
    batches = [(torch.randn(B, 6, 26, 2, generator=g).to(d), {'cross': torch.randint(0, 3, (B, 1), generator=g).to(d)}, {})
               for B in (5, 33, 23)]
    trainer = Trainer(device=d, use_graph=False).setup(flow, None)
    seen = {}
    compute = flow.compute_metrics

    def wrapped(*a, **kw):
        seen['rows'], seen['capacity'] = flow._rank_rows, flow._rank_targets.shape[0]
        seen['scores'] = flow._rank_scores[:flow._rank_rows].cpu().numpy().copy()
        seen['targets'] = flow._rank_targets[:flow._rank_rows].cpu().numpy().copy()
        return compute(*a, **kw)
    flow.compute_metrics = wrapped
    got = trainer.validate(flow, batches)
    return flow, got, seen, torch.cat([b[1]['cross'][:, 0] for b in batches]).cpu().numpy()


def test_flow_on_the_device_reports_the_metrics_of_its_own_scores():
    flow, got, seen, targets = _validate()
    assert seen['rows'] == 61 and seen['capacity'] == 64 and np.array_equal(seen['targets'], targets)     # 8 -> 64: it grew
    assert flow._rank_scores.is_cuda and not any(k.startswith('_rank') for k in flow.state_dict())
    want, n_valid = np_curves(seen['scores'], seen['targets'])
    assert n_valid == 61
    check_flow_metrics(got, want)
    assert flow._rank_rows == 0 and 'AUROC' not in flow.compute_metrics()                                  # empty afterwards


def test_flow_framework_arm_gives_the_same_values(monkeypatch):
    _, kernel, seen_k, _ = _validate()
    monkeypatch.setenv('P2C_RANK_FRAMEWORK', '1')
    _, tensor, seen_t, _ = _validate()
    assert np.array_equal(seen_k['scores'], seen_t['scores'])            # the scores are p2c_rank_scores' on both arms
    assert same(kernel['AUROC'], tensor['AUROC'])
    for key in ('ROCCurve', 'PRCurve'):
        for part in range(3):
            for c in range(3):
                assert same(kernel[key][part][c], tensor[key][part][c]), (key, part, c)


def test_framework_arm_of_rank_curves_gives_the_kernels_integers(monkeypatch):
    scores, targets = make_scores(5000, 5, 'score_ties', seed=3)
    kernel = rank(scores, targets)
    monkeypatch.setenv('P2C_RANK_FRAMEWORK', '1')
    tensor = rank(scores, targets)
    check_against_definitions(tensor, scores, targets)
    assert_same_bits(kernel, tensor)
