"""AUROC, ROCCurve and PRCurve of the classification flow on the host: the tensor-op path of ``ops.rank_curves`` against a plain
numpy restatement of the definitions (stable argsort, group ends, cumulative sums, Python integers for the AUROC sum) and against
scikit-learn, the flow's three keys, two gloo ranks with unequal shares, and the C ABI of K25. Counts, thresholds and the AUROC
quotient are compared for equality; the one bound is scikit-learn's own fp64 trapezoid (one rounding per point: n_points 2^-52)."""
import ctypes
import math
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

try:
    from sklearn import metrics as skm
    from sklearn.metrics._ranking import _binary_clf_curve
except ImportError:                                                       # the numpy restatement still holds every assertion
    skm = _binary_clf_curve = None


# ---------------------------------------------------------------------------------------------------------- the definitions
def np_curves(scores, targets):
    """The definitions, class by class: scores (N, C) float, targets (N) int -> list of dicts per class + n_valid."""
    scores = np.asarray(scores)
    if scores.ndim == 1:
        scores = scores[:, None]
    targets = np.asarray(targets).reshape(-1).astype(np.int64)
    N, C = scores.shape
    K = 2 if C == 1 else C
    keep = (targets >= 0) & (targets < K) & ~np.isnan(scores).any(axis=1)
    scores, targets = scores[keep], targets[keep]
    out = []
    for c in range(C):
        s = scores[:, c]
        pos = (targets == (1 if C == 1 else c)).astype(np.int64)
        order = np.argsort(-s, kind='stable')
        s, pos = s[order], pos[order]
        ends = np.ones(len(s), dtype=bool)
        ends[:-1] = s[1:] != s[:-1]
        idx = np.nonzero(ends)[0]
        tps = np.cumsum(pos)[idx]
        fps = idx + 1 - tps
        num, pt, pf = 0, 0, 0
        for t, f in zip(tps.tolist(), fps.tolist()):
            num += (f - pf) * (t + pt)
            pt, pf = t, f
        P, Q = (int(tps[-1]), int(fps[-1])) if len(idx) else (0, 0)
        out.append(dict(thresholds=s[idx], tps=tps, fps=fps, num=num, den=2 * P * Q, P=P, Q=Q,
                        auroc=num / (2 * P * Q) if P and Q else math.nan))
    return out, int(keep.sum())


def np_roc(d):
    th, tps, fps = d['thresholds'].astype(np.float64), d['tps'].astype(np.float64), d['fps'].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.r_[0.0, fps / d['Q']], np.r_[0.0, tps / d['P']], np.r_[th[0] + 1.0, th]


def np_pr(d):
    th, tps, fps = d['thresholds'].astype(np.float64), d['tps'].astype(np.float64), d['fps'].astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        precision, recall = tps / (tps + fps), tps / d['P']
    cut = int(np.nonzero(d['tps'] == d['P'])[0][0]) + 1
    return np.r_[precision[:cut][::-1], 1.0], np.r_[recall[:cut][::-1], 0.0], th[:cut][::-1]


def same(a, b):
    """Equal element for element, NaN equal to NaN."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | ((a != a) & (b != b))))


def check_against_definitions(got, scores, targets):
    """``ops.rank_curves``' dict against the numpy restatement: everything equal. Returns the restatement."""
    want, n_valid = np_curves(scores, targets)
    assert got['n_valid'] == n_valid
    au = got['auroc'].cpu().numpy()
    assert au.dtype == np.float64 and len(au) == len(want)
    for c, w in enumerate(want):
        th, tps, fps = (got[k][c].cpu().numpy() for k in ('thresholds', 'tps', 'fps'))
        assert tps.dtype == np.int32 and fps.dtype == np.int32
        assert got['n_points'][c] == len(w['thresholds']) == len(th) and got['n_pos'][c] == w['P']
        assert np.array_equal(th, w['thresholds']), c
        assert np.array_equal(tps, w['tps']) and np.array_equal(fps, w['fps']), c
        assert same(au[c], w['auroc']), (c, au[c], w['num'], w['den'])
    return want


def make_scores(N, C, kind, seed):
    g = np.random.default_rng(seed)
    logits = g.standard_normal((N, C)).astype(np.float32) * 2 if kind != 'ties' else g.integers(0, 8, (N, C)).astype(np.float32) * 0.5
    x = torch.from_numpy(logits)
    scores = torch.sigmoid(x) if C == 1 else torch.softmax(x, dim=-1)
    if kind == 'score_ties':        # softmax over many classes leaves 8-level logits almost distinct: 8 levels of the SCORE tie at any C
        scores = torch.floor(scores * 8) / 8
    targets = g.integers(0, 2 if C == 1 else C, N)
    return scores.numpy(), targets


# ---------------------------------------------------------------------------------------------------- ops.rank_curves, host
KINDS = ['continuous', 'ties', 'score_ties']


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C', [1, 2, 3, 32])
@pytest.mark.parametrize('N', [1, 2, 97, 5000])
def test_host_rank_curves_against_the_definitions_and_sklearn(N, C, kind):
    from pedestrians_video_2_carla_amd import ops
    scores, targets = make_scores(N, C, kind, seed=1000 * N + C)
    got = ops.rank_curves(torch.from_numpy(scores), torch.from_numpy(targets))
    want = check_against_definitions(got, scores, targets)
    if N >= 97 and (kind == 'score_ties' or (kind == 'ties' and C <= 3)):
        assert max(got['n_points']) < N                                   # the ties are there
    if skm is None:
        return
    for c, w in enumerate(want):
        y = (targets == (1 if C == 1 else c)).astype(np.int64)
        fps, tps, th = _binary_clf_curve(y, scores[:, c], pos_label=1)[:3]
        assert np.array_equal(th, w['thresholds']) and np.array_equal(tps, w['tps']) and np.array_equal(fps, w['fps'])
        if 0 < y.sum() < N:
            ref = skm.roc_auc_score(y, scores[:, c])
            assert abs(float(got['auroc'][c]) - ref) <= len(th) * 2.0 ** -52, (c, float(got['auroc'][c]), ref)


def test_host_rank_curves_drops_rows_and_groups_signed_zeros():
    from pedestrians_video_2_carla_amd import ops
    nan, inf = float('nan'), float('inf')
    scores = np.array([[0.0, 1.0], [-0.0, 2.0], [nan, 0.5], [0.5, -inf], [0.5, inf], [0.25, 1e-42], [0.1, 0.2], [0.3, 0.4]],
                      dtype=np.float32)
    targets = np.array([0, 1, 0, 1, 0, 1, -100, 2])
    got = ops.rank_curves(torch.from_numpy(scores), torch.from_numpy(targets))
    check_against_definitions(got, scores, targets)
    assert got['n_valid'] == 5 and got['n_points'] == [3, 5]
    assert got['thresholds'][0].tolist() == [0.5, 0.25, 0.0] and got['tps'][0].tolist() == [1, 1, 2]


# ----------------------------------------------------------------------------------------------------------------- the flow
def _flow(num_classes=3, binary=False, **kw):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules import classification
    from pedestrians_video_2_carla_amd.modules.flow.classification import LitClassificationFlow
    from pedestrians_video_2_carla_amd.modules.flow.output_types import ClassificationModelOutputType
    base = classification.GRU
    if binary:
        class Binary(base):
            output_type = property(lambda self: ClassificationModelOutputType.binary)
        base = Binary
    torch.manual_seed(3)
    model = base(input_nodes=CARLA_SKELETON, hidden_size=20, num_layers=1, num_classes=1 if binary else num_classes)
    return LitClassificationFlow(classification_model=model, classification_targets_key='cross', num_classes=num_classes, **kw)


def _batches(sizes, C, seed=11, T=5):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, T, 26, 2, generator=g), {'cross': torch.randint(0, C, (B, 1), generator=g)}, {}) for B in sizes]


def check_flow_metrics(got, want, binary=False):
    """The flow's three keys against the definitions' per-class dicts (counts, rates and AUROC equal)."""
    au = [w['auroc'] for w in want]
    assert isinstance(got['AUROC'], float) and same(got['AUROC'], au[0] if binary else float(np.mean(au)))
    for key, fn in (('ROCCurve', np_roc), ('PRCurve', np_pr)):
        curve = got[key]
        assert isinstance(curve, tuple) and len(curve) == 3
        for c, w in enumerate(want):
            for part, ref in zip(curve, fn(w)):
                arr = part if binary else part[c]
                assert isinstance(arr, np.ndarray) and arr.dtype == np.float64
                assert same(arr, ref), (key, c)
        if not binary:
            assert all(isinstance(part, list) and len(part) == len(want) for part in curve)


def test_flow_reports_auroc_and_curves_of_the_evaluation_epoch():
    flow = _flow()
    assert flow.get_metrics()['AUROC'] == 'macro' and {'ROCCurve', 'PRCurve'} <= set(flow.get_metrics())
    b = _batches([13, 9, 11], 3)
    logits = [flow.validation_step(b[0], 0)['preds']['cross_logits'], flow.validation_step(b[1], 1)['preds']['cross_logits'],
              flow.test_step(b[2], 0)['preds']['cross_logits']]
    logits = torch.cat(logits)
    targets = torch.cat([x[1]['cross'][:, 0] for x in b]).numpy()
    assert not any(k.startswith('_rank') for k in flow.state_dict())
    s64, s32 = torch.softmax(logits.double(), -1).numpy(), flow._rank_scores[:33].numpy().copy()
    for c in range(3):      # no two fp32 scores of a class collide, and fp32 ranks them as fp64 does
        assert len(np.unique(s32[:, c])) == 33 and np.array_equal(np.argsort(-s32[:, c]), np.argsort(-s64[:, c]))
    assert np.array_equal(flow._rank_targets[:33].numpy(), targets)
    got = flow.compute_metrics()
    assert {'AUROC', 'ROCCurve', 'PRCurve', 'ConfusionMatrix', 'Accuracy'} <= set(got)
    # the definitions on the fp64 softmax of the returned logits: every count, rate and the AUROC are equal; the thresholds are
    # the fp32 scores (K24's bound for the exp-sum-divide chain: 1e-5 of the column's largest)
    want64, _ = np_curves(s64, targets)
    want32, _ = np_curves(s32, targets)
    for a, bb in zip(want64, want32):
        assert np.array_equal(a['tps'], bb['tps']) and np.array_equal(a['fps'], bb['fps']) and a['num'] == bb['num']
        assert np.abs(a['thresholds'] - bb['thresholds']).max() <= 1e-5 * s64.max()
    check_flow_metrics(got, want32)
    if skm is not None:
        for c in range(3):
            y = (targets == c).astype(int)
            fpr, tpr, th = skm.roc_curve(y, s32[:, c], drop_intermediate=False)
            assert same(got['ROCCurve'][0][c], fpr) and same(got['ROCCurve'][1][c], tpr) and same(got['ROCCurve'][2][c][1:], th[1:])
            assert abs(want32[c]['auroc'] - skm.roc_auc_score(y, s32[:, c])) <= 33 * 2.0 ** -52
            # scikit-learn keeps the points past full recall: the torchmetrics form is its tail
            p, r, th = skm.precision_recall_curve(y, s32[:, c])
            gp, gr, gt = (got['PRCurve'][k][c] for k in range(3))
            n = len(gp)
            assert same(gp, p[-n:]) and same(gr, r[-n:]) and same(gt, th[len(th) - (n - 1):].astype(np.float64))
    after = flow.compute_metrics()
    assert 'AUROC' not in after and 'ROCCurve' not in after and flow._rank_rows == 0           # reset


def test_no_rank_metrics_without_evaluation_rows_or_when_turned_off():
    (b,) = _batches([8], 3)
    flow = _flow()
    flow.training_step(b, 0)
    assert set(flow.compute_metrics()) == {'ConfusionMatrix', 'Accuracy', 'Precision', 'Recall', 'F1Score'}
    off = _flow(classification_rank_metrics=False)
    off.validation_step(b, 0)
    assert set(off.compute_metrics()) == {'ConfusionMatrix', 'Accuracy', 'Precision', 'Recall', 'F1Score'}
    assert 'AUROC' not in off.get_metrics() and off._rank_scores is None
    flow.validation_step(b, 0)
    kept = flow.compute_metrics(reset=False)
    assert same(flow.compute_metrics()['AUROC'], kept['AUROC'])                                # reset=False kept the rows


def test_buffer_grows_by_doubling():
    flow = _flow()
    flow.rank_initial_capacity = 4
    b = _batches([3, 6, 2], 3)
    logits = torch.cat([flow.validation_step(x, i)['preds']['cross_logits'] for i, x in enumerate(b)])
    assert flow._rank_targets.shape[0] == 16 and flow._rank_rows == 11
    assert torch.equal(flow._rank_scores[:11], torch.softmax(logits, -1))


def test_binary_form():
    flow = _flow(num_classes=2, binary=True)
    b = _batches([12, 7], 2)
    logits = torch.cat([flow.validation_step(x, i)['preds']['cross_logits'] for i, x in enumerate(b)])
    assert logits.shape == (19, 1) and flow._rank_scores.shape[1] == 1
    targets = torch.cat([x[1]['cross'][:, 0] for x in b]).numpy()
    s32 = torch.sigmoid(logits[:, 0]).numpy()
    want, _ = np_curves(s32, targets)
    got = flow.compute_metrics()
    check_flow_metrics(got, want, binary=True)
    if skm is not None and 0 < targets.sum() < 19:
        assert abs(got['AUROC'] - skm.roc_auc_score(targets, s32)) <= 19 * 2.0 ** -52


def test_a_class_without_positives_gives_nan_and_still_returns_curves():
    flow = _flow()
    b = _batches([10], 3)[0]
    b[1]['cross'].clamp_(max=1)                                            # class 2 never occurs
    logits = flow.validation_step(b, 0)['preds']['cross_logits']
    want, _ = np_curves(torch.softmax(logits, -1).numpy(), b[1]['cross'][:, 0].numpy())
    assert math.isnan(want[2]['auroc']) and not math.isnan(want[0]['auroc'])
    got = flow.compute_metrics()
    assert math.isnan(got['AUROC'])
    check_flow_metrics(got, want)
    assert len(got['ROCCurve'][0][2]) == 11 and np.isnan(got['ROCCurve'][1][2][1:]).all() and len(got['PRCurve'][0][2]) == 2


def test_sample_curve_uses_the_reference_index_formula():
    from pedestrians_video_2_carla_amd.modules.flow.classification import LitClassificationFlow, sample_curve
    x, y = np.linspace(0, 1, 57), np.linspace(1, 0, 57) ** 2
    sx, sy = sample_curve(x, y)
    assert sx == [float(x[int(57 * k / 20)]) for k in range(20)] and sy == [float(y[int(57 * k / 20)]) for k in range(20)]
    sx, sy = LitClassificationFlow.sample_curve(x[:7], y[:7], samples=20)           # fewer points than samples
    assert sx == [float(v) for v in x[:7]] and len(sy) == 7
    sx, _ = sample_curve(x, y[:10], samples=5)                                     # x and y of different lengths (PR thresholds)
    assert sx == [float(x[int(57 * k / 5)]) for k in range(5)]


# ---------------------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


SHARES = (5, 9)


def _rank_worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from pedestrians_video_2_carla_amd.trainer import init_distributed
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    torch.set_num_threads(2)
    init_distributed('gloo')
    flow = _flow()
    batch = _batches(SHARES, 3, seed=21)[rank]
    logits = flow.validation_step(batch, 0)['preds']['cross_logits']
    got = flow.compute_metrics(sync=True)
    torch.save({'logits': logits, 'targets': batch[1]['cross'][:, 0], 'AUROC': got['AUROC'], 'ROCCurve': got['ROCCurve'],
                'PRCurve': got['PRCurve'], 'matrix': got['ConfusionMatrix']}, os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_with_unequal_shares_report_the_whole_set(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [torch.load(os.path.join(tmp_path, f'rank{k}.pt'), weights_only=False) for k in range(2)]
    assert [len(x['targets']) for x in r] == list(SHARES)
    scores = torch.softmax(torch.cat([x['logits'] for x in r]), -1).numpy()
    targets = torch.cat([x['targets'] for x in r]).numpy()
    want, n_valid = np_curves(scores, targets)
    assert n_valid == sum(SHARES) and np.sum(r[0]['matrix']) == sum(SHARES)
    for x in r:
        check_flow_metrics(x, want)


# --------------------------------------------------------------------------------------------------------------------- ABI
def _lib_loaded():
    from pedestrians_video_2_carla_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib, _lib.lib()


def test_rank_symbols_are_declared_bound_and_exported():
    _lib, lib = _lib_loaded()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    for name in ('p2c_rank_workspace_bytes', 'p2c_rank_curves', 'p2c_rank_scores'):
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
    for name in ('p2c_rank_curves', 'p2c_rank_scores'):       # the stream goes last: the LDS-poisoning audit wrapper covers them
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p


def test_rank_descriptor_layout_matches_the_header(tmp_path):
    from pedestrians_video_2_carla_amd._lib import P2C_RANK_GLOBAL, RankDesc
    fields = [f[0] for f in RankDesc._fields_]
    src = tmp_path / 'rank.c'
    body = '\n'.join(f'  printf("{f} %zu\\n", offsetof(p2c_rank_desc, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(p2c_rank_desc));\n'
                   '  printf("global %d\\n", P2C_RANK_GLOBAL);\n' + body + '\n  return 0;\n}\n')
    exe = tmp_path / 'rank'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(out['sizeof']) == ctypes.sizeof(RankDesc) and int(out['global']) == P2C_RANK_GLOBAL
    for f in fields:
        assert int(out[f]) == getattr(RankDesc, f).offset, f


def test_rank_argument_errors_are_answered_before_the_device():
    _lib, lib = _lib_loaded()

    def call(N, C, flags=0, pointers=0):
        d = _lib.RankDesc()
        d.N, d.C, d.flags = N, C, flags
        for f in ('scores', 'targets', 'thresholds', 'tps', 'fps', 'n_points', 'n_pos', 'auroc', 'n_valid')[:pointers]:
            setattr(d, f, 64)
        return lib.p2c_rank_curves(ctypes.byref(d), None, None)
    assert call(4, 0) == -2 and call(4, 33) == -2 and call((1 << 24) + 1, 3) == -2 and call(-1, 3) == -2
    assert call(4, 3, flags=2) == -3 and call(4, 3, flags=3) == -3
    assert call(4, 3) == -1 and call(4, 3, pointers=5) == -1 and call(4, 3, pointers=8) == -1
    assert call(4, 3, flags=_lib.P2C_RANK_GLOBAL, pointers=9) == -1          # the global regime needs its workspace
    assert call(20000, 3, pointers=9) == -1
    assert lib.p2c_rank_curves(None, None, None) == -1
    assert lib.p2c_rank_workspace_bytes(4, 0, 0) == -2 and lib.p2c_rank_workspace_bytes(4, 33, 0) == -2
    assert lib.p2c_rank_workspace_bytes((1 << 24) + 1, 3, 0) == -2 and lib.p2c_rank_workspace_bytes(4, 3, 2) == -3
    # p2c_rank_scores: flags, shapes (C, the rows of the buffer), pointers
    assert lib.p2c_rank_scores(None, None, 4, 3, 2, None, None, 0, 8, None) == -3
    assert lib.p2c_rank_scores(None, None, 4, 33, 0, None, None, 0, 8, None) == -2
    assert lib.p2c_rank_scores(None, None, 4, 1, 0, None, None, 0, 8, None) == -2
    assert lib.p2c_rank_scores(None, None, 4, 2, _lib.P2C_CLS_BINARY, None, None, 0, 8, None) == -2
    assert lib.p2c_rank_scores(None, None, 4, 3, 0, None, None, 5, 8, None) == -2               # rows 5..8 of 8
    assert lib.p2c_rank_scores(None, None, 4, 3, 0, None, None, -1, 8, None) == -2
    assert lib.p2c_rank_scores(None, None, 4, 3, 0, None, None, 4, 8, None) == -1
    assert lib.p2c_rank_scores(None, None, 0, 3, 0, None, None, 0, 0, None) == 0                # an empty batch: nothing to do


def test_rank_workspace_is_monotone_in_n():
    _lib, lib = _lib_loaded()
    for C in (1, 5, 32):
        for flags in (0, _lib.P2C_RANK_GLOBAL):
            sizes = [lib.p2c_rank_workspace_bytes(N, C, flags) for N in (0, 1, 2, 4096, 4097, 16384, 16385, 70001, 1 << 20, 1 << 24)]
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] == 0, (C, flags, sizes)
            assert sizes[-1] >= 2 * 8 * C * (1 << 24) and sizes[6] >= 2 * 8 * C * 16385      # two buffers of 8-byte elements
        assert lib.p2c_rank_workspace_bytes(16384, C, 0) == 0 < lib.p2c_rank_workspace_bytes(16384, C, _lib.P2C_RANK_GLOBAL)
