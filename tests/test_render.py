"""Host: the video logger (loggers/pedestrian, renderers/) and the definition of ``ops.render_points`` (K34's tensor restatement).

The tensor definition is pinned against a third, naive statement of the rules of include/p2c.h (K34): per-pixel Python loops in
Python integers on tiny canvases. The external ``pedestrians_scenarios`` PointsRenderer is not available: pixel parity with it is
unpinned and those rules are the definition. The logger and the writer restate the reference's policy (which renderers survive,
when clips are written, how panels merge, where files go); the trainer tests use a small host flow -- the pose-lifting flow and
``SyntheticCarlaRecordedDataModule.generate_batch`` have no host path -- on batches of the data module's structure."""
import argparse
import ctypes
import itertools
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

from pedestrians_video_2_carla_amd import _lib, ops
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.loggers.pedestrian import (DisabledPedestrianWriter, MergingMethod, PedestrianLogger,
                                                              PedestrianRenderers, PedestrianWriter)
from pedestrians_video_2_carla_amd.loggers.pedestrian.pedestrian_writer import grid_layout, npz_video_writer
from pedestrians_video_2_carla_amd.renderers import PointsRenderer, Renderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = PedestrianRenderers
H, W = 5, 8
COLORS = torch.tensor([[255, 0, 0], [0, 255, 0], [0, 0, 255]], dtype=torch.uint8)
EDGES = [[0, 1], [1, 2]]
NAN, INF = float('nan'), float('inf')


# ---- the naive statement ------------------------------------------------------------------------------------------------------
def naive_render(points, colors, edges, H, W, radius, line_width):
    V, T, J = points.shape[:3]
    out = np.zeros((V, T, H, W, 3), dtype=np.uint8)
    L2 = line_width * line_width
    for v, t in itertools.product(range(V), range(T)):
        centres = []
        for j in range(J):
            x, y = (np.rint(np.float32(points[v, t, j, i])) for i in (0, 1))
            ok = bool(np.isfinite(x) and np.isfinite(y) and abs(x) <= 16383 and abs(y) <= 16383)
            centres.append((int(x), int(y)) if ok else None)
        for py, px in itertools.product(range(H), range(W)):
            colour = (0, 0, 0)
            if line_width > 0:
                for a, b in edges:
                    if centres[a] is None or centres[b] is None:
                        continue
                    (ax, ay), (bx, by) = centres[a], centres[b]
                    dx, dy, qx, qy = bx - ax, by - ay, px - ax, py - ay
                    s, n = qx * dx + qy * dy, dx * dx + dy * dy
                    if s <= 0:
                        covers = 4 * (qx * qx + qy * qy) <= L2
                    elif s >= n:
                        covers = 4 * ((px - bx) ** 2 + (py - by) ** 2) <= L2
                    else:
                        covers = 4 * (qx * dy - qy * dx) ** 2 <= L2 * n
                    if covers:
                        colour = tuple(colors[b])
            for j in range(J):
                if centres[j] is not None and (px - centres[j][0]) ** 2 + (py - centres[j][1]) ** 2 <= radius * radius:
                    colour = tuple(colors[j])
            out[v, t, py, px] = colour
    return out


# (V = 1, T frames, J = 3): every frame of a case is one placement
CASES = {
    'half_integers': [[[2.5, 1.5], [3.5, 2.5], [0.5, 3.5]]],
    'corners': [[[0, 0], [7, 0], [0, 4]], [[7, 4], [0, 0], [7, 0]]],
    'outside_every_side': [[[-1, 2], [8, 2], [3, -1]], [[3, 5], [-2, 2], [9, 2]], [[3, -2], [3, 6], [-2, -2]]],
    'non_finite': [[[NAN, 1], [4, 2], [6, 3]], [[1, 1], [INF, 2], [6, 3]], [[1, 1], [4, 2], [3, -INF]], [[1e9, 1], [4, 2], [6, 3]],
                   [[1, 1], [4, -1e9], [6, 3]], [[16383, 1], [16384, 1], [-16384, 2]]],
    'coincident': [[[3, 2], [3, 2], [5, 2]], [[3, 2], [3, 2], [3, 2]]],
    'joints_over_bones': [[[1, 1], [6, 1], [6, 3]], [[1, 3], [4, 0], [7, 3]]],
    'degenerate_bone': [[[2, 2], [2, 2], [6, 2]], [[2.4, 2.4], [1.6, 1.6], [6, 4]]],
    'bone_crossing_from_outside': [[[-3, -2], [10, 6], [4, 2]], [[-4, 2], [12, 2], [4, -3]], [[3, -5], [3, 9], [-9, 2]]],
}


@pytest.mark.parametrize('name', list(CASES))
def test_the_tensor_definition_equals_the_naive_statement(name):
    points = torch.tensor([CASES[name]], dtype=torch.float32)
    for radius, line_width in itertools.product((0, 1, 2), (0, 1, 3)):
        got = ops.render_points([(points, COLORS, EDGES)], size=(H, W), layout=(1, 1), radius=radius, line_width=line_width)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, points.shape[1], H, W, 3)
        want = naive_render(points.numpy(), COLORS.tolist(), EDGES, H, W, radius, line_width)
        assert np.array_equal(got.numpy(), want), (name, radius, line_width)
        assert torch.equal(ops._render_points_tensor([(points, COLORS, torch.tensor(EDGES))], (H, W), (1, 1), radius, line_width), got)


def test_rounding_validity_and_overwrite_order_by_hand():
    one = lambda pts, **kw: ops.render_points([(torch.tensor([[pts]], dtype=torch.float32), COLORS, EDGES)], size=(H, W), **kw)[0, 0]
    # half to even: 2.5 -> 2, 3.5 -> 4, 0.5 -> 0, 1.5 -> 2; x is the column, y the row
    img = one([[2.5, 1.5], [3.5, 0.5], [0.5, 3.5]], radius=0)
    lit = {(int(r), int(c)): tuple(img[r, c].tolist()) for r, c in img.any(-1).nonzero().tolist()}
    assert lit == {(2, 2): (255, 0, 0), (0, 4): (0, 255, 0), (4, 0): (0, 0, 255)}
    # NaN / inf / 1e9 draw nothing, and neither do their bones
    for bad in (NAN, INF, -INF, 1e9, 16384):
        img = one([[1, 1], [bad, 2], [6, 3]], radius=1, line_width=3)
        assert torch.equal(img, one([[1, 1], [bad, 2], [6, 3]], radius=1, line_width=0))
        assert not (img == torch.tensor([0, 255, 0], dtype=torch.uint8)).all(-1).any()
    # coincident joints: the higher index wins; joints sit over bones; a bone has the colour of its second joint
    assert tuple(one([[3, 2], [3, 2], [3, 2]], radius=0)[2, 3].tolist()) == (0, 0, 255)
    img = one([[1, 2], [6, 2], [6, 2]], radius=0, line_width=1)
    assert tuple(img[2, 3].tolist()) == (0, 255, 0) and tuple(img[2, 1].tolist()) == (255, 0, 0) and tuple(img[2, 6].tolist()) == (0, 0, 255)
    # line_width 0: no bones; edges may be empty or None
    p = torch.tensor([[[[1., 1.], [6., 3.], [3., 2.]]]])
    assert torch.equal(ops.render_points([(p, COLORS, None)], size=(H, W), line_width=3),
                       ops.render_points([(p, COLORS, EDGES)], size=(H, W), line_width=0))
    # the confidence column is ignored; fp64 points give the same bytes
    p3 = torch.cat([p, torch.zeros(1, 1, 3, 1)], -1)
    assert torch.equal(ops.render_points([(p3, COLORS, EDGES)], size=(H, W), line_width=1),
                       ops.render_points([(p.double(), COLORS, EDGES)], size=(H, W), line_width=1))


def test_bad_arguments_raise():
    p = torch.zeros(1, 1, 3, 2)
    with pytest.raises(RuntimeError, match='outside'):
        ops.render_points([(p, COLORS, [[0, 3]])], size=(H, W), line_width=1)
    with pytest.raises(RuntimeError, match='colors'):
        ops.render_points([(p, COLORS[:2], None)], size=(H, W))
    with pytest.raises(RuntimeError, match='panels for a layout'):
        ops.render_points([(p, COLORS, None)] * 3, size=(H, W), layout=(1, 2))
    with pytest.raises(RuntimeError, match='at least one panel'):
        ops.render_points([None], size=(H, W))
    with pytest.raises(RuntimeError, match='expected'):
        ops.render_points([(p, COLORS, None), (torch.zeros(2, 1, 3, 2), COLORS, None)], size=(H, W), layout=(1, 2))
    assert tuple(ops.render_points([(torch.zeros(0, 4, 3, 2), COLORS, None)], size=(H, W)).shape) == (0, 4, H, W, 3)


# ---- layout -------------------------------------------------------------------------------------------------------------------
def test_grid_layout_rules():
    sq, ho, ve = MergingMethod.square, MergingMethod.horizontal, MergingMethod.vertical
    assert [grid_layout(n, sq) for n in (1, 2, 3, 4, 5)] == [(ho, 1, 1), (ho, 1, 2), (sq, 2, 2), (sq, 2, 2), (sq, 2, 3)]
    assert [grid_layout(n, ho)[1:] for n in (1, 2, 3, 4, 5)] == [(1, n) for n in (1, 2, 3, 4, 5)]
    assert [grid_layout(n, ve)[1:] for n in (1, 2, 3, 4, 5)] == [(n, 1) for n in (1, 2, 3, 4, 5)]


@pytest.mark.parametrize('n', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('method', list(MergingMethod))
def test_panels_land_in_their_cells(n, method):
    g = torch.Generator().manual_seed(n)
    panels = [(torch.rand(2, 2, 3, 2, generator=g) * torch.tensor([W, H]), COLORS.roll(k, 0), EDGES) for k in range(n)]
    if n >= 3:
        panels[1] = None                                    # a None panel is a zero cell
    _, rows, cols = grid_layout(n, method)
    out = ops.render_points(panels, size=(H, W), layout=(rows, cols), radius=1, line_width=1)
    assert tuple(out.shape) == (2, 2, rows * H, cols * W, 3)
    for k in range(rows * cols):
        r, c = divmod(k, cols)
        cell = out[:, :, r * H:(r + 1) * H, c * W:(c + 1) * W]
        if k < n and panels[k] is not None:
            assert torch.equal(cell, ops.render_points([panels[k]], size=(H, W), radius=1, line_width=1)) and cell.any()
        else:
            assert not cell.any()                            # 3 under square: a 2 x 2 grid with a zero cell; 5: 3 x 2 with one
    if method == MergingMethod.square:
        assert (rows, cols) == {1: (1, 1), 2: (1, 2), 3: (2, 2), 4: (2, 2), 5: (2, 3)}[n]


# ---- renderers ----------------------------------------------------------------------------------------------------------------
def test_points_renderer_hands_back_a_panel_description():
    r = PointsRenderer(CARLA_SKELETON)
    assert r.image_size == (800, 600) and r.radius == 2 and r.line_width == 0
    pts = torch.zeros(1, 2, 26, 3)
    points, colors, edges = r.render(pts)
    assert points is pts and colors.dtype == torch.uint8 and tuple(colors.shape) == (26, 3) and tuple(edges.shape) == (0, 2)
    assert colors.tolist() == [list(CARLA_SKELETON.get_colors()[k][:3]) for k in CARLA_SKELETON]
    edges = PointsRenderer(CARLA_SKELETON, line_width=2).render(pts)[2]
    assert edges.tolist() == [[a.value, b.value] for a, b in CARLA_SKELETON.get_edges()] and len(edges) == 25
    assert Renderer().render(pts) is None and Renderer().image_size == (800, 600)
    with pytest.raises(RuntimeError):
        r.render(torch.zeros(1, 2, 25, 2))


# ---- PedestrianLogger ---------------------------------------------------------------------------------------------------------
def test_enums_carry_the_reference_values():
    assert {m.name: m.value for m in PedestrianRenderers} == dict(none=0, source_videos=1, source_carla=2, target_points=3,
                                                                   input_points=4, projection_points=5, carla=6, smpl=7, zeros=100)
    assert {m.name: m.value for m in MergingMethod} == dict(vertical=0, horizontal=1, square=2)


def _logger(renderers, tmp_path, **kw):
    kw.setdefault('input_nodes', CARLA_SKELETON)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        logger = PedestrianLogger(str(tmp_path), 'run', renderers=renderers, **kw)
    return logger, [str(w.message) for w in caught]


def test_logger_disabling_rules_and_their_warnings(tmp_path):
    nodes = dict(output_nodes=CARLA_SKELETON)
    logger, said = _logger([R.input_points, R.projection_points], tmp_path, **nodes)
    assert logger.renderers == [R.input_points, R.projection_points] and said == [] and not logger.disabled
    assert logger.reduced_log_every_n_steps == 500 and isinstance(logger.experiment, PedestrianWriter)
    assert logger.experiment is logger.experiment and logger.name == 'run' and logger.version == 0
    # 1: an interval of one step or less disables the writer
    for every, reduction in ((50, 0), (1, 1), (0, 10)):
        logger, said = _logger([R.input_points], tmp_path, log_every_n_steps=every, video_saving_frequency_reduction=reduction)
        assert logger.disabled and isinstance(logger.experiment, DisabledPedestrianWriter) and any('interval' in s for s in said)
        assert logger.experiment.log_videos(meta={}, step=0, batch_idx=0, stage='val') is None
    assert not _logger([R.input_points], tmp_path, log_every_n_steps=1, video_saving_frequency_reduction=2)[0].disabled
    # 2: the CARLA renderers and smpl go, each with its warning
    logger, said = _logger([R.carla, R.input_points, R.source_carla, R.smpl], tmp_path)
    assert logger.renderers == [R.input_points] and sum('CARLA' in s for s in said) == 1 and sum('SMPL' in s for s in said) == 1
    # 3: none goes silently; alone it leaves nothing (6)
    logger, said = _logger([R.none, R.target_points], tmp_path)
    assert logger.renderers == [R.target_points] and said == []
    logger, said = _logger([R.none], tmp_path)
    assert logger.disabled and said == ['No renderers specified. Disabling video output.']
    # 4: source_videos always goes, with a warning, also with a directory
    logger, said = _logger([R.source_videos, R.input_points], tmp_path, source_videos_dir='/somewhere')
    assert logger.renderers == [R.input_points] and len(said) == 1 and 'ource videos' in said[0]
    # 5: projection_points needs output_nodes
    logger, said = _logger([R.input_points, R.projection_points], tmp_path)
    assert logger.renderers == [R.input_points] and len(said) == 1 and 'output_nodes' in said[0]
    # 6: nothing given, or nothing left
    for renderers in (None, [], [R.projection_points], [R.carla, R.source_videos]):
        logger, said = _logger(renderers, tmp_path)
        assert logger.disabled and said[-1] == 'No renderers specified. Disabling video output.'
    # the caller's list is not edited
    mine = [R.none, R.input_points]
    _logger(mine, tmp_path)
    assert mine == [R.none, R.input_points]
    assert logger.log_hyperparams({}) is None and logger.log_metrics({}, 0) is None


def test_logger_argparse_flags_and_defaults():
    parser = PedestrianLogger.add_logger_specific_args(argparse.ArgumentParser())
    a = parser.parse_args([])
    assert (a.video_saving_frequency_reduction, a.max_videos, a.renderers, a.merging_method) == (10, 10, [], MergingMethod.square)
    assert (a.source_videos_dir, a.source_videos_overlay_skeletons, a.source_videos_overlay_bboxes,
            a.source_videos_overlay_classes) == (None, False, False, False)
    a = parser.parse_args('--renderers input_points projection_points --merging_method vertical --max_videos -1 '
                          '--video_saving_frequency_reduction -3 --source_videos_dir d --source_videos_overlay_bboxes'.split())
    assert a.renderers == [R.input_points, R.projection_points] and a.merging_method == MergingMethod.vertical
    assert a.max_videos == -1 and a.video_saving_frequency_reduction == 0 and a.source_videos_dir == 'd' and a.source_videos_overlay_bboxes


# ---- PedestrianWriter ---------------------------------------------------------------------------------------------------------
def _batch(B=4, T=4, seed=0, extra_meta=None):
    g = torch.Generator().manual_seed(seed)
    p2d = torch.randn(B, T, 26, 2, generator=g)
    targets = {'projection_2d': p2d * 50 + 300, 'projection_2d_transformed': p2d}
    meta = {'age': ['adult', 'child'] * (B // 2), 'gender': ['female', 'male'] * (B // 2)}
    meta.update(extra_meta or {})
    return p2d + 0.01, targets, meta


def _writer(tmp_path, written, renderers=(R.input_points, R.projection_points), **kw):
    kw.setdefault('image_size', (16, 12))
    return PedestrianWriter(log_dir=str(tmp_path), renderers=list(renderers), input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON,
                            video_writer=lambda path, frames, fps: written.append((path, frames, fps)), **kw)


def test_writer_gate_slice_paths_callback_and_one_launch(tmp_path, monkeypatch):
    written, calls = [], []
    real = ops.render_points
    monkeypatch.setattr(ops, 'render_points', lambda *a, **k: (calls.append((a, k)), real(*a, **k))[1])
    w = _writer(tmp_path, written, reduced_log_every_n_steps=4, max_videos=3, fps=12.0)
    frames, targets, meta = _batch(extra_meta={'clip_id': [7, 8, 9, 10], 'set_name': ['train_set'] * 4})
    send = dict(meta=meta, batch_idx=5, inputs=frames, targets=targets, projection_2d_transformed=targets['projection_2d_transformed'] * 0.5)
    for step in (1, 2, 3, 5, 7):
        w.log_videos(step=step, stage='val', **send)
    assert written == [] and calls == [] and not w.wants(3) and w.wants(0) and w.wants(8) and w.wants(3, force=True)
    seen = []
    w.log_videos(step=8, stage='val', vid_callback=lambda *a: seen.append(a), **send)
    assert len(calls) == 1 and len(written) == 3                                   # one render_points call, max_videos clips
    assert calls[0][1]['layout'] == (1, 2) and calls[0][1]['size'] == (12, 16)      # (height, width); two panels side by side
    ids = ['adult_female-07', 'child_male-08', 'adult_female-09']
    assert [p for p, _, _ in written] == [os.path.join(str(tmp_path), 'val', 'train_set', f'video_05_{i:02d}', f'{ids[i]}-step=0008')
                                          for i in range(3)]
    assert all(os.path.isdir(os.path.dirname(p)) for p, _, _ in written)
    assert all(f.dtype == torch.uint8 and tuple(f.shape) == (4, 12, 32, 3) and fps == 12.0 for _, f, fps in written)
    for i, (vid, vid_idx, fps, stage, vid_meta) in enumerate(seen):
        assert vid is written[i][1] and vid_idx == i and fps == 12.0 and stage == 'val'
        assert vid_meta['video_id'] == f'video_05_{i:02d}' and vid_meta['clip_id'] == 7 + i and vid_meta['age'] == meta['age'][i]
    # force passes the gate; -1 keeps every video; default ids without age / gender / clip_id / set_name
    w = _writer(tmp_path, written := [], reduced_log_every_n_steps=500, max_videos=-1)
    frames, targets, _ = _batch()
    w.log_videos(meta={}, step=3, batch_idx=0, stage='test', force=True, inputs=frames, targets=targets,
                 projection_2d=targets['projection_2d'])
    assert [p for p, _, _ in written] == [os.path.join(str(tmp_path), 'test', f'video_00_{i:02d}', 'adult_female-00-step=0003') for i in range(4)]


def test_writer_panels_are_the_denormalised_points(tmp_path):
    """What is drawn: inputs / targets / projections through the reference skeleton's hips-neck scale, side by side; a padded square
    and a projection renderer without output nodes are black."""
    from pedestrians_video_2_carla_amd.data.carla import reference as ref
    frames, targets, meta = _batch()
    w = _writer(tmp_path, written := [], renderers=(R.input_points, R.target_points, R.projection_points), image_size=(800, 600),
                max_videos=2, merging_method=MergingMethod.square)
    assert w.layout == (2, 2) and w.used_renderers[-1] == R.zeros
    projected = targets['projection_2d_transformed'] * 0.5
    w.log_videos(meta=meta, step=0, batch_idx=0, stage='val', inputs=frames, targets=targets, projection_2d_transformed=projected)
    types = ref.skeleton_types_from_meta(meta, batch_size=4).long()[:2]
    proj = ref.get_projections(torch.device('cpu'))[types][..., :2]
    hips, neck = CARLA_SKELETON.get_hips_point().value, CARLA_SKELETON.get_neck_point().value
    shift = proj[:, hips]
    scale = torch.linalg.norm(proj[:, neck] - shift, dim=-1)
    den = lambda x: x[:2] * scale[:, None, None, None] + shift[:, None, None, :]
    renderer = PointsRenderer(CARLA_SKELETON)
    want = ops.render_points([renderer.render(den(frames)), renderer.render(den(targets['projection_2d_transformed'])),
                              renderer.render(den(projected)), None], size=(600, 800), layout=(2, 2))
    assert len(written) == 2 and all(torch.equal(written[i][1], want[i]) for i in range(2)) and want.any()
    assert not want[:, :, 600:, 800:].any()
    # without the transformed targets the input is normalised first (autonormalize): the same picture for these targets
    w2 = _writer(tmp_path, written2 := [], renderers=(R.target_points,), image_size=(800, 600), max_videos=2)
    w2.log_videos(meta=meta, step=0, batch_idx=0, stage='val', inputs=targets['projection_2d'], targets={'projection_2d': targets['projection_2d']})
    hn = targets['projection_2d'][:2]
    s = hn[..., hips, :]
    normalised = (hn - s[..., None, :]) / torch.linalg.norm(hn[..., neck, :] - s, dim=-1)[..., None, None]
    assert torch.equal(written2[0][1], ops.render_points([renderer.render(den(torch.cat([normalised, normalised])))], size=(600, 800))[0])
    # projection_points without output nodes is a black panel
    w3 = PedestrianWriter(log_dir=str(tmp_path), renderers=[R.input_points, R.projection_points], input_nodes=CARLA_SKELETON,
                          video_writer=lambda p, f, fps: written2.append((p, f, fps)), image_size=(800, 600), max_videos=1)
    w3.log_videos(meta=meta, step=0, batch_idx=0, stage='val', inputs=frames, targets=targets, projection_2d_transformed=projected)
    assert not written2[-1][1][:, :, 800:].any() and written2[-1][1][:, :, :800].any()


def test_npz_writer_round_trips(tmp_path):
    frames = torch.randint(0, 256, (3, 6, 8, 3), dtype=torch.uint8)
    path = npz_video_writer(str(tmp_path / 'clip'), frames, 29.97)
    assert path.endswith('clip.npz') and os.path.exists(path)
    with np.load(path) as d:
        assert np.array_equal(d['frames'], frames.numpy()) and float(d['fps']) == 29.97
    # the default writer of a PedestrianWriter: .mp4 through torchvision when it is installed, else this one
    w = PedestrianWriter(log_dir=str(tmp_path), renderers=[R.input_points], input_nodes=CARLA_SKELETON, image_size=(16, 12), max_videos=1)
    f, t, meta = _batch()
    w.log_videos(meta=meta, step=0, batch_idx=0, stage='val', inputs=f, targets=t)
    files = os.listdir(tmp_path / 'val' / 'video_00_00')
    assert files in (['adult_female-00-step=0000.npz'], ['adult_female-00-step=0000.mp4'])


# ---- Trainer(loggers=[...]) on the host --------------------------------------------------------------------------------------------
from pedestrians_video_2_carla_amd.modules.flow.base import LitBaseFlow            # noqa: E402
from pedestrians_video_2_carla_amd.modules.flow.lightning_shim import LightningModuleBase   # noqa: E402


class TinyFlow(LightningModuleBase):
    """A host flow over CarlaRecorded-shaped batches with everything a stray forward could disturb: dropout and BatchNorm."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.net = torch.nn.Sequential(torch.nn.Linear(52, 32), torch.nn.BatchNorm1d(32), torch.nn.Dropout(0.5), torch.nn.Linear(32, 52))
        self.predicted = []

    def configure_optimizers(self):
        return [{'optimizer': torch.optim.AdamW(self.parameters(), lr=1e-2)}]

    def _project(self, frames):
        return self.net(frames.reshape(-1, 52)).view(frames.shape)

    def on_train_batch_start(self, batch, batch_idx):
        pass

    on_validation_batch_start = on_train_batch_start

    def training_step(self, batch, batch_idx):
        frames, targets, _ = batch
        return {'loss': (self._project(frames) - targets['projection_2d_transformed']).pow(2).mean()}

    def _sliced(self, batch):
        frames, targets, _ = batch
        return {'inputs': frames, 'targets': targets, 'projection_2d': None, 'projection_2d_transformed': self._project(frames)}

    def predict_step(self, batch, batch_idx):
        assert not self.training and not torch.is_grad_enabled()
        self.predicted.append(batch_idx)
        return self._sliced(batch), batch[2]

    _log_videos = LitBaseFlow._log_videos

    def validation_step(self, batch, batch_idx):
        self._log_videos(meta=batch[2], batch_idx=batch_idx, stage='val', **self._sliced(batch))

    def compute_metrics(self, sync=False):
        return {}


def _fit(tmp_path, with_logger, steps=7, written=None):
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    from pedestrians_video_2_carla_amd.trainer import Trainer
    dm = SyntheticCarlaRecordedDataModule(clip_length=4, batch_size=4)
    flow = TinyFlow()
    loggers = [PedestrianLogger(str(tmp_path), 'run', version=3, log_every_n_steps=1, video_saving_frequency_reduction=3,
                                renderers=[R.input_points, R.projection_points], input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON,
                                image_size=(16, 12), video_writer=lambda p, f, fps: written.append((p, f)))] if with_logger else None
    trainer = Trainer(max_steps=steps, loggers=loggers)
    torch.manual_seed(99)                                    # the dropout masks of the run
    losses = trainer.fit(flow, dm, batches=[_batch(seed=i) for i in range(steps)])
    return trainer, flow, losses


def test_fit_logs_at_the_interval_and_leaves_training_untouched(tmp_path):
    written = []
    trainer, flow, losses = _fit(tmp_path, True, written=written)
    assert flow.predicted == [0, 3, 6] and flow.training                  # one extra forward at steps 0, 3, 6 and only there
    steps = sorted({int(re.search(r'step=(\d+)$', p).group(1)) for p, _ in written})
    assert steps == [0, 3, 6] and len(written) == 3 * 4
    assert all(p.startswith(os.path.join(str(tmp_path), 'run', '3', 'train', 'video_')) for p, _ in written)
    assert all(tuple(f.shape) == (4, 12, 32, 3) for _, f in written)
    plain_trainer, plain, plain_losses = _fit(tmp_path / 'none', False)
    assert plain.predicted == [] and plain_trainer.loggers == [] and not (tmp_path / 'none').exists()      # no logger: nothing written
    assert all(torch.equal(a, b) for a, b in zip(losses, plain_losses))
    assert torch.equal(trainer.flat.flat_param.data, plain_trainer.flat.flat_param.data)
    for a, b in zip(flow.buffers(), plain.buffers()):                     # BatchNorm statistics and step counts
        assert torch.equal(a, b)


def test_validate_logs_stage_val_through_the_flow_hook(tmp_path):
    written = []
    trainer, flow, _ = _fit(tmp_path, True, steps=3, written=written)
    del written[:]
    assert trainer.global_step == 3                         # a multiple of the interval: the writer's gate is open
    trainer.validate(flow, [_batch(seed=40), _batch(seed=41)])
    assert len(written) == 8 and flow.training
    assert all(os.sep + os.path.join('run', '3', 'val', 'video_') in p and p.endswith('step=0003') for p, _ in written)
    assert {os.path.basename(os.path.dirname(p)) for p, _ in written} == {f'video_{b:02d}_{v:02d}' for b in (0, 1) for v in range(4)}
    trainer.global_step = 4                                 # closed
    trainer.validate(flow, [_batch(seed=40)])
    assert len(written) == 8
    # stage train is a no-op in the flow, and so is every stage without a logger
    flow._log_videos(meta=_batch()[2], batch_idx=0, stage='train', **flow._sliced(_batch()))
    trainer.loggers = []
    trainer.global_step = 3
    trainer.validate(flow, [_batch(seed=40)])
    assert len(written) == 8


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
def test_render_symbols_are_declared_bound_and_exported():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    header = open(os.path.join(ROOT, 'include', 'p2c.h')).read()
    declared = set(re.findall(r'P2C_API[^;(]*?\b(p2c_\w+)\s*\(', header))
    lib = getattr(_lib.lib(), '_h', _lib.lib())
    for name in ('p2c_render_points_supported', 'p2c_render_points_fwd'):
        assert name in declared and name in _lib.SYMBOLS and getattr(lib, name) is not None
    assert declared == set(_lib.SYMBOLS)                                 # header, bindings (and, through lib(), exports) in step
    res, args = _lib.SYMBOLS['p2c_render_points_fwd']
    assert res is ctypes.c_int and args[-1] is ctypes.c_void_p          # the stream goes last: the LDS-poison audit wraps the call
    wrapped = _lib._PoisonedLib(lib)._wrap
    assert 'p2c_render_points_fwd' in wrapped and 'p2c_render_points_supported' not in wrapped
    for name in ('MAX_PANELS', 'MAX_PRIMS', 'MAX_REACH', 'MAX_SIDE', 'MAX_COORD'):
        assert int(re.search(rf'#define P2C_RENDER_{name} (\d+)', header).group(1)) == getattr(_lib, 'P2C_RENDER_' + name)
    # refusals come before any launch (no GPU is touched)
    assert lib.p2c_render_points_fwd(None, None) == -1 and lib.p2c_render_points_supported(None) == 0
    d = _lib.RenderPointsDesc()
    d.V, d.T, d.H, d.W, d.rows, d.cols, d.n_panels, d.radius = 1, 1, 8, 8, 1, 1, 1, 2
    d.panels[0].points, d.panels[0].J, d.panels[0].C = 1, 26, 2
    assert lib.p2c_render_points_supported(ctypes.byref(d)) == 1
    assert lib.p2c_render_points_fwd(ctypes.byref(d), None) == -1        # no out, no colors
    for field, bad in (('W', 6), ('W', 8196), ('H', 0), ('radius', 65), ('line_width', 65), ('n_panels', 9), ('n_panels', 2),
                       ('V', 0), ('max_blocks', -1)):
        good = getattr(d, field)
        setattr(d, field, bad)
        assert lib.p2c_render_points_fwd(ctypes.byref(d), None) == -2, (field, bad)
        assert lib.p2c_render_points_supported(ctypes.byref(d)) == (1 if field == 'max_blocks' else 0)
        setattr(d, field, good)
    for field, bad in (('J', 65), ('E', 65), ('C', 1)):
        good = getattr(d.panels[0], field)
        setattr(d.panels[0], field, bad)
        assert lib.p2c_render_points_supported(ctypes.byref(d)) == 0 and lib.p2c_render_points_fwd(ctypes.byref(d), None) == -2
        setattr(d.panels[0], field, good)


def test_render_descriptor_layout_matches_the_header(tmp_path):
    assert [f for f, _ in _lib.RenderPointsDesc._fields_] == ['V', 'T', 'H', 'W', 'rows', 'cols', 'n_panels', 'radius', 'line_width',
                                                              'max_blocks', 'out', 'panels']
    assert [f for f, _ in _lib.RenderPanel._fields_] == ['points', 'colors', 'edges', 'J', 'E', 'C', 'reserved']
    lines = ['  printf("sizeof %zu\\n", sizeof(p2c_render_points_desc));', '  printf("sizeof_panel %zu\\n", sizeof(p2c_render_panel));']
    lines += [f'  printf("{f} %zu\\n", offsetof(p2c_render_points_desc, {f}));' for f, _ in _lib.RenderPointsDesc._fields_]
    lines += [f'  printf("panel_{f} %zu\\n", offsetof(p2c_render_panel, {f}));' for f, _ in _lib.RenderPanel._fields_]
    src = tmp_path / 'render_desc.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "p2c.h"\nint main(void) {\n' + '\n'.join(lines) + '\n  return 0;\n}\n')
    exe = tmp_path / 'render_desc'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(out['sizeof']) == ctypes.sizeof(_lib.RenderPointsDesc) < 4096            # the panels travel in the kernel arguments
    assert int(out['sizeof_panel']) == ctypes.sizeof(_lib.RenderPanel)
    for f, _ in _lib.RenderPointsDesc._fields_:
        assert int(out[f]) == getattr(_lib.RenderPointsDesc, f).offset, f
    for f, _ in _lib.RenderPanel._fields_:
        assert int(out['panel_' + f]) == getattr(_lib.RenderPanel, f).offset, f
