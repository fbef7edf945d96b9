"""GPU: the two launches of the fused train step (csrc/p2c_train.hip) after their prologues were rearranged -- the clip kernel asks
for a clip's skeleton type ahead of everything and for the reference tables that hang on it only behind layer 0's barrier; the
second launch fetches its kernel arguments in one batch, reads the optimizer's step count on the vector path and finds its tile
without a loop. No arithmetic instruction and no summation order moved, so the rule of tests/test_clip_chain_gpu.py and
tests/test_train_fused_gpu.py holds against the separate kernels (P2C_FUSED_TRAIN=0): the losses are the same BITS; the flat
gradient is the same bits at B = 256, T = 16 only (elsewhere the two paths cut the frames into other sample tiles) and within
1e-4 of its scale otherwise. What is checked here is what the rearrangement could break:

  * the persistent form, where a workgroup's second clip must get the tables of ITS skeleton type;
  * the second launch when a slice has fewer clips than waves, waves without any clip, and the non-unrolled tail loop;
  * the step count behind the bias corrections, eager and replayed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_flow_gpu import close, dev, make  # noqa: E402


def _trainer(flow, dm, **kw):
    from pedestrians_video_2_carla_amd.trainer import Trainer
    return Trainer(device=dev(), **kw).setup(flow, dm)


@pytest.fixture
def latency_form():
    """train_clip_kernel (a workgroup per clip, persistent beyond one clip per CU) at every batch size; restored afterwards."""
    from pedestrians_video_2_carla_amd import _lib
    lib = _lib.lib()
    prev = lib.p2c_train_step_set_stream_min_batch(1 << 30)
    yield
    lib.p2c_train_step_set_stream_min_batch(prev)


def _one_step(monkeypatch, fused, **kw):
    """One forward + backward with the optimizer kept out: (loss, loc_2d, loc_3d, flat gradient, skeleton types)."""
    monkeypatch.setenv('P2C_FUSED_TRAIN', fused)
    flow, dm = make(**kw)
    trainer = _trainer(flow, dm)
    trainer.optimizers[0].zero_grad_in_step = False
    batch = dm.generate_batch(dev())
    loss = trainer._forward_backward(flow, batch, 0)
    torch.cuda.synchronize()
    assert (getattr(flow, '_pair_counts', None) is not None) == (fused == '1')
    return (loss.detach().cpu().clone(), flow.logged['train_loss/loc_2d'].cpu().clone(),
            flow.logged['train_loss/loc_3d'].cpu().clone(), trainer.flat.flat_grad.detach().cpu().clone(),
            batch[2]['skel_type'].cpu().clone())


def _same_as_separate(monkeypatch, **kw):
    monkeypatch.setenv('P2C_FUSED_UPDATE', '0')
    sep = _one_step(monkeypatch, '0', **kw)
    fus = _one_step(monkeypatch, '1', **kw)
    assert torch.equal(sep[4], fus[4])
    assert torch.isfinite(sep[3]).all() and sep[3].abs().max() > 0
    names = ('loss', 'loc_2d', 'loc_3d', 'flat gradient')
    for a, b, what in zip(sep, fus, names):
        print(f'{kw} {what}: max |diff| {(a - b).abs().max().item():.3e} at scale {a.abs().max().item():.3e}')
    for a, b, what in zip(sep[:3], fus[:3], names):
        assert torch.equal(a, b), f'{what}: max |diff| {(a - b).abs().max().item():.3e}'
    if kw['B'] == 256 and kw['T'] == 16:
        assert torch.equal(sep[3], fus[3]), f'flat gradient: max |diff| {(sep[3] - fus[3]).abs().max().item():.3e}'
    else:
        close(fus[3], sep[3], 'flat gradient', rtol=1e-4)
    return sep[4]


@pytest.mark.parametrize('otype', ['pose_changes', 'relative_rot'])
@pytest.mark.parametrize('T', [5, 16])
def test_second_clip_of_a_workgroup_gets_the_tables_of_its_own_skeleton(monkeypatch, latency_form, otype, T):
    """B = 258 in the latency form: workgroups 0 and 1 walk clips (0, 256) and (1, 257). The clips of a workgroup are of
    DIFFERENT skeleton types (checked), so reference tables carried over from the first clip would show in the losses at once."""
    st = _same_as_separate(monkeypatch, B=258, T=T, missing=0.3, otype=otype)
    assert st[0] != st[256] and st[1] != st[257], 'the case checks nothing: a workgroup walks two clips of one skeleton type'
    assert len(set(st.tolist())) == 4


@pytest.mark.parametrize('B', [1, 9, 65])
def test_second_launch_with_few_clips(monkeypatch, B):
    """The contraction of train_wgrad_kernel, slice q = clips q, q + 8, ... dealt to eight waves: B = 1 (seven slices
    without a clip, one wave with one), B = 9 (two waves with a clip in slice 0, one in every other slice: fewer clips than waves),
    B = 65 (a second clip for wave 0 of slice 0: the non-unrolled tail loop runs twice). The optimizer is a launch of its own here."""
    _same_as_separate(monkeypatch, B=B, T=16, missing=0.3, otype='pose_changes')


def _four_steps(monkeypatch, fused, graph):
    monkeypatch.setenv('P2C_FUSED_TRAIN', fused)
    flow, dm = make(B=9, missing=0.3)
    trainer = _trainer(flow, dm, use_graph=graph)
    batch = dm.generate_batch(dev())
    for i in range(4):
        if i == 2:
            for grp in trainer.optimizers[0].param_groups:
                grp['lr'] *= 0.1
        trainer.train_step(flow, batch, i)
    torch.cuda.synchronize()
    assert (getattr(flow, '_pair_counts', None) is not None) == (fused == '1')
    st = trainer.optimizers[0].state[trainer.flat.flat_param]
    # (a capture whose update differs from the eager step's is dropped by the trainer, which then goes on eagerly)
    kept = bool(trainer.use_graph) and trainer._direct is not None
    return (trainer.flat.flat_param.detach().cpu().clone(), st['exp_avg'].cpu().clone(), st['exp_avg_sq'].cpu().clone(),
            float(st['step']), kept)


def test_step_count_behind_the_bias_corrections(monkeypatch):
    """B = 9 with AdamW inside the second launch (most workgroups have waves that contract nothing and read the step count only):
    four steps from a fresh optimizer, the learning rate cut after the second. The count ends at 4; parameters and both moments
    agree with the separate kernels (a count read too late or too early is a wrong bias correction: at step 1 the corrections
    are 10 and 1 000, an error of order one, not of 1e-4); the captured step -- kept by the trainer and replayed as its recorded
    two-launch call (checked: a capture that fails the trainer's own comparison is dropped for eager steps) -- gives the eager steps'
    parameters, bit for bit."""
    monkeypatch.delenv('P2C_FUSED_UPDATE', raising=False)
    monkeypatch.setenv('P2C_DIRECT_REPLAY', '1')
    sep = _four_steps(monkeypatch, '0', False)
    eager = _four_steps(monkeypatch, '1', False)
    replay = _four_steps(monkeypatch, '1', True)
    assert sep[3] == eager[3] == replay[3] == 4.0, (sep[3], eager[3], replay[3])
    assert replay[4] and not eager[4], 'the captured step was dropped for eager steps: the replay leg compares nothing'
    for a, b, what in zip(eager[:3], sep[:3], ('parameters', 'exp_avg', 'exp_avg_sq')):
        print(f'{what}: max |diff| {(a - b).abs().max().item():.3e} at scale {b.abs().max().item():.3e}')
    for a, b, what in zip(eager[:3], sep[:3], ('parameters', 'exp_avg', 'exp_avg_sq')):
        close(a, b, what, rtol=1e-4)
    assert torch.equal(replay[0], eager[0]), f'parameters: max |diff| {(replay[0] - eager[0]).abs().max().item():.3e}'
