"""GPU: the epoch loop -- exact resume from a checkpoint, validation that leaves training alone, the plateau scheduler reaching
the captured step, top-k checkpoints with ``test('best')`` on a live captured trainer, and a step whose launches are untouched.

Shapes: clip_length 16, batch_size 16, 3 steps per epoch, 3 epochs, 2 validation batches of 16 and 8 clips (the weighted epoch mean
differs from the plain one). Every comparison is bit for bit: the train step is run-to-run deterministic (``Trainer._verify_replay``
asserts bit equality of eager against replay); each resume case first runs the uninterrupted run twice and, should those two ever
differ, compares within twice their spread -- never within a margin taken from the resumed run.
"""
import contextlib
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

T, B, STEPS, EPOCHS = 16, 16, 3, 3


def dev():
    return torch.device('cuda:0')


def _dm():
    from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
    return SyntheticCarlaRecordedDataModule(clip_length=T, batch_size=B)


# a StepLR that halves the LR every epoch: the resumed run must pick up the scheduler's state and the captured step the new LR
_SCHED = dict(movements_lr=1e-3, movements_enable_lr_scheduler=True, movements_scheduler_type='StepLR',
              movements_scheduler_gamma=0.5, movements_scheduler_step_size=1)


def _linear_ae(**kw):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    model = LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, **kw)
    return LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')


def _seq2seq(**kw):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
    from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
    from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqEmbeddings
    model = Seq2SeqEmbeddings(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, movements_output_type=MT.pose_2d,
                              p_dropout=0.2, **kw)
    return LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox')


def _baseline(**kw):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.baseline_3d_pose import Baseline3DPose
    model = Baseline3DPose(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON, p_dropout=0.5, linear_size=128, **kw)
    return LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')


CASES = {
    'a_linear_ae_direct_replay': (_linear_ae, True),       # two launches, the optimizer inside the backward, replayed directly
    'b_linear_ae_eager': (_linear_ae, False),
    'c_seq2seq_dropout_captured': (_seq2seq, True),        # in-kernel dropout streams + philox sites, one captured graph
    'd_baseline_3d_pose_eager': (_baseline, False),        # BatchNorm running statistics + hashed dropout
}


def _state(flow, trainer):
    from pedestrians_video_2_carla_amd import checkpoint
    out = {f'param/{n}': p.detach().clone() for n, p in flow.named_parameters()}
    out.update({f'buffer/{n}': b.detach().clone() for n, b in flow.named_buffers()})
    (st,) = trainer.optimizers[0].state.values()
    out.update({f'optimizer/{k}': torch.as_tensor(st[k]).detach().clone() for k in ('exp_avg', 'exp_avg_sq', 'step')})
    out['lr'] = torch.tensor(trainer.optimizers[0].param_groups[0]['lr'], dtype=torch.float64)
    out.update({f'dropout/{n}': w for n, w in checkpoint.dropout_words(flow).items()})
    return out


@contextlib.contextmanager
def _recorded_losses(trainer):
    """A copy of every step's loss: a captured trainer hands back its one static loss tensor step after step. The wrapper is taken
    off again: left on, it would tie the trainer into a reference cycle and leave its GPU objects to the cyclic collector."""
    losses, step = [], trainer.train_step

    def train_step(flow, batch, batch_idx=0):
        loss = step(flow, batch, batch_idx)
        losses.append(loss.detach().clone())
        return loss
    trainer.train_step = train_step
    try:
        yield losses
    finally:
        del trainer.train_step


def _fit(case, epochs, seed=11, ckpt_dir=None, ckpt_path=None, validate=True, **flow_kw):
    from pedestrians_video_2_carla_amd.callbacks import ModelCheckpoint
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    make, graph = CASES[case]
    seed_everything(seed)
    flow, dm = make(**{**_SCHED, **flow_kw}), _dm()
    callbacks = [ModelCheckpoint(ckpt_dir, save_top_k=1)] if ckpt_dir is not None else []
    trainer = Trainer(device=dev(), use_graph=graph, max_epochs=epochs, steps_per_epoch=STEPS, callbacks=callbacks,
                      check_val_every_n_epoch=1 if validate else 1000)
    with _recorded_losses(trainer) as losses:
        trainer.fit(flow, dm, ckpt_path=ckpt_path)            # the data module's own train / validation batches
    torch.cuda.synchronize()
    assert trainer.use_graph == graph, 'the captured step fell back to eager steps'
    return flow, trainer, torch.stack(losses)


@functools.lru_cache(maxsize=None)
def _uninterrupted(case):
    """Run X, once per case for every test that needs it: (state, losses, monitors of the last validation)."""
    flow, trainer, losses = _fit(case, EPOCHS)
    assert (trainer.current_epoch, trainer.global_step) == (EPOCHS, EPOCHS * STEPS)
    return _state(flow, trainer), losses, dict(trainer.callback_metrics)


def _spread(a, b):
    return max(float((a[k].double() - b[k].double()).abs().max()) for k in a if a[k].numel())


@pytest.mark.parametrize('case', list(CASES))
def test_resume_is_exact(case, tmp_path):
    x_state, x_losses, _ = _uninterrupted(case)
    flow, trainer, again = _fit(case, EPOCHS)                            # X a second time: the margin, if there is to be one
    x2 = _state(flow, trainer)
    assert set(x2) == set(x_state)
    spread = max(_spread(x_state, x2), float((again - x_losses).abs().max()))
    print(f'{case}: X-to-X spread {spread:.3e}')
    if 'linear_ae' not in case:
        assert any(k.startswith('dropout/') for k in x_state), 'this case is meant to carry in-kernel dropout streams'
    if 'baseline' in case:
        assert any('running_mean' in k for k in x_state)

    # run Y: one epoch with a checkpoint, then a NEW flow (other initial weights) and trainer resume for the other two
    _flow1, trainer1, _ = _fit(case, 1, ckpt_dir=str(tmp_path / 'ckpt'))
    (ckpt,) = [os.path.join(tmp_path / 'ckpt', f) for f in os.listdir(tmp_path / 'ckpt')]
    flow2, trainer2, y_losses = _fit(case, EPOCHS, seed=12, ckpt_path=ckpt)
    assert (trainer2.current_epoch, trainer2.global_step) == (EPOCHS, EPOCHS * STEPS) and len(y_losses) == (EPOCHS - 1) * STEPS
    y_state = _state(flow2, trainer2)
    assert set(y_state) == set(x_state)
    tol = 2.0 * spread
    worst = max(((float((y_state[k].double() - x_state[k].double()).abs().max()), k) for k in x_state if x_state[k].numel()))
    assert worst[0] <= tol, f'{worst[1]} differs by {worst[0]:.3e} between the resumed and the uninterrupted run (margin {tol:.3e})'
    assert float((y_losses - x_losses[STEPS:]).abs().max()) <= tol, (y_losses, x_losses[STEPS:])
    if spread == 0.0:
        assert all(torch.equal(y_state[k], x_state[k]) for k in x_state) and torch.equal(y_losses, x_losses[STEPS:])


def test_resume_over_a_device_loader_restores_its_epoch(tmp_path):
    """An epoch is one pass over a sized re-iterable; a shuffling ``DeviceLoader`` orders epoch e by seed + e, so the resumed run
    must start its loader at the stored epoch to see the batches the uninterrupted run saw."""
    from pedestrians_video_2_carla_amd.callbacks import ModelCheckpoint
    from pedestrians_video_2_carla_amd.data.base.subset_io import save_subset
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    d, dm = dev(), _dm()
    _frames, targets, meta = dm.generate_batch(d, batch_size=3 * B + 5)
    path = save_subset(str(tmp_path), 'train', targets['projection_2d'].cpu().numpy(),
                       {'absolute_pose_loc': targets['absolute_pose_loc'].cpu().numpy()},
                       {'age': meta['age'], 'gender': meta['gender']}, prefer_hdf5=False)

    def run(epochs, seed, ckpt_dir=None, ckpt_path=None):
        seed_everything(seed)
        flow = _linear_ae(**_SCHED)
        loader = dm.get_dataloader(path, d, shuffle=True, seed=5)
        assert len(loader) == STEPS and loader.epoch == 0
        callbacks = [ModelCheckpoint(ckpt_dir, save_top_k=-1)] if ckpt_dir else []
        trainer = Trainer(device=d, use_graph=True, max_epochs=epochs, callbacks=callbacks)
        with _recorded_losses(trainer) as losses:
            trainer.fit(flow, dm, batches=loader, ckpt_path=ckpt_path)
        torch.cuda.synchronize()
        assert loader.epoch == epochs and trainer.global_step == epochs * STEPS
        return _state(flow, trainer), torch.stack(losses)
    x_state, x_losses = run(2, 11)
    run(1, 11, ckpt_dir=str(tmp_path / 'ckpt'))
    (ckpt,) = os.listdir(tmp_path / 'ckpt')
    y_state, y_losses = run(2, 12, ckpt_path=os.path.join(tmp_path / 'ckpt', ckpt))
    assert torch.equal(y_losses, x_losses[STEPS:]) and not torch.equal(x_losses[STEPS:], x_losses[:STEPS])
    for k in x_state:
        assert torch.equal(x_state[k], y_state[k]), k


@pytest.mark.parametrize('case', ['a_linear_ae_direct_replay', 'c_seq2seq_dropout_captured'])
def test_a_captured_trainer_is_released_by_reference_count(case, tmp_path):
    """Dropping the flow and the trainer releases them and the captured graph at once, with the cyclic collector off: no object
    of a finished run whose destructor calls the runtime (graph, streams, a loader's events and pinned buffers -- all owned by the
    trainer) is left for the collector to destroy inside a later trainer's open stream capture. (Not asserted: the optimizer of
    the two-launch step, which the step's autograd node keeps through its own output buffer; it holds device tensors only, and
    the allocator takes those back without a runtime call.)"""
    import gc
    import weakref
    gc.collect()
    gc.disable()
    try:
        flow, trainer, _ = _fit(case, 1, ckpt_dir=str(tmp_path / 'ckpt'))
        assert trainer._flow is flow and trainer._graphs is not None
        refs = [weakref.ref(o) for o in (trainer, flow, trainer._graphs[0])]
        del flow, trainer
        assert [r() for r in refs] == [None] * len(refs)
    finally:
        gc.enable()


def test_validation_leaves_training_alone():
    case = 'c_seq2seq_dropout_captured'
    with_val, _, monitors = _uninterrupted(case)
    assert 'val_loss/primary' in monitors
    flow, trainer, _ = _fit(case, EPOCHS, validate=False)
    assert trainer.callback_metrics == {}
    without = _state(flow, trainer)
    assert set(without) == set(with_val)
    for k in with_val:
        assert torch.equal(with_val[k], without[k]), f'{k} differs between the runs with and without validation'


def _plateau_flow():
    flow = _linear_ae()
    model = flow.movements_model              # (the closure holds the model, not the flow: no reference cycle through the flow)

    def configure_optimizers():
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-8)
        # min mode, relative threshold 0.9: "better" means below a tenth of the best value so far, which three epochs of
        # training do not reach -- the validation loss cannot improve, whatever the weights do
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode='min', factor=0.5, patience=0, threshold=0.9)
        return [{'optimizer': opt, 'lr_scheduler': {'scheduler': sched, 'interval': 'epoch', 'monitor': 'val_loss/primary'}}]
    flow.configure_optimizers = configure_optimizers
    return flow


def test_plateau_scheduler_steps_and_the_captured_step_follows(tmp_path):
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    d = dev()
    seed_everything(21)
    flow, dm = _plateau_flow(), _dm()
    seen = []

    class Watch:
        def on_validation_end(self, trainer, flow, monitors):
            seen.append((monitors['val_loss/primary'], trainer.optimizers[0].param_groups[0]['lr']))
    trainer = Trainer(device=d, use_graph=True, max_epochs=2, steps_per_epoch=STEPS, callbacks=[Watch()])
    trainer.fit(flow, dm)
    assert trainer.use_graph and len(seen) == 2
    assert seen[0][1] == 1e-3 and seen[1][1] == 5e-4                      # halved by the second validation
    assert trainer.optimizers[0].param_groups[0]['lr'] == 5e-4
    assert seen[1][0] != seen[0][0]                                       # (training did move the weights)
    path = trainer.save_checkpoint(str(tmp_path / 'epoch2.ckpt'))
    batch = dm.generate_batch(d, seed_offset=777)
    before = trainer.flat.flat_param.detach().clone()
    trainer.train_step(flow, batch, trainer.global_step)                  # replayed, at the new LR
    torch.cuda.synchronize()
    replayed = trainer.flat.flat_param.detach() - before
    # the same step issued eagerly from the same state: a fresh eager trainer that loaded the checkpoint (LR 5e-4 inside)
    seed_everything(22)
    twin = _plateau_flow()
    eager = Trainer(device=d, use_graph=False).setup(twin, dm)
    eager.load_checkpoint(path)
    assert eager.optimizers[0].param_groups[0]['lr'] == 5e-4 and torch.equal(eager.flat.flat_param, before)
    eager.train_step(twin, batch, eager.global_step)
    torch.cuda.synchronize()
    update = eager.flat.flat_param.detach() - before
    assert float(update.abs().max()) > 0 and torch.equal(replayed, update)
    # and the update is the one of LR 5e-4, not of 1e-3: Adam's step is proportional to the LR
    third = _plateau_flow()
    stale = Trainer(device=d, use_graph=False).setup(third, dm)
    stale.load_checkpoint(path)
    stale.optimizers[0].param_groups[0]['lr'] = 1e-3
    stale.train_step(third, batch, stale.global_step)
    torch.cuda.synchronize()
    assert not torch.equal(stale.flat.flat_param.detach() - before, update)


def test_top_k_and_test_best_on_a_live_captured_trainer(tmp_path):
    from pedestrians_video_2_carla_amd.callbacks import ModelCheckpoint
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    d = dev()
    seed_everything(31)
    flow, dm = _linear_ae(movements_lr=1e-3), _dm()
    seen = []

    class Watch:
        def on_validation_end(self, trainer, flow, monitors):
            seen.append(monitors['val_loss/primary'])
    cb = ModelCheckpoint(str(tmp_path / 'ckpt'), save_top_k=1)
    trainer = Trainer(device=d, use_graph=True, max_epochs=EPOCHS, steps_per_epoch=STEPS, callbacks=[Watch(), cb])
    trainer.fit(flow, dm)
    assert trainer.use_graph and len(seen) == EPOCHS
    assert os.listdir(tmp_path / 'ckpt') == [os.path.basename(cb.best_model_path)]
    assert cb.best_model_score == min(seen) and list(cb.best_k_models.values()) == [min(seen)]

    tests = dm.test_batches(d)
    live = trainer.test(flow, tests, ckpt_path='best')
    assert flow.training and 'test_loss/primary' in live
    seed_everything(32)
    fresh = LitPoseLiftingFlow.load_from_checkpoint(cb.best_model_path, transform='hips_neck_bbox')
    assert type(fresh.movements_model) is type(flow.movements_model)
    other = Trainer(device=d).setup(fresh, dm).test(fresh, tests)
    print('test_loss/primary', live['test_loss/primary'], other['test_loss/primary'])
    assert live['test_loss/primary'] == other['test_loss/primary']
    assert {k: v for k, v in live.items() if k.startswith('test_loss/')} == {k: v for k, v in other.items() if k.startswith('test_loss/')}

    # the captured step still works on the weights that were just written under it: one more replayed step against the same
    # step issued eagerly from the same state (the comparison of Trainer._verify_replay)
    state = trainer.flat.flat_param.data
    snapshot = trainer._snapshot(flow)
    before = state.clone()
    batch = dm.generate_batch(d, seed_offset=778)
    trainer.train_step(flow, batch, trainer.global_step)
    torch.cuda.synchronize()
    replayed = state - before
    trainer._restore(flow, snapshot)
    assert torch.equal(state, before)
    trainer._forward_backward(flow, batch, trainer.global_step)
    trainer._optimizer_step()
    torch.cuda.synchronize()
    want = state - before
    scale, diff = float(want.abs().max()), float((replayed - want).abs().max())
    print(f'replayed against eager update: diff {diff:.3e} of {scale:.3e}')
    assert scale > 0 and diff <= 0.05 * scale


@pytest.mark.skipif(os.environ.get('P2C_POISON_EMPTY') == '1' or os.environ.get('P2C_POISON_LDS') == '1',
                    reason='asserts the launch structure of the captured step; the audit modes add launches')
@pytest.mark.parametrize('case', ['a_linear_ae_direct_replay', 'c_seq2seq_dropout_captured'])
def test_the_step_is_untouched(case, tmp_path):
    from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything
    make, graph = CASES[case]
    d = dev()
    seed_everything(41)
    bare_flow, dm = make(**_SCHED), _dm()
    bare = Trainer(device=d, use_graph=graph).setup(bare_flow, dm)
    for i, batch in enumerate(dm.train_batches(d, STEPS + 1)):
        bare.train_step(bare_flow, batch, i)
    _flow, full, _ = _fit(case, 2, seed=41, ckpt_dir=str(tmp_path / 'ckpt'))

    def structure(trainer):
        plan = trainer._direct
        handover = plan.get('handover') if plan is not None else None
        return {'graph_nodes': trainer._graph_nodes,
                'captured_nodes': Trainer._count_nodes(trainer._graphs[0]) if trainer._kept_graph else None,
                'optimizer_graph': trainer._graphs[1], 'direct': plan is not None,
                'handover': None if handover is None else (handover['key2'], handover['key3'], handover['shapes']),
                'optimizer_in_backward': trainer._opt_in_backward, 'packed': len(trainer._packed)}
    assert structure(full) == structure(bare)
    if case.startswith('a_'):
        assert full._direct is not None and full._direct.get('handover') is not None     # the two-launch step, by address
