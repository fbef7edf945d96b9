"""GPU: the launcher, in process (``modeling.main([...])``): train writes a checkpoint, test reproduces the monitor stored with it,
predict writes a subset that ``load_subset`` reads back."""
import os

import pytest

pytestmark = pytest.mark.gpu

COMMON = ['--flow', 'pose_lifting', '--movements_model_name', 'LinearAE', '--loss_modes', 'loc_2d_3d',
          '--data_module_name', 'SyntheticCarlaRecorded', '--batch_size', '16', '--clip_length', '16', '--seed', '5']


def test_train_then_test_then_predict(tmp_path):
    from pedestrians_video_2_carla_amd import checkpoint
    from pedestrians_video_2_carla_amd.data.base.subset_io import load_subset
    from pedestrians_video_2_carla_amd.modeling import main
    logs = ['--logs_dir', str(tmp_path / 'runs')]
    log_dir, trainer = main(COMMON + logs + ['--mode', 'train', '--max_epochs', '2', '--limit_train_batches', '3'])
    assert (trainer.current_epoch, trainer.global_step) == (2, 6) and trainer.use_graph
    (name,) = os.listdir(os.path.join(log_dir, 'checkpoints'))
    path = os.path.join(log_dir, 'checkpoints', name)
    (cb,) = [c for c in trainer.callbacks if hasattr(c, 'best_model_path')]
    assert cb.best_model_path == path
    stored = checkpoint.read(path)
    assert stored['callbacks']['ModelCheckpoint']['best_model_score'] == cb.best_model_score
    assert stored['hyper_parameters']['movements_model_name'] == 'LinearAE'

    test_dir, tester = main(COMMON + logs + ['--mode', 'test', '--ckpt_path', path])
    assert test_dir != log_dir and tester.global_step == 0
    print('val_loss/primary', tester.callback_metrics['val_loss/primary'], cb.best_model_score)
    assert tester.callback_metrics['val_loss/primary'] == cb.best_model_score       # the same weights on the same batches
    assert 'test_loss/primary' in tester.callback_metrics and 'test/MPJPE' in tester.callback_metrics

    _, predictor = main(COMMON + logs + ['--mode', 'predict', '--ckpt_path', path, '--predict_sets', 'val'])
    out_dir = predictor.predictions['val']
    (subset,) = [f for f in os.listdir(out_dir) if f.startswith('val.')]
    projection_2d, targets, meta = load_subset(os.path.join(out_dir, subset))
    assert projection_2d.shape[:3] == (16 + 8, 16, 26) and 'absolute_pose_loc' in targets and len(meta['age']) == 24

    # a resumed run goes on from the stored epoch
    _, resumed = main(COMMON + logs + ['--mode', 'train', '--max_epochs', '3', '--limit_train_batches', '3', '--ckpt_path', path])
    assert resumed.current_epoch == 3 and resumed.global_step == 9
    # tune: the checkpoint's weights, nothing else of it -- a fresh optimizer and epoch count (and a video logger attached)
    _, tuned = main(COMMON + logs + ['--mode', 'tune', '--max_epochs', '1', '--limit_train_batches', '3', '--ckpt_path', path,
                                     '--renderers', 'input_points'])
    (state,) = tuned.optimizers[0].state.values()
    assert (tuned.current_epoch, tuned.global_step, float(state['step'])) == (1, 3, 3.0) and len(tuned.loggers) == 1
    with pytest.raises(ValueError):
        main(COMMON + logs + ['--mode', 'test'])
