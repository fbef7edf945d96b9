"""CPU: the launcher's parser and registries (the runs themselves are in test_launcher_gpu.py)."""
import pytest


def test_parser_is_assembled_from_the_chosen_classes():
    from pedestrians_video_2_carla_amd.loss import LossModes
    from pedestrians_video_2_carla_amd.modeling import build_parser, data_modules, flow_modules
    assert set(flow_modules()) == {'pose_lifting', 'autoencoder', 'classification', 'pose_estimation'}
    assert {'SyntheticCarlaRecorded', 'JAADCarlaRec', 'CarlaRecAMASS', 'JAADCarlaRecAMASS'} <= set(data_modules())
    argv = ['--flow', 'pose_lifting', '--movements_model_name', 'Baseline3DPose', '--linear_size', '128', '--loss_modes', 'loc_3d',
            '--mode', 'tune', '--max_epochs', '4', '--limit_train_batches', '3', '--gradient_clip_val', '0.5',
            '--movements_lr', '0.01', '--ckpt_path', 'x.ckpt', '--predict_sets', 'val', 'test']
    parser, dm_cls, flow_cls, models = build_parser(argv)
    args = parser.parse_args(argv)
    assert flow_cls is flow_modules()['pose_lifting'] and dm_cls is data_modules()['SyntheticCarlaRecorded']
    assert models['movements'].__name__ == 'Baseline3DPose' and models['trajectory'].__name__ == 'ZeroTrajectory'
    assert (args.mode, args.max_epochs, args.limit_train_batches, args.linear_size) == ('tune', 4, 3, 128)
    assert args.loss_modes == [LossModes.loc_3d] and args.gradient_clip_val == 0.5 and args.movements_lr == 0.01
    assert args.predict_sets == ['val', 'test'] and args.check_val_every_n_epoch == 1 and args.max_steps == -1
    # a model's own flags are only there when that model is chosen
    parser, _, _, models = build_parser(['--flow', 'autoencoder'])
    assert models['movements'].__name__ == 'Seq2SeqEmbeddings'
    with pytest.raises(SystemExit):
        parser.parse_args(['--flow', 'autoencoder', '--linear_size', '128'])


def test_modes_that_need_a_checkpoint_say_so(tmp_path):
    from pedestrians_video_2_carla_amd.modeling import main
    with pytest.raises(ValueError, match='--ckpt_path'):
        main(['--mode', 'test', '--logs_dir', str(tmp_path)])
    with pytest.raises(ValueError, match='does not exist'):
        main(['--mode', 'test', '--logs_dir', str(tmp_path), '--ckpt_path', str(tmp_path / 'none.ckpt')])
    with pytest.raises(ValueError, match='max_epochs'):
        main(['--mode', 'train', '--logs_dir', str(tmp_path)])
