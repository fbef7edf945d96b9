"""Checkpoints under data-parallel training on CPU (world_size 2, gloo): rank 0 writes ONE file, every rank reads it, and the ranks
hold the same parameters and optimizer state after resuming from it."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

STEPS = 2


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _make_flow(seed=22742):
    from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
    from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
    from pedestrians_video_2_carla_amd.modules.movements.linear_ae import LinearAE
    from pedestrians_video_2_carla_amd.trainer import seed_everything
    seed_everything(seed)
    model = LinearAE(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON)
    return LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform='hips_neck_bbox')


def _shard(batch, rank, world):
    frames, targets, meta = batch
    n = len(frames) // world
    sl = slice(rank * n, (rank + 1) * n)
    return frames[sl], {k: v[sl] for k, v in targets.items()}, {k: v[sl] for k, v in meta.items()}


def _worker(rank, world, port, out_dir):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from cpu_backend import StubDataModule, batch_from_oracle, oracle_backend
    from pedestrians_video_2_carla_amd.trainer import Trainer, init_distributed
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR='127.0.0.1',
                      MASTER_PORT=str(port))
    torch.set_num_threads(2)
    init_distributed('gloo')
    ckpt_dir = os.path.join(out_dir, 'ckpt')
    path = os.path.join(ckpt_dir, 'step2.ckpt')
    flow = _make_flow()
    trainer = Trainer(max_steps=STEPS).setup(flow, StubDataModule())
    with oracle_backend():
        for step in range(STEPS):
            trainer.train_step(flow, _shard(batch_from_oracle(8, seed=100 + step, missing=0.1), rank, world), step)
        trainer.save_checkpoint(path)                       # every rank calls it; behind its barrier the file is complete
        assert os.listdir(ckpt_dir) == ['step2.ckpt'], os.listdir(ckpt_dir)
        # a NEW flow and trainer on every rank, with weights of its own before the load
        fresh = _make_flow(seed=1000 + rank)
        resumed = Trainer(max_steps=STEPS + 1)
        batch = _shard(batch_from_oracle(8, seed=100 + STEPS, missing=0.1), rank, world)
        losses = resumed.fit(fresh, StubDataModule(), batches=[batch], ckpt_path=path)
        # the uninterrupted run takes the same third step
        trainer.train_step(flow, batch, STEPS)
    assert len(losses) == 1 and resumed.global_step == STEPS + 1
    (state,) = resumed.optimizers[0].state.values()
    (state_x,) = trainer.optimizers[0].state.values()
    torch.save({'param': resumed.flat.flat_param.detach().clone(), 'uninterrupted': trainer.flat.flat_param.detach().clone(),
                'state': {k: torch.as_tensor(v).detach().clone() for k, v in state.items()},
                'state_uninterrupted': {k: torch.as_tensor(v).detach().clone() for k, v in state_x.items()}},
               os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_rank_0_writes_one_file_and_both_ranks_resume_equal(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert os.listdir(tmp_path / 'ckpt') == ['step2.ckpt']
    r0, r1 = (torch.load(os.path.join(tmp_path, f'rank{r}.pt')) for r in range(world))
    assert torch.equal(r0['param'], r1['param']), 'ranks diverged after resuming'
    assert set(r0['state']) == set(r1['state']) == {'step', 'exp_avg', 'exp_avg_sq'}
    for k in r0['state']:
        assert torch.equal(r0['state'][k], r1['state'][k]), k
        assert torch.equal(r0['state'][k], r0['state_uninterrupted'][k]), k     # and resuming changed nothing
    assert float(r0['state']['step']) == STEPS + 1
    assert torch.equal(r0['param'], r0['uninterrupted'])
