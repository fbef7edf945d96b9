"""cfg3 timing: autoencoder flow, Seq2SeqEmbeddings(pose_2d), B=512, T=16 -- eager train steps (MIOpen LSTM + HIP loss).
usage: bench_seq2seq.py [B=512] [steps=30] [graph|eager] [autoencoder|lifting]
  lifting: LitPoseLiftingFlow + Seq2SeqEmbeddings(pose_changes, O = 156) + loc_2d_3d -- the decoder loop of K7c's 64 < O <= 160 kernels;
  P2C_DECODER_WIDE=1 in the environment puts the decoder on those kernels; unset or 0 times the same step on the per-step path."""
import os, sys, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from pedestrians_video_2_carla_amd.data.carla.skeleton import CARLA_SKELETON
from pedestrians_video_2_carla_amd.data.carla.carla_recorded_synthetic import SyntheticCarlaRecordedDataModule
from pedestrians_video_2_carla_amd.modules.flow.autoencoder import LitAutoencoderFlow
from pedestrians_video_2_carla_amd.modules.flow.output_types import MovementsModelOutputType as MT
from pedestrians_video_2_carla_amd.modules.flow.pose_lifting import LitPoseLiftingFlow
from pedestrians_video_2_carla_amd.modules.movements.seq2seq import Seq2SeqEmbeddings
from pedestrians_video_2_carla_amd.trainer import Trainer, seed_everything

B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
use_graph = len(sys.argv) > 3 and sys.argv[3] == 'graph'
lifting = len(sys.argv) > 4 and sys.argv[4] == 'lifting'
if os.environ.get('P2C_BLAS'):
    torch.backends.cuda.preferred_blas_library(os.environ['P2C_BLAS'])
d = torch.device('cuda:0')
seed_everything(22742)
dm = SyntheticCarlaRecordedDataModule(clip_length=16, batch_size=B)
model = Seq2SeqEmbeddings(input_nodes=CARLA_SKELETON, output_nodes=CARLA_SKELETON,
                          movements_output_type=MT.pose_changes if lifting else MT.pose_2d)
if os.environ.get('P2C_NO_FOLD'):
    model.fold_embeddings = False
if lifting:
    flow = LitPoseLiftingFlow(movements_model=model, loss_modes=['loc_2d_3d'], transform=dm.transform.name)
else:
    flow = LitAutoencoderFlow(movements_model=model, loss_modes=['loc_2d'], transform='hips_neck_bbox')
trainer = Trainer(device=d, use_graph=use_graph).setup(flow, dm)
batch = dm.generate_batch(d)
first = []
for i in range(5):
    first.append(float(trainer.train_step(flow, batch, i)))
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(steps):
    loss = trainer.train_step(flow, batch, i)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / steps
config = 'pose lifting Seq2SeqEmbeddings pose_changes' if lifting else 'autoencoder Seq2SeqEmbeddings pose_2d'
if lifting:
    config += ' decoder=' + ('fused' if model._decoder_loop_fusable(batch[0]) else 'per-step')
print(json.dumps({'config': config, 'B': B, 'hip_graph': use_graph, 'ms_per_step': round(dt * 1e3, 3),
                  'clips_per_s': round(B / dt, 1), 'loss': float(loss), 'first_losses': first}))
