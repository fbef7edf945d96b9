"""GPU: the factor block of train_clip_kernel (csrc/p2c_train.hip) when its segments leave LDS early -- each from waves that idle
behind the barrier that published it (G_6 and the H half beside dgrad step 5, G_5 beside step 4, G_4 beside steps 3 -> 2, G_3 and
G_2 beside step 1, only G_1 at the end), write-through. The layout, every arithmetic instruction and every summation order are the
parent's; what the placement can break is WHICH bytes a store picks up: a segment read before its publishing barrier, a G row read
while scan plane 1 still aliases it, a read of clip i that the barrier at the top of clip i + 1 does not cover, an item dropped or
stored twice by the per-site flat index. Every factor row enters dW, so each of these is wrong bits in the gradient.

All cases run the latency form (train_clip_kernel at every batch size), forced as tests/test_step_prologue_gpu.py does."""
import ctypes
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(1, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (this file also runs as a script)
from test_flow_gpu import dev  # noqa: E402
from test_step_prologue_gpu import latency_form  # noqa: E402,F401
from test_clip_tail_gpu import F_ROWS, SEGMENTS, SLICE_FLOATS, TICKET_FLOATS, _both_paths, _check, _inputs  # noqa: E402

H_ROWS = SEGMENTS[6]                           # 214: H_0 .. H_5 | G_1 .. G_6


CASES = [(B, T, otype) for B in (1, 255, 257, 513) for T in (1, 15, 16) for otype in ('pose_changes', 'relative_rot')]


def _separate_kernels(inp):
    """(loss vector, flat gradient) of the separate kernels (mlp_fwd + pose head + mlp_bwd, loc_2d_3d) on the inputs of
    tests/test_clip_tail_gpu.py, with their weight gradient summed in the order of the two-launch step. That order is theirs where
    (a) they run the split weight gradient (factors out of mlp_bwd, mlp_wgrad_kernel over slices of eight sample tiles,
    mlp_reduce_small_kernel in slice order: csrc/p2c_mlp.hip, split_wgrad(); by itself only for 0.75 - 1.5 sample tiles per CU,
    P2C_MLP_WGRAD=split for every batch, read once per process) and (b) a sample tile is a clip. The fused step's tile IS the clip:
    T frames and 16 - T all-zero ones, whose output gradient is zero. For T < 16 the separate kernels get the same rows: every clip
    padded to sixteen frames with zero frames, the pose head on the first T of them (the slice's backward hands mlp_bwd exact
    zeros for the rest). The frames' forward is per sample, the padded samples add +-0 to every sum: nothing but the order moves."""
    from pedestrians_video_2_carla_amd import ops
    assert os.environ.get('P2C_MLP_WGRAD') == 'split', 'the reference needs the split weight gradient (child process)'
    spec = ops.PoseHeadSpec(kind=inp['kind'], transform=inp['transform'])
    frames = inp['frames']
    B, T = frames.shape[:2]
    n = len(inp['params']) // 2
    params = [p.clone().requires_grad_(True) for p in inp['params']]
    padded = torch.zeros(B, 16, *frames.shape[2:], device=frames.device)
    padded[:, :T] = frames
    with ops.deferred_loss_finalize(2):
        y = ops.fused_mlp(padded.reshape(B * 16, -1), params[:n], params[n:]).view(B, 16, 26, 6)
        losses, _ = ops.pose_head(y[:, :T].contiguous(), spec, inp['st'], None, None, inp['gt2d'], inp['gt3d'])
        losses['loc_2d_3d'].backward()
    torch.cuda.synchronize()
    return losses.vector.detach().cpu().clone(), torch.cat([p.grad.reshape(-1) for p in params]).cpu()


def _two_launch_step(inp):
    """(loss vector, flat gradient) of the two-launch step on the same inputs."""
    from pedestrians_video_2_carla_amd import ops
    spec = ops.PoseHeadSpec(kind=inp['kind'], transform=inp['transform'])
    n = len(inp['params']) // 2
    params = [p.clone().requires_grad_(True) for p in inp['params']]
    with ops.deferred_loss_finalize(2):
        counts = ops.count_target_pairs(spec, inp['gt2d'])
        losses = ops.fused_train_step(inp['frames'], params[:n], params[n:], spec, inp['st'], counts, gt2d=inp['gt2d'], gt3d=inp['gt3d'])
        losses['loc_2d_3d'].backward()
    torch.cuda.synchronize()
    return losses.vector.detach().cpu().clone(), torch.cat([p.grad.reshape(-1) for p in params]).cpu()


@pytest.fixture(scope='module')
def separate_reference():
    """The separate kernels' losses and gradients of all 24 cases, computed ONCE in a child process (P2C_MLP_WGRAD is read once
    per process) by this file run as a script."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'separate.pt')
        res = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, P2C_MLP_WGRAD='split'),
                             capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        return torch.load(out)


@pytest.mark.parametrize('B,T,otype', CASES)
def test_two_launch_step_is_the_separate_kernels_bit_for_bit(latency_form, separate_reference, B, T, otype):
    """Losses and flat gradient of the two-launch step against the separate kernels (mlp_fwd + pose head + mlp_bwd), bit for bit.
    B = 1, 255, 257, 513: one, one, two and three clips on workgroup 0 (the persistent loop's barrier in front of clip i + 1);
    T = 1 leaves seven waves without a frame that still carry stores; both 6-D kinds. The separate kernels run as
    `_separate_kernels` says, so that their fp32 sums are taken in the two-launch step's order (as they come, with another
    weight-gradient form at B = 1 and 513 and other sample tiles at T < 16, their gradient differs from it in the last bits, up to
    2.4e-7 of its scale, for the parent commit's library as for this one: profiles/k13_handoff, README 5)."""
    sep = separate_reference[f'{B}-{T}-{otype}']
    fus = _two_launch_step(_inputs(B, T, otype=otype))
    diff, scale = (sep[1] - fus[1]).abs().max().item(), sep[1].abs().max().item()
    print(f'B={B} T={T} {otype}: losses {fus[0].tolist()} (separate {sep[0].tolist()}), flat gradient max |diff| {diff:.3e} at '
          f'scale {scale:.3e}, {int((sep[1] != fus[1]).sum())} of {sep[1].numel()} elements differ')
    assert torch.isfinite(sep[0]).all() and torch.isfinite(sep[1]).all() and torch.isfinite(fus[1]).all() and sep[1].abs().max() > 0
    assert torch.equal(sep[0], fus[0]), f'losses {fus[0].tolist()} vs {sep[0].tolist()}'
    assert torch.equal(sep[1], fus[1]), f'flat gradient: max |diff| {diff:.3e} at scale {scale:.3e}'


class _FirstLaunch:
    """p2c_train_step_launch (which = 1) on the inputs of tests/test_clip_tail_gpu.py into a workspace full of NaN."""

    def __init__(self, inp):
        from pedestrians_video_2_carla_amd import _lib, ops
        self.lib, self._lib = _lib.lib(), _lib
        B = inp['frames'].shape[0]
        spec = ops.PoseHeadSpec(kind=inp['kind'], transform=inp['transform'])
        n = len(inp['params']) // 2
        weights, biases = inp['params'][:n], inp['params'][n:]
        f32 = dict(dtype=torch.float32, device=dev())
        self.bufs = {'partials': torch.empty(B * 4, **f32), 'loss_sums': torch.empty(4, **f32), 'losses': torch.empty(3, **f32)}
        self.gws, self.gbs = [torch.full_like(w, float('nan')) for w in weights], [torch.full_like(b, float('nan')) for b in biases]
        counts = ops.count_target_pairs(spec, inp['gt2d'])
        self.desc, self.keep = ops.train_step_desc(inp['frames'], spec, inp['st'], None, None, inp['gt2d'], inp['gt3d'], counts, weights,
                                                   biases, self.gws, self.gbs, self.bufs)
        self.ws, self.B = self.keep[2], B
        assert self.ws.numel() == B * F_ROWS * 16 + SLICE_FLOATS + TICKET_FLOATS
        self.ws.fill_(float('nan'))
        self.gl = torch.tensor([0.0, 0.0, 1.0], **f32)
        self.launch(1)

    def launch(self, which):
        glp = self._lib.grad_loss_pointers(vector=self.gl.data_ptr())
        self._lib.check(self.lib.p2c_train_step_launch(ctypes.byref(self.desc), glp, which, torch.cuda.current_stream().cuda_stream),
                        f'launch {which}')
        torch.cuda.synchronize()

    def block(self):
        return self.ws[:self.B * F_ROWS * 16].view(self.B, F_ROWS, 16).cpu()


@pytest.mark.parametrize('T', [1, 15])
def test_every_segment_arrives_whole_with_three_clips_per_workgroup(latency_form, T):
    """B = 513, T = 1 and 15 (cells tests/test_clip_tail_gpu.py does not have): no NaN inside [0, B 532 16), the four floats behind
    the last block untouched, H_0 and G_1 .. G_6 exactly zero in the sample columns >= T. Workgroup 0 stores clips 0, 256 and 512:
    a site that keeps the first clip's block address, or a round that runs past its segment, leaves NaN or clobbers a neighbour.
    The second launch alone on this early-stored block then gives the separate kernels' gradient."""
    B = 513
    inp = _inputs(B, T)
    run = _FirstLaunch(inp)
    block = run.block()
    holes = torch.isnan(block)
    print(f'B={B} T={T}: {int(holes.sum())} NaN in the block, per segment',
          [int(holes[:, a:b].sum()) for a, b in zip(SEGMENTS[:-1], SEGMENTS[1:])])
    assert not holes.any(), f'{int(holes.sum())} floats of the factor block were not written'
    assert torch.isfinite(block).all()
    assert torch.isnan(run.ws[B * F_ROWS * 16:B * F_ROWS * 16 + 4].cpu()).all(), 'a float behind the last block was written'
    assert (block[:, :SEGMENTS[1], T:] == 0).all(), 'H_0: sample columns beyond the clip are not zero'
    assert (block[:, H_ROWS:, T:] == 0).all(), 'G_l: sample columns beyond the clip are not zero'
    assert block[:, :SEGMENTS[1], :T].abs().max() > 0 and block[:, SEGMENTS[11]:, :T].abs().max() > 0     # H_0 = x^T, G_6 = grad_y^T
    run.launch(2)
    flat = torch.cat([g.reshape(-1) for g in run.gws] + [g.reshape(-1) for g in run.gbs]).cpu()
    sep, _ = _both_paths(inp)
    _check(sep, (run.bufs['losses'].cpu(), flat), f'second launch alone, B={B} T={T}')


def test_first_launch_gives_the_same_bits_twice(latency_form):
    """B = 257, T = 16: the first launch twice, each into a fresh workspace full of NaN. A store that races the barrier which
    publishes its rows picks up whatever the chain waves have written by then, and that differs from run to run."""
    inp = _inputs(257, 16)
    a, b = _FirstLaunch(inp), _FirstLaunch(inp)
    assert a.ws.data_ptr() != b.ws.data_ptr()
    ba, bb = a.block(), b.block()
    assert not torch.isnan(ba).any() and not torch.isnan(bb).any()
    differ = ba.view(torch.int32) != bb.view(torch.int32)
    print(f'{int(differ.sum())} of {ba.numel()} floats differ between the two runs')
    assert not differ.any(), f'{int(differ.sum())} floats differ, first at {differ.nonzero()[0].tolist()}'
    assert torch.equal(a.bufs['partials'].cpu().view(torch.int32), b.bufs['partials'].cpu().view(torch.int32))


if __name__ == '__main__':      # the child of `separate_reference`: the separate kernels of every case -> sys.argv[1]
    torch.save({f'{B}-{T}-{otype}': _separate_kernels(_inputs(B, T, otype=otype)) for B, T, otype in CASES}, sys.argv[1])
