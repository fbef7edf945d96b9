"""K39 (ops.smooth_carla_rows: one launch for bones and root) against its tensor definition on the device
(P2C_SMOOTH_FRAMEWORK=1), both modes.

    python tools/bench_smooth.py [N:T ...]        # default 1:64 256:16 4096:16 16:4096

J = 26, with root: bones (N,T,J,6), root (N,T,6) of smooth paths (a few degrees a frame plus jitter). ``gaussian`` with
sigma = 2, R = 6; ``one_euro`` at 30 fps with beta_loc = beta_rot = 0.5. Both arms get the same device tensors, and their results
are compared before timing (as rotation matrices, and the locations). Times are device events around windows of calls as an
export loop would issue them (launch gaps and the host's argument checks included: time per call, not kernel time), the two arms
alternating window by window; a window is sized to about a quarter of a second from a first timed pass (at least one call: the
tensor definition of ``one_euro`` issues some sixty small kernels per frame). The median window of each arm is reported with its
spread, and the bytes a call writes (24 per output row) and has to read (24 per source row, once) with the rate the K39 arm's
median makes of their sum. One JSON line per (mode, N, T).
"""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops

J, ROUNDS, WINDOW_US = 26, 7, 250e3
SHAPES = ((1, 64), (256, 16), (4096, 16), (16, 4096))
MODES = (dict(mode='gaussian', sigma=2.0, radius=6), dict(mode='one_euro', fps=30.0, beta_loc=0.5, beta_rot=0.5))
ARMS = (('k39', '0'), ('framework', '1'))
ENV = 'P2C_SMOOTH_FRAMEWORK'


def window(fn, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def alternate(fn):
    def armed(env):
        def run():
            os.environ[ENV] = env
            fn()
        return run
    calls = {name: armed(env) for name, env in ARMS}
    reps = {}
    for name, call in calls.items():                           # warm-up of every shape the windows use, and the window's size
        window(call, 1)
        reps[name] = max(1, min(2000, int(WINDOW_US / max(window(call, 3), 1.0))))
    times = {name: [] for name in calls}
    for _ in range(ROUNDS):
        for name, call in calls.items():
            times[name].append(window(call, reps[name]))
    os.environ[ENV] = '0'
    return {name: {'us_per_call': round(statistics.median(v), 2), 'min': round(min(v), 2), 'max': round(max(v), 2),
                   'calls_per_window': reps[name]} for name, v in times.items()}


def results(fn):
    out = {}
    for name, env in ARMS:
        os.environ[ENV] = env
        out[name] = [t.double().cpu() for t in fn()[:2]]
    os.environ[ENV] = '0'
    return out


def problem(N, T, device):
    """Rows whose angles drift by up to 2 degrees a frame with half a degree of jitter, pitch inside +-80 degrees."""
    g = torch.Generator().manual_seed(5)

    def make(*lead):
        start = (torch.rand(*lead[:1], 1, *lead[2:], 3, generator=g) * 2 - 1) * torch.tensor([40.0, 180.0, 180.0])
        drift = torch.cumsum((torch.rand(*lead, 3, generator=g) * 2 - 1) * 2.0, 1)
        drift[..., 0] = 40.0 * torch.sin(drift[..., 0] * (math.pi / 180.0))
        angles = start + drift + 0.5 * torch.randn(*lead, 3, generator=g)
        angles[..., 1:] = torch.remainder(angles[..., 1:] + 180.0, 360.0) - 180.0
        loc = torch.randn(*lead[:1], 1, *lead[2:], 3, generator=g) + torch.cumsum(0.02 * torch.randn(*lead, 3, generator=g), 1)
        return torch.cat((loc, angles), -1).to(device)
    return make(N, T, J), make(N, T)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_smooth.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    shapes = [tuple(int(v) for v in a.split(':')) for a in sys.argv[1:]] or SHAPES
    for N, T in shapes:
        bones, root = problem(N, T, device)
        for kw in MODES:
            call = lambda: ops.smooth_carla_rows(bones, root, **kw)          # noqa: E731
            got = results(call)
            agree = {'matrix_entries': max(float((ops.carla_pose_import(a.reshape(-1, 1, 6))[1]
                                                  - ops.carla_pose_import(b.reshape(-1, 1, 6))[1]).abs().max())
                                           for a, b in zip(got['k39'], got['framework'])),
                     'locations': max(float((a[..., :3] - b[..., :3]).abs().max()) for a, b in zip(got['k39'], got['framework']))}
            moved = 2 * N * T * (J + 1) * 24
            res = {'mode': kw['mode'], 'N': N, 'T': T, 'J': J, 'frames': N * T, 'arms_differ_by': agree,
                   'bytes_read_once_and_written': moved, **alternate(call)}
            res['k39_GB_per_s'] = round(moved / res['k39']['us_per_call'] / 1e3, 1)
            res['k39_share_of_8TB_per_s'] = round(moved / res['k39']['us_per_call'] / 1e3 / 8000.0, 4)
            res['framework_over_k39'] = round(res['framework']['us_per_call'] / res['k39']['us_per_call'], 1)
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
