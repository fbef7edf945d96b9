"""K37 (ops.resample_carla_rows: one launch for bones and root) against its tensor definition on the device
(P2C_RESAMPLE_FRAMEWORK=1).

    python tools/bench_resample.py [N ...]        # videos per batch, default 256 4096 (T = 16: 4 096 and 65 536 frames)

T = 16, J = 26, with root: bones (N,T,J,6), root (N,T,6) at 30 fps -> 20 fps (decimating: every second output is a copy) and
-> 120 fps (upsampling: neighbouring outputs re-read the same source rows). Both arms get the same device tensors, and their
results are compared before timing (as rotation matrices, and the locations). Times are device events around windows of calls as
an export loop would issue them (launch gaps and the host's argument checks included: time per call, not kernel time), the two
arms alternating window by window; a window is sized to about a quarter of a second from a first timed pass. The median window of
each arm is reported with its spread, and the bytes a call writes (24 per output row) and has to read (24 per source row, once)
with the rate the K37 arm's median makes of the bytes written. One JSON line per (N, rate pair).
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pedestrians_video_2_carla_amd import ops

T, J, ROUNDS, WINDOW_US = 16, 26, 7, 250e3
RATES = ((30.0, 20.0), (30.0, 120.0))
ARMS = (('k37', '0'), ('framework', '1'))
ENV = 'P2C_RESAMPLE_FRAMEWORK'


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
        window(call, 3)
        reps[name] = max(5, min(2000, int(WINDOW_US / max(window(call, 10), 1.0))))
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
        out[name] = [t.double().cpu() for t in fn()]
    os.environ[ENV] = '0'
    return out


def problem(N, device):
    g = torch.Generator().manual_seed(5)

    def make(*lead):
        loc = torch.randn(*lead, 3, generator=g)
        u = torch.rand(*lead, 3, generator=g) * 2 - 1
        return torch.cat((loc, u * torch.tensor([89.0, 180.0, 180.0])), -1).to(device)
    return make(N, T, J), make(N, T)


def main():
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample.py times device work: it needs the MI355X (there is nothing to fall back to)')
    device = torch.device('cuda:0')
    for N in [int(a) for a in sys.argv[1:]] or [256, 4096]:
        bones, root = problem(N, device)
        for src, dst in RATES:
            call = lambda: ops.resample_carla_rows(bones, root, src_fps=src, dst_fps=dst)          # noqa: E731
            got = results(call)
            K = got['k37'][0].shape[1]
            agree = {'matrix_entries': max(float((ops.carla_pose_import(a.reshape(-1, 1, 6))[1]
                                                  - ops.carla_pose_import(b.reshape(-1, 1, 6))[1]).abs().max())
                                           for a, b in zip(got['k37'], got['framework'])),
                     'locations': max(float((a[..., :3] - b[..., :3]).abs().max()) for a, b in zip(got['k37'], got['framework']))}
            written, read = N * K * (J + 1) * 24, N * T * (J + 1) * 24
            res = {'N': N, 'T': T, 'J': J, 'frames': N * T, 'src_fps': src, 'dst_fps': dst, 'outputs_per_video': K,
                   'arms_differ_by': agree, 'bytes_written': written, 'bytes_read_once': read, **alternate(call)}
            res['k37_written_GB_per_s'] = round(written / res['k37']['us_per_call'] / 1e3, 1)
            res['k37_share_of_8TB_per_s'] = round(written / res['k37']['us_per_call'] / 1e3 / 8000.0, 4)
            print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
