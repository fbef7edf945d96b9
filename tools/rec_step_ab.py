"""Developer tool: the one-launch-per-step recurrences (K18, K23) under two builds of the library -- the same bits? the same time?

  P2C_LIB_PATH=build/A/libp2c_hip.so python tools/rec_step_ab.py dump a.pt      # one fresh process per library: the path is
  P2C_LIB_PATH=build/B/libp2c_hip.so python tools/rec_step_ab.py dump b.pt      # read when the package is imported
  python tools/rec_step_ab.py compare a.pt b.pt outputs_equal.txt               # (no GPU) exit status 1 if any tensor differs
  P2C_LIB_PATH=... python tools/rec_step_ab.py time layer_ms.jsonl              # device ms of one layer, forward + backward

``dump`` runs ops.lstm_layer and ops.gru_layer forward + backward for every entry of CASES of tests/test_lstm_model_gpu.py and
tests/test_gru_gpu.py, with and without an initial state, from fixed seeds, and saves every output and every gradient. ``time``
takes shapes whose steps the device bounds, not the host: median over ROUNDS of the device-event time of STEPS eager calls.
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import torch  # noqa: E402

TIMED = [(15, 256, 52, 256), (15, 256, 52, 512), (15, 2048, 52, 191)]      # (T, B, I, H)
ROUNDS, STEPS = 7, 20


def layer(cell, T, B, I, H, with_state, d):
    """The inputs of one layer from a fixed seed, and a function that runs it forward + backward and returns what it produced."""
    from pedestrians_video_2_carla_amd import ops
    G = 4 if cell == 'lstm' else 3
    g = torch.Generator().manual_seed(T * 1000 + B + H)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).to(d).requires_grad_(True)
    x, w_ih, w_hh, b_ih, b_hh = rnd(T, B, I), rnd(G * H, I, scale=H ** -0.5), rnd(G * H, H, scale=H ** -0.5), rnd(G * H), rnd(G * H)
    state = [rnd(B, H) for _ in range(G - 2)] if with_state else [None] * (G - 2)       # (h0, c0) / (h0)
    ups = [rnd(T, B, H).detach()] + [rnd(B, H).detach() for _ in range(G - 2)]          # for (out, hT, cT) / (out, hT)
    leaves = dict(g_x=x, g_w_ih=w_ih, g_w_hh=w_hh, g_b_ih=b_ih, g_b_hh=b_hh, **dict(zip(('g_h0', 'g_c0'), state if with_state else [])))

    def step():
        for v in leaves.values():
            v.grad = None
        outs = getattr(ops, cell + '_layer')(x, *state, w_ih, w_hh, b_ih, b_hh)
        sum((o * u).sum() for o, u in zip(outs, ups)).backward()
        return dict(zip(('out', 'hT', 'cT'), outs), **{k: v.grad for k, v in leaves.items()})
    return step


def timed(step, d):
    ms = []
    for _ in range(ROUNDS + 1):                                 # (the first round warms up)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(STEPS):
            step()
        end.record()
        torch.cuda.synchronize(d)
        ms.append(start.elapsed_time(end) / STEPS)
    return ms[1:]


def main():
    mode = sys.argv[1]
    if mode == 'dump':
        from test_gru_gpu import CASES as GRU_CASES
        from test_lstm_model_gpu import CASES as LSTM_CASES
        d, saved = torch.device('cuda:0'), {}
        for cell, cases in (('lstm', LSTM_CASES), ('gru', GRU_CASES)):
            for T, B, I, H in cases:
                for with_state in (False, True):
                    got = layer(cell, T, B, I, H, with_state, d)()
                    saved.update({f'{cell} T={T} B={B} I={I} H={H} state={int(with_state)} {k}': v.detach().cpu() for k, v in got.items()})
        torch.save(saved, sys.argv[2])
        print(f'{len(saved)} tensors -> {sys.argv[2]}')
        return 0
    if mode == 'time':
        d = torch.device('cuda:0')
        with open(sys.argv[2], 'w') as out:
            for cell in ('lstm', 'gru'):
                for T, B, I, H in TIMED:
                    ms = timed(layer(cell, T, B, I, H, True, d), d)
                    line = json.dumps(dict(cell=cell, T=T, B=B, I=I, H=H, ms=round(statistics.median(ms), 4), rounds_ms=[round(v, 4) for v in ms]))
                    print(line, flush=True)
                    out.write(line + '\n')
        return 0
    a, b = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    assert list(a) == list(b) and a, 'the two dumps hold different cases'
    lines = [f'{k} {tuple(a[k].shape)} equal {torch.equal(a[k], b[k])} max|diff| {float((a[k] - b[k]).abs().max()) if a[k].numel() else 0.0}'
             for k in a]
    with open(sys.argv[4], 'w') as f:
        f.write('\n'.join(lines) + '\n')
    bad = [ln for ln in lines if ' equal False ' in ln]
    print(f'{len(lines) - len(bad)} of {len(lines)} tensors equal' + ''.join('\n' + ln for ln in bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
