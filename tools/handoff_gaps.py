"""Gaps at the two kernel boundaries of the two-launch train step, from a rocprofv3 --kernel-trace CSV of a bench.py run.

    rocprofv3 --kernel-trace --output-format csv -d OUT -- python bench.py --gpus 1 --steps 200 --warmup 20
    python tools/handoff_gaps.py OUT/**/*kernel_trace.csv

clip -> wgrad: train_clip_kernel's end to train_wgrad_kernel's start (the predecessor leaves the factor blocks, 8.7 MB at B = 256).
wgrad -> clip: train_wgrad_kernel's end to the next step's train_clip_kernel start (the predecessor leaves under 0.4 MB).
Printed: count, p10 / p50 / p90 in microseconds for both, the kernels' own durations, and the difference of the two medians."""
import csv
import statistics
import sys


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, int(q * len(v)))]


def main(path):
    rows = [r for r in csv.DictReader(open(path)) if 'train_clip_kernel' in r['Kernel_Name'] or 'train_wgrad_kernel' in r['Kernel_Name']]
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    gaps = {'clip->wgrad': [], 'wgrad->clip': []}
    dur = {'train_clip_kernel': [], 'train_wgrad_kernel': []}
    for a, b in zip(rows, rows[1:]):
        ka = 'train_clip_kernel' if 'train_clip_kernel' in a['Kernel_Name'] else 'train_wgrad_kernel'
        kb = 'train_clip_kernel' if 'train_clip_kernel' in b['Kernel_Name'] else 'train_wgrad_kernel'
        dur[ka].append((int(a['End_Timestamp']) - int(a['Start_Timestamp'])) / 1e3)
        if ka == kb:
            continue
        gaps['clip->wgrad' if ka == 'train_clip_kernel' else 'wgrad->clip'].append((int(b['Start_Timestamp']) - int(a['End_Timestamp'])) / 1e3)
    for k, v in dur.items():
        v = v[len(v) // 4:]          # the first quarter holds warm-up and capture
        print(f'{k:20s} n={len(v):5d} duration p10 {pct(v, .1):6.2f} p50 {statistics.median(v):6.2f} p90 {pct(v, .9):6.2f} us')
    med = {}
    for k, v in gaps.items():
        v = v[len(v) // 4:]
        med[k] = statistics.median(v)
        print(f'{k:20s} n={len(v):5d} gap      p10 {pct(v, .1):6.2f} p50 {med[k]:6.2f} p90 {pct(v, .9):6.2f} us')
    print(f"difference of the medians (clip->wgrad minus wgrad->clip): {med['clip->wgrad'] - med['wgrad->clip']:.2f} us")


if __name__ == '__main__':
    main(sys.argv[1])
