#!/usr/bin/env python
"""Static instruction-class counts of train_clip_kernel (csrc/p2c_train.hip), for work on its pose phase. No GPU needed.

    python tools/posecount.py                  # assembles csrc/p2c_train.hip with the Makefile's flags (about 6 s)
    python tools/posecount.py --extra=-DX=1    # ... plus more flags
    python tools/posecount.py --asm FILE.s     # counts a listing made earlier

For every instantiation train_clip_kernel<KIND, CFG> it prints two columns, the pose-phase region of the first-clip body and the
whole kernel, and the register figures of the code object's metadata. It only counts instruction classes in the listing: what a
wave EXECUTES depends on its path through the branches (profiles/k13_pose has the counter pass for that).

The region is found by landmarks, not by line numbers. The first-clip body is laid out first and in source order, and between two
s_barrier the number of MFMAs tells the steps apart: the barrier behind forward layer 5 is the first one with 40 or more MFMAs
since the barrier before it; from there the first barrier that has MFMAs in front of it again closes the suffix sum over time
(four 16x16x4), and the barrier after that one is dgrad step 5's, where the region ends. (A kind without the scan has no MFMA in
the phase: the first MFMAs are dgrad step 5's, and its barrier is the one in front of them.) The tool stops if the landmarks are
not there rather than count something else.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'pedestrians_video_2_carla_amd', 'csrc')
ROWS = ['instructions', 'VALU', '  v_mov', '  v_cndmask', '  lane read/write', '  DPP / permlane', 'MFMA', 'LDS', 'vector memory',
        's_nop', 's_waitcnt', 'branches', 's_barrier']


def makefile_flags():
    """FLAGS of csrc/Makefile without $(EXTRA), continuation lines joined."""
    text = open(os.path.join(CSRC, 'Makefile')).read().replace('\\\n', ' ')
    flags = re.search(r'^FLAGS\s*:=\s*(.*)$', text, re.M).group(1)
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    return flags.replace('$(ARCH)', arch).replace('$(EXTRA)', '').split()


def assemble(extra):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    out = os.path.join(tempfile.mkdtemp(prefix='posecount_'), 'p2c_train.s')
    cmd = [hipcc] + makefile_flags() + extra + ['--cuda-device-only', '-S', '-o', out, 'p2c_train.hip']
    subprocess.run(cmd, cwd=CSRC, check=True, stderr=subprocess.DEVNULL)
    return out


def classify(mn):
    """Rows of the table this mnemonic counts in."""
    rows = ['instructions']
    if mn.startswith(('v_mfma', 'v_smfmac')):
        rows.append('MFMA')
    elif mn.startswith('v_'):
        rows.append('VALU')
        if mn.startswith('v_mov_b'):
            rows.append('  v_mov')
        if mn.startswith('v_cndmask'):
            rows.append('  v_cndmask')
        if mn.startswith(('v_readlane', 'v_readfirstlane', 'v_writelane')):
            rows.append('  lane read/write')
        if '_dpp' in mn or mn.startswith('v_permlane'):
            rows.append('  DPP / permlane')
    elif mn.startswith('ds_'):
        rows.append('LDS')
    elif mn.startswith(('buffer_', 'global_', 'flat_', 'scratch_')):
        rows.append('vector memory')
    elif mn in ('s_nop', 's_waitcnt', 's_barrier'):
        rows.append(mn)
    elif mn.startswith(('s_cbranch', 's_branch')):
        rows.append('branches')
    return rows


def kernels(lines):
    """{symbol: label and instruction mnemonics} of every train_clip_kernel instantiation, in listing order."""
    out = collections.OrderedDict()
    name = None
    for ln in lines:
        m = re.match(r'^(_ZN9p2c_train17train_clip_kernelILi(\d+)E(?:Li(\d+)E)?E\w*):', ln)     # (<KIND> alone: a tree before CFG)
        if m:
            name = m.group(1)
            out[name] = {'label': 'train_clip_kernel<' + ', '.join(g for g in m.groups()[1:] if g) + '>', 'ins': []}
            continue
        if name and ln.startswith('.Lfunc_end'):
            name = None
            continue
        if name:
            m = re.match(r'^\s+([a-z][a-z0-9_]+)', ln)
            if m:
                out[name]['ins'].append(m.group(1))
    return out


def kernel_meta(lines, names):
    """The metadata entries name their kernel in the MIDDLE of the entry: collect each '- .args' block and key it by its .name."""
    meta, block = {}, []
    for ln in lines + ['  - .args:']:
        if re.match(r'^\s+- \.', ln) and not re.match(r'^\s{4,}- \.', ln):
            text = '\n'.join(block)
            m = re.search(r'^\s+\.name:\s+(\S+)', text, re.M)
            if m and m.group(1) in names:
                meta[m.group(1)] = {k: int(v) for k, v in re.findall(
                    r'^\s+\.(vgpr_count|agpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)', text, re.M)}
            block = []
        block.append(ln)
    return meta


def pose_region(ins):
    """(first, last) instruction index of the pose phase in the first-clip body; see the module docstring."""
    barriers, since = [], 0
    for i, mn in enumerate(ins):
        if mn.startswith('v_mfma'):
            since += 1
        elif mn == 's_barrier':
            barriers.append((i, since))
            since = 0
    start = next((k for k, (_, n) in enumerate(barriers) if n >= 40), None)
    if start is None:
        raise SystemExit('posecount: no barrier behind a run of >= 40 MFMAs (forward layer 5) found')
    suffix = next((k for k in range(start + 1, len(barriers)) if barriers[k][1] > 0), None)
    if suffix is None or suffix + 1 >= len(barriers) or suffix - 1 <= start:
        raise SystemExit('posecount: no MFMAs behind the pose phase found')
    if barriers[suffix][1] == 4:                       # the kinds with a scan over time
        return barriers[start][0] + 1, barriers[suffix + 1][0]
    return barriers[start][0] + 1, barriers[suffix - 1][0]   # no scan: these are dgrad step 5's MFMAs, its barrier is the one before


def count(ins):
    c = collections.Counter()
    for mn in ins:
        c.update(classify(mn))
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--asm', help='a device listing of p2c_train.hip (hipcc ... --cuda-device-only -S); made here if absent')
    ap.add_argument('--extra', action='append', default=[], help='one more compiler flag (repeatable)')
    a = ap.parse_args()
    path = a.asm or assemble(a.extra)
    lines = open(path).read().split('\n')
    ks = kernels(lines)
    if not ks:
        raise SystemExit(f'posecount: no train_clip_kernel in {path}')
    meta = kernel_meta(lines, set(ks))
    for name, k in ks.items():
        lo, hi = pose_region(k['ins'])
        region, whole = count(k['ins'][lo:hi]), count(k['ins'])
        md = meta.get(name, {})
        print(f"{k['label']}: vgpr_count {md.get('vgpr_count')}, sgpr_spill_count {md.get('sgpr_spill_count')}, "
              f"vgpr_spill_count {md.get('vgpr_spill_count')}, scratch {md.get('private_segment_fixed_size')} B")
        print(f"  {'class':<20}{'pose phase, first clip':>24}{'whole kernel':>16}")
        for r in ROWS:
            print(f'  {r:<20}{region[r]:>24}{whole[r]:>16}')
        print()
    return 0


if __name__ == '__main__':
    sys.exit(main())
