"""bench.py as it is run for the headline: a plain run prints the one JSON line with its contract fields and none of --full's
evidence, --steps sets the number of timed steps, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / 'outputs'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2',
                        '--dump-outputs', str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line['unit'] == 'clips/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['steps'] == 7 and line['warmup'] == 2 and line['n_gpus'] == 1
    assert line['ms_per_step'] > 0 and line['value'] == pytest.approx(256 * 1e3 / line['ms_per_step'], rel=1e-2)
    assert not {'repeat_ms_per_step', 'fresh_batch_ms_per_step', 'step_breakdown_us', 'roofline', 'roofline_sweep',
                'step_sweep', 'extra_configs', 'cpu_baseline'} & set(line), sorted(line)

    arrays = {p.stem: np.load(p) for p in out.glob('*.npy')}
    assert set(arrays) == {'loss', 'params', 'optim_exp_avg', 'optim_exp_avg_sq', 'optim_step'}, sorted(arrays)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays['params'].shape == arrays['optim_exp_avg'].shape == arrays['optim_exp_avg_sq'].shape
    assert float(arrays['loss']) == line['config']['final_loss']           # the value the last timed step returned
    assert (arrays['optim_exp_avg_sq'] > 0).any()                          # the optimizer has stepped
