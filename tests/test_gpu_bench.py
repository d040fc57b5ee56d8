"""bench.py on the device: a plain run prints the headline line only, --steps sets the number of timed steps, and
--dump-outputs writes what the last timed step computed - the same from run to run for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _bench(out):
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '3', '--dataset', '16384',
           '--dump-outputs', str(out)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


def test_plain_run_line_and_dumped_outputs(tmp_path):
    lines = [_bench(tmp_path / 'a'), _bench(tmp_path / 'b')]
    for line in lines:
        assert line['metric'] == 'ic_train_traces_per_sec' and line['unit'] == 'traces/s' and line['dtype'] == 'f32'
        assert line['steps'] == 7 and line['warmup'] == 3 and line['higher_is_better'] is True
        assert abs(line['value'] * line['ms_per_step'] / 1e3 - 1024) < 0.01 * 1024      # traces/s x s/step = the batch
        assert not {'roofline', 'is', 'cpu_baseline', 'ms_per_step_median'} & set(line)
    for name in ('loss', 'params', 'exp_avg', 'exp_avg_sq'):
        a, b = np.load(tmp_path / 'a' / (name + '.npy')), np.load(tmp_path / 'b' / (name + '.npy'))
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all()
        # the dumped step trains from the engine's initial state: only the order of its float-atomic sums may differ
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-6, err_msg=name)
    assert lines[0]['config']['final_loss'] == round(float(np.load(tmp_path / 'a' / 'loss.npy')[0]), 4)
