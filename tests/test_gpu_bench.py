"""A plain `bench.py` run on the GPU: the headline line alone, the number of timed steps it was given, and the outputs of its last
timed step under --dump-outputs (what two builds are compared on)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / 'outputs'
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '3', '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['steps'] == 7 and d['warmup'] == 3 and d['n_gpus'] == 1 and d['higher_is_better'] is True
    assert d['unit'] == 'utterances/s' and d['dtype'].startswith('bf16') and d['ms_per_step'] > 0
    assert abs(d['value'] - d['config']['global_batch'] * 1e3 / d['ms_per_step']) <= 2e-3 * d['value']
    for leg in ('roofline', 'cpu_baseline', 'inference', 'b_sweep', 'gpt2_small'):       # --full only
        assert leg not in d, leg
    files = {f: np.load(out / f) for f in os.listdir(out)}
    assert set(files) == {'loss.npy', 'params.npy', 'grads_sample.npy'}
    assert sum(os.path.getsize(out / f) for f in files) <= 64_000_000
    assert files['loss.npy'].dtype == np.float32 and files['loss.npy'].shape == (1,)
    np.testing.assert_allclose(files['loss.npy'][0], d['final_loss'], rtol=1e-4, atol=1e-5)      # the line rounds to 5 decimals
    assert files['params.npy'].shape == (13_207_712,) and files['grads_sample.npy'].shape == (1 << 20,)
    for a in files.values():
        assert np.isfinite(a).all()
    assert np.abs(files['grads_sample.npy']).max() > 0
