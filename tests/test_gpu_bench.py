"""The plain run of bench.py: exactly --steps timed steps, the headline fields only, and --dump-outputs writing what
the last timed step computed -- checked against the CPU oracle on that step's (seeded) input batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import normwise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_times_k_steps_and_dumps_the_last_step(tmp_path):
    import bench
    from oracle import dsp_oracle
    steps, buffers = 7, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(steps),
                        '--warmup', '2', '--buffers', str(buffers), '--dump-outputs', str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j['steps'] == steps and j['timing']['blocks_of_K_steps'] == 1
    assert j['ms_per_step'] > 0 and j['value'] > 0 and j['unit'] == 'frames/s' and j['dtype'] == 'f32'
    assert j['higher_is_better'] is True
    for key in ('roofline', 'parity_normwise_vs_oracle', 'other_paths', 'cpu_baseline', 'gather'):
        assert key not in j, f'{key} belongs to --full'
    assert sorted(os.listdir(tmp_path)) == ['features.npy']
    got = np.load(tmp_path / 'features.npy')
    assert got.dtype == np.float32 and got.shape == (bench.B * bench.T, 39)
    # the last timed step (index steps - 1) read input batch (steps - 1) % buffers of rank 0
    x = bench.synth_batch((steps - 1) % buffers)
    for b in (0, 1, bench.B - 1):
        ref = dsp_oracle.mfcc_delta(x[b].astype(np.float64), delta_n=bench.DELTA_N, winfunc=np.hamming, **bench.CFG)
        assert normwise(got[b * bench.T:(b + 1) * bench.T], ref) <= 1e-4, b
