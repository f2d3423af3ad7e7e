"""GPU: the benchmark's command line.  A plain `bench.py --gpus 1 --steps K --warmup W` run times
K steps and prints the result line without the figures that take runs of their own (--full);
--dump-outputs writes the arrays the last timed step returned, which are the exact optima of the
stored states (tests/golden/lmpc_N20_all.npz, the bound of tests/test_gpu_configs.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.mark.timeout(120)
def test_plain_run_dumps_last_step(tmp_path):
    B, K = 64, 3
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(K),
                        '--warmup', '1', '--batch', str(B), '--dump-outputs', str(tmp_path)],
                       capture_output=True, text=True, timeout=100, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r['steps'] == K and r['warmup'] == 1 and r['dtype'] == 'f64' and r['unit'] == 'QP-steps/s'
    assert r['higher_is_better'] is True and r['ms_per_step'] > 0
    # value = batch / step time (ms_per_step is rounded to 1e-4 ms; a step takes over 0.01 ms)
    assert abs(r['value'] - B / (r['ms_per_step'] * 1e-3)) <= 1e-2 * r['value']
    # nothing that takes a run of its own in a plain run
    assert r['roofline'] is None and r['cpu_baseline'] is None
    assert 'value_two_groups' not in r['check'] and 'kkt_mu_max' not in r['check']
    assert r['check']['converged_frac'] == 1.0
    d = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(d) == ['exitflag', 'fval', 'theta', 'u', 'x']
    assert all(a.dtype == np.float64 for a in d.values())
    assert d['x'].shape == (B, 21, 4) and d['u'].shape == (B, 20, 1) and d['theta'].shape == (B, 1)
    assert (d['exitflag'] == 1).all()
    g = golden('lmpc_N20_all.npz')
    z = np.concatenate([d['u'].reshape(B, -1), d['theta']], axis=1)
    err = np.abs(z - g['z_star'][:B])
    assert err.max() < TOL, err.max()
