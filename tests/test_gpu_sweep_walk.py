"""Device check of the fp64 Riccati sweeps' loops as csrc/bqp_ocp.hip has them: per-lane offsets that
walk with the stage, the last stage pair peeled off the loop, and the store forms (row 0's lanes
< NS under a guard; every lane of every 16-lane row without one, with the peeled pair reached from fresh
or from the walked offsets).  One wave runs the backward and the
forward sweep, (NS, NU) = (5, 1) and (4, 2), N = 1, 2, 3, 4, 5, 20, on LDS operands
(tests/hip/sweep_walk_check.hip) against a plain per-stage reference of the same recursion: the
swept vectors, the words around them and the stages the sweep leaves alone, and the accumulator of
every lane that stores, all bit for bit.  The program also prints the s_memtime cycles of the
20-stage sweeps; they are not asserted."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   'learning-based-mpc_amd', 'build', 'sweep_walk_check')


def test_sweep_walk_bitwise():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'x 3 forms, 0 differ' in r.stdout, r.stdout
    assert r.stdout.count('cycles, 20 stages') == 2, r.stdout
