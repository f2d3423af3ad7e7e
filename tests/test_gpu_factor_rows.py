"""Device check of the fp64 Riccati factorisation's stage loop as csrc/bqp_ocp.hip has it: one packed
entry of P_k per lane of every 16-lane row, P_{k+1} read as the DPP operand of the stage's
multiply-adds, the four rows' values exchanged with the row swaps, stores from every lane without a
guard.  One wave runs (NS, NU) = (5, 1) and (4, 2), N = 1, 2, 3, 20 and N = 20 with a non-positive
pivot planted at stage 10, on LDS operands with random SPD stage costs and the polytope term at one
stage (tests/hip/factor_rows_check.hip), against a plain reference of the same recursion in the same
association and against the quad / LDS form: the P table, K, the factors, the guard words around them,
`ok` and every lane's final register, all bit for bit.  The program also prints the s_memtime cycles
of the 20-stage loop in both forms; they are not asserted."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   'learning-based-mpc_amd', 'build', 'factor_rows_check')


def test_factor_rows_bitwise():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'x 2 forms, 0 differ' in r.stdout, r.stdout
    assert r.stdout.count('cycles, 20 stages') == 2, r.stdout
