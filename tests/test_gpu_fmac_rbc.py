"""Device check of the fp64 multiply-add with a DPP operand (fmac_rbc, fmac_rbc_seq, fmac_rbc_chain
of csrc/bqp_wave.h) and of the Riccati sweeps' step built on it: one wave runs
 - fmac_rbc<C>, C = 0..5, against fma(rbc<C>(v), ph, acc) on lane patterns carrying +-0, +-inf, a
   NaN payload, denormals and random values in all four rows;
 - chains of five multiply-adds whose broadcast source is written by the instruction just before
   them (the DPP read-after-write hazard the helpers' s_nop covers) against the chain with explicit
   moves;
 - a backward and a forward recursion in the sweeps' exact step forms, (NS, NU) = (5, 1) and (4, 2),
   N = 1, 2, 3, 20, 21, as the step was (rbc_all + plain multiply-adds, a copy kept in
   tests/hip/fmac_rbc_check.hip) and as it is now; every stage vector compared.
All comparisons are bit for bit.  The program also prints the s_memtime cycles of the 20-stage
recursions in both forms; they are not asserted."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   'learning-based-mpc_amd', 'build', 'fmac_rbc_check')


def test_fmac_rbc_bitwise():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(' 0 differ') == 3, r.stdout
    assert r.stdout.count('cycles, 20 stages') == 2, r.stdout
