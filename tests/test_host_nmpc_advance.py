"""Host check of the asynchronous nonlinear MPC loop's per-instance advance
(csrc/bqp_nmpc_advance.h) and its workspace (csrc/bqp_layout.h, CworkNmpc with the step counters):
tests/host/nmpc_advance_check.cpp runs the warm-start shift, the per-solve state reset and the
ts / nfin transition at N = 1, 2, 64, 127 on buffers of exactly the documented sizes - the last
step and an instance that is not done included - and checks the extended layout at batch 1 and
257.  The Makefile builds it with g++ under the address and undefined-behaviour sanitizers; it
runs on the host alone, outside Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'nmpc_advance_check')


def test_nmpc_advance_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
