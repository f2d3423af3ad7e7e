"""Host check of the nonlinear MPC stage route's index arithmetic (csrc/bqp_nmpc_stage.h: the
bound map of F_x / F_u, where a row's bound lies in the structured solve's arrays, the order map
between that solve's multipliers and the NMPC rows) and of its workspace (csrc/bqp_layout.h,
NworkStage): tests/host/nmpc_stage_check.cpp runs them at N = 1, 2, 64, 127 on heap buffers of
exactly the documented sizes and checks the layout at batch 1 and 257.  The Makefile builds it
with g++ under the address and undefined-behaviour sanitizers; it runs on the host alone, outside
Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'nmpc_stage_check')


def test_nmpc_stage_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
