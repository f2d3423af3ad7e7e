"""Host check of the nonlinear MPC workspace layout (csrc/bqp_layout.h, Nwork):
tests/host/nmpc_layout_check.cpp checks alignment, disjointness, bounds and the byte total of its
regions at N = 1, 10, 100, 127 and batch 1, 257.  The Makefile builds it with g++ under the
address and undefined-behaviour sanitizers; it runs on the host alone, outside Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'nmpc_layout_check')


def test_nmpc_layout_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
