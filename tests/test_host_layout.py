"""Host check of the device workspace layouts (csrc/bqp_layout.h): tests/host/layout_check.cpp
pins the offsets of every buffer of the handle at fixed shapes and checks alignment, disjointness
and bounds of every region over a grid of shapes.  The Makefile builds it with g++ under the
address and undefined-behaviour sanitizers; it runs on the host alone, outside Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'layout_check')


def test_layout_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
