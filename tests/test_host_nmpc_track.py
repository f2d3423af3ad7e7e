"""Host check of the set-point schedule's index arithmetic in the nonlinear MPC loop's advance
(csrc/bqp_nmpc_advance.h: NmpcTrackArgs and the nmpc_track_* functions of
bqp_closed_loop_nmpc_track) and of the workspace's current-reference buffer (csrc/bqp_layout.h,
CworkNmpc): tests/host/nmpc_track_check.cpp runs every instance through all its steps at
steps = 1, 2, N = 1, 64, 127, batch = 1, 257 with shared and per-instance schedules on buffers of
exactly the documented sizes - the last step, which reads no next set-point, included.  The Makefile
builds it with g++ under the address and undefined-behaviour sanitizers; it runs on the host alone,
outside Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'nmpc_track_check')


def test_nmpc_track_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
