"""Host check of the tracking loop's per-instance step (csrc/bqp_track.h) on the workspace of
csrc/bqp_layout.h CworkTrack: tests/host/track_step_check.cpp runs the host side of the loop -
record of a step's solve, linear plant with per-instance model and disturbance, the next step's
linear term w + Wr r - for the DI and MG shapes with shared and per-instance strides and a null
disturbance, on exactly sized heap buffers, against a plain loop nest.  The Makefile builds it
with g++ under the address and undefined-behaviour sanitizers; it runs on the host alone, outside
Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'track_step_check')


def test_track_step_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
