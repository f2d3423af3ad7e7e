"""Host check of the stage wave's lane-group mapping (csrc/bqp_lanes.h): tests/host/
lane_map_check.cpp checks, for every compiled (ns, nu, G) and every horizon N = 1..63, that each
(stage, entry) of s / pi has exactly one owner lane below 64, that the dispatch's choice of G
fits the wave, and that the BQP_OCP_LANE_GROUPS cap never selects an uncompiled instantiation.
The Makefile builds it with g++ under the address and undefined-behaviour sanitizers; it runs on
the host alone, outside Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'lane_map_check')


def test_lane_map_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
