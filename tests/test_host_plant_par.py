"""Host check of the plant coefficients' offset arithmetic (csrc/bqp_plant_par.h):
tests/host/plant_par_check.cpp loads every (instance, step) row for steps 1 and 2, batch 1 and 257,
shared and per-instance stride, constant and scheduled coefficients, from heap buffers of exactly
the documented sizes, against a plain loop nest - with a schedule it never touches row `steps` -
and runs the stride and value rules of the host entries.  The Makefile builds it with g++ under
the address and undefined-behaviour sanitizers; it runs on the host alone, outside Python."""
import os
import subprocess

from conftest import PKG

EXE = os.path.join(PKG, 'build', 'plant_par_check')


def test_plant_par_check_host():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert ' 0 failures' in r.stdout, r.stdout
