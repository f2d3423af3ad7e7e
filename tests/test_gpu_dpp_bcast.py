"""Device check of the DPP lane moves of csrc/bqp_wave.h that are issued with old = 0 and
bound_ctrl:1 (rbc / rbc_all, the first four steps of wsum, wsum_t's pair exchanges): one wave runs
rbc_all<0,5> and <0,6>, wsum, and wsum_t for K = 2, 7, 23, 32 in double and K = 23 in float, with
the helpers of the header and with copies of their earlier definitions (old = 0 written first, no
bound_ctrl) kept in tests/hip/dpp_bcast_check.hip, and the two outputs must be equal bit for bit.
The lane patterns carry +-0, +-inf, a NaN payload and denormals."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   'learning-based-mpc_amd', 'build', 'dpp_bcast_check')


def test_dpp_bound_ctrl_moves_bitwise():
    assert os.path.exists(EXE), 'build first: make -C learning-based-mpc_amd'
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count(' 0 differ') == 2, r.stdout
