#!/usr/bin/env python3
"""Writes tests/golden/nmpc_DSS_tNMPC.npz: the stored closed loop of the reference's tracking NMPC
(saved_data+plots/data/casadi/DSS_tNMPC.mat, `xnl` 4 x 500: the measured states of
DMS_tracking_NMPC_casadi.m's 500 steps from x_init = [0.15 1.2875 1.1547 0]).

usage: make_nmpc_fixture.py <path to DSS_tNMPC.mat>
The tests read the fixture, never the reference tree."""
import os
import sys

import numpy as np
import scipy.io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    xnl = np.ascontiguousarray(sio.loadmat(sys.argv[1])['xnl'], dtype=np.float64)
    assert xnl.shape == (4, 500), xnl.shape
    out = os.path.join(ROOT, 'tests', 'golden', 'nmpc_DSS_tNMPC.npz')
    np.savez(out, xnl=xnl)
    print('wrote %s (%d bytes)' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main()
