"""Lane groups of the short-horizon stage wave (csrc/bqp_lanes.h, bqp_ocp.hip stage_wave<.., G>):
where G (N + 1) lanes fit the wave, stage k is served by G lanes that each form a part of the
stage's entries in the per-stage passes, every entry by the operation sequence it has with one
lane per stage.  The default dispatch therefore computes, bit for bit, what the one-lane-per-stage
kernels compute (BQP_OCP_LANE_GROUPS=1): x, u, theta, fval, exit flags, iteration counts, the
polish marks and, where requested, the multipliers.

The MG family runs G = 3 for N <= 20 (63 lanes at N = 20); N = 21, 24 and 25 are past it (G = 1
on both sides: the dispatch edge and the edge of the four-box-rows-per-lane instantiation the
groups are tied to), fp64 and fp32 alike.  The DI family is compiled with one lane per stage
only: no DI case."""
import os

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

KEYS = ('x', 'u', 'theta', 'fval', 'exitflag', 'iterations', 'polished')
DUALS = ('pi', 'lam_x', 'lam_u', 'lam_p')


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


def _lmpc(mg, ts, N):
    import bqp
    return bqp.LMPC(mg['A'], mg['B'], mg['K'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'],
                    mg['LAMBDA'], mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'],
                    ts[0], ts[1], N=N)


def _both(run):
    """run() under the default dispatch and with one lane per stage"""
    assert 'BQP_OCP_LANE_GROUPS' not in os.environ
    rg = run()
    os.environ['BQP_OCP_LANE_GROUPS'] = '1'
    try:
        r1 = run()
    finally:
        del os.environ['BQP_OCP_LANE_GROUPS']
    return rg, r1


def _assert_equal(rg, r1, keys=KEYS):
    print('flags %s, iterations mean %.2f max %d, polished %d' % (
        np.unique(rg.exitflag, return_counts=True), rg.iterations.mean(), rg.iterations.max(),
        int(np.sum(rg.polished))))
    for k in keys:
        assert np.array_equal(rg[k], r1[k]), k


@pytest.mark.parametrize('N', [20, 19, 2, 7, 21, 24, 25])
def test_mg_horizons(mg, term_set, handle, N):
    """F1 on the 616-row terminal set, states dx[:96] (49-81: the 15-iteration instances with x2
    at its box limit): N = 20 fills 63 lanes, N = 19 leaves lanes 60-63 idle, N = 2 and 7 use far
    fewer stages than lanes with the terminal set at k = N - 1 in the first stages"""
    lm = _lmpc(mg, term_set, N)
    X = golden('lmpc_N20.npz')['dx'][:96]
    rg, r1 = _both(lambda: lm.solve(X, handle=handle))
    _assert_equal(rg, r1)
    assert (rg.exitflag == 1).mean() > 0.9      # the comparison is between solved problems


def test_mg_per_instance_models(mg, term_set, handle):
    """A and B per instance (the C4 generator, seed 4), 64 instances"""
    d = golden('mg_design.npz')
    rng = np.random.default_rng(4)
    n = 64
    A = d['A'] + 0.01 * rng.standard_normal((n, 4, 4)) * np.abs(d['A'])
    Bm = d['B'].reshape(4, 1) + 0.01 * rng.standard_normal((n, 4, 1)) * np.abs(d['B'].reshape(4, 1))
    X = golden('lmpc_N20.npz')['dx'][:n]
    lm = _lmpc(mg, term_set, 20)
    rg, r1 = _both(lambda: lm.solve(X, A=A, B=Bm, handle=handle))
    _assert_equal(rg, r1)


def test_mg_duals(mg, term_set, handle):
    """multipliers requested (as tests/test_gpu_ocp.py test_duals_kkt requests them)"""
    lm = _lmpc(mg, term_set, 20)
    X = golden('lmpc_N20.npz')['dx'][:96]
    rg, r1 = _both(lambda: lm.solve(X, handle=handle, want_duals=True))
    _assert_equal(rg, r1, KEYS + DUALS)
    assert np.abs(rg.pi).max() > 0


@pytest.mark.parametrize('opts', [dict(max_iter=4), dict(polish=2)], ids=['max_iter4', 'polish2'])
def test_mg_repair_launch(mg, term_set, handle, opts):
    """the repair kernel (the POL instantiation shares the passes): four iterations leave every
    instance unconverged, so the solve launch hands all of them to the repair launch (which ends
    some of them polished); polish = 2 also sends the converged instances with a weakly active
    row there"""
    lm = _lmpc(mg, term_set, 20)
    X = golden('lmpc_N20.npz')['dx'][:96]
    rg, r1 = _both(lambda: lm.solve(X, handle=handle, **opts))
    _assert_equal(rg, r1)


def test_mg_fp32(mg, term_set, handle):
    """the fp32 instantiation of the same source (G = 3 against G = 1): the per-stage passes write
    their multiply-adds as one fma there (MADD in bqp_ocp.hip), so both forms fuse the same
    products whichever way the compiler pairs neighbouring entries"""
    lm = _lmpc(mg, term_set, 20)
    X = golden('lmpc_N20.npz')['dx'][:96]
    rg, r1 = _both(lambda: lm.solve(X, handle=handle, precision=1))
    _assert_equal(rg, r1)
