"""Shared tables staged straight from the caller's arrays (bqp_ocp.hip ocp_body, raw_tables): at
short horizons with shared W and Fp the solve, repair and fp32 kernels form the prepared H / Fp
layout while they copy W and Fp into LDS, and the call launches no ocp_prep_kernel.  The staged
tables hold, element for element, what the prep kernel wrote (a copy or a zero), so the default
path computes bit for bit what BQP_OCP_PREP_LAUNCH=1 (the prep launch forced) computes: x, u, theta,
fval, exit flags, iteration counts, polish marks and, where requested, the multipliers."""
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


def _with_env(name, run):
    assert name not in os.environ
    os.environ[name] = '1'
    try:
        return run()
    finally:
        del os.environ[name]


def _both(run):
    """run() on the default path and with the prep launch forced"""
    assert 'BQP_OCP_PREP_LAUNCH' not in os.environ
    return run(), _with_env('BQP_OCP_PREP_LAUNCH', run)


def _assert_equal(rf, rp, keys=KEYS):
    print('flags %s, iterations mean %.2f max %d, polished %d' % (
        np.unique(rf.exitflag, return_counts=True), rf.iterations.mean(), rf.iterations.max(),
        int(np.sum(rf.polished))))
    for k in keys:
        assert np.array_equal(rf[k], rp[k]), k


@pytest.mark.parametrize('batch', [5, 9])
def test_mg_n20_partial_workgroup(mg, term_set, handle, batch):
    """F1 N = 20 on the 616-row set, four instances per workgroup: the last workgroup is partial"""
    lm = _lmpc(mg, term_set, 20)
    X = golden('lmpc_N20.npz')['dx'][:batch]
    rf, rp = _both(lambda: lm.solve(X, handle=handle, want_duals=True))
    _assert_equal(rf, rp, KEYS + DUALS)
    assert (rf.exitflag == 1).all() and np.abs(rf.lam_p).max() > 0


def test_mg_n2(mg, term_set, handle):
    """N = 2: three stages in the H table, the terminal set on stage 1 (its u columns stay)"""
    lm = _lmpc(mg, term_set, 2)
    X = golden('lmpc_N20.npz')['dx'][:32]
    rf, rp = _both(lambda: lm.solve(X, handle=handle))
    _assert_equal(rf, rp)
    assert (rf.exitflag == 1).mean() > 0.9


@pytest.mark.parametrize('N', [None, 5])
def test_di_terminal_set_at_stage_n(handle, N):
    """the DI tracking problem (NV = 6 as [2; 2; 2], 64-row table): its set sits at
    poly_stage == N, so the u columns of Fp and the u rows / columns of stage N are zeroed"""
    import bqp
    di = golden('di_design.npz')
    N = int(di['N']) if N is None else N
    tm = bqp.TrackingMPC(di['A'], di['B'], di['Q'], di['R'], di['P'], di['T'], di['LAMBDA'],
                         di['PSI'], di['F_x'], di['h_x'], di['F_u'], di['h_u'], di['F_T'],
                         di['h_T'], N=N)
    assert tm.prob.poly_stage == N
    gi = np.arange(0, len(di['x0']) * len(di['xs']), 37)[:96]
    X, XS = di['x0'][gi // len(di['xs'])], di['xs'][gi % len(di['xs'])]
    rf, rp = _both(lambda: tm.solve(X, XS, handle=handle, want_duals=True))
    _assert_equal(rf, rp, KEYS + DUALS)
    assert (rf.exitflag == 1).any()


def test_no_polytope(mg, term_set, handle):
    """n_poly = 0: the whole Fp table is zero and Fp itself is never read"""
    import bqp
    p = _lmpc(mg, term_set, 20).prob
    free = bqp.OcpProblem(p.A, p.B, p.W, p.N, 1, w=p.w, xlb=p.xlb, xub=p.xub, ulb=p.ulb, uub=p.uub)
    assert free.mp == 0
    X = golden('lmpc_N20.npz')['dx'][:16]
    rf, rp = _both(lambda: bqp.solve_ocp(free, X, handle=handle, route='structured'))
    _assert_equal(rf, rp)
    assert (rf.exitflag == 1).all()


def test_mg_fp32(mg, term_set, handle):
    """the fp32 instantiation: the double is read and converted on the store into LDS, as before"""
    lm = _lmpc(mg, term_set, 20)
    X = golden('lmpc_N20.npz')['dx'][:96]
    rf, rp = _both(lambda: lm.solve(X, handle=handle, precision=1))
    _assert_equal(rf, rp)


def test_mg_repair_launch(mg, term_set, handle):
    """max_iter = 4 leaves every instance unconverged: the repair kernel stages the tables too"""
    lm = _lmpc(mg, term_set, 20)
    X = golden('lmpc_N20.npz')['dx'][:96]
    rf, rp = _both(lambda: lm.solve(X, handle=handle, max_iter=4))
    _assert_equal(rf, rp)
    assert rf.polished.sum() > 0


def test_queue_counter_still_zeroed(mg, term_set, handle):
    """1100 instances of N = 2 are 275 workgroups, more than the device holds at once: the
    persistent kernel runs and its counter must start at zero without the prep launch.  Run twice
    on the default path (the first call leaves the counter advanced), against the forced prep
    launch and against one instance per slot (BQP_NO_QUEUE)"""
    lm = _lmpc(mg, term_set, 2)
    X = golden('lmpc_N20.npz')['dx'][np.arange(1100) % 1000]
    run = lambda: lm.solve(X, handle=handle)       # noqa: E731
    rf, rp = _both(run)
    rf2 = run()
    rs = _with_env('BQP_NO_QUEUE', run)
    _assert_equal(rf, rp)
    _assert_equal(rf2, rp)
    _assert_equal(rf, rs)
