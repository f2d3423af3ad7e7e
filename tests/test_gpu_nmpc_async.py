"""The asynchronous nonlinear MPC closed loop (bqp_closed_loop_nmpc, every instance at its own
step) against the library's own step-synchronous loop (BQP_NMPC_SYNC).  Per instance both run the
same kernels on the same data in the same order, so every comparison is bitwise: no tolerance.

The round count is checked against the GPU's own logs.  With r[b, t] = iterations[b, t] +
(exitflag[b, t] != 0) - a converged or failed solve uses iterations + 1 rounds (the round that
finds it so takes no step), one stopped at max_iter uses iterations rounds - the asynchronous loop
launches max_b sum_t r[b, t] rounds: the advance happens in the round that stops the solve and the
host polls every round."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import golden
from test_gpu_nmpc import DEVS

pytestmark = pytest.mark.gpu

KEYS = ('X', 'U', 'exitflag', 'iterations')


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


@pytest.fixture(scope='module')
def xnl():
    return golden('nmpc_DSS_tNMPC.npz')['xnl']


@pytest.fixture(scope='module')
def probs(mg, term_set):
    import bqp
    made = {}

    def get(N):
        if N not in made:
            made[N] = bqp.NMPC(mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'],
                               mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'], term_set[0], term_set[1],
                               mg['x_wp'], mg['u_wp'], N=N)
        return made[N]
    return get


def _loop(g, xi, steps, handle, sync, **kw):
    import bqp
    assert 'BQP_NMPC_SYNC' not in os.environ
    if not sync:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, **kw)
    os.environ['BQP_NMPC_SYNC'] = '1'
    try:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, **kw)
    finally:
        del os.environ['BQP_NMPC_SYNC']


def _rounds_from_logs(r):
    return int((r.iterations + (r.exitflag != 0)).sum(axis=1).max())


def _both(g, xi, steps, handle, **kw):
    """both modes, bitwise equal, the asynchronous round count as its own logs give it"""
    ra = _loop(g, xi, steps, handle, False, **kw)
    rs = _loop(g, xi, steps, handle, True, **kw)
    print('iterations\n%s\nflags\n%s\nrounds: asynchronous %d, from its logs %d, step-synchronous %d'
          % (ra.iterations, ra.exitflag, ra.rounds, _rounds_from_logs(ra), rs.rounds))
    for k in KEYS:
        assert np.array_equal(ra[k], rs[k]), k
    assert ra.rounds == _rounds_from_logs(ra)
    assert ra.launches == 6 * ra.rounds
    return ra, rs


@pytest.fixture(scope='module')
def crossing(probs, handle, xnl):
    """N = 20 (the wave form of the dense kernel), 8 steps, five stored states: the restatement's
    closed loop needs [4,2,3,3,2,3,2,2], [3,3,3,2,3,2,2,2] and three times [3,2,2,2,2,2,2,2]
    iterations, all flags 1, so the slowest instance changes over time: max_b sum_t r = 29 against
    sum_t max_b r = 31, and 36 launched by the step-synchronous loop, which polls every fourth
    iteration at n < 64"""
    xi = np.ascontiguousarray(xnl[:, [4, 12, 24, 40, 80]].T)
    return (xi,) + _both(probs(20), xi, 8, handle)


def test_crossing_batch_equal_and_fewer_rounds(crossing):
    _, ra, rs = crossing
    assert ra.rounds < rs.rounds, (ra.rounds, rs.rounds)


@pytest.mark.parametrize('N', [40, 100])
def test_other_dense_forms(probs, handle, xnl, N):
    """N = 40: the register-resident workgroup form; N = 100: the workspace form, n >= 64, where
    the step-synchronous loop polls every iteration"""
    g = probs(N)
    if N == 40:
        xi = g.x_eq + DEVS[[0, 1, 3, 4]]
    else:
        xi = xnl[:, [0, 20, 200, 0]].T.copy()
        xi[3, 0] += 0.02
    ra, rs = _both(g, np.ascontiguousarray(xi), 3, handle)
    assert ra.rounds <= rs.rounds, (ra.rounds, rs.rounds)


def _seven(g):
    return np.vstack([g.x_eq + DEVS, g.x_eq + np.array([-0.6, 0.0, 0.0, 0.0])])


def test_failed_instance(probs, handle):
    """N = 10, 5 steps, the six DEVS states and one whose sub-problem is infeasible (-2 in
    test_gpu_nmpc.py::test_isolation): its flags and its plant steps are compared as the others'"""
    ra, _ = _both(probs(10), _seven(probs(10)), 5, handle)
    assert ra.exitflag[6, 0] == -2, ra.exitflag[6]
    assert (ra.exitflag[:6] == 1).all(), ra.exitflag


def test_iteration_limit(probs, handle):
    """max_iter = 2: the DEVS instances need [3,3,1,3,2,2] iterations per step on the restatement,
    so several solves stop at the limit (flag 0) and use 2 rounds"""
    ra, _ = _both(probs(10), _seven(probs(10)), 5, handle, max_iter=2)
    lim = ra.exitflag == 0
    assert lim.any(), ra.exitflag
    assert (ra.iterations[lim] == 2).all()


def test_polish_per_instance(probs, handle):
    """polish = 1: the sub-problems' polish mode per instance from its own iteration count"""
    g = probs(10)
    _both(g, g.x_eq + DEVS, 3, handle, polish=1)


def test_isolation(probs, handle, crossing):
    """instance 1 of the crossing batch as a batch of one"""
    xi, ra, _ = crossing
    r1 = _loop(probs(20), xi[:1], 8, handle, False)
    for k in KEYS:
        assert np.array_equal(r1[k][0], ra[k][0]), k
    assert r1.rounds == _rounds_from_logs(r1)


def test_arguments(probs, handle):
    import bqp
    from bqp import _lib
    lib = _lib.load()
    g = probs(10)
    n = C.c_int(-7)
    fresh = bqp.Handle(0)
    assert lib.bqp_last_loop_rounds(fresh.value, C.byref(n)) == _lib.BQP_E_ARG
    assert lib.bqp_last_loop_rounds(None, C.byref(n)) == _lib.BQP_E_ARG
    assert lib.bqp_last_loop_rounds(handle.value, None) == _lib.BQP_E_ARG
    xi = g.x_eq + DEVS[:3]
    r = _loop(g, xi, 0, fresh, False)
    assert r.X.shape == (3, 1, 4) and np.array_equal(r.X[:, 0], xi)
    assert r.rounds == 0
    # a second loop on a handle reports its own count, not the first one's
    ra = _loop(g, xi, 2, fresh, False)
    assert ra.rounds == _rounds_from_logs(ra) and ra.rounds > 0
    rb = _loop(g, xi[2:], 1, fresh, False)
    assert rb.rounds == _rounds_from_logs(rb) and 0 < rb.rounds < ra.rounds
    assert np.array_equal(rb.X[0], ra.X[2, :2])
    assert _loop(g, xi, 0, fresh, True).rounds == 0
    fresh.close()
