"""The numpy restatement of the nonlinear MPC (tests/nmpc_ref.py) against central differences and
against the reference's stored tracking-NMPC closed loop (tests/golden/nmpc_DSS_tNMPC.npz)."""
import numpy as np
import pytest

import nmpc_ref as R
from conftest import golden
from oracle.mg_model import mg_rk4

STORED_T = (0, 10, 20, 200, 400)


@pytest.fixture(scope='module')
def xnl():
    return golden('nmpc_DSS_tNMPC.npz')['xnl']


@pytest.fixture(scope='module')
def cold(mg, term_set, xnl):
    """cold solves (u = u_eq, theta = 0) at the stored states, N = 100: computed once"""
    p = R.problem(mg, term_set[0], term_set[1], 100)
    return p, {t: R.sqp(p, xnl[:, t]) for t in STORED_T}


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_jacobians_against_central_differences(mg, term_set):
    """A_k, B_k, Jr and C against central differences (step 1e-6) of the restatement's own
    rollout at a non-trivial z, N = 10: 1e-7 relative (truncation h^2 plus round-off eps / h)"""
    N, h = 10, 1e-6
    p = R.problem(mg, term_set[0], term_set[1], N)
    rng = np.random.default_rng(3)
    x0 = p['x_eq'] + np.array([-0.2, -0.1, 0.05, 0.1])
    z = np.concatenate([rng.uniform(-0.3, 0.3, N), [0.07]])
    L = R.linearize(p, x0, z)
    for k in range(N):
        xk, uk = L['X'][k], z[k] + p['u_eq']
        Afd = np.zeros((4, 4))
        for j in range(4):
            e = np.zeros(4); e[j] = h
            Afd[:, j] = (mg_rk4(p['delta'], xk + e, uk) - mg_rk4(p['delta'], xk - e, uk)) / (2 * h)
        Bfd = (mg_rk4(p['delta'], xk, uk + h) - mg_rk4(p['delta'], xk, uk - h)) / (2 * h)
        assert _rel(L['A'][k], Afd) <= 1e-7, (k, _rel(L['A'][k], Afd))
        assert _rel(L['B'][k], Bfd) <= 1e-7, (k, _rel(L['B'][k], Bfd))
    Jfd = np.zeros_like(L['Jr']); Cfd = np.zeros_like(L['C'])
    for j in range(N + 1):
        e = np.zeros(N + 1); e[j] = h
        zp, zm = z + e, z - e
        Xp, Xm = R.rollout(p, x0, zp), R.rollout(p, x0, zm)
        Jfd[:, j] = (R.residuals(p, Xp, zp) - R.residuals(p, Xm, zm)) / (2 * h)
        Cfd[:, j] = (R.constraints(p, Xp, zp) - R.constraints(p, Xm, zm)) / (2 * h)
    assert _rel(L['Jr'], Jfd) <= 1e-7, _rel(L['Jr'], Jfd)
    assert _rel(L['C'], Cfd) <= 1e-7, _rel(L['C'], Cfd)


@pytest.mark.parametrize('t', STORED_T)
def test_cold_solve_reproduces_stored_transition(cold, xnl, t):
    """cold solves at stored states of DSS_tNMPC.mat, N = 100: mg_rk4(x_t, u_0) against the
    stored x_{t+1}.  The states t = 60 and 100 are left out on purpose: IPOPT's stored move there
    is 4.8e-4 off in x4 (the throttle rate, ~1000 du, amplifies its stopping tolerance)."""
    p, sol = cold
    z, lam, info = sol[t]
    assert info['exitflag'] == 1, info
    err = np.abs(mg_rk4(p['delta'], xnl[:, t], z[0] + p['u_eq']) - xnl[:, t + 1])
    print('t %d iterations %d err %s' % (t, info['iterations'], err))
    assert err[0] <= 1e-7 and err[1] <= 1e-7, err
    assert err[2] <= 1e-6, err
    assert err[3] <= 1e-4, err


@pytest.mark.parametrize('t', STORED_T)
def test_cold_solve_is_a_kkt_point(cold, xnl, t):
    p, sol = cold
    z, lam, _ = sol[t]
    k = R.kkt(p, xnl[:, t], z, lam)
    print('t %d kkt %s' % (t, k))
    assert k['stat'] <= 1e-6 * (1.0 + k['grad']), k
    assert k['cmax'] <= 1e-9, k
    assert k['lam_min'] >= 0.0, k


def test_infeasible_first_subproblem_is_flagged(mg, term_set):
    """x1 = -0.1 stays below 0 one step later whatever u is: the first sub-problem has a row
    that cannot hold"""
    p = R.problem(mg, term_set[0], term_set[1], 10)
    _, _, info = R.sqp(p, p['x_eq'] + np.array([-0.6, 0.0, 0.0, 0.0]))
    assert info['exitflag'] == -2, info
