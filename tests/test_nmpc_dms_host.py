"""CPU checks of the identities the nonlinear MPC's multiple shooting rests on
(tests/nmpc_dms_ref.py against tests/nmpc_stage_ref.py and tests/nmpc_ref.py): at a consistent
iterate the sub-problem is the stage route's, at an inconsistent one it condenses to a directly
assembled dense QP, and its SQP ends at a full-space KKT point with single shooting's z."""
import numpy as np
import pytest

import nmpc_dms_ref as DR
import nmpc_ref as R
import nmpc_stage_ref as SR
from conftest import golden
from test_nmpc_stage_host import DEVS, rel, seeded_z

STATES = (0, 5, 20, 40, 60, 80)        # CASES of tests/test_gpu_nmpc_stage.py at N = 10


@pytest.mark.parametrize('N', [1, 2, 3, 10, 40])
def test_consistent_iterate_is_the_stage_route(mg, term_set, N):
    """X = the rollout of z: c = 0 exactly, every other block bit for bit the stage problem's"""
    p = R.problem(mg, term_set[0], term_set[1], N)
    for i in range(6):
        x0, z = p['x_eq'] + DEVS[i], seeded_z(N, i)
        sp = DR.dms_problem(p, x0, DR.consistent(p, x0, z), z)
        ref = SR.stage_problem(p, x0, z)
        assert np.array_equal(sp['c'], np.zeros((N, 4)))
        for key in ('A', 'B', 'W', 'w', 'xlb', 'xub', 'ulb', 'uub', 'Fp', 'hp'):
            assert np.array_equal(sp[key], ref[key]), key
        assert sp['cost'] == R.linearize(p, x0, z)['cost']


@pytest.mark.parametrize('N', [1, 2, 3, 10, 40])
def test_condensed_with_defects_is_the_direct_dense_qp(mg, term_set, N):
    """X = rollout + a seeded 1e-2 perturbation: the stage QP condensed with the c_k propagated
    against the dense QP from the residual form; the bars of
    test_condensed_stage_problem_is_the_dense_subproblem"""
    p = R.problem(mg, term_set[0], term_set[1], N)
    worst = {}
    for i in range(6):
        x0, z = p['x_eq'] + DEVS[i], seeded_z(N, i)
        rng = np.random.default_rng(31 * N + i)
        X = DR.consistent(p, x0, z) + rng.uniform(-1e-2, 1e-2, (N + 1, 4))
        sp = DR.dms_problem(p, x0, X, z)
        assert np.abs(sp['c']).max() > 1e-3
        D, L = DR.condense(p, sp), DR.dense_direct(p, sp, z)
        for k in ('H', 'f', 'C', 'c'):
            worst[k] = max(worst.get(k, 0.0), rel(D[k], L[k]))
    print('N %d, relative to max-abs: %s' % (N, worst))
    assert worst['H'] <= 1e-13 and worst['f'] <= 1e-13, worst
    assert worst['C'] <= 1e-15 and worst['c'] <= 1e-15, worst


def kkt_ok(p, x0, X, z, lam, pi):
    """the constants of _kkt_ok in tests/test_gpu_nmpc_stage.py, full space"""
    k = DR.kkt(p, x0, X, z, lam, pi)
    assert k['stat'] <= 1e-6 * (1.0 + k['grad']), k
    assert k['cmax'] <= 1e-9 and k['dmax'] <= 1e-9, k
    assert k['lam_min'] >= 0.0, k


@pytest.mark.parametrize('N', [10, 20])
def test_sqp_ends_at_a_kkt_point_with_single_shootings_z(mg, term_set, N, monkeypatch):
    """from the cold z on the stored run's states, from the consistent and from the flat start"""
    monkeypatch.setattr(R.dense_qp, 'solve', DR.qp_solve)      # nmpc_ref.sqp's, on a degenerate vertex
    p = R.problem(mg, term_set[0], term_set[1], N)
    xnl = golden('nmpc_DSS_tNMPC.npz')['xnl']
    for t in STATES:
        x0 = xnl[:, t]
        zs, _, info = R.sqp(p, x0)
        assert info['exitflag'] == 1, info
        for X0 in (None, DR.flat(p, x0)):
            X, z, lam, pi, inf = DR.sqp(p, x0, X0=X0)
            assert inf['exitflag'] == 1, (t, inf)
            kkt_ok(p, x0, X, z, lam, pi)
            err = np.abs(z - zs).max()
            print('N %d t %d %s start: %d iterations (single shooting %d), |z - z_ss| %.2e'
                  % (N, t, 'consistent' if X0 is None else 'flat', inf['iterations'], info['iterations'], err))
            assert err <= 1e-6, (t, err)
            assert np.array_equal(X[0], x0)
