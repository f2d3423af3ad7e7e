"""CPU checks of the set-point on top of the restatements (tests/nmpc_track_ref.py): the three
restated forms of the problem - dense, stage, multiple shooting - agree with each other under a
set-point, a zero offset reproduces the restatements as they are bit for bit, and the restated loop
follows a schedule on a disturbed plant.

The grid: N = 3, 10, 20; x0 = x_eq + [-0.05, -0.05, 0, 0], and the stored run's states 0 and 40;
rho = x_ref - x_eq in {0.05 LAMBDA, [0.05, 0, 0, 0] (off the steady-state line), [-0.2, 0.1, 0.02, 0],
2 LAMBDA (outside the terminal set: theta stops at the set's limit, 0.98148)}.  The pair N = 20,
rho = 2 LAMBDA is left out of the z comparison: there the two SQPs stop 7.0e-7 apart, each within
its own stopping tolerance, which a 1e-6 bar does not separate from a difference."""
import numpy as np
import pytest

import nmpc_dms_ref as DR
import nmpc_ref as R
import nmpc_stage_ref as SR
import nmpc_track_ref as TR
from conftest import golden
from test_nmpc_stage_host import rel, seeded_z

NS = (3, 10, 20)


def rhos(p):
    lam = p['LAMBDA']
    return [0.05 * lam, np.array([0.05, 0.0, 0.0, 0.0]), np.array([-0.2, 0.1, 0.02, 0.0]), 2.0 * lam]


def starts(p):
    xnl = golden('nmpc_DSS_tNMPC.npz')['xnl']
    return [p['x_eq'] + np.array([-0.05, -0.05, 0.0, 0.0]), xnl[:, 0].copy(), xnl[:, 40].copy()]


@pytest.fixture(autouse=True)
def exact_fallback(monkeypatch):
    """the restatements' dense sub-problem solver hands a degenerate vertex to their exact one"""
    monkeypatch.setattr(R.dense_qp, 'solve', DR.qp_solve)


@pytest.mark.parametrize('N', NS)
def test_zero_offset_is_the_restatement(mg, term_set, N):
    """x_ref = x_eq: every quantity bit for bit that of the call without a set-point"""
    p = R.problem(mg, term_set[0], term_set[1], N)
    for i, x0 in enumerate(starts(p)):
        z = seeded_z(N, i)
        a, b = R.linearize(p, x0, z), TR.linearize(p, p['x_eq'], x0, z)
        for k in ('X', 'cost', 'c', 'C', 'H', 'f', 'e', 'Jr'):
            assert np.array_equal(a[k], b[k]), k
        a, b = SR.stage_problem(p, x0, z), TR.stage_problem(p, p['x_eq'], x0, z)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
        X = DR.consistent(p, x0, z) + 1e-3
        a, b = DR.dms_problem(p, x0, X, z), TR.dms_problem(p, p['x_eq'], x0, X, z)
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    # the with-block leaves the modules as they were
    assert R.residuals.__module__ == 'nmpc_ref' and SR.stage_problem.__module__ == 'nmpc_stage_ref'


@pytest.mark.parametrize('N', NS)
def test_forms_agree_at_a_seeded_z(mg, term_set, N):
    """dense f = 2 Jr'e against the stage problem's condensed gradient (the bar of
    test_condensed_stage_problem_is_the_dense_subproblem: 1e-13 of max-abs); only the T rows of e,
    f[N], w_N[theta] and the cost differ from the call without a set-point, by Lt rho, g and
    g theta + c0; the multiple-shooting problem at the rollout is the stage problem"""
    p = R.problem(mg, term_set[0], term_set[1], N)
    Lt = R._factors(p)[3]
    worst = 0.0
    for i, x0 in enumerate(starts(p)):
        z = seeded_z(N, i)
        L0, sp0 = R.linearize(p, x0, z), SR.stage_problem(p, x0, z)
        for rho in rhos(p):
            xr = p['x_eq'] + rho
            g, c0 = TR.offset(p, xr)
            L, sp = TR.linearize(p, xr, x0, z), TR.stage_problem(p, xr, x0, z)
            worst = max(worst, rel(TR.stage_f(p, xr, x0, z), L['f']))
            for k in ('X', 'c', 'C', 'H', 'Jr'):
                assert np.array_equal(L[k], L0[k]), k
            assert np.array_equal(L['e'][:5 * N + 4], L0['e'][:5 * N + 4])
            assert np.array_equal(L['e'][5 * N + 4:], L0['e'][5 * N + 4:] - Lt @ TR.rho_of(p, xr))
            assert np.array_equal(L['f'][:N], L0['f'][:N])
            assert abs(L['f'][N] - (L0['f'][N] + g)) <= 1e-12 * (abs(g) + abs(L0['f'][N]))
            assert abs(L['cost'] - (L0['cost'] + g * z[N] + c0)) <= 1e-12 * (abs(c0) + L0['cost'])
            for k in sp:
                if k != 'w':
                    assert np.array_equal(sp[k], sp0[k]), k
            dw = sp['w'] - sp0['w']
            assert dw[N, 5] != 0.0 and np.count_nonzero(dw) == 1
            dp = TR.dms_problem(p, xr, x0, DR.consistent(p, x0, z), z)
            assert np.array_equal(dp['w'], sp['w']) and dp['cost'] == L['cost']
    print('N %d: |stage f - dense f| relative to max-abs %.2e' % (N, worst))
    assert worst <= 1e-13, worst


def _kkt_ok(k):
    """the constants of _kkt_ok in tests/test_gpu_nmpc_stage.py"""
    assert k['stat'] <= 1e-6 * (1.0 + k['grad']), k
    assert k['cmax'] <= 1e-9 and k.get('dmax', 0.0) <= 1e-9, k
    assert k['lam_min'] >= 0.0, k


@pytest.mark.parametrize('N', NS)
def test_solves_agree(mg, term_set, N):
    """single shooting ends 1 at a KKT point of the problem with the set-point; multiple shooting
    from x_k = x0 ends 1 at a full-space KKT point with single shooting's z (1e-6); the target outside
    the terminal set gives theta = 0.98148 from the first start"""
    p = R.problem(mg, term_set[0], term_set[1], N)
    for i, x0 in enumerate(starts(p)):
        for j, rho in enumerate(rhos(p)):
            xr = p['x_eq'] + rho
            z, lam, info = TR.sqp(p, xr, x0)
            assert info['exitflag'] == 1 and info['iterations'] <= 6, info
            _kkt_ok(TR.kkt(p, xr, x0, z, lam))
            X, zm, lm, pi, im = TR.dms_sqp(p, xr, x0, X0=DR.flat(p, x0))
            assert im['exitflag'] == 1 and im['iterations'] <= 8, im
            _kkt_ok(TR.dms_kkt(p, xr, x0, X, zm, lm, pi))
            err = np.abs(zm - z).max()
            print('N %d start %d rho %d: theta %.5f, %d / %d iterations, |z - z_single| %.2e'
                  % (N, i, j, z[N], info['iterations'], im['iterations'], err))
            if not (N == 20 and j == 3):
                assert err <= 1e-6, (i, j, err)
            if i == 0 and j == 3:
                assert abs(z[N] - 0.98148) <= 5e-6 and abs(zm[N] - 0.98148) <= 5e-6, (z[N], zm[N])


def test_loop_follows_a_schedule_on_a_disturbed_plant(mg, term_set):
    """N = 10, 12 steps, each set-point held 4 steps, a seeded disturbance within
    +-[2e-3, 2e-3, 1e-3, 0]: every solve ends 1 in a few iterations, the plant transitions carry the
    disturbance; multiple shooting's loop gives the same moves"""
    p = R.problem(mg, term_set[0], term_set[1], 10)
    lam = p['LAMBDA']
    refs = p['x_eq'] + np.repeat(np.array([0.02, -0.02, 0.0]), 4)[:, None] * lam
    rng = np.random.default_rng(7)
    dist = rng.uniform(-1.0, 1.0, (12, 4)) * np.array([2e-3, 2e-3, 1e-3, 0.0])
    X, U, TH, fl, it = TR.loop(p, p['x_eq'], 12, refs, dist)
    print('iterations %s theta %s' % (it.tolist(), np.round(TH, 5).tolist()))
    assert (fl == 1).all() and it.max() <= 4, (fl, it)
    for t in range(12):
        assert np.array_equal(X[t + 1], R.mg_rk4(p['delta'], X[t], U[t]) + dist[t])
    Xm, Um, THm, flm, _ = TR.loop(p, p['x_eq'], 12, refs, dist, route='multiple')
    assert (flm == 1).all()
    assert np.abs(Um - U).max() <= 1e-6 and np.abs(THm - TH).max() <= 1e-6
