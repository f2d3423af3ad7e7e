"""The numpy restatement of the nonlinear MPC with soft state rows (tests/nmpc_soft_ref.py), pinned
to the values of the numpy prototype the feature was specified from: the starts whose first hard
sub-problem is infeasible solve with l1 = 100, l2 = 1000 on all eight rows of F_x; the starts from
which the hard terminal set cannot be reached stay -2; a large enough l1 reproduces the hard
solution; small weights trade slack for cost."""
import numpy as np
import pytest

import nmpc_ref as R
import nmpc_soft_ref as S
from conftest import golden

L1, L2 = 100.0, 1000.0


@pytest.fixture(scope='module')
def xnl():
    return golden('nmpc_DSS_tNMPC.npz')['xnl']


@pytest.fixture(scope='module')
def probs(mg, term_set):
    made = {}

    def get(N):
        if N not in made:
            made[N] = R.problem(mg, term_set[0], term_set[1], N)
        return made[N]
    return get


def starts(p, xnl):
    """the four start families: two stored states pushed 0.03 below the x2 bound, x2 0.05 outside
    the box on either side, and a corner"""
    d = np.array([0.0, -0.03, 0.0, 0.0])
    return [xnl[:, 60] + d, xnl[:, 20] + d, p['x_eq'] + [0, 0.55, 0, 0], p['x_eq'] + [0, -0.55, 0, 0],
            p['x_eq'] + [-0.3, -0.52, 0, 0]]


@pytest.mark.parametrize('N', [10, 20])
def test_soft_rows_solve_the_infeasible_starts(probs, xnl, N):
    p = probs(N)
    for i, x0 in enumerate(starts(p, xnl)):
        assert R.sqp(p, x0)[2]['exitflag'] == -2, i
        z, lam, info = S.sqp(p, x0, L1, L2)
        k = S.kkt(p, x0, z, lam, L1, L2)
        print('N %d start %d: flag %d in %d iterations, slack %.5f, soft lam %.3f'
              % (N, i, info['exitflag'], info['iterations'], k['slack_max'], k['soft_lam_max']))
        assert info['exitflag'] == 1, (i, info)
        assert info['iterations'] <= 5
        assert k['slack_max'] > 0
        assert k['stat'] <= 1e-6 * (1 + k['grad']) and k['cmax'] <= 1e-9 and k['lam_min'] >= -1e-9, k
        assert k['soft_rel'] <= 1e-6, k


def test_slack_and_multiplier_of_the_prototype(probs):
    p = probs(10)
    x0 = p['x_eq'] + [0, -0.55, 0, 0]
    z, lam, info = S.sqp(p, x0, L1, L2)
    k = S.kkt(p, x0, z, lam, L1, L2)
    assert info['exitflag'] == 1
    assert abs(k['slack_max'] - 0.047137) <= 5e-6, k['slack_max']
    assert abs(k['soft_lam_max'] - 147.137) <= 5e-3, k['soft_lam_max']
    assert abs(k['soft_lam_max'] - (L1 + L2 * k['slack_max'])) <= 1e-6
    assert abs(info['cost'] - R.cost(p, x0, z) - S.penalty(p, x0, z, L1, L2)) <= 1e-12 * info['cost']


def test_hard_infeasibility_stays(probs, xnl):
    """the terminal set stays hard: x1 0.52 below x_eq at N = 10, and every out-of-box start at N = 3"""
    p = probs(10)
    assert S.sqp(p, p['x_eq'] + [-0.52, 0, 0, 0], L1, L2)[2]['exitflag'] == -2
    p = probs(3)
    for i, x0 in enumerate(starts(p, xnl)):
        assert S.sqp(p, x0, L1, L2)[2]['exitflag'] == -2, i


@pytest.mark.parametrize('t', [0, 20, 40])
def test_penalty_is_exact(probs, xnl, t):
    """l1 above the hard problem's state-row multipliers: the hard solution (prototype: 5e-14)"""
    p = probs(10)
    zh, lamh, ih = R.sqp(p, xnl[:, t])
    assert ih['exitflag'] == 1
    l1 = 2.0 * lamh[:10 * 10].reshape(10, 10)[:, :8].max() + 1.0
    z, lam, info = S.sqp(p, xnl[:, t], l1, 10.0 * l1)
    print('t %d: l1 %.3f, |z - hard z| %.2e' % (t, l1, np.abs(z - zh).max()))
    assert info['exitflag'] == 1
    assert np.abs(z - zh).max() <= 1e-9


@pytest.mark.parametrize('N', [10, 20])
@pytest.mark.parametrize('w', [(5.0, 50.0), (1.0, 0.5)])
@pytest.mark.parametrize('t', [40, 60])
def test_low_weights_trade_slack_for_cost(probs, xnl, N, w, t):
    p = probs(N)
    x0 = xnl[:, t]
    zh, _, ih = R.sqp(p, x0)
    z, lam, info = S.sqp(p, x0, *w)
    k = S.kkt(p, x0, z, lam, *w)
    print('N %d t %d weights %s: slack %.4f, soft lam %.4f, |u0 - hard u0| %.4f, %d iterations'
          % (N, t, w, k['slack_max'], k['soft_lam_max'], abs(z[0] - zh[0]), info['iterations']))
    assert ih['exitflag'] == 1 and info['exitflag'] == 1
    assert k['slack_max'] > 0
    assert abs(k['soft_lam_max'] - (w[0] + w[1] * k['slack_max'])) <= 1e-6 * (1 + k['soft_lam_max'])
    assert abs(z[0] - zh[0]) > 1e-2
