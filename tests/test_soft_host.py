"""CPU: the soft-state-bound reference (tests/soft_ref.py) and the cases chosen with it
(tests/soft_cases.py): the reference's own KKT residuals on the augmented problem, the four
conditions every chosen instance meets, and exactness of the L1 penalty (with l1 above the largest
hard state-row multiplier the soft optimum is the hard one and every slack is 0)."""
import numpy as np
import pytest

import ltv_cases
import ltv_ref
import soft_cases
import soft_ref

# the exact solver ends with one fp64 KKT solve on the active set: residuals at round-off of the
# data (|H|, multipliers <= 1e4); measured <= 1e-11
TOL_REF = 1e-9


@pytest.mark.parametrize('family,N,model', [('mg', 3, 'stg'), ('mg', 25, 'one'), ('di', 3, 'stg'),
                                            ('di', 32, 'one')])
def test_reference_kkt_and_case_conditions(family, N, model):
    for pair in soft_cases.WEIGHTS:
        cs = soft_cases.case(family, N, model, pair)
        prob = cs['prob']
        assert len(cs['ref']) == soft_cases.n_instances(N)
        for i, r in enumerate(cs['ref']):
            A, B, c = (soft_cases._at(cs[k], i) for k in ('A', 'B', 'c'))
            assert ltv_ref.solve(prob, cs['X'][i], A, B, c)['status'] != 'optimal'   # infeasible when hard
            assert r['status'] == 'optimal'
            assert r['s'].max() > 1e-6 and r['lam_all'].max() <= 1e4
            st, comp, lmin, viol = soft_ref.kkt(r['aug'], r['zs'], r['lam_all'])
            assert st < TOL_REF and comp < TOL_REF and lmin > -1e-12 and viol < TOL_REF, (i, st, comp, lmin, viol)
            # a softened row's multiplier lies in [0, l1 + l2 s], the slack's own in [0, l1]
            lam_s = r['lam'][r['aug']['soft']]
            assert (lam_s <= r['aug']['l1'] + r['aug']['l2'] * r['s'] + 1e-9).all()
            assert np.abs(lam_s + r['nu'] - r['aug']['l1'] - r['aug']['l2'] * r['s']).max() < 1e-8


def exact_penalty_case(family='di', N=30):
    """a feasible case of ltv_cases with active state rows, and soft weights with l1 at 10 x the
    largest hard state-row multiplier (l2 = 1: the exact solver needs a strictly convex problem)"""
    cs = ltv_cases.case(family, N)
    prob = cs['prob']
    nst = len(soft_ref.state_rows(prob))
    lmax = max(r['lam'][:nst].max() for r in cs['ref'])
    assert lmax > 1e-6                                         # the construction: state rows are active
    lin = np.zeros((N + 1, prob.nx)); quad = np.zeros((N + 1, prob.nx))
    lin[1:] = 10.0 * lmax; quad[1:] = 1.0
    return cs, lin, quad


def test_exact_penalty_keeps_the_hard_optimum():
    cs, lin, quad = exact_penalty_case()
    prob = cs['prob']
    for i, hard in enumerate(cs['ref']):
        r = soft_ref.solve(prob, cs['X'][i], lin, quad, cs['A'][i], cs['B'][i], cs['c'][i])
        assert r['status'] == 'optimal'
        assert np.abs(r['z'] - hard['z']).max() <= 1e-9 * max(1.0, np.abs(hard['z']).max())
        assert r['s'].max() <= 1e-12
