"""CPU checks of the identity the nonlinear MPC's stage route rests on (tests/nmpc_stage_ref.py
against tests/nmpc_ref.py): the stage problem condensed is the dense route's sub-problem, the
adjoint sweep gives f and C'lam, and the bound map handles scaled and permuted rows and rejects a
general one."""
import numpy as np
import pytest

import nmpc_ref as R
import nmpc_stage_ref as SR

# the six states of tests/test_gpu_nmpc.py (deviations from x_eq)
DEVS = np.array([[-0.35, -0.4, 0, 0], [-0.2, -0.1, 0.05, 0.1], [0.0, 0.0, 0.0, 0.0],
                 [-0.1, 0.05, -0.02, 0.3], [-0.05, -0.05, 0, 0], [0.05, 0.1, 0.02, -0.2]])


def seeded_z(N, i):
    rng = np.random.default_rng(1000 * N + i)
    return np.concatenate([rng.uniform(-0.3, 0.3, N), rng.uniform(-0.1, 0.1, 1)])


def rel(a, ref):
    return np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300)


@pytest.mark.parametrize('N', [1, 2, 3, 10, 40])
def test_condensed_stage_problem_is_the_dense_subproblem(mg, term_set, N):
    """H and f to 1e-13 of their max-abs (2e-16 measured), C and c to 1e-15; and f, C'lam from the
    adjoint sweep to 1e-13 for a seeded lam >= 0"""
    p = R.problem(mg, term_set[0], term_set[1], N)
    worst = {}
    for i in range(6):
        x0, z = p['x_eq'] + DEVS[i], seeded_z(N, i)
        L = R.linearize(p, x0, z)
        sp = SR.stage_problem(p, x0, z, lin=L)
        D = SR.condense(p, sp)
        rng = np.random.default_rng(7 * N + i)
        lam = np.where(rng.uniform(size=R.rows(p)) < 0.2, rng.uniform(0.0, 5.0, R.rows(p)), 0.0)
        e = dict(H=rel(D['H'], L['H']), f=rel(D['f'], L['f']), C=rel(D['C'], L['C']), c=rel(D['c'], L['c']),
                 adj_f=rel(SR.adjoint(p, sp), L['f']), adj_Cl=rel(SR.adjoint(p, sp, lam), L['C'].T @ lam))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # the order map and its inverse
        lx, lu, lp = SR.stage_duals(p, lam)
        assert np.array_equal(SR.lam_rows(p, lx, lu, lp), lam)
    print('N %d, relative to max-abs: %s' % (N, worst))
    assert worst['H'] <= 1e-13 and worst['f'] <= 1e-13, worst
    assert worst['C'] <= 1e-15 and worst['c'] <= 1e-15, worst
    assert worst['adj_f'] <= 1e-13 and worst['adj_Cl'] <= 1e-13, worst


def test_bound_map_scaled_and_permuted_rows(mg, term_set):
    """F_x with its rows permuted and scaled by positive factors (powers of two and others): the
    condensed stage problem has the same rows, and a multiplier of the stage problem's bound maps
    to lam_bound / |a| on the row"""
    N = 3
    p = R.problem(mg, term_set[0], term_set[1], N)
    rng = np.random.default_rng(3)
    perm = rng.permutation(8)
    scale = np.array([2.0, 0.5, 3.0, 0.7, 1.0, 4.0, 1.3, 0.25])
    q = dict(p)
    q['F_x'] = (p['F_x'] * scale[:, None])[perm]
    q['h_x'] = (p['h_x'] * scale)[perm]
    q['F_u'] = p['F_u'] * 2.5
    q['h_u'] = p['h_u'] * 2.5
    x0, z = p['x_eq'] + DEVS[1], seeded_z(N, 1)
    L = R.linearize(q, x0, z)
    sp = SR.stage_problem(q, x0, z, lin=L)
    D = SR.condense(q, sp)
    assert rel(D['C'], L['C']) <= 1e-15 and rel(D['c'], L['c']) <= 1e-15
    assert rel(D['H'], L['H']) <= 1e-13 and rel(D['f'], L['f']) <= 1e-13
    # the bounds themselves do not depend on the scaling: those of the unit rows, up to the four
    # roundings of (h a - a dv) / a on |h| + |dv| <= 21: 4 x 2^-53 x 21 < 1e-14
    sp1 = SR.stage_problem(p, x0, z)
    for key in ('xlb', 'xub', 'ulb', 'uub'):
        fin = np.isfinite(sp1[key])
        assert np.array_equal(fin, np.isfinite(sp[key])), key
        assert np.abs(sp[key][fin] - sp1[key][fin]).max() <= 1e-14, key
    rows, rowof = SR.bound_map(q['F_x'], q['F_u'])
    for i, (var, side, a) in enumerate(rows):
        assert rowof[var, side] == i
        if i < 8:
            assert a == scale[perm[i]] and var == perm[i] % 4 and side == (0 if perm[i] >= 4 else 1)
    # multipliers: C'lam from the rows equals the adjoint sweep on the re-ordered duals
    lam = rng.uniform(0.0, 2.0, R.rows(q))
    lx, lu, lp = SR.stage_duals(q, lam)
    assert np.allclose(SR.lam_rows(q, lx, lu, lp), lam, rtol=4e-16, atol=0.0)
    assert rel(SR.adjoint(q, sp, lam), L['C'].T @ lam) <= 1e-13


def test_general_row_is_rejected(mg, term_set):
    p = R.problem(mg, term_set[0], term_set[1], 2)
    q = dict(p)
    q['F_x'] = p['F_x'].copy()
    q['F_x'][2, 0] = 0.5                      # a two-entry row
    with pytest.raises(SR.NotBox):
        SR.bound_map(q['F_x'], q['F_u'])
    with pytest.raises(SR.NotBox):
        SR.stage_problem(q, p['x_eq'] + DEVS[0], np.zeros(3))
    q['F_x'] = np.vstack([p['F_x'], 2.0 * p['F_x'][:1]])   # two rows on the same side of x1
    with pytest.raises(SR.NotBox):
        SR.bound_map(q['F_x'], q['F_u'])
    q['F_x'] = p['F_x'].copy()
    q['F_x'][5] = 0.0                         # an empty row
    with pytest.raises(SR.NotBox):
        SR.bound_map(q['F_x'], q['F_u'])
