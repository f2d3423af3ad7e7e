"""GPU checks of the soft state rows of the nonlinear MPC's stage route (bqp_nmpc_data.xs_lin /
xs_quad: an exact L1 plus quadratic penalty on the rows of F_x, the sub-problems on the structured
solve's soft state bounds) against the numpy restatement tests/nmpc_soft_ref.py, the library's own
hard route and its step-synchronous loop."""
import os

import numpy as np
import pytest

import nmpc_ref as R
import nmpc_soft_ref as S
from conftest import golden
from oracle.mg_model import mg_rk4

pytestmark = pytest.mark.gpu

# the six states of tests/test_gpu_nmpc.py (deviations from x_eq) and one 0.05 below the x2 bound
DEVS = np.array([[-0.35, -0.4, 0, 0], [-0.2, -0.1, 0.05, 0.1], [0.0, 0.0, 0.0, 0.0],
                 [-0.1, 0.05, -0.02, 0.3], [-0.05, -0.05, 0, 0], [0.05, 0.1, 0.02, -0.2],
                 [0.0, -0.55, 0.0, 0.0]])
L1, L2 = 100.0, 1000.0
LOW = ((5.0, 50.0), (1.0, 0.5))

# The penalty at the iterate (the stage linearisation's pen0) and cost0 - pen0 = J against the
# restatement, relative to max-abs over the 14 cases of a horizon: 10 x the maximum measured on the
# MI355X over N = 1, 2, 63, 64, 127 (DESIGN.md section 1 "Soft state rows"; the same operations with
# fused multiply-adds and a wave sum in another order).  Measured: penalty 5.28e-15 (N = 63; 0 at
# N = 1, 2, 64), J 1.01e-15 (N = 64).
PEN_BAR = dict(penalty=5.3e-14, J=1.1e-14)
# Distance of a softened row's multiplier from the subdifferential of its penalty, relative to
# 1 + l1 + l2 s (nmpc_soft_ref.kkt's soft_rel): the soft structured solve has no active-set polish,
# its multipliers are the interior point's.  Measured on the MI355X over the cases of this file: the
# GPU's maximum 1.25e-9 (N = 20, the corner start), where the restatement's own value is 2.18e-9;
# the restatement's maximum is 3.48e-9 (N = 64), the accuracy at which either SQP stops.  The bar is
# 10 x the GPU's maximum (DESIGN.md section 1 "Soft state rows").
SOFT_REL_BAR = 1.3e-8


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

    def get(N, scale=None):
        key = (N, None if scale is None else tuple(scale))
        if key not in made:
            p = R.problem(mg, term_set[0], term_set[1], N)
            Fx, hx = np.array(mg['F_x'], float), np.array(mg['h_x'], float)
            if scale is not None:
                Fx, hx = Fx * np.asarray(scale)[:, None], hx * np.asarray(scale)
                p = dict(p, F_x=Fx, h_x=hx)
            g = bqp.NMPC(mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'], Fx, hx,
                         mg['F_u'], mg['h_u'], term_set[0], term_set[1], mg['x_wp'], mg['u_wp'], N=N)
            made[key] = (p, g)
        return made[key]
    return get


def starts(p, xnl):
    """the start families whose first hard sub-problem is infeasible"""
    d = np.array([0.0, -0.03, 0.0, 0.0])
    return np.array([xnl[:, 60] + d, xnl[:, 20] + d, p['x_eq'] + [0, 0.55, 0, 0], p['x_eq'] + [0, -0.55, 0, 0],
                     p['x_eq'] + [-0.3, -0.52, 0, 0]])


@pytest.fixture(scope='module')
def restated(probs, xnl):
    """the restatement's solutions, computed once per (horizon, start, weights)"""
    made = {}

    def get(N, x0, l1, l2):
        key = (N, tuple(x0), l1, l2)
        if key not in made:
            made[key] = S.sqp(probs(N)[0], np.asarray(x0), l1, l2)
        return made[key]
    return get


# ---- 1. what the stage linearisation hands the merit function ------------------------------
@pytest.mark.parametrize('N', [1, 2, 63, 64, 127])
def test_penalty_at_the_iterate(probs, handle, N):
    """pen0 and cost0 - pen0 = J at z = 0 and at a seeded z, seven states (one outside the box)"""
    p, g = probs(N)
    rng = np.random.default_rng(100 + N)
    X0 = np.concatenate([p['x_eq'] + DEVS, p['x_eq'] + DEVS])
    Z = np.concatenate([np.zeros((7, N + 1)),
                        np.concatenate([rng.uniform(-0.3, 0.3, (7, N)), rng.uniform(-0.1, 0.1, (7, 1))], 1)])
    r = g.stage_cost(X0, Z, xs_lin=L1, xs_quad=L2, handle=handle)
    rh = g.stage_cost(X0, Z, handle=handle)
    pen = np.array([S.penalty(p, X0[i], Z[i], L1, L2) for i in range(14)])
    J = np.array([R.cost(p, X0[i], Z[i]) for i in range(14)])
    assert np.isfinite(pen).all() and np.isfinite(J).all()
    assert pen[6] > 0 and pen[13] > 0                   # the state outside the box pays
    ep = np.abs(r.penalty - pen).max() / np.abs(pen).max()
    eJ = np.abs(r.cost - r.penalty - J).max() / np.abs(J).max()
    print('N %d: penalty max %.3e, relative to max-abs: penalty %.2e, cost0 - pen0 against J %.2e'
          % (N, pen.max(), ep, eJ))
    assert ep <= PEN_BAR['penalty'] and eJ <= PEN_BAR['J'], (ep, eJ)
    assert (rh.penalty == 0).all() and np.abs(rh.cost - J).max() <= PEN_BAR['J'] * np.abs(J).max()


# ---- 2. solves ------------------------------------------------------------------------------
def _check_solves(p, g, handle, restated, N, X0, l1, l2, what):
    r = g.solve(X0, handle=handle, subproblem='stage', xs_lin=l1, xs_quad=l2)
    worst = 0.0
    for i in range(X0.shape[0]):
        z, lam, info = restated(N, X0[i], l1, l2)
        kr = S.kkt(p, X0[i], z, lam, l1, l2)
        k = S.kkt(p, X0[i], r.z[i], r.lam[i], l1, l2)
        du, dth = abs(r.z[i, 0] - z[0]), abs(r.z[i, N] - z[N])
        ds = np.abs(r.slack[i] - S.slack(p, X0[i], z, l1, l2)).max()
        print('%s N %d case %d: flag %d (ref %d), iterations %d (ref %d), |u0 - ref| %.2e |theta - ref| %.2e '
              '|slack - ref| %.2e, slack %.5f, soft lam %.4f, subdifferential distance rel. %.2e (ref %.2e)'
              % (what, N, i, r.exitflag[i], info['exitflag'], r.iterations[i], info['iterations'], du, dth, ds,
                 k['slack_max'], k['soft_lam_max'], k['soft_rel'], kr['soft_rel']))
        assert r.exitflag[i] == info['exitflag'] == 1, (i, r.exitflag[i], info)
        assert du <= 1e-6 and dth <= 1e-6, (i, du, dth)
        assert ds <= 1e-6, (i, ds)
        assert k['stat'] <= 1e-6 * (1.0 + k['grad']), k
        assert k['cmax'] <= 1e-9, k
        assert k['lam_min'] >= 0.0, k
        assert k['soft_rel'] <= SOFT_REL_BAR, k
        assert abs(r.penalty[i] - S.penalty(p, X0[i], r.z[i], l1, l2)) <= 1e-12 * (1 + r.penalty[i])
        assert abs(r.cost[i] - R.cost(p, X0[i], r.z[i]) - r.penalty[i]) <= 1e-12 * (1 + abs(r.cost[i]))
        worst = max(worst, k['soft_rel'])
    print('%s N %d: largest subdifferential distance rel. %.3e' % (what, N, worst))
    return r


@pytest.mark.parametrize('N', [10, 20])
def test_infeasible_starts_solve(probs, handle, xnl, restated, N):
    p, g = probs(N)
    r = _check_solves(p, g, handle, restated, N, starts(p, xnl), L1, L2, 'starts')
    assert (r.slack.max(axis=(1, 2)) > 0).all()


@pytest.mark.parametrize('N', [10, 20])
@pytest.mark.parametrize('w', LOW)
def test_low_weights(probs, handle, xnl, restated, N, w):
    p, g = probs(N)
    X0 = np.ascontiguousarray(xnl[:, [40, 60]].T)
    r = _check_solves(p, g, handle, restated, N, X0, w[0], w[1], 'low weights %s' % (w,))
    rh = g.solve(X0, handle=handle, subproblem='stage')
    assert (r.slack.max(axis=(1, 2)) > 0).all()
    assert (np.abs(r.u0 - rh.u0) > 1e-2).all(), np.abs(r.u0 - rh.u0)


@pytest.mark.parametrize('t', [0, 20, 40])
def test_exact_penalty(probs, handle, xnl, restated, t):
    """l1 above the hard problem's state-row multipliers: the hard solution"""
    p, g = probs(10)
    zh, lamh, ih = R.sqp(p, xnl[:, t])
    l1 = 2.0 * lamh[:100].reshape(10, 10)[:, :8].max() + 1.0
    X0 = np.ascontiguousarray(xnl[:, [t]].T)
    r = _check_solves(p, g, handle, restated, 10, X0, l1, 10.0 * l1, 'exact penalty t = %d' % t)
    print('|z - hard z| %.2e' % np.abs(r.z[0] - zh).max())
    assert np.abs(r.z[0] - zh).max() <= 1e-6


def test_long_horizon(probs, handle, xnl, restated):
    """N = 64 (the per-stage kernel's L2 instantiation): the prototype's three feasible cases"""
    p, g = probs(64)
    _check_solves(p, g, handle, restated, 64, starts(p, xnl)[[0, 2, 3]], L1, L2, 'N = 64')


# ---- 3. the feature ---------------------------------------------------------------------------
def test_weights_turn_infeasible_into_solved(probs, handle, xnl):
    p, g = probs(10)
    X0 = starts(p, xnl)[[3, 0]]
    hard = g.solve(X0, handle=handle, subproblem='stage')
    soft = g.solve(X0, handle=handle, subproblem='stage', xs_lin=L1, xs_quad=L2)
    print('hard %s soft %s' % (hard.exitflag, soft.exitflag))
    assert (hard.exitflag == -2).all() and (soft.exitflag == 1).all()


# ---- 4. hard infeasibility, isolation -----------------------------------------------------------
def test_hard_infeasible_instance_and_isolation(probs, handle, xnl):
    p, g = probs(10)
    X6 = np.vstack([starts(p, xnl), xnl[:, 40]])
    X7 = np.vstack([X6, p['x_eq'] + [-0.52, 0, 0, 0]])
    kw = dict(handle=handle, subproblem='stage', xs_lin=L1, xs_quad=L2)
    r7, r6 = g.solve(X7, **kw), g.solve(X6, **kw)
    assert r7.exitflag[6] == -2 and (r7.exitflag[:6] == 1).all(), r7.exitflag
    assert np.array_equal(r7.z[:6], r6.z) and np.array_equal(r7.lam[:6], r6.lam)
    assert np.array_equal(r7.iterations[:6], r6.iterations)
    r1 = g.solve(X7[3:4], **kw)
    assert np.array_equal(r1.z[0], r7.z[3]) and np.array_equal(r1.lam[0], r7.lam[3])
    assert r1.iterations[0] == r7.iterations[3]


# ---- 5. refusals ----------------------------------------------------------------------------
def test_refusals(probs, handle, xnl):
    import bqp
    p, g = probs(10)
    X0 = starts(p, xnl)[:1]
    with pytest.raises(bqp.BqpError, match=r'unsupported.*\(-4\)'):
        g.solve(X0, handle=handle, subproblem='dense', xs_lin=L1, xs_quad=L2)
    with pytest.raises(bqp.BqpError, match=r'unsupported.*\(-4\)'):
        bqp.closed_loop_nmpc(g, X0, 2, handle=handle, xs_lin=L1, xs_quad=L2)
    one = np.zeros(8); one[1] = L1                      # x2 <= . softened, -x2 <= . hard
    with pytest.raises(bqp.BqpError, match=r'unsupported.*\(-4\)'):
        g.solve(X0, handle=handle, subproblem='stage', xs_lin=one)
    two = np.full(8, L1); two[5] = 0.5 * L1            # the two rows of x2 with different weights
    with pytest.raises(bqp.BqpError, match=r'unsupported.*\(-4\)'):
        g.solve(X0, handle=handle, subproblem='stage', xs_lin=two, xs_quad=L2)
    for bad in (-1.0, np.nan, np.inf):
        with pytest.raises(bqp.BqpError, match=r'invalid argument \(-1\)'):
            g.solve(X0, handle=handle, subproblem='stage', xs_lin=L1, xs_quad=bad)
        with pytest.raises(bqp.BqpError, match=r'invalid argument \(-1\)'):
            bqp.closed_loop_nmpc(g, X0, 2, handle=handle, subproblem='stage', xs_lin=bad)
    # x2 alone, both sides: fine
    both = np.zeros(8); both[[1, 5]] = L1
    assert g.solve(X0, handle=handle, subproblem='stage', xs_lin=both, xs_quad=10 * both).exitflag[0] == 1


# ---- 6. scaled rows ---------------------------------------------------------------------------
def test_scaled_rows(probs, handle, xnl, restated):
    """F_x rows times positive factors with l1 / a, l2 / a^2: the same problem.  Both rows of x1 and
    of x4 share a factor; the rows of x2 and x3 differ by powers of two, which keeps the pairs equal.

    lam a = lam is asserted row by row where the problem determines the multiplier.  It does not
    on a softened row that sits on its bound (c = 0, subdifferential [0, l1]) while its gradient
    depends on the other active rows': in the two x2 - 0.03 starts the row -x2 <= 0.5 of stage N
    is at 0 and is also a face of the hard terminal set, which is active, so only the sum of the
    two multipliers is determined (the restatement's exact solver returns 0 on the soft row, an
    interior point some value inside; two solves differed by 0.154 there with z equal to 1e-15).
    Those rows (|c| <= 1e-9 at the restatement's solution, 2 of 400) are covered by what is
    determined, C' lam: each solve's stationarity is within 1e-6 (1 + |grad J|), this file's bar,
    so the two C' lam are within 2e-6 (1 + |grad J|) of each other."""
    a = np.array([3.0, 2.0, 0.25, 0.7, 3.0, 0.5, 4.0, 0.7])
    p, g = probs(10)
    _, gs = probs(10, a)
    X0 = starts(p, xnl)
    # both solves to tol = 1e-10: at the default 1e-8 two solves whose data differ in the last bit
    # stop within the step tolerance of each other, not within 1e-9 (the sub-problems' own
    # stationarity follows tol, bqp.h)
    r = g.solve(X0, handle=handle, subproblem='stage', xs_lin=L1, xs_quad=L2, tol=1e-10)
    rs = gs.solve(X0, handle=handle, subproblem='stage', xs_lin=L1 / a, xs_quad=L2 / a ** 2, tol=1e-10)
    print('iterations %s, scaled %s' % (r.iterations, rs.iterations))
    assert (r.exitflag == 1).all() and (rs.exitflag == 1).all()
    dz = np.abs(rs.z - r.z).max()
    lam = r.lam[:, :100].reshape(-1, 10, 10)[:, :, :8]
    lams = rs.lam[:, :100].reshape(-1, 10, 10)[:, :, :8] * a
    ds = np.abs(rs.slack / a - r.slack).max()
    # the rows whose multiplier the problem determines: not the softened rows that sit on their
    # bound at the restatement's solution (|c| <= 1e-9, nmpc_soft_ref.kkt's ctol)
    unique = np.ones(lam.shape, bool)
    dforce = 0.0
    for i in range(X0.shape[0]):
        z, _, info = restated(10, X0[i], L1, L2)
        assert info['exitflag'] == 1
        Lz = R.linearize(p, X0[i], z)
        c = Lz['c'][:100].reshape(10, 10)[:, :8]
        unique[i] = np.abs(c) > 1e-9
        la = np.array(rs.lam[i]); la[:100].reshape(10, 10)[:, :8] *= a
        dforce = max(dforce, np.abs(Lz['C'].T @ (la - r.lam[i])).max() / (1.0 + np.abs(Lz['f']).max()))
    dl = np.abs(lams - lam)[unique].max()
    print('scaled rows: |z - z| %.2e, |lam a - lam| %.2e of %.1f on the %d rows off their bound, %.2e on the %d on it '
          '(instances %s), |C\'(lam a - lam)| %.2e (1 + |grad J|), |slack / a - slack| %.2e'
          % (dz, dl, lam.max(), unique.sum(), np.abs(lams - lam)[~unique].max(initial=0.0), (~unique).sum(),
             np.unique(np.nonzero(~unique)[0]), dforce, ds))
    print('per instance |z - z| %s at entries %s; |u - u| %.2e |theta - theta| %.2e; cost difference %s'
          % (np.abs(rs.z - r.z).max(axis=1), np.abs(rs.z - r.z).argmax(axis=1), np.abs(rs.z - r.z)[:, :10].max(),
             np.abs(rs.z - r.z)[:, 10].max(), rs.cost - r.cost))
    assert dz <= 1e-9
    assert dl <= 1e-6 * (1 + lam.max())
    assert dforce <= 2e-6
    assert ds <= 1e-9
    # the unscaled weights on the scaled rows give unequal pairs
    import bqp
    with pytest.raises(bqp.BqpError, match='unsupported'):
        gs.solve(X0, handle=handle, subproblem='stage', xs_lin=L1, xs_quad=L2)


# ---- 7. closed loop -----------------------------------------------------------------------------
def _loop(g, xi, steps, handle, sync, **kw):
    import bqp
    assert 'BQP_NMPC_SYNC' not in os.environ
    if not sync:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, subproblem='stage', **kw)
    os.environ['BQP_NMPC_SYNC'] = '1'
    try:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, subproblem='stage', **kw)
    finally:
        del os.environ['BQP_NMPC_SYNC']


def test_closed_loop(probs, handle, xnl):
    p, g = probs(10)
    steps = 12
    base = starts(p, xnl)[:2]
    xi = np.vstack([base, base[0] + [0.01, 0, 0, 0], base[0] + [0, -0.01, 0, 0],
                    base[1] + [-0.01, 0, 0, 0], base[1] + [0, 0.01, 0, 0]])
    ra = _loop(g, xi, steps, handle, False, xs_lin=L1, xs_quad=L2)
    rs = _loop(g, xi, steps, handle, True, xs_lin=L1, xs_quad=L2)
    print('flags\n%s\niterations\n%s\nx2 - x_eq of the unperturbed instances\n%s\nu - u_eq\n%s'
          % (ra.exitflag, ra.iterations, ra.X[:2, :, 1] - p['x_eq'][1], ra.U[:2] - p['u_eq']))
    for k in ('X', 'U', 'exitflag', 'iterations'):
        assert np.array_equal(ra[k], rs[k]), k
    assert (ra.exitflag == 1).all(), ra.exitflag
    for b in range(6):
        for t in range(steps):
            assert np.abs(ra.X[b, t + 1] - mg_rk4(p['delta'], ra.X[b, t], ra.U[b, t])).max() <= 1e-14, (b, t)
    for b in range(6):
        for t in (0, 2, 5, 9):
            z, _, info = S.sqp(p, ra.X[b, t], L1, L2)
            assert info['exitflag'] == 1
            assert abs(ra.U[b, t] - p['u_eq'] - z[0]) <= 1e-6, (b, t, ra.U[b, t] - p['u_eq'], z[0])
    assert (ra.X[:2, 11, 1] - p['x_eq'][1] >= -0.5).all(), ra.X[:2, 11, 1] - p['x_eq'][1]
    rh = _loop(g, xi, steps, handle, False)
    assert (rh.exitflag[:, 0] == -2).all(), rh.exitflag


# ---- 8. the hard route ----------------------------------------------------------------------
def test_zero_weights_are_the_hard_route(probs, handle, xnl):
    p, g = probs(10)
    X0 = np.vstack([np.ascontiguousarray(xnl[:, [0, 20, 40]].T), starts(p, xnl)[:1]])
    a = g.solve(X0, handle=handle, subproblem='stage')
    b = g.solve(X0, handle=handle, subproblem='stage', xs_lin=np.zeros(8), xs_quad=np.zeros(8))
    for k in ('z', 'lam', 'cost', 'exitflag', 'iterations'):
        assert np.array_equal(a[k], b[k]), k
    assert (b.slack == 0).all() and (b.penalty == 0).all()
