"""GPU: the structured solve with soft state bounds (bqp_ocp_data.xs_lin / xs_quad) against the
exact optimum of the softened problem (tests/soft_ref.py, cases of tests/soft_cases.py): both
model families at the row layouts' edges, per-stage schedules and one model, the slacks and the
multipliers, exactness of the penalty, shared against per-instance weights, isolation of an
instance that is infeasible even when soft, the error codes, and the closed loop with a
disturbance that carries the state outside the box.

Measured on an MI355X (this file's prints): see DESIGN.md section 5."""
import ctypes as C
import types

import numpy as np
import pytest

import dual_map as dm
import ltv_cases
import ltv_ref
import soft_cases
import soft_ref

pytestmark = pytest.mark.gpu

TOL = 1e-8          # |[z; s] - ref|_inf / max(1, |ref|_inf): the project's standing bar
TOL_LAM = 1e-7      # multipliers, relative (test_gpu_ocp_ltv.py)


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


def _z(r):
    return np.concatenate([r.u.reshape(len(r.u), -1), r.theta], axis=1)


def _solve(handle, cs, **kw):
    import bqp
    return bqp.solve_ocp(cs['prob'], cs['X'], A=cs['A'], B=cs['B'], c=cs['c'], xs_lin=cs['lin'],
                         xs_quad=cs['quad'], handle=handle, want_duals=True, **kw)


def _cost(prob, x, u, th):
    """sum_k 0.5 v'W_k v + w_k'v of one instance (the u block of stage N ignored)"""
    N, nx, nu = prob.N, prob.nx, prob.nu
    f = 0.0
    for k in range(N + 1):
        v = np.concatenate([x[k], u[k] if k < N else np.zeros(nu), th])
        f += 0.5 * v @ prob.W[k] @ v + prob.w[k] @ v
    return f + prob.const


def _check(cs, r, tag):
    """flags, [z; s] and multipliers of a soft solve against the case's exact optima; returns the
    measured maxima (zs error, multiplier error)"""
    prob, ref = cs['prob'], cs['ref']
    assert all(q['status'] == 'optimal' for q in ref)           # the construction, not the solver
    ez, el, compared = 0.0, 0.0, 0
    flags_ok = (r.exitflag == 1).all()
    for i, q in enumerate(ref):
        aug = q['aug']
        zs = np.concatenate([_z(r)[i], soft_ref.slack_rows(aug, r.s_x[i])])
        ez = max(ez, np.abs(zs - q['zs']).max() / max(1.0, np.abs(q['zs']).max()))
        lam = ltv_ref.lam_rows(prob, r.lam_x[i], r.lam_u[i], r.lam_p[i])
        # the slack bounds' multipliers follow from the slack's stationarity
        s = zs[aug['nz']:]
        nu = aug['l1'] + aug['l2'] * s - lam[aug['soft']]
        full = np.concatenate([lam, nu])
        if dm.licq(aug['A'], np.maximum(full, 0.0), q['lam_all']):
            compared += 1
            el = max(el, np.abs(lam - q['lam']).max() / max(1.0, np.abs(q['lam_all']).max()))
    print('%s: flags %s iterations %s |[z; s] - ref| %.2e, |lam - ref| %.2e on %d of %d instances, '
          'max slack %.2e, slacks > 1e-9 %s' % (
              tag, r.exitflag.tolist(), r.iterations.tolist(), ez, el, compared, len(ref),
              max(q['s'].max() for q in ref), [int((q['s'] > 1e-9).sum()) for q in ref]))
    assert flags_ok, r.exitflag
    assert (r.polished == 0).all()
    assert ez <= TOL, ez
    assert compared >= 1 and el <= TOL_LAM, (compared, el)
    for i, q in enumerate(ref):
        aug = q['aug']
        lam = ltv_ref.lam_rows(prob, r.lam_x[i], r.lam_u[i], r.lam_p[i])
        s = soft_ref.slack_rows(aug, r.s_x[i])
        assert (s >= 0).all() and (lam >= 0).all()
        # a softened row's multiplier lies in [0, l1 + l2 s]
        assert (lam[aug['soft']] <= (aug['l1'] + aug['l2'] * s) * (1 + 1e-9) + 1e-9).all()
        # fval includes the penalty
        pen = (aug['l1'] * s + 0.5 * aug['l2'] * s * s).sum()
        f = _cost(prob, r.x[i], r.u[i], r.theta[i]) + pen
        assert abs(r.fval[i] - f) <= 1e-9 * max(1.0, abs(f)), (i, r.fval[i], f)
        # the softened rows x - s <= xub hold
        assert (r.x[i, 1:] - r.s_x[i, 1:, 1] <= prob.xub[1:] + 1e-9).all()
        assert (r.x[i, 1:] + r.s_x[i, 1:, 0] >= prob.xlb[1:] - 1e-9).all()
    return ez, el


_STG = [(f, N) for f, Ns in soft_cases.HORIZONS.items() for N in Ns if (f, N) != ('mg', 1)]
_ONE = [(f, N) for f, Ns in soft_cases.ONE_MODEL.items() for N in Ns]


@pytest.mark.parametrize('pair', soft_cases.WEIGHTS, ids=lambda p: 'w%g_%g' % p)
@pytest.mark.parametrize('family,N', _STG)
def test_parity_per_stage_schedules(handle, family, N, pair):
    cs = soft_cases.case(family, N, 'stg', pair)
    _check(cs, _solve(handle, cs), '%s N=%d stg %s' % (family, N, pair))


@pytest.mark.parametrize('pair', soft_cases.WEIGHTS, ids=lambda p: 'w%g_%g' % p)
@pytest.mark.parametrize('family,N', _ONE)
def test_parity_one_model(handle, family, N, pair):
    cs = soft_cases.case(family, N, 'one', pair)
    _check(cs, _solve(handle, cs), '%s N=%d one %s' % (family, N, pair))


def test_linear_only_and_quadratic_only_weights(handle):
    """l2 = 0 with l1 > 0 and l1 = 0 with l2 > 0 both run: the linear-only penalty (l1 = 1e3, exact)
    reproduces the optimum of (1e3, tiny l2) to the bar; the quadratic-only one against its own
    reference"""
    import bqp
    cs = soft_cases.case('di', 3, 'stg', soft_cases.WEIGHTS[0])
    prob = cs['prob']
    quad = cs['quad'] * 10.0                                  # l2 = 1e3, l1 = 0
    ref = [soft_ref.solve(prob, cs['X'][i], None, quad, cs['A'][i], cs['B'][i], cs['c'][i]) for i in range(len(cs['X']))]
    cq = dict(cs, lin=None, quad=quad, ref=ref)
    _check(cq, _solve(handle, cq), 'di N=3 l1 = 0')
    # linear only (l1 = 1e3, l2 = 0): the exact solver needs a strictly convex problem, so the
    # GPU's point is held to the KKT conditions of the augmented problem instead (convex: they
    # are sufficient); the slack bounds' multipliers nu = l1 - lam follow from the slack's
    # stationarity and must be >= 0 and complementary.  Bars of test_gpu_ocp_ltv.py
    lin = cs['lin'] * 100.0
    r = bqp.solve_ocp(prob, cs['X'], A=cs['A'], B=cs['B'], c=cs['c'], xs_lin=lin, handle=handle, want_duals=True)
    assert (r.exitflag == 1).all(), r.exitflag
    for i in range(len(cs['X'])):
        aug = soft_ref.augment(prob, cs['X'][i], lin, None, cs['A'][i], cs['B'][i], cs['c'][i], strict=False)
        s = soft_ref.slack_rows(aug, r.s_x[i])
        lam = ltv_ref.lam_rows(prob, r.lam_x[i], r.lam_u[i], r.lam_p[i])
        full = np.concatenate([lam, aug['l1'] - lam[aug['soft']]])
        st, comp, lmin, viol = soft_ref.kkt(aug, np.concatenate([_z(r)[i], s]), full)
        print('di N=3 l2 = 0, instance %d: iterations %d, kkt %.2e %.2e %.2e %.2e, max slack %.2e'
              % (i, r.iterations[i], st, comp, lmin, viol, s.max()))
        assert st < 1e-8 and comp < 1e-9 and lmin > -1e-9 and viol < 1e-9, (i, st, comp, lmin, viol)
        assert s.max() > 1e-6


def test_n1_layout_with_feasible_starts(handle):
    """MG N = 1 (soft_cases.N1_NOTE: no start is infeasible when hard and feasible when soft): the
    N = 1 layout runs the soft rows on feasible starts, and the optimum is the hard one"""
    import bqp
    prob = soft_cases.problem('mg', 1)
    X = ltv_cases.states('mg', 16, 0)
    A, B, c = ltv_cases.schedules(prob, 16, 100)
    hard = [ltv_ref.solve(prob, X[i], A[i], B[i], c[i]) for i in range(16)]
    keep = [i for i in range(16) if hard[i]['status'] == 'optimal'][:5]
    assert len(keep) == 5
    # l1 at 10 x the largest hard multiplier of the five: the penalty is exact
    lmax = max(hard[i]['lam'].max() for i in keep)
    lin, quad = soft_cases.weights(prob, 'mg', (10.0 * max(lmax, 1.0), 1e3))
    r = bqp.solve_ocp(prob, X[keep], A=A[keep], B=B[keep], c=c[keep], xs_lin=lin, xs_quad=quad,
                      handle=handle, want_duals=True)
    print('mg N=1: flags %s iterations %s l1 %.3g max slack %.2e' % (
        r.exitflag.tolist(), r.iterations.tolist(), lin.max(), r.s_x.max()))
    assert (r.exitflag == 1).all(), r.exitflag
    for j, i in enumerate(keep):
        assert np.abs(_z(r)[j] - hard[i]['z']).max() <= TOL * max(1.0, np.abs(hard[i]['z']).max())
    assert r.s_x.max() <= 1e-9


def test_exact_penalty_keeps_the_hard_optimum(handle):
    """feasible instances with l1 at 10 x their largest hard state-row multiplier: the soft optimum
    is the hard one and every slack is 0 (test_soft_host.py states the same of the reference).
    A soft problem has no active-set polish, so the flag is held to 1 on the instances on which
    the hard interior point itself converges without its polish (polish -1); on the others (one of
    five here: the hard solve also runs into the iteration limit and is repaired by the polish)
    the soft solve must end where the unpolished hard one does."""
    import bqp
    from test_soft_host import exact_penalty_case
    cs, lin, quad = exact_penalty_case()
    prob = cs['prob']
    kw = dict(A=cs['A'], B=cs['B'], c=cs['c'], handle=handle, want_duals=True)
    hard = bqp.solve_ocp(prob, cs['X'], polish=-1, **kw)
    r = bqp.solve_ocp(prob, cs['X'], xs_lin=lin, xs_quad=quad, **kw)
    ez = np.array([np.abs(_z(r)[i] - q['z']).max() / max(1.0, np.abs(q['z']).max()) for i, q in enumerate(cs['ref'])])
    print('exact penalty: flags %s (hard, unpolished: %s) iterations %s |z - z_hard| %s max slack %.2e' % (
        r.exitflag.tolist(), hard.exitflag.tolist(), r.iterations.tolist(), ez, r.s_x.max()))
    conv = hard.exitflag == 1
    assert conv.sum() >= 3
    assert (r.exitflag[conv] == 1).all()
    assert np.array_equal(r.exitflag[~conv], hard.exitflag[~conv])
    assert ez[conv].max() <= TOL
    assert r.s_x.max() <= 1e-9 and r.s_x.min() >= 0.0


def test_shared_weights_are_the_repeated_ones(handle):
    import bqp
    cs = soft_cases.case('mg', 25, 'stg', soft_cases.WEIGHTS[0])
    n = len(cs['X'])
    rs = _solve(handle, cs)
    rr = _solve(handle, dict(cs, lin=np.tile(cs['lin'], (n, 1, 1)), quad=np.tile(cs['quad'], (n, 1, 1))))
    assert (rs.exitflag == 1).all()
    for k in ('x', 'u', 'theta', 'fval', 'exitflag', 'iterations', 'pi', 'lam_x', 'lam_u', 'lam_p', 's_x'):
        assert np.array_equal(rs[k], rr[k]), k
    # per-instance weights are read per instance: instance 1 with ten times the weights
    lin = np.tile(cs['lin'], (n, 1, 1)); quad = np.tile(cs['quad'], (n, 1, 1))
    lin[1] *= 10; quad[1] *= 10
    rp = _solve(handle, dict(cs, lin=lin, quad=quad))
    assert not np.array_equal(rp.u[1], rs.u[1])
    for i in (0, 2, 3, 4):
        assert np.array_equal(rp.u[i], rs.u[i]) and np.array_equal(rp.s_x[i], rs.s_x[i])


def _raw(handle, prob, dims, data, n, opts=None):
    """bqp_solve_ocp_batched on a packed (dims, data) with every output, s_x included"""
    from bqp import _lib
    N, nx, nu, npar, mp = prob.N, prob.nx, prob.nu, prob.np, prob.mp
    r = dict(x=np.zeros((n, N + 1, nx)), u=np.zeros((n, N, nu)), theta=np.zeros((n, npar)),
             fval=np.zeros(n), exitflag=np.full(n, 77, np.int32), pi=np.zeros((n, N, nx)),
             lam_x=np.zeros((n, N + 1, 2, nx)), lam_u=np.zeros((n, N, 2, nu)), lam_p=np.zeros((n, mp)),
             s_x=np.zeros((n, N + 1, 2, nx)))
    out = (_lib.Output * n)()
    dd = _lib.OcpDuals(*(_lib.ptr(r[k]) for k in ('pi', 'lam_x', 'lam_u', 'lam_p', 's_x')))
    o = _lib.options(**(opts or {}))
    rc = _lib.load().bqp_solve_ocp_batched(handle.value, C.byref(dims), n, C.byref(data), C.byref(o),
                                           _lib.ptr(r['x']), _lib.ptr(r['u']), _lib.ptr(r['theta']),
                                           _lib.ptr(r['fval']), _lib.iptr(r['exitflag']), out, C.byref(dd))
    r['iterations'] = np.array([o_.iterations for o_ in out])
    return rc, r


_OUT = ('x', 'u', 'theta', 'fval', 'exitflag', 'iterations', 'pi', 'lam_x', 'lam_u', 'lam_p', 's_x')


def test_instance_infeasible_when_soft_is_isolated(handle):
    """an empty input box makes instance 2 infeasible whatever the slacks: it ends -2, and the
    other instances' bits are those of the batch without it"""
    from bqp import _lib
    from bqp.ocp import pack
    cs = soft_cases.case('mg', 25, 'stg', soft_cases.WEIGHTS[0])
    prob, X = cs['prob'], cs['X']
    N, n = prob.N, len(X)
    dims, data, _, keep = pack(prob, X, A=cs['A'], B=cs['B'], c=cs['c'], xs_lin=cs['lin'], xs_quad=cs['quad'])
    rc, base = _raw(handle, prob, dims, data, n)
    assert rc == 0 and (base['exitflag'] == 1).all()
    ulb = np.ascontiguousarray(np.tile(prob.ulb, (n, 1, 1)))
    uub = np.ascontiguousarray(np.tile(prob.uub, (n, 1, 1)))
    ulb[2, 3, 0], uub[2, 3, 0] = 0.5, -0.5
    data.ulb, data.uub, data.sub = _lib.ptr(ulb), _lib.ptr(uub), N * prob.nu
    rc, r = _raw(handle, prob, dims, data, n)
    assert rc == 0
    assert r['exitflag'][2] == -2, r['exitflag']
    others = np.array([0, 1, 3, 4])
    assert (r['exitflag'][others] == 1).all()
    for k in _OUT:
        assert np.array_equal(r[k][others], base[k][others]), k


def test_error_codes(handle):
    from bqp import _lib
    from bqp.ocp import pack
    cs = soft_cases.case('mg', 25, 'stg', soft_cases.WEIGHTS[0])
    prob, X = cs['prob'], cs['X']
    n = len(X)
    kw = dict(A=cs['A'], B=cs['B'], c=cs['c'])
    dims, data, _, keep = pack(prob, X, xs_lin=cs['lin'], xs_quad=cs['quad'], **kw)
    assert _raw(handle, prob, dims, data, n)[0] == _lib.BQP_OK
    assert _raw(handle, prob, dims, data, n, dict(precision=1))[0] == _lib.BQP_E_UNSUPPORTED
    assert _raw(handle, prob, dims, data, n, dict(precision=2))[0] == _lib.BQP_E_UNSUPPORTED
    for name in ('lin', 'quad'):
        for bad in (-1.0, np.nan, np.inf):
            wts = dict(lin=cs['lin'].copy(), quad=cs['quad'].copy())
            wts[name][3, 1] = bad
            dims, data, _, keep = pack(prob, X, xs_lin=wts['lin'], xs_quad=wts['quad'], **kw)
            assert _raw(handle, prob, dims, data, n)[0] == _lib.BQP_E_ARG, (name, bad)
    # a per-instance stride that does not span the instance's weights
    dims, data, _, keep = pack(prob, X, xs_lin=np.tile(cs['lin'], (n, 1, 1)), xs_quad=np.tile(cs['quad'], (n, 1, 1)), **kw)
    data.sxs -= 1
    assert _raw(handle, prob, dims, data, n)[0] == _lib.BQP_E_ARG
    # the condensed route has no soft form
    import bqp
    with pytest.raises(ValueError):
        bqp.solve_ocp(prob, X, xs_lin=cs['lin'], xs_quad=cs['quad'], route='condensed', handle=handle)


# ---- closed loop (bqp_closed_loop_track): DI N = 3, eight steps, a disturbance that carries the
#      state 0.05 outside the box after the first step ----
LOOP_PAIR = (10.0, 100.0)
LOOP_STEPS = 8
LOOP_OUT = 0.05


def loop_inputs():
    """(prob with soft weights, X0 (5, 2), dist (5, 8, 2)): the five DI N = 3 starts of
    soft_cases (stored velocities towards the bound) with x1 moved 0.05 inside its lower bound,
    and the disturbance of step 0 that puts x1 of the next state LOOP_OUT below the bound, from the
    reference's own first move.  Checked on the CPU with the reference in the loop: every step is
    optimal, and the slacks reach 0.04 .. 0.2 on the way back into the box."""
    prob = soft_cases.problem('di', 3)
    lin, quad = soft_cases.weights(prob, 'di', LOOP_PAIR)
    prob.xs_lin, prob.xs_quad = lin, quad
    seed, idx = soft_cases.PICKS[('di', 3, 'one')]
    X0 = soft_cases.pool('di', prob, seed, 'one')[0][list(idx)]
    X0[:, 0] = prob.xlb[1][0] + LOOP_OUT
    dist = np.zeros((len(X0), LOOP_STEPS, 2))
    for b, x in enumerate(X0):
        q = soft_ref.solve(prob, x, lin, quad)
        assert q['status'] == 'optimal'
        nxt = prob.A @ x + prob.B @ q['u'][0] + prob.c
        dist[b, 0, 0] = (prob.xlb[1][0] - LOOP_OUT) - nxt[0]
    return prob, X0, dist


def test_closed_loop_track_with_disturbance(handle):
    import bqp
    prob, X0, dist = loop_inputs()
    r = bqp.closed_loop(types.SimpleNamespace(prob=prob), X0, LOOP_STEPS, plant='linear', dist=dist,
                        handle=handle)
    assert (r.exitflag == 1).all(), r.exitflag
    assert np.abs(r.X[:, 1, 0] - (prob.xlb[1][0] - LOOP_OUT)).max() < 1e-7     # the state is outside
    eu, smax = 0.0, 0.0
    for b in range(len(X0)):
        for t in range(LOOP_STEPS):
            q = soft_ref.solve(prob, r.X[b, t], prob.xs_lin, prob.xs_quad)
            assert q['status'] == 'optimal', (b, t)
            eu = max(eu, np.abs(r.U[b, t] - q['u'][0]).max())
            smax = max(smax, q['s'].max())
            nxt = prob.A @ r.X[b, t] + prob.B @ r.U[b, t] + prob.c + dist[b, t]
            assert np.abs(r.X[b, t + 1] - nxt).max() < 1e-12
    print('closed loop: |u_0 - ref| %.2e, largest reference slack %.2e' % (eu, smax))
    assert smax > 1e-3                                         # slacks were active on the way
    assert eu <= 1e-8, eu
