"""GPU: the structured solve with per-stage models (bqp_ocp_dims.stage_models = 1) against the
exact optimum of the same problem condensed in numpy (tests/ltv_ref.py, cases of
tests/ltv_cases.py): both model families, one and two stages per lane (63 | 64) up to the limit
N = 127, shared and per-instance schedules, the multipliers, a batch beyond the resident slots,
isolation of an infeasible and of a skipped instance, and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import dual_map as dm
import ltv_cases
import ltv_ref

pytestmark = pytest.mark.gpu

TOL = 1e-8          # |z - z*|_inf / max(1, |z*|_inf): the project's standing bar
TOL_KKT = 1e-8      # the bars of test_gpu_duals.py
TOL_LAM = 1e-7


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


_cases = {}


def _case(family, N):
    if (family, N) not in _cases:
        _cases[(family, N)] = ltv_cases.case(family, N)
    return _cases[(family, N)]


def _z(r):
    return np.concatenate([r.u.reshape(len(r.u), -1), r.theta], axis=1)


def _zerr(r, ref):
    z = _z(r)
    return max(np.abs(z[i] - ref[i]['z']).max() / max(1.0, np.abs(ref[i]['z']).max())
               for i in range(len(ref)))


@pytest.mark.parametrize('family,N', [('mg', 3), ('mg', 20), ('mg', 63), ('mg', 64), ('mg', 100),
                                      ('mg', 127), ('di', 3), ('di', 30)])
def test_parity_with_exact_optimum(handle, family, N):
    import bqp
    cs = _case(family, N)
    prob, ref = cs['prob'], cs['ref']
    assert all(r['status'] == 'optimal' for r in ref)          # the construction, not the solver
    r = bqp.solve_ocp(prob, cs['X'], A=cs['A'], B=cs['B'], c=cs['c'], handle=handle, want_duals=True)
    print('%s N=%d: flags %s iterations %s polished %s |z - z*| %.2e' % (
        family, N, r.exitflag.tolist(), r.iterations.tolist(), r.polished.tolist(), _zerr(r, ref)))
    assert (r.exitflag == 1).all(), r.exitflag
    assert _zerr(r, ref) <= TOL
    nx = prob.nx
    compared = 0
    for i in range(len(ref)):
        qp = ref[i]['qp']
        lam = ltv_ref.lam_rows(prob, r.lam_x[i], r.lam_u[i], r.lam_p[i])
        st, comp, lmin, viol = dm.f1_kkt(qp, _z(r)[i], lam)
        assert st < TOL_KKT and comp < 1e-9 and lmin > -1e-12 and viol < 1e-9, (i, st, comp, lmin, viol)
        # the states follow the stage's own model, and so do the dynamics multipliers
        for k in range(N):
            xn = cs['A'][i, k] @ r.x[i, k] + cs['B'][i, k] @ r.u[i, k] + cs['c'][i, k]
            assert np.abs(xn - r.x[i, k + 1]).max() <= 1e-9 * max(1.0, np.abs(r.x[i]).max())
        if dm.licq(qp['A'], lam, ref[i]['lam']):
            compared += 1
            sc = max(1.0, np.abs(ref[i]['lam']).max())
            assert np.abs(lam - ref[i]['lam']).max() / sc < TOL_LAM, i
            # pi* from the exact optimum by stationarity in x_N .. x_1 through A_k'
            m = ref[i]['lam']
            lx = np.zeros_like(r.lam_x[i])
            pos = 0
            for k in range(1, N + 1):
                for h, bd in ((1, prob.xub[k]), (0, prob.xlb[k])):
                    sel = np.isfinite(bd)
                    lx[k, h][sel] = m[pos:pos + sel.sum()]; pos += sel.sum()
            pos += sum(int(np.isfinite(prob.uub[k]).sum() + np.isfinite(prob.ulb[k]).sum()) for k in range(N))
            pis = ltv_ref.pi_from(prob, ref[i]['x'], ref[i]['u'], ref[i]['theta'], cs['A'][i], lx, m[pos:])
            scp = max(1.0, np.abs(pis).max(), np.abs(ref[i]['lam']).max())
            assert np.abs(r.pi[i] - pis).max() / scp < TOL_LAM, (i, np.abs(r.pi[i] - pis).max(), scp)
            assert r.pi.shape[2] == nx
    print('%s N=%d: lam and pi compared with the exact multipliers on %d of %d instances; active rows %s'
          % (family, N, compared, len(ref), [int((q['lam'] > 1e-9).sum()) for q in ref]))
    # every instance has active rows (ltv_cases), and the multipliers were compared on some of them
    assert all((q['lam'] > 1e-9).any() for q in ref) and compared >= 1


def test_shared_schedule_is_the_repeated_one(handle):
    import bqp
    cs = _case('mg', 20)
    prob, X = cs['prob'], cs['X']
    A, B, c = cs['A'][1], cs['B'][1], cs['c'][1]
    rs = bqp.solve_ocp(prob, X, A=A, B=B, c=c, handle=handle, want_duals=True)
    n = len(X)
    rr = bqp.solve_ocp(prob, X, A=np.tile(A, (n, 1, 1, 1)), B=np.tile(B, (n, 1, 1, 1)),
                       c=np.tile(c, (n, 1, 1)), handle=handle, want_duals=True)
    assert (rs.exitflag == 1).all()
    for k in ('x', 'u', 'theta', 'fval', 'exitflag', 'iterations', 'pi', 'lam_x', 'lam_u', 'lam_p'):
        assert np.array_equal(rs[k], rr[k]), k


@pytest.mark.parametrize('family,N', [('mg', 20), ('mg', 100), ('di', 30)])
def test_equal_models_against_the_one_model_path(handle, family, N):
    import bqp
    cs = _case(family, N)
    prob, X = cs['prob'], cs['X']
    # the problem's own model with a constant drift c = 1e-3 N(0, 1) / N: the recipe's per-stage size
    # spread over the horizon, since a constant c accumulates to N c.  (c = 1e-3 N(0, 1) kept over
    # 100 stages carries two of the MG states out of the feasible set; at 1e-4 the N = 100 problems
    # sit at its edge, take 13 to 16 iterations, and the two calls, equal in every bit, were both
    # 7.7e-8 from the exact optimum: the interior-point accuracy on that problem, not the models.)
    A, B, c = prob.A, prob.B, cs['c'][0, 0] / N
    ref = [ltv_ref.solve(prob, x, A, B, c) for x in X]
    assert all(r['status'] == 'optimal' for r in ref)
    lti = bqp.solve_ocp(prob, X, A=np.tile(A, (len(X), 1, 1)), B=np.tile(B, (len(X), 1, 1)),
                        c=np.tile(c, (len(X), 1)), handle=handle)
    ltv = bqp.solve_ocp(prob, X, A=np.tile(A, (N, 1, 1)), B=np.tile(B, (N, 1, 1)), c=np.tile(c, (N, 1)),
                        stage_models=True, handle=handle)
    print('%s N=%d: |z_ltv - z_lti| %.2e, iterations lti %s ltv %s' % (
        family, N, np.abs(_z(ltv) - _z(lti)).max(), lti.iterations.tolist(), ltv.iterations.tolist()))
    assert _zerr(lti, ref) <= TOL and _zerr(ltv, ref) <= TOL
    assert np.array_equal(lti.exitflag, ltv.exitflag) and (ltv.exitflag == 1).all()


def test_large_batch(handle):
    """3000 instances (beyond the resident slots) cycling eight schedules and five states"""
    import bqp
    cs = _case('mg', 20)
    prob = ltv_cases.mg_prob(20)          # the original input box: all 40 (schedule, state) pairs feasible
    A, B, c = ltv_cases.schedules(prob, 8, 77)
    X5 = cs['X']
    n = 3000
    si, xi = np.arange(n) % 8, np.arange(n) % 5
    ref = {}
    for j in range(40):
        ref[(j % 8, j % 5)] = ltv_ref.solve(prob, X5[j % 5], A[j % 8], B[j % 8], c[j % 8])
        assert ref[(j % 8, j % 5)]['status'] == 'optimal'
    r = bqp.solve_ocp(prob, X5[xi], A=A[si], B=B[si], c=c[si], handle=handle)
    assert (r.exitflag == 1).all()
    z = _z(r)
    zs = np.array([ref[(int(s), int(x))]['z'] for s, x in zip(si, xi)])
    err = np.abs(z - zs).max(axis=1) / np.maximum(1.0, np.abs(zs).max(axis=1))
    assert err.max() <= TOL, err.max()


def _raw(handle, prob, dims, data, n, mark=0.0, duals=True):
    """bqp_solve_ocp_batched on a packed (dims, data) with outputs preset to mark"""
    from bqp import _lib
    N, nx, nu, npar, mp = prob.N, prob.nx, prob.nu, prob.np, prob.mp
    r = dict(x=np.full((n, N + 1, nx), mark), u=np.full((n, N, nu), mark), theta=np.full((n, npar), mark),
             fval=np.full(n, mark), exitflag=np.full(n, 77, np.int32), pi=np.full((n, N, nx), mark),
             lam_x=np.full((n, N + 1, 2, nx), mark), lam_u=np.full((n, N, 2, nu), mark),
             lam_p=np.full((n, mp), mark))
    out = (_lib.Output * n)()
    for o_ in out:
        o_.iterations = -5
    dd = _lib.OcpDuals(*(_lib.ptr(r[k]) for k in ('pi', 'lam_x', 'lam_u', 'lam_p')))
    o = _lib.options()
    rc = _lib.load().bqp_solve_ocp_batched(handle.value, C.byref(dims), n, C.byref(data), C.byref(o),
                                           _lib.ptr(r['x']), _lib.ptr(r['u']), _lib.ptr(r['theta']),
                                           _lib.ptr(r['fval']), _lib.iptr(r['exitflag']), out,
                                           C.byref(dd) if duals else None)
    assert rc == 0, rc
    r['iterations'] = np.array([o_.iterations for o_ in out])
    return r


_OUT = ('x', 'u', 'theta', 'fval', 'exitflag', 'iterations', 'pi', 'lam_x', 'lam_u', 'lam_p')


def test_infeasible_instance_is_isolated(handle):
    from bqp import _lib
    from bqp.ocp import pack
    cs = _case('mg', 20)
    prob, X = cs['prob'], cs['X']
    N, n = prob.N, len(X)
    dims, data, _, keep = pack(prob, X, A=cs['A'], B=cs['B'], c=cs['c'])
    base = _raw(handle, prob, dims, data, n)
    assert (base['exitflag'] == 1).all()
    # per-instance state bounds (stride (N + 1) nx); instance 2: lower above upper at stage 5
    xlb = np.ascontiguousarray(np.tile(prob.xlb, (n, 1, 1)))
    xub = np.ascontiguousarray(np.tile(prob.xub, (n, 1, 1)))
    xlb[2, 5, 0], xub[2, 5, 0] = 0.5, -0.5
    data.xlb, data.xub, data.sxb = _lib.ptr(xlb), _lib.ptr(xub), (N + 1) * 4
    r = _raw(handle, prob, dims, data, n)
    assert r['exitflag'][2] == -2, r['exitflag']
    others = np.array([0, 1, 3, 4])
    assert (r['exitflag'][others] == 1).all()
    for k in _OUT:
        assert np.array_equal(r[k][others], base[k][others]), k


def test_skipped_instance_is_untouched(handle):
    from bqp.ocp import pack
    cs = _case('mg', 100)
    prob, X = cs['prob'], cs['X']
    n = len(X)
    dims, data, _, keep = pack(prob, X, A=cs['A'], B=cs['B'], c=cs['c'])
    base = _raw(handle, prob, dims, data, n)
    dims, data, _, keep = pack(prob, X, A=cs['A'], B=cs['B'], c=cs['c'], skip=[0, 1, 0, 0, 1])
    mark = -7.25
    r = _raw(handle, prob, dims, data, n, mark=mark)
    for i in (1, 4):
        for k in _OUT:
            want = 77 if k == 'exitflag' else (-5 if k == 'iterations' else mark)
            assert (r[k][i] == want).all(), (i, k)
    for i in (0, 2, 3):
        assert r['exitflag'][i] == 1
        for k in _OUT:
            assert np.array_equal(r[k][i], base[k][i]), (i, k)


def test_arguments(handle):
    from bqp import _lib
    from bqp.ocp import pack
    cs = _case('mg', 20)
    prob, X = cs['prob'], cs['X']
    N, n = prob.N, len(X)
    lib = _lib.load()

    def call(dims, data, **opts):
        x = np.zeros((n, N + 1, 4)); u = np.zeros((n, N, 1)); th = np.zeros((n, 1))
        flag = np.zeros(n, np.int32)
        o = _lib.options(**opts)
        return lib.bqp_solve_ocp_batched(handle.value, C.byref(dims), n, C.byref(data), C.byref(o),
                                         _lib.ptr(x), _lib.ptr(u), _lib.ptr(th), None,
                                         _lib.iptr(flag), None, None)

    dims, data, _, keep = pack(prob, X, A=cs['A'], B=cs['B'], c=cs['c'])
    assert call(dims, data) == _lib.BQP_OK
    for name, full in (('sA', N * 16), ('sB', N * 4), ('sc', N * 4)):
        setattr(data, name, full - 1)
        assert call(dims, data) == _lib.BQP_E_ARG, name
        setattr(data, name, full)
    assert call(dims, data, precision=1) == _lib.BQP_E_UNSUPPORTED
    assert call(dims, data, precision=2) == _lib.BQP_E_UNSUPPORTED
    for v in (2, -1):
        dims.stage_models = v
        assert call(dims, data) == _lib.BQP_E_ARG
    # skip marks belong to the per-stage-model solve
    dims1, data1, _, keep1 = pack(prob, X)
    sk = np.zeros(n, np.int32)
    data1.skip = _lib.iptr(sk)
    assert call(dims1, data1) == _lib.BQP_E_UNSUPPORTED
