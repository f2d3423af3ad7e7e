"""GPU checks of the nonlinear MPC's direct multiple shooting (bqp_nmpc_dims.shooting = 1: the
states stay decision variables, the stage sub-problem carries the shooting defects) against the
numpy restatement (tests/nmpc_dms_ref.py), single shooting's solutions, the library's own
step-synchronous loop and the reference's stored tracking-NMPC closed loop."""
import ctypes as C
import os

import numpy as np
import pytest

import nmpc_dms_ref as DR
import nmpc_ref as R
import nmpc_stage_ref as SR
from oracle.mg_model import mg_rk4
from test_gpu_nmpc_stage import BAD, DEVS, KEYS, STAGE_BAR, _rel, handle, probs, xnl   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

# The defects c_k = f_k - x_{k+1} against the restatement, absolute: both sides run the same
# operations on the same (x_k, u_k, x_{k+1}); they differ where the compiler contracts a multiply-add,
# by at most one rounding of the partial sum.  The largest partial sums of `system` are 1000 x3 and
# 1000 u in its fourth entry (< 2^9, ulp 1.1e-13); some 12 such roundings over the four RK stages
# enter x4 with the weight 2 delta / 6 = 3.3e-3: 4.5e-15, and the final x + delta / 6 (..) rounds at
# 2.2e-16 |x|.  The bar is four times that.  (Relative to max |c| ~ 1e-3 it would be 2e-11.)
C_BAR = 2e-14

# the stored run's states of the solve tests: CASES of tests/test_gpu_nmpc_stage.py where it has the
# horizon, its N = 64 pair at 65
CASES = {3: (0, 5, 20, 40, 60, 80), 10: (0, 5, 20, 40, 60, 80), 64: (20, 40), 65: (20, 40)}


@pytest.fixture(autouse=True)
def exact_fallback(monkeypatch):
    """the restatements' dense sub-problem solver hands a degenerate vertex to their exact one"""
    monkeypatch.setattr(R.dense_qp, 'solve', DR.qp_solve)


def _box(p):
    """the state box of F_x, h_x in absolute coordinates"""
    rows, _ = SR.bound_map(p['F_x'], p['F_u'])
    lo, hi = np.full(4, -np.inf), np.full(4, np.inf)
    for i, (var, side, a) in enumerate(rows[:p['F_x'].shape[0]]):
        if side:
            hi[var] = p['x_eq'][var] + p['h_x'][i] / a
        else:
            lo[var] = p['x_eq'][var] - p['h_x'][i] / a
    return lo, hi


def kkt_ok(p, x0, X, z, lam, pi):
    """the constants of _kkt_ok in tests/test_gpu_nmpc_stage.py on the full-space residuals"""
    k = DR.kkt(p, x0, X, z, lam, pi)
    assert k['stat'] <= 1e-6 * (1.0 + k['grad']), k
    assert k['cmax'] <= 1e-9 and k['dmax'] <= 1e-9, k
    assert k['lam_min'] >= 0.0, k


# ---- 1. the sub-problem ---------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 2, 3, 63, 64, 65, 127])
def test_dms_qp_matches_restatement(probs, handle, N):
    """A, B, c, w, bounds, hp at X = rollout + a seeded 1e-3 perturbation kept inside the box, batch
    3.  N = 63 / 64 / 65: the lanes' second pass and the structured kernel's LDS-table edge"""
    p, g = probs(N)
    rng = np.random.default_rng(300 + N)
    X0 = p['x_eq'] + DEVS[[1, 3, 5]]
    Z = np.concatenate([rng.uniform(-0.3, 0.3, (3, N)), rng.uniform(-0.1, 0.1, (3, 1))], 1)
    lo, hi = _box(p)
    X = np.zeros((3, N + 1, 4))
    for i in range(3):
        Xr = DR.consistent(p, X0[i], Z[i])
        Xp = Xr + rng.uniform(-1e-3, 1e-3, Xr.shape)
        X[i] = np.where((Xr >= lo) & (Xr <= hi), np.clip(Xp, lo, hi), Xp)
        X[i, 0] = X0[i]
    r = g.dms_qp(X0, X, Z, handle=handle)
    worst = {}
    for i in range(3):
        sp = DR.dms_problem(p, X0[i], X[i], Z[i])
        assert np.abs(sp['c']).max() > 1e-4
        for key in STAGE_BAR:
            got = r[key] if key in ('W', 'Fp') else r[key][i]
            fin = np.isfinite(sp[key])
            assert np.array_equal(np.asarray(got)[~fin], sp[key][~fin]), key     # the infinite bounds
            worst[key] = max(worst.get(key, 0.0), _rel(got, sp[key]))
        worst['c'] = max(worst.get('c', 0.0), np.abs(r.c[i] - sp['c']).max())
    print('N %d multiple-shooting sub-problem, relative to max-abs (c absolute): %s' % (N, worst))
    for key, v in worst.items():
        assert v <= (C_BAR if key == 'c' else STAGE_BAR[key]), (key, v)
    # without states: the rollout of z, where the defects vanish to rounding
    r0 = g.dms_qp(X0, None, Z, handle=handle)
    assert np.abs(r0.c).max() <= C_BAR


# ---- 2. solves ------------------------------------------------------------------------------
def _raw_solve(lib, handle, g, dims, x0, z0, X=None, want_pi=False):
    """the C entries themselves: bqp_nmpc_dms_solve_batched with X (None: NULL), or
    bqp_nmpc_solve_batched where X is False"""
    from bqp import _lib
    b = x0.shape[0]
    z = z0.copy(); lam = np.zeros((b, g.m)); pi = np.zeros((b, g.N, 4)); cost = np.zeros(b)
    fl = np.zeros(b, np.int32); it = np.zeros(b, np.int32)
    dd = g._data(x0)
    o = _lib.options(max_iter=100, polish=0)
    if X is False:
        rc = lib.bqp_nmpc_solve_batched(handle.value, C.byref(dims), b, C.byref(dd), C.byref(o), _lib.ptr(z),
                                        _lib.ptr(lam), _lib.ptr(cost), _lib.iptr(fl), _lib.iptr(it))
    else:
        rc = lib.bqp_nmpc_dms_solve_batched(handle.value, C.byref(dims), b, C.byref(dd), C.byref(o), _lib.ptr(z),
                                            _lib.ptr(X) if X is not None else None, _lib.ptr(lam),
                                            _lib.ptr(pi) if want_pi else None, _lib.ptr(cost), _lib.iptr(fl),
                                            _lib.iptr(it))
    return rc, z, lam, pi, cost, fl, it


@pytest.mark.parametrize('N', sorted(CASES))
def test_dms_solve(probs, handle, xnl, N):
    """from the consistent and from the flat start: flag 1, the full-space KKT check on the returned
    (X, z, lam, pi), z within 1e-6 of the restatement's from the same start, X[:, 0] = x0; the entry
    without X is the entry with X = NULL bit for bit"""
    from bqp import _lib
    p, g = probs(N)
    X0 = np.ascontiguousarray(xnl[:, list(CASES[N])].T)
    b = X0.shape[0]
    flat = np.stack([DR.flat(p, x) for x in X0])
    for name, Xs in (('consistent', None), ('flat', flat)):
        r = g.solve(X0, handle=handle, subproblem='stage', shooting='multiple', X0=Xs)
        print('N %d %s start: flags %s iterations %s' % (N, name, r.exitflag.tolist(), r.iterations.tolist()))
        assert (r.exitflag == 1).all(), r.exitflag
        assert np.array_equal(r.X[:, 0], X0)
        for i in range(b):
            _, z, _, _, info = DR.sqp(p, X0[i], X0=None if Xs is None else Xs[i])
            assert info['exitflag'] == 1, info
            err = np.abs(r.z[i] - z).max()
            print('  t = %d: |z - restated| %.2e (%d iterations, restated %d)'
                  % (CASES[N][i], err, r.iterations[i], info['iterations']))
            assert err <= 1e-6, (i, err)
            kkt_ok(p, X0[i], r.X[i], r.z[i], r.lam[i], r.pi[i])
            assert np.array_equal(r.y_OL[i, :4 * (N + 1)], r.X[i].ravel())
    lib = _lib.load()
    dims = g._dims('stage', 'multiple')
    z0 = np.zeros((b, N + 1))
    a = _raw_solve(lib, handle, g, dims, X0, z0, X=False)
    c = _raw_solve(lib, handle, g, dims, X0, z0, X=None)
    assert a[0] == c[0] == _lib.BQP_OK and (a[5] == 1).all()
    for k in (1, 2, 4, 5, 6):
        assert np.array_equal(a[k], c[k]), k


# ---- 3. isolation ---------------------------------------------------------------------------
def test_isolation(probs, handle):
    """the instance that is infeasible in its hard rows ends -2 and leaves the other six bitwise as
    without it, and as alone"""
    p, g = probs(10)
    X7 = np.vstack([p['x_eq'] + DEVS, p['x_eq'] + BAD])
    kw = dict(handle=handle, subproblem='stage', shooting='multiple')
    r7 = g.solve(X7, **kw)
    r6 = g.solve(X7[:6], **kw)
    print('flags %s iterations %s' % (r7.exitflag.tolist(), r7.iterations.tolist()))
    assert r7.exitflag[6] == -2, r7.exitflag
    assert (r7.exitflag[:6] == 1).all(), r7.exitflag
    for k in ('z', 'X', 'lam', 'pi', 'iterations', 'cost'):
        assert np.array_equal(r7[k][:6], r6[k]), k
    for i in range(6):
        r1 = g.solve(X7[i:i + 1], **kw)
        for k in ('z', 'X', 'lam', 'pi', 'iterations', 'cost'):
            assert np.array_equal(r1[k][0], r7[k][i]), (i, k)


# ---- 4. closed loop -------------------------------------------------------------------------
def _loop(g, xi, steps, handle, sync, **kw):
    import bqp
    assert 'BQP_NMPC_SYNC' not in os.environ
    kw = dict(kw, handle=handle, subproblem='stage', shooting='multiple')
    if not sync:
        return bqp.closed_loop_nmpc(g, xi, steps, **kw)
    os.environ['BQP_NMPC_SYNC'] = '1'
    try:
        return bqp.closed_loop_nmpc(g, xi, steps, **kw)
    finally:
        del os.environ['BQP_NMPC_SYNC']


@pytest.mark.parametrize('N', [20, 65])
def test_loop_asynchronous_equals_synchronous(probs, handle, xnl, N):
    """batch 6, 5 steps, both loop modes bit for bit; the rounds identity of
    tests/test_gpu_nmpc_async.py; every plant transition against mg_rk4"""
    p, g = probs(N)
    xi, steps = np.ascontiguousarray(xnl[:, [4, 12, 24, 40, 80, 0]].T), 5
    ra = _loop(g, xi, steps, handle, False)
    rs = _loop(g, xi, steps, handle, True)
    rounds = int((ra.iterations + (ra.exitflag != 0)).sum(axis=1).max())
    print('iterations\n%s\nflags\n%s\nrounds: asynchronous %d, from its logs %d, step-synchronous %d; launches %d'
          % (ra.iterations, ra.exitflag, ra.rounds, rounds, rs.rounds, ra.launches))
    for k in KEYS:
        assert np.array_equal(ra[k], rs[k]), k
    assert ra.rounds == rounds
    assert (ra.exitflag == 1).all(), ra.exitflag
    for b in range(xi.shape[0]):
        for t in range(steps):
            assert np.abs(ra.X[b, t + 1] - mg_rk4(p['delta'], ra.X[b, t], ra.U[b, t])).max() <= 1e-14, (b, t)


def test_stored_closed_loop(probs, handle, xnl):
    """the first 40 steps of DSS_tNMPC.mat at N = 100, the bars of test_stored_closed_loop in
    tests/test_gpu_nmpc_stage.py.  The numpy restatement's loop over these steps (nmpc_dms_ref.sqp
    with warm_start) was run on the CPU first and meets them: 1.18e-9, 9.96e-9, 2.84e-7, 9.94e-5
    per state, every flag 1, 2-4 iterations per step.  Measured here on the MI355X: 1.18e-9, 9.96e-9,
    2.84e-7, 9.94e-5"""
    import bqp
    p, g = probs(100)
    steps = 40
    r = bqp.closed_loop_nmpc(g, xnl[:, :1].T.copy(), steps, handle=handle, subproblem='stage',
                             shooting='multiple')
    err = np.abs(r.X[0].T - xnl[:, :steps + 1]).max(axis=1)
    print('iterations per step: mean %.2f max %d; %.1f ms, %d rounds; max error over %d steps: %s'
          % (r.iterations.mean(), r.iterations.max(), r.kernel_ms, r.rounds, steps, err))
    assert (r.exitflag == 1).all(), r.exitflag
    assert err[0] <= 1e-7 and err[1] <= 1e-7 and err[2] <= 1e-5 and err[3] <= 1e-3, err
    for t in range(steps):
        assert np.abs(r.X[0, t + 1] - mg_rk4(p['delta'], r.X[0, t], r.U[0, t])).max() <= 1e-14, t


# ---- 5. arguments ---------------------------------------------------------------------------
def test_arguments(probs, handle, mg, term_set):
    import bqp
    from bqp import _lib
    p, g = probs(10)
    lib = _lib.load()
    x0 = np.ascontiguousarray(p['x_eq'][None, :] + DEVS[:1])
    z0 = np.zeros((1, 11))
    args = (10, g.mx, g.mu, g.mp)
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 1, 1), x0, z0, X=False)[0] == _lib.BQP_OK
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 1, 2), x0, z0, X=False)[0] == _lib.BQP_E_ARG
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 1, -1), x0, z0, X=False)[0] == _lib.BQP_E_ARG
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 1, 2), x0, z0)[0] == _lib.BQP_E_ARG
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 2, 1), x0, z0, X=False)[0] == _lib.BQP_E_ARG
    # multiple shooting lives on the stage route
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 0, 1), x0, z0, X=False)[0] == _lib.BQP_E_UNSUPPORTED
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 0, 1), x0, z0)[0] == _lib.BQP_E_UNSUPPORTED
    # the entry with the states in its signature is multiple shooting's alone
    assert _raw_solve(lib, handle, g, _lib.NmpcDims(*args, 1, 0), x0, z0)[0] == _lib.BQP_E_ARG
    kw = dict(handle=handle, subproblem='stage', shooting='multiple')
    with pytest.raises(bqp.BqpError, match='unsupported'):
        g.solve(x0, handle=handle, subproblem='dense', shooting='multiple')
    with pytest.raises(bqp.BqpError, match='unsupported'):
        bqp.closed_loop_nmpc(g, x0, 2, handle=handle, shooting='multiple')
    # a softening weight: refused; weights that soften nothing: the hard solve
    with pytest.raises(bqp.BqpError, match='unsupported'):
        g.solve(x0, xs_lin=100.0, **kw)
    with pytest.raises(bqp.BqpError, match='unsupported'):
        bqp.closed_loop_nmpc(g, x0, 2, xs_quad=10.0, **kw)
    rh, r0 = g.solve(x0, **kw), g.solve(x0, xs_lin=0.0, xs_quad=0.0, **kw)
    assert rh.exitflag[0] == 1 and np.array_equal(rh.z, r0.z) and np.array_equal(rh.X, r0.X)
    # a two-entry F_x row
    Fx = np.array(mg['F_x'], float)
    Fx[1, 0] = 0.05
    g2 = bqp.NMPC(mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'], Fx, mg['h_x'],
                  mg['F_u'], mg['h_u'], term_set[0], term_set[1], mg['x_wp'], mg['u_wp'], N=10)
    with pytest.raises(bqp.BqpError, match='unsupported'):
        g2.solve(x0, **kw)
    with pytest.raises(bqp.BqpError, match='unsupported'):
        g2.dms_qp(x0, handle=handle)
    with pytest.raises(bqp.BqpError, match='unsupported'):
        bqp.closed_loop_nmpc(g2, x0, 2, **kw)
    with pytest.raises(ValueError):
        g.solve(x0, handle=handle, shooting='both')
    with pytest.raises(ValueError):
        g.solve(x0, handle=handle, X0=np.zeros((1, 11, 4)))
    # shooting = 0: bitwise what a five-field construction (the field zero-initialised) gives, on
    # both routes and in the loop
    for sub in (0, 1):
        a = _raw_solve(lib, handle, g, _lib.NmpcDims(*args, sub), x0, z0, X=False)
        c = _raw_solve(lib, handle, g, _lib.NmpcDims(*args, sub, 0), x0, z0, X=False)
        assert a[0] == c[0] == _lib.BQP_OK and a[5][0] == 1
        for u, v in zip(a[1:], c[1:]):
            assert np.array_equal(u, v)
    la = bqp.closed_loop_nmpc(g, x0, 3, handle=handle, subproblem='stage')
    lc = bqp.closed_loop_nmpc(g, x0, 3, handle=handle, subproblem='stage', shooting='single')
    for k in KEYS:
        assert np.array_equal(la[k], lc[k]), k
