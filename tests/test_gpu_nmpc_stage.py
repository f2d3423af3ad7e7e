"""GPU checks of the nonlinear MPC's stage route (bqp_nmpc_dims.subproblem = 1: the SQP's
sub-problems in stage form on the structured kernel with per-stage models) against the numpy
restatements (tests/nmpc_ref.py, tests/nmpc_stage_ref.py), the library's own step-synchronous loop
and the reference's stored tracking-NMPC closed loop (tests/golden/nmpc_DSS_tNMPC.npz)."""
import ctypes as C
import os

import numpy as np
import pytest

import nmpc_ref as R
import nmpc_stage_ref as SR
from conftest import golden
from oracle.mg_model import mg_rk4

pytestmark = pytest.mark.gpu

# the six states of tests/test_gpu_nmpc.py (deviations from x_eq)
DEVS = np.array([[-0.35, -0.4, 0, 0], [-0.2, -0.1, 0.05, 0.1], [0.0, 0.0, 0.0, 0.0],
                 [-0.1, 0.05, -0.02, 0.3], [-0.05, -0.05, 0, 0], [0.05, 0.1, 0.02, -0.2]])
BAD = np.array([-0.6, 0.0, 0.0, 0.0])      # x1 = -0.1 < 0: the first sub-problem is infeasible

# The stage problem against tests/nmpc_stage_ref.py, each quantity relative to its own max-abs
# over its finite entries: 10 x the maximum measured on the MI355X over the 72 cases (N = 1, 2, 3,
# 63, 64, 127; DESIGN.md §1 "Nonlinear MPC"; the same operations, fused multiply-adds and another
# summation order).  Measured: A 2.8e-17, B 6.8e-21, w 1.15e-14, xlb 3.55e-16, xub 3.55e-16,
# hp 1.14e-15, W 9.3e-20; ulb, uub and Fp are exact (F_u = +-1 and copies).
STAGE_BAR = dict(A=2.8e-16, B=6.9e-20, w=1.2e-13, xlb=3.6e-15, xub=3.6e-15, ulb=0.0, uub=0.0, hp=1.2e-14,
                 W=9.4e-19, Fp=0.0)
# One case is apart, as in tests/test_gpu_nmpc.py: x = x_eq with z = 0, where w_k = 2 L'L (x_k -
# x_eq) with |x_k - x_eq| ~ 1e-7 .. 1e-6 inherits the rollouts' 1e-16 absolute difference
# (LIN_BAR_EQ's cancellation; f there was measured at 7.5e-10).  Measured 3.62e-10 (N = 63).
STAGE_BAR_EQ = dict(w=3.7e-9)

KEYS = ('X', 'U', 'exitflag', 'iterations')


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


@pytest.fixture(scope='module')
def xnl():
    return golden('nmpc_DSS_tNMPC.npz')['xnl']


@pytest.fixture(scope='module')
def probs(mg, term_set):
    """per horizon, made on demand: the restatement's problem and the GPU problem"""
    import bqp
    made = {}

    def get(N):
        if N not in made:
            p = R.problem(mg, term_set[0], term_set[1], N)
            g = bqp.NMPC(mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'], mg['F_x'],
                         mg['h_x'], mg['F_u'], mg['h_u'], term_set[0], term_set[1], mg['x_wp'],
                         mg['u_wp'], N=N)
            made[N] = (p, g)
        return made[N]
    return get


def _rel(a, ref):
    a, ref = np.asarray(a, float), np.asarray(ref, float)
    fin = np.isfinite(ref)
    assert np.array_equal(a[~fin], ref[~fin])          # the infinite bounds, signs included
    if not fin.any():
        return 0.0
    return np.abs(a[fin] - ref[fin]).max() / np.abs(ref[fin]).max()


# ---- 1. the stage problem -----------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 2, 3, 63, 64, 127])
def test_stage_qp_matches_restatement(probs, handle, N):
    """A, B, w, bounds, hp, W, Fp at z = 0 and at a seeded z from the six states.  N = 1 has no
    interior stage; N = 63 / 64 is the LDS-table / L2 boundary of the per-stage kernel"""
    p, g = probs(N)
    rng = np.random.default_rng(100 + N)
    X0 = p['x_eq'] + DEVS
    Z = np.concatenate([np.zeros((6, N + 1)),
                        np.concatenate([rng.uniform(-0.3, 0.3, (6, N)), rng.uniform(-0.1, 0.1, (6, 1))], 1)])
    X0 = np.concatenate([X0, X0])
    r = g.stage_qp(X0, Z, handle=handle)
    worst, worst_eq = {}, {}
    for i in range(X0.shape[0]):
        sp = SR.stage_problem(p, X0[i], Z[i])
        for key in STAGE_BAR:
            got = r[key] if key in ('W', 'Fp') else r[key][i]
            err = _rel(got, sp[key])
            w = worst_eq if (i == 2 and key in STAGE_BAR_EQ) else worst     # case 2: x_eq, z = 0
            w[key] = max(w.get(key, 0.0), err)
    print('N %d stage problem, relative to max-abs: %s; at x_eq, z = 0: %s' % (N, worst, worst_eq))
    for key, v in worst.items():
        assert v <= STAGE_BAR[key], (key, v)
    for key, v in worst_eq.items():
        assert v <= STAGE_BAR_EQ[key], (key, v)


# ---- 2. solves ----------------------------------------------------------------------------
CASES = {3: (0, 5, 20, 40, 60, 80), 10: (0, 5, 20, 40, 60, 80), 40: (0, 5, 20, 40, 60, 80),
         63: (20, 40), 64: (20, 40), 100: (0, 20, 200), 127: (20,)}


@pytest.fixture(scope='module')
def restated(probs, xnl):
    """the restatement's solutions of the stored states, computed once per horizon"""
    made = {}

    def get(N):
        if N not in made:
            p, _ = probs(N)
            made[N] = [R.sqp(p, xnl[:, t]) for t in CASES[N]]
        return made[N]
    return get


def _kkt_ok(p, x0, z, lam):
    k = R.kkt(p, x0, z, lam)
    assert k['stat'] <= 1e-6 * (1.0 + k['grad']), k
    assert k['cmax'] <= 1e-9, k
    assert k['lam_min'] >= 0.0, k


@pytest.mark.parametrize('N', sorted(CASES))
def test_stage_solve_matches_restatement(probs, handle, xnl, restated, N):
    p, g = probs(N)
    X0 = np.ascontiguousarray(xnl[:, list(CASES[N])].T)
    ref = restated(N)
    # the case set keeps its active rows: state rows (N >= 10), an input row (N = 3), terminal
    # rows (N <= 40), by the restatement's multipliers
    ms = 10
    act = np.array([[(lam[:N * ms].reshape(N, ms)[:, :8] > 1e-6).sum(), (lam[:N * ms].reshape(N, ms)[:, 8:] > 1e-6).sum(),
                     (lam[N * ms:] > 1e-6).sum()] for _, lam, _ in ref])
    print('N %d active rows per case [state, input, terminal]: %s' % (N, act.tolist()))
    if N >= 10:
        assert act[:, 0].max() > 0
    if N == 3:
        assert act[:, 1].max() > 0
    if N <= 40:
        assert act[:, 2].max() > 0
    r = g.solve(X0, handle=handle, subproblem='stage')
    rd = g.solve(X0, handle=handle)
    print('N %d stage flags %s iterations %s; dense route %s; restatement %s'
          % (N, r.exitflag.tolist(), r.iterations.tolist(), rd.iterations.tolist(),
             [info['iterations'] for _, _, info in ref]))
    assert (r.exitflag == 1).all(), r.exitflag
    for i in range(X0.shape[0]):
        z, _, info = ref[i]
        assert info['exitflag'] == 1, info
        du, dth = abs(r.z[i, 0] - z[0]), abs(r.z[i, N] - z[N])
        print('  t = %d: |u0 - ref| %.2e |theta - ref| %.2e' % (CASES[N][i], du, dth))
        assert du <= 1e-6 and dth <= 1e-6, (i, du, dth)
        _kkt_ok(p, X0[i], r.z[i], r.lam[i])          # checks the multiplier map
        assert np.abs(r.y_OL[i] - R.to_y(p, X0[i], r.z[i])).max() <= 1e-12


# ---- 3. isolation ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def seven(probs, handle):
    p, g = probs(10)
    X7 = np.vstack([p['x_eq'] + DEVS, p['x_eq'] + BAD])
    return X7, g.solve(X7, handle=handle, subproblem='stage')


def test_isolation(probs, handle, seven):
    """the infeasible instance ends -2 and leaves the other six bitwise as without it; a batch of 1
    equals the instance inside the batch of 7"""
    p, g = probs(10)
    X7, r7 = seven
    r6 = g.solve(X7[:6], handle=handle, subproblem='stage')
    assert r7.exitflag[6] == -2, r7.exitflag
    assert (r7.exitflag[:6] == 1).all(), r7.exitflag
    assert np.array_equal(r7.z[:6], r6.z) and np.array_equal(r7.lam[:6], r6.lam)
    assert np.array_equal(r7.iterations[:6], r6.iterations)
    r1 = g.solve(X7[3:4], handle=handle, subproblem='stage')
    assert np.array_equal(r1.z[0], r7.z[3]) and np.array_equal(r1.lam[0], r7.lam[3])
    assert r1.iterations[0] == r7.iterations[3]


def test_isolation_across_resident_slots(probs, handle, seven):
    """1,500 instances, the seven repeated: more than the structured kernel's resident slots, so
    its work queue hands instances to slots; each equals its small-batch result bitwise"""
    p, g = probs(10)
    X7, r7 = seven
    idx = np.arange(1500) % 7
    r = g.solve(np.ascontiguousarray(X7[idx]), handle=handle, subproblem='stage')
    assert np.array_equal(r.exitflag, r7.exitflag[idx])
    assert np.array_equal(r.iterations, r7.iterations[idx])
    good = idx != 6
    assert np.array_equal(r.z[good], r7.z[idx][good]) and np.array_equal(r.lam[good], r7.lam[idx][good])


# ---- 4. closed loop -------------------------------------------------------------------------
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


@pytest.mark.parametrize('N', [20, 100])
def test_loop_asynchronous_equals_synchronous(probs, handle, xnl, N):
    """the stage route in both loop modes, bit for bit; the round count from the run's own logs
    (tests/test_gpu_nmpc_async.py's shapes and states)"""
    p, g = probs(N)
    if N == 20:
        xi, steps = np.ascontiguousarray(xnl[:, [4, 12, 24, 40, 80]].T), 8
    else:
        xi, steps = xnl[:, [0, 20, 200, 0]].T.copy(), 3
        xi[3, 0] += 0.02
    ra = _loop(g, xi, steps, handle, False)
    rs = _loop(g, xi, steps, handle, True)
    rounds = int((ra.iterations + (ra.exitflag != 0)).sum(axis=1).max())
    print('iterations\n%s\nflags\n%s\nrounds: asynchronous %d, from its logs %d, step-synchronous %d; launches %d'
          % (ra.iterations, ra.exitflag, ra.rounds, rounds, rs.rounds, ra.launches))
    for k in KEYS:
        assert np.array_equal(ra[k], rs[k]), k
    assert ra.rounds == rounds
    # per round: stage linearisation, structured solve and its repair launch, back-map, trials,
    # update, advance; once: the table launch
    assert ra.launches == 7 * ra.rounds + 1
    for b in range(xi.shape[0]):
        for t in range(steps):
            assert np.abs(ra.X[b, t + 1] - mg_rk4(p['delta'], ra.X[b, t], ra.U[b, t])).max() <= 1e-14, (b, t)


def test_stored_closed_loop(probs, handle, xnl):
    """the first 40 steps of DSS_tNMPC.mat, N = 100, batch 8: the stored instance and seven with
    a +-0.02 seeded perturbation of x1 and x2 (tests/test_gpu_nmpc.py's)"""
    import bqp
    p, g = probs(100)
    steps = 40
    rng = np.random.default_rng(5)
    xi = np.tile(xnl[:, 0], (8, 1))
    xi[1:, :2] += rng.uniform(-0.02, 0.02, (7, 2))
    r = bqp.closed_loop_nmpc(g, xi, steps, handle=handle, subproblem='stage')
    print('iterations per step: mean %.2f max %d; %.1f ms, %d rounds'
          % (r.iterations.mean(), r.iterations.max(), r.kernel_ms, r.rounds))
    err = np.abs(r.X[0].T - xnl[:, :steps + 1]).max(axis=1)
    print('stored instance, max error over %d steps: %s' % (steps, err))
    assert (r.exitflag == 1).all(), r.exitflag
    assert err[0] <= 1e-7 and err[1] <= 1e-7 and err[2] <= 1e-5 and err[3] <= 1e-3, err
    for b in range(8):
        for t in range(steps):
            assert np.abs(r.X[b, t + 1] - mg_rk4(p['delta'], r.X[b, t], r.U[b, t])).max() <= 1e-14, (b, t)


# ---- 5. arguments ---------------------------------------------------------------------------
def test_arguments(probs, handle, mg, term_set):
    import bqp
    from bqp import _lib
    p, g = probs(10)
    lib = _lib.load()
    x0 = np.ascontiguousarray(p['x_eq'][None, :] + DEVS[:1])
    o = _lib.options(max_iter=100, polish=0)

    def solve(dims, dd):
        z = np.zeros((1, 11)); lam = np.zeros((1, g.m)); fl = np.zeros(1, np.int32); it = np.zeros(1, np.int32)
        rc = lib.bqp_nmpc_solve_batched(handle.value, C.byref(dims), 1, C.byref(dd), C.byref(o), _lib.ptr(z),
                                        _lib.ptr(lam), None, _lib.iptr(fl), _lib.iptr(it))
        return rc, z, lam, fl, it
    dd = g._data(x0)
    assert solve(_lib.NmpcDims(10, g.mx, g.mu, g.mp, 1), dd)[0] == _lib.BQP_OK
    assert solve(_lib.NmpcDims(10, g.mx, g.mu, g.mp, 2), dd)[0] == _lib.BQP_E_ARG
    assert solve(_lib.NmpcDims(10, g.mx, g.mu, g.mp, -1), dd)[0] == _lib.BQP_E_ARG
    # a terminal set outside the structured kernel's compiled row counts
    assert solve(_lib.NmpcDims(10, g.mx, g.mu, 5000, 1), dd)[0] == _lib.BQP_E_UNSUPPORTED
    # a zero-initialised dims struct (four-argument construction) runs the dense route
    a = solve(_lib.NmpcDims(10, g.mx, g.mu, g.mp), dd)
    b = solve(_lib.NmpcDims(10, g.mx, g.mu, g.mp, 0), dd)
    assert a[0] == b[0] == _lib.BQP_OK and a[3][0] == 1
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v)
    # a two-entry F_x row: refused on the stage route, solved on the dense one
    Fx = np.array(mg['F_x'], float)
    Fx[1, 0] = 0.05
    g2 = bqp.NMPC(mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'], Fx, mg['h_x'],
                  mg['F_u'], mg['h_u'], term_set[0], term_set[1], mg['x_wp'], mg['u_wp'], N=10)
    with pytest.raises(bqp.BqpError, match='unsupported'):
        g2.solve(x0, handle=handle, subproblem='stage')
    with pytest.raises(bqp.BqpError, match='unsupported'):
        g2.stage_qp(x0, handle=handle)
    with pytest.raises(bqp.BqpError, match='unsupported'):
        bqp.closed_loop_nmpc(g2, x0, 2, handle=handle, subproblem='stage')
    assert g2.solve(x0, handle=handle).exitflag[0] == 1
    with pytest.raises(ValueError):
        g.solve(x0, handle=handle, subproblem='sparse')
