"""GPU checks of the nonlinear MPC's set-point (bqp_nmpc_data.x_ref) on the three routes - dense,
stage, multiple shooting - and of the closed loop with a set-point schedule and a disturbed plant
(bqp_closed_loop_nmpc_track) against the numpy restatements with the set-point put on top
(tests/nmpc_track_ref.py), the library's own step-synchronous loop and the loop without a track."""
import ctypes as C
import os

import numpy as np
import pytest

import nmpc_dms_ref as DR
import nmpc_ref as R
import nmpc_track_ref as TR
from oracle.mg_model import mg_rk4
from test_gpu_nmpc import LIN_BAR, LIN_BAR_EQ
from test_gpu_nmpc_dms import C_BAR, _box
from test_gpu_nmpc_stage import DEVS, KEYS, STAGE_BAR, STAGE_BAR_EQ, _rel, handle, probs, xnl   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROUTES = {'dense': dict(subproblem='dense'), 'stage': dict(subproblem='stage'),
          'multiple': dict(subproblem='stage', shooting='multiple')}
STEPS = 12


@pytest.fixture(autouse=True)
def exact_fallback(monkeypatch):
    """the restatements' dense sub-problem solver hands a degenerate vertex to their exact one"""
    monkeypatch.setattr(R.dense_qp, 'solve', DR.qp_solve)


def grid_rhos(p):
    lam = p['LAMBDA']
    return np.array([0.05 * lam, [0.05, 0.0, 0.0, 0.0], [-0.2, 0.1, 0.02, 0.0], 2.0 * lam])


def grid_starts(p, xnl):
    return np.array([p['x_eq'] + np.array([-0.05, -0.05, 0.0, 0.0]), xnl[:, 0], xnl[:, 40]])


# ---- 1. linearisation -----------------------------------------------------------------------
@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 127])
def test_linearisation_with_a_set_point(probs, handle, N):
    """the six states at z = 0 and at a seeded z, every instance with a set-point of its own (the
    grid's four, then seeded ones).  The T rows are the last residual rows; with lanes over the
    stages, stage N is the last lane of pass 0 at N = 63, the first of pass 1 at N = 64 and the last
    of pass 1 at N = 127.  cost, f, w and the stage cost against the restatement at the bars of
    tests/test_gpu_nmpc.py and tests/test_gpu_nmpc_stage.py; everything the set-point does not enter
    bit for bit the call without it."""
    p, g = probs(N)
    rng = np.random.default_rng(500 + N)
    X0 = np.concatenate([p['x_eq'] + DEVS, p['x_eq'] + DEVS])
    Z = np.concatenate([np.zeros((6, N + 1)),
                        np.concatenate([rng.uniform(-0.3, 0.3, (6, N)), rng.uniform(-0.1, 0.1, (6, 1))], 1)])
    XR = p['x_eq'] + np.concatenate([grid_rhos(p), rng.uniform(-0.1, 0.1, (8, 4))])
    L, L0 = g.linearize(X0, Z, handle=handle, x_ref=XR), g.linearize(X0, Z, handle=handle)
    S, S0 = g.stage_qp(X0, Z, handle=handle, x_ref=XR), g.stage_qp(X0, Z, handle=handle)
    Xd = np.stack([DR.consistent(p, X0[i], Z[i]) for i in range(12)]) + rng.uniform(-1e-3, 1e-3, (12, N + 1, 4))
    M, M0 = g.dms_qp(X0, Xd, Z, handle=handle, x_ref=XR), g.dms_qp(X0, Xd, Z, handle=handle)
    sc, sc0 = g.stage_cost(X0, Z, handle=handle, x_ref=XR), g.stage_cost(X0, Z, handle=handle)
    # what the set-point does not enter
    for k in ('X', 'c', 'C', 'H'):
        assert np.array_equal(L[k], L0[k]), k
    assert np.array_equal(L.f[:, :N], L0.f[:, :N])
    for r, r0, keys in ((S, S0, ('A', 'B', 'xlb', 'xub', 'ulb', 'uub', 'hp', 'W', 'Fp')),
                        (M, M0, ('A', 'B', 'c', 'xlb', 'xub', 'ulb', 'uub', 'hp', 'W', 'Fp'))):
        for k in keys:
            assert np.array_equal(r[k], r0[k]), k
        wa, wb = r.w.reshape(12, -1), r0.w.reshape(12, -1)
        assert np.array_equal(wa[:, :-1], wb[:, :-1])
        assert (wa[:, -1] != wb[:, -1]).all()
    assert np.array_equal(sc.penalty, sc0.penalty)
    assert (L.cost != L0.cost).all() and (L.f[:, N] != L0.f[:, N]).all()
    # a set-point shared by the batch is the per-instance array with equal rows
    Ls = g.linearize(X0, Z, handle=handle, x_ref=XR[1])
    Lp = g.linearize(X0, Z, handle=handle, x_ref=np.tile(XR[1], (12, 1)))
    assert np.array_equal(Ls.cost, Lp.cost) and np.array_equal(Ls.f, Lp.f)
    worst, worst_eq = {}, {}

    def note(key, bars_eq, i, err):
        w = worst_eq if (i == 2 and key.split()[-1] in bars_eq) else worst     # case 2: x_eq, z = 0
        w[key] = max(w.get(key, 0.0), err)

    for i in range(12):
        ref = TR.linearize(p, XR[i], X0[i], Z[i])
        note('cost', LIN_BAR_EQ, i, abs(L.cost[i] - ref['cost']) / abs(ref['cost']))
        note('f', LIN_BAR_EQ, i, _rel(L.f[i], ref['f']))
        note('stage cost', LIN_BAR_EQ, i, abs(sc.cost[i] - ref['cost']) / abs(ref['cost']))
        note('stage w', STAGE_BAR_EQ, i, _rel(S.w[i], TR.stage_problem(p, XR[i], X0[i], Z[i])['w']))
        dp = TR.dms_problem(p, XR[i], X0[i], Xd[i], Z[i])
        note('dms w', STAGE_BAR_EQ, i, _rel(M.w[i], dp['w']))
        assert np.abs(M.c[i] - dp['c']).max() <= C_BAR
    print('N %d with set-points, relative to max-abs: %s; at x_eq, z = 0: %s' % (N, worst, worst_eq))
    bars = {'cost': LIN_BAR['cost'], 'f': LIN_BAR['f'], 'stage cost': LIN_BAR['cost'],
            'stage w': STAGE_BAR['w'], 'dms w': STAGE_BAR['w']}
    bars_eq = {'cost': LIN_BAR_EQ['cost'], 'f': LIN_BAR_EQ['f'], 'stage cost': LIN_BAR_EQ['cost'],
               'stage w': STAGE_BAR_EQ['w'], 'dms w': STAGE_BAR_EQ['w']}
    for key, v in worst.items():
        assert v <= bars[key], (key, v)
    for key, v in worst_eq.items():
        assert v <= bars_eq[key], (key, v)


# ---- 2. solves ------------------------------------------------------------------------------
def _kkt_ok(k):
    """the constants of _kkt_ok in tests/test_gpu_nmpc_stage.py (full space: and the defects)"""
    assert k['stat'] <= 1e-6 * (1.0 + k['grad']), k
    assert k['cmax'] <= 1e-9 and k.get('dmax', 0.0) <= 1e-9, k
    assert k['lam_min'] >= 0.0, k


@pytest.fixture(scope='module')
def restated(probs, xnl):
    """the restatement's solutions of the grid (3 starts x 4 set-points), once per horizon and form"""
    made = {}

    def get(N, multiple):
        if (N, multiple) not in made:
            p, _ = probs(N)
            out = []
            R.dense_qp.solve, keep = DR.qp_solve, R.dense_qp.solve
            try:
                for x0 in grid_starts(p, xnl):
                    for rho in grid_rhos(p):
                        xr = p['x_eq'] + rho
                        if multiple:
                            _, z, _, _, info = TR.dms_sqp(p, xr, x0)
                        else:
                            z, _, info = TR.sqp(p, xr, x0)
                        out.append((z, info))
            finally:
                R.dense_qp.solve = keep
            made[(N, multiple)] = out
        return made[(N, multiple)]
    return get


@pytest.mark.parametrize('route,N', [('dense', 3), ('dense', 10), ('stage', 3), ('stage', 10),
                                     ('multiple', 3), ('multiple', 10), ('multiple', 64), ('multiple', 65)])
def test_solves_with_a_set_point(probs, handle, xnl, restated, route, N):
    """the grid in one batch of 12, every instance with its own set-point: flags 1 and the
    restatement's, u_0 and theta within 1e-6 of it, the KKT check at the GPU's multipliers by the
    restatement with the set-point; the target outside the terminal set ends 1 with theta at the
    set's limit.

    Measured on the MI355X, largest |u_0 - restated|: dense 1.9e-10 (N = 3) and 1.9e-11 (N = 10), stage
    1.0e-8, multiple shooting 1.0e-9.  The dense route at N = 10 on the target outside the terminal set
    is the case the dense sub-problems' handling under a set-point exists for (DESIGN.md section 2c:
    their interior point stalls 5.0e-6 from the sub-problem's optimum there and is polished): 1.8e-13."""
    p, g = probs(N)
    X0 = np.repeat(grid_starts(p, xnl), 4, axis=0)
    XR = p['x_eq'] + np.tile(grid_rhos(p), (3, 1))
    r = g.solve(X0, handle=handle, x_ref=XR, **ROUTES[route])
    ref = restated(N, route == 'multiple')
    print('%s N %d flags %s iterations %s; restatement %s' % (route, N, r.exitflag.tolist(), r.iterations.tolist(),
                                                              [i['iterations'] for _, i in ref]))
    assert (r.exitflag == 1).all(), r.exitflag
    for i in range(12):
        z, info = ref[i]
        assert info['exitflag'] == r.exitflag[i], (i, info)
        du, dth = abs(r.z[i, 0] - z[0]), abs(r.z[i, N] - z[N])
        print('  start %d set-point %d: theta %.5f |u0 - ref| %.2e |theta - ref| %.2e' % (i // 4, i % 4, r.z[i, N], du, dth))
        assert du <= 1e-6 and dth <= 1e-6, (i, du, dth)
        if route == 'multiple':
            _kkt_ok(TR.dms_kkt(p, XR[i], X0[i], r.X[i], r.z[i], r.lam[i], r.pi[i]))
        else:
            _kkt_ok(TR.kkt(p, XR[i], X0[i], r.z[i], r.lam[i]))
    # the unreachable target from the first start: the restatement's theta is the set's limit
    if N <= 10:
        assert abs(ref[3][0][N] - 0.98148) <= 5e-6, ref[3][0][N]


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_reference_sweep_and_working_point(probs, handle, xnl, route):
    """four set-points for one measured state in a single batch: each instance bit for bit what it
    is when solved alone.  x_ref = x_eq: the flags and iteration counts of the call without a
    set-point; the largest difference in z is printed (the set-point instantiations differ from the
    others by e = fma(w, theta, -Lt rho) for e = w theta alone, which is the same value at rho = 0)"""
    p, g = probs(10)
    x0 = grid_starts(p, xnl)[1]
    XR = p['x_eq'] + grid_rhos(p)
    kw = dict(handle=handle, **ROUTES[route])
    keys = ('z', 'lam', 'cost', 'exitflag', 'iterations') + (('X', 'pi') if route == 'multiple' else ())
    r4 = g.solve(np.tile(x0, (4, 1)), x_ref=XR, **kw)
    assert (r4.exitflag == 1).all(), r4.exitflag
    assert len({tuple(z) for z in r4.z}) == 4
    for i in range(4):
        r1 = g.solve(x0[None], x_ref=XR[i], **kw)
        for k in keys:
            assert np.array_equal(r1[k][0], r4[k][i]), (i, k)
    X6 = p['x_eq'] + DEVS
    ra, rb = g.solve(X6, x_ref=p['x_eq'], **kw), g.solve(X6, **kw)
    dz = np.abs(ra.z - rb.z).max()
    print('%s: x_ref = x_eq against no set-point: flags %s iterations %s, max |z difference| %.3e'
          % (route, ra.exitflag.tolist(), ra.iterations.tolist(), dz))
    assert np.array_equal(ra.exitflag, rb.exitflag) and np.array_equal(ra.iterations, rb.iterations)
    assert dz == 0.0, dz


# ---- 3. loops -------------------------------------------------------------------------------
def _loop(g, xi, steps, handle, sync, **kw):
    import bqp
    assert 'BQP_NMPC_SYNC' not in os.environ
    if not sync:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, **kw)
    os.environ['BQP_NMPC_SYNC'] = '1'
    try:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, **kw)
    finally:
        del os.environ['BQP_NMPC_SYNC']


def _hold(p, vals, steps=STEPS):
    """LAMBDA-multiples, each held steps / len(vals) steps, as absolute set-points"""
    return p['x_eq'] + np.repeat(np.asarray(vals, float), steps // len(vals))[:, None] * p['LAMBDA']


def _schedules(p, xnl, shared):
    """(x_init (6, 4), refs, dist): the schedules of tests/test_nmpc_track_host.py's module doc and
    the issue's table, each set-point held 4 steps.  shared: LAMBDA {0.02, -0.02, 0} and a seeded
    disturbance within +-[2e-3, 2e-3, 1e-3, 0] for six starts; else one (start, schedule) pair per
    instance: LAMBDA {0.02, -0.02, 0} and LAMBDA {0.05, -0.05, 0.3} from x_eq and the stored run's
    first state, the off-line targets [0.05, 0, 0, 0] then [0, -0.04, 0.01, 0] from x_eq, and the
    first schedule with the disturbance from x_eq (the other five undisturbed)"""
    xe = p['x_eq']
    A, B = _hold(p, [0.02, -0.02, 0.0]), _hold(p, [0.05, -0.05, 0.3])
    Cc = xe + np.vstack([np.tile([0.05, 0.0, 0.0, 0.0], (4, 1)), np.tile([0.0, -0.04, 0.01, 0.0], (8, 1))])
    D = np.random.default_rng(7).uniform(-1.0, 1.0, (STEPS, 4)) * np.array([2e-3, 2e-3, 1e-3, 0.0])
    if shared:
        xi = np.array([xe, xnl[:, 0], xe + [-0.05, -0.05, 0.0, 0.0], xnl[:, 20], xe + DEVS[5],
                       xe + [-0.02, -0.02, 0.0, 0.0]])
        return xi, A, D
    xi = np.array([xe, xnl[:, 0], xe, xnl[:, 0], xe, xe])
    dist = np.zeros((6, STEPS, 4))
    dist[5] = D
    return xi, np.stack([A, A, B, B, Cc, A]), dist


def _check_loop(p, r, rs, xi, refs, dist, route, steps):
    """what every track loop must satisfy: both modes bit for bit, the rounds identity, the plant
    transitions with the disturbance, u_0 and theta against the restatement solved cold at the GPU's
    own states with the step's set-point"""
    b = xi.shape[0]
    for k in KEYS + ('theta',):
        assert np.array_equal(r[k], rs[k]), k
    rounds = int((r.iterations + (r.exitflag != 0)).sum(axis=1).max())
    assert r.rounds == rounds, (r.rounds, rounds)
    assert (r.exitflag == 1).all(), r.exitflag
    assert np.array_equal(r.X[:, 0], xi)
    worst = [0.0, 0.0, 0.0]
    for i in range(b):
        rf = refs if refs.ndim == 2 else refs[i]
        ds = dist if dist.ndim == 2 else dist[i]
        for t in range(steps):
            e = np.abs(r.X[i, t + 1] - (mg_rk4(p['delta'], r.X[i, t], r.U[i, t]) + ds[t])).max()
            assert e <= 1e-14, (i, t, e)
            if route == 'multiple':
                _, z, _, _, info = TR.dms_sqp(p, rf[t], r.X[i, t])
            else:
                z, _, info = TR.sqp(p, rf[t], r.X[i, t])
            assert info['exitflag'] == 1, (i, t, info)
            du, dth = abs(r.U[i, t] - (z[0] + p['u_eq'])), abs(r.theta[i, t] - z[p['N']])
            worst = [max(worst[0], e), max(worst[1], du), max(worst[2], dth)]
            assert du <= 1e-6 and dth <= 1e-6, (i, t, du, dth)
    print('  plant %.2e, |u0 - restated| %.2e, |theta - restated| %.2e' % tuple(worst))


@pytest.mark.parametrize('shared', [True, False])
@pytest.mark.parametrize('route', sorted(ROUTES))
def test_loop_follows_a_schedule(probs, handle, xnl, route, shared):
    """N = 10, batch 6, 12 steps.  Launches per round: those of the loop without a track on the same
    route (the advance launch does the track's work)"""
    p, g = probs(10)
    xi, refs, dist = _schedules(p, xnl, shared)
    kw = dict(refs=refs, dist=dist, **ROUTES[route])
    ra = _loop(g, xi, STEPS, handle, False, **kw)
    rs = _loop(g, xi, STEPS, handle, True, **kw)
    print('%s %s: iterations\n%s\nrounds %d (step-synchronous %d), launches %d'
          % (route, 'shared' if shared else 'per instance', ra.iterations, ra.rounds, rs.rounds, ra.launches))
    _check_loop(p, ra, rs, xi, refs, dist, route, STEPS)
    # per round what the loop without a track launches on this route: its launches are
    # fixed + per round * rounds (fixed: the table launch, multiple shooting's first rollout)
    r0 = _loop(g, xi, STEPS, handle, False, **ROUTES[route])
    fixed = {'dense': 0, 'stage': 1, 'multiple': 2}[route]
    per = (r0.launches - fixed) // r0.rounds
    assert r0.launches == fixed + per * r0.rounds, (r0.launches, r0.rounds)
    assert ra.launches == fixed + per * ra.rounds, (ra.launches, per, ra.rounds)
    # the schedule moves the loop
    assert not np.array_equal(ra.U, r0.U)


def test_multiple_shooting_loop_past_one_pass(probs, handle, xnl):
    """N = 65 (stage N is a second-pass lane), batch 3, 4 steps, per-instance schedules"""
    p, g = probs(65)
    xe = p['x_eq']
    xi = np.array([xe, xnl[:, 0], xe + [-0.05, -0.05, 0.0, 0.0]])
    A = _hold(p, [0.02, -0.02], steps=4)
    refs = np.stack([A, A[::-1].copy(), A])
    D = np.random.default_rng(7).uniform(-1.0, 1.0, (STEPS, 4)) * np.array([2e-3, 2e-3, 1e-3, 0.0])
    dist = np.stack([D[:4], np.zeros((4, 4)), D[4:8]])
    kw = dict(refs=refs, dist=dist, **ROUTES['multiple'])
    ra, rs = _loop(g, xi, 4, handle, False, **kw), _loop(g, xi, 4, handle, True, **kw)
    print('iterations\n%s' % ra.iterations)
    _check_loop(p, ra, rs, xi, refs, dist, 'multiple', 4)


def _raw_track(handle, g, route, xi, steps, tr, x_ref=None):
    """the C entry itself: bqp_closed_loop_nmpc_track with tr a bqp_nmpc_track or None (NULL), or
    bqp_closed_loop_nmpc where tr is False"""
    from bqp import _lib
    from bqp.loop import ClosedLoop
    lib = _lib.load()
    b = xi.shape[0]
    X = np.zeros((b, steps + 1, 4)); U = np.zeros((b, steps))
    fl = np.zeros((b, steps), np.int32); it = np.zeros((b, steps), np.int32)
    kw = ROUTES[route]
    dims = g._dims(kw['subproblem'], kw.get('shooting', 'single'))
    dd = g._data(x_ref=x_ref)
    cl = ClosedLoop(1, steps, g.delta, _lib.ptr(g.x_eq), _lib.ptr(g.u_eq))
    o = _lib.options(max_iter=100, polish=0)
    head = (handle.value, C.byref(dims), b, C.byref(dd), C.byref(o), C.byref(cl), _lib.ptr(xi))
    tail = (_lib.ptr(X), _lib.ptr(U), _lib.iptr(fl), _lib.iptr(it))
    if tr is False:
        rc = lib.bqp_closed_loop_nmpc(*head, *tail)
    else:
        rc = lib.bqp_closed_loop_nmpc_track(*head, C.byref(tr) if tr is not None else None, *tail)
    return rc, dict(X=X, U=U, exitflag=fl, iterations=it, rounds=handle.loop_rounds() if rc == 0 else None,
                    launches=handle.kernel_ms()[1] if rc == 0 else None)


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_null_track_and_short_loops(probs, handle, xnl, route):
    """tr = NULL and a track with nothing in it are bqp_closed_loop_nmpc bit for bit, rounds and
    launches included; a schedule of x_eq at every step gives that loop's moves with the same rounds;
    a constant data->x_ref is the schedule that repeats it; steps = 1, where the one step reads no
    next set-point, and steps = 0"""
    import bqp
    from bqp import _lib
    p, g = probs(10)
    xi = np.ascontiguousarray(np.array([p['x_eq'], xnl[:, 0], xnl[:, 20]]))
    rc0, plain = _raw_track(handle, g, route, xi, 5, False)
    rc1, null = _raw_track(handle, g, route, xi, 5, None)
    rc2, empty = _raw_track(handle, g, route, xi, 5, _lib.NmpcTrack(None, 0, None, 0, None))
    assert rc0 == rc1 == rc2 == _lib.BQP_OK
    for k in plain:
        assert np.array_equal(plain[k], null[k]) and np.array_equal(plain[k], empty[k]), k
    kw = dict(handle=handle, **ROUTES[route])
    req = bqp.closed_loop_nmpc(g, xi, 5, refs=np.tile(p['x_eq'], (5, 1)), **kw)
    for k in KEYS:
        assert np.array_equal(req[k], plain[k]), k
    assert req.rounds == plain['rounds'] and req.launches == plain['launches']
    xr = p['x_eq'] + 0.05 * p['LAMBDA']
    ra = bqp.closed_loop_nmpc(g, xi, 5, x_ref=xr, **kw)
    rb = bqp.closed_loop_nmpc(g, xi, 5, refs=np.tile(xr, (5, 1)), **kw)
    rc = bqp.closed_loop_nmpc(g, xi, 5, x_ref=np.tile(xr, (3, 1)), dist=np.zeros((5, 4)), **kw)
    for k in KEYS:
        assert np.array_equal(ra[k], rb[k]) and np.array_equal(ra[k], rc[k]), k
    assert np.array_equal(rb.theta, rc.theta) and not np.array_equal(ra.U, plain['U'])
    # one step: the solve with the step's set-point
    refs1 = (p['x_eq'] + grid_rhos(p)[:3])[:, None, :]
    d1 = np.zeros((3, 1, 4)); d1[1, 0] = [1e-3, -1e-3, 5e-4, 0.0]
    for sync in (False, True):
        r1 = _loop(g, xi, 1, handle, sync, refs=refs1, dist=d1, **ROUTES[route])
        s1 = g.solve(xi, x_ref=refs1[:, 0], **kw)
        if route == 'multiple':
            # the loop's first states are nmpc_dms_start_kernel's rollout, the solve's the linearisation's
            assert np.abs(r1.U[:, 0] - s1.u0[:, 0]).max() <= 1e-9 and np.abs(r1.theta[:, 0] - s1.theta[:, 0]).max() <= 1e-9
        else:
            assert np.array_equal(r1.U[:, 0], s1.u0[:, 0]) and np.array_equal(r1.theta[:, 0], s1.theta[:, 0])
        assert np.array_equal(r1.exitflag[:, 0], s1.exitflag) and np.array_equal(r1.iterations[:, 0], s1.iterations)
        for i in range(3):
            assert np.abs(r1.X[i, 1] - (mg_rk4(p['delta'], xi[i], r1.U[i, 0]) + d1[i, 0])).max() <= 1e-14
    r0 = bqp.closed_loop_nmpc(g, xi, 0, refs=np.zeros((0, 4)), **kw)
    assert np.array_equal(r0.X[:, 0], xi) and r0.theta.shape == (3, 0)


# ---- 4. disturbance with soft rows ------------------------------------------------------------
SOFT_W = (100.0, 1000.0)


def _soft_case(p, xnl):
    """N = 10, 12 steps from the stored run's state 20 and five states around it (+-0.02 in x1, x2);
    set-points 0.05 LAMBDA, [-0.2, 0.1, 0.02, 0], 0, each held 4 steps; the disturbance of step 0 pushes
    x2 below its bound"""
    lam = p['LAMBDA']
    refs = p['x_eq'] + np.vstack([np.tile(0.05 * lam, (4, 1)), np.tile([-0.2, 0.1, 0.02, 0.0], (4, 1)),
                                  np.zeros((4, 4))])
    dist = np.zeros((STEPS, 4))
    dist[0] = [0.0, -0.03, 0.0, 0.0]
    dist[5] = [0.002, -0.01, 0.001, 0.0]
    pert = np.array([[0.0, 0.0], [0.02, 0.0], [-0.02, 0.0], [0.0, 0.02], [0.0, -0.02], [0.02, -0.02]])
    return xnl[:, 20] + np.hstack([pert, np.zeros((6, 2))]), refs, dist


@pytest.fixture(scope='module')
def soft_loops(probs, handle, xnl):
    """the stage route's loop on the soft case: hard rows, and the weights (100, 1000) in both modes"""
    p, g = probs(10)
    xi, refs, dist = _soft_case(p, xnl)
    kw = dict(refs=refs, dist=dist, subproblem='stage')
    hard = _loop(g, xi, STEPS, handle, False, **kw)
    kw.update(xs_lin=SOFT_W[0], xs_quad=SOFT_W[1])
    return hard, _loop(g, xi, STEPS, handle, False, **kw), _loop(g, xi, STEPS, handle, True, **kw)


def test_disturbance_needs_the_soft_rows(probs, xnl, soft_loops):
    """hard rows: the solve after the disturbance ends -2 (the restatement: at step 1 from the state
    itself and from x1 +- 0.02; from x2 - 0.02 already at step 0).  With the weights every solve ends
    1, in both loop modes bit for bit, from measured states outside the box"""
    p, _ = probs(10)
    hard, soft, softs = soft_loops
    lo, _ = _box(p)
    print('hard rows: flags\n%s\nx2 after step 0: %s (bound %.4f)\nsoft rows: iterations\n%s'
          % (hard.exitflag, hard.X[:, 1, 1], lo[1], soft.iterations))
    assert hard.exitflag[0, 0] == 1 and hard.exitflag[0, 1] == -2, hard.exitflag[0]
    assert (hard.exitflag[[1, 2], 0] == 1).all() and (hard.exitflag[[1, 2], 1] == -2).all()
    assert (hard.exitflag[[4, 5], 0] == -2).all()
    for k in KEYS + ('theta',):
        assert np.array_equal(soft[k], softs[k]), k
    assert (soft.exitflag == 1).all(), soft.exitflag
    assert soft.X[0, 1, 1] < lo[1]          # the measured state of step 1 is outside the box


@pytest.mark.parametrize('i', range(6))
def test_soft_loop_against_restatement(probs, xnl, soft_loops, i):
    """instance i of the soft loop: every plant transition with the disturbance, u_0 within 1e-6 of
    the soft restatement solved cold at the GPU's own state with the step's set-point"""
    p, _ = probs(10)
    _, refs, dist = _soft_case(p, xnl)
    soft = soft_loops[1]
    worst = 0.0
    for t in range(STEPS):
        assert np.abs(soft.X[i, t + 1] - (mg_rk4(p['delta'], soft.X[i, t], soft.U[i, t]) + dist[t])).max() <= 1e-14
        z, _, info = TR.soft_sqp(p, refs[t], soft.X[i, t], SOFT_W[0], SOFT_W[1])
        assert info['exitflag'] == 1, (t, info)
        worst = max(worst, abs(soft.U[i, t] - (z[0] + p['u_eq'])))
    print('instance %d: |u0 - restated| %.2e' % (i, worst))
    assert worst <= 1e-6, worst


# ---- 5. arguments ---------------------------------------------------------------------------
def test_arguments(probs, handle, xnl):
    import bqp
    from bqp import _lib
    from bqp.loop import ClosedLoop
    p, g = probs(10)
    lib = _lib.load()
    x0 = np.ascontiguousarray(p['x_eq'][None, :] + DEVS[4:5])
    for bad in (np.nan, np.inf):
        xr = p['x_eq'].copy(); xr[2] = bad
        for call in (lambda: g.linearize(x0, handle=handle, x_ref=xr),
                     lambda: g.stage_qp(x0, handle=handle, x_ref=xr),
                     lambda: g.dms_qp(x0, handle=handle, x_ref=xr),
                     lambda: g.stage_cost(x0, handle=handle, x_ref=xr),
                     lambda: g.solve(x0, handle=handle, x_ref=xr),
                     lambda: g.solve(x0, handle=handle, x_ref=xr, subproblem='stage'),
                     lambda: g.solve(x0, handle=handle, x_ref=xr, subproblem='stage', shooting='multiple'),
                     lambda: bqp.closed_loop_nmpc(g, x0, 2, handle=handle, x_ref=xr),
                     lambda: bqp.closed_loop_nmpc(g, x0, 2, handle=handle, refs=np.stack([p['x_eq'], xr])),
                     lambda: bqp.closed_loop_nmpc(g, x0, 2, handle=handle, dist=np.stack([np.zeros(4), xr]))):
            with pytest.raises(bqp.BqpError, match='invalid argument'):
                call()
    # the second instance's set-point is checked too
    with pytest.raises(bqp.BqpError, match='invalid argument'):
        g.solve(np.tile(x0, (2, 1)), handle=handle, x_ref=np.array([p['x_eq'], [np.nan, 0, 0, 0]]))
    with pytest.raises(ValueError):
        g.solve(x0, handle=handle, x_ref=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        bqp.closed_loop_nmpc(g, x0, 2, handle=handle, refs=np.zeros((3, 4)))
    # a plant other than RK4, and a stride that is neither 0 nor a whole schedule
    refs = np.tile(p['x_eq'], (2, 1))
    X = np.zeros((1, 3, 4)); U = np.zeros((1, 2))
    dims, dd = g._dims('stage'), g._data()
    o = _lib.options(max_iter=100, polish=0)
    for plant, sref, want in ((2, 0, _lib.BQP_E_ARG), (3, 0, _lib.BQP_E_ARG), (1, 4, _lib.BQP_E_ARG),
                              (1, -8, _lib.BQP_E_ARG), (1, 8, _lib.BQP_OK), (1, 0, _lib.BQP_OK)):
        cl = ClosedLoop(plant, 2, g.delta, _lib.ptr(g.x_eq), _lib.ptr(g.u_eq))
        tr = _lib.NmpcTrack(_lib.ptr(refs), sref, None, 0, None)
        rc = lib.bqp_closed_loop_nmpc_track(handle.value, C.byref(dims), 1, C.byref(dd), C.byref(o), C.byref(cl),
                                            _lib.ptr(x0), C.byref(tr), _lib.ptr(X), _lib.ptr(U), None, None)
        assert rc == want, (plant, sref, rc)
    # either half of the track alone
    a = bqp.closed_loop_nmpc(g, x0, 3, handle=handle, refs=_hold(p, [0.02], steps=3))
    b = bqp.closed_loop_nmpc(g, x0, 3, handle=handle, dist=np.full((3, 4), 1e-4))
    assert (a.exitflag == 1).all() and (b.exitflag == 1).all() and a.theta.shape == b.theta.shape == (1, 3)
    assert np.abs(b.X[0, 1] - (mg_rk4(p['delta'], b.X[0, 0], b.U[0, 0]) + 1e-4)).max() <= 1e-14
    # soft rows live on the stage route, with a track as without
    with pytest.raises(bqp.BqpError, match='unsupported'):
        bqp.closed_loop_nmpc(g, x0, 2, handle=handle, refs=refs, xs_quad=10.0)
