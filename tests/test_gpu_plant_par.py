"""GPU checks of the per-instance Moore-Greitzer plant coefficients (bqp_closed_loop.plant_par,
plant_params= in Python) in every closed loop.  The coefficients are seeded +-10 % draws around the
nominal plant (x2_c within +-0.05, tests/mg_param_ref.py draw_params); every batch of more than one
instance with per-instance coefficients holds an instance at exactly the nominal ones.  Each logged
transition X[b, t] -> X[b, t + 1] is compared with the numpy restatement of the parametrised plant
(mg_rk4_p / mg_ode23_p) at that instance's, and step's, row, the disturbance added where there is
one, at the project's bars for plant transitions: 1e-14 for RK4, 1e-13 for ode23.  A +-10 % draw
moves a step by 1e-5 and more (tests/test_mg_param_host.py), nine orders above.

ode23 takes discrete accept / reject decisions: before a comparison, every error estimate the
restatement computes for the logged inputs is required to keep |err / rtol - 1| >= 1e-6, so no
rounding difference can flip a decision."""
import ctypes as C
import os

import numpy as np
import pytest

import mg_param_ref as M
import nmpc_ref as R
from conftest import golden
from oracle.mg_model import mg_rk4
from test_gpu_nmpc import DEVS

pytestmark = pytest.mark.gpu

BAR = {'rk4': 1e-14, 'ode23': 1e-13}
DELTA = 0.01
KEYS = ('X', 'U', 'exitflag', 'iterations')
SOFT_W = (100.0, 1000.0)
NMPC_ROUTES = {'dense': dict(subproblem='dense'), 'stage': dict(subproblem='stage'),
               'soft': dict(subproblem='stage', xs_lin=SOFT_W[0], xs_quad=SOFT_W[1]),
               'multiple': dict(subproblem='stage', shooting='multiple')}


@pytest.fixture(scope='module', autouse=True)
def torch_first():
    """torch opens the GPU before libbqp does (tests/test_gpu_tracking_loop.py says why): the device=
    calls of test_device_path need it when this file runs alone"""
    import torch
    torch.cuda.is_available()


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


def _tlmpc(mg, ts, N):
    import bqp
    return bqp.TrackingLMPC(mg['A'], mg['B'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'],
                            mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'], ts[0], ts[1],
                            mg['x_wp'], mg['u_wp'], N=N)


@pytest.fixture(scope='module')
def tl1(mg, term_set):
    """the MG tracking problem at N = 1, the shortest horizon tests/test_gpu_ocp_short_horizons.py
    runs for it"""
    return _tlmpc(mg, term_set, 1)


@pytest.fixture(scope='module')
def tl20(mg, term_set):
    """the MG tracking problem of tests/test_gpu_tracking_loop.py's moving set-point"""
    return _tlmpc(mg, term_set, 20)


@pytest.fixture(scope='module')
def learned(mg):
    """(TrackingLBMPC N = 100, DMSLBMPC N = 50): the problems of tests/test_gpu_lbmpc_loop.py and the
    shortest of tests/test_gpu_lbmpc_dms.py"""
    import bqp
    g = golden('lbmpc_instance.npz')
    args = (mg['A'], mg['B'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'],
            mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'], g['F_w_N'], g['h_w_N'], g['F_x_d'], g['h_x_d'],
            mg['x_wp'], mg['u_wp'])
    return bqp.TrackingLBMPC(*args, N=100), bqp.DMSLBMPC(*args, N=50)


@pytest.fixture(scope='module')
def nmpcs(mg, term_set):
    import bqp
    made = {}

    def get(N):
        if N not in made:
            made[N] = (R.problem(mg, term_set[0], term_set[1], N),
                       bqp.NMPC(mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'],
                                mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'], term_set[0], term_set[1],
                                mg['x_wp'], mg['u_wp'], N=N))
        return made[N]
    return get


def _draw(seed, b, steps=None):
    """per-instance coefficients, (b, 4) or with steps a schedule (b, steps, 4); instance 0 at exactly
    the nominal ones (the whole schedule), the last instance - the one past a block edge - perturbed"""
    P = M.draw_params(np.random.default_rng(seed), (b,) if steps is None else (b, steps))
    P[0] = M.NOMINAL
    return P


def _check(tag, r, P, plant, dist=None):
    """every logged transition against the restatement at its row, at BAR[plant]; returns the worst"""
    X = np.asarray(r.X if not hasattr(r.X, 'cpu') else r.X.cpu().numpy())
    U = np.asarray(r.U if not hasattr(r.U, 'cpu') else r.U.cpu().numpy())
    b, steps = X.shape[0], X.shape[1] - 1
    assert np.isfinite(X).all() and np.isfinite(U).all()
    Pf = M.full_params(P, b, steps)
    if dist is not None:
        dist = np.broadcast_to(dist, (b, steps, 4))
    if plant == 'ode23':
        margin = M.ode23_margin(Pf, DELTA, X, U)
        print('%s: ode23 decisions at least %.2e from the threshold' % (tag, margin))
        assert margin >= 1e-6, margin
    e = M.transition_errors(Pf, plant, DELTA, X, U, dist)
    print('%s: %s transitions against the restatement, worst %.2e (bar %.0e)' % (tag, plant, e.max(), BAR[plant]))
    assert e.max() <= BAR[plant], (tag, e.max(), np.unravel_index(e.argmax(), e.shape))
    return e.max()


def _x0(b):
    return np.ascontiguousarray(golden('dms_DSS_tLMPC.npz')['x'][:b])


# ---- 1. block edges of the plant kernel ---------------------------------------------------------
@pytest.mark.parametrize('plant', ['rk4', 'ode23'])
@pytest.mark.parametrize('b', [1, 129, 257])
def test_block_edges(tl1, handle, b, plant):
    """bqp_closed_loop_ocp, N = 1, 2 steps; batch one past the 128- and 256-thread blocks; stride 0
    (one perturbed row for the batch) and stride 4 (a row per instance)"""
    import bqp
    X0 = _x0(b)
    P = _draw(100 + b, b)
    for tag, par in (('stride 0', P[-1] if b > 1 else M.draw_params(np.random.default_rng(7))), ('stride 4', P)):
        r = bqp.closed_loop(tl1, X0, 2, delta=DELTA, plant=plant, handle=handle, plant_params=par)
        assert np.array_equal(r.X[:, 0], X0)
        _check('ocp N=1 batch %d %s' % (b, tag), r, par, plant)


# ---- 2. every loop family -----------------------------------------------------------------------
FORMS = ['constant', 'schedule']


def _form(seed, form, b=5, steps=3):
    return _draw(seed, b, steps if form == 'schedule' else None)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('plant', ['rk4', 'ode23'])
def test_learning_loop(mg, learned, handle, plant, form):
    """closed_loop with learning= (bqp_closed_loop_lbmpc): the transitions, and the window's Y rows
    against (x+ - x_eq) - (A dx + B du) recomputed from the logged X, U at 1e-13, the bar of
    tests/test_gpu_lbmpc_loop.py - the window learns each instance's own plant"""
    import bqp
    tl = learned[0]
    X0 = golden('lbmpc_loop.npz')['xlo'][[0, 10, 20, 30, 40]]
    P = _form(21, form)
    r = bqp.closed_loop(tl, X0, 3, delta=DELTA, plant=plant, handle=handle, learning=dict(q=8, mask=1),
                        plant_params=P)
    _check('lbmpc %s' % form, r, P, plant)
    A, B = np.asarray(mg['A'], float), np.asarray(mg['B'], float).ravel()
    worst = 0.0
    for b in range(5):
        for t in range(3):
            dx, du = r.X[b, t] - tl.x_eq, r.U[b, t, 0] - tl.u_eq[0]
            pt = r.window[b, t + 1]            # iteration t + 1 in ring point (t + 1) mod q
            Y = (r.X[b, t + 1] - tl.x_eq) - (A @ dx + B * du)
            assert np.array_equal(pt[:3], [dx[0], dx[1], du]) and pt[7] == 1.0
            worst = max(worst, np.abs(pt[3:7] - Y).max())
    print('window Y rows against the logged X, U: %.2e' % worst)
    assert worst <= 1e-13, worst
    # the windows of the perturbed instances differ from the nominal plant's
    r0 = bqp.closed_loop(tl, X0, 3, delta=DELTA, plant=plant, handle=handle, learning=dict(q=8, mask=1))
    assert np.abs(r.window[1:, 1:4, 3:7] - r0.window[1:, 1:4, 3:7]).max() > 1e-6


@pytest.mark.parametrize('form', FORMS)
def test_sqp_loop(learned, handle, form):
    """closed_loop_sqp (N = 50, q = 10): the asynchronous loop (sqp_loop_advance_kernel) and, selected
    by BQP_LB_SYNC, the step-synchronous one (mg_plant_kernel), both integrators"""
    import bqp
    mpc = learned[1]
    rng = np.random.default_rng(11)
    X0 = np.array([0.15, 1.2875, 1.1547, 0.0]) + rng.uniform(-1, 1, (5, 4)) * np.array([0.02, 0.02, 0.0, 0.0])
    P = _form(22, form)
    assert 'BQP_LB_SYNC' not in os.environ
    for plant in ('rk4', 'ode23'):
        kw = dict(learning=dict(q=10, mask=1), plant=plant, handle=handle, plant_params=P)
        ra = bqp.closed_loop_sqp(mpc, X0, 3, **kw)
        _check('sqp asynchronous %s' % form, ra, P, plant)
        os.environ['BQP_LB_SYNC'] = '1'
        try:
            rs = bqp.closed_loop_sqp(mpc, X0, 3, **kw)
        finally:
            del os.environ['BQP_LB_SYNC']
        _check('sqp step-synchronous %s' % form, rs, P, plant)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('plant', ['rk4', 'ode23'])
def test_track_loop(mg, tl20, handle, plant, form):
    """closed_loop with refs= on an MG plant (bqp_closed_loop_track, track_advance_kernel)"""
    import bqp
    X0 = golden('dms_DSS_tLMPC.npz')['x'][[0, 100, 200, 300, 450]]
    refs = np.array([0.0, 0.02, -0.02])[:, None] * np.ravel(mg['LAMBDA'])[None, :]
    P = _form(23, form)
    r = bqp.closed_loop(tl20, X0, 3, delta=DELTA, plant=plant, handle=handle, refs=refs, plant_params=P)
    assert r.theta.shape == (5, 3, 1)
    _check('track %s' % form, r, P, plant)


def _nmpc_inputs(p, N):
    xi = p['x_eq'] + DEVS[:5]
    refs = p['x_eq'] + np.array([0.02, -0.02, 0.0])[:, None] * p['LAMBDA']
    dist = np.random.default_rng(7).uniform(-1.0, 1.0, (5, 3, 4)) * np.array([2e-3, 2e-3, 1e-3, 0.0])
    return np.ascontiguousarray(xi), refs, dist


def _nmpc_loop(g, xi, steps, handle, sync, **kw):
    import bqp
    assert 'BQP_NMPC_SYNC' not in os.environ
    if not sync:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, **kw)
    os.environ['BQP_NMPC_SYNC'] = '1'
    try:
        return bqp.closed_loop_nmpc(g, xi, steps, handle=handle, **kw)
    finally:
        del os.environ['BQP_NMPC_SYNC']


def _modes_equal(ra, rs, keys=KEYS):
    for k in keys:
        assert np.array_equal(ra[k], rs[k]), k
    rounds = int((ra.iterations + (ra.exitflag != 0)).sum(axis=1).max())
    assert ra.rounds == rounds, (ra.rounds, rounds)


# ---- 2 (nonlinear MPC) and 3 (both loop modes) --------------------------------------------------
@pytest.mark.parametrize('N', [3, 65])
@pytest.mark.parametrize('route', sorted(NMPC_ROUTES))
def test_nmpc_loops(nmpcs, handle, route, N):
    """closed_loop_nmpc on every route at N = 3 and N = 65 (stage N in the second lane pass), 3 steps,
    batch 5, with and without refs= / dist= (bqp_closed_loop_nmpc_track / bqp_closed_loop_nmpc),
    constant coefficients and a per-instance schedule.  With the schedule both loop modes run: the
    asynchronous loop, where instance b reads the row of its own step ts[b], equals the
    step-synchronous one (BQP_NMPC_SYNC, set in the process as tests/test_gpu_nmpc_async.py sets it)
    bit for bit in X, U, flags and iterations, and its round count obeys that file's identity."""
    p, g = nmpcs(N)
    xi, refs, dist = _nmpc_inputs(p, N)
    for track in (False, True):
        kw = dict(NMPC_ROUTES[route])
        if track:
            kw.update(refs=refs, dist=dist)
        for form in FORMS:
            P = _form(30 + N, form)
            tag = 'nmpc %s N=%d %s %s' % (route, N, 'track' if track else 'plain', form)
            ra = _nmpc_loop(g, xi, 3, handle, False, plant_params=P, **kw)
            _check(tag, ra, P, 'rk4', dist if track else None)
            if form == 'schedule':
                rs = _nmpc_loop(g, xi, 3, handle, True, plant_params=P, **kw)
                _modes_equal(ra, rs, KEYS + (('theta',) if track else ()))
                print('%s: iterations\n%s' % (tag, ra.iterations))


def test_nmpc_modes_at_different_steps(nmpcs, handle):
    """N = 10, 5 steps, the six DEVS states of tests/test_gpu_nmpc_async.py::test_failed_instance's
    batch: their solves take different numbers of iterations, so in the asynchronous loop the
    instances are at different steps in the same round, each reading its own row of the schedule"""
    p, g = nmpcs(10)
    xi = np.ascontiguousarray(p['x_eq'] + DEVS)
    P = _draw(41, 6, 5)
    ra = _nmpc_loop(g, xi, 5, handle, False, plant_params=P)
    rs = _nmpc_loop(g, xi, 5, handle, True, plant_params=P)
    _modes_equal(ra, rs)
    print('iterations\n%s' % ra.iterations)
    assert len({tuple(np.cumsum(row)) for row in ra.iterations}) > 1    # the instances do drift apart
    _check('nmpc N=10 schedule', ra, P, 'rk4')


# ---- 4. isolation and sharing -------------------------------------------------------------------
def _runner(kind, tl1, nmpcs, handle):
    """a loop of 3 steps as a function of (initial states, plant_params) -> dict of arrays"""
    import bqp
    if kind == 'nmpc':
        p, g = nmpcs(3)
        return (np.ascontiguousarray(p['x_eq'] + DEVS[:5]),
                lambda xi, P: bqp.closed_loop_nmpc(g, xi, 3, handle=handle, subproblem='stage', plant_params=P))
    return _x0(5), lambda xi, P: bqp.closed_loop(tl1, xi, 3, delta=DELTA, plant=kind, handle=handle, plant_params=P)


@pytest.mark.parametrize('kind', ['rk4', 'ode23', 'nmpc'])
def test_isolation_and_sharing(tl1, nmpcs, handle, kind):
    xi, run = _runner(kind, tl1, nmpcs, handle)
    keys = ('X', 'U', 'exitflag')
    P = _draw(51, 5)
    mixed = run(xi, P)
    # the nominal instance of a mixed batch against the same instance in an all-nominal batch
    allnom = run(xi, np.tile(M.NOMINAL, (5, 1)))
    for k in keys:
        assert np.array_equal(mixed[k][0], allnom[k][0]), k
    assert not np.array_equal(mixed.X[1:], allnom.X[1:])
    # stride 0 with one row against the row replicated per instance
    shared, repl = run(xi, P[3]), run(xi, np.tile(P[3], (5, 1)))
    for k in keys:
        assert np.array_equal(shared[k], repl[k]), k
    assert np.array_equal(shared.X[3], mixed.X[3])
    # a schedule of equal rows against the constant form, per instance and shared
    for const, sched in ((P, np.repeat(P[:, None], 3, axis=1)), (P[3], np.tile(P[3], (3, 1)))):
        rc, rs = run(xi, const), run(xi, sched)
        for k in keys:
            assert np.array_equal(rc[k], rs[k]), k


# ---- 5. against the unparametrised launch -------------------------------------------------------
def test_nominal_against_unparametrised(mg, tl1, tl20, learned, nmpcs, handle):
    """nominal coefficients against plant_par = NULL on the same inputs, one step: the first
    transition, before any solve can amplify a difference, at the bars"""
    import bqp
    nom = M.NOMINAL
    X5 = _x0(5)
    refs1 = 0.02 * np.ravel(mg['LAMBDA'])[None, :]
    Xl = golden('lbmpc_loop.npz')['xlo'][[0, 10, 20, 30, 40]]
    Xs = np.array([0.15, 1.2875, 1.1547, 0.0]) + np.array([[0.0], [0.01], [-0.01]]) * np.array([1.0, 1.0, 0.0, 0.0])
    p3, g3 = nmpcs(3)
    xn, refsn, distn = _nmpc_inputs(p3, 3)
    cases = []
    for plant in ('rk4', 'ode23'):
        cases += [('ocp ' + plant, plant, lambda P, pl=plant: bqp.closed_loop(
                      tl1, X5, 1, delta=DELTA, plant=pl, handle=handle, plant_params=P)),
                  ('track ' + plant, plant, lambda P, pl=plant: bqp.closed_loop(
                      tl20, X5, 1, delta=DELTA, plant=pl, handle=handle, refs=refs1, plant_params=P)),
                  ('lbmpc ' + plant, plant, lambda P, pl=plant: bqp.closed_loop(
                      learned[0], Xl, 1, delta=DELTA, plant=pl, handle=handle, learning=dict(q=8, mask=1),
                      plant_params=P)),
                  ('sqp ' + plant, plant, lambda P, pl=plant: bqp.closed_loop_sqp(
                      learned[1], Xs, 1, learning=dict(q=10, mask=1), plant=pl, handle=handle, plant_params=P))]
    cases += [('nmpc', 'rk4', lambda P: bqp.closed_loop_nmpc(g3, xn, 1, handle=handle, plant_params=P)),
              ('nmpc track', 'rk4', lambda P: bqp.closed_loop_nmpc(
                  g3, xn, 1, handle=handle, refs=refsn[:1], dist=distn[:, :1], plant_params=P))]
    for tag, plant, run in cases:
        a, b = run(nom), run(None)
        assert np.array_equal(a.U, b.U), tag            # the same solve
        d = np.abs(a.X[:, 1] - b.X[:, 1]).max()
        print('%s: nominal coefficients against the unparametrised launch, first transition: %.3e' % (tag, d))
        assert d <= BAR[plant], (tag, d)


# ---- 6. a fault mid-run -------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['rk4', 'nmpc'])
def test_fault_mid_run(tl1, nmpcs, handle, kind):
    """a schedule nominal for 2 steps, then wn^2 at 0.8 x nominal: steps 0-1 are the nominal plant's
    (oracle.mg_model.mg_rk4), steps 2-3 the faulted plant's"""
    import bqp
    fault = M.NOMINAL * np.array([1.0, 1.0, 0.8, 1.0])
    sched = np.stack([M.NOMINAL, M.NOMINAL, fault, fault])
    if kind == 'nmpc':
        p, g = nmpcs(3)
        xi = np.ascontiguousarray(p['x_eq'] + DEVS[:5])
        r = bqp.closed_loop_nmpc(g, xi, 4, handle=handle, plant_params=sched)
        U = r.U
    else:
        r = bqp.closed_loop(tl1, _x0(5), 4, delta=DELTA, plant='rk4', handle=handle, plant_params=sched)
        U = r.U[:, :, 0]
    for b in range(5):
        for t in range(4):
            nominal = mg_rk4(DELTA, r.X[b, t], U[b, t])
            faulted = M.mg_rk4_p(fault, DELTA, r.X[b, t], U[b, t])
            want, other = (nominal, faulted) if t < 2 else (faulted, nominal)
            assert np.abs(r.X[b, t + 1] - want).max() <= BAR['rk4'], (b, t)
    # the fault is visible: at the logged states the two restated plants are 1,000 bars apart and more
    apart = max(np.abs(mg_rk4(DELTA, r.X[b, t], U[b, t]) - M.mg_rk4_p(fault, DELTA, r.X[b, t], U[b, t])).max()
                for b in range(5) for t in (2, 3))
    print('fault: the restated plants differ by up to %.2e at the logged states' % apart)
    assert apart >= 1e3 * BAR['rk4']
    _check('fault %s' % kind, r, sched, 'rk4')


# ---- 7. errors ----------------------------------------------------------------------------------
def _raw_ocp(handle, tl, b, steps, plant, par, stride, sched, device=False):
    """bqp_closed_loop_ocp itself with the trailing members as given"""
    from bqp import _lib, loop
    from bqp.ocp import pack
    lib = _lib.load()
    x0 = _x0(b)
    xeq = np.ascontiguousarray(tl.x_eq, dtype=np.float64); ueq = np.ascontiguousarray(tl.u_eq, dtype=np.float64)
    dims, data, _, keep = pack(tl.prob, x0 - xeq)
    cl = loop.ClosedLoop(plant, steps, DELTA, _lib.ptr(xeq), _lib.ptr(ueq))
    cl.splant_par, cl.plant_par_sched = stride, sched
    if par is not None:
        cl.plant_par = _lib.ptr(par)
    X = np.zeros((b, steps + 1, 4)); U = np.zeros((b, steps, 1)); F = np.zeros((b, steps), np.int32)
    o = _lib.options()
    return lib.bqp_closed_loop_ocp(handle.value, C.byref(dims), b, C.byref(data), C.byref(o), C.byref(cl),
                                   _lib.ptr(x0), _lib.ptr(X), _lib.ptr(U), _lib.iptr(F))


def test_argument_errors(mg, tl1, tl20, learned, nmpcs, handle):
    import bqp
    from bqp import _lib, loop
    E, OK, RK4 = _lib.BQP_E_ARG, _lib.BQP_OK, loop.BQP_PLANT_MG_RK4
    b, steps = 3, 2
    good = np.ascontiguousarray(_draw(61, b))
    gsch = np.ascontiguousarray(_draw(62, b, steps))
    assert _raw_ocp(handle, tl1, b, steps, RK4, good, 4, 0) == OK
    assert _raw_ocp(handle, tl1, b, steps, RK4, good, 0, 0) == OK
    assert _raw_ocp(handle, tl1, b, steps, RK4, gsch, steps * 4, 1) == OK
    assert _raw_ocp(handle, tl1, b, steps, RK4, gsch, 0, 1) == OK
    # non-finite coefficients, in the last instance's row and in a schedule's last row
    for i in range(4):
        for bad in (np.nan, np.inf, -np.inf):
            P = good.copy(); P[b - 1, i] = bad
            assert _raw_ocp(handle, tl1, b, steps, RK4, P, 4, 0) == E, (i, bad)
            P = gsch.copy(); P[b - 1, steps - 1, i] = bad
            assert _raw_ocp(handle, tl1, b, steps, RK4, P, steps * 4, 1) == E, (i, bad)
    # 1/beta^2 <= 0, wn^2 <= 0, 2 zeta wn < 0; no damping and a negative x2_c are admitted
    for i, bad in ((1, 0.0), (1, -1.0), (2, 0.0), (2, -1000.0), (3, -1e-9)):
        P = good.copy(); P[1, i] = bad
        assert _raw_ocp(handle, tl1, b, steps, RK4, P, 4, 0) == E, (i, bad)
        assert _raw_ocp(handle, tl1, b, steps, loop.BQP_PLANT_MG_ODE23, P, 4, 0) == E, (i, bad)
    P = good.copy(); P[1, 3] = 0.0; P[1, 0] = -0.05
    assert _raw_ocp(handle, tl1, b, steps, RK4, P, 4, 0) == OK
    # a row the loop does not read is not checked: shared stride reads instance 0's block alone
    P = good.copy(); P[2, 1] = np.nan
    assert _raw_ocp(handle, tl1, b, steps, RK4, P, 0, 0) == OK
    # strides that are neither 0 nor at least one instance's block
    for stride, sched, par in ((3, 0, good), (-4, 0, good), (steps * 4 - 1, 1, gsch), (4, 1, gsch)):
        assert _raw_ocp(handle, tl1, b, steps, RK4, par, stride, sched) == E, (stride, sched)
    big = np.ascontiguousarray(np.tile(good[:, None], (1, 3, 1)))      # stride 12 > 4: a gap is fine
    assert _raw_ocp(handle, tl1, b, steps, RK4, big, 12, 0) == OK
    for sched in (2, -1):
        assert _raw_ocp(handle, tl1, b, steps, RK4, gsch, steps * 4, sched) == E, sched
    # a null plant_par leaves the other two members unread
    assert _raw_ocp(handle, tl1, b, steps, RK4, None, -7, 9) == OK
    # every other host entry refuses a bad row; the linear plant refuses any coefficients
    bad = good.copy(); bad[1, 2] = 0.0
    X3 = _x0(b)
    refs = np.zeros((steps, 4))
    p3, g3 = nmpcs(3)
    xn = np.ascontiguousarray(p3['x_eq'] + DEVS[:b])
    Xs = np.array([0.15, 1.2875, 1.1547, 0.0]) + np.zeros((b, 4))
    calls = [lambda P: bqp.closed_loop(tl1, X3, steps, handle=handle, plant_params=P),
             lambda P: bqp.closed_loop(learned[0], X3, steps, handle=handle, learning=dict(q=8, mask=1), plant_params=P),
             lambda P: bqp.closed_loop(tl20, X3, steps, handle=handle, refs=refs, plant_params=P),
             lambda P: bqp.closed_loop_sqp(learned[1], Xs, steps, learning=dict(q=10, mask=1), handle=handle, plant_params=P),
             lambda P: bqp.closed_loop_nmpc(g3, xn, steps, handle=handle, plant_params=P),
             lambda P: bqp.closed_loop_nmpc(g3, xn, steps, handle=handle, dist=np.zeros((steps, 4)), plant_params=P)]
    for i, call in enumerate(calls):
        with pytest.raises(_lib.BqpError, match='invalid argument'):
            call(bad)
    di = golden('di_design.npz')
    tm = bqp.TrackingMPC(di['A'], di['B'], di['Q'], di['R'], di['P'], di['T'], di['LAMBDA'], di['PSI'],
                         di['F_x'], di['h_x'], di['F_u'], di['h_u'], di['F_T'], di['h_T'], N=3)
    r = bqp.closed_loop(tm, np.array([[0.0, -1.0]]), 2, plant='linear', refs=np.zeros((2, 2)), handle=handle)
    assert r.X.shape == (1, 3, 2)
    with pytest.raises(_lib.BqpError, match='invalid argument'):
        bqp.closed_loop(tm, np.array([[0.0, -1.0]]), 2, plant='linear', refs=np.zeros((2, 2)), handle=handle,
                        plant_params=M.NOMINAL)
    with pytest.raises(ValueError):
        bqp.closed_loop(tl1, X3, steps, handle=handle, plant_params=np.zeros((b, steps + 1, 4)))


def test_device_path(tl1, tl20, learned, mg, handle):
    """device=: the coefficients travel to the GPU with the loop description; the _device entries
    return what the host entries return, bit for bit"""
    import bqp
    X5 = _x0(5)
    P = _draw(71, 5, 3)
    refs = np.array([0.0, 0.02, -0.02])[:, None] * np.ravel(mg['LAMBDA'])[None, :]
    Xs = np.array([0.15, 1.2875, 1.1547, 0.0]) + np.array([[0.0], [0.01], [-0.01], [0.02], [-0.02]]) * np.array([1.0, 1.0, 0.0, 0.0])
    for tag, run in (('ocp', lambda **k: bqp.closed_loop(tl1, X5, 3, delta=DELTA, plant='ode23', handle=handle, plant_params=P, **k)),
                     ('lbmpc', lambda **k: bqp.closed_loop(learned[0], X5, 3, delta=DELTA, handle=handle,
                                                           learning=dict(q=8, mask=1), plant_params=P, **k)),
                     ('track', lambda **k: bqp.closed_loop(tl20, X5, 3, delta=DELTA, handle=handle, refs=refs, plant_params=P, **k)),
                     ('sqp', lambda **k: bqp.closed_loop_sqp(learned[1], Xs, 3, learning=dict(q=10, mask=1), handle=handle, plant_params=P, **k))):
        rh, rd = run(), run(device=0)
        assert np.array_equal(rh.X, rd.X.cpu().numpy()), tag
        assert np.array_equal(rh.U, rd.U.cpu().numpy()), tag
