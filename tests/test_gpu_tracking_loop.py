"""GPU closed loop with a reference schedule and a linear plant (bqp_closed_loop_track):
trackingMPC/RunExample.m:131-147 - xs = set_ref(k), the F5 solve, x = getTransitions(x, u_0),
art_refHistory - and its disturbed sibling RunExample_robust.m on the sampled double integrator,
and a moving set-point for the Moore-Greitzer tracking LMPC.

The loops are pinned step by step: every applied input is compared with the C restatement of the
solver (oracle/cpu_ref) and with the regularised exact optimum (oracle/make_full_pins.py::_one)
at the GPU's own measured state X[b, t] with that step's linear term, so that a difference does
not compound along the trajectory.  The inputs keep away from two degenerate situations the CPU
restatement itself does not resolve to 1e-8 (a reference on the boundary lambda x_max of the
admissible steady states; a measured state on the state bound): only the reference's own run
(case 4: first set-point 4.95 = 0.99 * 5) goes there, and is held to the F5 first-move bar 1e-6
of tests/test_gpu_ocp.py instead."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

TOL_ITER = 1e-8       # GPU vs C restatement of the same iteration (tests/test_gpu_ocp.py)
TOL_EXACT = 1e-8      # GPU vs the regularised exact optimum
STEPS = 24
SCHEDULES = np.array([[3.0, -3, 1], [-4, 4, 0], [1, -2, 4], [2, 2, -3]])


def _tm(N):
    import bqp
    g = golden('di_design.npz')
    return bqp.TrackingMPC(g['A'], g['B'], g['Q'], g['R'], g['P'], g['T'], g['LAMBDA'], g['PSI'],
                           g['F_x'], g['h_x'], g['F_u'], g['h_u'], g['F_T'], g['h_T'], N=N)


def _ocp(prob):
    p = prob
    return dict(nx=p.nx, nu=p.nu, np=p.np, N=p.N, A=p.A, B=p.B, c=p.c, W=p.W, w=p.w, xlb=p.xlb,
                xub=p.xub, ulb=p.ulb, uub=p.uub, Fp=p.Fp, hp=p.hp, kp=p.poly_stage)


def _refs(x1, hold):
    """(len(x1) * hold, 2) schedule: every x1-reference held for `hold` steps, x2-reference 0"""
    r = np.zeros((len(x1) * hold, 2))
    r[:, 0] = np.repeat(x1, hold)
    return r


@pytest.fixture(scope='module', autouse=True)
def torch_first():
    """torch opens the GPU before libbqp does, the order of smoke() and bench.py.  torch ships its
    own copy of the HIP runtime; in a fresh process whose first GPU call came from libbqp.so (the
    system's copy), torch.cuda.is_available() then answered False and the device= call of
    test_plumbing failed with "No HIP GPUs are available" (this file run alone)."""
    import torch
    torch.cuda.is_available()


@pytest.fixture(scope='module')
def tm30():
    return _tm(30)


@pytest.fixture(scope='module')
def inputs16():
    r = np.random.default_rng(2024)
    x1 = r.uniform(-3, 3, 16)
    x2 = r.uniform(-.5, .5, 16)
    X0 = np.stack([x1, x2], axis=1)
    refs = np.stack([_refs(SCHEDULES[b % 4], 8) for b in range(16)])
    return X0, refs


class _Exact:
    """the regularised exact optimum of oracle/make_full_pins.py::_one for one F5 problem: the
    condensed Hessian is singular exactly on u_{N-1}, which gets the weight 1e-10"""

    def __init__(self, ocp):
        from oracle import exact_qp
        self.ocp, self.eq = ocp, exact_qp
        H = exact_qp.condense_ocp(ocp, np.zeros(ocp['nx']))['H']
        ev, V = np.linalg.eigh(H)
        V0 = V[:, ev < 1e-9 * ev.max()]
        self.Hreg = H + 1e-10 * V0 @ V0.T

    def u0(self, x, w):
        qp = self.eq.condense_ocp(self.ocp, x, w=w)
        r = self.eq.solve(self.Hreg, qp['f'], qp['A'], qp['b'])
        assert r['status'] == 'optimal'
        return r['z'][:self.ocp['nu']]


def _stepwise(tm, r, refs, Ap, Bp, dist, exact=True, every=1):
    """the stepwise assertions of cases 1-3 on a DI run r with per-instance schedules refs
    (b, steps, 2): flags, U against the C restatement and the exact optimum at the GPU's own
    states, theta against single solves, the plant identity.  Returns the measured figures."""
    from oracle import cpu_ref
    b, steps = r.U.shape[:2]
    ocp = _ocp(tm.prob)
    X = r.X[:, :steps].reshape(b * steps, -1)
    XS = refs.reshape(b * steps, -1)
    w, _ = tm.linear_terms(XS)
    c = cpu_ref.solve(ocp, X, w=w)
    U = r.U.reshape(b * steps, -1)
    e_c = np.abs(U - c['u'][:, 0]).max()
    s = tm.solve(X, XS)
    e_th = np.abs(r.theta.reshape(b * steps, -1) - s.theta).max()
    Apb = np.broadcast_to(Ap, (b, 2, 2)); Bpb = np.broadcast_to(Bp, (b, 2, 2))
    pred = np.einsum('bij,btj->bti', Apb, r.X[:, :steps]) + np.einsum('bij,btj->bti', Bpb, r.U)
    if dist is not None:
        pred = pred + dist
    e_pl = np.abs(r.X[:, 1:] - pred).max()
    e_x = np.nan
    if exact:
        ex = _Exact(ocp)
        idx = np.arange(0, b * steps, every)
        e_x = max(np.abs(U[i] - ex.u0(X[i], w[i])).max() for i in idx)
    print('flags %s, cpu_ref flags %s iterations max %d; |U - cpu_ref| %.2e, |U - exact| %.2e, '
          '|theta - solve| %.2e, plant identity %.2e, max|x| %.3f'
          % (np.unique(r.exitflag), np.unique(c['exitflag']), c['iterations'].max(), e_c, e_x, e_th,
             e_pl, np.abs(r.X).max()))
    assert (r.exitflag == 1).all(), np.argwhere(r.exitflag != 1)
    assert e_c < TOL_ITER, e_c
    if exact:
        assert e_x < TOL_EXACT, e_x
    assert e_th < 1e-13, e_th
    assert e_pl < 1e-13, e_pl
    return e_c, e_x


def test_stepwise_parity(tm30, inputs16):
    """case 1: 16 initial states, four schedules of three references held 8 steps each, the
    nominal plant: every step's U against the C restatement and the exact optimum, theta against
    a single TrackingMPC.solve, every transition against x+ = A x + B u"""
    import bqp
    X0, refs = inputs16
    g = golden('di_design.npz')
    r = bqp.closed_loop(tm30, X0, STEPS, plant='linear', refs=refs)
    assert r.X.shape == (16, STEPS + 1, 2) and r.theta.shape == (16, STEPS, 2)
    assert np.array_equal(r.X[:, 0], X0)
    _stepwise(tm30, r, refs, g['A'], g['B'], None)


def test_mismatch_and_disturbance(tm30, inputs16):
    """case 2: per-instance plant (Ap, Bp) != the MPC's model and an additive disturbance
    (RunExample_robust.m's loop), the same stepwise assertions with the plant identity on
    Ap, Bp, d_t"""
    import bqp
    X0, refs = inputs16
    g = golden('di_design.npz')
    q = np.random.default_rng(7)
    Ap = g['A'] + q.uniform(-.02, .02, (16, 2, 2))
    Bp = g['B'] + q.uniform(-.02, .02, (16, 2, 2))
    dist = q.uniform(-.01, .01, (16, STEPS, 2))
    r = bqp.closed_loop(tm30, X0, STEPS, plant='linear', refs=refs, plant_model=(Ap, Bp), dist=dist)
    _stepwise(tm30, r, refs, Ap, Bp, dist)
    # the plant is not the nominal one
    rn = bqp.closed_loop(tm30, X0, STEPS, plant='linear', refs=refs)
    assert np.abs(rn.X - r.X).max() > 1e-3


@pytest.mark.parametrize('N', [30, 3])
def test_unreachable_reference(N):
    """case 3: a reference outside the state box (-6): the artificial reference LAMBDA theta
    stops at the admissible steady states, x1 >= -lambda x_max = -4.95.  N = 3 against the C
    restatement only (the regularised exact solve is unreliable there)"""
    import bqp
    tm = _tm(N)
    g = golden('di_design.npz')
    refs = _refs([3.0, -6.0, 1.0], 8)
    r = bqp.closed_loop(tm, np.array([[0.0, -2.0]]), STEPS, plant='linear', refs=refs)
    _stepwise(tm, r, refs[None], g['A'], g['B'], None, exact=(N == 30))
    art = r.theta[0] @ g['LAMBDA'].T
    print('N = %d: min artificial x1 reference in the -6 segment %.10f' % (N, art[8:16, 0].min()))
    assert (art[8:16, 0] >= -4.95 - 1e-8).all()


def test_reference_run():
    """case 4: RunExample.m's own run - N = 3, x = [0; -2], 100 steps, set_ref's schedule
    (:213-223: 4.95, -5.5, 2, 0 from steps 31 / 61 / 91) - against the same loop driven by the C
    restatement.  The first set-point is lambda x_max exactly, a degenerate optimum: the C
    restatement runs to its iteration limit there and is itself 1.5e-8 from the exact first
    move, so the states are held to the F5 first-move bar 1e-6."""
    import bqp
    from oracle import cpu_ref
    tm = _tm(3)
    g = golden('di_design.npz')
    k = np.arange(1, 101)
    x1 = np.where(k <= 30, 4.95, np.where(k <= 60, -5.5, np.where(k <= 90, 2.0, 0.0)))
    refs = np.stack([x1, np.zeros(100)], axis=1)
    r = bqp.closed_loop(tm, np.array([[0.0, -2.0]]), 100, plant='linear', refs=refs)
    ocp = _ocp(tm.prob)
    w, _ = tm.linear_terms(refs)
    x = np.array([0.0, -2.0]); Xc = [x]
    for t in range(100):
        c = cpu_ref.solve(ocp, x[None], w=w[t:t + 1])
        x = g['A'] @ x + g['B'] @ c['u'][0, 0]; Xc.append(x)
    e = np.abs(r.X[0] - np.array(Xc)).max()
    print('RunExample.m run: flags %s, |X - cpu_ref loop| %.2e' % (np.unique(r.exitflag, return_counts=True), e))
    assert (r.exitflag >= 0).all(), r.exitflag
    assert e < 1e-6, e


def test_mg_moving_setpoint(mg, term_set):
    """case 5: the MG tracking LMPC (N = 20, RK4 plant) with a set-point LAMBDA ths moving
    0 -> 0.02 -> -0.02: U against the C restatement with w[N] = Wr r, transitions against mg_rk4;
    an all-zero schedule equals today's bqp.closed_loop"""
    import bqp
    from oracle import cpu_ref, qp_forms
    from oracle.mg_model import mg_rk4
    tl = bqp.TrackingLMPC(mg['A'], mg['B'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'],
                          mg['LAMBDA'], mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'],
                          term_set[0], term_set[1], mg['x_wp'], mg['u_wp'], N=20)
    X0 = golden('dms_DSS_tLMPC.npz')['x'][[0, 100, 300, 450]]
    steps = 12
    ths = np.repeat([0.0, 0.02, -0.02], 4)
    refs = ths[:, None] * np.ravel(mg['LAMBDA'])[None, :]            # (steps, 4), deviation coords
    r = bqp.closed_loop(tl, X0, steps, delta=0.01, refs=refs)
    assert (r.exitflag == 1).all(), r.exitflag
    Wr = tl.reference_map()
    nv = 6
    assert Wr.shape == (21 * nv, 4) and not Wr[:20 * nv].any() and not Wr[20 * nv:20 * nv + 5].any()
    ocp = qp_forms.dms_ocp(mg, 20, *term_set)
    X = r.X[:, :steps].reshape(4 * steps, 4)
    w = np.tile((refs @ Wr.T).reshape(steps, 21, nv), (4, 1, 1))
    c = cpu_ref.solve(ocp, X - np.ravel(mg['x_wp']), w=w)
    e_c = np.abs(r.U.reshape(-1) - (c['u'][:, 0, 0] + np.ravel(mg['u_wp'])[0])).max()
    e_pl = max(np.abs(mg_rk4(0.01, r.X[i, t], r.U[i, t, 0]) - r.X[i, t + 1]).max()
               for i in range(4) for t in range(steps))
    moved = np.abs(r.theta[:, 4:8, 0] - 0.02).max()
    print('MG: cpu_ref flags %s iterations max %d, |U - cpu_ref| %.2e, |X+ - rk4| %.2e, '
          '|theta - 0.02| in segment 2 %.2e' % (np.unique(c['exitflag']), c['iterations'].max(), e_c, e_pl, moved))
    assert (c['exitflag'] == 1).all()
    assert e_c < TOL_ITER, e_c
    assert e_pl < 1e-13, e_pl
    # the schedule-free loop
    r0 = bqp.closed_loop(tl, X0, steps, delta=0.01)
    rz = bqp.closed_loop(tl, X0, steps, delta=0.01, refs=np.zeros((steps, 4)))
    assert np.abs(rz.X - r0.X).max() < 1e-13 and np.abs(rz.U - r0.U).max() < 1e-13
    assert np.array_equal(rz.exitflag, r0.exitflag)
    assert np.abs(r.X - r0.X).max() > 1e-6          # the moving set-point moves the loop


def test_plumbing(tm30, inputs16):
    """case 6: device=0 equals the host call; a shared schedule equals its per-instance copies;
    dist=None equals a zero dist; batch 1 and batch 130 (more than one block of the advance
    kernel) agree on instance 0 - all bit for bit"""
    import torch
    import bqp
    X0, refs = inputs16
    q = np.random.default_rng(7)
    g = golden('di_design.npz')
    Ap = g['A'] + q.uniform(-.02, .02, (16, 2, 2))
    dist = q.uniform(-.01, .01, (16, 8, 2))
    kw = dict(plant='linear', refs=refs[:, :8], plant_model=(Ap, g['B']), dist=dist)
    rh = bqp.closed_loop(tm30, X0, 8, **kw)
    rd = bqp.closed_loop(tm30, X0, 8, device=0, **kw)
    assert isinstance(rd.X, torch.Tensor) and rd.X.is_cuda
    for k in ('X', 'U', 'theta', 'exitflag'):
        assert np.array_equal(rd[k].cpu().numpy(), rh[k]), k
    shared = refs[0, :8]
    rs = bqp.closed_loop(tm30, X0, 8, plant='linear', refs=shared)
    rp = bqp.closed_loop(tm30, X0, 8, plant='linear', refs=np.tile(shared, (16, 1, 1)))
    rz = bqp.closed_loop(tm30, X0, 8, plant='linear', refs=shared, dist=np.zeros((16, 8, 2)))
    for k in ('X', 'U', 'theta', 'exitflag'):
        assert np.array_equal(rs[k], rp[k]), k
        assert np.array_equal(rs[k], rz[k]), k
    assert np.abs(rs.X - rh.X).max() > 1e-3
    big = np.tile(X0, (9, 1))[:130]
    big[1:] += 1e-3 * np.arange(1, 130)[:, None] / 130
    r1 = bqp.closed_loop(tm30, big[:1], 8, plant='linear', refs=shared)
    rb = bqp.closed_loop(tm30, big, 8, plant='linear', refs=np.tile(shared, (130, 1, 1)))
    for k in ('X', 'U', 'theta', 'exitflag'):
        assert np.array_equal(r1[k][0], rb[k][0]), k
    # the last instance, in the second block of the advance kernel, against its own run
    rl = bqp.closed_loop(tm30, big[129:], 8, plant='linear', refs=shared)
    for k in ('X', 'U', 'theta', 'exitflag'):
        assert np.array_equal(rl[k][0], rb[k][129]), k
    # a measured state outside the x_0 box rows: -2 from the host check, as TrackingMPC.solve
    out = np.array([[5.2, 0.0]])
    assert tm30.solve(out, shared[0]).exitflag[0] == -2
    assert bqp.closed_loop(tm30, out, 1, plant='linear', refs=shared[:1]).exitflag[0, 0] == -2
    assert int(bqp.closed_loop(tm30, out, 1, plant='linear', refs=shared[:1], device=0).exitflag[0, 0]) == -2


def test_argument_errors(mg, term_set, tm30):
    """case 7: Ap with an MG plant, nr > 0 without Wr or ref, steps = 0: BQP_E_ARG"""
    import bqp
    from bqp import _lib, loop
    from bqp.ocp import pack
    lib = bqp.load()
    h = bqp.Handle(0)
    tl = bqp.TrackingLMPC(mg['A'], mg['B'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'],
                          mg['LAMBDA'], mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'],
                          term_set[0], term_set[1], mg['x_wp'], mg['u_wp'], N=20)

    def call(mpc, plant, steps, nx, nu, **fields):
        x0 = np.zeros((1, nx))
        dims, data, _, keep = pack(mpc.prob, x0)
        xeq, ueq = np.zeros(nx), np.zeros(nu)
        cl = loop.ClosedLoop(plant, steps, 0.01, _lib.ptr(xeq), _lib.ptr(ueq))
        tr = _lib.Track()
        for k, v in fields.items():
            setattr(tr, k, _lib.ptr(v) if isinstance(v, np.ndarray) else v)
        S = max(steps, 1)
        X = np.zeros((1, S + 1, nx)); U = np.zeros((1, S, nu)); F = np.zeros((1, S), np.int32)
        o = _lib.options()
        return lib.bqp_closed_loop_track(h.value, C.byref(dims), 1, C.byref(data), C.byref(o),
                                         C.byref(cl), C.byref(tr), _lib.ptr(x0), _lib.ptr(X),
                                         _lib.ptr(U), _lib.iptr(F))

    A4 = np.eye(4)
    assert call(tl, loop.BQP_PLANT_MG_RK4, 2, 4, 1, Ap=A4) == _lib.BQP_E_ARG
    nw = 31 * 6
    Wr = np.zeros((2, nw)); ref = np.zeros((2, 2))
    assert call(tm30, loop.BQP_PLANT_LINEAR, 2, 2, 2, nr=2, ref=ref) == _lib.BQP_E_ARG
    assert call(tm30, loop.BQP_PLANT_LINEAR, 2, 2, 2, nr=2, Wr=Wr) == _lib.BQP_E_ARG
    assert call(tm30, loop.BQP_PLANT_LINEAR, 0, 2, 2, nr=2, Wr=Wr, ref=ref) == _lib.BQP_E_ARG
    assert call(tm30, 7, 2, 2, 2) == _lib.BQP_E_ARG
    # the same descriptions, valid: they run
    assert call(tm30, loop.BQP_PLANT_LINEAR, 2, 2, 2, nr=2, Wr=Wr, ref=ref) == _lib.BQP_OK
    assert call(tl, loop.BQP_PLANT_MG_RK4, 2, 4, 1) == _lib.BQP_OK
    with pytest.raises(ValueError):
        bqp.closed_loop(tl, np.zeros((1, 4)), 2, plant_model=(A4, np.zeros((4, 1))))
    h.close()
