"""TEST INFRASTRUCTURE ONLY: the set-point of the nonlinear MPC's tracking cost
(bqp_nmpc_data.x_ref) and the closed loop with a set-point schedule and a disturbed plant
(bqp_closed_loop_nmpc_track), put on top of the numpy restatements tests/nmpc_ref.py,
tests/nmpc_stage_ref.py, tests/nmpc_dms_ref.py and tests/nmpc_soft_ref.py, which stay as they are.
One instance at a time.

With the target state x_s (absolute) and rho = x_s - x_eq the offset term of the cost,
(LAMBDA th)'T(LAMBDA th), becomes (LAMBDA th - rho)'T(LAMBDA th - rho); nothing else changes, and the
set-point is constant over the horizon.  In the restatements that is

    the T rows of the weighted residuals:  e_T = Lt LAMBDA th - Lt rho      (nmpc_ref.residuals),
    the stage gradient:                    w_N[theta] += g,  g = -2 rho'T LAMBDA
                                                                        (nmpc_stage_ref.stage_problem),
    the cost:                              += g th + c0,  c0 = rho'T rho     (through e_T),

and `reference` below applies exactly these for the duration of a with-block: every function of the
four modules reaches the residuals and the stage problem through those two names, so linearize,
trial, sqp, kkt, dms_problem, the multiple-shooting sqp and the soft-row sqp all see the set-point.
rho = 0 subtracts 0 and adds -0: the restatements' own values, bit for bit.

The loop (`loop`): per step the solve at the measured state with the step's set-point, the plant
oracle.mg_model.mg_rk4 with u_0 plus the step's disturbance, and the warm start of the GPU loop (z
shifted one stage, the last move repeated, theta kept; with multiple shooting
nmpc_dms_ref.warm_start).
"""
import contextlib

import numpy as np

import nmpc_dms_ref as DR
import nmpc_ref as R
import nmpc_soft_ref as FR
import nmpc_stage_ref as SR


def rho_of(p, x_ref):
    return np.asarray(x_ref, float).reshape(4) - p['x_eq']


def offset(p, x_ref):
    """(g, c0): the cost gains g theta + c0"""
    rho = rho_of(p, x_ref)
    return float(-2.0 * rho @ p['T'] @ p['LAMBDA']), float(rho @ p['T'] @ rho)


@contextlib.contextmanager
def reference(p, x_ref):
    """the restatements with the set-point x_ref (None: as they are) inside the with-block"""
    if x_ref is None:
        yield
        return
    rho = rho_of(p, x_ref)
    g, _ = offset(p, x_ref)
    res0, sp0 = R.residuals, SR.stage_problem

    def residuals(pp, X, z, S=None):
        out = res0(pp, X, z, S)
        e = out[0] if S is not None else out
        e[5 * pp['N'] + 4:] -= R._factors(pp)[3] @ rho
        return out

    def stage_problem(pp, x0, z, lin=None):
        sp = sp0(pp, x0, z, lin)
        sp['w'][pp['N'], 5] += g
        return sp

    R.residuals, SR.stage_problem = residuals, stage_problem
    try:
        yield
    finally:
        R.residuals, SR.stage_problem = res0, sp0


def _with(mod, name):
    """mod.name(p, ...) with the set-point: call(p, x_ref, ...); the name is looked up inside the
    with-block, so that the two replaced functions themselves can be called this way"""
    def call(p, x_ref, *a, **kw):
        with reference(p, x_ref):
            return getattr(mod, name)(*((p,) + a), **kw)
    call.__doc__ = '%s.%s(p, ...) with the set-point x_ref: call(p, x_ref, ...)' % (mod.__name__, name)
    return call


linearize = _with(R, 'linearize')             # (p, x_ref, x0, z)
cost = _with(R, 'cost')
sqp = _with(R, 'sqp')                         # (p, x_ref, x0, z0=None, ...)
kkt = _with(R, 'kkt')                         # (p, x_ref, x0, z, lam)
stage_problem = _with(SR, 'stage_problem')    # (p, x_ref, x0, z)
dms_problem = _with(DR, 'dms_problem')        # (p, x_ref, x0, X, z)
dms_sqp = _with(DR, 'sqp')                    # (p, x_ref, x0, z0=None, X0=None, ...)
dms_kkt = _with(DR, 'kkt')                    # (p, x_ref, x0, X, z, lam, pi)
soft_sqp = _with(FR, 'sqp')                   # (p, x_ref, x0, l1, l2, z0=None, ...)
soft_kkt = _with(FR, 'kkt')                   # (p, x_ref, x0, z, lam, l1, l2)


def stage_f(p, x_ref, x0, z):
    """the condensed gradient of the stage problem (the adjoint sweep over its w_k): the dense f"""
    with reference(p, x_ref):
        return SR.adjoint(p, SR.stage_problem(p, x0, z))


def shift(p, z):
    """the loop's warm start of z: one stage on, the last move repeated, theta kept"""
    N = p['N']
    return np.concatenate([z[1:N], z[N - 1:N], z[N:]])


def loop(p, x_init, steps, refs=None, dist=None, route='single', l1=None, l2=None, tol=1e-8):
    """the closed loop of the module doc from x_init (absolute).  refs, dist: (steps, 4) or None.
    route: 'single' (nmpc_ref.sqp), 'multiple' (nmpc_dms_ref.sqp) or 'soft' (nmpc_soft_ref.sqp with
    the weights l1, l2).  Returns X (steps + 1, 4), U, theta, exitflag, iterations (steps each)."""
    N = p['N']
    X = np.zeros((steps + 1, 4)); X[0] = x_init
    U = np.zeros(steps); TH = np.zeros(steps)
    fl = np.zeros(steps, int); it = np.zeros(steps, int)
    z, Xs = np.zeros(N + 1), None
    for t in range(steps):
        x_ref = None if refs is None else refs[t]
        if route == 'multiple':
            Xs, z, _, _, info = dms_sqp(p, x_ref, X[t], z0=z, X0=Xs, tol=tol)
        elif route == 'soft':
            z, _, info = soft_sqp(p, x_ref, X[t], l1, l2, z0=z, tol=tol)
        else:
            z, _, info = sqp(p, x_ref, X[t], z0=z, tol=tol)
        fl[t], it[t] = info['exitflag'], info['iterations']
        U[t], TH[t] = z[0] + p['u_eq'], z[N]
        X[t + 1] = R.mg_rk4(p['delta'], X[t], U[t])
        if dist is not None:
            X[t + 1] = X[t + 1] + dist[t]
        if route == 'multiple':
            Xs, z = DR.warm_start(p, Xs, z, X[t + 1])
        else:
            z = shift(p, z)
    return X, U, TH, fl, it
