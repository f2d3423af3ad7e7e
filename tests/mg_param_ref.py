"""The Moore-Greitzer plant with per-instance coefficients p = [x2_c, 1/beta^2, wn^2, 2 zeta wn]
(bqp_closed_loop.plant_par, csrc/bqp_mg.h), restated in numpy: the right-hand side in the kernels'
operation order, the RK4 step and MATLAB's ode23 - the algorithm of oracle/mg_model.py mg_ode23,
statement for statement, on the parametrised right-hand side - and the steady state.  At the
nominal p the two integrators equal oracle.mg_model's bit for bit (tests/test_mg_param_host.py).
Also the seeded parameter draws and the transition comparison the GPU tests share."""
import numpy as np

NOMINAL = np.array([0.0, 1.0, 1000.0, 2.0 * np.sqrt(500.0)])


def mg_rhs_p(p, x, u):
    return np.array([
        -x[1] + p[0] + 1 + 3 * (x[0] / 2) - (x[0] ** 3 / 2),
        (x[0] + 1 - x[2] * np.sqrt(x[1])) * p[1],
        x[3],
        -p[2] * x[2] - p[3] * x[3] + p[2] * u,
    ])


def mg_rk4_p(p, delta, x, u):
    k1 = mg_rhs_p(p, x, u)
    k2 = mg_rhs_p(p, x + delta / 2 * k1, u)
    k3 = mg_rhs_p(p, x + delta / 2 * k2, u)
    k4 = mg_rhs_p(p, x + delta * k3, u)
    return x + delta / 6 * (k1 + 2 * k2 + 2 * k3 + k4)


def mg_ode23_p(p, delta, x, u, rtol=1e-3, atol=1e-6):
    """x(delta) and the error estimate `err` of every attempted step, accepted or rejected, in
    order: the numbers the accept / reject decisions compare with rtol."""
    f = lambda y: mg_rhs_p(p, y, u)                               # noqa: E731
    errs = []
    t, y = 0.0, np.array(x, float)
    T = float(delta)
    hmax, thr, pw = 0.1 * T, atol / rtol, 1.0 / 3.0
    Bt = np.array([[1 / 2, 0, 2 / 9], [0, 3 / 4, 1 / 3], [0, 0, 4 / 9], [0, 0, 0]])
    E = np.array([-5 / 72, 1 / 12, 1 / 9, -1 / 8])
    F = np.zeros((4, 4))
    F[:, 0] = f(y)
    absh = min(hmax, T)
    rh = np.max(np.abs(F[:, 0] / np.maximum(np.abs(y), thr))) / (0.8 * rtol ** pw)
    if absh * rh > 1:
        absh = 1 / rh
    done = False
    while not done:
        hmin = 16 * np.spacing(t)
        absh = min(hmax, max(hmin, absh))
        h = absh
        if 1.1 * absh >= abs(T - t):
            h = T - t
            absh = abs(h)
            done = True
        nofailed = True
        while True:
            hB = h * Bt
            F[:, 1] = f(y + F @ hB[:, 0])
            F[:, 2] = f(y + F @ hB[:, 1])
            tnew = T if done else t + h
            h = tnew - t
            ynew = y + F @ (h * Bt[:, 2])
            F[:, 3] = f(ynew)
            err = absh * np.max(np.abs((F @ E) / np.maximum(np.maximum(np.abs(y), np.abs(ynew)), thr)))
            errs.append(err)
            if not err > rtol:
                break
            if absh <= hmin:
                break
            absh = max(hmin, absh * max(0.5, 0.8 * (rtol / err) ** pw)) if nofailed \
                else max(hmin, 0.5 * absh)
            nofailed = False
            h = absh
            done = False
        if not done and nofailed:
            temp = 1.25 * (err / rtol) ** pw
            absh = absh / temp if temp > 0.2 else 5.0 * absh
        t, y = tnew, ynew
        F[:, 0] = F[:, 3]
    return y, np.array(errs)


def mg_steady_state(p, x1):
    """(x_s, u_s): f(x_s, u_s) = 0 at the mass flow x1; independent of p[1:]"""
    x2 = p[0] + 1.0 + 1.5 * x1 - x1 * x1 * x1 / 2.0
    x3 = (x1 + 1.0) / np.sqrt(x2)
    return np.array([x1, x2, x3, 0.0]), x3


def draw_params(rng, shape=()):
    """p = nominal (1 + U(-0.1, 0.1)) with x2_c = U(-0.05, 0.05), shape + (4,)"""
    p = NOMINAL * (1.0 + rng.uniform(-0.1, 0.1, tuple(shape) + (4,)))
    p[..., 0] = rng.uniform(-0.05, 0.05, tuple(shape))
    return p


def step_p(p, plant, delta, x, u):
    """one sampling period by the integrator `plant` ('rk4' / 'ode23')"""
    return mg_rk4_p(p, delta, x, u) if plant == 'rk4' else mg_ode23_p(p, delta, x, u)[0]


def transition_errors(P, plant, delta, X, U, dist=None):
    """max over (instance, step) of |X[b, t + 1] - (step_p(P[b, t], X[b, t], U[b, t]) + dist[b, t])|,
    as an array (batch, steps).  P is (batch, steps, 4) (broadcast it first)."""
    X = np.asarray(X, float)
    U = np.asarray(U, float).reshape(X.shape[0], X.shape[1] - 1)
    out = np.zeros(U.shape)
    for b in range(U.shape[0]):
        for t in range(U.shape[1]):
            xn = step_p(P[b, t], plant, delta, X[b, t], U[b, t])
            if dist is not None:
                xn = xn + dist[b, t]
            out[b, t] = np.max(np.abs(X[b, t + 1] - xn))
    return out


def ode23_margin(P, delta, X, U):
    """min over every ode23 attempt of the loop's transitions of |err / rtol - 1|: above 1e-6 no
    rounding difference between two evaluations can flip an accept / reject decision"""
    X = np.asarray(X, float)
    U = np.asarray(U, float).reshape(X.shape[0], X.shape[1] - 1)
    m = np.inf
    for b in range(U.shape[0]):
        for t in range(U.shape[1]):
            errs = mg_ode23_p(P[b, t], delta, X[b, t], U[b, t])[1]
            m = min(m, np.min(np.abs(errs / 1e-3 - 1.0)))
    return m


def full_params(p, b, steps):
    """any accepted plant_params shape as (batch, steps, 4), under the rule of bqp.loop._plant_params"""
    p = np.asarray(p, float)
    if p.shape == (4,):
        return np.broadcast_to(p, (b, steps, 4))
    if p.shape == (steps, 4):
        return np.broadcast_to(p[None], (b, steps, 4))
    if p.shape == (b, 4):
        return np.broadcast_to(p[:, None], (b, steps, 4))
    assert p.shape == (b, steps, 4), p.shape
    return p
