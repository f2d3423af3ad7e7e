"""TEST INFRASTRUCTURE ONLY: numpy restatement of the nonlinear MPC problem on the true
Moore-Greitzer model (examples/DMS_tracking_NMPC_casadi.m:121-126, 225-293) and of the algorithm
the GPU path (bqp/nmpc.py + csrc/bqp_nmpc.hip) uses for it.  One instance at a time.

Problem, states eliminated (single shooting): z = [u_0 - u_eq, .., u_{N-1} - u_eq; theta],
n = N + 1; x_{k+1} = dynamic(delta, x_k, u_k) (one RK4 step of `system`, oracle.mg_model.mg_rk4);
cost  sum_{k<N} delta [(x_k - x_eq - L th)'Q(.) + (u_k - u_eq - Psi th)'R(.)]
      + (x_N - x_eq - L th)'P(.) + (L th)'T(L th)        (a sum of squared weighted residuals e);
constraint rows c(z) <= 0, in this order: for k = 1..N  F_x (x_k - x_eq) - h_x, then
F_u (u_{k-1} - u_eq) - h_u; then F_T [x_N - x_eq; theta] - h_T.  That is IPOPT's lam_g order
with the dynamics rows removed.

Algorithm: Gauss-Newton SQP, H = 2 Jr'Jr, f = 2 Jr'e, sub-problem min 0.5 d'Hd + f'd s.t.
C d <= -c, L1 merit phi = J + nu V, V = sum max(c, 0), nu <- max(nu, 1.1 max lam) within a
solve, D = f'd - nu V(z), first alpha = 2^-t (t = 0..7) with phi(z + alpha d) <= phi(z) + 1e-4
alpha D (a trial whose rollout is not finite is rejected), else alpha = 2^-7.  Stopping as the
learned-model SQP's update kernel: feasible (max c <= 1e-9) and either the KKT test (step and
stationarity |f + C'lam|) or the step at the sub-problem's accuracy with a stagnant cost.
Flags: 1 converged, 0 iteration limit, -2 sub-problem infeasible, -8 numerical failure.
"""
import numpy as np

from oracle import dense_qp
from oracle.mg_model import mg_rk4   # noqa: F401  (re-exported for the tests)

SQ500 = np.sqrt(500.0)


def problem(mg, F_T, h_T, N, delta=0.01):
    """the data of DMS_tracking_NMPC_casadi.m from the offline design (oracle.mg_model.mg_problem)
    and the stored terminal set"""
    return dict(N=N, delta=delta, Q=np.asarray(mg['Q'], float), R=np.atleast_2d(mg['R']).astype(float),
                P=np.asarray(mg['P'], float), T=float(mg['Tscalar']) * np.eye(4),
                LAMBDA=np.asarray(mg['LAMBDA'], float).reshape(4), PSI=float(np.ravel(mg['PSI'])[0]),
                F_x=np.asarray(mg['F_x'], float), h_x=np.asarray(mg['h_x'], float),
                F_u=np.asarray(mg['F_u'], float).reshape(-1, 1), h_u=np.asarray(mg['h_u'], float),
                F_T=np.asarray(F_T, float), h_T=np.asarray(h_T, float).ravel(),
                x_eq=np.asarray(mg['x_wp'], float), u_eq=float(mg['u_wp']))


def rows(p):
    return p['N'] * (p['F_x'].shape[0] + p['F_u'].shape[0]) + p['F_T'].shape[0]


def mg_rhs(x, u):
    return np.array([-x[1] + 1 + 3 * (x[0] / 2) - (x[0] ** 3 / 2),
                     x[0] + 1 - x[2] * np.sqrt(x[1]),
                     x[3],
                     -1000 * x[2] - 2 * SQ500 * x[3] + 1000 * u])


def mg_jac(x):
    """analytic d system / dx (4 x 4); d system / du = [0 0 0 1000]'"""
    sq = np.sqrt(x[1])
    return np.array([[1.5 - 1.5 * x[0] ** 2, -1.0, 0.0, 0.0],
                     [1.0, -x[2] / (2.0 * sq), -sq, 0.0],
                     [0.0, 0.0, 0.0, 1.0],
                     [0.0, 0.0, -1000.0, -2.0 * SQ500]])


FU = np.array([0.0, 0.0, 0.0, 1000.0])


def rk4_jac(delta, x, u):
    """x+ = dynamic(delta, x, u) with A = dx+/dx and B = dx+/du, differentiated through the four
    RK stages"""
    h = delta
    eye = np.eye(4)
    k1 = mg_rhs(x, u); K1x = mg_jac(x); K1u = FU
    y = x + h / 2 * k1
    k2 = mg_rhs(y, u); Jy = mg_jac(y); K2x = Jy @ (eye + h / 2 * K1x); K2u = Jy @ (h / 2 * K1u) + FU
    y = x + h / 2 * k2
    k3 = mg_rhs(y, u); Jy = mg_jac(y); K3x = Jy @ (eye + h / 2 * K2x); K3u = Jy @ (h / 2 * K2u) + FU
    y = x + h * k3
    k4 = mg_rhs(y, u); Jy = mg_jac(y); K4x = Jy @ (eye + h * K3x); K4u = Jy @ (h * K3u) + FU
    xn = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    A = eye + h / 6 * (K1x + 2 * K2x + 2 * K3x + K4x)
    B = h / 6 * (K1u + 2 * K2u + 2 * K3u + K4u)
    return xn, A, B


def rollout(p, x0, z, jac=False):
    """X (N+1, 4) absolute from the measured state x0 (absolute); with jac also the stage
    Jacobians A (N, 4, 4), B (N, 4) and the sensitivities S (N+1, 4, n) = dX/dz"""
    N = p['N']
    n = N + 1
    X = np.zeros((N + 1, 4)); X[0] = x0
    if not jac:
        with np.errstate(invalid='ignore', over='ignore'):
            for k in range(N):
                X[k + 1] = mg_rk4(p['delta'], X[k], z[k] + p['u_eq'])
        return X
    A = np.zeros((N, 4, 4)); B = np.zeros((N, 4)); S = np.zeros((N + 1, 4, n))
    for k in range(N):
        X[k + 1], A[k], B[k] = rk4_jac(p['delta'], X[k], z[k] + p['u_eq'])
        S[k + 1] = A[k] @ S[k]
        S[k + 1][:, k] += B[k]
    return X, A, B, S


def _factors(p):
    up = lambda M: np.linalg.cholesky(np.atleast_2d(M)).T          # noqa: E731  U'U = M
    return up(p['delta'] * p['Q']), up(p['delta'] * p['R']), up(p['P']), up(p['T'])


def residuals(p, X, z, S=None):
    """weighted residuals e (5 N + 8) with J = e'e; with S also their Jacobian Jr (5 N + 8, n).
    Rows: per stage k the 4 state rows then the input row; then the P rows and the T rows."""
    N = p['N']
    n = N + 1
    Lq, Lr, Lp, Lt = _factors(p)
    th = z[N]
    lam, psi = p['LAMBDA'], p['PSI']
    e = np.zeros(5 * N + 8)
    Jr = np.zeros((5 * N + 8, n)) if S is not None else None
    for k in range(N):
        e[5 * k:5 * k + 4] = Lq @ (X[k] - p['x_eq'] - lam * th)
        e[5 * k + 4] = Lr[0, 0] * (z[k] - psi * th)
        if S is not None:
            Sx = S[k].copy(); Sx[:, N] -= lam
            Jr[5 * k:5 * k + 4] = Lq @ Sx
            Jr[5 * k + 4, k] = Lr[0, 0]
            Jr[5 * k + 4, N] = -Lr[0, 0] * psi
    e[5 * N:5 * N + 4] = Lp @ (X[N] - p['x_eq'] - lam * th)
    e[5 * N + 4:] = Lt @ (lam * th)
    if S is not None:
        Sx = S[N].copy(); Sx[:, N] -= lam
        Jr[5 * N:5 * N + 4] = Lp @ Sx
        Jr[5 * N + 4:, N] = Lt @ lam
    return (e, Jr) if S is not None else e


def constraints(p, X, z, S=None):
    """c (m); with S also C = dc/dz (m, n)"""
    N = p['N']
    n = N + 1
    Fx, Fu, FT = p['F_x'], p['F_u'], p['F_T']
    mx, mu = Fx.shape[0], Fu.shape[0]
    ms = mx + mu
    m = rows(p)
    c = np.zeros(m)
    C = np.zeros((m, n)) if S is not None else None
    for k in range(1, N + 1):
        r = ms * (k - 1)
        c[r:r + mx] = Fx @ (X[k] - p['x_eq']) - p['h_x']
        c[r + mx:r + ms] = Fu[:, 0] * z[k - 1] - p['h_u']
        if S is not None:
            C[r:r + mx] = Fx @ S[k]
            C[r + mx:r + ms, k - 1] = Fu[:, 0]
    r = ms * N
    c[r:] = FT[:, :4] @ (X[N] - p['x_eq']) + FT[:, 4] * z[N] - p['h_T']
    if S is not None:
        C[r:] = FT[:, :4] @ S[N]
        C[r:, N] += FT[:, 4]
    return (c, C) if S is not None else c


def cost(p, x0, z):
    e = residuals(p, rollout(p, x0, z), z)
    return float(e @ e)


def linearize(p, x0, z):
    """everything the GPU's linearisation returns: X, cost, c, C, H, f (and e, Jr, A, B)"""
    X, A, B, S = rollout(p, x0, z, jac=True)
    e, Jr = residuals(p, X, z, S)
    c, C = constraints(p, X, z, S)
    return dict(X=X, cost=float(e @ e), c=c, C=C, H=2.0 * Jr.T @ Jr, f=2.0 * Jr.T @ e, e=e, Jr=Jr,
                A=A, B=B, S=S)


def trial(p, x0, z):
    """cost and violation V at z without Jacobians; (nan, nan) if the rollout is not finite"""
    X = rollout(p, x0, z)
    if not np.all(np.isfinite(X)):
        return np.nan, np.nan
    e = residuals(p, X, z)
    c = constraints(p, X, z)
    return float(e @ e), float(np.maximum(c, 0.0).sum())


def sqp(p, x0, z0=None, max_iter=100, tol=1e-8, trace=None):
    """the SQP of the module doc.  Returns z, lam, info(exitflag, iterations, cost, stat)."""
    N = p['N']
    n = N + 1
    m = rows(p)
    z = np.zeros(n) if z0 is None else np.array(z0, float)
    lam = np.zeros(m)
    tol_step, tol_stat = tol, 10.0 * tol
    nu = 0.0
    cprev = np.inf
    flag, it, stat = 0, 0, np.inf
    J = np.nan
    while True:
        L = linearize(p, x0, z)
        H, f, c, C, J = L['H'], L['f'], L['c'], L['C'], L['cost']
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(C))):
            flag = -8
            break
        qp = dict(H=H, f=f, A=C, b=-c, Aeq=np.zeros((0, n)), beq=np.zeros(0),
                  lb=np.full(n, -np.inf), ub=np.full(n, np.inf))
        d, _, lamq, _ = dense_qp.solve(qp)
        lam = lamq['ineqlin']
        if not (np.all(np.isfinite(d)) and np.all(np.isfinite(lam))):
            from oracle import exact_qp
            r = exact_qp.solve(H, f, C, -c)
            if r['z'] is None:
                flag = -2                               # no point satisfies the linearised rows
                break
            d, lam = r['z'], r['lam']
        if not np.all(np.isfinite(d)):
            flag = -8
            break
        if (C @ d + c).max() > 1e-7 * (1.0 + np.abs(c).max()):
            flag = -2                                   # the linearised rows have no common point
            break
        stat = np.abs(f + C.T @ lam).max()
        dn, zn, fn = np.abs(d).max(), np.abs(z).max(), np.abs(f).max()
        feas0 = c.max() <= 1e-9
        if trace is not None:
            trace.append(dict(it=it, J=J, step=dn, stat=stat, viol=c.max()))
        if feas0 and ((dn <= tol_step * (1 + zn) and stat <= tol_stat * (1 + fn)) or
                      (it > 0 and dn <= 1e-6 * (1 + zn) and abs(cprev - J) <= 1e-12 * (1 + abs(J)))):
            flag = 1
            break
        V0 = np.maximum(c, 0.0).sum()
        nu = max(nu, 1.1 * lam.max(initial=0.0))
        D = f @ d - nu * V0
        phi0 = J + nu * V0
        tsel = 7
        for t in range(8):
            a = 0.5 ** t
            Jt, Vt = trial(p, x0, z + a * d)
            if np.isfinite(Jt) and np.isfinite(Vt) and Jt + nu * Vt <= phi0 + 1e-4 * a * D:
                tsel = t
                break
        a = 0.5 ** tsel
        if not np.isfinite(trial(p, x0, z + a * d)[0]):
            flag = -8
            break
        z = z + a * d
        cprev = J
        it += 1
        if it >= max_iter:
            flag = 0
            J = cost(p, x0, z)
            break
    return z, lam, dict(exitflag=flag, iterations=it, cost=J, stat=stat)


def kkt(p, x0, z, lam):
    """stationarity |grad J + C'lam|_inf, |grad J|_inf, max c and min lam at (z, lam), by this
    restatement's model"""
    L = linearize(p, x0, z)
    return dict(stat=np.abs(L['f'] + L['C'].T @ lam).max(), grad=np.abs(L['f']).max(),
                cmax=L['c'].max(), lam_min=lam.min(initial=0.0))


def to_y(p, x0, z):
    """y_OL in the script's layout [x_0..x_N; u; theta], absolute"""
    X = rollout(p, x0, z)
    return np.concatenate([X.ravel(), z[:p['N']] + p['u_eq'], z[p['N']:]])
