"""TEST INFRASTRUCTURE ONLY: numpy restatement of the nonlinear MPC's direct multiple shooting
(bqp_nmpc_dims.shooting = 1; csrc/bqp_nmpc.hip's nmpc_dms_* kernels, csrc/bqp_nmpc_dms.h), built
on tests/nmpc_ref.py and tests/nmpc_stage_ref.py.  One instance at a time.

The states stay decision variables: the iterate is (X, z), X (N + 1, 4) absolute with x_0 pinned
to the measured state, z = [u - u_eq; theta].  At the iterate, per stage k < N

    f_k = dynamic(delta, x_k, u_k) (nmpc_ref.rk4_jac: the operations of nm_rk4<true>),
    A_k, B_k its Jacobians at (x_k, u_k),  defect c_k = f_k - x_{k+1},

and the sub-problem is the stage QP of tests/nmpc_stage_ref.py with

    dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k du_k + c_k,

w_k, the bounds and hp formed from the iterate's own x_k; W, Fp and the bound map unchanged.  At
a consistent iterate (X the rollout of z) c = 0 and the sub-problem is the stage route's.

SQP: merit phi = J + nu (V + E), V = sum max(row, 0), E = sum_k |c_k|_1, nu <- max(nu, 1.1 max(max
lam, max |pi|)) within a solve; D = sum_k w_k'v_k - nu (V0 + E0) (the gradient along the step is a
stage sum); the first alpha = 2^-t (t = 0..7) with phi(y + alpha dy) <= phi(y) + 1e-4 alpha D, a
non-finite trial rejected, else alpha = 2^-7.  Stopping as nmpc_ref.sqp with the step over
(dX, dz), feasibility max(rows) <= 1e-9 and max |c_k| <= 1e-9, and the stationarity the full-space
residual of the Lagrangian of bqp_ocp_duals (bqp.h),

    cost + sum_k pi_k'(A_k x_k + B_k u_k + c_k - x_{k+1}) + lam'rows,

at the iterate (step zero) against 10 tol (1 + |grad J|):
    x_k (1 <= k <= N): w_k[x] + A_k'pi_k (k < N) - pi_{k-1} + F_x'lam_k (+ F_T[:, :4]'lam_T, k = N)
    u_k (k < N):       w_k[u] + B_k'pi_k + F_u'lam_{k+1}
    theta:             sum_k w_k[theta] + F_T[:, 4]'lam_T
Flags: 1 converged, 0 iteration limit, -2 sub-problem infeasible, -8 numerical failure.
"""
import numpy as np

import nmpc_ref as R
import nmpc_stage_ref as SR
from oracle import dense_qp


_dense_solve = dense_qp.solve


def qp_solve(qp, **kw):
    """oracle.dense_qp.solve; a sub-problem on which its linear solve is singular (a degenerate
    vertex) returns nan, which sends nmpc_ref.sqp and sqp below to the exact active-set solver"""
    try:
        return _dense_solve(qp, **kw)
    except np.linalg.LinAlgError:
        return np.full(1, np.nan), np.nan, dict(ineqlin=np.full(1, np.nan)), None


def consistent(p, x0, z):
    """X = the rollout of z by the operations of the linearisation (c = 0 exactly there)"""
    return R.rollout(p, x0, z, jac=True)[0]


def flat(p, x0):
    """x_k = x0 for every k"""
    return np.tile(np.asarray(x0, float), (p['N'] + 1, 1))


def interpolated(p, x0):
    """x_k from x0 to x_eq, linearly"""
    s = np.linspace(0.0, 1.0, p['N'] + 1)[:, None]
    return (1.0 - s) * np.asarray(x0, float) + s * p['x_eq']


def steps(p, X, z):
    """f (N, 4), A (N, 4, 4), B (N, 4) at the iterate's own (x_k, u_k)"""
    N = p['N']
    f = np.zeros((N, 4)); A = np.zeros((N, 4, 4)); B = np.zeros((N, 4))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for k in range(N):
            f[k], A[k], B[k] = R.rk4_jac(p['delta'], X[k], z[k] + p['u_eq'])
    return f, A, B


def dms_problem(p, x0, X, z):
    """the sub-problem at (X, z): nmpc_stage_ref.stage_problem's dict at the iterate's own states,
    with c (N, 4) and the values at the iterate: cost J, rows (m), X with x_0 = x0"""
    X = np.array(X, float)
    X[0] = x0
    f, A, B = steps(p, X, z)
    sp = SR.stage_problem(p, x0, z, lin=dict(X=X, A=A, B=B))
    e = R.residuals(p, X, z)
    sp.update(c=f - X[1:], X=X, cost=float(e @ e), rows=R.constraints(p, X, z))
    return sp


def propagate(p, sp):
    """S (N + 1, 4, n) and g (N + 1, 4): dx_k = S_k d + g_k with the defects propagated"""
    N = p['N']
    S = np.zeros((N + 1, 4, N + 1)); g = np.zeros((N + 1, 4))
    for k in range(N):
        S[k + 1] = sp['A'][k] @ S[k]
        S[k + 1][:, k] += sp['B'][k]
        g[k + 1] = sp['A'][k] @ g[k] + sp['c'][k]
    return S, g


def condense(p, sp):
    """the sub-problem condensed over d = [du; dtheta] through dx_k = S_k d + g_k: H, f, C, c in the
    NMPC row order (nmpc_stage_ref.condense's, with the defects' share in f and c), and S, g"""
    N = p['N']
    D = SR.condense(p, sp)                     # the c = 0 problem: H, C are those
    S, g = propagate(p, sp)
    W = sp['W']
    M = np.zeros((N + 1, 6, N + 1))
    for k in range(N + 1):
        M[k, :4] = S[k]
        if k < N:
            M[k, 4, k] = 1.0
        M[k, 5, N] = 1.0
    f = D['f'] + np.einsum('kai,kab,kb->i', M[:, :, :], W[:, :, :4], g)
    rows, _ = SR.bound_map(p['F_x'], p['F_u'])
    mx, ms = p['F_x'].shape[0], len(rows)
    c = D['c'].copy()
    for k in range(1, N + 1):
        for i, (var, side, a) in enumerate(rows[:mx]):
            c[ms * (k - 1) + i] += (1.0 if side else -1.0) * a * g[k][var]
    c[ms * N:] += sp['Fp'][:, :4] @ g[N]
    return dict(H=D['H'], f=f, C=D['C'], c=c, S=S, g=g)


def dense_direct(p, sp, z):
    """the same dense QP assembled without the stage form: the weighted residuals e (X, z) and the
    rows, linear in (X, z), with dX = S d + g put in: H = 2 Jr'Jr, f = 2 Jr'(e + Jx g),
    rows C d <= -(c + F g)"""
    N = p['N']
    S, g = propagate(p, sp)
    X = sp['X']
    e, Jr = R.residuals(p, X, z, S)
    c, C = R.constraints(p, X, z, S)
    Lq, _, Lp, _ = R._factors(p)
    eg = e.copy()
    for k in range(N):
        eg[5 * k:5 * k + 4] += Lq @ g[k]
    eg[5 * N:5 * N + 4] += Lp @ g[N]
    mx, mu = p['F_x'].shape[0], p['F_u'].shape[0]
    ms = mx + mu
    c = c.copy()
    for k in range(1, N + 1):
        c[ms * (k - 1):ms * (k - 1) + mx] += p['F_x'] @ g[k]
    c[ms * N:] += p['F_T'][:, :4] @ g[N]
    return dict(H=2.0 * Jr.T @ Jr, f=2.0 * Jr.T @ eg, C=C, c=c)


def multipliers_x(p, lam):
    """per stage k = 0..N the rows' share of the x and u stationarity: (F_x'lam_k (+ F_T[:, :4]'
    lam_T at N), F_u'lam_{k+1}), and the theta share F_T[:, 4]'lam_T"""
    N = p['N']
    mx, mu = p['F_x'].shape[0], p['F_u'].shape[0]
    ms = mx + mu
    xs = np.zeros((N + 1, 4)); us = np.zeros(N)
    for k in range(1, N + 1):
        lk = lam[ms * (k - 1):ms * k]
        xs[k] = p['F_x'].T @ lk[:mx]
        us[k - 1] = p['F_u'][:, 0] @ lk[mx:]
    lT = lam[ms * N:]
    xs[N] += p['F_T'][:, :4].T @ lT
    return xs, us, float(p['F_T'][:, 4] @ lT)


def pi_of(p, sp, v, lam):
    """the dynamics multipliers of the sub-problem's solution v (N + 1, 6) with row multipliers
    lam, from its stationarity in dx_k backwards: pi_{k-1} = (W_k v_k + w_k)[x] + A_k'pi_k + rows"""
    N = p['N']
    xs, _, _ = multipliers_x(p, lam)
    pi = np.zeros((N, 4))
    for k in range(N, 0, -1):
        q = (sp['W'][k] @ v[k] + sp['w'][k])[:4] + xs[k]
        if k < N:
            q = q + sp['A'][k].T @ pi[k]
        pi[k - 1] = q
    return pi


def stationarity(p, sp, lam, pi):
    """the full-space residual at the iterate (step zero): (max |residual|, |grad J|_inf)"""
    N = p['N']
    xs, us, ths = multipliers_x(p, lam)
    w = sp['w']
    r = []
    for k in range(1, N + 1):
        q = w[k][:4] + xs[k] - pi[k - 1]
        if k < N:
            q = q + sp['A'][k].T @ pi[k]
        r.append(q)
    ru = np.array([w[k][4] + sp['B'][k] @ pi[k] + us[k] for k in range(N)])
    rt = w[:, 5].sum() + ths
    res = max(np.abs(np.concatenate(r)).max(), np.abs(ru).max(), abs(rt))
    grad = max(np.abs(w[1:, :4]).max(), np.abs(w[:N, 4]).max(), abs(w[:, 5].sum()))
    return res, grad


def trial(p, x0, X, z):
    """cost, row violation V and defect norm E at (X, z); nan if anything is not finite"""
    X = np.array(X, float)
    X[0] = x0
    f, _, _ = steps(p, X, z)
    if not (np.all(np.isfinite(f)) and np.all(np.isfinite(X))):
        return np.nan, np.nan, np.nan
    e = R.residuals(p, X, z)
    c = R.constraints(p, X, z)
    return float(e @ e), float(np.maximum(c, 0.0).sum()), float(np.abs(f - X[1:]).sum())


def sqp(p, x0, z0=None, X0=None, max_iter=100, tol=1e-8, trace=None):
    """the SQP of the module doc from (X0, z0); X0 None: the rollout of z0.  Returns X, z, lam, pi,
    info(exitflag, iterations, cost, stat)."""
    N = p['N']
    n = N + 1
    m = R.rows(p)
    z = np.zeros(n) if z0 is None else np.array(z0, float)
    with np.errstate(invalid='ignore', over='ignore'):
        X = consistent(p, x0, z) if X0 is None else np.array(X0, float)
    X[0] = x0
    lam = np.zeros(m); pi = np.zeros((N, 4))
    nu, cprev = 0.0, np.inf
    flag, it, stat, J = 0, 0, np.inf, np.nan
    while True:
        sp = dms_problem(p, x0, X, z)
        J, rows, c = sp['cost'], sp['rows'], sp['c']
        if not (np.all(np.isfinite(sp['A'])) and np.all(np.isfinite(c)) and np.isfinite(J)):
            flag = -8
            break
        D = condense(p, sp)
        qp = dict(H=D['H'], f=D['f'], A=D['C'], b=-D['c'], Aeq=np.zeros((0, n)), beq=np.zeros(0),
                  lb=np.full(n, -np.inf), ub=np.full(n, np.inf))
        d, _, lamq, _ = qp_solve(qp)
        lam = lamq['ineqlin']
        if not (np.all(np.isfinite(d)) and np.all(np.isfinite(lam))):
            from oracle import exact_qp
            r = exact_qp.solve(D['H'], D['f'], D['C'], -D['c'])
            if r['z'] is None:
                flag = -2
                break
            d, lam = r['z'], r['lam']
        if not np.all(np.isfinite(d)):
            flag = -8
            break
        if (D['C'] @ d + D['c']).max() > 1e-7 * (1.0 + np.abs(D['c']).max()):
            flag = -2
            break
        dX = np.einsum('kij,j->ki', D['S'], d) + D['g']
        v = np.zeros((N + 1, 6))
        v[:, :4] = dX; v[:N, 4] = d[:N]; v[:, 5] = d[N]
        pi = pi_of(p, sp, v, lam)
        stat, gn = stationarity(p, sp, lam, pi)
        dn = max(np.abs(d).max(), np.abs(dX).max())
        zn = np.abs(z).max()
        feas0 = rows.max() <= 1e-9 and np.abs(c).max() <= 1e-9
        if trace is not None:
            trace.append(dict(it=it, J=J, step=dn, stat=stat, viol=rows.max(), defect=np.abs(c).max()))
        if feas0 and ((dn <= tol * (1 + zn) and stat <= 10.0 * tol * (1 + gn)) or
                      (it > 0 and dn <= 1e-6 * (1 + zn) and abs(cprev - J) <= 1e-12 * (1 + abs(J)))):
            flag = 1
            break
        VE0 = np.maximum(rows, 0.0).sum() + np.abs(c).sum()
        nu = max(nu, 1.1 * max(lam.max(initial=0.0), np.abs(pi).max()))
        Dd = float((sp['w'] * v).sum()) - nu * VE0
        phi0 = J + nu * VE0
        tsel = 7
        for t in range(8):
            a = 0.5 ** t
            Jt, Vt, Et = trial(p, x0, X + a * dX, z + a * d)
            if np.isfinite(Jt) and np.isfinite(Vt + Et) and Jt + nu * (Vt + Et) <= phi0 + 1e-4 * a * Dd:
                tsel = t
                break
        a = 0.5 ** tsel
        Js = trial(p, x0, X + a * dX, z + a * d)[0]
        if not np.isfinite(Js):
            flag = -8
            break
        X = X + a * dX
        X[0] = x0
        z = z + a * d
        cprev = J
        it += 1
        if it >= max_iter:
            flag = 0
            J = Js
            break
    return X, z, lam, pi, dict(exitflag=flag, iterations=it, cost=J, stat=stat)


def kkt(p, x0, X, z, lam, pi):
    """the full-space KKT residuals at (X, z, lam, pi) by this restatement's model: stat, grad,
    cmax (rows), dmax (defects), lam_min"""
    sp = dms_problem(p, x0, X, z)
    st, gn = stationarity(p, sp, np.asarray(lam, float), np.asarray(pi, float).reshape(p['N'], 4))
    return dict(stat=st, grad=gn, cmax=sp['rows'].max(), dmax=np.abs(sp['c']).max(),
                lam_min=np.min(lam, initial=0.0))


def warm_start(p, X, z, x_new):
    """the closed loop's warm start: z shifted with the last move repeated, x_k <- x_{k+1}, x_0 the
    new measured state, x_N <- dynamic(delta, x_N, u_{N-1})"""
    N = p['N']
    zs = np.concatenate([z[1:N], z[N - 1:N], z[N:]])
    Xs = np.vstack([X[1:], R.rk4_jac(p['delta'], X[N], z[N - 1] + p['u_eq'])[0][None]])
    Xs[0] = x_new
    return Xs, zs
