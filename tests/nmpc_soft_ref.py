"""TEST INFRASTRUCTURE ONLY: numpy restatement of the nonlinear MPC with soft state rows
(bqp_nmpc_data.xs_lin / xs_quad) on tests/nmpc_ref.py's linearize, rollout, residuals and
constraints.  One instance at a time.

Weights l1_i, l2_i >= 0 per row i of F_x; a row with l1_i > 0 or l2_i > 0 is softened, the rows of
F_u and F_T never are.  With phi_i(s) = l1_i s + 0.5 l2_i s^2 the problem is

    min J(z) + sum_{k=1..N} sum_{i soft} phi_i(max(c_{k,i}(z), 0))   s.t.  c_hard(z) <= 0.

Algorithm: nmpc_ref.sqp's, with
  - the sub-problem over [d; s], one slack per softened row (as tests/soft_ref.augment builds it
    for the structured solve): H + diag(l2), [f; l1], rows C d - E s <= -c and -s <= 0, solved by
    oracle.exact_qp.solve (which needs l2 > 0 on every softened row); no solution is -2;
  - lam = the multipliers of the rows C d - E s <= -c (on a softened row: of the softened row);
  - the merit function J + P + nu V with P = sum phi_i(max(c, 0)) over the softened rows and
    V = sum max(c, 0) over the hard rows; nu <- max(nu, 1.1 max hard lam);
    D = f'd + P_lin - P(z) - nu V(z) with the model penalty P_lin = sum phi_i(s);
  - the stopping test on the hard rows' feasibility, the cost in it being J + P.
"""
import numpy as np

import nmpc_ref as R
from oracle import exact_qp


def weights(p, l1, l2):
    """(l1, l2) as arrays of mx entries from scalars or arrays"""
    mx = p['F_x'].shape[0]
    return (np.broadcast_to(np.asarray(l1, float), (mx,)).copy(),
            np.broadcast_to(np.asarray(l2, float), (mx,)).copy())


def soft_rows(p, l1, l2):
    """row indices (in c's order) of the softened rows, and their weights"""
    l1, l2 = weights(p, l1, l2)
    mx, mu, N = p['F_x'].shape[0], p['F_u'].shape[0], p['N']
    on = np.flatnonzero((l1 > 0) | (l2 > 0))
    idx = np.array([(mx + mu) * k + i for k in range(N) for i in on], int)
    return idx, np.tile(l1[on], N), np.tile(l2[on], N)


def phi(w1, w2, s):
    return float((w1 * s + 0.5 * w2 * s * s).sum())


def slack(p, x0, z, l1, l2):
    """(N, mx): max(c, 0) on the softened rows, 0 elsewhere"""
    l1, l2 = weights(p, l1, l2)
    mx, mu, N = p['F_x'].shape[0], p['F_u'].shape[0], p['N']
    c = R.constraints(p, R.rollout(p, x0, z), z)
    return np.maximum(c[:N * (mx + mu)].reshape(N, mx + mu)[:, :mx], 0.0) * ((l1 > 0) | (l2 > 0))


def penalty(p, x0, z, l1, l2):
    l1, l2 = weights(p, l1, l2)
    s = slack(p, x0, z, l1, l2)
    return float((l1 * s + 0.5 * l2 * s * s).sum())


def trial(p, x0, z, idx, w1, w2, hard):
    """J + P and the hard rows' V at z; (nan, nan) if the rollout is not finite"""
    X = R.rollout(p, x0, z)
    if not np.all(np.isfinite(X)):
        return np.nan, np.nan
    e = R.residuals(p, X, z)
    c = R.constraints(p, X, z)
    return float(e @ e) + phi(w1, w2, np.maximum(c[idx], 0.0)), float(np.maximum(c[hard], 0.0).sum())


def sqp(p, x0, l1, l2, z0=None, max_iter=100, tol=1e-8, trace=None):
    """Returns z, lam, info(exitflag, iterations, cost (J + penalty), stat, slack_max)."""
    N = p['N']
    n = N + 1
    m = R.rows(p)
    idx, w1, w2 = soft_rows(p, l1, l2)
    assert (w2 > 0).all(), 'the exact solver needs a quadratic weight on every softened row'
    ns = idx.size
    hard = np.setdiff1d(np.arange(m), idx)
    z = np.zeros(n) if z0 is None else np.array(z0, float)
    lam = np.zeros(m)
    tol_step, tol_stat = tol, 10.0 * tol
    nu = 0.0
    cprev = np.inf
    flag, it, stat = 0, 0, np.inf
    J0 = np.nan
    while True:
        L = R.linearize(p, x0, z)
        H, f, c, C = L['H'], L['f'], L['c'], L['C']
        if not (np.all(np.isfinite(H)) and np.all(np.isfinite(C))):
            flag = -8
            break
        P0 = phi(w1, w2, np.maximum(c[idx], 0.0))
        J0 = L['cost'] + P0
        Ha = np.zeros((n + ns, n + ns)); Ha[:n, :n] = H; Ha[n:, n:] = np.diag(w2)
        fa = np.concatenate([f, w1])
        Aa = np.zeros((m + ns, n + ns)); Aa[:m, :n] = C
        Aa[idx, n + np.arange(ns)] = -1.0
        Aa[m + np.arange(ns), n + np.arange(ns)] = -1.0
        ba = np.concatenate([-c, np.zeros(ns)])
        r = exact_qp.solve(Ha, fa, Aa, ba)
        if r['z'] is None:
            flag = -2                               # the hard linearised rows have no common point
            break
        d, s, lam = r['z'][:n], r['z'][n:], r['lam'][:m]
        if not np.all(np.isfinite(d)):
            flag = -8
            break
        stat = np.abs(f + C.T @ lam).max()
        dn, zn, fn = np.abs(d).max(), np.abs(z).max(), np.abs(f).max()
        feas0 = c[hard].max(initial=-np.inf) <= 1e-9
        if trace is not None:
            trace.append(dict(it=it, J=J0, step=dn, stat=stat, viol=c[hard].max(initial=-np.inf), smax=s.max(initial=0.0)))
        if feas0 and ((dn <= tol_step * (1 + zn) and stat <= tol_stat * (1 + fn)) or
                      (it > 0 and dn <= 1e-6 * (1 + zn) and abs(cprev - J0) <= 1e-12 * (1 + abs(J0)))):
            flag = 1
            break
        V0 = np.maximum(c[hard], 0.0).sum()
        nu = max(nu, 1.1 * lam[hard].max(initial=0.0))
        D = f @ d + phi(w1, w2, s) - P0 - nu * V0
        phi0 = J0 + nu * V0
        tsel = 7
        for t in range(8):
            a = 0.5 ** t
            Jt, Vt = trial(p, x0, z + a * d, idx, w1, w2, hard)
            if np.isfinite(Jt) and np.isfinite(Vt) and Jt + nu * Vt <= phi0 + 1e-4 * a * D:
                tsel = t
                break
        a = 0.5 ** tsel
        Js = trial(p, x0, z + a * d, idx, w1, w2, hard)[0]
        if not np.isfinite(Js):
            flag = -8
            break
        z = z + a * d
        cprev = J0
        it += 1
        if it >= max_iter:
            flag = 0
            J0 = Js
            break
    return z, lam, dict(exitflag=flag, iterations=it, cost=J0, stat=stat)


def kkt(p, x0, z, lam, l1, l2, ctol=1e-9):
    """KKT residuals of the penalised NLP at (z, lam): stat = |grad J + C'lam|_inf, grad = |grad J|_inf,
    cmax = max hard c, lam_min, and per softened row the distance of lam_i from the subdifferential
    of phi_i(max(c_i, 0)): {l1 + l2 c_i} where c_i > 0, [0, l1] at c_i = 0, {0} where c_i < 0 -
    soft_dist (their maximum) and soft_rel (the maximum relative to 1 + l1 + l2 max(c_i, 0)).  A row
    with |c_i| <= ctol (the solvers' feasibility tolerance) counts as at c_i = 0 with the interval
    [0, l1 + l2 max(c_i, 0)]."""
    L = R.linearize(p, x0, z)
    idx, w1, w2 = soft_rows(p, l1, l2)
    hard = np.setdiff1d(np.arange(lam.size), idx)
    c, li = L['c'][idx], lam[idx]
    top = w1 + w2 * np.maximum(c, 0.0)
    dist = np.where(c > ctol, np.abs(li - top),
                    np.where(c < -ctol, np.abs(li), np.maximum(np.maximum(-li, li - top), 0.0)))
    return dict(stat=np.abs(L['f'] + L['C'].T @ lam).max(), grad=np.abs(L['f']).max(),
                cmax=L['c'][hard].max(initial=-np.inf), lam_min=lam.min(initial=0.0),
                soft_dist=dist.max(initial=0.0), soft_rel=(dist / (1.0 + top)).max(initial=0.0),
                slack_max=np.maximum(c, 0.0).max(initial=0.0), soft_lam_max=li.max(initial=0.0))
