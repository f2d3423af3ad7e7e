"""TEST INFRASTRUCTURE ONLY: numpy restatement of the stage form of the nonlinear MPC's
Gauss-Newton sub-problem (bqp_nmpc_dims.subproblem = 1; csrc/bqp_nmpc.hip, csrc/bqp_nmpc_stage.h),
built on tests/nmpc_ref.py.  One instance at a time.

At the iterate z = [u - u_eq; theta] with rollout X and stage Jacobians A_k, B_k the sub-problem
min 0.5 d'Hd + f'd s.t. C d <= -c of nmpc_ref.linearize is the condensed form of the stage problem
in v_k = [dx_k; du_k; dtheta] (nx = 4, nu = 1, np = 1):

    dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k du_k
    min  sum_{k=0}^{N} 0.5 v_k'W_k v_k + w_k'v_k          (the u block of stage N is not used)
    W_k = 2 (Mx'(delta Q) Mx + Mu'(delta R) Mu), k < N;   W_N = 2 (Mx'P Mx + Mt'T Mt)
    Mx = [I 0 -LAMBDA], Mu = [0 1 -PSI], Mt = [0 0 LAMBDA]
    w_k = 2 (Mx'(delta Q)(x_k - x_eq - LAMBDA th) + Mu'(delta R)(u_k - u_eq - PSI th)), k < N
    w_N = 2 Mx'P (x_N - x_eq - LAMBDA th) + 2 Mt'T LAMBDA th
    bounds on dx_k (k = 1..N) and du_k from the rows of F_x, F_u (each row one entry a:
        a v <= h is v <= h / a for a > 0 and v >= h / a for a < 0, at the iterate the bound
        (h - a (v - v_eq)) / |a| with the sign of the side)
    Fp [dx_N; du; dtheta] <= hp,  Fp = [F_T[:, :4] | 0 | F_T[:, 4]],  hp = h_T - F_T [x_N - x_eq; th]
"""
import numpy as np

import nmpc_ref as R


class NotBox(ValueError):
    """F_x or F_u has a row that is no bound"""


def bound_map(F_x, F_u):
    """per row of [F_x; F_u]: (variable 0..3 state / 4 input, side 0 lower / 1 upper, |entry|), and
    rowof[variable][side] = row or -1.  NotBox unless every row has exactly one finite non-zero
    entry and each (variable, side) at most one row (csrc/bqp_nmpc_stage.h nmpc_bound_map_build)"""
    F_x = np.asarray(F_x, float).reshape(-1, 4)
    F_u = np.asarray(F_u, float).reshape(-1)
    rows, rowof = [], -np.ones((5, 2), int)
    for i in range(F_x.shape[0] + F_u.shape[0]):
        if i < F_x.shape[0]:
            nz = np.flatnonzero(F_x[i] != 0.0)
            if len(nz) != 1:
                raise NotBox('row %d of F_x has %d entries' % (i, len(nz)))
            var, a = int(nz[0]), F_x[i, nz[0]]
        else:
            var, a = 4, F_u[i - F_x.shape[0]]
        if not (np.isfinite(a) and a != 0.0):
            raise NotBox('row %d: entry %r' % (i, a))
        side = 1 if a > 0 else 0
        if rowof[var, side] >= 0:
            raise NotBox('rows %d and %d bound the same side of variable %d' % (rowof[var, side], i, var))
        rowof[var, side] = i
        rows.append((var, side, abs(a)))
    return rows, rowof


def cost_blocks(p):
    """W (N + 1, 6, 6)"""
    N = p['N']
    lam, psi = p['LAMBDA'], p['PSI']
    Mx = np.hstack([np.eye(4), np.zeros((4, 1)), -lam[:, None]])
    Mu = np.array([[0.0, 0.0, 0.0, 0.0, 1.0, -psi]])
    Mt = np.hstack([np.zeros((4, 5)), lam[:, None]])
    dQ, dR = p['delta'] * p['Q'], p['delta'] * p['R']
    Wr = 2.0 * (Mx.T @ dQ @ Mx + Mu.T @ dR @ Mu)
    WN = 2.0 * (Mx.T @ p['P'] @ Mx + Mt.T @ p['T'] @ Mt)
    return np.concatenate([np.tile(Wr, (N, 1, 1)), WN[None]]), (Mx, Mu, Mt, dQ, dR)


def stage_problem(p, x0, z, lin=None):
    """dict(A (N, 4, 4), B (N, 4), W, w (N + 1, 6), xlb / xub (N + 1, 4), ulb / uub (N), Fp, hp) at
    z from the measured state x0; NotBox for general rows.  lin: nmpc_ref.linearize(p, x0, z)"""
    N = p['N']
    L = R.linearize(p, x0, z) if lin is None else lin
    X, th = L['X'], z[N]
    lam, psi = p['LAMBDA'], p['PSI']
    W, (Mx, Mu, Mt, dQ, dR) = cost_blocks(p)
    w = np.zeros((N + 1, 6))
    for k in range(N):
        w[k] = 2.0 * (Mx.T @ dQ @ (X[k] - p['x_eq'] - lam * th) +
                      (Mu.T @ dR @ np.array([z[k] - psi * th])))
    w[N] = 2.0 * Mx.T @ p['P'] @ (X[N] - p['x_eq'] - lam * th) + 2.0 * Mt.T @ p['T'] @ (lam * th)
    rows, _ = bound_map(p['F_x'], p['F_u'])
    mx = p['F_x'].shape[0]
    xlb = np.full((N + 1, 4), -np.inf); xub = np.full((N + 1, 4), np.inf)
    ulb = np.full(N, -np.inf); uub = np.full(N, np.inf)
    for k in range(1, N + 1):
        for i, (var, side, a) in enumerate(rows):
            if i < mx:
                rhs = p['h_x'][i] - p['F_x'][i] @ (X[k] - p['x_eq'])
                (xub if side else xlb)[k, var] = rhs / a if side else -(rhs / a)
            else:
                rhs = p['h_u'][i - mx] - p['F_u'][i - mx, 0] * z[k - 1]
                (uub if side else ulb)[k - 1] = rhs / a if side else -(rhs / a)
    FT = p['F_T']
    Fp = np.hstack([FT[:, :4], np.zeros((FT.shape[0], 1)), FT[:, 4:5]])
    hp = p['h_T'] - FT[:, :4] @ (X[N] - p['x_eq']) - FT[:, 4] * th
    return dict(A=L['A'], B=L['B'], W=W, w=w, xlb=xlb, xub=xub, ulb=ulb, uub=uub, Fp=Fp, hp=hp)


def condense(p, sp):
    """the stage problem condensed over d = [du; dtheta]: H, f, C, c with the rows in the NMPC
    order (per stage k = 1..N the rows of F_x then of F_u, then F_T), each bound written back as
    its row a v <= (bound) |a|"""
    N = p['N']
    n = N + 1
    A, B = sp['A'], sp['B']
    S = np.zeros((N + 1, 4, n))
    for k in range(N):
        S[k + 1] = A[k] @ S[k]
        S[k + 1][:, k] += B[k]
    M = np.zeros((N + 1, 6, n))
    for k in range(N + 1):
        M[k, :4] = S[k]
        if k < N:
            M[k, 4, k] = 1.0
        M[k, 5, N] = 1.0
    W, w = sp['W'].copy(), sp['w'].copy()
    W[N, 4, :] = 0.0; W[N, :, 4] = 0.0; w[N, 4] = 0.0
    H = np.einsum('kai,kab,kbj->ij', M, W, M)
    f = np.einsum('kai,ka->i', M, w)
    rows, _ = bound_map(p['F_x'], p['F_u'])
    mx, ms = p['F_x'].shape[0], len(rows)
    m = R.rows(p)
    C = np.zeros((m, n)); c = np.zeros(m)
    for k in range(1, N + 1):
        for i, (var, side, a) in enumerate(rows):
            r = ms * (k - 1) + i
            sgn = 1.0 if side else -1.0
            if i < mx:
                bnd = (sp['xub'] if side else sp['xlb'])[k, var]
                C[r] = sgn * a * S[k][var]
            else:
                bnd = (sp['uub'] if side else sp['ulb'])[k - 1]
                C[r, k - 1] = sgn * a
            c[r] = -(sgn * bnd * a)
    Fp = sp['Fp'].copy()
    Fp[:, 4] = 0.0
    C[ms * N:] = Fp @ M[N]
    c[ms * N:] = -sp['hp']
    return dict(H=0.5 * (H + H.T), f=f, C=C, c=c)


def adjoint(p, sp, lam=None):
    """one backward sweep over A_k, B_k: without lam the condensed gradient f from the w_k, with
    lam (NMPC row order) C'lam from the rows' multipliers.
        p_N = x part (+ F_x'lam_N + F_T[:, :4]'lam_T),  g_k = u part + B_k'p_{k+1} (+ F_u'lam),
        p_k = x part + A_k'p_{k+1} (+ F_x'lam_k),  theta entry = sum of theta parts (+ F_T[:, 4]'lam_T)"""
    N = p['N']
    mx, mu = p['F_x'].shape[0], p['F_u'].shape[0]
    ms = mx + mu
    g = np.zeros(N + 1)
    if lam is None:
        xs = sp['w'][:, :4]; us = sp['w'][:, 4]; g[N] = sp['w'][:, 5].sum()
    else:
        lam = np.asarray(lam, float)
        xs = np.zeros((N + 1, 4)); us = np.zeros(N + 1)
        for k in range(1, N + 1):
            lk = lam[ms * (k - 1):ms * k]
            xs[k] = p['F_x'].T @ lk[:mx]
            us[k - 1] = p['F_u'][:, 0] @ lk[mx:]
        lT = lam[ms * N:]
        xs[N] += p['F_T'][:, :4].T @ lT
        g[N] = p['F_T'][:, 4] @ lT
    pk = xs[N].copy()
    for k in range(N - 1, -1, -1):
        g[k] = us[k] + sp['B'][k] @ pk
        pk = xs[k] + sp['A'][k].T @ pk
    return g


def lam_rows(p, lam_x, lam_u, lam_p):
    """the structured solve's multipliers of one instance (lam_x (N + 1, 2, 4) [lower, upper],
    lam_u (N, 2), lam_p (mp,)) in NMPC row order: a row's multiplier is its bound's over |a|"""
    N = p['N']
    rows, _ = bound_map(p['F_x'], p['F_u'])
    mx = p['F_x'].shape[0]
    out = []
    for k in range(1, N + 1):
        for i, (var, side, a) in enumerate(rows):
            out.append((lam_x[k, side, var] if i < mx else lam_u[k - 1, side]) / a)
    return np.concatenate([np.array(out), np.asarray(lam_p, float)])


def stage_duals(p, lam):
    """the inverse of lam_rows: (lam_x, lam_u, lam_p) from multipliers in NMPC row order"""
    N = p['N']
    rows, _ = bound_map(p['F_x'], p['F_u'])
    mx, ms = p['F_x'].shape[0], len(rows)
    lam_x = np.zeros((N + 1, 2, 4)); lam_u = np.zeros((N, 2))
    for k in range(1, N + 1):
        for i, (var, side, a) in enumerate(rows):
            v = lam[ms * (k - 1) + i] * a
            if i < mx:
                lam_x[k, side, var] = v
            else:
                lam_u[k - 1, side] = v
    return lam_x, lam_u, np.array(lam[ms * N:], float)
