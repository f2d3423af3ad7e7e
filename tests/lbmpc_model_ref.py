"""TEST INFRASTRUCTURE ONLY.

Restatement of what the learned-model SQP's kernels (csrc/bqp_lbmpc.hip) compute at a given z, in
plain numpy with every array created in a `dtype` argument: the same code runs in float64 and in
np.longdouble (80-bit, eps 1.08e-19, where the platform has it), so the error of the float64
evaluation is measured and not assumed (tests/test_gpu_lbmpc_model.py sets its bars from it).

* nw()            the Nadaraya-Watson sums with first and second derivatives over a 7-row window
                  [X; Y] or an 8-row window [X; Y; v] (casadiL2NW.m:14-28: the denominator is
                  lambda + sum_j v_j k_j, the numerator is not masked)
* model()         learned and nominal rollouts u = K x + v with forward sensitivities, the residual
                  blocks and their Jacobian rows in the kernel's row order (row_order()),
                  H_GN = 2 Jr'Jr, f = 2 Jr'er, and - exact - the costate recursion, the rows
                  Xi_k (Jr2) and W_k Xi_k (Tr2), and H_GN + sum_k Xi_k' W_k Xi_k WITHOUT the PSD
                  clip: the kernel shifts instead of clipping, so the counterpart in
                  oracle/lbmpc.py is newton_model(clip=False)
* pivots()        the pivot test of oracle/lbmpc.py pd_cholesky, with the smallest pivot ratio
* shift_index()   the grid index k of hess_shift (shift 1e-12 hd 4^k)

Inputs are float64 values (the kernel's own inputs: the weight factors Lq, Lr, Lp, Lt as the
host shim forms them); converting them to `dtype` is exact, so both precisions evaluate the same
function.  nx = 4, nu = 1, np = 1 (the kernel's only instantiation).
"""
import numpy as np

H_BW = 0.5
LAM_NW = 1e-3
NTRIAL = 8
SHIFT_KMAX = 20


def nw(xi, data, dtype=np.float64, order=1):
    """g (4,) [order 0]; g, dg (4, 3) [1]; g, dg, d2g (4, 3, 3) [2] at xi (3,).
    With c = 2/h^2, d_j = X_j - xi: dk_j = c k_j d_j, d2k_j = k_j (c^2 d_j d_j' - c I);
    g = Nn / D, dg = (dNn - g dD') / D, d2g_i = (d2Nn_i - g_i d2D - dg_i dD' - dD dg_i') / D."""
    W = np.asarray(data, dtype)
    X, Y = W[:3], W[3:7]
    v = W[7] if W.shape[0] == 8 else np.ones(W.shape[1], dtype)
    xi = np.asarray(xi, dtype)
    hinv2 = dtype(1) / (dtype(H_BW) * dtype(H_BW))
    d = X - xi[:, None]                                   # (3, q)
    k = np.exp(-(d * d).sum(0) * hinv2)                   # (q,)
    D = dtype(LAM_NW) + (k * v).sum()
    Nn = (Y * k[None, :]).sum(1)
    g = Nn / D
    if order == 0:
        return g
    c = dtype(2) * hinv2
    dk = c * k[None, :] * d                               # (3, q)
    dNn = (Y[:, None, :] * dk[None, :, :]).sum(2)         # (4, 3)
    dD = (dk * v[None, :]).sum(1)                         # (3,)
    dg = (dNn - g[:, None] * dD[None, :]) / D
    if order == 1:
        return g, dg
    ddk = (c * c) * k[None, None, :] * d[:, None, :] * d[None, :, :] \
        - c * k[None, None, :] * np.eye(3, dtype=dtype)[:, :, None]      # (3, 3, q)
    d2Nn = (Y[:, None, None, :] * ddk[None]).sum(3)       # (4, 3, 3)
    d2D = (ddk * v[None, None, :]).sum(2)                 # (3, 3)
    d2g = (d2Nn - g[:, None, None] * d2D[None] - dg[:, :, None] * dD[None, None, :]
           - dD[None, :, None] * dg[:, None, :]) / D
    return g, dg, d2g


def from_oracle(p):
    """the kernel's problem data from a problem of oracle/lbmpc.py (f3_problem, f4_problem,
    dms_problem): the upper-triangular weight factors as bqp/lbmpc.py forms them"""
    up = lambda M: np.ascontiguousarray(np.linalg.cholesky(np.atleast_2d(np.asarray(M, float))).T)
    assert p['nx'] == 4 and p['nu'] == 1 and p['np'] == 1
    return dict(N=p['N'], n_run=p['n_run'], term_learned=bool(p['term_learned']),
                A=np.asarray(p['A'], float), B=np.asarray(p['B'], float).reshape(4),
                K=np.asarray(p['K'], float).reshape(4), LAMBDA=np.asarray(p['LAMBDA'], float).reshape(4),
                PSI=float(np.ravel(p['PSI'])[0]), xs=np.asarray(p['xs'], float).reshape(4),
                Lq=up(p['w_run'] * np.atleast_2d(p['Q'])), Lr=up(p['w_run'] * np.atleast_2d(p['R'])),
                Lp=up(p['P']), Lt=up(p['T']), data=np.asarray(p['data'], float))


def row_order(N, n_run):
    """the kernel's residual rows as (block, stage, component): per running stage k < n_run the 4
    rows of Lq (x_k - LAMBDA th) then the row of Lr (u_k - PSI th); then the 4 rows of the
    terminal Lp (x_N - LAMBDA th); then the 4 rows of Lt (LAMBDA th - xs)"""
    rows = []
    for k in range(n_run):
        rows += [('x', k, i) for i in range(4)] + [('u', k, 0)]
    rows += [('P', N, i) for i in range(4)] + [('T', N, i) for i in range(4)]
    return rows


def model(P, x0, z, dtype=np.float64, jac=True, exact=False):
    """cost, er (nr,) and - jac - Jr (nr, n), H = 2 Jr'Jr, f = 2 Jr'er; exact: also Jr2, Tr2
    (3N, n) and Hx = H + sum_k Xi_k' W_k Xi_k (no clip, no shift)."""
    c = lambda a: np.asarray(a, dtype)
    N, n_run = P['N'], P['n_run']
    n = N + 1
    A, B, K, LAM, xs = c(P['A']), c(P['B']), c(P['K']), c(P['LAMBDA']), c(P['xs'])
    PSI = dtype(P['PSI'])
    Lq, Lr, Lp, Lt = c(P['Lq']), c(P['Lr'])[0, 0], c(P['Lp']), c(P['Lt'])
    z = c(z)
    th = z[N]
    Et = np.zeros(n, dtype); Et[N] = 1
    x = c(x0).copy(); xn = x.copy()
    S = np.zeros((4, n), dtype); SN = np.zeros((4, n), dtype)
    er, Jr = [], []
    st = []                      # exact: per stage dg, d2g, dphi/dx, Xi
    two = dtype(2)
    order = 2 if exact else (1 if jac else 0)
    for k in range(N):
        u = K @ x + z[k]
        un = K @ xn + z[k]
        if jac:
            U = K @ S; U[k] += 1
            UN = K @ SN; UN[k] += 1
        gx = np.zeros(4, dtype)
        if k < n_run:
            ex = Lq @ (x - LAM * th)
            eu = Lr * (u - PSI * th)
            er += [ex, np.array([eu], dtype)]
            if jac:
                Jr += [Lq @ (S - LAM[:, None] * Et[None, :]), (Lr * (U - PSI * Et))[None, :]]
            gx = two * (Lq.T @ ex) + K * (two * Lr * eu)
        r = nw(np.array([x[0], x[1], u], dtype), P['data'], dtype, order)
        g = r if order == 0 else r[0]
        x1 = A @ x + B * u + g
        xn = A @ xn + B * un
        if jac:
            dg = r[1]
            if exact:
                st.append((dg, r[2], gx, np.vstack([S[0], S[1], U])))
            Ak = A.copy(); Ak[:, :2] += dg[:, :2]
            S = Ak @ S + (B + dg[:, 2])[:, None] * U[None, :]
            SN = A @ SN + B[:, None] * UN[None, :]
        x = x1
    xT, ST = (x, S) if P['term_learned'] else (xn, SN)
    eT = Lp @ (xT - LAM * th)
    es = Lt @ (LAM * th - xs)
    er += [eT, es]
    er = np.concatenate(er)
    out = dict(cost=(er * er).sum(), er=er)
    if not jac:
        return out
    Jr += [Lp @ (ST - LAM[:, None] * Et[None, :]), Lt @ (LAM[:, None] * Et[None, :])]
    Jr = np.vstack(Jr)
    out.update(Jr=Jr, H=two * (Jr.T @ Jr), f=two * (Jr.T @ er))
    if not exact:
        return out
    pc = two * (Lp.T @ eT) if P['term_learned'] else np.zeros(4, dtype)
    Hx = out['H'].copy()
    J2 = np.zeros((3 * N, n), dtype); T2 = np.zeros((3 * N, n), dtype)
    for k in range(N - 1, -1, -1):
        dg, d2g, gx, Xi = st[k]
        Wk = (pc[:, None, None] * d2g).sum(0)             # symmetric 3 x 3
        J2[3 * k:3 * k + 3] = Xi
        T2[3 * k:3 * k + 3] = Wk @ Xi
        Hx += Xi.T @ (Wk @ Xi)
        Jx = A + (B + dg[:, 2])[:, None] * K[None, :]
        Jx[:, :2] += dg[:, :2]
        pc = gx + Jx.T @ pc
    out.update(Jr2=J2, Tr2=T2, Hx=dtype(0.5) * (Hx + Hx.T))
    return out


def pivots(H, dtype=np.float64, tol=None, rel=1e-10):
    """right-looking Cholesky of H (oracle/lbmpc.py pd_cholesky): (every pivot above tol, the
    smallest pivot met over hd); tol defaults to rel hd, hd = max|H_ii|"""
    Kx = np.array(H, dtype)
    n = Kx.shape[0]
    hd = np.abs(np.diag(Kx)).max()
    if tol is None:
        tol = dtype(rel) * hd
    low = dtype(np.inf)
    for j in range(n):
        d = Kx[j, j]
        low = min(low, d)
        if not d > tol:
            return False, low / hd
        Kx[j + 1:, j] /= np.sqrt(d)
        Kx[j + 1:, j + 1:] -= np.outer(Kx[j + 1:, j], Kx[j + 1:, j])
    return True, low / hd


def shift_value(hd, k, dtype=np.float64):
    return np.ldexp(dtype(1e-12) * dtype(hd), 2 * k)


def shift_index(H, dtype=np.float64, tol_scale=1.0):
    """oracle/lbmpc.py hess_shift as a grid index: None if H passes the pivot test unshifted, else
    the smallest k in 0..20 (bisection, as the kernel) with H + 1e-12 hd 4^k I passing it, 21 if
    none does.  tol_scale multiplies the pivot threshold 1e-10 hd."""
    Hd = np.asarray(H, dtype)
    n = Hd.shape[0]
    hd = np.abs(np.diag(Hd)).max()
    tol = dtype(1e-10) * hd * dtype(tol_scale)
    ok = lambda k: pivots(Hd + shift_value(hd, k, dtype) * np.eye(n, dtype=dtype), dtype, tol=tol)[0]
    if pivots(Hd, dtype, tol=tol)[0]:
        return None
    lo, hi = -1, SHIFT_KMAX
    if not ok(hi):
        return SHIFT_KMAX + 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            hi = mid
        else:
            lo = mid
    return hi
