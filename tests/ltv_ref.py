"""Reference for the structured solve with per-stage models (bqp_ocp_dims.stage_models = 1):
the stage-wise problem with x_{k+1} = A_k x_k + B_k u_k + c_k condensed in numpy to the dense
form min 0.5 z'Hz + f'z s.t. Ain z <= b over z = [u_0..u_{N-1}; theta], and solved by the oracle's
exact active-set solver (oracle/exact_qp.solve).

Rows in the order of bqp.condense.Condensed (the project's condensed form of the one-model
problem): the finite state bounds of stages 1..N (per stage upper, then lower), the finite input
bounds of stages 0..N-1 (upper, lower), then the polytope rows.
"""
import numpy as np


def schedule(prob, A=None, B=None, c=None):
    """(N, nx, nx), (N, nx, nu), (N, nx) from schedules or single models (None: prob's)."""
    N, nx, nu = prob.N, prob.nx, prob.nu

    def sched(a, base, shape):
        a = np.asarray(base if a is None else a, float)
        if a.ndim == len(shape) + 1:
            assert a.shape == (N,) + shape, a.shape
            return a
        return np.broadcast_to(a.reshape(shape), (N,) + shape)

    return sched(A, prob.A, (nx, nx)), sched(B, prob.B, (nx, nu)), sched(c, prob.c, (nx,))


def condense(prob, x0, A=None, B=None, c=None, w=None, hp=None):
    """dict(H, f, A, b, S, s): x_k = S[k] z + s[k] along the per-stage models."""
    N, nx, nu, npar, nv = prob.N, prob.nx, prob.nu, prob.np, prob.nv
    A, B, c = schedule(prob, A, B, c)
    w = prob.w if w is None else np.asarray(w, float)
    hp = prob.hp if hp is None else np.asarray(hp, float)
    nz = N * nu + npar
    S = np.zeros((N + 1, nx, nz)); s = np.zeros((N + 1, nx))
    s[0] = x0
    for k in range(N):
        S[k + 1] = A[k] @ S[k]
        S[k + 1][:, k * nu:(k + 1) * nu] += B[k]
        s[k + 1] = A[k] @ s[k] + c[k]
    M = np.zeros((N + 1, nv, nz)); m = np.zeros((N + 1, nv))
    for k in range(N + 1):
        M[k, :nx] = S[k]; m[k, :nx] = s[k]
        if k < N:
            M[k, nx:nx + nu, k * nu:(k + 1) * nu] = np.eye(nu)
        M[k, nx + nu:, N * nu:] = np.eye(npar)
    W = prob.W.copy(); wl = w.copy()
    W[N, nx:nx + nu, :] = 0.0; W[N, :, nx:nx + nu] = 0.0; wl[N, nx:nx + nu] = 0.0
    H = np.einsum('kai,kab,kbj->ij', M, W, M)
    f = np.einsum('kai,kab,kb->i', M, W, m) + np.einsum('kai,ka->i', M, wl)
    rows, rhs = [], []
    for k in range(1, N + 1):
        up, lo = np.isfinite(prob.xub[k]), np.isfinite(prob.xlb[k])
        rows.append(S[k][up]); rhs.append(prob.xub[k][up] - s[k][up])
        rows.append(-S[k][lo]); rhs.append(s[k][lo] - prob.xlb[k][lo])
    for k in range(N):
        up, lo = np.isfinite(prob.uub[k]), np.isfinite(prob.ulb[k])
        Gu = M[k, nx:nx + nu]
        rows.append(Gu[up]); rhs.append(prob.uub[k][up])
        rows.append(-Gu[lo]); rhs.append(-prob.ulb[k][lo])
    if prob.mp:
        kp = prob.poly_stage
        Fp = prob.Fp.copy()
        if kp == N:
            Fp[:, nx:nx + nu] = 0.0
        rows.append(Fp @ M[kp]); rhs.append(hp - Fp @ m[kp])
    return dict(H=0.5 * (H + H.T), f=f, A=np.vstack(rows), b=np.concatenate(rhs), S=S, s=s)


def lam_rows(prob, lam_x, lam_u, lam_p):
    """The structured solve's multipliers of one instance (lam_x (N+1, 2, nx) [lower, upper],
    lam_u (N, 2, nu), lam_p (mp,)) in the row order of condense()."""
    N = prob.N
    out = []
    for k in range(1, N + 1):
        out += [lam_x[k, 1][np.isfinite(prob.xub[k])], lam_x[k, 0][np.isfinite(prob.xlb[k])]]
    for k in range(N):
        out += [lam_u[k, 1][np.isfinite(prob.uub[k])], lam_u[k, 0][np.isfinite(prob.ulb[k])]]
    if prob.mp:
        out.append(lam_p)
    return np.concatenate(out)


def solve(prob, x0, A=None, B=None, c=None, w=None, hp=None):
    """Exact optimum: dict(status, z, lam, u (N, nu), theta, x (N+1, nx), qp)."""
    from oracle import exact_qp
    qp = condense(prob, x0, A, B, c, w, hp)
    r = exact_qp.solve(qp['H'], qp['f'], qp['A'], qp['b'])
    out = dict(status=r['status'], qp=qp)
    if r['status'] == 'optimal':
        z = r['z']
        N, nu = prob.N, prob.nu
        out.update(z=z, lam=r['lam'], u=z[:N * nu].reshape(N, nu), theta=z[N * nu:],
                   x=np.einsum('kij,j->ki', qp['S'], z) + qp['s'])
    return out


def pi_from(prob, qp_x, u, theta, A, lam_x, lam_p, w=None):
    """Dynamics multipliers implied by stationarity in x_k, k = N..1 (the Lagrangian of
    include/bqp.h): pi_{k-1} = W_k(x rows) v_k + w_k(x) + A_k' pi_k + lam_xu_k - lam_xl_k
    + Fp(x cols)' lam_p [k = kp]; returns (N, nx) with pi[k-1] the multiplier of x_k."""
    N, nx, nu = prob.N, prob.nx, prob.nu
    w = prob.w if w is None else w
    pi = np.zeros((N + 1, nx))
    nxt = np.zeros(nx)
    for k in range(N, 0, -1):
        v = np.concatenate([qp_x[k], u[k] if k < N else np.zeros(nu), theta])
        Wk = prob.W[k].copy()
        if k == N:
            Wk[nx:nx + nu, :] = 0.0; Wk[:, nx:nx + nu] = 0.0
        g = Wk[:nx] @ v + w[k][:nx] + lam_x[k, 1] - lam_x[k, 0]
        if k < N:
            g = g + A[k].T @ nxt
        if prob.mp and k == prob.poly_stage:
            g = g + prob.Fp[:, :nx].T @ lam_p
        pi[k] = g
        nxt = g
    return pi[1:]
