"""Reference for the structured solve with soft state bounds (bqp_ocp_data.xs_lin / xs_quad): the
condensed problem of tests/ltv_ref.py with one slack column per softened row,

    min 0.5 z'Hz + f'z + sum_j (l1_j s_j + 0.5 l2_j s_j^2)
    s.t. A z - E s <= b,  -s <= 0        (E: one -1 per softened row, in that row)

over [z; s], solved by the oracle's exact active-set solver (oracle/exact_qp.solve).  A state row
(stage k, variable i, side) is softened when xs_lin[k, i] > 0 or xs_quad[k, i] > 0; the exact
solver needs a strictly convex problem, so every softened row must have xs_quad > 0.

Rows of the augmented problem: the rows of ltv_ref.condense (state bounds per stage upper then
lower, input bounds, polytope), then the ns rows -s <= 0.
"""
import numpy as np

import ltv_ref


def state_rows(prob):
    """(k, i, h) of the state-bound rows of ltv_ref.condense, in its order (h = 1 upper, 0 lower)."""
    tags = []
    for k in range(1, prob.N + 1):
        up, lo = np.isfinite(prob.xub[k]), np.isfinite(prob.xlb[k])
        tags += [(k, int(i), 1) for i in np.flatnonzero(up)] + [(k, int(i), 0) for i in np.flatnonzero(lo)]
    return tags


def augment(prob, x0, xs_lin, xs_quad, A=None, B=None, c=None, w=None, hp=None, strict=True):
    """dict(H, f, A, b, nz, soft, tags, qp): the problem over [z; s]; soft[t] is the condensed row
    of slack t.  strict=False admits xs_quad = 0 on a softened row (for kkt(); not for solve())."""
    qp = ltv_ref.condense(prob, x0, A, B, c, w, hp)
    xs_lin = np.zeros((prob.N + 1, prob.nx)) if xs_lin is None else np.asarray(xs_lin, float)
    xs_quad = np.zeros((prob.N + 1, prob.nx)) if xs_quad is None else np.asarray(xs_quad, float)
    tags = state_rows(prob)
    soft = [j for j, (k, i, h) in enumerate(tags) if xs_lin[k, i] > 0 or xs_quad[k, i] > 0]
    l1 = np.array([xs_lin[tags[j][0], tags[j][1]] for j in soft])
    l2 = np.array([xs_quad[tags[j][0], tags[j][1]] for j in soft])
    assert not strict or (l2 > 0).all(), 'the exact solver needs a quadratic weight on every softened row'
    ns, nz, m = len(soft), qp['H'].shape[0], qp['A'].shape[0]
    H = np.zeros((nz + ns, nz + ns)); H[:nz, :nz] = qp['H']; H[nz:, nz:] = np.diag(l2)
    f = np.concatenate([qp['f'], l1])
    Aa = np.zeros((m + ns, nz + ns)); Aa[:m, :nz] = qp['A']
    for t, j in enumerate(soft):
        Aa[j, nz + t] = -1.0
        Aa[m + t, nz + t] = -1.0
    b = np.concatenate([qp['b'], np.zeros(ns)])
    return dict(H=H, f=f, A=Aa, b=b, nz=nz, soft=soft, tags=tags, qp=qp, l1=l1, l2=l2)


def kkt(aug, zs, lam):
    """stationarity (relative as dual_map.f1_kkt), complementarity, min multiplier, max violation
    of the augmented problem at (zs, lam)."""
    H, f, A, b = aug['H'], aug['f'], aug['A'], aug['b']
    g = H @ zs + f + A.T @ lam
    sl = b - A @ zs
    return (np.abs(g).max() / (1 + np.abs(H @ zs + f).max()), np.abs(lam * sl).max(), lam.min(), -sl.min())


def solve(prob, x0, xs_lin, xs_quad, A=None, B=None, c=None, w=None, hp=None):
    """Exact optimum: dict(status, aug, zs, z, s, lam (condensed rows), nu (slack bounds), u, theta,
    x, s_x (N+1, 2, nx) [lower, upper], fval)."""
    from oracle import exact_qp
    aug = augment(prob, x0, xs_lin, xs_quad, A, B, c, w, hp)
    r = exact_qp.solve(aug['H'], aug['f'], aug['A'], aug['b'])
    out = dict(status=r['status'], aug=aug)
    if r['status'] == 'optimal':
        zs = r['z']
        nz, N, nu = aug['nz'], prob.N, prob.nu
        m = aug['qp']['A'].shape[0]
        z, s = zs[:nz], zs[nz:]
        s_x = np.zeros((N + 1, 2, prob.nx))
        for t, j in enumerate(aug['soft']):
            k, i, h = aug['tags'][j]
            s_x[k, h, i] = s[t]
        out.update(zs=zs, z=z, s=s, lam=r['lam'][:m], nu=r['lam'][m:], lam_all=r['lam'],
                   u=z[:N * nu].reshape(N, nu), theta=z[N * nu:],
                   x=np.einsum('kij,j->ki', aug['qp']['S'], z) + aug['qp']['s'], s_x=s_x,
                   fval=0.5 * zs @ aug['H'] @ zs + aug['f'] @ zs)
    return out


def slack_rows(aug, s_x):
    """The structured solve's s_x (N+1, 2, nx) of one instance in the slack order of augment()."""
    return np.array([s_x[aug['tags'][j][0], aug['tags'][j][2], aug['tags'][j][1]] for j in aug['soft']])
