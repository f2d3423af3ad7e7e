"""Structured batched OCP solve (bqp_solve_ocp_batched) — the fast path.

``OcpProblem`` holds one stage-wise problem description (shared by the whole batch unless a
per-instance array is given); ``solve_ocp`` solves a batch of instances that differ in x0 (and
optionally the linear terms w, the polytope right-hand side hp, or the model A/B).

Dimensions without a compiled structured kernel ((nx, nu, np) other than the MG (4, 1, 1) and
DI (2, 2, 2) families, or N + 1 > 128) take the condensed route: the states are eliminated on
the host once per problem (bqp.condense) and the batch runs through bqp_quadprog_batched, the
dense GPU kernels — same iterate semantics (exit flags, iterations), no CPU solve.
"""
import ctypes as C

import numpy as np

from . import _lib


class OcpProblem:
    """x_{k+1} = A x_k + B u_k + c; cost sum 0.5 v'W_k v + w_k'v, v = [x; u; theta];
    box bounds on x_k (k>=1), u_k; polytope Fp [x_kp; u_kp; theta] <= hp.

    Arrays use natural numpy shapes (row-major): W (N+1, nv, nv), w (N+1, nv),
    xlb/xub (N+1, nx), ulb/uub (N, nu), Fp (mp, nv), hp (mp,).

    xs_lin, xs_quad (N+1, nx), weights >= 0: soft state bounds (bqp_ocp_data.xs_lin / xs_quad) -
    xlb - s_l <= x <= xub + s_u with the penalty l1 s + 0.5 l2 s^2 on every slack; a variable whose
    weights are both 0 keeps hard bounds.  Structured kernel only, fp64, no polish."""

    def __init__(self, A, B, W, N, np_, w=None, c=None, xlb=None, xub=None, ulb=None, uub=None,
                 Fp=None, hp=None, poly_stage=None, const=0.0, xs_lin=None, xs_quad=None):
        self.A = np.asarray(A, float)
        self.B = np.asarray(B, float)
        self.nx, self.nu = self.B.shape
        self.np = int(np_)
        self.N = int(N)
        nv = self.nx + self.nu + self.np
        self.nv = nv
        self.W = np.asarray(W, float).reshape(self.N + 1, nv, nv)
        self.w = np.zeros((self.N + 1, nv)) if w is None else np.asarray(w, float).reshape(self.N + 1, nv)
        self.c = np.zeros(self.nx) if c is None else np.asarray(c, float)
        inf = np.inf
        self.xlb = np.full((self.N + 1, self.nx), -inf) if xlb is None else np.asarray(xlb, float)
        self.xub = np.full((self.N + 1, self.nx), inf) if xub is None else np.asarray(xub, float)
        self.ulb = np.full((self.N, self.nu), -inf) if ulb is None else np.asarray(ulb, float)
        self.uub = np.full((self.N, self.nu), inf) if uub is None else np.asarray(uub, float)
        self.Fp = np.zeros((0, nv)) if Fp is None else np.asarray(Fp, float).reshape(-1, nv)
        self.hp = np.zeros(0) if hp is None else np.asarray(hp, float).ravel()
        self.poly_stage = self.N if poly_stage is None else int(poly_stage)
        self.const = const
        self.xs_lin = None if xs_lin is None else np.asarray(xs_lin, float).reshape(self.N + 1, self.nx)
        self.xs_quad = None if xs_quad is None else np.asarray(xs_quad, float).reshape(self.N + 1, self.nx)

    @property
    def soft(self):
        return self.xs_lin is not None or self.xs_quad is not None

    @property
    def mp(self):
        return self.Fp.shape[0]


def _cm(a):
    """Column-major flattening of the trailing two axes (MATLAB layout)."""
    return np.ascontiguousarray(np.swapaxes(a, -1, -2), dtype=np.float64)


class OcpResult(dict):
    __getattr__ = dict.__getitem__


def _stage_models(prob, batch, A, B, c, stage_models):
    """True when A / B / c are per-stage schedules: (N, nx, nx) / (N, nx, nu) / (N, nx) shared by
    the batch, or (batch, N, ...) per instance - beside (nx, nx) and (batch, nx, nx) for one model
    per horizon.  A three-dimensional A (two-dimensional c) is a schedule when its first axis is
    N and not batch.  With batch == N the two readings coincide: the array is then one model per
    instance, as it was before schedules existed, and a schedule shared by the batch is asked
    for with stage_models=True."""
    if stage_models is not None:
        return bool(stage_models)
    sched = None
    for a, base in ((A, 2), (B, 2), (c, 1)):
        if a is None:
            continue
        nd = np.ndim(a)
        if nd == base + 2:
            return True
        if nd == base + 1:
            n0 = np.shape(a)[0]
            this = n0 == prob.N and n0 != batch
            if sched is not None and sched != this:
                raise ValueError('A, B and c must all be schedules or all single models')
            sched = this
    return bool(sched)


def pack(prob, x0, w=None, hp=None, A=None, B=None, Fp=None, W=None, c=None, stage_models=None,
         skip=None, xs_lin=None, xs_quad=None):
    """Builds (dims, data, keepalive) for a batch.  x0: (batch, nx); per-instance overrides
    w (batch, N+1, nv), hp (batch, mp), A (batch, nx, nx), B (batch, nx, nu), c (batch, nx) and the
    polytope Fp (batch, mp, nv) (same row count and stage as prob's) and the stage costs W (batch,
    N+1, nv, nv).  Per-stage models (bqp_ocp_dims.stage_models = 1): A (N, nx, nx), B (N, nx, nu),
    c (N, nx) as one schedule for the batch, or (batch, N, ...) per instance; what is not given is
    prob's model repeated over the stages.  skip (batch,) ints: with per-stage models, instances
    that are not solved.  xs_lin, xs_quad (batch, N+1, nx): per-instance soft-bound weights
    in place of prob's (what is not given is prob's, or zeros)."""
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    batch = x0.shape[0]
    keep = [x0]

    def arr(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        keep.append(a)
        return a

    nx, nu, nv, N, mp = prob.nx, prob.nu, prob.nv, prob.N, prob.mp
    stg = _stage_models(prob, batch, A, B, c, stage_models)
    if stg:
        def sched(a, base, shape):
            # (N, *shape) shared or (batch, N, *shape) per instance; a single model is repeated
            a = np.asarray(base if a is None else a, float)
            if a.ndim == len(shape):
                a = np.broadcast_to(a, (N,) + shape)
            if a.shape not in ((N,) + shape, (batch, N) + shape):
                raise ValueError('per-stage model of shape %r, expected %r or %r'
                                 % (a.shape, (N,) + shape, (batch, N) + shape))
            return a, (0 if a.ndim == len(shape) + 1 else N * int(np.prod(shape)))
        Am, sA = sched(A, prob.A, (nx, nx))
        Bm, sB = sched(B, prob.B, (nx, nu))
        cm, sc = sched(c, prob.c, (nx,))
        Aa, Ba, ca = arr(_cm(Am)), arr(_cm(Bm)), arr(cm)
    else:
        Aa = arr(_cm(prob.A if A is None else A))
        Ba = arr(_cm(prob.B if B is None else B))
        ca = arr(prob.c if c is None else c)
        sA = 0 if A is None else nx * nx
        sB = 0 if B is None else nx * nu
        sc = 0 if c is None or np.ndim(c) == 1 else nx
    Wa = arr(_cm(prob.W if W is None else W))
    wa = arr(prob.w if w is None else w)
    Fa = arr(_cm(prob.Fp if Fp is None else Fp)) if mp else None
    ha = arr(prob.hp if hp is None else hp) if mp else None
    xlb, xub, ulb, uub = arr(prob.xlb), arr(prob.xub), arr(prob.ulb), arr(prob.uub)
    sk = None
    if skip is not None:
        sk = np.ascontiguousarray(skip, dtype=np.int32)
        if sk.shape != (batch,):
            raise ValueError('skip must have one entry per instance')
        keep.append(sk)
    # soft state bounds: prob's weights shared by the batch, or per-instance overrides
    xl = getattr(prob, 'xs_lin', None) if xs_lin is None else xs_lin
    xq = getattr(prob, 'xs_quad', None) if xs_quad is None else xs_quad
    sxs = 0
    if xl is not None or xq is not None:
        per = any(a is not None and np.ndim(a) == 3 for a in (xl, xq))

        def wts(a):
            if a is None:
                return None
            a = np.asarray(a, float)
            if a.shape not in ((N + 1, nx), (batch, N + 1, nx)):
                raise ValueError('soft-bound weights of shape %r, expected %r or %r'
                                 % (a.shape, (N + 1, nx), (batch, N + 1, nx)))
            return arr(np.broadcast_to(a, (batch, N + 1, nx)) if per else a)
        xl, xq = wts(xl), wts(xq)
        sxs = (N + 1) * nx if per else 0
    dims = _lib.OcpDims(nx, nu, prob.np, N, mp, prob.poly_stage, 1 if stg else 0)
    data = _lib.OcpData(
        A=_lib.ptr(Aa), B=_lib.ptr(Ba), c=_lib.ptr(ca), W=_lib.ptr(Wa), w=_lib.ptr(wa),
        xlb=_lib.ptr(xlb), xub=_lib.ptr(xub), ulb=_lib.ptr(ulb), uub=_lib.ptr(uub),
        Fp=_lib.ptr(Fa), hp=_lib.ptr(ha), x0=_lib.ptr(x0),
        sA=sA, sB=sB, sc=sc,
        sW=0 if W is None else (N + 1) * nv * nv,
        sw=0 if w is None else (N + 1) * nv, sxb=0, sub=0, sFp=0 if Fp is None else mp * nv,
        shp=0 if hp is None else mp, sx0=nx, skip=_lib.iptr(sk) if sk is not None else None,
        xs_lin=_lib.ptr(xl), xs_quad=_lib.ptr(xq), sxs=sxs)
    return dims, data, batch, keep


def solve_ocp(prob, x0, w=None, hp=None, A=None, B=None, handle=None, want_duals=False, Fp=None,
              W=None, route='auto', c=None, stage_models=None, skip=None, xs_lin=None, xs_quad=None,
              **opts):
    """Solve a batch on the GPU.  Returns OcpResult(x (b,N+1,nx), u (b,N,nu), theta (b,np),
    fval, exitflag, iterations, firstorderopt, constrviolation, mu[, pi, lam_x, lam_u, lam_p, s_x]).
    xs_lin, xs_quad: per-instance soft-bound weights (batch, N+1, nx) in place of prob's; a soft
    problem runs on the structured kernel only (the condensed route raises ValueError), and s_x
    (b, N+1, 2, nx) [lower, upper] holds the slacks of the softened rows.
    A, B, c: one model (nx, nx) / (batch, nx, nx), or per-stage models (linear time-varying)
    (N, nx, nx) / (batch, N, nx, nx) - see pack; per-stage models run on the structured kernel
    only, in fp64.  skip: with per-stage models, instances left unsolved
    (their rows of the result keep the zeros they are created with).
    route: 'auto' (structured kernel; condensed when the C ABI reports the dimensions
    unsupported), 'structured' (no condensed route) or 'condensed'."""
    if route not in ('auto', 'structured', 'condensed'):
        raise ValueError("route must be 'auto', 'structured' or 'condensed', not %r" % (route,))
    lib = _lib.load()
    h = handle or _default_handle()
    dims, data, batch, keep = pack(prob, x0, w, hp, A, B, Fp, W, c, stage_models, skip, xs_lin, xs_quad)
    soft = bool(data.xs_lin) or bool(data.xs_quad)
    N, nx, nu, npar, mp = prob.N, prob.nx, prob.nu, prob.np, prob.mp
    x = np.zeros((batch, N + 1, nx)); u = np.zeros((batch, N, nu)); th = np.zeros((batch, npar))
    fval = np.zeros(batch); flag = np.zeros(batch, np.int32)
    out = (_lib.Output * batch)()
    duals = None
    dd = {}
    if want_duals:
        dd = dict(pi=np.zeros((batch, N, nx)), lam_x=np.zeros((batch, N + 1, 2, nx)),
                  lam_u=np.zeros((batch, N, 2, nu)), lam_p=np.zeros((batch, max(mp, 1))))
        duals = _lib.OcpDuals(*(_lib.ptr(dd[k]) for k in ('pi', 'lam_x', 'lam_u', 'lam_p')))
        if soft:
            dd['s_x'] = np.zeros((batch, N + 1, 2, nx))
            duals.s_x = _lib.ptr(dd['s_x'])
    if route == 'condensed':
        if soft:
            raise ValueError('condensed route: soft state bounds run on the structured kernel only')
        if c is not None or dims.stage_models:
            raise ValueError('condensed route: only x0 and hp may vary per instance')
        return solve_ocp_condensed(prob, x0, w, hp, A, B, handle, want_duals, Fp, W, **opts)
    o = _lib.options(**opts)
    rc = lib.bqp_solve_ocp_batched(h.value, C.byref(dims), batch, C.byref(data), C.byref(o),
                                   _lib.ptr(x), _lib.ptr(u), _lib.ptr(th), _lib.ptr(fval),
                                   _lib.iptr(flag), out, C.byref(duals) if duals else None)
    # the condensed route takes only x0 and hp per instance: anything else keeps the structured
    # solver's own error (an LDS fit failure is not a reason to change the algorithm)
    condensable = all(v is None for v in (w, A, B, Fp, W, c)) and not want_duals and not soft
    if rc == _lib.BQP_E_UNSUPPORTED and route == 'auto' and condensable and \
            not _lib.ocp_dims_supported(prob.nx, prob.nu, prob.np, prob.N, prob.mp):
        return solve_ocp_condensed(prob, x0, w, hp, A, B, handle, want_duals, Fp, W, **opts)
    _lib.check(rc, 'bqp_solve_ocp_batched')
    res = OcpResult(x=x, u=u, theta=th, fval=fval + prob.const, exitflag=flag,
                    iterations=np.array([o_.iterations for o_ in out]),
                    firstorderopt=np.array([o_.firstorderopt for o_ in out]),
                    constrviolation=np.array([o_.constrviolation for o_ in out]),
                    mu=np.array([o_.mu for o_ in out]),
                    polished=np.array([o_.polished for o_ in out], dtype=np.int32))
    if want_duals:
        dd['lam_p'] = dd['lam_p'][:, :mp]
        res.update(dd)
    return res


_handles = {}


def _default_handle(device=-1):
    h = _handles.get(device)
    if h is None:
        h = _lib.Handle(device)
        _handles[device] = h
    return h


def condensed_rhs(prob, X0, hp=None):
    """per-instance (f, b) of the condensed QP (bqp.condense) for states X0 (batch, nx) and
    optional per-instance polytope right-hand sides hp (batch, mp); the polytope rows are the
    last mp rows of Condensed.A"""
    from .condense import Condensed
    cd = getattr(prob, '_condensed', None)
    if cd is None:
        cd = prob._condensed = Condensed(prob)
    f, b = cd.rhs(X0)
    if hp is not None and prob.mp:
        b = b.copy()
        b[:, -prob.mp:] += np.asarray(hp, float).reshape(len(b), prob.mp) - prob.hp
    return cd, f, b


def solve_ocp_condensed(prob, x0, w=None, hp=None, A=None, B=None, handle=None, want_duals=False,
                        Fp=None, W=None, **opts):
    """The condensed route of solve_ocp: one host condensing per problem, the batch on the dense
    GPU kernels (bqp_quadprog_batched), trajectories recovered through the dynamics.  Per-instance
    x0 and hp; the model, costs and polytope matrix are shared (they define the dense H and A)."""
    from .quadprog import quadprog
    if any(a is not None for a in (w, A, B, Fp, W)):
        raise ValueError('condensed route: only x0 and hp may vary per instance')
    if getattr(prob, 'soft', False):
        raise ValueError('condensed route: soft state bounds run on the structured kernel only')
    if want_duals:
        raise ValueError('condensed route: stage-wise multipliers are not returned '
                         '(bqp.quadprog gives the condensed rows\' multipliers)')
    X0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=np.float64)
    cd, f, b = condensed_rhs(prob, X0, hp)
    z, _, flag, out, _ = quadprog(cd.H, f, cd.A, b, options=opts or None,
                                  handle=handle or _default_handle())
    N, nx, nu = prob.N, prob.nx, prob.nu
    V = np.einsum('kaj,bj->bka', cd.S, z) + np.einsum('kax,bx->bka', cd.T, X0) + cd.const_e[None]
    Wc = prob.W.copy(); wc = prob.w.copy()
    Wc[N, nx:nx + nu, :] = 0.0; Wc[N, :, nx:nx + nu] = 0.0; wc[N, nx:nx + nu] = 0.0
    fval = 0.5 * np.einsum('bka,kac,bkc->b', V, Wc, V) + np.einsum('bka,ka->b', V, wc)
    return OcpResult(x=V[:, :, :nx], u=V[:, :N, nx:nx + nu], theta=z[:, N * nu:],
                     fval=fval + prob.const, exitflag=flag, iterations=out['iterations'],
                     firstorderopt=out['firstorderopt'], constrviolation=out['constrviolation'],
                     mu=np.full(len(X0), np.nan))
