"""Nonlinear MPC on the true Moore-Greitzer model: the host-side mirror of the solve call of
``examples/DMS_tracking_NMPC_casadi.m:163-167`` (CasADi/IPOPT over ``y = [x_0..x_N; u; theta]``
with the RK4 dynamics as equality rows), mapped onto bqp_nmpc_solve_batched - a single-shooting
Gauss-Newton SQP with an L1 merit function on the GPU (csrc/bqp_nmpc.hip) - and its closed loop
(:153-207) onto bqp_closed_loop_nmpc.

The states are eliminated: the decision is ``z = [u - u_eq; theta]`` (n = N + 1).  The rows, and
the multipliers ``lam``, are in IPOPT's ``lam_g`` order with the dynamics rows removed: per stage
k = 1..N the rows of F_x then of F_u, then the terminal set.  ``functions/ocpNMPC.m`` (fmincon
around an ode23 rollout) is not covered.

With ``shooting='multiple'`` (stage route) the states are kept instead, as in the script: the
iterate is ``(X, z)``, the solve returns ``X`` and the multipliers ``pi`` of the dynamics rows, and
``lam`` with ``pi`` is ``lam_g`` (bqp_nmpc_dms_solve_batched, bqp_nmpc_dims.shooting in bqp.h).

This module only marshals data; everything iterative runs on the GPU.
"""
import ctypes as C

import numpy as np

from . import _lib
from .lbmpc import _upper_factor
from .loop import ClosedLoop, _set_plant_params
from .ocp import OcpResult, _default_handle

_BQP_PLANT_MG_RK4 = 1
_SUBPROBLEM = {'dense': 0, 'stage': 1}


def _subproblem(name):
    if name not in _SUBPROBLEM:
        raise ValueError("subproblem is 'dense' or 'stage', not %r" % (name,))
    return _SUBPROBLEM[name]


_SHOOTING = {'single': 0, 'multiple': 1}


def _shooting(name):
    if name not in _SHOOTING:
        raise ValueError("shooting is 'single' or 'multiple', not %r" % (name,))
    return _SHOOTING[name]


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class NMPC:
    """Tracking NMPC of DMS_tracking_NMPC_casadi.m (absolute coordinates, nx = 4, nu = 1, one
    artificial-reference parameter theta); N <= 127."""

    def __init__(self, Q, R, P, T, LAMBDA, PSI, F_x, h_x, F_u, h_u, F_w_N, h_w_N, x_eq, u_eq, N,
                 delta=0.01):
        self.N, self.n, self.delta = int(N), int(N) + 1, float(delta)
        Tm = np.asarray(T, float) * np.eye(4) if np.ndim(T) == 0 else np.asarray(T, float)
        F_x = np.atleast_2d(np.asarray(F_x, float))
        F_u = np.asarray(F_u, float).reshape(-1, 1)
        F_T = np.atleast_2d(np.asarray(F_w_N, float))
        if F_x.shape[1] != 4 or F_T.shape[1] != 5:
            raise ValueError('F_x has 4 columns and F_w_N 5 ([x_N - x_eq; theta])')
        self.mx, self.mu, self.mp = F_x.shape[0], F_u.shape[0], F_T.shape[0]
        self.m = self.N * (self.mx + self.mu) + self.mp
        self.x_eq = _f64(np.asarray(x_eq, float).ravel())
        self.u_eq = _f64(np.atleast_1d(np.asarray(u_eq, float)).ravel()[:1])
        # the arrays the C structure points to (kept alive with the object)
        self._keep = [_upper_factor(self.delta * np.atleast_2d(Q)),
                      _upper_factor(self.delta * np.atleast_2d(R)), _upper_factor(P),
                      _upper_factor(Tm), _f64(np.asarray(LAMBDA, float).ravel()),
                      _f64(np.asarray(PSI, float).ravel()), self.x_eq, self.u_eq,
                      _f64(F_x.T), _f64(np.asarray(h_x, float).ravel()),       # column-major
                      _f64(F_u.ravel()), _f64(np.asarray(h_u, float).ravel()),
                      _f64(F_T.T), _f64(np.asarray(h_w_N, float).ravel())]

    def _dims(self, subproblem='dense', shooting='single'):
        return _lib.NmpcDims(self.N, self.mx, self.mu, self.mp, _subproblem(subproblem), _shooting(shooting))

    def _data(self, x0=None, soft=(None, None), x_ref=None):
        """x_ref: None or what _ref returns, (4,) for the batch or (batch, 4) (the caller keeps it
        alive over the call)"""
        return _lib.NmpcData(*[_lib.ptr(a) for a in self._keep], self.delta,
                             _lib.ptr(x0) if x0 is not None else None, 4,
                             *[_lib.ptr(a) if a is not None else None for a in soft],
                             _lib.ptr(x_ref) if x_ref is not None else None,
                             0 if x_ref is None or x_ref.ndim == 1 else 4)

    @staticmethod
    def _ref(x_ref, b):
        """the set-point as the C structure takes it: None, (4,) shared by the batch, or (b, 4)"""
        if x_ref is None:
            return None
        r = _f64(np.asarray(x_ref, float))
        if r.shape not in ((4,), (b, 4)):
            raise ValueError('x_ref has the shape (4,) or (batch, 4) = (%d, 4), not %r' % (b, r.shape))
        return r

    def _soft(self, xs_lin, xs_quad):
        """the row weights as the C structure takes them: None, or mx doubles (a scalar is every
        row's weight).  The caller keeps the arrays alive over the call."""
        return tuple(None if a is None else _f64(np.broadcast_to(np.asarray(a, float), (self.mx,))).copy()
                     for a in (xs_lin, xs_quad))

    def _z(self, b, z):
        if z is None:
            return np.zeros((b, self.n))
        return _f64(np.broadcast_to(np.atleast_2d(np.asarray(z, float)), (b, self.n))).copy()

    def linearize(self, xmeasure, z=None, handle=None, x_ref=None):
        """rollout and linearisation at z (batch, N + 1) = [u - u_eq; theta] from the measured
        states xmeasure (batch, 4), absolute.  Returns X (batch, N + 1, 4), cost (batch,),
        c (batch, m), C (batch, m, n) = dc/dz, H (batch, n, n) = 2 Jr'Jr, f (batch, n).
        x_ref: the set-point of the tracking cost, absolute, (4,) for the whole batch or (batch, 4)
        (bqp_nmpc_data.x_ref; None: the working point x_eq) - here and in stage_qp, dms_qp,
        stage_cost and solve."""
        lib = _lib.load()
        h = handle or _default_handle()
        x0 = _f64(np.atleast_2d(xmeasure))
        b, n, m = x0.shape[0], self.n, self.m
        z = self._z(b, z)
        X = np.zeros((b, self.N + 1, 4)); cost = np.zeros(b); c = np.zeros((b, m))
        Ccm = np.zeros((b, n, m)); H = np.zeros((b, n, n)); f = np.zeros((b, n))
        xr = self._ref(x_ref, b)
        dims, dd = self._dims(), self._data(x0, x_ref=xr)
        rc = lib.bqp_nmpc_linearize(h.value, C.byref(dims), b, C.byref(dd), _lib.ptr(z), _lib.ptr(X),
                                    _lib.ptr(cost), _lib.ptr(c), _lib.ptr(Ccm), _lib.ptr(H),
                                    _lib.ptr(f))
        _lib.check(rc, 'bqp_nmpc_linearize')
        return OcpResult(X=X, cost=cost, c=c, C=np.swapaxes(Ccm, 1, 2), H=H, f=f)

    def stage_qp(self, xmeasure, z=None, handle=None, x_ref=None):
        """the stage sub-problem at z as the stage route hands it to the structured solve
        (bqp_nmpc_stage_qp), in v_k = [dx_k; du_k; dtheta]: A (batch, N, 4, 4), B (batch, N, 4),
        w (batch, N + 1, 6), xlb / xub (batch, N + 1, 4; stage 0 is -inf / +inf), ulb / uub
        (batch, N), hp (batch, mp), and the shared W (N + 1, 6, 6) and Fp (mp, 6)."""
        lib = _lib.load()
        h = handle or _default_handle()
        x0 = _f64(np.atleast_2d(xmeasure))
        b, N, mp = x0.shape[0], self.N, self.mp
        z = self._z(b, z)
        Acm = np.zeros((b, N, 4, 4)); B = np.zeros((b, N, 4)); w = np.zeros((b, N + 1, 6))
        xlb = np.zeros((b, N + 1, 4)); xub = np.zeros((b, N + 1, 4))
        ulb = np.zeros((b, N)); uub = np.zeros((b, N)); hp = np.zeros((b, mp))
        W = np.zeros((N + 1, 6, 6)); Fcm = np.zeros((6, mp))
        xr = self._ref(x_ref, b)
        dims, dd = self._dims(), self._data(x0, x_ref=xr)
        rc = lib.bqp_nmpc_stage_qp(h.value, C.byref(dims), b, C.byref(dd), _lib.ptr(z), _lib.ptr(Acm),
                                   _lib.ptr(B), _lib.ptr(w), _lib.ptr(xlb), _lib.ptr(xub),
                                   _lib.ptr(ulb), _lib.ptr(uub), _lib.ptr(hp), _lib.ptr(W),
                                   _lib.ptr(Fcm))
        _lib.check(rc, 'bqp_nmpc_stage_qp')
        return OcpResult(A=np.swapaxes(Acm, 2, 3), B=B, w=w, xlb=xlb, xub=xub, ulb=ulb, uub=uub, hp=hp,
                         W=np.swapaxes(W, 1, 2), Fp=Fcm.T)

    def dms_qp(self, xmeasure, X=None, z=None, handle=None, x_ref=None):
        """the multiple-shooting sub-problem at the iterate (X, z) (bqp_nmpc_dms_qp): X (batch,
        N + 1, 4) absolute states (stage 0 is taken from xmeasure; None: the rollout of z).  Returns
        stage_qp's blocks, formed at the iterate's own states, and c (batch, N, 4), the defects
        dynamic(delta, x_k, u_k) - x_{k+1}."""
        lib = _lib.load()
        h = handle or _default_handle()
        x0 = _f64(np.atleast_2d(xmeasure))
        b, N, mp = x0.shape[0], self.N, self.mp
        z = self._z(b, z)
        if X is not None:
            X = _f64(np.broadcast_to(np.asarray(X, float), (b, N + 1, 4))).copy()
        Acm = np.zeros((b, N, 4, 4)); B = np.zeros((b, N, 4)); c = np.zeros((b, N, 4))
        w = np.zeros((b, N + 1, 6))
        xlb = np.zeros((b, N + 1, 4)); xub = np.zeros((b, N + 1, 4))
        ulb = np.zeros((b, N)); uub = np.zeros((b, N)); hp = np.zeros((b, mp))
        W = np.zeros((N + 1, 6, 6)); Fcm = np.zeros((6, mp))
        xr = self._ref(x_ref, b)
        dims, dd = self._dims('stage', 'multiple'), self._data(x0, x_ref=xr)
        rc = lib.bqp_nmpc_dms_qp(h.value, C.byref(dims), b, C.byref(dd),
                                 _lib.ptr(X) if X is not None else None, _lib.ptr(z), _lib.ptr(Acm),
                                 _lib.ptr(B), _lib.ptr(c), _lib.ptr(w), _lib.ptr(xlb), _lib.ptr(xub),
                                 _lib.ptr(ulb), _lib.ptr(uub), _lib.ptr(hp), _lib.ptr(W), _lib.ptr(Fcm))
        _lib.check(rc, 'bqp_nmpc_dms_qp')
        return OcpResult(A=np.swapaxes(Acm, 2, 3), B=B, c=c, w=w, xlb=xlb, xub=xub, ulb=ulb, uub=uub,
                         hp=hp, W=np.swapaxes(W, 1, 2), Fp=Fcm.T)

    def stage_cost(self, xmeasure, z=None, xs_lin=None, xs_quad=None, handle=None, x_ref=None):
        """what the stage route's merit function starts from at z (bqp_nmpc_stage_cost): cost
        (batch,) = J + penalty and penalty (batch,), the penalty of the softened rows at z."""
        lib = _lib.load()
        h = handle or _default_handle()
        x0 = _f64(np.atleast_2d(xmeasure))
        b = x0.shape[0]
        z = self._z(b, z)
        cost = np.zeros(b); pen = np.zeros(b)
        soft = self._soft(xs_lin, xs_quad)
        xr = self._ref(x_ref, b)
        dims, dd = self._dims('stage'), self._data(x0, soft, xr)
        rc = lib.bqp_nmpc_stage_cost(h.value, C.byref(dims), b, C.byref(dd), _lib.ptr(z), _lib.ptr(cost),
                                     _lib.ptr(pen))
        _lib.check(rc, 'bqp_nmpc_stage_cost')
        return OcpResult(cost=cost, penalty=pen)

    def solve(self, xmeasure, y0=None, z0=None, handle=None, max_iter=100, tol=1e-8, polish=0,
              subproblem='dense', xs_lin=None, xs_quad=None, shooting='single', X0=None, x_ref=None):
        """xmeasure (batch, 4) absolute states; y0 a start in the script's layout
        [x_0..x_N; u; theta] (its states are ignored: they follow from u) or z0 = [u - u_eq;
        theta]; cold start u = u_eq, theta = 0 otherwise.  subproblem: 'dense' (the condensed
        sub-problem on the dense kernels) or 'stage' (the sub-problem in stage form on the
        structured kernel with per-stage models; F_x and F_u must be box rows; polish is then that
        solve's: 0 / 1 after a 0 / -8 exit, 2 also on weakly active rows, -1 off).  xs_lin, xs_quad:
        soft state rows, a scalar or mx weights l1, l2 >= 0 per row of F_x (stage route only): a row
        with a positive weight may be violated at the price l1 s + 0.5 l2 s^2 of its slack s; the
        two rows of one state variable must carry the same weights in the variable's units
        (bqp_nmpc_data in bqp.h).  Returns y_OL
        (batch, 4 (N + 1) + N + 1) in the script's layout, u0, theta, z, lam (batch, m), cost (with
        weights: J + penalty), exitflag, iterations, slack (batch, N, mx) = max(c, 0) on the
        softened rows and 0 elsewhere, penalty (batch,).
        shooting: 'single' (the states eliminated) or 'multiple' (bqp_nmpc_dims.shooting = 1, stage
        route only, no soft rows: the states stay decision variables).  With 'multiple', X0 (batch,
        N + 1, 4) is the start's states (stage 0 is taken from xmeasure; None: the rollout of the
        start's z), and the result also holds X (batch, N + 1, 4), the solution's states, and pi
        (batch, N, 4), the multipliers of the dynamics rows; y_OL is then [X; u; theta] itself.
        x_ref: the set-point, as in linearize; theta then settles where LAMBDA theta is closest to
        x_ref - x_eq in the T norm, within the terminal set."""
        if shooting == 'multiple':
            return self._solve_dms(xmeasure, y0, z0, handle, max_iter, tol, polish, subproblem, xs_lin,
                                   xs_quad, X0, x_ref)
        if X0 is not None:
            raise ValueError("X0 belongs to shooting='multiple'")
        _shooting(shooting)
        lib = _lib.load()
        h = handle or _default_handle()
        x0 = _f64(np.atleast_2d(xmeasure))
        b, N, n, m = x0.shape[0], self.N, self.n, self.m
        if y0 is not None:
            y0 = np.atleast_2d(np.asarray(y0, float))
            z0 = np.concatenate([y0[:, 4 * (N + 1):4 * (N + 1) + N] - self.u_eq[0], y0[:, -1:]], axis=1)
        z = self._z(b, z0)
        lam = np.zeros((b, m)); cost = np.zeros(b)
        flag = np.zeros(b, np.int32); it = np.zeros(b, np.int32)
        soft = self._soft(xs_lin, xs_quad)
        xr = self._ref(x_ref, b)
        dims, dd = self._dims(subproblem), self._data(x0, soft, xr)
        o = _lib.options(max_iter=max_iter, tol_stat=tol, polish=polish)
        rc = lib.bqp_nmpc_solve_batched(h.value, C.byref(dims), b, C.byref(dd), C.byref(o),
                                        _lib.ptr(z), _lib.ptr(lam), _lib.ptr(cost), _lib.iptr(flag),
                                        _lib.iptr(it))
        _lib.check(rc, 'bqp_nmpc_solve_batched')
        r = OcpResult(z=z, lam=lam, cost=cost, exitflag=flag, iterations=it)
        # the open-loop states of the solution: the rollout the solver itself computes
        # and the rows' values there, for the slacks of the softened rows
        X = np.zeros((b, N + 1, 4)); c = np.zeros((b, m))
        rc = lib.bqp_nmpc_linearize(h.value, C.byref(dims), b, C.byref(dd), _lib.ptr(z), _lib.ptr(X),
                                    None, _lib.ptr(c), None, None, None)
        _lib.check(rc, 'bqp_nmpc_linearize')
        l1, l2 = [np.zeros(self.mx) if a is None else a for a in soft]
        ms = self.mx + self.mu
        slack = np.maximum(c[:, :N * ms].reshape(b, N, ms)[:, :, :self.mx], 0.0) * ((l1 > 0) | (l2 > 0))
        r.update(slack=slack, penalty=(l1 * slack + 0.5 * l2 * slack ** 2).sum(axis=(1, 2)))
        r.update(y_OL=np.concatenate([X.reshape(b, -1), z[:, :N] + self.u_eq[0], z[:, N:]], axis=1),
                 u0=z[:, :1] + self.u_eq[0], theta=z[:, N:])
        return r

    def _solve_dms(self, xmeasure, y0, z0, handle, max_iter, tol, polish, subproblem, xs_lin, xs_quad, X0,
                   x_ref=None):
        """NMPC.solve with shooting='multiple' (bqp_nmpc_dms_solve_batched)"""
        lib = _lib.load()
        h = handle or _default_handle()
        x0 = _f64(np.atleast_2d(xmeasure))
        b, N, m = x0.shape[0], self.N, self.m
        if y0 is not None:
            y0 = np.atleast_2d(np.asarray(y0, float))
            z0 = np.concatenate([y0[:, 4 * (N + 1):4 * (N + 1) + N] - self.u_eq[0], y0[:, -1:]], axis=1)
            if X0 is None:
                X0 = y0[:, :4 * (N + 1)].reshape(-1, N + 1, 4)
        z = self._z(b, z0)
        soft = self._soft(xs_lin, xs_quad)
        xr = self._ref(x_ref, b)
        dims, dd = self._dims(subproblem, 'multiple'), self._data(x0, soft, xr)
        if X0 is None:
            # the rollout of the start's z, as the library's linearisation computes it
            X = np.zeros((b, N + 1, 4))
            d1 = self._dims()
            rc = lib.bqp_nmpc_linearize(h.value, C.byref(d1), b, C.byref(dd), _lib.ptr(z), _lib.ptr(X),
                                        None, None, None, None, None)
            _lib.check(rc, 'bqp_nmpc_linearize')
        else:
            X = _f64(np.broadcast_to(np.asarray(X0, float), (b, N + 1, 4))).copy()
        lam = np.zeros((b, m)); pi = np.zeros((b, N, 4)); cost = np.zeros(b)
        flag = np.zeros(b, np.int32); it = np.zeros(b, np.int32)
        o = _lib.options(max_iter=max_iter, tol_stat=tol, polish=polish)
        rc = lib.bqp_nmpc_dms_solve_batched(h.value, C.byref(dims), b, C.byref(dd), C.byref(o), _lib.ptr(z),
                                            _lib.ptr(X), _lib.ptr(lam), _lib.ptr(pi), _lib.ptr(cost),
                                            _lib.iptr(flag), _lib.iptr(it))
        _lib.check(rc, 'bqp_nmpc_dms_solve_batched')
        return OcpResult(z=z, X=X, lam=lam, pi=pi, cost=cost, exitflag=flag, iterations=it,
                         y_OL=np.concatenate([X.reshape(b, -1), z[:, :N] + self.u_eq[0], z[:, N:]], axis=1),
                         u0=z[:, :1] + self.u_eq[0], theta=z[:, N:])


def _schedule(a, b, steps, name):
    """a schedule as bqp_nmpc_track takes it: (array, stride) from (steps, 4), shared by the batch, or
    (batch, steps, 4)"""
    if a is None:
        return None, 0
    a = _f64(np.asarray(a, float))
    if a.shape == (steps, 4):
        return a, 0
    if a.shape == (b, steps, 4):
        return a, steps * 4
    raise ValueError('%s has the shape (steps, 4) or (batch, steps, 4) = (%d, %d, 4), not %r'
                     % (name, b, steps, a.shape))


def closed_loop_nmpc(prob, x_init, steps, handle=None, max_iter=100, tol=1e-8, polish=0,
                     subproblem='dense', xs_lin=None, xs_quad=None, shooting='single', refs=None,
                     dist=None, x_ref=None, plant_params=None):
    """Closed loop of DMS_tracking_NMPC_casadi.m:153-207 for a batch of initial states x_init
    (batch, 4), absolute: per step the solve at the measured state, the RK4 plant with u_0, and
    the warm start (z shifted one stage, last move repeated, theta kept).  Every instance advances
    at its own step (with BQP_NMPC_SYNC set in the environment: the whole batch step by step, same
    results).  subproblem, xs_lin, xs_quad and shooting as in NMPC.solve (with 'multiple' the warm
    start also carries the states: x_k <- x_{k+1}, x_N stepped with the repeated last move).  Returns X (batch, steps + 1, 4), U (batch, steps), exitflag and iterations
    (batch, steps), kernel_ms, launches and rounds, the SQP rounds the loop launched.
    refs: a set-point schedule, absolute, (steps, 4) for the whole batch or (batch, steps, 4): step t
    is solved with the set-point refs[t] (constant over the horizon; NMPC.linearize says how it enters
    the cost); dist, same shapes: X[t + 1] = dynamic(delta, X[t], U[t]) + dist[t].  With either, the
    loop is bqp_closed_loop_nmpc_track and the result also holds theta (batch, steps), the theta of
    every step's solution; with neither it is bqp_closed_loop_nmpc, as before.  x_ref: a constant
    set-point, (4,) or (batch, 4), for the steps no schedule covers.
    plant_params: the coefficients p = [x2_c, 1/beta^2, wn^2, 2 zeta wn] of the plant the loop steps
    (bqp.mg_plant_params), (4,), (batch, 4), or a schedule (steps, 4) / (batch, steps, 4) whose row t
    takes X[:, t] to X[:, t + 1]; with batch == steps a (steps, 4) array is the schedule shared by the
    batch, as for refs.  The model inside the solve stays nominal: the mismatch is the experiment.
    Default: the nominal plant, the launches as they were."""
    lib = _lib.load()
    h = handle or _default_handle()
    xi = _f64(np.atleast_2d(x_init))
    b, steps = xi.shape[0], int(steps)
    X = np.zeros((b, steps + 1, 4)); U = np.zeros((b, steps))
    fl = np.zeros((b, steps), np.int32); it = np.zeros((b, steps), np.int32)
    soft = prob._soft(xs_lin, xs_quad)
    xr = prob._ref(x_ref, b)
    dims, dd = prob._dims(subproblem, shooting), prob._data(soft=soft, x_ref=xr)
    cl = ClosedLoop(_BQP_PLANT_MG_RK4, steps, prob.delta, _lib.ptr(prob.x_eq), _lib.ptr(prob.u_eq))
    par = _set_plant_params(cl, plant_params, b, steps)   # kept alive over the call
    o = _lib.options(max_iter=max_iter, tol_stat=tol, polish=polish)
    r = OcpResult(X=X, U=U, exitflag=fl, iterations=it)
    if refs is None and dist is None:
        rc = lib.bqp_closed_loop_nmpc(h.value, C.byref(dims), b, C.byref(dd), C.byref(o), C.byref(cl),
                                      _lib.ptr(xi), _lib.ptr(X), _lib.ptr(U), _lib.iptr(fl), _lib.iptr(it))
        _lib.check(rc, 'bqp_closed_loop_nmpc')
    else:
        (ra, sr), (da, sd) = _schedule(refs, b, steps, 'refs'), _schedule(dist, b, steps, 'dist')
        theta = np.zeros((b, steps))
        tr = _lib.NmpcTrack(_lib.ptr(ra) if ra is not None else None, sr,
                            _lib.ptr(da) if da is not None else None, sd, _lib.ptr(theta))
        rc = lib.bqp_closed_loop_nmpc_track(h.value, C.byref(dims), b, C.byref(dd), C.byref(o), C.byref(cl),
                                            _lib.ptr(xi), C.byref(tr), _lib.ptr(X), _lib.ptr(U),
                                            _lib.iptr(fl), _lib.iptr(it))
        _lib.check(rc, 'bqp_closed_loop_nmpc_track')
        r.update(theta=theta)
    ms, launches = h.kernel_ms()
    r.update(kernel_ms=ms, launches=launches, rounds=h.loop_rounds())
    return r
