"""Closed-loop simulation on the GPU (bqp_closed_loop_ocp): the MPC loop of the reference's
tracking-LMPC examples - solve at the measured state, apply the first move to the true plant,
repeat - for a whole batch of initial states at once.

Reference: ``examples/DMS_tracking_LMPC_casadi.m:153-189`` / ``DSS_tracking_LMPC_casadi.m``
(``solver(...)`` then ``xmeasure = dynamic(delta, xmeasure, u_OL(1:m))``), with the
Moore-Greitzer plant ``system`` (:215-221) integrated by one RK4 step (``dynamic``, :297-304).
With a reference schedule and / or a linear plant (bqp_closed_loop_track):
``trackingMPC/RunExample.m:131-147`` and ``RunExample_robust.m``.
"""
import ctypes as C

import numpy as np

from . import _lib
from .ocp import OcpResult, _cm, _default_handle, pack

BQP_PLANT_MG_RK4 = 1
BQP_PLANT_MG_ODE23 = 2
BQP_PLANT_LINEAR = 3
_PLANTS = {'rk4': BQP_PLANT_MG_RK4, 'ode23': BQP_PLANT_MG_ODE23, 'linear': BQP_PLANT_LINEAR}


class ClosedLoop(C.Structure):
    # the trailing members (plant_params=) default to zero: the nominal plant
    _fields_ = [('plant', C.c_int), ('steps', C.c_int), ('delta', C.c_double),
                ('x_eq', _lib._PD), ('u_eq', _lib._PD),
                ('plant_par', _lib._PD), ('splant_par', C.c_int64), ('plant_par_sched', C.c_int)]


def mg_plant_params(x2_c=0.0, beta=1.0, wn2=1000.0, damping=2.0 * np.sqrt(500.0), wn=None, zeta=None):
    """The Moore-Greitzer plant's coefficient vector p = [x2_c, 1/beta^2, wn^2, 2 zeta wn]
    (models/trueModel.m:32-41 names x2_c, beta, wn, zeta) as plant_params= takes it; the arguments
    broadcast against each other, the result has their common shape + (4,).  wn2 and damping are
    wn^2 and 2 zeta wn themselves; wn= replaces wn2 by wn^2, and zeta= (with wn, or with sqrt(wn2))
    replaces damping by 2 zeta wn.  Without arguments: the nominal plant [0, 1, 1000, 2 sqrt(500)],
    exactly."""
    if wn is not None:
        wn2 = np.square(np.asarray(wn, float))
    if zeta is not None:
        w = np.asarray(wn, float) if wn is not None else np.sqrt(np.asarray(wn2, float))
        damping = 2.0 * np.asarray(zeta, float) * w
    beta = np.asarray(beta, float)
    parts = np.broadcast_arrays(np.asarray(x2_c, float), 1.0 / (beta * beta), np.asarray(wn2, float),
                                np.asarray(damping, float))
    return np.ascontiguousarray(np.stack(parts, axis=-1), dtype=np.float64)


def mg_steady_state(params, x1):
    """(x_s, u_s) of the plant with coefficients params (..., 4) at the mass flow x1:
    x2 = x2_c + 1 + 1.5 x1 - x1^3 / 2, x3 = (x1 + 1) / sqrt(x2), x4 = 0, u = x3 - independent of
    beta, wn and zeta.  x_s (..., 4), u_s (...,), broadcast over params[..., 0] and x1: the offset a
    controller designed at the nominal working point leaves on a perturbed plant is read off it."""
    p = np.asarray(params, float)
    x2c, x1 = np.broadcast_arrays(p[..., 0], np.asarray(x1, float))
    x2 = x2c + 1.0 + 1.5 * x1 - x1 * x1 * x1 / 2.0
    x3 = (x1 + 1.0) / np.sqrt(x2)
    return np.stack([x1, x2, x3, np.zeros_like(x3)], axis=-1), x3


def _plant_params(a, b, steps):
    """plant_params= as bqp_closed_loop takes it: (array, stride, sched) from (4,) - one plant for
    the batch -, (batch, 4), (steps, 4) - a schedule shared by the batch - or (batch, steps, 4).
    With batch == steps a (steps, 4) array is the shared schedule (the schedule shape is tried
    first, as nmpc._schedule tries its own)."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape == (4,):
        return a, 0, 0
    if a.shape == (steps, 4):
        return a, 0, 1
    if a.shape == (b, 4):
        return a, 4, 0
    if a.shape == (b, steps, 4):
        return a, steps * 4, 1
    raise ValueError('plant_params has the shape (4,), (batch, 4), (steps, 4) or (batch, steps, 4) with '
                     '(batch, steps) = (%d, %d), not %r' % (b, steps, a.shape))


def _set_plant_params(cl, plant_params, b, steps):
    """fills the trailing members of cl; returns the arrays to keep alive (and to move, device=)"""
    if plant_params is None:
        return []
    a, cl.splant_par, cl.plant_par_sched = _plant_params(plant_params, b, steps)
    cl.plant_par = _lib.ptr(a)
    return [a]


class Learning(C.Structure):
    _fields_ = [('q', C.c_int), ('mask', C.c_int), ('bandwidth', C.c_double),
                ('lambda_', C.c_double), ('XL', _lib._PD), ('window', _lib._PD)]


class _Dev:
    """device=... path of the closed loops: the inputs of a packed ctypes
    structure moved to the GPU (each pointer field replaced by a device copy of the numpy array it
    pointed to) and the outputs allocated there, so that the _device entry points run on device
    memory and the trajectories stay in HBM for bqp.dist.gather_rows (RCCL all-gather) - no host
    round trip between the loop and the collective.  torch brings its own copy of the HIP runtime:
    a process that uses device= lets torch open the GPU (torch.cuda.is_available()) before its
    first bqp call, as smoke() and bench.py do - opened after libbqp's, torch's copy finds no GPU."""

    def __init__(self, device):
        import torch
        self.torch = torch
        self.dev = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        self.keep = []

    def inputs(self, st, arrays):
        by_addr = {a.ctypes.data: a for a in arrays if a is not None}
        for name, typ in st._fields_:
            if typ not in (_lib._PD, _lib._PI):
                continue
            p = getattr(st, name)
            if not p:
                continue
            a = by_addr[C.cast(p, C.c_void_p).value]
            t = self.torch.from_numpy(a).to(self.dev)
            self.keep.append(t)
            setattr(st, name, C.cast(C.c_void_p(t.data_ptr()), typ))

    def array(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.keep.append(t)
        return t

    def out(self, shape, dtype=np.float64):
        t = self.torch.zeros(shape, dtype=self.torch.float64 if dtype == np.float64 else self.torch.int32,
                             device=self.dev)
        return t

    @staticmethod
    def p(t, typ=None):
        if t is None:
            return None
        return C.cast(C.c_void_p(t.data_ptr()), typ or (_lib._PD if t.dtype.is_floating_point else _lib._PI))

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream)


def closed_loop(mpc, x_init, steps, delta=0.01, handle=None, learning=None, plant='rk4',
                x_eq=None, u_eq=None, device=None, refs=None, dist=None, plant_model=None,
                plant_params=None, **opts):
    """mpc: a TrackingLMPC / TrackingLBMPC (deviation coordinates around mpc.x_eq, mpc.u_eq), or
    an LMPC with the working point passed as x_eq / u_eq (functions/ocpLMPC.m: x_wp, u_wp);
    x_init (batch, n) absolute initial states.  Returns X (batch, steps+1, n), U (batch, steps,
    m) absolute, and the per-step exit flags (batch, steps).
    plant: 'rk4' - one RK4 step per period (`dynamic` of the CasADi scripts); 'ode23' - MATLAB's
    ode23 at its default options (models/trueModel.m behind transitionTrue.m, the plant of the
    fmincon loops ocpLMPC.m / ocpLBMPC.m).

    learning=dict(q=100, mask=1[, bandwidth, lambda_]) also keeps the learned model's data window
    per instance (bqp_closed_loop_lbmpc: LBMPC_casadi.m:193-198 / DMS_LBMPC_casadi.m:198-207)
    and returns XL (batch, steps+1, n), the learned one-step predictions, and window
    (batch, q, 8), the final windows [X; Y; v] per point in ring order (iteration it's sample
    in point it mod q).

    device (a GPU index or torch device): run on device memory through the _device entry points
    (bqp_closed_loop_ocp_device / _lbmpc_device) on torch's current stream of that device; the
    results are torch tensors there (the trajectories stay in HBM, e.g. for bqp.dist.gather_rows).

    Reference schedules and linear plants (bqp_closed_loop_track: trackingMPC/RunExample.m:131-147
    and RunExample_robust.m) - any of the following, or an mpc without a working point (a
    TrackingMPC; the working point is then zero), selects that loop, which also returns theta
    (batch, steps, p), the artificial steady state of every step (art_refHistory = Mtheta theta):
    refs (steps, nr) or (batch, steps, nr): the reference of every step, mapped to the solve's
    linear term by mpc.reference_map() (TrackingMPC: xs = set_ref(k); TrackingLMPC / LBMPC: the
    set-point in deviation from x_eq);
    plant='linear': x+ = x_eq + Ap (x - x_eq) + Bp (u - u_eq) + d_t (getTransitions.m) with
    plant_model=(Ap, Bp), each shared or per instance (default: the MPC's own A, B), and
    dist (steps, n) or (batch, steps, n), the additive disturbance d_t (default: none).

    plant_params (MG plants, every loop above, device= included): the plant's coefficients
    p = [x2_c, 1/beta^2, wn^2, 2 zeta wn] (mg_plant_params builds them), (4,) for the batch,
    (batch, 4) per instance, or a schedule (steps, 4) / (batch, steps, 4) whose row t is the plant
    that takes X[:, t] to X[:, t + 1].  With batch == steps a (steps, 4) array is the schedule
    shared by the batch.  The controller's model stays as it is; with learning= the window's Y and
    XL see the perturbed plant.  Default: the nominal plant, the launches as they were."""
    lib = _lib.load()
    h = handle or _default_handle()
    x_init = np.ascontiguousarray(np.atleast_2d(x_init), dtype=np.float64)
    b = x_init.shape[0]
    prob = mpc.prob
    no_wp = x_eq is None and not hasattr(mpc, 'x_eq')
    if plant == 'linear' or no_wp or any(v is not None for v in (refs, dist, plant_model)):
        if learning is not None:
            raise ValueError('closed_loop: learning= does not combine with refs / dist / '
                             'plant_model / plant=\'linear\'')
        return _closed_loop_track(lib, h, mpc, x_init, b, int(steps), delta, plant, x_eq, u_eq,
                                  device, refs, dist, plant_model, plant_params, opts)
    xeq = np.ascontiguousarray(mpc.x_eq if x_eq is None else np.ravel(x_eq), dtype=np.float64)
    ueq = np.ascontiguousarray(mpc.u_eq if u_eq is None else np.ravel(u_eq), dtype=np.float64)
    dims, data, batch, keep = pack(prob, x_init - xeq)
    cl = ClosedLoop(_PLANTS[plant], int(steps), float(delta), _lib.ptr(xeq), _lib.ptr(ueq))
    par = _set_plant_params(cl, plant_params, b, int(steps))
    if device is not None:
        return _closed_loop_device(lib, h, mpc, dims, data, keep, cl, [xeq, ueq] + par, x_init, b, steps,
                                   learning, device, opts)
    X = np.zeros((b, steps + 1, prob.nx)); U = np.zeros((b, steps, prob.nu))
    flags = np.zeros((b, steps), np.int32)
    o = _lib.options(**opts)
    if learning is None:
        rc = lib.bqp_closed_loop_ocp(h.value, C.byref(dims), b, C.byref(data), C.byref(o),
                                     C.byref(cl), _lib.ptr(x_init), _lib.ptr(X), _lib.ptr(U),
                                     _lib.iptr(flags))
        _lib.check(rc, 'bqp_closed_loop_ocp')
        return OcpResult(X=X, U=U, exitflag=flags)
    q = int(learning.get('q', 100))
    XL = np.zeros_like(X)
    win = np.zeros((b, q, 8))
    lw = Learning(q, int(learning.get('mask', 1)), float(learning.get('bandwidth', 0.0)),
                  float(learning.get('lambda_', 0.0)), _lib.ptr(XL), _lib.ptr(win))
    rc = lib.bqp_closed_loop_lbmpc(h.value, C.byref(dims), b, C.byref(data), C.byref(o),
                                   C.byref(cl), C.byref(lw), _lib.ptr(x_init), _lib.ptr(X),
                                   _lib.ptr(U), _lib.iptr(flags))
    _lib.check(rc, 'bqp_closed_loop_lbmpc')
    return OcpResult(X=X, U=U, exitflag=flags, XL=XL, window=win)


def _closed_loop_device(lib, h, mpc, dims, data, keep, cl, wp, x_init, b, steps, learning, device,
                        opts):
    prob = mpc.prob
    d = _Dev(device)
    d.inputs(data, keep)
    d.inputs(cl, wp)
    xi = d.array(x_init)
    X = d.out((b, steps + 1, prob.nx)); U = d.out((b, steps, prob.nu))
    flags = d.out((b, steps), np.int32)
    o = _lib.options(**opts)
    if learning is None:
        rc = lib.bqp_closed_loop_ocp_device(h.value, C.byref(dims), b, C.byref(data), C.byref(o),
                                            C.byref(cl), d.p(xi), d.p(X), d.p(U), d.p(flags),
                                            d.stream())
        _lib.check(rc, 'bqp_closed_loop_ocp_device')
        d.torch.cuda.current_stream(d.dev).synchronize()
        return OcpResult(X=X, U=U, exitflag=flags)
    q = int(learning.get('q', 100))
    XL = d.out((b, steps + 1, prob.nx)); win = d.out((b, q, 8))
    lw = Learning(q, int(learning.get('mask', 1)), float(learning.get('bandwidth', 0.0)),
                  float(learning.get('lambda_', 0.0)), d.p(XL), d.p(win))
    rc = lib.bqp_closed_loop_lbmpc_device(h.value, C.byref(dims), b, C.byref(data), C.byref(o),
                                          C.byref(cl), C.byref(lw), d.p(xi), d.p(X), d.p(U),
                                          d.p(flags), d.stream())
    _lib.check(rc, 'bqp_closed_loop_lbmpc_device')
    d.torch.cuda.current_stream(d.dev).synchronize()
    return OcpResult(X=X, U=U, exitflag=flags, XL=XL, window=win)


def _shared_or_batch(a, b, shape, name):
    """a of the given shape (one copy for the batch) or (batch,) + shape: the contiguous array and
    its element stride between instances (0 = shared)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape == tuple(shape):
        return a, 0
    if a.shape == (b,) + tuple(shape):
        return a, int(np.prod(shape))
    raise ValueError('%s: shape %s, expected %s or %s' % (name, a.shape, tuple(shape), (b,) + tuple(shape)))


def _closed_loop_track(lib, h, mpc, x_init, b, steps, delta, plant, x_eq, u_eq, device, refs, dist,
                       plant_model, plant_params, opts):
    """bqp_closed_loop_track(_device): the closed loop with a reference schedule and / or the
    linear plant (see closed_loop)"""
    prob = mpc.prob
    nx, nu, npar = prob.nx, prob.nu, prob.np
    xeq = np.ascontiguousarray(getattr(mpc, 'x_eq', np.zeros(nx)) if x_eq is None else np.ravel(x_eq),
                               dtype=np.float64)
    ueq = np.ascontiguousarray(getattr(mpc, 'u_eq', np.zeros(nu)) if u_eq is None else np.ravel(u_eq),
                               dtype=np.float64)
    if plant != 'linear' and (dist is not None or plant_model is not None):
        raise ValueError("closed_loop: dist= and plant_model= belong to plant='linear'")
    dims, data, _, keep = pack(prob, x_init - xeq)
    cl = ClosedLoop(_PLANTS[plant], steps, float(delta), _lib.ptr(xeq), _lib.ptr(ueq))
    par = _set_plant_params(cl, plant_params, b, steps)
    tr = _lib.Track()
    arrays = []
    if plant_model is not None:
        Ap, sAp = _shared_or_batch(_cm(np.asarray(plant_model[0], float)), b, (nx, nx), 'plant_model[0]')
        Bp, sBp = _shared_or_batch(_cm(np.asarray(plant_model[1], float)), b, (nu, nx), 'plant_model[1]')
        tr.Ap, tr.sAp, tr.Bp, tr.sBp = _lib.ptr(Ap), sAp, _lib.ptr(Bp), sBp
        arrays += [Ap, Bp]
    if dist is not None:
        dd, tr.sdist = _shared_or_batch(dist, b, (steps, nx), 'dist')
        tr.dist = _lib.ptr(dd)
        arrays.append(dd)
    if refs is not None:
        Wr = np.asarray(mpc.reference_map(), float)
        nr = Wr.shape[1]
        Wc = np.ascontiguousarray(Wr.T)                  # column-major (N+1)*nv x nr
        rr, tr.sref = _shared_or_batch(refs, b, (steps, nr), 'refs')
        tr.nr, tr.Wr, tr.ref = nr, _lib.ptr(Wc), _lib.ptr(rr)
        arrays += [Wc, rr]
    o = _lib.options(**opts)
    if device is None:
        X = np.zeros((b, steps + 1, nx)); U = np.zeros((b, steps, nu))
        theta = np.zeros((b, steps, npar)); flags = np.zeros((b, steps), np.int32)
        tr.THETA = _lib.ptr(theta)
        rc = lib.bqp_closed_loop_track(h.value, C.byref(dims), b, C.byref(data), C.byref(o),
                                       C.byref(cl), C.byref(tr), _lib.ptr(x_init), _lib.ptr(X),
                                       _lib.ptr(U), _lib.iptr(flags))
        _lib.check(rc, 'bqp_closed_loop_track')
        lo, hi = getattr(mpc, 'xlb0', None), getattr(mpc, 'xub0', None)
    else:
        d = _Dev(device)
        d.inputs(data, keep)
        d.inputs(cl, [xeq, ueq] + par)
        d.inputs(tr, arrays)
        xi = d.array(x_init)
        X = d.out((b, steps + 1, nx)); U = d.out((b, steps, nu))
        theta = d.out((b, steps, npar)); flags = d.out((b, steps), np.int32)
        tr.THETA = d.p(theta)
        rc = lib.bqp_closed_loop_track_device(h.value, C.byref(dims), b, C.byref(data), C.byref(o),
                                              C.byref(cl), C.byref(tr), d.p(xi), d.p(X), d.p(U),
                                              d.p(flags), d.stream())
        _lib.check(rc, 'bqp_closed_loop_track_device')
        d.torch.cuda.current_stream(d.dev).synchronize()
        lo, hi = (d.array(v) if v is not None else None
                  for v in (getattr(mpc, 'xlb0', None), getattr(mpc, 'xub0', None)))
    if lo is not None:
        # TrackingMPC: the constant rows on x_0 (constraintsFunction.m, k = 1) are checked on the
        # host, as TrackingMPC.solve does: a measured state outside them makes the step's
        # problem infeasible
        xm = X[:, :steps]
        flags[((xm > hi + 1e-12) | (xm < lo - 1e-12)).any(2)] = -2
    return OcpResult(X=X, U=U, exitflag=flags, theta=theta)


def closed_loop_sqp(mpc, x_init, steps, learning=None, warm=True, delta=0.01, handle=None,
                    max_iter=200, tol=1e-8, log_z=False, plant='rk4', x_eq=None,
                    u_eq=None, polish=0, device=None, plant_params=None):
    """Learned-model NLP closed loop on the GPU (bqp_closed_loop_sqp): per step the batched
    Gauss-Newton SQP of mpc (a DMSLBMPC - DMS_LBMPC_casadi.m:163-218 -, HybridLBMPC -
    hybrid_LBMPC_casadi.m:163-204 - or LBMPC) at the measured states, one RK4 plant step with the
    first move, and get_data.m's window update.  x_init (batch, n) absolute.
    learning=dict(q=100, mask=1[, bandwidth, lambda_]): mask 1 is DMS_LBMPC_casadi.m's 8 x q
    window (only the first, zero point valid at the start), mask 0 counts every point (the 7-row
    window of hybrid_LBMPC_casadi.m).  warm: the scripts' shifted guess (previous inputs moved one
    stage, zero last move, theta kept); otherwise z = 0 each step.
    plant: 'rk4' (the CasADi scripts' `dynamic`) or 'ode23' (models/trueModel.m, the fmincon loop
    functions/ocpLBMPC.m; its update_data.m window of q points equals this ring with q - 1: the
    initial zero point leaves when the q-th sample arrives).  polish: the QP sub-problems'
    active-set polish (bqp_options.polish encoding; 0 = the loop's default 3, polish only once the
    SQP stalls at a step; 1 also after -8 sub-problem exits; -1 off).
    Returns X (batch, steps+1, n), U (batch, steps, m) absolute, exitflag and iterations (batch,
    steps), XL (batch, steps+1, n) the learned one-step predictions, window (batch, q, 8) the
    final windows in ring order, and with log_z every step's solution Z (batch, steps, nz).
    device (a GPU index or torch device): bqp_closed_loop_sqp_device on device memory and torch's
    current stream there; every result is a torch tensor on that device.
    plant_params: the plant's coefficients, as closed_loop takes them ((4,), (batch, 4), (steps, 4)
    or (batch, steps, 4); with batch == steps a (steps, 4) array is the shared schedule): each
    instance's window then learns its own plant's mismatch."""
    lib = _lib.load()
    h = handle or _default_handle()
    learning = dict(learning or {})
    x_init = np.ascontiguousarray(np.atleast_2d(x_init), dtype=np.float64)
    b = x_init.shape[0]
    q = int(learning.get('q', 100))
    mask = int(learning.get('mask', 1))
    # working point: the caller's (LBMPC, ocpLBMPC.m's x_wp / u_wp), else the shim's own
    x_eq = np.ascontiguousarray(getattr(mpc, 'x_eq', np.zeros(mpc.n)) if x_eq is None else np.ravel(x_eq),
                                dtype=np.float64)
    u_eq = np.ascontiguousarray(getattr(mpc, 'u_eq', np.zeros(mpc.m)) if u_eq is None else np.ravel(u_eq),
                                dtype=np.float64)
    mrows = mpc.Ain.shape[0]
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in
            (mpc.A.T, mpc.B.T, mpc.K.T, mpc.Lq, mpc.Lr, mpc.Lp, mpc.Lt, mpc.LAMBDA.T, mpc.PSI.T,
             mpc.xs)]
    bin0 = np.ascontiguousarray(mpc.b0, dtype=np.float64)
    Bx = np.ascontiguousarray(mpc.Bx.T, dtype=np.float64)        # column-major m x n
    dims = _lib.LbmpcDims(mpc.n, mpc.m, mpc.p, mpc.N, mpc.n_run, int(mpc.term_learned), q, mrows, 1,
                          int(getattr(mpc, 'hessian', 'exact') == 'exact'))
    dd = _lib.LbmpcData(*[_lib.ptr(a) for a in keep], None, 0, None, 0, _lib.ptr(mpc.Ain_cm), None,
                        0, mpc.bandwidth, mpc.lam)
    if device is not None:
        return _closed_loop_sqp_device(lib, h, mpc, dims, dd, keep, bin0, Bx, x_eq, u_eq, x_init, b,
                                       steps, q, mask, learning, warm, delta, plant, max_iter, tol,
                                       log_z, polish, device, plant_params)
    X = np.zeros((b, steps + 1, mpc.n)); U = np.zeros((b, steps, mpc.m))
    XL = np.zeros_like(X); win = np.zeros((b, q, 8))
    flags = np.zeros((b, steps), np.int32); its = np.zeros((b, steps), np.int32)
    Z = np.zeros((b, steps, mpc.nz)) if log_z else None
    sl = _lib.SqpLoop(_lib.ptr(bin0), _lib.ptr(Bx), int(bool(warm)), _lib.ptr(Z), _lib.iptr(its))
    cl = ClosedLoop(_PLANTS[plant], int(steps), float(delta), _lib.ptr(x_eq), _lib.ptr(u_eq))
    par = _set_plant_params(cl, plant_params, b, int(steps))
    lw = Learning(q, mask, float(learning.get('bandwidth', 0.0)), float(learning.get('lambda_', 0.0)),
                  _lib.ptr(XL), _lib.ptr(win))
    o = _lib.options(max_iter=max_iter, tol_stat=tol, polish=polish)
    rc = lib.bqp_closed_loop_sqp(h.value, C.byref(dims), b, C.byref(dd), C.byref(sl), C.byref(o),
                                 C.byref(cl), C.byref(lw), _lib.ptr(x_init), _lib.ptr(X),
                                 _lib.ptr(U), _lib.iptr(flags))
    _lib.check(rc, 'bqp_closed_loop_sqp')
    out = OcpResult(X=X, U=U, exitflag=flags, iterations=its, XL=XL, window=win)
    if log_z:
        out.update(Z=Z)
    return out


def _closed_loop_sqp_device(lib, h, mpc, dims, dd, keep, bin0, Bx, x_eq, u_eq, x_init, b, steps, q,
                            mask, learning, warm, delta, plant, max_iter, tol, log_z, polish,
                            device, plant_params=None):
    d = _Dev(device)
    d.inputs(dd, keep + [mpc.Ain_cm])
    X = d.out((b, steps + 1, mpc.n)); U = d.out((b, steps, mpc.m))
    XL = d.out((b, steps + 1, mpc.n)); win = d.out((b, q, 8))
    flags = d.out((b, steps), np.int32); its = d.out((b, steps), np.int32)
    Z = d.out((b, steps, mpc.nz)) if log_z else None
    sl = _lib.SqpLoop(d.p(d.array(bin0)), d.p(d.array(Bx)), int(bool(warm)), d.p(Z), d.p(its))
    cl = ClosedLoop(_PLANTS[plant], int(steps), float(delta), d.p(d.array(x_eq)), d.p(d.array(u_eq)))
    for a in _set_plant_params(cl, plant_params, b, int(steps)):
        cl.plant_par = d.p(d.array(a))
    lw = Learning(q, mask, float(learning.get('bandwidth', 0.0)), float(learning.get('lambda_', 0.0)),
                  d.p(XL), d.p(win))
    o = _lib.options(max_iter=max_iter, tol_stat=tol, polish=polish)
    xi = d.array(x_init)
    rc = lib.bqp_closed_loop_sqp_device(h.value, C.byref(dims), b, C.byref(dd), C.byref(sl), C.byref(o),
                                        C.byref(cl), C.byref(lw), d.p(xi), d.p(X), d.p(U), d.p(flags),
                                        d.stream())
    _lib.check(rc, 'bqp_closed_loop_sqp_device')
    d.torch.cuda.current_stream(d.dev).synchronize()
    out = OcpResult(X=X, U=U, exitflag=flags, iterations=its, XL=XL, window=win)
    if log_z:
        out.update(Z=Z)
    return out
