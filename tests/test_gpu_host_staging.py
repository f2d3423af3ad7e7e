"""GPU tests of the host-pointer entry points' staging (csrc/bqp_api.cpp): the optional outputs
(a null host pointer is not copied back and changes nothing else) and the grow-only workspaces
(a handle that has solved other shapes before answers like a fresh one).  Short horizons only."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lmpc(mg, term_set):
    import bqp
    return bqp.LMPC(mg['A'], mg['B'], mg['K'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'],
                    mg['LAMBDA'], mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'],
                    term_set[0], term_set[1], N=20)


@pytest.fixture(scope='module')
def states():
    g = golden('lmpc_N20.npz')
    return g['dx'][g['idx']]


def _ocp_call(handle, prob, X0, fval=True, out=True, duals='all'):
    """bqp_solve_ocp_batched through ctypes with the chosen optional outputs"""
    from bqp import _lib, ocp
    lib = _lib.load()
    dims, data, batch, keep = ocp.pack(prob, X0)
    N, nx, nu, npar, mp = prob.N, prob.nx, prob.nu, prob.np, prob.mp
    r = dict(x=np.zeros((batch, N + 1, nx)), u=np.zeros((batch, N, nu)), theta=np.zeros((batch, npar)),
             exitflag=np.zeros(batch, np.int32), fval=np.zeros(batch),
             pi=np.zeros((batch, N, nx)), lam_x=np.zeros((batch, N + 1, 2, nx)),
             lam_u=np.zeros((batch, N, 2, nu)), lam_p=np.zeros((batch, mp)))
    outs = (_lib.Output * batch)()
    dd = None
    if duals == 'all':
        dd = _lib.OcpDuals(*(_lib.ptr(r[k]) for k in ('pi', 'lam_x', 'lam_u', 'lam_p')))
    elif duals == 'pi':
        dd = _lib.OcpDuals(_lib.ptr(r['pi']), None, None, None)
    o = _lib.options()
    rc = lib.bqp_solve_ocp_batched(handle.value, C.byref(dims), batch, C.byref(data), C.byref(o),
                                   _lib.ptr(r['x']), _lib.ptr(r['u']), _lib.ptr(r['theta']),
                                   _lib.ptr(r['fval']) if fval else None, _lib.iptr(r['exitflag']),
                                   outs if out else None, C.byref(dd) if dd else None)
    _lib.check(rc, 'bqp_solve_ocp_batched')
    r['iterations'] = np.array([q.iterations for q in outs])
    return r


def test_ocp_optional_outputs(lmpc, states):
    import bqp
    h = bqp.Handle(0)
    X0 = states[:3]
    full = _ocp_call(h, lmpc.prob, X0)
    bare = _ocp_call(h, lmpc.prob, X0, fval=False, out=False, duals=None)
    only_pi = _ocp_call(h, lmpc.prob, X0, duals='pi')
    assert (full['exitflag'] == 1).all(), full['exitflag']
    assert np.abs(full['pi']).max() > 0 and full['fval'].all() and (full['iterations'] > 0).all()
    for r in (bare, only_pi):
        for k in ('x', 'u', 'theta', 'exitflag'):
            assert np.array_equal(full[k], r[k]), k
    # what was not asked for is not written
    for k in ('fval', 'pi', 'lam_x', 'lam_u', 'lam_p', 'iterations'):
        assert not bare[k].any(), k
    assert np.array_equal(only_pi['pi'], full['pi']) and np.array_equal(only_pi['fval'], full['fval'])
    for k in ('lam_x', 'lam_u', 'lam_p'):
        assert not only_pi[k].any(), k


def test_quadprog_optional_multipliers():
    """the m = 300 case of tests/test_gpu_quadprog.py at batch 3: all four multiplier pointers
    null against all present"""
    import bqp
    from bqp import _lib
    lib = _lib.load()
    h = bqp.Handle(0)
    n, m, B = 101, 300, 3
    rng = np.random.default_rng(7 + m)
    M = rng.standard_normal((n, n))
    H = np.ascontiguousarray((M @ M.T / n + np.eye(n)).T)
    A = np.ascontiguousarray(rng.standard_normal((m, n)).T)      # column-major m x n
    f = rng.standard_normal((4, n))[:B].copy()
    b = rng.uniform(0.2, 1.0, (4, m))[:B].copy()
    lb, ub = -2.0 * np.ones(n), 2.0 * np.ones(n)
    dims = _lib.Dims(n, m, 0)
    st = _lib.Strides(0, n, 0, m, 0, 0, 0, 0)
    o = _lib.options()

    def call(lams):
        x = np.zeros((B, n)); fval = np.zeros(B); flag = np.zeros(B, np.int32)
        lam = [np.zeros((B, m)), np.zeros((B, 1)), np.zeros((B, n)), np.zeros((B, n))]
        out = (_lib.Output * B)()
        rc = lib.bqp_quadprog_batched(h.value, C.byref(dims), B, C.byref(st), _lib.ptr(H), _lib.ptr(f),
                                      _lib.ptr(A), _lib.ptr(b), None, None, _lib.ptr(lb), _lib.ptr(ub),
                                      None, C.byref(o), _lib.ptr(x), _lib.ptr(fval), _lib.iptr(flag),
                                      *[_lib.ptr(a) if lams else None for a in lam], out)
        _lib.check(rc, 'bqp_quadprog_batched')
        return x, fval, flag, lam

    x1, f1, e1, lam1 = call(True)
    x0, f0, e0, lam0 = call(False)
    assert (e1 == 1).all(), e1
    assert np.abs(lam1[0]).max() > 0
    assert np.array_equal(x1, x0) and np.array_equal(e1, e0) and np.array_equal(f1, f0)
    assert not any(a.any() for a in lam0)


def test_workspace_regrowth(lmpc, states):
    """one handle through MG N = 20 at batch 5, 3, 7 with the double-integrator problem (another
    layout in the same buffers) in between: every result equals a fresh handle's"""
    import bqp
    di = golden('di_design.npz')
    tm = bqp.TrackingMPC(di['A'], di['B'], di['Q'], di['R'], di['P'], di['T'], di['LAMBDA'],
                         di['PSI'], di['F_x'], di['h_x'], di['F_u'], di['h_u'], di['F_T'],
                         di['h_T'], N=int(di['N']))
    gi = np.arange(4)   # the first instances of config C3's grid (tests/test_gpu_ocp.py)
    Xd, XSd = di['x0'][gi // len(di['xs'])], di['xs'][gi % len(di['xs'])]

    def mg_solve(h, nb):
        return bqp.solve_ocp(lmpc.prob, states[:nb], handle=h, want_duals=True)

    def di_solve(h, nb):
        return tm.solve(Xd[:nb], XSd[:nb], handle=h)

    steps = [(mg_solve, 5), (di_solve, 4), (mg_solve, 3), (di_solve, 4), (mg_solve, 7)]
    used = bqp.Handle(0)
    for solve, nb in steps:
        r, ref = solve(used, nb), solve(bqp.Handle(0), nb)
        arrays = [k for k in ref if isinstance(ref[k], np.ndarray)]
        assert {'x', 'u', 'theta', 'exitflag', 'iterations'} <= set(arrays)
        assert (ref['iterations'] > 0).all()
        if solve is mg_solve:
            assert (ref['exitflag'] == 1).all(), ref['exitflag']
        for k in arrays:
            assert np.array_equal(r[k], ref[k], equal_nan=True), (solve.__name__, nb, k)
