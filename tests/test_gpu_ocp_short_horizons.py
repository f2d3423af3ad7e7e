"""The Riccati sweeps at horizons shorter than, and around, their refill distance.  The backward and
forward sweeps of the stage wave (bqp_ocp.hip solve()) keep two register sets that are refilled two
stages ahead with a clamped stage index, whole stage pairs in the loop and the single stage of an
odd N after it, so N = 1 (no trip, only the single stage), 2 (one trip, every refill clamped), 3, 4
and 5 each take a different way through them; both compiled families, (4, 1, 1) and (2, 2, 2).

Instances: box-constrained problems built from the golden designs - the MG F1 problem for N >= 2
(at N = 1 it has no box row left: boxes sit on x_1..x_{N-1}, u_0..u_{N-2}), the MG tracking problem
(boxes on every x_k, k >= 1, and every u_k) for N = 1..5, and the DI tracking problem for N = 1..5.
The GPU is held to the C restatement of the same iteration (oracle/cpu_ipm.c): equal exit flags,
equal iteration counts, and per instance |z - z*|_inf <= 1e-8 max(1, |z*|_inf) over the whole
z = [x; u; theta] (the measure of DESIGN.md section 1).  The figures per array are printed beside it:
the DI tracking problem has no cost on u_{N-1}, its last input is only weakly determined, and at
N = 4 one state measures |du|_inf = 1.43e-8 at |u| <= 0.3, |dx|_inf = 7e-9 at |x| up to 5
(2.2e-9 .. 5.8e-9 in the measure above); every other case is below 5e-10, most at 1e-14.

Choice of states, made from the C restatement alone: of the first 64 candidate states a case keeps
the first 16 that (a) end with flag 1 unpolished, and (b) end with the same flag after the same
number of iterations when all three stopping tolerances are scaled by 4 and by 1/4.  (b) keeps the
comparison of iteration counts meaningful: GPU and C iterates differ by rounding order (1e-11
median), which can only move the stop by an iteration where a residual sits within that distance of
its threshold; a state whose stop does not move under a factor 4 either way is not such a state.
Every case must find its 16 states (asserted on the CPU side before the GPU runs)."""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

TOL = 1e-8
NSEL = 16
TOLS = dict(tol_stat=1e-8, tol_feas=1e-10, tol_comp=1e-14)     # the solver's defaults


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


def _ocp_dict(p):
    return dict(nx=p.nx, nu=p.nu, np=p.np, N=p.N, A=p.A, B=p.B, c=p.c, W=p.W, w=p.w, xlb=p.xlb,
                xub=p.xub, ulb=p.ulb, uub=p.uub, Fp=p.Fp, hp=p.hp, kp=p.poly_stage)


def _case(mg, ts, form, N):
    """(problem, candidate states, per-instance linear terms or None)"""
    import bqp
    if form == 'mg_f1':
        pr = bqp.LMPC(mg['A'], mg['B'], mg['K'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'],
                      mg['LAMBDA'], mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'],
                      ts[0], ts[1], N=N).prob
        return pr, golden('lmpc_N20.npz')['dx'][:64], None
    if form == 'mg_track':
        pr = bqp.TrackingLMPC(mg['A'], mg['B'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'],
                              mg['LAMBDA'], mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'],
                              ts[0], ts[1], mg['x_wp'], mg['u_wp'], N=N).prob
        g = golden('dms_DSS_tLMPC.npz')
        return pr, g['x'][:64] - np.asarray(mg['x_wp'], float).ravel(), None
    di = golden('di_design.npz')
    tm = bqp.TrackingMPC(di['A'], di['B'], di['Q'], di['R'], di['P'], di['T'], di['LAMBDA'],
                         di['PSI'], di['F_x'], di['h_x'], di['F_u'], di['h_u'], di['F_T'],
                         di['h_T'], N=N)
    gi = (np.arange(64) * 61) % (len(di['x0']) * len(di['xs']))
    X, XS = di['x0'][gi // len(di['xs'])], di['xs'][gi % len(di['xs'])]
    return tm.prob, X, tm.linear_terms(XS)[0]


def _select(ocp, X, w):
    """indices of the first NSEL candidates whose C-restatement solve ends with flag 1, unpolished,
    at an iteration count that does not move with the stopping tolerances (x4, /4); and that solve"""
    from oracle import cpu_ref
    c = cpu_ref.solve(ocp, X, w=w, **TOLS)
    keep = (c['exitflag'] == 1) & (c['polished'] == 0)
    for s in (4.0, 0.25):
        cs = cpu_ref.solve(ocp, X, w=w, **{k: v * s for k, v in TOLS.items()})
        keep &= (cs['exitflag'] == 1) & (cs['iterations'] == c['iterations'])
    idx = np.flatnonzero(keep)[:NSEL]
    return idx, {k: v[idx] for k, v in c.items()}


CASES = [('mg_f1', N) for N in (2, 3, 4, 5)] + [('mg_track', N) for N in (1, 2, 3, 4, 5)] + \
        [('di_track', N) for N in (1, 2, 3, 4, 5)]


@pytest.mark.parametrize('form,N', CASES, ids=['%s-N%d' % c for c in CASES])
def test_short_horizon_vs_cpu_restatement(mg, term_set, handle, form, N):
    import bqp
    pr, X, w = _case(mg, term_set, form, N)
    assert np.isfinite(pr.ulb).any() and np.isfinite(pr.uub).any()      # box-constrained
    idx, c = _select(_ocp_dict(pr), X, w)
    assert len(idx) == NSEL, 'only %d states pass the selection' % len(idx)
    assert (c['exitflag'] == 1).all()
    r = bqp.solve_ocp(pr, X[idx], w=None if w is None else w[idx], handle=handle,
                      route='structured')
    zg = np.concatenate([r[k].reshape(NSEL, -1) for k in ('x', 'u', 'theta')], axis=1)
    zc = np.concatenate([c[k].reshape(NSEL, -1) for k in ('x', 'u', 'theta')], axis=1)
    err = np.abs(zg - zc).max(axis=1) / np.maximum(1.0, np.abs(zc).max(axis=1))
    per = {k: np.abs(r[k] - c[k]).max() for k in ('x', 'u', 'theta')}
    print('%s N=%d: flags %s, iterations gpu %s cpu %s, max rel err %.2e, max |diff| per array %s' % (
        form, N, r.exitflag.tolist(), r.iterations.tolist(), c['iterations'].tolist(), err.max(),
        {k: '%.2e' % v for k, v in per.items()}))
    assert np.array_equal(r.exitflag, c['exitflag'])
    assert np.array_equal(r.iterations, c['iterations'])
    assert err.max() <= TOL, err
