"""The Riccati sweeps' loop edges in the solve.  The fp64 sweeps of the stage wave (bqp_ocp.hip solve())
walk per-lane offsets through the stages, run the trips whose refills exist in a loop and the last
stage pair behind it, and store from all lanes at one stage per lane (N + 1 <= 64) and from row 0's
lanes < NS at two: N = 1 (the single stage alone), 2 (the peeled pair alone), 3, 4 (the first trip
in the loop), 5, 6, and for MG N = 63 and 64, the last horizon with the all-lane store and the first
with the guarded one.  Both compiled families, (4, 1, 1) and (2, 2, 2), and the per-stage-model
kernels (stage_models = 1, the problem's own model repeated over the stages) at N = 2 and 5.

Problems, measure and bars are those of test_gpu_ocp_short_horizons.py (its _case): the MG and DI
tracking problems at N = 1..6, the MG F1 problem at N = 63 and 64; against the C restatement of the
iteration (oracle/cpu_ipm.c) equal exit flags, equal iteration counts and per instance
|z - z*|_inf <= 1e-8 max(1, |z*|_inf) over z = [x; u; theta].  Eight states per case, chosen from the
C restatement alone by that test's rule: flag 1 unpolished, and the same flag after the same number
of iterations with the three stopping tolerances scaled by 4 and by 1/4.  The C solves of a case are
shared between its one-model and its per-stage-model test."""
import numpy as np
import pytest

from test_gpu_ocp_short_horizons import TOL, TOLS, _case, _ocp_dict

pytestmark = pytest.mark.gpu

NSEL = 8


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


_sel = {}


def _select(mg, ts, form, N):
    """(problem, states, linear terms or None, C-restatement solve) of the case's NSEL states"""
    if (form, N) not in _sel:
        from oracle import cpu_ref
        pr, X, w = _case(mg, ts, form, N)
        ocp = _ocp_dict(pr)
        c = cpu_ref.solve(ocp, X, w=w, **TOLS)
        keep = (c['exitflag'] == 1) & (c['polished'] == 0)
        for s in (4.0, 0.25):
            cs = cpu_ref.solve(ocp, X, w=w, **{k: v * s for k, v in TOLS.items()})
            keep &= (cs['exitflag'] == 1) & (cs['iterations'] == c['iterations'])
        idx = np.flatnonzero(keep)[:NSEL]
        assert len(idx) == NSEL, 'only %d states pass the selection' % len(idx)
        _sel[(form, N)] = (pr, X[idx], None if w is None else w[idx], {k: v[idx] for k, v in c.items()})
    return _sel[(form, N)]


def _compare(tag, r, c):
    zg = np.concatenate([r[k].reshape(NSEL, -1) for k in ('x', 'u', 'theta')], axis=1)
    zc = np.concatenate([c[k].reshape(NSEL, -1) for k in ('x', 'u', 'theta')], axis=1)
    err = np.abs(zg - zc).max(axis=1) / np.maximum(1.0, np.abs(zc).max(axis=1))
    print('%s: flags %s, iterations gpu %s cpu %s, max rel err %.2e' % (
        tag, r.exitflag.tolist(), r.iterations.tolist(), c['iterations'].tolist(), err.max()))
    assert np.array_equal(r.exitflag, c['exitflag'])
    assert np.array_equal(r.iterations, c['iterations'])
    assert err.max() <= TOL, err


CASES = [('mg_track', N) for N in (1, 2, 3, 4, 5, 6)] + [('di_track', N) for N in (1, 2, 3, 4, 5, 6)] + \
        [('mg_f1', 63), ('mg_f1', 64)]


@pytest.mark.parametrize('form,N', CASES, ids=['%s-N%d' % c for c in CASES])
def test_sweep_edges_vs_cpu_restatement(mg, term_set, handle, form, N):
    import bqp
    pr, X, w, c = _select(mg, term_set, form, N)
    assert (c['exitflag'] == 1).all()
    r = bqp.solve_ocp(pr, X, w=w, handle=handle, route='structured')
    _compare('%s N=%d' % (form, N), r, c)


@pytest.mark.parametrize('N', [2, 5])
def test_sweep_edges_per_stage_models(mg, term_set, handle, N):
    """the per-stage-model kernel on the problem's own model at every stage: the same problem, so
    the same C restatement"""
    import bqp
    pr, X, w, c = _select(mg, term_set, 'mg_track', N)
    r = bqp.solve_ocp(pr, X, w=w, A=np.tile(pr.A, (N, 1, 1)), B=np.tile(pr.B, (N, 1, 1)),
                      stage_models=True, handle=handle)
    _compare('mg_track N=%d, per-stage models' % N, r, c)
