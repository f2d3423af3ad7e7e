"""The Riccati factorisation with P_k in lanes (bqp_ocp.hip factor(), FACTOR_ROWS), in the solve.  The
fp64 kernels at one stage per lane keep P_{k+1} in one register per lane of every 16-lane row and
store P_k, K_k and the factors from all lanes; the later passes read those tables as before.  Cases
the sweep-edge tests do not have:
 - MG and DI tracking problems at N = 20 and 21, the last horizon with three lane groups on the
   per-stage passes (3 * 21 <= 64) and the first without;
 - the per-stage-model kernel at N = 21 (the problem's own model at every stage);
 - MG F1 at N = 20 on eight stored states that the C restatement polishes: the repair kernel runs
   factor() once per polish round, from the branch of a new active set.  At the default polish level
   (after 0 / -8 exits) the restatement polishes none of the 1000 stored states - all end with flag
   1 - so the case runs both sides at polish level 2 (also with weakly active rows), where it polishes
   48 of them.  The selection is the sweep-edge tests' rule with "polished" in the place of
   "unpolished": flag 1 polished, and the same flag, mark and iteration count with the three
   stopping tolerances scaled by 4 and by 1/4 (26 states; eight are asserted to exist).  Without
   the second part the first eight polished states stop an iteration apart on the GPU and in the
   restatement on four of them, and the GPU keeps the IPM iterate on two (those marks differ with
   the quad / LDS form of the factorisation too).  The polish marks are printed beside the bar;
 - a first factorisation that fails: the MG tracking problem at N = 20 with the input weight set to
   -1e3 at every stage, so that R^_{N-1} = R + B' P_N B < 0.  The C restatement returns flag -8 after 0
   iterations for every state (asserted on the CPU side); the bar is the same flag.

Problems, selection rule and bars are those of test_gpu_ocp_sweep_edges.py (its _select and
_compare): against the C restatement of the iteration (oracle/cpu_ipm.c) equal exit flags, equal
iteration counts and per instance |z - z*|_inf <= 1e-8 max(1, |z*|_inf) over z = [x; u; theta]; eight
states per case chosen from the C restatement alone."""
import copy

import numpy as np
import pytest

from conftest import golden
from test_gpu_ocp_short_horizons import TOLS, _case, _ocp_dict
from test_gpu_ocp_sweep_edges import NSEL, _compare, _select

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


CASES = [('mg_track', 20), ('mg_track', 21), ('di_track', 20), ('di_track', 21)]


@pytest.mark.parametrize('form,N', CASES, ids=['%s-N%d' % c for c in CASES])
def test_factor_rows_vs_cpu_restatement(mg, term_set, handle, form, N):
    import bqp
    pr, X, w, c = _select(mg, term_set, form, N)
    assert (c['exitflag'] == 1).all()
    r = bqp.solve_ocp(pr, X, w=w, handle=handle, route='structured')
    _compare('%s N=%d' % (form, N), r, c)


def test_factor_rows_per_stage_models(mg, term_set, handle):
    """the per-stage-model kernel on the problem's own model at every stage: the same problem, so
    the same C restatement"""
    import bqp
    N = 21
    pr, X, w, c = _select(mg, term_set, 'mg_track', N)
    r = bqp.solve_ocp(pr, X, w=w, A=np.tile(pr.A, (N, 1, 1)), B=np.tile(pr.B, (N, 1, 1)),
                      stage_models=True, handle=handle)
    _compare('mg_track N=%d, per-stage models' % N, r, c)


def test_factor_rows_polished_states(mg, term_set, handle):
    """the repair kernel's factorisations (one per polish round), on states the C restatement polishes"""
    import bqp
    from oracle import cpu_ref
    pr, X, _ = _case(mg, term_set, 'mg_f1', 20)
    X = golden('lmpc_N20.npz')['dx']          # all stored states, not the first 64
    ocp = _ocp_dict(pr)
    c = cpu_ref.solve(ocp, X, polish=2, **TOLS)
    keep = (c['exitflag'] == 1) & (c['polished'] == 1)
    for s in (4.0, 0.25):
        cs = cpu_ref.solve(ocp, X, polish=2, **{k: v * s for k, v in TOLS.items()})
        keep &= (cs['exitflag'] == 1) & (cs['polished'] == 1) & (cs['iterations'] == c['iterations'])
    idx = np.flatnonzero(keep)[:NSEL]
    assert len(idx) == NSEL, 'the C restatement polishes only %d states that pass the selection' % len(idx)
    c = {k: v[idx] for k, v in c.items()}
    r = bqp.solve_ocp(pr, X[idx], handle=handle, route='structured', polish=2)
    print('polished: gpu %s cpu %s' % (r.polished.tolist(), c['polished'].tolist()))
    _compare('mg_f1 N=20, polished', r, c)


def test_factor_rows_failed_first_factorisation(mg, term_set, handle):
    """R^_{N-1} < 0: the first factorisation fails, flag -8 after 0 iterations on both sides"""
    import bqp
    from oracle import cpu_ref
    pr, X, w = _case(mg, term_set, 'mg_track', 20)
    pr = copy.copy(pr)
    nx, nu = pr.nx, pr.nu
    pr.W = pr.W.copy()
    pr.W[:, nx:nx + nu, nx:nx + nu] = -1e3 * np.eye(nu)
    X = X[:NSEL]
    c = cpu_ref.solve(_ocp_dict(pr), X, w=w, **TOLS)
    assert (c['exitflag'] == -8).all() and (c['iterations'] == 0).all(), (c['exitflag'], c['iterations'])
    r = bqp.solve_ocp(pr, X, w=w, handle=handle, route='structured')
    print('failed first factorisation: gpu flags %s iterations %s' % (r.exitflag.tolist(), r.iterations.tolist()))
    assert np.array_equal(r.exitflag, c['exitflag'])
