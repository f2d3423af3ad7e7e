"""bqp.quadprog against planted optima (tests/planted_qp.py: z* and every multiplier known by
construction, no solver in the reference) at every shape where launch_dense or a kernel changes
path: the two wave kernels, the three workgroup forms, the polish with K in LDS / the workspace,
the A staging, MFMA row-group, row-sparsity and tile-bound edges, per-instance strides, fixed
variables and the entry point's limits.

Bars (tests/test_planted_qp_host.py holds the algorithm statement 10 x inside each):
    x                       |x - z*|_inf <= 1e-8 max(1, |z*|_inf)   (the suite's bar of this entry point)
    every multiplier field  <= 1e-6 max(1, |lam*|_inf)              (the suite's stationarity bar)
    fval                    1e-8 relative, against 0.5 z*'Hz* + f'z* in longdouble
    x after the polish      1e-10: a direct KKT solve, 100 x tighter than the IPM's exit
Iteration counts, GPU against statement, are printed and not asserted: rounding moves them
between the separately compiled forms (test_dense_rows_in_registers_equals_workspace_form)."""
import os

import numpy as np
import pytest

import planted_qp as pq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def handle():
    import bqp
    return bqp.Handle(0)


def _solve(args, handle, **options):
    import bqp
    x, fval, flag, out, lam = bqp.quadprog(handle=handle, options=options or None, **args)
    return dict(x=x, fval=fval, flag=flag, out=out, lam=lam)


def _inst(g, i):
    return dict(x=g['x'][i], **{k: g['lam'][k][i] for k in pq.FIELDS})


def _check(name, form, g, sols, qs, its_statement, xbar=1e-8):
    """print the measured distances, then assert flag 1 and the bars on every instance"""
    ex, el = zip(*[pq.errors(_inst(g, i), s) for i, s in enumerate(sols)])
    worst = max(max(e.values()) for e in el)
    print('PLANTED | %s | %s | %s / %s | %.1e | %.1e |' % (
        name, form, '/'.join(map(str, g['out']['iterations'])), '/'.join(map(str, its_statement)),
        max(ex), worst))
    assert (g['flag'] == 1).all(), g['flag']
    assert max(ex) <= xbar, ex
    for e in el:
        assert max(e.values()) <= 1e-6, e
    for i, (q, s) in enumerate(zip(qs, sols)):
        fv = pq.fval_exact(q, s)
        assert abs(g['fval'][i] - fv) <= 1e-8 * max(1.0, abs(fv))


def _its(c, nb=3, **kw):
    return [pq.case_statement(c, i, **kw)['iterations'] for i in range(nb)]


@pytest.mark.parametrize('c', pq.TABLE, ids=[pq.case_id(c) for c in pq.TABLE])
def test_dispatch_table(c, handle):
    args, sols, qs = pq.case_batch(c)
    _check(pq.case_id(c), c['form'], _solve(args, handle), sols, qs, _its(c))


def test_limits_answer_without_a_launch(handle):
    """n = 257, me = 257 and m = 8193 are refused by the host entry's dimension check (no kernel
    is launched); the handle solves the first table case correctly afterwards"""
    import bqp
    with pytest.raises(bqp.BqpError):
        bqp.quadprog(np.eye(257), np.zeros(257), handle=handle)
    with pytest.raises(bqp.BqpError):
        bqp.quadprog(np.eye(4), np.zeros(4), Aeq=np.zeros((257, 4)), beq=np.zeros(257), handle=handle)
    with pytest.raises(bqp.BqpError):
        bqp.quadprog(np.eye(4), np.zeros(4), A=np.zeros((8193, 4)), b=np.ones(8193), handle=handle)
    c = pq.TABLE[0]
    args, sols, qs = pq.case_batch(c)
    _check('after the refusals: ' + pq.case_id(c), c['form'], _solve(args, handle), sols, qs, _its(c))


STRIDES = [(c, k) for c in pq.STRIDE_SHAPES for k in pq.STRIDE_PER]


@pytest.mark.parametrize('c,k', STRIDES, ids=['%s-%s' % (pq.case_id(c), k) for c, k in STRIDES])
def test_strides(c, k, handle):
    """batch 5; per instance: only f and b / everything / H and lb (A and ub shared) - each
    instance against its own planted optimum"""
    per = pq.STRIDE_PER[k]
    args, sols, qs = pq.case_batch(c, batch=5, per=per, salt=1)
    its = [pq.case_statement(c, i, batch=5, per=per, salt=1)['iterations'] for i in range(5)]
    _check('%s strides %s' % (pq.case_id(c), k), c['form'], _solve(args, handle), sols, qs, its)


@pytest.mark.parametrize('c', pq.TRUNCATED, ids=[pq.case_id(c) for c in pq.TRUNCATED])
def test_polish_after_truncated_solve(c, handle):
    """max_iter three short of the statement's exit: the IPM ends 0 and dense_polish_kernel (K in
    LDS up to n = 128, in the workspace above) must land on z* - flag 1, polished, 1e-10.  With the
    polish off the same call returns flag 0 and an x that is not within 1e-10 of z*: the first
    assertion tests the polish kernel, not the IPM."""
    k = pq.truncation_k(c)
    args, sols, qs = pq.case_batch(c)
    g = _solve(args, handle, max_iter=k)
    g0 = _solve(args, handle, max_iter=k, polish=-1)
    Z = np.stack([s['z'] for s in sols])
    print('max_iter %d: polished %s, |x - z*| %.1e; polish off: flags %s, |x - z*| %s' % (
        k, g['out']['polished'], np.abs(g['x'] - Z).max(), g0['flag'], np.abs(g0['x'] - Z).max(axis=1)))
    assert (g['out']['polished'] == 1).all(), g['out']['polished']
    assert np.abs(g['x'] - Z).max() <= 1e-10
    _check(pq.case_id(c) + ' polished', c['form'], g, sols, qs, _its(c, max_iter=k))
    assert (g0['flag'] == 0).all() and (g0['out']['polished'] == 0).all()
    assert (np.abs(g0['x'] - Z).max(axis=1) > 1e-10).all()


def test_fixed_variables(handle):
    """lb == ub on three variables: the shim's equality rows; their multipliers come back on
    lam.lower / lam.upper by sign and lam.eqlin keeps the genuine equality rows only"""
    c = pq.FIXED
    args, sols, qs = pq.case_batch(c)
    g = _solve(args, handle)
    _check(pq.case_id(c), c['form'], g, sols, qs, _its(c))
    assert g['lam']['eqlin'].shape == (3, c['me'])
    for i, s in enumerate(sols):
        jf = s['fixed']
        assert np.abs(g['lam']['lower'][i][jf] - s['lower'][jf]).max() <= 1e-6 * 2.0
        assert np.abs(g['lam']['upper'][i][jf] - s['upper'][jf]).max() <= 1e-6 * 2.0
        assert np.abs(g['lam']['eqlin'][i] - s['eqlin']).max() <= 1e-6 * 2.0
        assert np.abs(g['x'][i][jf] - qs[i]['lb'][jf]).max() <= 1e-8


def test_learned_loop_shape_in_both_compilations(handle):
    """n = 101, m = 1024 (the learned loop's SQP sub-problem): the register form and, under
    BQP_DENSE_NO_RG=1, the workspace form are pinned to the same planted optimum"""
    c = [c for c in pq.TABLE if (c['n'], c['m']) == (101, 1024)][0]
    args, sols, qs = pq.case_batch(c)
    _check(pq.case_id(c), 'regs', _solve(args, handle), sols, qs, _its(c))
    os.environ['BQP_DENSE_NO_RG'] = '1'
    try:
        g = _solve(args, handle)
    finally:
        del os.environ['BQP_DENSE_NO_RG']
    _check(pq.case_id(c) + ' NO_RG', 'lds', g, sols, qs, _its(c))
