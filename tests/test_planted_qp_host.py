"""CPU checks of the planted QPs (tests/planted_qp.py) that tests/test_gpu_quadprog_planted.py
solves on the GPU: the generator's own KKT / LICQ guarantees in longdouble, each case landing on
the kernel form its table names (launch_dense's predicates, restated in planted_qp), and the
algorithm statement oracle/dense_ipm.py reaching every planted optimum at least 10 x inside the
GPU bars (x 1e-9 against 1e-8, multipliers 1e-7 against 1e-6) - so a GPU miss is the kernel's."""
import os
import re

import numpy as np
import pytest

import planted_qp as pq
from conftest import PKG

ALL = pq.TABLE + pq.TRUNCATED + [pq.FIXED]
STRIDES = [(c, k) for c in pq.STRIDE_SHAPES for k in pq.STRIDE_PER]


def _ids(cases):
    return [pq.case_id(c) for c in cases]


def _check_planted(q, s):
    n = q['H'].shape[0]
    scale = max([1.0, np.abs(q['f']).max()] + [np.abs(q[k]).max() for k in ('b', 'beq') if q[k] is not None])
    stat, viol, comp, neg = pq.kkt_residuals(q, s)
    assert stat <= 1e-13 * scale and viol <= 1e-13 * scale and comp <= 1e-13 * scale, (stat, viol, comp)
    assert neg >= 0.0
    assert pq.strict_complementarity(q, s) >= 0.2 - 1e-12
    assert s['licq'] >= pq.LICQ_MIN
    ar, au, al = s['active']
    me = 0 if q['Aeq'] is None else q['Aeq'].shape[0]
    assert 1 <= len(ar) + len(au) + len(al) and len(ar) + len(au) + len(al) + me + len(s['fixed']) <= n
    assert not set(au) & set(al)
    for k, v in (('ineqlin', ar), ('upper', au), ('lower', al)):
        lam = s[k][v]
        assert ((lam >= 0.5) & (lam <= 2.0)).all()


def _check_statement(q, s, r):
    assert r['exitflag'] == 1
    ex, el = pq.errors(r, s)
    assert ex <= 1e-9, ex
    assert max(el.values()) <= 1e-7, el
    fv = pq.fval_exact(q, s)
    assert abs(r['fval'] - fv) <= 1e-9 * max(1.0, abs(fv))


def test_predicates_match_the_kernel_source():
    """the constants restated in planted_qp are the ones csrc/bqp_dense.hip is compiled with"""
    src = open(os.path.join(PKG, 'csrc', 'bqp_dense.hip')).read()

    def define(name):
        v = re.search(r'#define\s+%s\s+(.+?)\s*(//.*)?$' % name, src, re.M).group(1)
        return int(eval(v, {'DQ_THL': pq.DQ_THL}))
    for name in ('DT', 'TILE', 'DQ_THL', 'DQ_RPT', 'DQ_GB', 'DQ_NVEC', 'DQ_TAIL', 'DENSE_LDS_MAX', 'SW_NMAX',
                 'SW_LDS_MAX', 'SW_A_LDS_MAX', 'DQ_POL_KLDS'):
        assert define(name) == getattr(pq, name), name
    assert 'return 2 * n * n + 8 * n + 12 * n + 8 * m + (m * n <= SW_A_LDS_MAX ? m * n : 0);' in src
    assert 'return 32 * ((n + 31) / 32) + 1;' in src


@pytest.mark.parametrize('c', ALL + pq.STRIDE_SHAPES, ids=_ids(ALL + pq.STRIDE_SHAPES))
def test_case_lands_on_its_kernel_form(c):
    assert pq.kernel_form(c['n'], c['m'], c['me']) == c['form']


def test_dispatch_edges():
    """the edges the table sits on, read off the predicates"""
    kf = pq.kernel_form
    assert (kf(16, 64, 0), kf(17, 65, 0), kf(32, 688, 0), kf(32, 689, 0)) == ('wave1', 'wave2', 'wave2', 'regs')
    assert kf(33, 130, 0) == 'regs' and kf(12, 30, 0) == 'wave1' and kf(12, 30, 3) == 'regs'
    assert pq.wave_a_in_lds(16, 256) and not pq.wave_a_in_lds(16, 257)
    assert pq.wave_a_in_lds(32, 128) and not pq.wave_a_in_lds(32, 129)
    # rows in registers: m <= 1024 and n <= 101 (102 .. 108 keep the two A'DA buffers but not
    # the 17 n-vectors in LDS; 109 .. 122 one row tile; from 123 the factor leaves LDS)
    assert (kf(101, 1024, 0), kf(101, 1025, 0), kf(102, 1024, 0)) == ('regs', 'lds', 'lds')
    assert pq.dense_glds(108) and not pq.dense_glds(109)
    assert (kf(122, 161, 4), kf(123, 161, 7)) == ('lds', 'work')
    assert kf(40, 0, 0) == 'lds'
    assert not pq.atw_tiled(109, 300) and pq.atw_tiled(109, 4100) and pq.atw_tiled(40, 8192)
    assert pq.polish_k_in_lds(128) and not pq.polish_k_in_lds(129)
    assert 8192 == pq.TILE * pq.DQ_THL and 8161 == 8192 - 31
    assert kf(256, 40, 200) == 'work' and kf(257, 1, 0) is None and kf(4, 1, 257) is None and kf(4, 8193, 0) is None


def test_patterns():
    """'stair': the row ends of the issue's list, four tiles with bound <= 16, an all-zero tile,
    interior zeros inside the rows; 'causal': every row ends at column n while most of it is zero"""
    rng = np.random.default_rng(0)
    n, m = 40, 300
    A, prio = pq.make_A(rng, n, m, 'stair')
    hr = np.array([np.flatnonzero(r).max() + 1 if r.any() else 0 for r in A])
    assert hr[:10].tolist() == [0, 1, 15, 16, 17, 31, 32, 33, 39, 40]
    assert hr[128:256].max() <= 16 and hr[128:256].min() >= 1 and (hr[256:288] == 0).all()
    assert hr[288:].max() > 16
    j = n // 3
    odd = np.arange(m) % 2 == 1
    assert (A[odd, j] == 0).all() and (hr[odd] > j + 1).any() and (A[~odd & (hr > j), j] != 0).all()
    assert set(range(10)) <= set(prio) and len(prio) == 14
    A15, _ = pq.make_A(rng, 15, 33, 'stair')
    assert max(np.flatnonzero(r).max() + 1 if r.any() else 0 for r in A15[:10]) == 15
    C, _ = pq.make_A(rng, 21, 806, 'causal', nu=1, npar=1)
    assert (C[:, -1] != 0).all() and (C == 0).mean() > 0.4
    assert (C[0, 1:-1] == 0).all() and C[0, 0] != 0 and (C[-1] != 0).all()


@pytest.mark.parametrize('c', ALL, ids=_ids(ALL))
def test_generator_kkt_and_statement(c):
    args, sols, qs = pq.case_batch(c)
    for i, (q, s) in enumerate(zip(qs, sols)):
        _check_planted(q, s)
        _check_statement(q, s, pq.case_statement(c, i))
    if c['pattern'] == 'stair' and c['m'] >= 10:
        assert any(r < 10 for s in sols for r in s['active'][0])      # a staircase head row binds
    if c['pattern'] == 'stair' and c['m'] >= 256:
        assert any(128 <= r < 256 for s in sols for r in s['active'][0])


@pytest.mark.parametrize('c,k', STRIDES, ids=['%s-%s' % (pq.case_id(c), k) for c, k in STRIDES])
def test_stride_batches(c, k):
    per = pq.STRIDE_PER[k]
    args, sols, qs = pq.case_batch(c, batch=5, per=per, salt=1)
    for name in ('H', 'A', 'Aeq', 'lb', 'ub'):
        if args[name] is not None:
            want = {'H': 2, 'A': 2, 'Aeq': 2, 'lb': 1, 'ub': 1}[name] + (name in per)
            assert args[name].ndim == want, name
            if name in per:
                assert not np.array_equal(args[name][0], args[name][1])
    assert not np.array_equal(sols[0]['z'], sols[1]['z'])
    for i, (q, s) in enumerate(zip(qs, sols)):
        _check_planted(q, s)
        _check_statement(q, s, pq.case_statement(c, i, batch=5, per=per, salt=1))


def test_fixed_case_has_both_signs():
    args, sols, qs = pq.case_batch(pq.FIXED)
    for q, s in zip(qs, sols):
        jf = s['fixed']
        assert jf.size == 3 and (q['lb'][jf] == q['ub'][jf]).all()
        assert (s['upper'][jf] > 0).any() and (s['lower'][jf] > 0).any()
        assert ((s['upper'][jf] > 0) ^ (s['lower'][jf] > 0)).all()


@pytest.mark.parametrize('c', pq.TRUNCATED, ids=_ids(pq.TRUNCATED))
def test_truncated_statement_is_polished_to_the_optimum(c):
    """three iterations short of its exit the statement ends 0, and its active-set polish lands on
    z* (a direct KKT solve): flag 1, polished, 10 x inside the GPU test's 1e-10; without the polish
    the iterate is not within 1e-10 - what the GPU test of the polish kernel relies on"""
    k = pq.truncation_k(c)
    assert k >= 1
    args, sols, qs = pq.case_batch(c)
    for i, s in enumerate(sols):
        r = pq.case_statement(c, i, max_iter=k)
        assert r['exitflag'] == 1 and r['polished']
        assert np.abs(r['x'] - s['z']).max() <= 1e-11
        r0 = pq.case_statement(c, i, max_iter=k, polish=False)
        assert r0['exitflag'] == 0 and not r0['polished']
        assert np.abs(r0['x'] - s['z']).max() > 1e-10
