"""CPU: the numpy reference of the per-stage-model solve (tests/ltv_ref.py) against the project's
own condensed form, the cases of the GPU test (tests/ltv_cases.py), and the Python packing of the
per-stage arrays (bqp.ocp.pack) - no GPU and no library call."""
import ctypes as C

import numpy as np
import pytest

import ltv_cases
import ltv_ref


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize('family,N', [('mg', 20), ('di', 30)])
def test_equal_models_reproduce_condensed_form(family, N):
    """all A_k = A, B_k = B, c_k = c: ltv_ref's (H, f, A, b) are bqp.condense.Condensed's."""
    from bqp.condense import Condensed
    prob = ltv_cases.mg_prob(N) if family == 'mg' else ltv_cases.di_prob(N)
    prob.c = 1e-3 * np.arange(1, prob.nx + 1)           # a non-zero affine term
    cd = Condensed(prob)
    X = ltv_cases.states(family, 3, 0)
    f, b = cd.rhs(X)
    for i in range(3):
        qp = ltv_ref.condense(prob, X[i], np.tile(prob.A, (N, 1, 1)), np.tile(prob.B, (N, 1, 1)),
                              np.tile(prob.c, (N, 1)))
        assert qp['A'].shape == cd.A.shape
        assert _rel(qp['H'], cd.H) < 1e-12
        assert _rel(qp['f'], f[i]) < 1e-12
        assert _rel(qp['A'], cd.A) < 1e-12
        assert _rel(qp['b'], b[i]) < 1e-12


@pytest.mark.parametrize('family,N', sorted(ltv_cases.SEEDS))
def test_cases_are_feasible(family, N):
    """every instance of every GPU case has an exact optimum, and it satisfies the dense KKT
    conditions with the schedule's own models"""
    cs = ltv_cases.case(family, N)
    for i, r in enumerate(cs['ref']):
        assert r['status'] == 'optimal', (family, N, i)
        qp = r['qp']
        g = qp['H'] @ r['z'] + qp['f'] + qp['A'].T @ r['lam']
        assert np.abs(g).max() <= 1e-9 * (1 + np.abs(qp['H'] @ r['z'] + qp['f']).max())
        assert (qp['A'] @ r['z'] - qp['b']).max() <= 1e-10
        # the states of the reference follow the per-stage models
        x = r['x']
        for k in range(N):
            xn = cs['A'][i, k] @ x[k] + cs['B'][i, k] @ r['u'][k] + cs['c'][i, k]
            assert np.abs(xn - x[k + 1]).max() <= 1e-12 * max(1.0, np.abs(x).max())


def test_pack_shapes_and_strides():
    from bqp import ocp
    prob = ltv_cases.mg_prob(6)
    N, nx, nu = 6, 4, 1
    X = ltv_cases.states('mg', 3, 0)
    A, B, c = ltv_cases.schedules(prob, 3, 5)

    def blocks(ptr, n):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), (n,)).copy()

    # one model: today's call, six positional fields' worth of meaning
    d, D, batch, keep = ocp.pack(prob, X)
    assert (d.stage_models, D.sA, D.sB, D.sc) == (0, 0, 0, 0) and not D.skip
    d, D, _, keep = ocp.pack(prob, X, A=A[:, 0], B=B[:, 0])
    assert (d.stage_models, D.sA, D.sB) == (0, nx * nx, nx * nu)
    # a schedule shared by the batch
    d, D, _, keep = ocp.pack(prob, X, A=A[0], B=B[0], c=c[0])
    assert (d.stage_models, D.sA, D.sB, D.sc) == (1, 0, 0, 0)
    a = blocks(D.A, N * nx * nx).reshape(N, nx, nx)
    assert np.array_equal(a, np.swapaxes(A[0], 1, 2))           # column-major blocks, stage-major
    # per instance; a missing c is prob's repeated, shared
    d, D, _, keep = ocp.pack(prob, X, A=A, B=B)
    assert (d.stage_models, D.sA, D.sB, D.sc) == (1, N * nx * nx, N * nx * nu, 0)
    assert np.array_equal(blocks(D.B, 3 * N * nx * nu).reshape(3, N, nu, nx), np.swapaxes(B, 2, 3))
    assert np.array_equal(blocks(D.c, N * nx), np.zeros(N * nx))
    # only A varies over the stages: B is prob's B in every stage
    d, D, _, keep = ocp.pack(prob, X, A=A)
    assert d.stage_models == 1 and D.sB == 0
    assert np.array_equal(blocks(D.B, N * nx * nu).reshape(N, nu, nx), np.tile(prob.B.T, (N, 1, 1)))
    # batch == N: one model per instance as before schedules existed; a schedule has to be asked for
    X6 = ltv_cases.states('mg', 6, 0)
    d, D, _, keep = ocp.pack(prob, X6, A=A[0], B=B[0])
    assert (d.stage_models, D.sA, D.sB) == (0, nx * nx, nx * nu)
    assert np.array_equal(blocks(D.A, 6 * nx * nx).reshape(6, nx, nx), np.swapaxes(A[0], 1, 2))
    assert ocp.pack(prob, X6, A=A[0], stage_models=True)[0].stage_models == 1
    assert ocp.pack(prob, X6, A=A[0], stage_models=False)[0].stage_models == 0
    with pytest.raises(ValueError):
        ocp.pack(prob, X, A=A[:, :4])                           # a schedule of the wrong length
    d, D, _, keep = ocp.pack(prob, X, A=A, skip=[0, 1, 0])
    assert [D.skip[i] for i in range(3)] == [0, 1, 0]
