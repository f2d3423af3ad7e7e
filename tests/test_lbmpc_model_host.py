"""Host checks of tests/lbmpc_model_ref.py, the precision-independent restatement of what the
learned-model SQP's kernels compute at a given z: in float64 it equals oracle/lbmpc.py on 7-row
windows (nw, nw_hess, nw_window, gn_model, newton_model(clip=False)), its gradient is the
derivative of its own longdouble cost, and it restates the kernel's row order."""
import numpy as np
import pytest

from conftest import golden

import lbmpc_model_ref as ref

LD = np.longdouble


@pytest.fixture(scope='module')
def sets():
    return golden('lbmpc_instance.npz')


@pytest.fixture(scope='module')
def td():
    return golden('train_data.npz')['data']


def masked(w7, seed):
    """8-row window: about a third of the points invalid, Y = 0 there"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(size=w7.shape[1]) > 1.0 / 3.0).astype(float)
    w = np.vstack([w7, v[None, :]])
    w[3:7, v == 0] = 0.0
    return w


def problem(mg, sets, form, N, data):
    from oracle import lbmpc
    mk = dict(f3=lbmpc.f3_problem, f4=lbmpc.f4_problem, dms=lbmpc.dms_problem)[form]
    return mk(mg, N, data, sets['F_w_N'], sets['h_w_N'], sets['F_x_d'], sets['h_x_d'])


def point(N, seed):
    rng = np.random.default_rng(seed)
    x0 = np.array([rng.uniform(-0.3, 0.0), rng.uniform(-0.3, 0.0), 0.01 * rng.standard_normal(),
                   0.1 * rng.standard_normal()])
    z = np.concatenate([rng.uniform(-0.1, 0.1, N), rng.uniform(-0.05, 0.05, 1)])
    return x0, z


def test_nw_equals_oracle_on_7_row_windows(td):
    from oracle import lbmpc
    rng = np.random.default_rng(0)
    for q in (1, 2, 65, 100):
        w = td[:, 30:30 + q]
        for _ in range(4):
            xi = w[:3, rng.integers(q)] + 0.05 * rng.standard_normal(3)
            g, dg, d2g = ref.nw(xi, w, np.float64, 2)
            go, dgo = lbmpc.nw(xi, w)
            gh, dgh, d2gh = lbmpc.nw_hess(xi, w)
            gw, dgw = lbmpc.nw_window(xi, w)
            for a, b in ((g, go), (dg, dgo), (g, gh), (dg, dgh), (d2g, d2gh), (g, gw), (dg, dgw)):
                assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
            assert np.array_equal(ref.nw(xi, w, np.float64, 0), g)


def test_nw_masked_window_denominator(td):
    """8 rows: the denominator counts the valid points only, the numerator every point"""
    from oracle import lbmpc
    w = masked(td[:, :100], 1)
    w[3:7, 5] = 1.0                       # an invalid point with Y != 0 still enters the numerator
    w[7, 5] = 0.0
    xi = w[:3, 5] + 0.01
    g, dg, d2g = ref.nw(xi, w, np.float64, 2)
    gw, dgw = lbmpc.nw_window(xi, w)
    gh, dgh, d2gh = lbmpc.nw_hess(xi, w)
    assert np.abs(g - gw).max() <= 1e-13 and np.abs(dg - dgw).max() <= 1e-12
    assert np.abs(d2g - d2gh).max() <= 1e-12 * np.abs(d2gh).max()
    d = w[:3] - xi[:, None]
    k = np.exp(-(d * d).sum(0) / 0.25)
    assert np.abs(g - w[3:7] @ k / (1e-3 + k @ w[7])).max() <= 1e-14
    assert np.abs(g - w[3:7] @ k / (1e-3 + k.sum())).max() > 1e-3      # not the unmasked sum


@pytest.mark.parametrize('form,N', [('f3', 1), ('f3', 2), ('f3', 10), ('f4', 16), ('dms', 33)])
def test_model_equals_oracle(mg, sets, td, form, N):
    from oracle import lbmpc
    p = problem(mg, sets, form, N, td[:, 100:200])
    P = ref.from_oracle(p)
    x0, z = point(N, N)
    m = ref.model(P, x0, z, np.float64, exact=True)
    H, f = lbmpc.gn_model(p, x0, z)
    Hx, fx = lbmpc.newton_model(p, x0, z, clip=False)
    assert abs(m['cost'] - lbmpc.cost(p, x0, z)) <= 1e-13 * max(1.0, abs(m['cost']))
    for a, b in ((m['H'], H), (m['f'], f), (m['Hx'], Hx), (m['f'], fx)):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert np.abs(m['Hx'] - m['H']).max() > 0                          # the term is not empty
    # Jr2' Tr2 is the second-order term
    assert np.abs(m['H'] + m['Jr2'].T @ m['Tr2'] - m['Hx']).max() <= 1e-12 * np.abs(Hx).max()
    assert ref.pivots(Hx)[0] == lbmpc.pd_cholesky(Hx)


@pytest.mark.parametrize('form,N,mask', [('f3', 3, False), ('f4', 17, False), ('dms', 9, True)])
def test_gradient_is_the_derivative_of_the_longdouble_cost(mg, sets, td, form, N, mask):
    w = td[:, 200:265]
    p = problem(mg, sets, form, N, masked(w, 2) if mask else w)
    P = ref.from_oracle(p)
    x0, z = point(N, 100 + N)
    f = ref.model(P, x0, z, LD)['f']
    h = LD(2) ** -24                      # central difference: h^2 f''' ~ 4e-15, round-off eps / h ~ 2e-12
    fd = np.zeros(N + 1, LD)
    for j in range(N + 1):
        e = np.zeros(N + 1, LD); e[j] = h
        fd[j] = (ref.model(P, x0, z.astype(LD) + e, LD, jac=False)['cost']
                 - ref.model(P, x0, z.astype(LD) - e, LD, jac=False)['cost']) / (2 * h)
    assert np.abs(f - fd).max() <= 1e-10 * max(1.0, np.abs(f).max())
    # and the float64 evaluation is the same function
    assert np.abs(ref.model(P, x0, z)['f'] - f).max() <= 1e-12 * max(1.0, np.abs(f).max())


def test_row_order(mg, sets, td):
    """rows: per running stage 4 state rows then the input row; terminal P; terminal T"""
    N = 5
    p = problem(mg, sets, 'f3', N, td[:, :64])
    P = ref.from_oracle(p)
    rows = ref.row_order(N, P['n_run'])
    assert len(rows) == P['n_run'] * 5 + 8 == 23
    assert rows[4] == ('u', 0, 0) and rows[5] == ('x', 1, 0) and rows[15] == ('P', N, 0) and rows[22] == ('T', N, 3)
    x0, z = point(N, 5)
    m = ref.model(P, x0, z)
    assert m['Jr'].shape == (23, N + 1) and m['er'].shape == (23,)
    for r, (blk, k, i) in enumerate(rows):
        Jrow = m['Jr'][r]
        if blk == 'x':
            assert np.all(Jrow[k:N] == 0)           # x_k depends on v_0 .. v_{k-1} and theta only
        elif blk == 'u':
            assert Jrow[k] == P['Lr'][0, 0] and np.all(Jrow[k + 1:N] == 0)
        elif blk == 'T':
            assert np.all(Jrow[:N] == 0)
    # the theta column of the last block is Lt LAMBDA
    assert np.allclose(m['Jr'][19:, N], P['Lt'] @ P['LAMBDA'], rtol=0, atol=1e-15)
    assert abs(m['cost'] - (m['er'] ** 2).sum()) == 0


def test_shift_index_is_hess_shift(mg, sets, td):
    from oracle import lbmpc
    rng = np.random.default_rng(4)
    Q = np.linalg.qr(rng.standard_normal((12, 12)))[0]
    for lowest in (1.0, 1e-11, -1e-7, -1e-3, -10.0):
        H = (Q * np.concatenate([[lowest], np.linspace(0.5, 30.0, 11)])) @ Q.T
        H = 0.5 * (H + H.T)
        k = ref.shift_index(H)
        assert (k is None) == lbmpc.pd_cholesky(H)
        if k is not None:
            sh = lbmpc.hess_shift(H)
            hd = np.abs(np.diag(H)).max()
            assert (k == 21 and sh is None) or sh == ref.shift_value(hd, k)
