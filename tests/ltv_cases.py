"""Problems, model schedules and exact optima shared by the per-stage-model tests
(test_ltv_host.py, test_gpu_ocp_ltv.py).

MG (4, 1, 1): the DMS tracking LMPC problem (bqp.TrackingLMPC: every stage carries the running
cost, boxes on every stage, the 616-row terminal set on [x_N; theta]) at any horizon, from the
stored C2 states (tests/golden/lmpc_N20.npz, deviation coordinates).
DI (2, 2, 2): the double integrator of tests/golden/di_design.npz (C3) with the same cost
structure - running cost on every stage k < N, terminal P and offset cost T on stage N.  The
reference's own DI cost (bqp.TrackingMPC) leaves u_{N-1} without cost, so its optimum is not
unique there and cannot be held to a bar on |z - z*|; this form has a unique optimum.
Schedules follow C4's recipe drawn per stage: A_k = A + 0.01 E_k o |A|, B_k = B + 0.01 e_k o |B|,
c_k ~ 1e-3 N(0, 1).
"""
import numpy as np

from conftest import golden

import ltv_ref


def mg_prob(N):
    import bqp
    from oracle.mg_model import mg_problem
    mg = mg_problem()
    ts = golden('term_set.npz')
    return bqp.TrackingLMPC(mg['A'], mg['B'], mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'],
                            mg['PSI'], mg['F_x'], mg['h_x'], mg['F_u'], mg['h_u'], ts['F_w_N'],
                            ts['h_w_N'], mg['x_wp'], mg['u_wp'], N=N).prob


def di_prob(N):
    import bqp
    from bqp.mpc import _tracking_blocks
    g = golden('di_design.npz')
    tm = bqp.TrackingMPC(g['A'], g['B'], g['Q'], g['R'], g['P'], g['T'], g['LAMBDA'], g['PSI'],
                         g['F_x'], g['h_x'], g['F_u'], g['h_u'], g['F_T'], g['h_T'], N=N)
    p = tm.prob
    Ex, Eu, Eth = _tracking_blocks(2, 2, 2, np.asarray(g['LAMBDA'], float), np.asarray(g['PSI'], float))
    W = np.zeros_like(p.W)
    for k in range(N):
        W[k] = 2 * (Ex.T @ g['Q'] @ Ex + Eu.T @ g['R'] @ Eu)
    W[N] = 2 * (Ex.T @ g['P'] @ Ex + Eth.T @ g['T'] @ Eth)
    w = np.zeros_like(p.w)
    w[N] = -2 * Eth.T @ g['T'] @ g['xs'][1]        # offset cost towards the second stored reference
    xlb, xub = p.xlb.copy(), p.xub.copy()
    xlb[N], xub[N] = xlb[1], xub[1]
    return bqp.OcpProblem(p.A, p.B, W, N, 2, w=w, xlb=xlb, xub=xub, ulb=p.ulb, uub=p.uub, Fp=p.Fp,
                          hp=p.hp, poly_stage=N)


def states(family, n, seed):
    """n stored states of the family's configuration (C2 for MG, C3 for DI), drawn by seed."""
    X = golden('lmpc_N20.npz')['dx'] if family == 'mg' else golden('di_design.npz')['x0']
    return X[np.random.default_rng(seed).choice(len(X), n, replace=False)]


def schedules(prob, n, seed):
    """n schedules: A (n, N, nx, nx), B (n, N, nx, nu), c (n, N, nx)."""
    rng = np.random.default_rng(seed)
    N, nx, nu = prob.N, prob.nx, prob.nu
    A = prob.A + 0.01 * rng.standard_normal((n, N, nx, nx)) * np.abs(prob.A)
    B = prob.B + 0.01 * rng.standard_normal((n, N, nx, nu)) * np.abs(prob.B)
    c = 1e-3 * rng.standard_normal((n, N, nx))
    return A, B, c


# (family, N) -> seed of the states and schedules, chosen on the CPU with the exact solver.
# DI: the first seed of 0..11 with all five instances feasible and the most active rows (7 to 33
# in every instance).  MG: most stored C2 states lie inside this problem's constraints (input box
# +-1) or outside its feasible set, so few draws have any active row.  The MG cases therefore
# tighten the input box to +-UBOUND, 0.8 of the smallest max_k |u*_k| over the five instances of
# the draw under the original box: every instance then has an input that wants to leave the box.
# The seed is the first of 0..15 for which all five instances stay feasible under that box and
# each has active rows; their counts per instance are listed beside the bound.
SEEDS = {('mg', 3): 0, ('mg', 20): 1, ('mg', 63): 0, ('mg', 64): 0, ('mg', 100): 0, ('mg', 127): 0,
         ('di', 3): 0, ('di', 30): 11}
UBOUND = {3: 0.462,      # active rows 1, 2, 1, 2, 2
          20: 0.0617,    # 3, 18, 20, 15, 19
          63: 0.0882,    # 62, 4, 63, 63, 63
          64: 0.0761,    # 64, 14, 64, 64, 64
          100: 0.108,    # 93, 6, 100, 100, 100
          127: 0.108}    # 120, 7, 127, 127, 127


def case(family, N, n=5):
    """dict(prob, X, A, B, c, ref): ref[i] the exact optimum of instance i (ltv_ref.solve)."""
    prob = mg_prob(N) if family == 'mg' else di_prob(N)
    if family == 'mg':
        prob.uub[:] = UBOUND[N]
        prob.ulb[:] = -UBOUND[N]
    seed = SEEDS[(family, N)]
    X = states(family, n, seed)
    A, B, c = schedules(prob, n, 100 + seed)
    ref = [ltv_ref.solve(prob, X[i], A[i], B[i], c[i]) for i in range(n)]
    return dict(prob=prob, X=X, A=A, B=B, c=c, ref=ref)
