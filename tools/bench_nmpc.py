#!/usr/bin/env python3
"""Timing of the nonlinear MPC path on the GPU (reported, not a gate; bench.py is the project's
benchmark).  Workload: cold solves at N = 100 for a batch of seeded perturbations of the stored
states of the reference's tracking-NMPC run, and a closed loop from perturbed initial states.
Warmed up; timed with the library's device events around work that ends in a synchronise
(bqp_last_kernel_ms).  Prints one JSON line.

  --batch B --steps S --warmup W   sizes (defaults 256, 100, 1)
  --sync     the closed loop step-synchronous (BQP_NMPC_SYNC set for the loop run alone; the
             default is the asynchronous loop); `loop_rounds` is printed in both modes
  --subproblem dense|stage   how the SQP's sub-problems are solved (default dense): condensed on
             the dense kernels, or in stage form on the structured kernel with per-stage models
  --shooting single|multiple   bqp_nmpc_dims.shooting (default single; multiple needs --subproblem
             stage): the states eliminated, or kept as decision variables
  --polish P the sub-problems' polish (bqp_options.polish; default 0)
  --split    also the split of an SQP iteration over linearise / normal equations / dense /
             trials / update (stage route: stage linearisation / structured solve / back-map /
             trials / update): a child process runs the cold solves with BQP_LB_TRACE=2 and its
             per-iteration lines are summed here, per iteration index too (the first is the cold
             one); the stage route's child also reports the workspace bytes it reserved
  --dump F   X, U, exitflag, iterations of the loop into the .npz file F
The bytes of the dense solve's stream of the instances' C are computed from the shapes."""
import argparse
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'learning-based-mpc_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

N = 100


def problem():
    import bqp
    from oracle.mg_model import mg_problem
    mg = mg_problem()
    ts = np.load(os.path.join(ROOT, 'tests', 'golden', 'term_set.npz'))
    return bqp.NMPC(mg['Q'], mg['R'], mg['P'], mg['Tscalar'], mg['LAMBDA'], mg['PSI'], mg['F_x'],
                    mg['h_x'], mg['F_u'], mg['h_u'], ts['F_w_N'], ts['h_w_N'], mg['x_wp'],
                    mg['u_wp'], N=N)


def starts(batch, seed=11):
    """seeded +-0.02 perturbations (x1, x2) of stored states of DSS_tNMPC.mat, spread over the run"""
    xnl = np.load(os.path.join(ROOT, 'tests', 'golden', 'nmpc_DSS_tNMPC.npz'))['xnl']
    rng = np.random.default_rng(seed)
    x = xnl[:, rng.integers(0, 400, batch)].T.copy()
    x[:, :2] += rng.uniform(-0.02, 0.02, (batch, 2))
    return np.ascontiguousarray(x)


def child(batch, subproblem, polish, shooting):
    import bqp
    bqp.NMPC.solve(problem(), starts(batch), handle=bqp.Handle(0), subproblem=subproblem, polish=polish,
                   shooting=shooting)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--sync', action='store_true')
    ap.add_argument('--split', action='store_true')
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--subproblem', choices=('dense', 'stage'), default='dense')
    ap.add_argument('--shooting', choices=('single', 'multiple'), default='single')
    ap.add_argument('--polish', type=int, default=0)
    ap.add_argument('--dump', default=None)
    ap.add_argument('--soft', type=float, nargs=2, metavar=('L1', 'L2'), default=None,
                    help='soft state rows in the closed loop: the weights on all rows of F_x (stage route)')
    a = ap.parse_args()
    soft = dict(xs_lin=a.soft[0], xs_quad=a.soft[1]) if a.soft else {}
    if a.child:
        return child(a.batch, a.subproblem, a.polish, a.shooting)
    import torch
    assert torch.cuda.is_available(), 'bench_nmpc.py needs a GPU'
    import bqp
    h = bqp.Handle(0)
    g = problem()
    x = starts(a.batch)
    for _ in range(a.warmup):
        g.solve(x, handle=h, subproblem=a.subproblem, polish=a.polish, shooting=a.shooting)
    lib = bqp.load()
    import ctypes as C
    from bqp import _lib
    # the solve alone (g.solve also rolls the solution out for y_OL): events around the SQP
    z = np.zeros((a.batch, N + 1)); lam = np.zeros((a.batch, g.m)); cost = np.zeros(a.batch)
    fl = np.zeros(a.batch, np.int32); it = np.zeros(a.batch, np.int32)
    dims, dd = g._dims(a.subproblem, a.shooting), g._data(x)
    o = _lib.options(max_iter=100, tol_stat=1e-8, polish=a.polish)
    _lib.check(lib.bqp_nmpc_solve_batched(h.value, C.byref(dims), a.batch, C.byref(dd), C.byref(o),
                                          _lib.ptr(z), _lib.ptr(lam), _lib.ptr(cost), _lib.iptr(fl),
                                          _lib.iptr(it)), 'bqp_nmpc_solve_batched')
    ms, launches = h.kernel_ms()
    out = dict(N=N, batch=a.batch, m=g.m, subproblem=a.subproblem, shooting=a.shooting, polish=a.polish, solve_ms=ms, solves_per_s=a.batch / ms * 1e3,
               solve_iterations_mean=float(it.mean()), solve_iterations_max=int(it.max()),
               solve_converged=float((fl == 1).mean()), solve_launches=launches,
               solve_flags={str(int(k)): int((fl == k).sum()) for k in np.unique(fl)})
    # per SQP iteration the dense solve reads the instance's C (m x n doubles) once per
    # interior-point iteration at least: bytes per pass over the batch, from the shapes
    if a.subproblem == 'dense':
        out['C_bytes_per_pass'] = int(a.batch) * g.m * (N + 1) * 8
    if a.steps > 0:
        rng = np.random.default_rng(12)
        xnl = np.load(os.path.join(ROOT, 'tests', 'golden', 'nmpc_DSS_tNMPC.npz'))['xnl']
        xi = np.tile(xnl[:, 0], (a.batch, 1))
        xi[1:, :2] += rng.uniform(-0.02, 0.02, (a.batch - 1, 2))
        assert 'BQP_NMPC_SYNC' not in os.environ, 'select the loop with --sync'
        if a.sync:
            os.environ['BQP_NMPC_SYNC'] = '1'
        try:
            if a.warmup:
                bqp.closed_loop_nmpc(g, xi, 2, handle=h, subproblem=a.subproblem, polish=a.polish,
                                     shooting=a.shooting, **soft)
            r = bqp.closed_loop_nmpc(g, xi, a.steps, handle=h, subproblem=a.subproblem, polish=a.polish,
                                     shooting=a.shooting, **soft)
        finally:
            os.environ.pop('BQP_NMPC_SYNC', None)
        out.update(loop_soft=a.soft, loop_infeasible=int((r.exitflag == -2).sum()))
        out.update(loop_mode='sync' if a.sync else 'async', loop_steps=a.steps, loop_ms=r.kernel_ms,
                   loop_rounds=r.rounds,
                   loop_rounds_from_logs=int((r.iterations + (r.exitflag != 0)).sum(axis=1).max()),
                   loop_rounds_stepwise=int((r.iterations + (r.exitflag != 0)).max(axis=0).sum()),
                   loop_flags={str(int(k)): int((r.exitflag == k).sum()) for k in np.unique(r.exitflag)},
                   instance_steps_per_s=a.batch * a.steps / r.kernel_ms * 1e3,
                   loop_iterations_mean=float(r.iterations.mean()),
                   loop_iterations_max=int(r.iterations.max()),
                   loop_iteration_histogram={str(int(k)): int((r.iterations == k).sum())
                                             for k in np.unique(r.iterations)},
                   loop_at_iteration_limit=int((r.exitflag == 0).sum()),
                   loop_converged=float((r.exitflag == 1).mean()), loop_launches=r.launches)
        if a.dump:
            np.savez(a.dump, X=r.X, U=r.U, exitflag=r.exitflag, iterations=r.iterations)
    if a.split:
        env = dict(os.environ, BQP_LB_TRACE='2')
        c = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--batch', str(a.batch),
                            '--subproblem', a.subproblem, '--polish', str(a.polish), '--shooting', a.shooting],
                           env=env, capture_output=True, text=True, timeout=600, check=True)
        if a.subproblem == 'dense':
            names = ('linearise', 'normal', 'dense', 'trials', 'update')
            pat = (r'bqp nmpc it (\d+) ms: linearise ([\d.]+) normal ([\d.]+) dense\(\+polish\) ([\d.]+) '
                   r'trials ([\d.]+) update ([\d.]+)')
        else:
            names = ('stage_linearise', 'structured', 'back_map', 'trials', 'update')
            pat = (r'bqp nmpc it (\d+) ms: stage-linearise ([\d.]+) structured\(\+repair\) ([\d.]+) '
                   r'back-map ([\d.]+) trials ([\d.]+) update ([\d.]+)')
        tot = dict.fromkeys(names, 0.0)
        per_it = []
        for line in c.stderr.splitlines():
            mt = re.match(pat, line)
            if mt:
                vals = [float(v) for v in mt.groups()[1:]]
                per_it.append(dict(zip(names, vals)))
                for k, v in zip(names, vals):
                    tot[k] += v
            mw = re.match(r'bqp nmpc stage route: workspace (\d+) bytes', line)
            if mw:
                out['stage_workspace_bytes'] = int(mw.group(1))
        rows = len(per_it)
        out['split_ms_per_iteration'] = {k: v / max(rows, 1) for k, v in tot.items()}
        out['split_ms_by_iteration'] = per_it
        out['split_iterations'] = rows
    print(json.dumps(out))


if __name__ == '__main__':
    main()
