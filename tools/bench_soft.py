"""Price of the soft state bounds: the structured solve of one problem with hard state bounds
against the same problem with every bounded state softened (bqp_ocp_data.xs_lin / xs_quad) at
weights large enough that no slack is active (l1 = l2 = 1e6: the optimum is the hard one),
alternated in one process.  Both calls skip the repair launch (polish -1; a soft problem never has
one), so the kernel time (bqp_last_kernel_ms) is the solve launch alone.  The soft call runs the
soft instantiation, a per-stage-model one that reads the one model at every stage, one instance
per slot; the hard call runs the one-model kernels (persistent launch on large batches).

    python tools/bench_soft.py [--config C2|C5] [--batch B] [--runs 3] [--calls 20] [--weight 1e6]

Prints one line per run (median / min kernel ms over the calls, after three warm-up calls, and the
instances per workgroup the launch used) and a JSON summary.  It sets no target."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'learning-based-mpc_amd'))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='C2', choices=['C2', 'C5'])
    ap.add_argument('--batch', type=int, default=0)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--weight', type=float, default=1e6)
    args = ap.parse_args()
    import bench
    import bqp
    wl = bench.workload(args.config, args.batch, 0, 1)
    prob, X = wl['prob'], wl['X']
    N = prob.N
    h = bqp.Handle(0)
    wts = np.zeros((N + 1, prob.nx))
    wts[1:] = args.weight
    soft = dict(xs_lin=wts, xs_quad=wts, want_duals=True)

    def run(kw):
        ms = []
        for i in range(3 + args.calls):
            r = bqp.solve_ocp(prob, X, handle=h, polish=-1, **kw)
            if i >= 3:
                ms.append(h.kernel_ms()[0])
        return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), wpb=h.ocp_wpb(),
                    flags_ok=bool((r.exitflag == 1).all()), iterations=int(r.iterations.sum())), r

    res = {'hard': [], 'soft': []}
    for k in range(args.runs):
        for name, kw in (('hard', {}), ('soft', soft)):
            s, r = run(kw)
            res[name].append(s)
            print('run %d %s: median %.4f ms, min %.4f ms, instances per workgroup %d, flags ok %s, iterations %d'
                  % (k, name, s['median_ms'], s['min_ms'], s['wpb'], s['flags_ok'], s['iterations']))
            z = np.concatenate([r.u.reshape(len(X), -1), r.theta], axis=1)
            if name == 'hard':
                zh = z
            else:
                zs, smax = z, float(r.s_x.max())
    med = {n: float(np.median([s['median_ms'] for s in res[n]])) for n in res}
    print(json.dumps(dict(config=args.config, N=N, batch=len(X), weight=args.weight, hard_ms=med['hard'],
                          soft_ms=med['soft'], ratio=med['soft'] / med['hard'],
                          max_abs_diff=float(np.abs(zh - zs).max()), max_slack=smax, runs=res)))


if __name__ == '__main__':
    main()
