"""Price of the per-stage model table: the structured solve of one problem with one model for the
horizon (bqp_ocp_dims.stage_models = 0) against the same problem given as N equal per-stage models
(stage_models = 1), alternated in one process.  Both calls skip the repair launch (polish -1), so
the kernel time (bqp_last_kernel_ms) is the solve launch alone.

    python tools/bench_ltv.py [--config C2|C5] [--batch B] [--runs 3] [--calls 20]

Prints one line per run (median / min kernel ms over the calls, after three warm-up calls, and the
instances per workgroup the launch used) and a JSON summary."""
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
    args = ap.parse_args()
    import bench
    import bqp
    wl = bench.workload(args.config, args.batch, 0, 1)
    prob, X = wl['prob'], wl['X']
    N = prob.N
    h = bqp.Handle(0)
    sched = dict(A=np.tile(prob.A, (N, 1, 1)), B=np.tile(prob.B, (N, 1, 1)), stage_models=True)

    def run(kw):
        ms = []
        for i in range(3 + args.calls):
            r = bqp.solve_ocp(prob, X, handle=h, polish=-1, **kw)
            if i >= 3:
                ms.append(h.kernel_ms()[0])
        return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), wpb=h.ocp_wpb(),
                    flags_ok=bool((r.exitflag == 1).all()), iterations=int(r.iterations.sum())), r

    res = {'lti': [], 'ltv': []}
    for k in range(args.runs):
        for name, kw in (('lti', {}), ('ltv', sched)):
            s, r = run(kw)
            res[name].append(s)
            print('run %d %s: median %.4f ms, min %.4f ms, instances per workgroup %d, flags ok %s, iterations %d'
                  % (k, name, s['median_ms'], s['min_ms'], s['wpb'], s['flags_ok'], s['iterations']))
            if name == 'lti':
                zl = np.concatenate([r.u.reshape(len(X), -1), r.theta], axis=1)
            else:
                zv = np.concatenate([r.u.reshape(len(X), -1), r.theta], axis=1)
    med = {n: float(np.median([s['median_ms'] for s in res[n]])) for n in res}
    print(json.dumps(dict(config=args.config, N=N, batch=len(X), lti_ms=med['lti'], ltv_ms=med['ltv'],
                          ratio=med['ltv'] / med['lti'], max_abs_diff=float(np.abs(zl - zv).max()),
                          runs=res)))


if __name__ == '__main__':
    main()
