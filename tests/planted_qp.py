"""Dense QPs whose optimum is known by construction (shared by tests/test_planted_qp_host.py and
tests/test_gpu_quadprog_planted.py; a plain helper module like status_cases.py).

    min 0.5 z'Hz + f'z   s.t.  A z <= b,  Aeq z = beq,  lb <= z <= ub

planted() draws H = MM'/n + I, A, Aeq, an active set with multipliers in [0.5, 2] (equality
multipliers of either sign), inactive slacks in [0.2, 1] and the point z*, then sets
b = A z* + slack, beq = Aeq z*, the active bounds to z*_j and

    f = -(H z* + A'lam + Aeq'y + lam_u - lam_l)      (in np.longdouble)

so that (z*, lam, y, lam_l, lam_u) satisfies the KKT conditions with strict complementarity:
sufficient for a convex QP, no solver is involved in the reference.

Condition on the active set (licq()): the equality rows, the active rows of A and the active
bounds, each scaled to unit norm, form a matrix of at most n rows with sigma_min / sigma_max >=
LICQ_MIN.  The multipliers are then unique and well conditioned; without it the staircase
patterns give dependent active rows whose multipliers no solver can be compared on.  The active
set is grown greedily (a candidate row joins only if the condition still holds) and the condition
is asserted on what is returned.
"""
import contextlib

import numpy as np

try:
    from threadpoolctl import threadpool_limits
except ImportError:                      # optional: only the run time depends on it
    threadpool_limits = None


def one_blas_thread():
    """the matrices here are at most 8272 x 256: a BLAS thread pool only contends on them (the
    256 x 256 SVDs of the greedy active set ran 50 x slower on 8 threads than on one)"""
    return threadpool_limits(limits=1) if threadpool_limits else contextlib.nullcontext()


LD = np.longdouble
LICQ_MIN = 1e-2
STAIR_HEAD = (0, 1, 15, 16, 17, 31, 32, 33, -1, 0x7fffffff)   # c(r) of the first rows (-1: n - 1)


# ----------------------------------------------------------------------------------------------
# launch_dense's predicates (csrc/bqp_dense.hip), restated to name the kernel form of a shape
# ----------------------------------------------------------------------------------------------
DT, TILE, DQ_THL, DQ_RPT, DQ_GB, DQ_NVEC = 256, 32, 256, 4, 34, 17
DQ_TAIL = 48 + DQ_THL
DENSE_LDS_MAX = 152 * 1024
SW_NMAX, SW_LDS_MAX, SW_A_LDS_MAX = 32, 64 * 1024 // 8, 4096
DQ_POL_KLDS = 16 * 1024


def small_lds_doubles(n, m):
    return 2 * n * n + 8 * n + 12 * n + 8 * m + (m * n if m * n <= SW_A_LDS_MAX else 0)


def dense_ts(n):
    return 32 * ((n + 31) // 32) + 1


def dense_gbuf(n):
    return DQ_GB * (n + 2)


def dense_glds(n):
    a, b = TILE * dense_ts(n), 2 * dense_gbuf(n)
    return n <= 128 and (max(a, b) + n * n + DQ_TAIL) * 8 <= DENSE_LDS_MAX


def dense_tiles(n):
    a, b = TILE * dense_ts(n), 2 * dense_gbuf(n)
    return b if dense_glds(n) and b > a else a


def dense_k_lds(n):
    return (dense_tiles(n) + n * n + DQ_TAIL) * 8 <= DENSE_LDS_MAX


def dense_lds_bytes(n):
    return 8 * (dense_tiles(n) + (n * n if dense_k_lds(n) else 0) + DQ_TAIL)


def dense_rows_in_regs(n, m):
    return (0 < m <= DQ_RPT * DT and dense_k_lds(n) and dense_glds(n) and m + n <= TILE * dense_ts(n)
            and dense_lds_bytes(n) + 8 * DQ_NVEC * n <= DENSE_LDS_MAX)


def kernel_form(n, m, me):
    """the kernel launch_dense picks for (n, m, me), or None where the entry point refuses"""
    if n <= 0 or n > 256 or me > 256 or m > 8192:
        return None
    if me == 0 and n <= SW_NMAX and small_lds_doubles(n, m) <= SW_LDS_MAX:
        return 'wave1' if n <= 16 else 'wave2'
    if dense_lds_bytes(n) > DENSE_LDS_MAX:
        return None
    if dense_rows_in_regs(n, m):
        return 'regs'
    return 'lds' if dense_k_lds(n) else 'work'


def polish_k_in_lds(n):
    return n * n <= DQ_POL_KLDS


def wave_a_in_lds(n, m):
    return m * n <= SW_A_LDS_MAX


def atw_tiled(n, m):
    """dense_ipm_kernel's A'w: the row weights no longer fit the tile area whole"""
    return m + n > TILE * dense_ts(n)


# ----------------------------------------------------------------------------------------------
# the generator
# ----------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v)


def licq(rows):
    """sigma_min / sigma_max of the unit-scaled rows (1 for none; 0 for more rows than columns)"""
    if len(rows) == 0:
        return 1.0
    R = np.asarray(rows, float)
    if R.shape[0] > R.shape[1]:
        return 0.0
    s = np.linalg.svd(R, compute_uv=False)
    return float(s[-1] / s[0])


def stair_bounds(n, m, rng):
    """c(r) of the 'stair' pattern: row r is non-zero only in columns < c(r)"""
    c = rng.integers(1, n + 1, m)
    head = [min(n, max(0, n - 1 if v < 0 else v)) for v in STAIR_HEAD]
    c[:min(m, len(head))] = head[:m]
    if m >= 256:
        c[128:256] = rng.integers(1, min(16, n) + 1, 128)    # four tiles with bound <= 16
    if m >= 288:
        c[256:288] = 0                                       # a tile of all-zero rows
    return c


def make_A(rng, n, m, pattern, nu=1, npar=1):
    """(A, priority rows): the rows the active set tries first, so the pattern's edges bind"""
    A = rng.standard_normal((m, n))
    prio = []
    if pattern == 'dense' or m == 0:
        return A, prio
    if pattern == 'stair':
        c = stair_bounds(n, m, rng)
        A[np.arange(n)[None, :] >= c[:, None]] = 0.0
        if n >= 3:
            A[1::2, n // 3] = 0.0                            # an interior zero, not a row end
        prio = list(range(min(m, len(STAIR_HEAD))))
        if m >= 256:
            prio += [int(r) for r in rng.choice(np.arange(128, 256), 4, replace=False)]
        return A, prio
    if pattern == 'causal':
        N = max(1, (n - npar) // nu)
        k = (np.arange(m) * N) // m                          # the stage of row r
        see = np.arange(n)[None, :] < ((k + 1) * nu)[:, None]
        see[:, n - npar:] = True
        A[~see] = 0.0
        return A, prio
    raise ValueError(pattern)


def bound_masks(rng, n, bounds, nfixed):
    """(has_lb, has_ub, fixed) per variable"""
    fixed = np.zeros(n, bool)
    if bounds == 'none':
        return np.zeros(n, bool), np.zeros(n, bool), fixed
    if bounds in ('all', 'fixed'):
        hl, hu = np.ones(n, bool), np.ones(n, bool)
        if bounds == 'fixed':
            fixed[rng.choice(n, nfixed, replace=False)] = True
        return hl, hu, fixed
    if bounds == 'partial':
        kind = rng.integers(0, 4, n)                         # neither, lb, ub, both
        kind[:min(n, 4)] = rng.permutation(4)[:min(n, 4)]    # every kind present once n >= 4
        return (kind == 1) | (kind == 3), (kind == 2) | (kind == 3), fixed
    raise ValueError(bounds)


def _active_set(rng, n, A, prio, E, hl, hu, fixed):
    """greedy LICQ active set: (rows of A, upper-bound indices, lower-bound indices)"""
    m = A.shape[0]
    base = [_unit(e) for e in E] + [np.eye(n)[j] for j in np.flatnonzero(fixed)]
    assert licq(base) >= LICQ_MIN, 'equality rows alone miss the LICQ condition'
    cap = n - len(base)
    nz = np.abs(A).max(axis=1) > 0 if m else np.zeros(0, bool)
    cand = [('a', int(r)) for r in np.flatnonzero(nz)]
    cand += [('u', int(j)) for j in np.flatnonzero(hu & ~fixed)]
    cand += [('l', int(j)) for j in np.flatnonzero(hl & ~fixed)]
    if cap <= 0 or not cand:
        return [], [], [], base
    target = max(1, min(n // 3 + 1, cap // 2))
    order = [cand[i] for i in rng.permutation(len(cand))]
    first = [('a', r) for r in prio if nz[r]]
    order = first + [c for c in order if c not in first]
    rows, act, used = list(base), {'a': [], 'u': [], 'l': []}, set()
    for kind, i in order[:4 * target + 24]:
        if len(rows) - len(base) >= target:
            break
        if kind != 'a' and i in used:
            continue                                         # one active bound per variable
        v = _unit(A[i]) if kind == 'a' else np.eye(n)[i]
        if licq(rows + [v]) < LICQ_MIN:
            continue
        rows.append(v)
        act[kind].append(i)
        if kind != 'a':
            used.add(i)
    return act['a'], act['u'], act['l'], rows


def planted(rng, n, m, me, bounds='none', pattern='dense', nu=1, npar=1, nfixed=3,
            H=None, A=None, Aeq=None, lb=None, ub=None, shared=None):
    """One planted QP.  H, A (a (matrix, priority rows) pair), Aeq given: used as they are.
    lb / ub given (shared bounds of a batch): z* is placed inside them and on the active ones;
    `shared` carries the bound masks and the fixed values that go with them.
    Returns (qp, sol): qp = dict(H, f, A, b, Aeq, beq, lb, ub) with None for what is absent,
    sol = dict(z, ineqlin, eqlin, lower, upper, active=(rows, upper, lower), licq)."""
    if H is None:
        M = rng.standard_normal((n, n))
        H = M @ M.T / n + np.eye(n)
    Am, prio = make_A(rng, n, m, pattern, nu, npar) if A is None else A
    E = rng.standard_normal((me, n)) if Aeq is None else Aeq
    if shared is None:
        hl, hu, fixed = bound_masks(rng, n, bounds, nfixed)
        centre = None
    else:
        hl, hu, fixed, centre = shared
    ar, au, al, rows = _active_set(rng, n, Am, prio, E, hl, hu, fixed)
    sig = licq(rows)
    assert sig >= LICQ_MIN and len(rows) <= n, (sig, len(rows), n)

    # z*, then the bounds around it (or z* inside the bounds that are given)
    z = rng.standard_normal(n)
    L = np.full(n, -np.inf)
    U = np.full(n, np.inf)
    if ub is not None and lb is not None:
        z = centre + rng.uniform(-0.4, 0.4, n)               # both slacks in [0.2, 1]
    elif ub is not None:
        z = np.where(hu, ub - rng.uniform(0.2, 1.0, n), z)
    elif lb is not None:
        z = np.where(hl, lb + rng.uniform(0.2, 1.0, n), z)
    if centre is not None:
        z[fixed] = centre[fixed]
    if ub is not None:
        U = ub.copy()
        z[au] = U[au]
    if lb is not None:
        L = lb.copy()
        z[al] = L[al]
    if ub is None:
        U = np.where(hu, z + rng.uniform(0.2, 1.0, n), np.inf)
        U[au] = z[au]
        U[fixed] = z[fixed]
    if lb is None:
        L = np.where(hl, z - rng.uniform(0.2, 1.0, n), -np.inf)
        L[al] = z[al]
        L[fixed] = z[fixed]

    lam = np.zeros(m)
    lam[ar] = rng.uniform(0.5, 2.0, len(ar))
    slack = rng.uniform(0.2, 1.0, m)
    slack[ar] = 0.0
    y = rng.uniform(0.5, 2.0, me) * rng.choice([-1.0, 1.0], me)
    lu = np.zeros(n)
    ll = np.zeros(n)
    lu[au] = rng.uniform(0.5, 2.0, len(au))
    ll[al] = rng.uniform(0.5, 2.0, len(al))
    jf = np.flatnonzero(fixed)
    yf = rng.uniform(0.5, 2.0, jf.size) * np.where(np.arange(jf.size) % 2, -1.0, 1.0)   # both signs
    lu[jf] = np.maximum(yf, 0.0)
    ll[jf] = np.maximum(-yf, 0.0)

    zl = z.astype(LD)
    b = (Am.astype(LD) @ zl + slack.astype(LD)).astype(float)
    b[ar] = (Am[ar].astype(LD) @ zl).astype(float)
    beq = (E.astype(LD) @ zl).astype(float)
    # with b, beq rounded to double the residual of the active rows is ~1 ulp, inside every bar
    f = -(H.astype(LD) @ zl + Am.T.astype(LD) @ lam.astype(LD) + E.T.astype(LD) @ y.astype(LD)
          + lu.astype(LD) - ll.astype(LD))
    f = f.astype(float)
    qp = dict(H=H, f=f, A=Am if m else None, b=b if m else None, Aeq=E if me else None,
              beq=beq if me else None, lb=L if hl.any() else None, ub=U if hu.any() else None)
    sol = dict(z=z, ineqlin=lam, eqlin=y, lower=ll, upper=lu, active=(ar, au, al), licq=sig,
               fixed=jf)
    return qp, sol


def kkt_residuals(qp, sol):
    """(stationarity, primal violation, complementarity, most negative multiplier), in longdouble"""
    n = qp['H'].shape[0]
    z = sol['z'].astype(LD)
    r = qp['H'].astype(LD) @ z + qp['f'].astype(LD) + sol['upper'].astype(LD) - sol['lower'].astype(LD)
    viol = LD(0)
    comp = LD(0)
    if qp['A'] is not None:
        s = qp['b'].astype(LD) - qp['A'].astype(LD) @ z
        r = r + qp['A'].T.astype(LD) @ sol['ineqlin'].astype(LD)
        viol = max(viol, (-s).max())
        comp = max(comp, np.abs(s * sol['ineqlin']).max())
    if qp['Aeq'] is not None:
        r = r + qp['Aeq'].T.astype(LD) @ sol['eqlin'].astype(LD)
        viol = max(viol, np.abs(qp['Aeq'].astype(LD) @ z - qp['beq'].astype(LD)).max())
    lb = np.full(n, -np.inf) if qp['lb'] is None else qp['lb']
    ub = np.full(n, np.inf) if qp['ub'] is None else qp['ub']
    fu, fl = np.isfinite(ub), np.isfinite(lb)
    if fu.any():
        viol = max(viol, (z - ub)[fu].max())
        comp = max(comp, np.abs((ub - z)[fu] * sol['upper'][fu]).max())
    if fl.any():
        viol = max(viol, (lb - z)[fl].max())
        comp = max(comp, np.abs((z - lb)[fl] * sol['lower'][fl]).max())
    neg = min(sol['ineqlin'].min(initial=0.0), sol['lower'].min(), sol['upper'].min())
    return float(np.abs(r).max()), float(max(viol, 0)), float(comp), float(neg)


def strict_complementarity(qp, sol):
    """min over rows and bounds of slack + multiplier (>= 0.2 by construction), fixed ones aside"""
    n = qp['H'].shape[0]
    v = [np.inf]
    if qp['A'] is not None:
        v.append((qp['b'] - qp['A'] @ sol['z'] + sol['ineqlin']).min())
    free = np.ones(n, bool)
    free[sol['fixed']] = False
    if qp['ub'] is not None:
        fu = np.isfinite(qp['ub']) & free
        if fu.any():
            v.append(((qp['ub'] - sol['z']) + sol['upper'])[fu].min())
    if qp['lb'] is not None:
        fl = np.isfinite(qp['lb']) & free
        if fl.any():
            v.append(((sol['z'] - qp['lb']) + sol['lower'])[fl].min())
    return float(min(v))


PER_DEFAULT = ('lb', 'ub')


def planted_batch(seed, n, m, me, bounds='none', pattern='dense', batch=3, per=PER_DEFAULT,
                  nu=1, npar=1, nfixed=3):
    """`batch` planted instances.  `per` names what each instance has of its own among H, A, Aeq,
    lb, ub; the rest is shared by the batch.  z*, the active set, f, b and beq are always
    per instance.  Returns (args, sols): args the keyword arguments of bqp.quadprog (a leading
    batch axis on the per-instance ones), sols the list of planted solutions; qps(args, i)
    gives instance i's own QP."""
    rng = np.random.default_rng(seed)
    per = set(per)
    H = A = E = None
    if 'H' not in per:
        M = rng.standard_normal((n, n))
        H = M @ M.T / n + np.eye(n)
    if 'A' not in per:
        A = make_A(rng, n, m, pattern, nu, npar)
    if 'Aeq' not in per:
        E = rng.standard_normal((me, n))
    hl, hu, fixed = bound_masks(rng, n, bounds, nfixed)
    centre = rng.standard_normal(n)
    lb = ub = None
    if 'lb' not in per and 'ub' not in per:
        lb = np.where(hl, centre - 0.6, -np.inf)
        ub = np.where(hu, centre + 0.6, np.inf)
        lb[fixed] = ub[fixed] = centre[fixed]
    elif 'ub' not in per:
        ub = np.where(hu, centre, np.inf)
    elif 'lb' not in per:
        lb = np.where(hl, centre, -np.inf)
    inst = [planted(rng, n, m, me, bounds, pattern, nu, npar, nfixed, H=H, A=A, Aeq=E, lb=lb, ub=ub,
                    shared=(hl, hu, fixed, centre)) for _ in range(batch)]
    qs = [q for q, _ in inst]
    sols = [s for _, s in inst]

    def field(k, own):
        if qs[0][k] is None:
            return None
        return np.stack([q[k] for q in qs]) if own else qs[0][k]

    args = dict(H=field('H', 'H' in per), f=field('f', True), A=field('A', 'A' in per),
                b=field('b', True), Aeq=field('Aeq', 'Aeq' in per), beq=field('beq', True),
                lb=field('lb', 'lb' in per), ub=field('ub', 'ub' in per))
    return args, sols, qs


# ----------------------------------------------------------------------------------------------
# the algorithm statement (oracle/dense_ipm.py) on a planted QP, in quadprog's multiplier fields
# ----------------------------------------------------------------------------------------------
def statement(qp, **kw):
    """oracle.dense_ipm.solve with lb == ub turned into equality rows as bqp/quadprog.py does;
    returns dict(x, exitflag, iterations, polished, fval, ineqlin, eqlin, lower, upper)"""
    from oracle import dense_ipm
    n = qp['H'].shape[0]
    lb = np.full(n, -np.inf) if qp['lb'] is None else qp['lb'].copy()
    ub = np.full(n, np.inf) if qp['ub'] is None else qp['ub'].copy()
    E = np.zeros((0, n)) if qp['Aeq'] is None else qp['Aeq']
    e = np.zeros(0) if qp['beq'] is None else qp['beq']
    me0 = E.shape[0]
    jf = np.flatnonzero(np.isfinite(lb) & (lb == ub))
    if jf.size:
        E = np.vstack([E, np.eye(n)[jf]])
        e = np.concatenate([e, lb[jf]])
        lb[jf], ub[jf] = -np.inf, np.inf
    r = dense_ipm.solve(qp['H'], qp['f'], qp['A'], qp['b'], E, e, lb, ub, **kw)
    m = 0 if qp['A'] is None else qp['A'].shape[0]
    iu, il = np.flatnonzero(np.isfinite(ub)), np.flatnonzero(np.isfinite(lb))
    lam = r['lam']
    up, lo = np.zeros(n), np.zeros(n)
    up[iu] = lam[m:m + iu.size]
    lo[il] = lam[m + iu.size:]
    yf = r['y'][me0:]
    up[jf], lo[jf] = np.maximum(yf, 0.0), np.maximum(-yf, 0.0)
    return dict(x=r['x'], exitflag=r['exitflag'], iterations=r['iterations'],
                polished=r.get('polished', False), fval=r.get('fval'), ineqlin=lam[:m],
                eqlin=r['y'][:me0], lower=lo, upper=up)


FIELDS = ('ineqlin', 'eqlin', 'lower', 'upper')


def errors(got, sol):
    """(|x - z*|_inf / max(1, |z*|_inf), {field: error / max(1, |lam*|_inf)})"""
    ex = np.abs(got['x'] - sol['z']).max() / max(1.0, np.abs(sol['z']).max())
    el = {}
    for k in FIELDS:
        ref = sol[k]
        el[k] = (np.abs(np.asarray(got[k]) - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0
    return float(ex), el


def fval_exact(qp, sol):
    z = sol['z'].astype(LD)
    return float(0.5 * z @ (qp['H'].astype(LD) @ z) + qp['f'].astype(LD) @ z)


# ----------------------------------------------------------------------------------------------
# the case tables
# ----------------------------------------------------------------------------------------------
def _c(form, n, m, me=0, bounds='none', pattern='dense', **kw):
    return dict(form=form, n=n, m=m, me=me, bounds=bounds, pattern=pattern, kw=kw)


# ordered from shapes the suite already runs to the new extremes within each kernel form
TABLE = [
    _c('wave1', 1, 0, 0, 'all'),
    _c('wave1', 1, 3),
    _c('wave1', 2, 5, 0, 'partial'),
    _c('wave1', 7, 1), _c('wave1', 7, 2), _c('wave1', 7, 3),
    _c('wave1', 15, 33, 0, 'none', 'stair'),
    _c('wave1', 16, 64, 0, 'all', 'stair'),
    _c('wave1', 16, 256), _c('wave1', 16, 257),
    _c('wave2', 17, 65, 0, 'partial', 'stair'),
    _c('wave2', 31, 127, 0, 'none', 'stair'),
    _c('wave2', 32, 128), _c('wave2', 32, 129),
    _c('wave2', 21, 806, 0, 'none', 'causal', nu=1, npar=1),
    _c('wave2', 32, 688),
    _c('regs', 32, 689),
    _c('regs', 33, 130, 0, 'none', 'stair'),
    _c('regs', 12, 30, 3, 'partial'),
    _c('regs', 40, 97, 5, 'all', 'stair'),
    _c('regs', 64, 1),
    _c('regs', 101, 1024, 0, 'all', 'causal', nu=1, npar=1),
    # the register form ends at n = 101 (its 17 n-vectors join the two A'DA buffers and the
    # factor in the 152 KB of LDS): the stair case with a partial last 4-row group sits there
    _c('regs', 101, 1023, 0, 'none', 'stair'),
    _c('lds', 40, 0, 0, 'all'),
    _c('lds', 101, 1025, 0, 'none', 'stair'),
    _c('lds', 106, 1023, 0, 'none', 'stair'),
    _c('lds', 109, 300, 0, 'none', 'stair'),
    _c('lds', 122, 161, 4),
    _c('lds', 109, 4100, 0, 'none', 'stair'),
    _c('work', 123, 161, 7, 'partial', 'stair'),
    _c('work', 128, 160),
    _c('work', 129, 160, 3),
    _c('work', 256, 64, 0, 'none', 'stair'),
    _c('work', 256, 40, 200),
    _c('lds', 40, 8161, 0, 'none', 'stair'),
    _c('lds', 40, 8192, 0, 'none', 'stair'),
]

# polish after a truncated solve (section d)
TRUNCATED = [
    _c('wave2', 20, 60, 0, 'all'),
    _c('regs', 40, 97, 5, 'all', 'stair'),
    _c('regs', 101, 300, 0, 'all'),
    _c('work', 128, 160, 0, 'all'),
    _c('work', 129, 160, 3, 'all'),
]

# three fixed variables (lb == ub, multipliers of both signs) beside two genuine equality rows
FIXED = _c('regs', 24, 50, 2, 'fixed', 'dense', nfixed=3)

STRIDE_SHAPES = [_c('wave1', 16, 64, 0, 'all'), _c('regs', 40, 97, 5, 'all'),
                 _c('work', 123, 161, 7, 'all')]
STRIDE_PER = {'f-b': (), 'all': ('H', 'A', 'Aeq', 'lb', 'ub'), 'H-lb': ('H', 'lb')}


def case_id(c):
    s = '%s-n%d-m%d' % (c['form'], c['n'], c['m'])
    if c['me']:
        s += '-me%d' % c['me']
    if c['bounds'] != 'none':
        s += '-' + c['bounds']
    if c['pattern'] != 'dense':
        s += '-' + c['pattern']
    return s


def case_seed(c, salt=0):
    return 1000003 * c['n'] + 101 * c['m'] + 7 * c['me'] + salt


_CACHE = {}


def case_batch(c, batch=3, per=PER_DEFAULT, salt=0):
    """planted_batch of a table case, drawn once per process (read-only: do not modify)"""
    key = (case_id(c), batch, tuple(per), salt)
    if key not in _CACHE:
        with one_blas_thread():
            _CACHE[key] = planted_batch(case_seed(c, salt), c['n'], c['m'], c['me'], c['bounds'],
                                        c['pattern'], batch=batch, per=per, **c['kw'])
    return _CACHE[key]


def case_statement(c, i, batch=3, per=PER_DEFAULT, salt=0, **kw):
    """the statement's solve of instance i of a table case, once per process"""
    key = (case_id(c), batch, tuple(per), salt, i, tuple(sorted(kw.items())))
    if key not in _CACHE:
        qs = case_batch(c, batch, per, salt)[2]
        with one_blas_thread():
            _CACHE[key] = statement(qs[i], **kw)
    return _CACHE[key]


def truncation_k(c):
    """max_iter of section (d): three iterations short of the statement's earliest exit in the batch"""
    return min(case_statement(c, i)['iterations'] for i in range(3)) - 3
