/*
 * bqp.h — C ABI of the MI355X batched MPC QP solver (libbqp.so).
 *
 * Drop-in boundary for the per-step optimal-control solve of bevanda/Learning-Based-MPC.
 * The reference issues that solve through two MATLAB call surfaces; each entry point below
 * names the one it replaces:
 *
 *   fmincon(COSTFUN, opt_var, [],[],[],[],[],[], CONSFUN, options)
 *       matlab/LBMPC/functions/ocpLMPC.m:20-24      (LMPC, form F1)
 *       matlab/LBMPC/functions/ocpLBMPC.m:27-31      (LBMPC, form F3: Gauss-Newton SQP whose
 *                                                     QP sub-problems run in the dense kernel)
 *       matlab/trackingMPC/RunExample.m:134-136      (tracking MPC, form F5)
 *   solver('x0',..,'lbx',..,'ubx',..,'lbg',..,'ubg',..)  (CasADi nlpsol/IPOPT)
 *       matlab/LBMPC/examples/DMS_tracking_LMPC_casadi.m:163-167  (form F2)
 *       matlab/LBMPC/examples/DSS_tracking_LMPC_casadi.m:155-160
 *
 * Two solver entry points:
 *   bqp_solve_ocp_batched   structured stage-wise OCP (the fast path; Riccati KKT on GPU)
 *   bqp_quadprog_batched    MATLAB quadprog semantics on dense per-instance (H,f,A,b,Aeq,beq,lb,ub)
 * and *_device variants taking device pointers + a hipStream_t (passed as void*).
 *
 * Conventions
 *   - all matrices are column-major (MATLAB layout), fp64;
 *   - every input array carries an element stride between instances; stride 0 = one copy shared
 *     by the whole batch (broadcast);
 *   - return code: BQP_OK (0) or a negative BQP_E_* (API error: bad dims, HIP failure, missing
 *     GPU); per-instance status is exitflag[] with quadprog meanings:
 *       1 converged, 0 iteration limit, -2 primal infeasible, -3 dual infeasible/unbounded,
 *       -6 non-convex, -8 numerical failure;
 *   - thread safety: one bqp_handle per host thread / stream; no global mutable state.
 */
#ifndef BQP_H
#define BQP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BQP_OK 0
#define BQP_E_ARG (-1)       /* invalid dimensions / NULL required pointer */
#define BQP_E_HIP (-2)       /* HIP runtime error (allocation, launch, copy) */
#define BQP_E_NODEV (-3)     /* no usable gfx950 device */
#define BQP_E_UNSUPPORTED (-4) /* dimensions outside the compiled kernel set */

typedef struct bqp_handle_s* bqp_handle;

typedef struct {
    int max_iter;      /* default 50 */
    double tol_stat;   /* stationarity inf-norm / (1 + |cost gradient|_inf), default 1e-8 */
    double tol_feas;   /* primal residual inf-norm / (1 + |bounds, rhs|_inf), default 1e-10 */
    double tol_comp;   /* average complementarity mu (absolute), default 1e-14 */
    double tau;        /* fraction-to-boundary, default 0.995.  At tau >= 0.995 the structured
                          solver's step rule lets the corrector step go to 0.99999 of the boundary
                          on a well-centred iterate; a smaller tau bounds every
                          step */
    int precision;     /* structured API: 0 = fp64 (default); 1 = fp32 solver arithmetic/LDS state
                          (inputs and outputs stay fp64; tolerances floored at 1e-5 / 1e-6 / 1e-9);
                          2 = mixed: an fp32 launch to those floored tolerances, then an fp64 launch
                          that continues every instance from its fp32 iterate to the fp64
                          tolerances (fp64 results; instances the fp32 phase ends with -2/-8,
                          or whose continuation does not converge, restart in fp64); applies to
                          long horizons (N >= 64), shorter ones are solved in fp64.  In mixed
                          mode max_iter applies per phase, and bqp_output.iterations counts the
                          fp32 + fp64 iterations of a continued instance, or only the fp64
                          restart's iterations for an instance that restarts */
    int want_duals;    /* reserved (set 0): the structured API writes the multiplier outputs
                          whenever its `duals` argument is non-NULL */
    int polish;        /* structured API, fp64 active-set polish: the rows with lam > t are solved
                          as equalities (augmented-Lagrangian steps and conjugate gradients on
                          their multipliers, on the Riccati factorisation with weight rho on
                          the active rows, with active-set corrections) and the result replaces
                          the interior-point iterate if it passes the KKT checks
                          (bqp_output.polished).  It runs in a separate repair launch over the
                          instances the solve launch marks, so the solve kernel carries no
                          polish state.
                          0 (default) or 1: after an iteration-limit or numerical-failure exit
                          (e.g. multipliers ~1e3-1e5 drive D = lam/t out of fp64 range);
                          2: also when a row is left weakly active (slack and multiplier both
                          above 1e-10); 3 (SQP routines bqp_lbmpc_* / bqp_closed_loop_sqp;
                          the closed loop's default): the sub-problems are polished only once
                          the SQP has stalled at a step; -1: off (interior-point iterate only) */
} bqp_options;

typedef struct {
    int iterations;
    double constrviolation;  /* max(primal eq, primal ineq) at exit */
    double firstorderopt;    /* stationarity inf-norm at exit */
    double mu;               /* average complementarity at exit */
    double kkt[4];           /* stationarity, primal eq, primal ineq (inf-norms of the solver's
                                residuals at exit), complementarity (average t.lam = mu) */
    int polished;            /* 1: the answer is the active-set polish (bqp_options.polish) */
} bqp_output;

/* ------------------------------------------------------------------------------------------
 * Structured OCP (form F1/F2/F4/F5 after the host shim's change of variables):
 *
 *   x_{k+1} = A x_k + B u_k + c              k = 0..N-1,   x_0 = x0 (fixed)
 *             (A_k x_k + B_k u_k + c_k with bqp_ocp_dims.stage_models = 1)
 *   theta  in R^np  (global steady-state parameter, free)
 *   min  sum_{k=0}^{N} 0.5 v_k' W_k v_k + w_k' v_k,  v_k = [x_k; u_k; theta]  (nv = nx+nu+np;
 *        for k = N the u block of W_N / w_N is ignored)
 *   s.t. xlb_k <= x_k <= xub_k (k = 1..N),  ulb_k <= u_k <= uub_k (k = 0..N-1)  (+-INFINITY ok)
 *        Fp [x_kp; u_kp; theta] <= hp     (n_poly rows, polytope at stage kp = poly_stage)
 *
 * Reference mapping: costLMPC.m:20-45 / constraintsLMPC.m:15-41 (F1),
 * DMS_tracking_LMPC_casadi.m:223-287 (F2), trackingMPC/costFunction.m:20-39 /
 * constraintsFunction.m:20-38 (F5); the terminal polytope is term_set.mat's F_w_N (616x5).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int nx, nu, np, N;
    int n_poly;      /* rows of the polytope block (>= 0) */
    int poly_stage;  /* stage the polytope acts on, 0..N */
    int stage_models; /* 0 (a zero-initialised caller): A, B, c are one model for the whole horizon.
                         1: per-stage models (linear time-varying),
                             x_{k+1} = A_k x_k + B_k u_k + c_k,
                         A holds N blocks nx*nx (stage k's block at A + k*nx*nx maps x_k to
                         x_{k+1}), B N blocks nx*nu, c N blocks nx (NULL = 0).  Strides sA / sB /
                         sc: 0 = one schedule shared by the batch, otherwise >= N*nx*nx (N*nx*nu,
                         N*nx); a smaller non-zero stride is BQP_E_ARG.  fp64 only: with
                         bqp_options.precision 1 or 2 the call returns BQP_E_UNSUPPORTED.  The
                         active-set polish's repair launch carries the per-stage models (it runs
                         on the same Riccati routines as the solve, each reading stage k's A_k,
                         B_k, c_k), so bqp_options.polish means what it means with one model.
                         bqp_ocp_duals.pi is written against the
                         stage's own A_k, B_k.  bqp_solve_ocp_batched[_device] only: the closed-loop
                         routines return BQP_E_UNSUPPORTED.  Any other value is BQP_E_ARG */
} bqp_ocp_dims;

typedef struct {
    const double* A;    /* nx*nx      (stage_models = 1: N blocks) stride sA  */
    const double* B;    /* nx*nu      (stage_models = 1: N blocks) stride sB  */
    const double* c;    /* nx, NULL = 0 (stage_models = 1: N blocks) stride sc  */
    const double* W;    /* (N+1) blocks nv*nv                     stride sW  */
    const double* w;    /* (N+1)*nv, NULL = 0                     stride sw  */
    const double* xlb;  /* (N+1)*nx, NULL = -inf (stage 0 unused) stride sxb */
    const double* xub;  /* (N+1)*nx, NULL = +inf                  stride sxb */
    const double* ulb;  /* N*nu, NULL = -inf                      stride sub */
    const double* uub;  /* N*nu, NULL = +inf                      stride sub */
    const double* Fp;   /* n_poly*nv (column-major, n_poly rows)  stride sFp */
    const double* hp;   /* n_poly                                 stride shp */
    const double* x0;   /* nx                                     stride sx0 */
    int64_t sA, sB, sc, sW, sw, sxb, sub, sFp, shp, sx0;
    const int* skip;    /* batch ints, NULL (a zero-initialised caller) = solve every instance;
                           with bqp_ocp_dims.stage_models = 1 an instance with skip[i] != 0 is
                           not solved and none of its outputs is written (finished instances
                           of an outer iteration).  Non-NULL with stage_models = 0 is
                           BQP_E_UNSUPPORTED */
    /* Soft state bounds (both NULL, a zero-initialised caller: every bound is hard).  With weights
     * l1 = xs_lin, l2 = xs_quad >= 0 per state variable and stage the problem becomes
     *   min cost + sum_{k=1..N, i, side} (l1_{k,i} s + 0.5 l2_{k,i} s^2)
     *   s.t. xlb_{k,i} - s^l_{k,i} <= x_{k,i} <= xub_{k,i} + s^u_{k,i},  s >= 0
     * (an exact L1 plus quadratic penalty; each finite side has its own slack; a variable whose
     * weights are both 0 keeps hard bounds; input bounds and polytope rows are always hard).
     * Each array is (N+1)*nx (stage 0 unused), stride sxs (0 = shared by the batch, otherwise
     * >= (N+1)*nx); either pointer NULL = zeros.  A negative or non-finite weight is BQP_E_ARG on
     * the host entry points; on the device entry points it is the caller's duty.
     * fval includes the penalty; bqp_output.constrviolation measures the softened rows
     * (x - s <= xub), not the slack; the softened rows' stationarity l1 + l2 s - lam - nu joins the
     * stop test and bqp_output.firstorderopt.  Limits: fp64 only (bqp_options.precision 1 or 2
     * returns BQP_E_UNSUPPORTED); bqp_options.polish is taken as -1 and bqp_output.polished is 0 (an
     * active-set polish of softened rows does not exist yet); one model or
     * stage_models = 1, N <= 127, both families; honoured by bqp_closed_loop_ocp and
     * bqp_closed_loop_track, while bqp_closed_loop_lbmpc returns BQP_E_UNSUPPORTED; no MEX field. */
    const double* xs_lin;
    const double* xs_quad;
    int64_t sxs;
} bqp_ocp_data;

/* Optional multiplier outputs of the structured solve (NULL members are skipped).  Sign
 * convention: the Lagrangian is  cost + sum_k pi_k'(A x_k + B u_k + c - x_{k+1})
 * + sum lam_upper (v - ub) + sum lam_lower (lb - v) + lam_p'(Fp v - hp), all lam >= 0. */
typedef struct {
    double* pi;     /* batch*N*nx: dynamics multipliers for x_{k+1} = A x_k + B u_k + c   */
    double* lam_x;  /* batch*(N+1)*nx*2: [lower, upper] per stage (0 for absent bounds) */
    double* lam_u;  /* batch*N*nu*2                                                    */
    double* lam_p;  /* batch*n_poly                                                    */
    double* s_x;    /* batch*(N+1)*nx*2, layout of lam_x: the slacks of the softened state rows
                       (bqp_ocp_data.xs_lin / xs_quad), 0 for hard or absent rows; written by a
                       soft solve only.  lam_x of a softened row is the multiplier of the softened
                       row; at the optimum it lies in [0, l1 + l2 s] */
} bqp_ocp_duals;

/* Lifecycle.  device < 0 selects the current HIP device. */
int bqp_create(bqp_handle* h, int device);
int bqp_destroy(bqp_handle h);
void bqp_default_options(bqp_options* opt);
const char* bqp_version(void);
/* SHA-1 of the sources the library was built from (csrc files in name order, then include/bqp.h) */
const char* bqp_build_source_sha1(void);

/* Host-pointer structured solve.  Outputs (host): x batch*(N+1)*nx, u batch*N*nu,
 * theta batch*np, fval batch, exitflag batch, out batch (out/fval/duals may be NULL). */
int bqp_solve_ocp_batched(bqp_handle h, const bqp_ocp_dims* dims, int batch,
                          const bqp_ocp_data* data, const bqp_options* opt,
                          double* x, double* u, double* theta, double* fval, int* exitflag,
                          bqp_output* out, const bqp_ocp_duals* duals);

/* Device-pointer structured solve (all data/output pointers are device memory owned by the
 * caller; stream is a hipStream_t, NULL = default stream).  Asynchronous: returns after the
 * launch; synchronise the stream before reading outputs. */
int bqp_solve_ocp_batched_device(bqp_handle h, const bqp_ocp_dims* dims, int batch,
                                 const bqp_ocp_data* data, const bqp_options* opt,
                                 double* x, double* u, double* theta, double* fval,
                                 int* exitflag, bqp_output* out, const bqp_ocp_duals* duals,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * quadprog-compatible dense batched solve:
 *   [x,fval,exitflag,output,lambda] = quadprog(H,f,A,b,Aeq,beq,lb,ub,x0,options)
 *   min 0.5 x'Hx + f'x  s.t.  A x <= b, Aeq x = beq, lb <= x <= ub.
 * H n*n, f n, A m*n, b m, Aeq me*n, beq me, lb/ub n (NULL = unbounded), x0 ignored (IPM).
 * lambda outputs follow quadprog: H x + f + A'l_ineqlin + Aeq'l_eqlin - l_lower + l_upper = 0.
 * H: as quadprog, the host entry solves with the symmetric part (H + H')/2 (a symmetric H is
 * used bit for bit); the _device entry takes H as given and requires it symmetric (the kernels
 * read both triangles).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int n;   /* variables */
    int m;   /* inequality rows */
    int me;  /* equality rows */
} bqp_dims;

typedef struct {
    int64_t sH, sf, sA, sb, sAeq, sbeq, slb, sub;  /* element strides, 0 = shared */
} bqp_strides;

int bqp_quadprog_batched(bqp_handle h, const bqp_dims* d, int batch, const bqp_strides* st,
                         const double* H, const double* f, const double* A, const double* b,
                         const double* Aeq, const double* beq, const double* lb,
                         const double* ub, const double* x0, const bqp_options* opt,
                         double* x, double* fval, int* exitflag, double* lam_ineqlin,
                         double* lam_eqlin, double* lam_lower, double* lam_upper,
                         bqp_output* out);

int bqp_quadprog_batched_device(bqp_handle h, const bqp_dims* d, int batch,
                                const bqp_strides* st, const double* H, const double* f,
                                const double* A, const double* b, const double* Aeq,
                                const double* beq, const double* lb, const double* ub,
                                const bqp_options* opt, double* x, double* fval, int* exitflag,
                                double* lam_ineqlin, double* lam_eqlin, double* lam_lower,
                                double* lam_upper, bqp_output* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Learning-based MPC (forms F3/F4): the learned prediction model
 *   x+ = A x + B u + g(x, u),  g = Nadaraya-Watson oracle over a data window (oracleL2NW.m)
 * makes the per-step problem an NLP; it is solved by a Gauss-Newton SQP whose QP sub-problems
 * run in the dense kernel.  Replaces
 *   fmincon(costLBMPC, constraintsLBMPC)   matlab/LBMPC/functions/ocpLBMPC.m:27-31   (F3)
 *   solver(..., 'p', data)                 matlab/LBMPC/examples/hybrid_LBMPC_casadi.m:173-178 (F4)
 *   oracleL2NW(x, u, data)                 matlab/LBMPC/functions/oracleL2NW.m:1-36
 *
 * Decision z = [v_0..v_{N-1}; theta] (n = N*nu + np) with the rollout input u_k = K x_k + v_k
 * (F3: v = c, K = Kstabil; F4: v = u - u_eq, K = 0), deviation coordinates.  Cost:
 *   sum_{k < n_run} |Lq (x^L_k - LAMBDA th)|^2 + |Lr (u^L_k - PSI th)|^2
 *     + |Lp (x^T_N - LAMBDA th)|^2 + |Lt (LAMBDA th - xs)|^2
 * on the LEARNED rollout x^L (terminal x^T = learned or nominal x_N), subject to the condensed
 * NOMINAL-model constraints Ain z <= bin (the host shim builds them from constraintsLBMPC.m /
 * hybrid_LBMPC_casadi.m:283-310).  The NW window is 7 x q column-major per instance: rows 1-3
 * X = [dx1; dx2; du], rows 4-7 Y (hybrid_LBMPC_casadi.m:128 layout; no validity mask), or with
 * mask = 1 the 8 x q window of DMS_LBMPC_casadi.m:158-161 whose row 8 is the validity v of
 * casadiL2NW.m:14-28 (normaliser lambda + sum_j v_j k_j).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int nx, nu, np, N;
    int n_run;          /* running-cost stages k = 0..n_run-1 (F3: N-2, costLBMPC.m:30; F4: N) */
    int term_learned;   /* terminal P cost on the learned (1, F3) or nominal (0, F4) x_N */
    int q;              /* points in the NW window (<= 512) */
    int m;              /* rows of Ain */
    int mask;           /* 0: 7 x q window, every point counts; 1: 8 x q window with validity row */
    int hessian;        /* 0: Gauss-Newton; 1: + the second-order term of the learned dynamics
                           (costate-weighted NW Hessians) whenever the sum is positive definite
                           (Cholesky pivots > 1e-10 max|H_ii|), Gauss-Newton otherwise.  GN
                           converges linearly (rate ~0.5) on DMS_LBMPC_casadi.m's learned-state
                           costs: 60-200 SQP iterations against 4-6 with 1.  The exact
                           term needs n = N nu + np <= 127 (its n x n sum lives in LDS);
                           longer horizons run Gauss-Newton */
} bqp_lbmpc_dims;

typedef struct {
    const double *A, *B, *K;          /* nx*nx, nx*nu, nu*nx (column-major), shared */
    const double *Lq, *Lr, *Lp, *Lt;  /* upper-triangular ROW-major weight factors:
                                         Lq'Lq = w Q, Lr'Lr = w R (w = running weight), Lp'Lp = P, Lt'Lt = T */
    const double *LAMBDA, *PSI, *xs;  /* nx*np, nu*np (column-major), nx */
    const double* data; int64_t sdata;  /* NW window (7 or 8)*q per instance (stride; 0 = shared) */
    const double* x0;   int64_t sx0;    /* nx per instance */
    const double* Ain;                  /* m*n column-major, shared */
    const double* bin;  int64_t sbin;   /* m per instance */
    double bandwidth, lambda;           /* NW kernel; <= 0 selects the reference's 0.5, 1e-3 */
} bqp_lbmpc_data;

/* Batched NW oracle: g (batch*4) and optionally dg/dxi (batch*4*3, row-major per instance) at
 * the query points xi (batch*3). */
int bqp_nw_oracle(bqp_handle h, int batch, int q, const double* data, int64_t sdata,
                  const double* xi, double* g, double* dg, double bandwidth, double lambda);
int bqp_nw_oracle_device(bqp_handle h, int batch, int q, const double* data, int64_t sdata,
                         const double* xi, double* g, double* dg, double bandwidth,
                         double lambda, void* stream);

/* SQP solve.  z (batch*n): in = start (fmincon's opt_var warm start), out = solution; lam
 * (batch*m, may be NULL): multipliers of Ain z <= bin; cost (batch, may be NULL); exitflag:
 * 1 converged, 0 iteration limit (opt->max_iter SQP iterations), -2 QP sub-problem infeasible,
 * -8 numerical failure.  The _device variant synchronises its stream every 4 SQP iterations
 * (early exit when the whole batch has converged). */
int bqp_lbmpc_solve_batched(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                            const bqp_lbmpc_data* data, const bqp_options* opt, double* z,
                            double* lam, double* cost, int* exitflag, int* iterations);
int bqp_lbmpc_solve_batched_device(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                                   const bqp_lbmpc_data* data, const bqp_options* opt, double* z,
                                   double* lam, double* cost, int* exitflag, int* iterations,
                                   void* stream);

/* The SQP's model at a given z (batch*n, read only), for tests and diagnostics: the launches of
 * one SQP iteration that form the QP sub-problem (rollout with sensitivities, normal equations,
 * with d->hessian = 1 and n <= 127 the exact-Hessian kernel) and, with dstep (batch*n, may be
 * NULL), the line search's trial rollouts; neither the QP solve nor the update runs.  Every
 * output may be NULL:
 *   cost  (batch)         the cost at z
 *   Jr    (batch*nr*n)    residual Jacobian, row-major nr x n per instance,
 *                         nr = n_run (nx + nu) + 2 nx.  Row order: per running stage k < n_run
 *                         the nx rows Lq (x^L_k - LAMBDA th), then the nu rows Lr (u^L_k - PSI th);
 *                         then the nx rows Lp (x^T_N - LAMBDA th); then the nx rows
 *                         Lt (LAMBDA th - xs).  cost = |er|^2
 *   er    (batch*nr)      the residuals, in the same order
 *   H     (batch*n*n)     the QP sub-problem's Hessian, n x n per instance with BOTH triangles
 *                         written and exactly symmetric (so row- and column-major coincide).
 *                         hused = 0: the Gauss-Newton 2 Jr'Jr.  hused = 1: the exact one,
 *                         2 Jr'Jr + sum_k Xi_k' W_k Xi_k, plus the grid shift 1e-12 hd 4^k on its
 *                         diagonal where it needed one to be positive definite (hd = max|H_ii|)
 *   f     (batch*n)       gradient 2 Jr'er
 *   rhs   (batch*m)       bin - Ain z
 *   hused (batch)         1 where H is the exact Hessian; 0 with d->hessian = 0, with n > 127
 *                         (silently Gauss-Newton), or where no grid shift made it definite
 *   Jr2, Tr2 (batch*3N*n) row-major 3N x n per instance, rows 3k..3k+2: Xi_k = d[x_1; x_2; u]_k/dz
 *                         and W_k Xi_k (W_k = sum_i p_{k+1,i} d2g_i).  Written only where the
 *                         exact-Hessian kernel runs (d->hessian = 1 and n <= 127)
 *   costT (batch*8)       the cost at z + 2^-t dstep, t = 0..7.  Written only with dstep */
int bqp_lbmpc_linearize(bqp_handle h, const bqp_lbmpc_dims* d, int batch, const bqp_lbmpc_data* data,
                        const double* z, const double* dstep, double* cost, double* Jr, double* er,
                        double* H, double* f, double* rhs, int* hused, double* Jr2, double* Tr2,
                        double* costT);
int bqp_lbmpc_linearize_device(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                               const bqp_lbmpc_data* data, const double* z, const double* dstep,
                               double* cost, double* Jr, double* er, double* H, double* f,
                               double* rhs, int* hused, double* Jr2, double* Tr2, double* costT,
                               void* stream);

/* ------------------------------------------------------------------------------------------
 * Closed-loop simulation: per time step, the batched structured solve at
 * the measured states, then one step of the true plant with the first input - the loop of
 * DMS_tracking_LMPC_casadi.m:153-189 / DSS_tracking_LMPC_casadi.m (solver(...), then
 * xmeasure = dynamic(delta, xmeasure, u_OL(1:m))) for a whole batch of initial states.
 * The OCP is posed in deviation coordinates around (x_eq, u_eq); data->x0 is ignored (the
 * measured states are fed back).  x_init (batch*nx), X (batch*(steps+1)*nx) and
 * U (batch*steps*nu) are absolute; exitflag (batch*steps, may be NULL) per solve.
 * Plant BQP_PLANT_MG_RK4: Moore-Greitzer `system` (:215-221) under one RK4 step of length
 * delta (`dynamic`, :297-304); nx = 4, nu = 1.  BQP_PLANT_MG_ODE23: the same model integrated
 * over delta by MATLAB's ode23 at its default options (RelTol 1e-3, AbsTol 1e-6, MaxStep
 * delta/10) - models/trueModel.m:14/48 behind functions/transitionTrue.m, the plant of the
 * fmincon loops (functions/ocpLMPC.m:11-40, ocpLBMPC.m); with bqp.LMPC's problem this runs
 * examples/LMPC_RunExample.m's loop.
 *
 * Per-instance plant coefficients (plant_par; models/trueModel.m:32-41 names them wn, zeta, beta,
 * x2_c): p = [x2_c, 1/beta^2, wn^2, 2 zeta wn] in
 *   f0 = -x1 + p0 + 1 + 3 (x0/2) - x0^3/2        f2 = x3
 *   f1 = (x0 + 1 - x2 sqrt(x1)) p1               f3 = -p2 x2 - p3 x3 + p2 u
 * with the nominal plant p = [0, 1, 1000, 2 sqrt(500)].  Honoured, with both MG plants wherever the
 * loop admits them, by every closed loop below: bqp_closed_loop_ocp, _lbmpc (the window's Y and XL
 * then see the perturbed plant), _sqp, _track (MG plants; BQP_PLANT_LINEAR has Ap, Bp and returns
 * BQP_E_ARG), _nmpc and _nmpc_track (every route, both loop modes; the model inside the solve
 * stays nominal), host and _device forms.  plant_par = NULL launches exactly the kernels it
 * launched before the member existed.  The host entries return BQP_E_ARG for a non-finite
 * coefficient, p1 <= 0, p2 <= 0, p3 < 0, a stride that is neither 0 nor at least one instance's
 * block, and a plant_par_sched other than 0 or 1; on the _device entries the values are the
 * caller's duty, as for x_eq.  No MEX field.
 * ---------------------------------------------------------------------------------------- */
#define BQP_PLANT_MG_RK4 1
#define BQP_PLANT_MG_ODE23 2
typedef struct {
    int plant;           /* BQP_PLANT_MG_RK4 or BQP_PLANT_MG_ODE23 (bqp_closed_loop_track: also
                            BQP_PLANT_LINEAR) */
    int steps;           /* closed-loop steps (mpciterations) */
    double delta;        /* plant step (s) */
    const double* x_eq;  /* nx working point (device memory in the _device variant) */
    const double* u_eq;  /* nu */
    /* trailing members: a zero-initialised structure is the loop as it was */
    const double* plant_par;   /* NULL: the nominal plant, every kernel as before (device memory
                                  in the _device variant) */
    int64_t       splant_par;  /* doubles between two instances' parameters; 0 = shared by the batch */
    int           plant_par_sched; /* 0: 4 doubles per instance, constant over the loop;
                                      1: steps*4 per instance, row t is the plant that takes
                                      X[b,t] to X[b,t+1]; row `steps` is never read */
} bqp_closed_loop;

int bqp_closed_loop_ocp(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* data,
                        const bqp_options* opt, const bqp_closed_loop* cl, const double* x_init,
                        double* X, double* U, int* exitflag);
int bqp_closed_loop_ocp_device(bqp_handle h, const bqp_ocp_dims* d, int batch,
                               const bqp_ocp_data* data, const bqp_options* opt,
                               const bqp_closed_loop* cl, const double* x_init, double* X,
                               double* U, int* exitflag, void* stream);

/* ------------------------------------------------------------------------------------------
 * LBMPC closed loop with the learned model's data window: the data
 * acquisition of matlab/LBMPC/examples/DMS_LBMPC_casadi.m:198-207 around a structured QP
 * solve (LBMPC_casadi.m:163-218).  Per step: the structured solve at the
 * measured state, the plant step, then the data acquisition of the reference -
 *   X = [dx1; dx2; du], Y = (x+ - x_eq) - (A dx + B du)          (:202-206, deviation coords)
 *   window <- get_data(X, Y, q, it, window)                     (utilities/get_data.m)
 * and the logged learned prediction xl = x_eq + A dx + B du + g(X, Y, v) with the window before
 * the update (:199, casadiL2NW.m).  The per-step OCP is the QP the caller poses in `data`: the
 * loop of matlab/LBMPC/examples/LBMPC_casadi.m (its learned dynamics are commented out of the
 * constraints, :292, so the per-step problem is the tracking QP with F_x_d and the terminal set
 * on x_1, polytope at stage 1; the window drives xl).  The learned-model NLP loop of
 * DMS_LBMPC_casadi.m, whose cost reads the learned states, is bqp_closed_loop_sqp below.  A, B of
 * the window update are data->A / data->B.  Same loop and outputs as bqp_closed_loop_ocp, plus: */
typedef struct {
    int q;               /* points in the data window (get_data.m's q) */
    int mask;            /* 1: 8 x q window with validity row v, only the first (zero) point valid
                            at the start (DMS_LBMPC_casadi.m:160-161); 0: every point counts (the
                            7-row window of hybrid_LBMPC_casadi.m:160) */
    double bandwidth, lambda;  /* NW kernel; <= 0 selects the reference's 0.5, 1e-3 */
    double* XL;          /* out: batch*(steps+1)*nx learned predictions xl (XL[:,0] = x_init) */
    double* window;      /* out, may be NULL: batch*q*8 final windows, [X; Y; v] per point, ring
                            order (iteration it's sample in point it mod q) */
} bqp_learning;

int bqp_closed_loop_lbmpc(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* data,
                          const bqp_options* opt, const bqp_closed_loop* cl,
                          const bqp_learning* lw, const double* x_init, double* X, double* U,
                          int* exitflag);
int bqp_closed_loop_lbmpc_device(bqp_handle h, const bqp_ocp_dims* d, int batch,
                                 const bqp_ocp_data* data, const bqp_options* opt,
                                 const bqp_closed_loop* cl, const bqp_learning* lw,
                                 const double* x_init, double* X, double* U, int* exitflag,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Learned-model NLP closed loop: per time step the batched SQP of
 * bqp_lbmpc_solve_batched at the measured states, one plant step with the first input, and the
 * data acquisition of the reference into each instance's window - the loops of
 *   matlab/LBMPC/examples/DMS_LBMPC_casadi.m:163-218   (d->mask = 1, lw->mask = 1: 8 x q window,
 *       learned states in the cost incl. the terminal term: term_learned = 1, K = 0, n_run = N)
 *   matlab/LBMPC/examples/hybrid_LBMPC_casadi.m:163-204 (F4: term_learned = 0, K = 0, n_run = N;
 *       7-row window: lw->mask = 0 keeps every point valid)
 *   matlab/LBMPC/examples/LBMPC_RunExample.m / functions/ocpLBMPC.m (F3: K = Kstabil)
 * The solver's window is the loop's own ring buffer (8 doubles per point, data->data, data->sdata,
 * data->x0 and data->bin are ignored): get_data.m's window with its columns in ring order (the NW
 * sums do not depend on the column order).  The condensed nominal constraints of each step are
 *   Ain z <= bin0 + Bx dx0   (dx0 = measured state - x_eq; bin0: m, Bx: m*nx column-major),
 * the first input applied is u_0 = u_eq + K dx0 + z_0.  Warm start (warm = 1): the previous
 * solution shifted one stage with a zero last move and the same theta (the scripts' guess
 * u0 = [u_OL(2:end); u_eq + Kstabil x_N], DMS_LBMPC_casadi.m:209-213, with the tail move of the
 * scripts' Kstabil = 0 case); warm = 0: z = 0 every step (u = u_eq, theta = 0).  opt->max_iter
 * bounds the SQP iterations per step.  The NW kernel parameters are lw->bandwidth / lw->lambda
 * when > 0, else data->bandwidth / data->lambda, else the reference's 0.5 / 1e-3.  X, U, exitflag
 * and lw->XL / lw->window as in bqp_closed_loop_lbmpc; Z (batch*steps*n, may be NULL): every step's SQP solution z;
 * iterations (batch*steps, may be NULL): SQP iterations per step.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    const double* bin0;  /* m */
    const double* Bx;    /* m * nx, column-major */
    int warm;
    double* Z;           /* out, may be NULL */
    int* iterations;     /* out, may be NULL */
} bqp_sqp_loop;

int bqp_closed_loop_sqp(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                        const bqp_lbmpc_data* data, const bqp_sqp_loop* sl,
                        const bqp_options* opt, const bqp_closed_loop* cl, const bqp_learning* lw,
                        const double* x_init, double* X, double* U, int* exitflag);
int bqp_closed_loop_sqp_device(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                               const bqp_lbmpc_data* data, const bqp_sqp_loop* sl,
                               const bqp_options* opt, const bqp_closed_loop* cl,
                               const bqp_learning* lw, const double* x_init, double* X, double* U,
                               int* exitflag, void* stream);

/* ------------------------------------------------------------------------------------------
 * Closed loop with a reference schedule and a linear plant: the loop of
 *   matlab/trackingMPC/RunExample.m:131-147  ("MPC for tracking piecewise constant references":
 *       xs = set_ref(k), the F5 solve, x = getTransitions(x, u_0), art_refHistory)
 * and of RunExample_robust.m (the same with an additive disturbance), for a whole batch; the
 * schedule also moves the set-point of the Moore-Greitzer tracking loops above.
 * Per step t the linear term of the structured solve is
 *   w_t = w + Wr r_t      (w = data->w, NULL = 0: shared or per instance; r_t = ref[b, t, :])
 * so a reference enters exactly as a per-instance data->w would (for F5 only the theta block of
 * stage N is non-zero: -2 [0 0 LAMBDA]' T, costFunction.m:261).  With nr = 0 every step solves
 * `data` as it is.  Plant BQP_PLANT_LINEAR:
 *   x+ = x_eq + Ap (x - x_eq) + Bp (u - u_eq) + d_t     (d_t = dist[b, t, :])
 * for any (nx, nu, np) the structured solve accepts; cl->delta is not used.  Ap, Bp and dist
 * belong to that plant alone: with the MG plants (nx = 4, nu = 1) a non-NULL one is BQP_E_ARG.
 * cl->plant_par belongs to the MG plants alone: with BQP_PLANT_LINEAR a non-NULL one is BQP_E_ARG.
 * Otherwise as bqp_closed_loop_ocp: data->x0 is ignored (and may be NULL), a step whose solve
 * ends != 1 still applies the solver's u_0, the loop's time goes to bqp_last_kernel_ms.
 * ---------------------------------------------------------------------------------------- */
#define BQP_PLANT_LINEAR 3
typedef struct {
    const double* Ap;  int64_t sAp;    /* nx*nx column-major; NULL = data->A (stride data->sA) */
    const double* Bp;  int64_t sBp;    /* nx*nu column-major; NULL = data->B (stride data->sB) */
    const double* dist; int64_t sdist; /* steps*nx per instance, NULL = 0; stride 0 = shared */
    int nr;                            /* reference dimension (0: no schedule) */
    const double* Wr;                  /* (N+1)*nv x nr column-major, shared */
    const double* ref; int64_t sref;   /* steps*nr per instance; stride 0 = one schedule */
    double* THETA;                     /* out, may be NULL: batch*steps*np, the theta of every
                                          step's solve (art_refHistory up to Mtheta) */
} bqp_track;

int bqp_closed_loop_track(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* data,
                          const bqp_options* opt, const bqp_closed_loop* cl, const bqp_track* tr,
                          const double* x_init, double* X, double* U, int* exitflag);
int bqp_closed_loop_track_device(bqp_handle h, const bqp_ocp_dims* d, int batch,
                                 const bqp_ocp_data* data, const bqp_options* opt,
                                 const bqp_closed_loop* cl, const bqp_track* tr,
                                 const double* x_init, double* X, double* U, int* exitflag,
                                 void* stream);

/* ------------------------------------------------------------------------------------------
 * Nonlinear MPC on the true Moore-Greitzer model: the NLP of
 *   matlab/LBMPC/examples/DMS_tracking_NMPC_casadi.m:121-126, 225-293
 * with the states eliminated (single shooting).  Decision z = [u_0 - u_eq, .., u_{N-1} - u_eq;
 * theta], n = N + 1 (nx = 4, nu = 1, np = 1), N <= 127.
 *   dynamics    x_{k+1} = dynamic(delta, x_k, u_k): one RK4 step of `system` (:217-223, :286-293),
 *               the plant BQP_PLANT_MG_RK4 steps; x_0 = the measured state (absolute)
 *   cost        sum_{k<N} [(x_k - x_eq - LAMBDA th)'(delta Q)(.) + (u_k - u_eq - PSI th)'(delta R)(.)]
 *               + (x_N - x_eq - LAMBDA th)'P(.) + (LAMBDA th - rho)'T(LAMBDA th - rho),
 *               rho = x_ref - x_eq the set-point (bqp_nmpc_data.x_ref; 0 without one)
 *   rows c(z) <= 0, in this order: for k = 1..N  F_x (x_k - x_eq) - h_x (mx rows), then
 *               F_u (u_{k-1} - u_eq) - h_u (mu rows); then F_T [x_N - x_eq; theta] - h_T (n_poly
 *               rows).  m = N (mx + mu) + n_poly: IPOPT's lam_g order without the dynamics rows.
 * Solved by a Gauss-Newton SQP with an L1 merit function: per iteration the rollout with the
 * stage Jacobians differentiated through the four RK stages (analytic Jacobian of `system`) and
 * the forward sensitivities, H = 2 Jr'Jr, f = 2 Jr'e, the sub-problem min 0.5 d'Hd + f'd s.t.
 * C d <= -c on the dense kernels with the instance's own C, eight trial steps alpha = 2^-t, the
 * penalty nu <- max(nu, 1.1 max lam), merit phi = J + nu sum max(c, 0).  The second-order terms of
 * the dynamics are not formed.  functions/ocpNMPC.m (fmincon around an ode23 rollout) is not
 * covered.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int N;        /* horizon, 1..127 */
    int mx, mu;   /* rows of F_x (<= 32) and F_u (<= 8) */
    int n_poly;   /* rows of F_T */
    int subproblem; /* how the SQP's sub-problems are solved.  0 (a zero-initialised caller): the
                       dense route above - condensed H, f and the instance's own C on the dense
                       kernels.  1: the stage route - the sub-problem stays in stage form, a linear
                       time-varying tracking QP in v_k = [dx_k; du_k; dtheta] with the rollout's
                       A_k, B_k (dx_0 = 0), the tracking cost's W_k shared by the batch, plain
                       bounds on dx_k and du_k and the terminal rows on [dx_N; dtheta], solved by
                       bqp_solve_ocp_batched_device with stage_models = 1; neither H nor C is
                       formed.  The stage route needs box rows: every row of F_x and of F_u has
                       exactly one non-zero entry and each (variable, side) at most one row; a
                       positive scale is allowed (a x_i <= h is the bound h / a, its multiplier
                       lam_bound / a).  Anything else returns BQP_E_UNSUPPORTED (the _device
                       entries read one flag back from the device for it before the first
                       round), as does an n_poly outside the structured kernel's compiled row
                       counts.  lam, exitflag, iterations and cost mean what they mean on the
                       dense route.  opt->polish goes to the structured solve as that solve
                       defines it (bqp_options.polish: 0 / 1 after a 0 / -8 exit, 2 also on a
                       weakly active row, -1 off; 3, the SQP routines' "after a stall", is taken
                       as 2 from the first iteration).  Honoured by bqp_nmpc_solve_batched[_device] and
                       bqp_closed_loop_nmpc[_device] in both loop modes; bqp_nmpc_linearize
                       ignores it.  Any other value is BQP_E_ARG */
    int shooting;   /* 0 (a zero-initialised caller): single shooting - the states are eliminated,
                       every SQP iterate is a rollout from the measured state.  1: direct multiple
                       shooting, the form of the reference's NLP (y = [x_0..x_N; u; theta], the
                       dynamics as equality rows): the states x_1..x_N stay decision variables (x_0
                       is pinned to the measured state), the iterate is (X, z), and the stage
                       sub-problem carries the defects c_k = dynamic(delta, x_k, u_k) - x_{k+1},
                         dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k du_k + c_k,
                       with A_k, B_k, w_k, the bounds and hp formed at the iterate's own x_k - the
                       structured solve's per-stage offset.  Merit function J + nu (V + E), V the
                       rows' violation, E = sum_k |c_k|_1, nu <- max(nu, 1.1 max(max lam, max |pi|));
                       the step test is over (dX, dz), feasibility is max(rows) <= 1e-9 and
                       max |c_k| <= 1e-9, stationarity the full-space residual of bqp_ocp_duals'
                       Lagrangian at the iterate against 10 tol (1 + |grad J|).  exitflag keeps its
                       meaning; a non-finite dynamic() at an accepted iterate is -8.  No kernel of a
                       round rolls out: the stages are linearised and the trial points evaluated
                       in parallel; only a solve that is given no states rolls out z once, for its
                       start.  Needs subproblem = 1; with subproblem = 0, with a weight in xs_lin /
                       xs_quad that softens a row, or with rows that are no box rows it returns
                       BQP_E_UNSUPPORTED.  Honoured by bqp_nmpc_solve_batched[_device] (which start
                       from the rollout of z and return z alone), bqp_nmpc_dms_solve_batched[_device]
                       and bqp_closed_loop_nmpc[_device] in both loop modes (warm start: z shifted,
                       x_k <- x_{k+1}, x_N <- dynamic(delta, x_N, u_{N-1}) with the repeated move);
                       bqp_nmpc_linearize, bqp_nmpc_stage_qp and bqp_nmpc_stage_cost do not read it.
                       No MEX field.  Any other value is BQP_E_ARG */
} bqp_nmpc_dims;

typedef struct {
    const double *Lq, *Lr, *Lp, *Lt;   /* upper-triangular ROW-major factors: Lq'Lq = delta Q (4x4),
                                          Lr'Lr = delta R (1x1), Lp'Lp = P, Lt'Lt = T (4x4) */
    const double *LAMBDA, *PSI;        /* 4, 1 */
    const double *x_eq, *u_eq;         /* 4, 1 */
    const double *F_x, *h_x;           /* mx*4 column-major, mx */
    const double *F_u, *h_u;           /* mu, mu */
    const double *F_T, *h_T;           /* n_poly*5 column-major ([x_N - x_eq; theta]), n_poly */
    double delta;                      /* RK4 step and running-cost weight (in Lq, Lr) */
    const double* x0; int64_t sx0;     /* measured states, absolute, 4 per instance */
    /* Soft state rows (both NULL, a zero-initialised caller: every row is hard, and every kernel
     * runs as it did before these members existed).  Each array holds mx doubles, one per row of
     * F_x, shared by the batch; either pointer NULL = zeros.  With weights l1_i = xs_lin[i],
     * l2_i = xs_quad[i] >= 0 and phi_i(s) = l1_i s + 0.5 l2_i s^2 the problem becomes
     *   min J(z) + sum_{k=1..N} sum_{i soft} phi_i(max(c_{k,i}(z), 0))   s.t.  c_hard(z) <= 0
     * (an exact L1 plus quadratic penalty).  A row with both weights 0 stays hard; the rows of F_u
     * and F_T are always hard, so a start from which the terminal set cannot be reached still ends
     * -2.  Stage route only: with subproblem = 0 the solve and loop entries return
     * BQP_E_UNSUPPORTED.  The sub-problem's softened bounds are the structured solve's soft state
     * bounds (bqp_ocp_data.xs_lin / xs_quad), which carry one weight pair per (stage, variable)
     * for both sides, in the variable's units: the row a (x_v - x_eq,v) <= h gives the pair
     * (l1 |a|, l2 a^2).  Hence the equal-pair rule: the two rows of one state variable must be
     * softened together and give the same pair, exactly (rows +-x_v with equal weights do; rows
     * scaled by a take l1 / |a| and l2 / a^2); one row softened and the other hard, or unequal
     * pairs, is BQP_E_UNSUPPORTED (found on the device with the box-row flag, before the first
     * round); a variable with a single row may be softened.
     * cost is J + penalty.  lam keeps its layout; on a softened row it is the multiplier of the
     * softened row, at the optimum in the subdifferential of phi_i: l1 + l2 c where c > 0, within
     * [0, l1] at c = 0, 0 where c < 0.  exitflag -2 is a sub-problem that is infeasible in its
     * hard rows; feasibility in the stopping test is that of the hard rows.
     * Limits: fp64; no active-set polish of the sub-problems (the structured solve takes polish
     * as -1 on a soft problem, so lam on softened rows is the interior point's, and the soft
     * sub-problems are solved to a stationarity of 1e-4 opt->tol_stat, at most the structured
     * solve's default, since nothing after them sharpens z); bqp_nmpc_linearize
     * and bqp_nmpc_stage_qp do not read the weights.  A negative or non-finite weight is
     * BQP_E_ARG on the host entry points; on the _device entry points it is the caller's duty.
     * Honoured by bqp_nmpc_solve_batched[_device], bqp_closed_loop_nmpc[_device] in both loop
     * modes, and bqp_nmpc_stage_cost; no MEX field. */
    const double* xs_lin;
    const double* xs_quad;
    /* Set-point of the tracking cost (NULL, a zero-initialised caller: the working point x_eq, and
     * every kernel runs as it did before these members existed).  x_ref holds 4 doubles per
     * instance, the target state x_s in absolute coordinates; sx_ref is the distance in doubles
     * between two instances' set-points, 0 = one set-point for the whole batch.  With
     * rho = x_s - x_eq the offset term of the cost, (LAMBDA th)'T(LAMBDA th), becomes
     *   (LAMBDA th - rho)'T(LAMBDA th - rho),
     * in residual form the four rows (Lt LAMBDA) th - Lt rho; everything else - the running and
     * terminal P cost, every row, the terminal set on [x_N - x_eq; theta] - is unchanged, and the
     * set-point is constant over the horizon.  rho need not lie on the steady-state line LAMBDA th;
     * a target the terminal set does not admit makes theta stop at that set's limit.  On the dense
     * route only cost, the T rows of the residual and f[N] change, on the stage route and with
     * multiple shooting only cost and the theta entry of w_N.  Honoured by bqp_nmpc_linearize,
     * bqp_nmpc_stage_qp, bqp_nmpc_dms_qp, bqp_nmpc_stage_cost, bqp_nmpc_solve_batched,
     * bqp_nmpc_dms_solve_batched (host and _device forms), on every route and with soft state
     * rows, and by the closed loops (bqp_closed_loop_nmpc: a constant set-point;
     * bqp_closed_loop_nmpc_track: a schedule).  On the dense route (subproblem = 0) a set-point
     * also holds the sub-problems to 1e-2 opt->tol_stat and, with opt->polish = 0, polishes a
     * sub-problem whose interior point ends 0 / -8 (opt->polish < 0 keeps the polish off): with
     * theta on a terminal row the interior point otherwise reports convergence 5e-6 from the
     * sub-problem's optimum.  A non-finite entry is BQP_E_ARG on the host entry
     * points; on the _device entry points it is the caller's duty.  No MEX field. */
    const double* x_ref;
    int64_t sx_ref;
} bqp_nmpc_data;

/* Rollout and linearisation at given z (batch*n).  Outputs, each may be NULL: X (batch*(N+1)*4,
 * absolute), cost (batch), c (batch*m), C (batch*m*n, column-major m x n per instance),
 * H (batch*n*n, column-major, symmetric), f (batch*n). */
int bqp_nmpc_linearize(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* data,
                       const double* z, double* X, double* cost, double* c, double* C, double* H,
                       double* f);
int bqp_nmpc_linearize_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                              const bqp_nmpc_data* data, const double* z, double* X, double* cost,
                              double* c, double* C, double* H, double* f, void* stream);

/* The stage sub-problem at given z (batch*n), as the stage route (subproblem = 1) hands it to the
 * structured solve - the diagnostic counterpart of bqp_nmpc_linearize; d->subproblem is not read,
 * the box-row restriction of the stage route applies.  Outputs, each may be NULL: A (batch*N*16,
 * column-major 4 x 4 blocks), B (batch*N*4), w (batch*(N+1)*6), xlb / xub (batch*(N+1)*4; stage 0
 * is -inf / +inf), ulb / uub (batch*N), hp (batch*n_poly), and the shared W ((N+1)*36) and
 * Fp (n_poly*6, column-major). */
int bqp_nmpc_stage_qp(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* data,
                      const double* z, double* A, double* B, double* w, double* xlb, double* xub,
                      double* ulb, double* uub, double* hp, double* W, double* Fp);
int bqp_nmpc_stage_qp_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                             const bqp_nmpc_data* data, const double* z, double* A, double* B,
                             double* w, double* xlb, double* xub, double* ulb, double* uub,
                             double* hp, double* W, double* Fp, void* stream);

/* The stage route's cost at given z (batch*n), as its stage linearisation forms it - diagnostic;
 * d->subproblem is not read, the box-row restriction and the soft rows' pairing rule apply.
 * cost (batch): J + penalty, what the merit function of the SQP starts from; penalty (batch): the
 * penalty of the softened rows at z, 0 without weights.  Host entry only. */
int bqp_nmpc_stage_cost(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* data,
                        const double* z, double* cost, double* penalty);

/* SQP solve.  z (batch*n): in = start, out = solution; lam (batch*m, may be NULL): multipliers
 * of the rows above; cost (batch, may be NULL); exitflag: 1 converged, 0 iteration limit
 * (opt->max_iter SQP iterations), -2 sub-problem infeasible, -8 numerical failure (a non-finite
 * accepted iterate included).  With subproblem = 0 the workspace holds every instance's C (m*n
 * doubles: 1.3 MB at N = 100 with 616 terminal rows); a batch that does not fit returns
 * BQP_E_HIP.  The stage route (subproblem = 1) keeps 79 KB per instance at N = 100 (325 MB for 4,096).  On the
 * dense route the sub-problems
 * are polished only with opt->polish > 0 (modes as bqp_lbmpc_solve_batched): on the warm starts
 * of the closed loop, which lie on active state rows, the polish can fail.  The _device
 * variant synchronises its stream while it polls for the batch's convergence. */
int bqp_nmpc_solve_batched(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                           const bqp_nmpc_data* data, const bqp_options* opt, double* z,
                           double* lam, double* cost, int* exitflag, int* iterations);
int bqp_nmpc_solve_batched_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                  const bqp_nmpc_data* data, const bqp_options* opt, double* z,
                                  double* lam, double* cost, int* exitflag, int* iterations,
                                  void* stream);

/* Multiple shooting (d->shooting must be 1, d->subproblem 1): the SQP solve with the states and the
 * dynamics multipliers.  X (batch*(N+1)*4, absolute): in = the states of the start, out = those of
 * the solution; X[:, 0] is overwritten with x0; X = NULL starts from the rollout of z (and returns
 * no states) - bqp_nmpc_solve_batched's start.  pi (batch*N*4, may be NULL): the multipliers of
 * x_{k+1} = dynamic(delta, x_k, u_k) in bqp_ocp_duals' sign convention; with lam, IPOPT's lam_g.
 * Everything else as bqp_nmpc_solve_batched. */
int bqp_nmpc_dms_solve_batched(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                               const bqp_nmpc_data* data, const bqp_options* opt, double* z, double* X,
                               double* lam, double* pi, double* cost, int* exitflag, int* iterations);
int bqp_nmpc_dms_solve_batched_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                      const bqp_nmpc_data* data, const bqp_options* opt, double* z,
                                      double* X, double* lam, double* pi, double* cost, int* exitflag,
                                      int* iterations, void* stream);

/* The multiple-shooting sub-problem at given states X (batch*(N+1)*4; stage 0 is taken from x0; NULL:
 * the rollout of z) and z (batch*n) - the diagnostic counterpart of bqp_nmpc_stage_qp, whose
 * outputs it has, and c (batch*N*4, may be NULL), the defects.  d->subproblem and d->shooting are
 * not read. */
int bqp_nmpc_dms_qp(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* data,
                    const double* X, const double* z, double* A, double* B, double* c, double* w,
                    double* xlb, double* xub, double* ulb, double* uub, double* hp, double* W, double* Fp);
int bqp_nmpc_dms_qp_device(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* data,
                           const double* X, const double* z, double* A, double* B, double* c, double* w,
                           double* xlb, double* xub, double* ulb, double* uub, double* hp, double* W,
                           double* Fp, void* stream);

/* Closed loop of DMS_tracking_NMPC_casadi.m:153-207 for a batch of initial states: per step the
 * solve at the measured state, the RK4 plant with u_0 (cl->plant must be BQP_PLANT_MG_RK4,
 * cl->delta the plant's step; data->x0 is ignored), then the warm start - z shifted one stage
 * with the last move repeated and theta kept.  Every instance advances at its own step: one round
 * is one SQP iteration of every instance that has steps to go (rollout, normal equations, dense
 * sub-problem, trial rollouts, update) and one advance launch that moves the instances whose SQP
 * stopped in this round to their next step, so the loop takes as many rounds as its slowest
 * instance needs over all steps, not the sum over the steps of the slowest instance of each.
 * With the environment variable BQP_NMPC_SYNC set (read at each call) the loop is step
 * synchronous instead - every step's SQP runs until the whole batch has stopped; per instance both
 * forms do the same operations in the same order and return the same bits.  steps = 0 is allowed
 * and returns X = x_init.  X (batch*(steps+1)*4), U (batch*steps) absolute; exitflag and iterations
 * (batch*steps, may be NULL) per solve.  The loop's time goes to bqp_last_kernel_ms (6 launches
 * per round; on the stage route 6 and the structured solve's repair launch where opt->polish
 * asks for one; with shooting = 1 one more, the warm start of the states), its rounds to bqp_last_loop_rounds.  The _device variant synchronises its stream
 * while it polls for the instances that have finished.  cl->plant_par steps a plant with other
 * coefficients than the model's (every route, both loop modes, the same bits in both); the solve's
 * model stays the nominal one. */
int bqp_closed_loop_nmpc(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* data,
                         const bqp_options* opt, const bqp_closed_loop* cl, const double* x_init,
                         double* X, double* U, int* exitflag, int* iterations);
int bqp_closed_loop_nmpc_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                const bqp_nmpc_data* data, const bqp_options* opt,
                                const bqp_closed_loop* cl, const double* x_init, double* X,
                                double* U, int* exitflag, int* iterations, void* stream);

/* Set-point schedule and disturbed plant of bqp_closed_loop_nmpc_track.  sref / sdist: the distance
 * in doubles between two instances' schedules (>= steps*4), 0 = one schedule shared by the batch. */
typedef struct {
    const double* ref;   int64_t sref;   /* steps*4 per instance: the set-point x_s of every step,
                                            absolute; NULL: data->x_ref at every step (NULL: x_eq) */
    const double* dist;  int64_t sdist;  /* steps*4 per instance: added to the plant's state after
                                            every step; NULL: 0 */
    double* THETA;                       /* out, batch*steps, may be NULL: theta of every step's solution */
} bqp_nmpc_track;

/* bqp_closed_loop_nmpc with a set-point schedule and an additive state disturbance.  Step t of
 * instance b: the solve at X[b,t] with the set-point ref[b,t] (bqp_nmpc_data.x_ref says how it enters
 * the cost; constant over the horizon), U[b,t] = u_0, X[b,t+1] = dynamic(delta, X[b,t], U[b,t]) +
 * dist[b,t] - one addition, rounded once, the value the log stores and the next solve measures - and
 * THETA[b,t] = theta of that solution.  The warm start, the exit flags (a solve that ends != 1 still
 * applies its u_0), the iteration counts, bqp_last_kernel_ms, bqp_last_loop_rounds and both loop
 * modes (BQP_NMPC_SYNC) are bqp_closed_loop_nmpc's, on every route it has - dense, stage, stage
 * with soft state rows, multiple shooting - with the same launches per round: the advance launch
 * also logs theta, adds the disturbance and, while steps remain, takes the instance's next
 * set-point (it never reads ref[b, steps]); both modes return the same bits.  tr = NULL is
 * bqp_closed_loop_nmpc.  steps = 0 returns X = x_init.  A non-finite entry of ref or dist is
 * BQP_E_ARG on the host entry point.  A plant whose parameters differ from the model's is
 * cl->plant_par (bqp_closed_loop), with or without a track: in the asynchronous loop instance b
 * reads the row of its own step.  Not covered: a set-point that varies over the horizon, plant
 * parameters inside the solve's model (it stays nominal), a MEX field. */
int bqp_closed_loop_nmpc_track(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* data,
                               const bqp_options* opt, const bqp_closed_loop* cl, const double* x_init,
                               const bqp_nmpc_track* tr, double* X, double* U, int* exitflag,
                               int* iterations);
int bqp_closed_loop_nmpc_track_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                      const bqp_nmpc_data* data, const bqp_options* opt,
                                      const bqp_closed_loop* cl, const double* x_init,
                                      const bqp_nmpc_track* tr, double* X, double* U, int* exitflag,
                                      int* iterations, void* stream);

/* Timing of the most recent solve on this handle: kernel time measured with hipEvents on the
 * launch stream (ms), and the number of kernel launches it covered. */
int bqp_last_kernel_ms(bqp_handle h, double* ms, int* launches);

/* SQP rounds that the most recent bqp_closed_loop_nmpc[_device] on this handle launched, in either
 * of its modes; a round is one launch of rollout, normal equations, dense sub-problem, trial
 * rollouts and update (stage route: stage linearisation, structured solve, back-map, trial
 * rollouts and update).  BQP_E_ARG before any such loop has run on the handle. */
int bqp_last_loop_rounds(bqp_handle h, int* rounds);

/* Diagnostic: per instance of the most recent mixed-precision structured solve on this handle
 * (bqp_options.precision = 2, N + 1 > 64), the fp32 phase's exit flag (1 / 0: continued in fp64
 * from its iterate; -2 / -8: solved from the fp64 initial point), or 2 where the continuation did
 * not converge and the retry launch solved the instance again from the fp64 initial point
 * (tests/test_gpu_mixed.py).  batch must equal that solve's. */
int bqp_debug_mixed_flags(bqp_handle h, int batch, int* flags);
/* Diagnostic: instances per workgroup the last structured solve on this handle was launched with
 * (the most that fit the 160 KB of LDS, at most 4, 2 at N + 1 > 64); BQP_E_ARG before any solve. */
int bqp_debug_ocp_wpb(bqp_handle h, int* wpb);

#ifdef __cplusplus
}
#endif
#endif /* BQP_H */
