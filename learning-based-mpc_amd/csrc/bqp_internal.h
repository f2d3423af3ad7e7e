// bqp_internal.h — kernel argument blocks and launch helpers shared by the HIP kernels and the
// C-ABI implementation (bqp_api.cpp).  Not part of the public ABI (include/bqp.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bqp_nmpc_advance.h"
#include "bqp_nmpc_dms.h"
#include "bqp_nmpc_stage.h"
#include "bqp_plant_par.h"
#include "bqp_track.h"

namespace bqp {

// per-instance exit statistics written by every solve kernel and turned into bqp_output by
// finalize_kernel: iterations, stationarity, max(primal eq, primal ineq), mu, primal eq,
// primal ineq (inf-norms at exit), 1 if the answer is the structured solver's active-set polish
constexpr int STATS_W = 7;

// Structured OCP kernel arguments (device pointers).  H and Fp are the prepared shared tables:
//   H  : (N+1) stages x hstride doubles, stage cost in internal order [x; theta; u], row-major
//   Fp : column-major [NV][mpad] polytope matrix in internal order
// All other arrays are in the public (external) layout with per-instance element strides.
constexpr int OCP_QUEUES = 4;   // work-queue counters per structured solve (one per launch)
struct OcpKernelArgs {
    int N, mp, kp, batch, wpb, hstride, mpad, shared_doubles, max_iter;
    // persistent work queue: when the batch needs more workgroups than the
    // device holds at once, the launch is sized to the resident workgroups and every instance
    // slot (stage / row wave pair) takes its next instance from this counter as soon as its
    // current one is done; nullptr: one instance per slot, grid = batch.  The counter is zeroed by
    // the prep kernel where that runs (queue_zeroed = 1), else by the launch helper right before a
    // persistent launch (launch_ocp_queue_zero) - a launch of one instance per slot never reads it
    int* queue;
    int queue_zeroed;
    // 1: H and Fp are the caller's arrays (bqp_ocp_data W and Fp, external order) and the kernel
    // forms the prepared layout below while it stages them into LDS, so no prep launch is needed
    // (shared tables, N + 1 <= 64); 0: H and Fp are the tables ocp_prep_kernel wrote
    int raw_tables;
    double tol_stat, tol_feas, tol_comp, tau;
    const double* H;
    const double* Fp;
    const double *A, *B, *c, *w, *xlb, *xub, *ulb, *uub, *hp, *x0;
    int64_t sA, sB, sc, sw, sxb, sub, shp, sx0;
    double *x, *u, *theta, *fval;
    int* exitflag;
    double* stats;  // batch x STATS_W (see STATS_W)
    double *pi_out, *lamx_out, *lamu_out, *lamp_out;
    double* stamps;  // diagnostic build (BQP_STAMPS): batch x 16 phase cycle counts
    // mixed precision (bqp_options.precision = 2): the fp32 launch ends each instance at its
    // (floored) tolerances and writes its iterate (s, pi, u, row slacks and multipliers) to
    // hand_out; the fp64 launch continues from hand_in the instances whose fp32 exit flag
    // (hand_flag) is 1 or 0, and starts the others (-2, -8) from its own initial point
    float* hand_out;
    const float* hand_in;
    const int* hand_flag;
    int* hand_it;           // fp32-phase iterations (written by the fp32 launch, added by the fp64 one)
    int64_t hand_stride;    // floats per instance (ocp_hand_floats)
    // third launch of the mixed mode (cold fp64): only the instances whose warm continuation
    // did not converge (exitflag != 1 with a warm hand_flag) are solved again from the fp64
    // initial point; every other instance leaves at once
    const int* redo_flag;
    // per-instance polytope (bqp_ocp_data.sFp != 0): the caller's column-major n_poly x nv
    // blocks, stride sFp; the shared Fp table is then unused
    const double* Fp_inst;
    int64_t sFp;
    // long-horizon layout (two stages per lane, N + 1 > 64; QpLds lng): Riccati tables in global
    // scratch (batch x (N+1) x ocp_pstride elements of the instantiation's precision) and the
    // shared-LDS offsets of the polytope matrix, polytope rhs and box bounds (-1: not shared).
    // The stage-cost table H is then read from global (L2) instead of LDS.
    void* Pg;
    int sh_F, sh_hp, sh_bnd;
    // per-instance stage costs (bqp_ocp_data.sW != 0): prepared tables batch x (N+1) x hstride;
    // short horizons copy the instance's table into its LDS slot, long ones read it from L2
    const double* H_inst;
    // active-set polish (fp64 instantiation, bqp_options.polish): 0 off, 1 after a 0 / -8 exit,
    // 2 also with a weakly active row.  The solve kernel marks the instances that need it in
    // pol_need (batch ints); the repair launch (launch_ocp(..., pol = true)) solves those again
    // and polishes them
    int polish;
    int* pol_need;
    // per-stage models (bqp_ocp_dims.stage_models = 1; fp64 solve launch only): A, B, c hold N
    // blocks per instance (strides sA, sB, sc over whole schedules), and instances with
    // skip[i] != 0 (may be null) leave at once without writing an output
    int stage_models;
    const int* skip;
    // soft state bounds (bqp_ocp_data.xs_lin / xs_quad; fp64, plain grid, no polish): soft = 1 runs
    // the soft instantiations, which are per-stage-model ones; one_model = 1 hands them a one-model
    // problem (every stage reads block 0 of A, B, c).  xs_lin / xs_quad: (N+1) nx weights per
    // instance (stride sxs; either may be null = zeros); sx_out (may be null): the slacks in the
    // layout of lamx_out
    int soft, one_model;
    const double *xs_lin, *xs_quad;
    int64_t sxs;
    double* sx_out;
};

bool ocp_supported(int nx, int nu, int np);
int ocp_rpl_for(int mp);
int ocp_bpl_for(int N, int nx, int nu);
int ocp_hand_floats(int N, int nx, int nu, int np, int mp);
int ocp_wave_lds_doubles(int N, int nx, int nu, int np, int mpad, bool fpi, bool lng, bool hpsh,
                         bool bndsh, bool hinst, bool stg = false);
int ocp_pstride(int ns);
hipError_t launch_ocp(const OcpKernelArgs& a, int nx, int nu, int np, hipStream_t st, bool pol = false);
// fp32 instantiation (bqp_ocp_f32.hip): LDS element count per instance (floats) and launch
int ocp_wave_lds_doubles_f32(int N, int nx, int nu, int np, int mpad, bool fpi, bool lng,
                             bool hpsh, bool bndsh, bool hinst, bool stg = false);
hipError_t launch_ocp_f32(const OcpKernelArgs& a, int nx, int nu, int np, hipStream_t st, bool pol = false);
hipError_t launch_ocp_prep(const double* W, const double* Fp, int nx, int nu, int np, int N,
                           int mp, int kp, int hstride, int mpad, double* Hout, double* Fout,
                           int* qzero, hipStream_t st);
hipError_t launch_ocp_queue_zero(int* q, hipStream_t st);   // one work-queue counter to 0
hipError_t launch_ocp_prep_h(const double* W, int64_t sW, int batch, int nx, int nu, int np,
                             int N, int hstride, double* Hout, hipStream_t st);
hipError_t launch_ocp_finalize(const double* stats, int batch, void* out, hipStream_t st,
                               const int* skip = nullptr);

// Dense quadprog kernel arguments.
struct DenseKernelArgs {
    int n, m, me, batch, max_iter, mrows;  // mrows = m + finite bound rows (set per instance)
    double tol_stat, tol_feas, tol_comp, tau;
    const double *H, *f, *A, *b, *Aeq, *beq, *lb, *ub;
    int64_t sH, sf, sA, sb, sAeq, sbeq, slb, sub;
    double *x, *fval, *lam_ineqlin, *lam_eqlin, *lam_lower, *lam_upper;
    int* exitflag;
    double* stats;
    double* work;      // per-instance scratch (global), work_stride doubles each
    int64_t work_stride;
    int polish;        // 1: active-set polish after a 0 / -8 exit (bqp_dense.hip::dense_polish);
                       // 2: also after a converged exit (exact active-set steps for the SQP)
    const int* pol_it; // optional: per-instance SQP iteration counts; mode 2 where >= pol_stall
    int pol_stall;     // (the learned-model loop, whose instances run at their own SQP iteration)
    const int* skip;   // optional: instances with skip[i] != 0 are not solved (finished SQPs)
    int res_every;     // exact residual evaluation at least every res_every iterations (0: 8;
                       // 1: every iteration, the diagnostic BQP_DENSE_RES_EVERY)
};

int dense_work_doubles(int n, int m, int me);
hipError_t launch_dense(const DenseKernelArgs& a, hipStream_t st);
hipError_t launch_dense_symmetrize(double* H, int n, int count, int64_t stride, hipStream_t st);

// Learning-based MPC (Gauss-Newton SQP on the NW-learned model), bqp_lbmpc.hip.  Small
// matrices column-major (A nx*nx, B nx*nu, K nu*nx, LAMBDA nx*np, PSI nu*np); weight factors
// upper-triangular row-major (Lq nx*nx, Lr nu*nu, Lp, Lt nx*nx); NW window wrows x q
// column-major (7: [X; Y], 8: [X; Y; v] with the validity row of casadiL2NW.m).
struct LbmpcArgs {
    int N, n, nr, m, q, n_run, term_learned, batch, ntrial, max_iter, wrows;
    double hinv2, lam_nw, tol_step, tol_stat;
    const double *A, *B, *K, *Lq, *Lr, *Lp, *Lt, *LAM, *PSI, *xs;
    const double* data; int64_t sdata;
    const double* x0; int64_t sx0;
    const double* Ain;                  // m x n column-major, shared
    const double* bin; int64_t sbin;    // m per instance
    double* z;                          // batch x n iterate (in: start, out: solution)
    double* d;                          // batch x n QP step
    double* lam;                        // batch x m QP multipliers
    double *Jr, *er;                    // batch x nr x n (row-major), batch x nr
    double *H, *f, *bsh;                // batch x n x n (column-major), batch x n, batch x m
    double *cost0, *costT, *stat, *cprev;  // batch, batch x ntrial, batch, batch
    int *qpflag, *flag, *done, *iters, *ndone;
    // exact Hessian (hess = 1): rows Xi_k (Jr2) and W_k Xi_k (Tr2), batch x 3N x n row-major;
    // hused (may be null): per instance, the iterations that used the exact Hessian
    int hess;
    double *Jr2, *Tr2;
    int* hused;
};

hipError_t launch_nw_oracle(int batch, int q, const double* data, int64_t sdata, const double* xi,
                            double* g, double* dg, double bw, double lam, hipStream_t st);
bool lbmpc_hess_fits(int n);   // exact-Hessian LDS fits (n <= 127); else Gauss-Newton
bool lbmpc_supported(int nx, int nu, int np, int n, int q);
hipError_t launch_lbmpc_rollout(const LbmpcArgs& a, int gn, hipStream_t st);
hipError_t launch_lbmpc_normal(const LbmpcArgs& a, hipStream_t st);
hipError_t launch_lbmpc_update(const LbmpcArgs& a, hipStream_t st);
hipError_t launch_lbmpc_hess(const LbmpcArgs& a, hipStream_t st);

// Nonlinear MPC on the true Moore-Greitzer model (single-shooting Gauss-Newton SQP with an L1
// merit function), bqp_nmpc.hip.  n = N + 1, nr = 5 N + 8, m = N (mx + mu) + mp.  Weight factors
// as LbmpcArgs; F_x mx x 4 and F_T mp x 5 column-major; x0 absolute.
constexpr int NMPC_MAXN = 127;     // n = N + 1 <= 128: two sensitivity columns per lane
constexpr int NMPC_MAXMX = 32, NMPC_MAXMU = 8;
struct NmpcArgs {
    int N, n, nr, m, mx, mu, mp, batch, ntrial, max_iter;
    double delta, tol_step, tol_stat;
    const double *Lq, *Lr, *Lp, *Lt, *LAM, *PSI, *xeq, *ueq, *Fx, *hx, *Fu, *hu, *FT, *hT;
    const double* x0; int64_t sx0;
    double* z;                          // batch x n iterate (in: start, out: solution)
    double* d;                          // batch x n QP step
    double* lam;                        // batch x m QP multipliers
    double *Jr, *er;                    // batch x nr x n (row-major), batch x nr
    double *H, *f;                      // batch x n x n (column-major), batch x n
    double *C, *rhs;                    // batch x m x n (column-major per instance), batch x m: -c
    double *cost0, *costT, *violT;      // batch, batch x ntrial, batch x ntrial
    double *stat, *cprev, *nu;          // batch each; nu: the merit function's penalty
    double *Xout, *cout;                // linearisation only (may be null): rollout, c
    int *qpflag, *flag, *done, *iters, *ndone;
    double* ctl;                        // stage route: batch x n, C'lam ready-made (C is null)
};
static_assert(NMS_MAXMX == NMPC_MAXMX && NMS_MAXMU == NMPC_MAXMU, "bqp_nmpc_stage.h's row limits");
// Stage route (bqp_nmpc_dims.subproblem = 1): the stage problem of the structured solve and that
// solve's outputs, per instance unless said (strides: bqp_layout.h NworkStage)
struct NmpcStageArgs {
    double *A, *B, *w, *xlb, *xub, *ulb, *uub, *hp;   // 16 N, 4 N, 6 (N+1), 4 (N+1) x 2, N x 2, mp
    double *W, *Fp;                                  // shared: 36 (N+1), 6 mp column-major
    NmpcBoundMap* map;                               // shared
    const double *uo, *tho, *lamx, *lamu, *lamp;     // the solve's u, theta and multipliers
    const int* sflag;                                // and exit flags
};
// Soft state rows of the stage route (bqp_nmpc_data.xs_lin / xs_quad).  A separate, trailing kernel
// argument: NmpcArgs and NmpcStageArgs keep their layout, so the hard instantiations read their
// arguments where they always did.  The launchers take a null pointer for "every row hard".
struct NmpcSoftArgs {
    const double *xs_lin, *xs_quad;   // shared: mx row weights each, either may be null (zeros)
    double *xsl, *xsq;                // shared: (N+1) x 4, the structured solve's xs_lin / xs_quad
    const double* sx;                 // batch x 8 (N+1): the structured solve's s_x
    double *pen0, *plin;              // batch each: the penalty at z, the sub-problem's model penalty
};
// Multiple shooting on the stage route (bqp_nmpc_dims.shooting = 1): the states of the iterate, the
// defects and what the back-map hands to the update.  A separate, trailing kernel argument of the
// nmpc_dms_* kernels; the indices are bqp_nmpc_dms.h's.
static_assert(NMD_MAXN == NMPC_MAXN, "bqp_nmpc_dms.h's horizon limit");
struct NmpcDmsArgs {
    double* X;                 // batch x 4 (N+1): the iterate's states, absolute (in: start, out: solution)
    double* c;                 // batch x 4 N: the defects c_k = f_k - x_{k+1}
    const double* dX;          // batch x 4 (N+1): the structured solve's x
    const double* pi;          // batch x 4 N: the structured solve's pi
    double *sw, *gn, *pimax;   // batch each: sum w_k'v_k, |grad J|, max |pi|
};
// Set-point of the tracking cost (bqp_nmpc_data.x_ref): the offset term pulls LAMBDA theta to
// rho = x_ref - x_eq, its four residual rows are (Lt LAMBDA) theta - Lt rho.  A separate, trailing
// kernel argument of the kernels that evaluate that term, read by their reference instantiations
// alone; the launchers take a null pointer for "the working point", and then launch the
// instantiations that existed before the member did.
struct NmpcRefArgs {
    const double* xref;   // 4 per instance, absolute
    int64_t sref;         // doubles between two instances' set-points; 0: one for the batch
};
bool nmpc_supported(int N, int mx, int mu);
// multiple shooting: X = the rollout of z, for a solve that is given no states (once per solve)
hipError_t launch_nmpc_dms_start(const NmpcArgs& a, const NmpcDmsArgs& m, hipStream_t st);
// the linearisation at (X, z), lanes over the stages: A, B, c, w, bounds, hp, rhs, cost0
hipError_t launch_nmpc_dms_linearize(const NmpcArgs& a, const NmpcStageArgs& s, const NmpcDmsArgs& m,
                                     hipStream_t st, const NmpcRefArgs* r = nullptr);
// after the structured solve: d, lam in NMPC row order, qpflag, sum w_k'v_k, the full-space
// stationarity residual (a.stat), |grad J|, max |pi|
hipError_t launch_nmpc_dms_backmap(const NmpcArgs& a, const NmpcStageArgs& s, const NmpcDmsArgs& m,
                                   hipStream_t st);
// the ntrial trial points (X, z) + 2^-t (dX, d): costT = J, violT = V + E
hipError_t launch_nmpc_dms_trial(const NmpcArgs& a, const NmpcDmsArgs& m, hipStream_t st,
                                 const NmpcRefArgs* r = nullptr);
hipError_t launch_nmpc_dms_update(const NmpcArgs& a, const NmpcDmsArgs& m, hipStream_t st);
// closed loop, after a step's solve and before the warm start of z: the warm start of the states,
// x_k <- x_{k+1}, x_N <- dynamic(delta, x_N, u_{N-1}) with the repeated last move (x_0 is the next
// linearisation's, from the measured state).  done / ts null: every instance (step-synchronous
// loop); else the instances nmpc_loop_advance_kernel is about to move to their next step
hipError_t launch_nmpc_dms_loop_states(int batch, int N, int steps, double delta, const double* ueq,
                                       const double* z, double* X, const int* done, const int* ts,
                                       hipStream_t st);
// stage route: the shared tables (W, Fp, bound map; with q also the weight tables), once per solve
hipError_t launch_nmpc_stage_table(const NmpcArgs& a, const NmpcStageArgs& s, hipStream_t st,
                                   const NmpcSoftArgs* q = nullptr);
// the rollout at z with the stage Jacobians: A, B, w, bounds, hp, rhs, cost0 (with q: pen0, and
// cost0 = J + pen0)
hipError_t launch_nmpc_stage_rollout(const NmpcArgs& a, const NmpcStageArgs& s, hipStream_t st,
                                     const NmpcSoftArgs* q = nullptr, const NmpcRefArgs* r = nullptr);
// after the structured solve: d, lam in NMPC row order, qpflag, f and C'lam by the adjoint sweep
// (with q: plin from the solve's slacks)
hipError_t launch_nmpc_stage_backmap(const NmpcArgs& a, const NmpcStageArgs& s, hipStream_t st,
                                     const NmpcSoftArgs* q = nullptr);
// gn = 1: rollout with sensitivities at z (Jr, er, C, rhs, cost0); gn = 0: the ntrial trial points
// (with q: costT = J + penalty, violT over the hard rows)
hipError_t launch_nmpc_rollout(const NmpcArgs& a, int gn, hipStream_t st, const NmpcSoftArgs* q = nullptr,
                               const NmpcRefArgs* r = nullptr);
// with q (stage route only): the hard rows' reductions and D = f'd + plin - pen0 - nu V0
hipError_t launch_nmpc_update(const NmpcArgs& a, hipStream_t st, const NmpcSoftArgs* q = nullptr);
// closed loop: after the plant step of step t, the step's SQP iteration counts into the log and
// the warm start (z shifted one stage, last move repeated, theta kept)
hipError_t launch_nmpc_loop_shift(int batch, int N, int steps, int t, double* z, const int* it,
                                  int* itlog, hipStream_t st);
// asynchronous closed loop (NmpcAdvanceArgs: bqp_nmpc_advance.h): after an SQP round, every instance
// whose SQP has stopped logs its step, steps the plant and sets up its next solve
// k (bqp_closed_loop_nmpc_track): also theta into its log, the disturbance onto the plant's state
// and the next step's set-point; null: the advance as it was
// pp (bqp_closed_loop.plant_par): the plant of each instance's own step; null: the nominal plant
hipError_t launch_nmpc_loop_advance(const NmpcAdvanceArgs& a, hipStream_t st, const NmpcTrackArgs* k = nullptr,
                                    const PlantPar* pp = nullptr);
// bqp_closed_loop_nmpc_track, once per loop: the set-points of step 0 into k.xr
hipError_t launch_nmpc_track_init(int batch, const NmpcTrackArgs& k, hipStream_t st);
// bqp_closed_loop_nmpc_track, step-synchronous loop: mg_plant_kernel's step t of every instance from
// z[b, 0] with the disturbance added and theta logged (the advance's arithmetic, lane for lane)
hipError_t launch_nmpc_track_plant(const NmpcAdvanceArgs& a, const NmpcTrackArgs& k, int t, hipStream_t st,
                                   const PlantPar* pp = nullptr);

// closed-loop simulation (bqp_plant.hip): Moore-Greitzer plant (RK4 step or MATLAB ode23,
// BQP_PLANT_*) between batched solves
hipError_t launch_closed_loop_init(int batch, int nx, int steps, const double* xinit,
                                   const double* xeq, double* s, double* X, hipStream_t st);
hipError_t launch_mg_plant(int plant, int batch, int N, int steps, int t, double delta,
                           const double* uo, const int* fl, const double* xeq, const double* ueq,
                           double* s, double* X, double* U, int* flags, hipStream_t st,
                           const PlantPar* pp = nullptr);
// closed loop with a reference schedule (bqp_closed_loop_track; TrackArgs: bqp_track.h): after
// the step-t solve, record it, step the plant and form the linear terms of step t + 1; t = -1
// forms those of step 0 alone
// pp (bqp_closed_loop.plant_par, MG plants only): per-instance plant coefficients; null: nominal
hipError_t launch_track_advance(const TrackArgs& a, int t, hipStream_t st, const PlantPar* pp = nullptr);
// learned-model NLP closed loop glue (bqp_closed_loop_sqp): per instance bin = bin0 + Bx s and
// the warm start (z shifted one stage, zero last move, theta kept) before the SQP; u_0 = K s + z_0
// for the plant, and the step's z / iteration count into the caller's logs after it
// asynchronous learned-model loop: one instance's advance to its next closed-loop step
struct SqpAdvanceArgs {
    int batch, nx, nu, n, m, nv, warm, steps, q, plant;
    double delta, hinv2, lam;
    const double *K, *bin0, *Bx, *xeq, *ueq, *A, *Bm;
    double *s, *z, *bin, *X, *U, *win, *XL, *Zlog;
    int *done, *iters, *flag, *hused, *ts, *nfin, *flags, *itlog;
};
hipError_t launch_sqp_loop_advance(const SqpAdvanceArgs& a, hipStream_t st, const PlantPar* pp = nullptr);
hipError_t launch_sqp_loop_prep(int batch, int nx, int n, int m, int nv, int shift, const double* s,
                                const double* bin0, const double* Bx, double* bin, double* z,
                                hipStream_t st);
hipError_t launch_sqp_loop_u0(int batch, int nx, int n, const double* K, const double* s,
                              const double* z, double* uo, const int* it, int steps, int t,
                              double* Zlog, int* itlog, hipStream_t st);
hipError_t launch_lbmpc_window_init(int batch, int steps, int q, int mask, const double* xinit,
                                    double* win, double* XL, hipStream_t st);
hipError_t launch_lbmpc_window(int batch, int steps, int t, int q, double bw, double lam,
                               const double* A, int64_t sA, const double* B, int64_t sB,
                               const double* xeq, const double* ueq, const double* X,
                               const double* U, double* win, double* XL, hipStream_t st);

}  // namespace bqp
