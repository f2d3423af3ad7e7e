// bqp_nmpc.hip — nonlinear MPC on the true Moore-Greitzer model on gfx950: the device side of the
// single-shooting Gauss-Newton SQP that solves the reference's tracking NMPC problem.
//
// Reference: examples/DMS_tracking_NMPC_casadi.m:121-126 (the NLP), :225-254 (cost), :256-283
// (constraint rows), :217-223 / :286-293 (`system`, `dynamic`: one RK4 step).  The algorithm is
// stated in tests/nmpc_ref.py; the host loop is bqp_nmpc_solve_batched_device (bqp_api.cpp).
//
// One SQP iteration = rollout(GN) -> normal equations -> dense QP -> rollout(trials) -> update:
//   nmpc_rollout_kernel<true>   one wave per instance: the RK4 rollout from the measured state
//                               with the stage Jacobians A_k, B_k differentiated through the four
//                               RK stages (analytic Jacobian of `system`), the forward
//                               sensitivities S_{k+1} = A_k S_k + B_k e_k' (lanes over the columns
//                               of z, two per lane), the weighted residuals e and the rows of
//                               their Jacobian Jr (row-major, the layout of the learned-model
//                               path), the constraint values (rhs = -c) and the instance's own
//                               constraint Jacobian C (column-major m x n, as the dense kernels
//                               read A)
//   nmpc_rollout_kernel<false>  one wave per (instance, trial): cost and violation
//                               V = sum max(c, 0) at z + 2^-t d, no Jacobians
//   lbmpc_normal_kernel         (bqp_lbmpc.hip, launched with m = 0) H = 2 Jr'Jr on the fp64
//                               matrix cores, f = 2 Jr'e
//   nmpc_update_kernel          one wave per instance: stationarity |f + C'lam| over the
//                               instance's C, penalty, L1 merit line search, z += alpha d
//                               (<true>: from the back-map's ready C'lam)
// Stage route (bqp_nmpc_dims.subproblem = 1) = stage rollout -> structured solve with per-stage
// models (bqp_ocp.hip) -> back-map -> rollout(trials) -> update<true>; no Jr, H or C:
//   nmpc_stage_table_kernel     once per solve: the shared cost blocks W, the polytope matrix Fp,
//                               the bound map of F_x / F_u and its "not a box" flag
//   nmpc_stage_rollout_kernel   one wave per instance: the rollout of <true> without
//                               sensitivities; A_k, B_k, the stage gradients w_k, the rows as
//                               bounds on dx_k, du_k, hp, rhs = -c, cost
//   nmpc_stage_backmap_kernel   one wave per instance: d, lam in NMPC row order, the sub-problem's
//                               flag, f and C'lam by one adjoint sweep over A_k, B_k
//   nmpc_loop_shift_kernel      step-synchronous closed loop: the warm start of the next step
//   nmpc_loop_advance_kernel    asynchronous closed loop, after every iteration: the instances
//                               whose SQP has stopped move to their next closed-loop step
// Set-points (bqp_nmpc_data.x_ref): the kernels that evaluate the T term - the rollouts, the stage
// rollout, multiple shooting's linearisation and trials - have a REF instantiation each, which reads
// the instance's set-point through a trailing NmpcRefArgs (NmLtRho).  The loop with a schedule
// (bqp_closed_loop_nmpc_track): nmpc_loop_advance_kernel<true>, nmpc_track_init_kernel once per
// loop, nmpc_track_plant_kernel in the step-synchronous loop.
// Multiple shooting on the stage route (bqp_nmpc_dims.shooting = 1; the nmpc_dms_* kernels below) =
// dms linearise -> structured solve with the defects as its per-stage offset -> dms back-map ->
// dms trials -> dms update: the states stay variables, lanes run over the stages, no rollout in a round
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "bqp_internal.h"
#include "bqp_mg.h"
#include "bqp_wave.h"

namespace bqp {

#define NM_WAVE 64
#define NM_CPL 2         // z columns per lane: n = N + 1 <= 128

// Moore-Greitzer `system` (as bqp_plant.hip steps it)
__device__ __forceinline__ void nm_system(const double (&x)[4], double u, double (&f)[4]) {
    f[0] = -x[1] + 1.0 + 3.0 * (x[0] / 2.0) - (x[0] * x[0] * x[0] / 2.0);
    f[1] = (x[0] + 1.0 - x[2] * sqrt(x[1]));
    f[2] = x[3];
    f[3] = -1000.0 * x[2] - 2.0 * sqrt(500.0) * x[3] + 1000.0 * u;
}

// R = Jf(y) M + [0 | fu] for a 4 x 5 block M = [d./dx | d./du]: Jf the analytic Jacobian of
// `system` w.r.t. x (its sparsity written out), fu = d system / du = [0 0 0 1000]'
__device__ __forceinline__ void nm_jmul(const double (&y)[4], const double (&M)[4][5], double (&R)[4][5]) {
    const double sq = sqrt(y[1]);
    const double a00 = 1.5 - 1.5 * y[0] * y[0], a11 = -y[2] / (2.0 * sq), c33 = 2.0 * sqrt(500.0);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        R[0][j] = a00 * M[0][j] - M[1][j];
        R[1][j] = M[0][j] + a11 * M[1][j] - sq * M[2][j];
        R[2][j] = M[3][j];
        R[3][j] = -1000.0 * M[2][j] - c33 * M[3][j];
    }
    R[3][4] += 1000.0;
}

// xn = dynamic(h, x, u); JAC: AB = [dxn/dx | dxn/du], the chain rule through the four stages
template <bool JAC>
__device__ __forceinline__ void nm_rk4(double h, const double (&x)[4], double u, double (&xn)[4],
                                       double (&AB)[4][5]) {
    double k[4], y[4], ks[4], M[4][5], K[4][5];
    const double hs[3] = {h / 2.0, h / 2.0, h}, wk[4] = {1.0, 2.0, 2.0, 1.0};
#pragma unroll
    for (int i = 0; i < 4; ++i) { y[i] = x[i]; ks[i] = 0.0; }
    if (JAC) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) { M[i][j] = i == j ? 1.0 : 0.0; AB[i][j] = 0.0; }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        nm_system(y, u, k);
        if (JAC) {
            nm_jmul(y, M, K);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 5; ++j) AB[i][j] += wk[s] * K[i][j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) ks[i] += wk[s] * k[i];
        if (s < 3) {
#pragma unroll
            for (int i = 0; i < 4; ++i) y[i] = x[i] + hs[s] * k[i];
            if (JAC) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 5; ++j) M[i][j] = (i == j ? 1.0 : 0.0) + hs[s] * K[i][j];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) xn[i] = x[i] + h / 6.0 * ks[i];
    if (JAC) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) AB[i][j] = (i == j ? 1.0 : 0.0) + h / 6.0 * AB[i][j];
    }
}

// ------------------------------------------------------------------------------------------
// rollout: cost and constraint values (all modes); GN: the residual Jacobian Jr and the
// constraint Jacobian C from the forward sensitivities
// ------------------------------------------------------------------------------------------
// the shared constants, copied to LDS once (read from global memory inside the stage loop they
// would be reloaded after every store: the compiler cannot rule out aliasing)
constexpr int NO_Q = 0, NO_R = NO_Q + 16, NO_P = NO_R + 1, NO_T = NO_P + 16, NO_L = NO_T + 16,
              NO_PSI = NO_L + 4, NO_XE = NO_PSI + 1, NO_UE = NO_XE + 4, NO_FX = NO_UE + 1,
              NO_HX = NO_FX + 4 * NMPC_MAXMX, NO_FU = NO_HX + NMPC_MAXMX, NO_HU = NO_FU + NMPC_MAXMU,
              NO_END = NO_HU + NMPC_MAXMU;

// the constant block into LDS, lanes over its entries (the caller syncs the wave)
__device__ __forceinline__ void nm_load_consts(const NmpcArgs& a, int lane, double* cst) {
    const int mx = a.mx, mu = a.mu;
    for (int i = lane; i < NO_END; i += NM_WAVE) {
        double v = 0.0;
        if (i < NO_R) v = a.Lq[i - NO_Q];
        else if (i < NO_P) v = a.Lr[0];
        else if (i < NO_T) v = a.Lp[i - NO_P];
        else if (i < NO_L) v = a.Lt[i - NO_T];
        else if (i < NO_PSI) v = a.LAM[i - NO_L];
        else if (i < NO_XE) v = a.PSI[0];
        else if (i < NO_UE) v = a.xeq[i - NO_XE];
        else if (i < NO_FX) v = a.ueq[0];
        else if (i < NO_HX) { const int e = i - NO_FX; if (e < 4 * mx) v = a.Fx[e]; }
        else if (i < NO_FU) { const int e = i - NO_HX; if (e < mx) v = a.hx[e]; }
        else if (i < NO_HU) { const int e = i - NO_FU; if (e < mu) v = a.Fu[e]; }
        else { const int e = i - NO_HU; if (e < mu) v = a.hu[e]; }
        cst[i] = v;
    }
}

// REF instantiations (bqp_nmpc_data.x_ref): Lt rho for the set-point rho = x_ref - x_eq of instance
// b, from the constant block in LDS.  Every lane forms it (the T term is wave-uniform work): 4
// subtractions and 10 multiply-adds; the T rows are then (Lt LAMBDA) theta - Lt rho, so rho = 0
// gives the values of the instantiations without a set-point.  Without REF the type is empty and row()
// hands the product back: those instantiations keep their code
template <bool REF> struct NmLtRho {
    __device__ __forceinline__ NmLtRho(const NmpcRefArgs&, int, const double*) {}
    __device__ __forceinline__ double row(double e, int) const { return e; }
};
template <> struct NmLtRho<true> {
    double lt[4];
    __device__ __forceinline__ NmLtRho(const NmpcRefArgs& rf, int b, const double* cst) {
        double rho[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) rho[i] = rf.xref[(int64_t)b * rf.sref + i] - cst[NO_XE + i];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double v = 0.0;
#pragma unroll
            for (int c2 = r; c2 < 4; ++c2) v += cst[NO_T + 4 * r + c2] * rho[c2];
            lt[r] = v;
        }
    }
    __device__ __forceinline__ double row(double e, int r) const { return e - lt[r]; }
};

// SOFT (trial points of the stage route only): lane i < mx owns row i of F_x with its weights; a
// softened row's max(c, 0) goes into the lane's penalty instead of V, costT = J + sum of the
// penalties.  q is read by the SOFT instantiations alone, rf by the REF ones (the set-point of the T
// term: NmLtRho).
template <bool GN, bool SOFT = false, bool REF = false>
__global__ void __launch_bounds__(64) nmpc_rollout_kernel(NmpcArgs a, NmpcSoftArgs q, NmpcRefArgs rf) {
    static_assert(!(GN && SOFT), "the soft rows belong to the stage route: no linearisation here");
    const int lane = threadIdx.x;
    const int nt = GN ? 1 : a.ntrial;
    const int b = blockIdx.x / nt, t = blockIdx.x % nt;
    if (b >= a.batch || a.done[b]) return;
    const int N = a.N, n = a.n, m = a.m, mx = a.mx, mu = a.mu, ms = mx + mu, mp = a.mp;
    __shared__ double zsh[NM_WAVE * NM_CPL];
    __shared__ double cst[NO_END];
    __shared__ double SNs[GN ? 4 * NM_WAVE * NM_CPL : 1];   // S_N, row c at SNs[128 c ..]
    {
        const double alpha = GN ? 0.0 : ldexp(1.0, -t);
        const double* z = a.z + (int64_t)b * n;
        const double* dz = a.d + (int64_t)b * n;
        for (int j = lane; j < n; j += NM_WAVE) zsh[j] = GN ? z[j] : z[j] + alpha * dz[j];
    }
    nm_load_consts(a, lane, cst);
    wave_sync();
    const double th = zsh[N];
    const double ueq = cst[NO_UE], psi = cst[NO_PSI];
    double x[4];
    {
        const double* x0 = a.x0 + (int64_t)b * a.sx0;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = x0[i];
    }
    // sensitivities dx_k/dz for the lane's columns j = lane + 64 c
    double S[NM_CPL][4];
#pragma unroll
    for (int c = 0; c < NM_CPL; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) S[c][i] = 0.0;
    double* Jr = GN ? a.Jr + (int64_t)b * a.nr * n : nullptr;
    double* er = GN ? a.er + (int64_t)b * a.nr : nullptr;
    double* C = GN ? a.C + (int64_t)b * m * n : nullptr;
    double* rhs = GN ? a.rhs + (int64_t)b * m : nullptr;
    double* cout = (GN && a.cout) ? a.cout + (int64_t)b * m : nullptr;
    double* Xout = (GN && a.Xout) ? a.Xout + (int64_t)b * (N + 1) * 4 : nullptr;
    double J = 0.0, V = 0.0;
    int row = 0;
    // SOFT: the lane's row weights, the wave's mask of softened rows, the lane's penalty
    double wl1 = 0.0, wl2 = 0.0, pen = 0.0;
    unsigned long long softmask = 0;
    if constexpr (SOFT) {
        if (lane < mx) {
            wl1 = q.xs_lin ? q.xs_lin[lane] : 0.0;
            wl2 = q.xs_quad ? q.xs_quad[lane] : 0.0;
        }
        softmask = __ballot(wl1 > 0.0 || wl2 > 0.0);
    }
    // weighted residual block L (v - LAMBDA theta) on the deviation v = x - x_eq, L upper
    // triangular 4 x 4 row-major at cst[oL]; GN: its Jacobian rows from the sensitivities
    auto xresidual = [&](int oL, const double (&xx)[4]) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double e = 0.0;
#pragma unroll
            for (int c2 = r; c2 < 4; ++c2) e += cst[oL + 4 * r + c2] * (xx[c2] - cst[NO_XE + c2] - cst[NO_L + c2] * th);
            J += e * e;
            if (GN) {
                if (lane == 0) er[row + r] = e;
#pragma unroll
                for (int c = 0; c < NM_CPL; ++c) {
                    const int j = lane + NM_WAVE * c;
                    if (j < n) {
                        double acc = 0.0;
#pragma unroll
                        for (int c2 = r; c2 < 4; ++c2)
                            acc += cst[oL + 4 * r + c2] * (S[c][c2] - (j == N ? cst[NO_L + c2] : 0.0));
                        Jr[(int64_t)(row + r) * n + j] = acc;
                    }
                }
            }
        }
        row += 4;
    };
    for (int k = 0; k < N; ++k) {
        const double vk = zsh[k];
        if (Xout && lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) Xout[4 * k + i] = x[i];
        }
        // running cost on (x_k, u_k)
        xresidual(NO_Q, x);
        {
            const double lr = cst[NO_R];
            const double e = lr * (vk - psi * th);
            J += e * e;
            if (GN) {
                if (lane == 0) er[row] = e;
#pragma unroll
                for (int c = 0; c < NM_CPL; ++c) {
                    const int j = lane + NM_WAVE * c;
                    if (j < n) Jr[(int64_t)row * n + j] = lr * ((j == k ? 1.0 : 0.0) - (j == N ? psi : 0.0));
                }
            }
            row += 1;
        }
        // x_{k+1} = dynamic(delta, x_k, u_k), S_{k+1} = A_k S_k + B_k e_k'
        double xn[4], AB[4][5];
        nm_rk4<GN>(a.delta, x, vk + ueq, xn, AB);
        if (GN) {
#pragma unroll
            for (int c = 0; c < NM_CPL; ++c) {
                const int j = lane + NM_WAVE * c;
                double sn[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    double v = j == k ? AB[i][4] : 0.0;
#pragma unroll
                    for (int c2 = 0; c2 < 4; ++c2) v += AB[i][c2] * S[c][c2];
                    sn[i] = v;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) S[c][i] = sn[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = xn[i];
        // rows of stage k + 1: F_x (x_{k+1} - x_eq) <= h_x, F_u (u_k - u_eq) <= h_u
        const int r0 = ms * k;
        for (int i = 0; i < ms; ++i) {
            double cv;
            if (i < mx) {
                cv = -cst[NO_HX + i];
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) cv += cst[NO_FX + i + mx * c2] * (x[c2] - cst[NO_XE + c2]);
            } else {
                cv = cst[NO_FU + i - mx] * vk - cst[NO_HU + i - mx];
            }
            if constexpr (SOFT) {
                if ((softmask >> i) & 1) { if (lane == i) pen += nmpc_phi(wl1, wl2, fmax(cv, 0.0)); }
                else V += fmax(cv, 0.0);
            } else {
                V += fmax(cv, 0.0);
            }
            if (GN) {
                if (lane == 0) {
                    rhs[r0 + i] = -cv;
                    if (cout) cout[r0 + i] = cv;
                }
#pragma unroll
                for (int c = 0; c < NM_CPL; ++c) {
                    const int j = lane + NM_WAVE * c;
                    if (j < n) {
                        double v;
                        if (i < mx) {
                            v = 0.0;
#pragma unroll
                            for (int c2 = 0; c2 < 4; ++c2) v += cst[NO_FX + i + mx * c2] * S[c][c2];
                        } else {
                            v = j == k ? cst[NO_FU + i - mx] : 0.0;
                        }
                        C[(int64_t)j * m + r0 + i] = v;
                    }
                }
            }
        }
    }
    if (Xout && lane == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) Xout[4 * N + i] = x[i];
    }
    // terminal P on x_N, T on LAMBDA theta (REF: on LAMBDA theta - rho)
    xresidual(NO_P, x);
    const NmLtRho<REF> ltr(rf, b, cst);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double w = 0.0;
#pragma unroll
        for (int c2 = r; c2 < 4; ++c2) w += cst[NO_T + 4 * r + c2] * cst[NO_L + c2];
        const double e = ltr.row(w * th, r);
        J += e * e;
        if (GN) {
            if (lane == 0) er[row + r] = e;
#pragma unroll
            for (int c = 0; c < NM_CPL; ++c) {
                const int j = lane + NM_WAVE * c;
                if (j < n) Jr[(int64_t)(row + r) * n + j] = j == N ? w : 0.0;
            }
        }
    }
    // terminal rows F_T [x_N - x_eq; theta] <= h_T: lanes over the rows, so that the stores of a
    // column of C are contiguous across the wave; S_N staged in LDS
    if (GN) {
#pragma unroll
        for (int c = 0; c < NM_CPL; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) SNs[NM_WAVE * NM_CPL * i + lane + NM_WAVE * c] = S[c][i];
        wave_sync();
    }
    const int rT = ms * N;
    double Vt = 0.0;
    for (int r = lane; r < mp; r += NM_WAVE) {
        double F[5];
#pragma unroll
        for (int c2 = 0; c2 < 5; ++c2) F[c2] = a.FT[r + (int64_t)mp * c2];
        double cv = F[4] * th - a.hT[r];
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) cv += F[c2] * (x[c2] - cst[NO_XE + c2]);
        Vt += fmax(cv, 0.0);
        if (GN) {
            rhs[rT + r] = -cv;
            if (cout) cout[rT + r] = cv;
            for (int j = 0; j < n; ++j) {
                double v = j == N ? F[4] : 0.0;
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) v += F[c2] * SNs[NM_WAVE * NM_CPL * c2 + j];
                C[(int64_t)j * m + rT + r] = v;
            }
        }
    }
    if (!GN) V += wsum(Vt);
    if constexpr (SOFT) J += wsum(pen);
    if (lane == 0) {
        if (GN) {
            a.cost0[b] = J;
        } else {
            a.costT[(int64_t)b * nt + t] = J;
            a.violT[(int64_t)b * nt + t] = V;
        }
    }
}

// ------------------------------------------------------------------------------------------
// convergence test + penalty + L1 merit line search + step (one wave per instance)
// ------------------------------------------------------------------------------------------
// STAGE: C'lam is the back-map's ready n-vector a.ctl (stage route), not the product over C
// SOFT (stage route): the merit function is J + P + nu V with the penalty P of the softened rows in
// the cost (cost0, costT) and V, the feasibility test and the multiplier bound of nu over the hard
// rows alone; D = f'd + plin - pen0 - nu V0 with the sub-problem's model penalty plin
template <bool STAGE, bool SOFT = false>
__global__ void __launch_bounds__(64) nmpc_update_kernel(NmpcArgs a, NmpcSoftArgs q) {
    static_assert(STAGE || !SOFT, "the soft rows belong to the stage route");
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= a.batch || a.done[b]) return;
    const int n = a.n, m = a.m;
    double* z = a.z + (int64_t)b * n;
    const double* d = a.d + (int64_t)b * n;
    const double* f = a.f + (int64_t)b * n;
    const double* lam = a.lam + (int64_t)b * m;
    const double* rhs = a.rhs + (int64_t)b * m;
    const double* C = STAGE ? nullptr : a.C + (int64_t)b * m * n;
    const int qflag = a.qpflag[b];
    double st = 0.0, fn = 0.0, dn = 0.0, zn = 0.0, sl = 0.0, viol = -INFINITY, V0 = 0.0, lmax = 0.0;
    // C'lam by groups of 16 columns: lanes over the rows (coalesced loads, 16 in flight), one
    // transposed wave sum per group - the pattern of lbmpc_update_kernel over the instance's own C
    __shared__ double sg[NM_WAVE * NM_CPL];
    if (STAGE) {
        for (int j = lane; j < n; j += NM_WAVE) sg[j] = a.ctl[(int64_t)b * n + j];
    }
    for (int g0 = 0; !STAGE && g0 < n; g0 += 16) {
        double ac[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) ac[c] = 0.0;
        for (int r = lane; r < m; r += NM_WAVE) {
            const double lr = lam[r];
            double av[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) av[c] = C[(int64_t)min(g0 + c, n - 1) * m + r];
#pragma unroll
            for (int c = 0; c < 16; ++c) ac[c] = fma(av[c], lr, ac[c]);
        }
        const double tot = wsum_t(ac, lane);
        if (lane < 16 && g0 + lane < n) sg[g0 + lane] = tot;
    }
    wave_sync();
    for (int j = lane; j < n; j += NM_WAVE) {
        const double g = f[j] + sg[j];
        st = fmax(st, fabs(g));
        fn = fmax(fn, fabs(f[j]));
        dn = fmax(dn, fabs(d[j]));
        zn = fmax(zn, fabs(z[j]));
        sl += f[j] * d[j];
    }
    for (int r = lane; r < m; r += NM_WAVE) {
        if constexpr (SOFT) {
            const int ms = a.mx + a.mu, i = r % ms;
            if (r < ms * a.N && i < a.mx &&
                ((q.xs_lin && q.xs_lin[i] > 0.0) || (q.xs_quad && q.xs_quad[i] > 0.0)))
                continue;
        }
        const double cv = -rhs[r];
        viol = fmax(viol, cv);
        V0 += fmax(cv, 0.0);
        lmax = fmax(lmax, lam[r]);
    }
    st = wmax(st); fn = wmax(fn); dn = wmax(dn); zn = wmax(zn); sl = wsum(sl);
    viol = wmax(viol); V0 = wsum(V0); lmax = wmax(lmax);
    const bool feas0 = viol <= 1e-9;
    const double J0 = a.cost0[b];
    int it = a.iters[b];
    int flag = 0;
    bool fin = false;
    // as lbmpc_update_kernel: a QP that stopped on its iteration limit or numerically (-8) still
    // returns its last interior iterate, and the step is used as is
    const bool qp_ok = qflag == 1 || ((qflag == 0 || qflag == -8) && isfinite(dn) && isfinite(st));
    if (qflag == -2 || !qp_ok || !isfinite(J0) || !isfinite(V0)) {
        flag = (qflag == -2) ? -2 : -8;   // sub-problem infeasible / failed, or a non-finite iterate
        fin = true;
    } else if (feas0 && ((qflag == 1 && dn <= a.tol_step * (1.0 + zn) && st <= a.tol_stat * (1.0 + fn)) ||
                         (it > 0 && dn <= 1e-6 * (1.0 + zn) &&
                          (qflag != 1 || fabs(a.cprev[b] - J0) <= 1e-12 * (1.0 + fabs(J0)))))) {
        flag = 1;
        fin = true;
    }
    if (!fin) {
        // penalty of the L1 merit function phi = J + nu V, kept within the solve
        const double nu = fmax(a.nu[b], 1.1 * lmax);
        double D = sl - nu * V0;
        if constexpr (SOFT) D = sl + q.plin[b] - q.pen0[b] - nu * V0;
        const double phi0 = J0 + nu * V0;
        int tsel = a.ntrial - 1;
        for (int t = 0; t < a.ntrial; ++t) {
            const double al = ldexp(1.0, -t);
            const double Jt = a.costT[(int64_t)b * a.ntrial + t], Vt = a.violT[(int64_t)b * a.ntrial + t];
            // a trial whose rollout is not finite (sqrt of x2 <= 0) is rejected
            if (isfinite(Jt) && isfinite(Vt) && Jt + nu * Vt <= phi0 + 1e-4 * al * D) { tsel = t; break; }
        }
        const double Js = a.costT[(int64_t)b * a.ntrial + tsel];
        if (!isfinite(Js) || !isfinite(a.violT[(int64_t)b * a.ntrial + tsel])) {
            flag = -8;                    // the accepted iterate would not be finite
            fin = true;
        } else {
            const double al = ldexp(1.0, -tsel);
            for (int j = lane; j < n; j += NM_WAVE) z[j] += al * d[j];
            if (lane == 0) { a.cprev[b] = J0; a.nu[b] = nu; }
            ++it;
            if (it >= a.max_iter) {
                flag = 0;
                fin = true;
                if (lane == 0) a.cost0[b] = Js;   // the returned z is the stepped iterate
            }
        }
    }
    if (lane == 0) {
        a.iters[b] = it;
        a.stat[b] = st;
        if (fin) {
            a.flag[b] = flag;
            a.done[b] = 1;
            atomicAdd(a.ndone, 1);
        }
    }
}

// closed loop, after the plant step of step t: the step's iteration count into the log, then the
// warm start of step t + 1: z shifted one stage, the last move repeated, theta kept
__global__ void __launch_bounds__(64) nmpc_loop_shift_kernel(int batch, int N, int steps, int t, double* z,
                                                             const int* it, int* itlog) {
    __shared__ double zs[NM_WAVE * NM_CPL];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    double* zb = z + (int64_t)b * (N + 1);
    for (int j = lane; j < N; j += NM_WAVE) zs[j] = zb[min(j + 1, N - 1)];
    wave_sync();
    for (int j = lane; j < N; j += NM_WAVE) zb[j] = zs[j];
    if (lane == 0 && itlog) itlog[(int64_t)b * steps + t] = it[b];
}

// asynchronous closed loop (bqp_closed_loop_nmpc_device): every instance runs at its own
// closed-loop step ts[b].  Launched after every SQP round, one wave per instance: an instance whose
// SQP stopped in this round and that has steps to go logs the step, steps the plant with u_0
// (mg_plant_kernel's arithmetic on the shared mg_plant_step: bqp_mg.h says why not mg_rk4 alone)
// and, unless that was its last step, takes the warm start (nmpc_loop_shift_kernel's) and the
// measured state for its next solve with the
// per-solve state reset - per instance the operations of the step-synchronous loop in its order.
// Every other wave leaves at once.  The indices are bqp_nmpc_advance.h's (checked on the host).
// TRACK (bqp_closed_loop_nmpc_track; k is read by that instantiation alone): lane 0 also logs theta
// of the step's solution, adds the step's disturbance to the plant's state - one addition after
// mg_plant_step, rounded once: the state the log stores and the next solve measures - and, while
// steps remain, copies the next step's set-point into the instance's slot of k.xr.
// PAR (bqp_closed_loop.plant_par; pp is read by those instantiations alone): the plant of the
// instance's own step ts[b], its four coefficients loaded before the parametrised mg_plant_step.
template <bool TRACK, bool PAR>
__global__ void __launch_bounds__(64) nmpc_loop_advance_kernel(NmpcAdvanceArgs a, NmpcTrackArgs k, PlantPar pp) {
    __shared__ double zs[NM_WAVE * NM_CPL];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.batch || !nmpc_advance_due(a, b)) return;   // uniform per wave
    const int t = a.ts[b], N = a.N;
    const bool more = t + 1 < a.steps;
    double* zb = a.z + (int64_t)b * (N + 1);
    // every read of z (u_0, the shift's sources) and of the counters before the wave sync, every
    // write after it
    const double u0 = zb[0];
    if constexpr (TRACK) {
        if (lane == 0) nmpc_track_log(k, a.steps, N, b, t, zb);
    }
    if (more)
        for (int j = lane; j < N; j += NM_WAVE) nmpc_shift_stage(zb, N, j, zs);
    wave_sync();
    if (more)
        for (int j = lane; j < N; j += NM_WAVE) nmpc_shift_store(zb, j, zs);
    if (lane == 0) {
        nmpc_advance_log(a, b, t);
        double x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = a.s[(int64_t)b * 4 + i] + a.xeq[i];
        const double u = u0 + a.ueq[0];
        if constexpr (PAR) {
            double p[4];
            plant_par_load(pp, b, t, p);
            mg_plant_step(p, a.plant, a.delta, x, u);
        } else {
            mg_plant_step(a.plant, a.delta, x, u);
        }
        if constexpr (TRACK) {
            nmpc_track_disturb(k, b, t, x);
            nmpc_track_next_ref(k, a.steps, b, t);
        }
        nmpc_advance_record(a, b, t, x, u);
        nmpc_advance_next(a, b, t);
    }
}

// bqp_closed_loop_nmpc_track, once per loop: the set-points of step 0 into the instances' slots
__global__ void nmpc_track_init_kernel(int batch, NmpcTrackArgs k) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * 4) return;
    k.xr[i] = k.ref[nmpc_track_at(k.sref, i >> 2, 0, i & 3)];
}

// bqp_closed_loop_nmpc_track, step-synchronous loop: step t of every instance, one thread each -
// what lane 0 of nmpc_loop_advance_kernel<true> does with the plant (the same inlined mg_plant_step,
// the same single addition) and with the logs, from the solve's flags; the warm start and the
// iteration log stay nmpc_loop_shift_kernel's, the set-point is the host's pointer into the schedule
template <bool PAR>
__global__ void nmpc_track_plant_kernel(NmpcAdvanceArgs a, NmpcTrackArgs k, int t, PlantPar pp) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.batch) return;
    const double* zb = a.z + (int64_t)b * (a.N + 1);
    nmpc_track_log(k, a.steps, a.N, b, t, zb);
    double x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = a.s[(int64_t)b * 4 + i] + a.xeq[i];
    const double u = zb[0] + a.ueq[0];
    if constexpr (PAR) {
        double p[4];
        plant_par_load(pp, b, t, p);
        mg_plant_step(p, a.plant, a.delta, x, u);
    } else {
        mg_plant_step(a.plant, a.delta, x, u);
    }
    nmpc_track_disturb(k, b, t, x);
    double* Xn = a.X + ((int64_t)b * (a.steps + 1) + t + 1) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a.s[(int64_t)b * 4 + i] = x[i] - a.xeq[i];
        Xn[i] = x[i];
    }
    a.U[(int64_t)b * a.steps + t] = u;
    if (a.flags) a.flags[(int64_t)b * a.steps + t] = a.flag[b];
}

// ------------------------------------------------------------------------------------------
// stage route (bqp_nmpc_dims.subproblem = 1): the sub-problem stays in stage form,
//   v_k = [dx_k; du_k; dtheta],  dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k du_k,
//   cost sum 0.5 v_k'W_k v_k + w_k'v_k,  bounds on dx_k (k = 1..N) and du_k, F_T rows at stage N,
// and is solved by the structured kernel with per-stage models (bqp_ocp.hip).  Condensed, it is
// the dense route's H, f, C, c (tests/nmpc_stage_ref.py).
// ------------------------------------------------------------------------------------------
// entry (r, c) of the 6 x 6 cost block in v = [x (4); u; theta]: running
//   2 (Mx'(delta Q) Mx + Mu'(delta R) Mu),  Mx = [I 0 -LAMBDA], Mu = [0 1 -PSI]
// or terminal 2 (Mx' P Mx + Mt' T Mt), Mt = [0 0 LAMBDA]; L'L = delta Q (or P), factors row-major
__device__ inline double nm_wentry(const double* L, const double* Lt, double lr, const double* LAM,
                                   double psi, bool term, int r, int c) {
    auto gram = [&](const double* F, int i, int j) {      // (F'F)[i][j]
        double v = 0.0;
        for (int q = 0; q < 4; ++q) v += F[4 * q + i] * F[4 * q + j];
        return v;
    };
    auto gl = [&](const double* F, int i) {               // (F'F LAMBDA)[i]
        double v = 0.0;
        for (int j = 0; j < 4; ++j) v += gram(F, i, j) * LAM[j];
        return v;
    };
    auto lgl = [&](const double* F) {                     // LAMBDA'F'F LAMBDA
        double v = 0.0;
        for (int i = 0; i < 4; ++i) v += LAM[i] * gl(F, i);
        return v;
    };
    const double R = lr * lr;
    if (r > c) { const int t = r; r = c; c = t; }
    if (c < 4) return 2.0 * gram(L, r, c);
    if (r < 4) return c == 4 ? 0.0 : -2.0 * gl(L, r);
    if (term) return (r == 5 && c == 5) ? 2.0 * (lgl(L) + lgl(Lt)) : 0.0;
    if (r == 4) return c == 4 ? 2.0 * R : -2.0 * R * psi;
    return 2.0 * (lgl(L) + psi * psi * R);
}

// once per solve: the shared cost blocks W ((N + 1) x 36), the polytope matrix
// Fp = [F_T[:, :4] | 0 | F_T[:, 4]] (mp x 6, column-major) and the bound map of F_x, F_u with its
// "not a box" flag; the map's soft members from the row weights (all hard without them) and, where
// q.xsl is set, the structured solve's weight tables xs_lin / xs_quad ((N + 1) x 4, shared by the
// batch; stage 0 is not read): the pair of the variable's softened row, 0 for a hard variable
__global__ void __launch_bounds__(64) nmpc_stage_table_kernel(NmpcArgs a, NmpcStageArgs s, NmpcSoftArgs q) {
    const int lane = threadIdx.x, N = a.N, mp = a.mp;
    for (int i = lane; i < 36 * (N + 1); i += NM_WAVE) {
        const int blk = i / 36, e = i % 36;
        const bool term = blk == N;
        s.W[i] = nm_wentry(term ? a.Lp : a.Lq, a.Lt, a.Lr[0], a.LAM, a.PSI[0], term, e % 6, e / 6);
    }
    for (int i = lane; i < 6 * mp; i += NM_WAVE) {
        const int c = i / mp, r = i % mp;
        s.Fp[i] = c < 4 ? a.FT[r + (int64_t)mp * c] : (c == 4 ? 0.0 : a.FT[r + (int64_t)mp * 4]);
    }
    if (lane == 0) {
        nmpc_bound_map_build(a.Fx, a.mx, a.Fu, a.mu, s.map);
        nmpc_bound_map_soften(s.map, a.mx, q.xs_lin, q.xs_quad);
    }
    if (q.xsl) {                     // uniform over the block
        __syncthreads();             // lane 0's map
        for (int i = lane; i < 4 * (N + 1); i += NM_WAVE) {
            double lin, quad;
            nmpc_var_pair(*s.map, i & 3, &lin, &quad);
            q.xsl[i] = i < 4 ? 0.0 : lin;
            q.xsq[i] = i < 4 ? 0.0 : quad;
        }
    }
}

// the bound map into LDS, lanes over its words (the caller syncs the wave)
// Map = NmpcBoundBox (the hard route: the box part alone) or NmpcBoundMap
template <class Map>
__device__ __forceinline__ void nm_load_map(const NmpcBoundMap* g, int lane, Map* l) {
    static_assert(sizeof(Map) % sizeof(int) == 0, "copied by ints");
    for (int i = lane; i < (int)(sizeof(Map) / sizeof(int)); i += NM_WAVE)
        ((int*)l)[i] = ((const int*)static_cast<const Map*>(g))[i];
}
template <bool SOFT> struct NmMapOf { typedef NmpcBoundBox type; };
template <> struct NmMapOf<true> { typedef NmpcBoundMap type; };

// The third mode of the rollout, one wave per instance: nm_rk4<true> from the measured state
// without sensitivities - the rollout and the stage Jacobians are the operation sequence of
// nmpc_rollout_kernel<true>.  Every lane carries the rollout (the work per stage is wave-uniform);
// lanes 0..25 store the stage's A_k | B_k | w_k, lanes i < mx + mu the value of row i of the next
// stage (rhs = -c) and the bound it stands for, lanes over the rows of F_T the terminal rhs and hp.
// SOFT: lane i < mx also sums its row's penalty phi_i(max(c, 0)) over the stages; one wave sum gives
// pen0, and cost0 = J + pen0.  The bounds stay as they are: the structured solve softens them.
// REF: the T term on LAMBDA theta - rho (NmLtRho); cost0 and the theta entry of w_N alone change.
template <bool SOFT, bool REF = false>
__global__ void __launch_bounds__(64) nmpc_stage_rollout_kernel(NmpcArgs a, NmpcStageArgs s, NmpcSoftArgs q,
                                                                NmpcRefArgs rf) {
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch || a.done[b]) return;
    const int N = a.N, n = a.n, m = a.m, mx = a.mx, mu = a.mu, ms = mx + mu, mp = a.mp;
    __shared__ double zsh[NM_WAVE * NM_CPL];
    __shared__ double cst[NO_END];
    __shared__ typename NmMapOf<SOFT>::type map;
    {
        const double* z = a.z + (int64_t)b * n;
        for (int j = lane; j < n; j += NM_WAVE) zsh[j] = z[j];
    }
    nm_load_consts(a, lane, cst);
    nm_load_map(s.map, lane, &map);
    wave_sync();
    const double th = zsh[N];
    const double ueq = cst[NO_UE], psi = cst[NO_PSI];
    double x[4];
    {
        const double* x0 = a.x0 + (int64_t)b * a.sx0;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = x0[i];
    }
    double* xlb = s.xlb + (int64_t)b * (N + 1) * 4;
    double* xub = s.xub + (int64_t)b * (N + 1) * 4;
    double* ulb = s.ulb + (int64_t)b * N;
    double* uub = s.uub + (int64_t)b * N;
    double* rhs = a.rhs + (int64_t)b * m;
    // the bounds no row stands for (stage 0 of the state bounds is not read by the solve)
    for (int i = lane; i < 4 * (N + 1); i += NM_WAVE) {
        if (i < 4 || map.rowof[i & 3][0] < 0) xlb[i] = -INFINITY;
        if (i < 4 || map.rowof[i & 3][1] < 0) xub[i] = INFINITY;
    }
    for (int i = lane; i < N; i += NM_WAVE) {
        if (map.rowof[4][0] < 0) ulb[i] = -INFINITY;
        if (map.rowof[4][1] < 0) uub[i] = INFINITY;
    }
    // the lane's slot in the stage record [A_k (16, column-major) | B_k (4) | w_k (6)]
    double* rec = nullptr;
    int rstride = 0;
    if (lane < 16) { rec = s.A + (int64_t)b * N * 16 + lane; rstride = 16; }
    else if (lane < 20) { rec = s.B + (int64_t)b * N * 4 + (lane - 16); rstride = 4; }
    else if (lane < 26) { rec = s.w + (int64_t)b * (N + 1) * 6 + (lane - 20); rstride = 6; }
    // the lane's row of [F_x; F_u] as a bound: array and stride over the stages
    double* bnd = nullptr;
    int bstride = 0;
    if (lane < ms) {
        const bool isx = nmpc_row_is_state(mx, lane);
        bnd = (isx ? (map.side[lane] ? xub : xlb) : (map.side[lane] ? uub : ulb)) + nmpc_bound_index(map, mx, 1, lane);
        bstride = isx ? 4 : 1;
    }
    double J = 0.0;
    double pen = 0.0;                // SOFT: the lane's row's penalty over the stages
    // weighted residual e = L (xx - x_eq - LAMBDA theta) as nmpc_rollout_kernel's xresidual forms
    // it, and the x block of the stage gradient 2 L'e
    auto xgrad = [&](int oL, const double (&xx)[4], double (&wx)[4]) __attribute__((always_inline)) {
        double e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double er = 0.0;
#pragma unroll
            for (int c2 = r; c2 < 4; ++c2) er += cst[oL + 4 * r + c2] * (xx[c2] - cst[NO_XE + c2] - cst[NO_L + c2] * th);
            J += er * er;
            e[r] = er;
        }
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r <= c2; ++r) v += cst[oL + 4 * r + c2] * e[r];
            wx[c2] = 2.0 * v;
        }
    };
    // theta entry of the stage gradient from its x and u entries: -LAMBDA'wx - PSI wu
    auto thgrad = [&](const double (&wx)[4], double wu) __attribute__((always_inline)) {
        double v = 0.0;
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) v += cst[NO_L + c2] * wx[c2];
        return -v - psi * wu;
    };
    for (int k = 0; k < N; ++k) {
        const double vk = zsh[k];
        double wx[4];
        xgrad(NO_Q, x, wx);
        const double lr = cst[NO_R];
        const double eu = lr * (vk - psi * th);
        J += eu * eu;
        const double wu = 2.0 * lr * eu;
        const double wt = thgrad(wx, wu);
        double xn[4], AB[4][5];
        nm_rk4<true>(a.delta, x, vk + ueq, xn, AB);
        // the lane's entry of the record, picked by compares (no indexed register array)
        double rv = 0.0;
#pragma unroll
        for (int l = 0; l < 16; ++l) rv = lane == l ? AB[l & 3][l >> 2] : rv;
#pragma unroll
        for (int i = 0; i < 4; ++i) rv = lane == 16 + i ? AB[i][4] : rv;
#pragma unroll
        for (int i = 0; i < 4; ++i) rv = lane == 20 + i ? wx[i] : rv;
        rv = lane == 24 ? wu : rv;
        rv = lane == 25 ? wt : rv;
        if (rec) rec[(int64_t)k * rstride] = rv;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = xn[i];
        // row `lane` of stage k + 1: F_x (x_{k+1} - x_eq) <= h_x, F_u (u_k - u_eq) <= h_u
        if (lane < ms) {
            double cv;
            if (lane < mx) {
                cv = -cst[NO_HX + lane];
#pragma unroll
                for (int c2 = 0; c2 < 4; ++c2) cv += cst[NO_FX + lane + mx * c2] * (x[c2] - cst[NO_XE + c2]);
            } else {
                cv = cst[NO_FU + lane - mx] * vk - cst[NO_HU + lane - mx];
            }
            rhs[nmpc_stage_row(mx, mu, k + 1, lane)] = -cv;
            bnd[(int64_t)k * bstride] = nmpc_bound_value(map, lane, -cv);
            if constexpr (SOFT) {
                if (lane < mx) pen += nmpc_phi(map.l1[lane], map.l2[lane], fmax(cv, 0.0));
            }
        }
    }
    // terminal P on x_N, T on LAMBDA theta: w_N = [2 Lp'e; 0; -LAMBDA'(2 Lp'e) + 2 (Lt LAMBDA)'(Lt LAMBDA) theta]
    {
        double wx[4];
        xgrad(NO_P, x, wx);
        double wt = thgrad(wx, 0.0);
        const NmLtRho<REF> ltr(rf, b, cst);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double w = 0.0;
#pragma unroll
            for (int c2 = r; c2 < 4; ++c2) w += cst[NO_T + 4 * r + c2] * cst[NO_L + c2];
            const double e = ltr.row(w * th, r);
            J += e * e;
            wt += 2.0 * w * e;
        }
        double rv = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) rv = lane == 20 + i ? wx[i] : rv;
        rv = lane == 25 ? wt : rv;
        if (lane >= 20 && lane < 26) rec[(int64_t)N * rstride] = rv;
    }
    // terminal rows F_T [x_N - x_eq; theta] <= h_T, lanes over the rows
    const int64_t rT = nmpc_term_row(N, mx, mu, 0);
    double* hp = s.hp + (int64_t)b * mp;
    for (int r = lane; r < mp; r += NM_WAVE) {
        double F[5];
#pragma unroll
        for (int c2 = 0; c2 < 5; ++c2) F[c2] = a.FT[r + (int64_t)mp * c2];
        double cv = F[4] * th - a.hT[r];
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) cv += F[c2] * (x[c2] - cst[NO_XE + c2]);
        rhs[rT + r] = -cv;
        hp[r] = -cv;
    }
    if constexpr (SOFT) {
        const double P0 = wsum(pen);
        if (lane == 0) { q.pen0[b] = P0; a.cost0[b] = J + P0; }
    } else {
        if (lane == 0) a.cost0[b] = J;
    }
}

// After the structured solve, one wave per instance (a finished instance leaves at once): the step
// d = [du; dtheta], the multipliers in NMPC row order through the bound map, the sub-problem's
// exit flag, and by one backward adjoint sweep over A_k, B_k the condensed gradient f (from the
// w_k) and C'lam (from the multipliers) that nmpc_update_kernel<true> reads:
//   p_N = x part (+ F_x'lam_N + F_T[:, :4]'lam_T),  g_k = u part + B_k'p_{k+1} (+ F_u lam),
//   p_k = x part + A_k'p_{k+1} (+ F_x'lam_k),  theta entry = sum of the theta parts (+ F_T[:, 4]'lam_T)
// SOFT: a softened row's multiplier is that of the softened bound, lam_x / |a|, by the same map;
// the structured solve's slacks s_x give the row slacks |a| s_x and the sub-problem's model penalty
// plin = sum phi_i(|a| s_x), lanes over the rows, one wave sum.
template <bool SOFT>
__global__ void __launch_bounds__(64) nmpc_stage_backmap_kernel(NmpcArgs a, NmpcStageArgs s, NmpcSoftArgs q) {
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch || a.done[b]) return;
    const int N = a.N, n = a.n, m = a.m, mx = a.mx, mu = a.mu, mp = a.mp;
    __shared__ typename NmMapOf<SOFT>::type map;
    __shared__ double gf[NM_WAVE * NM_CPL], gl[NM_WAVE * NM_CPL];
    nm_load_map(s.map, lane, &map);
    wave_sync();
    const double* uo = s.uo + (int64_t)b * N;
    const double* lamx = s.lamx + (int64_t)b * (N + 1) * 8;
    const double* lamu = s.lamu + (int64_t)b * N * 2;
    const double* lamp = s.lamp + (int64_t)b * mp;
    double* d = a.d + (int64_t)b * n;
    double* lam = a.lam + (int64_t)b * m;
    for (int j = lane; j < N; j += NM_WAVE) d[j] = uo[j];
    if (lane == 0) {
        d[N] = s.tho[b];
        a.qpflag[b] = s.sflag[b];
    }
    for (int r = lane; r < m; r += NM_WAVE) lam[r] = nmpc_stage_dual(map, N, mx, mu, r, lamx, lamu, lamp);
    if constexpr (SOFT) {
        const double* sx = q.sx + (int64_t)b * (N + 1) * 8;
        const int ms = mx + mu;
        double pl = 0.0;
        for (int r = lane; r < ms * N; r += NM_WAVE) {
            const int k = r / ms + 1, i = r % ms;
            if (i < mx && map.soft[i])
                pl += nmpc_phi(map.l1[i], map.l2[i], nmpc_row_slack(map, i, sx[nmpc_sx_index(map, k, i)]));
        }
        pl = wsum(pl);
        if (lane == 0) q.plin[b] = pl;
    }
    // F_T'lam_T: lanes over the rows, five wave sums
    double tT[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = lane; r < mp; r += NM_WAVE) {
        const double lr = lamp[r];
#pragma unroll
        for (int c2 = 0; c2 < 5; ++c2) tT[c2] = fma(a.FT[r + (int64_t)mp * c2], lr, tT[c2]);
    }
#pragma unroll
    for (int c2 = 0; c2 < 5; ++c2) tT[c2] = wsum(tT[c2]);
    // per (variable, side) the row's entry of F_x / F_u and its scale (0 and 1 where no row is):
    // the row's share of C'lam is entry * (bound multiplier / scale), as lam above
    double Fe[NMS_NVAR][2], sc[NMS_NVAR][2];
#pragma unroll
    for (int v = 0; v < NMS_NVAR; ++v)
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
            const int i = map.rowof[v][sd];
            Fe[v][sd] = i < 0 ? 0.0 : (v < 4 ? a.Fx[i + mx * v] : a.Fu[i - mx]);
            sc[v][sd] = i < 0 ? 1.0 : map.scale[i];
        }
    auto xrows = [&](int k, double (&p)[4]) __attribute__((always_inline)) {   // p += F_x'lam_k
#pragma unroll
        for (int v = 0; v < 4; ++v)
            p[v] += Fe[v][0] * (lamx[nmpc_lamx_index(k, 0, v)] / sc[v][0]) +
                    Fe[v][1] * (lamx[nmpc_lamx_index(k, 1, v)] / sc[v][1]);
    };
    const double* A = s.A + (int64_t)b * N * 16;
    const double* B = s.B + (int64_t)b * N * 4;
    const double* w = s.w + (int64_t)b * (N + 1) * 6;
    double pf[4], pl[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { pf[i] = w[6 * N + i]; pl[i] = tT[i]; }
    xrows(N, pl);
    double thf = w[6 * N + 5];
    for (int k = N - 1; k >= 0; --k) {
        double Ak[16], Bk[4], wk[6];
#pragma unroll
        for (int i = 0; i < 16; ++i) Ak[i] = A[16 * k + i];
#pragma unroll
        for (int i = 0; i < 4; ++i) Bk[i] = B[4 * k + i];
#pragma unroll
        for (int i = 0; i < 6; ++i) wk[i] = w[6 * k + i];
        double g1 = wk[4], g2 = Fe[4][0] * (lamu[nmpc_lamu_index(k, 0)] / sc[4][0]) +
                                Fe[4][1] * (lamu[nmpc_lamu_index(k, 1)] / sc[4][1]);
#pragma unroll
        for (int i = 0; i < 4; ++i) { g1 += Bk[i] * pf[i]; g2 += Bk[i] * pl[i]; }
        if (lane == 0) { gf[k] = g1; gl[k] = g2; }
        thf += wk[5];
        if (k > 0) {
            double qf[4], ql[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v1 = wk[j], v2 = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) { v1 += Ak[i + 4 * j] * pf[i]; v2 += Ak[i + 4 * j] * pl[i]; }
                qf[j] = v1; ql[j] = v2;
            }
            xrows(k, ql);
#pragma unroll
            for (int j = 0; j < 4; ++j) { pf[j] = qf[j]; pl[j] = ql[j]; }
        }
    }
    if (lane == 0) { gf[N] = thf; gl[N] = tT[4]; }
    wave_sync();
    for (int j = lane; j < n; j += NM_WAVE) {
        a.f[(int64_t)b * n + j] = gf[j];
        a.ctl[(int64_t)b * n + j] = gl[j];
    }
}

// ------------------------------------------------------------------------------------------
// multiple shooting on the stage route (bqp_nmpc_dims.shooting = 1): the states stay decision
// variables.  The iterate is (X, z), X (N + 1) x 4 absolute with x_0 pinned to the measured state;
// per stage k < N  f_k = dynamic(delta, x_k, u_k) (nm_rk4<true>, as the rollouts above), A_k, B_k its
// Jacobians and the defect c_k = f_k - x_{k+1}; the sub-problem is the stage route's with
//   dx_0 = 0,  dx_{k+1} = A_k dx_k + B_k du_k + c_k
// and w_k, the bounds and hp from the iterate's own x_k (tests/nmpc_dms_ref.py).  Everything a
// stage needs depends on (x_k, u_k, x_{k+1}, theta) alone, so a lane owns a stage: one wave per
// instance, lanes over the stages in nmpc_dms_passes(N) <= 2 passes (bqp_nmpc_dms.h), the iterate
// in LDS, wave sums for what is summed over the stages.  Only nmpc_dms_start_kernel, once per solve
// that is given no states, rolls out.
//   nmpc_dms_start_kernel      X = the rollout of z (a solve that starts without states)
//   nmpc_dms_linearize_kernel  A_k | B_k | c_k | w_k, the rows as bounds, rhs = -rows, hp, cost0
//   nmpc_dms_backmap_kernel    d, lam in NMPC row order, the sub-problem's flag, sum w_k'v_k, the
//                              full-space stationarity residual, |grad J|, max |pi|
//   nmpc_dms_trial_kernel      one wave per (instance, trial): J, V + E at (X, z) + 2^-t (dX, d)
//   nmpc_dms_update_kernel     nu, Armijo, (X, z) += alpha (dX, d), the stopping clauses
//   nmpc_dms_loop_states_kernel  closed loop: the warm start of the states
// ------------------------------------------------------------------------------------------
// weighted residual e = L (xx - x_eq - LAMBDA theta) as nmpc_stage_rollout_kernel's xgrad forms it:
// J += e'e, wx = 2 L'e
__device__ __forceinline__ void nmd_xgrad(const double* cst, int oL, const double (&xx)[4], double th,
                                          double& J, double (&wx)[4]) {
    double e[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double er = 0.0;
#pragma unroll
        for (int c2 = r; c2 < 4; ++c2) er += cst[oL + 4 * r + c2] * (xx[c2] - cst[NO_XE + c2] - cst[NO_L + c2] * th);
        J += er * er;
        e[r] = er;
    }
#pragma unroll
    for (int c2 = 0; c2 < 4; ++c2) {
        double v = 0.0;
#pragma unroll
        for (int r = 0; r <= c2; ++r) v += cst[oL + 4 * r + c2] * e[r];
        wx[c2] = 2.0 * v;
    }
}
// theta entry of the stage gradient from its x and u entries: -LAMBDA'wx - PSI wu
__device__ __forceinline__ double nmd_thgrad(const double* cst, const double (&wx)[4], double wu) {
    double v = 0.0;
#pragma unroll
    for (int c2 = 0; c2 < 4; ++c2) v += cst[NO_L + c2] * wx[c2];
    return -v - cst[NO_PSI] * wu;
}
// the terminal T term on LAMBDA theta: J += |Lt LAMBDA theta|^2, returns its theta gradient
__device__ __forceinline__ double nmd_tterm(const double* cst, double th, double& J) {
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double w = 0.0;
#pragma unroll
        for (int c2 = r; c2 < 4; ++c2) w += cst[NO_T + 4 * r + c2] * cst[NO_L + c2];
        const double e = w * th;
        J += e * e;
        g += 2.0 * w * e;
    }
    return g;
}
// the same on LAMBDA theta - rho (a set-point: NmLtRho<true>)
__device__ __forceinline__ double nmd_tterm(const double* cst, double th, double& J, const NmLtRho<true>& ltr) {
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double w = 0.0;
#pragma unroll
        for (int c2 = r; c2 < 4; ++c2) w += cst[NO_T + 4 * r + c2] * cst[NO_L + c2];
        const double e = ltr.row(w * th, r);
        J += e * e;
        g += 2.0 * w * e;
    }
    return g;
}
// value of row i of [F_x; F_u]: F_x (x - x_eq) - h_x (i < mx) or F_u v - h_u
__device__ __forceinline__ double nmd_xrow(const double* cst, int mx, int i, const double (&x)[4]) {
    double cv = -cst[NO_HX + i];
#pragma unroll
    for (int c2 = 0; c2 < 4; ++c2) cv += cst[NO_FX + i + mx * c2] * (x[c2] - cst[NO_XE + c2]);
    return cv;
}
__device__ __forceinline__ double nmd_urow(const double* cst, int mx, int i, double v) {
    return cst[NO_FU + i - mx] * v - cst[NO_HU + i - mx];
}
// the terminal rows F_T [x_N - x_eq; theta] - h_T, lanes over the rows: sum max(row, 0); STORE:
// rhs = hp = -row
template <bool STORE>
__device__ __forceinline__ double nmd_term_rows(const NmpcArgs& a, const double* cst, int lane,
                                                const double (&xN)[4], double th, double* rhsT, double* hp) {
    const int mp = a.mp;
    double Vt = 0.0;
    for (int r = lane; r < mp; r += NM_WAVE) {
        double F[5];
#pragma unroll
        for (int c2 = 0; c2 < 5; ++c2) F[c2] = a.FT[r + (int64_t)mp * c2];
        double cv = F[4] * th - a.hT[r];
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) cv += F[c2] * (xN[c2] - cst[NO_XE + c2]);
        Vt += fmax(cv, 0.0);
        if (STORE) { rhsT[r] = -cv; hp[r] = -cv; }
    }
    return Vt;
}

// a solve that is given no states starts from the rollout of z: the one serial chain of this route,
// once per solve (every lane carries it, lane 0 stores); a solve given states does not launch it
__global__ void __launch_bounds__(64) nmpc_dms_start_kernel(NmpcArgs a, NmpcDmsArgs m) {
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch) return;
    const int N = a.N;
    const double* z = a.z + (int64_t)b * a.n;
    double* X = m.X + (int64_t)b * nmpc_dms_x_stride(N);
    const double ueq = a.ueq[0];
    double x[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = a.x0[(int64_t)b * a.sx0 + i];
    for (int k = 0; k <= N; ++k) {
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) X[nmpc_dms_x_index(k, i)] = x[i];
        }
        if (k == N) break;
        double xn[4], AB[4][5];
        nm_rk4<true>(a.delta, x, z[k] + ueq, xn, AB);   // <true>: the bits of the linearisation's f_k
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = xn[i];
    }
}

// the iterate into LDS: zs = z + alpha d, Xs = X + alpha dX with stage 0 the measured state (the
// caller syncs the wave); alpha = 0 reads neither d nor dX
__device__ __forceinline__ void nmd_load_iterate(const NmpcArgs& a, const NmpcDmsArgs& m, int b, int lane,
                                                 double alpha, double* zs, double* Xs) {
    const int N = a.N, n = a.n;
    const double* z = a.z + (int64_t)b * n;
    const double* d = a.d + (int64_t)b * n;
    const double* X = m.X + (int64_t)b * nmpc_dms_x_stride(N);
    const double* dX = m.dX + (int64_t)b * nmpc_dms_x_stride(N);
    for (int j = lane; j < n; j += NM_WAVE) zs[j] = alpha != 0.0 ? z[j] + alpha * d[j] : z[j];
    for (int j = lane; j < 4 * (N + 1); j += NM_WAVE) {
        double v;
        if (j < 4) v = a.x0[(int64_t)b * a.sx0 + j];
        else v = alpha != 0.0 ? X[j] + alpha * dX[j] : X[j];
        Xs[j] = v;
    }
}

// REF: the lane that owns stage N forms Lt rho for its T term (NmLtRho); rf is read by that
// instantiation alone
template <bool REF>
__global__ void __launch_bounds__(64) nmpc_dms_linearize_kernel(NmpcArgs a, NmpcStageArgs s, NmpcDmsArgs m,
                                                                NmpcRefArgs rf) {
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch || a.done[b]) return;
    const int N = a.N, mx = a.mx, mu = a.mu, ms = mx + mu, mp = a.mp;
    __shared__ double zsh[NM_WAVE * NM_CPL];
    __shared__ double Xs[NMD_XLDS];
    __shared__ double cst[NO_END];
    __shared__ NmpcBoundBox map;
    nmd_load_iterate(a, m, b, lane, 0.0, zsh, Xs);
    nm_load_consts(a, lane, cst);
    nm_load_map(s.map, lane, &map);
    wave_sync();
    const double th = zsh[N], ueq = cst[NO_UE], psi = cst[NO_PSI];
    double* Xg = m.X + (int64_t)b * nmpc_dms_x_stride(N);
    double* cg = m.c + (int64_t)b * nmpc_dms_c_stride(N);
    double* Ag = s.A + (int64_t)b * N * 16;
    double* Bg = s.B + (int64_t)b * N * 4;
    double* wg = s.w + (int64_t)b * (N + 1) * 6;
    double* xlb = s.xlb + (int64_t)b * (N + 1) * 4;
    double* xub = s.xub + (int64_t)b * (N + 1) * 4;
    double* ulb = s.ulb + (int64_t)b * N;
    double* uub = s.uub + (int64_t)b * N;
    double* rhs = a.rhs + (int64_t)b * a.m;
    if (lane < 4) Xg[lane] = Xs[lane];          // x_0 = the measured state, in the returned X too
    // the bounds no row stands for (stage 0 of the state bounds is not read by the solve)
    for (int i = lane; i < 4 * (N + 1); i += NM_WAVE) {
        if (i < 4 || map.rowof[i & 3][0] < 0) xlb[i] = -INFINITY;
        if (i < 4 || map.rowof[i & 3][1] < 0) xub[i] = INFINITY;
    }
    for (int i = lane; i < N; i += NM_WAVE) {
        if (map.rowof[4][0] < 0) ulb[i] = -INFINITY;
        if (map.rowof[4][1] < 0) uub[i] = INFINITY;
    }
    double J = 0.0;
    const int np = nmpc_dms_passes(N);
    for (int ps = 0; ps < np; ++ps) {
        const int k = nmpc_dms_stage(N, lane, ps);
        if (k < 0) continue;
        double x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = Xs[nmpc_dms_x_index(k, i)];
        double wx[4], wu = 0.0, wt;
        if (nmpc_dms_has_step(N, k)) {
            const double vk = zsh[k];
            nmd_xgrad(cst, NO_Q, x, th, J, wx);
            const double lr = cst[NO_R];
            const double eu = lr * (vk - psi * th);
            J += eu * eu;
            wu = 2.0 * lr * eu;
            wt = nmd_thgrad(cst, wx, wu);
            double xn[4], AB[4][5];
            nm_rk4<true>(a.delta, x, vk + ueq, xn, AB);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) Ag[nmpc_dms_a_index(k, i, j)] = AB[i][j];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                Bg[nmpc_dms_b_index(k, i)] = AB[i][4];
                cg[nmpc_dms_c_index(k, i)] = xn[i] - Xs[nmpc_dms_x_index(k + 1, i)];
            }
            // the rows of F_u on u_k: NMPC stage k + 1
            for (int i = mx; i < ms; ++i) {
                const double cv = nmd_urow(cst, mx, i, vk);
                rhs[nmpc_stage_row(mx, mu, k + 1, i)] = -cv;
                (map.side[i] ? uub : ulb)[nmpc_bound_index(map, mx, k + 1, i)] = nmpc_bound_value(map, i, -cv);
            }
        } else {
            // terminal P on x_N, T on LAMBDA theta
            nmd_xgrad(cst, NO_P, x, th, J, wx);
            wt = nmd_thgrad(cst, wx, 0.0);
            if constexpr (REF) wt += nmd_tterm(cst, th, J, NmLtRho<true>(rf, b, cst));
            else wt += nmd_tterm(cst, th, J);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) wg[nmpc_dms_w_index(k, i)] = wx[i];
        wg[nmpc_dms_w_index(k, 4)] = wu;
        wg[nmpc_dms_w_index(k, 5)] = wt;
        // the rows of F_x on x_k: NMPC stage k
        if (nmpc_dms_has_state_rows(N, k)) {
            for (int i = 0; i < mx; ++i) {
                const double cv = nmd_xrow(cst, mx, i, x);
                rhs[nmpc_stage_row(mx, mu, k, i)] = -cv;
                (map.side[i] ? xub : xlb)[nmpc_bound_index(map, mx, k, i)] = nmpc_bound_value(map, i, -cv);
            }
        }
    }
    double xN[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xN[i] = Xs[nmpc_dms_x_index(N, i)];
    nmd_term_rows<true>(a, cst, lane, xN, th, rhs + nmpc_term_row(N, mx, mu, 0), s.hp + (int64_t)b * mp);
    J = wsum(J);
    if (lane == 0) a.cost0[b] = J;
}

// After the structured solve, one wave per instance (a finished instance leaves at once), lanes over
// the stages.  The residual is that of the Lagrangian of bqp_ocp_duals (bqp.h) at the iterate:
//   x_k (1 <= k <= N): w_k[x] + A_k'pi_k (k < N) - pi_{k-1} + F_x'lam_k (+ F_T[:, :4]'lam_T at N)
//   u_k (k < N):       w_k[u] + B_k'pi_k + F_u'lam_{k+1}
//   theta:             sum_k w_k[theta] + F_T[:, 4]'lam_T
// and |grad J| the largest of the w entries it sums (theta: of the sum)
__global__ void __launch_bounds__(64) nmpc_dms_backmap_kernel(NmpcArgs a, NmpcStageArgs s, NmpcDmsArgs m) {
    const int lane = threadIdx.x, b = blockIdx.x;
    if (b >= a.batch || a.done[b]) return;
    const int N = a.N, n = a.n, mx = a.mx, mu = a.mu, mp = a.mp;
    __shared__ NmpcBoundBox map;
    nm_load_map(s.map, lane, &map);
    wave_sync();
    const double* uo = s.uo + (int64_t)b * N;
    const double* lamx = s.lamx + (int64_t)b * (N + 1) * 8;
    const double* lamu = s.lamu + (int64_t)b * N * 2;
    const double* lamp = s.lamp + (int64_t)b * mp;
    const double* dX = m.dX + (int64_t)b * nmpc_dms_x_stride(N);
    const double* pi = m.pi + (int64_t)b * nmpc_dms_c_stride(N);
    const double* A = s.A + (int64_t)b * N * 16;
    const double* B = s.B + (int64_t)b * N * 4;
    const double* w = s.w + (int64_t)b * (N + 1) * 6;
    double* d = a.d + (int64_t)b * n;
    double* lam = a.lam + (int64_t)b * a.m;
    const double dth = s.tho[b];
    for (int j = lane; j < N; j += NM_WAVE) d[j] = uo[j];
    if (lane == 0) {
        d[N] = dth;
        a.qpflag[b] = s.sflag[b];
    }
    for (int r = lane; r < a.m; r += NM_WAVE) lam[r] = nmpc_stage_dual(map, N, mx, mu, r, lamx, lamu, lamp);
    // F_T'lam_T: lanes over the rows, five wave sums
    double tT[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int r = lane; r < mp; r += NM_WAVE) {
        const double lr = lamp[r];
#pragma unroll
        for (int c2 = 0; c2 < 5; ++c2) tT[c2] = fma(a.FT[r + (int64_t)mp * c2], lr, tT[c2]);
    }
#pragma unroll
    for (int c2 = 0; c2 < 5; ++c2) tT[c2] = wsum(tT[c2]);
    // per (variable, side) the row's entry of F_x / F_u and its scale, as nmpc_stage_backmap_kernel
    double Fe[NMS_NVAR][2], sc[NMS_NVAR][2];
#pragma unroll
    for (int v = 0; v < NMS_NVAR; ++v)
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
            const int i = map.rowof[v][sd];
            Fe[v][sd] = i < 0 ? 0.0 : (v < 4 ? a.Fx[i + mx * v] : a.Fu[i - mx]);
            sc[v][sd] = i < 0 ? 1.0 : map.scale[i];
        }
    double sw = 0.0, ths = 0.0, st = 0.0, gn = 0.0, pim = 0.0;
    const int np = nmpc_dms_passes(N);
    for (int ps = 0; ps < np; ++ps) {
        const int k = nmpc_dms_stage(N, lane, ps);
        if (k < 0) continue;
        double wk[6], pk[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int e = 0; e < 6; ++e) wk[e] = w[nmpc_dms_w_index(k, e)];
#pragma unroll
        for (int i = 0; i < 4; ++i) sw += wk[i] * dX[nmpc_dms_x_index(k, i)];
        sw += wk[5] * dth;
        ths += wk[5];
        if (nmpc_dms_has_step(N, k)) {
            sw += wk[4] * uo[k];
            double ru = wk[4] + Fe[4][0] * (lamu[nmpc_lamu_index(k, 0)] / sc[4][0]) +
                        Fe[4][1] * (lamu[nmpc_lamu_index(k, 1)] / sc[4][1]);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pk[i] = pi[nmpc_dms_pi_index(k, i)];
                pim = fmax(pim, fabs(pk[i]));
                ru += B[nmpc_dms_b_index(k, i)] * pk[i];
            }
            st = fmax(st, fabs(ru));
            gn = fmax(gn, fabs(wk[4]));
        }
        if (nmpc_dms_has_state_rows(N, k)) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double r = wk[j] - pi[nmpc_dms_pi_index(k - 1, j)] +
                           Fe[j][0] * (lamx[nmpc_lamx_index(k, 0, j)] / sc[j][0]) +
                           Fe[j][1] * (lamx[nmpc_lamx_index(k, 1, j)] / sc[j][1]);
                if (k == N) r += tT[j];
                else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) r += A[nmpc_dms_a_index(k, i, j)] * pk[i];
                }
                st = fmax(st, fabs(r));
                gn = fmax(gn, fabs(wk[j]));
            }
        }
    }
    sw = wsum(sw); ths = wsum(ths); st = wmax(st); gn = wmax(gn); pim = wmax(pim);
    st = fmax(st, fabs(ths + tT[4]));
    gn = fmax(gn, fabs(ths));
    if (lane == 0) {
        a.stat[b] = st;
        m.sw[b] = sw;
        m.gn[b] = gn;
        m.pimax[b] = pim;
    }
}

// one wave per (instance, trial): cost, row violation V and defect norm E = sum_k |f_k - x_{k+1}|_1
// at (X, z) + 2^-t (dX, d), the stages in parallel; costT = J, violT = V + E (not finite where an f_k
// is not: the update rejects the trial)
template <bool REF>
__global__ void __launch_bounds__(64) nmpc_dms_trial_kernel(NmpcArgs a, NmpcDmsArgs m, NmpcRefArgs rf) {
    const int lane = threadIdx.x;
    const int nt = a.ntrial;
    const int b = blockIdx.x / nt, t = blockIdx.x % nt;
    if (b >= a.batch || a.done[b]) return;
    const int N = a.N, mx = a.mx, ms = mx + a.mu;
    __shared__ double zsh[NM_WAVE * NM_CPL];
    __shared__ double Xs[NMD_XLDS];
    __shared__ double cst[NO_END];
    nmd_load_iterate(a, m, b, lane, ldexp(1.0, -t), zsh, Xs);
    nm_load_consts(a, lane, cst);
    wave_sync();
    const double th = zsh[N], ueq = cst[NO_UE], psi = cst[NO_PSI];
    double J = 0.0, V = 0.0, E = 0.0;
    const int np = nmpc_dms_passes(N);
    for (int ps = 0; ps < np; ++ps) {
        const int k = nmpc_dms_stage(N, lane, ps);
        if (k < 0) continue;
        double x[4], wx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = Xs[nmpc_dms_x_index(k, i)];
        if (nmpc_dms_has_step(N, k)) {
            const double vk = zsh[k];
            nmd_xgrad(cst, NO_Q, x, th, J, wx);
            const double eu = cst[NO_R] * (vk - psi * th);
            J += eu * eu;
            double xn[4], AB[4][5];
            nm_rk4<false>(a.delta, x, vk + ueq, xn, AB);
#pragma unroll
            for (int i = 0; i < 4; ++i) E += fabs(xn[i] - Xs[nmpc_dms_x_index(k + 1, i)]);
            for (int i = mx; i < ms; ++i) V += fmax(nmd_urow(cst, mx, i, vk), 0.0);
        } else {
            nmd_xgrad(cst, NO_P, x, th, J, wx);
            if constexpr (REF) nmd_tterm(cst, th, J, NmLtRho<true>(rf, b, cst));
            else nmd_tterm(cst, th, J);
        }
        if (nmpc_dms_has_state_rows(N, k))
            for (int i = 0; i < mx; ++i) V += fmax(nmd_xrow(cst, mx, i, x), 0.0);
    }
    double xN[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) xN[i] = Xs[nmpc_dms_x_index(N, i)];
    V += nmd_term_rows<false>(a, cst, lane, xN, th, nullptr, nullptr);
    J = wsum(J); V = wsum(V); E = wsum(E);
    if (lane == 0) {
        a.costT[(int64_t)b * nt + t] = J;
        a.violT[(int64_t)b * nt + t] = V + E;
    }
}

// nmpc_update_kernel<true> for the iterate (X, z): the step over (dX, d), feasibility of the rows
// and of the defects, the back-map's full-space stationarity against 10 tol (1 + |grad J|), the
// merit function phi = J + nu (V + E) with nu <- max(nu, 1.1 max(max lam, max |pi|)) and
// D = sum w_k'v_k - nu (V0 + E0)
__global__ void __launch_bounds__(64) nmpc_dms_update_kernel(NmpcArgs a, NmpcDmsArgs m) {
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    if (b >= a.batch || a.done[b]) return;
    const int N = a.N, n = a.n, mr = a.m;
    double* z = a.z + (int64_t)b * n;
    const double* d = a.d + (int64_t)b * n;
    double* X = m.X + (int64_t)b * nmpc_dms_x_stride(N);
    const double* dX = m.dX + (int64_t)b * nmpc_dms_x_stride(N);
    const double* c = m.c + (int64_t)b * nmpc_dms_c_stride(N);
    const double* lam = a.lam + (int64_t)b * mr;
    const double* rhs = a.rhs + (int64_t)b * mr;
    const int qflag = a.qpflag[b];
    double dn = 0.0, zn = 0.0, viol = -INFINITY, V0 = 0.0, lmax = 0.0, cmax = 0.0, E0 = 0.0;
    for (int j = lane; j < n; j += NM_WAVE) {
        dn = fmax(dn, fabs(d[j]));
        zn = fmax(zn, fabs(z[j]));
    }
    for (int j = 4 + lane; j < 4 * (N + 1); j += NM_WAVE) dn = fmax(dn, fabs(dX[j]));
    for (int r = lane; r < mr; r += NM_WAVE) {
        const double cv = -rhs[r];
        viol = fmax(viol, cv);
        V0 += fmax(cv, 0.0);
        lmax = fmax(lmax, lam[r]);
    }
    for (int j = lane; j < 4 * N; j += NM_WAVE) {
        cmax = fmax(cmax, fabs(c[j]));
        E0 += fabs(c[j]);
    }
    dn = wmax(dn); zn = wmax(zn); viol = wmax(viol); V0 = wsum(V0); lmax = wmax(lmax);
    cmax = wmax(cmax); E0 = wsum(E0);
    const double st = a.stat[b], gn = m.gn[b];
    const bool feas0 = viol <= 1e-9 && cmax <= 1e-9;
    const double VE0 = V0 + E0;
    const double J0 = a.cost0[b];
    int it = a.iters[b];
    int flag = 0;
    bool fin = false;
    const bool qp_ok = qflag == 1 || ((qflag == 0 || qflag == -8) && isfinite(dn) && isfinite(st));
    if (qflag == -2 || !qp_ok || !isfinite(J0) || !isfinite(VE0)) {
        flag = (qflag == -2) ? -2 : -8;   // sub-problem infeasible / failed, or a non-finite iterate
        fin = true;
    } else if (feas0 && ((qflag == 1 && dn <= a.tol_step * (1.0 + zn) && st <= a.tol_stat * (1.0 + gn)) ||
                         (it > 0 && dn <= 1e-6 * (1.0 + zn) &&
                          (qflag != 1 || fabs(a.cprev[b] - J0) <= 1e-12 * (1.0 + fabs(J0)))))) {
        flag = 1;
        fin = true;
    }
    if (!fin) {
        const double nu = fmax(a.nu[b], 1.1 * fmax(lmax, m.pimax[b]));
        const double D = m.sw[b] - nu * VE0;
        const double phi0 = J0 + nu * VE0;
        int tsel = a.ntrial - 1;
        for (int t = 0; t < a.ntrial; ++t) {
            const double al = ldexp(1.0, -t);
            const double Jt = a.costT[(int64_t)b * a.ntrial + t], Vt = a.violT[(int64_t)b * a.ntrial + t];
            if (isfinite(Jt) && isfinite(Vt) && Jt + nu * Vt <= phi0 + 1e-4 * al * D) { tsel = t; break; }
        }
        const double Js = a.costT[(int64_t)b * a.ntrial + tsel];
        if (!isfinite(Js) || !isfinite(a.violT[(int64_t)b * a.ntrial + tsel])) {
            flag = -8;                    // the accepted iterate would not be finite
            fin = true;
        } else {
            const double al = ldexp(1.0, -tsel);
            for (int j = lane; j < n; j += NM_WAVE) z[j] += al * d[j];
            for (int j = 4 + lane; j < 4 * (N + 1); j += NM_WAVE) X[j] += al * dX[j];
            if (lane == 0) { a.cprev[b] = J0; a.nu[b] = nu; }
            ++it;
            if (it >= a.max_iter) {
                flag = 0;
                fin = true;
                if (lane == 0) a.cost0[b] = Js;   // the returned iterate is the stepped one
            }
        }
    }
    if (lane == 0) {
        a.iters[b] = it;
        if (fin) {
            a.flag[b] = flag;
            a.done[b] = 1;
            atomicAdd(a.ndone, 1);
        }
    }
}

// closed loop, after a step's solve and before the warm start of z (both loop modes launch this
// kernel, so both step x_N with the same arithmetic): x_k <- x_{k+1} for k < N,
// x_N <- dynamic(delta, x_N, u_{N-1}) with the move the shift of z repeats.  Stage 0 is the next
// linearisation's, from the measured state.  done / ts null: every instance; else the instances
// that nmpc_loop_advance_kernel moves to their next step in this round
__global__ void __launch_bounds__(64) nmpc_dms_loop_states_kernel(int batch, int N, int steps, double delta,
                                                                  const double* ueq, const double* z,
                                                                  double* X, const int* done, const int* ts) {
    __shared__ double Xs[NMD_XLDS];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= batch) return;
    if (done && !(done[b] != 0 && ts[b] + 1 < steps)) return;   // uniform per wave
    double* Xb = X + (int64_t)b * nmpc_dms_x_stride(N);
    for (int j = lane; j < 4 * (N + 1); j += NM_WAVE) Xs[j] = Xb[j];
    wave_sync();
    for (int j = lane; j < 4 * N; j += NM_WAVE)
        Xb[j] = Xs[nmpc_dms_x_index(nmpc_dms_shift_source(N, j >> 2), j & 3)];
    double x[4], xn[4], AB[4][5];
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = Xs[nmpc_dms_x_index(N, i)];
    nm_rk4<true>(delta, x, z[(int64_t)b * (N + 1) + N - 1] + ueq[0], xn, AB);
    if (lane < 4) {
        double v = xn[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) v = lane == i ? xn[i] : v;
        Xb[nmpc_dms_x_index(N, lane)] = v;
    }
}

// ------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------
static bool nmpc_stage_args_ok(const NmpcArgs& a) {
    return nmpc_supported(a.N, a.mx, a.mu) && a.n == a.N + 1 && a.m == a.N * (a.mx + a.mu) + a.mp &&
           a.n <= NM_WAVE * NM_CPL && a.mx + a.mu <= NM_WAVE && a.batch >= 1 && a.mp >= 0;
}

// the soft arguments of a launch: complete (q given) or all null
static const NmpcSoftArgs nm_hard = {};
static bool nmpc_soft_args_ok(const NmpcSoftArgs* q) {
    return !q || ((q->xs_lin || q->xs_quad) && q->xsl && q->xsq && q->sx && q->pen0 && q->plin);
}
// the set-point of a launch: given with its array, or null
static const NmpcRefArgs nm_noref = {};
static bool nmpc_ref_args_ok(const NmpcRefArgs* r) { return !r || (r->xref && r->sref >= 0); }

hipError_t launch_nmpc_stage_table(const NmpcArgs& a, const NmpcStageArgs& s, hipStream_t st,
                                   const NmpcSoftArgs* q) {
    if (!nmpc_stage_args_ok(a) || !s.W || !s.map || (a.mp > 0 && !s.Fp) || !nmpc_soft_args_ok(q))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmpc_stage_table_kernel, dim3(1), dim3(64), 0, st, a, s, q ? *q : nm_hard);
    return hipGetLastError();
}

hipError_t launch_nmpc_stage_rollout(const NmpcArgs& a, const NmpcStageArgs& s, hipStream_t st,
                                     const NmpcSoftArgs* q, const NmpcRefArgs* r) {
    if (!nmpc_stage_args_ok(a) || !s.A || !s.B || !s.w || !s.xlb || !s.xub || !s.ulb || !s.uub ||
        (a.mp > 0 && !s.hp) || !s.map || !a.rhs || !a.cost0 || !nmpc_soft_args_ok(q) || !nmpc_ref_args_ok(r))
        return hipErrorInvalidValue;
    const dim3 g(a.batch), w(64);
    if (q && r) hipLaunchKernelGGL((nmpc_stage_rollout_kernel<true, true>), g, w, 0, st, a, s, *q, *r);
    else if (r) hipLaunchKernelGGL((nmpc_stage_rollout_kernel<false, true>), g, w, 0, st, a, s, nm_hard, *r);
    else if (q) hipLaunchKernelGGL((nmpc_stage_rollout_kernel<true>), g, w, 0, st, a, s, *q, nm_noref);
    else hipLaunchKernelGGL((nmpc_stage_rollout_kernel<false>), g, w, 0, st, a, s, nm_hard, nm_noref);
    return hipGetLastError();
}

hipError_t launch_nmpc_stage_backmap(const NmpcArgs& a, const NmpcStageArgs& s, hipStream_t st,
                                     const NmpcSoftArgs* q) {
    if (!nmpc_stage_args_ok(a) || !s.uo || !s.tho || !s.lamx || !s.lamu || (a.mp > 0 && !s.lamp) ||
        !s.sflag || !s.map || !a.ctl || !a.f || !a.d || !a.lam || !nmpc_soft_args_ok(q))
        return hipErrorInvalidValue;
    if (q) hipLaunchKernelGGL(nmpc_stage_backmap_kernel<true>, dim3(a.batch), dim3(64), 0, st, a, s, *q);
    else hipLaunchKernelGGL(nmpc_stage_backmap_kernel<false>, dim3(a.batch), dim3(64), 0, st, a, s, nm_hard);
    return hipGetLastError();
}

static bool nmpc_dms_args_ok(const NmpcArgs& a, const NmpcDmsArgs& m) {
    return nmpc_stage_args_ok(a) && 4 * (a.N + 1) <= NMD_XLDS && m.X && a.z && a.x0;
}

hipError_t launch_nmpc_dms_start(const NmpcArgs& a, const NmpcDmsArgs& m, hipStream_t st) {
    if (!nmpc_dms_args_ok(a, m)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmpc_dms_start_kernel, dim3(a.batch), dim3(64), 0, st, a, m);
    return hipGetLastError();
}

hipError_t launch_nmpc_dms_linearize(const NmpcArgs& a, const NmpcStageArgs& s, const NmpcDmsArgs& m,
                                     hipStream_t st, const NmpcRefArgs* r) {
    if (!nmpc_dms_args_ok(a, m) || !m.c || !s.A || !s.B || !s.w || !s.xlb || !s.xub || !s.ulb || !s.uub ||
        (a.mp > 0 && !s.hp) || !s.map || !a.rhs || !a.cost0 || !a.done || !nmpc_ref_args_ok(r))
        return hipErrorInvalidValue;
    if (r) hipLaunchKernelGGL(nmpc_dms_linearize_kernel<true>, dim3(a.batch), dim3(64), 0, st, a, s, m, *r);
    else hipLaunchKernelGGL(nmpc_dms_linearize_kernel<false>, dim3(a.batch), dim3(64), 0, st, a, s, m, nm_noref);
    return hipGetLastError();
}

hipError_t launch_nmpc_dms_backmap(const NmpcArgs& a, const NmpcStageArgs& s, const NmpcDmsArgs& m,
                                   hipStream_t st) {
    if (!nmpc_dms_args_ok(a, m) || !m.dX || !m.pi || !m.sw || !m.gn || !m.pimax || !s.A || !s.B || !s.w ||
        !s.uo || !s.tho || !s.lamx || !s.lamu || (a.mp > 0 && !s.lamp) || !s.sflag || !s.map || !a.d ||
        !a.lam || !a.stat || !a.qpflag)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmpc_dms_backmap_kernel, dim3(a.batch), dim3(64), 0, st, a, s, m);
    return hipGetLastError();
}

hipError_t launch_nmpc_dms_trial(const NmpcArgs& a, const NmpcDmsArgs& m, hipStream_t st, const NmpcRefArgs* r) {
    if (!nmpc_dms_args_ok(a, m) || !m.dX || !a.d || !a.costT || !a.violT || a.ntrial < 1 || !nmpc_ref_args_ok(r))
        return hipErrorInvalidValue;
    const dim3 g(a.batch * a.ntrial), w(64);
    if (r) hipLaunchKernelGGL(nmpc_dms_trial_kernel<true>, g, w, 0, st, a, m, *r);
    else hipLaunchKernelGGL(nmpc_dms_trial_kernel<false>, g, w, 0, st, a, m, nm_noref);
    return hipGetLastError();
}

hipError_t launch_nmpc_dms_update(const NmpcArgs& a, const NmpcDmsArgs& m, hipStream_t st) {
    if (!nmpc_dms_args_ok(a, m) || !m.dX || !m.c || !m.sw || !m.gn || !m.pimax || !a.d || !a.lam || !a.rhs ||
        !a.costT || !a.violT || !a.stat || !a.cprev || !a.nu || !a.iters || !a.flag || !a.ndone)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmpc_dms_update_kernel, dim3(a.batch), dim3(64), 0, st, a, m);
    return hipGetLastError();
}

hipError_t launch_nmpc_dms_loop_states(int batch, int N, int steps, double delta, const double* ueq,
                                       const double* z, double* X, const int* done, const int* ts,
                                       hipStream_t st) {
    if (batch < 1 || N < 1 || N > NMPC_MAXN || 4 * (N + 1) > NMD_XLDS || !ueq || !z || !X || (!done != !ts))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmpc_dms_loop_states_kernel, dim3(batch), dim3(64), 0, st, batch, N, steps, delta, ueq,
                       z, X, done, ts);
    return hipGetLastError();
}

bool nmpc_supported(int N, int mx, int mu) {
    return N >= 1 && N <= NMPC_MAXN && N + 1 <= NM_WAVE * NM_CPL && mx >= 0 && mx <= NMPC_MAXMX &&
           mu >= 0 && mu <= NMPC_MAXMU;
}

hipError_t launch_nmpc_rollout(const NmpcArgs& a, int gn, hipStream_t st, const NmpcSoftArgs* q,
                               const NmpcRefArgs* r) {
    if (!nmpc_supported(a.N, a.mx, a.mu) || a.n != a.N + 1 || a.nr != 5 * a.N + 8 ||
        a.m != a.N * (a.mx + a.mu) + a.mp || (q && (gn || !nmpc_soft_args_ok(q))) || !nmpc_ref_args_ok(r))
        return hipErrorInvalidValue;
    const dim3 g1(a.batch), gt(a.batch * a.ntrial), w(64);
    if (r) {
        if (gn) hipLaunchKernelGGL((nmpc_rollout_kernel<true, false, true>), g1, w, 0, st, a, nm_hard, *r);
        else if (q) hipLaunchKernelGGL((nmpc_rollout_kernel<false, true, true>), gt, w, 0, st, a, *q, *r);
        else hipLaunchKernelGGL((nmpc_rollout_kernel<false, false, true>), gt, w, 0, st, a, nm_hard, *r);
        return hipGetLastError();
    }
    if (gn) hipLaunchKernelGGL((nmpc_rollout_kernel<true>), g1, w, 0, st, a, nm_hard, nm_noref);
    else if (q) hipLaunchKernelGGL((nmpc_rollout_kernel<false, true>), gt, w, 0, st, a, *q, nm_noref);
    else hipLaunchKernelGGL((nmpc_rollout_kernel<false>), gt, w, 0, st, a, nm_hard, nm_noref);
    return hipGetLastError();
}

hipError_t launch_nmpc_update(const NmpcArgs& a, hipStream_t st, const NmpcSoftArgs* q) {
    if (a.n > NM_WAVE * NM_CPL || (q && (a.C || !nmpc_soft_args_ok(q)))) return hipErrorInvalidValue;
    if (a.C) hipLaunchKernelGGL((nmpc_update_kernel<false>), dim3(a.batch), dim3(64), 0, st, a, nm_hard);
    else if (a.ctl && q) hipLaunchKernelGGL((nmpc_update_kernel<true, true>), dim3(a.batch), dim3(64), 0, st, a, *q);
    else if (a.ctl) hipLaunchKernelGGL((nmpc_update_kernel<true>), dim3(a.batch), dim3(64), 0, st, a, nm_hard);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_nmpc_loop_shift(int batch, int N, int steps, int t, double* z, const int* it,
                                  int* itlog, hipStream_t st) {
    if (N < 1 || N > NMPC_MAXN) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmpc_loop_shift_kernel, dim3(batch), dim3(64), 0, st, batch, N, steps, t, z, it, itlog);
    return hipGetLastError();
}

static const NmpcTrackArgs nm_notrack = {};
static const PlantPar nm_nominal = {};
// a schedule comes with the slot array it is copied into
static bool nmpc_track_args_ok(const NmpcTrackArgs& k) {
    return k.sref >= 0 && k.sdist >= 0 && (!k.ref) == (!k.xr);
}

hipError_t launch_nmpc_loop_advance(const NmpcAdvanceArgs& a, hipStream_t st, const NmpcTrackArgs* k,
                                    const PlantPar* pp) {
    // the shift stages N <= 128 doubles in LDS
    if (a.batch < 1 || a.N < 1 || a.N > NMPC_MAXN || a.N > NM_WAVE * NM_CPL || a.steps < 1 ||
        (k && !nmpc_track_args_ok(*k)) || (pp && !plant_par_args_ok(*pp)))
        return hipErrorInvalidValue;
    const dim3 grid(a.batch), block(64);
    if (pp) {
        if (k) hipLaunchKernelGGL((nmpc_loop_advance_kernel<true, true>), grid, block, 0, st, a, *k, *pp);
        else hipLaunchKernelGGL((nmpc_loop_advance_kernel<false, true>), grid, block, 0, st, a, nm_notrack, *pp);
    } else {
        if (k) hipLaunchKernelGGL((nmpc_loop_advance_kernel<true, false>), grid, block, 0, st, a, *k, nm_nominal);
        else hipLaunchKernelGGL((nmpc_loop_advance_kernel<false, false>), grid, block, 0, st, a, nm_notrack, nm_nominal);
    }
    return hipGetLastError();
}

hipError_t launch_nmpc_track_init(int batch, const NmpcTrackArgs& k, hipStream_t st) {
    if (batch < 1 || !k.ref || !k.xr || k.sref < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(nmpc_track_init_kernel, dim3((4 * batch + 255) / 256), dim3(256), 0, st, batch, k);
    return hipGetLastError();
}

hipError_t launch_nmpc_track_plant(const NmpcAdvanceArgs& a, const NmpcTrackArgs& k, int t, hipStream_t st,
                                   const PlantPar* pp) {
    // the step-synchronous loop points the solves at the schedule itself: no slot array
    if (a.batch < 1 || a.N < 1 || a.N > NMPC_MAXN || t < 0 || t >= a.steps || k.sdist < 0 || !a.z || !a.s ||
        !a.X || !a.U || !a.flag || (pp && !plant_par_args_ok(*pp)))
        return hipErrorInvalidValue;
    const dim3 grid((a.batch + 255) / 256), block(256);
    if (pp) hipLaunchKernelGGL(nmpc_track_plant_kernel<true>, grid, block, 0, st, a, k, t, *pp);
    else hipLaunchKernelGGL(nmpc_track_plant_kernel<false>, grid, block, 0, st, a, k, t, nm_nominal);
    return hipGetLastError();
}

}  // namespace bqp
