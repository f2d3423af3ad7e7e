// bqp_mg.h — the Moore-Greitzer compressor of the reference's closed loops and its integrators
// over one sampling period, shared by the kernels that step the true plant (bqp_plant.hip:
// mg_plant_kernel, track_advance_kernel, sqp_loop_advance_kernel; bqp_nmpc.hip:
// nmpc_loop_advance_kernel, nmpc_track_plant_kernel), so that every loop steps the plant with the same arithmetic
// (mg_plant_step below).  Device code only.
//
// `system` of examples/DMS_tracking_LMPC_casadi.m:215-221 (the same model as
// models/trueModel.m:32-41); `dynamic` (:297-304), one classical RK4 step; MATLAB's ode23.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/bqp.h"

namespace bqp {

__device__ __forceinline__ void mg_system(const double (&x)[4], double u, double (&f)[4]) {
    f[0] = -x[1] + 1.0 + 3.0 * (x[0] / 2.0) - (x[0] * x[0] * x[0] / 2.0);   // mass flow rate
    f[1] = (x[0] + 1.0 - x[2] * sqrt(x[1]));                              // pressure rise rate
    f[2] = x[3];                                                          // throttle opening rate
    f[3] = -1000.0 * x[2] - 2.0 * sqrt(500.0) * x[3] + 1000.0 * u;        // throttle acceleration
}

__device__ __forceinline__ void mg_rk4(double delta, double (&x)[4], double u) {
    double k1[4], k2[4], k3[4], k4[4], y[4];
    mg_system(x, u, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = x[i] + delta / 2.0 * k1[i];
    mg_system(y, u, k2);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = x[i] + delta / 2.0 * k2[i];
    mg_system(y, u, k3);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = x[i] + delta * k3[i];
    mg_system(y, u, k4);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = x[i] + delta / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
}

// MATLAB ode23 over [0, T] from y with the input held: the Bogacki-Shampine 3(2) pair with
// first-same-as-last, local extrapolation and the step-size control of the MATLAB ODE suite
// (Shampine & Reichelt 1997) at the defaults RelTol 1e-3, AbsTol 1e-6 (threshold AbsTol/RelTol),
// MaxStep 0.1 T; initial step min(MaxStep, T) capped by 0.8 RelTol^(1/3) / |f0 / max(|y|, thr)|;
// a step within 10 % of the end is stretched to it.  Error estimate
// err = h |f E ./ max(|y|, |ynew|, thr)|_inf with E = [-5/72 1/12 1/9 -1/8]; a failed step
// shrinks h by max(0.5, 0.8 (RelTol/err)^(1/3)) the first time, by 0.5 after; a step without
// failure grows h by 1 / (1.25 (err/RelTol)^(1/3)), at most 5x.  The restatement
// (oracle/mg_model.py mg_ode23) reproduces every stored transition x_k -> x_{k+1} of the
// reference's fmincon runs (LMPC_N20/40/50, LBMPC_N40/50_sys_full.mat) to 1.4e-15.
__device__ __forceinline__ void mg_ode23(double T, double (&y)[4], double u) {
    constexpr double rtol = 1e-3, thr = 1e-6 / 1e-3;
    constexpr double E0 = -5.0 / 72.0, E1 = 1.0 / 12.0, E2 = 1.0 / 9.0, E3 = -1.0 / 8.0;
    const double pw = 1.0 / 3.0, hmax = 0.1 * T;
    double F0[4], F1[4], F2[4], F3[4], ys[4], yn[4];
    mg_system(y, u, F0);
    double absh = fmin(hmax, T), rh = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) rh = fmax(rh, fabs(F0[i] / fmax(fabs(y[i]), thr)));
    rh /= 0.8 * pow(rtol, pw);
    if (absh * rh > 1.0) absh = 1.0 / rh;
    double t = 0.0;
    bool done = false;
    // at most 4096 step attempts (the MG plant takes 10-14 per 0.01 s sampling period)
    for (int guard = 0; !done && guard < 4096; ++guard) {
        const double hmin = 16.0 * (nextafter(t, INFINITY) - t);
        absh = fmin(hmax, fmax(hmin, absh));
        double h = absh;
        if (1.1 * absh >= fabs(T - t)) {
            h = T - t;
            absh = fabs(h);
            done = true;
        }
        bool nofailed = true;
        double err = 0.0;
        for (;; ++guard) {
            const double h1 = h * 0.5, h2 = h * 0.75;
#pragma unroll
            for (int i = 0; i < 4; ++i) ys[i] = y[i] + F0[i] * h1;
            mg_system(ys, u, F1);
#pragma unroll
            for (int i = 0; i < 4; ++i) ys[i] = y[i] + F1[i] * h2;
            mg_system(ys, u, F2);
            const double tnew = done ? T : t + h;
            h = tnew - t;
            const double b0 = h * (2.0 / 9.0), b1 = h * (1.0 / 3.0), b2 = h * (4.0 / 9.0);
#pragma unroll
            for (int i = 0; i < 4; ++i) yn[i] = y[i] + (F0[i] * b0 + F1[i] * b1 + F2[i] * b2);
            mg_system(yn, u, F3);
            double e = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double fe = F0[i] * E0 + F1[i] * E1 + F2[i] * E2 + F3[i] * E3;
                e = fmax(e, fabs(fe / fmax(fmax(fabs(y[i]), fabs(yn[i])), thr)));
            }
            err = absh * e;
            if (!(err > rtol)) {
                t = tnew;
                break;
            }
            if (absh <= hmin || guard >= 4096) {   // MATLAB warns and returns here
                done = true;
                t = tnew;
                break;
            }
            absh = nofailed ? fmax(hmin, absh * fmax(0.5, 0.8 * pow(rtol / err, pw)))
                            : fmax(hmin, 0.5 * absh);
            nofailed = false;
            h = absh;
            done = false;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[i] = yn[i];
            F0[i] = F3[i];
        }
        if (!done && nofailed) {
            const double temp = 1.25 * pow(err / rtol, pw);
            absh = temp > 0.2 ? absh / temp : 5.0 * absh;
        }
    }
}

// One sampling period of the plant `plant` (BQP_PLANT_MG_RK4 / BQP_PLANT_MG_ODE23).  Every kernel
// that steps the plant calls this, and none calls mg_rk4 or mg_ode23 itself: which multiply-adds
// the compiler contracts in mg_rk4 depends on the code it is inlined into (the first evaluation of
// `system` is shared with mg_ode23's), so only kernels that inline the same dispatch step the
// plant to the same bits - what the asynchronous loops' bitwise tests against the
// step-synchronous ones rely on.
__device__ __forceinline__ void mg_plant_step(int plant, double delta, double (&x)[4], double u) {
    if (plant == BQP_PLANT_MG_ODE23) mg_ode23(delta, x, u);
    else mg_rk4(delta, x, u);
}

// ------------------------------------------------------------------------------------------
// The plant with per-instance coefficients (bqp_closed_loop.plant_par; models/trueModel.m:32-41
// names them): p = [x2_c, 1/beta^2, wn^2, 2 zeta wn], in registers (the caller loads them once,
// bqp_plant_par.h plant_par_load, before the integrator).  The nominal plant is
// p = [0, 1, 1000, 2 sqrt(500)].  Overloads with p in front; the functions above stay as they are,
// for the reason mg_plant_step gives: a call without parameters steps the plant to the bits it
// always did.  The integrators are the ones above, statement for statement, on this `system`.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void mg_system(const double (&p)[4], const double (&x)[4], double u, double (&f)[4]) {
    f[0] = -x[1] + p[0] + 1.0 + 3.0 * (x[0] / 2.0) - (x[0] * x[0] * x[0] / 2.0);
    f[1] = (x[0] + 1.0 - x[2] * sqrt(x[1])) * p[1];
    f[2] = x[3];
    f[3] = -p[2] * x[2] - p[3] * x[3] + p[2] * u;
}

__device__ __forceinline__ void mg_rk4(const double (&p)[4], double delta, double (&x)[4], double u) {
    double k1[4], k2[4], k3[4], k4[4], y[4];
    mg_system(p, x, u, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = x[i] + delta / 2.0 * k1[i];
    mg_system(p, y, u, k2);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = x[i] + delta / 2.0 * k2[i];
    mg_system(p, y, u, k3);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = x[i] + delta * k3[i];
    mg_system(p, y, u, k4);
#pragma unroll
    for (int i = 0; i < 4; ++i) x[i] = x[i] + delta / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]);
}

__device__ __forceinline__ void mg_ode23(const double (&p)[4], double T, double (&y)[4], double u) {
    constexpr double rtol = 1e-3, thr = 1e-6 / 1e-3;
    constexpr double E0 = -5.0 / 72.0, E1 = 1.0 / 12.0, E2 = 1.0 / 9.0, E3 = -1.0 / 8.0;
    const double pw = 1.0 / 3.0, hmax = 0.1 * T;
    double F0[4], F1[4], F2[4], F3[4], ys[4], yn[4];
    mg_system(p, y, u, F0);
    double absh = fmin(hmax, T), rh = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) rh = fmax(rh, fabs(F0[i] / fmax(fabs(y[i]), thr)));
    rh /= 0.8 * pow(rtol, pw);
    if (absh * rh > 1.0) absh = 1.0 / rh;
    double t = 0.0;
    bool done = false;
    for (int guard = 0; !done && guard < 4096; ++guard) {
        const double hmin = 16.0 * (nextafter(t, INFINITY) - t);
        absh = fmin(hmax, fmax(hmin, absh));
        double h = absh;
        if (1.1 * absh >= fabs(T - t)) {
            h = T - t;
            absh = fabs(h);
            done = true;
        }
        bool nofailed = true;
        double err = 0.0;
        for (;; ++guard) {
            const double h1 = h * 0.5, h2 = h * 0.75;
#pragma unroll
            for (int i = 0; i < 4; ++i) ys[i] = y[i] + F0[i] * h1;
            mg_system(p, ys, u, F1);
#pragma unroll
            for (int i = 0; i < 4; ++i) ys[i] = y[i] + F1[i] * h2;
            mg_system(p, ys, u, F2);
            const double tnew = done ? T : t + h;
            h = tnew - t;
            const double b0 = h * (2.0 / 9.0), b1 = h * (1.0 / 3.0), b2 = h * (4.0 / 9.0);
#pragma unroll
            for (int i = 0; i < 4; ++i) yn[i] = y[i] + (F0[i] * b0 + F1[i] * b1 + F2[i] * b2);
            mg_system(p, yn, u, F3);
            double e = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double fe = F0[i] * E0 + F1[i] * E1 + F2[i] * E2 + F3[i] * E3;
                e = fmax(e, fabs(fe / fmax(fmax(fabs(y[i]), fabs(yn[i])), thr)));
            }
            err = absh * e;
            if (!(err > rtol)) {
                t = tnew;
                break;
            }
            if (absh <= hmin || guard >= 4096) {
                done = true;
                t = tnew;
                break;
            }
            absh = nofailed ? fmax(hmin, absh * fmax(0.5, 0.8 * pow(rtol / err, pw)))
                            : fmax(hmin, 0.5 * absh);
            nofailed = false;
            h = absh;
            done = false;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            y[i] = yn[i];
            F0[i] = F3[i];
        }
        if (!done && nofailed) {
            const double temp = 1.25 * pow(err / rtol, pw);
            absh = temp > 0.2 ? absh / temp : 5.0 * absh;
        }
    }
}

// One sampling period of the parametrised plant.  Every kernel that steps it calls this one, as the
// nominal kernels call the one above, so the asynchronous and the step-synchronous nonlinear MPC
// loops stay bitwise equal with parameters too.
__device__ __forceinline__ void mg_plant_step(const double (&p)[4], int plant, double delta, double (&x)[4], double u) {
    if (plant == BQP_PLANT_MG_ODE23) mg_ode23(p, delta, x, u);
    else mg_rk4(p, delta, x, u);
}

}  // namespace bqp
