// bqp_nmpc_advance.h — the index arithmetic of one instance's advance in the asynchronous
// nonlinear MPC loop (bqp_closed_loop_nmpc): when an instance is due, where its step's logs and
// its plant step go, the warm-start shift, the reset of the per-solve state and the step counter's
// transition.
//
// Plain C++ that compiles for the host and the device: nmpc_loop_advance_kernel (bqp_nmpc.hip)
// calls these functions with one wave per instance (the shift lanes over j, the rest lane 0),
// tests/host/nmpc_advance_check.cpp calls them from loops under the host sanitizers.  No HIP
// header, no LDS (the shift's staging array is the caller's), plain stores; the one atomic, the
// count of finished instances, is a plain increment on the host.
#pragma once
#include <stdint.h>

#ifndef BQP_HD
#if defined(__HIPCC__)
#define BQP_HD __host__ __device__
#else
#define BQP_HD
#endif
#endif

namespace bqp {

// Device pointers (host pointers in the host check); the per-instance arrays of the loop's
// workspace (bqp_layout.h CworkNmpc) and of the SQP's (Nwork)
struct NmpcAdvanceArgs {
    int batch, N, steps;      // n = N + 1 variables per instance: N moves, then theta
    int plant;                // BQP_PLANT_* (the loop admits BQP_PLANT_MG_RK4)
    double delta;             // the plant's sampling period
    const double *xeq, *ueq;  // working point: 4, 1
    double* s;                // batch x 4, measured state in deviation from x_eq
    double* z;                // batch x n, SQP iterate: the step's solution, then the warm start
    double* x0;               // batch x 4, measured state, absolute: the next solve's x0
    double* X;                // batch x (steps + 1) x 4, absolute
    double* U;                // batch x steps, absolute
    double* nu;               // batch, the merit function's penalty (kept within a solve)
    int *done, *iters, *flag; // batch each: the SQP's per-solve state
    int* ts;                  // batch: the closed-loop step the instance is at; steps = finished
    int* nfin;                // 1: finished instances
    int* flags;               // batch x steps, may be null
    int* itlog;               // batch x steps, may be null
};

// an instance advances in the round in which its SQP has stopped, while it has steps to go
BQP_HD inline bool nmpc_advance_due(const NmpcAdvanceArgs& a, int b) {
    return a.done[b] != 0 && a.ts[b] < a.steps;
}

// the step-t solve of instance b into the logs
BQP_HD inline void nmpc_advance_log(const NmpcAdvanceArgs& a, int b, int t) {
    if (a.flags) a.flags[(int64_t)b * a.steps + t] = a.flag[b];
    if (a.itlog) a.itlog[(int64_t)b * a.steps + t] = a.iters[b];
}

// the plant's step t of instance b: x = X[b, t + 1] (absolute), u = U[b, t]; the measured state
// of the next solve in deviation (s, as the plant kernel forms it) and absolute (x0, the bits of
// X[b, t + 1])
BQP_HD inline void nmpc_advance_record(const NmpcAdvanceArgs& a, int b, int t, const double (&x)[4], double u) {
    double* Xn = a.X + ((int64_t)b * (a.steps + 1) + t + 1) * 4;
    for (int i = 0; i < 4; ++i) {
        a.s[(int64_t)b * 4 + i] = x[i] - a.xeq[i];
        Xn[i] = x[i];
        a.x0[(int64_t)b * 4 + i] = x[i];
    }
    a.U[(int64_t)b * a.steps + t] = u;
}

// warm start: z[j] <- z[min(j + 1, N - 1)] for j < N (one stage on, the last move repeated),
// theta = z[N] kept.  Two passes over j through a staging array of N doubles, so that every read
// precedes every write
BQP_HD inline int nmpc_shift_src(int N, int j) { return j + 1 < N ? j + 1 : N - 1; }
BQP_HD inline void nmpc_shift_stage(const double* zb, int N, int j, double* stage) { stage[j] = zb[nmpc_shift_src(N, j)]; }
BQP_HD inline void nmpc_shift_store(double* zb, int j, const double* stage) { zb[j] = stage[j]; }

// after step t of instance b: with steps to go the per-solve state as the solve's entry sets it
// (iterations, exit flag, penalty, done) and the step counter; at the last step the instance
// stays done and is counted once (nmpc_advance_due is false from then on)
BQP_HD inline void nmpc_advance_next(const NmpcAdvanceArgs& a, int b, int t) {
    if (t + 1 < a.steps) {
        a.iters[b] = 0;
        a.flag[b] = 0;
        a.nu[b] = 0.0;
        a.ts[b] = t + 1;
        a.done[b] = 0;
    } else {
        a.ts[b] = a.steps;
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(a.nfin, 1);
#else
        ++*a.nfin;
#endif
    }
}

// ------------------------------------------------------------------------------------------
// set-point schedule and disturbed plant (bqp_closed_loop_nmpc_track): what the advance does in
// addition for a due instance.  A separate, trailing kernel argument of the advance and of the
// step-synchronous loop's plant launch, so that NmpcAdvanceArgs keeps its layout.
// ------------------------------------------------------------------------------------------
struct NmpcTrackArgs {
    const double* ref;    // set-point schedule, absolute: steps x 4 per instance; may be null
    int64_t sref;         // doubles between two instances' schedules; 0: one schedule for the batch
    const double* dist;   // additive state disturbance: steps x 4 per instance; may be null (zero)
    int64_t sdist;        // as sref
    double* THETA;        // batch x steps, theta of every step's solution; may be null
    double* xr;           // batch x 4: the set-point of the step each instance is at (the solves'
                          // x_ref); null without a schedule
};

// entry i of step t of instance b in a schedule of stride `stride` (0: shared by the batch)
BQP_HD inline int64_t nmpc_track_at(int64_t stride, int b, int t, int i) {
    return (int64_t)b * stride + (int64_t)t * 4 + i;
}

// the next set-point is read only while steps remain: ref[b, steps] does not exist
BQP_HD inline bool nmpc_track_has_next(int steps, int t) { return t + 1 < steps; }

BQP_HD inline int64_t nmpc_track_theta_at(int steps, int b, int t) { return (int64_t)b * steps + t; }

// theta of the step-t solution of instance b into the log (z: the instance's N + 1 variables,
// before the shift, which keeps theta anyway)
BQP_HD inline void nmpc_track_log(const NmpcTrackArgs& k, int steps, int N, int b, int t, const double* zb) {
    if (k.THETA) k.THETA[nmpc_track_theta_at(steps, b, t)] = zb[N];
}

// the plant's state after step t, disturbed: one addition per entry, rounded once - the value the
// log stores and the next solve measures
BQP_HD inline void nmpc_track_disturb(const NmpcTrackArgs& k, int b, int t, double (&x)[4]) {
    if (!k.dist) return;
    for (int i = 0; i < 4; ++i) x[i] = x[i] + k.dist[nmpc_track_at(k.sdist, b, t, i)];
}

// the set-point of step t + 1 into the instance's current-reference slot, while steps remain
BQP_HD inline void nmpc_track_next_ref(const NmpcTrackArgs& k, int steps, int b, int t) {
    if (!k.ref || !k.xr || !nmpc_track_has_next(steps, t)) return;
    for (int i = 0; i < 4; ++i) k.xr[(int64_t)b * 4 + i] = k.ref[nmpc_track_at(k.sref, b, t + 1, i)];
}

}  // namespace bqp
