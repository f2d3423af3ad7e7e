// bqp_track.h — the per-instance step of the closed loop with a reference schedule
// (bqp_closed_loop_track): where X, U, THETA, ref, dist and w lie with their strides, the record
// of a step's solve, the linear plant, and one entry of the next step's linear term.
//
// Plain C++ that compiles for the host and the device: track_advance_kernel (bqp_plant.hip)
// calls these functions with one thread per instance / per entry, tests/host/track_step_check.cpp
// calls them from loops under the host sanitizers.  No HIP header, no LDS, plain stores.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BQP_HD __host__ __device__
#else
#define BQP_HD
#endif

namespace bqp {

// Device pointers (host pointers in the host check).  Matrices are column-major.
struct TrackArgs {
    int batch, nx, nu, np, N, steps, nr;
    int plant;                // BQP_PLANT_*
    double delta;             // MG plants: sampling period
    int64_t nw;               // (N + 1) * nv, the doubles of one instance's linear term
    // the step's solve, in the loop's workspace (bqp_layout.h CworkTrack)
    const double* uo;         // batch x N x nu (deviation from u_eq)
    const double* th;         // batch x np
    const int* fl;            // batch
    const double *xeq, *ueq;  // working point: nx, nu
    // linear plant: x+ = x_eq + A (x - x_eq) + B (u - u_eq) + d_t
    const double* A; int64_t sA;        // nx x nx
    const double* B; int64_t sB;        // nx x nu
    const double* dist; int64_t sdist;  // steps x nx per instance, null = 0
    // linear term of step t: w_t = wbase + Wr r_t
    const double* wbase; int64_t swbase;  // nw per instance, null = 0
    const double* Wr;                     // nw x nr, shared
    const double* ref; int64_t sref;      // steps x nr per instance
    double* s;        // batch x nx, the measured state in deviation from x_eq (the solve's x0)
    double* w;        // batch x nw (the solve reads it with stride nw)
    double* X;        // batch x (steps + 1) x nx, absolute
    double* U;        // batch x steps x nu, absolute
    double* THETA;    // batch x steps x np, may be null
    int* flags;       // batch x steps, may be null
};

BQP_HD inline int64_t track_x_at(const TrackArgs& a, int b, int t) { return ((int64_t)b * (a.steps + 1) + t) * a.nx; }
BQP_HD inline int64_t track_u_at(const TrackArgs& a, int b, int t) { return ((int64_t)b * a.steps + t) * a.nu; }
BQP_HD inline int64_t track_theta_at(const TrackArgs& a, int b, int t) { return ((int64_t)b * a.steps + t) * a.np; }
BQP_HD inline int64_t track_flag_at(const TrackArgs& a, int b, int t) { return (int64_t)b * a.steps + t; }
BQP_HD inline int64_t track_ref_at(const TrackArgs& a, int b, int t) { return (int64_t)b * a.sref + (int64_t)t * a.nr; }
BQP_HD inline int64_t track_dist_at(const TrackArgs& a, int b, int t) { return (int64_t)b * a.sdist + (int64_t)t * a.nx; }

// the step-t solve of instance b into the logs: U = u_eq + u_0, theta, exit flag
BQP_HD inline void track_record(const TrackArgs& a, int b, int t) {
    const double* u0 = a.uo + (int64_t)b * a.N * a.nu;
    double* U = a.U + track_u_at(a, b, t);
    for (int k = 0; k < a.nu; ++k) U[k] = u0[k] + a.ueq[k];
    if (a.THETA) {
        double* T = a.THETA + track_theta_at(a, b, t);
        for (int j = 0; j < a.np; ++j) T[j] = a.th[(int64_t)b * a.np + j];
    }
    if (a.flags) a.flags[track_flag_at(a, b, t)] = a.fl[b];
}

// linear plant step t of instance b with the solve's first move: X[b, t + 1], then the measured
// deviation state s = X[b, t + 1] - x_eq (as the MG plant kernels form it)
BQP_HD inline void track_linear_step(const TrackArgs& a, int b, int t) {
    const int nx = a.nx, nu = a.nu;
    const double* Ab = a.A + (int64_t)b * a.sA;
    const double* Bb = a.B + (int64_t)b * a.sB;
    const double* u0 = a.uo + (int64_t)b * a.N * nu;
    const double* d = a.dist ? a.dist + track_dist_at(a, b, t) : nullptr;
    double* sb = a.s + (int64_t)b * nx;
    double* xn = a.X + track_x_at(a, b, t + 1);
    for (int i = 0; i < nx; ++i) {
        double v = d ? d[i] : 0.0;
        for (int j = 0; j < nx; ++j) v += Ab[j * nx + i] * sb[j];
        for (int k = 0; k < nu; ++k) v += Bb[k * nx + i] * u0[k];
        xn[i] = v + a.xeq[i];
    }
    for (int i = 0; i < nx; ++i) sb[i] = xn[i] - a.xeq[i];
}

// entry i = b * nw + e of the step-t linear terms: w[b, e] = wbase[b, e] + sum_j Wr[e, j] r_t[j]
BQP_HD inline void track_w_entry(const TrackArgs& a, int64_t i, int t) {
    const int b = (int)(i / a.nw);
    const int64_t e = i - (int64_t)b * a.nw;
    const double* r = a.ref + track_ref_at(a, b, t);
    double v = a.wbase ? a.wbase[(int64_t)b * a.swbase + e] : 0.0;
    for (int j = 0; j < a.nr; ++j) v += a.Wr[(int64_t)j * a.nw + e] * r[j];
    a.w[i] = v;
}

}  // namespace bqp
