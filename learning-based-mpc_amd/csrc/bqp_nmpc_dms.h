// bqp_nmpc_dms.h — the index arithmetic of the nonlinear MPC's direct multiple shooting
// (bqp_nmpc_dims.shooting = 1): which stage a lane owns in which pass of a wave over the N + 1
// stages, and where a stage's entries of the iterate X, the defects c, the dynamics multipliers pi
// and the stage records A, B, w lie in an instance's arrays.
//
// Plain C++ that compiles for the host and the device: the nmpc_dms_* kernels of bqp_nmpc.hip call
// these functions, tests/host/nmpc_dms_check.cpp calls them on exactly sized heap buffers under the
// host sanitizers.  No HIP header.
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

constexpr int NMD_WAVE = 64;       // lanes of a wave
constexpr int NMD_MAXN = 127;      // = NMPC_MAXN (bqp_internal.h): N + 1 <= 2 passes of a wave
constexpr int NMD_XLDS = 4 * (NMD_MAXN + 1);   // doubles of X in LDS: N + 1 <= 128 stages x 4

// one wave per instance, lanes over the stages 0..N: passes of 64 stages
BQP_HD inline int nmpc_dms_passes(int N) { return (N + 1 + NMD_WAVE - 1) / NMD_WAVE; }
// the stage of a lane in a pass, or -1 where the lane has none (past N)
BQP_HD inline int nmpc_dms_stage(int N, int lane, int pass) {
    const int k = lane + NMD_WAVE * pass;
    return k <= N ? k : -1;
}
// stage k has a step to stage k + 1 (f_k, A_k, B_k, c_k, pi_k, u_k), and rows on its state
BQP_HD inline bool nmpc_dms_has_step(int N, int k) { return k >= 0 && k < N; }
BQP_HD inline bool nmpc_dms_has_state_rows(int N, int k) { return k >= 1 && k <= N; }

// per instance: X (N + 1) x 4, c and pi N x 4 (entry k: the step from stage k to k + 1),
// A N x 16 column-major, B N x 4, w (N + 1) x 6 [x (4); u; theta]
BQP_HD inline int nmpc_dms_x_index(int k, int i) { return 4 * k + i; }
BQP_HD inline int nmpc_dms_c_index(int k, int i) { return 4 * k + i; }
BQP_HD inline int nmpc_dms_pi_index(int k, int i) { return 4 * k + i; }
BQP_HD inline int nmpc_dms_a_index(int k, int i, int j) { return 16 * k + i + 4 * j; }
BQP_HD inline int nmpc_dms_b_index(int k, int i) { return 4 * k + i; }
BQP_HD inline int nmpc_dms_w_index(int k, int e) { return 6 * k + e; }
BQP_HD inline int64_t nmpc_dms_x_stride(int N) { return 4 * (int64_t)(N + 1); }
BQP_HD inline int64_t nmpc_dms_c_stride(int N) { return 4 * (int64_t)N; }

// the closed loop's warm start of the states: stage k takes stage k + 1 (k < N); stage N is
// stepped from the old x_N with the repeated last move, stage 0 is the new measured state
BQP_HD inline int nmpc_dms_shift_source(int N, int k) { return k < N ? k + 1 : N; }

}  // namespace bqp
