// Stand-alone check of the nonlinear MPC multiple shooting's host/device index arithmetic
// (csrc/bqp_nmpc_dms.h) and of its share of the workspaces (csrc/bqp_layout.h: NworkStage and
// CworkNmpc with dms = 1): the Makefile builds it with g++ -std=c++17 -fsanitize=address,undefined
// (build/nmpc_dms_check), tests/test_host_nmpc_dms.py runs it.
//
//   - the stage-of-lane map at N = 1, 63, 64, 65, 127: over the passes of a wave every stage 0..N
//     is owned exactly once, no lane owns a stage past N;
//   - the stores of the linearisation (A, B, c, w per stage), the reads of the back-map (pi_{k-1},
//     pi_k, A_k, dX) and the loop's shift of the states, done as the kernels do them on heap
//     buffers of exactly the documented sizes: every element written exactly once;
//   - dms = 0 leaves NworkStage and CworkNmpc byte for byte as they were; dms = 1 adds regions of
//     the documented sizes, aligned, disjoint and inside `bytes`.
#include <stdio.h>

#include <vector>

#include "bqp_layout.h"
#include "bqp_nmpc_dms.h"
#include "bqp_nmpc_stage.h"

using namespace bqp;
using namespace bqp::layout;

static int failures = 0;
static long checks = 0;

#define EXPECT(cond)                                                          \
    do {                                                                      \
        ++checks;                                                             \
        if (!(cond)) {                                                        \
            ++failures;                                                       \
            fprintf(stderr, "%s:%d: %s fails\n", __FILE__, __LINE__, #cond);  \
        }                                                                     \
    } while (0)

static void check_stages(int N) {
    const int np = nmpc_dms_passes(N);
    EXPECT(np >= 1 && np <= 2);
    EXPECT(4 * (N + 1) <= NMD_XLDS);
    std::vector<int> owned(N + 1, 0);
    // exactly sized heap buffers, as the kernels address them
    std::vector<double> X(4 * (size_t)(N + 1), 1.0), c(4 * (size_t)N, 0.0), pi(4 * (size_t)N, 2.0),
        A(16 * (size_t)N, 0.0), B(4 * (size_t)N, 0.0), w(6 * (size_t)(N + 1), 0.0);
    EXPECT((int64_t)X.size() == nmpc_dms_x_stride(N) && (int64_t)c.size() == nmpc_dms_c_stride(N));
    double acc = 0.0;
    for (int ps = 0; ps < np; ++ps)
        for (int lane = 0; lane < NMD_WAVE; ++lane) {
            const int k = nmpc_dms_stage(N, lane, ps);
            if (k < 0) continue;
            EXPECT(k <= N);
            ++owned[k];
            // linearisation
            if (nmpc_dms_has_step(N, k)) {
                for (int j = 0; j < 4; ++j)
                    for (int i = 0; i < 4; ++i) A[nmpc_dms_a_index(k, i, j)] += 1.0;
                for (int i = 0; i < 4; ++i) {
                    B[nmpc_dms_b_index(k, i)] += 1.0;
                    c[nmpc_dms_c_index(k, i)] += X[nmpc_dms_x_index(k, i)] - X[nmpc_dms_x_index(k + 1, i)] + 1.0;
                }
            }
            for (int e = 0; e < 6; ++e) w[nmpc_dms_w_index(k, e)] += 1.0;
            // back-map
            if (nmpc_dms_has_step(N, k))
                for (int i = 0; i < 4; ++i) acc += pi[nmpc_dms_pi_index(k, i)] * B[nmpc_dms_b_index(k, i)];
            if (nmpc_dms_has_state_rows(N, k))
                for (int j = 0; j < 4; ++j) {
                    acc += pi[nmpc_dms_pi_index(k - 1, j)] + X[nmpc_dms_x_index(k, j)];
                    if (k < N)
                        for (int i = 0; i < 4; ++i) acc += A[nmpc_dms_a_index(k, i, j)] * pi[nmpc_dms_pi_index(k, i)];
                }
        }
    for (int k = 0; k <= N; ++k) EXPECT(owned[k] == 1);
    for (double v : A) EXPECT(v == 1.0);
    for (double v : B) EXPECT(v == 1.0);
    for (double v : c) EXPECT(v == 1.0);
    for (double v : w) EXPECT(v == 1.0);
    EXPECT(acc == acc);
    EXPECT(!nmpc_dms_has_step(N, N) && nmpc_dms_has_step(N, 0) && !nmpc_dms_has_state_rows(N, 0) &&
           nmpc_dms_has_state_rows(N, N));
    // the loop's shift of the states: stage k < N takes stage k + 1 through a staging copy
    for (int k = 0; k <= N; ++k)
        for (int i = 0; i < 4; ++i) X[nmpc_dms_x_index(k, i)] = 10.0 * k + i;
    const std::vector<double> Xs = X;
    for (int j = 0; j < 4 * N; ++j) X[j] = Xs[nmpc_dms_x_index(nmpc_dms_shift_source(N, j >> 2), j & 3)];
    for (int k = 0; k < N; ++k)
        for (int i = 0; i < 4; ++i) EXPECT(X[nmpc_dms_x_index(k, i)] == 10.0 * (k + 1) + i);
    EXPECT(nmpc_dms_shift_source(N, N) == N);
}

static void check_layouts(size_t Bt, size_t N, size_t mp) {
    const size_t n = N + 1, m = 10 * N + mp, MB = sizeof(NmpcBoundMap), D = sizeof(double);
    const NworkStage L0(Bt, N, mp, m, 8, MB), L1(Bt, N, mp, m, 8, MB, 0, 1);
    EXPECT(L0.Xw.bytes == 0 && L0.cdef.bytes == 0 && L0.piw.bytes == 0 && L0.pimax.bytes == 0);
    // dms = 0: what it was before the members existed (every region the same, here the ends)
    EXPECT(L0.A.off == L1.A.off && L0.nu.off == L1.nu.off && L0.plin.off == L1.plin.off);
    EXPECT(L1.bytes == L0.bytes + (Bt * n * 4 + 2 * Bt * N * 4 + 3 * Bt) * D);
    const Region rs[] = {L1.Xw, L1.cdef, L1.piw, L1.sw, L1.gn, L1.pimax};
    EXPECT(L1.Xw.bytes == Bt * n * 4 * D && L1.cdef.bytes == Bt * N * 4 * D && L1.piw.bytes == L1.cdef.bytes);
    EXPECT(L1.sw.bytes == Bt * D && L1.gn.bytes == Bt * D && L1.pimax.bytes == Bt * D);
    for (size_t i = 0; i < 6; ++i) {
        EXPECT(rs[i].off % D == 0 && rs[i].off + rs[i].bytes <= L1.bytes);
        EXPECT(rs[i].off >= L1.nu.off + L1.nu.bytes && rs[i].off + rs[i].bytes <= L1.W.off);
        for (size_t j = i + 1; j < 6; ++j) EXPECT(rs[i].off + rs[i].bytes <= rs[j].off);
    }
    for (int own = 0; own < 2; ++own) {
        const CworkNmpc C0(Bt, n, own != 0), C1(Bt, n, own != 0, true);
        EXPECT(C0.Xit.bytes == 0);
        EXPECT(C0.s.off == C1.s.off && C0.z.off == C1.z.off && C0.iters.off == C1.iters.off && C0.x0.off == C1.x0.off);
        EXPECT(C1.Xit.bytes == Bt * n * 4 * D && C1.Xit.off % D == 0 && C1.Xit.off >= C0.bytes &&
               C1.Xit.off + C1.Xit.bytes == C1.bytes);
    }
}

int main() {
    for (int N : {1, 63, 64, 65, 127}) check_stages(N);
    for (size_t Bt : {(size_t)1, (size_t)257})
        for (size_t N : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)127}) check_layouts(Bt, N, 616);
    printf("nmpc_dms_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
