// Stand-alone check of the set-point schedule's index arithmetic in csrc/bqp_nmpc_advance.h
// (NmpcTrackArgs and the nmpc_track_* functions of bqp_closed_loop_nmpc_track), on the workspace
// csrc/bqp_layout.h CworkNmpc describes with its current-reference buffer: the Makefile builds it
// with g++ -std=c++17 -fsanitize=address,undefined (build/nmpc_track_check),
// tests/test_host_nmpc_track.py runs it.
//
// For steps = 1, 2, N = 1, 64, 127, batch = 1, 257, with the schedule and the disturbance shared
// (stride 0) and per instance (stride steps * 4): the host side of nmpc_loop_advance_kernel<true> -
// the theta log, the shift, the logs, a made-up plant step, the disturbance, the next set-point,
// the record and the transition, in the kernel's order - runs every instance through all its steps
// on heap buffers of exactly the documented sizes (ref and dist steps * 4 doubles per instance, or
// steps * 4 in all; THETA batch * steps; xr batch * 4), so an index past one of them, the read of
// ref[b, steps] at the last step included, stops the program under the address sanitizer.
// Checked: THETA[b, t] is the theta of the step; X[b, t + 1] is the plant's state plus dist[b, t],
// added once; after step t < steps - 1 the instance's slot of xr holds ref[b, t + 1], after the last
// step it is left as it was; without ref, dist or THETA the advance is the one without a track.
// Then the layout: xr is the last region, 4 doubles per instance, and the layout without it is
// unchanged.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bqp_layout.h"
#include "bqp_nmpc_advance.h"

using bqp::NmpcAdvanceArgs;
using bqp::NmpcTrackArgs;
namespace layout = bqp::layout;

static int failures = 0;
static long checks = 0;
static char what[96] = "";

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        ++checks;                                                                     \
        if (!(cond)) {                                                                \
            ++failures;                                                               \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, what); \
        }                                                                             \
    } while (0)

// exactly n elements on the heap
template <class T>
struct Heap {
    T* p;
    size_t n;
    explicit Heap(size_t n_) : p((T*)malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {
        for (size_t i = 0; i < n; ++i) p[i] = (T)0;
    }
    ~Heap() { free(p); }
    T* ptr() const { return n ? p : nullptr; }
};

// a made-up plant step, exact in binary: x+ = x / 2 + u
static void fake_plant(double (&x)[4], double u) {
    for (int i = 0; i < 4; ++i) x[i] = 0.5 * x[i] + u;
}

// one instance's part of nmpc_loop_advance_kernel<true>, the lanes as loops
static void advance(const NmpcAdvanceArgs& a, const NmpcTrackArgs& k, int b, double* stage) {
    if (b >= a.batch || !nmpc_advance_due(a, b)) return;
    const int t = a.ts[b], N = a.N;
    const bool more = t + 1 < a.steps;
    double* zb = a.z + (int64_t)b * (N + 1);
    const double u0 = zb[0];
    nmpc_track_log(k, a.steps, N, b, t, zb);
    if (more)
        for (int j = 0; j < N; ++j) bqp::nmpc_shift_stage(zb, N, j, stage);
    if (more)
        for (int j = 0; j < N; ++j) bqp::nmpc_shift_store(zb, j, stage);
    nmpc_advance_log(a, b, t);
    double x[4];
    for (int i = 0; i < 4; ++i) x[i] = a.s[(int64_t)b * 4 + i] + a.xeq[i];
    const double u = u0 + a.ueq[0];
    fake_plant(x, u);
    nmpc_track_disturb(k, b, t, x);
    nmpc_track_next_ref(k, a.steps, b, t);
    nmpc_advance_record(a, b, t, x, u);
    nmpc_advance_next(a, b, t);
}

// exact in binary
static double ref_val(int b, int t, int i) { return 8.0 * b + 0.5 * t + 0.0625 * i + 1.0; }
static double dist_val(int b, int t, int i) { return 0.25 * ((b + t + i) % 5) - 0.5; }
static double theta_val(int b, int t) { return 0.125 * b - 0.5 * t; }

// mode bits: 1 schedule, 2 disturbance, 4 theta log; shared: stride 0 for both
static void run(int B, int N, int S, int mode, bool shared) {
    snprintf(what, sizeof(what), "B %d N %d steps %d mode %d %s", B, N, S, mode, shared ? "shared" : "per instance");
    const int n = N + 1;
    const bool has_ref = mode & 1, has_dist = mode & 2, has_th = mode & 4;
    const layout::CworkNmpc CL(B, n, true, false, has_ref);
    Heap<char> cw(CL.bytes);
    Heap<double> X((size_t)B * (S + 1) * 4), U((size_t)B * S), nu(B), stage(N);
    Heap<int> done(B);
    const size_t sched = (size_t)(shared ? 1 : B) * S * 4;
    Heap<double> ref(has_ref ? sched : 0), dist(has_dist ? sched : 0), TH(has_th ? (size_t)B * S : 0);
    const int64_t stride = shared ? 0 : (int64_t)S * 4;
    const double xeq[4] = {0.5, 1.5, 1.25, 0.0}, ueq[1] = {1.25};
    NmpcAdvanceArgs a;
    memset(&a, 0, sizeof(a));
    a.batch = B; a.N = N; a.steps = S; a.delta = 0.01; a.xeq = xeq; a.ueq = ueq;
    a.s = layout::at<double>(cw.p, CL.s);
    a.z = layout::at<double>(cw.p, CL.z);
    a.x0 = layout::at<double>(cw.p, CL.x0);
    a.flag = layout::at<int>(cw.p, CL.flags);
    a.iters = layout::at<int>(cw.p, CL.iters);
    a.ts = layout::at<int>(cw.p, CL.ts);
    a.nfin = layout::at<int>(cw.p, CL.nfin);
    a.X = X.p; a.U = U.p; a.nu = nu.p; a.done = done.p;
    NmpcTrackArgs k;
    memset(&k, 0, sizeof(k));
    k.ref = ref.ptr(); k.sref = stride; k.dist = dist.ptr(); k.sdist = stride; k.THETA = TH.ptr();
    k.xr = has_ref ? layout::at<double>(cw.p, CL.xr) : nullptr;
    for (int b = 0; b < (shared ? 1 : B); ++b)
        for (int t = 0; t < S; ++t)
            for (int i = 0; i < 4; ++i) {
                if (has_ref) ref.p[bqp::nmpc_track_at(stride, b, t, i)] = ref_val(b, t, i);
                if (has_dist) dist.p[bqp::nmpc_track_at(stride, b, t, i)] = dist_val(b, t, i);
            }
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < 4; ++i) {
            a.s[b * 4 + i] = 0.0625 * ((b + i) % 7);
            a.x0[b * 4 + i] = a.s[b * 4 + i] + xeq[i];
            X.p[(size_t)b * (S + 1) * 4 + i] = a.x0[b * 4 + i];
            // step 0's set-point, as nmpc_track_init_kernel copies it
            if (has_ref) k.xr[b * 4 + i] = ref.p[bqp::nmpc_track_at(stride, b, 0, i)];
        }
    for (int t = 0; t < S; ++t) {
        std::vector<double> xs((size_t)B * 4), xr0;
        if (has_ref) xr0.assign(k.xr, k.xr + (size_t)B * 4);
        for (int b = 0; b < B; ++b) {
            // the SQP of step t has stopped: its state as the update kernel leaves it
            done.p[b] = 1; a.flag[b] = 1; a.iters[b] = 2; nu.p[b] = 2.5;
            for (int j = 0; j < N; ++j) a.z[(size_t)b * n + j] = 0.25 * (b % 3) + 0.125 * (j % 5);
            a.z[(size_t)b * n + N] = theta_val(b, t);
            double x[4];
            for (int i = 0; i < 4; ++i) x[i] = a.s[b * 4 + i] + xeq[i];
            fake_plant(x, a.z[(size_t)b * n] + ueq[0]);
            for (int i = 0; i < 4; ++i) xs[(size_t)b * 4 + i] = x[i];
        }
        for (int b = 0; b < B; ++b) advance(a, k, b, stage.p);
        const int sb = shared ? 0 : 1;
        for (int b = 0; b < B; ++b) {
            EXPECT(a.ts[b] == t + 1);
            for (int i = 0; i < 4; ++i) {
                const double want = has_dist ? xs[(size_t)b * 4 + i] + dist_val(sb * b, t, i) : xs[(size_t)b * 4 + i];
                EXPECT(X.p[((size_t)b * (S + 1) + t + 1) * 4 + i] == want);
                EXPECT(a.x0[b * 4 + i] == want);
                EXPECT(a.s[b * 4 + i] == want - xeq[i]);
                if (has_ref) {
                    // the next step's set-point while steps remain; the last step leaves the slot
                    if (bqp::nmpc_track_has_next(S, t)) EXPECT(k.xr[b * 4 + i] == ref_val(sb * b, t + 1, i));
                    else EXPECT(k.xr[b * 4 + i] == xr0[(size_t)b * 4 + i]);
                }
            }
            if (has_th) EXPECT(TH.p[bqp::nmpc_track_theta_at(S, b, t)] == theta_val(b, t));
            if (t + 1 < S) EXPECT(a.z[(size_t)b * n + N] == theta_val(b, t));   // theta kept by the shift
        }
    }
    EXPECT(*a.nfin == B);
}

static void check_index() {
    snprintf(what, sizeof(what), "index functions");
    EXPECT(bqp::nmpc_track_at(0, 256, 1, 3) == 7);              // shared: the instance does not enter
    EXPECT(bqp::nmpc_track_at(8, 256, 1, 3) == 256 * 8 + 7);
    EXPECT(bqp::nmpc_track_at(4, 0, 0, 0) == 0);
    // past 2^31: 64-bit throughout
    EXPECT(bqp::nmpc_track_at((int64_t)1 << 20, 4096, 2, 1) == ((int64_t)4096 << 20) + 9);
    EXPECT(!bqp::nmpc_track_has_next(1, 0));
    EXPECT(bqp::nmpc_track_has_next(2, 0) && !bqp::nmpc_track_has_next(2, 1));
    EXPECT(bqp::nmpc_track_theta_at(2, 256, 1) == 513);
    EXPECT(bqp::nmpc_track_theta_at(1, 0, 0) == 0);
}

static void check_layout(size_t B, size_t N) {
    snprintf(what, sizeof(what), "layout B %zu N %zu", B, N);
    constexpr size_t D = sizeof(double);
    const size_t n = N + 1;
    for (int dms = 0; dms < 2; ++dms) {
        const layout::CworkNmpc L0(B, n, true, dms != 0), L(B, n, true, dms != 0, true);
        EXPECT(L.s.off == L0.s.off && L.z.off == L0.z.off && L.flags.off == L0.flags.off && L.iters.off == L0.iters.off);
        EXPECT(L.ts.off == L0.ts.off && L.nfin.off == L0.nfin.off && L.x0.off == L0.x0.off && L.Xit.off == L0.Xit.off);
        EXPECT(L0.xr.bytes == 0);
        EXPECT(L.xr.bytes == 4 * B * D && L.xr.off % D == 0);
        EXPECT(L.xr.off >= L0.bytes);                       // behind everything the loop had
        EXPECT(L.bytes == L.xr.off + L.xr.bytes);
    }
    // the step-synchronous loop points the solves at the schedule itself: no buffer
    const layout::CworkNmpc Ls(B, n, false, false, false), Ls0(B, n);
    EXPECT(Ls.bytes == Ls0.bytes && Ls.xr.bytes == 0);
}

int main() {
    const int Ns[] = {1, 64, 127}, Bs[] = {1, 257}, Ss[] = {1, 2};
    for (int B : Bs)
        for (int N : Ns)
            for (int S : Ss)
                for (int shared = 0; shared < 2; ++shared) {
                    run(B, N, S, 7, shared != 0);
                    run(B, N, S, 1, shared != 0);      // a schedule alone
                    run(B, N, S, 2, shared != 0);      // a disturbance alone
                }
    run(257, 127, 2, 4, false);                        // the theta log alone
    run(257, 127, 2, 0, false);                        // nothing: the advance without a track
    check_index();
    for (int B : Bs)
        for (int N : Ns) check_layout((size_t)B, (size_t)N);
    printf("nmpc_track_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
