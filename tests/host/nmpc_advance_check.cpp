// Stand-alone check of csrc/bqp_nmpc_advance.h, the per-instance advance of the asynchronous
// nonlinear MPC loop, on the workspace csrc/bqp_layout.h CworkNmpc describes: the Makefile builds
// it with g++ -std=c++17 -fsanitize=address,undefined (build/nmpc_advance_check),
// tests/test_host_nmpc_advance.py runs it.
//
// For N = 1, 2, 64, 127, batch 3, 3 steps: the host side of nmpc_loop_advance_kernel - due test,
// the shift's two passes over a staging array of exactly N doubles, the logs, a made-up plant
// step, the record and the transition, in the kernel's order - runs on heap buffers of exactly the
// documented sizes (an index past one of them stops the program under the address sanitizer).
// Checked: the warm start against z[min(j + 1, N - 1)] with theta kept; the per-solve state after
// the reset; ts and nfin; the last step, where z is left as it is and nfin counts the instance
// once, also when the advance is called again; an instance that is not done, where no byte of any
// buffer changes.  Then the extended CworkNmpc at batch 1 and 257: alignment, disjointness, nfin
// straight after ts, the byte total, and the step-synchronous form unchanged.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "bqp_layout.h"
#include "bqp_nmpc_advance.h"

using bqp::NmpcAdvanceArgs;
namespace layout = bqp::layout;

static int failures = 0;
static long checks = 0;
static char what[64] = "";

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
    std::vector<T> copy() const { return std::vector<T>(p, p + n); }
    bool equals(const std::vector<T>& v) const { return v.size() == n && (n == 0 || memcmp(v.data(), p, n * sizeof(T)) == 0); }
};

// a made-up plant step, exact in binary: x+ = x / 2 + u
static void fake_plant(double (&x)[4], double u) {
    for (int i = 0; i < 4; ++i) x[i] = 0.5 * x[i] + u;
}

// one instance's part of nmpc_loop_advance_kernel, the lanes as loops; `stage` stands for its LDS
static void advance(const NmpcAdvanceArgs& a, int b, double* stage) {
    if (b >= a.batch || !nmpc_advance_due(a, b)) return;
    const int t = a.ts[b], N = a.N;
    const bool more = t + 1 < a.steps;
    double* zb = a.z + (int64_t)b * (N + 1);
    const double u0 = zb[0];
    if (more)
        for (int j = 0; j < N; ++j) bqp::nmpc_shift_stage(zb, N, j, stage);
    if (more)
        for (int j = 0; j < N; ++j) bqp::nmpc_shift_store(zb, j, stage);
    nmpc_advance_log(a, b, t);
    double x[4];
    for (int i = 0; i < 4; ++i) x[i] = a.s[(int64_t)b * 4 + i] + a.xeq[i];
    const double u = u0 + a.ueq[0];
    fake_plant(x, u);
    nmpc_advance_record(a, b, t, x, u);
    nmpc_advance_next(a, b, t);
}

static double z_init(int b, int j) { return 0.25 * (b + 1) + 0.125 * j; }

static void run(int N, bool with_logs) {
    snprintf(what, sizeof(what), "N %d%s", N, with_logs ? "" : ", no logs");
    const int B = 3, S = 3, n = N + 1;
    const layout::CworkNmpc CL(B, n, true);
    Heap<char> cw(CL.bytes);                 // the loop's workspace, as bqp_api.cpp carves it
    Heap<double> X((size_t)B * (S + 1) * 4), U((size_t)B * S), nu(B), stage(N);
    Heap<int> done(B), flagsl(with_logs ? (size_t)B * S : 0), itlog(with_logs ? (size_t)B * S : 0);
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
    a.flags = with_logs ? flagsl.p : nullptr;
    a.itlog = with_logs ? itlog.p : nullptr;
    for (int b = 0; b < B; ++b) {
        for (int j = 0; j < n; ++j) a.z[(size_t)b * n + j] = z_init(b, j);
        for (int i = 0; i < 4; ++i) {
            a.s[b * 4 + i] = 0.0625 * (b + i);
            a.x0[b * 4 + i] = a.s[b * 4 + i] + xeq[i];
            X.p[(size_t)b * (S + 1) * 4 + i] = a.x0[b * 4 + i];
        }
    }
    // instance 1 runs through its steps alone: 0 and 2 are not done and must not change
    const int b = 1;
    for (int t = 0; t < S; ++t) {
        // the SQP of step t has stopped: its state as the update kernel leaves it
        done.p[b] = 1; a.flag[b] = t == 1 ? -2 : 1; a.iters[b] = 3 + t; nu.p[b] = 2.5;
        const std::vector<double> z0(a.z + (size_t)b * n, a.z + (size_t)(b + 1) * n);
        double xs[4];
        for (int i = 0; i < 4; ++i) xs[i] = a.s[b * 4 + i] + xeq[i];
        const double u = z0[0] + ueq[0];
        fake_plant(xs, u);
        const std::vector<char> before = cw.copy();
        for (int i = 0; i < B; ++i) advance(a, i, stage.p);
        EXPECT(a.ts[b] == t + 1);
        for (int i = 0; i < 4; ++i) {
            EXPECT(X.p[((size_t)b * (S + 1) + t + 1) * 4 + i] == xs[i]);
            EXPECT(a.x0[b * 4 + i] == xs[i]);
            EXPECT(a.s[b * 4 + i] == xs[i] - xeq[i]);
        }
        EXPECT(U.p[(size_t)b * S + t] == u);
        if (with_logs) {
            EXPECT(flagsl.p[(size_t)b * S + t] == (t == 1 ? -2 : 1));
            EXPECT(itlog.p[(size_t)b * S + t] == 3 + t);
        }
        if (t + 1 < S) {
            for (int j = 0; j < N; ++j) EXPECT(a.z[(size_t)b * n + j] == z0[j + 1 < N ? j + 1 : N - 1]);
            EXPECT(a.z[(size_t)b * n + N] == z0[N]);   // theta kept
            EXPECT(a.iters[b] == 0 && a.flag[b] == 0 && nu.p[b] == 0.0 && done.p[b] == 0);
            EXPECT(*a.nfin == 0);
        } else {
            // last step: no shift, the instance stays done and is counted once
            for (int j = 0; j < n; ++j) EXPECT(a.z[(size_t)b * n + j] == z0[j]);
            EXPECT(done.p[b] == 1 && a.ts[b] == S);
            EXPECT(*a.nfin == 1);
        }
        // the other instances' rows of the workspace are as they were
        for (int o = 0; o < B; o += 2) {
            EXPECT(memcmp(a.z + (size_t)o * n, before.data() + CL.z.off + (size_t)o * n * sizeof(double), n * sizeof(double)) == 0);
            EXPECT(memcmp(a.s + o * 4, before.data() + CL.s.off + (size_t)o * 4 * sizeof(double), 4 * sizeof(double)) == 0);
            EXPECT(a.ts[o] == 0 && a.iters[o] == 0 && a.flag[o] == 0);
        }
    }
    {   // a finished instance and instances that are not done: nothing changes anywhere
        const std::vector<char> c0 = cw.copy();
        const std::vector<double> X0 = X.copy(), U0 = U.copy(), n0 = nu.copy();
        const std::vector<int> d0 = done.copy(), f0 = flagsl.copy(), i0 = itlog.copy();
        for (int r = 0; r < 2; ++r)
            for (int i = 0; i < B; ++i) advance(a, i, stage.p);
        EXPECT(cw.equals(c0) && X.equals(X0) && U.equals(U0) && nu.equals(n0));
        EXPECT(done.equals(d0) && flagsl.equals(f0) && itlog.equals(i0));
        EXPECT(*a.nfin == 1);
    }
    // steps 1 .. S of the untouched instances were never written
    for (int o = 0; o < B; o += 2)
        for (int k = 4; k < (S + 1) * 4; ++k) EXPECT(X.p[(size_t)o * (S + 1) * 4 + k] == 0.0);
}

static void check_layout(size_t B, size_t N) {
    snprintf(what, sizeof(what), "layout B %zu N %zu", B, N);
    constexpr size_t D = sizeof(double), I = sizeof(int);
    const size_t n = N + 1;
    const layout::CworkNmpc L(B, n, true);
    struct Named { const char* name; layout::Region r; size_t elem, count; };
    const Named rs[] = {{"s", L.s, D, 4 * B}, {"z", L.z, D, n * B}, {"flags", L.flags, I, B},
                        {"iters", L.iters, I, B}, {"ts", L.ts, I, B}, {"nfin", L.nfin, I, 1},
                        {"x0", L.x0, D, 4 * B}};
    const size_t R = sizeof(rs) / sizeof(rs[0]);
    for (size_t i = 0; i < R; ++i) {
        EXPECT(rs[i].r.off % rs[i].elem == 0);
        EXPECT(rs[i].r.bytes == rs[i].elem * rs[i].count);
        EXPECT(rs[i].r.off + rs[i].r.bytes <= L.bytes);
        for (size_t j = i + 1; j < R; ++j) {
            const bool apart = rs[i].r.off + rs[i].r.bytes <= rs[j].r.off ||
                               rs[j].r.off + rs[j].r.bytes <= rs[i].r.off;
            if (!apart) fprintf(stderr, "B %zu N %zu: %s overlaps %s\n", B, N, rs[i].name, rs[j].name);
            EXPECT(apart);
        }
    }
    EXPECT(L.nfin.off == L.ts.off + B * I);   // one memset zeroes ts[] and nfin
    // doubles, then 3 B + 1 ints padded to a double boundary, then x0
    const size_t ints = ((3 * B + 1) * I + D - 1) / D * D;
    EXPECT(L.x0.off == (4 + n) * B * D + ints);
    EXPECT(L.bytes == (4 + n) * B * D + ints + 4 * B * D);
    // the step-synchronous form: the earlier regions where they were, none of the new ones
    const layout::CworkNmpc L0(B, n);
    EXPECT(L0.s.off == L.s.off && L0.z.off == L.z.off && L0.flags.off == L.flags.off && L0.iters.off == L.iters.off);
    EXPECT(L0.ts.bytes == 0 && L0.nfin.bytes == 0 && L0.x0.bytes == 0);
    EXPECT(L0.bytes == (4 + n) * B * D + 2 * B * I);
}

int main() {
    const int Ns[] = {1, 2, 64, 127};
    for (int N : Ns) {
        run(N, true);
        run(N, false);
    }
    EXPECT(bqp::nmpc_shift_src(1, 0) == 0);
    EXPECT(bqp::nmpc_shift_src(127, 125) == 126 && bqp::nmpc_shift_src(127, 126) == 126);
    const size_t Bs[] = {1, 257};
    for (size_t B : Bs)
        for (int N : Ns) check_layout(B, (size_t)N);
    printf("nmpc_advance_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
