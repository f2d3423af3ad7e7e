// Stand-alone check of csrc/bqp_layout.h: the Makefile builds it with g++ -std=c++17
// -fsanitize=address,undefined (build/layout_check), tests/test_host_layout.py runs it.
//
// 1. pinned offsets: literals worked out by hand from the arithmetic bqp_api.cpp carried before
//    the layouts were described in one place (the formula stands beside each literal);
// 2. properties over a grid of shapes: every region aligned to its element, regions pairwise
//    disjoint, every region inside `bytes`.
#include <stdio.h>

#include <vector>

#include "bqp_layout.h"

using namespace bqp::layout;

static int failures = 0;
static long checks = 0;

#define EXPECT_EQ(got, want)                                                              \
    do {                                                                                  \
        ++checks;                                                                         \
        const size_t g_ = (size_t)(got), w_ = (size_t)(want);                             \
        if (g_ != w_) {                                                                   \
            ++failures;                                                                   \
            fprintf(stderr, "%s:%d: %s = %zu, expected %zu\n", __FILE__, __LINE__, #got, g_, w_); \
        }                                                                                 \
    } while (0)

constexpr size_t D = sizeof(double), I = sizeof(int);
constexpr int STATS_W = 7, QUEUES = 4, NTRIAL = 8;   // bqp_internal.h / bqp_api.cpp values

static void pinned() {
    {   // work, config C2: N = 20, nv = 6 (hstride = 37), mpad = 640, batch 1024, 4 queues, no stamps
        const Work L(20, 37, 6, 640, 1024, STATS_W, 0, QUEUES);
        EXPECT_EQ(L.H.off, 0);
        EXPECT_EQ(L.F.off, 777 * D);         // nH = (N + 1) hstride = 21 * 37
        EXPECT_EQ(L.stats.off, 4617 * D);    // + nF = nv mpad = 3840
        EXPECT_EQ(L.stamps.off, 11793 * D);  // + nS = 1024 * 7 = 7168, + 8 slack
        EXPECT_EQ(L.stamps.bytes, 0);
        EXPECT_EQ(L.marks.off, 11793 * D);   // + nStamp = 0
        EXPECT_EQ(L.queues.off, 12305 * D);  // + nPol = (1024 + 1) / 2 = 512
        EXPECT_EQ(L.bytes, 98456);           // + nQ = (4 + 1) / 2 = 2: 12307 doubles
    }
    {   // the same with the diagnostic build's stamps: 32 per instance = 32768 doubles
        const Work L(20, 37, 6, 640, 1024, STATS_W, 32, QUEUES);
        EXPECT_EQ(L.stamps.off, 11793 * D);
        EXPECT_EQ(L.stamps.bytes, 32768 * D);
        EXPECT_EQ(L.marks.off, 44561 * D);   // 11793 + 32768
        EXPECT_EQ(L.queues.off, 45073 * D);  // + 512
        EXPECT_EQ(L.bytes, 45075 * D);
    }
    {   // work, odd batch: N = 1, hstride 37, mpad 64, batch 3: nPol = (3 + 1) / 2 = 2 doubles
        const Work L(1, 37, 6, 64, 3, STATS_W, 0, QUEUES);
        EXPECT_EQ(L.F.off, 74 * D);          // 2 * 37
        EXPECT_EQ(L.stats.off, 458 * D);     // + 6 * 64
        EXPECT_EQ(L.marks.off, 487 * D);     // + 3 * 7 + 8
        EXPECT_EQ(L.marks.bytes, 3 * I);
        EXPECT_EQ(L.queues.off, 489 * D);    // + 2 (three ints rounded up to two doubles)
        EXPECT_EQ(L.bytes, 491 * D);
    }
    {   // hwork: 1000-float record, batch 64: stride (1000 + 63) & ~63 = 1024
        const Hwork L(1000, 64);
        EXPECT_EQ(L.stride, 1024);
        EXPECT_EQ(L.records.off, 0);
        EXPECT_EQ(L.flags.off, 262144);      // 4 * 1024 * 64
        EXPECT_EQ(L.iters.off, 262144 + 256);
        EXPECT_EQ(L.cont.off, 262144 + 512);
        EXPECT_EQ(L.bytes, 262912);          // + 3 * 4 * 64
    }
    {   // lwork: batch B = 3, N = 5, n = 6, nr = 13, m = 10, 8 trials, exact Hessian
        const Lwork L(3, 5, 6, 13, 10, NTRIAL, true);
        EXPECT_EQ(L.Jr.off, 0);
        EXPECT_EQ(L.er.off, 234 * D);        // B nr n
        EXPECT_EQ(L.H.off, 273 * D);         // + B nr = 39
        EXPECT_EQ(L.f.off, 381 * D);         // + B n n = 108
        EXPECT_EQ(L.bsh.off, 399 * D);       // + B n = 18
        EXPECT_EQ(L.lam.off, 429 * D);       // + B m = 30
        EXPECT_EQ(L.d.off, 459 * D);         // + B m
        EXPECT_EQ(L.cost0.off, 477 * D);     // + B n
        EXPECT_EQ(L.costT.off, 480 * D);     // + B
        EXPECT_EQ(L.stat.off, 504 * D);      // + 8 B
        EXPECT_EQ(L.cprev.off, 507 * D);     // + B
        EXPECT_EQ(L.Jr2.off, 510 * D);       // + B
        EXPECT_EQ(L.Tr2.off, 780 * D);       // + n2 = 3 B N n = 270
        EXPECT_EQ(L.qpflag.off, 1050 * D);   // + n2: nd = 1050 doubles
        EXPECT_EQ(L.hused.off, 1050 * D + 3 * I);
        EXPECT_EQ(L.done.off, 1050 * D + 6 * I);
        EXPECT_EQ(L.ndone.off, 1050 * D + 9 * I);   // straight after done (one memset)
        EXPECT_EQ(L.bytes, 1050 * D + 13 * I);      // ni = 3 B + 4
        // Gauss-Newton: no Jr2 / Tr2
        const Lwork G(3, 5, 6, 13, 10, NTRIAL, false);
        EXPECT_EQ(G.Jr2.bytes, 0);
        EXPECT_EQ(G.qpflag.off, 510 * D);
        EXPECT_EQ(G.bytes, 510 * D + 13 * I);
    }
    {   // dwork: 100 scratch doubles per instance, batch 3
        const Dwork L(100, 3, STATS_W);
        EXPECT_EQ(L.scratch.off, 0);
        EXPECT_EQ(L.stats.off, 300 * D);
        EXPECT_EQ(L.bytes, 329 * D);         // wst B + B STATS_W + 8
    }
    {   // cwork, structured loop: B = 3, MG (4, 1, 1), N = 5, window of q = 2 points
        const CworkOcp L(3, 4, 1, 1, 5, 2);
        EXPECT_EQ(L.s.off, 0);
        EXPECT_EQ(L.x.off, 12 * D);          // B nx
        EXPECT_EQ(L.u.off, 84 * D);          // + B (N + 1) nx = 72
        EXPECT_EQ(L.theta.off, 99 * D);      // + B N nu = 15
        EXPECT_EQ(L.window.off, 102 * D);    // + B np = 3
        EXPECT_EQ(L.flags.off, 150 * D);     // + 8 B q = 48
        EXPECT_EQ(L.bytes, 150 * D + 3 * I);
        const CworkOcp P(3, 4, 1, 1, 5, 0);   // no learning: no window
        EXPECT_EQ(P.flags.off, 102 * D);
        EXPECT_EQ(P.bytes, 102 * D + 3 * I);
    }
    {   // cwork, SQP loop: B = 3, nx = 4, n = 6, m = 10, q = 2
        const CworkSqp L(3, 4, 6, 10, 2);
        EXPECT_EQ(L.s.off, 0);
        EXPECT_EQ(L.z.off, 12 * D);          // B nx
        EXPECT_EQ(L.bin.off, 30 * D);        // + B n = 18
        EXPECT_EQ(L.u0.off, 60 * D);         // + B m = 30
        EXPECT_EQ(L.window.off, 63 * D);     // + B
        EXPECT_EQ(L.flags.off, 111 * D);     // + 8 B q = 48
        EXPECT_EQ(L.iters.off, 111 * D + 3 * I);
        EXPECT_EQ(L.ts.off, 111 * D + 6 * I);
        EXPECT_EQ(L.nfin.off, 111 * D + 9 * I);    // straight after ts (one memset)
        EXPECT_EQ(L.bytes, 111 * D + 11 * I);      // 3 B + 2 ints
    }
}

// the regions of each layout with their element's alignment: every Region member is listed here
struct R {
    Region r;
    size_t align;
    size_t end() const { return r.off + r.bytes; }
};
typedef std::vector<R> Rs;
static Rs regions(const Work& l) { return {{l.H, D}, {l.F, D}, {l.stats, D}, {l.stamps, D}, {l.marks, I}, {l.queues, I}}; }
static Rs regions(const Hwork& l) { return {{l.records, sizeof(float)}, {l.flags, I}, {l.iters, I}, {l.cont, I}}; }
static Rs regions(const Lwork& l) {
    return {{l.Jr, D}, {l.er, D}, {l.H, D}, {l.f, D}, {l.bsh, D}, {l.lam, D}, {l.d, D}, {l.cost0, D}, {l.costT, D},
            {l.stat, D}, {l.cprev, D}, {l.Jr2, D}, {l.Tr2, D}, {l.qpflag, I}, {l.hused, I}, {l.done, I}, {l.ndone, I}};
}
static Rs regions(const Dwork& l) { return {{l.scratch, D}, {l.stats, D}}; }
static Rs regions(const CworkOcp& l) { return {{l.s, D}, {l.x, D}, {l.u, D}, {l.theta, D}, {l.window, D}, {l.flags, I}}; }
static Rs regions(const CworkSqp& l) {
    return {{l.s, D}, {l.z, D}, {l.bin, D}, {l.u0, D}, {l.window, D}, {l.flags, I}, {l.iters, I}, {l.ts, I}, {l.nfin, I}};
}
// a listing that misses a member would miss its checks: the structs hold Regions and the arena's
// running total only
static_assert(sizeof(Work) == sizeof(Arena) + 6 * sizeof(Region), "Work");
static_assert(sizeof(Hwork) == sizeof(Arena) + sizeof(size_t) + 4 * sizeof(Region), "Hwork");
static_assert(sizeof(Lwork) == sizeof(Arena) + 17 * sizeof(Region), "Lwork");
static_assert(sizeof(Dwork) == sizeof(Arena) + 2 * sizeof(Region), "Dwork");
static_assert(sizeof(CworkOcp) == sizeof(Arena) + 6 * sizeof(Region), "CworkOcp");
static_assert(sizeof(CworkSqp) == sizeof(Arena) + 9 * sizeof(Region), "CworkSqp");

template <class L>
static void check(const L& l, const char* what, int batch, int N, int mp) {
    const Rs r = regions(l);
    for (size_t i = 0; i < r.size(); ++i) {
        ++checks;
        bool ok = r[i].r.off % r[i].align == 0 && r[i].end() <= l.bytes;
        for (size_t j = 0; j < i; ++j) ok = ok && (r[j].end() <= r[i].r.off || r[i].end() <= r[j].r.off);
        if (!ok) {
            ++failures;
            fprintf(stderr, "%s (batch %d, N %d, mp %d): region %zu [%zu, %zu) align %zu in %zu bytes\n",
                    what, batch, N, mp, i, r[i].r.off, r[i].end(), r[i].align, l.bytes);
        }
    }
}

static void grid() {
    const int batches[] = {1, 2, 3, 1024}, Ns[] = {1, 20, 63, 64, 127}, mps[] = {0, 22, 616, 1024};
    const int fam[2][3] = {{4, 1, 1}, {2, 2, 2}};   // (nx, nu, np): Moore-Greitzer, double integrator
    const int qs[] = {1, 100};
    for (int batch : batches)
        for (int N : Ns)
            for (int mp : mps)
                for (const auto& f : fam) {
                    const int nx = f[0], nu = f[1], np = f[2], nv = nx + nu + np;
                    // whole 64-row blocks, as the kernels pad the polytope (at least one block)
                    const int mpad = 64 * (((mp > 1 ? mp : 1) + 63) / 64);
                    for (int stamps : {0, 32})
                        check(Work(N, nv * nv + 1, nv, mpad, batch, STATS_W, stamps, QUEUES), "work", batch, N, mp);
                    // record lengths around the 64-float block, and one that grows with the shape
                    for (int hf : {1, 63, 64, 65, (N + 1) * (3 * nx + nu) + 2 * mp + 7})
                        check(Hwork(hf, batch), "hwork", batch, N, mp);
                    // the condensed sub-problem of the learned model: n variables, mp rows
                    const int n = N * nu + np, nr = N * (nx + nu) + 2 * nx;
                    for (bool hess : {false, true})
                        check(Lwork(batch, N, n, nr, mp, NTRIAL, hess), "lwork", batch, N, mp);
                    check(Dwork((int64_t)n * n + (int64_t)mp * n + 5, batch, STATS_W), "dwork", batch, N, mp);
                    check(CworkOcp(batch, nx, nu, np, N, 0), "cwork_ocp", batch, N, mp);
                    // (no cwork region is sized by the number of steps, 1 or 7: the loops keep
                    // their trajectories in the caller's arrays, so steps is no axis of this grid)
                    for (int q : qs) {
                        check(CworkOcp(batch, nx, nu, np, N, q), "cwork_ocp", batch, N, mp);
                        check(CworkSqp(batch, nx, n, mp, q), "cwork_sqp", batch, N, mp);
                    }
                }
}

int main() {
    pinned();
    grid();
    printf("layout_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
