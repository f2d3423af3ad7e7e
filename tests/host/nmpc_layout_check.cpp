// Stand-alone check of the nonlinear MPC workspace layout (csrc/bqp_layout.h, Nwork): the
// Makefile builds it with g++ -std=c++17 -fsanitize=address,undefined (build/nmpc_layout_check),
// tests/test_host_nmpc_layout.py runs it.
//
// At N = 1, 10, 100, 127 and batch 1, 257 (m = 10 N + 616, 8 trials): every region aligned to its
// element, regions pairwise disjoint and inside `bytes`, ndone straight after done, and the byte
// total against the sum worked out from the shapes alone.  Pinned: 1.3 MB of C per instance at
// N = 100 and the 334 MB of a batch of 256.
#include <stdio.h>

#include <vector>

#include "bqp_layout.h"

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

constexpr size_t D = sizeof(double), I = sizeof(int), NTRIAL = 8;

struct Named { const char* name; Region r; size_t elem; };

static void check(size_t B, size_t N) {
    const size_t n = N + 1, nr = 5 * N + 8, m = 10 * N + 616;
    const Nwork L(B, N, m, NTRIAL);
    EXPECT(L.n == n);
    EXPECT(L.nr == nr);
    const std::vector<Named> rs = {
        {"Jr", L.Jr, D}, {"er", L.er, D}, {"H", L.H, D}, {"f", L.f, D}, {"C", L.C, D},
        {"rhs", L.rhs, D}, {"lam", L.lam, D}, {"d", L.d, D}, {"cost0", L.cost0, D},
        {"costT", L.costT, D}, {"violT", L.violT, D}, {"stat", L.stat, D}, {"cprev", L.cprev, D},
        {"nu", L.nu, D}, {"qpflag", L.qpflag, I}, {"done", L.done, I}, {"ndone", L.ndone, I}};
    size_t sum = 0;
    for (size_t i = 0; i < rs.size(); ++i) {
        EXPECT(rs[i].r.off % rs[i].elem == 0);
        EXPECT(rs[i].r.bytes > 0);
        EXPECT(rs[i].r.off + rs[i].r.bytes <= L.bytes);
        sum += rs[i].r.bytes;
        for (size_t j = i + 1; j < rs.size(); ++j) {
            const bool apart = rs[i].r.off + rs[i].r.bytes <= rs[j].r.off ||
                               rs[j].r.off + rs[j].r.bytes <= rs[i].r.off;
            if (!apart) fprintf(stderr, "N %zu B %zu: %s overlaps %s\n", N, B, rs[i].name, rs[j].name);
            EXPECT(apart);
        }
    }
    // sizes from the shapes
    EXPECT(L.Jr.bytes == B * nr * n * D);
    EXPECT(L.er.bytes == B * nr * D);
    EXPECT(L.H.bytes == B * n * n * D);
    EXPECT(L.f.bytes == B * n * D);
    EXPECT(L.C.bytes == B * m * n * D);
    EXPECT(L.rhs.bytes == B * m * D);
    EXPECT(L.lam.bytes == B * m * D);
    EXPECT(L.d.bytes == B * n * D);
    EXPECT(L.costT.bytes == B * NTRIAL * D);
    EXPECT(L.violT.bytes == B * NTRIAL * D);
    EXPECT(L.ndone.off == L.done.off + B * I);   // one memset zeroes done[] and ndone
    // the doubles come first, so nothing is padded: the total is the sum of the regions
    const size_t doubles = B * (nr * n + nr + n * n + 2 * n + m * n + 2 * m + 4 + 2 * NTRIAL);
    EXPECT(sum == L.bytes);
    EXPECT(L.bytes == doubles * D + (2 * B + 1) * I);
}

int main() {
    const size_t Ns[] = {1, 10, 100, 127}, Bs[] = {1, 257};
    for (size_t N : Ns)
        for (size_t B : Bs) check(B, N);
    {   // N = 100: C is 1616 x 101 doubles = 1.3 MB per instance; a batch of 256 takes 334 MB of C
        const Nwork L(256, 100, 1616, NTRIAL);
        EXPECT(L.C.bytes == (size_t)256 * 1305728);
        EXPECT(L.C.bytes / 1000000 == 334);
        EXPECT(L.bytes == (size_t)256 * (51308 + 508 + 10201 + 202 + 163216 + 3232 + 20) * D + 513 * I);
    }
    {   // a batch whose bytes pass 2^32: the arithmetic is size_t throughout
        const Nwork L(4096, 127, 1886, NTRIAL);
        EXPECT(L.C.bytes == (size_t)4096 * 1886 * 128 * D);
        EXPECT(L.bytes > ((size_t)1 << 32));
    }
    for (size_t N : Ns)
        for (size_t B : Bs) {   // the closed loop's cwork: s (4), z (n), flags, iteration counts
            const CworkNmpc L(B, N + 1);
            EXPECT(L.s.off == 0 && L.z.off == 4 * B * D);
            EXPECT(L.flags.off == (5 + N) * B * D && L.flags.off % I == 0);
            EXPECT(L.iters.off == L.flags.off + B * I);
            EXPECT(L.bytes == (5 + N) * B * D + 2 * B * I);
        }
    printf("nmpc_layout_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
