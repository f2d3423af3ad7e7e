// Stand-alone check of the nonlinear MPC stage route's host/device arithmetic
// (csrc/bqp_nmpc_stage.h) and workspace (csrc/bqp_layout.h, NworkStage): the Makefile builds it
// with g++ -std=c++17 -fsanitize=address,undefined (build/nmpc_stage_check),
// tests/test_host_nmpc_stage.py runs it.
//
//   - the NworkStage layout at N = 1, 2, 64, 100, 127 and batch 1, 257: regions aligned, disjoint,
//     inside `bytes`, sized from the shapes, ndone straight after done; the bytes per instance at
//     N = 100 with the 616-row terminal set;
//   - the bound map: unit rows, scaled and permuted rows, and the rows it must refuse;
//   - the stores of the stage linearisation (rhs in NMPC row order, every bound in the structured
//     solve's arrays) and the row-order map back (lam_x, lam_u, lam_p -> lam) at N = 1, 2, 64, 127
//     on heap buffers of exactly the documented sizes.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "bqp_layout.h"
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

constexpr size_t D = sizeof(double), I = sizeof(int), NTRIAL = 8;

struct Named { const char* name; Region r; size_t elem; };

static void check_layout(size_t B, size_t N, size_t mp) {
    const size_t n = N + 1, m = 10 * N + mp, MB = sizeof(NmpcBoundMap);
    const NworkStage L(B, N, mp, m, NTRIAL, MB);
    EXPECT(L.n == n);
    const std::vector<Named> rs = {
        {"A", L.A, D}, {"B", L.B, D}, {"w", L.w, D}, {"xlb", L.xlb, D}, {"xub", L.xub, D},
        {"ulb", L.ulb, D}, {"uub", L.uub, D}, {"hp", L.hp, D}, {"xo", L.xo, D}, {"uo", L.uo, D},
        {"tho", L.tho, D}, {"fv", L.fv, D}, {"lamx", L.lamx, D}, {"lamu", L.lamu, D},
        {"lamp", L.lamp, D}, {"rhs", L.rhs, D}, {"lam", L.lam, D}, {"d", L.d, D}, {"f", L.f, D},
        {"ctl", L.ctl, D}, {"cost0", L.cost0, D}, {"costT", L.costT, D}, {"violT", L.violT, D},
        {"stat", L.stat, D}, {"cprev", L.cprev, D}, {"nu", L.nu, D}, {"W", L.W, D}, {"Fp", L.Fp, D},
        {"x0z", L.x0z, D}, {"map", L.map, D}, {"sflag", L.sflag, I}, {"qpflag", L.qpflag, I},
        {"done", L.done, I}, {"ndone", L.ndone, I}};
    size_t sum = 0;
    for (size_t i = 0; i < rs.size(); ++i) {
        EXPECT(rs[i].r.off % rs[i].elem == 0);
        EXPECT(rs[i].r.off + rs[i].r.bytes <= L.bytes);
        sum += rs[i].r.bytes;
        for (size_t j = i + 1; j < rs.size(); ++j) {
            const bool apart = rs[i].r.off + rs[i].r.bytes <= rs[j].r.off ||
                               rs[j].r.off + rs[j].r.bytes <= rs[i].r.off;
            if (!apart) fprintf(stderr, "N %zu B %zu: %s overlaps %s\n", N, B, rs[i].name, rs[j].name);
            EXPECT(apart);
        }
    }
    EXPECT(L.A.bytes == B * N * 16 * D);
    EXPECT(L.B.bytes == B * N * 4 * D);
    EXPECT(L.w.bytes == B * n * 6 * D);
    EXPECT(L.xlb.bytes == B * n * 4 * D && L.xub.bytes == L.xlb.bytes);
    EXPECT(L.ulb.bytes == B * N * D && L.uub.bytes == L.ulb.bytes);
    EXPECT(L.hp.bytes == B * mp * D && L.lamp.bytes == B * mp * D);
    EXPECT(L.xo.bytes == B * n * 4 * D && L.uo.bytes == B * N * D);
    EXPECT(L.lamx.bytes == B * n * 8 * D && L.lamu.bytes == B * N * 2 * D);
    EXPECT(L.rhs.bytes == B * m * D && L.lam.bytes == B * m * D);
    EXPECT(L.d.bytes == B * n * D && L.f.bytes == B * n * D && L.ctl.bytes == B * n * D);
    EXPECT(L.W.bytes == n * 36 * D && L.Fp.bytes == mp * 6 * D && L.x0z.bytes == 4 * D);
    EXPECT(L.map.bytes == MB);
    EXPECT(L.ndone.off == L.done.off + B * I);   // one memset zeroes done[] and ndone
    // doubles first, then the 8-aligned map, then ints: nothing is padded
    EXPECT(MB % D == 0);
    EXPECT(sum == L.bytes);
}

static void check_bound_map() {
    // the Moore-Greitzer problem's rows: F_x = [I; -I], F_u = [1; -1]
    double Fx[8 * 4] = {0}, Fu[2] = {1.0, -1.0};
    for (int v = 0; v < 4; ++v) { Fx[v + 8 * v] = 1.0; Fx[4 + v + 8 * v] = -1.0; }
    NmpcBoundMap m;
    EXPECT(nmpc_bound_map_build(Fx, 8, Fu, 2, &m) == 0 && m.notbox == 0);
    for (int v = 0; v < 4; ++v) {
        EXPECT(m.rowof[v][1] == v && m.rowof[v][0] == 4 + v);
        EXPECT(m.var[v] == v && m.side[v] == 1 && m.var[4 + v] == v && m.side[4 + v] == 0);
        EXPECT(m.scale[v] == 1.0 && m.scale[4 + v] == 1.0);
    }
    EXPECT(m.rowof[4][1] == 8 && m.rowof[4][0] == 9 && m.var[8] == 4 && m.var[9] == 4);
    EXPECT(m.side[8] == 1 && m.side[9] == 0);
    // permuted and scaled: row i bounds variable pv[i] on side ps[i] with scale sc[i]
    const int pv[6] = {2, 0, 3, 0, 1, 2}, ps[6] = {0, 1, 1, 0, 1, 1};
    const double sc[6] = {2.0, 0.5, 3.0, 0.7, 1.0, 1.3};
    std::vector<double> G(6 * 4, 0.0);
    for (int i = 0; i < 6; ++i) G[i + 6 * pv[i]] = ps[i] ? sc[i] : -sc[i];
    const double Gu[1] = {-2.5};
    EXPECT(nmpc_bound_map_build(G.data(), 6, Gu, 1, &m) == 0);
    for (int i = 0; i < 6; ++i) {
        EXPECT(m.var[i] == pv[i] && m.side[i] == ps[i] && m.scale[i] == sc[i]);
        EXPECT(m.rowof[pv[i]][ps[i]] == i);
    }
    EXPECT(m.rowof[1][0] == -1 && m.rowof[3][0] == -1 && m.rowof[4][1] == -1 && m.rowof[4][0] == 6);
    EXPECT(nmpc_bound_value(m, 0, 3.0) == -1.5 && nmpc_bound_value(m, 1, 3.0) == 6.0);
    EXPECT(nmpc_bound_value(m, 6, 5.0) == -2.0);
    // refused: a two-entry row, two rows on one side, an empty row, a non-finite entry, too many rows
    std::vector<double> H = G;
    H[0 + 6 * 0] = 0.25;
    EXPECT(nmpc_bound_map_build(H.data(), 6, Gu, 1, &m) == 1 && m.notbox == 1);
    H = G; H[3 + 6 * 0] = 0.7;                   // rows 1 and 3 both bound x1 from above
    EXPECT(nmpc_bound_map_build(H.data(), 6, Gu, 1, &m) == 1);
    H = G; H[4 + 6 * 1] = 0.0;
    EXPECT(nmpc_bound_map_build(H.data(), 6, Gu, 1, &m) == 1);
    H = G; H[4 + 6 * 1] = NAN;
    EXPECT(nmpc_bound_map_build(H.data(), 6, Gu, 1, &m) == 1);
    H = G; H[4 + 6 * 1] = INFINITY;
    EXPECT(nmpc_bound_map_build(H.data(), 6, Gu, 1, &m) == 1);
    const double Gz[1] = {0.0};
    EXPECT(nmpc_bound_map_build(G.data(), 6, Gz, 1, &m) == 1);
    EXPECT(nmpc_bound_map_build(G.data(), NMS_MAXMX + 1, Gu, 1, &m) == 1);   // reads nothing
    for (int i = 0; i < NMS_MAXROWS; ++i) EXPECT(m.var[i] >= 0 && m.var[i] < NMS_NVAR && m.side[i] >= 0 && m.side[i] <= 1);
    // no rows at all is a box
    EXPECT(nmpc_bound_map_build(nullptr, 0, nullptr, 0, &m) == 0);
}

// the stage linearisation's stores and the back-map's loads, as the kernels index them
static void check_maps(int N, int mx, int mu, int mp, const NmpcBoundMap& m) {
    const int ms = mx + mu;
    const size_t M = (size_t)N * ms + mp;
    std::vector<double> xlb((size_t)(N + 1) * 4, 0.0), xub((size_t)(N + 1) * 4, 0.0), ulb(N, 0.0), uub(N, 0.0);
    std::vector<double> rhs(M, 0.0);
    for (int k = 0; k < N; ++k)
        for (int lane = 0; lane < ms; ++lane) {
            const bool isx = nmpc_row_is_state(mx, lane);
            double* bnd = (isx ? (m.side[lane] ? xub.data() : xlb.data()) : (m.side[lane] ? uub.data() : ulb.data())) +
                          nmpc_bound_index(m, mx, 1, lane);
            const int bstride = isx ? 4 : 1;
            rhs[(size_t)nmpc_stage_row(mx, mu, k + 1, lane)] += 1.0;
            bnd[(size_t)k * bstride] += 1.0;
        }
    for (int r = 0; r < mp; ++r) rhs[(size_t)nmpc_term_row(N, mx, mu, r)] += 1.0;
    for (size_t r = 0; r < M; ++r) EXPECT(rhs[r] == 1.0);          // every row once
    for (int k = 0; k <= N; ++k)
        for (int v = 0; v < 4; ++v) {                              // stage 0 untouched
            EXPECT(xlb[nmpc_xb_index(k, v)] == ((k > 0 && m.rowof[v][0] >= 0) ? 1.0 : 0.0));
            EXPECT(xub[nmpc_xb_index(k, v)] == ((k > 0 && m.rowof[v][1] >= 0) ? 1.0 : 0.0));
        }
    for (int k = 0; k < N; ++k) {
        EXPECT(ulb[k] == (m.rowof[4][0] >= 0 ? 1.0 : 0.0));
        EXPECT(uub[k] == (m.rowof[4][1] >= 0 ? 1.0 : 0.0));
    }
    // duals: every entry its own value; the rows pick theirs, scaled
    std::vector<double> lx((size_t)(N + 1) * 8), lu((size_t)N * 2), lp(mp);
    for (size_t i = 0; i < lx.size(); ++i) lx[i] = 1000.0 + (double)i;
    for (size_t i = 0; i < lu.size(); ++i) lu[i] = 5000.0 + (double)i;
    for (size_t i = 0; i < lp.size(); ++i) lp[i] = 9000.0 + (double)i;
    for (int k = 1; k <= N; ++k)
        for (int i = 0; i < ms; ++i) {
            const double got = nmpc_stage_dual(m, N, mx, mu, nmpc_stage_row(mx, mu, k, i), lx.data(), lu.data(), lp.data());
            const double want = i < mx ? (1000.0 + 8 * k + 4 * m.side[i] + m.var[i]) / m.scale[i]
                                       : (5000.0 + 2 * (k - 1) + m.side[i]) / m.scale[i];
            EXPECT(got == want);
        }
    for (int r = 0; r < mp; ++r)
        EXPECT(nmpc_stage_dual(m, N, mx, mu, nmpc_term_row(N, mx, mu, r), lx.data(), lu.data(), lp.data()) == 9000.0 + r);
    EXPECT(nmpc_lamx_index(N, 1, 3) == 8 * N + 7 && nmpc_lamu_index(N - 1, 1) == 2 * N - 1);
}

int main() {
    const size_t Ns[] = {1, 2, 64, 100, 127}, Bs[] = {1, 257};
    for (size_t N : Ns)
        for (size_t B : Bs) {
            check_layout(B, N, 616);
            check_layout(B, N, 0);
        }
    {   // N = 100 with the 616-row terminal set: 9,915 doubles and 3 ints per instance (79 KB), so
        // 4,096 instances take 325 MB where the dense route's Nwork takes 7.5 GB
        const NworkStage L1(1, 100, 616, 1616, NTRIAL, sizeof(NmpcBoundMap));
        const NworkStage L2(2, 100, 616, 1616, NTRIAL, sizeof(NmpcBoundMap));
        EXPECT(L2.bytes - L1.bytes == 9915 * D + 3 * I);
        const NworkStage L(4096, 100, 616, 1616, NTRIAL, sizeof(NmpcBoundMap));
        EXPECT(L.bytes / 1000000 == 325);
        const Nwork Ld(4096, 100, 1616, NTRIAL);
        EXPECT(Ld.bytes / 1000000000 == 7);
    }
    check_bound_map();
    {
        double Fx[8 * 4] = {0}, Fu[2] = {1.0, -1.0};
        for (int v = 0; v < 4; ++v) { Fx[v + 8 * v] = 1.0; Fx[4 + v + 8 * v] = -1.0; }
        NmpcBoundMap unit, part;
        nmpc_bound_map_build(Fx, 8, Fu, 2, &unit);
        const int pv[6] = {2, 0, 3, 0, 1, 2}, ps[6] = {0, 1, 1, 0, 1, 1};
        const double sc[6] = {2.0, 0.5, 3.0, 0.7, 1.0, 1.3};
        std::vector<double> G(6 * 4, 0.0);
        for (int i = 0; i < 6; ++i) G[i + 6 * pv[i]] = ps[i] ? sc[i] : -sc[i];
        const double Gu[1] = {-2.5};
        nmpc_bound_map_build(G.data(), 6, Gu, 1, &part);
        const int Nm[] = {1, 2, 64, 127};
        for (int N : Nm) {
            check_maps(N, 8, 2, 616, unit);
            check_maps(N, 8, 2, 0, unit);
            check_maps(N, 6, 1, 616, part);
        }
    }
    printf("nmpc_stage_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
