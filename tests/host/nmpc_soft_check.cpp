// Stand-alone check of the soft state rows of the nonlinear MPC's stage route
// (csrc/bqp_nmpc_stage.h: the map's soft members, the weight pairs, the slack maps, phi) and of the
// workspace members that go with them (csrc/bqp_layout.h, NworkStage with soft = 1): the Makefile
// builds it with g++ -std=c++17 -fsanitize=address,undefined (build/nmpc_soft_check),
// tests/test_host_nmpc_soft.py runs it.
//
//   - the pairing rule: both rows of a variable softened with equal pairs in the variable's units,
//     and the refusals (one side soft, unequal pairs after scaling); scaled rows a = 2 and
//     a = -0.5 map to equal structured pairs exactly when the row weights are l1 / |a|, l2 / a^2;
//   - the weight tables, the penalty at the iterate and the model penalty from s_x, as the kernels
//     index them, at N = 1, 2, 64, 127 on heap buffers of exactly the documented sizes;
//   - the layout with soft = 1 at batch 1 and 257: the new regions sized from the shapes, every
//     region aligned, disjoint and inside `bytes`; soft = 0 is the layout of before.
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

static void check_layout(size_t B, size_t N, size_t mp) {
    const size_t n = N + 1, m = 10 * N + mp, MB = sizeof(NmpcBoundMap);
    const NworkStage H(B, N, mp, m, NTRIAL, MB), H0(B, N, mp, m, NTRIAL, MB, 0), L(B, N, mp, m, NTRIAL, MB, 1);
    EXPECT(H.bytes == H0.bytes);
    EXPECT(H.xsl.bytes == 0 && H.xsq.bytes == 0 && H.sx.bytes == 0 && H.pen0.bytes == 0 && H.plin.bytes == 0);
    EXPECT(L.xsl.bytes == n * 4 * D && L.xsq.bytes == n * 4 * D);
    EXPECT(L.sx.bytes == B * n * 8 * D && L.sx.bytes == L.lamx.bytes);
    EXPECT(L.pen0.bytes == B * D && L.plin.bytes == B * D);
    EXPECT(L.bytes == H.bytes + (2 * n * 4 + B * n * 8 + 2 * B) * D);
    const Region rs[] = {L.A, L.B, L.w, L.xlb, L.xub, L.ulb, L.uub, L.hp, L.xo, L.uo, L.tho, L.fv, L.lamx,
                         L.lamu, L.lamp, L.rhs, L.lam, L.d, L.f, L.ctl, L.cost0, L.costT, L.violT, L.stat,
                         L.cprev, L.nu, L.xsl, L.xsq, L.sx, L.pen0, L.plin, L.W, L.Fp, L.x0z, L.map,
                         L.sflag, L.qpflag, L.done, L.ndone};
    const size_t R = sizeof(rs) / sizeof(rs[0]);
    size_t sum = 0;
    for (size_t i = 0; i < R; ++i) {
        EXPECT(rs[i].off % (i + 4 < R ? D : I) == 0);
        EXPECT(rs[i].off + rs[i].bytes <= L.bytes);
        sum += rs[i].bytes;
        for (size_t j = i + 1; j < R; ++j)
            EXPECT(rs[i].off + rs[i].bytes <= rs[j].off || rs[j].off + rs[j].bytes <= rs[i].off);
    }
    EXPECT(sum == L.bytes);
    EXPECT(L.ndone.off == L.done.off + B * I);
    EXPECT(MB % D == 0 && sizeof(NmpcBoundBox) % D == 0);
}

// F_x = [diag(up); -diag(lo)] (8 rows), F_u = [1; -1]
static void build(const double (&up)[4], const double (&lo)[4], NmpcBoundMap* m) {
    double Fx[8 * 4] = {0}, Fu[2] = {1.0, -1.0};
    for (int v = 0; v < 4; ++v) { Fx[v + 8 * v] = up[v]; Fx[4 + v + 8 * v] = -lo[v]; }
    EXPECT(nmpc_bound_map_build(Fx, 8, Fu, 2, m) == 0);
}

static void check_pairing() {
    const double one[4] = {1, 1, 1, 1};
    NmpcBoundMap m;
    build(one, one, &m);
    // no weights: all hard
    EXPECT(nmpc_bound_map_soften(&m, 8, nullptr, nullptr) == 0 && m.unsupported == 0 && m.anysoft == 0);
    for (int i = 0; i < NMS_MAXROWS; ++i) EXPECT(m.soft[i] == 0 && m.l1[i] == 0.0 && m.l2[i] == 0.0);
    const double z8[8] = {0};
    EXPECT(nmpc_bound_map_soften(&m, 8, z8, z8) == 0 && m.anysoft == 0);
    // all eight rows, equal weights; one array null = zeros
    const double a8[8] = {100, 100, 100, 100, 100, 100, 100, 100}, q8[8] = {1e3, 1e3, 1e3, 1e3, 1e3, 1e3, 1e3, 1e3};
    EXPECT(nmpc_bound_map_soften(&m, 8, a8, q8) == 0 && m.anysoft == 1);
    for (int i = 0; i < 8; ++i) EXPECT(m.soft[i] == 1 && m.l1[i] == 100.0 && m.l2[i] == 1e3);
    EXPECT(m.soft[8] == 0 && m.soft[9] == 0);                       // the rows of F_u never
    EXPECT(nmpc_bound_map_soften(&m, 8, a8, nullptr) == 0 && m.anysoft == 1 && m.l2[3] == 0.0 && m.soft[3] == 1);
    EXPECT(nmpc_bound_map_soften(&m, 8, nullptr, q8) == 0 && m.anysoft == 1 && m.l1[3] == 0.0 && m.soft[3] == 1);
    // x2 alone, both sides: fine, the other variables hard
    double a[8] = {0}, q[8] = {0};
    a[1] = a[5] = 5.0; q[1] = q[5] = 50.0;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 0 && m.anysoft == 1);
    double lin, quad;
    EXPECT(nmpc_var_pair(m, 1, &lin, &quad) && lin == 5.0 && quad == 50.0);
    EXPECT(!nmpc_var_pair(m, 0, &lin, &quad) && lin == 0.0 && quad == 0.0);
    // one side soft, the other hard
    a[5] = 0.0; q[5] = 0.0;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 1 && m.unsupported == 1);
    // unequal pairs
    a[5] = 5.0; q[5] = 49.0;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 1);
    a[5] = 4.0; q[5] = 50.0;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 1);
    // scaled rows: upper row of x2 times 2, lower row times 0.5 (entry -0.5)
    const double up[4] = {1, 2, 1, 1}, lo[4] = {1, 0.5, 1, 1};
    build(up, lo, &m);
    EXPECT(m.scale[1] == 2.0 && m.scale[5] == 0.5);
    a[1] = 5.0 / 2.0; q[1] = 50.0 / 4.0; a[5] = 5.0 / 0.5; q[5] = 50.0 / 0.25;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 0);
    EXPECT(nmpc_var_pair(m, 1, &lin, &quad) && lin == 5.0 && quad == 50.0);
    double l5, q5;
    nmpc_row_pair(m, 5, &l5, &q5);
    EXPECT(l5 == 5.0 && q5 == 50.0);
    // the unscaled weights on the scaled rows: pairs (10, 200) and (2.5, 12.5)
    a[1] = a[5] = 5.0; q[1] = q[5] = 50.0;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 1);
    // the linear weight scaled, the quadratic not
    a[1] = 2.5; a[5] = 10.0;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 1);
    // a variable with a single row may be softened
    double G[3 * 4] = {0};
    G[0 + 3 * 1] = -2.0; G[1 + 3 * 0] = 1.0; G[2 + 3 * 0] = -1.0;   // x2 >= ., x1 both sides
    EXPECT(nmpc_bound_map_build(G, 3, nullptr, 0, &m) == 0);
    const double a3[3] = {7.0, 0, 0}, q3[3] = {3.0, 0, 0};
    EXPECT(nmpc_bound_map_soften(&m, 3, a3, q3) == 0 && m.anysoft == 1 && m.soft[0] == 1 && m.soft[1] == 0);
    EXPECT(nmpc_var_pair(m, 1, &lin, &quad) && lin == 14.0 && quad == 12.0);
    // a map that is no box stays hard
    G[0 + 3 * 0] = 0.3;
    EXPECT(nmpc_bound_map_build(G, 3, nullptr, 0, &m) == 1);
    EXPECT(nmpc_bound_map_soften(&m, 3, a3, q3) == 0 && m.anysoft == 0);
    // phi and the slack maps
    EXPECT(nmpc_phi(100.0, 1000.0, 0.0) == 0.0 && nmpc_phi(100.0, 1000.0, 0.5) == 50.0 + 125.0);
    EXPECT(nmpc_phi(0.0, 0.0, 3.0) == 0.0);
    build(up, lo, &m);
    EXPECT(nmpc_row_slack(m, 1, 0.25) == 0.5 && nmpc_sx_of_row_slack(m, 1, 0.5) == 0.25);
    EXPECT(nmpc_row_slack(m, 5, 0.25) == 0.125 && nmpc_sx_of_row_slack(m, 5, 0.125) == 0.25);
    // the price is the same in either unit: phi_row(s) = phi_var(s / |a|) with the variable's pair
    a[1] = 2.5; q[1] = 12.5; a[5] = 10.0; q[5] = 200.0;
    EXPECT(nmpc_bound_map_soften(&m, 8, a, q) == 0);
    EXPECT(nmpc_phi(m.l1[1], m.l2[1], 0.5) == nmpc_phi(5.0, 50.0, nmpc_sx_of_row_slack(m, 1, 0.5)));
    EXPECT(nmpc_phi(m.l1[5], m.l2[5], 0.125) == nmpc_phi(5.0, 50.0, nmpc_sx_of_row_slack(m, 5, 0.125)));
}

// the table kernel's stores, the stage rollout's penalty and the back-map's loads of s_x
static void check_tables(int N, const NmpcBoundMap& m, int mx, int mu) {
    const int ms = mx + mu;
    std::vector<double> xsl((size_t)4 * (N + 1), -1.0), xsq((size_t)4 * (N + 1), -1.0);
    for (int i = 0; i < 4 * (N + 1); ++i) {
        double lin, quad;
        nmpc_var_pair(m, i & 3, &lin, &quad);
        xsl[(size_t)i] = i < 4 ? 0.0 : lin;
        xsq[(size_t)i] = i < 4 ? 0.0 : quad;
    }
    for (int k = 0; k <= N; ++k)
        for (int v = 0; v < 4; ++v) {
            double lin, quad;
            const bool on = nmpc_var_pair(m, v, &lin, &quad);
            EXPECT(xsl[(size_t)nmpc_xb_index(k, v)] == (k > 0 && on ? lin : 0.0));
            EXPECT(xsq[(size_t)nmpc_xb_index(k, v)] == (k > 0 && on ? quad : 0.0));
        }
    // s_x in lam_x's layout, every entry its own value; the rows pick theirs, each entry at most once
    std::vector<double> sx((size_t)(N + 1) * 8);
    std::vector<int> hit(sx.size(), 0);
    for (size_t i = 0; i < sx.size(); ++i) sx[i] = 0.001 * (double)(i + 1);
    double plin = 0.0, want = 0.0;
    for (int r = 0; r < ms * N; ++r) {
        const int k = r / ms + 1, i = r % ms;
        if (i < mx && m.soft[i]) {
            const int at = nmpc_sx_index(m, k, i);
            EXPECT(at >= 8 && at < 8 * (N + 1));
            ++hit[(size_t)at];
            EXPECT(at == 8 * k + 4 * m.side[i] + m.var[i]);
            plin += nmpc_phi(m.l1[i], m.l2[i], nmpc_row_slack(m, i, sx[(size_t)at]));
            // the structured solve prices the same slack with the variable's pair
            double lin, quad;
            nmpc_var_pair(m, m.var[i], &lin, &quad);
            want += nmpc_phi(lin, quad, sx[(size_t)at]);
        }
    }
    for (int h : hit) EXPECT(h <= 1);
    EXPECT(fabs(plin - want) <= 1e-12 * (1.0 + want));
}

int main() {
    const size_t Ns[] = {1, 2, 64, 127}, Bs[] = {1, 257};
    for (size_t N : Ns)
        for (size_t B : Bs) {
            check_layout(B, N, 616);
            check_layout(B, N, 0);
        }
    check_pairing();
    {
        const double one[4] = {1, 1, 1, 1}, up[4] = {1, 2, 1, 3}, lo[4] = {1, 0.5, 1, 3};
        NmpcBoundMap unit, scaled;
        build(one, one, &unit);
        const double a8[8] = {100, 100, 0, 100, 100, 100, 0, 100}, q8[8] = {1e3, 1e3, 0, 1e3, 1e3, 1e3, 0, 1e3};
        EXPECT(nmpc_bound_map_soften(&unit, 8, a8, q8) == 0);
        build(up, lo, &scaled);
        const double as[8] = {0, 2.5, 0, 7.0, 0, 10.0, 0, 7.0}, qs[8] = {0, 12.5, 0, 2.0, 0, 200.0, 0, 2.0};
        EXPECT(nmpc_bound_map_soften(&scaled, 8, as, qs) == 0);
        const int Nm[] = {1, 2, 64, 127};
        for (int N : Nm) {
            check_tables(N, unit, 8, 2);
            check_tables(N, scaled, 8, 2);
        }
    }
    printf("nmpc_soft_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
