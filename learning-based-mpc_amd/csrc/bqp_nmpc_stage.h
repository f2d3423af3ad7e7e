// bqp_nmpc_stage.h — the index arithmetic of the nonlinear MPC's stage route
// (bqp_nmpc_dims.subproblem = 1): the bound map that turns the rows of F_x and F_u into plain
// bounds of the stage problem, where a row's bound lies in the structured solve's bound arrays,
// and the order map between that solve's multipliers (lam_x, lam_u, lam_p) and the NMPC rows.
//
// Plain C++ that compiles for the host and the device: the kernels of bqp_nmpc.hip call these
// functions, tests/host/nmpc_stage_check.cpp calls them on exactly sized heap buffers under the
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

constexpr int NMS_MAXMX = 32, NMS_MAXMU = 8;   // = NMPC_MAXMX, NMPC_MAXMU (bqp_internal.h)
constexpr int NMS_MAXROWS = NMS_MAXMX + NMS_MAXMU;
constexpr int NMS_NVAR = 5;                    // x1..x4, then u

// Rows i < mx are F_x's, rows mx <= i < mx + mu are F_u's.  Written once per solve by
// nmpc_stage_table_kernel, read by the stage linearisation and the back-map.  NmpcBoundBox is the
// part the hard route reads (its kernels hold and copy this part alone); NmpcBoundMap adds the soft
// state rows' members.
struct NmpcBoundBox {
    int notbox;                  // 1: a row is no bound (not exactly one non-zero entry, or that
                                 // entry is not finite) or a (variable, side) has two rows
    int var[NMS_MAXROWS];        // the row's variable: 0..3 a state, 4 the input
    int side[NMS_MAXROWS];       // 0: lower bound (negative entry), 1: upper bound
    int rowof[NMS_NVAR][2];      // the row of (variable, side), -1: none
    double scale[NMS_MAXROWS];   // |entry|: a x <= h is the bound x <= h / a
};

// Soft state rows (bqp_nmpc_data.xs_lin / xs_quad, one weight pair per row of F_x): row i with
// l1 > 0 or l2 > 0 may be violated by a slack s >= 0 at the price phi(s) = l1 s + 0.5 l2 s^2.
// The structured solve softens a (stage, variable) with one pair for both sides, in the variable's
// units: the row a (x_v - x_eq,v) <= h has the slack s / |a| there, so its pair is (l1 |a|, l2 a^2).
struct NmpcBoundMap : NmpcBoundBox {
    int unsupported;             // 1: a state variable has one row softened and the other hard, or
                                 // its two rows give different pairs
    int anysoft;                 // 1: some row of F_x is softened
    int soft[NMS_MAXROWS];       // 1: the row is softened (rows of F_u never are)
    double l1[NMS_MAXROWS];      // the row's weights, 0 for a hard row
    double l2[NMS_MAXROWS];
};

// Fx mx x 4 column-major, Fu mu.  Returns notbox; on 1 the map's other members are unspecified
// but every index in them is in range
BQP_HD inline int nmpc_bound_map_build(const double* Fx, int mx, const double* Fu, int mu, NmpcBoundBox* m) {
    int bad = (mx < 0 || mx > NMS_MAXMX || mu < 0 || mu > NMS_MAXMU) ? 1 : 0;
    for (int v = 0; v < NMS_NVAR; ++v) m->rowof[v][0] = m->rowof[v][1] = -1;
    for (int i = 0; i < NMS_MAXROWS; ++i) { m->var[i] = 0; m->side[i] = 0; m->scale[i] = 1.0; }
    if (!bad) {
        for (int i = 0; i < mx + mu; ++i) {
            int nz = 0, var = 0;
            double a = 0.0;
            if (i < mx) {
                for (int c = 0; c < 4; ++c) {
                    const double e = Fx[i + (int64_t)mx * c];
                    if (e != 0.0) { ++nz; var = c; a = e; }     // a NaN counts as an entry
                }
            } else {
                a = Fu[i - mx];
                var = 4;
                nz = a != 0.0 ? 1 : 0;
            }
            const double mag = a < 0.0 ? -a : a;
            if (nz != 1 || !(mag > 0.0) || !(mag * 0.0 == 0.0)) { bad = 1; continue; }   // one finite entry
            const int side = a > 0.0 ? 1 : 0;
            if (m->rowof[var][side] >= 0) { bad = 1; continue; }
            m->rowof[var][side] = i;
            m->var[i] = var;
            m->side[i] = side;
            m->scale[i] = mag;
        }
    }
    m->notbox = bad;
    return bad;
}

// NMPC row order: per stage k = 1..N the mx rows of F_x then the mu rows of F_u, then F_T
BQP_HD inline int64_t nmpc_stage_row(int mx, int mu, int k, int i) { return (int64_t)(mx + mu) * (k - 1) + i; }
BQP_HD inline int64_t nmpc_term_row(int N, int mx, int mu, int r) { return (int64_t)(mx + mu) * N + r; }

// the structured solve's arrays, per instance: xlb / xub (N+1) x 4 (stage 0 unused), ulb / uub N,
// lam_x (N+1) x [lower 4, upper 4], lam_u N x [lower, upper]
BQP_HD inline int nmpc_xb_index(int k, int v) { return 4 * k + v; }
BQP_HD inline int nmpc_lamx_index(int k, int side, int v) { return 8 * k + 4 * side + v; }
BQP_HD inline int nmpc_lamu_index(int k, int side) { return 2 * k + side; }

// row i of stage k (1..N) as a bound: which array (x: xub / xlb by side; u: uub / ulb) and where.
// A row of F_x bounds x_k, a row of F_u bounds u_{k-1}
BQP_HD inline bool nmpc_row_is_state(int mx, int i) { return i < mx; }
BQP_HD inline int nmpc_bound_index(const NmpcBoundBox& m, int mx, int k, int i) {
    return nmpc_row_is_state(mx, i) ? nmpc_xb_index(k, m.var[i]) : k - 1;
}
// the bound from the row's right-hand side at the iterate, rhs = h - F (v - v_eq) = -c
BQP_HD inline double nmpc_bound_value(const NmpcBoundBox& m, int i, double rhs) {
    const double q = rhs / m.scale[i];
    return m.side[i] ? q : -q;
}

// the multiplier of NMPC row r (0 <= r < N (mx + mu) + mp) from the structured solve's duals of
// the instance
BQP_HD inline double nmpc_stage_dual(const NmpcBoundBox& m, int N, int mx, int mu, int64_t r,
                                     const double* lam_x, const double* lam_u, const double* lam_p) {
    const int ms = mx + mu;
    const int64_t rT = (int64_t)ms * N;
    if (r >= rT) return lam_p[r - rT];
    const int k = (int)(r / ms) + 1, i = (int)(r % ms);
    const double lb = nmpc_row_is_state(mx, i) ? lam_x[nmpc_lamx_index(k, m.side[i], m.var[i])]
                                               : lam_u[nmpc_lamu_index(k - 1, m.side[i])];
    return lb / m.scale[i];
}

// ---- soft state rows ------------------------------------------------------------------------
// the penalty of a row slack s >= 0
BQP_HD inline double nmpc_phi(double l1, double l2, double s) { return l1 * s + 0.5 * l2 * s * s; }

// row i's weights in the structured solve's units: (xs_lin, xs_quad) = (l1 |a|, l2 a^2)
BQP_HD inline void nmpc_row_pair(const NmpcBoundMap& m, int i, double* lin, double* quad) {
    *lin = m.l1[i] * m.scale[i];
    *quad = m.l2[i] * m.scale[i] * m.scale[i];
}

// the pair of state variable v (0..3) from whichever of its rows is softened; false and (0, 0)
// where none is
BQP_HD inline bool nmpc_var_pair(const NmpcBoundMap& m, int v, double* lin, double* quad) {
    *lin = 0.0;
    *quad = 0.0;
    for (int sd = 0; sd < 2; ++sd) {
        const int i = m.rowof[v][sd];
        if (i >= 0 && m.soft[i]) { nmpc_row_pair(m, i, lin, quad); return true; }
    }
    return false;
}

// row slack <-> the structured solve's slack s_x of the row's (stage, side, variable); s_x has
// lam_x's layout
BQP_HD inline double nmpc_row_slack(const NmpcBoundBox& m, int i, double sx) { return m.scale[i] * sx; }
BQP_HD inline double nmpc_sx_of_row_slack(const NmpcBoundBox& m, int i, double s) { return s / m.scale[i]; }
BQP_HD inline int nmpc_sx_index(const NmpcBoundBox& m, int k, int i) { return nmpc_lamx_index(k, m.side[i], m.var[i]); }

// The soft members of a built map from the row weights (mx each; a null array is zeros).  Returns
// `unsupported`.  A variable with a single row may be softened; the rows of a map that is no box
// are left hard.
BQP_HD inline int nmpc_bound_map_soften(NmpcBoundMap* m, int mx, const double* xs_lin, const double* xs_quad) {
    int bad = 0, any = 0;
    for (int i = 0; i < NMS_MAXROWS; ++i) { m->soft[i] = 0; m->l1[i] = 0.0; m->l2[i] = 0.0; }
    if (!m->notbox && mx >= 0 && mx <= NMS_MAXMX) {
        for (int i = 0; i < mx; ++i) {
            const double a = xs_lin ? xs_lin[i] : 0.0, q = xs_quad ? xs_quad[i] : 0.0;
            if (a > 0.0 || q > 0.0) { m->soft[i] = 1; m->l1[i] = a; m->l2[i] = q; any = 1; }
        }
        for (int v = 0; v < 4; ++v) {
            const int lo = m->rowof[v][0], up = m->rowof[v][1];
            if (lo < 0 || up < 0) continue;
            if (m->soft[lo] != m->soft[up]) { bad = 1; continue; }
            if (!m->soft[lo]) continue;
            double al, aq, bl, bq;
            nmpc_row_pair(*m, lo, &al, &aq);
            nmpc_row_pair(*m, up, &bl, &bq);
            if (al != bl || aq != bq) bad = 1;
        }
    }
    m->unsupported = bad;
    m->anysoft = any;
    return bad;
}

}  // namespace bqp
