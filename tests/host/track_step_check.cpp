// Stand-alone check of csrc/bqp_track.h, the per-instance step of the closed loop with a reference
// schedule, on the workspace csrc/bqp_layout.h CworkTrack describes: the Makefile builds it with
// g++ -std=c++17 -fsanitize=address,undefined (build/track_step_check),
// tests/test_host_track_step.py runs it.
//
// For (nx, nu, np, N, nr) = (2, 2, 2, 3, 2) and (4, 1, 1, 20, 4), batch 3, 5 steps, with shared
// (stride 0) and per-instance model, schedule, disturbance and base term, and with a null
// disturbance and base term: the host side of the loop - w_0, then per step a made-up solve in
// the workspace, the record, the linear plant step and w_{t+1}, in the order of
// track_advance_kernel - runs on heap buffers of exactly the documented sizes (an index past
// one of them stops the program under the address sanitizer) and must equal a plain loop nest
// over (instance, step, entry) bit for bit.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "bqp_layout.h"
#include "bqp_track.h"

using bqp::TrackArgs;
namespace layout = bqp::layout;

static int failures = 0;
static long checks = 0;
static const char* what = "";

#define EXPECT(cond)                                                                  \
    do {                                                                              \
        ++checks;                                                                     \
        if (!(cond)) {                                                                \
            ++failures;                                                               \
            fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, what); \
        }                                                                             \
    } while (0)

// exactly n elements on the heap, filled with reproducible values in (-1, 1)
template <class T>
static T* heap(size_t n, unsigned& seed, bool fill) {
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    for (size_t i = 0; i < n; ++i) {
        seed = seed * 1664525u + 1013904223u;
        p[i] = fill ? (T)(((double)(seed >> 8) / (double)(1u << 24)) * 2.0 - 1.0) : (T)0;
    }
    return p;
}

// the made-up solve of step t: u (N x nu), theta and the exit flag of instance b
static double fake_u(int b, int t, int k) { return 0.125 * (b + 1) - 0.03125 * t + 0.5 * k; }
static double fake_th(int b, int t, int j) { return 0.25 * b + 0.0625 * t - j; }
static int fake_flag(int b, int t) { return (b + t) % 3 == 0 ? 0 : 1; }

static void run(int nx, int nu, int np, int N, int nr, bool shared, bool with_dist, bool with_base) {
    static char name[128];
    snprintf(name, sizeof(name), "nx %d nu %d np %d N %d nr %d %s%s%s", nx, nu, np, N, nr,
             shared ? "shared" : "per-instance", with_dist ? "" : ", no dist", with_base ? "" : ", no base");
    what = name;
    const int B = 3, S = 5, nv = nx + nu + np;
    const size_t nw = (size_t)(N + 1) * nv;
    unsigned seed = 12345u + (unsigned)(nx * 7 + N);
    const size_t per = shared ? 0 : 1;   // stride factor
    const size_t cnt = shared ? 1 : B;   // copies
    // inputs, each of exactly its documented size
    double* A = heap<double>(cnt * nx * nx, seed, true);
    double* Bm = heap<double>(cnt * nx * nu, seed, true);
    double* dist = with_dist ? heap<double>(cnt * S * nx, seed, true) : nullptr;
    double* wbase = with_base ? heap<double>(cnt * nw, seed, true) : nullptr;
    double* Wr = heap<double>(nw * nr, seed, true);
    double* ref = heap<double>(cnt * S * nr, seed, true);
    double* xeq = heap<double>(nx, seed, true);
    double* ueq = heap<double>(nu, seed, true);
    double* xinit = heap<double>((size_t)B * nx, seed, true);
    // outputs
    double* X = heap<double>((size_t)B * (S + 1) * nx, seed, false);
    double* U = heap<double>((size_t)B * S * nu, seed, false);
    double* TH = heap<double>((size_t)B * S * np, seed, false);
    int* F = heap<int>((size_t)B * S, seed, false);
    // the loop's workspace
    const layout::CworkTrack CL(B, nx, nu, np, N, nw);
    EXPECT(CL.s.bytes == sizeof(double) * B * nx && CL.w.bytes == sizeof(double) * B * nw);
    EXPECT(CL.u.bytes == sizeof(double) * B * N * nu && CL.theta.bytes == sizeof(double) * B * np);
    EXPECT(CL.flags.bytes == sizeof(int) * B && CL.flags.off + CL.flags.bytes == CL.bytes);
    EXPECT(CL.x.off == CL.s.off + CL.s.bytes && CL.w.off % sizeof(double) == 0);
    void* ws = malloc(CL.bytes);
    double* s = layout::at<double>(ws, CL.s);
    double* uo = layout::at<double>(ws, CL.u);
    double* th = layout::at<double>(ws, CL.theta);
    int* fl = layout::at<int>(ws, CL.flags);

    TrackArgs a = {};
    a.batch = B; a.nx = nx; a.nu = nu; a.np = np; a.N = N; a.steps = S; a.nr = nr;
    a.plant = 3; a.delta = 0.0; a.nw = (int64_t)nw;
    a.uo = uo; a.th = th; a.fl = fl; a.xeq = xeq; a.ueq = ueq;
    a.A = A; a.sA = (int64_t)(per * nx * nx); a.B = Bm; a.sB = (int64_t)(per * nx * nu);
    a.dist = dist; a.sdist = (int64_t)(per * S * nx);
    a.wbase = wbase; a.swbase = (int64_t)(per * nw);
    a.Wr = Wr; a.ref = ref; a.sref = (int64_t)(per * S * nr);
    a.s = s; a.w = layout::at<double>(ws, CL.w); a.X = X; a.U = U; a.THETA = TH; a.flags = F;

    // the plain loop nest: states, inputs, theta, flags and every step's linear term
    std::vector<double> Xr((size_t)B * (S + 1) * nx), Ur((size_t)B * S * nu), Tr((size_t)B * S * np);
    std::vector<double> Wt((size_t)S * B * nw);
    std::vector<int> Fr((size_t)B * S);
    for (int b = 0; b < B; ++b) {
        const double* Ab = A + (shared ? 0 : (size_t)b * nx * nx);
        const double* Bb = Bm + (shared ? 0 : (size_t)b * nx * nu);
        std::vector<double> dev(nx);
        for (int i = 0; i < nx; ++i) {
            Xr[(size_t)b * (S + 1) * nx + i] = xinit[(size_t)b * nx + i];
            dev[i] = xinit[(size_t)b * nx + i] - xeq[i];
        }
        for (int t = 0; t < S; ++t) {
            for (int k = 0; k < nu; ++k) Ur[((size_t)b * S + t) * nu + k] = fake_u(b, t, k) + ueq[k];
            for (int j = 0; j < np; ++j) Tr[((size_t)b * S + t) * np + j] = fake_th(b, t, j);
            Fr[(size_t)b * S + t] = fake_flag(b, t);
            std::vector<double> nxt(nx);
            for (int i = 0; i < nx; ++i) {
                double v = dist ? dist[(shared ? 0 : (size_t)b * S * nx) + (size_t)t * nx + i] : 0.0;
                for (int j = 0; j < nx; ++j) v += Ab[j * nx + i] * dev[j];
                for (int k = 0; k < nu; ++k) v += Bb[k * nx + i] * fake_u(b, t, k);
                nxt[i] = v + xeq[i];
            }
            for (int i = 0; i < nx; ++i) {
                Xr[((size_t)b * (S + 1) + t + 1) * nx + i] = nxt[i];
                dev[i] = nxt[i] - xeq[i];
            }
            for (size_t e = 0; e < nw; ++e) {
                double v = wbase ? wbase[(shared ? 0 : (size_t)b * nw) + e] : 0.0;
                for (int j = 0; j < nr; ++j)
                    v += Wr[(size_t)j * nw + e] * ref[(shared ? 0 : (size_t)b * S * nr) + (size_t)t * nr + j];
                Wt[((size_t)t * B + b) * nw + e] = v;
            }
        }
    }

    // the loop as the device runs it: init (closed_loop_init_kernel), w_0, then per step the
    // solve's outputs, every instance's record and plant step, every entry of w_{t+1}
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < nx; ++i) {
            s[(size_t)b * nx + i] = xinit[(size_t)b * nx + i] - xeq[i];
            X[bqp::track_x_at(a, b, 0) + i] = xinit[(size_t)b * nx + i];
        }
    for (int64_t i = 0; i < (int64_t)B * a.nw; ++i) bqp::track_w_entry(a, i, 0);
    for (int t = 0; t < S; ++t) {
        for (size_t i = 0; i < (size_t)B * nw; ++i) EXPECT(a.w[i] == Wt[(size_t)t * B * nw + i]);
        for (int b = 0; b < B; ++b) {
            for (int k = 0; k < N * nu; ++k) uo[(size_t)b * N * nu + k] = k < nu ? fake_u(b, t, k) : 1e300;
            for (int j = 0; j < np; ++j) th[(size_t)b * np + j] = fake_th(b, t, j);
            fl[b] = fake_flag(b, t);
        }
        for (int b = 0; b < B; ++b) {
            bqp::track_record(a, b, t);
            bqp::track_linear_step(a, b, t);
        }
        if (t + 1 < S)
            for (int64_t i = 0; i < (int64_t)B * a.nw; ++i) bqp::track_w_entry(a, i, t + 1);
    }
    for (size_t i = 0; i < Xr.size(); ++i) EXPECT(X[i] == Xr[i]);
    for (size_t i = 0; i < Ur.size(); ++i) EXPECT(U[i] == Ur[i]);
    for (size_t i = 0; i < Tr.size(); ++i) EXPECT(TH[i] == Tr[i]);
    for (size_t i = 0; i < Fr.size(); ++i) EXPECT(F[i] == Fr[i]);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < nx; ++i)
            EXPECT(s[(size_t)b * nx + i] == Xr[((size_t)b * (S + 1) + S) * nx + i] - xeq[i]);
    // null THETA / flags are skipped
    a.THETA = nullptr; a.flags = nullptr;
    bqp::track_record(a, 0, 0);

    free(ws); free(F); free(TH); free(U); free(X); free(xinit); free(ueq); free(xeq); free(ref);
    free(Wr); free(wbase); free(dist); free(Bm); free(A);
}

int main() {
    const int cfg[2][5] = {{2, 2, 2, 3, 2}, {4, 1, 1, 20, 4}};   // nx, nu, np, N, nr
    for (const auto& c : cfg)
        for (int shared = 0; shared < 2; ++shared) {
            run(c[0], c[1], c[2], c[3], c[4], shared != 0, false, false);   // NULL dist (and base)
            run(c[0], c[1], c[2], c[3], c[4], shared != 0, true, true);
        }
    printf("track_step_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
