// Device check of the Riccati sweeps' loops as bqp_ocp.hip has them since round 10 (fp64): operands
// reached through per-lane offsets that walk with the stage (no stage index turned into an address
// inside the loop), the clamp of the refills gone by peeling the last stage pair, and the two store
// forms: the guarded store of row 0 (lane < NS; two stages per lane) and the store from all lanes
// (every 16-lane row runs the recursion on entry min(lane mod 16, NS - 1); one stage per lane), the
// latter also with the peeled pair reached from the walked offsets (the (2, 2, 2) repair kernels).
// One wave per launch, LDS operands.  Each loop is compared bit for bit against a plain per-stage
// reference of the same recursion (one stage per trip, explicit broadcasts and fused multiply-adds,
// no register sets, no refills):
//  - (NS, NU) = (5, 1) and (4, 2); N = 1 (odd tail only), 2 (peeled pair only), 3, 4 (first trip
//    with refills), 5 and 20; backward and forward;
//  - the swept vectors in LDS, together with 16 words in front of and behind them and the stages
//    the sweep does not write, which must keep the fill pattern;
//  - every lane's accumulator of every stage: row 0's lanes < NS in the guarded form, every lane
//    of every row in the all-lane form.
// Printed, not asserted: s_memtime cycles of the 20-stage sweeps in the three forms.
// Built by learning-based-mpc_amd/Makefile (build/sweep_walk_check), run by
// tests/test_gpu_sweep_walk.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "bqp_wave.h"

using bqp::fmac_rbc_chain;
using bqp::rbc_all;

#define CK(x) do { if ((x) != hipSuccess) { printf("HIP error at line %d\n", __LINE__); return 2; } } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static double rnd() {   // uniform in (-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(rng_state >> 11) / 4503599627370496.0 - 1.0;
}

constexpr int NMAX = 20;
constexpr int GUARD = 16;
// operand block in LDS, as the kernel's workspace: A (NS x NS), B (NS x NU), K (N x NU x NS),
// rhs (N x NS: qh_k backward, f_k forward), start (NS), a guard, the swept vectors
// ((N + 1) x NS), a guard
template <int NS, int NU>
struct Off {
    static constexpr int A = 0, B = A + NS * NS, K = B + NS * NU, R = K + NMAX * NU * NS,
                         S = R + NMAX * NS, G0 = S + NS, V = G0 + GUARD, G1 = V + (NMAX + 1) * NS,
                         END = G1 + GUARD;
    static constexpr int OUT = END - G0;            // words compared: guard, vectors, guard
};

// MODE 0: the plain reference; 1: walked offsets, guarded store; 2: walked offsets, all-lane store;
// 3: as 2 with the peeled pair and the odd stage reached from the walked offsets and the entry
// index formed per sweep (SWEEP_TAIL_WALK: the (2, 2, 2) repair kernels).
// DUMP: also every lane's accumulator of the stage stored as k, to dump[k][lane] (global memory);
// the vectors compared and the cycles come from the runs without it
template <int NS, int NU, int MODE, bool FWD, bool DUMP>
__device__ __forceinline__ void sweep(double* W, int N, int lane, double* dump) {
    using O = Off<NS, NU>;
    auto Abar = [&](int r, int c) { return W[O::A + r * NS + c]; };
    auto Bbar = [&](int r, int x) { return W[O::B + r * NU + x]; };
    constexpr bool ROWS = MODE >= 2, TAILW = MODE == 3;
    const int li = lane < NS ? lane : NS - 1;
    const int lx = ROWS ? ((lane & 15) < NS ? (lane & 15) : NS - 1) : li;
    constexpr int KS = NU * NS;
    if constexpr (MODE == 0 && !FWD) {
        double p[NS];
        for (int i = 0; i < NS; ++i) p[i] = W[O::S + i];
        for (int k = N - 1; k >= 0; --k) {
            double acc = W[O::R + k * NS + li];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                double ph = Abar(c, li);
#pragma unroll
                for (int x = 0; x < NU; ++x) ph = __builtin_fma(Bbar(c, x), W[O::K + k * KS + x * NS + li], ph);
                acc = __builtin_fma(ph, p[c], acc);
            }
            if constexpr (DUMP) dump[k * 64 + lane] = acc;
            if (lane < NS) W[O::V + k * NS + lane] = acc;
            rbc_all<0, NS>(acc, p);
        }
    } else if constexpr (MODE == 0 && FWD) {
        double d[NS];
        for (int i = 0; i < NS; ++i) d[i] = W[O::S + i];
        for (int k = 0; k < N; ++k) {
            double acc = W[O::R + k * NS + li];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                double ph = Abar(li, c);
#pragma unroll
                for (int x = 0; x < NU; ++x) ph = __builtin_fma(Bbar(li, x), W[O::K + k * KS + x * NS + c], ph);
                acc = __builtin_fma(ph, d[c], acc);
            }
            if constexpr (DUMP) dump[(k + 1) * 64 + lane] = acc;
            if (lane < NS) W[O::V + (k + 1) * NS + lane] = acc;
            rbc_all<0, NS>(acc, d);
        }
    } else if constexpr (!FWD) {
        // backward sweep as bqp_ocp.hip has it (fp64, one model)
        double Acol[NS], Bl[NS][NU];
        for (int c = 0; c < NS; ++c) {
            Acol[c] = Abar(c, lx);
            for (int x = 0; x < NU; ++x) Bl[c][x] = Bbar(c, x);
        }
        double pv = W[O::S + lx];
        auto store_b = [&](int o) __attribute__((always_inline)) {
            if constexpr (DUMP) dump[(o - (O::V + lx)) / NS * 64 + lane] = pv;
            if constexpr (ROWS) W[o] = pv;
            else if (lane < NS) W[o] = pv;
        };
        auto load_k = [&](int o, double (&kc)[NU]) __attribute__((always_inline)) {
#pragma unroll
            for (int x = 0; x < NU; ++x) kc[x] = W[o + x * NS];
        };
        const int bK = O::K + lx, bQ = O::R + lx, bS = O::V + lx;
        double k0[NU], q0, k1[NU], q1;
        load_k(bK + (N - 1) * KS, k0);
        q0 = W[bQ + (N - 1) * NS];
        const int kn = max(N - 2, 0);
        load_k(bK + kn * KS, k1);
        q1 = W[bQ + kn * NS];
        auto step_b = [&](int o, const double (&kc)[NU], double q) __attribute__((always_inline)) {
            double ph[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                ph[c] = Acol[c];
#pragma unroll
                for (int x = 0; x < NU; ++x) ph[c] += Bl[c][x] * kc[x];
            }
            pv = fmac_rbc_chain(q, pv, ph);
            store_b(o);
        };
        int oK = bK + (N - 4) * KS, oQ = bQ + (N - 4) * NS, oS = bS + (N - 4) * NS;
        int k = N - 1;
        for (; k >= 3; k -= 2) {
            step_b(oS + 3 * NS, k0, q0);
            load_k(oK + KS, k0);
            q0 = W[oQ + NS];
            step_b(oS + 2 * NS, k1, q1);
            load_k(oK, k1);
            q1 = W[oQ];
            oK -= 2 * KS;
            oQ -= 2 * NS;
            oS -= 2 * NS;
        }
        if constexpr (TAILW) {
            const int z = 3 - k;                         // the offsets stand at stage k - 3
            if (N >= 2) {
                step_b(oS + 3 * NS, k0, q0);
                load_k(oK + z * KS, k0);
                q0 = W[oQ + z * NS];
                step_b(oS + 2 * NS, k1, q1);
            }
            if (N & 1) step_b(oS + z * NS, k0, q0);
        } else {
        if (N >= 2) {
            const int kl = 1 + (N & 1);
            step_b(bS + kl * NS, k0, q0);
            load_k(bK, k0);
            q0 = W[bQ];
            step_b(bS + (kl - 1) * NS, k1, q1);
        }
        if (N & 1) step_b(bS, k0, q0);
        }
    } else {
        // forward sweep as bqp_ocp.hip has it (fp64, one model)
        double dv = W[O::S + lx];
        double Arow[NS], Bli[NU];
        for (int c = 0; c < NS; ++c) Arow[c] = Abar(lx, c);
        for (int x = 0; x < NU; ++x) Bli[x] = Bbar(lx, x);
        auto store_f = [&](int o) __attribute__((always_inline)) {
            if constexpr (DUMP) dump[(o - (O::V + lx)) / NS * 64 + lane] = dv;
            if constexpr (ROWS) W[o] = dv;
            else if (lane < NS) W[o] = dv;
        };
        auto load_kw = [&](int o, double (&kr)[NU][NS]) __attribute__((always_inline)) {
#pragma unroll
            for (int x = 0; x < NU; ++x)
#pragma unroll
                for (int c = 0; c < NS; ++c) kr[x][c] = W[o + x * NS + c];
        };
        int bK = O::K;
        asm volatile("" : "+v"(bK));
        const int bF = O::R + lx, bS = O::V + lx;
        double k0[NU][NS], f0, k1[NU][NS], f1;
        load_kw(bK, k0);
        f0 = W[bF];
        const int kn = min(1, N - 1);
        load_kw(bK + kn * KS, k1);
        f1 = W[bF + kn * NS];
        auto step_f = [&](int o, const double (&kr)[NU][NS], double f) __attribute__((always_inline)) {
            double ph[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                ph[c] = Arow[c];
#pragma unroll
                for (int x = 0; x < NU; ++x) ph[c] += Bli[x] * kr[x][c];
            }
            dv = fmac_rbc_chain(f, dv, ph);
            store_f(o);
        };
        int oK = bK, oF = bF, oS = bS;
        int k = 0;
        for (; k + 3 < N; k += 2) {
            step_f(oS + NS, k0, f0);
            load_kw(oK + 2 * KS, k0);
            f0 = W[oF + 2 * NS];
            step_f(oS + 2 * NS, k1, f1);
            load_kw(oK + 3 * KS, k1);
            f1 = W[oF + 3 * NS];
            oK += 2 * KS;
            oF += 2 * NS;
            oS += 2 * NS;
        }
        if constexpr (TAILW) {
            const int z = N - 1 - k;                     // the offsets stand at stage k
            if (N >= 2) {
                step_f(oS + NS, k0, f0);
                load_kw(oK + z * KS, k0);
                f0 = W[oF + z * NS];
                step_f(oS + 2 * NS, k1, f1);
            }
            if (N & 1) step_f(oS + (z + 1) * NS, k0, f0);
        } else {
        if (N >= 2) {
            const int kl = N - 2 - (N & 1);
            step_f(bS + (kl + 1) * NS, k0, f0);
            load_kw(bK + (N - 1) * KS, k0);
            f0 = W[bF + (N - 1) * NS];
            step_f(bS + (kl + 2) * NS, k1, f1);
        }
        if (N & 1) step_f(bS + N * NS, k0, f0);
        }
    }
}

// out: guard, swept vectors, guard (Off::OUT words, from LDS); dump: (NMAX + 1) x 64 accumulators
template <int NS, int NU, int MODE, bool FWD, bool DUMP>
__global__ void __launch_bounds__(64) k_run(const double* in, int N, uint64_t* out, double* dump,
                                            unsigned long long* cyc) {
    using O = Off<NS, NU>;
    __shared__ double W[O::END];
    const int lane = threadIdx.x;
    for (int i = lane; i < O::G0; i += 64) W[i] = in[i];
    for (int i = O::G0 + lane; i < O::END; i += 64) W[i] = __builtin_bit_cast(double, ~0ull);
    bqp::wave_sync();
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    sweep<NS, NU, MODE, FWD, DUMP>(W, N, lane, dump);
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    bqp::wave_sync();
    if constexpr (!DUMP) {
        for (int i = lane; i < O::OUT; i += 64) out[i] = __builtin_bit_cast(uint64_t, W[O::G0 + i]);
        if (lane == 0) cyc[0] = t1 - t0;
    }
}

template <int NS, int NU>
static int run(double* d_in, uint64_t* d_out, double* d_dump, unsigned long long* d_cyc, int* diff,
               unsigned long long (&cycles)[2][4]) {
    using O = Off<NS, NU>;
    static double h[O::G0];
    static uint64_t o[4][O::OUT];
    static uint64_t dmp[4][(NMAX + 1) * 64];
    for (int i = 0; i < O::G0; ++i) h[i] = rnd() * (i < O::K ? 0.5 : (i < O::R ? 0.25 : 1.0));
    CK(hipMemcpy(d_in, h, sizeof h, hipMemcpyHostToDevice));
    const int Ns[6] = {1, 2, 3, 4, 5, 20};
    for (int fwd = 0; fwd < 2; ++fwd)
        for (int n = 0; n < 6; ++n) {
            const int N = Ns[n];
            for (int m = 0; m < 4; ++m) {
                CK(hipMemset(d_out, 0, sizeof o[0]));
                CK(hipMemset(d_dump, 0xff, sizeof dmp[0]));
#define LAUNCH(MODE, FWD) \
    hipLaunchKernelGGL((k_run<NS, NU, MODE, FWD, false>), dim3(1), dim3(64), 0, 0, d_in, N, d_out, d_dump, d_cyc); \
    hipLaunchKernelGGL((k_run<NS, NU, MODE, FWD, true>), dim3(1), dim3(64), 0, 0, d_in, N, d_out, d_dump, d_cyc)
                if (fwd) { if (m == 0) { LAUNCH(0, true); } else if (m == 1) { LAUNCH(1, true); } else if (m == 2) { LAUNCH(2, true); } else { LAUNCH(3, true); } }
                else { if (m == 0) { LAUNCH(0, false); } else if (m == 1) { LAUNCH(1, false); } else if (m == 2) { LAUNCH(2, false); } else { LAUNCH(3, false); } }
#undef LAUNCH
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(o[m], d_out, sizeof o[0], hipMemcpyDeviceToHost));
                CK(hipMemcpy(dmp[m], d_dump, sizeof dmp[0], hipMemcpyDeviceToHost));
                if (N == 20) CK(hipMemcpy(&cycles[fwd][m], d_cyc, sizeof(unsigned long long), hipMemcpyDeviceToHost));
            }
            // stages written: backward k = 0 .. N - 1, forward k = 1 .. N
            const int lo = fwd ? 1 : 0, hi = fwd ? N : N - 1;
            int d = 0;
            for (int i = 0; i < O::OUT; ++i) {
                const int v = i - GUARD;                       // word of the swept vectors
                const bool written = v >= lo * NS && v < (hi + 1) * NS;
                if (written ? (o[0][i] == ~0ull) : (o[0][i] != ~0ull)) ++d;   // the reference itself
                if (o[1][i] != o[0][i]) ++d;
                if (o[2][i] != o[0][i]) ++d;
                if (o[3][i] != o[0][i]) ++d;
            }
            for (int k = lo; k <= hi; ++k) {
                for (int l = 0; l < NS; ++l)                   // guarded form: row 0's lanes < NS
                    if (dmp[1][k * 64 + l] != o[0][GUARD + k * NS + l]) ++d;
                for (int l = 0; l < 64; ++l) {                 // all-lane form: every lane of every row
                    const int e = (l & 15) < NS ? (l & 15) : NS - 1;
                    if (dmp[2][k * 64 + l] != o[0][GUARD + k * NS + e]) ++d;
                    if (dmp[3][k * 64 + l] != o[0][GUARD + k * NS + e]) ++d;
                }
            }
            if (d) printf("NS %d NU %d %s N %d: %d words differ\n", NS, NU, fwd ? "forward" : "backward", N, d);
            *diff += d;
        }
    return 0;
}

int main() {
    double* d_in;
    uint64_t* d_out;
    double* d_dump;
    unsigned long long* d_cyc;
    CK(hipMalloc(&d_in, 4096 * sizeof(double)));
    CK(hipMalloc(&d_out, 4096 * sizeof(uint64_t)));
    CK(hipMalloc(&d_dump, (NMAX + 1) * 64 * sizeof(double)));
    CK(hipMalloc(&d_cyc, sizeof(unsigned long long)));
    int diff = 0;
    unsigned long long c51[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, c42[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
    if (run<5, 1>(d_in, d_out, d_dump, d_cyc, &diff, c51)) return 2;
    if (run<4, 2>(d_in, d_out, d_dump, d_cyc, &diff, c42)) return 2;
    printf("walked sweeps: 2 families x 2 sweeps x 6 horizons x 3 forms, %d differ\n", diff);
    printf("cycles, 20 stages, NS 5 NU 1: backward plain %llu guarded %llu all-lane %llu tail-walk %llu, forward plain %llu guarded %llu all-lane %llu tail-walk %llu\n",
           c51[0][0], c51[0][1], c51[0][2], c51[0][3], c51[1][0], c51[1][1], c51[1][2], c51[1][3]);
    printf("cycles, 20 stages, NS 4 NU 2: backward plain %llu guarded %llu all-lane %llu tail-walk %llu, forward plain %llu guarded %llu all-lane %llu tail-walk %llu\n",
           c42[0][0], c42[0][1], c42[0][2], c42[0][3], c42[1][0], c42[1][1], c42[1][2], c42[1][3]);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_dump);
    (void)hipFree(d_cyc);
    return diff ? 1 : 0;
}
