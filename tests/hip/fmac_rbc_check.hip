// Device check of fmac_rbc / fmac_rbc_seq / fmac_rbc_chain (bqp_wave.h): the fp64 multiply-add
// that reads one lane of its 16-lane row as a DPP operand, and the Riccati sweeps' step built on
// it.  One wave per launch.  Four parts, the first three compared bit for bit:
//  1. lane patterns: fmac_rbc<C>(acc, v, ph), C = 0..5, against fma(rbc<C>(v), ph, acc) on
//     patterns carrying +-0, +-inf, a NaN payload, denormals and random values in all four rows;
//  2. hazard: chains of five multiply-adds whose v is written by the instruction just before the
//     first of them (the DPP read-after-VALU-write case the helpers' s_nop covers), as separate
//     statements (fmac_rbc_seq) and as one (fmac_rbc_chain), against the chain with explicit
//     v_mov_b64_dpp copies;
//  3. recursions: a backward and a forward sweep in the kernel's exact step forms, (NS, NU) =
//     (5, 1) and (4, 2), over N = 1, 2, 3, 20, 21 stages of random operands: once as the step
//     was before (rbc_all + plain multiply-adds, the copy kept below and still the fp32 form) and
//     once as bqp_ocp.hip has it now (fmac_rbc_chain on the previous accumulator).  Every stage
//     vector must be equal, and in the new form lanes >= NS of row 0 must repeat entry NS - 1;
//  4. printed, not asserted: s_memtime cycles of the two 20-stage recursions in either form.
// Built by learning-based-mpc_amd/Makefile (build/fmac_rbc_check), run by
// tests/test_gpu_fmac_rbc.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "bqp_wave.h"

using bqp::fmac_rbc;
using bqp::fmac_rbc_chain;
using bqp::fmac_rbc_seq;
using bqp::rbc;
using bqp::rbc_all;

#define CK(x) do { if ((x) != hipSuccess) { printf("HIP error at line %d\n", __LINE__); return 2; } } while (0)

static double bits(uint64_t b) { double d; memcpy(&d, &b, sizeof d); return d; }
static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() {   // uniform in (-1, 1)
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(rng_state >> 11) / 4503599627370496.0 - 1.0;
}

// ---- 1. lane patterns ----------------------------------------------------------------------
constexpr int NPAT = 6;   // C = 0..5
template <int C>
__device__ __forceinline__ void pat_one(double acc, double v, double ph, uint64_t* o_new, uint64_t* o_ref) {
    double a = acc;
    fmac_rbc<C, true>(a, v, ph);
    o_new[C] = __builtin_bit_cast(uint64_t, a);
    o_ref[C] = __builtin_bit_cast(uint64_t, __builtin_fma(rbc<C>(v), ph, acc));
}
__global__ void k_pat(const double* in, uint64_t* out) {   // in: [64][3], out: [2][64][NPAT]
    const int lane = threadIdx.x;
    const double v = in[lane * 3], ph = in[lane * 3 + 1], acc = in[lane * 3 + 2];
    uint64_t* o_new = out + lane * NPAT;
    uint64_t* o_ref = out + (64 + lane) * NPAT;
    pat_one<0>(acc, v, ph, o_new, o_ref);
    pat_one<1>(acc, v, ph, o_new, o_ref);
    pat_one<2>(acc, v, ph, o_new, o_ref);
    pat_one<3>(acc, v, ph, o_new, o_ref);
    pat_one<4>(acc, v, ph, o_new, o_ref);
    pat_one<5>(acc, v, ph, o_new, o_ref);
}

// ---- 2. hazard -----------------------------------------------------------------------------
// MODE 0: explicit moves (reference), 1: fmac_rbc_seq, 2: fmac_rbc_chain.  v = a + b is an asm
// statement right in front of the chain, nothing else left to schedule between them.  (Behind an
// asm statement whose result the next instruction reads the compiler puts one `s_nop 0` of its
// own; that single wait state is less than the two the DPP read needs, so the result is right
// only with the helpers' own wait states.)
template <int MODE>
__global__ void k_haz(const double* in, uint64_t* out) {   // in: [64][8]: a, b, q, ph[5]
    const int lane = threadIdx.x;
    const double a = in[lane * 8], b = in[lane * 8 + 1], q = in[lane * 8 + 2];
    double ph[5];
    for (int c = 0; c < 5; ++c) ph[c] = in[lane * 8 + 3 + c];
    double v, acc = q;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("v_add_f64 %0, %1, %2" : "=v"(v) : "v"(a), "v"(b));
    if constexpr (MODE == 0) {
        double p[5];
        rbc_all<0, 5>(v, p);
        for (int c = 0; c < 5; ++c) acc = __builtin_fma(p[c], ph[c], acc);
    } else if constexpr (MODE == 1) {
        fmac_rbc_seq<0, 5>(acc, v, ph);
    } else {
        acc = fmac_rbc_chain(q, v, ph);
    }
    out[lane] = __builtin_bit_cast(uint64_t, acc);
}

// ---- 3. / 4. recursions --------------------------------------------------------------------
constexpr int NMAX = 21;
// operand block in LDS, as the kernel's workspace: A (NS x NS), B (NS x NU), K (N x NU x NS),
// rhs (N x NS: qh_k backward, f_k forward), start (NS), then the swept vectors ((N + 1) x NS)
template <int NS, int NU>
struct Off {
    static constexpr int A = 0, B = A + NS * NS, K = B + NS * NU, R = K + NMAX * NU * NS,
                         S = R + NMAX * NS, V = S + NS, END = V + (NMAX + 1) * NS;
};

// DUMP: every lane's accumulator of every stage to global memory (dump[k][lane]) instead of the
// LDS store of the sweep; the timed runs use the LDS store
template <int NS, int NU, bool NEW, bool FWD, bool DUMP>
__device__ __forceinline__ void sweep(double* W, int N, int lane, double* dump) {
    using O = Off<NS, NU>;
    auto Abar = [&](int r, int c) { return W[O::A + r * NS + c]; };
    auto Bbar = [&](int r, int x) { return W[O::B + r * NU + x]; };
    const int li = lane < NS ? lane : NS - 1;
    if constexpr (!NEW && !FWD) {
        // backward step as it was (bqp_ocp.hip before the DPP-operand form; still the fp32 form)
        double Acol[NS], Bl[NS][NU];
        for (int c = 0; c < NS; ++c) {
            Acol[c] = Abar(c, li);
            for (int x = 0; x < NU; ++x) Bl[c][x] = Bbar(c, x);
        }
        double p[NS];
        for (int i = 0; i < NS; ++i) p[i] = W[O::S + i];
        auto load_b = [&](int k, double (&kc)[NU], double& q) __attribute__((always_inline)) {
            q = W[O::R + k * NS + li];
            for (int x = 0; x < NU; ++x) kc[x] = W[O::K + k * NU * NS + x * NS + li];
        };
        double k0[NU], q0, k1[NU], q1;
        load_b(N - 1, k0, q0);
        load_b(max(N - 2, 0), k1, q1);
        auto step_b = [&](int k, const double (&kc)[NU], double q) __attribute__((always_inline)) {
            double acc = q;
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                double ph = Acol[c];
#pragma unroll
                for (int x = 0; x < NU; ++x) ph += Bl[c][x] * kc[x];
                acc += ph * p[c];
            }
            if constexpr (DUMP) dump[k * 64 + lane] = acc;
            else if (lane < NS) W[O::V + k * NS + lane] = acc;
            rbc_all<0, NS>(acc, p);
        };
        for (int k = N - 1; k >= 1; k -= 2) {
            step_b(k, k0, q0);
            load_b(max(k - 2, 0), k0, q0);
            step_b(k - 1, k1, q1);
            load_b(max(k - 3, 0), k1, q1);
        }
        if (N & 1) step_b(0, k0, q0);
    } else if constexpr (!NEW && FWD) {
        // forward step as it was
        double d[NS];
        for (int i = 0; i < NS; ++i) d[i] = W[O::S + i];
        double Arow[NS], Bli[NU];
        for (int c = 0; c < NS; ++c) Arow[c] = Abar(li, c);
        for (int x = 0; x < NU; ++x) Bli[x] = Bbar(li, x);
        auto load_f = [&](int k, double (&kr)[NU][NS], double& f) __attribute__((always_inline)) {
            f = W[O::R + k * NS + li];
            for (int x = 0; x < NU; ++x)
                for (int c = 0; c < NS; ++c) kr[x][c] = W[O::K + k * NU * NS + x * NS + c];
        };
        double k0[NU][NS], f0, k1[NU][NS], f1;
        load_f(0, k0, f0);
        load_f(min(1, N - 1), k1, f1);
        auto step_f = [&](int k, const double (&kr)[NU][NS], double f) __attribute__((always_inline)) {
            double acc = f;
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                double ph = Arow[c];
#pragma unroll
                for (int x = 0; x < NU; ++x) ph += Bli[x] * kr[x][c];
                acc += ph * d[c];
            }
            if constexpr (DUMP) dump[(k + 1) * 64 + lane] = acc;
            else if (lane < NS) W[O::V + (k + 1) * NS + lane] = acc;
            rbc_all<0, NS>(acc, d);
        };
        for (int k = 0; k + 1 < N; k += 2) {
            step_f(k, k0, f0);
            load_f(min(k + 2, N - 1), k0, f0);
            step_f(k + 1, k1, f1);
            load_f(min(k + 3, N - 1), k1, f1);
        }
        if (N & 1) step_f(N - 1, k0, f0);
    } else if constexpr (NEW && !FWD) {
        // backward step as bqp_ocp.hip has it (fp64)
        double Acol[NS], Bl[NS][NU];
        for (int c = 0; c < NS; ++c) {
            Acol[c] = Abar(c, li);
            for (int x = 0; x < NU; ++x) Bl[c][x] = Bbar(c, x);
        }
        double pv = W[O::S + li];
        auto load_b = [&](int k, double (&kc)[NU], double& q) __attribute__((always_inline)) {
            for (int x = 0; x < NU; ++x) kc[x] = W[O::K + k * NU * NS + x * NS + li];
            q = W[O::R + k * NS + li];
        };
        double k0[NU], q0, k1[NU], q1;
        load_b(N - 1, k0, q0);
        load_b(max(N - 2, 0), k1, q1);
        auto step_b = [&](int k, const double (&kc)[NU], double q) __attribute__((always_inline)) {
            double ph[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                ph[c] = Acol[c];
#pragma unroll
                for (int x = 0; x < NU; ++x) ph[c] += Bl[c][x] * kc[x];
            }
            pv = fmac_rbc_chain(q, pv, ph);
            if constexpr (DUMP) dump[k * 64 + lane] = pv;
            else if (lane < NS) W[O::V + k * NS + lane] = pv;
        };
        for (int k = N - 1; k >= 1; k -= 2) {
            step_b(k, k0, q0);
            load_b(max(k - 2, 0), k0, q0);
            step_b(k - 1, k1, q1);
            load_b(max(k - 3, 0), k1, q1);
        }
        if (N & 1) step_b(0, k0, q0);
    } else {
        // forward step as bqp_ocp.hip has it (fp64)
        double dv = W[O::S + li];
        double Arow[NS], Bli[NU];
        for (int c = 0; c < NS; ++c) Arow[c] = Abar(li, c);
        for (int x = 0; x < NU; ++x) Bli[x] = Bbar(li, x);
        auto load_f = [&](int k, double (&kr)[NU][NS], double& f) __attribute__((always_inline)) {
            for (int x = 0; x < NU; ++x)
                for (int c = 0; c < NS; ++c) kr[x][c] = W[O::K + k * NU * NS + x * NS + c];
            f = W[O::R + k * NS + li];
        };
        double k0[NU][NS], f0, k1[NU][NS], f1;
        load_f(0, k0, f0);
        load_f(min(1, N - 1), k1, f1);
        auto step_f = [&](int k, const double (&kr)[NU][NS], double f) __attribute__((always_inline)) {
            double ph[NS];
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                ph[c] = Arow[c];
#pragma unroll
                for (int x = 0; x < NU; ++x) ph[c] += Bli[x] * kr[x][c];
            }
            dv = fmac_rbc_chain(f, dv, ph);
            if constexpr (DUMP) dump[(k + 1) * 64 + lane] = dv;
            else if (lane < NS) W[O::V + (k + 1) * NS + lane] = dv;
        };
        for (int k = 0; k + 1 < N; k += 2) {
            step_f(k, k0, f0);
            load_f(min(k + 2, N - 1), k0, f0);
            step_f(k + 1, k1, f1);
            load_f(min(k + 3, N - 1), k1, f1);
        }
        if (N & 1) step_f(N - 1, k0, f0);
    }
}

// out: the swept vectors ((NMAX + 1) x NS words, from LDS), cyc: cycles of the sweep;
// dump != nullptr selects the per-lane form ((NMAX + 1) x 64 words) and leaves out / cyc alone
template <int NS, int NU, bool NEW, bool FWD, bool DUMP>
__global__ void __launch_bounds__(64) k_rec(const double* in, int N, uint64_t* out, double* dump,
                                            unsigned long long* cyc) {
    using O = Off<NS, NU>;
    __shared__ double W[O::END];
    const int lane = threadIdx.x;
    for (int i = lane; i < O::V; i += 64) W[i] = in[i];
    for (int i = O::V + lane; i < O::END; i += 64) W[i] = 0.0;
    bqp::wave_sync();
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    sweep<NS, NU, NEW, FWD, DUMP>(W, N, lane, dump);
    __builtin_amdgcn_s_waitcnt(0);
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    bqp::wave_sync();
    if constexpr (!DUMP) {
        for (int i = lane; i < (NMAX + 1) * NS; i += 64) out[i] = __builtin_bit_cast(uint64_t, W[O::V + i]);
        if (lane == 0) cyc[0] = t1 - t0;
    }
}

template <int NS, int NU>
static int run_rec(double* d_in, uint64_t* d_out, double* d_dump, unsigned long long* d_cyc, int* diff,
                   unsigned long long (&cycles)[2][2]) {
    using O = Off<NS, NU>;
    static double h[O::V];
    static uint64_t o[2][(NMAX + 1) * NS];
    static uint64_t dmp[2][(NMAX + 1) * 64];
    for (int i = 0; i < O::V; ++i) h[i] = rnd() * (i < O::K ? 0.5 : (i < O::R ? 0.25 : 1.0));
    CK(hipMemcpy(d_in, h, sizeof h, hipMemcpyHostToDevice));
    const int Ns[5] = {1, 2, 3, 20, 21};
    for (int fwd = 0; fwd < 2; ++fwd)
        for (int n = 0; n < 5; ++n) {
            const int N = Ns[n];
            for (int w = 0; w < 2; ++w) {
                CK(hipMemset(d_out, 0xff, sizeof o[0]));
                CK(hipMemset(d_dump, 0xff, sizeof dmp[0]));
#define LAUNCH(NEW, FWD) \
    hipLaunchKernelGGL((k_rec<NS, NU, NEW, FWD, false>), dim3(1), dim3(64), 0, 0, d_in, N, d_out, d_dump, d_cyc); \
    hipLaunchKernelGGL((k_rec<NS, NU, NEW, FWD, true>), dim3(1), dim3(64), 0, 0, d_in, N, d_out, d_dump, d_cyc)
                if (w && fwd) { LAUNCH(true, true); }
                else if (w) { LAUNCH(true, false); }
                else if (fwd) { LAUNCH(false, true); }
                else { LAUNCH(false, false); }
#undef LAUNCH
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(o[w], d_out, sizeof o[0], hipMemcpyDeviceToHost));
                CK(hipMemcpy(dmp[w], d_dump, sizeof dmp[0], hipMemcpyDeviceToHost));
                if (N == 20) CK(hipMemcpy(&cycles[fwd][w], d_cyc, sizeof(unsigned long long), hipMemcpyDeviceToHost));
            }
            // stages written: backward k = 0 .. N - 1, forward k = 1 .. N
            const int lo = fwd ? 1 : 0, hi = fwd ? N : N - 1;
            int d = 0;
            for (int k = lo; k <= hi; ++k) {
                for (int i = 0; i < NS; ++i) {
                    const uint64_t ref = o[0][k * NS + i];
                    if (ref == 0 || ref == ~0ull) ++d;   // the stage must really have been written
                    if (o[1][k * NS + i] != ref) ++d;
                    if (dmp[0][k * 64 + i] != ref) ++d;  // the old form's lane i (row 0)
                }
                for (int l = 0; l < 16; ++l) {           // the new form: every lane of row 0
                    const int li = l < NS ? l : NS - 1;
                    if (dmp[1][k * 64 + l] != o[0][k * NS + li]) ++d;
                }
            }
            if (d) printf("recursion NS %d NU %d %s N %d: %d words differ\n", NS, NU, fwd ? "forward" : "backward", N, d);
            *diff += d;
        }
    return 0;
}

int main() {
    int bad = 0;
    double* d_in;
    uint64_t* d_out;
    double* d_dump;
    unsigned long long* d_cyc;
    CK(hipMalloc(&d_in, 4096 * sizeof(double)));
    CK(hipMalloc(&d_out, 4096 * sizeof(uint64_t)));
    CK(hipMalloc(&d_dump, (NMAX + 1) * 64 * sizeof(double)));
    CK(hipMalloc(&d_cyc, sizeof(unsigned long long)));
    const double sp[8] = {0.0, -0.0, bits(0x0000000000000001ull), bits(0x800fffffffffffffull),
                          bits(0x7ff0000000000000ull), bits(0xfff0000000000000ull),
                          bits(0x7ff80000dead0001ull), bits(0x7ff4000000000042ull)};
    {   // 1. lane patterns: v, ph and acc each see every special in some lane of every row
        static double h[64 * 3];
        static uint64_t o[2 * 64 * NPAT];
        int diff = 0, words = 0, nan = 0;
        for (int pat = 0; pat < 4; ++pat) {
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 3; ++j) {
                    double x = rnd() * (1 + (l % 7));
                    const int pick = (l * (3 + 2 * j) + pat * 5 + j * 7) % 16;
                    if (pat > 0 && pick < 8) x = sp[pick];               // pattern 0: random values only
                    if (pat == 3 && j == 1 && (l & 1)) x *= 0x1p-1040;    // denormal products
                    h[l * 3 + j] = x;
                }
            CK(hipMemcpy(d_in, h, sizeof h, hipMemcpyHostToDevice));
            CK(hipMemset(d_out, 0xff, sizeof o));
            hipLaunchKernelGGL(k_pat, dim3(1), dim3(64), 0, 0, d_in, d_out);
            CK(hipMemcpy(o, d_out, sizeof o, hipMemcpyDeviceToHost));
            for (int i = 0; i < 64 * NPAT; ++i) {
                if (o[i] != o[64 * NPAT + i]) {
                    if (!diff) printf("pattern %d lane %d C %d: ref %016llx new %016llx\n", pat, i / NPAT, i % NPAT,
                                      (unsigned long long)o[64 * NPAT + i], (unsigned long long)o[i]);
                    ++diff;
                }
                const double d = bits(o[i]);
                if (pat > 0 && d != d) ++nan;
                if (pat == 0 && d != d) { printf("pattern 0: NaN word\n"); ++bad; }
                ++words;
            }
        }
        if (!nan) { printf("special patterns: no NaN word\n"); ++bad; }
        printf("lane patterns: %d words, %d differ\n", words, diff);
        bad += diff;
    }
    {   // 2. hazard
        static double h[64 * 8];
        static uint64_t o[3][64];
        int diff = 0;
        for (int rep = 0; rep < 4; ++rep) {
            for (int i = 0; i < 64 * 8; ++i) h[i] = rnd();
            CK(hipMemcpy(d_in, h, sizeof h, hipMemcpyHostToDevice));
            for (int m = 0; m < 3; ++m) {
                CK(hipMemset(d_out, 0xff, sizeof o[0]));
                if (m == 0) hipLaunchKernelGGL(k_haz<0>, dim3(1), dim3(64), 0, 0, d_in, d_out);
                if (m == 1) hipLaunchKernelGGL(k_haz<1>, dim3(1), dim3(64), 0, 0, d_in, d_out);
                if (m == 2) hipLaunchKernelGGL(k_haz<2>, dim3(1), dim3(64), 0, 0, d_in, d_out);
                CK(hipMemcpy(o[m], d_out, sizeof o[0], hipMemcpyDeviceToHost));
            }
            for (int l = 0; l < 64; ++l) {
                if (o[0][l] == ~0ull) ++diff;
                if (o[1][l] != o[0][l]) ++diff;
                if (o[2][l] != o[0][l]) ++diff;
            }
        }
        printf("hazard chains: %d words, %d differ\n", 4 * 64 * 2, diff);
        bad += diff;
    }
    {   // 3. recursions, 4. cycles
        int diff = 0;
        unsigned long long c51[2][2] = {{0, 0}, {0, 0}}, c42[2][2] = {{0, 0}, {0, 0}};
        if (run_rec<5, 1>(d_in, d_out, d_dump, d_cyc, &diff, c51)) return 2;
        if (run_rec<4, 2>(d_in, d_out, d_dump, d_cyc, &diff, c42)) return 2;
        printf("recursions: 2 families x 2 sweeps x 5 horizons, %d differ\n", diff);
        bad += diff;
        printf("cycles, 20 stages, NS 5 NU 1: backward old %llu new %llu, forward old %llu new %llu\n",
               c51[0][0], c51[0][1], c51[1][0], c51[1][1]);
        printf("cycles, 20 stages, NS 4 NU 2: backward old %llu new %llu, forward old %llu new %llu\n",
               c42[0][0], c42[0][1], c42[1][0], c42[1][1]);
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    (void)hipFree(d_dump);
    (void)hipFree(d_cyc);
    return bad ? 1 : 0;
}
