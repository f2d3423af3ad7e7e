// bqp_wave.h — wavefront-level helpers shared by the HIP kernels (gfx950, wave64): intra-wave
// sync, DPP reductions, readlane broadcast, fast reciprocal.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace bqp {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wave-wide reductions on DPP lane moves (quad_perm xor1/xor2, row_half_mirror, row_mirror
// inside each 16-lane row, then row_bcast15/31 across rows) + a readlane of lane 63: no LDS
// traffic, result uniform in every lane.  EXEC must be full (all call sites are wave-uniform).
//
// Two forms of the lane move.  dpp_mov<CTRL, ROWM>(old, v) keeps `old` where the move delivers
// nothing (rows outside ROWM, source lanes that are out of range or disabled), so the compiler
// first writes `old` into the destination: one more VALU instruction per move.  dpp_mov0<CTRL>(v)
// is the move with old = 0 and the full row mask, issued with bound_ctrl:1: a source lane that
// is out of range or disabled then reads as 0, which is what the untouched old = 0 gave, and a
// valid one delivers its value either way - the same function for every EXEC and every bit
// pattern (the move copies bits; tests/hip/dpp_bcast_check.hip compares the two), without the
// zero write.  Only that case may use it: a partial row mask (the row_bcast:15 / :31 steps)
// leaves the masked rows at `old`, which bound_ctrl does not provide, and a non-zero `old`
// (wmax's -inf) would only be equivalent while EXEC is full, so both stay on dpp_mov.
template <int CTRL, int ROWM>
__device__ __forceinline__ double dpp_mov(double old, double v) {
    const int2 o = __builtin_bit_cast(int2, old);
    const int2 x = __builtin_bit_cast(int2, v);
    int2 r;
    r.x = __builtin_amdgcn_update_dpp(o.x, x.x, CTRL, ROWM, 0xf, false);
    r.y = __builtin_amdgcn_update_dpp(o.y, x.y, CTRL, ROWM, 0xf, false);
    return __builtin_bit_cast(double, r);
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov0(double v) {
    const int2 x = __builtin_bit_cast(int2, v);
    int2 r;
    r.x = __builtin_amdgcn_update_dpp(0, x.x, CTRL, 0xf, 0xf, true);
    r.y = __builtin_amdgcn_update_dpp(0, x.y, CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, r);
}
__device__ __forceinline__ double lane63(double v) {
    const int2 x = __builtin_bit_cast(int2, v);
    int2 r;
    r.x = __builtin_amdgcn_readlane(x.x, 63);
    r.y = __builtin_amdgcn_readlane(x.y, 63);
    return __builtin_bit_cast(double, r);
}
__device__ __forceinline__ double wsum(double v) {
    v += dpp_mov0<0xB1>(v);
    v += dpp_mov0<0x4E>(v);
    v += dpp_mov0<0x141>(v);
    v += dpp_mov0<0x140>(v);
    v += dpp_mov<0x142, 0xa>(0.0, v);
    v += dpp_mov<0x143, 0xc>(0.0, v);
    return lane63(v);
}
__device__ __forceinline__ double wmax(double v) {
    v = fmax(v, dpp_mov<0xB1, 0xf>(-INFINITY, v));
    v = fmax(v, dpp_mov<0x4E, 0xf>(-INFINITY, v));
    v = fmax(v, dpp_mov<0x141, 0xf>(-INFINITY, v));
    v = fmax(v, dpp_mov<0x140, 0xf>(-INFINITY, v));
    v = fmax(v, dpp_mov<0x142, 0xa>(-INFINITY, v));
    v = fmax(v, dpp_mov<0x143, 0xc>(-INFINITY, v));
    return lane63(v);
}
__device__ __forceinline__ double wmin(double v) { return -wmax(-v); }
// value of lane `src` broadcast to the wave (scalar register pair): the sequential Riccati
// sweeps pass their NS-vector from stage to stage this way instead of through LDS
__device__ __forceinline__ double rl(double v, int src) {
    const int2 x = __builtin_bit_cast(int2, v);
    int2 r;
    r.x = __builtin_amdgcn_readlane(x.x, src);
    r.y = __builtin_amdgcn_readlane(x.y, src);
    return __builtin_bit_cast(double, r);
}

// ---- transposed multi-value sums: K <= 32 per-lane partials reduced over the wave at once ----
// Each exchange step halves the number of values a lane carries: of a pair (a, b) a lane keeps a
// or b by one bit of its lane id and adds the partner lane's other one (quad_perm xor1, xor2,
// row_ror 4, row_ror 8 inside 16-lane rows; then the gfx950 row swaps v_permlane16_swap /
// v_permlane32_swap across rows).  K values cost ~K pair steps instead of 6 K DPP steps.
// Afterwards lane l holds the wave total of value (l & 31) (0 for ids >= K).
__device__ __forceinline__ void pl16_swap(double& a, double& b) {
    const int2 A = __builtin_bit_cast(int2, a), B = __builtin_bit_cast(int2, b);
    const auto x = __builtin_amdgcn_permlane16_swap((unsigned)A.x, (unsigned)B.x, false, false);
    const auto y = __builtin_amdgcn_permlane16_swap((unsigned)A.y, (unsigned)B.y, false, false);
    a = __builtin_bit_cast(double, make_int2((int)x[0], (int)y[0]));
    b = __builtin_bit_cast(double, make_int2((int)x[1], (int)y[1]));
}
__device__ __forceinline__ void pl32_swap(double& a, double& b) {
    const int2 A = __builtin_bit_cast(int2, a), B = __builtin_bit_cast(int2, b);
    const auto x = __builtin_amdgcn_permlane32_swap((unsigned)A.x, (unsigned)B.x, false, false);
    const auto y = __builtin_amdgcn_permlane32_swap((unsigned)A.y, (unsigned)B.y, false, false);
    a = __builtin_bit_cast(double, make_int2((int)x[0], (int)y[0]));
    b = __builtin_bit_cast(double, make_int2((int)x[1], (int)y[1]));
}
__device__ __forceinline__ void pl16_swap(float& a, float& b) {
    const auto x = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a),
                                                    __builtin_bit_cast(unsigned, b), false, false);
    a = __builtin_bit_cast(float, (unsigned)x[0]);
    b = __builtin_bit_cast(float, (unsigned)x[1]);
}
__device__ __forceinline__ void pl32_swap(float& a, float& b) {
    const auto x = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a),
                                                    __builtin_bit_cast(unsigned, b), false, false);
    a = __builtin_bit_cast(float, (unsigned)x[0]);
    b = __builtin_bit_cast(float, (unsigned)x[1]);
}
// fp32 overloads (the structured kernel's fp32 instantiation, bqp_ocp_f32.hip)
template <int CTRL, int ROWM>
__device__ __forceinline__ float dpp_mov(float old, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                                  __builtin_bit_cast(int, v), CTRL,
                                                                  ROWM, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov0(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL,
                                                                  0xf, 0xf, true));
}
__device__ __forceinline__ float lane63(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}
__device__ __forceinline__ float wsum(float v) {
    v += dpp_mov0<0xB1>(v);
    v += dpp_mov0<0x4E>(v);
    v += dpp_mov0<0x141>(v);
    v += dpp_mov0<0x140>(v);
    v += dpp_mov<0x142, 0xa>(0.0f, v);
    v += dpp_mov<0x143, 0xc>(0.0f, v);
    return lane63(v);
}
__device__ __forceinline__ float wmax(float v) {
    v = fmaxf(v, dpp_mov<0xB1, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x4E, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x141, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x140, 0xf>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x142, 0xa>(-INFINITY, v));
    v = fmaxf(v, dpp_mov<0x143, 0xc>(-INFINITY, v));
    return lane63(v);
}
__device__ __forceinline__ float wmin(float v) { return -wmax(-v); }
__device__ __forceinline__ float rl(float v, int src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// lane C's value in every lane of its 16-lane row (gfx950 DPP row_newbcast: one v_mov_b64_dpp
// / v_mov_b32_dpp, the value stays in vector registers); rbc_all fills p[c] = lane c's v for
// c < NC (NC <= 16), the sweep broadcast without a scalar round trip.  old = 0 with bound_ctrl:1,
// as dpp_mov0: no zero write in front of the move
template <int C>
__device__ __forceinline__ double rbc(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + C, 0xf, 0xf, true);
}
template <int C>
__device__ __forceinline__ float rbc(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v),
                                                                 0x150 + C, 0xf, 0xf, true));
}
// the value of 16-lane row Q (lane 16 Q + l%16) in lane l of every row: v_permlane16_swap of a
// register with itself gives the even / odd row pairs, v_permlane32_swap the halves - VALU only
// (the ds_bpermute form took an LDS round trip)
template <int Q>
__device__ __forceinline__ double xrow_bcast(double v) {
    double a = v, b = v;
    pl16_swap(a, b);                 // a: rows (0, 0, 2, 2), b: rows (1, 1, 3, 3)
    double c = (Q & 1) ? b : a, d = c;
    pl32_swap(c, d);                 // c: rows (q, q, q, q) of the lower pair, d: of the upper pair
    return (Q >> 1) ? d : c;
}

template <int C, int NC, typename T>
__device__ __forceinline__ void rbc_all(T v, T (&p)[NC]) {
    p[C] = rbc<C>(v);
    if constexpr (C + 1 < NC) rbc_all<C + 1, NC>(v, p);
}

// acc += (lane C of this 16-lane row of v) * ph as ONE instruction: v_fmac_f64 is VOP2 on gfx950
// and takes the DPP operand itself, so a broadcast value that is used once, as a multiplicand,
// needs no v_mov_b64_dpp and no register of its own.  The same fused multiply-add on the same
// operands as fma(rbc<C>(v), ph, acc): every bit equal (tests/hip/fmac_rbc_check.hip).  A source
// lane that is disabled reads as 0 (bound_ctrl:1), as rbc.
//
// The compiler's hazard recogniser does not look into inline asm, so the two DPP hazards of
// gfx9 are the caller's:
//  - a VGPR written by a VALU instruction needs 2 wait states before a DPP instruction reads it.
//    FRESH = true puts `s_nop 1` (2 wait states) in front of the multiply-add; it is for the call
//    whose v may come from the instruction just before it (in the sweeps: the first multiply-add
//    of a step, which reads the accumulator that the previous step's last one wrote).  The
//    following calls on the same v have that first one between them and the writer.
//  - a VALU write of EXEC (v_cmpx) needs 5 wait states before a DPP instruction.  hipcc emits no
//    v_cmpx for gfx950 in these kernels: a guard changes EXEC with SALU instructions
//    (s_and_saveexec / s_or, as around the sweeps' guarded store), which carry no such rule.
//    A caller that writes EXEC from the VALU by hand has to add the wait itself.
template <int C, bool FRESH = false, typename T>
__device__ __forceinline__ void fmac_rbc(T& acc, T v, T ph) {
    static_assert(sizeof(T) == 8, "fmac_rbc: fp64 only (the fp32 sweeps keep rbc + plain products)");
    static_assert(C >= 0 && C < 16, "fmac_rbc: lane of a 16-lane row");
    if constexpr (FRESH)
        asm("s_nop 1\n\t"   // DPP read of a VGPR the previous VALU instruction may have written
            "v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf bound_ctrl:1"
            : "+v"(acc) : "v"(v), "v"(ph), "n"(C));
    else
        asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf bound_ctrl:1"
            : "+v"(acc) : "v"(v), "v"(ph), "n"(C));
}
template <int C, int NC, typename T>
__device__ __forceinline__ void fmac_rbc_seq(T& acc, T v, const T (&ph)[NC]) {
    fmac_rbc<C, C == 0>(acc, v, ph[C]);
    if constexpr (C + 1 < NC) fmac_rbc_seq<C + 1, NC>(acc, v, ph);
}
// The chain of a sweep step: returns q + sum_c (lane c of v) * ph[c], the products added in the
// order c = 0 .. NC-1, v possibly written by the instruction just before.  NC = 4, 5 (the model
// families' NS) are ONE asm statement that starts with the copy of q into the result register:
//  - between two asm statements that depend on each other the compiler puts an `s_nop 0` (it
//    must assume that the first writes part of a register), NC - 1 of them per chain;
//  - q is a loaded value whose register is refilled while the chain's result is still read by the
//    next step, so a copy is needed somewhere, and the register allocator put it behind the
//    previous result or in front of the last multiply-add: on the dependent chain.  Written
//    here it depends on q alone and issues while the previous step's last result is pending.
// Hazard: the first multiply-add reads v through DPP and v may be the previous VALU instruction's
// result, which needs 2 wait states: the copy is one, `s_nop 0` the other.  The later ones have
// those in between.
#define BQP_FMAC_RBC(OP, C) \
    "v_fmac_f64_dpp %0, %2, %" #OP " row_newbcast:" #C " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
#define BQP_CHAIN_HEAD \
    "v_mov_b64 %0, %1\n\t" \
    "s_nop 0\n\t"   /* with the copy: 2 wait states between v's writer and the DPP read of v */
template <int NC, typename T>
__device__ __forceinline__ T fmac_rbc_chain(T q, T v, const T (&ph)[NC]) {
    static_assert(sizeof(T) == 8, "fmac_rbc_chain: fp64 only");
    T acc;
    if constexpr (NC == 4) {
        asm(BQP_CHAIN_HEAD BQP_FMAC_RBC(3, 0) BQP_FMAC_RBC(4, 1) BQP_FMAC_RBC(5, 2) BQP_FMAC_RBC(6, 3)
            : "=&v"(acc) : "v"(q), "v"(v), "v"(ph[0]), "v"(ph[1]), "v"(ph[2]), "v"(ph[3]));
    } else if constexpr (NC == 5) {
        asm(BQP_CHAIN_HEAD BQP_FMAC_RBC(3, 0) BQP_FMAC_RBC(4, 1) BQP_FMAC_RBC(5, 2) BQP_FMAC_RBC(6, 3)
            BQP_FMAC_RBC(7, 4)
            : "=&v"(acc) : "v"(q), "v"(v), "v"(ph[0]), "v"(ph[1]), "v"(ph[2]), "v"(ph[3]), "v"(ph[4]));
    } else {
        acc = q;
        fmac_rbc_seq<0, NC>(acc, v, ph);   // any other length: one statement per multiply-add
    }
    return acc;
}
#undef BQP_CHAIN_HEAD
#undef BQP_FMAC_RBC

// The dot product of a Riccati factor stage (stage_wave's factor(), FACTOR_ROWS): lane m of every
// 16-lane row holds entry m of a vector v, and each lane has NC coefficients of its own.  Forms the
// four partial sums s_j = sum over m = j mod 4 of c[m] * (lane m of v), each from 0 in the order of
// m, as fma(c[m], v_m, s_j): the caller adds them as (s0 + s1) + (s2 + s3).  NC = 10, 15 (the model
// families' packed P: NS = 4, 5) are ONE asm statement:
//  - the four accumulators are independent, so the scheduler would be free to reorder separate
//    statements, and the one that must wait for v's writer would no longer be known;
//  - the four zero writes in front are the 2 wait states between a VALU write of v and its first
//    DPP read (fmac_rbc's first hazard), so the statement needs no s_nop at all: consecutive
//    multiply-adds are on different accumulators, and each reads its accumulator as a plain operand.
// A source lane that is disabled reads as 0 (bound_ctrl:1): callers run with all lanes enabled.
#define BQP_DOT4_ZERO \
    "v_mov_b64 %0, 0\n\tv_mov_b64 %1, 0\n\tv_mov_b64 %2, 0\n\tv_mov_b64 %3, 0\n\t"
#define BQP_DOT4_FMAC(ACC, OP, C) \
    "v_fmac_f64_dpp %" #ACC ", %4, %" #OP " row_newbcast:" #C " row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
template <int M, int NC, typename T>
__device__ __forceinline__ void fmac_rbc_dot4_seq(T (&s)[4], T v, const T (&c)[NC]) {
    fmac_rbc<M, (M < 4)>(s[M & 3], v, c[M]);   // the first of each accumulator may follow v's writer
    if constexpr (M + 1 < NC) fmac_rbc_dot4_seq<M + 1, NC>(s, v, c);
}
template <int NC, typename T>
__device__ __forceinline__ void fmac_rbc_dot4(T (&s)[4], T v, const T (&c)[NC]) {
    static_assert(sizeof(T) == 8, "fmac_rbc_dot4: fp64 only");
    static_assert(NC >= 4 && NC <= 16, "fmac_rbc_dot4: one entry per lane of a 16-lane row");
    if constexpr (NC == 10) {
        asm(BQP_DOT4_ZERO
            BQP_DOT4_FMAC(0, 5, 0) BQP_DOT4_FMAC(1, 6, 1) BQP_DOT4_FMAC(2, 7, 2) BQP_DOT4_FMAC(3, 8, 3)
            BQP_DOT4_FMAC(0, 9, 4) BQP_DOT4_FMAC(1, 10, 5) BQP_DOT4_FMAC(2, 11, 6) BQP_DOT4_FMAC(3, 12, 7)
            BQP_DOT4_FMAC(0, 13, 8) BQP_DOT4_FMAC(1, 14, 9)
            : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3])
            : "v"(v), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]),
              "v"(c[7]), "v"(c[8]), "v"(c[9]));
    } else if constexpr (NC == 15) {
        asm(BQP_DOT4_ZERO
            BQP_DOT4_FMAC(0, 5, 0) BQP_DOT4_FMAC(1, 6, 1) BQP_DOT4_FMAC(2, 7, 2) BQP_DOT4_FMAC(3, 8, 3)
            BQP_DOT4_FMAC(0, 9, 4) BQP_DOT4_FMAC(1, 10, 5) BQP_DOT4_FMAC(2, 11, 6) BQP_DOT4_FMAC(3, 12, 7)
            BQP_DOT4_FMAC(0, 13, 8) BQP_DOT4_FMAC(1, 14, 9) BQP_DOT4_FMAC(2, 15, 10) BQP_DOT4_FMAC(3, 16, 11)
            BQP_DOT4_FMAC(0, 17, 12) BQP_DOT4_FMAC(1, 18, 13) BQP_DOT4_FMAC(2, 19, 14)
            : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3])
            : "v"(v), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]), "v"(c[6]),
              "v"(c[7]), "v"(c[8]), "v"(c[9]), "v"(c[10]), "v"(c[11]), "v"(c[12]), "v"(c[13]),
              "v"(c[14]));
    } else {
        s[0] = s[1] = s[2] = s[3] = T(0);
        fmac_rbc_dot4_seq<0, NC>(s, v, c);       // any other length: one statement per multiply-add
    }
}
#undef BQP_DOT4_FMAC
#undef BQP_DOT4_ZERO

// the values of the four 16-lane rows (lane 16 q + l%16, q = 0..3) in lane l of every row: the
// four xrow_bcast<q> sharing their swaps (one v_permlane16_swap pair, two v_permlane32_swap pairs)
template <typename T>
__device__ __forceinline__ void xrow_gather(T v, T (&g)[4]) {
    T a = v, b = v;
    pl16_swap(a, b);                 // a: rows (0, 0, 2, 2), b: rows (1, 1, 3, 3)
    g[0] = a; g[2] = a;
    pl32_swap(g[0], g[2]);           // row 0 everywhere, row 2 everywhere
    g[1] = b; g[3] = b;
    pl32_swap(g[1], g[3]);           // row 1, row 3
}

template <int CTRL, typename T, int KI, int KO>
__device__ __forceinline__ void tsum_step(const T (&in)[KI], T (&out)[KO], bool hi) {
#pragma unroll
    for (int p = 0; p < KO; ++p) {
        const T a = in[2 * p];
        const T b = (2 * p + 1 < KI) ? in[2 * p + 1] : T(0);
        const T keep = hi ? b : a;
        const T send = hi ? a : b;
        out[p] = keep + dpp_mov0<CTRL>(send);
    }
}
template <typename T, int K>
__device__ __forceinline__ T wsum_t(const T (&v)[K], int lane) {
    static_assert(K >= 2 && K <= 32, "wsum_t: 2..32 values");
    constexpr int K1 = (K + 1) / 2, K2 = (K1 + 1) / 2, K3 = (K2 + 1) / 2, K4 = (K3 + 1) / 2;
    T w1[K1], w2[K2], w3[K3], w4[K4];
    tsum_step<0xB1>(v, w1, (lane & 1) != 0);     // quad_perm [1,0,3,2]
    tsum_step<0x4E>(w1, w2, (lane & 2) != 0);    // quad_perm [2,3,0,1]
    tsum_step<0x124>(w2, w3, (lane & 4) != 0);   // row_ror:4
    tsum_step<0x128>(w3, w4, (lane & 8) != 0);   // row_ror:8
    T a = w4[0], b = T(0);
    if constexpr (K4 > 1) b = w4[K4 - 1];
    pl16_swap(a, b);                             // even rows: value a over rows {0,1} / {2,3}
    T c = a + b, d = c;
    pl32_swap(c, d);                             // halves {0,1} + {2,3}
    return c + d;
}

}  // namespace bqp
