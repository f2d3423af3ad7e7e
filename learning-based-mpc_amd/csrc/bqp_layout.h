// bqp_layout.h — where every array of the handle's device workspaces lies.
//
// One struct per buffer, built from integers alone: the byte offsets of its arrays and the bytes
// to reserve.  bqp_api.cpp reserves L.bytes and forms every pointer as base + region offset from
// the same struct, so the size and the pointers cannot disagree.  Host-only, plain C++17, no HIP:
// tests/host/layout_check.cpp compiles it with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace bqp::layout {

// bytes [off, off + bytes) of a buffer
struct Region { size_t off = 0, bytes = 0; };

// bump allocator over byte offsets; `bytes` is the running total.  Every layout below is an
// arena that keeps the regions it handed out
struct Arena {
    size_t bytes = 0;
    void align_to(size_t align) { bytes = (bytes + align - 1) / align * align; }
    Region take_aligned(size_t n, size_t align) {
        align_to(align);
        bytes += n;
        return {bytes - n, n};
    }
    template <class T>
    Region take(size_t n) { return take_aligned(sizeof(T) * n, alignof(T)); }
    void skip(size_t n) { bytes += n; }   // padding that belongs to no region
};

template <class T>
inline T* at(void* base, const Region& r) { return (T*)((char*)base + r.off); }

// Slack inherited from the first version of the host layer; what needs it, if anything, is
// unknown.  Kept byte for byte: removing any of it is a decision of its own.
constexpr size_t WORK_STATS_SLACK = 8 * sizeof(double);    // after work's stats
constexpr size_t DWORK_STATS_SLACK = 8 * sizeof(double);   // after dwork's stats
constexpr size_t LWORK_INT_SLACK = 3 * sizeof(int);        // after lwork's ndone
constexpr size_t CWORK_SQP_INT_SLACK = 1 * sizeof(int);    // after the SQP loop's nfin

// work: the structured solve's prepared tables and per-instance records.
//   H (N+1) x hstride, F nv x mpad, stats batch x stats_w, [stamps batch x stamps_per_instance:
//   the diagnostic build's phase cycle counts, 0 in the product], repair marks (one int per
//   instance), queue counters (nqueues ints); the two int arrays each end on a double boundary
struct Work : Arena {
    Region H, F, stats, stamps, marks, queues;
    Work(size_t N, size_t hstride, size_t nv, size_t mpad, size_t batch, size_t stats_w,
         size_t stamps_per_instance, size_t nqueues) {
        H = take<double>((N + 1) * hstride);
        F = take<double>(nv * mpad);
        stats = take<double>(batch * stats_w);
        skip(WORK_STATS_SLACK);
        stamps = take<double>(batch * stamps_per_instance);
        marks = take<int>(batch);
        align_to(alignof(double));
        queues = take<int>(nqueues);
        align_to(alignof(double));
    }
};

// hwork: the mixed mode's fp32 -> fp64 handoff.  One record of hand_floats floats per instance at
// a stride of whole 64-float blocks, then per instance the fp32 phase's exit flag, its iteration
// count and the continuation's exit flag
struct Hwork : Arena {
    size_t stride;   // floats per record
    Region records, flags, iters, cont;
    Hwork(size_t hand_floats, size_t batch) : stride((hand_floats + 63) & ~(size_t)63) {
        records = take<float>(stride * batch);
        flags = take<int>(batch);
        iters = take<int>(batch);
        cont = take<int>(batch);
    }
};

// lwork: the learned-model SQP's per-instance state (n variables, nr residual rows, m constraint
// rows, ntrial line-search trials; Jr2 / Tr2 only with the exact Hessian).  ndone follows done
// directly: one memset zeroes both
struct Lwork : Arena {
    Region Jr, er, H, f, bsh, lam, d, cost0, costT, stat, cprev, Jr2, Tr2;
    Region qpflag, hused, done, ndone;
    Lwork(size_t B, size_t N, size_t n, size_t nr, size_t m, size_t ntrial, bool hessian) {
        const size_t n2 = hessian ? B * 3 * N * n : 0;
        Jr = take<double>(B * nr * n);
        er = take<double>(B * nr);
        H = take<double>(B * n * n);
        f = take<double>(B * n);
        bsh = take<double>(B * m);
        lam = take<double>(B * m);
        d = take<double>(B * n);
        cost0 = take<double>(B);
        costT = take<double>(B * ntrial);
        stat = take<double>(B);
        cprev = take<double>(B);
        Jr2 = take<double>(n2);
        Tr2 = take<double>(n2);
        qpflag = take<int>(B);
        hused = take<int>(B);
        done = take<int>(B);
        ndone = take<int>(1);
        skip(LWORK_INT_SLACK);
    }
};

// nwork: the nonlinear MPC SQP's per-instance state (horizon N: n = N + 1 variables, nr = 5 N + 8
// residual rows, m constraint rows, ntrial line-search trials).  C is the instance's own
// constraint Jacobian (column-major m x n: 1.3 MB at N = 100 with the 616-row terminal set), so
// the bytes grow with the batch as no other workspace does; every count is size_t from the
// start.  ndone follows done directly: one memset zeroes both
struct Nwork : Arena {
    size_t n, nr;
    Region Jr, er, H, f, C, rhs, lam, d, cost0, costT, violT, stat, cprev, nu;
    Region qpflag, done, ndone;
    Nwork(size_t B, size_t N, size_t m, size_t ntrial) : n(N + 1), nr(5 * N + 8) {
        Jr = take<double>(B * nr * n);
        er = take<double>(B * nr);
        H = take<double>(B * n * n);
        f = take<double>(B * n);
        C = take<double>(B * m * n);
        rhs = take<double>(B * m);
        lam = take<double>(B * m);
        d = take<double>(B * n);
        cost0 = take<double>(B);
        costT = take<double>(B * ntrial);
        violT = take<double>(B * ntrial);
        stat = take<double>(B);
        cprev = take<double>(B);
        nu = take<double>(B);
        qpflag = take<int>(B);
        done = take<int>(B);
        ndone = take<int>(1);
    }
};

// nwork on the stage route (bqp_nmpc_dims.subproblem = 1): no Jr, H or C.  Per instance the stage
// problem the structured solve reads (A 16 N, B 4 N, w 6 (N+1), bounds, hp), that solve's outputs
// (x, u, theta, fval, lam_x, lam_u, lam_p, exit flag), the SQP's vectors as Nwork has them, and
// the back-map's f and C'lam (n each); shared by the batch the cost blocks W (36 (N+1)), the
// polytope matrix Fp (6 mp), the zero initial state and the bound map (map_bytes, 8-aligned).
// 79 KB per instance at N = 100 with the 616-row terminal set, against Nwork's 1.8 MB.
// ndone follows done directly: one memset zeroes both
struct NworkStage : Arena {
    size_t n;
    Region A, B, w, xlb, xub, ulb, uub, hp, xo, uo, tho, fv, lamx, lamu, lamp;
    Region rhs, lam, d, f, ctl, cost0, costT, violT, stat, cprev, nu;
    Region xsl, xsq, sx, pen0, plin;   // soft state rows (soft = 1); empty otherwise
    Region Xw, cdef, piw, sw, gn, pimax;   // multiple shooting (dms = 1); empty otherwise
    Region W, Fp, x0z, map;
    Region sflag, qpflag, done, ndone;
    NworkStage(size_t Bt, size_t N, size_t mp, size_t m, size_t ntrial, size_t map_bytes, size_t soft = 0,
               size_t dms = 0)
        : n(N + 1) {
        A = take<double>(Bt * N * 16);
        B = take<double>(Bt * N * 4);
        w = take<double>(Bt * (N + 1) * 6);
        xlb = take<double>(Bt * (N + 1) * 4);
        xub = take<double>(Bt * (N + 1) * 4);
        ulb = take<double>(Bt * N);
        uub = take<double>(Bt * N);
        hp = take<double>(Bt * mp);
        xo = take<double>(Bt * (N + 1) * 4);
        uo = take<double>(Bt * N);
        tho = take<double>(Bt);
        fv = take<double>(Bt);
        lamx = take<double>(Bt * (N + 1) * 8);
        lamu = take<double>(Bt * N * 2);
        lamp = take<double>(Bt * mp);
        rhs = take<double>(Bt * m);
        lam = take<double>(Bt * m);
        d = take<double>(Bt * n);
        f = take<double>(Bt * n);
        ctl = take<double>(Bt * n);
        cost0 = take<double>(Bt);
        costT = take<double>(Bt * ntrial);
        violT = take<double>(Bt * ntrial);
        stat = take<double>(Bt);
        cprev = take<double>(Bt);
        nu = take<double>(Bt);
        // the structured solve's shared weight tables and its slacks s_x, the penalty at the
        // iterate and the sub-problem's model penalty
        xsl = take<double>(soft * (N + 1) * 4);
        xsq = take<double>(soft * (N + 1) * 4);
        sx = take<double>(soft * Bt * (N + 1) * 8);
        pen0 = take<double>(soft * Bt);
        plin = take<double>(soft * Bt);
        // the iterate's states where the caller keeps none, the defects c_k, the structured solve's
        // pi, and the back-map's sum w_k'v_k, |grad J| and max |pi|
        Xw = take<double>(dms * Bt * (N + 1) * 4);
        cdef = take<double>(dms * Bt * N * 4);
        piw = take<double>(dms * Bt * N * 4);
        sw = take<double>(dms * Bt);
        gn = take<double>(dms * Bt);
        pimax = take<double>(dms * Bt);
        W = take<double>((N + 1) * 36);
        Fp = take<double>(mp * 6);
        x0z = take<double>(4);
        map = take_aligned(map_bytes, alignof(double));
        sflag = take<int>(Bt);
        qpflag = take<int>(Bt);
        done = take<int>(Bt);
        ndone = take<int>(1);
    }
};

// dwork: the dense kernel's scratch (work_doubles per instance) and its stats
struct Dwork : Arena {
    Region scratch, stats;
    Dwork(size_t work_doubles, size_t batch, size_t stats_w) {
        scratch = take<double>(work_doubles * batch);
        stats = take<double>(batch * stats_w);
        skip(DWORK_STATS_SLACK);
    }
};

// cwork of the structured closed loop: measured state, the step's solution (x, u, theta), the
// learning window (q points of 8 doubles per instance; q = 0 without learning) and exit flags
struct CworkOcp : Arena {
    Region s, x, u, theta, window, flags;
    CworkOcp(size_t B, size_t nx, size_t nu, size_t np, size_t N, size_t q) {
        s = take<double>(B * nx);
        x = take<double>(B * (N + 1) * nx);
        u = take<double>(B * N * nu);
        theta = take<double>(B * np);
        window = take<double>(B * q * 8);
        flags = take<int>(B);
    }
};

// cwork of the closed loop with a reference schedule (bqp_closed_loop_track): measured state, the
// step's solution (x, u, theta), the step's linear term w_t = w + Wr r_t (nw = (N+1) nv doubles
// per instance; nw = 0 without a schedule) and exit flags
struct CworkTrack : Arena {
    Region s, x, u, theta, w, flags;
    CworkTrack(size_t B, size_t nx, size_t nu, size_t np, size_t N, size_t nw) {
        s = take<double>(B * nx);
        x = take<double>(B * (N + 1) * nx);
        u = take<double>(B * N * nu);
        theta = take<double>(B * np);
        w = take<double>(B * nw);
        flags = take<int>(B);
    }
};

// cwork of the learned-model SQP loop: measured state, SQP iterate (n), the step's constraint rhs
// (m), first input, window; exit flags, SQP iteration counts, and the asynchronous loop's step
// counters.  nfin follows ts directly: one memset zeroes both
struct CworkSqp : Arena {
    Region s, z, bin, u0, window, flags, iters, ts, nfin;
    CworkSqp(size_t B, size_t nx, size_t n, size_t m, size_t q) {
        s = take<double>(B * nx);
        z = take<double>(B * n);
        bin = take<double>(B * m);
        u0 = take<double>(B);
        window = take<double>(B * q * 8);
        flags = take<int>(B);
        iters = take<int>(B);
        ts = take<int>(B);
        nfin = take<int>(1);
        skip(CWORK_SQP_INT_SLACK);
    }
};

// cwork of the nonlinear MPC loop: measured deviation state (the plant kernel's, nx = 4), SQP
// iterate (n), exit flags and iteration counts of the step.  The asynchronous loop (own_step)
// adds the instances' step counters, the count of finished instances - nfin follows ts directly:
// one memset zeroes both - and the measured state in absolute coordinates (4 per instance, the
// solve's x0); the step-synchronous loop's layout is unchanged by it.  Multiple shooting (dms) adds
// the iterate's states (4 n per instance) after everything else; a set-point schedule in the
// asynchronous loop (track) then adds the set-point each instance is at (4 per instance, the
// solve's x_ref), kept as x0 is
struct CworkNmpc : Arena {
    Region s, z, flags, iters, ts, nfin, x0, Xit, xr;
    CworkNmpc(size_t B, size_t n, bool own_step = false, bool dms = false, bool track = false) {
        s = take<double>(B * 4);
        z = take<double>(B * n);
        flags = take<int>(B);
        iters = take<int>(B);
        if (own_step) {
            ts = take<int>(B);
            nfin = take<int>(1);
            x0 = take<double>(B * 4);
        }
        if (dms) Xit = take<double>(B * n * 4);
        if (track) xr = take<double>(B * 4);
    }
};

}  // namespace bqp::layout
