// bqp_api.cpp — implementation of the C ABI declared in include/bqp.h.
//
// Host-side responsibilities only: argument validation, workspace management (grow-only device
// buffers owned by the handle), host<->device staging for the host-pointer entry points, and
// dispatch of the HIP kernels (bqp_ocp.hip, bqp_dense.hip, bqp_prep.hip).  No arithmetic of
// the solve happens on the host: there is no CPU fallback path.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/bqp.h"
#include "bqp_internal.h"
#include "bqp_layout.h"

namespace layout = bqp::layout;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t reserve(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() {
        if (p) hipFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct bqp_handle_s {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    int launches = 0;
    DevBuf work;   // tables + stats (device entry points)
    DevBuf stage;  // staging of host-pointer calls
    DevBuf dwork;  // dense per-instance scratch
    DevBuf lwork;  // learning-based MPC (SQP) buffers
    DevBuf nwork;  // nonlinear MPC (SQP) buffers, every instance's constraint Jacobian included
    DevBuf cwork;  // closed-loop simulation buffers
    DevBuf hwork;  // mixed precision: fp32 -> fp64 handoff records
    DevBuf pwork;  // long-horizon layout: global Riccati tables
    DevBuf wwork;  // per-instance stage-cost tables
    int last_batch = 0;
    int* mixed_flags = nullptr;   // the last mixed-mode solve's fp32-phase flags
    int* mixed_cont = nullptr;    // and its continuation's exit flags (bqp_debug_mixed_flags)
    int mixed_batch = 0;
    int ocp_wpb = 0;              // instances per workgroup of the last structured solve (bqp_debug_ocp_wpb)
    int nmpc_rounds = 0;          // SQP rounds of the last bqp_nmpc_solve_batched_device
    int loop_rounds = -1;         // and of the last bqp_closed_loop_nmpc_device (-1: none yet)
};

namespace {

struct DevScope {
    int prev = -1;
    explicit DevScope(int d) {
        hipGetDevice(&prev);
        if (prev != d) hipSetDevice(d);
    }
    ~DevScope() {
        int cur = -1;
        hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) hipSetDevice(prev);
    }
};

inline size_t span(int batch, int64_t stride, size_t n) {
    return n == 0 ? 0 : (size_t)(batch - 1) * (size_t)stride + n;
}

void resolve(const bqp_options* in, bqp_options* o) {
    bqp_default_options(o);
    if (!in) return;
    if (in->max_iter > 0) o->max_iter = in->max_iter;
    if (in->tol_stat > 0) o->tol_stat = in->tol_stat;
    if (in->tol_feas > 0) o->tol_feas = in->tol_feas;
    if (in->tol_comp > 0) o->tol_comp = in->tol_comp;
    if (in->tau > 0 && in->tau < 1) o->tau = in->tau;
    o->precision = in->precision;
    o->want_duals = in->want_duals;
    o->polish = in->polish;
}

#define HIP_TRY(x)                                                        \
    do {                                                                  \
        hipError_t _e = (x);                                              \
        if (_e != hipSuccess) {                                           \
            fprintf(stderr, "bqp: %s failed: %s\n", #x, hipGetErrorString(_e)); \
            return BQP_E_HIP;                                             \
        }                                                                 \
    } while (0)

#define BQP_TRY(x) do { const int _rc = (x); if (_rc) return _rc; } while (0)

// an event owned by an entry point's scope: destroyed on every return (HIP_TRY included)
struct EventGuard {
    hipEvent_t e = nullptr;
    ~EventGuard() { if (e) hipEventDestroy(e); }
};

// diagnostic build (make stamps): phase cycle counts per instance in the work buffer
#ifdef BQP_STAMPS
constexpr int STAMPS_PER_INSTANCE = 32;
#else
constexpr int STAMPS_PER_INSTANCE = 0;
#endif

layout::Work work_layout(int N, int nv, int mpad, int batch) {
    return layout::Work(N, nv * nv + 1, nv, mpad, batch, bqp::STATS_W, STAMPS_PER_INSTANCE, bqp::OCP_QUEUES);
}

// Slack the two solve entry points reserve past their packed staging (16 doubles + 64 bytes):
// inherited, need unknown (bqp_layout.h keeps the other buffers' slack)
constexpr size_t STAGE_SOLVE_SLACK = 16 * sizeof(double) + 64;

// Staging of a host-pointer entry point in h->stage: the inputs' device copies, then the outputs',
// packed in the order they are registered.  Registration takes the address of the pointer that
// is to hold the device copy; commit() reserves the buffer, sets those pointers and issues the
// H2D copies on h->stream; finish() copies back the outputs the caller asked for and waits.
struct Stage : layout::Arena {
    struct Item { void* slot; const void* src; void* host; layout::Region r; };
    bqp_handle_s* h;
    std::vector<Item> items;
    explicit Stage(bqp_handle_s* h_) : h(h_) { items.reserve(32); }
    // n elements of src; a null src or n = 0 registers nothing and leaves *dev null.  back: the
    // call updates the array in place, so it is an output too
    template <class P, class T>
    void in(P* dev, const T* src, size_t n, T* back = nullptr) {
        *dev = nullptr;
        if (src && n) items.push_back({dev, src, back, take<T>(n)});
    }
    // n elements that are input and output (the call may leave some of them as they were): as out(),
    // with the caller's contents copied to the device first.  A null host array is a plain out()
    template <class T>
    void inout(T** dev, size_t n, T* host, size_t align = alignof(T)) {
        items.push_back({dev, n ? host : nullptr, host, take_aligned(sizeof(T) * n, align)});
    }
    // n elements copied to host by finish() unless host is null
    template <class T>
    void out(T** dev, size_t n, T* host, size_t align = alignof(T)) {
        items.push_back({dev, nullptr, host, take_aligned(sizeof(T) * n, align)});
    }
    int commit(size_t slack = 0) {
        HIP_TRY(h->stage.reserve(bytes + slack));
        for (const Item& e : items) {
            char* p = (char*)h->stage.p + e.r.off;
            memcpy(e.slot, &p, sizeof(p));   // *dev = p, whatever *dev points to
            if (e.src) HIP_TRY(hipMemcpyAsync(p, e.src, e.r.bytes, hipMemcpyHostToDevice, h->stream));
        }
        return BQP_OK;
    }
    int finish() {
        for (const Item& e : items)
            if (e.host && e.r.bytes)
                HIP_TRY(hipMemcpyAsync(e.host, (char*)h->stage.p + e.r.off, e.r.bytes, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return BQP_OK;
    }
};

}  // namespace

extern "C" {

const char* bqp_version(void) { return "bqp 0.1.0 (gfx950, structured Riccati Mehrotra IPM)"; }

#ifndef BQP_SRC_SHA1
#define BQP_SRC_SHA1 "unknown"
#endif
const char* bqp_build_source_sha1(void) { return BQP_SRC_SHA1; }

void bqp_default_options(bqp_options* o) {
    if (!o) return;
    o->max_iter = 50;
    o->tol_stat = 1e-8;
    o->tol_feas = 1e-10;
    o->tol_comp = 1e-14;
    o->tau = 0.995;
    o->precision = 0;
    o->want_duals = 0;
    o->polish = 0;
}

int bqp_create(bqp_handle* h, int device) {
    if (!h) return BQP_E_ARG;
    *h = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return BQP_E_NODEV;
    int dev = device;
    if (dev < 0) hipGetDevice(&dev);
    if (dev >= n) return BQP_E_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return BQP_E_NODEV;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        fprintf(stderr, "bqp: device %d is %s; this build targets gfx950 only\n", dev, prop.gcnArchName);
        return BQP_E_NODEV;
    }
    bqp_handle_s* s = new bqp_handle_s();
    s->device = dev;
    DevScope ds(dev);
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) {
        delete s;
        return BQP_E_HIP;
    }
    *h = s;
    return BQP_OK;
}

int bqp_destroy(bqp_handle h) {
    if (!h) return BQP_OK;
    {
        DevScope ds(h->device);
        if (h->stream) hipStreamSynchronize(h->stream);
        h->work.release();
        h->stage.release();
        h->dwork.release();
        h->lwork.release();
        h->nwork.release();
        h->cwork.release();
        h->hwork.release();
        h->pwork.release();
        h->wwork.release();
        if (h->ev0) hipEventDestroy(h->ev0);
        if (h->ev1) hipEventDestroy(h->ev1);
        if (h->stream) hipStreamDestroy(h->stream);
    }
    delete h;
    return BQP_OK;
}

int bqp_debug_ocp_wpb(bqp_handle h, int* wpb) {
    if (!h || !wpb || h->ocp_wpb <= 0) return BQP_E_ARG;
    *wpb = h->ocp_wpb;
    return BQP_OK;
}

int bqp_debug_mixed_flags(bqp_handle h, int batch, int* flags) {
    if (!h || !flags || batch <= 0) return BQP_E_ARG;
    if (!h->mixed_flags || batch != h->mixed_batch) return BQP_E_ARG;
    DevScope ds(h->device);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<int> f2((size_t)2 * batch);
    HIP_TRY(hipMemcpy(f2.data(), h->mixed_flags, sizeof(int) * batch, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(f2.data() + batch, h->mixed_cont, sizeof(int) * batch, hipMemcpyDeviceToHost));
    // the retry launch solved again the instances whose continuation ended != 1 after a warm
    // start (fp32-phase flag 0 / 1): reported as 2
    for (int i = 0; i < batch; ++i) {
        const int hf = f2[i], c2 = f2[(size_t)batch + i];
        flags[i] = ((hf == 0 || hf == 1) && c2 != 1) ? 2 : hf;
    }
    return BQP_OK;
}

int bqp_last_kernel_ms(bqp_handle h, double* ms, int* launches) {
    if (!h || !ms) return BQP_E_ARG;
    *ms = 0.0;
    if (launches) *launches = h->launches;
    if (!h->timed) return BQP_OK;
    DevScope ds(h->device);
    HIP_TRY(hipEventSynchronize(h->ev1));
    float f = 0.f;
    HIP_TRY(hipEventElapsedTime(&f, h->ev0, h->ev1));
    *ms = (double)f;
    return BQP_OK;
}

int bqp_last_loop_rounds(bqp_handle h, int* rounds) {
    if (!h || !rounds || h->loop_rounds < 0) return BQP_E_ARG;
    *rounds = h->loop_rounds;
    return BQP_OK;
}

// ------------------------------------------------------------------------------------------
// structured OCP
// ------------------------------------------------------------------------------------------
// soft state bounds: a weight array is given (bqp_ocp_data.xs_lin / xs_quad)
static bool ocp_soft(const bqp_ocp_data* D) { return D->xs_lin || D->xs_quad; }

static int ocp_check(const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D) {
    if (!d || !D || batch <= 0) return BQP_E_ARG;
    if (d->nx <= 0 || d->nu <= 0 || d->np <= 0 || d->N < 1 || d->n_poly < 0) return BQP_E_ARG;
    if (d->poly_stage < 0 || d->poly_stage > d->N) return BQP_E_ARG;
    if (!D->A || !D->B || !D->W || !D->x0) return BQP_E_ARG;
    if (d->n_poly > 0 && (!D->Fp || !D->hp)) return BQP_E_ARG;
    if (!bqp::ocp_supported(d->nx, d->nu, d->np)) return BQP_E_UNSUPPORTED;
    if (d->N > 127 || bqp::ocp_rpl_for(std::max(d->n_poly, 1)) < 0) return BQP_E_UNSUPPORTED;
    if (D->sW != 0 && D->sW < (int64_t)(d->N + 1) * (d->nx + d->nu + d->np) * (d->nx + d->nu + d->np))
        return BQP_E_ARG;                                     // per-instance stage costs overlap
    if (D->sFp != 0 && D->sFp < (int64_t)d->n_poly * (d->nx + d->nu + d->np)) return BQP_E_ARG;
    if (d->stage_models != 0 && d->stage_models != 1) return BQP_E_ARG;
    if (d->stage_models) {
        // per-stage models: a per-instance stride spans the instance's whole schedule
        const int64_t N = d->N, nx = d->nx, nu = d->nu;
        if (D->sA != 0 && D->sA < N * nx * nx) return BQP_E_ARG;
        if (D->sB != 0 && D->sB < N * nx * nu) return BQP_E_ARG;
        if (D->c && D->sc != 0 && D->sc < N * nx) return BQP_E_ARG;
    } else if (D->skip) {
        return BQP_E_UNSUPPORTED;
    }
    // soft state bounds: a per-instance stride spans the instance's (N + 1) nx weights
    if (ocp_soft(D) && (D->sxs < 0 || (D->sxs != 0 && D->sxs < (int64_t)(d->N + 1) * d->nx))) return BQP_E_ARG;
    return BQP_OK;
}

// host entry points: every weight finite and >= 0 (the device entries leave that to the caller)
static int ocp_soft_host_check(const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D) {
    if (!ocp_soft(D)) return BQP_OK;
    const size_t n = (size_t)(d->N + 1) * d->nx, tot = D->sxs == 0 ? n : (size_t)(batch - 1) * (size_t)D->sxs + n;
    for (const double* w : {D->xs_lin, D->xs_quad})
        if (w)
            for (size_t i = 0; i < tot; ++i)
                if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return BQP_E_ARG;
    return BQP_OK;
}

// elements of the model arrays A, B, c per instance: one model, or N of them (stage_models)
static size_t ocp_model_blocks(const bqp_ocp_dims* d) { return d->stage_models ? (size_t)d->N : 1; }

int bqp_solve_ocp_batched_device(bqp_handle h, const bqp_ocp_dims* d, int batch,
                                 const bqp_ocp_data* D, const bqp_options* opt, double* x,
                                 double* u, double* theta, double* fval, int* exitflag,
                                 bqp_output* out, const bqp_ocp_duals* duals, void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(ocp_check(d, batch, D));
    if (!x || !u || !theta || !exitflag) return BQP_E_ARG;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(opt, &o);
    if (o.precision < 0 || o.precision > 2) return BQP_E_ARG;
    // per-stage models: fp64 instantiations only (their repair launch carries the per-stage
    // models: the polish runs on the same Riccati routines as the solve)
    // soft state bounds: the soft instantiations are per-stage-model ones (a one-model problem reads
    // block 0 of A, B, c at every stage), fp64, without the active-set polish
    const bool soft = ocp_soft(D);
    const bool stg = d->stage_models == 1 || soft;
    if (stg && o.precision != 0) return BQP_E_UNSUPPORTED;
    if (soft) o.polish = -1;
    const bool f32 = o.precision == 1;     // fp32 instantiation (bqp_ocp_f32.hip)
    // fp32 phase, then fp64 from the fp32 iterate; long horizons only (N + 1 > 64, the
    // instantiations that carry the handoff): shorter ones are solved in fp64 alone
    const bool mixed = o.precision == 2 && d->N + 1 > 64;
    bqp_options o32 = o;
    // fp32 arithmetic cannot resolve the fp64 defaults: floor the stopping tolerances
    o32.tol_stat = std::max(o.tol_stat, 1e-5);
    o32.tol_feas = std::max(o.tol_feas, 1e-6);
    o32.tol_comp = std::max(o.tol_comp, 1e-9);
    if (mixed) {
        // hand over once the fp32 iterate is feasible to 1e-6 and mu <= 1e-6: the fp64 launch then
        // needs ~4 iterations and ends at the fp64 solve's KKT accuracy (duals within ~3e-8 of
        // lambda*); later switches (mu 1e-7 .. 1e-9) save 3-7 % of the time but leave the duals
        // of some instances at 1e-7 .. 2e-7 (tools/diag_mixed.py, profiles/r02_mx/diag_switch.log).
        // BQP_MIXED_MU overrides, for that sweep (values outside (0, 1e-3] are ignored).
        o32.tol_comp = std::max(o.tol_comp, 1e-6);
        if (const char* e = getenv("BQP_MIXED_MU")) {
            char* end = nullptr;
            const double v = strtod(e, &end);
            if (end != e && *end == '\0' && v > 0.0 && v <= 1e-3) o32.tol_comp = v;
        }
    }
    if (f32) o = o32;
    const int nx = d->nx, nu = d->nu, np = d->np, N = d->N;
    const int nv = nx + nu + np;
    const int mp = d->n_poly;
    const int hstride = nv * nv + 1;
    const int mpad = 64 * bqp::ocp_rpl_for(std::max(mp, 1));   // = the kernel's RPL * 64
    // per-instance polytope (sFp != 0): each instance's LDS slot holds its own NV x mpad table
    const bool fpi = mp > 0 && D->sFp != 0;
    const bool hinst = D->sW != 0;        // per-instance stage costs (the instance's H table)
    // long horizons (two stages per lane): H read from global, Riccati tables in global scratch,
    // polytope rhs / box bounds in the shared tables when the batch shares them (QpLds lng)
    // (fp64 instantiation only; the fp32 one keeps the plain layout)
    struct Shared { bool lng, hpsh, bndsh; int sh_F, sh_hp, sh_bnd, doubles; };
    auto shared_layout = [&](bool single) {
        Shared o;
        o.lng = !single && N + 1 > 64;
        o.hpsh = mp > 0 && D->shp == 0;       // the shared polytope rhs (every horizon)
        o.bndsh = o.lng && D->sxb == 0 && D->sub == 0;
        const int nbr = (N + 1) * 2 * (nx + nu);
        int sh = (o.lng || hinst) ? 0 : (N + 1) * hstride;
        o.sh_F = sh;
        sh += fpi ? 0 : nv * mpad;
        o.sh_hp = o.hpsh ? sh : -1;
        sh += o.hpsh ? mpad : 0;
        o.sh_bnd = o.bndsh ? sh : -1;
        sh += o.bndsh ? nbr : 0;
        o.doubles = (sh + 1) & ~1;   // elements
        return o;
    };
    const Shared L64 = shared_layout(f32), L32 = shared_layout(true);
    const bool lng = L64.lng;
    // instances per workgroup (two waves each) that fit the 160 KB of LDS
    auto fit_wpb = [&](bool single, int& wpb) -> bool {
        const Shared& S = single ? L32 : L64;
        const int shared_doubles = S.doubles;
        const int per_wave = single ? bqp::ocp_wave_lds_doubles_f32(N, nx, nu, np, mpad, fpi, false, S.hpsh, false, hinst)
                                    : bqp::ocp_wave_lds_doubles(N, nx, nu, np, mpad, fpi, S.lng, S.hpsh, S.bndsh, hinst, stg);
        // 160 KB per workgroup less the repair kernel's 256 B of static LDS (its
        // __syncthreads_or scratch): N = 50 at two instances per workgroup sits exactly there
        const size_t lds_budget = (160 * 1024 - 256) / (single ? sizeof(float) : sizeof(double));
        // long horizons (N + 1 > 64, two stages per lane) are compiled for <= 256 threads per
        // workgroup: one wave per SIMD, whose 512 registers hold the doubled stage state
        wpb = (N + 1 > 64) ? 2 : 4;
        // diagnostic (the A/B library variants of `make ab`): BQP_OCP_WPB sets the instances per
        // workgroup the LDS budget then caps
        if (const char* e = getenv("BQP_OCP_WPB")) {
            const int v = atoi(e);
            if (v >= 1 && v <= 8) wpb = v;
        }
        while (wpb > 1 && (size_t)shared_doubles + (size_t)wpb * per_wave > lds_budget) --wpb;
        return (size_t)shared_doubles + (size_t)per_wave <= lds_budget;
    };
    int wpb = 1, wpb32 = 1;
    if (!fit_wpb(f32, wpb)) return BQP_E_UNSUPPORTED;
    if (mixed && !fit_wpb(true, wpb32)) return BQP_E_UNSUPPORTED;
    h->ocp_wpb = wpb;
    // workspace: H, Fp, stats, the repair marks, the work-queue counters of the launches
    const layout::Work WL = work_layout(N, nv, mpad, batch);
    HIP_TRY(h->work.reserve(WL.bytes));
    double* Hd = layout::at<double>(h->work.p, WL.H);
    double* Fd = layout::at<double>(h->work.p, WL.F);
    double* Sd = layout::at<double>(h->work.p, WL.stats);
    int* polneed = layout::at<int>(h->work.p, WL.marks);
    int* queues = layout::at<int>(h->work.p, WL.queues);
    const double* Hinst = nullptr;
    if (hinst) {   // per-instance prepared stage-cost tables
        HIP_TRY(h->wwork.reserve(sizeof(double) * (size_t)batch * (N + 1) * hstride));
        HIP_TRY(bqp::launch_ocp_prep_h(D->W, D->sW, batch, nx, nu, np, N, hstride, (double*)h->wwork.p, st));
        Hinst = (const double*)h->wwork.p;
    }
    void* Pg = nullptr;
    if (lng) {   // global Riccati tables of the long-horizon layout
        HIP_TRY(h->pwork.reserve(sizeof(double) * (size_t)batch * (N + 1) * bqp::ocp_pstride(nx + np)));
        Pg = h->pwork.p;
    }
    // Shared tables at short horizons: the solve and repair kernels form the prepared layout
    // themselves while they stage the caller's W and Fp into LDS, so the call has no prep launch
    // (and no dependent dispatch in front of the solve).  Long horizons read H from global, and
    // per-instance W / Fp have their own paths: those keep the prepared tables.
    // BQP_OCP_PREP_LAUNCH=1 forces the prep launch everywhere (A/B timing, the bitwise test).
    const char* prep_env = getenv("BQP_OCP_PREP_LAUNCH");
    const bool raw_tables = N + 1 <= 64 && !hinst && !fpi && !(prep_env && atoi(prep_env) == 1);
    if (!raw_tables)
        HIP_TRY(bqp::launch_ocp_prep(D->W, mp > 0 ? D->Fp : D->W, nx, nu, np, N, mp, d->poly_stage,
                                     hstride, mpad, Hd, Fd, queues, st));
    bqp::OcpKernelArgs a;
    memset(&a, 0, sizeof(a));
    a.raw_tables = raw_tables ? 1 : 0;
    a.queue_zeroed = raw_tables ? 0 : 1;
    // the solve launch's work queue (used when the batch exceeds the resident workgroups)
    a.queue = queues;
    a.N = N; a.mp = mp; a.kp = d->poly_stage; a.batch = batch; a.wpb = wpb;
    const Shared& LS = f32 ? L32 : L64;
    a.hstride = hstride; a.mpad = mpad; a.shared_doubles = LS.doubles;
    a.Pg = Pg; a.sh_F = LS.sh_F; a.sh_hp = LS.sh_hp; a.sh_bnd = LS.sh_bnd; a.H_inst = Hinst;
    a.max_iter = o.max_iter; a.tol_stat = o.tol_stat; a.tol_feas = o.tol_feas;
    a.tol_comp = o.tol_comp; a.tau = o.tau;
    a.polish = o.polish < 0 ? 0 : (o.polish == 0 ? 1 : std::min(o.polish, 2));
    a.pol_need = polneed;
    a.H = raw_tables ? D->W : Hd;
    a.Fp = raw_tables ? (mp > 0 ? D->Fp : D->W) : Fd;
    a.A = D->A; a.B = D->B; a.c = D->c; a.w = D->w; a.xlb = D->xlb; a.xub = D->xub;
    a.ulb = D->ulb; a.uub = D->uub; a.hp = mp > 0 ? D->hp : Hd; a.x0 = D->x0;
    a.sA = D->sA; a.sB = D->sB; a.sc = D->sc; a.sw = D->sw; a.sxb = D->sxb; a.sub = D->sub;
    a.shp = D->shp; a.sx0 = D->sx0;
    if (fpi) { a.Fp_inst = D->Fp; a.sFp = D->sFp; }
    a.stage_models = stg ? 1 : 0;
    a.skip = stg ? D->skip : nullptr;
    if (soft) {
        a.soft = 1;
        a.one_model = d->stage_models == 1 ? 0 : 1;
        a.xs_lin = D->xs_lin; a.xs_quad = D->xs_quad; a.sxs = D->sxs;
        a.sx_out = duals ? duals->s_x : nullptr;
    }
    a.x = x; a.u = u; a.theta = theta; a.fval = fval; a.exitflag = exitflag; a.stats = Sd;
    if (duals) {
        a.pi_out = duals->pi; a.lamx_out = duals->lam_x; a.lamu_out = duals->lam_u;
        a.lamp_out = duals->lam_p;
    }
#ifdef BQP_STAMPS
    a.stamps = layout::at<double>(h->work.p, WL.stamps);
    h->last_batch = batch;
#endif
    HIP_TRY(hipEventRecord(h->ev0, st));
    if (mixed) {
        // phase 1: fp32 to the floored tolerances, iterate to the handoff records
        const int hf = bqp::ocp_hand_floats(N, nx, nu, np, mp);
        if (hf <= 0) return BQP_E_UNSUPPORTED;
        const layout::Hwork HL(hf, batch);
        const size_t hrec = HL.stride;
        HIP_TRY(h->hwork.reserve(HL.bytes));
        float* hb = layout::at<float>(h->hwork.p, HL.records);
        int* hflag = layout::at<int>(h->hwork.p, HL.flags);
        int* hit = layout::at<int>(h->hwork.p, HL.iters);
        int* c2flag = layout::at<int>(h->hwork.p, HL.cont);    // the continuation's exit flags (diagnostic)
        h->mixed_flags = hflag;
        h->mixed_cont = c2flag;
        h->mixed_batch = batch;
        bqp::OcpKernelArgs a1 = a;
        a1.wpb = wpb32;
        a1.shared_doubles = L32.doubles; a1.sh_F = L32.sh_F; a1.sh_hp = L32.sh_hp; a1.sh_bnd = L32.sh_bnd;
        a1.max_iter = o32.max_iter; a1.tol_stat = o32.tol_stat; a1.tol_feas = o32.tol_feas;
        a1.tol_comp = o32.tol_comp;
        a1.exitflag = hflag;
        a1.hand_out = hb; a1.hand_it = hit; a1.hand_stride = (int64_t)hrec;
        a1.pi_out = a1.lamx_out = a1.lamu_out = a1.lamp_out = nullptr;
        a1.queue = queues + 1;
        HIP_TRY(bqp::launch_ocp_f32(a1, nx, nu, np, st));
        // phase 2: fp64 from the handed-over iterates
        a.hand_in = hb; a.hand_flag = hflag; a.hand_it = hit; a.hand_stride = (int64_t)hrec;
        HIP_TRY(bqp::launch_ocp(a, nx, nu, np, st));
        // (diagnostic record of the continuation's exit flags, for bqp_debug_mixed_flags)
        HIP_TRY(hipMemcpyAsync(c2flag, exitflag, sizeof(int) * batch, hipMemcpyDeviceToDevice, st));
        // phase 3: a continuation that did not converge (-8 / -2 / 0: marginal instances, e.g.
        // nearly infeasible perturbed models) is solved again from the fp64 initial point, so
        // the mixed mode reports the fp64 solve's status there; the others leave at once
        bqp::OcpKernelArgs a3 = a;
        a3.hand_in = nullptr; a3.hand_it = nullptr; a3.redo_flag = hflag;
        a3.queue = nullptr;           // sparse: most workgroups leave at once
        HIP_TRY(bqp::launch_ocp(a3, nx, nu, np, st));
    } else if (f32) {
        HIP_TRY(bqp::launch_ocp_f32(a, nx, nu, np, st));
    } else {
        HIP_TRY(bqp::launch_ocp(a, nx, nu, np, st));
    }
    // repair launch (fp64): the instances the solve launch marked (0 / -8 exits; with polish 2
    // also weakly active rows) are solved again and polished to their active-set solution; a
    // workgroup with no marked instance leaves at once.  The mixed mode repairs with the
    // continuation's arguments.
    if (!f32 && a.polish > 0) HIP_TRY(bqp::launch_ocp(a, nx, nu, np, st, true));
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->timed = true;
    h->launches = (mixed ? 3 : 1) + ((!f32 && a.polish > 0) ? 1 : 0);
    if (out) HIP_TRY(bqp::launch_ocp_finalize(Sd, batch, out, st, a.skip));
    return BQP_OK;
}

// registers the arrays of D with the stage, and nx0 doubles of x0 as the initial states; once
// st.commit() has run, *Dd is D with the device copies for pointers
static void stage_ocp_data(Stage& st, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                           const double* x0, size_t nx0, bqp_ocp_data* Dd) {
    const size_t nx = d->nx, nu = d->nu, N = d->N, mp = d->n_poly, nv = nx + nu + d->np;
    *Dd = *D;
    const size_t nm = ocp_model_blocks(d);
    st.in(&Dd->A, D->A, span(batch, D->sA, nm * nx * nx));
    st.in(&Dd->B, D->B, span(batch, D->sB, nm * nx * nu));
    st.in(&Dd->c, D->c, span(batch, D->sc, nm * nx));
    st.in(&Dd->W, D->W, span(batch, D->sW, (N + 1) * nv * nv));
    st.in(&Dd->w, D->w, span(batch, D->sw, (N + 1) * nv));
    st.in(&Dd->xlb, D->xlb, span(batch, D->sxb, (N + 1) * nx));
    st.in(&Dd->xub, D->xub, span(batch, D->sxb, (N + 1) * nx));
    st.in(&Dd->ulb, D->ulb, span(batch, D->sub, N * nu));
    st.in(&Dd->uub, D->uub, span(batch, D->sub, N * nu));
    st.in(&Dd->Fp, D->Fp, span(batch, D->sFp, mp * nv));
    st.in(&Dd->hp, D->hp, span(batch, D->shp, mp));
    st.in(&Dd->x0, x0, nx0);
    st.in(&Dd->skip, D->skip, (size_t)batch);
    st.in(&Dd->xs_lin, D->xs_lin, span(batch, D->sxs, (N + 1) * nx));
    st.in(&Dd->xs_quad, D->xs_quad, span(batch, D->sxs, (N + 1) * nx));
}

int bqp_solve_ocp_batched(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                          const bqp_options* opt, double* x, double* u, double* theta,
                          double* fval, int* exitflag, bqp_output* out,
                          const bqp_ocp_duals* duals) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(ocp_check(d, batch, D));
    BQP_TRY(ocp_soft_host_check(d, batch, D));
    if (!x || !u || !theta || !exitflag) return BQP_E_ARG;
    DevScope ds(h->device);
    const size_t B = batch, nx = d->nx, nu = d->nu, np = d->np, N = d->N, mp = d->n_poly;
    Stage st(h);
    bqp_ocp_data Dd;
    stage_ocp_data(st, d, batch, D, D->x0, span(batch, D->sx0, nx), &Dd);
    double *xd, *ud, *td, *fd;
    int* ed;
    bqp_output* od;
    bqp_ocp_duals dd = {};
    // with skipped instances (per-stage models) the outputs are arrays updated in place: the
    // caller's contents go to the device first, so that a skipped instance's come back as they were
    const bool inout = D->skip != nullptr;
    auto res = [&](auto** dev, size_t n, auto* host, size_t align) {
        if (inout) st.inout(dev, n, host, align);
        else st.out(dev, n, host, align);
    };
    res(&xd, B * (N + 1) * nx, x, alignof(double));
    res(&ud, B * N * nu, u, alignof(double));
    res(&td, B * np, theta, alignof(double));
    res(&fd, B, fval, alignof(double));
    if (duals) {
        res(&dd.pi, B * N * nx, duals->pi, alignof(double));
        res(&dd.lam_x, B * (N + 1) * nx * 2, duals->lam_x, alignof(double));
        res(&dd.lam_u, B * N * nu * 2, duals->lam_u, alignof(double));
        res(&dd.lam_p, B * mp, duals->lam_p, alignof(double));
        if (duals->s_x) res(&dd.s_x, B * (N + 1) * nx * 2, duals->s_x, alignof(double));
    }
    res(&ed, B, exitflag, alignof(int));
    res(&od, B, out, 64);
    BQP_TRY(st.commit(STAGE_SOLVE_SLACK));
    BQP_TRY(bqp_solve_ocp_batched_device(h, d, batch, &Dd, opt, xd, ud, td, fd, ed, out ? od : nullptr,
                                         duals ? &dd : nullptr, h->stream));
    return st.finish();
}

// ------------------------------------------------------------------------------------------
// dense quadprog
// ------------------------------------------------------------------------------------------
static int dense_check(const bqp_dims* d, int batch, const double* H, const double* f) {
    if (!d || batch <= 0 || !H || !f) return BQP_E_ARG;
    if (d->n <= 0 || d->m < 0 || d->me < 0) return BQP_E_ARG;
    if (d->n > 256 || d->me > 256 || d->m > 8192) return BQP_E_UNSUPPORTED;
    return BQP_OK;
}

int bqp_quadprog_batched_device(bqp_handle h, const bqp_dims* d, int batch, const bqp_strides* s,
                                const double* H, const double* f, const double* A,
                                const double* b, const double* Aeq, const double* beq,
                                const double* lb, const double* ub, const bqp_options* opt,
                                double* x, double* fval, int* exitflag, double* lam_ineqlin,
                                double* lam_eqlin, double* lam_lower, double* lam_upper,
                                bqp_output* out, void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(dense_check(d, batch, H, f));
    if (!x || !exitflag || !s) return BQP_E_ARG;
    if ((d->m > 0 && (!A || !b)) || (d->me > 0 && (!Aeq || !beq))) return BQP_E_ARG;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(opt, &o);
    const int64_t wst = bqp::dense_work_doubles(d->n, d->m, d->me);
    const layout::Dwork DL(wst, batch, bqp::STATS_W);
    HIP_TRY(h->dwork.reserve(DL.bytes));
    double* wk = layout::at<double>(h->dwork.p, DL.scratch);
    double* Sd = layout::at<double>(h->dwork.p, DL.stats);
    bqp::DenseKernelArgs a;
    memset(&a, 0, sizeof(a));
    a.n = d->n; a.m = d->m; a.me = d->me; a.batch = batch; a.max_iter = o.max_iter;
    a.tol_stat = o.tol_stat; a.tol_feas = o.tol_feas; a.tol_comp = o.tol_comp; a.tau = o.tau;
    a.H = H; a.f = f; a.A = A; a.b = b; a.Aeq = Aeq; a.beq = beq; a.lb = lb; a.ub = ub;
    a.sH = s->sH; a.sf = s->sf; a.sA = s->sA; a.sb = s->sb; a.sAeq = s->sAeq; a.sbeq = s->sbeq;
    a.slb = s->slb; a.sub = s->sub;
    a.x = x; a.fval = fval; a.lam_ineqlin = lam_ineqlin; a.lam_eqlin = lam_eqlin;
    a.lam_lower = lam_lower; a.lam_upper = lam_upper; a.exitflag = exitflag; a.stats = Sd;
    a.work = wk; a.work_stride = wst;
    a.polish = o.polish < 0 ? 0 : 1;
    HIP_TRY(hipEventRecord(h->ev0, st));
    HIP_TRY(bqp::launch_dense(a, st));
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->timed = true;
    h->launches = 1;
    if (out) HIP_TRY(bqp::launch_ocp_finalize(Sd, batch, out, st));
    return BQP_OK;
}

int bqp_quadprog_batched(bqp_handle h, const bqp_dims* d, int batch, const bqp_strides* s,
                         const double* H, const double* f, const double* A, const double* b,
                         const double* Aeq, const double* beq, const double* lb, const double* ub,
                         const double* x0, const bqp_options* opt, double* x, double* fval,
                         int* exitflag, double* lam_ineqlin, double* lam_eqlin,
                         double* lam_lower, double* lam_upper, bqp_output* out) {
    (void)x0;
    if (!h) return BQP_E_ARG;
    BQP_TRY(dense_check(d, batch, H, f));
    if (!x || !exitflag) return BQP_E_ARG;
    bqp_strides zs = {};
    if (!s) s = &zs;
    DevScope ds(h->device);
    const size_t B = batch, n = d->n, m = d->m, me = d->me;
    Stage st(h);
    double *Hd, *xd, *fd, *lid, *led, *lld, *lud;
    const double *fi, *Ad, *bd, *Aeqd, *beqd, *lbd, *ubd;
    int* ed;
    bqp_output* od;
    st.in(&Hd, H, span(batch, s->sH, n * n));
    st.in(&fi, f, span(batch, s->sf, n));
    st.in(&Ad, A, span(batch, s->sA, m * n));
    st.in(&bd, b, span(batch, s->sb, m));
    st.in(&Aeqd, Aeq, span(batch, s->sAeq, me * n));
    st.in(&beqd, beq, span(batch, s->sbeq, me));
    st.in(&lbd, lb, span(batch, s->slb, n));
    st.in(&ubd, ub, span(batch, s->sub, n));
    st.out(&xd, B * n, x);
    st.out(&fd, B, fval);
    st.out(&lid, B * m, lam_ineqlin);
    st.out(&led, B * me, lam_eqlin);
    st.out(&lld, B * n, lam_lower);
    st.out(&lud, B * n, lam_upper);
    st.out(&ed, B, exitflag);
    st.out(&od, B, out, 64);
    BQP_TRY(st.commit(STAGE_SOLVE_SLACK));
    // quadprog semantics: the symmetric part of H (a no-op on a symmetric H)
    HIP_TRY(bqp::launch_dense_symmetrize(Hd, (int)n, s->sH ? batch : 1, s->sH, h->stream));
    BQP_TRY(bqp_quadprog_batched_device(h, d, batch, s, Hd, fi, Ad, bd, Aeqd, beqd, lbd, ubd, opt, xd, fd,
                                        ed, lid, led, lld, lud, out ? od : nullptr, h->stream));
    return st.finish();
}

// ------------------------------------------------------------------------------------------
// learning-based MPC: Nadaraya-Watson oracle and the Gauss-Newton SQP (bqp_lbmpc.hip)
// ------------------------------------------------------------------------------------------
constexpr int LB_NTRIAL = 8;   // line-search trial steps per SQP iteration
// SQP iterations at one step after which every QP sub-problem is polished (bqp_lbmpc_solve_batched)
constexpr int LB_POLISH_STALL = 6;

// the NW model's bandwidth and regularisation, oracleL2NW.m's defaults where unset (<= 0)
static double nw_bandwidth(double v) { return v > 0 ? v : 0.5; }
static double nw_lambda(double v) { return v > 0 ? v : 1e-3; }

// polish mode of a QP sub-problem (dense kernel) under the SQP's polish option: after 0 / -8 exits
// (modes 0-2; mode 3: not before the stall), and on every sub-problem (mode 2) once the SQP has
// stalled, i.e. has run LB_POLISH_STALL iterations at a step
static int sub_polish(int polish, bool stalled) {
    return polish < 0 ? 0 : (stalled ? 2 : (polish == 3 ? 0 : 1));
}

int bqp_nw_oracle_device(bqp_handle h, int batch, int q, const double* data, int64_t sdata,
                         const double* xi, double* g, double* dg, double bandwidth,
                         double lambda, void* stream) {
    if (!h || batch <= 0 || q <= 0 || !data || !xi || !g) return BQP_E_ARG;
    if (q > 512) return BQP_E_UNSUPPORTED;
    DevScope ds(h->device);
    HIP_TRY(bqp::launch_nw_oracle(batch, q, data, sdata, xi, g, dg, nw_bandwidth(bandwidth), nw_lambda(lambda),
                                  (hipStream_t)stream));
    return BQP_OK;
}

int bqp_nw_oracle(bqp_handle h, int batch, int q, const double* data, int64_t sdata,
                  const double* xi, double* g, double* dg, double bandwidth, double lambda) {
    if (!h || batch <= 0 || q <= 0 || !data || !xi || !g) return BQP_E_ARG;
    if (q > 512) return BQP_E_UNSUPPORTED;
    DevScope ds(h->device);
    const size_t B = batch;
    Stage st(h);
    const double *dd, *dx;
    double *dgv, *ddg;
    st.in(&dd, data, span(batch, sdata, (size_t)7 * q));
    st.in(&dx, xi, 3 * B);
    st.out(&dgv, 4 * B, g);
    st.out(&ddg, 12 * B, dg);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_nw_oracle_device(h, batch, q, dd, sdata, dx, dgv, ddg, bandwidth, lambda, h->stream));
    return st.finish();
}

static int lbmpc_check(const bqp_lbmpc_dims* d, int batch, const bqp_lbmpc_data* D) {
    if (!d || !D || batch <= 0) return BQP_E_ARG;
    if (d->N <= 0 || d->n_run < 0 || d->n_run > d->N || d->q <= 0 || d->m < 0 ||
        (d->mask != 0 && d->mask != 1) || (d->hessian != 0 && d->hessian != 1))
        return BQP_E_ARG;
    if (!D->A || !D->B || !D->K || !D->Lq || !D->Lr || !D->Lp || !D->Lt || !D->LAMBDA ||
        !D->PSI || !D->xs || !D->data || !D->x0 || (d->m > 0 && (!D->Ain || !D->bin)))
        return BQP_E_ARG;
    const int n = d->N * d->nu + d->np;
    if (!bqp::lbmpc_supported(d->nx, d->nu, d->np, n, d->q) || d->m > 8192) return BQP_E_UNSUPPORTED;
    return BQP_OK;
}

// the learned-model SQP's kernel arguments and per-instance state (done, iteration counts, flags
// zeroed), and the QP sub-problem's dense-kernel arguments: shared by the batched solve and the
// asynchronous closed loop
static hipError_t lbmpc_setup(bqp_handle h, const bqp_lbmpc_dims* d, int batch, const bqp_lbmpc_data* D,
                              const bqp_options& o, double* z, double* lam, int* exitflag, int* iterations,
                              hipStream_t st, bqp::LbmpcArgs& a, bqp::DenseKernelArgs& q) {
    const int N = d->N, n = N * d->nu + d->np, m = d->m;
    const int nr = d->n_run * (d->nx + d->nu) + 2 * d->nx;
    const size_t B = batch;
    const layout::Lwork LL(batch, N, n, nr, m, LB_NTRIAL, d->hessian != 0);
    hipError_t e = h->lwork.reserve(LL.bytes);
    if (e != hipSuccess) return e;
    void* lw = h->lwork.p;
    memset(&a, 0, sizeof(a));
    a.Jr = layout::at<double>(lw, LL.Jr);
    a.er = layout::at<double>(lw, LL.er);
    a.H = layout::at<double>(lw, LL.H);
    a.f = layout::at<double>(lw, LL.f);
    a.bsh = layout::at<double>(lw, LL.bsh);
    a.d = layout::at<double>(lw, LL.d);
    a.cost0 = layout::at<double>(lw, LL.cost0);
    a.costT = layout::at<double>(lw, LL.costT);
    a.stat = layout::at<double>(lw, LL.stat);
    a.cprev = layout::at<double>(lw, LL.cprev);
    a.Jr2 = layout::at<double>(lw, LL.Jr2);
    a.Tr2 = layout::at<double>(lw, LL.Tr2);
    a.qpflag = layout::at<int>(lw, LL.qpflag);
    a.hused = layout::at<int>(lw, LL.hused);
    a.done = layout::at<int>(lw, LL.done);
    a.ndone = layout::at<int>(lw, LL.ndone);
    // exact Hessian where its LDS fits (n <= 127), Gauss-Newton otherwise (include/bqp.h)
    a.hess = d->hessian && bqp::lbmpc_hess_fits(n);
    a.lam = lam ? lam : layout::at<double>(lw, LL.lam);
    a.z = z; a.flag = exitflag; a.iters = iterations;
    a.N = N; a.n = n; a.nr = nr; a.m = m; a.q = d->q; a.n_run = d->n_run;
    a.term_learned = d->term_learned; a.batch = batch; a.ntrial = LB_NTRIAL;
    a.wrows = d->mask ? 8 : 7;
    a.max_iter = o.max_iter;
    const double bw = nw_bandwidth(D->bandwidth);
    a.hinv2 = 1.0 / (bw * bw);
    a.lam_nw = nw_lambda(D->lambda);
    a.tol_step = o.tol_stat;            // |d| <= tol_stat (1 + |z|)
    a.tol_stat = 10.0 * o.tol_stat;     // |grad J + Ain' lam| <= 10 tol_stat (1 + |grad J|)
    a.A = D->A; a.B = D->B; a.K = D->K; a.Lq = D->Lq; a.Lr = D->Lr; a.Lp = D->Lp; a.Lt = D->Lt;
    a.LAM = D->LAMBDA; a.PSI = D->PSI; a.xs = D->xs;
    a.data = D->data; a.sdata = D->sdata; a.x0 = D->x0; a.sx0 = D->sx0;
    a.Ain = D->Ain; a.bin = D->bin; a.sbin = D->sbin;
    if ((e = hipMemsetAsync(a.done, 0, sizeof(int) * (B + 1), st)) != hipSuccess) return e;   // done[], ndone
    if ((e = hipMemsetAsync(a.hused, 0, sizeof(int) * B, st)) != hipSuccess) return e;
    // (null in bqp_lbmpc_linearize, which launches no kernel that reads them)
    if (a.iters && (e = hipMemsetAsync(a.iters, 0, sizeof(int) * B, st)) != hipSuccess) return e;
    if (a.flag && (e = hipMemsetAsync(a.flag, 0, sizeof(int) * B, st)) != hipSuccess) return e;
    // QP sub-problem (dense kernel): min 0.5 d'Hd + f'd  s.t.  Ain d <= bin - Ain z
    const int64_t wst = bqp::dense_work_doubles(n, m, 0);
    const layout::Dwork DL(wst, batch, bqp::STATS_W);
    if ((e = h->dwork.reserve(DL.bytes)) != hipSuccess) return e;
    bqp_options qo;
    bqp_default_options(&qo);
    qo.max_iter = 100;
    memset(&q, 0, sizeof(q));
    q.n = n; q.m = m; q.me = 0; q.batch = batch; q.max_iter = qo.max_iter;
    q.tol_stat = qo.tol_stat; q.tol_feas = qo.tol_feas; q.tol_comp = qo.tol_comp; q.tau = qo.tau;
    q.H = a.H; q.f = a.f; q.A = D->Ain; q.b = a.bsh;
    q.sH = (int64_t)n * n; q.sf = n; q.sA = 0; q.sb = m;
    q.x = a.d; q.lam_ineqlin = a.lam; q.exitflag = a.qpflag;
    q.work = layout::at<double>(h->dwork.p, DL.scratch); q.work_stride = wst;
    // The caller sets the sub-problem's polish mode (sub_polish).  Why every sub-problem is polished
    // once the SQP stalls: the Gauss-Newton iteration converges linearly on the learned costs of
    // DMS_LBMPC_casadi.m, and interior-point steps accurate to ~1e-8 left it wandering at that
    // level (tools/diag_dms_gpu.py); with the exact Hessian the SQP ends in 1-4 iterations.  Why
    // mode 3 (the closed loop's default) leaves -8 exits unpolished before the stall: in the
    // learned loop ~10 % of the sub-problems end -8 once mu ~ 1e-15 (the factor leaves fp64 range
    // one step past an accurate iterate, which the update kernel takes as is), and the polish
    // launch for them was ~1/3 of each SQP iteration (5.5 of 16 ms, BQP_LB_TRACE=2).  A single
    // solve keeps mode 1: its weakly determined tail inputs move ~1e-6 without the polish.
    // instances whose SQP has finished are not solved again (the update kernel skips them too)
    q.skip = a.done;
    q.stats = layout::at<double>(h->dwork.p, DL.stats);
    return hipSuccess;
}

// BQP_LB_TRACE diagnostics of the batched solve's SQP iterations, on stderr: the sub-problems'
// exit flags per iteration, from 2 on per-launch event times instead.  Both wait for the stream
// at each iteration; neither launches a kernel.
struct SqpTrace {
    const char* env = getenv("BQP_LB_TRACE");
    const int level = !env ? 0 : (atoi(env) >= 2 ? 2 : 1);   // 0: unset
    int it = 0;                                              // the SQP iteration being traced
    EventGuard ev[6];
    // point k of sqp_iteration: 0 its start, then after rollout, normal (+ hess), dense, trials, update
    int mark(int k, const bqp::LbmpcArgs& a, hipStream_t st) {
        if (level == 2) {
            if (!ev[k].e) HIP_TRY(hipEventCreate(&ev[k].e));
            HIP_TRY(hipEventRecord(ev[k].e, st));
            if (k < 5) return BQP_OK;
            HIP_TRY(hipEventSynchronize(ev[5].e));
            float ms[5];
            for (int j = 0; j < 5; ++j) HIP_TRY(hipEventElapsedTime(&ms[j], ev[j].e, ev[j + 1].e));
            fprintf(stderr, "bqp sqp it %d ms: rollout+sens %.3f normal+hess %.3f dense(+polish) %.3f trials %.3f update %.3f\n",
                    it, ms[0], ms[1], ms[2], ms[3], ms[4]);
        } else if (k == 3) {
            std::vector<int> fl(a.batch), dn(a.batch);
            HIP_TRY(hipMemcpyAsync(fl.data(), a.qpflag, sizeof(int) * a.batch, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(dn.data(), a.done, sizeof(int) * a.batch, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            int c1 = 0, c0 = 0, c8 = 0, co = 0, act = 0;
            for (int b = 0; b < a.batch; ++b) {
                if (dn[b]) continue;
                ++act;
                if (fl[b] == 1) ++c1; else if (fl[b] == 0) ++c0; else if (fl[b] == -8) ++c8; else ++co;
            }
            fprintf(stderr, "bqp sqp it %d: active %d, sub-problem flags 1:%d 0:%d -8:%d other:%d\n", it, act, c1, c0, c8, co);
        }
        return BQP_OK;
    }
};

// One SQP iteration of every unfinished instance: rollout with sensitivities, normal equations
// (+ the exact Hessian), the QP sub-problems, the trial rollouts, the update.  tr: diagnostics of
// the batched solve, null on the plain path.
static int sqp_iteration(const bqp::LbmpcArgs& a, const bqp::DenseKernelArgs& q, hipStream_t st,
                         SqpTrace* tr = nullptr) {
    if (tr) BQP_TRY(tr->mark(0, a, st));
    HIP_TRY(bqp::launch_lbmpc_rollout(a, 1, st));
    if (tr) BQP_TRY(tr->mark(1, a, st));
    HIP_TRY(bqp::launch_lbmpc_normal(a, st));
    if (a.hess) HIP_TRY(bqp::launch_lbmpc_hess(a, st));
    if (tr) BQP_TRY(tr->mark(2, a, st));
    HIP_TRY(bqp::launch_dense(q, st));
    if (tr) BQP_TRY(tr->mark(3, a, st));
    HIP_TRY(bqp::launch_lbmpc_rollout(a, 0, st));
    if (tr) BQP_TRY(tr->mark(4, a, st));
    HIP_TRY(bqp::launch_lbmpc_update(a, st));
    if (tr) BQP_TRY(tr->mark(5, a, st));
    return BQP_OK;
}
static int sqp_iteration_launches(const bqp::LbmpcArgs& a) { return a.hess ? 6 : 5; }

int bqp_lbmpc_solve_batched_device(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                                   const bqp_lbmpc_data* D, const bqp_options* opt, double* z,
                                   double* lam, double* cost, int* exitflag, int* iterations,
                                   void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(lbmpc_check(d, batch, D));
    if (!z || !exitflag || !iterations) return BQP_E_ARG;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(opt, &o);
    const int N = d->N, n = N * d->nu + d->np;
    const size_t B = batch;
    bqp::LbmpcArgs a;
    bqp::DenseKernelArgs q;
    HIP_TRY(lbmpc_setup(h, d, batch, D, o, z, lam, exitflag, iterations, st, a, q));
    HIP_TRY(hipEventRecord(h->ev0, st));
    int launches = 0;
    SqpTrace trace;
    for (int it = 0; it < o.max_iter; ++it) {
        trace.it = it;
        q.polish = sub_polish(o.polish, it >= LB_POLISH_STALL);
        BQP_TRY(sqp_iteration(a, q, st, trace.level ? &trace : nullptr));
        launches += sqp_iteration_launches(a);
        // the batch is done when every instance is: polled after each iteration for large
        // sub-problems (an SQP iteration is ~20 ms of kernels at the learned loop's N = 100 shape,
        // and polling every 4th ran up to three iterations past the last instance's convergence),
        // every 4th for small ones (the host round trip against ~0.3 ms iterations at N = 10)
        if ((it + 1) % (n >= 64 ? 1 : 4) == 0 || it + 1 == o.max_iter) {
            int nd_h = 0;
            HIP_TRY(hipMemcpyAsync(&nd_h, a.ndone, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (nd_h >= batch) break;
        }
    }
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->timed = true;
    h->launches = launches;
    if (cost) HIP_TRY(hipMemcpyAsync(cost, a.cost0, sizeof(double) * B, hipMemcpyDeviceToDevice, st));
    return BQP_OK;
}

// registers the shared model, gain and weight matrices of D with the stage; once st.commit() has
// run, *Dd is D with their device copies (data, x0, Ain and bin are the caller's to set)
static void stage_lbmpc_model(Stage& st, const bqp_lbmpc_dims* d, const bqp_lbmpc_data* D, bqp_lbmpc_data* Dd) {
    const size_t nx = d->nx, nu = d->nu, np = d->np;
    *Dd = *D;
    st.in(&Dd->A, D->A, nx * nx);            st.in(&Dd->B, D->B, nx * nu);
    st.in(&Dd->K, D->K, nu * nx);            st.in(&Dd->Lq, D->Lq, nx * nx);
    st.in(&Dd->Lr, D->Lr, nu * nu);          st.in(&Dd->Lp, D->Lp, nx * nx);
    st.in(&Dd->Lt, D->Lt, nx * nx);          st.in(&Dd->LAMBDA, D->LAMBDA, nx * np);
    st.in(&Dd->PSI, D->PSI, nu * np);        st.in(&Dd->xs, D->xs, nx);
}

int bqp_lbmpc_solve_batched(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                            const bqp_lbmpc_data* D, const bqp_options* opt, double* z,
                            double* lam, double* cost, int* exitflag, int* iterations) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(lbmpc_check(d, batch, D));
    if (!z || !exitflag || !iterations) return BQP_E_ARG;
    DevScope ds(h->device);
    const size_t B = batch, nx = d->nx, m = d->m, n = (size_t)d->N * d->nu + d->np;
    Stage st(h);
    bqp_lbmpc_data Dd;
    double *zd, *ld, *cd;
    int *ed, *itd;
    stage_lbmpc_model(st, d, D, &Dd);
    st.in(&Dd.data, D->data, span(batch, D->sdata, (size_t)(d->mask ? 8 : 7) * d->q));
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, nx));
    st.in(&Dd.Ain, D->Ain, m * n);
    st.in(&Dd.bin, D->bin, span(batch, D->sbin, m));
    st.in(&zd, z, B * n, z);   // the initial iterate, and the solution
    st.out(&ld, B * m, lam);
    st.out(&cd, B, cost);
    st.out(&ed, B, exitflag);
    st.out(&itd, B, iterations);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_lbmpc_solve_batched_device(h, d, batch, &Dd, opt, zd, ld, cd, ed, itd, h->stream));
    return st.finish();
}

// the model's exact Hessian is formed: asked for and its LDS fits (lbmpc_setup's a.hess)
static bool lbmpc_exact(const bqp_lbmpc_dims* d) {
    return d->hessian && bqp::lbmpc_hess_fits(d->N * d->nu + d->np);
}

int bqp_lbmpc_linearize_device(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                               const bqp_lbmpc_data* D, const double* z, const double* dstep,
                               double* cost, double* Jr, double* er, double* H, double* f,
                               double* rhs, int* hused, double* Jr2, double* Tr2, double* costT,
                               void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(lbmpc_check(d, batch, D));
    if (!z) return BQP_E_ARG;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(nullptr, &o);
    const size_t B = batch, n = (size_t)d->N * d->nu + d->np, m = d->m;
    bqp::LbmpcArgs a;
    bqp::DenseKernelArgs q;
    HIP_TRY(lbmpc_setup(h, d, batch, D, o, const_cast<double*>(z), nullptr, nullptr, nullptr, st, a, q));
    const size_t nr = a.nr, n2 = (size_t)3 * d->N * n;
    // one SQP iteration's model launches at the caller's z (read only: no update kernel)
    HIP_TRY(bqp::launch_lbmpc_rollout(a, 1, st));
    HIP_TRY(bqp::launch_lbmpc_normal(a, st));
    if (a.hess) HIP_TRY(bqp::launch_lbmpc_hess(a, st));
    if (dstep) {
        HIP_TRY(hipMemcpyAsync(a.d, dstep, sizeof(double) * B * n, hipMemcpyDeviceToDevice, st));
        HIP_TRY(bqp::launch_lbmpc_rollout(a, 0, st));
    }
    auto copy = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) : hipSuccess;
    };
    HIP_TRY(copy(cost, a.cost0, sizeof(double) * B));
    HIP_TRY(copy(Jr, a.Jr, sizeof(double) * B * nr * n));
    HIP_TRY(copy(er, a.er, sizeof(double) * B * nr));
    HIP_TRY(copy(H, a.H, sizeof(double) * B * n * n));
    HIP_TRY(copy(f, a.f, sizeof(double) * B * n));
    HIP_TRY(copy(rhs, a.bsh, sizeof(double) * B * m));
    HIP_TRY(copy(hused, a.hused, sizeof(int) * B));
    if (a.hess) {
        HIP_TRY(copy(Jr2, a.Jr2, sizeof(double) * B * n2));
        HIP_TRY(copy(Tr2, a.Tr2, sizeof(double) * B * n2));
    }
    if (dstep) HIP_TRY(copy(costT, a.costT, sizeof(double) * B * LB_NTRIAL));
    return BQP_OK;
}

int bqp_lbmpc_linearize(bqp_handle h, const bqp_lbmpc_dims* d, int batch, const bqp_lbmpc_data* D,
                        const double* z, const double* dstep, double* cost, double* Jr, double* er,
                        double* H, double* f, double* rhs, int* hused, double* Jr2, double* Tr2,
                        double* costT) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(lbmpc_check(d, batch, D));
    if (!z) return BQP_E_ARG;
    DevScope ds(h->device);
    const size_t B = batch, nx = d->nx, m = d->m, n = (size_t)d->N * d->nu + d->np;
    const size_t nr = (size_t)d->n_run * (d->nx + d->nu) + 2 * nx, n2 = (size_t)3 * d->N * n;
    const bool exact = lbmpc_exact(d);
    Stage st(h);
    bqp_lbmpc_data Dd;
    const double *zd, *dd;
    double *cd = nullptr, *Jd = nullptr, *ed = nullptr, *Hd = nullptr, *fd = nullptr, *rd = nullptr,
           *J2d = nullptr, *T2d = nullptr, *cTd = nullptr;
    int* hud = nullptr;
    stage_lbmpc_model(st, d, D, &Dd);
    st.in(&Dd.data, D->data, span(batch, D->sdata, (size_t)(d->mask ? 8 : 7) * d->q));
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, nx));
    st.in(&Dd.Ain, D->Ain, m * n);
    st.in(&Dd.bin, D->bin, span(batch, D->sbin, m));
    st.in(&zd, z, B * n);
    st.in(&dd, dstep, B * n);
    // only what the call writes is staged: an output it leaves alone stays the caller's
    if (cost) st.out(&cd, B, cost);
    if (Jr) st.out(&Jd, B * nr * n, Jr);
    if (er) st.out(&ed, B * nr, er);
    if (H) st.out(&Hd, B * n * n, H);
    if (f) st.out(&fd, B * n, f);
    if (rhs && m) st.out(&rd, B * m, rhs);
    if (hused) st.out(&hud, B, hused);
    if (Jr2 && exact) st.out(&J2d, B * n2, Jr2);
    if (Tr2 && exact) st.out(&T2d, B * n2, Tr2);
    if (costT && dstep) st.out(&cTd, B * LB_NTRIAL, costT);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_lbmpc_linearize_device(h, d, batch, &Dd, zd, dd, cd, Jd, ed, Hd, fd, rd, hud, J2d, T2d,
                                       cTd, h->stream));
    return st.finish();
}

// ------------------------------------------------------------------------------------------
// closed-loop simulation: batched structured solve + true-plant step, per time step
// ------------------------------------------------------------------------------------------
// the loop description of the closed-loop entry points (cl non-null): plant, steps, sampling time
// and working point; the plants are the Moore-Greitzer model's
// bqp_closed_loop.plant_par (per-instance Moore-Greitzer coefficients, bqp_plant_par.h).  Every
// entry: none with the linear plant, the schedule flag 0 or 1, a stride of 0 or at least one
// instance's block.  A null plant_par leaves the other two members unread.
static int plant_par_check(const bqp_closed_loop* cl) {
    if (!cl->plant_par) return BQP_OK;
    if (cl->plant == BQP_PLANT_LINEAR) return BQP_E_ARG;
    if (cl->plant_par_sched != 0 && cl->plant_par_sched != 1) return BQP_E_ARG;
    return bqp::plant_par_stride_ok(cl->splant_par, cl->steps, cl->plant_par_sched) ? BQP_OK : BQP_E_ARG;
}

// host entries, after plant_par_check: every row finite with 1/beta^2 > 0, wn^2 > 0, 2 zeta wn >= 0
// (the device entries leave the values to the caller)
static int plant_par_host_check(const bqp_closed_loop* cl, int batch) {
    if (!cl->plant_par) return BQP_OK;
    const int rows = cl->plant_par_sched ? cl->steps : 1;
    for (int b = 0; b < (cl->splant_par == 0 ? 1 : batch); ++b)
        for (int t = 0; t < rows; ++t)
            if (!bqp::plant_par_row_ok(cl->plant_par + bqp::plant_par_at(cl->splant_par, cl->plant_par_sched, b, t)))
                return BQP_E_ARG;
    return BQP_OK;
}

// the host entries' copy of the coefficients to the device, into the loop description's copy
static void stage_plant_par(Stage& st, const bqp_closed_loop* cl, int batch, bqp_closed_loop* cd) {
    st.in(&cd->plant_par, cl->plant_par,
          cl->plant_par ? (size_t)bqp::plant_par_span(batch, cl->splant_par, cl->steps, cl->plant_par_sched) : 0);
}

// what the plant and advance launchers take: null for the nominal plant (the kernels as they were)
struct LoopPlantPar {
    bqp::PlantPar pp;
    explicit LoopPlantPar(const bqp_closed_loop* cl) : pp{cl->plant_par, cl->splant_par, cl->plant_par_sched} {}
    const bqp::PlantPar* get() const { return pp.p ? &pp : nullptr; }
};

static int loop_check(const bqp_closed_loop* cl, int nx, int nu) {
    if ((cl->plant != BQP_PLANT_MG_RK4 && cl->plant != BQP_PLANT_MG_ODE23) || cl->steps <= 0 ||
        !(cl->delta > 0) || !cl->x_eq || !cl->u_eq)
        return BQP_E_ARG;
    if (nx != 4 || nu != 1) return BQP_E_UNSUPPORTED;
    return plant_par_check(cl);
}

static int closed_loop_impl(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                            const bqp_options* opt, const bqp_closed_loop* cl,
                            const bqp_learning* lw, const double* x_init, double* X, double* U,
                            int* exitflag, void* stream) {
    if (!h || !cl || !x_init || !X || !U) return BQP_E_ARG;
    BQP_TRY(ocp_check(d, batch, D));
    if (d->stage_models) return BQP_E_UNSUPPORTED;   // per-stage models: the plain solves only
    if (lw && ocp_soft(D)) return BQP_E_UNSUPPORTED;  // soft state bounds: not in the learned-model loop
    BQP_TRY(loop_check(cl, d->nx, d->nu));
    if (lw && (lw->q < 1 || lw->q > (1 << 20) || !lw->XL)) return BQP_E_ARG;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int nx = d->nx, nu = d->nu, np = d->np, N = d->N;
    const layout::CworkOcp CL(batch, nx, nu, np, N, lw ? lw->q : 0);
    HIP_TRY(h->cwork.reserve(CL.bytes));
    double* s = layout::at<double>(h->cwork.p, CL.s);
    double* xo = layout::at<double>(h->cwork.p, CL.x);
    double* uo = layout::at<double>(h->cwork.p, CL.u);
    double* th = layout::at<double>(h->cwork.p, CL.theta);
    double* win = layout::at<double>(h->cwork.p, CL.window);
    int* fl = layout::at<int>(h->cwork.p, CL.flags);
    if (lw && lw->window) win = lw->window;   // the caller's buffer (device) keeps the final window
    HIP_TRY(bqp::launch_closed_loop_init(batch, nx, cl->steps, x_init, cl->x_eq, s, X, st));
    const double bw = nw_bandwidth(lw ? lw->bandwidth : 0), lam = nw_lambda(lw ? lw->lambda : 0);
    if (lw) HIP_TRY(bqp::launch_lbmpc_window_init(batch, cl->steps, lw->q, lw->mask, x_init, win, lw->XL, st));
    bqp_ocp_data Dm = *D;
    Dm.x0 = s;
    Dm.sx0 = nx;
    EventGuard e0;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventRecord(e0.e, st));
    int launches = 0;
    const LoopPlantPar par(cl);
    for (int t = 0; t < cl->steps; ++t) {
        BQP_TRY(bqp_solve_ocp_batched_device(h, d, batch, &Dm, opt, xo, uo, th, nullptr, fl, nullptr,
                                             nullptr, stream));
        launches += h->launches + (lw ? 2 : 1);
        HIP_TRY(bqp::launch_mg_plant(cl->plant, batch, N, cl->steps, t, cl->delta, uo, fl, cl->x_eq, cl->u_eq,
                                     s, X, U, exitflag, st, par.get()));
        if (lw)
            HIP_TRY(bqp::launch_lbmpc_window(batch, cl->steps, t, lw->q, bw, lam, D->A, D->sA, D->B,
                                             D->sB, cl->x_eq, cl->u_eq, X, U, win, lw->XL, st));
    }
    // timing of the whole loop (solves + plant steps) on this stream
    HIP_TRY(hipEventRecord(h->ev1, st));
    HIP_TRY(hipEventSynchronize(h->ev1));
    std::swap(h->ev0, e0.e);   // the guard destroys the previous start event
    h->timed = true;
    h->launches = launches;
    return BQP_OK;
}

int bqp_closed_loop_ocp_device(bqp_handle h, const bqp_ocp_dims* d, int batch,
                               const bqp_ocp_data* D, const bqp_options* opt,
                               const bqp_closed_loop* cl, const double* x_init, double* X,
                               double* U, int* exitflag, void* stream) {
    return closed_loop_impl(h, d, batch, D, opt, cl, nullptr, x_init, X, U, exitflag, stream);
}

int bqp_closed_loop_lbmpc_device(bqp_handle h, const bqp_ocp_dims* d, int batch,
                                 const bqp_ocp_data* D, const bqp_options* opt,
                                 const bqp_closed_loop* cl, const bqp_learning* lw,
                                 const double* x_init, double* X, double* U, int* exitflag,
                                 void* stream) {
    if (!lw) return BQP_E_ARG;
    return closed_loop_impl(h, d, batch, D, opt, cl, lw, x_init, X, U, exitflag, stream);
}

static int closed_loop_host(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                            const bqp_options* opt, const bqp_closed_loop* cl,
                            const bqp_learning* lw, const double* x_init, double* X, double* U,
                            int* exitflag) {
    if (!h || !cl || !x_init || !X || !U) return BQP_E_ARG;
    if (lw && (lw->q < 1 || lw->q > (1 << 20) || !lw->XL)) return BQP_E_ARG;
    BQP_TRY(ocp_check(d, batch, D));
    if (d->stage_models) return BQP_E_UNSUPPORTED;   // per-stage models: the plain solves only
    if (lw && ocp_soft(D)) return BQP_E_UNSUPPORTED;  // soft state bounds: not in the learned-model loop
    BQP_TRY(ocp_soft_host_check(d, batch, D));
    // validate the loop description before sizing the staging buffers from it
    BQP_TRY(loop_check(cl, d->nx, d->nu));
    BQP_TRY(plant_par_host_check(cl, batch));
    DevScope ds(h->device);
    const size_t B = batch, S = cl->steps, nx = d->nx, nu = d->nu;
    const size_t nX = B * (S + 1) * nx;
    Stage st(h);
    bqp_ocp_data Dd;
    bqp_closed_loop cd = *cl;
    bqp_learning ld = lw ? *lw : bqp_learning{};
    double *Xd, *Ud;
    int* Fd;
    // Dd.x0: the initial states (a placeholder: the loop feeds the measured states)
    stage_ocp_data(st, d, batch, D, x_init, B * nx, &Dd);
    st.in(&cd.x_eq, cl->x_eq, nx);
    st.in(&cd.u_eq, cl->u_eq, nu);
    stage_plant_par(st, cl, batch, &cd);
    st.out(&Xd, nX, X);
    st.out(&Ud, B * S * nu, U);
    if (lw) {
        st.out(&ld.XL, nX, lw->XL);
        st.out(&ld.window, B * lw->q * 8, lw->window);
    }
    st.out(&Fd, B * S, exitflag);
    BQP_TRY(st.commit());
    BQP_TRY(closed_loop_impl(h, d, batch, &Dd, opt, &cd, lw ? &ld : nullptr, Dd.x0, Xd, Ud,
                             exitflag ? Fd : nullptr, h->stream));
    return st.finish();
}

int bqp_closed_loop_ocp(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                        const bqp_options* opt, const bqp_closed_loop* cl, const double* x_init,
                        double* X, double* U, int* exitflag) {
    return closed_loop_host(h, d, batch, D, opt, cl, nullptr, x_init, X, U, exitflag);
}

int bqp_closed_loop_lbmpc(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                          const bqp_options* opt, const bqp_closed_loop* cl,
                          const bqp_learning* lw, const double* x_init, double* X, double* U,
                          int* exitflag) {
    if (!lw) return BQP_E_ARG;
    return closed_loop_host(h, d, batch, D, opt, cl, lw, x_init, X, U, exitflag);
}

// ------------------------------------------------------------------------------------------
// closed loop with a reference schedule and a linear plant: batched structured solve at
// w_t = w + Wr r_t, then one advance launch (record, plant step, w_{t+1}), per time step
// ------------------------------------------------------------------------------------------
// everything the two entry points take, checked before any buffer is sized from it.  data->x0 is
// not read by the loop: the check of the problem runs with the initial states in its place
static int track_check(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                       const bqp_closed_loop* cl, const bqp_track* tr, const double* x_init,
                       const double* X, const double* U) {
    if (!h || !D || !cl || !tr || !x_init || !X || !U) return BQP_E_ARG;
    bqp_ocp_data Dc = *D;
    Dc.x0 = x_init;
    BQP_TRY(ocp_check(d, batch, &Dc));
    if (d->stage_models) return BQP_E_UNSUPPORTED;   // per-stage models: the plain solves only
    if (cl->steps <= 0 || !cl->x_eq || !cl->u_eq) return BQP_E_ARG;
    if (cl->plant == BQP_PLANT_LINEAR) {
        if (tr->sAp < 0 || tr->sBp < 0 || tr->sdist < 0) return BQP_E_ARG;
    } else if (cl->plant == BQP_PLANT_MG_RK4 || cl->plant == BQP_PLANT_MG_ODE23) {
        if (tr->Ap || tr->Bp || tr->dist || !(cl->delta > 0)) return BQP_E_ARG;
        if (d->nx != 4 || d->nu != 1) return BQP_E_UNSUPPORTED;
    } else {
        return BQP_E_ARG;
    }
    BQP_TRY(plant_par_check(cl));
    if (tr->nr < 0 || tr->sref < 0) return BQP_E_ARG;
    if (tr->nr > 0 && (!tr->Wr || !tr->ref)) return BQP_E_ARG;
    if (D->w && D->sw < 0) return BQP_E_ARG;
    return BQP_OK;
}

static int track_impl(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                      const bqp_options* opt, const bqp_closed_loop* cl, const bqp_track* tr,
                      const double* x_init, double* X, double* U, int* exitflag, void* stream) {
    BQP_TRY(track_check(h, d, batch, D, cl, tr, x_init, X, U));
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int nx = d->nx, nu = d->nu, np = d->np, N = d->N;
    const size_t nw = (size_t)(N + 1) * (nx + nu + np);
    const bool sched = tr->nr > 0;
    const layout::CworkTrack CL(batch, nx, nu, np, N, sched ? nw : 0);
    HIP_TRY(h->cwork.reserve(CL.bytes));
    bqp::TrackArgs a;
    memset(&a, 0, sizeof(a));
    a.batch = batch; a.nx = nx; a.nu = nu; a.np = np; a.N = N; a.steps = cl->steps; a.nr = tr->nr;
    a.plant = cl->plant; a.delta = cl->delta; a.nw = (int64_t)nw;
    a.s = layout::at<double>(h->cwork.p, CL.s);
    double* xo = layout::at<double>(h->cwork.p, CL.x);
    double* uo = layout::at<double>(h->cwork.p, CL.u);
    double* th = layout::at<double>(h->cwork.p, CL.theta);
    int* fl = layout::at<int>(h->cwork.p, CL.flags);
    a.uo = uo; a.th = th; a.fl = fl;
    a.w = layout::at<double>(h->cwork.p, CL.w);
    a.xeq = cl->x_eq; a.ueq = cl->u_eq;
    a.A = tr->Ap ? tr->Ap : D->A; a.sA = tr->Ap ? tr->sAp : D->sA;
    a.B = tr->Bp ? tr->Bp : D->B; a.sB = tr->Bp ? tr->sBp : D->sB;
    a.dist = tr->dist; a.sdist = tr->sdist;
    a.wbase = D->w; a.swbase = D->sw;
    a.Wr = tr->Wr; a.ref = tr->ref; a.sref = tr->sref;
    a.X = X; a.U = U; a.THETA = tr->THETA; a.flags = exitflag;
    HIP_TRY(bqp::launch_closed_loop_init(batch, nx, cl->steps, x_init, cl->x_eq, a.s, X, st));
    bqp_ocp_data Dm = *D;
    Dm.x0 = a.s;
    Dm.sx0 = nx;
    if (sched) {   // the solve reads the loop's own linear terms; the init launch forms w_0
        Dm.w = a.w;
        Dm.sw = (int64_t)nw;
        HIP_TRY(bqp::launch_track_advance(a, -1, st));
    }
    EventGuard e0;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventRecord(e0.e, st));
    int launches = 0;
    const LoopPlantPar par(cl);
    for (int t = 0; t < cl->steps; ++t) {
        BQP_TRY(bqp_solve_ocp_batched_device(h, d, batch, &Dm, opt, xo, uo, th, nullptr, fl, nullptr,
                                             nullptr, stream));
        launches += h->launches + 1;
        HIP_TRY(bqp::launch_track_advance(a, t, st, par.get()));
    }
    // timing of the whole loop (solves + advance launches) on this stream
    HIP_TRY(hipEventRecord(h->ev1, st));
    HIP_TRY(hipEventSynchronize(h->ev1));
    std::swap(h->ev0, e0.e);   // the guard destroys the previous start event
    h->timed = true;
    h->launches = launches;
    return BQP_OK;
}

int bqp_closed_loop_track_device(bqp_handle h, const bqp_ocp_dims* d, int batch,
                                 const bqp_ocp_data* D, const bqp_options* opt,
                                 const bqp_closed_loop* cl, const bqp_track* tr,
                                 const double* x_init, double* X, double* U, int* exitflag,
                                 void* stream) {
    return track_impl(h, d, batch, D, opt, cl, tr, x_init, X, U, exitflag, stream);
}

int bqp_closed_loop_track(bqp_handle h, const bqp_ocp_dims* d, int batch, const bqp_ocp_data* D,
                          const bqp_options* opt, const bqp_closed_loop* cl, const bqp_track* tr,
                          const double* x_init, double* X, double* U, int* exitflag) {
    // validate the whole description before sizing the staging buffers from it
    BQP_TRY(track_check(h, d, batch, D, cl, tr, x_init, X, U));
    BQP_TRY(ocp_soft_host_check(d, batch, D));
    BQP_TRY(plant_par_host_check(cl, batch));
    DevScope ds(h->device);
    const size_t B = batch, S = cl->steps, nx = d->nx, nu = d->nu, np = d->np;
    const size_t nw = (size_t)(d->N + 1) * (nx + nu + np), nr = tr->nr;
    const bool linear = cl->plant == BQP_PLANT_LINEAR;
    Stage st(h);
    bqp_ocp_data Dd;
    bqp_closed_loop cd = *cl;
    bqp_track td = *tr;
    double *Xd, *Ud;
    int* Fd;
    // Dd.x0: the initial states (a placeholder: the loop feeds the measured states)
    stage_ocp_data(st, d, batch, D, x_init, B * nx, &Dd);
    st.in(&cd.x_eq, cl->x_eq, nx);
    st.in(&cd.u_eq, cl->u_eq, nu);
    stage_plant_par(st, cl, batch, &cd);
    st.in(&td.Ap, linear ? tr->Ap : nullptr, span(batch, tr->sAp, nx * nx));
    st.in(&td.Bp, linear ? tr->Bp : nullptr, span(batch, tr->sBp, nx * nu));
    st.in(&td.dist, linear ? tr->dist : nullptr, span(batch, tr->sdist, S * nx));
    st.in(&td.Wr, tr->Wr, nw * nr);
    st.in(&td.ref, tr->ref, span(batch, tr->sref, S * nr));
    st.out(&Xd, B * (S + 1) * nx, X);
    st.out(&Ud, B * S * nu, U);
    td.THETA = nullptr;
    if (tr->THETA) st.out(&td.THETA, B * S * np, tr->THETA);
    st.out(&Fd, B * S, exitflag);
    BQP_TRY(st.commit());
    BQP_TRY(track_impl(h, d, batch, &Dd, opt, &cd, &td, Dd.x0, Xd, Ud, exitflag ? Fd : nullptr,
                       h->stream));
    return st.finish();
}

// ------------------------------------------------------------------------------------------
// learned-model NLP closed loop: batched SQP + true-plant step + data window, per time step
// ------------------------------------------------------------------------------------------
static int sqp_loop_check(const bqp_lbmpc_dims* d, int batch, const bqp_lbmpc_data* D,
                          const bqp_sqp_loop* sl, const bqp_closed_loop* cl,
                          const bqp_learning* lw, const double* x_init, const double* X,
                          const double* U) {
    if (!d || !D || !sl || !cl || !lw || !x_init || !X || !U || batch <= 0) return BQP_E_ARG;
    BQP_TRY(loop_check(cl, d->nx, d->nu));
    if (lw->q != d->q || !lw->XL || (lw->mask != 0 && lw->mask != 1)) return BQP_E_ARG;
    if (d->m > 0 && (!sl->bin0 || !sl->Bx)) return BQP_E_ARG;
    // the loop supplies the window, the measured state and the rhs: check the rest
    bqp_lbmpc_data Dc = *D;
    double dummy = 0.0;
    Dc.data = &dummy; Dc.x0 = &dummy; Dc.bin = &dummy;
    bqp_lbmpc_dims dc = *d;
    dc.mask = 1;
    return lbmpc_check(&dc, batch, &Dc);
}

int bqp_closed_loop_sqp_device(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                               const bqp_lbmpc_data* D, const bqp_sqp_loop* sl,
                               const bqp_options* opt, const bqp_closed_loop* cl,
                               const bqp_learning* lw, const double* x_init, double* X, double* U,
                               int* exitflag, void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(sqp_loop_check(d, batch, D, sl, cl, lw, x_init, X, U));
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int nx = d->nx, N = d->N, m = d->m, q = d->q;
    const int n = N * d->nu + d->np;
    const size_t B = batch;
    const layout::CworkSqp CL(batch, nx, n, m, q);
    HIP_TRY(h->cwork.reserve(CL.bytes));
    double* s = layout::at<double>(h->cwork.p, CL.s);         // measured deviation state
    double* z = layout::at<double>(h->cwork.p, CL.z);         // SQP iterate / solution
    double* bin = layout::at<double>(h->cwork.p, CL.bin);     // rhs of the step's constraints
    double* uo = layout::at<double>(h->cwork.p, CL.u0);       // first input (deviation)
    double* win = layout::at<double>(h->cwork.p, CL.window);  // window ring, 8 doubles per point
    int* fl = layout::at<int>(h->cwork.p, CL.flags);
    int* it = layout::at<int>(h->cwork.p, CL.iters);
    if (lw->window) win = lw->window;
    bqp_options ol;                       // the loop's default polish: only once the SQP stalls
    resolve(opt, &ol);
    if (ol.polish == 0) ol.polish = 3;
    opt = &ol;
    HIP_TRY(bqp::launch_closed_loop_init(batch, nx, cl->steps, x_init, cl->x_eq, s, X, st));
    HIP_TRY(bqp::launch_lbmpc_window_init(batch, cl->steps, q, lw->mask, x_init, win, lw->XL, st));
    HIP_TRY(hipMemsetAsync(z, 0, sizeof(double) * B * n, st));
    // the learned model's NW parameters: the loop's (bqp_learning) when set, else the model's own
    // (bqp_lbmpc_data), else the defaults
    const double bw = nw_bandwidth(lw->bandwidth > 0 ? lw->bandwidth : D->bandwidth);
    const double lam = nw_lambda(lw->lambda > 0 ? lw->lambda : D->lambda);
    bqp_lbmpc_dims dl = *d;
    dl.mask = 1;                          // the loop's window always carries the validity row
    bqp_lbmpc_data Dl = *D;
    Dl.data = win; Dl.sdata = (int64_t)q * 8;
    Dl.x0 = s; Dl.sx0 = nx;
    Dl.bin = bin; Dl.sbin = m;
    Dl.bandwidth = bw; Dl.lambda = lam;
    EventGuard e0;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventRecord(e0.e, st));
    int launches = 0;
    const LoopPlantPar par(cl);
    // BQP_LB_SYNC selects the step-synchronous loop below (the asynchronous loop's bitwise
    // reference in tests/test_gpu_lbmpc_dms.py); BQP_LB_TRACE only adds diagnostics to either
    const bool sync_loop = getenv("BQP_LB_SYNC") != nullptr;
    if (!sync_loop) {
        // asynchronous (round 5): every instance runs at its own closed-loop step.  Each round is
        // one SQP iteration of every unfinished instance, then sqp_loop_advance_kernel moves the
        // instances whose SQP has finished to their next step (u_0, plant, window, constraints,
        // warm start).  The step-synchronous form below ran every step's SQP launches until the
        // batch's slowest instance had converged (2.4 SQP iterations per step on average against
        // up to 6 at a step) while the converged ones idled; per instance the two forms do the
        // same operations in the same order (tests/test_gpu_lbmpc_dms.py compares them).
        int* ts = layout::at<int>(h->cwork.p, CL.ts);
        int* nfin = layout::at<int>(h->cwork.p, CL.nfin);
        HIP_TRY(hipMemsetAsync(ts, 0, sizeof(int) * (B + 1), st));   // ts[], nfin
        HIP_TRY(bqp::launch_sqp_loop_prep(batch, nx, n, m, N * d->nu, 0, s, sl->bin0, sl->Bx, bin, z, st));
        bqp::LbmpcArgs a;
        bqp::DenseKernelArgs qd;
        HIP_TRY(lbmpc_setup(h, &dl, batch, &Dl, *opt, z, nullptr, fl, it, st, a, qd));
        // sub-problem polish per instance: from its own SQP iteration count (lbmpc solve: mode 2
        // from LB_POLISH_STALL on, before it the loop's mode 3 - none - or 1)
        qd.polish = sub_polish(opt->polish, false);
        qd.pol_it = opt->polish < 0 ? nullptr : a.iters;
        qd.pol_stall = LB_POLISH_STALL;
        bqp::SqpAdvanceArgs v;
        memset(&v, 0, sizeof(v));
        v.batch = batch; v.nx = nx; v.nu = d->nu; v.n = n; v.m = m; v.nv = N * d->nu; v.warm = sl->warm;
        v.steps = cl->steps; v.q = q; v.plant = cl->plant; v.delta = cl->delta;
        v.hinv2 = 1.0 / (bw * bw); v.lam = lam;
        v.K = D->K; v.bin0 = sl->bin0; v.Bx = sl->Bx; v.xeq = cl->x_eq; v.ueq = cl->u_eq;
        v.A = D->A; v.Bm = D->B;
        v.s = s; v.z = z; v.bin = bin; v.X = X; v.U = U; v.win = win; v.XL = lw->XL; v.Zlog = sl->Z;
        v.done = a.done; v.iters = a.iters; v.flag = fl; v.hused = a.hused; v.ts = ts; v.nfin = nfin;
        v.flags = exitflag; v.itlog = sl->iterations;
        const int max_rounds = cl->steps * opt->max_iter;
        for (int r = 0; r < max_rounds; ++r) {
            BQP_TRY(sqp_iteration(a, qd, st));
            HIP_TRY(bqp::launch_sqp_loop_advance(v, st, par.get()));
            launches += sqp_iteration_launches(a) + 1;
            int nf = 0;
            HIP_TRY(hipMemcpyAsync(&nf, nfin, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (nf >= batch) break;
        }
    }
    for (int t = 0; t < (sync_loop ? cl->steps : 0); ++t) {
        HIP_TRY(bqp::launch_sqp_loop_prep(batch, nx, n, m, N * d->nu, t > 0 && sl->warm, s,
                                          sl->bin0, sl->Bx, bin, z, st));
        if (t > 0 && !sl->warm) HIP_TRY(hipMemsetAsync(z, 0, sizeof(double) * B * n, st));
        BQP_TRY(bqp_lbmpc_solve_batched_device(h, &dl, batch, &Dl, opt, z, nullptr, nullptr, fl, it,
                                               stream));
        launches += h->launches;
        HIP_TRY(bqp::launch_sqp_loop_u0(batch, nx, n, D->K, s, z, uo, it, cl->steps, t,
                                        sl->Z, sl->iterations, st));
        HIP_TRY(bqp::launch_mg_plant(cl->plant, batch, 1, cl->steps, t, cl->delta, uo, fl, cl->x_eq, cl->u_eq,
                                     s, X, U, exitflag, st, par.get()));
        HIP_TRY(bqp::launch_lbmpc_window(batch, cl->steps, t, q, bw, lam, D->A, 0, D->B, 0,
                                         cl->x_eq, cl->u_eq, X, U, win, lw->XL, st));
        launches += 3;
    }
    HIP_TRY(hipEventRecord(h->ev1, st));
    HIP_TRY(hipEventSynchronize(h->ev1));
    std::swap(h->ev0, e0.e);   // the guard destroys the previous start event
    h->timed = true;
    h->launches = launches;
    return BQP_OK;
}

int bqp_closed_loop_sqp(bqp_handle h, const bqp_lbmpc_dims* d, int batch,
                        const bqp_lbmpc_data* D, const bqp_sqp_loop* sl, const bqp_options* opt,
                        const bqp_closed_loop* cl, const bqp_learning* lw, const double* x_init,
                        double* X, double* U, int* exitflag) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(sqp_loop_check(d, batch, D, sl, cl, lw, x_init, X, U));
    BQP_TRY(plant_par_host_check(cl, batch));
    DevScope ds(h->device);
    const size_t B = batch, S = cl->steps, nx = d->nx, nu = d->nu, m = d->m, q = d->q;
    const size_t n = (size_t)d->N * nu + d->np;
    const size_t nX = B * (S + 1) * nx;
    Stage st(h);
    bqp_lbmpc_data Dd;
    bqp_sqp_loop sd = *sl;
    bqp_closed_loop cd = *cl;
    bqp_learning ld = *lw;
    const double* xi;
    double *Xd, *Ud;
    int *Fd, *Id;
    stage_lbmpc_model(st, d, D, &Dd);
    st.in(&Dd.Ain, D->Ain, m * n);
    st.in(&sd.bin0, sl->bin0, m);
    st.in(&sd.Bx, sl->Bx, m * nx);
    st.in(&xi, x_init, B * nx);
    st.in(&cd.x_eq, cl->x_eq, nx);
    st.in(&cd.u_eq, cl->u_eq, nu);
    stage_plant_par(st, cl, batch, &cd);
    st.out(&Xd, nX, X);
    st.out(&Ud, B * S * nu, U);
    st.out(&ld.XL, nX, lw->XL);
    st.out(&ld.window, B * q * 8, lw->window);
    if (sl->Z) st.out(&sd.Z, B * S * n, sl->Z);
    st.out(&Fd, B * S, exitflag);
    st.out(&Id, B * S, sl->iterations);
    BQP_TRY(st.commit());
    sd.iterations = sl->iterations ? Id : nullptr;
    BQP_TRY(bqp_closed_loop_sqp_device(h, d, batch, &Dd, &sd, opt, &cd, &ld, xi, Xd, Ud,
                                       exitflag ? Fd : nullptr, h->stream));
    return st.finish();
}

// ------------------------------------------------------------------------------------------
// nonlinear MPC on the true Moore-Greitzer model: single-shooting Gauss-Newton SQP (bqp_nmpc.hip)
// ------------------------------------------------------------------------------------------
static int nmpc_check(const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D, bool need_x0) {
    if (!d || !D || batch <= 0) return BQP_E_ARG;
    if (d->N <= 0 || d->mx < 0 || d->mu < 0 || d->n_poly < 0 || !(D->delta > 0)) return BQP_E_ARG;
    if (!D->Lq || !D->Lr || !D->Lp || !D->Lt || !D->LAMBDA || !D->PSI || !D->x_eq || !D->u_eq ||
        (d->mx > 0 && (!D->F_x || !D->h_x)) || (d->mu > 0 && (!D->F_u || !D->h_u)) ||
        (d->n_poly > 0 && (!D->F_T || !D->h_T)) || (need_x0 && !D->x0))
        return BQP_E_ARG;
    if (d->subproblem != 0 && d->subproblem != 1) return BQP_E_ARG;
    if (d->shooting != 0 && d->shooting != 1) return BQP_E_ARG;
    if (D->x_ref && D->sx_ref < 0) return BQP_E_ARG;
    if (!bqp::nmpc_supported(d->N, d->mx, d->mu)) return BQP_E_UNSUPPORTED;
    // multiple shooting lives on the stage route: its sub-problem is the stage QP with defects
    if (d->shooting == 1 && d->subproblem != 1) return BQP_E_UNSUPPORTED;
    const int64_t m = (int64_t)d->N * (d->mx + d->mu) + d->n_poly;
    if (m < 1 || m > 8192) return BQP_E_UNSUPPORTED;
    // stage route: the terminal rows are the structured kernel's polytope block
    if (d->subproblem == 1 && bqp::ocp_rpl_for(std::max(d->n_poly, 1)) < 0) return BQP_E_UNSUPPORTED;
    return BQP_OK;
}

// the set-point of D (bqp_nmpc_data.x_ref) as the launchers take it: null without one, and then
// every launch is the one it was before the member existed
struct NmpcRef {
    bqp::NmpcRefArgs r;
    explicit NmpcRef(const bqp_nmpc_data* D) : r{D->x_ref, D->sx_ref} {}
    const bqp::NmpcRefArgs* p() const { return r.xref ? &r : nullptr; }
    // Dense route with a set-point.  The dense interior-point sub-problem stops at a stationarity of
    // tol (1 + |f|), and the set-point adds g = -2 rho'T LAMBDA to f[N]: 1.9e3 for a target outside
    // the terminal set (rho = 2 LAMBDA, T = 1000 I).  There theta sits on a terminal row with a
    // multiplier of 7.6e2, the interior point stalls at a residual of 6.8e-6 - inside that bound at
    // the default 1e-8, so it reports convergence - and the smallest curvature over the moves (0.52)
    // turns it into 5.0e-6 in u_0 at N = 10, which the SQP then returns with flag 1.  Measured on
    // that sub-problem alone: the interior point does not get below the 5.0e-6 at any tolerance; the
    // active-set polish, reached once the tolerance makes it give up, is exact (3.6e-16).  So with a
    // set-point the sub-problems are held to 1e-2 of the caller's tolerance (1e-10 at the default;
    // at 1e-11 well-conditioned sub-problems of the same cases no longer end 1), and where the
    // caller leaves polish at its default 0 a sub-problem that ends 0 / -8 is polished (mode 1).
    // polish < 0 keeps it off.  Every other sub-problem measured ends 1 in the iterations it took
    // before (7-14), with the same error.
    void sharpen(bqp::DenseKernelArgs& q, const bqp_options& o) const {
        if (r.xref) q.tol_stat = std::min(q.tol_stat, 1e-2 * o.tol_stat);
    }
    int polish(const bqp_options& o) const { return (r.xref && o.polish == 0) ? 1 : 0; }
};

// the SQP's kernel arguments over the handle's nwork (done, ndone and the penalty zeroed) and
// the dense-kernel arguments of its sub-problem with the instance's own C; C, H, f: the
// caller's arrays (the linearisation's outputs) or null for the workspace's
static hipError_t nmpc_setup(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                             const bqp_options& o, double* C, double* H, double* f, hipStream_t st,
                             bqp::NmpcArgs& a, bqp::LbmpcArgs& ne, bqp::DenseKernelArgs* q) {
    const int N = d->N, n = N + 1, m = N * (d->mx + d->mu) + d->n_poly;
    const size_t B = batch;
    const layout::Nwork NL(batch, N, m, LB_NTRIAL);
    hipError_t e = h->nwork.reserve(NL.bytes);
    if (e != hipSuccess) return e;
    void* nw = h->nwork.p;
    memset(&a, 0, sizeof(a));
    a.N = N; a.n = n; a.nr = (int)NL.nr; a.m = m; a.mx = d->mx; a.mu = d->mu; a.mp = d->n_poly;
    a.batch = batch; a.ntrial = LB_NTRIAL; a.max_iter = o.max_iter;
    a.delta = D->delta;
    a.tol_step = o.tol_stat;            // as the learned-model SQP
    a.tol_stat = 10.0 * o.tol_stat;
    a.Lq = D->Lq; a.Lr = D->Lr; a.Lp = D->Lp; a.Lt = D->Lt; a.LAM = D->LAMBDA; a.PSI = D->PSI;
    a.xeq = D->x_eq; a.ueq = D->u_eq; a.Fx = D->F_x; a.hx = D->h_x; a.Fu = D->F_u; a.hu = D->h_u;
    a.FT = D->F_T; a.hT = D->h_T;
    a.x0 = D->x0; a.sx0 = D->sx0;
    a.Jr = layout::at<double>(nw, NL.Jr);
    a.er = layout::at<double>(nw, NL.er);
    a.H = H ? H : layout::at<double>(nw, NL.H);
    a.f = f ? f : layout::at<double>(nw, NL.f);
    a.C = C ? C : layout::at<double>(nw, NL.C);
    a.rhs = layout::at<double>(nw, NL.rhs);
    a.lam = layout::at<double>(nw, NL.lam);
    a.d = layout::at<double>(nw, NL.d);
    a.cost0 = layout::at<double>(nw, NL.cost0);
    a.costT = layout::at<double>(nw, NL.costT);
    a.violT = layout::at<double>(nw, NL.violT);
    a.stat = layout::at<double>(nw, NL.stat);
    a.cprev = layout::at<double>(nw, NL.cprev);
    a.nu = layout::at<double>(nw, NL.nu);
    a.qpflag = layout::at<int>(nw, NL.qpflag);
    a.done = layout::at<int>(nw, NL.done);
    a.ndone = layout::at<int>(nw, NL.ndone);
    if ((e = hipMemsetAsync(a.done, 0, sizeof(int) * (B + 1), st)) != hipSuccess) return e;   // done[], ndone
    if ((e = hipMemsetAsync(a.nu, 0, sizeof(double) * B, st)) != hipSuccess) return e;
    // normal equations: the learned-model path's kernel on this Jr / er; with m = 0 it forms no
    // constraint right-hand side and reads neither Ain nor bin
    memset(&ne, 0, sizeof(ne));
    ne.N = N; ne.n = n; ne.nr = a.nr; ne.m = 0; ne.batch = batch;
    ne.Jr = a.Jr; ne.er = a.er; ne.H = a.H; ne.f = a.f; ne.done = a.done;
    if (!q) return hipSuccess;
    // QP sub-problem (dense kernel): min 0.5 d'Hd + f'd  s.t.  C d <= -c, C per instance
    const int64_t wst = bqp::dense_work_doubles(n, m, 0);
    const layout::Dwork DL(wst, batch, bqp::STATS_W);
    if ((e = h->dwork.reserve(DL.bytes)) != hipSuccess) return e;
    bqp_options qo;
    bqp_default_options(&qo);
    memset(q, 0, sizeof(*q));
    q->n = n; q->m = m; q->me = 0; q->batch = batch; q->max_iter = 100;
    q->tol_stat = qo.tol_stat; q->tol_feas = qo.tol_feas; q->tol_comp = qo.tol_comp; q->tau = qo.tau;
    q->H = a.H; q->f = a.f; q->A = a.C; q->b = a.rhs;
    q->sH = (int64_t)n * n; q->sf = n; q->sA = (int64_t)m * n; q->sb = m;
    q->x = a.d; q->lam_ineqlin = a.lam; q->exitflag = a.qpflag;
    q->work = layout::at<double>(h->dwork.p, DL.scratch); q->work_stride = wst;
    q->skip = a.done;
    q->stats = layout::at<double>(h->dwork.p, DL.stats);
    return hipSuccess;
}

int bqp_nmpc_linearize_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                              const bqp_nmpc_data* D, const double* z, double* X, double* cost,
                              double* c, double* C, double* H, double* f, void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z) return BQP_E_ARG;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(nullptr, &o);
    bqp::NmpcArgs a;
    bqp::LbmpcArgs ne;
    HIP_TRY(nmpc_setup(h, d, batch, D, o, C, H, f, st, a, ne, nullptr));
    a.z = const_cast<double*>(z);       // read only by the rollout
    ne.z = a.z;
    a.Xout = X; a.cout = c;
    const NmpcRef ref(D);
    HIP_TRY(bqp::launch_nmpc_rollout(a, 1, st, nullptr, ref.p()));
    if (H || f) HIP_TRY(bqp::launch_lbmpc_normal(ne, st));
    if (cost) HIP_TRY(hipMemcpyAsync(cost, a.cost0, sizeof(double) * batch, hipMemcpyDeviceToDevice, st));
    return BQP_OK;
}

// registers the shared problem data of D with the stage; after st.commit() *Dd holds the device
// copies (x0 is the caller's to set); the set-points of the batch's instances with them
static void stage_nmpc_data(Stage& st, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                            bqp_nmpc_data* Dd) {
    const size_t mx = d->mx, mu = d->mu, mp = d->n_poly;
    *Dd = *D;
    st.in(&Dd->Lq, D->Lq, 16);          st.in(&Dd->Lr, D->Lr, 1);
    st.in(&Dd->Lp, D->Lp, 16);          st.in(&Dd->Lt, D->Lt, 16);
    st.in(&Dd->LAMBDA, D->LAMBDA, 4);   st.in(&Dd->PSI, D->PSI, 1);
    st.in(&Dd->x_eq, D->x_eq, 4);       st.in(&Dd->u_eq, D->u_eq, 1);
    st.in(&Dd->F_x, D->F_x, 4 * mx);    st.in(&Dd->h_x, D->h_x, mx);
    st.in(&Dd->F_u, D->F_u, mu);        st.in(&Dd->h_u, D->h_u, mu);
    st.in(&Dd->F_T, D->F_T, 5 * mp);    st.in(&Dd->h_T, D->h_T, mp);
    st.in(&Dd->xs_lin, D->xs_lin, mx);  st.in(&Dd->xs_quad, D->xs_quad, mx);
    st.in(&Dd->x_ref, D->x_ref, span(batch, D->sx_ref, 4));
}

// soft state rows (bqp_nmpc_data.xs_lin / xs_quad): a weight array is given
static bool nmpc_soft(const bqp_nmpc_data* D) { return D->xs_lin || D->xs_quad; }

// the solve and loop entries: the soft rows exist on the stage route only
static int nmpc_soft_check(const bqp_nmpc_dims* d, const bqp_nmpc_data* D) {
    return (nmpc_soft(D) && d->subproblem != 1) ? BQP_E_UNSUPPORTED : BQP_OK;
}

// every entry of a per-instance array of `per` doubles (stride 0: one block for the batch) finite
static bool nmpc_all_finite(const double* p, int batch, int64_t stride, size_t per) {
    if (!p) return true;
    for (int b = 0; b < (stride == 0 ? 1 : batch); ++b)
        for (size_t i = 0; i < per; ++i)
            if (!std::isfinite(p[(int64_t)b * stride + i])) return false;
    return true;
}

// host entry points: every weight finite and >= 0, every set-point finite (the device entries leave
// that to the caller)
static int nmpc_host_check(const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D) {
    for (const double* w : {D->xs_lin, D->xs_quad})
        if (w)
            for (int i = 0; i < d->mx; ++i)
                if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return BQP_E_ARG;
    return nmpc_all_finite(D->x_ref, batch, D->sx_ref, 4) ? BQP_OK : BQP_E_ARG;
}

// Stage route (bqp_nmpc_dims.subproblem = 1): the SQP's kernel arguments over the handle's nwork
// in its NworkStage layout, and the structured solve's call over the same arrays - per-stage models
// A_k, B_k (c = 0), the shared W and Fp, per-instance w, bounds and hp, x0 = 0, skip = done, duals
// requested.  The caller's A .. Fp (the diagnostic entry's outputs) replace the workspace's where
// non-null.
struct NmpcStageRoute {
    bqp::NmpcArgs a;
    bqp::NmpcStageArgs s;
    bqp_ocp_dims od;
    bqp_ocp_data oD;
    bqp_ocp_duals du;
    bqp_options qo;
    double *xo, *uo, *tho, *fv;
    int* sflag;
    // soft state rows: set where a weight is given and some row is softened by it (the table
    // kernel's finding); otherwise every launch is the hard route's own
    bool soft;
    bqp::NmpcSoftArgs q;
    const bqp::NmpcSoftArgs* softp() const { return soft ? &q : nullptr; }
    // the set-point (bqp_nmpc_data.x_ref): null without one
    bqp::NmpcRefArgs r;
    const bqp::NmpcRefArgs* refp() const { return r.xref ? &r : nullptr; }
    // multiple shooting (bqp_nmpc_dims.shooting = 1): the states of the iterate over the workspace's
    // Xw (the callers put their own array there), c_k = the defects, pi requested from the solve
    bool dms;
    bqp::NmpcDmsArgs m;
};

// use_soft = false: the weights of D are not read (the diagnostic bqp_nmpc_stage_qp)
static int nmpc_stage_setup(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                            const bqp_options& o, hipStream_t st, NmpcStageRoute& R,
                            const bqp::NmpcStageArgs* user = nullptr, bool use_soft = true,
                            bool dms = false) {
    const int N = d->N, n = N + 1, mp = d->n_poly, m = N * (d->mx + d->mu) + mp;
    const size_t B = batch;
    const bool want_soft = use_soft && nmpc_soft(D);
    const layout::NworkStage NL(batch, N, mp, m, LB_NTRIAL, sizeof(bqp::NmpcBoundMap), want_soft ? 1 : 0,
                                dms ? 1 : 0);
    if (getenv("BQP_LB_TRACE"))
        fprintf(stderr, "bqp nmpc stage route: workspace %zu bytes for %d instances\n", NL.bytes, batch);
    HIP_TRY(h->nwork.reserve(NL.bytes));
    void* nw = h->nwork.p;
    bqp::NmpcArgs& a = R.a;
    memset(&a, 0, sizeof(a));
    a.N = N; a.n = n; a.nr = 5 * N + 8; a.m = m; a.mx = d->mx; a.mu = d->mu; a.mp = mp;
    a.batch = batch; a.ntrial = LB_NTRIAL; a.max_iter = o.max_iter;
    a.delta = D->delta;
    a.tol_step = o.tol_stat;            // as the dense route
    a.tol_stat = 10.0 * o.tol_stat;
    a.Lq = D->Lq; a.Lr = D->Lr; a.Lp = D->Lp; a.Lt = D->Lt; a.LAM = D->LAMBDA; a.PSI = D->PSI;
    a.xeq = D->x_eq; a.ueq = D->u_eq; a.Fx = D->F_x; a.hx = D->h_x; a.Fu = D->F_u; a.hu = D->h_u;
    a.FT = D->F_T; a.hT = D->h_T;
    a.x0 = D->x0; a.sx0 = D->sx0;
    R.r = NmpcRef(D).r;
    a.f = layout::at<double>(nw, NL.f);
    a.ctl = layout::at<double>(nw, NL.ctl);
    a.rhs = layout::at<double>(nw, NL.rhs);
    a.lam = layout::at<double>(nw, NL.lam);
    a.d = layout::at<double>(nw, NL.d);
    a.cost0 = layout::at<double>(nw, NL.cost0);
    a.costT = layout::at<double>(nw, NL.costT);
    a.violT = layout::at<double>(nw, NL.violT);
    a.stat = layout::at<double>(nw, NL.stat);
    a.cprev = layout::at<double>(nw, NL.cprev);
    a.nu = layout::at<double>(nw, NL.nu);
    a.qpflag = layout::at<int>(nw, NL.qpflag);
    a.done = layout::at<int>(nw, NL.done);
    a.ndone = layout::at<int>(nw, NL.ndone);
    HIP_TRY(hipMemsetAsync(a.done, 0, sizeof(int) * (B + 1), st));   // done[], ndone
    HIP_TRY(hipMemsetAsync(a.nu, 0, sizeof(double) * B, st));
    bqp::NmpcStageArgs& s = R.s;
    memset(&s, 0, sizeof(s));
    auto pick = [&](double* u, const layout::Region& r) { return u ? u : layout::at<double>(nw, r); };
    s.A = pick(user ? user->A : nullptr, NL.A);
    s.B = pick(user ? user->B : nullptr, NL.B);
    s.w = pick(user ? user->w : nullptr, NL.w);
    s.xlb = pick(user ? user->xlb : nullptr, NL.xlb);
    s.xub = pick(user ? user->xub : nullptr, NL.xub);
    s.ulb = pick(user ? user->ulb : nullptr, NL.ulb);
    s.uub = pick(user ? user->uub : nullptr, NL.uub);
    s.hp = pick(user ? user->hp : nullptr, NL.hp);
    s.W = pick(user ? user->W : nullptr, NL.W);
    s.Fp = pick(user ? user->Fp : nullptr, NL.Fp);
    s.map = layout::at<bqp::NmpcBoundMap>(nw, NL.map);
    R.xo = layout::at<double>(nw, NL.xo);
    R.uo = layout::at<double>(nw, NL.uo);
    R.tho = layout::at<double>(nw, NL.tho);
    R.fv = layout::at<double>(nw, NL.fv);
    R.sflag = layout::at<int>(nw, NL.sflag);
    R.du.pi = nullptr;
    R.du.s_x = nullptr;
    R.du.lam_x = layout::at<double>(nw, NL.lamx);
    R.du.lam_u = layout::at<double>(nw, NL.lamu);
    R.du.lam_p = layout::at<double>(nw, NL.lamp);
    s.uo = R.uo; s.tho = R.tho; s.lamx = R.du.lam_x; s.lamu = R.du.lam_u; s.lamp = R.du.lam_p;
    s.sflag = R.sflag;
    double* x0z = layout::at<double>(nw, NL.x0z);
    HIP_TRY(hipMemsetAsync(x0z, 0, sizeof(double) * 4, st));
    R.soft = false;
    memset(&R.q, 0, sizeof(R.q));
    if (want_soft) {
        R.q.xs_lin = D->xs_lin; R.q.xs_quad = D->xs_quad;
        R.q.xsl = layout::at<double>(nw, NL.xsl);
        R.q.xsq = layout::at<double>(nw, NL.xsq);
        R.q.sx = layout::at<double>(nw, NL.sx);
        R.q.pen0 = layout::at<double>(nw, NL.pen0);
        R.q.plin = layout::at<double>(nw, NL.plin);
    }
    // the shared tables and the bound map; the map back, in one copy: F_x, F_u must be box rows,
    // and the softened rows must pair up as the structured solve's weights do
    HIP_TRY(bqp::launch_nmpc_stage_table(a, s, st, want_soft ? &R.q : nullptr));
    bqp::NmpcBoundMap hm;
    HIP_TRY(hipMemcpyAsync(&hm, s.map, sizeof(hm), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (hm.notbox || hm.unsupported) return BQP_E_UNSUPPORTED;
    if (dms && want_soft && hm.anysoft) return BQP_E_UNSUPPORTED;   // soft rows: single shooting only
    R.soft = want_soft && hm.anysoft;
    memset(&R.od, 0, sizeof(R.od));
    R.od.nx = 4; R.od.nu = 1; R.od.np = 1; R.od.N = N; R.od.n_poly = mp; R.od.poly_stage = N;
    R.od.stage_models = 1;
    bqp_ocp_data& oD = R.oD;
    memset(&oD, 0, sizeof(oD));
    oD.A = s.A; oD.sA = 16 * (int64_t)N;
    oD.B = s.B; oD.sB = 4 * (int64_t)N;
    oD.c = nullptr;
    oD.W = s.W; oD.sW = 0;
    oD.w = s.w; oD.sw = 6 * (int64_t)(N + 1);
    oD.xlb = s.xlb; oD.xub = s.xub; oD.sxb = 4 * (int64_t)(N + 1);
    oD.ulb = s.ulb; oD.uub = s.uub; oD.sub = N;
    oD.Fp = mp > 0 ? s.Fp : nullptr; oD.sFp = 0;
    oD.hp = mp > 0 ? s.hp : nullptr; oD.shp = mp;
    oD.x0 = x0z; oD.sx0 = 0;
    oD.skip = a.done;
    R.dms = dms;
    memset(&R.m, 0, sizeof(R.m));
    if (dms) {
        R.m.X = layout::at<double>(nw, NL.Xw);
        R.m.c = layout::at<double>(nw, NL.cdef);
        R.m.dX = R.xo;
        R.du.pi = layout::at<double>(nw, NL.piw);
        R.m.pi = R.du.pi;
        R.m.sw = layout::at<double>(nw, NL.sw);
        R.m.gn = layout::at<double>(nw, NL.gn);
        R.m.pimax = layout::at<double>(nw, NL.pimax);
        oD.c = R.m.c; oD.sc = 4 * (int64_t)N;
    }
    if (R.soft) {
        // the structured solve's soft state bounds: the tables shared by the batch, the slacks back
        oD.xs_lin = R.q.xsl; oD.xs_quad = R.q.xsq; oD.sxs = 0;
        R.du.s_x = const_cast<double*>(R.q.sx);
    }
    // the sub-problem's options: the structured solve's defaults with the dense sub-problem's
    // iteration limit; polish as the caller set it, in that solve's own encoding
    bqp_default_options(&R.qo);
    R.qo.max_iter = 100;
    R.qo.polish = o.polish;
    // Soft sub-problems have no active-set polish: the interior point's own stationarity bounds
    // the accuracy of the SQP's fixed point, so it follows the caller's tolerance, 1e-4 below it.
    // Measured (N = 10, start 0.05 above the x2 bound, tol 1e-10): the first free move is 9e-9
    // off the exact sub-problems' with the residual at 1e-13 (1 + |g|), 3e-10 at 1e-14.  A
    // sub-problem that cannot reach it ends 0 / -8 on its last interior iterate, which the update
    // kernel takes as is.
    if (R.soft) R.qo.tol_stat = std::min(R.qo.tol_stat, 1e-4 * o.tol_stat);
    return BQP_OK;
}

// one SQP round of the stage route: stage linearisation, structured solve (+ its repair launch),
// back-map, trial rollouts, update.  The structured call records the handle's own events and
// launch count; the callers keep theirs.  ev (may be null): 6 events around the 5 phases
static int nmpc_stage_round(bqp_handle h, const NmpcStageRoute& R, hipStream_t st, int* launches,
                            EventGuard* ev = nullptr) {
    auto mark = [&](int k) -> int {
        if (!ev) return BQP_OK;
        if (!ev[k].e) HIP_TRY(hipEventCreate(&ev[k].e));
        HIP_TRY(hipEventRecord(ev[k].e, st));
        return BQP_OK;
    };
    BQP_TRY(mark(0));
    if (R.dms) HIP_TRY(bqp::launch_nmpc_dms_linearize(R.a, R.s, R.m, st, R.refp()));
    else HIP_TRY(bqp::launch_nmpc_stage_rollout(R.a, R.s, st, R.softp(), R.refp()));
    BQP_TRY(mark(1));
    BQP_TRY(bqp_solve_ocp_batched_device(h, &R.od, R.a.batch, &R.oD, &R.qo, R.xo, R.uo, R.tho, R.fv, R.sflag,
                                         nullptr, &R.du, st));
    *launches += h->launches;
    BQP_TRY(mark(2));
    if (R.dms) {
        HIP_TRY(bqp::launch_nmpc_dms_backmap(R.a, R.s, R.m, st));
        BQP_TRY(mark(3));
        HIP_TRY(bqp::launch_nmpc_dms_trial(R.a, R.m, st, R.refp()));
        BQP_TRY(mark(4));
        HIP_TRY(bqp::launch_nmpc_dms_update(R.a, R.m, st));
        BQP_TRY(mark(5));
        *launches += 4;
        return BQP_OK;
    }
    HIP_TRY(bqp::launch_nmpc_stage_backmap(R.a, R.s, st, R.softp()));
    BQP_TRY(mark(3));
    HIP_TRY(bqp::launch_nmpc_rollout(R.a, 0, st, R.softp(), R.refp()));
    BQP_TRY(mark(4));
    HIP_TRY(bqp::launch_nmpc_update(R.a, st, R.softp()));
    BQP_TRY(mark(5));
    *launches += 4;
    return BQP_OK;
}

// the stage route's form of bqp_nmpc_solve_batched_device (arguments checked there).  Multiple
// shooting (d->shooting = 1): X (may be null: the workspace's) holds the states of the iterate, the
// start where roll = false, else the rollout of z is the start; pi (may be null) takes the dynamics
// multipliers
static int nmpc_solve_stage(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                            const bqp_options& o, double* z, double* lam, double* cost, int* exitflag,
                            int* iterations, hipStream_t st, double* X = nullptr, bool roll = true,
                            double* pi = nullptr) {
    const size_t B = batch;
    NmpcStageRoute R;
    BQP_TRY(nmpc_stage_setup(h, d, batch, D, o, st, R, nullptr, true, d->shooting == 1));
    bqp::NmpcArgs& a = R.a;
    a.z = z; a.flag = exitflag; a.iters = iterations;
    if (lam) a.lam = lam;
    if (R.dms) {
        if (X) R.m.X = X;
        if (pi) { R.du.pi = pi; R.m.pi = pi; }
        if (roll || !X) HIP_TRY(bqp::launch_nmpc_dms_start(a, R.m, st));
    }
    HIP_TRY(hipMemsetAsync(a.iters, 0, sizeof(int) * B, st));
    HIP_TRY(hipMemsetAsync(a.flag, 0, sizeof(int) * B, st));
    // the structured call records h->ev0 / ev1 for itself: this solve's start is an event of its own
    EventGuard e0;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventRecord(e0.e, st));
    int launches = 1 + ((R.dms && (roll || !X)) ? 1 : 0);   // the table launch, the start's rollout
    h->nmpc_rounds = 0;
    // BQP_LB_TRACE as on the dense route: 1 the sub-problems' exit flags, 2 per-launch event times
    const char* tenv = getenv("BQP_LB_TRACE");
    const bool trace = tenv && atoi(tenv) >= 2, trace_flags = tenv && !trace;
    EventGuard ev[6];
    for (int it = 0; it < o.max_iter; ++it) {
        BQP_TRY(nmpc_stage_round(h, R, st, &launches, trace ? ev : nullptr));
        ++h->nmpc_rounds;
        if (trace) {
            HIP_TRY(hipEventSynchronize(ev[5].e));
            float ms[5];
            for (int j = 0; j < 5; ++j) HIP_TRY(hipEventElapsedTime(&ms[j], ev[j].e, ev[j + 1].e));
            fprintf(stderr, "bqp nmpc it %d ms: stage-linearise %.3f structured(+repair) %.3f back-map %.3f trials %.3f update %.3f\n",
                    it, ms[0], ms[1], ms[2], ms[3], ms[4]);
        }
        if (trace_flags) {
            std::vector<int> fl(B), dn(B);
            HIP_TRY(hipMemcpyAsync(fl.data(), R.sflag, sizeof(int) * B, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(dn.data(), a.done, sizeof(int) * B, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            // (done as of the end of the round: an instance that stopped in it is still listed)
            for (size_t b = 0; b < B; ++b)
                fprintf(stderr, "bqp nmpc it %d instance %zu: stage sub-problem flag %d%s\n", it, b, fl[b],
                        dn[b] ? " (stopped)" : "");
        }
        if ((it + 1) % (a.n >= 64 ? 1 : 4) == 0 || it + 1 == o.max_iter) {
            int nd_h = 0;
            HIP_TRY(hipMemcpyAsync(&nd_h, a.ndone, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (nd_h >= batch) break;
        }
    }
    HIP_TRY(hipEventRecord(h->ev1, st));
    std::swap(h->ev0, e0.e);   // the guard destroys the previous start event
    h->timed = true;
    h->launches = launches;
    if (cost) HIP_TRY(hipMemcpyAsync(cost, a.cost0, sizeof(double) * B, hipMemcpyDeviceToDevice, st));
    return BQP_OK;
}

int bqp_nmpc_stage_qp_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                             const bqp_nmpc_data* D, const double* z, double* A, double* B,
                             double* w, double* xlb, double* xub, double* ulb, double* uub,
                             double* hp, double* W, double* Fp, void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z) return BQP_E_ARG;
    if (bqp::ocp_rpl_for(std::max(d->n_poly, 1)) < 0) return BQP_E_UNSUPPORTED;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(nullptr, &o);
    bqp::NmpcStageArgs user;
    memset(&user, 0, sizeof(user));
    user.A = A; user.B = B; user.w = w; user.xlb = xlb; user.xub = xub; user.ulb = ulb; user.uub = uub;
    user.hp = hp; user.W = W; user.Fp = Fp;
    NmpcStageRoute R;
    BQP_TRY(nmpc_stage_setup(h, d, batch, D, o, st, R, &user, false));
    R.a.z = const_cast<double*>(z);     // read only by the rollout
    HIP_TRY(bqp::launch_nmpc_stage_rollout(R.a, R.s, st, nullptr, R.refp()));
    return BQP_OK;
}

int bqp_nmpc_stage_cost(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                        const double* z, double* cost, double* penalty) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z) return BQP_E_ARG;
    BQP_TRY(nmpc_host_check(d, batch, D));
    if (bqp::ocp_rpl_for(std::max(d->n_poly, 1)) < 0) return BQP_E_UNSUPPORTED;
    DevScope ds(h->device);
    const size_t Bt = batch, N = d->N;
    Stage st(h);
    bqp_nmpc_data Dd;
    const double* zd;
    double *cd = nullptr, *pd = nullptr;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, 4));
    st.in(&zd, z, Bt * (N + 1));
    st.out(&cd, Bt, cost);
    st.out(&pd, Bt, penalty);
    BQP_TRY(st.commit());
    bqp_options o;
    resolve(nullptr, &o);
    NmpcStageRoute R;
    BQP_TRY(nmpc_stage_setup(h, d, batch, &Dd, o, h->stream, R));
    R.a.z = const_cast<double*>(zd);    // read only by the rollout
    HIP_TRY(bqp::launch_nmpc_stage_rollout(R.a, R.s, h->stream, R.softp(), R.refp()));
    HIP_TRY(hipMemcpyAsync(cd, R.a.cost0, sizeof(double) * Bt, hipMemcpyDeviceToDevice, h->stream));
    if (R.soft) HIP_TRY(hipMemcpyAsync(pd, R.q.pen0, sizeof(double) * Bt, hipMemcpyDeviceToDevice, h->stream));
    else HIP_TRY(hipMemsetAsync(pd, 0, sizeof(double) * Bt, h->stream));
    return st.finish();
}

int bqp_nmpc_stage_qp(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                      const double* z, double* A, double* B, double* w, double* xlb, double* xub,
                      double* ulb, double* uub, double* hp, double* W, double* Fp) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z) return BQP_E_ARG;
    BQP_TRY(nmpc_host_check(d, batch, D));
    DevScope ds(h->device);
    const size_t Bt = batch, N = d->N, mp = d->n_poly;
    Stage st(h);
    bqp_nmpc_data Dd;
    const double* zd;
    double *Ad = nullptr, *Bd = nullptr, *wd = nullptr, *xld = nullptr, *xud = nullptr, *uld = nullptr,
           *uud = nullptr, *hpd = nullptr, *Wd = nullptr, *Fpd = nullptr;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, 4));
    st.in(&zd, z, Bt * (N + 1));
    if (A) st.out(&Ad, Bt * N * 16, A);
    if (B) st.out(&Bd, Bt * N * 4, B);
    if (w) st.out(&wd, Bt * (N + 1) * 6, w);
    if (xlb) st.out(&xld, Bt * (N + 1) * 4, xlb);
    if (xub) st.out(&xud, Bt * (N + 1) * 4, xub);
    if (ulb) st.out(&uld, Bt * N, ulb);
    if (uub) st.out(&uud, Bt * N, uub);
    if (hp && mp) st.out(&hpd, Bt * mp, hp);
    if (W) st.out(&Wd, (N + 1) * 36, W);
    if (Fp && mp) st.out(&Fpd, mp * 6, Fp);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_nmpc_stage_qp_device(h, d, batch, &Dd, zd, Ad, Bd, wd, xld, xud, uld, uud, hpd, Wd, Fpd,
                                     h->stream));
    return st.finish();
}


int bqp_nmpc_linearize(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                       const double* z, double* X, double* cost, double* c, double* C, double* H,
                       double* f) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z) return BQP_E_ARG;
    BQP_TRY(nmpc_host_check(d, batch, D));
    DevScope ds(h->device);
    const size_t B = batch, N = d->N, n = N + 1, m = N * (size_t)(d->mx + d->mu) + d->n_poly;
    Stage st(h);
    bqp_nmpc_data Dd;
    const double* zd;
    double *Xd = nullptr, *cd = nullptr, *cvd = nullptr, *Cd = nullptr, *Hd = nullptr, *fd = nullptr;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, 4));
    st.in(&zd, z, B * n);
    if (X) st.out(&Xd, B * (N + 1) * 4, X);
    if (cost) st.out(&cd, B, cost);
    if (c) st.out(&cvd, B * m, c);
    if (C) st.out(&Cd, B * m * n, C);
    if (H) st.out(&Hd, B * n * n, H);
    if (f) st.out(&fd, B * n, f);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_nmpc_linearize_device(h, d, batch, &Dd, zd, Xd, cd, cvd, Cd, Hd, fd, h->stream));
    return st.finish();
}

int bqp_nmpc_solve_batched_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                  const bqp_nmpc_data* D, const bqp_options* opt, double* z,
                                  double* lam, double* cost, int* exitflag, int* iterations,
                                  void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z || !exitflag || !iterations) return BQP_E_ARG;
    BQP_TRY(nmpc_soft_check(d, D));
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(opt, &o);
    if (d->subproblem == 1) return nmpc_solve_stage(h, d, batch, D, o, z, lam, cost, exitflag, iterations, st);
    const size_t B = batch;
    bqp::NmpcArgs a;
    bqp::LbmpcArgs ne;
    bqp::DenseKernelArgs q;
    HIP_TRY(nmpc_setup(h, d, batch, D, o, nullptr, nullptr, nullptr, st, a, ne, &q));
    const NmpcRef ref(D);
    ref.sharpen(q, o);
    a.z = z; ne.z = z; a.flag = exitflag; a.iters = iterations;
    if (lam) { a.lam = lam; q.lam_ineqlin = lam; }
    HIP_TRY(hipMemsetAsync(a.iters, 0, sizeof(int) * B, st));
    HIP_TRY(hipMemsetAsync(a.flag, 0, sizeof(int) * B, st));
    HIP_TRY(hipEventRecord(h->ev0, st));
    int launches = 0;
    h->nmpc_rounds = 0;
    // BQP_LB_TRACE diagnostics on stderr, as the learned-model solve's: 1 the sub-problems' exit
    // flags per iteration (and whether their steps are finite), 2 per-launch event times instead.
    // Both wait for the stream at each iteration; neither launches a kernel.
    const char* tenv = getenv("BQP_LB_TRACE");
    const bool trace = tenv && atoi(tenv) >= 2, trace_flags = tenv && !trace;
    EventGuard ev[6];
    auto mark = [&](int k) -> int {
        if (!trace) return BQP_OK;
        if (!ev[k].e) HIP_TRY(hipEventCreate(&ev[k].e));
        HIP_TRY(hipEventRecord(ev[k].e, st));
        return BQP_OK;
    };
    for (int it = 0; it < o.max_iter; ++it) {
        // The sub-problems are polished only where the caller asks for it (opt->polish > 0), not by
        // default as in the learned-model solve.  A warm start of the closed loop lies on the state
        // rows that were active a step before (x2 at its lower bound in the stored run's
        // neighbourhood); the Jacobian of such a row of stage 1 w.r.t. u_0 is O(delta^3), the
        // polish's active-set system is then singular to working precision, and it returned a
        // non-finite step flagged converged (10 of 280 instance-steps of the perturbed stored run
        // ended -8 that way).  The interior-point iterate of those sub-problems (exit -8 once
        // mu ~ 1e-15, which the update kernel takes as is) is accurate: the same solves converge
        // in 2-3 SQP iterations without the polish.
        q.polish = o.polish > 0 ? sub_polish(o.polish, it >= LB_POLISH_STALL) : ref.polish(o);
        BQP_TRY(mark(0));
        HIP_TRY(bqp::launch_nmpc_rollout(a, 1, st, nullptr, ref.p()));
        BQP_TRY(mark(1));
        HIP_TRY(bqp::launch_lbmpc_normal(ne, st));
        BQP_TRY(mark(2));
        HIP_TRY(bqp::launch_dense(q, st));
        BQP_TRY(mark(3));
        if (trace_flags) {
            std::vector<int> fl(B), dn(B);
            std::vector<double> dv(B * a.n);
            HIP_TRY(hipMemcpyAsync(fl.data(), a.qpflag, sizeof(int) * B, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(dn.data(), a.done, sizeof(int) * B, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(dv.data(), a.d, sizeof(double) * B * a.n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (size_t b = 0; b < B; ++b) {
                if (dn[b]) continue;
                double dm = 0.0;
                for (int j = 0; j < a.n; ++j) dm = std::isfinite(dv[b * a.n + j]) ? std::max(dm, fabs(dv[b * a.n + j])) : INFINITY;
                fprintf(stderr, "bqp nmpc it %d instance %zu: sub-problem flag %d, |d| %.3e\n", it, b, fl[b], dm);
            }
        }
        HIP_TRY(bqp::launch_nmpc_rollout(a, 0, st, nullptr, ref.p()));
        BQP_TRY(mark(4));
        HIP_TRY(bqp::launch_nmpc_update(a, st));
        BQP_TRY(mark(5));
        launches += 5;
        ++h->nmpc_rounds;
        if (trace) {
            HIP_TRY(hipEventSynchronize(ev[5].e));
            float ms[5];
            for (int j = 0; j < 5; ++j) HIP_TRY(hipEventElapsedTime(&ms[j], ev[j].e, ev[j + 1].e));
            fprintf(stderr, "bqp nmpc it %d ms: linearise %.3f normal %.3f dense(+polish) %.3f trials %.3f update %.3f\n",
                    it, ms[0], ms[1], ms[2], ms[3], ms[4]);
        }
        // polled as the learned-model solve polls: after each iteration for large sub-problems
        if ((it + 1) % (a.n >= 64 ? 1 : 4) == 0 || it + 1 == o.max_iter) {
            int nd_h = 0;
            HIP_TRY(hipMemcpyAsync(&nd_h, a.ndone, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (nd_h >= batch) break;
        }
    }
    HIP_TRY(hipEventRecord(h->ev1, st));
    h->timed = true;
    h->launches = launches;
    if (cost) HIP_TRY(hipMemcpyAsync(cost, a.cost0, sizeof(double) * B, hipMemcpyDeviceToDevice, st));
    return BQP_OK;
}

int bqp_nmpc_solve_batched(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                           const bqp_nmpc_data* D, const bqp_options* opt, double* z,
                           double* lam, double* cost, int* exitflag, int* iterations) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z || !exitflag || !iterations) return BQP_E_ARG;
    BQP_TRY(nmpc_host_check(d, batch, D));
    BQP_TRY(nmpc_soft_check(d, D));
    DevScope ds(h->device);
    const size_t B = batch, N = d->N, n = N + 1, m = N * (size_t)(d->mx + d->mu) + d->n_poly;
    Stage st(h);
    bqp_nmpc_data Dd;
    double *zd, *ld, *cd;
    int *ed, *itd;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, 4));
    st.in(&zd, z, B * n, z);   // the initial iterate, and the solution
    st.out(&ld, B * m, lam);
    st.out(&cd, B, cost);
    st.out(&ed, B, exitflag);
    st.out(&itd, B, iterations);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_nmpc_solve_batched_device(h, d, batch, &Dd, opt, zd, ld, cd, ed, itd, h->stream));
    return st.finish();
}

// multiple shooting (bqp_nmpc_dims.shooting = 1): the solve with the states and the dynamics
// multipliers in its signature
int bqp_nmpc_dms_solve_batched_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                      const bqp_nmpc_data* D, const bqp_options* opt, double* z,
                                      double* X, double* lam, double* pi, double* cost, int* exitflag,
                                      int* iterations, void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z || !exitflag || !iterations || d->shooting != 1) return BQP_E_ARG;
    BQP_TRY(nmpc_soft_check(d, D));
    DevScope ds(h->device);
    bqp_options o;
    resolve(opt, &o);
    return nmpc_solve_stage(h, d, batch, D, o, z, lam, cost, exitflag, iterations, (hipStream_t)stream, X,
                            X == nullptr, pi);
}

int bqp_nmpc_dms_solve_batched(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                               const bqp_nmpc_data* D, const bqp_options* opt, double* z, double* X,
                               double* lam, double* pi, double* cost, int* exitflag, int* iterations) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z || !exitflag || !iterations || d->shooting != 1) return BQP_E_ARG;
    BQP_TRY(nmpc_host_check(d, batch, D));
    BQP_TRY(nmpc_soft_check(d, D));
    DevScope ds(h->device);
    const size_t B = batch, N = d->N, n = N + 1, m = N * (size_t)(d->mx + d->mu) + d->n_poly;
    Stage st(h);
    bqp_nmpc_data Dd;
    double *zd, *Xd = nullptr, *ld, *pd, *cd;
    int *ed, *itd;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, 4));
    st.in(&zd, z, B * n, z);   // the initial iterate, and the solution
    st.in(&Xd, X, B * n * 4, X);
    st.out(&ld, B * m, lam);
    st.out(&pd, B * N * 4, pi);
    st.out(&cd, B, cost);
    st.out(&ed, B, exitflag);
    st.out(&itd, B, iterations);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_nmpc_dms_solve_batched_device(h, d, batch, &Dd, opt, zd, Xd, ld, pd, cd, ed, itd, h->stream));
    return st.finish();
}

// the sub-problem at a given (X, z): the diagnostic counterpart of bqp_nmpc_stage_qp
int bqp_nmpc_dms_qp_device(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                           const double* X, const double* z, double* A, double* B, double* c, double* w,
                           double* xlb, double* xub, double* ulb, double* uub, double* hp, double* W,
                           double* Fp, void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z) return BQP_E_ARG;
    if (bqp::ocp_rpl_for(std::max(d->n_poly, 1)) < 0) return BQP_E_UNSUPPORTED;
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    bqp_options o;
    resolve(nullptr, &o);
    bqp::NmpcStageArgs user;
    memset(&user, 0, sizeof(user));
    user.A = A; user.B = B; user.w = w; user.xlb = xlb; user.xub = xub; user.ulb = ulb; user.uub = uub;
    user.hp = hp; user.W = W; user.Fp = Fp;
    NmpcStageRoute R;
    BQP_TRY(nmpc_stage_setup(h, d, batch, D, o, st, R, &user, false, true));
    R.a.z = const_cast<double*>(z);     // read only
    if (c) R.m.c = c;
    // the states into the workspace's copy (the linearisation pins its stage 0 to the measured state)
    if (X) HIP_TRY(hipMemcpyAsync(R.m.X, X, sizeof(double) * batch * 4 * (size_t)(d->N + 1), hipMemcpyDeviceToDevice, st));
    else HIP_TRY(bqp::launch_nmpc_dms_start(R.a, R.m, st));
    HIP_TRY(bqp::launch_nmpc_dms_linearize(R.a, R.s, R.m, st, R.refp()));
    return BQP_OK;
}

int bqp_nmpc_dms_qp(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                    const double* X, const double* z, double* A, double* B, double* c, double* w,
                    double* xlb, double* xub, double* ulb, double* uub, double* hp, double* W, double* Fp) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, true));
    if (!z) return BQP_E_ARG;
    BQP_TRY(nmpc_host_check(d, batch, D));
    DevScope ds(h->device);
    const size_t Bt = batch, N = d->N, mp = d->n_poly;
    Stage st(h);
    bqp_nmpc_data Dd;
    const double *zd, *Xd = nullptr;
    double *Ad = nullptr, *Bd = nullptr, *cd = nullptr, *wd = nullptr, *xld = nullptr, *xud = nullptr,
           *uld = nullptr, *uud = nullptr, *hpd = nullptr, *Wd = nullptr, *Fpd = nullptr;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&Dd.x0, D->x0, span(batch, D->sx0, 4));
    st.in(&zd, z, Bt * (N + 1));
    st.in(&Xd, X, Bt * (N + 1) * 4);
    if (A) st.out(&Ad, Bt * N * 16, A);
    if (B) st.out(&Bd, Bt * N * 4, B);
    if (c) st.out(&cd, Bt * N * 4, c);
    if (w) st.out(&wd, Bt * (N + 1) * 6, w);
    if (xlb) st.out(&xld, Bt * (N + 1) * 4, xlb);
    if (xub) st.out(&xud, Bt * (N + 1) * 4, xub);
    if (ulb) st.out(&uld, Bt * N, ulb);
    if (uub) st.out(&uud, Bt * N, uub);
    if (hp && mp) st.out(&hpd, Bt * mp, hp);
    if (W) st.out(&Wd, (N + 1) * 36, W);
    if (Fp && mp) st.out(&Fpd, mp * 6, Fp);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_nmpc_dms_qp_device(h, d, batch, &Dd, Xd, zd, Ad, Bd, cd, wd, xld, xud, uld, uud, hpd, Wd, Fpd,
                                   h->stream));
    return st.finish();
}

static int nmpc_loop_check(const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                           const bqp_closed_loop* cl, const double* x_init, const double* X,
                           const double* U) {
    if (!cl || !x_init || !X) return BQP_E_ARG;
    BQP_TRY(nmpc_check(d, batch, D, false));
    if (cl->plant != BQP_PLANT_MG_RK4 || cl->steps < 0 || !(cl->delta > 0) || !cl->x_eq || !cl->u_eq ||
        (cl->steps > 0 && !U))
        return BQP_E_ARG;
    BQP_TRY(plant_par_check(cl));
    return nmpc_soft_check(d, D);
}

// a schedule's stride: 0 (shared by the batch) or at least one instance's steps * 4
static int nmpc_track_check(const bqp_nmpc_track* tr, int steps) {
    if (!tr) return BQP_OK;
    for (int64_t sd : {tr->ref ? tr->sref : 0, tr->dist ? tr->sdist : 0})
        if (sd != 0 && sd < (int64_t)steps * 4) return BQP_E_ARG;
    return BQP_OK;
}

// bqp_closed_loop_nmpc_device (tr null: every launch is that loop's own) and
// bqp_closed_loop_nmpc_track_device
static int nmpc_loop_device(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                            const bqp_options* opt, const bqp_closed_loop* cl, const double* x_init,
                            const bqp_nmpc_track* tr, double* X, double* U, int* exitflag, int* iterations,
                            void* stream) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_loop_check(d, batch, D, cl, x_init, X, U));
    BQP_TRY(nmpc_track_check(tr, cl->steps));
    DevScope ds(h->device);
    hipStream_t st = (hipStream_t)stream;
    const int N = d->N, n = N + 1, S = cl->steps;
    const size_t B = batch;
    // BQP_NMPC_SYNC selects the step-synchronous loop below (the asynchronous loop's bitwise
    // reference in tests/test_gpu_nmpc_async.py, and the path BQP_LB_TRACE reports on)
    const bool sync_loop = getenv("BQP_NMPC_SYNC") != nullptr;
    const bool dms = d->shooting == 1;
    // a track with nothing in it is no track; a schedule replaces data->x_ref step by step
    const bool track = tr && S > 0 && (tr->ref || tr->dist || tr->THETA);
    const bool sched = track && tr->ref;
    const layout::CworkNmpc CL(batch, n, !sync_loop, dms, sched && !sync_loop);
    HIP_TRY(h->cwork.reserve(CL.bytes));
    bqp::NmpcTrackArgs k;
    memset(&k, 0, sizeof(k));
    if (track) {
        k.ref = tr->ref; k.sref = tr->ref ? tr->sref : 0;
        k.dist = tr->dist; k.sdist = tr->dist ? tr->sdist : 0;
        k.THETA = tr->THETA;
    }
    double* s = layout::at<double>(h->cwork.p, CL.s);
    double* z = layout::at<double>(h->cwork.p, CL.z);
    int* fl = layout::at<int>(h->cwork.p, CL.flags);
    int* it = layout::at<int>(h->cwork.p, CL.iters);
    double* Xit = dms ? layout::at<double>(h->cwork.p, CL.Xit) : nullptr;   // the iterate's states
    HIP_TRY(bqp::launch_closed_loop_init(batch, 4, S, x_init, cl->x_eq, s, X, st));
    HIP_TRY(hipMemsetAsync(z, 0, sizeof(double) * B * n, st));   // cold start: u = u_eq, theta = 0
    bqp_nmpc_data Dl = *D;
    if (sched && !sync_loop) {
        // the set-point each instance is at, kept as x0 is: step 0's here, the advance copies the rest
        k.xr = layout::at<double>(h->cwork.p, CL.xr);
        HIP_TRY(bqp::launch_nmpc_track_init(batch, k, st));
        Dl.x_ref = k.xr;
        Dl.sx_ref = 4;
    }
    EventGuard e0;
    HIP_TRY(hipEventCreate(&e0.e));
    HIP_TRY(hipEventRecord(e0.e, st));
    int launches = 0, rounds = 0;
    const LoopPlantPar par(cl);
    // the arguments of the advance (asynchronous) and of the track's plant launch (step-synchronous)
    bqp::NmpcAdvanceArgs v;
    memset(&v, 0, sizeof(v));
    v.batch = batch; v.N = N; v.steps = S; v.plant = cl->plant; v.delta = cl->delta;
    v.xeq = cl->x_eq; v.ueq = cl->u_eq;
    v.s = s; v.z = z; v.X = X; v.U = U; v.iters = it; v.flag = fl;
    v.flags = exitflag; v.itlog = iterations;
    if (!sync_loop && S > 0) {
        // asynchronous: every instance runs at its own closed-loop step.  Each round is one SQP
        // iteration of every unfinished instance, then nmpc_loop_advance_kernel moves the instances
        // whose SQP has stopped to their next step (logs, plant, warm start, measured state, the
        // per-solve state reset).  The step-synchronous form below runs every step's SQP launches
        // until the batch's slowest instance has stopped while the others idle; per instance the
        // two forms do the same operations in the same order.
        int* ts = layout::at<int>(h->cwork.p, CL.ts);
        int* nfin = layout::at<int>(h->cwork.p, CL.nfin);
        double* x0 = layout::at<double>(h->cwork.p, CL.x0);
        HIP_TRY(hipMemsetAsync(ts, 0, sizeof(int) * (B + 1), st));   // ts[], nfin
        HIP_TRY(hipMemcpyAsync(x0, x_init, sizeof(double) * B * 4, hipMemcpyDeviceToDevice, st));
        Dl.x0 = x0;                      // the measured states, absolute: the bits of X[b, ts[b]]
        Dl.sx0 = 4;
        bqp_options o;
        resolve(opt, &o);
        const bool stage = d->subproblem == 1;
        NmpcStageRoute R;
        bqp::NmpcArgs ad;
        bqp::LbmpcArgs ne;
        bqp::DenseKernelArgs q;
        if (stage) {
            BQP_TRY(nmpc_stage_setup(h, d, batch, &Dl, o, st, R, nullptr, true, dms));
            launches += 1;               // the table launch
        } else {
            HIP_TRY(nmpc_setup(h, d, batch, &Dl, o, nullptr, nullptr, nullptr, st, ad, ne, &q));
        }
        bqp::NmpcArgs& a = stage ? R.a : ad;
        a.z = z; ne.z = z; a.flag = fl; a.iters = it;
        HIP_TRY(hipMemsetAsync(it, 0, sizeof(int) * B, st));
        HIP_TRY(hipMemsetAsync(fl, 0, sizeof(int) * B, st));
        if (dms) {
            // multiple shooting: the first solve starts from the rollout of the cold z, every later
            // one from the warm start of the states
            R.m.X = Xit;
            HIP_TRY(bqp::launch_nmpc_dms_start(a, R.m, st));
            launches += 1;
        }
        // sub-problem polish only where the caller asks for it (bqp_nmpc_solve_batched_device), per
        // instance from its own SQP iteration count: mode 2 from LB_POLISH_STALL on
        q.polish = o.polish > 0 ? sub_polish(o.polish, false) : 0;
        q.pol_it = o.polish > 0 ? a.iters : nullptr;
        q.pol_stall = LB_POLISH_STALL;
        v.x0 = x0; v.nu = a.nu; v.done = a.done; v.ts = ts; v.nfin = nfin;
        const NmpcRef ref(&Dl);
        if (!stage) {                    // dense route with a set-point: NmpcRef::sharpen
            ref.sharpen(q, o);
            if (o.polish <= 0) q.polish = ref.polish(o);
        }
        // an instance stops within max_iter rounds of its step's first: the bound is never reached
        const int64_t max_rounds = (int64_t)S * o.max_iter;
        for (int64_t r = 0; r < max_rounds; ++r) {
            if (stage) {
                BQP_TRY(nmpc_stage_round(h, R, st, &launches));
            } else {
                HIP_TRY(bqp::launch_nmpc_rollout(a, 1, st, nullptr, ref.p()));
                HIP_TRY(bqp::launch_lbmpc_normal(ne, st));
                HIP_TRY(bqp::launch_dense(q, st));
                HIP_TRY(bqp::launch_nmpc_rollout(a, 0, st, nullptr, ref.p()));
                HIP_TRY(bqp::launch_nmpc_update(a, st));
                launches += 5;
            }
            if (dms) {
                HIP_TRY(bqp::launch_nmpc_dms_loop_states(batch, N, S, D->delta, D->u_eq, z, Xit, a.done, ts, st));
                launches += 1;
            }
            HIP_TRY(bqp::launch_nmpc_loop_advance(v, st, track ? &k : nullptr, par.get()));
            launches += 1;
            ++rounds;
            int nf = 0;
            HIP_TRY(hipMemcpyAsync(&nf, nfin, sizeof(int), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (nf >= batch) break;
        }
    }
    for (int t = 0; t < (sync_loop ? S : 0); ++t) {
        Dl.x0 = X + (int64_t)t * 4;      // the measured states X[:, t], absolute
        Dl.sx0 = (int64_t)(S + 1) * 4;
        if (sched) {                     // the set-points ref[:, t]
            Dl.x_ref = k.ref + (int64_t)t * 4;
            Dl.sx_ref = k.sref;
        }
        if (dms) {
            bqp_options o;
            resolve(opt, &o);
            BQP_TRY(nmpc_solve_stage(h, d, batch, &Dl, o, z, nullptr, nullptr, fl, it, st, Xit, t == 0));
        } else {
            BQP_TRY(bqp_nmpc_solve_batched_device(h, d, batch, &Dl, opt, z, nullptr, nullptr, fl, it, stream));
        }
        launches += h->launches;
        rounds += h->nmpc_rounds;
        // the plant reads u_0 - u_eq = z[b, 0] (stride n); a track's plant launch also adds the
        // disturbance and logs theta
        if (track) HIP_TRY(bqp::launch_nmpc_track_plant(v, k, t, st, par.get()));
        else HIP_TRY(bqp::launch_mg_plant(cl->plant, batch, n, S, t, cl->delta, z, fl, cl->x_eq, cl->u_eq,
                                          s, X, U, exitflag, st, par.get()));
        if (dms) {
            HIP_TRY(bqp::launch_nmpc_dms_loop_states(batch, N, S, D->delta, D->u_eq, z, Xit, nullptr, nullptr, st));
            launches += 1;
        }
        HIP_TRY(bqp::launch_nmpc_loop_shift(batch, N, S, t, z, it, iterations, st));
        launches += 2;
    }
    HIP_TRY(hipEventRecord(h->ev1, st));
    HIP_TRY(hipEventSynchronize(h->ev1));
    std::swap(h->ev0, e0.e);   // the guard destroys the previous start event
    h->timed = true;
    h->launches = launches;
    h->loop_rounds = rounds;
    return BQP_OK;
}

int bqp_closed_loop_nmpc_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                const bqp_nmpc_data* D, const bqp_options* opt,
                                const bqp_closed_loop* cl, const double* x_init, double* X,
                                double* U, int* exitflag, int* iterations, void* stream) {
    return nmpc_loop_device(h, d, batch, D, opt, cl, x_init, nullptr, X, U, exitflag, iterations, stream);
}

int bqp_closed_loop_nmpc_track_device(bqp_handle h, const bqp_nmpc_dims* d, int batch,
                                      const bqp_nmpc_data* D, const bqp_options* opt,
                                      const bqp_closed_loop* cl, const double* x_init,
                                      const bqp_nmpc_track* tr, double* X, double* U, int* exitflag,
                                      int* iterations, void* stream) {
    return nmpc_loop_device(h, d, batch, D, opt, cl, x_init, tr, X, U, exitflag, iterations, stream);
}

int bqp_closed_loop_nmpc_track(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                               const bqp_options* opt, const bqp_closed_loop* cl, const double* x_init,
                               const bqp_nmpc_track* tr, double* X, double* U, int* exitflag,
                               int* iterations) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_loop_check(d, batch, D, cl, x_init, X, U));
    BQP_TRY(nmpc_track_check(tr, cl->steps));
    BQP_TRY(nmpc_host_check(d, batch, D));
    BQP_TRY(plant_par_host_check(cl, batch));
    const size_t B = batch, S = cl->steps;
    if (tr && (!nmpc_all_finite(tr->ref, batch, tr->sref, S * 4) ||
               !nmpc_all_finite(tr->dist, batch, tr->sdist, S * 4)))
        return BQP_E_ARG;
    DevScope ds(h->device);
    Stage st(h);
    bqp_nmpc_data Dd;
    bqp_closed_loop cd = *cl;
    bqp_nmpc_track td;
    memset(&td, 0, sizeof(td));
    const double* xi;
    double *Xd, *Ud, *Td = nullptr;
    int *Fd, *Id;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&xi, x_init, B * 4);
    st.in(&cd.x_eq, cl->x_eq, 4);
    st.in(&cd.u_eq, cl->u_eq, 1);
    stage_plant_par(st, cl, batch, &cd);
    if (tr) {
        td.sref = tr->sref; td.sdist = tr->sdist;
        st.in(&td.ref, tr->ref, span(batch, tr->sref, S * 4));
        st.in(&td.dist, tr->dist, span(batch, tr->sdist, S * 4));
        if (tr->THETA) st.out(&Td, B * S, tr->THETA);
    }
    st.out(&Xd, B * (S + 1) * 4, X);
    st.out(&Ud, B * S, U);
    st.out(&Fd, B * S, exitflag);
    st.out(&Id, B * S, iterations);
    BQP_TRY(st.commit());
    td.THETA = Td;
    BQP_TRY(nmpc_loop_device(h, d, batch, &Dd, opt, &cd, xi, tr ? &td : nullptr, Xd, Ud,
                             exitflag ? Fd : nullptr, iterations ? Id : nullptr, h->stream));
    return st.finish();
}

int bqp_closed_loop_nmpc(bqp_handle h, const bqp_nmpc_dims* d, int batch, const bqp_nmpc_data* D,
                         const bqp_options* opt, const bqp_closed_loop* cl, const double* x_init,
                         double* X, double* U, int* exitflag, int* iterations) {
    if (!h) return BQP_E_ARG;
    BQP_TRY(nmpc_loop_check(d, batch, D, cl, x_init, X, U));
    BQP_TRY(nmpc_host_check(d, batch, D));
    BQP_TRY(plant_par_host_check(cl, batch));
    DevScope ds(h->device);
    const size_t B = batch, S = cl->steps;
    Stage st(h);
    bqp_nmpc_data Dd;
    bqp_closed_loop cd = *cl;
    const double* xi;
    double *Xd, *Ud;
    int *Fd, *Id;
    stage_nmpc_data(st, d, batch, D, &Dd);
    st.in(&xi, x_init, B * 4);
    st.in(&cd.x_eq, cl->x_eq, 4);
    st.in(&cd.u_eq, cl->u_eq, 1);
    stage_plant_par(st, cl, batch, &cd);
    st.out(&Xd, B * (S + 1) * 4, X);
    st.out(&Ud, B * S, U);
    st.out(&Fd, B * S, exitflag);
    st.out(&Id, B * S, iterations);
    BQP_TRY(st.commit());
    BQP_TRY(bqp_closed_loop_nmpc_device(h, d, batch, &Dd, opt, &cd, xi, Xd, Ud, exitflag ? Fd : nullptr,
                                        iterations ? Id : nullptr, h->stream));
    return st.finish();
}

#ifdef BQP_STAMPS
// diagnostic build only: per-instance phase cycle counts of the last structured solve
// (32 per instance: 16 stage-wave phases, 16 row-wave phases)
int bqp_debug_stamps(bqp_handle h, int N, int nv, int mp, double* out) {
    if (!h || !out) return BQP_E_ARG;
    DevScope ds(h->device);
    const int mpad = 64 * bqp::ocp_rpl_for(std::max(mp, 1));
    const layout::Work WL = work_layout(N, nv, mpad, h->last_batch);
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, layout::at<double>(h->work.p, WL.stamps), WL.stamps.bytes, hipMemcpyDeviceToHost));
    return BQP_OK;
}
#endif

}  // extern "C"
