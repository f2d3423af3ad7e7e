// bqp_plant_par.h — where the Moore-Greitzer plant's coefficients of one instance and one step lie
// (bqp_closed_loop.plant_par): p = [x2_c, 1/beta^2, wn^2, 2 zeta wn], four doubles, shared by the
// batch or per instance, constant over the loop or one row per step (a schedule).
//
// Plain C++ that compiles for the host and the device: the plant and advance kernels
// (bqp_plant.hip, bqp_nmpc.hip) load an instance's row with these functions, bqp_api.cpp checks the
// host entries' values with them, tests/host/plant_par_check.cpp calls them from loops under the
// host sanitizers.  No HIP header, no LDS.
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

constexpr int PLANT_NPAR = 4;

// Device pointer (host pointer in the host check).  A separate, trailing kernel argument of the
// parametrised instantiations; the nominal ones never read it.
struct PlantPar {
    const double* p;   // null: the nominal plant (the kernels that existed before the member did)
    int64_t stride;    // doubles between two instances' blocks; 0: one block for the batch
    int sched;         // 0: 4 doubles per instance; 1: steps x 4, row t is the plant of step t
};

// a launch with coefficients: a pointer, a stride and a schedule flag in range
BQP_HD inline bool plant_par_args_ok(const PlantPar& k) {
    return k.p && k.stride >= 0 && (k.sched == 0 || k.sched == 1);
}

// the doubles of one instance's block
BQP_HD inline int64_t plant_par_block(int steps, int sched) {
    return sched ? (int64_t)steps * PLANT_NPAR : PLANT_NPAR;
}

// a stride is 0 or at least one instance's block
BQP_HD inline bool plant_par_stride_ok(int64_t stride, int steps, int sched) {
    return stride == 0 || stride >= plant_par_block(steps, sched);
}

// the doubles the loop reads through p for `batch` instances (the last instance's block ends there)
BQP_HD inline int64_t plant_par_span(int batch, int64_t stride, int steps, int sched) {
    return (int64_t)(batch - 1) * stride + plant_par_block(steps, sched);
}

// first coefficient of the plant that takes X[b, t] to X[b, t + 1], t < steps: row steps does not exist
BQP_HD inline int64_t plant_par_at(int64_t stride, int sched, int b, int t) {
    return (int64_t)b * stride + (sched ? (int64_t)t * PLANT_NPAR : 0);
}

// the four coefficients of instance b at step t, into registers before the integrator
BQP_HD inline void plant_par_load(const PlantPar& k, int b, int t, double (&p)[4]) {
    const double* r = k.p + plant_par_at(k.stride, k.sched, b, t);
    for (int i = 0; i < PLANT_NPAR; ++i) p[i] = r[i];
}

// what the host entries admit: finite, 1/beta^2 > 0, wn^2 > 0, 2 zeta wn >= 0
BQP_HD inline bool plant_par_row_ok(const double* r) {
    for (int i = 0; i < PLANT_NPAR; ++i)
        if (!(r[i] - r[i] == 0.0)) return false;   // NaN or infinite
    return r[1] > 0.0 && r[2] > 0.0 && r[3] >= 0.0;
}

}  // namespace bqp
