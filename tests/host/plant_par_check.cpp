// Stand-alone check of csrc/bqp_plant_par.h, where the Moore-Greitzer plant's coefficients of one
// instance and one step lie (bqp_closed_loop.plant_par): the Makefile builds it with
// g++ -std=c++17 -fsanitize=address,undefined (build/plant_par_check),
// tests/test_host_plant_par.py runs it.
//
// For steps 1 and 2, batch 1 and 257, shared (stride 0) and per-instance stride - the tight one
// and one with a gap -, constant and scheduled coefficients: the coefficients sit in a heap buffer
// of exactly plant_par_span doubles (an index past it stops the program under the address
// sanitizer), and plant_par_load of every (instance, step < steps) must return what a plain loop
// nest wrote there.  A schedule's row `steps` does not exist: the buffer ends where the last
// instance's row steps - 1 ends, which the span check pins.  Also the stride rule and the value
// rule of the host entries.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <initializer_list>

#include "bqp_plant_par.h"

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

// the value a plain loop nest puts at coefficient i of (instance b, row t)
static double value(int b, int t, int i) { return 1000.0 * b + 10.0 * t + i + 0.5; }

static void run(int steps, int batch, int64_t stride, int sched) {
    static char name[96];
    snprintf(name, sizeof(name), "steps %d batch %d stride %lld sched %d", steps, batch, (long long)stride, sched);
    what = name;
    const int rows = sched ? steps : 1;
    EXPECT(bqp::plant_par_block(steps, sched) == (int64_t)rows * 4);
    EXPECT(bqp::plant_par_stride_ok(stride, steps, sched));
    // the documented size: the last instance's block ends the buffer
    const int64_t n = bqp::plant_par_span(batch, stride, steps, sched);
    EXPECT(n == (int64_t)(batch - 1) * stride + (int64_t)rows * 4);
    double* buf = (double*)malloc((size_t)n * sizeof(double));
    for (int64_t i = 0; i < n; ++i) buf[i] = -1.0;   // a gap between blocks stays -1
    // plain loop nest; with a shared block every instance writes the same values
    for (int b = 0; b < batch; ++b)
        for (int t = 0; t < rows; ++t)
            for (int i = 0; i < 4; ++i)
                buf[(stride ? (int64_t)b * stride : 0) + (int64_t)t * 4 + i] = value(stride ? b : 0, t, i);
    const bqp::PlantPar k = {buf, stride, sched};
    EXPECT(bqp::plant_par_args_ok(k));
    int64_t hi = -1;
    for (int b = 0; b < batch; ++b)
        for (int t = 0; t < steps; ++t) {   // every step the loop takes; never row `steps`
            const int64_t at = bqp::plant_par_at(stride, sched, b, t);
            EXPECT(at >= 0 && at + 4 <= n);
            if (at + 4 > hi) hi = at + 4;
            double p[4] = {0, 0, 0, 0};
            bqp::plant_par_load(k, b, t, p);
            for (int i = 0; i < 4; ++i) EXPECT(p[i] == value(stride ? b : 0, sched ? t : 0, i));
        }
    EXPECT(hi == n);   // the last step of the last instance reads the buffer's last double
    free(buf);
}

int main() {
    for (int steps : {1, 2})
        for (int batch : {1, 257})
            for (int sched : {0, 1}) {
                const int64_t block = bqp::plant_par_block(steps, sched);
                for (int64_t stride : {(int64_t)0, block, block + 3}) run(steps, batch, stride, sched);
            }
    what = "stride rule";
    EXPECT(bqp::plant_par_stride_ok(0, 5, 1) && bqp::plant_par_stride_ok(20, 5, 1) && bqp::plant_par_stride_ok(4, 5, 0));
    EXPECT(!bqp::plant_par_stride_ok(19, 5, 1) && !bqp::plant_par_stride_ok(3, 5, 0) && !bqp::plant_par_stride_ok(-4, 5, 0));
    EXPECT(!bqp::plant_par_stride_ok(4, 2, 1));
    what = "value rule";
    const double nominal[4] = {0.0, 1.0, 1000.0, 2.0 * sqrt(500.0)};
    EXPECT(bqp::plant_par_row_ok(nominal));
    for (int i = 0; i < 4; ++i)
        for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
            double p[4] = {nominal[0], nominal[1], nominal[2], nominal[3]};
            p[i] = bad;
            EXPECT(!bqp::plant_par_row_ok(p));
        }
    {
        double p[4] = {-0.05, 1.0, 1000.0, 0.0};   // x2_c of either sign, no damping: admitted
        EXPECT(bqp::plant_par_row_ok(p));
        p[1] = 0.0; EXPECT(!bqp::plant_par_row_ok(p)); p[1] = -1.0; EXPECT(!bqp::plant_par_row_ok(p)); p[1] = 1.0;
        p[2] = 0.0; EXPECT(!bqp::plant_par_row_ok(p)); p[2] = -1.0; EXPECT(!bqp::plant_par_row_ok(p)); p[2] = 1000.0;
        p[3] = -1e-300; EXPECT(!bqp::plant_par_row_ok(p));
    }
    const bqp::PlantPar none = {nullptr, 0, 0}, neg = {nominal, -4, 0}, sch = {nominal, 0, 2};
    EXPECT(!bqp::plant_par_args_ok(none) && !bqp::plant_par_args_ok(neg) && !bqp::plant_par_args_ok(sch));
    printf("plant_par_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
