// Stand-alone check of csrc/bqp_lanes.h, the lane-group mapping of the short-horizon stage wave:
// the Makefile builds it with g++ -std=c++17 -fsanitize=address,undefined
// (build/lane_map_check), tests/test_host_lane_map.py runs it.
//
// For both model families (MG: nx 4, nu 1, np 1; DI: nx 2, nu 2, np 2), every lane-group count G
// and every horizon N = 1..63:
//   1. where G is compiled and G (N + 1) <= 64: every (stage, entry) of s_k / pi_k is formed by
//      exactly one unclamped slot, that slot's lane is owner_lane(), no lane index reaches 64, the
//      lanes of group 0 are lanes 0..N (the G = 1 lanes, which write the outputs), and a clamped
//      slot repeats entry ns - 1;
//   2. the dispatch's choice satisfies G (N + 1) <= 64, is compiled, and is never larger than the
//      BQP_OCP_LANE_GROUPS cap (1, 2, 3 or unset); a cap of 1 always selects G = 1.
#include <stdio.h>

#include <vector>

#include "bqp_lanes.h"

using namespace bqp::lanes;

static int failures = 0;
static long checks = 0;

#define EXPECT(cond)                                                                       \
    do {                                                                                   \
        ++checks;                                                                          \
        if (!(cond)) {                                                                     \
            ++failures;                                                                    \
            fprintf(stderr, "%s:%d: %s failed (ns %d nu %d G %d N %d)\n", __FILE__, __LINE__, #cond, ns, nu, G, N); \
        }                                                                                  \
    } while (0)

// box rows per lane of the instantiation the launch selects for a one-stage-per-lane horizon
// (bqp_ocp.hip launch_spl): all (N + 1) 2 (nx + nu) box rows over 64 lanes, 4 or 10 per lane
static int bpl_for(int N, int nx, int nu) {
    const int nbr = (N + 1) * 2 * (nx + nu);
    return nbr <= 4 * WAVE_LANES ? 4 : (nbr <= 10 * WAVE_LANES ? 10 : -1);
}

static void check_map(int ns, int nu, int G, int N) {
    const int ES = entries_per_lane(ns, G);
    EXPECT(ES * G >= ns);
    // owners[k * ns + i]: lanes whose unclamped slot is entry i of stage k
    std::vector<std::vector<int>> owners((size_t)(N + 1) * ns);
    std::vector<int> lanes_of_stage(N + 1, 0);
    for (int lane = 0; lane < WAVE_LANES; ++lane) {
        const StageLane sl = stage_lane(lane, N, G);
        EXPECT(sl.g >= 0 && sl.g < G);
        EXPECT(sl.k >= 0);
        if (sl.k > N) {
            EXPECT(lane >= G * (N + 1));     // only the lanes past the last group are idle
            continue;
        }
        EXPECT(lane == sl.k + sl.g * (N + 1));
        if (sl.g == 0) EXPECT(lane == sl.k); // group 0 = the G = 1 lanes
        ++lanes_of_stage[sl.k];
        for (int t = 0; t < ES; ++t) {
            const int raw = sl.g * ES + t, e = entry(ns, G, sl.g, t);
            EXPECT(e >= 0 && e < ns);
            if (raw < ns) {
                EXPECT(e == raw);
                owners[(size_t)sl.k * ns + e].push_back(lane);
            } else {
                EXPECT(e == ns - 1);         // a slot past the last entry repeats it
            }
        }
    }
    for (int k = 0; k <= N; ++k) {
        EXPECT(lanes_of_stage[k] == G);
        for (int i = 0; i < ns; ++i) {
            const std::vector<int>& o = owners[(size_t)k * ns + i];
            EXPECT(o.size() == 1);
            if (o.size() == 1) {
                EXPECT(o[0] == owner_lane(ns, G, N, k, i));
                EXPECT(o[0] < WAVE_LANES);
            }
        }
    }
}

int main() {
    const int fam[2][3] = {{4, 1, 1}, {2, 2, 2}};   // nx, nu, np
    for (const auto& f : fam) {
        const int nx = f[0], nu = f[1], ns = f[0] + f[2];
        for (int N = 1; N <= 63; ++N) {
            for (int G = 1; G <= MAX_GROUPS; ++G)
                if (compiled(ns, nu, G) && G * (N + 1) <= WAVE_LANES) check_map(ns, nu, G, N);
            const int bpl = bpl_for(N, nx, nu);
            int prev = 0;
            for (int cap = 1; cap <= MAX_GROUPS; ++cap) {
                const int G = groups_for(N, ns, nu, bpl, cap);
                EXPECT(G >= 1 && G <= cap);
                EXPECT(compiled(ns, nu, G));
                EXPECT(G * (N + 1) <= WAVE_LANES);
                EXPECT(G == 1 || bpl == 4);
                EXPECT(G >= prev);           // a larger cap never selects fewer groups
                if (cap == 1) EXPECT(G == 1);
                prev = G;
            }
        }
    }
    {   // the flagship shape: MG, N = 20 runs three groups on 63 lanes; N = 21 one
        const int ns = 5, nu = 1;
        int G = 3, N = 20;
        EXPECT(groups_for(20, ns, nu, 4, MAX_GROUPS) == 3);
        EXPECT(groups_for(21, ns, nu, 4, MAX_GROUPS) == 1);
        EXPECT(groups_for(20, ns, nu, 4, 2) == 1);   // MG has no G = 2 instantiation
        EXPECT(groups_for(20, 4, 2, 4, MAX_GROUPS) == 1);   // DI stays at one lane per stage
        EXPECT(stage_lane(62, N, G).k == 20 && stage_lane(62, N, G).g == 2);
        EXPECT(stage_lane(63, N, G).k > N);
        EXPECT(entry(ns, G, 2, 0) == 4 && entry(ns, G, 2, 1) == 4);
    }
    printf("lane_map_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
