// bqp_lanes.h — lane groups of the short-horizon stage wave (bqp_ocp.hip).
//
// With one stage per lane a horizon of N = 20 uses 21 of the 64 lanes, and each of them walks
// through all entries of its stage in the per-stage passes.  With G lane groups stage k is served
// by the G lanes k + g (N + 1), g < G: the s-part entries (s_k, pi_k and the vectors shaped like
// them) are dealt out in runs of ES = ceil(NS / G), lane (k, g) forms entries g ES .. g ES + ES - 1.
// A slot past the last entry repeats entry NS - 1: the same operations on the same operands, the
// same value stored to the same address.  The u part (NU entries) and the iterate registers are
// replicated: every lane of a stage holds the stage's whole s_k, u_k, pi_k and applies the same
// updates to them, and group 0 (lanes 0..N, the G = 1 lanes) writes the outputs.
//
// Plain C++17 constexpr, no HIP: tests/host/lane_map_check.cpp compiles it with g++.
#pragma once

#if defined(__HIPCC__)
#define BQP_LANES_HD __host__ __device__
#else
#define BQP_LANES_HD
#endif

namespace bqp::lanes {

constexpr int WAVE_LANES = 64;
constexpr int MAX_GROUPS = 3;

// the lane-group counts compiled for a model family (ns = nx + np), fp64 and fp32 alike: G = 1
// always; G = 3 for the MG family (ns 5, nu 1).  The DI family (ns 4, nu 2) stays at one lane per
// stage.  The dispatch (bqp_ocp.hip launch_rpl) instantiates from this predicate alone.
BQP_LANES_HD constexpr bool compiled(int ns, int nu, int G) {
    return G == 1 || (G == 3 && ns == 5 && nu == 1);
}

struct StageLane { int k, g; };   // k > N: the lane serves no stage

// lane -> (stage, group); compares instead of a division by N + 1 (G <= 3)
BQP_LANES_HD constexpr StageLane stage_lane(int lane, int N, int G) {
    const int n1 = N + 1;
    const int g = (G > 1 && lane >= n1 ? 1 : 0) + (G > 2 && lane >= 2 * n1 ? 1 : 0);
    return {lane - g * n1, g};
}

// s-part entries per lane
BQP_LANES_HD constexpr int entries_per_lane(int ns, int G) { return (ns + G - 1) / G; }

// s-part entry formed by slot t < entries_per_lane of group g (clamped: see above)
BQP_LANES_HD constexpr int entry(int ns, int G, int g, int t) {
    const int e = g * entries_per_lane(ns, G) + t;
    return e < ns ? e : ns - 1;
}

// the lane that owns entry i of s_k / pi_k: the one slot with the unclamped index i
BQP_LANES_HD constexpr int owner_lane(int ns, int G, int N, int k, int i) {
    return k + (i / entries_per_lane(ns, G)) * (N + 1);
}

// the dispatch's choice for horizon N: the largest compiled G <= cap whose G (N + 1) lanes fit the
// wave (cap: the BQP_OCP_LANE_GROUPS override, MAX_GROUPS when unset); G > 1 exists only in the
// one-stage-per-lane instantiations with four box rows per lane (bpl 4)
BQP_LANES_HD constexpr int groups_for(int N, int ns, int nu, int bpl, int cap) {
    for (int G = cap < MAX_GROUPS ? cap : MAX_GROUPS; G > 1; --G)
        if (compiled(ns, nu, G) && bpl == 4 && G * (N + 1) <= WAVE_LANES) return G;
    return 1;
}

}  // namespace bqp::lanes
