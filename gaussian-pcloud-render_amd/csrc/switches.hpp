// switches.hpp -- every process-wide switch of the library: its environment variable, its default, when the variable is read and what a
// setter call does.  Host code without a HIP include (tests/switches_main.cpp compiles it with g++), and the only place under csrc/
// that reads the environment.
//
//   switch                        variable            unset  read              from the variable's text               setter call with set >= 0
//   forward_half_views            GSR_FWD_HALF_V      1      first use         atoi; negative -> 0                    stored as given
//   render_math                   GSR_RENDER_MATH     0      first use         1 iff atoi == 1                        0 / 1 stored; above 1 refused
//   train_math                    GSR_TRAIN_MATH      0      first use         1 iff atoi == 1                        0 / 1 stored; above 1 refused
//   backward_subquadrant_moments  GSR_BWD_SUBQ        2      first use         atoi; outside 0..2 -> 2                stored as min(set, 2)
//   block_tickets                 GSR_TICKETS         1      library load      0 iff atoi == 0                        stored as set != 0
//   tile_order_params             GSR_ORDER_KNEE      2048   first use, once   atof                                   (no setter)
//                                 GSR_ORDER_EXP       0.3    first use, once   atof                                   (no setter)
//   contrib_lane_reduce           GSR_CONTRIB_REDUCE  0      every launch      1 iff atoi == 1                        (no setter)
//
// A setter call with set < 0 only queries; every call returns the value in force.  "First use" is the first call of the switch's
// function, query or set: a value set before anything read the variable wins over the variable.
#pragma once

#include <atomic>
#include <cstdlib>

namespace gsr {

struct Switch {
    const char* var;
    int (*from_env)(const char* text);   // text: the variable's, NULL when it is unset
    int (*accept)(int set);              // what a setter call with set >= 0 stores; negative: the call is refused
    std::atomic<int> held{-1};           // negative: the variable has not been read yet
};

// the one query / set body of the rows above that have a setter
inline int switch_value(Switch& s, int set)
{
    if (set >= 0) {
        const int v = s.accept(set);
        if (v >= 0) s.held.store(v);
    }
    int v = s.held.load();
    if (v < 0) {
        v = s.from_env(getenv(s.var));
        s.held.store(v);
    }
    return v;
}

inline int one_iff_1(const char* e) { return (e && atoi(e) == 1) ? 1 : 0; }
inline int zero_or_one(int set) { return set <= 1 ? set : -1; }

// views per submission up to which the forward runs in half-quadrant mode (0: never); gsr_set_forward_half_views() (tests compare
// the two kernels in one process)
inline Switch g_fwd_half_v{"GSR_FWD_HALF_V", [](const char* e) { const int v = e ? atoi(e) : 1; return v < 0 ? 0 : v; },
                           [](int set) { return set; }};
inline int forward_half_views(int set) { return switch_value(g_fwd_half_v, set); }

// arithmetic of the forwards that save nothing for a backward (0 exact, 1 fast); gsr_set_render_math()
inline Switch g_render_math{"GSR_RENDER_MATH", one_iff_1, zero_or_one};
inline int render_math(int set) { return switch_value(g_render_math, set); }

// arithmetic of the colour forwards that DO save for a backward (need_backward = 1; the backward then runs the matching fast kernels,
// render_bwd.hip RenderBwdFast); gsr_set_train_math().  Neither of the two switches moves the other.
inline Switch g_train_math{"GSR_TRAIN_MATH", one_iff_1, zero_or_one};
inline int train_math(int set) { return switch_value(g_train_math, set); }

// which arithmetic a render forward runs: the inference switch without saves, the training switch with them; a channels forward that
// saves stays exact (the channels backward has no fast variant)
inline bool forward_fast_math(bool with_ckpt, bool channels)
{
    if (!with_ckpt) return render_math(-1) == 1;
    return !channels && train_math(-1) == 1;
}

// Which moments the render backward's contraction takes: 0 about the quadrant centre, 1 about the four sub-quadrant centres (mean2D /
// conic sums at the reference build's accuracy, for more flush arithmetic), 2 the sub-quadrant ones only for the batches that hold a
// flagged splat (render_bwd.hip MODE).  gsr_set_backward_moments() (tests, scripts/bwd_accuracy.py).
constexpr int BWD_SUBQ_DEFAULT = 2;
inline Switch g_bwd_subq{"GSR_BWD_SUBQ", [](const char* e) { const int v = e ? atoi(e) : BWD_SUBQ_DEFAULT; return v < 0 || v > 2 ? BWD_SUBQ_DEFAULT : v; },
                         [](int set) { return set > 2 ? 2 : set; }};
inline int backward_subquadrant_moments(int set) { return switch_value(g_bwd_subq, set); }

// How the pair emission, whose workgroups wait for lower-numbered workgroups of the same launch, numbers its workgroups.
// 1 (default): by a ticket drawn with an atomic when the workgroup STARTS -- a lower number has started earlier, so the
// waits below can only be for workgroups that are running or done, whatever order the hardware dispatches blockIdx in (HIP promises
// none; rocPRIM's look-back scans draw tickets for the same reason).  The price: every workgroup of a launch hits ONE address, and
// same-address atomics from eight XCDs complete at about one per 13-70 ns: 10 us of a single view's 52-us emission.
// 0 (GSR_TICKETS=0, opt-in): by blockIdx -- correct as long as the hardware hands the workgroups of a launch to each XCD in
// increasing order (it does today: workgroup i goes to XCD i mod 8, each XCD takes its share in order; the lowest-numbered unfinished
// workgroup is then always resident or next in line, waits for nothing unfinished, and by induction every wait ends), which is an
// observation about this part, not a contract.  Every wait is bounded either way (CNT_STALL: the frame fails, it does not hang).
inline int tickets_from_env(const char* e) { return e && atoi(e) == 0 ? 0 : 1; }
inline Switch g_tickets{"GSR_TICKETS", tickets_from_env, [](int set) { return set != 0 ? 1 : 0; }, {tickets_from_env(getenv("GSR_TICKETS"))}};
inline int block_tickets(int set) { return switch_value(g_tickets, set); }

// knee and exponent of the work estimate the forward's tiles are ordered by (binning.hip k_tile_order)
inline float env_float(const char* var, float unset)
{
    const char* e = getenv(var);
    return e ? (float)atof(e) : unset;
}
inline void tile_order_params(float& knee, float& expo)
{
    static const float k = env_float("GSR_ORDER_KNEE", 2048.f), x = env_float("GSR_ORDER_EXP", 0.3f);
    knee = k;
    expo = x;
}

// which lane reduction k_contrib_stats runs (0: DPP; 1: shuffle butterflies -- for measurements that alternate the two in one
// process, same results)
inline int contrib_lane_reduce() { return one_iff_1(getenv("GSR_CONTRIB_REDUCE")); }

}  // namespace gsr
