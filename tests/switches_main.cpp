// Stand-alone host program over csrc/switches.hpp (tests/test_cpu_switches.py compiles it with g++ under the address and
// undefined-behaviour sanitizers and runs it once per value of the environment variables).
//
//   switches_main            every variable unset
//   switches_main VALUE      every variable set to VALUE with setenv before the first use of any switch
//
// GSR_TICKETS is the one variable the header reads when the program is loaded, before main: the test passes that one through the
// program's environment as well.  Prints one line per row of the header's table: the name, then what the switch answers -- for the
// rows with a setter the query and the setter sequence of tests/switch_pins.py.
#include <cstdio>
#include <cstdlib>

#include "switches.hpp"

static void row(const char* name, int (*f)(int))
{
    static const int sequence[] = {-1, 0, -7, 1, 2, 3, 255, -1};
    printf("%s %d", name, f(-1));
    for (int s : sequence) printf(" %d", f(s));
    printf("\n");
}

int main(int argc, char** argv)
{
    static const char* const vars[] = {"GSR_FWD_HALF_V", "GSR_RENDER_MATH", "GSR_TRAIN_MATH", "GSR_BWD_SUBQ", "GSR_TICKETS",
                                       "GSR_ORDER_KNEE", "GSR_ORDER_EXP", "GSR_CONTRIB_REDUCE"};
    for (const char* v : vars) {
        if (argc > 1) setenv(v, argv[1], 1);
        else unsetenv(v);
    }
    printf("block_tickets %d\n", gsr::block_tickets(-1));   // (before the rows below: what the load left)
    row("forward_half_views", gsr::forward_half_views);
    row("render_math", gsr::render_math);
    row("train_math", gsr::train_math);
    row("backward_subquadrant_moments", gsr::backward_subquadrant_moments);
    row("block_tickets_set", gsr::block_tickets);
    float knee = 0.f, expo = 0.f;
    gsr::tile_order_params(knee, expo);
    printf("tile_order_knee %.9g\ntile_order_exp %.9g\n", (double)knee, (double)expo);
    setenv("GSR_ORDER_KNEE", "7", 1);   // read once: a later change is not seen ...
    gsr::tile_order_params(knee, expo);
    printf("tile_order_knee_again %.9g\n", (double)knee);
    printf("contrib_lane_reduce %d", gsr::contrib_lane_reduce());
    setenv("GSR_CONTRIB_REDUCE", "1", 1);   // ... read at every launch: it is
    printf(" %d", gsr::contrib_lane_reduce());
    setenv("GSR_CONTRIB_REDUCE", "0", 1);
    printf(" %d\n", gsr::contrib_lane_reduce());
    printf("forward_fast_math %d %d %d %d\n", (int)gsr::forward_fast_math(false, false), (int)gsr::forward_fast_math(false, true),
           (int)gsr::forward_fast_math(true, false), (int)gsr::forward_fast_math(true, true));
    return 0;
}
