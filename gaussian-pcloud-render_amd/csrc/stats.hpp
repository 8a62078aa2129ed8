// stats.hpp -- the instrumentation layer (builds with -DGSR_STATS only) of the kernels that time their phases: the render kernels
// (through render_walk.hpp), k_radix_scatter (sort.hip) and k_duplicate (binning.hip).
// The kernels time their phases and count their work through these two macros, which expand to nothing in the product build, so
// that the arithmetic can be read without the bookkeeping: WALK_T(t) takes a time stamp (10-ns ticks), WALK_STAT(...) holds
// declarations or statements of the instrumentation build.  The record arrays and their readers (debug_* of common.hpp) stay with
// their kernels, outside any kernel, and read the device's rows through read_wave_records.
#pragma once

#include <hip/hip_runtime.h>

namespace gsr {

#ifdef GSR_STATS
#define WALK_T(var) const unsigned long long var = wall_clock64()
#define WALK_STAT(...) __VA_ARGS__
// The host's copy of a per-wave record array (one row of W words per wave of the LAST launch -- same-address atomics from 390 K
// waves would be what gets measured); with `reset` the device's rows are cleared once they are copied.  NULL: a HIP call failed.
template <int REC, int W>
const unsigned (*read_wave_records(unsigned (&dev)[REC][W], int reset))[W]
{
    static unsigned host[REC][W], zeros[REC][W];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(dev), sizeof(host)) != hipSuccess) return nullptr;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(dev), zeros, sizeof(zeros)) != hipSuccess) return nullptr;
    return host;
}
#else
#define WALK_T(var)
#define WALK_STAT(...)
#endif

}  // namespace gsr
