// tu_f32_grid.hip — Float32 pipeline of a metric sampled on a grid (RTGR_GRID): the same kernels over the Float32 copy of the samples.
#include "rtgr_pipeline.hpp"
namespace rtgr {
int launch_f32_grid(LaunchEnv& E, const TraceArgs<float>& A, hipStream_t st) {
    return launch_trace<float, RTGR_GENERIC_BASE + RTGR_GRID, true>(E, A, st);
}
}  // namespace rtgr
