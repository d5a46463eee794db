// tu_f64_grid.hip — Float64 pipeline of a metric SAMPLED ON A GRID (RTGR_GRID, include/rtgr.h): the tricubic interpolant's g and ∂g
// (rtgr_grid_interp.hpp: grid_eval, sampled_accel) into the generic contraction, and the OUTSIDE rule of the integrate loop (rtgr_integrate.hpp).
#include "rtgr_pipeline.hpp"
namespace rtgr {
int launch_f64_grid(LaunchEnv& E, const TraceArgs<double>& A, hipStream_t st) {
    return launch_trace<double, RTGR_GENERIC_BASE + RTGR_GRID, true>(E, A, st);
}
}  // namespace rtgr
