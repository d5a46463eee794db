// tu_f64_grid4.hip — Float64 pipeline of a TIME-DEPENDENT metric sampled on a 4-D grid (rtgr_grid4_metric_load): the
// 4-D interpolant's g and four partials (rtgr_grid_interp.hpp: grid4_eval, sampled_accel) into the generic contraction at every stage's own t, and
// the OUTSIDE rule on four axes (rtgr_integrate.hpp).
#include "rtgr_pipeline.hpp"
namespace rtgr {
int launch_f64_grid4(LaunchEnv& E, const TraceArgs<double>& A, hipStream_t st) {
    return launch_trace<double, RTGR_GENERIC_BASE + (int)RTGR_GRID4, true>(E, A, st);
}
}  // namespace rtgr
