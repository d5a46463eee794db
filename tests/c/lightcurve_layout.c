/* lightcurve_layout.c — a plain C caller of the hot-spot light-curve part of include/rtgr.h, compiled with gcc by tests/test_light_curve.py.
 *
 * Pins the byte layout of rtgr_hot_spot (what julia/RayTraceGRHIP.jl's RtgrHotSpot and raytracegr.jl_amd/_abi.py mirror) as
 * _Static_asserts, and with a library path resolves the eight entry points:
 *   lightcurve_layout           prints "hot_spot <size> rho_s <off> phi0 <off> sigma <off> cut <off> amp <off> g_power <off> t_start <off> dt <off>
 *                               nt <off> flags <off> pad <off>"
 *   lightcurve_layout <lib>     … exits 2 when one of the entry points does not resolve
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_hot_spot) == 80, "rtgr_hot_spot");
_Static_assert(offsetof(rtgr_hot_spot, rho_s) == 0 && offsetof(rtgr_hot_spot, phi0) == 8 && offsetof(rtgr_hot_spot, sigma) == 16 &&
               offsetof(rtgr_hot_spot, cut) == 24 && offsetof(rtgr_hot_spot, amp) == 32 && offsetof(rtgr_hot_spot, g_power) == 40 &&
               offsetof(rtgr_hot_spot, t_start) == 48 && offsetof(rtgr_hot_spot, dt) == 56 && offsetof(rtgr_hot_spot, nt) == 64 &&
               offsetof(rtgr_hot_spot, flags) == 72 && offsetof(rtgr_hot_spot, pad) == 76,
               "rtgr_hot_spot fields");
_Static_assert(RTGR_HOT_SPOT_MAX_SAMPLES == (1ull << 20), "constants");

int main(int argc, char** argv) {
    printf("hot_spot %zu rho_s %zu phi0 %zu sigma %zu cut %zu amp %zu g_power %zu t_start %zu dt %zu nt %zu flags %zu pad %zu\n", sizeof(rtgr_hot_spot),
           offsetof(rtgr_hot_spot, rho_s), offsetof(rtgr_hot_spot, phi0), offsetof(rtgr_hot_spot, sigma), offsetof(rtgr_hot_spot, cut),
           offsetof(rtgr_hot_spot, amp), offsetof(rtgr_hot_spot, g_power), offsetof(rtgr_hot_spot, t_start), offsetof(rtgr_hot_spot, dt),
           offsetof(rtgr_hot_spot, nt), offsetof(rtgr_hot_spot, flags), offsetof(rtgr_hot_spot, pad));
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        static const char* const names[] = {"rtgr_light_curve_device_f64", "rtgr_light_curve_device_f32", "rtgr_trace_light_curve_device_f64",
                                            "rtgr_trace_light_curve_device_f32", "rtgr_trace_light_curve_f64", "rtgr_trace_light_curve_f32",
                                            "rtgr_eval_hot_spot_f64", "rtgr_eval_hot_spot_f32"};
        for (unsigned k = 0; k < sizeof names / sizeof names[0]; k++)
            if (!dlsym(h, names[k])) { fprintf(stderr, "%s\n", names[k]); return 2; }
    }
    return 0;
}
