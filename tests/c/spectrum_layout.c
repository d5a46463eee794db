/* spectrum_layout.c — a plain C caller of the disk-spectra part of include/rtgr.h, compiled with gcc by tests/test_spectrum.py.
 *
 * Pins the byte layout of rtgr_spectrum (what julia/RayTraceGRHIP.jl's RtgrSpectrum and raytracegr.jl_amd/_abi.py mirror) as
 * _Static_asserts, and with a library path resolves the eight entry points:
 *   spectrum_layout           prints "spectrum <size> kind <off> flags <off> nb <off> lo <off> hi <off> amp <off> alpha <off> rho_min <off>
 *                             rho_max <off> g_power <off> reserved <off>"
 *   spectrum_layout <lib>     … exits 2 when one of the entry points does not resolve
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_spectrum) == 80, "rtgr_spectrum");
_Static_assert(offsetof(rtgr_spectrum, kind) == 0 && offsetof(rtgr_spectrum, flags) == 4 && offsetof(rtgr_spectrum, nb) == 8 &&
               offsetof(rtgr_spectrum, lo) == 16 && offsetof(rtgr_spectrum, hi) == 24 && offsetof(rtgr_spectrum, amp) == 32 &&
               offsetof(rtgr_spectrum, alpha) == 40 && offsetof(rtgr_spectrum, rho_min) == 48 && offsetof(rtgr_spectrum, rho_max) == 56 &&
               offsetof(rtgr_spectrum, g_power) == 64 && offsetof(rtgr_spectrum, reserved) == 72,
               "rtgr_spectrum fields");
_Static_assert(RTGR_SPECTRUM_MAX_BINS == (1ull << 16) && RTGR_SPEC_LINE == 0 && RTGR_SPEC_THERMAL == 1 && RTGR_SPEC_LOG == 1u && RTGR_SPEC_NU3 == 2u,
               "constants");

int main(int argc, char** argv) {
    printf("spectrum %zu kind %zu flags %zu nb %zu lo %zu hi %zu amp %zu alpha %zu rho_min %zu rho_max %zu g_power %zu reserved %zu\n",
           sizeof(rtgr_spectrum), offsetof(rtgr_spectrum, kind), offsetof(rtgr_spectrum, flags), offsetof(rtgr_spectrum, nb),
           offsetof(rtgr_spectrum, lo), offsetof(rtgr_spectrum, hi), offsetof(rtgr_spectrum, amp), offsetof(rtgr_spectrum, alpha),
           offsetof(rtgr_spectrum, rho_min), offsetof(rtgr_spectrum, rho_max), offsetof(rtgr_spectrum, g_power), offsetof(rtgr_spectrum, reserved));
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        static const char* const names[] = {"rtgr_spectrum_device_f64", "rtgr_spectrum_device_f32", "rtgr_trace_spectrum_device_f64",
                                            "rtgr_trace_spectrum_device_f32", "rtgr_trace_spectrum_f64", "rtgr_trace_spectrum_f32",
                                            "rtgr_eval_spectrum_f64", "rtgr_eval_spectrum_f32"};
        for (unsigned k = 0; k < sizeof names / sizeof names[0]; k++)
            if (!dlsym(h, names[k])) { fprintf(stderr, "%s\n", names[k]); return 2; }
    }
    return 0;
}
