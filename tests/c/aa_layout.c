/* aa_layout.c — a plain C caller of the anti-aliasing part of include/rtgr.h, compiled with gcc by tests/test_aa.py.
 *
 * Pins the byte layout of rtgr_aa and rtgr_aa_stats (what julia/RayTraceGRHIP.jl's RtgrAA / RtgrAAStats and raytracegr.jl_amd/_abi.py
 * mirror) as _Static_asserts, and with a library path resolves the four entry points and calls the host-pointer one:
 *   aa_layout                prints "aa <size> k <off> flags <off> contrast <off> max_batch_rays <off> stats <size> pixels <off> refined <off>
 *                            sub_rays <off> batches <off>"
 *   aa_layout <lib>          … exits 2 when one of rtgr_trace_aa_device_f64 / _f32, rtgr_trace_aa_f64 / _f32 does not resolve; otherwise
 *                            calls rtgr_trace_aa_f64 on a 2 x 2 Minkowski canvas and prints "rc <code> touched <0|1>" (touched: the
 *                            rgb array no longer holds what the caller put there)
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_aa) == 24, "rtgr_aa");
_Static_assert(offsetof(rtgr_aa, k) == 0 && offsetof(rtgr_aa, flags) == 4 && offsetof(rtgr_aa, contrast) == 8 &&
               offsetof(rtgr_aa, max_batch_rays) == 16, "rtgr_aa fields");
_Static_assert(sizeof(rtgr_aa_stats) == 32, "rtgr_aa_stats");
_Static_assert(offsetof(rtgr_aa_stats, pixels) == 0 && offsetof(rtgr_aa_stats, refined) == 8 && offsetof(rtgr_aa_stats, sub_rays) == 16 &&
               offsetof(rtgr_aa_stats, batches) == 24, "rtgr_aa_stats fields");

typedef int (*aa_f64_fn)(rtgr_context*, const rtgr_scene*, const rtgr_solver*, const rtgr_camera*, uint64_t, uint64_t, const rtgr_aa*, double*,
                         const rtgr_ray_outputs*, uint8_t*, rtgr_counters*, rtgr_aa_stats*);
typedef int (*defaults_fn)(rtgr_solver*, int);

int main(int argc, char** argv) {
    printf("aa %zu k %zu flags %zu contrast %zu max_batch_rays %zu stats %zu pixels %zu refined %zu sub_rays %zu batches %zu\n", sizeof(rtgr_aa),
           offsetof(rtgr_aa, k), offsetof(rtgr_aa, flags), offsetof(rtgr_aa, contrast), offsetof(rtgr_aa, max_batch_rays), sizeof(rtgr_aa_stats),
           offsetof(rtgr_aa_stats, pixels), offsetof(rtgr_aa_stats, refined), offsetof(rtgr_aa_stats, sub_rays), offsetof(rtgr_aa_stats, batches));
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        aa_f64_fn aa_f64 = (aa_f64_fn)dlsym(h, "rtgr_trace_aa_f64");
        defaults_fn defaults = (defaults_fn)dlsym(h, "rtgr_solver_defaults");
        if (!aa_f64 || !defaults || !dlsym(h, "rtgr_trace_aa_f32") || !dlsym(h, "rtgr_trace_aa_device_f64") || !dlsym(h, "rtgr_trace_aa_device_f32"))
            return 2;
        rtgr_scene sc;
        memset(&sc, 0, sizeof sc);
        sc.metric = RTGR_MINKOWSKI;
        sc.M = 1.0;
        rtgr_solver opt;
        if (defaults(&opt, 0) != 0) return 3;
        rtgr_camera cam = {{0, 0, -2, 0}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}};
        rtgr_aa aa = {2, 0, 1.0 / 255.0, 0};
        double rgb[12];
        for (int q = 0; q < 12; q++) rgb[q] = -7.0;
        rtgr_aa_stats stats;
        const int rc = aa_f64(NULL, &sc, &opt, &cam, 2, 2, &aa, rgb, NULL, NULL, NULL, &stats);
        int touched = 0;
        for (int q = 0; q < 12; q++) touched |= rgb[q] != -7.0;
        printf("rc %d touched %d\n", rc, touched);
    }
    return 0;
}
