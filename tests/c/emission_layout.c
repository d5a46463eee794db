/* emission_layout.c — a plain C caller of the disk-emission part of include/rtgr.h, compiled with gcc by tests/test_emission.py.
 *
 * Pins the byte layout of rtgr_disk_emission (what julia/RayTraceGRHIP.jl's RtgrDiskEmission and raytracegr.jl_amd/_abi.py mirror) as
 * _Static_asserts, and with a library path resolves the six entry points and calls two of them:
 *   emission_layout           prints "emission <size> object <off> emitter <off> flags <off> pad <off> orbit <off> T_in <off> p <off>
 *                             gain <off> theta <off> weight <off>"
 *   emission_layout <lib>     … exits 2 when one of the entry points does not resolve; otherwise calls rtgr_trace_emission_f64 (a 2 x 2
 *                             Kerr-Schild canvas with one emitting disk) and rtgr_eval_disk_emission_f64 (one pair of states) and prints
 *                             "trace <code> eval <code> touched <0|1>" (touched: one of the caller's output arrays no longer holds what
 *                             the caller put there)
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_disk_emission) == 96, "rtgr_disk_emission");
_Static_assert(offsetof(rtgr_disk_emission, object) == 0 && offsetof(rtgr_disk_emission, emitter) == 4 && offsetof(rtgr_disk_emission, flags) == 8 &&
               offsetof(rtgr_disk_emission, pad) == 12 && offsetof(rtgr_disk_emission, orbit) == 16 && offsetof(rtgr_disk_emission, T_in) == 24 &&
               offsetof(rtgr_disk_emission, p) == 32 && offsetof(rtgr_disk_emission, gain) == 40 && offsetof(rtgr_disk_emission, theta) == 48 &&
               offsetof(rtgr_disk_emission, weight) == 72, "rtgr_disk_emission fields");
_Static_assert(RTGR_EMIT_KEPLER == 0 && RTGR_EMIT_RIGID == 1 && RTGR_EMIT_INNER_EDGE == 1u, "constants");

typedef int (*emission_f64_fn)(rtgr_context*, const rtgr_scene*, const rtgr_solver*, const rtgr_camera*, uint64_t, uint64_t, const rtgr_shade*,
                               const rtgr_disk_emission*, const rtgr_aa*, double*, const rtgr_ray_outputs*, double*, uint8_t*, rtgr_counters*,
                               rtgr_aa_stats*);
typedef int (*eval_f64_fn)(rtgr_context*, const rtgr_scene*, const rtgr_disk_emission*, const double*, const double*, uint64_t, double*, double*,
                           double*, double*);
typedef int (*defaults_fn)(rtgr_solver*, int);

int main(int argc, char** argv) {
    printf("emission %zu object %zu emitter %zu flags %zu pad %zu orbit %zu T_in %zu p %zu gain %zu theta %zu weight %zu\n", sizeof(rtgr_disk_emission),
           offsetof(rtgr_disk_emission, object), offsetof(rtgr_disk_emission, emitter), offsetof(rtgr_disk_emission, flags),
           offsetof(rtgr_disk_emission, pad), offsetof(rtgr_disk_emission, orbit), offsetof(rtgr_disk_emission, T_in), offsetof(rtgr_disk_emission, p),
           offsetof(rtgr_disk_emission, gain), offsetof(rtgr_disk_emission, theta), offsetof(rtgr_disk_emission, weight));
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        emission_f64_fn trace = (emission_f64_fn)dlsym(h, "rtgr_trace_emission_f64");
        eval_f64_fn eval = (eval_f64_fn)dlsym(h, "rtgr_eval_disk_emission_f64");
        defaults_fn defaults = (defaults_fn)dlsym(h, "rtgr_solver_defaults");
        if (!trace || !eval || !defaults || !dlsym(h, "rtgr_trace_emission_f32") || !dlsym(h, "rtgr_trace_emission_device_f64") ||
            !dlsym(h, "rtgr_trace_emission_device_f32") || !dlsym(h, "rtgr_eval_disk_emission_f32"))
            return 2;
        rtgr_scene sc;
        memset(&sc, 0, sizeof sc);
        sc.metric = RTGR_KS_TRUE;
        sc.M = 1.0;
        sc.a = 0.5;
        sc.nobj = 1;
        sc.obj[0].kind = RTGR_DISK;
        sc.obj[0].p[0] = 0.05;
        sc.obj[0].p[1] = 3.0;
        sc.obj[0].p[2] = 6.0;
        rtgr_solver opt;
        if (defaults(&opt, 0) != 0) return 3;
        rtgr_camera cam = {{0, 8, -2, 1}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}};
        rtgr_disk_emission em = {1, RTGR_EMIT_KEPLER, 0, 0, 1.0, 6000.0, 0.75, 1.0, {20554.0, 26346.0, 33014.0}, {0.29, 1.0, 3.09}};
        double rgb[12], g[4], one[9];
        for (int q = 0; q < 12; q++) rgb[q] = -7.0;
        for (int q = 0; q < 4; q++) g[q] = -7.0;
        for (int q = 0; q < 9; q++) one[q] = -7.0;
        const int rc_trace = trace(NULL, &sc, &opt, &cam, 2, 2, NULL, &em, NULL, rgb, NULL, g, NULL, NULL, NULL);
        const double s0[8] = {0, 8, -2, 1, -1, 0, 1, 0}, se[8] = {0, 4, 0, 0.05, -1, 0, 1, 0};
        const int rc_eval = eval(NULL, &sc, &em, s0, se, 1, one, one + 1, one + 5, one + 6);
        int touched = 0;
        for (int q = 0; q < 12; q++) touched |= rgb[q] != -7.0;
        for (int q = 0; q < 4; q++) touched |= g[q] != -7.0;
        for (int q = 0; q < 9; q++) touched |= one[q] != -7.0;
        printf("trace %d eval %d touched %d\n", rc_trace, rc_eval, touched);
    }
    return 0;
}
