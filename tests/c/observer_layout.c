/* observer_layout.c — a plain C caller of the observer-camera part of include/rtgr.h, compiled with gcc by tests/test_observer.py.
 *
 * Pins the byte layout of rtgr_observer (what julia/RayTraceGRHIP.jl's RtgrObserver and raytracegr.jl_amd/_abi.py mirror) as
 * _Static_asserts, and with a library path resolves the twelve entry points:
 *   observer_layout           prints "observer <size> pos <off> vel <off> look <off> up <off> fov_x <off> fov_y <off> orbit <off> kind <off>
 *                             projection <off> flags <off> pad <off> max_batch_rays <off>"
 *   observer_layout <lib>     … exits 2 when one of the entry points does not resolve
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_observer) == 176, "rtgr_observer");
_Static_assert(offsetof(rtgr_observer, pos) == 0 && offsetof(rtgr_observer, vel) == 32 && offsetof(rtgr_observer, look) == 64 &&
               offsetof(rtgr_observer, up) == 96 && offsetof(rtgr_observer, fov_x) == 128 && offsetof(rtgr_observer, fov_y) == 136 &&
               offsetof(rtgr_observer, orbit) == 144 && offsetof(rtgr_observer, kind) == 152 && offsetof(rtgr_observer, projection) == 156 &&
               offsetof(rtgr_observer, flags) == 160 && offsetof(rtgr_observer, pad) == 164 && offsetof(rtgr_observer, max_batch_rays) == 168,
               "rtgr_observer fields");
_Static_assert(RTGR_OBS_STATIC == 0 && RTGR_OBS_VELOCITY == 1 && RTGR_OBS_CIRCULAR == 2 && RTGR_PROJ_PERSPECTIVE == 0 && RTGR_PROJ_EQUIRECT == 1,
               "constants");

int main(int argc, char** argv) {
    printf("observer %zu pos %zu vel %zu look %zu up %zu fov_x %zu fov_y %zu orbit %zu kind %zu projection %zu flags %zu pad %zu max_batch_rays %zu\n",
           sizeof(rtgr_observer), offsetof(rtgr_observer, pos), offsetof(rtgr_observer, vel), offsetof(rtgr_observer, look), offsetof(rtgr_observer, up),
           offsetof(rtgr_observer, fov_x), offsetof(rtgr_observer, fov_y), offsetof(rtgr_observer, orbit), offsetof(rtgr_observer, kind),
           offsetof(rtgr_observer, projection), offsetof(rtgr_observer, flags), offsetof(rtgr_observer, pad), offsetof(rtgr_observer, max_batch_rays));
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        static const char* const names[] = {"rtgr_trace_observer_device_f64", "rtgr_trace_observer_device_f32", "rtgr_trace_observer_f64",
                                            "rtgr_trace_observer_f32", "rtgr_make_observer_canvas_device_f64", "rtgr_make_observer_canvas_device_f32",
                                            "rtgr_make_observer_canvas_f64", "rtgr_make_observer_canvas_f32", "rtgr_eval_observer_f64",
                                            "rtgr_eval_observer_f32", "rtgr_eval_disk_emission_observer_f64", "rtgr_eval_disk_emission_observer_f32"};
        for (unsigned k = 0; k < sizeof names / sizeof names[0]; k++)
            if (!dlsym(h, names[k])) { fprintf(stderr, "%s\n", names[k]); return 2; }
    }
    return 0;
}
