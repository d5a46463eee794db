/* grid4_layout.c — a plain C caller of the time-dependent grid part of include/rtgr.h, compiled with gcc by tests/test_grid_metric_4d.py.
 *
 * Pins the byte layout of rtgr_grid4 (what julia/RayTraceGRHIP.jl's RtgrGrid4 and raytracegr.jl_amd/_abi.py's rtgr_grid4 mirror) as
 * _Static_asserts, and with a library path resolves the entry point:
 *   grid4_layout               prints "grid4 <size> n <off> origin <off> spacing <off>"
 *   grid4_layout <lib>         … and exits 2 when rtgr_grid4_metric_load does not resolve
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_grid4) == 80, "rtgr_grid4");
_Static_assert(offsetof(rtgr_grid4, n) == 0 && offsetof(rtgr_grid4, origin) == 16 && offsetof(rtgr_grid4, spacing) == 48, "rtgr_grid4 fields");

typedef int (*load4_fn)(rtgr_context*, const rtgr_grid4*, const double*, uint64_t*);

int main(int argc, char** argv) {
    printf("grid4 %zu n %zu origin %zu spacing %zu\n", sizeof(rtgr_grid4), offsetof(rtgr_grid4, n), offsetof(rtgr_grid4, origin),
           offsetof(rtgr_grid4, spacing));
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        load4_fn load = (load4_fn)dlsym(h, "rtgr_grid4_metric_load");
        if (!load) return 2;
    }
    return 0;
}
