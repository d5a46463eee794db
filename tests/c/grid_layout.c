/* grid_layout.c — a plain C caller of the grid-metric part of include/rtgr.h, compiled with gcc by tests/test_grid_metric.py.
 *
 * Pins the byte layout of rtgr_grid (what julia/RayTraceGRHIP.jl's RtgrGrid and raytracegr.jl_amd/_abi.py's rtgr_grid mirror) as
 * _Static_asserts, and with a library path resolves the two entry points:
 *   grid_layout                prints "grid <size> n <off> pad <off> origin <off> spacing <off> RTGR_GRID <v> RTGR_RAY_OUTSIDE <v>"
 *   grid_layout <lib>          … and exits 2 when rtgr_grid_metric_load / rtgr_grid_metric_unload do not resolve
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_grid) == 64, "rtgr_grid");
_Static_assert(offsetof(rtgr_grid, n) == 0 && offsetof(rtgr_grid, pad) == 12 && offsetof(rtgr_grid, origin) == 16 &&
               offsetof(rtgr_grid, spacing) == 40, "rtgr_grid fields");
_Static_assert(RTGR_GRID == 4 && RTGR_RAY_OUTSIDE == 5, "enum values");

typedef int (*load_fn)(rtgr_context*, const rtgr_grid*, const double*, uint64_t*);
typedef int (*unload_fn)(rtgr_context*, uint64_t);

int main(int argc, char** argv) {
    printf("grid %zu n %zu pad %zu origin %zu spacing %zu RTGR_GRID %d RTGR_RAY_OUTSIDE %d\n", sizeof(rtgr_grid), offsetof(rtgr_grid, n),
           offsetof(rtgr_grid, pad), offsetof(rtgr_grid, origin), offsetof(rtgr_grid, spacing), (int)RTGR_GRID, (int)RTGR_RAY_OUTSIDE);
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        load_fn load = (load_fn)dlsym(h, "rtgr_grid_metric_load");
        unload_fn unload = (unload_fn)dlsym(h, "rtgr_grid_metric_unload");
        if (!load || !unload) return 2;
    }
    return 0;
}
