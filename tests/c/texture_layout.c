/* texture_layout.c — a plain C caller of the image-texture part of include/rtgr.h, compiled with gcc by tests/test_textures.py.
 *
 * Pins the byte layout of rtgr_texture_desc, rtgr_texture_bind and rtgr_shade (what julia/RayTraceGRHIP.jl's RtgrTextureDesc /
 * RtgrTextureBind / RtgrShade and raytracegr.jl_amd/_abi.py mirror) as _Static_asserts, and with a library path resolves the eight entry
 * points and calls three of them:
 *   texture_layout           prints "desc <size> width <off> height <off> flags <off> pad <off> bind <size> object <off> filter <off>
 *                            texture <off> shade <size> nbind <off> sflags <off> sbind <off> r_escape <off>"
 *   texture_layout <lib>     … exits 2 when one of the entry points does not resolve; otherwise calls rtgr_texture_load (a 2 x 2 texture),
 *                            rtgr_trace_shaded_f64 (a 2 x 2 Minkowski canvas, no binds) and rtgr_eval_texture_f64 (one point, texture
 *                            id 0) and prints "load <code> id <0|1> shaded <code> eval <code> touched <0|1>" (id: an id was written;
 *                            touched: one of the caller's output arrays no longer holds what the caller put there)
 */
#include <dlfcn.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rtgr.h"

_Static_assert(sizeof(rtgr_texture_desc) == 16, "rtgr_texture_desc");
_Static_assert(offsetof(rtgr_texture_desc, width) == 0 && offsetof(rtgr_texture_desc, height) == 4 && offsetof(rtgr_texture_desc, flags) == 8 &&
               offsetof(rtgr_texture_desc, pad) == 12, "rtgr_texture_desc fields");
_Static_assert(sizeof(rtgr_texture_bind) == 16, "rtgr_texture_bind");
_Static_assert(offsetof(rtgr_texture_bind, object) == 0 && offsetof(rtgr_texture_bind, filter) == 4 && offsetof(rtgr_texture_bind, texture) == 8,
               "rtgr_texture_bind fields");
_Static_assert(sizeof(rtgr_shade) == 24, "rtgr_shade");
_Static_assert(offsetof(rtgr_shade, nbind) == 0 && offsetof(rtgr_shade, flags) == 4 && offsetof(rtgr_shade, bind) == 8 &&
               offsetof(rtgr_shade, r_escape) == 16, "rtgr_shade fields");
_Static_assert(RTGR_MAX_TEXTURE_BINDS == 16 && RTGR_TEX_NEAREST == 0 && RTGR_TEX_BILINEAR == 1, "constants");

typedef int (*load_fn)(rtgr_context*, const rtgr_texture_desc*, const double*, uint64_t*);
typedef int (*shaded_f64_fn)(rtgr_context*, const rtgr_scene*, const rtgr_solver*, const rtgr_camera*, uint64_t, uint64_t, const rtgr_shade*,
                             const rtgr_aa*, double*, const rtgr_ray_outputs*, uint8_t*, rtgr_counters*, rtgr_aa_stats*);
typedef int (*eval_f64_fn)(rtgr_context*, uint64_t, uint32_t, const double*, uint64_t, const double*, double*);
typedef int (*defaults_fn)(rtgr_solver*, int);

int main(int argc, char** argv) {
    printf("desc %zu width %zu height %zu flags %zu pad %zu bind %zu object %zu filter %zu texture %zu shade %zu nbind %zu sflags %zu sbind %zu "
           "r_escape %zu\n",
           sizeof(rtgr_texture_desc), offsetof(rtgr_texture_desc, width), offsetof(rtgr_texture_desc, height), offsetof(rtgr_texture_desc, flags),
           offsetof(rtgr_texture_desc, pad), sizeof(rtgr_texture_bind), offsetof(rtgr_texture_bind, object), offsetof(rtgr_texture_bind, filter),
           offsetof(rtgr_texture_bind, texture), sizeof(rtgr_shade), offsetof(rtgr_shade, nbind), offsetof(rtgr_shade, flags),
           offsetof(rtgr_shade, bind), offsetof(rtgr_shade, r_escape));
    if (argc > 1) {
        void* h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
        if (!h) { fprintf(stderr, "%s\n", dlerror()); return 1; }
        load_fn load = (load_fn)dlsym(h, "rtgr_texture_load");
        shaded_f64_fn shaded = (shaded_f64_fn)dlsym(h, "rtgr_trace_shaded_f64");
        eval_f64_fn eval = (eval_f64_fn)dlsym(h, "rtgr_eval_texture_f64");
        defaults_fn defaults = (defaults_fn)dlsym(h, "rtgr_solver_defaults");
        if (!load || !shaded || !eval || !defaults || !dlsym(h, "rtgr_texture_unload") || !dlsym(h, "rtgr_trace_shaded_f32") ||
            !dlsym(h, "rtgr_trace_shaded_device_f64") || !dlsym(h, "rtgr_trace_shaded_device_f32") || !dlsym(h, "rtgr_eval_texture_f32"))
            return 2;
        rtgr_scene sc;
        memset(&sc, 0, sizeof sc);
        sc.metric = RTGR_MINKOWSKI;
        sc.M = 1.0;
        rtgr_solver opt;
        if (defaults(&opt, 0) != 0) return 3;
        rtgr_camera cam = {{0, 0, -2, 0}, {0, 1, 0, 0}, {0, 0, 0, 1}, {0, 0, 1, 0}};
        rtgr_texture_desc desc = {2, 2, 0, 0};
        double texels[12];
        for (int q = 0; q < 12; q++) texels[q] = q / 12.0;
        uint64_t id = 0;
        const int rc_load = load(NULL, &desc, texels, &id);
        rtgr_shade shade = {0, 0, NULL, 0.0};
        double rgb[12], one[3] = {-7.0, -7.0, -7.0};
        for (int q = 0; q < 12; q++) rgb[q] = -7.0;
        const int rc_shaded = shaded(NULL, &sc, &opt, &cam, 2, 2, &shade, NULL, rgb, NULL, NULL, NULL, NULL);
        const double d[3] = {1.0, 0.0, 0.0};
        const int rc_eval = eval(NULL, 0, RTGR_TEX_NEAREST, d, 1, NULL, one);
        int touched = 0;
        for (int q = 0; q < 12; q++) touched |= rgb[q] != -7.0;
        for (int q = 0; q < 3; q++) touched |= one[q] != -7.0;
        printf("load %d id %d shaded %d eval %d touched %d\n", rc_load, id != 0, rc_shaded, rc_eval, touched);
    }
    return 0;
}
