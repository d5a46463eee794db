// rtgr_hooks.hip — the small entry points around the hot path: make_canvas (src/RayTraceGR.jl:457-478), the parity hooks the reference's
// unit tests exercise (metric / dmetric / christoffel / geodesic, test/runtests.jl:12-61; objects and the colour rule), N0f8
// quantisation.  Host side only: the kernels are rtgr_misc.hip's, or the scene's unit's.
#include "rtgr_internal.hpp"

namespace rtgr {

// ---- camera / hooks ------------------------------------------------------------------------------------------------------
template <class R>
int api::make_canvas_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                            uint64_t j0, uint64_t j1, R* d_state0, void* stream) {
    if (!cam || !d_state0) return fail(RTGR_ERR_BAD_ARG, "NULL argument");
    RESOLVE_DEVICE(d_state0);
    if (ni == 0 || nj == 0 || j1 <= j0 || j1 > nj) return fail(RTGR_ERR_BAD_ARG, "bad canvas range");
    DeviceGuard guard(D->dev);
    std::lock_guard<std::mutex> lk(D->mu);
    DevScene<R> sc;
    const UserModule* user = nullptr;
    if ((rc = convert_scene<R>(*D, scene, sc, &user))) return rc;
    DevCamera<R> cm;
    convert_camera<R>(cam, cm);
    const uint64_t n = ni * (j1 - j0);
    if (sc.metric == RTGR_USER) {
        hipFunction_t f = sizeof(R) == 8 ? user->canvas : user->canvas_f32;
        if (!f) return fail(RTGR_ERR_BAD_ARG, "this user-metric code object carries no Float32 kernels");
        HIP_TRY(launch_module(f, (unsigned)((n + 255) / 256), 256, (hipStream_t)stream, sc, cm, ni, nj, j0, (uint64_t)1,
                              (uint64_t)0, n, d_state0));
        return RTGR_OK;
    }
    return misc_canvas<R>(sc, cm, ni, nj, j0, n, d_state0, (hipStream_t)stream);
}
template <class R>
int api::make_canvas(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0,
                     uint64_t j1, R* state0) {
    RESOLVE_CONTEXT();
    if (!state0) return fail(RTGR_ERR_BAD_ARG, "NULL argument");
    if (ni == 0 || nj == 0 || j1 <= j0 || j1 > nj) return fail(RTGR_ERR_BAD_ARG, "bad canvas range");
    const uint64_t n = ni * (j1 - j0);
    HostMirror m(c);   // (D.mu not held: make_canvas_device takes it)
    R* d_state0 = m.out(state0, n * 8);
    if ((rc = m.status())) return rc;
    if ((rc = make_canvas_device<R>(c, scene, cam, ni, nj, j0, j1, d_state0, nullptr))) return rc;
    return m.fetch();
}
RTGR_INSTANTIATE_F64_F32(api::make_canvas_device);
RTGR_INSTANTIATE_F64_F32(api::make_canvas);

template <class R>
int api::eval_metric(rtgr_context* ctx, const rtgr_scene* scene, const R* x, uint64_t n, R* g, R* dg, R* Gam) {
    RESOLVE_CONTEXT();
    if (!x) return fail(RTGR_ERR_BAD_ARG, "x is NULL");
    if (n == 0) return RTGR_OK;
    if (host_has_nan(x, 4 * n)) return fail(RTGR_ERR_NAN_INPUT, "NaN coordinate (AssertionError in the reference, :279)");
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    const UserModule* user = nullptr;
    if ((rc = convert_scene<R>(D, scene, sc, &user))) return rc;
    const R* d_x = m.in(x, n * 4);
    R *d_g = m.out(g, n * 16), *d_dg = m.out(dg, n * 64), *d_Gam = m.out(Gam, n * 64);
    if ((rc = m.status())) return rc;
    if (sc.metric == RTGR_USER) {
        if (sizeof(R) != 8) return fail(RTGR_ERR_BAD_ARG, "user metrics are evaluated in Float64");
        HIP_TRY(launch_module(user->eval_metric, (unsigned)((n + 255) / 256), 256, (hipStream_t) nullptr, sc, d_x, n, d_g, d_dg, d_Gam));
    } else {
        if ((rc = misc_eval_metric<R>(sc, d_x, n, d_g, d_dg, d_Gam, nullptr))) return rc;
    }
    return m.fetch();
}
RTGR_INSTANTIATE_F64_F32(api::eval_metric);

template <class R>
int api::eval_geodesic(rtgr_context* ctx, const rtgr_scene* scene, const R* s, uint64_t n, int path, R* ds) {
    RESOLVE_CONTEXT();
    if (!s || !ds) return fail(RTGR_ERR_BAD_ARG, "NULL argument");
    if (path < 0 || path > 2)
        return fail(RTGR_ERR_BAD_ARG, "path must be 0 (closed contraction, IEEE division), 1 (generic duals) or 2 (the integrate loop's own RHS)");
    if (n == 0) return RTGR_OK;
    if (host_has_nan(s, 8 * n)) return fail(RTGR_ERR_NAN_INPUT, "NaN state (AssertionError in the reference, :279)");
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    const UserModule* user = nullptr;
    if ((rc = convert_scene<R>(D, scene, sc, &user))) return rc;
    const R* d_s = m.in(s, n * 8);
    R* d_ds = m.out(ds, n * 8);
    if ((rc = m.status())) return rc;
    if (sc.metric == RTGR_USER) {  // paths 0 / 1: the reference formulation (4-wide duals through g); path 2: the unit's own loop RHS
        if (sizeof(R) != 8) return fail(RTGR_ERR_BAD_ARG, "user metrics are evaluated in Float64");
        if (path == 2 && !user->eval_accel) return fail(RTGR_ERR_BAD_ARG, "this user-metric code object carries no rtgr_user_eval_accel");
        HIP_TRY(launch_module(path == 2 ? user->eval_accel : user->eval_geodesic, (unsigned)((n + 255) / 256), 256,
                              (hipStream_t) nullptr, sc, d_s, n, d_ds));
    } else {
        if ((rc = misc_eval_geodesic<R>(sc, d_s, n, path, d_ds, nullptr))) return rc;
    }
    return m.fetch();
}
template <class R>
int api::eval_objects(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const R* x, uint64_t n, R* d, R* dmin, uint8_t* hit, R* rgb) {
    RESOLVE_CONTEXT();
    if (!x) return fail(RTGR_ERR_BAD_ARG, "x is NULL");
    if (n == 0) return RTGR_OK;
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    DevSolver<R> so;
    const UserModule* user = nullptr;
    if ((rc = convert_scene<R>(D, scene, sc, &user))) return rc;
    if ((rc = convert_solver<R>(opt, so))) return rc;
    if (hit && sc.nobj > 255u) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_objects: `hit` is a byte per point and the scene has more than 255 objects");
    const size_t nd = (size_t)n * (sc.nobj ? sc.nobj : 1);
    const R* d_x = m.in(x, n * 4);
    R *d_d = m.out(d, nd), *d_dmin = m.out(dmin, n);
    uint8_t* d_hit = m.out(hit, n);
    R* d_rgb = m.out(rgb, n * 3);
    if ((rc = m.status())) return rc;
    if (user && user->has_objects) {   // the scene's unit knows its objects' methods: its kernel
        hipFunction_t f = sizeof(R) == 8 ? user->eval_objects : user->eval_objects_f32;
        if (!f) return fail(RTGR_ERR_BAD_ARG, "this unit carries no rtgr_user_eval_objects kernel (rebuild the unit)");
        HIP_TRY(launch_module(f, (unsigned)((n + 255) / 256), 256, (hipStream_t) nullptr, sc, so, d_x, n, d_d, d_dmin, d_hit, d_rgb));
    } else {
        if ((rc = misc_eval_objects<R>(sc, so, d_x, n, d_d, d_dmin, d_hit, d_rgb, nullptr))) return rc;
    }
    return m.fetch();
}
RTGR_INSTANTIATE_F64_F32(api::eval_geodesic);
RTGR_INSTANTIATE_F64_F32(api::eval_objects);

int api::eval_fastmath_f64(rtgr_context* ctx, const double* x, uint64_t n, double* rcp, double* rsq) {
    RESOLVE_CONTEXT();
    if (!x) return fail(RTGR_ERR_BAD_ARG, "x is NULL");
    if (n == 0) return RTGR_OK;
    HostMirror m(c);
    const double* d_x = m.in(x, n);
    double *d_rcp = m.out(rcp, n), *d_rsq = m.out(rsq, n);
    if ((rc = m.status())) return rc;
    if ((rc = misc_eval_fastmath_f64(d_x, n, d_rcp, d_rsq, nullptr))) return rc;
    return m.fetch();
}

int api::quantize_device_f64(rtgr_context* ctx, const double* d_rgb, uint64_t ni, uint64_t nj, uint8_t* d_img, void* stream) {
    if (!d_rgb || !d_img || ni == 0 || nj == 0) return fail(RTGR_ERR_BAD_ARG, "bad argument");
    RESOLVE_DEVICE(d_rgb);
    DeviceGuard guard(D->dev);
    return misc_quantize(d_rgb, ni, nj, d_img, (hipStream_t)stream);
}

}  // namespace rtgr
