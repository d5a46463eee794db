// rtgr_emission_host.hip — disk emission (include/rtgr.h "disk emission"): the checks of an rtgr_disk_emission, the entry points of the
// emitted trace — the camera frame of rtgr_frame_host.hip with an emitting disk — and the pointwise hook.  Host code only: the kernels
// are rtgr_emit.hip's, the model rtgr_emission.hpp's.
#include "rtgr_internal.hpp"

namespace rtgr {

constexpr EntryWords EMISSION_WORDS = {"rtgr_trace_emission_*", "emission", true};

// the caller's parameters into the record the kernels read, for scalar type R; `shade` (may be null): the binds of the same call
template <class R>
int emission_resolve(const rtgr_scene* scene, const rtgr_shade* shade, const rtgr_disk_emission* emit, DevEmission<R>& em) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    int rc;
    if ((rc = builtin_metric_check(scene, "disk emission in", "its kernels live"))) return rc;
    if (scene->nobj > RTGR_OBJECTS_LIMIT || (!scene->objects && scene->nobj > RTGR_MAX_OBJECTS))
        return fail(RTGR_ERR_BAD_ARG, "bad object list: more than RTGR_MAX_OBJECTS objects need rtgr_scene.objects");
    if (emit->object == 0 || emit->object > scene->nobj)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.object = " + std::to_string(emit->object) + " of a list of " + std::to_string(scene->nobj) +
                                      " (1-based index of a Disk)");
    const rtgr_object& o = scene_objects(scene)[emit->object - 1];
    if (o.kind != RTGR_DISK)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.object " + std::to_string(emit->object) + " is a " +
                                      (o.kind == RTGR_PLANE ? "Plane" : o.kind == RTGR_SPHERE ? "Sphere" : o.kind == RTGR_USER_OBJECT ? "user object" : "unknown kind") +
                                      ": only a Disk emits");
    if (shade)
        for (uint32_t k = 0; k < shade->nbind && shade->bind; k++)
            if (shade->bind[k].object == emit->object)
                return fail(RTGR_ERR_BAD_ARG, "object " + std::to_string(emit->object) + " is bound to a texture (rtgr_shade.bind[" + std::to_string(k) +
                                              "]) and emits: a disk takes one or the other");
    if (emit->emitter != RTGR_EMIT_KEPLER && emit->emitter != RTGR_EMIT_RIGID)
        return fail(RTGR_ERR_BAD_ARG, "unknown emitter " + std::to_string(emit->emitter) + " (RTGR_EMIT_KEPLER = 0, RTGR_EMIT_RIGID = 1)");
    if (emit->flags & ~RTGR_EMIT_INNER_EDGE) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.flags: unknown bits (0 or RTGR_EMIT_INNER_EDGE)");
    if (emit->pad != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.pad must be 0");
    if (!std::isfinite(emit->orbit)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.orbit must be finite");
    if (emit->emitter == RTGR_EMIT_KEPLER && emit->orbit != 1.0 && emit->orbit != -1.0)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.orbit of RTGR_EMIT_KEPLER names a root: +1 (Omega_+) or -1 (Omega_-)");
    if (!(emit->T_in > 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.T_in must be > 0 (and not NaN)");
    if (!(emit->gain > 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.gain must be > 0 (and not NaN)");
    if (!std::isfinite(emit->p)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.p must be finite");
    for (int c = 0; c < 3; c++) {
        if (!(emit->theta[c] > 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.theta[" + std::to_string(c) + "] must be > 0 (and not NaN)");
        if (!(emit->weight[c] >= 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission.weight[" + std::to_string(c) + "] must be >= 0 (and not NaN)");
    }
    std::memset(&em, 0, sizeof em);
    em.object = emit->object; em.emitter = emit->emitter; em.flags = emit->flags;
    em.orbit = (R)emit->orbit; em.T_in = (R)emit->T_in; em.p = (R)emit->p; em.gain = (R)emit->gain;
    em.r_in = (R)o.p[1];
    for (int c = 0; c < 3; c++) { em.theta[c] = (R)emit->theta[c]; em.weight[c] = (R)emit->weight[c]; }
    return RTGR_OK;
}

template <class R>
int api::trace_emission_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                               const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out,
                               R* d_g, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream) {
    RESOLVE_CONTEXT();
    if (!d_rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if ((rc = shaded_check(cam, aa, d_refined, stats, ni, nj))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_camera_frame_on<R>(*D, scene, opt, cam, ni, nj, shade, emit, aa, d_rgb, out, d_g, d_refined, ctr, stats, (hipStream_t)stream, EMISSION_WORDS);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream, and the frame copied out
template <class R>
int api::trace_emission(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                        const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_aa* aa, R* rgb, const rtgr_ray_outputs* out, R* g,
                        uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats) {
    RESOLVE_CONTEXT();
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if ((rc = shaded_check(cam, aa, refined, stats, ni, nj))) return rc;
    if ((rc = check_redshift_outputs(out))) return rc;
    return staged_frame<R>(c, ni * nj, rgb, out, refined, g, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t* d_refined, R* d_g, hipStream_t st) {
        return trace_camera_frame_on<R>(D, scene, opt, cam, ni, nj, shade, emit, aa, d_rgb, d_out, d_g, d_refined, ctr, stats, st, EMISSION_WORDS);
    });
}

// the model at n pairs of states, on device 0 of the context (host pointers): the emission kernel itself, in point mode.  obs (may be
// null): u_obs is the e_0 of that observer camera's frame (rtgr_observer_host.hip), built by the frame kernel ahead of the points
template <class R>
int api::eval_disk_emission_observer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_observer* obs, const R* s0,
                                     const R* s_end, uint64_t n, R* omega, R* u_emit, R* g, R* rgb) {
    RESOLVE_CONTEXT();
    if (n && (!s0 || !s_end)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_disk_emission: NULL argument");
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_disk_emission: at most 2^32 points per call");
    EmitArgs<R> E;
    std::memset(&E, 0, sizeof E);
    if ((rc = emission_resolve<R>(scene, nullptr, emit, E.em))) return rc;
    DevObserver<R> ob;
    if (obs && (rc = observer_resolve<R>(scene, obs, ob))) return rc;
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    if ((rc = stationary_scene<R>(D, scene, E.sc, nullptr, EMISSION_NEEDS_STATIONARY))) return rc;
    if (n == 0) return RTGR_OK;
    // the emission kernel in point mode: no hit map, the start states given, n x 3 colours
    E.state0 = m.in(s0, (size_t)n * 8); E.state_end = m.in(s_end, (size_t)n * 8);
    ObsFrame<R>* d_frame = obs ? m.scratch<ObsFrame<R>>(1) : nullptr;
    E.omega = m.out(omega, n); E.u_emit = m.out(u_emit, (size_t)n * 4); E.g = m.out(g, n); E.rgb = m.out(rgb, (size_t)n * 3);
    if ((rc = m.status())) return rc;
    if (obs && (rc = observer_frame_launch<R>(E.sc, ob, d_frame, nullptr))) return rc;
    E.obs = d_frame;
    E.n = n; E.plane_stride = 1; E.pixel_stride = 3;
    if ((rc = emit_launch<R>(E, nullptr))) return rc;
    return m.fetch();
}

RTGR_INSTANTIATE_F64_F32(api::trace_emission_device);
RTGR_INSTANTIATE_F64_F32(api::trace_emission);
template <class R>
int api::eval_disk_emission(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const R* s0, const R* s_end, uint64_t n,
                            R* omega, R* u_emit, R* g, R* rgb) {
    return eval_disk_emission_observer<R>(ctx, scene, emit, nullptr, s0, s_end, n, omega, u_emit, g, rgb);
}
RTGR_INSTANTIATE_F64_F32(emission_resolve);
RTGR_INSTANTIATE_F64_F32(api::eval_disk_emission_observer);
RTGR_INSTANTIATE_F64_F32(api::eval_disk_emission);

}  // namespace rtgr
