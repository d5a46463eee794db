// rtgr_polarization_host.hip — polarized disk images (include/rtgr.h "polarized disk images"): the checks of an rtgr_polarization, the
// stage alone, the polarized observer trace — rtgr_observer_host.hip's trace with the polarization kernel behind each batch's emission
// kernel — and the two hooks.  Host code only: the kernel is rtgr_polarize.hip's, the model rtgr_polarization.hpp's.
#include "rtgr_internal.hpp"

namespace rtgr {

constexpr EntryWords POLARIZATION_WORDS = {"rtgr_polarization_device_*", "polarization", false};
constexpr const char* POLARIZATION_CANVAS = "a polarized frame";
constexpr const char* POLARIZATION_NEEDS_STATIONARY = "polarization in a time-dependent (4-D) grid metric is not supported";

// the caller's record, checked against its scene, into the record the kernel reads, for scalar type R
template <class R>
static int polarization_resolve(const rtgr_scene* scene, const rtgr_polarization* pol, DevPolarization<R>& dp) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!pol) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization is NULL (pol)");
    const uint32_t kind = scene->metric & ~RTGR_METRIC_GENERIC;
    if (kind != RTGR_KS_TRUE && kind != RTGR_MINKOWSKI)
        return fail(RTGR_ERR_BAD_ARG, "polarization needs the Kerr metric with Kerr's own radius: rtgr_scene.metric must be RTGR_KS_TRUE or RTGR_MINKOWSKI "
                                      "(the Walker-Penrose constants do not exist for RTGR_KS_REF, whose radius is not Kerr's, a grid or a user metric)");
    if (pol->kind != RTGR_POL_SCATTER && pol->kind != RTGR_POL_FIELD)
        return fail(RTGR_ERR_BAD_ARG, "unknown rtgr_polarization.kind " + std::to_string(pol->kind) + " (RTGR_POL_SCATTER = 0, RTGR_POL_FIELD = 1)");
    if (pol->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.flags must be 0");
    if (pol->reserved[0] != 0.0 || pol->reserved[1] != 0.0) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.reserved must be 0");
    if (!std::isfinite(pol->deg0) || !std::isfinite(pol->deg1)) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.deg0 and deg1 must be finite");
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(pol->field[c])) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.field must be finite");
    if (pol->deg0 < 0.0) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.deg0 must be >= 0");
    const bool zero_field = pol->field[0] == 0.0 && pol->field[1] == 0.0 && pol->field[2] == 0.0;
    if (pol->kind == RTGR_POL_SCATTER) {
        if (pol->deg1 <= -1.0) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.deg1 of RTGR_POL_SCATTER must be > -1");
        if (!zero_field) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.field of RTGR_POL_SCATTER must be 0");
    } else if (zero_field) {
        return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization.field of RTGR_POL_FIELD must not be zero");
    }
    std::memset(&dp, 0, sizeof dp);
    dp.kind = pol->kind;
    dp.deg0 = (R)pol->deg0; dp.deg1 = (R)pol->deg1;
    for (int c = 0; c < 3; c++) dp.field[c] = (R)pol->field[c];
    return RTGR_OK;
}

// the stage alone on the device that holds d_q: the frame kernel into the stream's scratch, then the polarization kernel
template <class R>
int api::polarization_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol,
                             const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state0, const R* d_state_end, R* d_q,
                             R* d_u, R* d_aux, void* stream) {
    if (!pol) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization is NULL (pol)");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!d_hit32 || !d_state0 || !d_state_end) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization_device_*: hit32, state0 or state_end is NULL");
    if (!d_q || !d_u) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization_device_*: q or u is NULL");
    RESOLVE_DEVICE(d_q);
    if ((rc = canvas_check(ni, nj, POLARIZATION_CANVAS))) return rc;
    PolArgs<R> P;
    std::memset(&P, 0, sizeof P);
    if ((rc = polarization_resolve<R>(scene, pol, P.pol))) return rc;
    if ((rc = emission_resolve<R>(scene, nullptr, emit, P.em))) return rc;
    DevObserver<R> ob;
    if ((rc = observer_resolve<R>(scene, obs, ob))) return rc;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(D->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    bool capturing;
    if ((rc = capture_check(st, POLARIZATION_WORDS, nullptr, &capturing))) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    if ((rc = stationary_scene<R>(*D, scene, P.sc, st, POLARIZATION_NEEDS_STATIONARY))) return rc;
    FrameNeeds need;
    need.obs = true;
    FrameScratch fs;
    if ((rc = frame_scratch(*D, st, capturing, POLARIZATION_WORDS, 0, sizeof(R), need, 0, nullptr, nullptr, fs))) return rc;
    ObsFrame<R>* d_frame = (ObsFrame<R>*)(fs.base + fs.at.obs);
    KernelTimer timer(*D, st, 0);
    if ((rc = observer_frame_launch<R>(P.sc, ob, d_frame, st))) return rc;
    P.q = d_q; P.u = d_u; P.aux = d_aux;
    P.hit32 = d_hit32; P.state0 = d_state0; P.state_end = d_state_end;
    P.n = ni * nj; P.mode = POL_FRAME; P.obs = d_frame;
    return polarize_launch<R>(P, st);
}

// what every traced entry refuses before it touches a device, beyond what the observer trace refuses itself
template <class R>
static int polarized_check(const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol, const rtgr_observer* obs, const void* q,
                           const void* u, PolStage<R>& stage) {
    if (!pol) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization is NULL (pol)");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!q || !u) return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_polarized_*: q or u is NULL");
    return polarization_resolve<R>(scene, pol, stage.pol);
}

template <class R>
int api::trace_polarized_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                                const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_polarization* pol, R* d_rgb, const rtgr_ray_outputs* out,
                                R* d_g, R* d_q, R* d_u, R* d_aux, rtgr_counters* ctr, void* stream) {
    RESOLVE_CONTEXT();
    PolStage<R> stage;
    if ((rc = polarized_check<R>(scene, emit, pol, obs, d_q, d_u, stage))) return rc;
    if (!d_rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    stage.q = d_q; stage.u = d_u; stage.aux = d_aux;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_observer_on<R>(*D, scene, opt, obs, ni, nj, shade, emit, d_rgb, out, d_g, ctr, (hipStream_t)stream, &stage);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream; the frame and the three planes copied out
template <class R>
int api::trace_polarized(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                         const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_polarization* pol, R* rgb, const rtgr_ray_outputs* out, R* g,
                         R* q, R* u, R* aux, rtgr_counters* ctr) {
    RESOLVE_CONTEXT();
    PolStage<R> stage;
    if ((rc = polarized_check<R>(scene, emit, pol, obs, q, u, stage))) return rc;
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if ((rc = canvas_check(ni, nj, POLARIZATION_CANVAS))) return rc;
    const uint64_t n = ni * nj;
    HostMirror m(c);
    stage.q = m.out(q, n); stage.u = m.out(u, n); stage.aux = m.out(aux, n);
    if ((rc = m.status())) return rc;
    return staged_frame<R>(c, n, rgb, out, nullptr, g, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t*, R* d_g, hipStream_t st) {
        int r = trace_observer_on<R>(D, scene, opt, obs, ni, nj, shade, emit, d_rgb, d_out, d_g, ctr, st, &stage);
        return r ? r : m.fetch(st);
    });
}

// the model at n pairs of states under obs, on device 0 of the context (host pointers): the polarization kernel itself, in point mode
template <class R>
int api::eval_polarization(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol,
                           const rtgr_observer* obs, const R* s0, const R* s_end, uint64_t n, R* kappa, R* f_em, R* aux, R* delta, R* q, R* u, int* valid) {
    RESOLVE_CONTEXT();
    if (!pol) return fail(RTGR_ERR_BAD_ARG, "rtgr_polarization is NULL (pol)");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (n && (!s0 || !s_end)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_polarization: NULL argument");
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_polarization: at most 2^32 points per call");
    PolArgs<R> P;
    std::memset(&P, 0, sizeof P);
    if ((rc = polarization_resolve<R>(scene, pol, P.pol))) return rc;
    if ((rc = emission_resolve<R>(scene, nullptr, emit, P.em))) return rc;
    DevObserver<R> ob;
    if ((rc = observer_resolve<R>(scene, obs, ob))) return rc;
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    if ((rc = stationary_scene<R>(D, scene, P.sc, nullptr, POLARIZATION_NEEDS_STATIONARY))) return rc;
    if (n == 0) return RTGR_OK;
    P.state0 = m.in(s0, (size_t)n * 8); P.state_end = m.in(s_end, (size_t)n * 8);
    ObsFrame<R>* d_frame = m.scratch<ObsFrame<R>>(1);
    P.kappa = m.out(kappa, (size_t)n * 2); P.f_em = m.out(f_em, (size_t)n * 4); P.aux = m.out(aux, n); P.delta = m.out(delta, n);
    P.q = m.out(q, n); P.u = m.out(u, n); P.valid = m.out(valid, n);
    if ((rc = m.status())) return rc;
    if ((rc = observer_frame_launch<R>(P.sc, ob, d_frame, nullptr))) return rc;
    P.n = n; P.mode = POL_POINTS; P.obs = d_frame;
    if ((rc = polarize_launch<R>(P, nullptr))) return rc;
    return m.fetch();
}

// (Y(k, f), h(k, f)) at n states and vectors: the kernel's own forms
template <class R>
int api::eval_walker_penrose(rtgr_context* ctx, const rtgr_scene* scene, const R* s, const R* f, uint64_t n, R* kappa) {
    RESOLVE_CONTEXT();
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (n && (!s || !f || !kappa)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_walker_penrose: NULL argument");
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_walker_penrose: at most 2^32 points per call");
    const uint32_t kind = scene->metric & ~RTGR_METRIC_GENERIC;
    if (kind != RTGR_KS_TRUE && kind != RTGR_MINKOWSKI)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_walker_penrose: rtgr_scene.metric must be RTGR_KS_TRUE or RTGR_MINKOWSKI (the Walker-Penrose constants "
                                      "do not exist for RTGR_KS_REF, whose radius is not Kerr's, a grid or a user metric)");
    PolArgs<R> P;
    std::memset(&P, 0, sizeof P);
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    if ((rc = stationary_scene<R>(D, scene, P.sc, nullptr, POLARIZATION_NEEDS_STATIONARY))) return rc;
    if (n == 0) return RTGR_OK;
    P.state0 = m.in(s, (size_t)n * 8); P.fvec = m.in(f, (size_t)n * 4); P.kappa = m.out(kappa, (size_t)n * 2);
    if ((rc = m.status())) return rc;
    P.n = n; P.mode = POL_FORMS;
    if ((rc = polarize_launch<R>(P, nullptr))) return rc;
    return m.fetch();
}

RTGR_INSTANTIATE_F64_F32(api::polarization_device);
RTGR_INSTANTIATE_F64_F32(api::trace_polarized_device);
RTGR_INSTANTIATE_F64_F32(api::trace_polarized);
RTGR_INSTANTIATE_F64_F32(api::eval_polarization);
RTGR_INSTANTIATE_F64_F32(api::eval_walker_penrose);

}  // namespace rtgr
