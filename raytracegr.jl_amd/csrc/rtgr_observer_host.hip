// rtgr_observer_host.hip — the observer camera (include/rtgr.h "observer camera"): the checks of an rtgr_observer, the observer trace —
// the frame kernel, then batch by batch the ray kernel, a plain trace_device of those states into a window of the caller's planes, the
// post-trace stage of rtgr_frame_host.hip (the shading kernel if textures are bound, the emission kernel if a disk emits) — and the hooks.
// Host code only: the kernels are rtgr_observer.hip's, rtgr_shade.hip's and rtgr_emit.hip's, the frame's model rtgr_observer.hpp's.
#include "rtgr_internal.hpp"

namespace rtgr {

constexpr uint64_t OBS_DEFAULT_BATCH = 1ull << 22;   // rays per batch (rtgr_observer.max_batch_rays = 0), as rtgr_aa's
constexpr EntryWords OBSERVER_WORDS = {"rtgr_trace_observer_*", "observer", true};
constexpr EntryWords POLARIZED_WORDS = {"rtgr_trace_polarized_*", "observer", true};
constexpr EntryWords TRANSFER_WORDS = {"rtgr_trace_transfer_*", "observer", true};
constexpr EntryWords OBSERVER_CANVAS_WORDS = {"rtgr_make_observer_canvas_device_*", "observer", false};
constexpr const char* OBSERVER_CANVAS = "an observer frame";
// (its metric must not depend on time through a 4-D grid: stationary_scene)
constexpr const char* OBSERVER_NEEDS_STATIONARY = "an observer camera in a time-dependent (4-D) grid metric is not supported";
constexpr double OBS_PI = 3.14159265358979323846;

static bool finite4(const double v[4]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]) && std::isfinite(v[3]); }

// the caller's record, checked against its scene, into the record the frame kernel reads, for scalar type R
template <class R>
int observer_resolve(const rtgr_scene* scene, const rtgr_observer* obs, DevObserver<R>& ob) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    int rc;
    if ((rc = builtin_metric_check(scene, "an observer camera in", "its kernels live"))) return rc;
    if (obs->kind != RTGR_OBS_STATIC && obs->kind != RTGR_OBS_VELOCITY && obs->kind != RTGR_OBS_CIRCULAR)
        return fail(RTGR_ERR_BAD_ARG, "unknown rtgr_observer.kind " + std::to_string(obs->kind) + " (RTGR_OBS_STATIC = 0, RTGR_OBS_VELOCITY = 1, RTGR_OBS_CIRCULAR = 2)");
    if (obs->projection != RTGR_PROJ_PERSPECTIVE && obs->projection != RTGR_PROJ_EQUIRECT)
        return fail(RTGR_ERR_BAD_ARG, "unknown rtgr_observer.projection " + std::to_string(obs->projection) + " (RTGR_PROJ_PERSPECTIVE = 0, RTGR_PROJ_EQUIRECT = 1)");
    if (obs->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.flags must be 0");
    if (obs->pad != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.pad must be 0");
    if (!finite4(obs->pos)) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.pos must be finite");
    if (!finite4(obs->look)) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.look must be finite");
    if (!finite4(obs->up)) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.up must be finite");
    if (obs->kind == RTGR_OBS_VELOCITY && !finite4(obs->vel)) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.vel of RTGR_OBS_VELOCITY must be finite");
    if (!std::isfinite(obs->fov_x) || !std::isfinite(obs->fov_y)) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.fov_x and fov_y must be finite");
    if (obs->projection == RTGR_PROJ_PERSPECTIVE) {
        if (!(obs->fov_x > 0.0 && obs->fov_x < OBS_PI && obs->fov_y > 0.0 && obs->fov_y < OBS_PI))
            return fail(RTGR_ERR_BAD_ARG, "rtgr_observer: fov_x and fov_y of RTGR_PROJ_PERSPECTIVE must lie in (0, pi) radians");
    } else if (!(obs->fov_x > 0.0 && obs->fov_x <= 2.0 * OBS_PI && obs->fov_y > 0.0 && obs->fov_y <= OBS_PI)) {
        return fail(RTGR_ERR_BAD_ARG, "rtgr_observer: RTGR_PROJ_EQUIRECT needs 0 < fov_x <= 2 pi and 0 < fov_y <= pi radians");
    }
    if (obs->kind == RTGR_OBS_CIRCULAR) {
        if (!std::isfinite(obs->orbit)) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.orbit must be finite");
        if (obs->orbit != 1.0 && obs->orbit != -1.0)
            return fail(RTGR_ERR_BAD_ARG, "rtgr_observer.orbit of RTGR_OBS_CIRCULAR names a root: +1 (Omega_+) or -1 (Omega_-)");
        if (obs->pos[3] != 0.0) return fail(RTGR_ERR_BAD_ARG, "RTGR_OBS_CIRCULAR: the orbit lies in the equatorial plane, rtgr_observer.pos[3] (z) must be 0");
    }
    std::memset(&ob, 0, sizeof ob);
    for (int c = 0; c < 4; c++) { ob.pos[c] = (R)obs->pos[c]; ob.vel[c] = (R)obs->vel[c]; ob.look[c] = (R)obs->look[c]; ob.up[c] = (R)obs->up[c]; }
    if (obs->kind != RTGR_OBS_VELOCITY) for (int c = 0; c < 4; c++) ob.vel[c] = R(0);
    ob.orbit = obs->kind == RTGR_OBS_CIRCULAR ? (R)obs->orbit : R(0);
    ob.hx = (R)(obs->projection == RTGR_PROJ_PERSPECTIVE ? std::tan(0.5 * obs->fov_x) : 0.5 * obs->fov_x);
    ob.hy = (R)(obs->projection == RTGR_PROJ_PERSPECTIVE ? std::tan(0.5 * obs->fov_y) : 0.5 * obs->fov_y);
    ob.kind = obs->kind; ob.projection = obs->projection;
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(observer_resolve);

// what every entry of the observer trace refuses before it touches a device
static int observer_trace_check(const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_disk_emission* emit,
                                const void* rgb, const rtgr_ray_outputs* out, const void* g) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    int rc;
    if ((rc = canvas_check(ni, nj, OBSERVER_CANVAS))) return rc;
    if (out && out->redshift)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_ray_outputs.redshift is defined against the static observer of make_canvas: an observer trace does not deliver it "
                                      "(the frequency ratio against THIS observer and an orbiting disk is d_g, with emit)");
    if (g && !emit) return fail(RTGR_ERR_BAD_ARG, "g is the frequency ratio of an emitting disk: it must be NULL when emit is NULL");
    return RTGR_OK;
}

// the call on device D, stream st; d_rgb, d_g and the members of `out` are pointers of that device.  pol (may be null): the polarization
// kernel behind the emission kernel of each batch (rtgr_polarization_host.hip, which has checked the record against the scene)
template <class R>
int trace_observer_on(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                      const rtgr_shade* shade, const rtgr_disk_emission* emit, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, rtgr_counters* ctr,
                      hipStream_t st, const PolStage<R>* pol, const TransferStage<R>* xfer) {
    int rc;
    const EntryWords& WORDS = xfer ? TRANSFER_WORDS : pol ? POLARIZED_WORDS : OBSERVER_WORDS;
    if ((rc = observer_trace_check(scene, obs, ni, nj, emit, d_rgb, out, d_g))) return rc;
    DevObserver<R> ob;
    if ((rc = observer_resolve<R>(scene, obs, ob))) return rc;
    DevEmission<R> em;
    if (emit && (rc = emission_resolve<R>(scene, shade, emit, em))) return rc;
    ShadeDesc<R> sd;
    sd.nbind = 0;
    if (shade && (rc = shade_resolve<R>(D, scene, shade, sd))) return rc;
    AfterTrace<R> after;
    after.shade = sd.nbind ? &sd : nullptr;
    after.emit = emit ? &em : nullptr;
    const bool post = after.shade || after.emit;
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    bool capturing;
    if ((rc = capture_check(st, WORDS, ctr, &capturing))) return rc;
    const uint64_t n = ni * nj;
    const uint64_t budget = obs->max_batch_rays ? obs->max_batch_rays : OBS_DEFAULT_BATCH;
    const uint64_t rows = budget / ni ? (budget / ni < nj ? budget / ni : nj) : 1;   // rows per batch
    if (rows < nj && (tl_knobs_override ? tl_knobs_override->tile : D.knobs.tile))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_observer_*: option tile = 1 writes whole frames only and this observer frame takes more than one batch "
                                      "(rtgr_observer.max_batch_rays): raise max_batch_rays to the frame's rays, or use the persistent pipeline (tile = 0)");
    // ---- frame scratch: the counters, the frame record, and what the shading and emission kernels read and the caller did not ask for;
    // batch scratch: the states of `rows` rows --------------------------------------------------------------------------------------------
    FrameNeeds need;
    need.obs = true;
    need.state_end = post && !(out && out->state_end);
    need.hit32 = post && !(out && out->hit32);
    need.status = (after.shade || xfer) && !(out && out->status);
    need.lambda_end = xfer && !(out && out->lambda_end);   // (the transfer kernel integrates each ray as far as the trace went)
    DevScene<R> sc;
    DevSolver<R> ds;
    if (xfer && (rc = convert_solver<R>(opt, ds))) return rc;
    FrameScratch fs;
    unsigned long long* d_tctr = nullptr;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if ((rc = stationary_scene<R>(D, scene, sc, st, emit ? EMISSION_NEEDS_STATIONARY : OBSERVER_NEEDS_STATIONARY))) return rc;
        if ((rc = frame_scratch(D, st, capturing, WORDS, n, sizeof(R), need, align256((size_t)rows * ni * 8 * sizeof(R)), out, ctr, fs))) return rc;
        if (xfer && xfer->tctr) {
            d_tctr = (unsigned long long*)(fs.base + FRAME_HEAD_TCTR);
            HIP_TRY(hipMemsetAsync(d_tctr, 0, sizeof(rtgr_counters), st));
        }
    }
    R* d_states = (R*)fs.ss->batch;
    ObsFrame<R>* d_frame = (ObsFrame<R>*)(fs.base + fs.at.obs);
    const rtgr_ray_outputs& o1 = fs.o1;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        KernelTimer timer(D, st, 0);
        if ((rc = observer_frame_launch<R>(sc, ob, d_frame, st))) return rc;
    }
    // ---- batch by batch: whole rows [ja, jb) --------------------------------------------------------------------------------------
    for (uint64_t ja = 0; ja < nj; ja += rows) {
        const uint64_t jb = ja + rows < nj ? ja + rows : nj, first = ja * ni, m = (jb - ja) * ni;
        {
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = observer_rays_launch<R>(d_frame, ni, nj, first, m, d_states, st))) return rc;
        }
        Window win;
        win.plane_stride = n; win.out_offset = first;
        if ((rc = trace_device<R>(D, scene, opt, d_states, nullptr, ni, nj, ja, jb, d_rgb, &o1, fs.d_ctr, st, 1, 0, rows < nj ? &win : nullptr))) return rc;
        if (post) {   // the batch as a window of the frame: planes n apart; each pixel emitted from its own start state, against this observer's e_0
            TracedPixels<R> px;
            px.rgb = d_rgb + first; px.plane_stride = n; px.g = d_g ? d_g + first : nullptr;
            px.hit32 = o1.hit32 + first; px.status = o1.status ? o1.status + first : nullptr; px.state_end = (const R*)o1.state_end + first * 8;
            px.state0 = d_states; px.obs = d_frame;
            px.n = m; px.ni = ni; px.nj = nj;
            px.sc = &sc;
            if ((rc = after_trace<R>(D, st, after, px))) return rc;
            if (pol) {   // the same window, the same start states: read, not regenerated
                PolArgs<R> P;
                std::memset(&P, 0, sizeof P);
                P.q = pol->q + first; P.u = pol->u + first; P.aux = pol->aux ? pol->aux + first : nullptr;
                P.hit32 = px.hit32; P.state0 = d_states; P.state_end = px.state_end;
                P.n = m; P.mode = POL_FRAME;
                P.sc = sc; P.em = em; P.pol = pol->pol; P.obs = d_frame;
                std::lock_guard<std::mutex> lk(D.mu);
                KernelTimer timer(D, st, 0);
                if ((rc = polarize_launch<R>(P, st))) return rc;
            }
        }
        if (xfer) {   // the same window, the same start states, as far as the trace went: behind every kernel that colours the pixel
            TransferArgs<R> T;
            std::memset(&T, 0, sizeof T);
            T.state0 = d_states; T.lambda_end = (const R*)o1.lambda_end + first; T.status = o1.status + first;
            T.rgb = d_rgb + first; T.plane_stride = n;
            T.I = xfer->I ? xfer->I + first : nullptr; T.tau = xfer->tau ? xfer->tau + first : nullptr;
            T.tstatus = xfer->tstatus ? xfer->tstatus + first : nullptr; T.tsteps = xfer->tsteps ? xfer->tsteps + first : nullptr;
            T.counters = d_tctr; T.obs = d_frame;
            T.ni = ni; T.nrows = jb - ja; T.n = m;
            T.sc = sc; T.opt = ds; T.fl = xfer->fl;
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = transfer_launch<R>(T, st))) return rc;
        }
    }
    // the end of a call that counts — ONE path for the trace's counters and the transfer pass's: both copies, then one wait
    if (ctr) HIP_TRY(hipMemcpyAsync(ctr, fs.d_ctr, sizeof *ctr, hipMemcpyDeviceToHost, st));
    if (d_tctr) HIP_TRY(hipMemcpyAsync(xfer->tctr, d_tctr, sizeof(rtgr_counters), hipMemcpyDeviceToHost, st));
    if (ctr || d_tctr) HIP_TRY(hipStreamSynchronize(st));
    return RTGR_OK;
}

template <class R>
int api::trace_observer_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                               const rtgr_shade* shade, const rtgr_disk_emission* emit, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, rtgr_counters* ctr,
                               void* stream) {
    RESOLVE_CONTEXT();
    if ((rc = observer_trace_check(scene, obs, ni, nj, emit, d_rgb, out, d_g))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_observer_on<R>(*D, scene, opt, obs, ni, nj, shade, emit, d_rgb, out, d_g, ctr, (hipStream_t)stream);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream, and the frame copied out
template <class R>
int api::trace_observer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                        const rtgr_shade* shade, const rtgr_disk_emission* emit, R* rgb, const rtgr_ray_outputs* out, R* g, rtgr_counters* ctr) {
    RESOLVE_CONTEXT();
    if ((rc = observer_trace_check(scene, obs, ni, nj, emit, rgb, out, g))) return rc;
    return staged_frame<R>(c, ni * nj, rgb, out, nullptr, g, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t*, R* d_g, hipStream_t st) {
        return trace_observer_on<R>(D, scene, opt, obs, ni, nj, shade, emit, d_rgb, d_out, d_g, ctr, st);
    });
}

// the states of rows [j0, j1) on device D, stream st: the frame kernel into the stream's scratch, the ray kernel into the caller's array
template <class R>
int api::make_observer_canvas_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, uint64_t j0,
                                     uint64_t j1, R* d_state0, void* stream) {
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!d_state0) return fail(RTGR_ERR_BAD_ARG, "NULL argument");
    RESOLVE_DEVICE(d_state0);
    if ((rc = canvas_check(ni, nj, OBSERVER_CANVAS))) return rc;
    if (j1 <= j0 || j1 > nj) return fail(RTGR_ERR_BAD_ARG, "bad canvas range");
    DevObserver<R> ob;
    if ((rc = observer_resolve<R>(scene, obs, ob))) return rc;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(D->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    bool capturing;
    if ((rc = capture_check(st, OBSERVER_CANVAS_WORDS, nullptr, &capturing))) return rc;
    std::lock_guard<std::mutex> lk(D->mu);
    DevScene<R> sc;
    if ((rc = stationary_scene<R>(*D, scene, sc, st, OBSERVER_NEEDS_STATIONARY))) return rc;
    FrameNeeds need;
    need.obs = true;
    FrameScratch fs;
    if ((rc = frame_scratch(*D, st, capturing, OBSERVER_CANVAS_WORDS, 0, sizeof(R), need, 0, nullptr, nullptr, fs))) return rc;
    ObsFrame<R>* d_frame = (ObsFrame<R>*)(fs.base + fs.at.obs);
    if ((rc = observer_frame_launch<R>(sc, ob, d_frame, st))) return rc;
    return observer_rays_launch<R>(d_frame, ni, nj, j0 * ni, (j1 - j0) * ni, d_state0, st);
}
template <class R>
int api::make_observer_canvas(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1,
                              R* state0) {
    RESOLVE_CONTEXT();
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!state0) return fail(RTGR_ERR_BAD_ARG, "NULL argument");
    if ((rc = canvas_check(ni, nj, OBSERVER_CANVAS))) return rc;
    if (j1 <= j0 || j1 > nj) return fail(RTGR_ERR_BAD_ARG, "bad canvas range");
    const uint64_t n = ni * (j1 - j0);
    HostMirror m(c);   // (D.mu not held: make_observer_canvas_device takes it)
    R* d_state0 = m.out(state0, n * 8);
    if ((rc = m.status())) return rc;
    if ((rc = make_observer_canvas_device<R>(c, scene, obs, ni, nj, j0, j1, d_state0, nullptr))) return rc;
    return m.fetch();
}

// the frame the kernels would use, on device 0 of the context (host pointers, blocking): the frame kernel itself
template <class R>
int api::eval_observer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, R* frame, R* omega, int* valid) {
    RESOLVE_CONTEXT();
    DevObserver<R> ob;
    if ((rc = observer_resolve<R>(scene, obs, ob))) return rc;
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    if ((rc = stationary_scene<R>(D, scene, sc, nullptr, OBSERVER_NEEDS_STATIONARY))) return rc;
    ObsFrame<R> F;
    ObsFrame<R>* d_frame = m.out(&F, 1);
    if ((rc = m.status())) return rc;
    if ((rc = observer_frame_launch<R>(sc, ob, d_frame, nullptr))) return rc;
    if ((rc = m.fetch())) return rc;
    if (frame) std::memcpy(frame, F.e, sizeof F.e);
    if (omega) *omega = F.omega;
    if (valid) *valid = F.valid ? 1 : 0;
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(trace_observer_on);
RTGR_INSTANTIATE_F64_F32(api::trace_observer_device);
RTGR_INSTANTIATE_F64_F32(api::trace_observer);
RTGR_INSTANTIATE_F64_F32(api::make_observer_canvas_device);
RTGR_INSTANTIATE_F64_F32(api::make_observer_canvas);
RTGR_INSTANTIATE_F64_F32(api::eval_observer);

}  // namespace rtgr
