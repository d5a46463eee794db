// rtgr_lightcurve_host.hip — hot-spot light curves (include/rtgr.h "hot-spot light curves"): the checks of an rtgr_hot_spot, a stream's
// light-curve scratch, the light-curve stage — the seed kernel, the emission kernel in point mode for Omega_s, the reduction — the traced
// light curve (the observer trace of rtgr_observer_host.hip, untouched, then one stage over the whole frame) and the hook.  Host code
// only: the kernels are rtgr_lightcurve.hip's and rtgr_emit.hip's, the model rtgr_lightcurve.hpp's.
#include "rtgr_internal.hpp"

namespace rtgr {

constexpr EntryWords LIGHT_CURVE_WORDS = {"rtgr_light_curve_device_*", "light-curve", true};
constexpr EntryWords TRACE_LIGHT_CURVE_WORDS = {"rtgr_trace_light_curve_*", "light-curve", true};

// the caller's record, checked against the emitting disk of its scene, into what the kernels read
static int spot_resolve(const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, LcSpot& S) {
    if (!spot) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot is NULL (spot)");
    if (spot->nt == 0 || spot->nt > RTGR_HOT_SPOT_MAX_SAMPLES)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.nt = " + std::to_string(spot->nt) + ": need 1 .. 2^20 observer time samples");
    if (spot->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.flags must be 0");
    if (spot->pad != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.pad must be 0");
    if (!(spot->sigma > 0.0) || !std::isfinite(spot->sigma)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.sigma must be > 0 and finite");
    if (!(spot->cut > 0.0) || !std::isfinite(spot->cut)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.cut must be > 0 and finite");
    if (!(spot->amp >= 0.0) || !std::isfinite(spot->amp)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.amp must be >= 0 and finite");
    if (!std::isfinite(spot->rho_s)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.rho_s must be finite");
    if (!std::isfinite(spot->phi0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.phi0 must be finite");
    if (!std::isfinite(spot->g_power)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.g_power must be finite");
    if (!std::isfinite(spot->t_start)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.t_start must be finite");
    if (!std::isfinite(spot->dt)) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.dt must be finite");
    const rtgr_object& o = scene_objects(scene)[emit->object - 1];   // (a Disk: emission_resolve has checked)
    if (!(spot->rho_s >= o.p[1] && spot->rho_s <= o.p[2]))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot.rho_s = " + std::to_string(spot->rho_s) + " lies outside the emitting Disk's [r_in, r_out] = [" +
                                      std::to_string(o.p[1]) + ", " + std::to_string(o.p[2]) + "]");
    S.rho_s = spot->rho_s; S.phi0 = spot->phi0;
    S.inv_2s2 = 1.0 / (2.0 * spot->sigma * spot->sigma);
    S.cut_sigma = spot->cut * spot->sigma;
    S.r2_cut = S.cut_sigma * S.cut_sigma;
    S.e_cut = std::exp(-0.5 * spot->cut * spot->cut);
    S.amp = spot->amp; S.q = spot->g_power; S.t_start = spot->t_start; S.dt = spot->dt;
    return RTGR_OK;
}

// the pixel weight of `obs` (may be null: w = 1) on an ni x nj canvas, as lc_pixel_weight reads it — shared with the disk spectra
// (rtgr_spectrum_host.hip)
template <class R>
int pixel_weight_resolve(const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, LcWeight& W) {
    W.proj = 0; W.pad = 0; W.hx = W.hy = 0.0; W.scale = 1.0;
    if (obs) {
        int rc;
        DevObserver<R> ob;
        if ((rc = observer_resolve<R>(scene, obs, ob))) return rc;
        if (obs->projection == RTGR_PROJ_PERSPECTIVE) {
            W.proj = 1;
            W.hx = std::tan(0.5 * obs->fov_x); W.hy = std::tan(0.5 * obs->fov_y);
            W.scale = W.hx * W.hy * (2.0 / (double)ni) * (2.0 / (double)nj);
        } else {
            W.proj = 2;
            W.hx = 0.5 * obs->fov_x; W.hy = 0.5 * obs->fov_y;
            W.scale = (obs->fov_x / (double)ni) * (obs->fov_y / (double)nj);
        }
    }
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(pixel_weight_resolve);

// everything a light-curve call resolves before it touches a device: the emitter, the spot, the pixel weight of `obs` (may be null)
template <class R>
struct LcResolved {
    DevEmission<R> em;
    LcSpot S;
    LcWeight W;
};
template <class R>
static int lc_resolve(const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, const rtgr_observer* obs, uint64_t ni,
                      uint64_t nj, LcResolved<R>& L) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!spot) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot is NULL (spot)");
    int rc;
    if ((rc = emission_resolve<R>(scene, nullptr, emit, L.em))) return rc;
    if ((rc = spot_resolve(scene, emit, spot, L.S))) return rc;
    return pixel_weight_resolve<R>(scene, obs, ni, nj, L.W);
}

// The light-curve scratch of a stream: the head, the partial sums of one pass, then `borrow` bytes (the planes a traced light curve
// keeps there).  D.mu held.  Grow-only and retired like the frame scratch; growth is refused while the stream is captured.
static int lc_scratch(DeviceCtx& D, hipStream_t st, bool capturing, const EntryWords& who, uint64_t n, uint64_t nt, size_t borrow, char** base,
                      size_t* off_borrow) {
    int rc;
    StreamState* ss = nullptr;
    if ((rc = stream_state(D, st, &ss))) return rc;
    *off_borrow = LC_HEAD + lc_partial_bytes(n, nt);
    const size_t bytes = *off_borrow + borrow;
    if (capturing && bytes > ss->lc_bytes)
        return fail(RTGR_ERR_BAD_ARG, std::string(who.entry) + ": the stream's " + who.scratch + " scratch must grow but the stream is being captured: make a "
                                      "call of this size on the stream before hipStreamBeginCapture");
    if ((rc = scratch_need(*ss, ss->lc, ss->lc_bytes, bytes))) return rc;
    *base = (char*)ss->lc;
    return RTGR_OK;
}

// Omega_s into the head: the seed kernel, then the emission kernel in point mode on the one pair of states (D.mu held)
template <class R>
static int lc_omega(const DevScene<R>& sc, const DevEmission<R>& em, double rho_s, char* head, hipStream_t st) {
    int rc;
    if ((rc = lc_seed_launch<R>((R)rho_s, head, st))) return rc;
    EmitArgs<R> E;
    std::memset(&E, 0, sizeof E);
    E.omega = (R*)(head + LC_HEAD_OMEGA);
    E.state_end = (const R*)(head + LC_HEAD_SE); E.state0 = (const R*)(head + LC_HEAD_S0);
    E.obs = (const ObsFrame<R>*)(head + LC_HEAD_FRAME);
    E.n = 1; E.plane_stride = 1; E.pixel_stride = 3;
    E.sc = sc; E.em = em;
    return emit_launch<R>(E, st);
}

// the stage on device D, stream st, over planes of that device; `head` / `partial`: the stream's scratch
template <class R>
static int lc_stage(DeviceCtx& D, const DevScene<R>& sc, const LcResolved<R>& L, uint64_t ni, uint64_t nj, uint64_t nt, const uint32_t* d_hit32,
                    const R* d_state_end, const R* d_g, char* base, double* d_lc, hipStream_t st) {
    int rc;
    std::lock_guard<std::mutex> lk(D.mu);
    KernelTimer timer(D, st, 0);
    if ((rc = lc_omega<R>(sc, L.em, L.S.rho_s, base, st))) return rc;
    LcPlanes<R> P;
    P.hit32 = d_hit32; P.state_end = d_state_end; P.g = d_g;
    P.n = ni * nj; P.ni = ni; P.nj = nj; P.object = L.em.object; P.pad = 0;
    return lc_reduce_launch<R>(P, L.S, L.W, nt, base, (double*)(base + LC_HEAD), d_lc, st);
}

template <class R>
int api::light_curve_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                            const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state_end, const R* d_g,
                            double* d_lc, void* stream) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (!d_hit32) return fail(RTGR_ERR_BAD_ARG, "rtgr_light_curve_device_*: hit32 is NULL");
    if (!d_state_end) return fail(RTGR_ERR_BAD_ARG, "rtgr_light_curve_device_*: state_end is NULL");
    if (!d_g) return fail(RTGR_ERR_BAD_ARG, "rtgr_light_curve_device_*: g is NULL");
    if (!d_lc) return fail(RTGR_ERR_BAD_ARG, "rtgr_light_curve_device_*: lc is NULL");
    if ((rc = canvas_check(ni, nj, "a light curve"))) return rc;
    LcResolved<R> L;
    if ((rc = lc_resolve<R>(scene, emit, spot, obs, ni, nj, L))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_lc, &D))) return rc;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(D->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    bool capturing;
    if ((rc = capture_check(st, LIGHT_CURVE_WORDS, nullptr, &capturing))) return rc;
    DevScene<R> sc;
    char* base = nullptr;
    size_t off_borrow = 0;
    {
        std::lock_guard<std::mutex> lk(D->mu);
        if ((rc = stationary_scene<R>(*D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
        if ((rc = lc_scratch(*D, st, capturing, LIGHT_CURVE_WORDS, ni * nj, spot->nt, 0, &base, &off_borrow))) return rc;
    }
    return lc_stage<R>(*D, sc, L, ni, nj, spot->nt, d_hit32, d_state_end, d_g, base, d_lc, st);
}

// the traced light curve on device D, stream st: rtgr_trace_observer_device_* with the planes the stage reads borrowed from the stream's
// light-curve scratch where the caller gave none, then the stage
template <class R>
static int trace_light_curve_on(rtgr_context* c, DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, R* d_rgb,
                                const rtgr_ray_outputs* out, R* d_g, double* d_lc, rtgr_counters* ctr, hipStream_t st) {
    int rc;
    LcResolved<R> L;
    if ((rc = lc_resolve<R>(scene, emit, spot, obs, ni, nj, L))) return rc;
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if ((rc = canvas_check(ni, nj, "an observer frame"))) return rc;
    const uint64_t n = ni * nj;
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    bool capturing;
    if ((rc = capture_check(st, TRACE_LIGHT_CURVE_WORDS, ctr, &capturing))) return rc;
    rtgr_ray_outputs o2;
    if (out) o2 = *out; else std::memset(&o2, 0, sizeof o2);
    const size_t b_state = o2.state_end ? 0 : align256((size_t)n * 8 * sizeof(R)), b_hit = o2.hit32 ? 0 : align256((size_t)n * sizeof(uint32_t)),
                 b_g = d_g ? 0 : align256((size_t)n * sizeof(R));
    DevScene<R> sc;
    char* base = nullptr;
    size_t at = 0;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if ((rc = stationary_scene<R>(D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
        if ((rc = lc_scratch(D, st, capturing, TRACE_LIGHT_CURVE_WORDS, n, spot->nt, b_state + b_hit + b_g, &base, &at))) return rc;
    }
    if (!o2.state_end) { o2.state_end = base + at; at += b_state; }
    if (!o2.hit32) { o2.hit32 = (uint32_t*)(base + at); at += b_hit; }
    R* g2 = d_g ? d_g : (R*)(base + at);
    if ((rc = api::trace_observer_device<R>(c, scene, opt, obs, ni, nj, shade, emit, d_rgb, &o2, g2, ctr, (void*)st))) return rc;
    return lc_stage<R>(D, sc, L, ni, nj, spot->nt, o2.hit32, (const R*)o2.state_end, g2, base, d_lc, st);
}

static int trace_light_curve_check(const rtgr_scene* scene, const rtgr_observer* obs, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                                   const void* rgb, const void* lc) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!spot) return fail(RTGR_ERR_BAD_ARG, "rtgr_hot_spot is NULL (spot)");
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if (!lc) return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_light_curve_*: lc is NULL");
    return RTGR_OK;
}

template <class R>
int api::trace_light_curve_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                                  const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, R* d_rgb,
                                  const rtgr_ray_outputs* out, R* d_g, double* d_lc, rtgr_counters* ctr, void* stream) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if ((rc = trace_light_curve_check(scene, obs, emit, spot, d_rgb, d_lc))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_light_curve_on<R>(c, *D, scene, opt, obs, ni, nj, shade, emit, spot, d_rgb, out, d_g, d_lc, ctr, (hipStream_t)stream);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream; the frame and the light curve copied out
template <class R>
int api::trace_light_curve(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                           const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, R* rgb, const rtgr_ray_outputs* out, R* g,
                           double* lc, rtgr_counters* ctr) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if ((rc = trace_light_curve_check(scene, obs, emit, spot, rgb, lc))) return rc;
    if ((rc = canvas_check(ni, nj, "an observer frame"))) return rc;
    {
        LcResolved<R> L;   // (every refusal before anything is allocated or written)
        if ((rc = lc_resolve<R>(scene, emit, spot, obs, ni, nj, L))) return rc;
    }
    const size_t lc_bytes = (size_t)spot->nt * 3 * sizeof(double);
    DeviceGuard guard(c->devs[0]->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    DevBuf d_lc;
    if ((rc = d_lc.alloc(lc_bytes))) return rc;
    rc = staged_frame<R>(c, ni * nj, rgb, out, nullptr, g, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t*, R* d_g, hipStream_t st) {
        return trace_light_curve_on<R>(c, D, scene, opt, obs, ni, nj, shade, emit, spot, d_rgb, d_out, d_g, (double*)d_lc.p, ctr, st);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(lc, d_lc.p, lc_bytes, hipMemcpyDeviceToHost));   // (staged_frame has synchronised its stream)
    return RTGR_OK;
}

// the hook, on device 0 of the context (host pointers, blocking): the stage's own Omega_s, and the point kernel
template <class R>
int api::eval_hot_spot(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, const R* xyt, uint64_t n,
                       R* omega_s, int* valid, double* j) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (n && (!xyt || !j)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_hot_spot: NULL argument");
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_hot_spot: at most 2^32 points per call");
    LcResolved<R> L;
    if ((rc = lc_resolve<R>(scene, emit, spot, nullptr, 1, 1, L))) return rc;
    DeviceCtx& D = *c->devs[0];
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    if ((rc = stationary_scene<R>(D, scene, sc, nullptr, EMISSION_NEEDS_STATIONARY))) return rc;
    DevBuf head, d_xyt, d_j;
    if ((rc = head.alloc(LC_HEAD)) || (rc = d_xyt.alloc((size_t)n * 3 * sizeof(R))) || (rc = d_j.alloc((size_t)n * sizeof(double)))) return rc;
    if ((rc = lc_omega<R>(sc, L.em, L.S.rho_s, (char*)head.p, nullptr))) return rc;
    if (n) {
        HIP_TRY(hipMemcpy(d_xyt.p, xyt, (size_t)n * 3 * sizeof(R), hipMemcpyHostToDevice));
        if ((rc = lc_points_launch<R>((const R*)d_xyt.p, n, L.S, (const char*)head.p, (double*)d_j.p, nullptr))) return rc;
    }
    HIP_TRY(hipDeviceSynchronize());
    R om;
    HIP_TRY(hipMemcpy(&om, (char*)head.p + LC_HEAD_OMEGA, sizeof om, hipMemcpyDeviceToHost));
    if (omega_s) *omega_s = om;
    if (valid) *valid = std::isfinite((double)om) ? 1 : 0;
    if (n) HIP_TRY(hipMemcpy(j, d_j.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(api::light_curve_device);
RTGR_INSTANTIATE_F64_F32(api::trace_light_curve_device);
RTGR_INSTANTIATE_F64_F32(api::trace_light_curve);
RTGR_INSTANTIATE_F64_F32(api::eval_hot_spot);

}  // namespace rtgr
