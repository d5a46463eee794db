// rtgr_lightcurve_host.hip — hot-spot light curves (include/rtgr.h "hot-spot light curves"): the checks of an rtgr_hot_spot, the
// light-curve stage — the seed kernel, the emission kernel in point mode for Omega_s, the reduction —, the entry points as a Reduction
// each (the path from a traced frame to the table: rtgr_reduce_host.hip) and the hook.  Host code only: the kernels are
// rtgr_lightcurve.hip's and rtgr_emit.hip's, the model rtgr_lightcurve.hpp's.
#include "rtgr_internal.hpp"
#include "rtgr_reduce.hpp"

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

// everything a light-curve call resolves before it touches a device: the emitter, the spot, the pixel weight of `obs` (may be null)
template <class R>
struct LcResolved {
    DevEmission<R> em;
    LcSpot S;
    PixelWeight W;
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

// A light-curve call as a Reduction (rtgr_internal.hpp; the bodies: rtgr_reduce_host.hip).  `L`: the caller's, filled by the resolve step
// and read by the stage — Omega_s into the scratch's head, then the reduction over the observer times behind it
template <class R>
static Reduction<R> lc_reduction(const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, const rtgr_observer* obs,
                                 LcResolved<R>& L) {
    Reduction<R> red;
    red.device = LIGHT_CURVE_WORDS; red.traced = TRACE_LIGHT_CURVE_WORDS;
    red.canvas = "a light curve"; red.out_name = "lc";
    red.record = spot; red.record_null = "rtgr_hot_spot is NULL (spot)";
    red.head_bytes = LC_HEAD;
    red.rows = spot ? spot->nt : 0;
    red.resolve = [=, &L](uint64_t ni, uint64_t nj) { return lc_resolve<R>(scene, emit, spot, obs, ni, nj, L); };
    red.stage = [&L, nt = red.rows](DeviceCtx&, const DevScene<R>& sc, const ReducePlanes<R>& P, char* base, double* d_lc, hipStream_t st) {
        int rc;
        if ((rc = lc_omega<R>(sc, L.em, L.S.rho_s, base, st))) return rc;
        return lc_reduce_launch<R>(P, L.S, L.W, nt, base, (double*)(base + LC_HEAD), d_lc, st);
    };
    return red;
}

template <class R>
int api::light_curve_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                            const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state_end, const R* d_g,
                            double* d_lc, void* stream) {
    LcResolved<R> L;
    return reduce_device<R>(ctx, lc_reduction<R>(scene, emit, spot, obs, L), scene, emit, ni, nj, d_hit32, d_state_end, d_g, d_lc, stream);
}

template <class R>
int api::trace_light_curve_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                                  const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, R* d_rgb,
                                  const rtgr_ray_outputs* out, R* d_g, double* d_lc, rtgr_counters* ctr, void* stream) {
    LcResolved<R> L;
    return trace_reduce_device<R>(ctx, lc_reduction<R>(scene, emit, spot, obs, L), scene, opt, obs, ni, nj, shade, emit, d_rgb, out, d_g, d_lc, ctr, stream);
}

template <class R>
int api::trace_light_curve(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                           const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, R* rgb, const rtgr_ray_outputs* out, R* g,
                           double* lc, rtgr_counters* ctr) {
    LcResolved<R> L;
    return trace_reduce<R>(ctx, lc_reduction<R>(scene, emit, spot, obs, L), scene, opt, obs, ni, nj, shade, emit, rgb, out, g, lc, ctr);
}

// the hook, on device 0 of the context (host pointers, blocking): the stage's own Omega_s, and the point kernel
template <class R>
int api::eval_hot_spot(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, const R* xyt, uint64_t n,
                       R* omega_s, int* valid, double* j) {
    RESOLVE_CONTEXT();
    if (n && (!xyt || !j)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_hot_spot: NULL argument");
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_hot_spot: at most 2^32 points per call");
    LcResolved<R> L;
    if ((rc = lc_resolve<R>(scene, emit, spot, nullptr, 1, 1, L))) return rc;
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    if ((rc = stationary_scene<R>(D, scene, sc, nullptr, EMISSION_NEEDS_STATIONARY))) return rc;
    char head[LC_HEAD];   // the whole head comes back: Omega_s is read from it
    char* d_head = m.out(head, LC_HEAD);
    const R* d_xyt = m.in(xyt, (size_t)n * 3);
    double* d_j = m.out(j, n);
    if ((rc = m.status())) return rc;
    if ((rc = lc_omega<R>(sc, L.em, L.S.rho_s, d_head, nullptr))) return rc;
    if (n && (rc = lc_points_launch<R>(d_xyt, n, L.S, d_head, d_j, nullptr))) return rc;
    if ((rc = m.fetch())) return rc;
    R om;
    std::memcpy(&om, head + LC_HEAD_OMEGA, sizeof om);
    if (omega_s) *omega_s = om;
    if (valid) *valid = std::isfinite((double)om) ? 1 : 0;
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(api::light_curve_device);
RTGR_INSTANTIATE_F64_F32(api::trace_light_curve_device);
RTGR_INSTANTIATE_F64_F32(api::trace_light_curve);
RTGR_INSTANTIATE_F64_F32(api::eval_hot_spot);

}  // namespace rtgr
