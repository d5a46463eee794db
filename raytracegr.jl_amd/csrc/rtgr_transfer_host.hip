// rtgr_transfer_host.hip — volume emission (include/rtgr.h "volume emission"): the checks of an rtgr_flow, the transfer trace —
// rtgr_observer_host.hip's trace with the transfer kernel behind everything else of each batch — and the two hooks.  Host code only: the
// kernels are tu_transfer_f64.hip's and tu_transfer_f32.hip's, the model rtgr_transfer.hpp's.
#include "rtgr_internal.hpp"

namespace rtgr {

constexpr const char* TRANSFER_CANVAS = "a transfer frame";
constexpr const char* TRANSFER_NEEDS_STATIONARY = "volume emission in a time-dependent (4-D) grid metric is not supported";

// the caller's record, checked against its scene, into the record the kernels read, for scalar type R
template <class R>
static int flow_resolve(const rtgr_scene* scene, const rtgr_flow* flow, DevFlow<R>& fl) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!flow) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow is NULL (flow)");
    int rc;
    if ((rc = builtin_metric_check(scene, "volume emission in", "the transfer kernels integrate the closed right-hand sides; none lives"))) return rc;
    const uint32_t kind = scene->metric & ~(uint32_t)RTGR_METRIC_GENERIC;
    if (kind != RTGR_MINKOWSKI && kind != RTGR_KS_REF && kind != RTGR_KS_TRUE)
        return fail(RTGR_ERR_BAD_ARG, "volume emission needs a closed right-hand side: rtgr_scene.metric must be RTGR_MINKOWSKI, RTGR_KS_REF or RTGR_KS_TRUE "
                                      "(metrics sampled on a grid, RTGR_GRID and 4-D grids, are not supported)");
    if (flow->emitter != RTGR_EMIT_KEPLER && flow->emitter != RTGR_EMIT_RIGID)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.emitter: unknown emitter " + std::to_string(flow->emitter) + " (RTGR_EMIT_KEPLER = 0, RTGR_EMIT_RIGID = 1)");
    if (flow->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.flags must be 0");
    if (!std::isfinite(flow->orbit)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.orbit must be finite");
    if (flow->emitter == RTGR_EMIT_KEPLER && flow->orbit != 1.0 && flow->orbit != -1.0)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.orbit of RTGR_EMIT_KEPLER names a root: +1 (Omega_+) or -1 (Omega_-)");
    if (!(flow->j0 >= 0.0) || !std::isfinite(flow->j0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.j0 must be >= 0 and finite");
    if (!(flow->kappa >= 0.0) || !std::isfinite(flow->kappa)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.kappa must be >= 0 and finite (0: optically thin)");
    if (!(flow->r0 > 0.0) || !std::isfinite(flow->r0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.r0 must be > 0 and finite");
    if (!std::isfinite(flow->alpha)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.alpha must be finite");
    if (!(flow->H > 0.0) || !std::isfinite(flow->H)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.H must be > 0 and finite");
    if (!std::isfinite(flow->s)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.s must be finite");
    if (!(flow->r_stop >= 0.0) || !std::isfinite(flow->r_stop)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.r_stop must be >= 0 and finite");
    if (!std::isfinite(flow->gain)) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.gain must be finite");
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(flow->weight[c])) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow.weight[" + std::to_string(c) + "] must be finite");
    std::memset(&fl, 0, sizeof fl);
    fl.emitter = flow->emitter;
    fl.orbit = (R)flow->orbit; fl.j0 = (R)flow->j0; fl.kappa = (R)flow->kappa; fl.r0 = (R)flow->r0; fl.alpha = (R)flow->alpha; fl.H = (R)flow->H;
    fl.s = (R)flow->s; fl.r_stop = (R)flow->r_stop; fl.gain = (R)flow->gain;
    for (int c = 0; c < 3; c++) fl.weight[c] = (R)flow->weight[c];
    return RTGR_OK;
}

// what both traced entries refuse before they touch a device, beyond what the observer trace refuses itself
template <class R>
static int transfer_check(const rtgr_scene* scene, const rtgr_flow* flow, const rtgr_observer* obs, const void* rgb, TransferStage<R>& stage) {
    if (!flow) return fail(RTGR_ERR_BAD_ARG, "rtgr_flow is NULL (flow)");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    return flow_resolve<R>(scene, flow, stage.fl);
}

template <class R>
int api::trace_transfer_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                               const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_flow* flow, R* d_rgb, const rtgr_ray_outputs* out,
                               R* d_g, R* d_I, R* d_tau, uint8_t* d_tstatus, uint32_t* d_tsteps, rtgr_counters* ctr, rtgr_counters* tctr, void* stream) {
    RESOLVE_CONTEXT();
    TransferStage<R> stage;
    if ((rc = transfer_check<R>(scene, flow, obs, d_rgb, stage))) return rc;
    if (tctr && stream_capturing((hipStream_t)stream))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_transfer_*: the stream is being captured and `tctr` asks for a synchronisation at the end of the call "
                                      "(which cannot be captured): pass tctr = NULL");
    stage.I = d_I; stage.tau = d_tau; stage.tstatus = d_tstatus; stage.tsteps = d_tsteps; stage.tctr = tctr;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_observer_on<R>(*D, scene, opt, obs, ni, nj, shade, emit, d_rgb, out, d_g, ctr, (hipStream_t)stream, nullptr, &stage);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream; the frame and the four planes copied out
template <class R>
int api::trace_transfer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                        const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_flow* flow, R* rgb, const rtgr_ray_outputs* out, R* g, R* I,
                        R* tau, uint8_t* tstatus, uint32_t* tsteps, rtgr_counters* ctr, rtgr_counters* tctr) {
    RESOLVE_CONTEXT();
    TransferStage<R> stage;
    if ((rc = transfer_check<R>(scene, flow, obs, rgb, stage))) return rc;
    if ((rc = canvas_check(ni, nj, TRANSFER_CANVAS))) return rc;
    const uint64_t n = ni * nj;
    HostMirror m(c);
    stage.I = m.out(I, n); stage.tau = m.out(tau, n); stage.tstatus = m.out(tstatus, n); stage.tsteps = m.out(tsteps, n);
    stage.tctr = tctr;
    if ((rc = m.status())) return rc;
    return staged_frame<R>(c, n, rgb, out, nullptr, g, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t*, R* d_g, hipStream_t st) {
        int r = trace_observer_on<R>(D, scene, opt, obs, ni, nj, shade, emit, d_rgb, d_out, d_g, ctr, st, nullptr, &stage);
        return r ? r : m.fetch(st);
    });
}

// the transfer kernel itself over n listed rays, on device 0 of the context (host pointers, blocking).  obs (may be null): u_obs is the
// e_0 of that observer's frame, built by the frame kernel ahead of the rays; null: the static observer at each ray's start
template <class R>
int api::eval_transfer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_flow* flow, const rtgr_observer* obs, const R* s0,
                       const R* lambda_end, uint64_t n, R* I, R* tau, R* s_end, uint8_t* tstatus, uint32_t* tsteps) {
    RESOLVE_CONTEXT();
    if (!opt) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_transfer: solver is NULL (opt)");
    if (n && (!s0 || !lambda_end)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_transfer: NULL argument (s0, lambda_end)");
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_transfer: at most 2^32 rays per call");
    TransferArgs<R> T;
    std::memset(&T, 0, sizeof T);
    if ((rc = flow_resolve<R>(scene, flow, T.fl))) return rc;
    if ((rc = convert_solver<R>(opt, T.opt))) return rc;
    DevObserver<R> ob;
    if (obs && (rc = observer_resolve<R>(scene, obs, ob))) return rc;
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    if ((rc = stationary_scene<R>(D, scene, T.sc, nullptr, TRANSFER_NEEDS_STATIONARY))) return rc;
    if (n == 0) return RTGR_OK;
    T.state0 = m.in(s0, (size_t)n * 8); T.lambda_end = m.in(lambda_end, n);
    ObsFrame<R>* d_frame = obs ? m.scratch<ObsFrame<R>>(1) : nullptr;
    T.I = m.out(I, n); T.tau = m.out(tau, n); T.s_end = m.out(s_end, (size_t)n * 8); T.tstatus = m.out(tstatus, n); T.tsteps = m.out(tsteps, n);
    if ((rc = m.status())) return rc;
    if (obs && (rc = observer_frame_launch<R>(T.sc, ob, d_frame, nullptr))) return rc;
    T.obs = d_frame;
    T.n = n;
    if ((rc = transfer_launch<R>(T, nullptr))) return rc;
    return m.fetch();
}

// the model at n points s = (x, k) of rays started at s0, on device 0 of the context (host pointers, blocking)
template <class R>
int api::eval_flow(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_flow* flow, const rtgr_observer* obs, const R* s0, const R* s, uint64_t n,
                   R* dens, R* omega, R* u_f, R* gfac, R* dtau, R* dI0) {
    RESOLVE_CONTEXT();
    if (n && (!s0 || !s)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_flow: NULL argument (s0, s)");
    if (n > (1ull << 32)) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_flow: at most 2^32 points per call");
    FlowArgs<R> F;
    std::memset(&F, 0, sizeof F);
    if ((rc = flow_resolve<R>(scene, flow, F.fl))) return rc;
    DevObserver<R> ob;
    if (obs && (rc = observer_resolve<R>(scene, obs, ob))) return rc;
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    if ((rc = stationary_scene<R>(D, scene, F.sc, nullptr, TRANSFER_NEEDS_STATIONARY))) return rc;
    if (n == 0) return RTGR_OK;
    F.state0 = m.in(s0, (size_t)n * 8); F.state = m.in(s, (size_t)n * 8);
    ObsFrame<R>* d_frame = obs ? m.scratch<ObsFrame<R>>(1) : nullptr;
    F.dens = m.out(dens, n); F.omega = m.out(omega, n); F.u_f = m.out(u_f, (size_t)n * 4); F.gfac = m.out(gfac, n); F.dtau = m.out(dtau, n);
    F.dI0 = m.out(dI0, n);
    if ((rc = m.status())) return rc;
    if (obs && (rc = observer_frame_launch<R>(F.sc, ob, d_frame, nullptr))) return rc;
    F.obs = d_frame;
    F.n = n;
    if ((rc = flow_launch<R>(F, nullptr))) return rc;
    return m.fetch();
}

RTGR_INSTANTIATE_F64_F32(api::trace_transfer_device);
RTGR_INSTANTIATE_F64_F32(api::trace_transfer);
RTGR_INSTANTIATE_F64_F32(api::eval_transfer);
RTGR_INSTANTIATE_F64_F32(api::eval_flow);

}  // namespace rtgr
