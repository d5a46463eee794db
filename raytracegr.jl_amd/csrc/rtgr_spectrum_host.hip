// rtgr_spectrum_host.hip — disk spectra (include/rtgr.h "disk spectra"): the checks of an rtgr_spectrum, the stage's share of a stream's
// light-curve scratch, the spectrum stage, the traced spectrum (the observer trace of rtgr_observer_host.hip, untouched, then one stage
// over the whole frame) and the hook.  Host code only: the kernels are rtgr_spectrum.hip's, the model rtgr_spectrum.hpp's.
#include "rtgr_internal.hpp"

namespace rtgr {

constexpr EntryWords SPECTRUM_WORDS = {"rtgr_spectrum_device_*", "light-curve", true};
constexpr EntryWords TRACE_SPECTRUM_WORDS = {"rtgr_trace_spectrum_*", "light-curve", true};
constexpr uint64_t SPEC_MAX_POINT_VALUES = 1ull << 26;   // n x nb of the hook at most

// the caller's record, checked against the emitting disk of its scene, into what the kernels read (S.em is set by the caller)
static int spectrum_fields(const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, SpecDev& S) {
    if (!spec) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum is NULL (spec)");
    if (spec->kind != RTGR_SPEC_LINE && spec->kind != RTGR_SPEC_THERMAL)
        return fail(RTGR_ERR_BAD_ARG, "unknown rtgr_spectrum.kind " + std::to_string(spec->kind));
    if (spec->flags & ~(RTGR_SPEC_LOG | RTGR_SPEC_NU3)) return fail(RTGR_ERR_BAD_ARG, "unknown rtgr_spectrum.flags " + std::to_string(spec->flags));
    if (spec->nb == 0 || spec->nb > RTGR_SPECTRUM_MAX_BINS)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.nb = " + std::to_string(spec->nb) + ": need 1 .. 2^16 bins or sample frequencies");
    if (!(spec->reserved == 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.reserved must be 0");
    const struct { const char* name; double v; } fields[] = {{"lo", spec->lo}, {"hi", spec->hi}, {"amp", spec->amp}, {"alpha", spec->alpha},
                                                              {"rho_min", spec->rho_min}, {"rho_max", spec->rho_max}, {"g_power", spec->g_power}};
    for (const auto& f : fields)
        if (!std::isfinite(f.v)) return fail(RTGR_ERR_BAD_ARG, std::string("rtgr_spectrum.") + f.name + " must be finite");
    S.kind = spec->kind; S.flags = spec->flags; S.nb = spec->nb;
    S.lo = spec->lo; S.hi = spec->hi; S.s = 0.0; S.span = 0.0;
    S.amp = spec->amp; S.alpha = spec->alpha; S.rho_min = spec->rho_min; S.rho_max = spec->rho_max; S.q = spec->g_power;
    if (spec->kind == RTGR_SPEC_LINE) {
        if (spec->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.flags must be 0 for RTGR_SPEC_LINE (RTGR_SPEC_LOG and RTGR_SPEC_NU3 are THERMAL's)");
        if (!(spec->amp >= 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.amp must be >= 0");
        if (!(spec->lo >= 0.0) || !(spec->lo < spec->hi)) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.lo, hi: RTGR_SPEC_LINE needs 0 <= lo < hi");
        const rtgr_object& o = scene_objects(scene)[emit->object - 1];   // (a Disk: emission_resolve has checked)
        if (!(spec->rho_min > 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.rho_min must be > 0");
        if (!(spec->rho_min < spec->rho_max)) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.rho_min must be < rho_max");
        if (!(spec->rho_min >= o.p[1] && spec->rho_max <= o.p[2]))
            return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.rho_min, rho_max = " + std::to_string(spec->rho_min) + ", " + std::to_string(spec->rho_max) +
                                          " lie outside the emitting Disk's [r_in, r_out] = [" + std::to_string(o.p[1]) + ", " + std::to_string(o.p[2]) + "]");
        S.s = (double)spec->nb / (spec->hi - spec->lo);
    } else {
        if (!(spec->lo > 0.0) || !(spec->lo <= spec->hi)) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum.lo, hi: RTGR_SPEC_THERMAL needs 0 < lo <= hi");
        for (int k = 2; k < 7; k++)
            if (fields[k].v != 0.0)
                return fail(RTGR_ERR_BAD_ARG, std::string("rtgr_spectrum.") + fields[k].name + " must be 0 for RTGR_SPEC_THERMAL (a field of RTGR_SPEC_LINE)");
        S.span = (spec->flags & RTGR_SPEC_LOG) ? std::log(spec->hi / spec->lo) : spec->hi - spec->lo;
    }
    return RTGR_OK;
}

// everything a spectrum call resolves before it touches a device: the emitter (in double, whatever the entry's scalar type), the
// record, the pixel weight of `obs` (may be null)
template <class R>
static int spectrum_resolve(const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const rtgr_observer* obs, uint64_t ni,
                            uint64_t nj, SpecDev& S, LcWeight& W) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!spec) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum is NULL (spec)");
    int rc;
    DevEmission<R> em;   // (the entry's own conversion refuses what the trace would refuse)
    if ((rc = emission_resolve<R>(scene, nullptr, emit, em))) return rc;
    if ((rc = emission_resolve<double>(scene, nullptr, emit, S.em))) return rc;
    if ((rc = spectrum_fields(scene, emit, spec, S))) return rc;
    return pixel_weight_resolve<R>(scene, obs, ni, nj, W);
}

// The stage's share of the stream's light-curve scratch: the partial sums of one pass at its start (the light curve's stage and this
// one are ordered on the stream, and no head is needed), then `borrow` bytes (the planes a traced spectrum keeps there).  D.mu held.
// Grow-only and retired like the frame scratch; growth is refused while the stream is captured.
static int spectrum_scratch(DeviceCtx& D, hipStream_t st, bool capturing, const EntryWords& who, uint64_t n, uint64_t nb, size_t borrow, char** base,
                            size_t* off_borrow) {
    int rc;
    StreamState* ss = nullptr;
    if ((rc = stream_state(D, st, &ss))) return rc;
    *off_borrow = spec_partial_bytes(n, nb);
    const size_t bytes = *off_borrow + borrow;
    if (capturing && bytes > ss->lc_bytes)
        return fail(RTGR_ERR_BAD_ARG, std::string(who.entry) + ": the stream's " + who.scratch + " scratch must grow but the stream is being captured: make a "
                                      "call of this size on the stream before hipStreamBeginCapture");
    if ((rc = scratch_need(*ss, ss->lc, ss->lc_bytes, bytes))) return rc;
    *base = (char*)ss->lc;
    return RTGR_OK;
}

// the stage on device D, stream st, over planes of that device; `base`: the stream's scratch
template <class R>
static int spectrum_stage(DeviceCtx& D, const SpecDev& S, const LcWeight& W, uint32_t object, uint64_t ni, uint64_t nj, const uint32_t* d_hit32,
                          const R* d_state_end, const R* d_g, char* base, double* d_out, hipStream_t st) {
    std::lock_guard<std::mutex> lk(D.mu);
    KernelTimer timer(D, st, 0);
    LcPlanes<R> P;
    P.hit32 = d_hit32; P.state_end = d_state_end; P.g = d_g;
    P.n = ni * nj; P.ni = ni; P.nj = nj; P.object = object; P.pad = 0;
    return spec_reduce_launch<R>(P, S, W, (double*)base, d_out, st);
}

template <class R>
int api::spectrum_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const rtgr_observer* obs,
                         uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state_end, const R* d_g, double* d_out, void* stream) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (!d_hit32) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum_device_*: hit32 is NULL");
    if (!d_state_end) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum_device_*: state_end is NULL");
    if (!d_g) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum_device_*: g is NULL");
    if (!d_out) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum_device_*: the output (spectrum) is NULL");
    if ((rc = canvas_check(ni, nj, "a spectrum"))) return rc;
    SpecDev S;
    LcWeight W;
    if ((rc = spectrum_resolve<R>(scene, emit, spec, obs, ni, nj, S, W))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_out, &D))) return rc;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(D->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    bool capturing;
    if ((rc = capture_check(st, SPECTRUM_WORDS, nullptr, &capturing))) return rc;
    char* base = nullptr;
    size_t off_borrow = 0;
    {
        std::lock_guard<std::mutex> lk(D->mu);
        DevScene<R> sc;   // (the scene's refusals: a 4-D grid is not stationary)
        if ((rc = stationary_scene<R>(*D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
        if ((rc = spectrum_scratch(*D, st, capturing, SPECTRUM_WORDS, ni * nj, spec->nb, 0, &base, &off_borrow))) return rc;
    }
    return spectrum_stage<R>(*D, S, W, emit->object, ni, nj, d_hit32, d_state_end, d_g, base, d_out, st);
}

// the traced spectrum on device D, stream st: rtgr_trace_observer_device_* with the planes the stage reads borrowed from the stream's
// light-curve scratch where the caller gave none, then the stage
template <class R>
static int trace_spectrum_on(rtgr_context* c, DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                             uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, R* d_rgb,
                             const rtgr_ray_outputs* out, R* d_g, double* d_out, rtgr_counters* ctr, hipStream_t st) {
    int rc;
    SpecDev S;
    LcWeight W;
    if ((rc = spectrum_resolve<R>(scene, emit, spec, obs, ni, nj, S, W))) return rc;
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if ((rc = canvas_check(ni, nj, "an observer frame"))) return rc;
    const uint64_t n = ni * nj;
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    bool capturing;
    if ((rc = capture_check(st, TRACE_SPECTRUM_WORDS, ctr, &capturing))) return rc;
    rtgr_ray_outputs o2;
    if (out) o2 = *out; else std::memset(&o2, 0, sizeof o2);
    const size_t b_state = o2.state_end ? 0 : align256((size_t)n * 8 * sizeof(R)), b_hit = o2.hit32 ? 0 : align256((size_t)n * sizeof(uint32_t)),
                 b_g = d_g ? 0 : align256((size_t)n * sizeof(R));
    char* base = nullptr;
    size_t at = 0;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        DevScene<R> sc;
        if ((rc = stationary_scene<R>(D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
        if ((rc = spectrum_scratch(D, st, capturing, TRACE_SPECTRUM_WORDS, n, spec->nb, b_state + b_hit + b_g, &base, &at))) return rc;
    }
    if (!o2.state_end) { o2.state_end = base + at; at += b_state; }
    if (!o2.hit32) { o2.hit32 = (uint32_t*)(base + at); at += b_hit; }
    R* g2 = d_g ? d_g : (R*)(base + at);
    if ((rc = api::trace_observer_device<R>(c, scene, opt, obs, ni, nj, shade, emit, d_rgb, &o2, g2, ctr, (void*)st))) return rc;
    return spectrum_stage<R>(D, S, W, emit->object, ni, nj, o2.hit32, (const R*)o2.state_end, g2, base, d_out, st);
}

static int trace_spectrum_check(const rtgr_scene* scene, const rtgr_observer* obs, const rtgr_disk_emission* emit, const rtgr_spectrum* spec,
                                const void* rgb, const void* out) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!spec) return fail(RTGR_ERR_BAD_ARG, "rtgr_spectrum is NULL (spec)");
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if (!out) return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_spectrum_*: the output (spectrum) is NULL");
    return RTGR_OK;
}

template <class R>
int api::trace_spectrum_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                               const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, R* d_rgb, const rtgr_ray_outputs* out,
                               R* d_g, double* d_out, rtgr_counters* ctr, void* stream) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if ((rc = trace_spectrum_check(scene, obs, emit, spec, d_rgb, d_out))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_spectrum_on<R>(c, *D, scene, opt, obs, ni, nj, shade, emit, spec, d_rgb, out, d_g, d_out, ctr, (hipStream_t)stream);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream; the frame and the spectrum copied out
template <class R>
int api::trace_spectrum(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                        const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, R* rgb, const rtgr_ray_outputs* out, R* g,
                        double* spectrum, rtgr_counters* ctr) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if ((rc = trace_spectrum_check(scene, obs, emit, spec, rgb, spectrum))) return rc;
    if ((rc = canvas_check(ni, nj, "an observer frame"))) return rc;
    {
        SpecDev S;   // (every refusal before anything is allocated or written)
        LcWeight W;
        if ((rc = spectrum_resolve<R>(scene, emit, spec, obs, ni, nj, S, W))) return rc;
    }
    const size_t out_bytes = (size_t)spec->nb * 3 * sizeof(double);
    DeviceGuard guard(c->devs[0]->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    DevBuf d_out;
    if ((rc = d_out.alloc(out_bytes))) return rc;
    rc = staged_frame<R>(c, ni * nj, rgb, out, nullptr, g, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_o, uint8_t*, R* d_g, hipStream_t st) {
        return trace_spectrum_on<R>(c, D, scene, opt, obs, ni, nj, shade, emit, spec, d_rgb, d_o, d_g, (double*)d_out.p, ctr, st);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(spectrum, d_out.p, out_bytes, hipMemcpyDeviceToHost));   // (staged_frame has synchronised its stream)
    return RTGR_OK;
}

// the hook, on device 0 of the context (host pointers, blocking): the point kernel
template <class R>
int api::eval_spectrum(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const R* xyg, uint64_t n,
                       double* axis, int64_t* bin, double* val) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (n && !xyg) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_spectrum: xyg is NULL");
    SpecDev S;
    LcWeight W;
    if ((rc = spectrum_resolve<R>(scene, emit, spec, nullptr, 1, 1, S, W))) return rc;
    if (n > SPEC_MAX_POINT_VALUES || n * S.nb > SPEC_MAX_POINT_VALUES)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_spectrum: n x nb = " + std::to_string(n) + " x " + std::to_string(S.nb) + ": at most 2^26 per call");
    DeviceCtx& D = *c->devs[0];
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    if ((rc = stationary_scene<R>(D, scene, sc, nullptr, EMISSION_NEEDS_STATIONARY))) return rc;
    const size_t nval = (size_t)(S.kind == RTGR_SPEC_THERMAL ? n * S.nb : n);
    DevBuf d_xyg, d_axis, d_bin, d_val;
    if ((n && (rc = d_xyg.alloc((size_t)n * 3 * sizeof(R)))) || (axis && (rc = d_axis.alloc((size_t)S.nb * sizeof(double)))) ||
        (bin && n && (rc = d_bin.alloc((size_t)n * sizeof(int64_t)))) || (val && nval && (rc = d_val.alloc(nval * sizeof(double)))))
        return rc;
    if (n) HIP_TRY(hipMemcpy(d_xyg.p, xyg, (size_t)n * 3 * sizeof(R), hipMemcpyHostToDevice));
    if ((rc = spec_points_launch<R>((const R*)d_xyg.p, n, S, (double*)d_axis.p, (int64_t*)d_bin.p, (double*)d_val.p, nullptr))) return rc;
    HIP_TRY(hipDeviceSynchronize());
    if (axis) HIP_TRY(hipMemcpy(axis, d_axis.p, (size_t)S.nb * sizeof(double), hipMemcpyDeviceToHost));
    if (bin && n) HIP_TRY(hipMemcpy(bin, d_bin.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (val && nval) HIP_TRY(hipMemcpy(val, d_val.p, nval * sizeof(double), hipMemcpyDeviceToHost));
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(api::spectrum_device);
RTGR_INSTANTIATE_F64_F32(api::trace_spectrum_device);
RTGR_INSTANTIATE_F64_F32(api::trace_spectrum);
RTGR_INSTANTIATE_F64_F32(api::eval_spectrum);

}  // namespace rtgr
