// rtgr_spectrum_host.hip — disk spectra (include/rtgr.h "disk spectra"): the checks of an rtgr_spectrum, the spectrum stage, the entry
// points as a Reduction each (the path from a traced frame to the table: rtgr_reduce_host.hip) and the hook.  Host code only: the
// kernels are rtgr_spectrum.hip's, the model rtgr_spectrum.hpp's.
#include "rtgr_internal.hpp"
#include "rtgr_reduce.hpp"

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
                            uint64_t nj, SpecDev& S, PixelWeight& W) {
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

// A spectrum call as a Reduction (rtgr_internal.hpp; the bodies: rtgr_reduce_host.hip).  `S`, `W`: the caller's, filled by the resolve
// step and read by the stage — the reduction over the bins or sample frequencies; no head
template <class R>
static Reduction<R> spectrum_reduction(const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const rtgr_observer* obs,
                                       SpecDev& S, PixelWeight& W) {
    Reduction<R> red;
    red.device = SPECTRUM_WORDS; red.traced = TRACE_SPECTRUM_WORDS;
    red.canvas = "a spectrum"; red.out_name = "the output (spectrum)";
    red.record = spec; red.record_null = "rtgr_spectrum is NULL (spec)";
    red.head_bytes = 0;
    red.rows = spec ? spec->nb : 0;
    red.resolve = [=, &S, &W](uint64_t ni, uint64_t nj) { return spectrum_resolve<R>(scene, emit, spec, obs, ni, nj, S, W); };
    red.stage = [&S, &W](DeviceCtx&, const DevScene<R>&, const ReducePlanes<R>& P, char* base, double* d_out, hipStream_t st) {
        return spec_reduce_launch<R>(P, S, W, (double*)base, d_out, st);
    };
    return red;
}

template <class R>
int api::spectrum_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const rtgr_observer* obs,
                         uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state_end, const R* d_g, double* d_out, void* stream) {
    SpecDev S;
    PixelWeight W;
    return reduce_device<R>(ctx, spectrum_reduction<R>(scene, emit, spec, obs, S, W), scene, emit, ni, nj, d_hit32, d_state_end, d_g, d_out, stream);
}

template <class R>
int api::trace_spectrum_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                               const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, R* d_rgb, const rtgr_ray_outputs* out,
                               R* d_g, double* d_out, rtgr_counters* ctr, void* stream) {
    SpecDev S;
    PixelWeight W;
    return trace_reduce_device<R>(ctx, spectrum_reduction<R>(scene, emit, spec, obs, S, W), scene, opt, obs, ni, nj, shade, emit, d_rgb, out, d_g, d_out, ctr,
                                  stream);
}

template <class R>
int api::trace_spectrum(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                        const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, R* rgb, const rtgr_ray_outputs* out, R* g,
                        double* spectrum, rtgr_counters* ctr) {
    SpecDev S;
    PixelWeight W;
    return trace_reduce<R>(ctx, spectrum_reduction<R>(scene, emit, spec, obs, S, W), scene, opt, obs, ni, nj, shade, emit, rgb, out, g, spectrum, ctr);
}

// the hook, on device 0 of the context (host pointers, blocking): the point kernel
template <class R>
int api::eval_spectrum(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const R* xyg, uint64_t n,
                       double* axis, int64_t* bin, double* val) {
    RESOLVE_CONTEXT();
    if (n && !xyg) return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_spectrum: xyg is NULL");
    SpecDev S;
    PixelWeight W;
    if ((rc = spectrum_resolve<R>(scene, emit, spec, nullptr, 1, 1, S, W))) return rc;
    if (n > SPEC_MAX_POINT_VALUES || n * S.nb > SPEC_MAX_POINT_VALUES)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_eval_spectrum: n x nb = " + std::to_string(n) + " x " + std::to_string(S.nb) + ": at most 2^26 per call");
    DeviceCtx& D = *c->devs[0];
    HostMirror m(D);
    if ((rc = m.status())) return rc;
    std::lock_guard<std::mutex> lk(D.mu);
    DevScene<R> sc;
    if ((rc = stationary_scene<R>(D, scene, sc, nullptr, EMISSION_NEEDS_STATIONARY))) return rc;
    const R* d_xyg = m.in(xyg, (size_t)n * 3);
    double* d_axis = m.out(axis, S.nb);
    int64_t* d_bin = m.out(bin, n);
    double* d_val = m.out(val, (size_t)(S.kind == RTGR_SPEC_THERMAL ? n * S.nb : n));
    if ((rc = m.status())) return rc;
    if ((rc = spec_points_launch<R>(d_xyg, n, S, d_axis, d_bin, d_val, nullptr))) return rc;
    return m.fetch();
}

RTGR_INSTANTIATE_F64_F32(api::spectrum_device);
RTGR_INSTANTIATE_F64_F32(api::trace_spectrum_device);
RTGR_INSTANTIATE_F64_F32(api::trace_spectrum);
RTGR_INSTANTIATE_F64_F32(api::eval_spectrum);

}  // namespace rtgr
