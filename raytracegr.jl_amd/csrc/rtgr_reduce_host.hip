// rtgr_reduce_host.hip — THE path from a traced frame of an emitting disk to a reduced table of (F, A, B) rows, shared by the hot-spot
// light curves (rtgr_lightcurve_host.hip) and the disk spectra (rtgr_spectrum_host.hip): the pixel weight of an observer's canvas, the
// stream's reduction scratch, the stage over given planes, the traced call (the observer trace of rtgr_observer_host.hip, untouched, then
// one stage over the whole frame) on a device, its device entry and its host-pointer entry.  What differs between the two features is a
// Reduction (rtgr_internal.hpp).  Host code only: the kernels are rtgr_reduce.hpp's, instantiated in rtgr_lightcurve.hip and rtgr_spectrum.hip.
#include "rtgr_internal.hpp"
#include "rtgr_reduce.hpp"

namespace rtgr {

template <class R>
int pixel_weight_resolve(const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, PixelWeight& W) {
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

// The reduction scratch of a stream, grown to `bytes` (ReduceLayout::bytes).  D.mu held.  Grow-only and retired like the frame scratch;
// growth is refused while the stream is captured.
static int reduce_scratch(DeviceCtx& D, hipStream_t st, bool capturing, const EntryWords& who, size_t bytes, char** base) {
    int rc;
    StreamState* ss = nullptr;
    if ((rc = stream_state(D, st, &ss))) return rc;
    if (capturing && bytes > ss->reduce_bytes)
        return fail(RTGR_ERR_BAD_ARG, std::string(who.entry) + ": the stream's " + who.scratch + " scratch must grow but the stream is being captured: make a "
                                      "call of this size on the stream before hipStreamBeginCapture");
    if ((rc = scratch_need(*ss, ss->reduce, ss->reduce_bytes, bytes))) return rc;
    *base = (char*)ss->reduce;
    return RTGR_OK;
}

// what every call does between its refusals and its kernels, on the current device: whether st is captured, the scene as the emitter
// reads it, and the stream's scratch laid out for n pixels with the planes `given`
template <class R>
static int reduce_prepare(DeviceCtx& D, hipStream_t st, const EntryWords& who, const Reduction<R>& red, const rtgr_scene* scene, uint64_t n,
                          const ReduceGiven& given, const rtgr_counters* ctr, DevScene<R>& sc, char** base, ReduceLayout& at) {
    int rc;
    bool capturing;
    if ((rc = capture_check(st, who, ctr, &capturing))) return rc;
    at = reduce_layout(red.head_bytes, reduce_partial_bytes(n, red.rows), n, sizeof(R), given);
    std::lock_guard<std::mutex> lk(D.mu);
    if ((rc = stationary_scene<R>(D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
    return reduce_scratch(D, st, capturing, who, at.bytes, base);
}

// the stage on device D, stream st, over planes of that device
template <class R>
static int reduce_stage(DeviceCtx& D, const Reduction<R>& red, const DevScene<R>& sc, uint32_t object, uint64_t ni, uint64_t nj, const uint32_t* d_hit32,
                        const R* d_state_end, const R* d_g, char* base, double* d_out, hipStream_t st) {
    std::lock_guard<std::mutex> lk(D.mu);
    KernelTimer timer(D, st, 0);
    ReducePlanes<R> P;
    P.hit32 = d_hit32; P.state_end = d_state_end; P.g = d_g;
    P.n = ni * nj; P.ni = ni; P.nj = nj; P.object = object; P.pad = 0;
    return red.stage(D, sc, P, base, d_out, st);
}

template <class R>
int reduce_device(rtgr_context* ctx, const Reduction<R>& red, const rtgr_scene* scene, const rtgr_disk_emission* emit, uint64_t ni, uint64_t nj,
                  const uint32_t* d_hit32, const R* d_state_end, const R* d_g, double* d_out, void* stream) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    const std::string entry = std::string(red.device.entry) + ": ";
    if (!d_hit32) return fail(RTGR_ERR_BAD_ARG, entry + "hit32 is NULL");
    if (!d_state_end) return fail(RTGR_ERR_BAD_ARG, entry + "state_end is NULL");
    if (!d_g) return fail(RTGR_ERR_BAD_ARG, entry + "g is NULL");
    if (!d_out) return fail(RTGR_ERR_BAD_ARG, entry + red.out_name + " is NULL");
    if ((rc = canvas_check(ni, nj, red.canvas))) return rc;
    if ((rc = red.resolve(ni, nj))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_out, &D))) return rc;
    hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard(D->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    DevScene<R> sc;
    char* base = nullptr;
    ReduceLayout at;
    ReduceGiven all;
    all.state_end = all.hit32 = all.g = true;
    if ((rc = reduce_prepare<R>(*D, st, red.device, red, scene, ni * nj, all, nullptr, sc, &base, at))) return rc;
    return reduce_stage<R>(*D, red, sc, emit->object, ni, nj, d_hit32, d_state_end, d_g, base, d_out, st);
}

// the traced call on device D, stream st
template <class R>
static int trace_reduce_on(rtgr_context* c, DeviceCtx& D, const Reduction<R>& red, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs,
                           uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, R* d_rgb, const rtgr_ray_outputs* out, R* d_g,
                           double* d_out, rtgr_counters* ctr, hipStream_t st) {
    int rc;
    if ((rc = red.resolve(ni, nj))) return rc;
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if ((rc = canvas_check(ni, nj, "an observer frame"))) return rc;
    const uint64_t n = ni * nj;
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    rtgr_ray_outputs o2;
    if (out) o2 = *out; else std::memset(&o2, 0, sizeof o2);
    ReduceGiven given;
    given.state_end = o2.state_end != nullptr; given.hit32 = o2.hit32 != nullptr; given.g = d_g != nullptr;
    DevScene<R> sc;
    char* base = nullptr;
    ReduceLayout at;
    if ((rc = reduce_prepare<R>(D, st, red.traced, red, scene, n, given, ctr, sc, &base, at))) return rc;
    if (!given.state_end) o2.state_end = base + at.state_end;
    if (!given.hit32) o2.hit32 = (uint32_t*)(base + at.hit32);
    R* g2 = given.g ? d_g : (R*)(base + at.g);
    if ((rc = api::trace_observer_device<R>(c, scene, opt, obs, ni, nj, shade, emit, d_rgb, &o2, g2, ctr, (void*)st))) return rc;
    return reduce_stage<R>(D, red, sc, emit->object, ni, nj, o2.hit32, (const R*)o2.state_end, g2, base, d_out, st);
}

template <class R>
static int trace_reduce_check(const Reduction<R>& red, const rtgr_scene* scene, const rtgr_observer* obs, const rtgr_disk_emission* emit, const void* rgb,
                              const void* table) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!obs) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs)");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!red.record) return fail(RTGR_ERR_BAD_ARG, red.record_null);
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if (!table) return fail(RTGR_ERR_BAD_ARG, std::string(red.traced.entry) + ": " + red.out_name + " is NULL");
    return RTGR_OK;
}

template <class R>
int trace_reduce_device(rtgr_context* ctx, const Reduction<R>& red, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                        uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, double* d_out,
                        rtgr_counters* ctr, void* stream) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if ((rc = trace_reduce_check<R>(red, scene, obs, emit, d_rgb, d_out))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_reduce_on<R>(c, *D, red, scene, opt, obs, ni, nj, shade, emit, d_rgb, out, d_g, d_out, ctr, (hipStream_t)stream);
}

template <class R>
int trace_reduce(rtgr_context* ctx, const Reduction<R>& red, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                 uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, R* rgb, const rtgr_ray_outputs* out, R* g, double* table,
                 rtgr_counters* ctr) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if ((rc = trace_reduce_check<R>(red, scene, obs, emit, rgb, table))) return rc;
    if ((rc = canvas_check(ni, nj, "an observer frame"))) return rc;
    if ((rc = red.resolve(ni, nj))) return rc;   // (every refusal before anything is allocated or written)
    const size_t table_bytes = (size_t)red.rows * 3 * sizeof(double);
    DeviceGuard guard(c->devs[0]->dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    DevBuf d_table;
    if ((rc = d_table.alloc(table_bytes))) return rc;
    rc = staged_frame<R>(c, ni * nj, rgb, out, nullptr, g, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t*, R* d_g, hipStream_t st) {
        return trace_reduce_on<R>(c, D, red, scene, opt, obs, ni, nj, shade, emit, d_rgb, d_out, d_g, (double*)d_table.p, ctr, st);
    });
    if (rc) return rc;
    HIP_TRY(hipMemcpy(table, d_table.p, table_bytes, hipMemcpyDeviceToHost));   // (staged_frame has synchronised its stream)
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(pixel_weight_resolve);
RTGR_INSTANTIATE_F64_F32(reduce_device);
RTGR_INSTANTIATE_F64_F32(trace_reduce_device);
RTGR_INSTANTIATE_F64_F32(trace_reduce);

}  // namespace rtgr
