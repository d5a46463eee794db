// rtgr_aa_host.hip — adaptive anti-aliasing (include/rtgr.h "adaptive anti-aliasing"): the plain frame, the edge rule over it, and a
// sparse second trace of the flagged pixels' k x k sub-rays, averaged back into the frame.  Host side only: both traces are
// trace_device — the integrate / prepare / resolve kernels run as for any other call, the sub-rays as caller-supplied ray states —
// and the three small kernels in between are rtgr_aa.hip's.  With an AfterTrace — what is applied to a traced frame before its colours
// are read: the textures of rtgr_trace_shaded_* (rtgr_texture_host.hip), the emitting disk of rtgr_trace_emission_* (rtgr_emission_host.hip)
// or both — the two traces also deliver their end states and the shading / emission kernels run behind each; without one nothing of
// that exists.
#include "rtgr_internal.hpp"

namespace rtgr {

constexpr uint64_t AA_DEFAULT_BATCH = 1ull << 22;   // sub-rays per batch (rtgr_aa.max_batch_rays = 0)
constexpr size_t AA_HEAD = 256;                     // head of the frame scratch: rtgr_counters (64 bytes), then the refined count

static int aa_check(const rtgr_scene* scene, const rtgr_camera* cam, const rtgr_aa* aa, uint64_t ni, uint64_t nj) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!aa) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa is NULL");
    if (aa->k < 2 || aa->k > 8) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa.k must be 2..8 (k x k sub-rays per refined pixel), got " + std::to_string(aa->k));
    if (aa->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa.flags must be 0");
    if (aa->contrast != aa->contrast) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa.contrast is NaN (< 0: every pixel, +Inf: class edges only)");
    if (!cam) return fail(RTGR_ERR_BAD_ARG, "anti-aliasing needs a camera (cam is NULL): the sub-rays are generated from it");
    if ((scene->metric & ~RTGR_METRIC_GENERIC) == RTGR_USER)
        return fail(RTGR_ERR_BAD_ARG, "anti-aliasing of a scene whose METRIC is RTGR_USER is not supported (its camera kernel lives in the run-time "
                                      "unit); user objects under a built-in metric are");
    if (ni == 0 || nj == 0 || ni > (1ull << 32) || nj > (1ull << 32) || ni * nj > (1ull << 34))
        return fail(RTGR_ERR_BAD_ARG, "bad canvas: need ni, nj > 0 and at most 2^34 pixels for an anti-aliased frame");
    return RTGR_OK;
}

// grow-only scratch of a stream, retired like its workspace (D.mu held; never called during capture: the entry point refuses first)
int aa_need(StreamState& ss, void*& p, size_t& have, size_t bytes) {
    if (bytes <= have) return RTGR_OK;
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, bytes));
    if (p) ss.retired.push_back(p);   // kernels of an earlier call may still be in flight on it
    p = q;
    have = bytes;
    return RTGR_OK;
}

// the call on device D, stream st; d_rgb, the members of `out` and d_refined are pointers of that device
template <class R>
int trace_aa_on(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats,
                hipStream_t st, const AfterTrace<R>* after) {
    int rc;
    if ((rc = aa_check(scene, cam, aa, ni, nj))) return rc;
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_aa_*: the stream is being captured, and the call must read the number of refined pixels back "
                                      "between its two passes (a synchronisation cannot be captured)");
    const uint64_t n = ni * nj;
    const uint32_t k = aa->k, kk = k * k;
    const bool want_status = !(out && out->status), want_hit32 = !(out && out->hit32);
    const ShadeDesc<R>* shade = after ? after->shade : nullptr;
    const DevEmission<R>* emit = after ? after->emit : nullptr;
    const bool post = shade || emit;
    const bool want_state = post && !(out && out->state_end);   // (the shading and emission kernels read the end states)

    // ---- frame scratch: [counters | count] [hit32] [status] [list] [end states: shaded / emitted frames only] -------------------------------
    const size_t off_hit = AA_HEAD, off_status = off_hit + (want_hit32 ? align256(n * sizeof(uint32_t)) : 0),
                 off_list = off_status + (want_status ? align256(n) : 0), off_state = off_list + align256(n * sizeof(uint64_t)),
                 frame_bytes = off_state + (want_state ? align256(n * 8 * sizeof(R)) : 0);
    StreamState* ss = nullptr;
    DevScene<R> sc;
    DevCamera<R> cm;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if ((rc = stream_state(D, st, &ss))) return rc;   // (entries of the map stay where they are: `ss` outlives the lock)
        if ((rc = aa_need(*ss, ss->aa_frame, ss->aa_frame_bytes, frame_bytes))) return rc;
    }
    char* frame = (char*)ss->aa_frame;
    rtgr_counters* d_ctr = (rtgr_counters*)frame;
    unsigned long long* d_count = (unsigned long long*)(frame + sizeof(rtgr_counters));
    uint64_t* d_list = (uint64_t*)(frame + off_list);
    HIP_TRY(hipMemsetAsync(frame, 0, AA_HEAD, st));

    // ---- pass 1: the plain frame, with the hit map and the status bytes the edge rule reads --------------------------------------
    rtgr_ray_outputs o1;
    if (out) o1 = *out; else std::memset(&o1, 0, sizeof o1);
    if (want_hit32) o1.hit32 = (uint32_t*)(frame + off_hit);
    if (want_status) o1.status = (uint8_t*)(frame + off_status);
    if (want_state) o1.state_end = frame + off_state;
    if ((rc = trace_device<R>(D, scene, opt, nullptr, cam, ni, nj, 0, nj, d_rgb, &o1, ctr ? d_ctr : nullptr, st))) return rc;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        const UserModule* user = nullptr;
        if ((rc = convert_scene<R>(D, scene, sc, &user, st))) return rc;   // (what the sub-ray and emission kernels read of the scene: its metric)
        convert_camera<R>(cam, cm);
    }
    if (shade) {   // the edge rule reads the SHADED colours
        std::lock_guard<std::mutex> lk(D.mu);
        KernelTimer timer(D, st, 0);
        if ((rc = shade_launch<R>(ShadeArgs<R>{d_rgb, o1.hit32, o1.status, (const R*)o1.state_end, n, n, *shade}, st))) return rc;
    }
    if (emit) {    // … and the EMITTED ones; the pixel-centre rays start from the camera's own pixels
        std::lock_guard<std::mutex> lk(D.mu);
        KernelTimer timer(D, st, 0);
        if ((rc = emit_launch<R>(EmitArgs<R>{d_rgb, after->d_g, nullptr, nullptr, o1.hit32, (const R*)o1.state_end, nullptr, n, n, 1, ni, nj, sc, cm, *emit}, st))) return rc;
    }

    // ---- the edge rule -------------------------------------------------------------------------------------------------------------
    {
        std::lock_guard<std::mutex> lk(D.mu);
        KernelTimer timer(D, st, 0);
        if ((rc = aa_flag<R>(d_rgb, o1.hit32, o1.status, ni, nj, (R)aa->contrast, aa->contrast < 0.0, d_refined, d_list, d_count, st))) return rc;
    }
    unsigned long long count = 0;
    HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // THE synchronisation between the passes
    if (count > n) return fail(RTGR_ERR_HIP, "anti-aliasing: the refined count read back exceeds the canvas");

    // ---- pass 2: the listed pixels' sub-rays, a batch of whole pixels at a time ------------------------------------------------------
    const uint64_t budget = aa->max_batch_rays ? aa->max_batch_rays : AA_DEFAULT_BATCH;
    const uint64_t per = budget / kk ? budget / kk : 1;                      // pixels per batch
    const uint64_t batches = (count + per - 1) / per;
    const uint64_t m_max = count < per ? count : per;
    const size_t off_sub = align256((size_t)m_max * kk * 8 * sizeof(R));   // batch scratch: [sub-ray states] [sub-colours, 3 planes]
    // … and for a shaded or emitted frame what those kernels read of the sub-rays: [end states] [hit32] [status]
    const size_t off_end = off_sub + align256((size_t)m_max * kk * 3 * sizeof(R)), off_hit2 = off_end + (post ? align256((size_t)m_max * kk * 8 * sizeof(R)) : 0),
                 off_status2 = off_hit2 + (post ? align256((size_t)m_max * kk * sizeof(uint32_t)) : 0),
                 batch_bytes = off_status2 + (post ? align256((size_t)m_max * kk) : 0);
    if (count) {
        std::lock_guard<std::mutex> lk(D.mu);
        if ((rc = aa_need(*ss, ss->aa_batch, ss->aa_batch_bytes, batch_bytes))) return rc;
    }
    for (uint64_t b = 0; b < batches; b++) {
        const uint64_t first = b * per, m = count - first < per ? count - first : per;
        R* d_states = (R*)ss->aa_batch;
        R* d_sub = (R*)((char*)ss->aa_batch + off_sub);
        {
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = aa_subrays<R>(sc, cm, ni, nj, k, d_list + first, m, d_states, st))) return rc;
        }
        rtgr_ray_outputs o2;
        std::memset(&o2, 0, sizeof o2);
        if (post) {
            o2.state_end = (char*)ss->aa_batch + off_end;
            o2.hit32 = (uint32_t*)((char*)ss->aa_batch + off_hit2);
            o2.status = (uint8_t*)((char*)ss->aa_batch + off_status2);
        }
        if ((rc = trace_device<R>(D, scene, opt, d_states, nullptr, m * kk, 1, 0, 1, d_sub, post ? &o2 : nullptr, ctr ? d_ctr : nullptr, st))) return rc;
        if (shade) {   // the sub-rays as a one-row canvas of m k² pixels
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = shade_launch<R>(ShadeArgs<R>{d_sub, o2.hit32, o2.status, (const R*)o2.state_end, m * kk, m * kk, *shade}, st))) return rc;
        }
        if (emit) {    // … each emitted from its own sub-ray state
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = emit_launch<R>(EmitArgs<R>{d_sub, nullptr, nullptr, nullptr, o2.hit32, (const R*)o2.state_end, d_states, m * kk, m * kk, 1, 0, 0, sc, cm, *emit}, st))) return rc;
        }
        {
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = aa_reduce<R>(d_sub, d_list + first, m, k, d_rgb, n, st))) return rc;
        }
    }
    if (ctr) {
        HIP_TRY(hipMemcpyAsync(ctr, d_ctr, sizeof *ctr, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (stats) { stats->pixels = n; stats->refined = count; stats->sub_rays = count * kk; stats->batches = batches; }
    return RTGR_OK;
}

template <class R>
int api::trace_aa_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                         const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats,
                         void* stream) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (!d_rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if ((rc = aa_check(scene, cam, aa, ni, nj))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_aa_on<R>(*D, scene, opt, cam, ni, nj, aa, d_rgb, out, d_refined, ctr, stats, (hipStream_t)stream, nullptr);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream, and the frame copied out
template <class R>
int api::trace_aa(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                  const rtgr_aa* aa, R* rgb, const rtgr_ray_outputs* out, uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats) {
    rtgr_context* c = nullptr;
    int rc = resolve_ctx(ctx, &c);
    if (rc) return rc;
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    if ((rc = aa_check(scene, cam, aa, ni, nj))) return rc;
    if ((rc = check_redshift_outputs(out))) return rc;
    DeviceCtx& D = *c->devs[0];
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    Staging* S = nullptr;
    { std::lock_guard<std::mutex> lk(D.mu); if ((rc = staging_of(D, &S))) return rc; }
    std::lock_guard<std::mutex> call_lock(S->mu);
    HIP_TRY(hipStreamSynchronize(S->s_comp));   // (a previous call that failed half-way; the stream is idle otherwise)
    const uint64_t n = ni * nj;
    std::vector<RayArray> arrs = ray_arrays(rgb, out, sizeof(R));
    const size_t off_refined = ray_arrays_layout(arrs, n);
    if ((rc = S->d_out.need(off_refined + (refined ? align256(n) : 0)))) return rc;
    char* base = (char*)S->d_out.p;
    const rtgr_ray_outputs o = ray_outputs_at(base, arrs, out);
    uint8_t* d_refined = refined ? (uint8_t*)(base + off_refined) : nullptr;
    if ((rc = trace_aa_on<R>(D, scene, opt, cam, ni, nj, aa, (R*)(base + arrs[0].off), out ? &o : nullptr, d_refined, ctr, stats, S->s_comp, nullptr))) {
        (void)hipStreamSynchronize(S->s_comp);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(S->s_comp));
    for (const RayArray& a : arrs) HIP_TRY(hipMemcpy(a.ptr, base + a.off, (size_t)n * a.elem * a.planes, hipMemcpyDeviceToHost));
    if (refined) HIP_TRY(hipMemcpy(refined, d_refined, n, hipMemcpyDeviceToHost));
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(trace_aa_on);
RTGR_INSTANTIATE_F64_F32(api::trace_aa_device);
RTGR_INSTANTIATE_F64_F32(api::trace_aa);

}  // namespace rtgr
