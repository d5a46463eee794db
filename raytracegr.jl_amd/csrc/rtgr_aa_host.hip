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
constexpr EntryWords AA_WORDS = {"rtgr_trace_aa_*", "anti-aliasing", true};

static int aa_check(const rtgr_scene* scene, const rtgr_camera* cam, const rtgr_aa* aa, uint64_t ni, uint64_t nj) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!aa) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa is NULL");
    if (aa->k < 2 || aa->k > 8) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa.k must be 2..8 (k x k sub-rays per refined pixel), got " + std::to_string(aa->k));
    if (aa->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa.flags must be 0");
    if (aa->contrast != aa->contrast) return fail(RTGR_ERR_BAD_ARG, "rtgr_aa.contrast is NaN (< 0: every pixel, +Inf: class edges only)");
    if (!cam) return fail(RTGR_ERR_BAD_ARG, "anti-aliasing needs a camera (cam is NULL): the sub-rays are generated from it");
    int rc;
    if ((rc = builtin_metric_check(scene, "anti-aliasing of", "its camera kernel lives"))) return rc;
    return canvas_check(ni, nj, "an anti-aliased frame");
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
    if (stream_capturing(st))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_aa_*: the stream is being captured, and the call must read the number of refined pixels back "
                                      "between its two passes (a synchronisation cannot be captured)");
    const uint64_t n = ni * nj;
    const uint32_t k = aa->k, kk = k * k;
    const AfterTrace<R> none;
    const AfterTrace<R>& aft = after ? *after : none;
    const bool post = aft.shade || aft.emit;

    // ---- frame scratch: the counters and the refined count, the list, and what the caller did not ask for of the hit map and the status
    // bytes the edge rule reads — and of the end states the shading and emission kernels read --------------------------------------------------
    FrameNeeds need;
    need.list = true;
    need.hit32 = !(out && out->hit32);
    need.status = !(out && out->status);
    need.state_end = post && !(out && out->state_end);
    FrameScratch fs;
    DevScene<R> sc;
    DevCamera<R> cm;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if ((rc = frame_scratch(D, st, false, AA_WORDS, n, sizeof(R), need, 0, out, ctr, fs))) return rc;
    }
    StreamState* ss = fs.ss;
    unsigned long long* d_count = (unsigned long long*)(fs.base + sizeof(rtgr_counters));
    uint64_t* d_list = (uint64_t*)(fs.base + fs.at.list);
    const rtgr_ray_outputs& o1 = fs.o1;

    // ---- pass 1: the plain frame, with the hit map and the status bytes the edge rule reads --------------------------------------
    if ((rc = trace_device<R>(D, scene, opt, nullptr, cam, ni, nj, 0, nj, d_rgb, &o1, fs.d_ctr, st))) return rc;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        const UserModule* user = nullptr;
        if ((rc = convert_scene<R>(D, scene, sc, &user, st))) return rc;   // (what the sub-ray and emission kernels read of the scene: its metric)
        convert_camera<R>(cam, cm);
    }
    TracedPixels<R> px;   // the edge rule reads the SHADED and EMITTED colours; the pixel-centre rays start from the camera's own pixels
    px.rgb = d_rgb; px.plane_stride = n; px.g = aft.d_g;
    px.hit32 = o1.hit32; px.status = o1.status; px.state_end = (const R*)o1.state_end;
    px.n = n; px.ni = ni; px.nj = nj;
    px.sc = &sc; px.cam = &cm;
    if (post && (rc = after_trace<R>(D, st, aft, px))) return rc;

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
        if ((rc = scratch_need(*ss, ss->batch, ss->batch_bytes, batch_bytes))) return rc;
    }
    for (uint64_t b = 0; b < batches; b++) {
        const uint64_t first = b * per, m = count - first < per ? count - first : per;
        R* d_states = (R*)ss->batch;
        R* d_sub = (R*)((char*)ss->batch + off_sub);
        {
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = aa_subrays<R>(sc, cm, ni, nj, k, d_list + first, m, d_states, st))) return rc;
        }
        rtgr_ray_outputs o2;
        std::memset(&o2, 0, sizeof o2);
        if (post) {
            o2.state_end = (char*)ss->batch + off_end;
            o2.hit32 = (uint32_t*)((char*)ss->batch + off_hit2);
            o2.status = (uint8_t*)((char*)ss->batch + off_status2);
        }
        if ((rc = trace_device<R>(D, scene, opt, d_states, nullptr, m * kk, 1, 0, 1, d_sub, post ? &o2 : nullptr, fs.d_ctr, st))) return rc;
        if (post) {   // the sub-rays as a one-row canvas of m k² pixels, each emitted from its own sub-ray state
            TracedPixels<R> sub;
            sub.rgb = d_sub; sub.plane_stride = m * kk;
            sub.hit32 = o2.hit32; sub.status = o2.status; sub.state_end = (const R*)o2.state_end;
            sub.state0 = d_states;
            sub.n = m * kk;
            sub.sc = &sc; sub.cam = &cm;
            if ((rc = after_trace<R>(D, st, aft, sub))) return rc;
        }
        {
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = aa_reduce<R>(d_sub, d_list + first, m, k, d_rgb, n, st))) return rc;
        }
    }
    if ((rc = counters_back(fs, ctr, st))) return rc;
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
    return staged_frame<R>(c, ni * nj, rgb, out, refined, nullptr, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t* d_refined, R*, hipStream_t st) {
        return trace_aa_on<R>(D, scene, opt, cam, ni, nj, aa, d_rgb, d_out, d_refined, ctr, stats, st, nullptr);
    });
}
RTGR_INSTANTIATE_F64_F32(trace_aa_on);
RTGR_INSTANTIATE_F64_F32(api::trace_aa_device);
RTGR_INSTANTIATE_F64_F32(api::trace_aa);

}  // namespace rtgr
