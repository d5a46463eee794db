// rtgr_frame_host.hip — what the frame calls share (rtgr_aa_host.hip, rtgr_texture_host.hip, rtgr_emission_host.hip, rtgr_observer_host.hip):
// a stream's frame scratch, the post-trace stage — the textures, then the emitting disk, applied to the pixels a trace just wrote — the
// camera frame of rtgr_trace_shaded_* / rtgr_trace_emission_*, the staged call behind every host-pointer frame entry, and the small checks
// they all make.  Host code only: the kernels are rtgr_shade.hip's and rtgr_emit.hip's.
#include "rtgr_internal.hpp"

namespace rtgr {

// ---- the small checks --------------------------------------------------------------------------------------------------------------
int canvas_check(uint64_t ni, uint64_t nj, const char* what) {
    if (ni == 0 || nj == 0 || ni > (1ull << 32) || nj > (1ull << 32) || ni * nj > (1ull << 34))
        return fail(RTGR_ERR_BAD_ARG, std::string("bad canvas: need ni, nj > 0 and at most 2^34 pixels for ") + what);
    return RTGR_OK;
}

int builtin_metric_check(const rtgr_scene* scene, const char* what, const char* why) {
    if ((scene->metric & ~(uint32_t)RTGR_METRIC_GENERIC) == RTGR_USER)
        return fail(RTGR_ERR_BAD_ARG, std::string(what) + " a scene whose METRIC is RTGR_USER is not supported (" + why +
                                      " in the run-time unit); user objects under a built-in metric are");
    return RTGR_OK;
}

template <class R>
int stationary_scene(DeviceCtx& D, const rtgr_scene* scene, DevScene<R>& sc, hipStream_t st, const char* refusal) {
    const UserModule* user = nullptr;
    int rc;
    if ((rc = convert_scene<R>(D, scene, sc, &user, st))) return rc;
    if (sampled_on(sc.metric, 4)) return fail(RTGR_ERR_BAD_ARG, refusal);
    return RTGR_OK;
}

// ---- the frame scratch of a stream ---------------------------------------------------------------------------------------------------
int scratch_need(StreamState& ss, void*& p, size_t& have, size_t bytes) {
    if (bytes <= have) return RTGR_OK;
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, bytes));
    if (p) ss.retired.push_back(p);   // kernels of an earlier call may still be in flight on it, a graph captured earlier may replay it
    p = q;
    have = bytes;
    return RTGR_OK;
}

int capture_check(hipStream_t st, const EntryWords& who, const rtgr_counters* ctr, bool* capturing) {
    *capturing = stream_capturing(st);
    if (*capturing && ctr)
        return fail(RTGR_ERR_BAD_ARG, std::string(who.entry) + ": the stream is being captured and `ctr` asks for a synchronisation at the end of the call "
                                      "(which cannot be captured): pass ctr = NULL");
    return RTGR_OK;
}

int frame_scratch(DeviceCtx& D, hipStream_t st, bool capturing, const EntryWords& who, uint64_t n, size_t scalar, const FrameNeeds& need,
                  size_t batch_bytes, const rtgr_ray_outputs* out, const rtgr_counters* ctr, FrameScratch& fs) {
    int rc;
    fs.at = frame_layout(n, scalar, need);
    if (out) fs.o1 = *out; else std::memset(&fs.o1, 0, sizeof fs.o1);
    if (!ctr && fs.at.bytes == FRAME_HEAD && batch_bytes == 0) return RTGR_OK;   // nothing to count, to keep or to borrow
    if ((rc = stream_state(D, st, &fs.ss))) return rc;
    StreamState& ss = *fs.ss;
    if (capturing && (fs.at.bytes > ss.frame_bytes || batch_bytes > ss.batch_bytes))
        return fail(RTGR_ERR_BAD_ARG, std::string(who.entry) + ": the stream's " + who.scratch + " scratch must grow but the stream is being captured" +
                                      (who.advise ? ": make a call of this size on the stream before hipStreamBeginCapture" : ""));
    if ((rc = scratch_need(ss, ss.frame, ss.frame_bytes, fs.at.bytes))) return rc;
    if ((rc = scratch_need(ss, ss.batch, ss.batch_bytes, batch_bytes))) return rc;
    fs.base = (char*)ss.frame;
    if (need.state_end) fs.o1.state_end = fs.base + fs.at.state_end;
    if (need.hit32) fs.o1.hit32 = (uint32_t*)(fs.base + fs.at.hit32);
    if (need.status) fs.o1.status = (uint8_t*)(fs.base + fs.at.status);
    if (need.lambda_end) fs.o1.lambda_end = fs.base + fs.at.lambda_end;
    if (ctr) fs.d_ctr = (rtgr_counters*)fs.base;
    if (ctr || need.list) HIP_TRY(hipMemsetAsync(fs.base, 0, FRAME_HEAD, st));
    return RTGR_OK;
}

int counters_back(const FrameScratch& fs, rtgr_counters* ctr, hipStream_t st) {
    if (!ctr) return RTGR_OK;
    HIP_TRY(hipMemcpyAsync(ctr, fs.d_ctr, sizeof *ctr, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RTGR_OK;
}

// ---- the post-trace stage -------------------------------------------------------------------------------------------------------------
template <class R>
int after_trace(DeviceCtx& D, hipStream_t st, const AfterTrace<R>& after, const TracedPixels<R>& px) {
    int rc;
    std::lock_guard<std::mutex> lk(D.mu);
    if (after.shade) {
        KernelTimer timer(D, st, 0);
        ShadeArgs<R> A;
        A.rgb = px.rgb; A.hit32 = px.hit32; A.status = px.status; A.state_end = px.state_end;
        A.n = px.n; A.plane_stride = px.plane_stride;
        A.desc = *after.shade;
        if ((rc = shade_launch<R>(A, st))) return rc;
    }
    if (after.emit) {   // frame mode: no omega, no u_emit, one colour per pixel of a plane
        KernelTimer timer(D, st, 0);
        EmitArgs<R> E;
        std::memset(&E, 0, sizeof E);
        E.rgb = px.rgb; E.g = px.g; E.hit32 = px.hit32; E.state_end = px.state_end; E.state0 = px.state0; E.obs = px.obs;
        E.n = px.n; E.plane_stride = px.plane_stride; E.pixel_stride = 1; E.ni = px.ni; E.nj = px.nj;
        E.sc = *px.sc;
        if (px.cam) E.cam = *px.cam;
        E.em = *after.emit;
        if ((rc = emit_launch<R>(E, st))) return rc;
    }
    return RTGR_OK;
}

// ---- the camera frame of rtgr_trace_shaded_* and rtgr_trace_emission_* ---------------------------------------------------------------------
template <class R>
int trace_camera_frame_on(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                          const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, R* d_g,
                          uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, hipStream_t st, const EntryWords& who) {
    int rc;
    if ((rc = shaded_check(cam, aa, d_refined, stats, ni, nj))) return rc;
    if ((rc = check_redshift_outputs(out))) return rc;
    DevEmission<R> em;
    if (emit && (rc = emission_resolve<R>(scene, shade, emit, em))) return rc;
    ShadeDesc<R> sd;
    sd.nbind = 0;
    if ((shade || !emit) && (rc = shade_resolve<R>(D, scene, shade, sd))) return rc;   // (a shaded frame needs its rtgr_shade)
    AfterTrace<R> after;
    after.shade = sd.nbind ? &sd : nullptr;
    after.emit = emit ? &em : nullptr;
    after.d_g = d_g;
    const bool post = after.shade || after.emit;
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    DevScene<R> sc;
    DevCamera<R> cm;
    if (aa) {
        if (emit) {   // (a time-dependent grid has no stationary emitter)
            std::lock_guard<std::mutex> lk(D.mu);
            if ((rc = stationary_scene<R>(D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
        }
        return trace_aa_on<R>(D, scene, opt, cam, ni, nj, aa, d_rgb, out, d_refined, ctr, stats, st, post ? &after : nullptr);
    }
    bool capturing;
    if ((rc = capture_check(st, who, ctr, &capturing))) return rc;
    // ---- the plain frame, with what the shading and emission kernels read of it: both the end states and the hit map, the shading
    // kernel also the status bytes -----------------------------------------------------------------------------------------------------
    const uint64_t n = ni * nj;
    FrameNeeds need;
    need.state_end = post && !(out && out->state_end);
    need.hit32 = post && !(out && out->hit32);
    need.status = after.shade && !(out && out->status);
    FrameScratch fs;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if (emit) {
            if ((rc = stationary_scene<R>(D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
            convert_camera<R>(cam, cm);
        }
        if ((rc = frame_scratch(D, st, capturing, who, n, sizeof(R), need, 0, out, ctr, fs))) return rc;
    }
    if ((rc = trace_device<R>(D, scene, opt, nullptr, cam, ni, nj, 0, nj, d_rgb, (out || post) ? &fs.o1 : nullptr, fs.d_ctr, st))) return rc;
    if (post) {
        TracedPixels<R> px;
        px.rgb = d_rgb; px.plane_stride = n; px.g = d_g;
        px.hit32 = fs.o1.hit32; px.status = fs.o1.status; px.state_end = (const R*)fs.o1.state_end;
        px.n = n; px.ni = ni; px.nj = nj;
        if (emit) { px.sc = &sc; px.cam = &cm; }
        if ((rc = after_trace<R>(D, st, after, px))) return rc;
    }
    return counters_back(fs, ctr, st);
}

// ---- host pointers: a frame call on device 0 of the context, on its staging's compute stream, and the frame copied out ----------------
template <class R>
int staged_frame(rtgr_context* c, uint64_t n, R* rgb, const rtgr_ray_outputs* out, uint8_t* refined, R* g, const StagedCall<R>& call) {
    int rc;
    DeviceCtx& D = *c->devs[0];
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    Staging* S = nullptr;
    { std::lock_guard<std::mutex> lk(D.mu); if ((rc = staging_of(D, &S))) return rc; }
    std::lock_guard<std::mutex> call_lock(S->mu);
    HIP_TRY(hipStreamSynchronize(S->s_comp));   // (a previous call that failed half-way; the stream is idle otherwise)
    std::vector<RayArray> arrs = ray_arrays(rgb, out, sizeof(R));
    const size_t off_refined = ray_arrays_layout(arrs, n);
    const size_t off_g = off_refined + (refined ? align256(n) : 0);
    if ((rc = S->d_out.need(off_g + (g ? align256(n * sizeof(R)) : 0)))) return rc;
    char* base = (char*)S->d_out.p;
    const rtgr_ray_outputs o = ray_outputs_at(base, arrs, out);
    uint8_t* d_refined = refined ? (uint8_t*)(base + off_refined) : nullptr;
    R* d_g = g ? (R*)(base + off_g) : nullptr;
    if ((rc = call(D, (R*)(base + arrs[0].off), out ? &o : nullptr, d_refined, d_g, S->s_comp))) {
        (void)hipStreamSynchronize(S->s_comp);
        return rc;
    }
    HIP_TRY(hipStreamSynchronize(S->s_comp));
    for (const RayArray& a : arrs) HIP_TRY(hipMemcpy(a.ptr, base + a.off, (size_t)n * a.elem * a.planes, hipMemcpyDeviceToHost));
    if (refined) HIP_TRY(hipMemcpy(refined, d_refined, n, hipMemcpyDeviceToHost));
    if (g) HIP_TRY(hipMemcpy(g, d_g, (size_t)n * sizeof(R), hipMemcpyDeviceToHost));
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(stationary_scene);
RTGR_INSTANTIATE_F64_F32(after_trace);
RTGR_INSTANTIATE_F64_F32(trace_camera_frame_on);
RTGR_INSTANTIATE_F64_F32(staged_frame);

}  // namespace rtgr
