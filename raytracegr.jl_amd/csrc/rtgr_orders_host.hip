// rtgr_orders_host.hip — higher-order disk images (include/rtgr.h "higher-order disk images"): the checks of an rtgr_disk_orders, the
// chain of legs — leg 0 as the observer trace runs it, then per order a crossing leg in the one-object scene of the inflated disk and a
// continuation leg in the caller's scene, each a plain trace_device of caller-supplied states, the post-trace stage of
// rtgr_frame_host.hip behind every leg in the caller's scene — and the entry points.  Host code only: the legs' kernels are the
// trace's, the emission kernel is rtgr_emit.hip's, the four small kernels in between are rtgr_orders.hip's.
#include "rtgr_internal.hpp"
#include "rtgr_orders.hpp"

namespace rtgr {

constexpr uint64_t ORDERS_DEFAULT_BATCH = 1ull << 22;   // rays per chunk of a leg (rtgr_observer.max_batch_rays = 0, or no observer)
constexpr EntryWords ORDERS_WORDS = {"rtgr_trace_orders_*", "orders", true};
constexpr const char* ORDERS_CANVAS = "a frame of disk orders";

// what the checks leave behind: N, and the scene S+ of the crossing legs
struct OrdersPlan {
    uint32_t N = 0;
    rtgr_scene plus;
};

// every refusal the arguments deserve, and the records the kernels read; touches no device
template <class R>
static int orders_resolve(const rtgr_scene* scene, const rtgr_observer* obs, const R* state0, uint64_t ni, uint64_t nj, const rtgr_shade* shade,
                          const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, const R* rgb, OrdersPlan& plan, DevObserver<R>& ob,
                          DevEmission<R>& em) {
    if (!scene) return fail(RTGR_ERR_BAD_ARG, "scene is NULL");
    if (!ord) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders is NULL (ord)");
    if (!emit) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_emission is NULL (emit)");
    if (!obs && !state0) return fail(RTGR_ERR_BAD_ARG, "rtgr_observer is NULL (obs) and so is state0: rtgr_trace_orders_* needs one of them");
    if (!rgb) return fail(RTGR_ERR_BAD_ARG, "rgb is NULL");
    int rc;
    if ((rc = canvas_check(ni, nj, ORDERS_CANVAS))) return rc;
    if (obs && (rc = observer_resolve<R>(scene, obs, ob))) return rc;
    if ((rc = emission_resolve<R>(scene, shade, emit, em))) return rc;
    if (ord->max_order == 0 || ord->max_order > RTGR_MAX_DISK_ORDER)
        return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders.max_order must be 1.." + std::to_string(RTGR_MAX_DISK_ORDER) + ", got " + std::to_string(ord->max_order));
    if (ord->flags != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders.flags must be 0");
    if (ord->pad != 0) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders.pad must be 0");
    if (!(ord->transmission >= 0.0 && ord->transmission <= 1.0))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders.transmission must lie in [0, 1] (and not be NaN)");
    const rtgr_object& disk = scene_objects(scene)[emit->object - 1];   // (a Disk: emission_resolve)
    const double h = disk.p[0], r_in = disk.p[1], r_out = disk.p[2];
    const double eta = ord->margin == 0.0 ? 0.5 * h : ord->margin;
    if (!std::isfinite(eta)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders.margin must be finite");
    if (!(eta > 0.0)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders.margin must be > 0 (0 means half the disk's half thickness, which is not > 0 here)");
    if (!(eta < r_in)) return fail(RTGR_ERR_BAD_ARG, "rtgr_disk_orders.margin must be < r_in of the emitting disk (the inflated disk keeps a hole)");
    plan.N = ord->max_order;
    std::memset(&plan.plus, 0, sizeof plan.plus);
    plan.plus.metric = scene->metric; plan.plus.M = scene->M; plan.plus.a = scene->a; plan.plus.user_metric = scene->user_metric;
    plan.plus.nobj = 1;
    plan.plus.obj[0].kind = RTGR_DISK;
    plan.plus.obj[0].p[0] = h + eta; plan.plus.obj[0].p[1] = r_in - eta; plan.plus.obj[0].p[2] = r_out + eta;
    return RTGR_OK;
}

// one leg: m rays from d_states (m x 8) through `scene`, in chunks of at most `budget`, into compact arrays m long (colour planes m apart)
template <class R>
static int orders_leg(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const R* d_states, uint64_t m, uint64_t budget, R* d_rgb,
                      const rtgr_ray_outputs& o, rtgr_counters* d_ctr, hipStream_t st) {
    int rc;
    for (uint64_t first = 0; first < m; first += budget) {
        const uint64_t c = m - first < budget ? m - first : budget;
        Window win;
        win.plane_stride = m; win.out_offset = first;
        if ((rc = trace_device<R>(D, scene, opt, d_states + first * 8, nullptr, c, 1, 0, 1, d_rgb, &o, d_ctr, st, 1, 0, c < m ? &win : nullptr))) return rc;
    }
    return RTGR_OK;
}

// the call on device D, stream st; d_state0, d_rgb and the members of `planes` are pointers of that device
template <class R>
static int trace_orders_on(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, const R* d_state0, uint64_t ni,
                           uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, R* d_rgb,
                           const rtgr_order_planes* planes, rtgr_counters* ctr, hipStream_t st) {
    int rc;
    OrdersPlan plan;
    DevObserver<R> ob;
    DevEmission<R> em;
    if ((rc = orders_resolve<R>(scene, obs, d_state0, ni, nj, shade, emit, ord, d_rgb, plan, ob, em))) return rc;
    ShadeDesc<R> sd;
    sd.nbind = 0;
    if (shade && (rc = shade_resolve<R>(D, scene, shade, sd))) return rc;
    AfterTrace<R> after;
    after.shade = sd.nbind ? &sd : nullptr;
    after.emit = &em;
    DeviceGuard guard(D.dev);
    if (!guard.ok) return fail(RTGR_ERR_HIP, "hipSetDevice failed");
    if (stream_capturing(st))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_trace_orders_*: the stream is being captured, and the call must read the length of each leg's list back "
                                      "(a synchronisation cannot be captured)");
    const uint64_t n = ni * nj, N = plan.N;
    rtgr_order_planes pl;
    std::memset(&pl, 0, sizeof pl);
    if (planes) pl = *planes;
    const uint64_t budget = obs && obs->max_batch_rays ? obs->max_batch_rays : ORDERS_DEFAULT_BATCH;

    // ---- frame scratch: the counters and the list length, the observer's record, the two index lists of leg 0, and what the caller did
    // not ask for of leg 0's end states, hit map and status bytes and of the start states ------------------------------------------------
    FrameNeeds need;
    need.obs = obs != nullptr;
    need.list = need.orders = true;
    need.state_end = !pl.state_end;
    need.hit32 = !pl.hit32;
    need.status = after.shade != nullptr;
    need.orders_state0 = !d_state0 && !pl.state0;
    rtgr_ray_outputs o0;
    std::memset(&o0, 0, sizeof o0);
    o0.state_end = pl.state_end; o0.hit32 = pl.hit32;
    DevScene<R> sc;
    FrameScratch fs;
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if ((rc = stationary_scene<R>(D, scene, sc, st, EMISSION_NEEDS_STATIONARY))) return rc;
        if ((rc = frame_scratch(D, st, false, ORDERS_WORDS, n, sizeof(R), need, 0, &o0, ctr, fs))) return rc;
    }
    StreamState* ss = fs.ss;
    unsigned long long* d_count = (unsigned long long*)(fs.base + sizeof(rtgr_counters));   // (zeroed with the head)
    uint64_t* d_slot0 = (uint64_t*)(fs.base + fs.at.list);
    uint64_t* d_pix0 = (uint64_t*)(fs.base + fs.at.orders_list);
    ObsFrame<R>* d_frame = obs ? (ObsFrame<R>*)(fs.base + fs.at.obs) : nullptr;
    const rtgr_ray_outputs& o1 = fs.o1;

    // ---- the start states: the caller's, or the observer's own (the frame kernel, then the ray kernel over the whole canvas) -------------
    if (obs) {
        std::lock_guard<std::mutex> lk(D.mu);
        KernelTimer timer(D, st, 0);
        if ((rc = observer_frame_launch<R>(sc, ob, d_frame, st))) return rc;
    }
    const R* d_s0 = d_state0;
    if (!d_s0) {
        R* gen = pl.state0 ? (R*)pl.state0 : (R*)(fs.base + fs.at.orders_state0);
        std::lock_guard<std::mutex> lk(D.mu);
        KernelTimer timer(D, st, 0);
        if ((rc = observer_rays_launch<R>(d_frame, ni, nj, 0, n, gen, st))) return rc;
        d_s0 = gen;
    } else if (pl.state0) {
        HIP_TRY(hipMemcpyAsync(pl.state0, d_s0, (size_t)n * 8 * sizeof(R), hipMemcpyDeviceToDevice, st));
    }

    // ---- leg 0: the emitted observer frame, every pixel from its own start state ----------------------------------------------------------
    if ((rc = orders_leg<R>(D, scene, opt, d_s0, n, budget, d_rgb, o1, fs.d_ctr, st))) return rc;
    {
        TracedPixels<R> px;
        px.rgb = d_rgb; px.plane_stride = n; px.g = (R*)pl.g;
        px.hit32 = o1.hit32; px.status = o1.status; px.state_end = (const R*)o1.state_end;
        px.state0 = d_s0; px.obs = d_frame;
        px.n = n; px.ni = ni; px.nj = nj;
        px.sc = &sc;
        if ((rc = after_trace<R>(D, st, after, px))) return rc;
    }
    if (pl.rgb_order) HIP_TRY(hipMemcpyAsync(pl.rgb_order, d_rgb, (size_t)n * 3 * sizeof(R), hipMemcpyDeviceToDevice, st));
    OrdersSelectArgs S;
    std::memset(&S, 0, sizeof S);
    {   // blocks 1 .. N of the planes: "no such order" everywhere; and the continuing set of order 0
        OrdersFillArgs<R> F;
        F.hit32 = pl.hit32 ? pl.hit32 + n : nullptr;
        F.state_end = pl.state_end ? (R*)pl.state_end + n * 8 : nullptr;
        F.g = pl.g ? (R*)pl.g + n : nullptr;
        F.rgb_order = pl.rgb_order ? (R*)pl.rgb_order + n * 3 : nullptr;
        F.per = N * n;
        S.hit32 = o1.hit32; S.m_in = n; S.object = em.object;
        S.slot = d_slot0; S.pix = d_pix0; S.count = d_count; S.count_plane = pl.count;
        std::lock_guard<std::mutex> lk(D.mu);
        KernelTimer timer(D, st, 0);
        if ((rc = orders_fill_launch<R>(F, st))) return rc;
        if ((rc = orders_select_launch(S, st))) return rc;
    }
    // the length of the list just made, behind a synchronisation; the counter zeroed for the next one
    auto read_count = [&](uint64_t bound, uint64_t& m) -> int {
        unsigned long long count = 0;
        HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemsetAsync(d_count, 0, sizeof count, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (count > bound) return fail(RTGR_ERR_HIP, "rtgr_trace_orders_*: a list length read back exceeds the leg it was made from");
        m = count;
        return RTGR_OK;
    };
    uint64_t m = 0;
    if ((rc = read_count(n, m))) return rc;
    if (m == 0) return counters_back(fs, ctr, st);

    // ---- batch scratch: compact arrays for m rays — no later list is longer.  [pixels A] [pixels B] [slots] [states in] [end states]
    // [start states] [colours, 3 planes] [ratio] [hit32] [status] -----------------------------------------------------------------------------
    const size_t idx_bytes = align256((size_t)m * sizeof(uint64_t)), st_bytes = align256((size_t)m * 8 * sizeof(R));
    const size_t off_pa = 0, off_pb = off_pa + idx_bytes, off_slot = off_pb + idx_bytes, off_x = off_slot + idx_bytes, off_se = off_x + st_bytes,
                 off_s0 = off_se + st_bytes, off_rgb = off_s0 + st_bytes, off_g = off_rgb + align256((size_t)m * 3 * sizeof(R)),
                 off_hit = off_g + align256((size_t)m * sizeof(R)), off_status = off_hit + align256((size_t)m * sizeof(uint32_t)),
                 batch_bytes = off_status + align256((size_t)m);
    {
        std::lock_guard<std::mutex> lk(D.mu);
        if ((rc = scratch_need(*ss, ss->batch, ss->batch_bytes, batch_bytes))) return rc;
    }
    char* B = (char*)ss->batch;
    uint64_t* d_pa = (uint64_t*)(B + off_pa);
    uint64_t* d_pb = (uint64_t*)(B + off_pb);
    uint64_t* d_slot = (uint64_t*)(B + off_slot);
    R* d_x = (R*)(B + off_x);
    R* d_se = (R*)(B + off_se);
    R* d_s0c = (R*)(B + off_s0);
    R* d_col = (R*)(B + off_rgb);
    R* d_g = (R*)(B + off_g);
    rtgr_ray_outputs oc;
    std::memset(&oc, 0, sizeof oc);
    oc.state_end = d_se; oc.hit32 = (uint32_t*)(B + off_hit); oc.status = (uint8_t*)(B + off_status);

    // ---- order by order.  In: the list (src_slot, src_pix) of m rays that ended on the disk at order k - 1, their end states in src_se ------
    const uint64_t* src_slot = d_slot0;
    const uint64_t* src_pix = d_pix0;
    const R* src_se = (const R*)o1.state_end;
    const R T = (R)ord->transmission;
    R t = T;
    for (uint64_t k = 1; k <= N && m; k++) {
        {
            OrdersGatherArgs<R> G{src_se, src_slot, m, d_x};
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = orders_gather_launch<R>(G, st))) return rc;
        }
        // the crossing leg: from the surface of D, inside D+, to the surface of D+
        if ((rc = orders_leg<R>(D, &plan.plus, opt, d_x, m, budget, d_col, oc, fs.d_ctr, st))) return rc;
        {
            S.hit32 = oc.hit32; S.status = oc.status; S.src_pix = src_pix; S.m_in = m; S.object = 1; S.need_event = 1;
            S.slot = d_slot; S.pix = d_pb; S.count_plane = nullptr;
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = orders_select_launch(S, st))) return rc;
        }
        uint64_t mb = 0;
        if ((rc = read_count(m, mb))) return rc;
        if (mb == 0) break;
        {
            OrdersGatherArgs<R> G{d_se, d_slot, mb, d_x};
            OrdersGatherArgs<R> G0{d_s0, d_pb, mb, d_s0c};
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = orders_gather_launch<R>(G, st))) return rc;
            if ((rc = orders_gather_launch<R>(G0, st))) return rc;
        }
        // the continuation leg in the caller's scene, shaded and emitted like any frame: each ray from its pixel's own start state
        if ((rc = orders_leg<R>(D, scene, opt, d_x, mb, budget, d_col, oc, fs.d_ctr, st))) return rc;
        {
            TracedPixels<R> sub;
            sub.rgb = d_col; sub.plane_stride = mb; sub.g = d_g;
            sub.hit32 = oc.hit32; sub.status = oc.status; sub.state_end = d_se;
            sub.state0 = d_s0c; sub.obs = d_frame;
            sub.n = mb;
            sub.sc = &sc;
            if ((rc = after_trace<R>(D, st, after, sub))) return rc;
        }
        {
            OrdersScatterArgs<R> C;
            std::memset(&C, 0, sizeof C);
            C.pix = d_pb; C.hit32 = oc.hit32; C.state_end = d_se; C.g = d_g; C.rgb_leg = d_col;
            C.m = mb; C.n = n; C.object = em.object; C.t = t;
            C.rgb = d_rgb; C.count = pl.count;
            C.hit32_k = pl.hit32 ? pl.hit32 + k * n : nullptr;
            C.state_end_k = pl.state_end ? (R*)pl.state_end + k * n * 8 : nullptr;
            C.g_k = pl.g ? (R*)pl.g + k * n : nullptr;
            C.rgb_order_k = pl.rgb_order ? (R*)pl.rgb_order + k * n * 3 : nullptr;
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = orders_scatter_launch<R>(C, st))) return rc;
        }
        t = t * T;
        if (k == N) break;   // a pixel that still continues after order N stops there
        {
            S.hit32 = oc.hit32; S.status = nullptr; S.src_pix = d_pb; S.m_in = mb; S.object = em.object; S.need_event = 0;
            S.slot = d_slot; S.pix = d_pa;
            std::lock_guard<std::mutex> lk(D.mu);
            KernelTimer timer(D, st, 0);
            if ((rc = orders_select_launch(S, st))) return rc;
        }
        if ((rc = read_count(mb, m))) return rc;
        src_slot = d_slot; src_pix = d_pa; src_se = d_se;
    }
    return counters_back(fs, ctr, st);
}

template <class R>
int api::trace_orders_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, const R* d_state0, uint64_t ni,
                             uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, R* d_rgb,
                             const rtgr_order_planes* planes, rtgr_counters* ctr, void* stream) {
    RESOLVE_CONTEXT();
    OrdersPlan plan;
    DevObserver<R> ob;
    DevEmission<R> em;
    if ((rc = orders_resolve<R>(scene, obs, d_state0, ni, nj, shade, emit, ord, d_rgb, plan, ob, em))) return rc;
    DeviceCtx* D = nullptr;
    if ((rc = device_of(c, d_rgb, &D))) return rc;
    return trace_orders_on<R>(*D, scene, opt, obs, d_state0, ni, nj, shade, emit, ord, d_rgb, planes, ctr, (hipStream_t)stream);
}

// host pointers: the same call on device 0 of the context, on its staging's compute stream; the frame and the planes copied out
template <class R>
int api::trace_orders(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, const R* state0, uint64_t ni,
                      uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, R* rgb,
                      const rtgr_order_planes* planes, rtgr_counters* ctr) {
    RESOLVE_CONTEXT();
    OrdersPlan plan;
    DevObserver<R> ob;
    DevEmission<R> em;
    if ((rc = orders_resolve<R>(scene, obs, state0, ni, nj, shade, emit, ord, rgb, plan, ob, em))) return rc;
    const uint64_t n = ni * nj, blocks = plan.N + 1;
    rtgr_order_planes host;
    std::memset(&host, 0, sizeof host);
    if (planes) host = *planes;
    // the planes the caller asks for, in the order of rtgr_order_planes, then the start states given
    HostMirror m(c);
    rtgr_order_planes dev;
    dev.count = m.out(host.count, n); dev.hit32 = m.out(host.hit32, blocks * n); dev.state_end = m.out((R*)host.state_end, blocks * n * 8);
    dev.g = m.out((R*)host.g, blocks * n); dev.rgb_order = m.out((R*)host.rgb_order, blocks * n * 3); dev.state0 = m.out((R*)host.state0, n * 8);
    const R* d_state0 = m.in(state0, n * 8);
    if ((rc = m.status())) return rc;
    return staged_frame<R>(c, n, rgb, nullptr, nullptr, nullptr, [&](DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs*, uint8_t*, R*, hipStream_t st) {
        int r = trace_orders_on<R>(D, scene, opt, obs, d_state0, ni, nj, shade, emit, ord, d_rgb, planes ? &dev : nullptr, ctr, st);
        return r ? r : m.fetch(st);
    });
}

RTGR_INSTANTIATE_F64_F32(api::trace_orders_device);
RTGR_INSTANTIATE_F64_F32(api::trace_orders);

}  // namespace rtgr
