// rtgr_internal.hpp — what the HOST translation units of librtgr_hip.so share (no kernel, no device code):
//
//   rtgr_context.hip        error plumbing, launch options, contexts and their per-device / per-stream state, the enqueue of one trace:
//                           dispatch to the kernels' translation units (tu_*.hip), the device entry points
//   rtgr_tables.hip         what a context keeps resident on its devices under one lifetime rule: the load / unload path of the tables
//                           named by an id (grid metrics, image textures), the tables of long object lists, the table-count test hooks
//   rtgr_scene_host.hip     argument conversion: a scene (its object list regrouped, the spheres of a long list in groups), a solver and a
//                           camera into what the kernels read
//   rtgr_grid.hip           metrics sampled on a grid: the checks of a load, the axes, the entry points
//   rtgr_host_pipeline.hip  the host-pointer entry points: pinned staging + a three-stream H2D / compute / D2H pipeline
//   rtgr_sharded.hip        one call over every device of a context: cyclic rows, peer copies to device 0
//   rtgr_hooks.hip          make_canvas and the parity hooks (rtgr_eval_*), image quantisation
//   rtgr_units.hip          run-time compiled units: build, audit, load-time probe, load, scene check
//   rtgr_frame_host.hip     what the frame calls below share: a stream's frame scratch, the post-trace stage (textures, then the emitting disk),
//                           the camera frame of rtgr_trace_shaded_* / rtgr_trace_emission_*, the staged host-pointer call, the small checks
//   rtgr_aa_host.hip        adaptive anti-aliasing: the plain frame, the edge rule, a sparse second trace (kernels: rtgr_aa.hip)
//   rtgr_texture_host.hip   image textures: load / unload, the binds of a call into the records the shading kernel reads, the entry points of the
//                           shaded trace, the sampler hook (kernels: rtgr_shade.hip)
//   rtgr_emission_host.hip  disk emission: the checks of an rtgr_disk_emission, the entry points of the emitted trace, the pointwise hook
//                           (kernels: rtgr_emit.hip)
//   rtgr_observer_host.hip  the observer camera: the checks of an rtgr_observer, the observer trace (the frame and ray kernels + a plain trace of
//                           their states, batch by batch, + the post-trace stage), the canvas and frame hooks (kernels: rtgr_observer.hip)
//   rtgr_reduce_host.hip    THE path from a traced frame of an emitting disk to a reduced table, for the two files below: the stream's
//                           reduction scratch, the pixel weight, the four bodies behind rtgr_<x>_device_*, rtgr_trace_<x>_device_* and
//                           rtgr_trace_<x>_* (a Reduction says what <x> is; kernels: rtgr_reduce.hpp, instantiated in the two kernel units)
//   rtgr_lightcurve_host.hip  hot-spot light curves: the checks of an rtgr_hot_spot, the stage (Omega_s from the emission kernel in point
//                           mode, then the reduction), the entry points as a Reduction each, the hook (kernels: rtgr_lightcurve.hip)
//   rtgr_spectrum_host.hip  disk spectra: the checks of an rtgr_spectrum, the stage, the entry points as a Reduction each, the hook
//                           (kernels: rtgr_spectrum.hip)
//   rtgr_polarization_host.hip  polarized disk images: the checks of an rtgr_polarization, the stage alone, the polarized observer trace,
//                           the two hooks (kernel: rtgr_polarize.hip)
//   rtgr_orders_host.hip    higher-order disk images: the checks of an rtgr_disk_orders, the chain of legs through the inflated disk and the
//                           caller's scene, the entry points (kernels: rtgr_orders.hip; argument blocks: rtgr_orders.hpp)
//   rtgr_transfer_host.hip  volume emission: the checks of an rtgr_flow, the observer trace with the transfer kernel behind each batch, the
//                           listed-ray and pointwise hooks (kernels: tu_transfer_f64.hip, tu_transfer_f32.hip; model: rtgr_transfer.hpp)
//   rtgr_abi.hip            the `extern "C"` symbols of include/rtgr.h, each a one-line shim onto rtgr::api::<name> (an _f64 / _f32
//                           pair: onto rtgr::api::<name><double> / <float>, defined and instantiated in the unit that holds the code)
//
// Everything here is internal to the library: nothing in this header crosses the C ABI.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <limits>
#include <thread>

#include "rtgr_host.hpp"

namespace rtgr {

// ---- staging of the host-pointer entry points and of the multi-device path (one per DeviceCtx, created on first use) ----------
struct PinnedBuf {
    void* p = nullptr; size_t bytes = 0;
    int need(size_t b) {
        if (b <= bytes) return RTGR_OK;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        HIP_TRY(hipHostMalloc(&p, b, hipHostMallocDefault));
        bytes = b;
        return RTGR_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; bytes = 0; }
};
struct DevBufG {  // grow-only device buffer
    void* p = nullptr; size_t bytes = 0;
    int need(size_t b) {
        if (b <= bytes) return RTGR_OK;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }  // only called with the owning streams idle
        HIP_TRY(hipMalloc(&p, b));
        bytes = b;
        return RTGR_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

// staging of the host-pointer entry points and of the multi-device path (one per DeviceCtx, created on first use)
struct Staging {
    hipStream_t s_up = nullptr, s_comp = nullptr, s_down = nullptr;
    static constexpr int IN_SLOTS = 3, OUT_SLOTS = 2;
    PinnedBuf pin_in[IN_SLOTS], pin_out[OUT_SLOTS], pin_small;
    hipEvent_t ev_in[IN_SLOTS] = {nullptr, nullptr, nullptr};
    DevBufG d_in, d_out, d_small;  // device-side inputs (ray states), outputs (all requested arrays), counters + flags
    DevBufG d_recv;                // device 0 of a multi-device context: rows received from the peers
    std::mutex mu;                 // one host-pointer call at a time per device (they share the staging buffers)
};
void staging_delete(Staging* s);

}  // namespace rtgr

struct rtgr_context {
    std::vector<std::unique_ptr<rtgr::DeviceCtx>> devs;
    // peer access device 0 <-> device k, established by rtgr_create: 1 = enabled both ways (or the same physical device),
    // 0 = not available, with the reason (the multi-device gather then stages through pinned host memory, or fails when the
    // option peer = 1 requires peer copies)
    std::vector<char> peer_ok;
    std::vector<std::string> peer_why;
    std::mutex modules_mu;   // run-time metric modules are loaded / unloaded on all devices under ONE lock
    // rtgr_user_unit_compile: hash of (source, what it is built for, device headers) -> id of the unit it gave; the same call again is
    // answered from here while that unit is resident (a C or Julia caller need not keep a table of its own to avoid a 5 s rebuild)
    std::mutex compiled_mu;
    std::unordered_map<uint64_t, uint64_t> compiled;
};

namespace rtgr {

struct DeviceGuard {  // the calling thread's current device is restored on scope exit
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = (prev == dev) || hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// ---- contexts (rtgr_context.hip) -------------------------------------------------------------------------------------------
extern std::mutex g_default_mu;      // guards g_default
extern rtgr_context* g_default;      // the process's default context (ctx == NULL), created on first use
const std::string& last_error_string();   // the calling thread's last failure message
int staging_of(DeviceCtx& d, Staging** out, int slot = 0);   // slot 1: the second frame in flight (rtgr_trace_frames_*)
void free_device_state(DeviceCtx& d, bool all);
int create_context(const int* ids, int n, rtgr_context** out);
void destroy_context(rtgr_context* c);
int resolve_ctx(rtgr_context* in, rtgr_context** out);   // ctx == NULL: the default context
int device_of(rtgr_context* c, const void* d_ptr, DeviceCtx** out);
int stream_state(DeviceCtx& d, hipStream_t st, StreamState** out);
int collect_timed(DeviceCtx& d);
uint64_t fnv1a(const std::vector<char>& b);

#define RESOLVE_CONTEXT()                            \
    rtgr_context* c = nullptr;                       \
    int rc = resolve_ctx(ctx, &c);                   \
    if (rc) return rc
#define RESOLVE_DEVICE(ptr)                          \
    RESOLVE_CONTEXT();                               \
    DeviceCtx* D = nullptr;                          \
    if ((rc = device_of(c, (ptr), &D))) return rc

// ---- resident tables (rtgr_tables.hip) -----------------------------------------------------------------------------------------
void free_all(const std::vector<void*>& ptrs);   // hipFree of each (the device is current and idle)
struct TableIds { uint64_t tag, mask; std::atomic<uint64_t> next{1}; };   // the ids of one kind: tag | (counter & ~mask)
struct TableSegment { const void* p; size_t bytes; };
typedef std::vector<TableSegment> TableImage;   // what is uploaded as one table: segments, one behind the other
// THE load of a table named by an id (`kind`: its Resident in DeviceCtx): a fresh id, the Float64 and the Float32 image uploaded to every
// device of the context — or to none: a failure rolls back —, `t` with the id and the two addresses published on each.  Takes
// c->modules_mu, then each D.mu briefly.  `who`: the entry point, for the refusal.
template <class T>
int table_load(rtgr_context* c, const char* who, TableIds& ids, Resident<T> DeviceCtx::*kind, T t, const TableImage& image64,
               const TableImage& image32, uint64_t* id_out);
// … and the unload: the table retired on every device (same locks); whether any device knew the id
template <class T> bool table_unload(rtgr_context* c, Resident<T> DeviceCtx::*kind, uint64_t id, bool zero_means_all);
// (D.mu held; `st`: the stream the scene's kernels go on)  The device table with this content, uploaded on first sight — which a stream
// under capture cannot wait for; a table found during capture is kept until rtgr_trim / rtgr_destroy
int object_table(DeviceCtx& D, const std::vector<char>& content, hipStream_t st, const void** dev);
std::vector<void*> drain_object_tables(DeviceCtx& d);   // every table's address, to be freed; the device forgets them

// ---- argument conversion (rtgr_scene_host.hip) and the device-side enqueue (rtgr_context.hip) --------------------------------------
void scene_variant(const rtgr_scene* s, uint32_t* metric, bool* spin);
// The load-time probe of a unit of OBJECTS traces a scene of built-in objects (it knows no parameters of the user's) and must still run
// the UNIT's kernels, not the library's: while this is set on the calling thread, a scene that names a unit runs with it even though
// nothing in the scene requires one.  (Everywhere else a built-in scene ignores rtgr_scene.user_metric, as it always has.)
extern thread_local bool tl_probe_forces_unit;
// … and the probe (and rtgr_scene_check) choose the launch options of THEIR calls — pass structure, queue order, grid size — without
// touching the device's options, which other threads' calls on the same device read: null = the device's options decide.
extern thread_local const Knobs* tl_knobs_override;
// (D.mu held.  `st`: the stream the scene's kernels will be enqueued on: object_table above)
template <class R> int convert_scene(DeviceCtx& D, const rtgr_scene* s, DevScene<R>& d, const UserModule** user, hipStream_t st = nullptr);
// the object list of a scene: rtgr_scene.objects when given, else the inline slots
inline const rtgr_object* scene_objects(const rtgr_scene* s) { return s->objects ? s->objects : s->obj; }
template <class R> int convert_solver(const rtgr_solver* s, DevSolver<R>& d);
template <class R> void convert_camera(const rtgr_camera* c, DevCamera<R>& d);
// window of a larger output: see TraceArgs::plane_stride / out_offset
struct Window { uint64_t plane_stride = 0, out_offset = 0; uint32_t* nan_flag = nullptr; hipEvent_t after_setup = nullptr; };
// Enqueue the pipeline for rows of a canvas on device D, stream st.  The caller holds no lock; this takes D.mu for the
// duration of the enqueue.
template <class R>
int trace_device(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const R* d_state0, const rtgr_camera* cam,
                 uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, R* d_rgb, const rtgr_ray_outputs* out,
                 rtgr_counters* d_counters, hipStream_t st, uint64_t jstride = 1, uint64_t nrows_strided = 0,
                 const Window* win = nullptr);

// ---- what the frame calls share (rtgr_frame_host.hip) ------------------------------------------------------------------------------
// The frame scratch of a stream (StreamState::frame): what a frame call keeps there, each block 256-aligned and an absent one no bytes.
// Pure arithmetic: the head — rtgr_counters (64 bytes), then the refined count of an anti-aliased frame — always; `obs`: the observer's
// frame record; `list`: the index list of the refined pixels; then the end states / hit map / status bytes to borrow, n rays of each.
constexpr size_t FRAME_HEAD = 256, FRAME_OBS = 512;
// `orders`: what the lists of a higher-order disk image add (rtgr_orders_host.hip): a second index list of n pixels behind the first, and,
// with orders_state0, the start states of the n rays
// `lambda_end`: the end parameters of n rays, which the transfer kernel of volume emission reads (rtgr_transfer_host.hip) — the last block,
// so every other frame's layout is what it was
struct FrameNeeds { bool state_end = false, hit32 = false, status = false, list = false, obs = false, orders = false, orders_state0 = false, lambda_end = false; };
struct FrameLayout { size_t obs, list, state_end, hit32, status, orders_list, orders_state0, lambda_end, bytes; };
static_assert(sizeof(rtgr_counters) + sizeof(unsigned long long) <= FRAME_HEAD && sizeof(ObsFrame<double>) <= FRAME_OBS, "the head holds them");
inline FrameLayout frame_layout(uint64_t n, size_t scalar, const FrameNeeds& need) {
    FrameLayout at;
    at.obs = FRAME_HEAD;
    at.list = at.obs + (need.obs ? FRAME_OBS : 0);
    at.state_end = at.list + (need.list ? align256((size_t)n * sizeof(uint64_t)) : 0);
    at.hit32 = at.state_end + (need.state_end ? align256((size_t)n * 8 * scalar) : 0);
    at.status = at.hit32 + (need.hit32 ? align256((size_t)n * sizeof(uint32_t)) : 0);
    at.orders_list = at.status + (need.status ? align256((size_t)n) : 0);
    at.orders_state0 = at.orders_list + (need.orders ? align256((size_t)n * sizeof(uint64_t)) : 0);
    at.lambda_end = at.orders_state0 + (need.orders_state0 ? align256((size_t)n * 8 * scalar) : 0);
    at.bytes = at.lambda_end + (need.lambda_end ? align256((size_t)n * scalar) : 0);
    return at;
}
// the words of an entry point in its refusals: its name ("rtgr_trace_shaded_*"), what it calls its scratch ("shading"), and whether
// the refusal to grow it says what to do instead
struct EntryWords { const char* entry; const char* scratch; bool advise; };
// A frame call's share of the stream's scratch, as frame_scratch leaves it: `o1` is the caller's rtgr_ray_outputs with the members the
// call must borrow pointed into the scratch; d_ctr the device counters when the caller counts (the head is zeroed on the stream), else null.
struct FrameScratch {
    StreamState* ss = nullptr;   // (entries of the map stay where they are: it outlives the lock)
    char* base = nullptr;        // null: the call needs nothing of the scratch
    FrameLayout at;
    rtgr_ray_outputs o1;
    rtgr_counters* d_ctr = nullptr;
};
// grow-only scratch of a stream, retired like its workspace (D.mu held; never called during capture: frame_scratch refuses first)
int scratch_need(StreamState& ss, void*& p, size_t& have, size_t bytes);
// whether st is being captured; a call that counts (ctr) synchronises at its end and is refused then, by a message with "ctr"
int capture_check(hipStream_t st, const EntryWords& who, const rtgr_counters* ctr, bool* capturing);
// (D.mu held)  The stream's state, its frame scratch grown to what `need` asks for n rays of `scalar` bytes and its batch scratch to
// batch_bytes — refused while the stream is captured — and the head zeroed when someone counts in it (ctr, or the refined count)
int frame_scratch(DeviceCtx& D, hipStream_t st, bool capturing, const EntryWords& who, uint64_t n, size_t scalar, const FrameNeeds& need,
                  size_t batch_bytes, const rtgr_ray_outputs* out, const rtgr_counters* ctr, FrameScratch& fs);
// the end of a call that counts: the counters to the caller, behind a synchronisation
int counters_back(const FrameScratch& fs, rtgr_counters* ctr, hipStream_t st);
// THE post-trace stage: `after` applied to the pixels a trace just wrote on st — the shading kernel if there are binds, then the emission
// kernel if a disk emits; takes D.mu, each launch timed in slot 0
template <class R> int after_trace(DeviceCtx& D, hipStream_t st, const AfterTrace<R>& after, const TracedPixels<R>& px);
// the small checks: the canvas of `what` ("a shaded frame"), the scene's metric not the user's own (`what`: "disk emission in", `why`: "its
// kernels live"), and the scene as a kernel that needs a stationary metric reads it (D.mu held; a 4-D grid is refused with `refusal`)
int canvas_check(uint64_t ni, uint64_t nj, const char* what);
int builtin_metric_check(const rtgr_scene* scene, const char* what, const char* why);
template <class R> int stationary_scene(DeviceCtx& D, const rtgr_scene* scene, DevScene<R>& sc, hipStream_t st, const char* refusal);
constexpr const char* EMISSION_NEEDS_STATIONARY =
    "disk emission in a time-dependent (4-D) grid metric is not supported: the emitter's orbit needs a stationary metric";
// The frame of a camera with textures and / or an emitting disk (rtgr_trace_shaded_* / rtgr_trace_emission_*) on device D, stream st; d_rgb,
// d_g, the members of `out` and d_refined are pointers of that device.  emit == NULL: a shaded frame, which needs `shade`; aa: the
// anti-aliased frame of rtgr_aa_host.hip with both as its AfterTrace
template <class R>
int trace_camera_frame_on(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                          const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, R* d_g,
                          uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, hipStream_t st, const EntryWords& who);
// A host-pointer frame call: `call` — a device-side frame call, given device 0 of the context, its staging's compute stream and device
// arrays for rgb, `out` and (where not null) refined and g — and all of them copied out.  n: the pixels of the frame
template <class R>
using StagedCall = std::function<int(DeviceCtx& D, R* d_rgb, const rtgr_ray_outputs* d_out, uint8_t* d_refined, R* d_g, hipStream_t st)>;
template <class R>
int staged_frame(rtgr_context* c, uint64_t n, R* rgb, const rtgr_ray_outputs* out, uint8_t* refined, R* g, const StagedCall<R>& call);

// ---- adaptive anti-aliasing on one device (rtgr_aa_host.hip) ------------------------------------------------------------------------
// the call on device D, stream st; d_rgb, the members of `out` and d_refined are pointers of that device.  after == nullptr: the plain
// anti-aliased frame; otherwise both passes are shaded with its (resolved) binds and / or emitted with its disk (AfterTrace, rtgr_host.hpp)
template <class R>
int trace_aa_on(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats,
                hipStream_t st, const AfterTrace<R>* after);
// image textures (rtgr_texture_host.hip): the caller's binds into the records the shading kernel reads, for device D and scalar type R
// (takes D.mu), and the checks of a camera frame's arguments
template <class R> int shade_resolve(DeviceCtx& D, const rtgr_scene* scene, const rtgr_shade* shade, ShadeDesc<R>& sd);
int shaded_check(const rtgr_camera* cam, const rtgr_aa* aa, const uint8_t* refined, const rtgr_aa_stats* stats, uint64_t ni, uint64_t nj);
// disk emission (rtgr_emission_host.hip): the caller's parameters into the record the kernels read (`shade`, may be null: the binds of
// the same call)
template <class R> int emission_resolve(const rtgr_scene* scene, const rtgr_shade* shade, const rtgr_disk_emission* emit, DevEmission<R>& em);
// the observer camera (rtgr_observer_host.hip): the checks of an rtgr_observer against its scene, and the record the frame kernel reads
template <class R> int observer_resolve(const rtgr_scene* scene, const rtgr_observer* obs, DevObserver<R>& ob);
// … and its trace on device D, stream st; d_rgb, d_g and the members of `out` are pointers of that device.  pol (may be null; needs emit):
// the polarization kernel on each batch's window behind the emission kernel (rtgr_trace_polarized_*, with its words in the refusals)
template <class R>
int trace_observer_on(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                      const rtgr_shade* shade, const rtgr_disk_emission* emit, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, rtgr_counters* ctr,
                      hipStream_t st, const PolStage<R>* pol = nullptr, const TransferStage<R>* xfer = nullptr);
// (xfer, may be null: the transfer kernel of volume emission on each batch's window behind everything else — rtgr_trace_transfer_*, with
// its words in the refusals; its counters sit in the frame scratch's head, FRAME_HEAD_TCTR bytes in)
constexpr size_t FRAME_HEAD_TCTR = 128;
static_assert(FRAME_HEAD_TCTR >= sizeof(rtgr_counters) + sizeof(unsigned long long) && FRAME_HEAD_TCTR + sizeof(rtgr_counters) <= FRAME_HEAD, "the head holds both");

// ---- a traced frame of an emitting disk reduced to a table of (F, A, B) rows (rtgr_reduce_host.hip) -----------------------------------
// The reduction scratch of a stream (StreamState::reduce) in one call, each block 256-aligned and an absent one no bytes.  Pure
// arithmetic: the reduction's head (head_bytes, a multiple of 256), the partial sums of one pass (partial_bytes: reduce_partial_bytes,
// rtgr_reduce.hpp), then the planes a traced call keeps there because the caller gave none — end states, hit map, frequency ratio, n
// pixels of each, the scalars `scalar` bytes wide.
struct ReduceGiven { bool state_end = false, hit32 = false, g = false; };
struct ReduceLayout { size_t partial, state_end, hit32, g, bytes; };
inline ReduceLayout reduce_layout(size_t head_bytes, size_t partial_bytes, uint64_t n, size_t scalar, const ReduceGiven& given) {
    ReduceLayout at;
    at.partial = head_bytes;
    at.state_end = at.partial + align256(partial_bytes);
    at.hit32 = at.state_end + (given.state_end ? 0 : align256((size_t)n * 8 * scalar));
    at.g = at.hit32 + (given.hit32 ? 0 : align256((size_t)n * sizeof(uint32_t)));
    at.bytes = at.g + (given.g ? 0 : align256((size_t)n * scalar));
    return at;
}
// What differs between the reductions — a value per entry-point family, made by the caller for one call:
template <class R>
struct Reduction {
    EntryWords device, traced;   // the words of rtgr_<x>_device_* and of rtgr_trace_<x>_* / rtgr_trace_<x>_device_*
    const char* canvas;          // what the device entry calls its canvas ("a light curve")
    const char* out_name;        // … and every entry its output, in "<entry>: <out_name> is NULL"
    const void* record;          // the caller's record (rtgr_hot_spot, rtgr_spectrum) and the refusal of a NULL one
    const char* record_null;
    size_t head_bytes;           // the head of the scratch the stage wants in front of the partial sums
    uint64_t rows;               // rows of the output table (read after `resolve` has accepted the record)
    // every refusal the arguments deserve, and what the stage reads of them (kept by the caller); touches no device
    std::function<int(uint64_t ni, uint64_t nj)> resolve;
    // the kernels, enqueued on st (D.mu held, timed in slot 0): `base`: the stream's scratch — head, then the partial sums
    std::function<int(DeviceCtx& D, const DevScene<R>& sc, const ReducePlanes<R>& P, char* base, double* d_out, hipStream_t st)> stage;
};
// rtgr_<x>_device_*: the stage over the caller's planes, on the device that holds d_out
template <class R>
int reduce_device(rtgr_context* ctx, const Reduction<R>& red, const rtgr_scene* scene, const rtgr_disk_emission* emit, uint64_t ni, uint64_t nj,
                  const uint32_t* d_hit32, const R* d_state_end, const R* d_g, double* d_out, void* stream);
// rtgr_trace_<x>_device_*: rtgr_trace_observer_device_* on the device that holds d_rgb, with the planes the stage reads borrowed from the
// stream's reduction scratch where the caller gave none, then the stage
template <class R>
int trace_reduce_device(rtgr_context* ctx, const Reduction<R>& red, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                        uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, double* d_out,
                        rtgr_counters* ctr, void* stream);
// rtgr_trace_<x>_*, host pointers: the same on device 0 of the context, on its staging's compute stream; the frame and the table copied out
template <class R>
int trace_reduce(rtgr_context* ctx, const Reduction<R>& red, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                 uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, R* rgb, const rtgr_ray_outputs* out, R* g, double* table,
                 rtgr_counters* ctr);
// the pixel weight of an observer's canvas (obs may be null: w = 1): what pixel_weight (rtgr_reduce.hpp) reads
template <class R> int pixel_weight_resolve(const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, PixelWeight& W);

// a device buffer of one call that mirrors no host array (the table of trace_reduce, the sampled states of auto_scene_check): RAII, synchronous
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) {
        if (bytes == 0) return RTGR_OK;
        HIP_TRY(hipMalloc(&p, bytes));
        return RTGR_OK;
    }
};

// The device-side mirror of the arrays of ONE blocking host-pointer call on one device (make_canvas, the rtgr_eval_* hooks, the probe,
// the planes a host-pointer frame call adds to staged_frame's): each array is declared once, its count stated once — `in` goes up at
// once, `out` and `inout` come back in `fetch`, `scratch` stays on the device.  One hipMalloc per array (a kernel that overruns one stays
// as detectable as it is with an array of its own), blocking copies.  The mirror makes its device current for its lifetime and takes no
// lock: who holds D.mu, and for how long, is the call's own business.  An omitted optional output legitimately gets a null device pointer,
// so a failure is not told by the pointer: the first one is kept (what is declared after it gets null and no HIP call) and asked for
// by status(), at once for the device and once more behind the declarations.
// fetch is THE place where these calls wait for the device — hipDeviceSynchronize for a hook, the stream inside a staged frame call:
// what they wait with is changed here, not hook by hook.
class HostMirror {
    DeviceGuard guard_;   // ahead of the arrays: they are freed on their device, then the calling thread's device is restored
    struct Array { void* dev; void* host; size_t bytes; };   // host: where fetch copies it back to (null: nowhere)
    std::vector<Array> arrays_;
    int rc_ = RTGR_OK;

    int alloc(const void* up, void* back, size_t bytes, void*& p) {
        HIP_TRY(hipMalloc(&p, bytes));
        arrays_.push_back({p, back, bytes});
        if (up) HIP_TRY(hipMemcpy(p, up, bytes, hipMemcpyHostToDevice));
        return RTGR_OK;
    }
    void* add(const void* up, void* back, size_t bytes) {
        void* p = nullptr;
        if (rc_ == RTGR_OK && bytes) rc_ = alloc(up, back, bytes, p);
        return rc_ == RTGR_OK ? p : nullptr;
    }
    int back() {
        for (const Array& a : arrays_)
            if (a.host) HIP_TRY(hipMemcpy(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost));
        return RTGR_OK;
    }

public:
    explicit HostMirror(DeviceCtx& D) : guard_(D.dev) { if (!guard_.ok) rc_ = fail(RTGR_ERR_HIP, "hipSetDevice failed"); }
    explicit HostMirror(rtgr_context* c) : HostMirror(*c->devs[0]) {}
    HostMirror(const HostMirror&) = delete;
    HostMirror& operator=(const HostMirror&) = delete;
    ~HostMirror() { for (const Array& a : arrays_) (void)hipFree(a.dev); }
    int status() const { return rc_; }
    // count elements of T each; count = 0, or a null `host`: a null device pointer and no HIP call
    template <class T> const T* in(const T* host, size_t count) { return (const T*)add(host, nullptr, host ? count * sizeof(T) : 0); }
    template <class T> T* out(T* host, size_t count) { return (T*)add(nullptr, host, host ? count * sizeof(T) : 0); }
    template <class T> T* inout(T* host, size_t count) { return (T*)add(host, host, host ? count * sizeof(T) : 0); }
    template <class T> T* scratch(size_t count) { return (T*)add(nullptr, nullptr, count * sizeof(T)); }
    int zero() {   // every array declared so far, blocking, on the null stream
        for (const Array& a : arrays_) HIP_TRY(hipMemset(a.dev, 0, a.bytes));
        return rc_;
    }
    // behind the launch: wait, then every out and inout back to its host array, in the order of their declaration
    int fetch() {
        if (rc_) return rc_;
        HIP_TRY(hipDeviceSynchronize());
        return back();
    }
    int fetch(hipStream_t st) {
        if (rc_) return rc_;
        HIP_TRY(hipStreamSynchronize(st));
        return back();
    }
};

template <class R>
int host_has_nan(const R* v, uint64_t count) {
    for (uint64_t q = 0; q < count; q++)
        if (v[q] != v[q]) return 1;
    return 0;
}

// ---- the per-ray output arrays of a call: rgb plus what rtgr_ray_outputs asks for ------------------------------------------------
// THE list of the optional arrays, in the order the staging buffers hold them: where the pointer sits in rtgr_ray_outputs, and the
// bytes per ray — `scalars` of the entry point's type (sizeof(R)) plus `bytes` — in `planes` planes.  A new output is a new row here
// (and a member of the kernels' TraceArgs, which trace_device copies by name).
struct RayOutputField { size_t pos, scalars, bytes; int planes; };
constexpr RayOutputField RAY_OUTPUT_FIELDS[] = {
    {offsetof(rtgr_ray_outputs, state_end), 8, 0, 1}, {offsetof(rtgr_ray_outputs, lambda_end), 1, 0, 1},
    {offsetof(rtgr_ray_outputs, status), 0, 1, 1},    {offsetof(rtgr_ray_outputs, hit), 0, 1, 1},
    {offsetof(rtgr_ray_outputs, n_accept), 0, 4, 1},  {offsetof(rtgr_ray_outputs, n_reject), 0, 4, 1},
    {offsetof(rtgr_ray_outputs, redshift), 1, 0, 1},  {offsetof(rtgr_ray_outputs, hit32), 0, 4, 1},
};
static_assert(sizeof(rtgr_ray_outputs) == sizeof(RAY_OUTPUT_FIELDS) / sizeof(RAY_OUTPUT_FIELDS[0]) * sizeof(void*), "a row per member of rtgr_ray_outputs");
inline void* ray_output(const rtgr_ray_outputs& o, const RayOutputField& f) {
    void* p;
    std::memcpy(&p, (const char*)&o + f.pos, sizeof p);
    return p;
}
// One requested array: `planes` planes (rgb: 3, else 1) of `elem` bytes per ray; `ptr` is the caller's array (host, or the full frame
// on device 0), `off` its place in a staging buffer (ray_arrays_layout).
struct RayArray { void* ptr; size_t elem; int planes; size_t off; };
// [0] = rgb, always; then the arrays `out` asks for.  `scalar` = sizeof(R).
inline std::vector<RayArray> ray_arrays(void* rgb, const rtgr_ray_outputs* out, size_t scalar) {
    std::vector<RayArray> arrs{{rgb, scalar, 3, 0}};
    if (out)
        for (const RayOutputField& f : RAY_OUTPUT_FIELDS)
            if (void* p = ray_output(*out, f)) arrs.push_back({p, f.scalars * scalar + f.bytes, f.planes, 0});
    return arrs;
}
// their places in a buffer that holds `m` rays of each; returns the bytes of the buffer
inline size_t ray_arrays_layout(std::vector<RayArray>& arrs, uint64_t m) {
    size_t bytes = 0;
    for (RayArray& a : arrs) { a.off = bytes; bytes += align256((size_t)m * a.elem * a.planes); }
    return bytes;
}
// what `out` asks for, pointing into the buffer at `base` that `arrs` (= ray_arrays(…, out, …), laid out) describes
inline rtgr_ray_outputs ray_outputs_at(char* base, const std::vector<RayArray>& arrs, const rtgr_ray_outputs* out) {
    rtgr_ray_outputs o;
    std::memset(&o, 0, sizeof o);
    size_t k = 1;
    if (out)
        for (const RayOutputField& f : RAY_OUTPUT_FIELDS)
            if (ray_output(*out, f)) { void* p = base + arrs[k++].off; std::memcpy((char*)&o + f.pos, &p, sizeof p); }
    return o;
}
inline int check_redshift_outputs(const rtgr_ray_outputs* out) {
    if (out && out->redshift && (!out->state_end || !(out->hit || out->hit32)))
        return fail(RTGR_ERR_BAD_ARG, "rtgr_ray_outputs.redshift needs state_end and hit (or hit32) in the same call");
    return RTGR_OK;
}
// the counters of one device's share into those of the call: sums, except [7], a maximum (diagnostics)
inline void merge_counters(rtgr_counters& into, const rtgr_counters& part) {
    const uint64_t* p = (const uint64_t*)&part;
    uint64_t* q = (uint64_t*)&into;
    for (int w = 0; w < 8; w++) q[w] = (w == 7) ? (q[w] > p[w] ? q[w] : p[w]) : q[w] + p[w];
}

// ---- run-time units (rtgr_units.hip) ---------------------------------------------------------------------------------------------
int unload_locked(rtgr_context* c, uint64_t id);   // drop unit `id` (0: all) from every device; the caller holds c->modules_mu
// The scene check nobody has to remember: called by trace_device ahead of every enqueue, answers from the device's
// table of checked scenes in all but the first call for a scene.  D.mu NOT held.
template <class R>
int auto_scene_check(DeviceCtx& D, const rtgr_scene* scene, const rtgr_solver* opt, const R* d_state0, const rtgr_camera* cam,
                     uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, uint64_t jstride, uint64_t nrows_strided, hipStream_t st);

// ---- the entry points of include/rtgr.h, by the name behind the rtgr_ prefix (rtgr_abi.hip holds the extern "C" shims); an
// _f64 / _f32 pair is one template over the scalar type -------------------------------------------------------------------------
namespace api {
int create(const int* device_ids, int n_devices, rtgr_context** ctx_out);
int destroy(rtgr_context* ctx);
int context_devices(rtgr_context* ctx);
int trim(rtgr_context* ctx);
int init(int device);
int shutdown(void);
const char* last_error(void);
int abi_version(void);
int solver_defaults(rtgr_solver* s, int is_f32);
int device_info(rtgr_context* ctx, int index, char* name, uint64_t name_len, int* n_cu, int* clock_mhz, int* wavefront);
int set_option(rtgr_context* ctx, const char* name, long value);
int get_option(rtgr_context* ctx, const char* name, long* value);
int reserve_workspace(rtgr_context* ctx, const void* d_any, void* stream, uint64_t n_rays, int with_state_end, int is_f32);
int timing_enable(rtgr_context* ctx, int index, int on);
int timing_read(rtgr_context* ctx, int index, double ms[4], uint64_t launches[4]);
int timing_read_exchange(rtgr_context* ctx, int index, double ms[2], uint64_t launches[2]);
int peer_access(rtgr_context* ctx, int index, char* why, uint64_t why_len);
template <class R> int trace_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const R* d_state0, const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, R* d_rgb, const rtgr_ray_outputs* out, rtgr_counters* d_counters, void* stream);
template <class R> int trace_rows_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t jstride, uint64_t nrows, R* d_rgb, const rtgr_ray_outputs* out, rtgr_counters* d_counters, void* stream);
template <class R> int trace(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const R* state0, const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, R* rgb, const rtgr_ray_outputs* out, rtgr_counters* ctr);
template <class R> int trace_pixels(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const R* pixels_in, uint64_t ni, uint64_t nj, R* pixels_out, rtgr_counters* ctr);
template <class R> int trace_frames(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, uint32_t nframes, const rtgr_camera* cams, const R* const* state0s, uint64_t ni, uint64_t nj, R* const* rgb, const rtgr_ray_outputs* outs, rtgr_counters* ctrs);
template <class R> int trace_frames_pixels(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, uint32_t nframes, const R* const* pixels_in, uint64_t ni, uint64_t nj, R* const* pixels_out, rtgr_counters* ctrs);
template <class R> int trace_one(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const R pos[4], const R normal[4], R rgb[3], R state_end[8], uint8_t* status);
template <class R> int trace_sharded(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, R* rgb, const rtgr_ray_outputs* out, rtgr_counters* ctr);
template <class R> int trace_sharded_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, R* d_rgb, const rtgr_ray_outputs* out, rtgr_counters* ctr);
template <class R> int trace_aa_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
template <class R> int trace_aa(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, const rtgr_aa* aa, R* rgb, const rtgr_ray_outputs* out, uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats);
template <class R> int make_canvas_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, R* d_state0, void* stream);
template <class R> int make_canvas(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, R* state0);
template <class R> int eval_metric(rtgr_context* ctx, const rtgr_scene* scene, const R* x, uint64_t n, R* g, R* dg, R* Gam);
template <class R> int eval_geodesic(rtgr_context* ctx, const rtgr_scene* scene, const R* s, uint64_t n, int path, R* ds);
template <class R> int eval_objects(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const R* x, uint64_t n, R* d, R* dmin, uint8_t* hit, R* rgb);
int eval_fastmath_f64(rtgr_context* ctx, const double* x, uint64_t n, double* rcp, double* rsq);
int user_metric_load(rtgr_context* ctx, const char* code_object_path, uint64_t* id_out);
int user_metric_compile(rtgr_context* ctx, const char* source, int stationary, uint64_t* id_out);
int user_metric_build(const char* source, int stationary, const char* code_object_path);
int user_metric_unload(rtgr_context* ctx, uint64_t id);
int user_unit_compile(rtgr_context* ctx, const char* source, int stationary, const rtgr_scene* built_for, uint64_t* id_out);
int user_unit_build(const char* source, int stationary, const rtgr_scene* built_for, const char* code_object_path);
int user_source_join(const char* const* sources, const uint32_t* ntypes, int n, char* out, uint64_t cap, uint64_t* need);
int user_unit_info(rtgr_context* ctx, uint64_t id, rtgr_unit_info* info);
int scene_check(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, int is_f32);
int code_object_audit(const char* code_object_path, int* found, char* report, uint64_t report_len);
int listing_repair(const char* listing_path, const char* repaired_path, int* blocks);
int user_metric_loaded(rtgr_context* ctx, uint64_t id);
int grid_metric_load(rtgr_context* ctx, const rtgr_grid* grid, const double* g, uint64_t* id_out);
int grid_metric_unload(rtgr_context* ctx, uint64_t id);
int grid4_metric_load(rtgr_context* ctx, const rtgr_grid4* grid, const double* g, uint64_t* id_out);
int texture_load(rtgr_context* ctx, const rtgr_texture_desc* desc, const double* texels, uint64_t* id_out);
int texture_unload(rtgr_context* ctx, uint64_t id);
template <class R> int trace_shaded_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
template <class R> int trace_shaded(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_aa* aa, R* rgb, const rtgr_ray_outputs* out, uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats);
template <class R> int eval_texture(rtgr_context* ctx, uint64_t texture, uint32_t filter, const R* p, uint64_t n, const R* disk_range, R* rgb);
template <class R> int trace_emission_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_aa* aa, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
template <class R> int trace_emission(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_aa* aa, R* rgb, const rtgr_ray_outputs* out, R* g, uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats);
template <class R> int eval_disk_emission(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const R* s0, const R* s_end, uint64_t n, R* omega, R* u_emit, R* g, R* rgb);
template <class R> int eval_disk_emission_observer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_observer* obs, const R* s0, const R* s_end, uint64_t n, R* omega, R* u_emit, R* g, R* rgb);
template <class R> int trace_observer_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, rtgr_counters* ctr, void* stream);
template <class R> int trace_observer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, R* rgb, const rtgr_ray_outputs* out, R* g, rtgr_counters* ctr);
template <class R> int make_observer_canvas_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, R* d_state0, void* stream);
template <class R> int make_observer_canvas(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, R* state0);
template <class R> int eval_observer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, R* frame, R* omega, int* valid);
template <class R> int light_curve_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state_end, const R* d_g, double* d_lc, void* stream);
template <class R> int trace_light_curve_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, double* d_lc, rtgr_counters* ctr, void* stream);
template <class R> int trace_light_curve(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, R* rgb, const rtgr_ray_outputs* out, R* g, double* lc, rtgr_counters* ctr);
template <class R> int eval_hot_spot(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot, const R* xyt, uint64_t n, R* omega_s, int* valid, double* j);
template <class R> int spectrum_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state_end, const R* d_g, double* d_out, void* stream);
template <class R> int trace_spectrum_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, double* d_out, rtgr_counters* ctr, void* stream);
template <class R> int trace_spectrum(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, R* rgb, const rtgr_ray_outputs* out, R* g, double* spectrum, rtgr_counters* ctr);
template <class R> int eval_spectrum(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec, const R* xyg, uint64_t n, double* axis, int64_t* bin, double* val);
template <class R> int polarization_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32, const R* d_state0, const R* d_state_end, R* d_q, R* d_u, R* d_aux, void* stream);
template <class R> int trace_polarized_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_polarization* pol, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, R* d_q, R* d_u, R* d_aux, rtgr_counters* ctr, void* stream);
template <class R> int trace_polarized(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_polarization* pol, R* rgb, const rtgr_ray_outputs* out, R* g, R* q, R* u, R* aux, rtgr_counters* ctr);
template <class R> int eval_polarization(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol, const rtgr_observer* obs, const R* s0, const R* s_end, uint64_t n, R* kappa, R* f_em, R* aux, R* delta, R* q, R* u, int* valid);
template <class R> int eval_walker_penrose(rtgr_context* ctx, const rtgr_scene* scene, const R* s, const R* f, uint64_t n, R* kappa);
template <class R> int trace_orders_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, const R* d_state0, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, R* d_rgb, const rtgr_order_planes* planes, rtgr_counters* ctr, void* stream);
template <class R> int trace_orders(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, const R* state0, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, R* rgb, const rtgr_order_planes* planes, rtgr_counters* ctr);
template <class R> int trace_transfer_device(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_flow* flow, R* d_rgb, const rtgr_ray_outputs* out, R* d_g, R* d_I, R* d_tau, uint8_t* d_tstatus, uint32_t* d_tsteps, rtgr_counters* ctr, rtgr_counters* tctr, void* stream);
template <class R> int trace_transfer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni, uint64_t nj, const rtgr_shade* shade, const rtgr_disk_emission* emit, const rtgr_flow* flow, R* rgb, const rtgr_ray_outputs* out, R* g, R* I, R* tau, uint8_t* tstatus, uint32_t* tsteps, rtgr_counters* ctr, rtgr_counters* tctr);
template <class R> int eval_transfer(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_flow* flow, const rtgr_observer* obs, const R* s0, const R* lambda_end, uint64_t n, R* I, R* tau, R* s_end, uint8_t* tstatus, uint32_t* tsteps);
template <class R> int eval_flow(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_flow* flow, const rtgr_observer* obs, const R* s0, const R* s, uint64_t n, R* dens, R* omega, R* u_f, R* gfac, R* dtau, R* dI0);
int quantize_device_f64(rtgr_context* ctx, const double* d_rgb, uint64_t ni, uint64_t nj, uint8_t* d_img, void* stream);
}  // namespace api

}  // namespace rtgr
