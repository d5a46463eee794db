// rtgr_host.hpp — host-side state of librtgr_hip.so: contexts, per-stream workspaces, launch policy knobs.
//
// SURVEY §8(b) "Ownership / Threading": the library owns device buffers and streams inside an OPAQUE CONTEXT
// (rtgr_context, include/rtgr.h); calls are re-entrant per context, one host thread may drive several devices and
// several host threads may drive one.  Layout of that state:
//
//   rtgr_context            the devices one host process drives (rtgr_create(device_ids, n))
//     DeviceCtx[n]          one per entry of device_ids (the same physical GPU may be listed twice: two "logical
//                           devices" with streams and workspaces of their own — how the multi-device path is tested on a
//                           one-GPU box)
//       StreamState[*]      one per hipStream_t the caller has used on that device: the pipeline workspace (start /
//                           hand-over / event records, per-ray meta, queue order, work-queue heads).  Launches on ONE
//                           stream are ordered by the stream and share a workspace; launches on DIFFERENT streams get
//                           different workspaces, so they never race (round 1 had one process-global workspace)
//       resident tables     grid metrics and image textures by id (Resident<T>), the tables of long object lists by content
//       user modules        run-time compiled units (a metric, Object subtypes, or both), keyed by the 64-bit id a scene carries
//                           (rtgr_scene.user_metric)
//       staging             pinned host buffers + device buffers + 3 streams of the host-pointer entry points
//
// A workspace only grows; the superseded allocation is RETIRED, not freed (a hipGraph captured earlier may still
// reference it) until rtgr_destroy / rtgr_trim.  Growth during stream capture is refused (hipMalloc is not capturable):
// reserve first (rtgr_reserve_workspace).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/rtgr.h"
#include "rtgr_args.hpp"

namespace rtgr {

int fail(int code, const std::string& msg);  // records the calling thread's last error, returns `code`
#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return ::rtgr::fail(RTGR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)
// behind every kernel launch of the library's own kernel units
#define CHECK_LAUNCH()                                     \
    do {                                                   \
        hipError_t e_ = hipGetLastError();                 \
        if (e_ != hipSuccess) return ::rtgr::fail(RTGR_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

// whether work enqueued on st is being recorded into a hipGraph rather than run
inline bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

// ---- launch policy knobs ------------------------------------------------------------------------------------------------
// Parsed ONCE from the environment when a context is created (RTGR_<NAME>), changeable per context with
// rtgr_set_option(ctx, "name", value).  -1 = "auto" (the library decides from the launch size).  Experiments and
// schedule-invariance tests only: no knob changes a result bit, except `tile` and `pack`, which select another formulation of
// the same algorithm (results equal up to rounding).
struct Knobs {
    long waves_per_cu = -1;       // resident waves per CU of the integrate kernels (auto: 4 x waves/SIMD of the instantiation)
    long waves_per_cu_near = -1;  // ... of the NEAR pass (auto: 4 below 2.4 M rays, 6.3 M with spin)
    long chunk = -1;              // rays per pipeline chunk (auto: 2^26, less if memory is short)
    long split = -1;              // 0: one FULL pass instead of FAR + NEAR (auto: on for f64, off for f32)
    long order = -1;              // 0: natural ray order, 1: longest-expected-first (auto: ordered from 4096 rays; Float32 only up to 2 M)
    long fair = -1;               // log2 of the priority-rotation time slice in clocks, 0 = off (auto: by launch size)
    long near_early = 64;         // accepted steps at hand-over below which a ray goes on the NEAR pass's early list (0: no list)
    long far4 = -1;               // 0/1: force the 3- / 4-waves-per-SIMD a = 0 FAR instantiation (auto: by launch size)
    long rounds = -1;             // FAR / NEAR hand-back rounds (1..3); auto: 2 for object lists of 32..199, else 1 (rtgr_pipeline.hpp)
    long handback_after = 0;      // rounds > 1: the NEAR pass hands back only rays that have stayed this many accepted steps (experiment)
    long qchunk = -1;             // ray ids per queue atomic, FAR / FULL pass (auto)
    long qchunk_near = -1;        // ... NEAR pass (auto)
    long tile = 0;                // 1: the simple tile-per-wave kernel (RTGR_KERNEL=tile), an independent formulation
    long host_chunk = -1;         // host entry points: rays per H2D/compute/D2H pipeline piece (auto: 2^20)
    long dbg_pass_far = 0;        // debug builds: which pass reports its wave timeline
    long pack = -1;               // Float32 closed-form FULL pass: 0 = scalar kernel (one ray per lane), 1 = packed two-rays-per-lane
                                  // kernel, -1 = packed where it pays (a != 0)
    long packfar = 0;             // Float32 experiment: 1 = packed scan-free FAR pass at three waves per SIMD + the scalar NEAR pass
    long peer = -1;               // multi-device gather (rtgr_trace_sharded_device_*): 0 = always stage the rows through pinned
                                  // host memory (the no-peer-access fallback, forced), 1 = peer copies or fail, -1 = peer copies
                                  // where rtgr_create could enable peer access, the fallback elsewhere
    long max_waves = -1;          // cap of the integrate kernels' grid, in waves (the load-time probe: three waves over its 1024 rays make
                                  // every lane refill many times; results never depend on it)
    long unit_probe = 1;          // run-time units: trace a small probe frame through both pass structures at load and refuse a unit
                                  // whose frames are irreproducible or disagree (rtgr_units.hip: probe_unit); 0 = skip
    long unit_audit = 1;          // … and audit the code object for the compiler's EXEC-flip fault before loading it; 0 = skip
                                  // (a test hook: the probe must catch a faulty unit on its own)
    long groups = 1;              // object lists beyond the argument block: 1 = their spheres are sorted into groups of neighbours with a bounding
                                  // sphere each, which the FAR pass's reach test asks first (DevScene, rtgr_args.hpp); 0 = every object is asked; >= 2: on, with
                                  // that many spheres per group at most (experiments; 8 = RTGR_GROUP_MAX is the measured optimum)
    long scene_check = 1;         // scenes whose USER OBJECTS bring their own reach bound: the first trace of each (unit, object list, metric
                                  // parameters, solver, camera) runs rtgr_scene_check's comparison on a coarse sample of the call's own rays and
                                  // refuses a scene whose FAR + NEAR passes lose what the FULL pass finds (rtgr_units.hip: auto_scene_check); 0 = off
};
const char* const* knob_names();  // NULL-terminated
long* knob_slot(Knobs& k, const char* name);

// ---- run-time loaded unit: the kernels of the pipeline that depend on the caller's metric / objects, from a code object ------
struct UserModule {
    uint64_t id = 0;
    hipModule_t module = nullptr;
    bool owned = true;   // false: a logical duplicate of a device shares its twin's module and must not unload it
    unsigned far_waves = 0;  // waves per SIMD the unit's FAR pass is built for (0: the generic default)
    unsigned near_waves = 0, f32_waves = 0;   // … its NEAR / FULL passes, Float64 and Float32 (0: the generic defaults)
    hipFunction_t far = nullptr, near = nullptr, full10 = nullptr, fulln = nullptr, canvas = nullptr, prepare = nullptr,
                  eval_metric = nullptr, eval_geodesic = nullptr, eval_accel = nullptr;
    // Float32 twins (absent in units built without them)
    hipFunction_t full10_f32 = nullptr, fulln_f32 = nullptr, prepare_f32 = nullptr, canvas_f32 = nullptr;
    hipFunction_t redshift = nullptr, redshift_f32 = nullptr;   // optional (units built before round 3 have none)
    hipFunction_t resolve = nullptr, resolve_f32 = nullptr;     // the resolve kernel with the unit's objects (used when has_objects)
    hipFunction_t eval_objects = nullptr, eval_objects_f32 = nullptr;   // rtgr_eval_objects_* with the unit's objects
    hipFunction_t samples = nullptr;   // optional: one sample object per type the source offers one for (rtgr_user_sample)
    // what the unit was built for (rtgr_user_unit_desc): a scene runs with it only if its own variant is this one
    uint32_t metric = RTGR_USER;   // rtgr_metric (| RTGR_METRIC_GENERIC) of its kernels; RTGR_USER: a metric of its own
    bool spin = true;              // closed-form built-in kernels: the a != 0 instantiation
    bool has_metric = true, has_objects = false, has_reach = false;
    bool probe_ok = false;         // the load-time probe ran and passed (rtgr_units.hip: probe_unit)
};

struct TimedLaunch { hipEvent_t a, b; int which; };

// ---- what a context keeps resident on a device for its kernels to read -------------------------------------------------------------
// ONE lifetime rule (include/rtgr.h): memory a kernel may read is immutable and is freed by rtgr_trim / rtgr_destroy only — a
// kernel in flight, or a hipGraph captured earlier, never sees it change or go away.  Load and unload: rtgr_tables.hip.
//
// The tables of one kind that are named by an id (T: GridTable, TextureTable, below — `id`, `d64`, `d32`) on one device: unloading
// RETIRES a table — its id becomes unknown, its memory stays.  Bookkeeping only, no HIP call: whoever drains frees what is handed back
// (tests/c/resident_tables.cpp runs it without a device).
template <class T>
struct Resident {
    std::vector<T> live, retired;
    const T* find(uint64_t id) const {
        for (auto& t : live) if (t.id == id) return &t;
        return nullptr;
    }
    void publish(const T& t) { live.push_back(t); }
    // table `id` — every table when id is 0 and zero_means_all — from live to retired; whether there was one (an "all" always is)
    bool retire(uint64_t id, bool zero_means_all) {
        const bool all = id == 0 && zero_means_all;
        const auto gone = std::stable_partition(live.begin(), live.end(), [&](const T& t) { return !all && t.id != id; });
        const bool found = all || gone != live.end();
        retired.insert(retired.end(), gone, live.end());
        live.erase(gone, live.end());
        return found;
    }
    size_t n_resident() const { return live.size(); }
    size_t n_retired() const { return retired.size(); }
    // the device pointers to free now — of the retired tables, or (all) of every table — which the container forgets
    std::vector<void*> drain(bool all) {
        if (all) retire(0, true);
        std::vector<void*> out;
        for (auto& t : retired) { out.push_back(t.d64); out.push_back(t.d32); }
        retired.clear();
        return out;
    }
};
// A scene whose list is longer than the kernels' argument block holds (DevScene::more): the whole list, its groups and runs of groups in
// one immutable device table per distinct (scalar type, list, layout) a device has seen, found again by content.  An animation of a
// 100000-object list is 9 MB a frame, on the device and in the host copy the lookup compares with, so past a number and a size
// (rtgr_tables.hip: object_table) the tables are freed, behind a device synchronisation — EXCEPT those `kept`: a table found while the
// call's stream was being captured is held by that graph and goes with rtgr_trim / rtgr_destroy, like everything a graph may replay.
struct ObjectTable { std::vector<char> content; void* dev = nullptr; bool kept = false; };

// A metric sampled on a grid (rtgr_grid_metric_load): the samples on one device, in Float64 and Float32.  Immutable; rtgr_grid_metric_unload
// retires the table (Resident above: a hipGraph captured earlier may still replay it), rtgr_trim / rtgr_destroy free it.
// The axes of either kind, described once: t, x, y, z as in rtgr_grid4 (include/rtgr.h); a 3-D grid has dims = 3 and no axis 0.
struct GridAxes {
    int dims = 3;   // 3: RTGR_GRID as loaded by rtgr_grid_metric_load; 4: time-dependent (rtgr_grid4_metric_load; RTGR_GRID4 on the device)
    uint32_t n[4] = {0, 0, 0, 0};
    double origin[4] = {0, 0, 0, 0}, spacing[4] = {0, 0, 0, 0};
};
struct GridTable {
    uint64_t id = 0;
    GridAxes axes;
    // n_z n_y n_x x 10 doubles / floats, x fastest (the caller's layout); a time-dependent grid: slice after slice, behind the
    // GRID4_HEADER bytes of the time axis' DevGridTime (rtgr_args.hpp)
    void* d64 = nullptr, *d32 = nullptr;
};
// what the kernels read of a grid's axes, in their scalar type: the time axis' descriptor (uploaded in front of the samples) …
template <class R> inline DevGridTime<R> dev_grid_time(const GridAxes& A) {
    DevGridTime<R> T{};
    if (A.dims == 4) {
        T.st = 10ull * A.n[1] * A.n[2] * A.n[3];
        T.origin = (R)A.origin[0]; T.inv_h = (R)(1.0 / A.spacing[0]); T.hi = (R)(A.n[0] - 3u); T.top = (R)(A.n[0] - 2u);
    }
    return T;
}
// … and the spatial axes with the samples' address (DevScene::grid)
template <class R> inline DevGrid<R> dev_grid(const GridTable& t) {
    const GridAxes& A = t.axes;
    DevGrid<R> G{};
    G.g = (const R*)((const char*)(sizeof(R) == 8 ? t.d64 : t.d32) + (A.dims == 4 ? GRID4_HEADER : 0));
    G.sy = 10ull * A.n[1];
    G.sz = 10ull * A.n[1] * A.n[2];
    for (int ax = 0; ax < 3; ax++) {
        G.origin[ax] = (R)A.origin[1 + ax]; G.inv_h[ax] = (R)(1.0 / A.spacing[1 + ax]);
        G.hi[ax] = (R)(A.n[1 + ax] - 3u); G.top[ax] = (R)(A.n[1 + ax] - 2u);
    }
    return G;
}
// An image texture (rtgr_texture_load): the texels on one device, four scalars per texel (r, g, b, 0), row after row, in Float64 and
// Float32.  Immutable; rtgr_texture_unload retires the table, rtgr_trim / rtgr_destroy free it.
struct TextureTable {
    uint64_t id = 0;
    uint32_t W = 0, H = 0;
    void* d64 = nullptr, *d32 = nullptr;
};
// pipeline workspace of one (device, stream)
struct StreamState {
    void* ws = nullptr;
    size_t ws_bytes = 0;
    unsigned long long* queue = nullptr;  // 8 work-queue heads; stream order makes one slot per stream enough
    std::vector<void*> retired;           // superseded workspaces: kept alive for graphs captured earlier
    // scratch of the frame calls on this stream (rtgr_frame_host.hip: frame_scratch), grow-only and retired like the workspace.  One of
    // each for every entry point — anti-aliased, shaded, emitted and observer frames, rtgr_make_observer_canvas_device_*: a call has
    // at most one of each live and the calls on a stream are ordered.  Per FRAME (FrameLayout, rtgr_internal.hpp): the counters and
    // the refined count, the observer's frame record, the index list of the refined pixels, then the end states / hit map / status
    // bytes the post-trace kernels read and the caller did not ask for.  Per BATCH: the sub-ray states, sub-colours and what the
    // post-trace kernels read of the sub-rays (rtgr_aa_host.hip), or the ray states of an observer's rows (rtgr_observer_host.hip)
    void* frame = nullptr; size_t frame_bytes = 0;
    void* batch = nullptr; size_t batch_bytes = 0;
    // scratch of the reductions of a traced frame on this stream — light curves and disk spectra (rtgr_reduce_host.hip: reduce_scratch;
    // ReduceLayout, rtgr_internal.hpp) —, grow-only and retired likewise: the reduction's head (the light curve's LC_HEAD, none for the
    // spectra), the partial sums of one pass over the item axis, then the planes a traced call borrows (end states, hit map, ratio).  One
    // buffer for all of them: the stages on a stream are ordered
    void* reduce = nullptr; size_t reduce_bytes = 0;
};

struct Staging;  // host entry points (rtgr_internal.hpp)

struct DeviceCtx {
    int dev = -1;       // HIP device ordinal
    int num_cu = 0;
    std::string name;
    std::mutex mu;      // held while a call enqueues its kernels: the enqueue sequences of two host threads never interleave
    std::unordered_map<hipStream_t, StreamState> streams;
    std::vector<UserModule> modules;
    Resident<GridTable> grids;         // grid metrics, by id
    Resident<TextureTable> textures;   // image textures, by id
    std::unordered_multimap<uint64_t, ObjectTable> object_tables;   // by FNV-1a of the content
    size_t object_table_bytes = 0;                                   // … and what they hold together
    std::unordered_map<uint64_t, int> checked_scenes;                // auto_scene_check: key of a scene -> the verdict it got (RTGR_OK or the refusal)
    Knobs knobs;
    // optional per-kernel timing (bench.py's roofline leg): hipEvents around each kernel of the pipeline
    bool timing = false;
    std::vector<TimedLaunch> timed;
    double acc_ms[6] = {0, 0, 0, 0, 0, 0};       // summed durations since the last read: [0..3] rtgr_timing_read, [4..5] rtgr_timing_read_exchange
    uint64_t acc_n[6] = {0, 0, 0, 0, 0, 0};
    std::vector<hipEvent_t> event_pool;
    // the host-pointer entry points' pipelines: [0] every blocking call's; [1] the second frame in flight of rtgr_trace_frames_*
    std::unique_ptr<Staging, void (*)(Staging*)> staging{nullptr, nullptr}, staging2{nullptr, nullptr};
#ifdef RTGR_ROOT_STATS
    unsigned long long* dbg = nullptr;
#endif
    hipEvent_t take_event() {
        if (!event_pool.empty()) { hipEvent_t e = event_pool.back(); event_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
    const UserModule* find_module(uint64_t id) const {
        for (auto& m : modules) if (m.id == id) return &m;
        return nullptr;
    }
};

struct KernelTimer {  // RAII: records start now, stop at scope exit
    DeviceCtx& d; hipStream_t st; int which; hipEvent_t a = nullptr, b = nullptr;
    KernelTimer(DeviceCtx& dc, hipStream_t s, int w) : d(dc), st(s), which(w) {
        if (d.timing) { a = d.take_event(); b = d.take_event(); (void)hipEventRecord(a, st); }
    }
    ~KernelTimer() {
        if (!a) return;
        (void)hipEventRecord(b, st);
        d.timed.push_back({a, b, which});
        // timing left on and never read: keep the newest launches only (their events go back to the pool)
        constexpr size_t CAP = 4096;
        if (d.timed.size() > CAP) {
            for (size_t i = 0; i < CAP / 2; i++) { d.event_pool.push_back(d.timed[i].a); d.event_pool.push_back(d.timed[i].b); }
            d.timed.erase(d.timed.begin(), d.timed.begin() + CAP / 2);
        }
    }
};

// what one pipeline launch needs from the context
struct LaunchEnv {
    DeviceCtx& d;
    StreamState& ss;
    const UserModule* user;  // the scene's unit (rtgr_scene.user_metric: RTGR_USER metric and / or RTGR_USER_OBJECT objects) or null
    hipEvent_t after_setup = nullptr;  // optional: recorded on the launch stream behind the ray set-up / queue-order kernels
    const Knobs* knobs = nullptr;      // this call's own launch options (the load-time probe, rtgr_scene_check); null: the device's
};

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
template <class R> size_t workspace_bytes(uint64_t rays, bool with_state);
template <class R> uint64_t pick_chunk(const DeviceCtx& d, const StreamState& ss, uint64_t n, bool with_state);
int ensure_workspace(DeviceCtx& d, StreamState& ss, size_t bytes, hipStream_t st);

// hipModuleLaunchKernel with the arguments given as C++ values
template <class... Args>
static inline hipError_t launch_module(hipFunction_t f, unsigned grid, unsigned block, hipStream_t st, Args... args) {
    void* params[] = {(void*)&args...};
    return hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, 0, st, params, nullptr);
}

// ---- the pipeline, one function per translation unit (each TU instantiates the kernels of its metric variants) ----------
int launch_f64_mink(LaunchEnv& E, const TraceArgs<double>& A, hipStream_t st);
int launch_f64_ksref(LaunchEnv& E, const TraceArgs<double>& A, bool spin, hipStream_t st);
int launch_f64_kstrue(LaunchEnv& E, const TraceArgs<double>& A, bool spin, hipStream_t st);
int launch_f64_generic(LaunchEnv& E, const TraceArgs<double>& A, hipStream_t st);  // KS_REF / KS_TRUE / RTGR_USER
int launch_f32_closed(LaunchEnv& E, const TraceArgs<float>& A, bool spin, hipStream_t st);  // all three built-ins
int launch_f32_generic(LaunchEnv& E, const TraceArgs<float>& A, hipStream_t st);
int launch_f64_grid(LaunchEnv& E, const TraceArgs<double>& A, hipStream_t st);   // RTGR_GRID (tu_f64_grid.hip)
int launch_f32_grid(LaunchEnv& E, const TraceArgs<float>& A, hipStream_t st);
int launch_f64_grid4(LaunchEnv& E, const TraceArgs<double>& A, hipStream_t st);   // a time-dependent grid (tu_f64_grid4.hip)
int launch_f32_grid4(LaunchEnv& E, const TraceArgs<float>& A, hipStream_t st);

// ---- small kernels (rtgr_misc.hip) -------------------------------------------------------------------------------------
// (templates over the scalar type: defined and instantiated for double and float in rtgr_misc.hip)
#define RTGR_INSTANTIATE_F64_F32(fn) template decltype(fn<double>) fn<double>; template decltype(fn<float>) fn<float>
template <class R>
int misc_canvas(const DevScene<R>& sc, const DevCamera<R>& cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t n, R* d_state0, hipStream_t st);
template <class R>
int misc_eval_metric(const DevScene<R>& sc, const R* d_x, uint64_t n, R* g, R* dg, R* Gam, hipStream_t st);
template <class R>
int misc_eval_geodesic(const DevScene<R>& sc, const R* d_s, uint64_t n, int path, R* d_ds, hipStream_t st);
template <class R>
int misc_eval_objects(const DevScene<R>& sc, const DevSolver<R>& opt, const R* d_x, uint64_t n, R* d, R* dmin, uint8_t* hit, R* rgb, hipStream_t st);
template <class R>
int misc_redshift(const DevScene<R>& sc, const DevCamera<R>& cam, const R* d_state0, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t jstride,
                  uint64_t n, uint64_t out_offset, const R* d_state_end, const uint8_t* d_hit, const uint32_t* d_hit32, R* d_red, hipStream_t st);
int misc_eval_fastmath_f64(const double* d_x, uint64_t n, double* d_rcp, double* d_rsq, hipStream_t st);
int misc_quantize(const double* d_rgb, uint64_t ni, uint64_t nj, uint8_t* d_img, hipStream_t st);
// multi-device gather on device 0: rows of rank r (cyclic over nranks) back into place; `planes` planes of `elem` T per ray
// (T = double / float / uint8_t)
template <class T>
int misc_place_rows(const T* d_part, uint64_t ni, uint64_t nj, uint64_t rank, uint64_t nranks, uint64_t planes, uint64_t elem, T* d_full, hipStream_t st);
int misc_poison_registers(int n_cu, unsigned pattern, hipStream_t st);   // the load-time probe's scrubber (rtgr_misc.hip)
// adaptive anti-aliasing (rtgr_aa.hip; include/rtgr.h "adaptive anti-aliasing"): the edge rule over a traced frame -> flag bytes (d_flag
// may be null) and the list of flagged pixels (*d_count entries, in no particular order; the caller zeroes *d_count on the stream) …
template <class R>
int aa_flag(const R* d_rgb, const uint32_t* d_hit32, const uint8_t* d_status, uint64_t ni, uint64_t nj, R contrast, bool all, uint8_t* d_flag,
            uint64_t* d_list, unsigned long long* d_count, hipStream_t st);
// … the k x k sub-rays of the npix listed pixels (states of the k ni x k nj canvas; a pixel's sub-rays contiguous, t outer, s inner) …
template <class R>
int aa_subrays(const DevScene<R>& sc, const DevCamera<R>& cam, uint64_t ni, uint64_t nj, uint32_t k, const uint64_t* d_list, uint64_t npix,
               R* d_state0, hipStream_t st);
// … and their colours (3 planes of npix k²) averaged into the listed pixels of d_rgb (3 planes of n)
template <class R>
int aa_reduce(const R* d_sub, const uint64_t* d_list, uint64_t npix, uint32_t k, R* d_rgb, uint64_t n, hipStream_t st);
// image textures (rtgr_shade.hip; include/rtgr.h "image textures").  A bind as the shading kernel reads it, resolved by the host at call
// time for one device and scalar type: the texels, the filter, and what the mapping needs of the caller's object — kind 0: rays that
// escape; RTGR_SPHERE: (a, b, c) = the centre; RTGR_DISK: a = r_in, b = r_out.
template <class R>
struct DevTexBind {
    const R* tex;
    uint32_t W, H, filter, kind;
    uint32_t object, pad;   // 1-based index in the caller's list (what hit32 holds); 0: the escape bind
    R a, b, c;
};
template <class R>
struct ShadeDesc {
    uint32_t nbind;
    R r_escape;
    DevTexBind<R> bind[RTGR_MAX_TEXTURE_BINDS];
};
// the shading kernel's argument block: n pixels, colour planes plane_stride apart
template <class R>
struct ShadeArgs {
    R* rgb;
    const uint32_t* hit32;
    const uint8_t* status;
    const R* state_end;
    uint64_t n, plane_stride;
    ShadeDesc<R> desc;
};
template <class R>
int shade_launch(const ShadeArgs<R>& A, hipStream_t st);
template <class R>
int eval_texture_launch(const R* d_tex, uint32_t W, uint32_t H, uint32_t filter, bool disk, R r_in, R r_out, const R* d_p, uint64_t n, R* d_rgb,
                        hipStream_t st);
// disk emission (rtgr_emit.hip; include/rtgr.h "disk emission").  The caller's rtgr_disk_emission as the kernels read it, converted by
// the host for one scalar type; r_in is the emitting disk's, from the caller's object list.
template <class R>
struct DevEmission {
    uint32_t object, emitter, flags, pad;
    R orbit, T_in, p, gain, r_in;
    R theta[3], weight[3];
};
// the observer camera (rtgr_observer.hip; include/rtgr.h "observer camera").  The caller's rtgr_observer as the frame kernel reads it,
// converted by the host for one scalar type: hx, hy = tan(fov / 2) for RTGR_PROJ_PERSPECTIVE, fov / 2 for RTGR_PROJ_EQUIRECT.
template <class R>
struct DevObserver {
    R pos[4], vel[4], look[4], up[4];
    R orbit, hx, hy;
    uint32_t kind, projection;
};
// … and what the frame kernel makes of it, once per call, in the stream's scratch: the metric at pos, the tetrad (rows e_0, e_right, e_up,
// e_look), Omega of a circular orbit (NaN for the other kinds) and whether the frame is valid.  The ray kernel and the emission kernel
// read it with scalar loads.
template <class R>
struct ObsFrame {
    R pos[4];
    R g[4][4];
    R e[4][4];
    R omega, hx, hy;
    uint32_t valid, projection;
};
// the frame kernel (one wave), and the ray kernel: the states of the n pixels from `first` on (row-major, i fastest) of the ni x nj canvas
template <class R>
int observer_frame_launch(const DevScene<R>& sc, const DevObserver<R>& ob, ObsFrame<R>* d_frame, hipStream_t st);
template <class R>
int observer_rays_launch(const ObsFrame<R>* d_frame, uint64_t ni, uint64_t nj, uint64_t first, uint64_t n, R* d_state0, hipStream_t st);
// the emission kernel's argument block.  Frame mode (hit32 given): n pixels, colour planes plane_stride apart (pixel_stride 1), g: the
// frequency ratio per pixel (may be null); state0: the rays' start states when they were caller-supplied (the sub-rays of anti-aliasing),
// null: pixel idx of the ni x nj canvas of cam.  Point mode (hit32 null; rtgr_eval_disk_emission_*): n pairs (state0, state_end), every
// output optional, rgb n x 3 (plane_stride 1, pixel_stride 3).  (Aggregate initialisation without the last member leaves obs null.)
template <class R>
struct EmitArgs {
    R* rgb;
    R* g;
    R* omega;
    R* u_emit;
    const uint32_t* hit32;
    const R* state_end;
    const R* state0;
    uint64_t n, plane_stride, pixel_stride, ni, nj;
    DevScene<R> sc;
    DevCamera<R> cam;
    DevEmission<R> em;
    const ObsFrame<R>* obs;   // null: u_obs is the static observer at the ray's start; else the e_0 of this frame (rtgr_trace_observer_*)
};
template <class R>
int emit_launch(const EmitArgs<R>& A, hipStream_t st);
// What is applied to a traced frame before anyone reads its colours: the textures of a shaded frame, then the emission of a disk —
// either may be null.  d_g: the frequency ratios of the pixel-centre rays (pass 1 of trace_aa_on, rtgr_aa_host.hip), or null.
template <class R>
struct AfterTrace {
    const ShadeDesc<R>* shade = nullptr;
    const DevEmission<R>* emit = nullptr;
    R* d_g = nullptr;
};
// … and the run of pixels a trace just wrote that it is applied to (after_trace, rtgr_frame_host.hip), every member by name
template <class R>
struct TracedPixels {
    R* rgb = nullptr;                     // the run's colours: three planes …
    uint64_t plane_stride = 0;            // … this far apart
    R* g = nullptr;                       // the frequency ratio per pixel, or null
    const uint32_t* hit32 = nullptr;      // what the trace delivered of the run
    const uint8_t* status = nullptr;      // (read by the shading kernel only)
    const R* state_end = nullptr;
    const R* state0 = nullptr;            // the rays' start states when they were caller-supplied; null: pixel idx of the ni x nj canvas of cam
    const ObsFrame<R>* obs = nullptr;     // the observer whose e_0 is u_obs; null: the static observer at the ray's start
    uint64_t n = 0, ni = 0, nj = 0;
    const DevScene<R>* sc = nullptr;      // what the emission kernel reads of the scene and the camera (null where nothing emits;
    const DevCamera<R>* cam = nullptr;    // cam also where state0 is given)
};
// hot-spot light curves (rtgr_lightcurve.hip; include/rtgr.h "hot-spot light curves").  The caller's rtgr_hot_spot as the kernels read
// it, in double whatever the entry's scalar type: inv_2s2 = 1 / (2 sigma²), r2_cut = (cut sigma)², e_cut = exp(-cut² / 2).
struct LcSpot {
    double rho_s, phi0, inv_2s2, r2_cut, cut_sigma, e_cut, amp, q, t_start, dt;
};
// what every reduction of a traced frame reads (rtgr_reduce.hpp, which the trace's units do not include): the planes of the frame and
// the pixel weight
template <class R> struct ReducePlanes;
struct PixelWeight;
// The head of the stream's reduction scratch in a light-curve call (LC_HEAD bytes): the synthetic pair of states and the synthetic observer
// record the emission kernel evaluates in point mode, and the Omega_s it writes (scalar type R), at these offsets.  Behind it: the partial sums.
constexpr size_t LC_HEAD = 1024, LC_HEAD_S0 = 0, LC_HEAD_SE = 64, LC_HEAD_OMEGA = 128, LC_HEAD_FRAME = 256;
static_assert(LC_HEAD_FRAME + sizeof(ObsFrame<double>) <= LC_HEAD, "the head holds the record");
// the states and the record for a spot at rho_s into the head (one wave) …
template <class R> int lc_seed_launch(R rho_s, char* d_head, hipStream_t st);
// … the reduction (rtgr_reduce.hpp: reduce_launch): nt x 3 doubles into d_lc, pass by pass over the time axis — the partial sums of a pass
// in d_partial, then their sum in range order (NaN everywhere when the head's Omega_s is not finite) …
template <class R>
int lc_reduce_launch(const ReducePlanes<R>& P, const LcSpot& S, const PixelWeight& W, uint64_t nt, const char* d_head, double* d_partial, double* d_lc,
                     hipStream_t st);
// … and the hook: j at n triples (x, y, t), from the same device functions
template <class R> int lc_points_launch(const R* d_xyt, uint64_t n, const LcSpot& S, const char* d_head, double* d_j, hipStream_t st);
// disk spectra (rtgr_spectrum.hip; include/rtgr.h "disk spectra").  The caller's rtgr_spectrum as the kernels read it, in double whatever
// the entry's scalar type: LINE: s = nb / (hi - lo); THERMAL: span = hi - lo, or log(hi / lo) with RTGR_SPEC_LOG.  `em`: the emitter's
// record in double (the temperature law and the gain of THERMAL).
struct SpecDev {
    uint32_t kind, flags;
    uint64_t nb;
    double lo, hi, s, span;
    double amp, alpha, rho_min, rho_max, q;
    DevEmission<double> em;
};
// the reduction (rtgr_reduce.hpp: reduce_launch): nb x 3 doubles into d_out, pass by pass over the spectral axis — the partial sums of a
// pass in d_partial, then their sum in range order (times c_k for THERMAL) …
template <class R>
int spec_reduce_launch(const ReducePlanes<R>& P, const SpecDev& S, const PixelWeight& W, double* d_partial, double* d_out, hipStream_t st);
// … and the hook: the axis (nb), and bin and val at n triples (x, y, g), from the same device functions; any output may be null
template <class R>
int spec_points_launch(const R* d_xyg, uint64_t n, const SpecDev& S, double* d_axis, int64_t* d_bin, double* d_val, hipStream_t st);
// polarized disk images (rtgr_polarize.hip; include/rtgr.h "polarized disk images").  The caller's rtgr_polarization as the kernel reads
// it, converted by the host for one scalar type.
template <class R>
struct DevPolarization {
    uint32_t kind, pad;
    R deg0, deg1;
    R field[3];
};
// the polarization kernel's argument block.  mode POL_FRAME: n pixels, hit32 given; q, u, aux: a plane each, every one optional.
// POL_POINTS (rtgr_eval_polarization_*): n pairs (state0, state_end), every output optional.  POL_FORMS (rtgr_eval_walker_penrose_*): n
// states (state0) and n vectors (fvec) into kappa.  The start states are read, never regenerated.
enum PolMode : uint32_t { POL_FRAME = 0, POL_POINTS = 1, POL_FORMS = 2 };
template <class R>
struct PolArgs {
    R* q;
    R* u;
    R* aux;
    R* kappa;     // n x 2 (POL_POINTS, POL_FORMS)
    R* f_em;      // n x 4 (POL_POINTS)
    R* delta;     // n     (POL_POINTS)
    int* valid;   // n     (POL_POINTS)
    const uint32_t* hit32;
    const R* state0;
    const R* state_end;
    const R* fvec;   // n x 4 (POL_FORMS)
    uint64_t n;
    uint32_t mode, pad;
    DevScene<R> sc;
    DevEmission<R> em;
    DevPolarization<R> pol;
    const ObsFrame<R>* obs;
};
template <class R>
int polarize_launch(const PolArgs<R>& A, hipStream_t st);
// what an observer trace applies to each batch behind the emission kernel when the call is rtgr_trace_polarized_*: the record and the
// caller's three planes (whole frames; aux may be null)
template <class R>
struct PolStage {
    DevPolarization<R> pol;
    R* q = nullptr;
    R* u = nullptr;
    R* aux = nullptr;
};
// volume emission (tu_transfer_f64.hip / tu_transfer_f32.hip; include/rtgr.h "volume emission"; the model and the kernels:
// rtgr_transfer.hpp).  The caller's rtgr_flow as the kernels read it, converted by the host for one scalar type.
template <class R>
struct DevFlow {
    uint32_t emitter, pad;
    R orbit, j0, kappa, r0, alpha, H, s, r_stop, gain;
    R weight[3];
};
// the transfer kernel's argument block.  Frame mode (ni > 0): a batch of nrows rows of ni pixels — state0 the batch's start states
// (nrows ni x 8); lambda_end, status (the trace's), rgb (three planes plane_stride apart) and the four optional planes I, tau, tstatus,
// tsteps already point at the batch's first pixel.  List mode (ni == 0; rtgr_eval_transfer_*): n rays, status and rgb null, s_end
// (n x 8) optional as well.  counters: the eight words of an rtgr_counters of the transfer pass, or null.
template <class R>
struct TransferArgs {
    const R* state0;
    const R* lambda_end;
    const uint8_t* status;
    R* rgb;
    R* I;
    R* tau;
    uint8_t* tstatus;
    uint32_t* tsteps;
    R* s_end;
    unsigned long long* counters;
    const ObsFrame<R>* obs;   // null: u_obs is the static observer at the ray's start
    uint64_t ni, nrows, n, plane_stride;
    DevScene<R> sc;
    DevSolver<R> opt;
    DevFlow<R> fl;
};
// the instantiation the scene's (metric, a) selects — the closed right-hand side also under RTGR_METRIC_GENERIC
template <class R>
int transfer_launch(const TransferArgs<R>& A, hipStream_t st);
// the pointwise hook's argument block (rtgr_eval_flow_*): n pairs (state0, state); every output optional
template <class R>
struct FlowArgs {
    const R* state0;
    const R* state;
    R* dens;
    R* omega;
    R* u_f;
    R* gfac;
    R* dtau;
    R* dI0;
    const ObsFrame<R>* obs;
    uint64_t n;
    DevScene<R> sc;
    DevFlow<R> fl;
};
template <class R>
int flow_launch(const FlowArgs<R>& A, hipStream_t st);
// what an observer trace applies to each batch behind its post-trace stage when the call is rtgr_trace_transfer_*: the record, the
// caller's four planes (whole frames; each may be null) and the device counters of the transfer pass (or null)
template <class R>
struct TransferStage {
    DevFlow<R> fl;
    R* I = nullptr;
    R* tau = nullptr;
    uint8_t* tstatus = nullptr;
    uint32_t* tsteps = nullptr;
    rtgr_counters* tctr = nullptr;      // the caller's (host) record: filled behind the call's one synchronisation
};

}  // namespace rtgr
