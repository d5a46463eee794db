/*
 * rtgr.h — C ABI of the MI355X-native geodesic ray tracer (librtgr_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of eschnett/RayTraceGR.jl: the per-pixel
 * geodesic integration + object intersection + colouring that the reference performs in
 *
 *     trace_rays(metric, objs::Vector{Object{T}}, c::Canvas{T})   src/RayTraceGR.jl:482-536
 *
 * i.e. everything between building the EnsembleProblem (:488-509), the
 * `solve(probs, Tsit5(), callback=cb, trajectories=N, reltol=tol, abstol=tol)` call (:510-511) and the
 * colouring loop (:513-533), plus the camera that feeds it (make_canvas, :457-478) and the legacy
 * single-ray shape `trace_ray(metric, objs, cb, p)::Pixel` (test/runtests.jl:65-79).
 *
 * Every entry point is plain C: pointers, sizes, PODs.  No torch / C++ types cross this line.
 * A Julia `ccall`, a Python `ctypes` or a C caller bind exactly these symbols.
 *
 * Conventions
 *  - Coordinates are (t, x, y, z); D = 4 (src/RayTraceGR.jl:253-254).
 *  - A ray state is 8 scalars (x^a, u^a) — `r2s(Ray{T}(x,u))` (src/RayTraceGR.jl:345-347).
 *  - Pixels are indexed as the reference's column-major `pixels[i,j]`: linear index i + j*ni (0-based),
 *    i fastest.  A slab is the j-range [j0, j1); its local linear index is i + (j-j0)*ni.
 *  - RGB output is three planes (SoA) of n = ni*(j1-j0) scalars each: rgb[c*n + idx]
 *    (what `colorview(RGB, R', G', B')` consumes, src/RayTraceGR.jl:566-569).
 *  - All functions return 0 on success and a negative rtgr_status on failure; they never throw or abort.
 *    The message of the last failure on the calling thread is rtgr_last_error().
 *  - The library never keeps a caller pointer after a call returns.
 *
 * Contexts, ownership, threading
 *  - All device state — workspaces, work-queue heads, run-time loaded metric modules, staging buffers, streams,
 *    timing events, launch-policy options — lives in an opaque rtgr_context created for a list of devices
 *    (rtgr_create).  Every entry point takes the context first; NULL means the process's DEFAULT context, which is
 *    created on first use on the calling thread's current HIP device (or by rtgr_init).  There is no other global state.
 *  - The reference's caller is ONE thread and the parallelism is inside the call (src/RayTraceGR.jl:510-511).  The
 *    same holds here, and more: one host thread can drive every device of a context (rtgr_trace_sharded_f64 deals the
 *    image rows to all of them and collects the frame on device 0 — one call, no MPI / torch / second process), and
 *    several host threads may use one context concurrently.
 *  - Device entry points are asynchronous on the caller's stream.  Two calls on the SAME stream are ordered by the
 *    stream and share that stream's workspace; calls on DIFFERENT streams (or devices) use different workspaces and
 *    may run concurrently.  Results are bit-identical to serial execution either way (tests: two streams, two threads).
 *  - A workspace only grows.  The superseded allocation stays alive until rtgr_trim / rtgr_destroy, so a hipGraph
 *    captured earlier never dangles; growth DURING stream capture is refused with RTGR_ERR_BAD_ARG (hipMalloc cannot be
 *    captured): call rtgr_reserve_workspace before capturing.  The device tables of object lists longer than
 *    RTGR_MAX_OBJECTS are covered by the same promise: one that a captured call uses stays until rtgr_trim / rtgr_destroy.
 */
#ifndef RTGR_H
#define RTGR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 5): run-time units may carry OBJECTS (RTGR_USER_OBJECT) and a resolve kernel; rtgr_object.reserved became .type;
 * the device-side record layout changed in round 4 (event-record tails, RecRef) without a bump — a unit built against the
 * older headers would have loaded and overrun the workspace.  Units also carry a hash of the device headers they were built
 * from (rtgr_user_header_hash), checked at load. */
/* 4 (round 6): `objs::Vector{Object{T}}` has no length limit in the reference (src/RayTraceGR.jl:433-441, :483, :520-526) and has none
 * here any more: rtgr_scene.objects (a caller array of any length) beside the 16 inline slots; rtgr_ray_outputs.hit32; frames in
 * flight (rtgr_trace_frames_*); rtgr_scene_check runs by itself the first time a scene with user objects is traced. */
#define RTGR_ABI_VERSION 4
#define RTGR_MAX_OBJECTS 16         /* objects held INLINE in rtgr_scene.obj; a longer list goes through rtgr_scene.objects */
#define RTGR_OBJECTS_LIMIT 1048576  /* sanity bound on rtgr_scene.nobj (2^20; beyond ~10^4 the per-step cost grows as nobj / 64)  */
#define RTGR_MAX_DEVICES 16
#define RTGR_MAX_SOURCES 16         /* object sources rtgr_user_source_join joins in one call                               */
#define RTGR_MAX_SAMPLES 32         /* type tags 0 .. 31 of a unit are asked for a sample object (rtgr_user_sample)         */

/* ---- return codes -------------------------------------------------------------------------------------- */
enum rtgr_status {
    RTGR_OK = 0,
    RTGR_ERR_BAD_ARG = -1,     /* null pointer, bad enum, empty/oversized range ...                           */
    RTGR_ERR_NO_DEVICE = -2,   /* no usable HIP device; the library has NO CPU fallback                       */
    RTGR_ERR_HIP = -3,         /* a HIP runtime call failed (message has the hipError string)                 */
    RTGR_ERR_NAN_INPUT = -4,   /* NaN in an input ray — the reference's `@assert !any(isnan,…)` (:279)        */
    RTGR_ERR_NOT_INIT = -5
};

/* ---- metric: replaces the `metric` callable argument (src/RayTraceGR.jl:262-264, :274-294) -------------- */
enum rtgr_metric {
    RTGR_MINKOWSKI = 0, /* minkowski(x)                                           src/RayTraceGR.jl:262-264   */
    RTGR_KS_REF = 1,    /* kerr_schild(x) exactly AS WRITTEN, r = sqrt(rho^2-a^2)/2 + sqrt(a^2 z^2+((rho^2-a^2)/2)^2)
                           (src/RayTraceGR.jl:284); the reference hard-wires M=1, a=0 (:275-276)               */
    RTGR_KS_TRUE = 2,   /* textbook Kerr–Schild radius r^2 = (q + sqrt(q^2 + 4 a^2 z^2))/2, q = rho^2 - a^2
                           (no reference counterpart; needed for a != 0 configs)                               */
    RTGR_USER = 3,      /* the metric function rtgr_scene.user_metric names (rtgr_user_metric_load); always traced
                           with the generic dual-number RHS (RTGR_METRIC_GENERIC is implied)                   */
    RTGR_GRID = 4       /* a stationary metric given as SAMPLES on a uniform 3-D grid: rtgr_scene.user_metric holds the
                           grid's id (rtgr_grid_metric_load, below).  Always the generic contraction (RTGR_GRID |
                           RTGR_METRIC_GENERIC means the same).                                                */
};

/* OR-ed into rtgr_scene.metric: evaluate the geodesic RHS the way the reference does for ANY metric callable — 4-wide
 * forward duals through the metric, symmetric g / dg, 4x4 inverse, Christoffel contraction (the "generic" path of
 * DESIGN.md §4.2) — instead of the closed Kerr–Schild contraction.  Same results to rounding; ~5x the flops.  It is the
 * path a new (non-Kerr–Schild-form) metric functor would take, and the one whose executed flops equal the algorithmic
 * count of SURVEY §8(d).  Float64 and Float32 (the reference's own test runs T = Float32 through it, test/runtests.jl:37). */
#define RTGR_METRIC_GENERIC 0x100u

/* ---- objects: replaces Vector{Object{T}} (src/RayTraceGR.jl:374-428); ORDER MATTERS (:518-530) ---------- */
enum rtgr_object_kind {
    RTGR_PLANE = 1,  /* Plane{T}(time)            p[0] = time                     src/RayTraceGR.jl:394-404  */
    RTGR_SPHERE = 2, /* Sphere{T}(pos, vel, radius)  p[0..3]=pos  p[4..7]=vel  p[8]=radius   (:409-413)
                        vel is dead data in the reference (:411, "TODO: Use metric?" :416); here it is the emitter's
                        coordinate 4-velocity for the optional redshift output (rtgr_ray_outputs.redshift)       */
    RTGR_DISK = 3,   /* thin disk (no reference counterpart): p[0]=half thickness h, p[1]=r_in, p[2]=r_out;
                        distance = max(|z|-h, r_in-rho_cyl, rho_cyl-r_out) obeying the contract at :377-383    */
    RTGR_USER_OBJECT = 4 /* a NEW subtype of the reference's open `abstract type Object{T}` (:374-389): its two methods,
                        `distance(obj, pos)::T` and `objcolor(obj, pos)::SVector{3,T}`, are given as device source and
                        compiled at run time into the scene's unit (rtgr_user_unit_compile, below); `type` tells the
                        caller's own object types apart inside that source, p[0..8] are the object's fields           */
};

typedef struct rtgr_object {
    uint32_t kind; /* rtgr_object_kind */
    uint32_t type; /* RTGR_USER_OBJECT: the tag handed to rtgr_user_distance / rtgr_user_objcolor; 0 otherwise */
    double p[9];
} rtgr_object;

typedef struct rtgr_scene {
    uint32_t metric; /* rtgr_metric (| RTGR_METRIC_GENERIC) */
    uint32_t nobj;   /* length of the object list: 0..RTGR_MAX_OBJECTS in obj[], or any number (<= RTGR_OBJECTS_LIMIT) in objects[] */
    double M;        /* mass  (reference: 1, :275) */
    double a;        /* spin  (reference: 0, :276) */
    uint64_t user_metric; /* RTGR_GRID: the id of the grid (rtgr_grid_metric_load).  Otherwise: the id of the run-time compiled UNIT this scene is written for — the module that carries the kernels
                             of a user metric (RTGR_USER), of user objects (RTGR_USER_OBJECT), or of both
                             (rtgr_user_metric_load / _compile, rtgr_user_unit_compile); a scene can never run with another
                             unit's kernels.  0: built-in metric and built-in objects only. */
    rtgr_object obj[RTGR_MAX_OBJECTS];
    const rtgr_object* objects; /* NULL: the list is obj[0 .. nobj).  Otherwise the WHOLE list, nobj objects in the caller's (host)
                             memory, and obj[] is not read — `objs::Vector{Object{T}}` of any length (src/RayTraceGR.jl:433-441, :483).
                             Read during the call only, like every caller pointer.  On the device the first RTGR_MAX_OBJECTS
                             objects travel in the kernels' argument block as before; a longer list sits, whole, in a device table
                             the context keeps per distinct list (uploaded when a list is first seen — blocking, microseconds; a
                             first sight during hipGraph capture is refused: trace the scene once before capturing), its spheres
                             sorted into groups of neighbours that the kernels ask before their members (option "groups").  Cost:
                             64 objects ~1.8 x, 256-512 objects ~1.5-1.85 x the 3-object frame. */
} rtgr_scene;

/* ---- solver constants (src/RayTraceGR.jl:485, :497, :510-511, :519, :528; OrdinaryDiffEq 5.38 defaults) -- */
typedef struct rtgr_solver {
    double reltol;        /* eps(T)^(3/4)                                       :485               */
    double abstol;        /* eps(T)^(3/4)                                       :485               */
    double lambda0;       /* 0                                                  :497               */
    double lambda1;       /* 100                                                :497               */
    double hit_threshold; /* 0.01                                               :519               */
    double miss_rgb[3];   /* (1,0,0)                                            :528               */
    uint32_t max_steps;   /* step-attempt cap per ray (reference: maxiters, never binds)           */
    uint32_t interp_points; /* ContinuousCallback interp_points = 10 (DiffEqBase 6.35 default)      */
} rtgr_solver;

/* ---- camera: arguments of make_canvas (src/RayTraceGR.jl:458-462) ---------------------------------------- */
typedef struct rtgr_camera {
    double pos[4];
    double widthx[4];
    double widthy[4];
    double normal[4];
} rtgr_camera;

/* ---- per-ray status byte (the reference ignores solver retcodes, :502-505; we report them) -------------- */
enum rtgr_ray_status {
    RTGR_RAY_EVENT = 0,     /* terminated by the ContinuousCallback (terminate!, :489)      */
    RTGR_RAY_LAMBDA1 = 1,   /* reached lambda1 without an event                              */
    RTGR_RAY_MAXSTEPS = 2,  /* hit max_steps                                                 */
    RTGR_RAY_DTMIN = 3,     /* step size underflow                                           */
    RTGR_RAY_NAN = 4,       /* state became non-finite                                       */
    RTGR_RAY_OUTSIDE = 5    /* RTGR_GRID only: the ray left the grid's valid box before any event
                               (counted in not_finished; coloured like a ray that reached lambda1) */
};

/* ---- counters accumulated over a call (8 x uint64) -------------------------------------------------------- */
typedef struct rtgr_counters {
    uint64_t rays;
    uint64_t accepted;        /* accepted Tsit5 steps                                         */
    uint64_t rejected;        /* rejected Tsit5 step attempts                                 */
    uint64_t rhs_evals;       /* geodesic RHS evaluations actually executed                   */
    uint64_t events;          /* rays terminated by an event                                  */
    uint64_t events_interior; /* events found only by the interior dense-output sample points */
    uint64_t not_finished;    /* rays with status >= RTGR_RAY_MAXSTEPS                        */
    uint64_t reserved;
} rtgr_counters;

/* optional per-ray outputs; any member may be NULL.  Device or host pointers according to the call. */
typedef struct rtgr_ray_outputs {
    void* state_end;      /* n x 8 scalars (AoS)  — `sols.u[i]` (src/RayTraceGR.jl:516)                    */
    void* lambda_end;     /* n scalars            — `sol.t[end]` (:503)                                     */
    uint8_t* status;      /* n x rtgr_ray_status                                                            */
    uint8_t* hit;         /* n: omin of the colouring rule (0 = miss, else 1-based object index, :518-526); scenes of
                             more than 255 objects: RTGR_ERR_BAD_ARG, ask for hit32 instead                        */
    uint32_t* n_accept;   /* n: accepted steps per ray                                                      */
    uint32_t* n_reject;   /* n: rejected attempts per ray                                                   */
    void* redshift;       /* n scalars: g = (k.u_obs)/(k.u_emit), the frequency ratio observed/emitted of the light that
                             reaches the pixel (k = the ray's tangent, . = the metric's inner product).  u_obs = the
                             camera's static observer at the pixel, future-directed: -g^-1 e_t normalised (make_canvas
                             builds its past-directed rays from +g^-1 e_t, :471-472); u_emit = the hit Sphere's `vel`
                             (:411; a future-directed coordinate 4-velocity such as the examples' (1,0,0,0)) normalised
                             at the end point, or the static observer there for planes / disks; NaN where the ray hits
                             nothing or u_emit is not timelike.
                             No reference counterpart (`vel` is stored and never used, :411, :416).  Every metric
                             (built-in, run-time compiled) and both scalar types, like `Sphere{T}` and the metric
                             argument of the reference (:409-413, :302-309); n scalars of the entry point's type. */
    uint32_t* hit32;      /* n: omin as 32 bits — for object lists of any length (may be asked for beside `hit`)              */
} rtgr_ray_outputs;

/* ---- lifecycle --------------------------------------------------------------------------------------------- */
typedef struct rtgr_context rtgr_context;

/* A context over n_devices HIP devices (device_ids[k] = HIP ordinal; the same ordinal may appear more than once: each
 * entry gets streams and workspaces of its own).  device_ids == NULL: the calling thread's current device. */
int rtgr_create(const int* device_ids, int n_devices, rtgr_context** ctx_out);
int rtgr_destroy(rtgr_context* ctx);
/* number of devices of the context (negative rtgr_status on error) */
int rtgr_context_devices(rtgr_context* ctx);
/* Synchronise the context's devices and free retired workspaces (and staging buffers). */
int rtgr_trim(rtgr_context* ctx);
/* (Re)create the process's default context on HIP device `device` (< 0: the current device).  Optional: the default
 * context is otherwise created on first use. */
int rtgr_init(int device);
/* Destroy the default context. */
int rtgr_shutdown(void);
const char* rtgr_last_error(void);
/* (The library also exports `rtgr_testhook_*` symbols — host-only probes of internal layouts for the CPU tests, e.g. how a long object
 * list's spheres are grouped — and, in debug builds, `rtgr_debug_*`: neither is part of this ABI; nothing outside tests/ may bind them.) */
int rtgr_abi_version(void);
/* Fill `s` with the reference's constants for T = Float64 (is_f32 = 0) or Float32 (is_f32 = 1). */
int rtgr_solver_defaults(rtgr_solver* s, int is_f32);
/* Name / CU count / clock of device `index` of the context, for bench reports. */
int rtgr_device_info(rtgr_context* ctx, int index, char* name, uint64_t name_len, int* n_cu, int* clock_mhz, int* wavefront);

/* Launch-policy options (experiments and schedule-invariance tests).  Names: "waves_per_cu", "waves_per_cu_near", "chunk",
 * "split", "order", "fair", "near_early", "far4", "rounds", "handback_after", "qchunk", "qchunk_near", "host_chunk", "peer" (multi-device gather:
 * 0 = through the host, 1 = peer copies or fail) — these decide WHEN and WHERE a ray is integrated and never change a result
 * bit —, and three that select another FORMULATION of the same algorithm, with results equal up to rounding: "tile" (1: the
 * simple tile-per-wave kernel), "pack" (Float32: 0 = one ray per lane, 1 = two rays per lane in packed arithmetic) and "packfar"
 * (Float32 experiment, default 0: 1 = the packed kernel without its scan as a FAR pass + the scalar NEAR pass; measured slower).
 * value -1 = automatic.  Initial values come from the environment variables RTGR_<NAME> read ONCE when the context is created.
 * "scene_check" (default 1): the automatic first-trace check of scenes with user objects (see "user objects" below); 0 = off.
 * "groups" (default 1): object lists longer than RTGR_MAX_OBJECTS have their spheres sorted into groups of neighbours, each with a
 * bounding sphere that the per-step reach test asks first, and the event root-find narrows the list to the objects the event's step
 * can meet; 0 = every object is asked every time (A/B and tests: the frames are equal bit for bit); a value >= 2 = that many spheres
 * per group at most instead of 8 (experiments: 8 is the measured optimum for 32-256 objects).  In Float64 no option changes
 * a result bit except "tile" / "pack"; in Float32 "split" (and "groups", "rounds" through it) selects kernels whose compiled
 * arithmetic differs in the last bit, as "pack" does — Float32 lists of 32 objects and more run the FAR + NEAR pair by default.
 * Two options govern how run-time units are LOADED: "unit_audit" (default 1; 0 = skip the audit of the code object for the
 * compiler's EXEC-flip fault) and "unit_probe" (default 1; 0 = skip the load-time probe) — test hooks, see rtgr_user_metric_load. */
int rtgr_set_option(rtgr_context* ctx, const char* name, long value);
int rtgr_get_option(rtgr_context* ctx, const char* name, long* value);

/* The device entry points never allocate once the stream's workspace (start / hand-over / event records, per-ray meta,
 * queue order: 213 B per ray, 373 B when end states are asked for; bounded by a pipeline chunk of 2^26 rays — fewer when that would not fit a quarter of
 * the free device memory) is large enough.  Call this once up front (e.g. before hipGraph capture) to size the workspace
 * of `stream` on the device that owns `d_any` (any device pointer of the later call; NULL: device 0 of the context). */
int rtgr_reserve_workspace(rtgr_context* ctx, const void* d_any, void* stream, uint64_t n_rays, int with_state_end, int is_f32);

/* Optional per-kernel timing for benchmarks: when enabled the library brackets every kernel it launches on device
 * `index` with HIP events on the launch stream.  rtgr_timing_read waits for them and returns, since the previous read,
 * the summed milliseconds and launch counts of [0] the ray set-up and queue-order kernels, [1] the integrate kernel's main
 * pass (FAR, or FULL when the far/near split is off — the hot kernel), [2] the resolve kernel, [3] the integrate kernel's
 * NEAR pass.  Not for use during hipGraph capture. */
int rtgr_timing_enable(rtgr_context* ctx, int index, int on);
int rtgr_timing_read(rtgr_context* ctx, int index, double ms[4], uint64_t launches[4]);
/* … and of the multi-device exchange of rtgr_trace_sharded_device_* on device `index`, since the previous read: [0] this device's
 * rows leaving it for device 0 (the peer copy, or the device -> pinned host leg of the fallback), measured on the source device's
 * stream behind its trace; [1] device 0 only: the placement kernels that put the ranks' rows back into the frame. */
int rtgr_timing_read_exchange(rtgr_context* ctx, int index, double ms[2], uint64_t launches[2]);
/* Peer access between device 0 and device `index` of the context as rtgr_create established it: 1 = peer copies (or the same
 * physical device, or index 0), 0 = not available — the gather then stages that device's rows through pinned host memory — with
 * the reason copied into `why` (may be NULL).  Negative rtgr_status on error. */
int rtgr_peer_access(rtgr_context* ctx, int index, char* why, uint64_t why_len);

/* ---- the hot path, device-resident buffers ------------------------------------------------------------------
 * Replaces the body of trace_rays (src/RayTraceGR.jl:482-536) for rows j in [j0, j1) of an ni x nj canvas.
 *   d_state0 : n x 8 initial ray states on the DEVICE (n = ni*(j1-j0)), as `input_func(i)` yields (:492-496),
 *              or NULL — then rays are generated on the device from `cam` exactly as make_canvas does (:464-476).
 *   d_rgb    : 3*n scalars on the device, plane-major (required).  The device of the context that owns this
 *              pointer runs the call.
 *   out      : optional per-ray device outputs.
 *   d_counters : optional device pointer to one rtgr_counters; the call ADDS to it (caller zeroes it).
 *   stream   : hipStream_t to enqueue on (NULL = default stream).  The call is asynchronous: it only enqueues.
 */
int rtgr_trace_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const double* d_state0,
                          const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1,
                          double* d_rgb, const rtgr_ray_outputs* out, rtgr_counters* d_counters, void* stream);
int rtgr_trace_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const float* d_state0,
                          const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1,
                          float* d_rgb, const rtgr_ray_outputs* out, rtgr_counters* d_counters, void* stream);

/* Strided rows: traces image rows j0, j0+jstride, …, j0+(nrows-1)*jstride of the camera's ni x nj canvas (rays generated
 * on the device); local row k of the output planes (n = ni*nrows) is image row j0 + k*jstride.  jstride = 1 is a
 * contiguous slab; jstride = N, j0 = rank is the CYCLIC row split used for multi-GPU runs — contiguous slabs of a
 * black-hole image are unbalanced (rows through the hole cost ~1.8x the edge rows), cyclic rows are not. */
int rtgr_trace_rows_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam,
                               uint64_t ni, uint64_t nj, uint64_t j0, uint64_t jstride, uint64_t nrows, double* d_rgb,
                               const rtgr_ray_outputs* out, rtgr_counters* d_counters, void* stream);
int rtgr_trace_rows_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam,
                               uint64_t ni, uint64_t nj, uint64_t j0, uint64_t jstride, uint64_t nrows, float* d_rgb,
                               const rtgr_ray_outputs* out, rtgr_counters* d_counters, void* stream);

/* ---- the hot path, host buffers (what a Julia ccall passes) ---------------------------------------------------
 * Same semantics with HOST pointers; the library stages through pinned buffers of the context, pipelines H2D copy /
 * integration / D2H copy of successive pieces on three streams, and blocks until done.
 *   state0 may be NULL (device-side make_canvas from `cam`).  `ctr` (host, optional) is overwritten.
 * EVERY device of the context takes part (the reference's caller is `trace_rays(metric, objs, canvas)`,
 * src/RayTraceGR.jl:483-484, :560, :596 — one call, parallel inside): the rows of the slab are dealt cyclically, device k
 * of N takes slab rows k, k+N, …; each device is driven by a host thread of its own inside the call, uploads ITS rows from
 * the caller's array and downloads them straight back into it over its own PCIe link (no hop through device 0, no peer
 * copies); counters are summed.  The results do not depend on the number of devices, bit for bit.  A context of one device
 * (the default context) runs on the calling thread.
 */
int rtgr_trace_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const double* state0,
                   const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, double* rgb,
                   const rtgr_ray_outputs* out, rtgr_counters* ctr);
int rtgr_trace_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const float* state0,
                   const rtgr_camera* cam, uint64_t ni, uint64_t nj, uint64_t j0, uint64_t j1, float* rgb,
                   const rtgr_ray_outputs* out, rtgr_counters* ctr);

/* Accepts the reference's own pixel array: `pointer(c.pixels)` of an Array{Pixel{Float64},2} — 11 doubles per
 * pixel (pos 4, normal 4, rgb 3; src/RayTraceGR.jl:446-450), column-major ni x nj.  Traces every pixel and
 * writes rgb back into the same AoS layout of `pixels_out` (may alias pixels_in), as trace_rays does (:532). */
int rtgr_trace_pixels_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const double* pixels_in,
                          uint64_t ni, uint64_t nj, double* pixels_out, rtgr_counters* ctr);
/* ... of an Array{Pixel{Float32},2}: 11 floats (44 bytes) per pixel — `Canvas{T}` is generic in T (:452-455). */
int rtgr_trace_pixels_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const float* pixels_in,
                          uint64_t ni, uint64_t nj, float* pixels_out, rtgr_counters* ctr);

/* ---- several frames in one call, two in flight ------------------------------------------------------------------------
 * AN EXTENSION: the reference renders one frame per call (example1 / example2, src/RayTraceGR.jl:560, :596).  A render loop delivers
 * frame after frame, and every frame's pipeline ends thin (the last rays of the FAR pass, the long stayers of the NEAR pass, the
 * last download); with two frames in flight the thin end of one overlaps the start of the next — 8-11 % per frame at 1024², 5 % for
 * one GPU's share of a 4096² frame split eight ways.  A caller that owns two HIP streams gets that from the
 * device entry points; these calls give it to the blocking ones: nframes frames of ONE scene and canvas size, frame k from cams[k]
 * (rays generated on the device), or from state0s[k] (ni*nj x 8 ray states; state0s may be NULL, and so may single entries when cams
 * is given), into rgb[k] (3 planes of ni*nj), outs[k] (outs may be NULL) and ctrs[k] (may be NULL).  The library alternates the
 * frames between two pipelines of its own — staging buffers, streams and workspace each — on every device of the context (the rows of
 * EVERY frame are dealt to all devices, as in rtgr_trace_f64).  Frame k's results are those of the single call, bit for bit.
 * Blocking; returns the first failure with the frame's number in rtgr_last_error().  The _pixels twins take and fill the reference's
 * own Array{Pixel{T},2} per frame, as rtgr_trace_pixels_f64 does. */
int rtgr_trace_frames_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, uint32_t nframes, const rtgr_camera* cams,
                          const double* const* state0s, uint64_t ni, uint64_t nj, double* const* rgb, const rtgr_ray_outputs* outs,
                          rtgr_counters* ctrs);
int rtgr_trace_frames_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, uint32_t nframes, const rtgr_camera* cams,
                          const float* const* state0s, uint64_t ni, uint64_t nj, float* const* rgb, const rtgr_ray_outputs* outs,
                          rtgr_counters* ctrs);
int rtgr_trace_frames_pixels_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, uint32_t nframes,
                                 const double* const* pixels_in, uint64_t ni, uint64_t nj, double* const* pixels_out, rtgr_counters* ctrs);
int rtgr_trace_frames_pixels_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, uint32_t nframes,
                                 const float* const* pixels_in, uint64_t ni, uint64_t nj, float* const* pixels_out, rtgr_counters* ctrs);

/* Legacy single-ray shape `trace_ray(metric, objs, cb, p)::Pixel` (test/runtests.jl:76): one pixel in, rgb out. */
int rtgr_trace_one_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const double pos[4],
                       const double normal[4], double rgb[3], double state_end[8], uint8_t* status);
int rtgr_trace_one_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const float pos[4],
                       const float normal[4], float rgb[3], float state_end[8], uint8_t* status);

/* ---- the hot path over ALL devices of the context, frame assembled in DEVICE memory ---------------------
 * rtgr_trace_sharded_device_*: one blocking call from one host thread: image rows are dealt cyclically to the context's N
 * devices (device k traces rows k, k+N, …), every device runs the pipeline on a stream of its own, and the rows — RGB
 * planes and, when asked for, status / hit / step counts / end states / lambda_end / redshift — are copied peer-to-peer
 * (hipMemcpyPeerAsync on the source device's stream: one xGMI link per peer, no reduction, no halo) to device 0 and put
 * back in place there: d_rgb (3 planes of ni*nj) and the members of `out` are device-0 pointers.  Counters of all devices
 * are summed into `ctr` (host).
 *   Peer access is established by rtgr_create.  Where it could not be (the reason is kept), the rows of that device travel
 * device -> pinned host -> device 0 instead; option "peer" = 0 forces that path for every device (also between two entries
 * of one physical GPU: how it is tested on a one-GPU box), "peer" = 1 makes the call fail with RTGR_ERR_HIP naming the
 * device pair instead of falling back.  A failing hipMemcpyPeerAsync is RTGR_ERR_HIP with the pair in the message.
 * rtgr_trace_sharded_f64 / _f32 (host destination) need no gather: they are rtgr_trace_f64 / _f32 with state0 = NULL over
 * the whole canvas (every device downloads its own rows). */
int rtgr_trace_sharded_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam,
                           uint64_t ni, uint64_t nj, double* rgb, const rtgr_ray_outputs* out, rtgr_counters* ctr);
int rtgr_trace_sharded_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt,
                                  const rtgr_camera* cam, uint64_t ni, uint64_t nj, double* d_rgb,
                                  const rtgr_ray_outputs* out, rtgr_counters* ctr);
int rtgr_trace_sharded_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam,
                           uint64_t ni, uint64_t nj, float* rgb, const rtgr_ray_outputs* out, rtgr_counters* ctr);
int rtgr_trace_sharded_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt,
                                  const rtgr_camera* cam, uint64_t ni, uint64_t nj, float* d_rgb,
                                  const rtgr_ray_outputs* out, rtgr_counters* ctr);

/* ---- adaptive anti-aliasing: supersample only the pixels on an edge ----------------------------------------------------
 * AN EXTENSION: every other entry point delivers one ray through each pixel centre, and the reference's colour rule is discontinuous
 * (a 24-band sawtooth in theta and phi, src/RayTraceGR.jl:427; an integer object index; a hard miss colour): staircase silhouettes,
 * moire towards the photon ring.  These calls trace the plain frame, find the pixels that need more rays and trace only those again:
 *   Pass 1     the plain camera frame of the whole ni x nj canvas into d_rgb, exactly as rtgr_trace_device_* does with `cam`, j0 = 0,
 *              j1 = nj.  `out` describes that pixel-centre ray and is never changed by the refinement.
 *   Edge rule  pixel p is refined if an in-frame 4-neighbour q (i +- 1 or j +- 1) has hit32(q) != hit32(p), or status(q) != status(p), or
 *              max_c |rgb_c(p) - rgb_c(q)| > aa->contrast — the difference and the comparison in the entry point's scalar type,
 *              `contrast` rounded to it; a NaN difference is not an edge.  Symmetric: both pixels of a differing pair are refined.
 *              contrast < 0: EVERY pixel is refined (uniform supersampling); +Inf: class edges (hit / status) only.
 *              d_refined (optional, ni*nj bytes): 1 where the pixel was refined, else 0.
 *   Pass 2     sub-ray (s, t), s, t in [0, k), of a refined pixel (i, j) is the camera ray of pixel (k i + s, k j + t) of the
 *              (k ni) x (k nj) canvas of the same camera, so the k x k block is exactly the block of the k-times finer plain frame.
 *              The sub-rays go through the same trace as caller-supplied ray states, aa->max_batch_rays at a time.
 *   Reduce     per channel, in the scalar type: 0, plus the sub-colours with t outer and s inner, then ONE division by k*k (no fused
 *              operation, no reciprocal); the result overwrites the pixel in d_rgb.  Unrefined pixels keep pass 1's bits.
 * So the frame equals where(refined, box filter of the plain (k ni) x (k nj) frame, plain ni x nj frame) bit for bit, whatever the
 * batch size, and does not depend on the order in which the library lists the refined pixels.
 *   ctr (host, optional) is OVERWRITTEN with the counters of both passes summed; stats (host, optional): the canvas' pixels, the
 *   refined ones, the sub-rays traced (k*k per refined pixel) and the batches they were traced in.
 *   Streams: the call reads the number of refined pixels back, so it SYNCHRONISES `stream` once between the passes (and once more at
 * its end when `ctr` is asked for); everything else is enqueued on `stream`.  It is refused during stream capture (RTGR_ERR_BAD_ARG),
 * like workspace growth.  The device entry runs on the device that owns d_rgb; its scratch — refined count and counters, the hit /
 * status arrays `out` does not ask for, the index list (8 bytes per pixel), the sub-ray states and sub-colours of one batch (11 scalars
 * per sub-ray) — lives with that stream's state, only grows, and is retired, not freed, until rtgr_trim, like the workspace.  Calls on
 * different streams may run concurrently; two such calls on ONE stream from two host threads at once are not supported.
 *   rtgr_trace_aa_f64 / _f32 (host pointers) run the same thing on device 0 of the context and copy out: dealing an anti-aliased
 * frame over several devices is out of scope.
 *   RTGR_ERR_BAD_ARG (with a message): k outside 2..8, flags != 0, a NaN contrast, a null cam, and a scene whose metric is RTGR_USER (its
 * camera kernel lives in the run-time unit; user OBJECTS under a built-in metric are fine: only the camera needs the metric).
 * In scope: the built-in metrics (closed and generic), 3-D and 4-D grids, every object kind, both scalar types.  Out of scope:
 * recursive refinement, filters other than the box, jittered samples. */
typedef struct rtgr_aa {
    uint32_t k;              /* k x k sub-rays per refined pixel, 2..8                                                        */
    uint32_t flags;          /* 0                                                                                             */
    double contrast;         /* refine where max_c |rgb_c(p) - rgb_c(q)| > contrast for a 4-neighbour q;
                                < 0: refine EVERY pixel (uniform supersampling); +Inf: class edges only; NaN: RTGR_ERR_BAD_ARG */
    uint64_t max_batch_rays; /* sub-rays traced per batch at most; 0 = default (2^22); rounded down to whole pixels, at least
                                one pixel                                                                                     */
} rtgr_aa;                   /* 24 bytes: k 0, flags 4, contrast 8, max_batch_rays 16 */
typedef struct rtgr_aa_stats {
    uint64_t pixels;         /* ni * nj                                  */
    uint64_t refined;        /* pixels the edge rule selected            */
    uint64_t sub_rays;       /* k * k * refined                          */
    uint64_t batches;        /* traces of pass 2 (0 when refined == 0)   */
} rtgr_aa_stats;             /* 32 bytes */
int rtgr_trace_aa_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                             uint64_t nj, const rtgr_aa* aa, double* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined,
                             rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
int rtgr_trace_aa_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                             uint64_t nj, const rtgr_aa* aa, float* d_rgb, const rtgr_ray_outputs* out, uint8_t* d_refined,
                             rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
int rtgr_trace_aa_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                      const rtgr_aa* aa, double* rgb, const rtgr_ray_outputs* out, uint8_t* refined, rtgr_counters* ctr,
                      rtgr_aa_stats* stats);
int rtgr_trace_aa_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                      const rtgr_aa* aa, float* rgb, const rtgr_ray_outputs* out, uint8_t* refined, rtgr_counters* ctr,
                      rtgr_aa_stats* stats);

/* ---- image textures for spheres, disks and escaping rays ------------------------------------------------------------------
 * AN EXTENSION: the reference colours by fixed rules (a 24-band sawtooth on spheres, :427; constant green on planes; a hard miss
 * colour, :528); nothing reads a picture.  A TEXTURE is an image the context keeps on its devices; a shaded trace is the plain trace
 * followed by one shading kernel that overwrites the colour of the pixels whose object — or whose escape — has a texture bound.  No
 * kernel of the trace itself changes, and a pixel that is not shaded keeps the plain frame's bits.
 *
 * Textures.  rtgr_texture_load takes `texels`: three planes of height*width doubles, column fastest, texels[(c*height + r)*width + q] —
 * the layout of every `rgb` output of the library, so a traced ni x nj frame is a loadable width = ni, height = nj texture as it stands.
 * RTGR_ERR_BAD_ARG: width or height outside 2 .. 16384, flags or pad non-zero, any non-finite texel (the index of the first one in
 * rtgr_last_error()).  The texels are uploaded to every device of the context as a Float64 and a Float32 copy (the double rounded
 * once; the _f32 entry points read the latter), each texel four scalars (r, g, b, 0) so that a corner is one aligned 32- / 16-byte
 * load.  Texture ids come from a counter of their own and never coincide with grid ids or unit ids.  Lifetime as for grids:
 * rtgr_texture_unload (id 0: every texture of the context) makes the id unknown at once — a later call naming it is RTGR_ERR_BAD_ARG —,
 * the device memory is RETIRED and freed only by rtgr_trim / rtgr_destroy, so a hipGraph captured earlier may still replay it.
 *
 * The mapping and the sampler (one device function, csrc/rtgr_texture.hpp, in the entry point's scalar type; W = width, H = height).
 *   From a 3-vector d (direction mapping):
 *     theta = atan2(hypot(d_x, d_y), d_z)   (not acos: it is ill-conditioned at the poles),   phi = atan2(d_y, d_x),
 *     s = (phi + pi) W / (2 pi) - 1/2,   v = theta H / pi - 1/2.
 *     Column q has its centre at phi = -pi + (q + 1/2) 2 pi / W, row r at theta = (r + 1/2) pi / H.  These are the theta, phi of the
 *     reference's objcolor(::Sphere) (:420-427).  A zero or non-finite d means "no sample": the pixel keeps its colour.
 *   Disk mapping, from a position x with r_in and r_out of the disk: phi and s as above from (x, y);
 *     v = (hypot(x, y) - r_in) / (r_out - r_in) H - 1/2   (a non-finite x, y or v: no sample).
 *   RTGR_TEX_NEAREST:  column floor(s + 1/2) mod W, row clamp(floor(v + 1/2), 0, H - 1); the result is the texel's stored value, bit
 *     for bit.
 *   RTGR_TEX_BILINEAR: q0 = floor(s), f_x = s - q0, columns q0 mod W and (q0 + 1) mod W (the seam at phi = +-pi wraps); r0 = floor(v),
 *     f_y = v - r0, rows clamp(r0, 0, H - 1) and clamp(r0 + 1, 0, H - 1) (clamped at the poles and rims, not reflected); per channel
 *     a = t00 + f_x (t10 - t00), b = t01 + f_x (t11 - t01), result = a + f_y (b - a), no fused operation.  The form is written relative
 *     to a corner, like the grid interpolant relative to its centre sample: a constant texture comes back to the bit.
 *
 * Shading, per pixel of the traced frame (rtgr_shade: nbind binds, at most RTGR_MAX_TEXTURE_BINDS; bind.object is the 1-based index
 * in the caller's object list, 0 = rays that escape):
 *   A hit on a bound object (hit32 == bind.object): the position is state_end[0..3]; for a Sphere of either radius sign d = x_end -
 *     centre in the spatial components (so the inverted sky sphere `caelum` is covered); for a Disk the disk mapping.
 *   A bound escape (bind.object == 0): hit32 == 0, status RTGR_RAY_LAMBDA1 or RTGR_RAY_OUTSIDE and the Euclidean |x_end| >= r_escape;
 *     d is the spatial part of the end VELOCITY state_end[5..7] — the ray is traced backwards from the camera, so this is where on the
 *     sky the light came from.  It is the coordinate direction, with no asymptotic correction.
 *   Colour: the texel as sampled; the reference's omin / length(objs) dimming is not applied.
 *   Every other pixel — unbound objects, planes, user objects, misses that did not escape, "no sample" — is not written.  A caller who
 *     wants a black hole sets miss_rgb to black.
 *
 * rtgr_trace_shaded_device_*.  aa == NULL: a camera frame of the whole ni x nj canvas (as rtgr_trace_device_* with `cam`, j0 = 0,
 * j1 = nj), then the shading kernel.  state_end, hit32 and status go to the caller's arrays where `out` asks for them, otherwise to a
 * grow-only scratch of the stream, retired like the workspace; `out` describes the plain ray and is never changed by shading;
 * d_refined and stats must be NULL.  The call only enqueues — unless `ctr` (host) is given: then it synchronises `stream` once at its
 * end to copy the counters out.  With ctr == NULL it may be captured once the workspace and the scratch are large enough (a call of
 * the same size before the capture makes them so); growth during capture is RTGR_ERR_BAD_ARG, like workspace growth.
 *   aa != NULL: adaptive anti-aliasing (above) of the SHADED frame: pass 1 is the shaded plain frame, the edge rule reads the shaded
 * colours, the sub-rays of pass 2 are traced with their end states and shaded before the reduction (8 + 11 scalars + 5 bytes of batch
 * scratch per sub-ray).  So uniform == the box filter of the shaded (k ni) x (k nj) frame, adaptive == where(refined, uniform, shaded
 * plain), bit for bit.  The rules of rtgr_trace_aa_device_* for ctr, stats, d_refined, streams and capture apply.
 *   rtgr_trace_shaded_f64 / _f32 (host pointers) run the same on device 0 of the context and copy out, as rtgr_trace_aa_* do.
 *   RTGR_ERR_BAD_ARG (with a message): a null shade or cam, flags != 0, nbind > RTGR_MAX_TEXTURE_BINDS, an unknown texture id or
 * filter, object > nobj, an object (or the escape) bound twice, a bind to a Plane or a user object, a NaN or negative r_escape, and
 * the anti-aliasing refusals.  nbind == 0 is legal: the frame is the plain frame, bit for bit.
 *   In scope: every metric (RTGR_USER when aa == NULL, both grid kinds), object lists of any length, both scalar types.
 *   Out of scope: the sharded, frames-in-flight, pixel-array and single-ray entry points; mip-mapping or any minification filter
 * (anti-aliasing is the answer to minification); pole-aware bilinear; planes and user objects; emission or redshift weighting of the
 * TEXEL (a disk that glows by itself is "disk emission" below; a textured disk is coloured as sampled); several devices for one
 * shaded frame.
 *
 * rtgr_eval_texture_*: the sampler at n points on device 0 (host pointers) — p: n x 3 (d, or a position whose x, y are read when
 * disk_range = {r_in, r_out} is given; NULL: the direction mapping); rgb: n x 3 (AoS), read and written: a "no sample" point keeps
 * what the caller put there. */
enum rtgr_tex_filter { RTGR_TEX_NEAREST = 0, RTGR_TEX_BILINEAR = 1 };
#define RTGR_MAX_TEXTURE_BINDS 16
#define RTGR_TEXTURE_MAX_SIDE 16384
typedef struct rtgr_texture_desc {
    uint32_t width, height; /* 2 .. RTGR_TEXTURE_MAX_SIDE */
    uint32_t flags;         /* 0 */
    uint32_t pad;           /* 0 */
} rtgr_texture_desc;        /* 16 bytes: width 0, height 4, flags 8, pad 12 */
typedef struct rtgr_texture_bind {
    uint32_t object;        /* 1-based index in the caller's object list; 0 = rays that escape */
    uint32_t filter;        /* rtgr_tex_filter */
    uint64_t texture;       /* id from rtgr_texture_load */
} rtgr_texture_bind;        /* 16 bytes: object 0, filter 4, texture 8 */
typedef struct rtgr_shade {
    uint32_t nbind;         /* 0 .. RTGR_MAX_TEXTURE_BINDS */
    uint32_t flags;         /* 0 */
    const rtgr_texture_bind* bind; /* nbind binds (host memory; may be NULL when nbind == 0) */
    double r_escape;        /* a miss counts as escaped when the Euclidean |x_end| >= r_escape; >= 0 */
} rtgr_shade;               /* 24 bytes: nbind 0, flags 4, bind 8, r_escape 16 */
int rtgr_texture_load(rtgr_context* ctx, const rtgr_texture_desc* desc, const double* texels, uint64_t* id_out);
int rtgr_texture_unload(rtgr_context* ctx, uint64_t id); /* id 0: all */
int rtgr_trace_shaded_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                                 uint64_t nj, const rtgr_shade* shade, const rtgr_aa* aa, double* d_rgb, const rtgr_ray_outputs* out,
                                 uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
int rtgr_trace_shaded_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                                 uint64_t nj, const rtgr_shade* shade, const rtgr_aa* aa, float* d_rgb, const rtgr_ray_outputs* out,
                                 uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
int rtgr_trace_shaded_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                          uint64_t nj, const rtgr_shade* shade, const rtgr_aa* aa, double* rgb, const rtgr_ray_outputs* out,
                          uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats);
int rtgr_trace_shaded_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                          uint64_t nj, const rtgr_shade* shade, const rtgr_aa* aa, float* rgb, const rtgr_ray_outputs* out,
                          uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats);
int rtgr_eval_texture_f64(rtgr_context* ctx, uint64_t texture, uint32_t filter, const double* p /* n x 3 */, uint64_t n,
                          const double* disk_range /* NULL, or {r_in, r_out} */, double* rgb /* n x 3 */);
int rtgr_eval_texture_f32(rtgr_context* ctx, uint64_t texture, uint32_t filter, const float* p /* n x 3 */, uint64_t n,
                          const float* disk_range /* NULL, or {r_in, r_out} */, float* rgb /* n x 3 */);

/* ---- disk emission: an orbiting disk that glows as a black body -------------------------------------------------------------
 * AN EXTENSION: the reference colours a hit by fixed rules, and rtgr_ray_outputs.redshift takes a disk's emitter to be the observer at
 * rest in the slicing.  A disk ORBITS: an emitted trace is the plain trace (then the textures of `shade`, if any) followed by one
 * emission kernel over the pixels with hit32 == emit->object, which replaces their colour by the black-body colour of gas on circular
 * orbits, shifted by the Doppler and gravitational frequency ratio g.  No kernel of the trace itself changes; every other pixel keeps
 * its bits; rtgr_ray_outputs.redshift keeps its documented (static) emitter.
 *
 * The model (one device function, csrc/rtgr_emission.hpp, in the entry point's scalar type; x_0, k_0: the ray's state at the camera,
 * x_end, k_end: its state where it ended on the disk).
 *   The orbital rate comes from the metric, not from a closed form.  The metric must be stationary, axisymmetric about z and symmetric
 *   under z -> -z.  With psi = (0, -y, x, 0) the orbit of xi = d_t + Omega psi is a geodesic iff the gradient of g(xi, xi) vanishes at
 *   fixed Omega.  At the equatorial projection P = (t, x_end, y_end, 0), with D = x d_x + y d_y acting on the metric's components:
 *     g_tpsi = -y g_tx + x g_ty,   g_psipsi = y^2 g_xx - 2 x y g_xy + x^2 g_yy,
 *     A = D g_tt,   B = (-y D g_tx + x D g_ty) + g_tpsi,   C = (y^2 D g_xx - 2 x y D g_xy + x^2 D g_yy) + 2 g_psipsi,
 *     C Omega^2 + 2 B Omega + A = 0:   Omega_+- = (-B +- sqrt(B^2 - A C)) / C.
 *   g and dg at P are those of rtgr_eval_metric_* (forward duals through a built-in metric; the interpolant of a 3-D grid).  For the
 *   textbook Kerr metric Omega_+- are sqrt(M) / (r^(3/2) + a sqrt(M)) and -sqrt(M) / (r^(3/2) - a sqrt(M)); for the reference's own
 *   metric (RTGR_KS_REF, whose radius is not Kerr's) and for grids the closed form would be wrong and this is not.
 *   RTGR_EMIT_KEPLER: Omega = the root `orbit` names (+1: Omega_+, counter-clockwise seen from +z for a > 0; -1: Omega_-).
 *   RTGR_EMIT_RIGID:  Omega = orbit itself (0: xi = d_t, the static emitter).
 *   Emitter: xi = (1, -Omega y_end, Omega x_end, 0) at x_end (the disk has a half thickness, z_end != 0: it rotates on cylinders at the
 *   equatorial rate), n^2 = g(x_end)(xi, xi), u_emit = xi / sqrt(-n^2).  VALID iff B^2 - A C >= 0, C != 0, every quantity finite and
 *   n^2 < 0 (and the camera's static observer is timelike).
 *   g = (k_0 . u_obs) / (k_end . u_emit), u_obs the static observer at the pixel exactly as for rtgr_ray_outputs.redshift; every
 *   inner product with the metric at the point where its vectors live.
 *   Colour: a black body's I_nu / nu^3 is invariant, so the observed spectrum is Planck's at g T_em:
 *     rho = hypot(x_end, y_end),   T_em = T_in (rho / r_in)^(-p)   [RTGR_EMIT_INNER_EDGE: times (max(1 - sqrt(r_in / rho), 0))^(1/4),
 *     evaluated as two square roots],   rgb_c = gain weight_c / expm1(theta_c / (g T_em)),   theta_c = h c / (lambda_c k_B).
 *   An invalid emitter, g <= 0 or T_em <= 0 gives BLACK (0, 0, 0) and g = NaN: a disk region with no circular orbit emits nothing.
 *   r_in is the Disk's own (rtgr_object.p[1]).  No operation of the function is fused, so the hook below predicts a pixel to the bit.
 *
 * rtgr_trace_emission_device_*.  Order of work: the plain frame (as rtgr_trace_shaded_device_*: the whole ni x nj canvas of `cam`), the
 * textures of `shade` (may be NULL), the emission kernel.  d_g (n scalars, may be NULL) receives g on the disk's pixels and NaN on every
 * other.  `out`, ctr, d_refined, stats, the scratch (grow-only, with the stream's state, retired until rtgr_trim) and the capture rules
 * are those of rtgr_trace_shaded_device_*: the call may be captured when aa == NULL and ctr == NULL, once workspace and scratch are
 * large enough.  With `aa`: pass 1 is shaded and emitted before the edge rule reads it, the sub-rays of pass 2 are emitted from their
 * own sub-ray states before the reduction, and d_g is pass 1's (the pixel-centre rays').  So uniform == the box filter of the emitted
 * (k ni) x (k nj) frame and adaptive == where(refined, uniform, emitted plain), bit for bit.
 *   rtgr_trace_emission_f64 / _f32 (host pointers) run the same on device 0 of the context and copy out.
 *   RTGR_ERR_BAD_ARG (with a message): a null emit or cam; object 0, > nobj or not a Disk; a disk that `shade` also binds; an unknown
 * emitter or flags, pad != 0; KEPLER with orbit other than +1 / -1; a non-finite orbit; T_in, gain or a theta_c that is <= 0 or NaN; a
 * weight_c < 0 (or NaN); a non-finite p; a scene whose metric is RTGR_USER (its kernels live in the unit) or a 4-D grid (not
 * stationary); the refusals of rtgr_trace_shaded_* and of anti-aliasing.
 *   In scope: the built-in metrics (closed and generic flags alike), 3-D grids, object lists of any length, both scalar types.
 *   Out of scope: emission inside the innermost stable orbit (plunging gas), more than one emitting disk per call, limb darkening, a
 * colour-matching-function integral, RTGR_USER metrics and 4-D grids, the sharded, frames-in-flight, pixel-array and single-ray entry
 * points.
 *
 * rtgr_eval_disk_emission_*: the same device function at n pairs of states on device 0 (host pointers) — s0, s_end: n x 8; omega: n;
 * u_emit: n x 4; g: n; rgb: n x 3 (AoS).  Any output may be NULL.  An invalid point gives NaN, NaN, NaN and black. */
enum rtgr_emitter { RTGR_EMIT_KEPLER = 0, RTGR_EMIT_RIGID = 1 };
#define RTGR_EMIT_INNER_EDGE 1u
typedef struct rtgr_disk_emission {
    uint32_t object;   /* 1-based index of a Disk in the caller's list */
    uint32_t emitter;  /* rtgr_emitter */
    uint32_t flags;    /* 0 | RTGR_EMIT_INNER_EDGE */
    uint32_t pad;      /* 0 */
    double orbit;      /* KEPLER: +1 = the root Omega_+ (counter-clockwise from +z), -1 = Omega_-; RIGID: Omega itself (0: xi = d_t) */
    double T_in, p, gain;
    double theta[3], weight[3];
} rtgr_disk_emission;  /* 96 bytes: object 0, emitter 4, flags 8, pad 12, orbit 16, T_in 24, p 32, gain 40, theta 48, weight 72 */
int rtgr_trace_emission_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                   const rtgr_aa* aa /* may be NULL */, double* d_rgb, const rtgr_ray_outputs* out,
                                   double* d_g /* n, may be NULL */, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
int rtgr_trace_emission_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                   const rtgr_aa* aa /* may be NULL */, float* d_rgb, const rtgr_ray_outputs* out,
                                   float* d_g /* n, may be NULL */, uint8_t* d_refined, rtgr_counters* ctr, rtgr_aa_stats* stats, void* stream);
int rtgr_trace_emission_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                            const rtgr_aa* aa /* may be NULL */, double* rgb, const rtgr_ray_outputs* out, double* g /* n, may be NULL */,
                            uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats);
int rtgr_trace_emission_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                            const rtgr_aa* aa /* may be NULL */, float* rgb, const rtgr_ray_outputs* out, float* g /* n, may be NULL */,
                            uint8_t* refined, rtgr_counters* ctr, rtgr_aa_stats* stats);
int rtgr_eval_disk_emission_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const double* s0 /* n x 8 */,
                                const double* s_end /* n x 8 */, uint64_t n, double* omega /* n */, double* u_emit /* n x 4 */,
                                double* g /* n */, double* rgb /* n x 3 */);
int rtgr_eval_disk_emission_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const float* s0 /* n x 8 */,
                                const float* s_end /* n x 8 */, uint64_t n, float* omega /* n */, float* u_emit /* n x 4 */,
                                float* g /* n */, float* rgb /* n x 3 */);

/* ---- observer camera: a pinhole carried by a static, moving or orbiting observer ---------------------------------------------
 * AN EXTENSION: the reference's make_canvas spreads its ray origins over a plane and gives every pixel a static observer of its own.
 * An rtgr_observer is a camera one can aim: ONE event, an observer with a 4-velocity, an orthonormal frame (tetrad) built from "look"
 * and "up", a field of view.  An observer trace builds the frame (one small kernel), writes the rays' start states (one kernel, 8
 * scalars per ray) and hands them to the untouched trace as caller-supplied states, a batch of whole rows at a time; no kernel of the
 * trace itself changes, and a ray is, bit for bit, the ray rtgr_trace_* traces from the state rtgr_make_observer_canvas_* delivers.
 *
 * The frame (csrc/rtgr_observer.hpp, in the entry point's scalar type; every inner product with g = the metric at pos).
 *   kind   RTGR_OBS_STATIC    u = -g^{-1} e_t, normalised, future-directed: exactly the observer of make_canvas and of
 *                             rtgr_ray_outputs.redshift.
 *          RTGR_OBS_VELOCITY  u = vel, the caller's coordinate 4-velocity, normalised with g (as rtgr_object's `vel` of a Sphere is).
 *          RTGR_OBS_CIRCULAR  u along xi = d_t + Omega psi, psi = (0, -y, x, 0), Omega the root `orbit` (+1 / -1) of the quadratic of
 *                             "disk emission" above at pos — the same device function, the same bits; pos must lie in the plane z = 0.
 *   e_0     = u / sqrt(-g(u, u))
 *   e_look  = normalise(look + g(look, e_0) e_0)
 *   e_up    = normalise(up + g(up, e_0) e_0 - g(up, e_look) e_look)
 *   e_right = the unit vector orthogonal to the three, oriented "right = look x up in flat space at rest": lowered,
 *             (e_right)_a = -sqrt(-det g) eps_{abcd} e_0^b e_look^c e_up^d with eps_0123 = +1; raised with g^{-1}.  (Minkowski, u = d_t,
 *             look = +y, up = +z: e_right = +x — example2's widthx / normal / widthy.)
 *   look and up are coordinate vectors; only their parts orthogonal to u (and, for up, to the look axis) matter.
 *   INVALID (no error: the frame is built on the device) iff u is not timelike or not future-directed (u^t <= 0); for CIRCULAR the
 *   quadratic has no real root, C = 0 or g(xi, xi) >= 0; det g >= 0; look or up is degenerate after projection (squared norm of the
 *   projected vector <= 4096 eps times sum |v^a g_ab v^b| of the given one); anything is not finite.
 * The pixel (i, j), 0-based, i along e_right, j along e_up, output index i + j ni:  a = 2 (i + 1/2) / ni - 1,  b = 2 (j + 1/2) / nj - 1.
 *   RTGR_PROJ_PERSPECTIVE  n = normalise(e_look + a tan(fov_x / 2) e_right + b tan(fov_y / 2) e_up); fov_x, fov_y in (0, pi), radians.
 *   RTGR_PROJ_EQUIRECT     alpha = a fov_x / 2, beta = b fov_y / 2, n = cos beta (cos alpha e_look + sin alpha e_right) + sin beta e_up;
 *                          0 < fov_x <= 2 pi, 0 < fov_y <= pi (the full sky: 2 pi x pi).
 *   state: x = pos, k = (-e_0 + n) / sqrt(2): null, past-directed, make_canvas' normalisation (g(k, e_0) = +1 / sqrt(2)).
 *   No operation of the frame's and the pixel's own arithmetic is fused; tan(fov / 2) is taken on the host in double.
 *   An INVALID frame writes NaN into every state: the trace ends those rays as RTGR_RAY_NAN (not_finished = n) and returns RTGR_OK.
 *   rtgr_eval_observer_* says up front whether a frame is valid.
 *
 * rtgr_trace_observer_device_*.  Order of work: the frame kernel; then, for batches of whole rows of at most max_batch_rays rays (at
 * least one row): the ray kernel into the stream's scratch, the plain trace of those states into the caller's planes, the textures of
 * `shade` (may be NULL), the emission kernel of `emit` (may be NULL).  d_g (n scalars, may be NULL; needs emit) receives the frequency
 * ratio on the disk's pixels and NaN elsewhere.  With `emit`, u_obs in g = (k_0 . u_obs) / (k_end . u_emit) is THIS observer's e_0 —
 * not the static observer — so an orbiting camera sees its own Doppler shift and beaming.  Textures need the end states only.
 *   The call only enqueues, apart from one synchronisation at the end when `ctr` is given; it may be captured with ctr == NULL once
 * workspace and scratch (grow-only, with the stream's state, retired until rtgr_trim) are large enough — make one call of the same size
 * on the stream first.  The result does not depend on max_batch_rays or on the stream.  (Under the experiment option tile = 1, whose
 * kernel writes whole frames only, a frame of more than one batch is refused, as adaptive anti-aliasing's windows are.)
 *   rtgr_trace_observer_f64 / _f32 (host pointers) run the same on device 0 of the context and copy out.
 * rtgr_make_observer_canvas_device_* / rtgr_make_observer_canvas_*: the states of rows [j0, j1) (ni (j1 - j0) x 8), as rtgr_make_canvas_*.
 * rtgr_eval_observer_* (blocking, host pointers): frame = 4 x 4, rows e_0, e_right, e_up, e_look; omega (NaN unless CIRCULAR); valid.
 * Any output may be NULL.  rtgr_eval_disk_emission_observer_*: rtgr_eval_disk_emission_* with u_obs = the e_0 of `obs` (obs == NULL: the
 * static observer, the same call as rtgr_eval_disk_emission_*).
 *   RTGR_ERR_BAD_ARG (with a message): a null obs; an unknown kind or projection; flags or pad != 0; a non-finite pos, look, up, fov,
 * orbit (CIRCULAR) or vel (VELOCITY); a fov outside its range; CIRCULAR with orbit other than +1 / -1 or with pos[3] != 0; a scene
 * whose metric is RTGR_USER or a 4-D grid; out->redshift (its definition names the static observer: use d_g); ni or nj = 0 (or more
 * than 2^34 pixels); d_g without emit; more than one batch under option tile = 1; the refusals of rtgr_trace_shaded_* and rtgr_trace_emission_*.
 *   In scope: the built-in metrics (closed and generic), 3-D grids, object lists of any length, both scalar types, textures, emission.
 *   Out of scope: anti-aliasing with this camera; the sharded, frames-in-flight, pixel-array and single-ray entry points; RTGR_USER
 * metrics and 4-D grids; the redshift output; lenses other than the two projections; a camera path over time. */
enum rtgr_observer_kind { RTGR_OBS_STATIC = 0, RTGR_OBS_VELOCITY = 1, RTGR_OBS_CIRCULAR = 2 };
enum rtgr_projection { RTGR_PROJ_PERSPECTIVE = 0, RTGR_PROJ_EQUIRECT = 1 };
typedef struct rtgr_observer {
    double pos[4];            /* the event the observer is at */
    double vel[4];            /* VELOCITY: coordinate 4-velocity (any normalisation); ignored otherwise */
    double look[4], up[4];    /* coordinate vectors */
    double fov_x, fov_y;      /* radians */
    double orbit;             /* CIRCULAR: +1 = the root Omega_+, -1 = Omega_-; ignored otherwise */
    uint32_t kind;            /* rtgr_observer_kind */
    uint32_t projection;      /* rtgr_projection */
    uint32_t flags;           /* 0 */
    uint32_t pad;             /* 0 */
    uint64_t max_batch_rays;  /* rays traced per batch at most; 0 = default (2^22); rounded down to whole rows, at least one */
} rtgr_observer;  /* 176 bytes: pos 0, vel 32, look 64, up 96, fov_x 128, fov_y 136, orbit 144, kind 152, projection 156, flags 160,
                     pad 164, max_batch_rays 168 */
int rtgr_trace_observer_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                                   double* d_rgb, const rtgr_ray_outputs* out, double* d_g /* n, may be NULL */, rtgr_counters* ctr,
                                   void* stream);
int rtgr_trace_observer_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                                   float* d_rgb, const rtgr_ray_outputs* out, float* d_g /* n, may be NULL */, rtgr_counters* ctr,
                                   void* stream);
int rtgr_trace_observer_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                            double* rgb, const rtgr_ray_outputs* out, double* g /* n, may be NULL */, rtgr_counters* ctr);
int rtgr_trace_observer_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                            float* rgb, const rtgr_ray_outputs* out, float* g /* n, may be NULL */, rtgr_counters* ctr);
int rtgr_make_observer_canvas_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                                         uint64_t j0, uint64_t j1, double* d_state0, void* stream);
int rtgr_make_observer_canvas_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj,
                                         uint64_t j0, uint64_t j1, float* d_state0, void* stream);
int rtgr_make_observer_canvas_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, uint64_t j0,
                                  uint64_t j1, double* state0);
int rtgr_make_observer_canvas_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, uint64_t ni, uint64_t nj, uint64_t j0,
                                  uint64_t j1, float* state0);
int rtgr_eval_observer_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, double* frame /* 4 x 4 */, double* omega,
                           int* valid);
int rtgr_eval_observer_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_observer* obs, float* frame /* 4 x 4 */, float* omega,
                           int* valid);
int rtgr_eval_disk_emission_observer_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit,
                                         const rtgr_observer* obs /* may be NULL */, const double* s0 /* n x 8 */,
                                         const double* s_end /* n x 8 */, uint64_t n, double* omega /* n */, double* u_emit /* n x 4 */,
                                         double* g /* n */, double* rgb /* n x 3 */);
int rtgr_eval_disk_emission_observer_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit,
                                         const rtgr_observer* obs /* may be NULL */, const float* s0 /* n x 8 */,
                                         const float* s_end /* n x 8 */, uint64_t n, float* omega /* n */, float* u_emit /* n x 4 */,
                                         float* g /* n */, float* rgb /* n x 3 */);

/* ---- hot-spot light curves: one traced frame reduced over many observer times ---------------------------------------------------
 * AN EXTENSION.  The emitting scenes are stationary: shifting the camera by tau in coordinate time shifts every ray by tau and changes
 * nothing else, and a ray's end state carries the coordinate time at which it met the disk (state_end[8 p + 0], relative to the camera's
 * event; rays are past-directed).  So ONE traced frame determines what the observer sees of a time-dependent emitter at EVERY observer
 * time.  The emitter with a clock is an rtgr_hot_spot: a compact bright region that rides in the emitting disk of an rtgr_disk_emission.
 *
 * The model (csrc/rtgr_lightcurve.hpp restates it; the reduction runs in double for both entry types, Float32 planes promoted on read).
 *   Rate.   Omega_s = the orbital rate of the disk's own emitter model at the equatorial point (0, rho_s, 0, 0): RTGR_EMIT_KEPLER the root
 *           emit->orbit names, RTGR_EMIT_RIGID emit->orbit itself — the emission kernel itself, in point mode, on one synthetic pair of
 *           states: the bits of rtgr_eval_disk_emission_*'s `omega` at an end state with (x, y, z) = (rho_s, 0, 0), in the entry's scalar
 *           type, then promoted.
 *   Clock.  The centre at coordinate time t is c(t) = rho_s (cos(phi0 + Omega_s t), sin(phi0 + Omega_s t)); the spot is rigid (no shear).
 *           Observer sample k is the camera shifted by tau_k = t_start + k dt: pixel p then sees the disk at t_end,p + tau_k.
 *   Emissivity at pixel p's end point (x_p, y_p), sample k:  d^2 = (x_p - c_x)^2 + (y_p - c_y)^2,
 *           j = amp max(exp(-d^2 / (2 sigma^2)) - exp(-cut^2 / 2), 0)    (continuous at the cut).
 *           THE CONTRACT is the expanded form: with theta_p = phi0 + Omega_s t_end,p, beta_k = Omega_s tau_k,
 *             P0 = (x_p^2 + y_p^2) + rho_s^2,  P1 = -2 rho_s (x_p cos theta_p + y_p sin theta_p),  P2 = -2 rho_s (y_p cos theta_p - x_p sin theta_p),
 *             d^2 = P0 + (P1 cos beta_k + P2 sin beta_k)   [= rho_p^2 + rho_s^2 - 2 rho_p rho_s cos(gamma_p - beta_k), gamma_p = psi_p - theta_p]
 *           (its cancellation error is eps rho^2, i.e. eps rho^2 / sigma^2 relative in j), and j = 0 where d^2 >= cut^2 sigma^2.
 *   Gas.    The gas that emits is the disk's: the pixel's frequency ratio is the g the emission kernel wrote for it (d_g).
 *   Weight. With the pixel's a = 2 (i + 1/2) / ni - 1, b = 2 (j + 1/2) / nj - 1 (p = i + j ni), t_x = tan(fov_x / 2), t_y = tan(fov_y / 2):
 *           obs == NULL: w_p = 1;  RTGR_PROJ_PERSPECTIVE: w_p = t_x t_y (2 / ni)(2 / nj) / (1 + a^2 t_x^2 + b^2 t_y^2)^(3/2)  (the solid angle);
 *           RTGR_PROJ_EQUIRECT: w_p = cos(b fov_y / 2) (fov_x / ni)(fov_y / nj).
 *   Output. lc: nt x 3 doubles (F_k, A_k, B_k), whatever the scalar type of the planes:
 *             F_k = sum_p w_p g_p^q j_pk      A_k = sum_p w_p g_p^q j_pk a_p      B_k = sum_p w_p g_p^q j_pk b_p        (q = g_power)
 *           over the pixels with hit32 == emit->object, g_p finite and > 0 and a finite end point; the image centroid is (A_k / F_k,
 *           B_k / F_k).  The sums run in pixel order within fixed ranges of pixels and in range order across them, with no floating-point
 *           atomics: bit-identical from run to run, from stream to stream and — for the traced entries — from one max_batch_rays to another.
 *   Invalid spot: no circular orbit at rho_s (or a spacelike one), or Omega_s not finite: every entry of lc is NaN and the call still
 *           returns RTGR_OK (it only enqueues, as an invalid observer frame does).  rtgr_eval_hot_spot_* says so up front.
 *
 * rtgr_light_curve_device_*: the reduction alone over planes already on the device — d_hit32 (n), d_state_end (n x 8), d_g (n), from
 * rtgr_trace_emission_device_* with the plane camera (obs = NULL), rtgr_trace_observer_device_* or the caller.  It only enqueues; its
 * scratch (grow-only, with the stream's state, retired until rtgr_trim) is at most 24 bytes x min(nt, 1024) x min(ceil(n / 256), 1024)
 * + 4 KB, so the call may be captured once one call of the same nt and n was made on the stream.
 * rtgr_trace_light_curve_device_* / rtgr_trace_light_curve_* (host pointers): the arguments of rtgr_trace_observer_* with `emit` required,
 * plus `spot` and `lc`.  Order of work: the observer trace with emission exactly as rtgr_trace_observer_* does it — d_rgb, d_g, every
 * per-ray output and the counters are its bits; state_end, hit32 and g go into the caller's planes where given, else into the stream's
 * scratch — then ONE light-curve stage over the whole frame after the last batch.  The picture is the tau-independent disk: the spot
 * does not change it.
 * rtgr_eval_hot_spot_* (blocking, host pointers): omega_s, valid, and j at n triples (x, y, t) (xyt: n x 3; j: n doubles; tau = 0: the
 * spot as it stands at coordinate time t) from the same device functions as the reduction.  Any output may be NULL.
 *   RTGR_ERR_BAD_ARG (with a message; lc is left untouched): a null emit, spot, lc or plane; nt = 0 or > 2^20; sigma or cut <= 0 or NaN;
 * amp < 0 or NaN; a non-finite rho_s, phi0, g_power, t_start or dt; rho_s outside the Disk's [r_in, r_out]; flags or pad != 0; and
 * everything rtgr_trace_emission_* and rtgr_trace_observer_* refuse (RTGR_USER metrics, 4-D grids, ...).
 *   Out of scope: a spot that shears, or more than one spot per call; a frame that shows the spot; spectra of the spot; non-stationary
 * scenes; the sharded, frames-in-flight, pixel-array and single-ray entry points; anti-aliasing. */
#define RTGR_HOT_SPOT_MAX_SAMPLES (1ull << 20)
typedef struct rtgr_hot_spot {
    double rho_s;      /* cylindrical radius of the spot's centre, in the plane z = 0 */
    double phi0;       /* azimuth of the centre at coordinate time t = 0 */
    double sigma;      /* Gaussian width, coordinate length in the plane z = 0, > 0 */
    double cut;        /* support in units of sigma, > 0 (4 is typical) */
    double amp;        /* emissivity at the centre, >= 0 */
    double g_power;    /* q in the weight g^q: 4 bolometric, 3 specific intensity of a flat spectrum; finite */
    double t_start;    /* observer time samples tau_k = t_start + k dt, k = 0 .. nt-1 */
    double dt;         /* may be 0 or negative; finite */
    uint64_t nt;       /* 1 .. RTGR_HOT_SPOT_MAX_SAMPLES */
    uint32_t flags;    /* 0 */
    uint32_t pad;      /* 0 */
} rtgr_hot_spot;       /* 80 bytes: rho_s 0, phi0 8, sigma 16, cut 24, amp 32, g_power 40, t_start 48, dt 56, nt 64, flags 72, pad 76 */
int rtgr_light_curve_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                                const rtgr_observer* obs /* may be NULL */, uint64_t ni, uint64_t nj, const uint32_t* d_hit32 /* n */,
                                const double* d_state_end /* n x 8 */, const double* d_g /* n */, double* d_lc /* nt x 3 */, void* stream);
int rtgr_light_curve_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                                const rtgr_observer* obs /* may be NULL */, uint64_t ni, uint64_t nj, const uint32_t* d_hit32 /* n */,
                                const float* d_state_end /* n x 8 */, const float* d_g /* n */, double* d_lc /* nt x 3 */, void* stream);
int rtgr_trace_light_curve_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                      uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                      const rtgr_hot_spot* spot, double* d_rgb, const rtgr_ray_outputs* out, double* d_g /* n, may be NULL */,
                                      double* d_lc /* nt x 3 */, rtgr_counters* ctr, void* stream);
int rtgr_trace_light_curve_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                      uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                      const rtgr_hot_spot* spot, float* d_rgb, const rtgr_ray_outputs* out, float* d_g /* n, may be NULL */,
                                      double* d_lc /* nt x 3 */, rtgr_counters* ctr, void* stream);
int rtgr_trace_light_curve_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                               uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                               double* rgb, const rtgr_ray_outputs* out, double* g /* n, may be NULL */, double* lc /* nt x 3 */,
                               rtgr_counters* ctr);
int rtgr_trace_light_curve_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                               uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                               float* rgb, const rtgr_ray_outputs* out, float* g /* n, may be NULL */, double* lc /* nt x 3 */,
                               rtgr_counters* ctr);
int rtgr_eval_hot_spot_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                           const double* xyt /* n x 3 */, uint64_t n, double* omega_s, int* valid, double* j /* n */);
int rtgr_eval_hot_spot_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_hot_spot* spot,
                           const float* xyt /* n x 3 */, uint64_t n, float* omega_s, int* valid, double* j /* n */);

/* ---- disk spectra: line profiles and thermal spectra from one traced frame --------------------------------------------------------
 * AN EXTENSION.  The traced frame of an emitting disk — hit32, state_end and the frequency ratio g the emission kernel wrote — holds
 * everything a SPECTRUM of the disk needs: the broadened, skewed profile of a narrow emission line is the flux-weighted histogram of g
 * over the disk's image, and the spectrum of the multi-colour black-body disk is the picture's own Planck law summed over the image at
 * many frequencies instead of three.  One small deterministic stage over the disk's pixels, as the light curve's.
 *
 * The model (csrc/rtgr_spectrum.hpp restates it).  Everything runs in double; Float32 planes are promoted on read.
 *   Pixel set.  A pixel p takes part iff hit32[p] == emit->object, g_p is finite and > 0, (x_p, y_p) from state_end is finite, and the
 *           mode's own condition below holds.  rho_p = sqrt(x_p^2 + y_p^2).
 *   Pixel terms.  w_p, a_p, b_p are the light curve's (its "Weight" above: the same device function); obs == NULL: w_p = 1.
 *   RTGR_SPEC_LINE.  The axis is the frequency ratio g itself — a line of rest energy 1 — with nb bins over [lo, hi); 0 <= lo < hi.
 *           s = (double)nb / (hi - lo), computed once on the host;  u = (g_p - lo) * s  (a subtraction, then a multiply: nothing to fuse).
 *           The pixel counts iff 0 <= u < nb and rho_min <= rho_p < rho_max; its bin is b = (uint64)u.
 *           W_p = amp w_p (rho_p / rho_min)^(-alpha) g_p^g_power   (a power-law emissivity; g_power 3: the specific intensity of a line,
 *           4: its flux per unit g).  Output nb x 3 doubles: F_b = sum W_p, A_b = sum W_p a_p, B_b = sum W_p b_p over the pixels of
 *           bin b — plain additions; the flux centroid per energy is (A_b / F_b, B_b / F_b).
 *   RTGR_SPEC_THERMAL.  nb sample frequencies theta_k in the units of emit->theta; 0 < lo <= hi; rho_min, rho_max, alpha, amp and
 *           g_power must be 0.  theta_k = lo + k (hi - lo) / (nb - 1); with RTGR_SPEC_LOG theta_k = lo exp(k log(hi / lo) / (nb - 1));
 *           nb = 1: theta_0 = lo.  T_p = the emission record's temperature law at rho_p ("disk emission" above: the same device
 *           function); the pixel counts iff T_p > 0.  tau_p = 1 / (g_p T_p).
 *           F_k = c_k sum_p w_p / expm1(theta_k tau_p), A_k and B_k likewise with w_p a_p and w_p b_p, accumulated as fma(W, e, F);
 *           c_k = emit->gain, or emit->gain theta_k^3 with RTGR_SPEC_NU3 (the flux density F_nu up to a constant), applied once, after
 *           the sum.  So without RTGR_SPEC_NU3, weight_c F(theta = theta_c) is the w-weighted sum of the picture's channel c over the disk.
 *   Order of operations, both modes: pixel order within a fixed range of pixels, then range order across the ranges; the ranges depend
 *           on n = ni nj only (the light curve's).  No floating-point atomics, no cross-lane reduction: bit-identical from run to run,
 *           from stream to stream and — for the traced entries — from one max_batch_rays to another.
 *
 * rtgr_spectrum_device_*: the stage alone over planes already on the device (d_hit32: n, d_state_end: n x 8, d_g: n, as for
 * rtgr_light_curve_device_*); d_out: nb x 3 doubles.  It only enqueues; its scratch is the stream's light-curve scratch (at most
 * 24 bytes x min(nb, 1024) x min(ceil(n / 256), 1024), grow-only, retired until rtgr_trim), so the call may be captured once a call
 * of that size was made on the stream.
 * rtgr_trace_spectrum_device_* / rtgr_trace_spectrum_* (host pointers): the arguments of rtgr_trace_observer_* with `emit` required,
 * plus `spec` and the output.  rgb, g, every per-ray output and the counters are rtgr_trace_observer_*'s bit for bit; then ONE stage
 * runs over the whole frame after the last batch.  Planes the caller did not give are borrowed from the stream's scratch.
 * rtgr_eval_spectrum_* (blocking, host pointers), from the reduction's own device functions: xyg: n x 3 = (x, y, g);
 * axis: nb doubles — LINE the bin centres lo + (b + 1/2)(hi - lo) / nb, THERMAL theta_k; bin: n int64 — LINE the bin of the point or
 * -1 where it does not count, THERMAL 0 or -1; val: LINE n doubles amp (rho / rho_min)^(-alpha) g^g_power, THERMAL n x nb doubles
 * c_k / expm1(theta_k tau); 0 where the point does not count.  n nb > 2^26 is refused.  Any output may be NULL.
 *   RTGR_ERR_BAD_ARG (with a message; the output is left untouched): a null spec, plane or output; nb = 0 or > RTGR_SPECTRUM_MAX_BINS;
 * an unknown kind or flags; reserved != 0; a non-finite field; LINE: RTGR_SPEC_LOG or RTGR_SPEC_NU3, amp < 0, rho_min or rho_max outside
 * the Disk's [r_in, r_out], rho_min >= rho_max, rho_min <= 0, lo < 0, lo >= hi; THERMAL: lo <= 0, lo > hi, a non-zero line-only field
 * (amp, alpha, rho_min, rho_max, g_power); and everything rtgr_trace_emission_* and rtgr_trace_observer_* refuse (RTGR_USER metrics,
 * 4-D grids, ...).
 *   Out of scope: spectra of the hot spot; line emissivity other than a power law; limb darkening; a colour-matching integral; linear
 * (two-bin) deposit; anti-aliasing; the sharded, frames-in-flight, pixel-array and single-ray entry points. */
enum rtgr_spectrum_kind { RTGR_SPEC_LINE = 0, RTGR_SPEC_THERMAL = 1 };
#define RTGR_SPEC_LOG 1u
#define RTGR_SPEC_NU3 2u
#define RTGR_SPECTRUM_MAX_BINS (1ull << 16)
typedef struct rtgr_spectrum {
    uint32_t kind;     /* rtgr_spectrum_kind */
    uint32_t flags;    /* 0 | RTGR_SPEC_LOG | RTGR_SPEC_NU3 (THERMAL only) */
    uint64_t nb;       /* bins (LINE) or sample frequencies (THERMAL): 1 .. RTGR_SPECTRUM_MAX_BINS */
    double lo, hi;     /* LINE: the bins cover [lo, hi) of g; THERMAL: theta_0 = lo, theta_(nb-1) = hi */
    double amp;        /* LINE: emissivity at rho_min, >= 0 */
    double alpha;      /* LINE: emissivity index, (rho / rho_min)^(-alpha) */
    double rho_min;    /* LINE: the window rho_min <= rho < rho_max, inside the Disk's [r_in, r_out] */
    double rho_max;
    double g_power;    /* LINE: q of the weight g^q */
    double reserved;   /* 0 */
} rtgr_spectrum;       /* 80 bytes: kind 0, flags 4, nb 8, lo 16, hi 24, amp 32, alpha 40, rho_min 48, rho_max 56, g_power 64, reserved 72 */
int rtgr_spectrum_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec,
                             const rtgr_observer* obs /* may be NULL */, uint64_t ni, uint64_t nj, const uint32_t* d_hit32 /* n */,
                             const double* d_state_end /* n x 8 */, const double* d_g /* n */, double* d_out /* nb x 3 */, void* stream);
int rtgr_spectrum_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec,
                             const rtgr_observer* obs /* may be NULL */, uint64_t ni, uint64_t nj, const uint32_t* d_hit32 /* n */,
                             const float* d_state_end /* n x 8 */, const float* d_g /* n */, double* d_out /* nb x 3 */, void* stream);
int rtgr_trace_spectrum_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                   const rtgr_spectrum* spec, double* d_rgb, const rtgr_ray_outputs* out, double* d_g /* n, may be NULL */,
                                   double* d_out /* nb x 3 */, rtgr_counters* ctr, void* stream);
int rtgr_trace_spectrum_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                   const rtgr_spectrum* spec, float* d_rgb, const rtgr_ray_outputs* out, float* d_g /* n, may be NULL */,
                                   double* d_out /* nb x 3 */, rtgr_counters* ctr, void* stream);
int rtgr_trace_spectrum_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit, const rtgr_spectrum* spec,
                            double* rgb, const rtgr_ray_outputs* out, double* g /* n, may be NULL */, double* spectrum /* nb x 3 */,
                            rtgr_counters* ctr);
int rtgr_trace_spectrum_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit, const rtgr_spectrum* spec,
                            float* rgb, const rtgr_ray_outputs* out, float* g /* n, may be NULL */, double* spectrum /* nb x 3 */,
                            rtgr_counters* ctr);
int rtgr_eval_spectrum_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec,
                           const double* xyg /* n x 3 */, uint64_t n, double* axis /* nb */, int64_t* bin /* n */, double* val);
int rtgr_eval_spectrum_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_spectrum* spec,
                           const float* xyg /* n x 3 */, uint64_t n, double* axis /* nb */, int64_t* bin /* n */, double* val);

/* ---- polarized disk images: Stokes Q, U by Walker-Penrose transport -----------------------------------------------------------------
 * AN EXTENSION.  In Kerr the parallel transport of a polarization vector f along a null geodesic has a closed first integral, the
 * Walker-Penrose constant.  So the linear polarization a camera sees of a disk pixel is a function of the two ray states a traced frame
 * already holds — the start state and state_end on the disk: one more small kernel around the untouched trace.
 *
 * The model (csrc/rtgr_polarization.hpp restates it; everything in the entry point's scalar type; no operation of it is fused).
 * Coordinates are the library's Kerr-Schild ones, (t, x, y, z); the metric is RTGR_KS_TRUE with the scene's `a` (the forms do not contain
 * M); RTGR_MINKOWSKI runs the same code with a = 0.
 *   Scalars and 1-forms.  pw^2 = x^2 + y^2, r the textbook Kerr radius: r^2 = (q + sqrt(q^2 + 4 a^2 z^2)) / 2, q = x^2 + y^2 + z^2 - a^2.
 *     dr     = (2 r^2 x, 2 r^2 y, 2 r^2 z + 2 a^2 z) / (4 r^3 - 2 q r)   on (dx, dy, dz)
 *     c      = z / r,   dc = dz / r - (z / r^2) dr,   s^2 = 1 - c^2
 *     dphi~  = (x dy - y dx) / pw^2 + a dr / (r^2 + a^2)
 *     w1     = dt - a s^2 dphi~          (= l - dr, l the metric's own null covector (1, (r x + a y)/(r^2 + a^2), (r y - a x)/(r^2 + a^2), z/r))
 *     w2     = (r^2 + a^2) dphi~ - a dt - a dr
 *   The two 2-forms.   Y = -a c dr^w1 + r dc^w2  (Killing-Yano);   h = -r dr^w1 - a c dc^w2  (its dual, conformal Killing-Yano).
 *   The constants.     For a null geodesic with tangent k and a vector f parallel-transported along it with g(k, f) = 0,
 *                      kappa_1 = Y_ab k^a f^b and kappa_2 = h_ab k^a f^b are constant along the ray.  Adding a multiple of k to f changes
 *                      neither; rescaling or reversing k scales both ends alike, so the traced ray's own past-directed tangent is used
 *                      at both ends as it is.
 *   Axis.              s^2 dphi~ is evaluated as (x dy - y dx)/(r^2 + a^2) + a s^2 dr/(r^2 + a^2) — regular on the axis — and
 *                      (r^2 + a^2) dphi~ as (r^2 + a^2)(x dy - y dx)/pw^2 + a dr: only this term keeps a 1/pw^2.  A point with
 *                      pw^2 <= 4096 eps (r^2 + a^2) is flagged INVALID (the forms are not evaluated there).  The disk is never there;
 *                      an observer on the axis gets NaN planes.
 *   The emitter's triad at the ray's end on the disk.  u = u_emit of "disk emission" above (the same device functions: KEPLER, RIGID).
 *     cross(v, w)_a = -sqrt(-det g) eps_abcd u^b v^c w^d (eps_0123 = +1), raised with g^{-1}: the convention of e_right = look x up.
 *     e_z'   = normalise(d_z + g(d_z, u) u)
 *     e_rho' = normalise of (0, x, y, 0)/pw made orthogonal to u and e_z'
 *     e_phi' = cross(e_z', e_rho')
 *     p = k_end + g(k_end, u) u,   p^ = p / sqrt(g(p, p))
 *   The emission law (rtgr_polarization).
 *     RTGR_POL_SCATTER  an electron-scattering atmosphere, the electric vector in the disk plane:  f_em = normalise(cross(p^, e_z')),
 *                       mu = |g(p^, e_z')|,  delta = deg0 (1 - mu) / (1 + deg1 mu),  aux = mu.
 *     RTGR_POL_FIELD    synchrotron emission in an ordered field B^ = normalise(B_rho e_rho' + B_phi e_phi' + B_z e_z'):
 *                       f_em = normalise(cross(p^, B^)),  delta = deg0,  aux = sin zeta = |cross(p^, B^)|.
 *     The pixel is INVALID if the emitter is invalid or |cross|^2 <= 4096 eps (the direction is undefined): q = u = 0 there if delta
 *     is finite, else NaN.  aux (and the hook's kappa, f_em, delta) is written before validity is known: at an invalid point it holds
 *     whatever the formulas give there — finite, infinite or NaN — and means nothing; `valid` of the hook, or q = u = 0, tells.
 *   At the camera.  State x_0, k_0 = (-e_0 + n)/sqrt(2); the frame record of `obs` (e_0, e_right, e_up, e_look).
 *     n = sqrt(2) k_0 + e_0,   e^_y = normalise(e_up - g(e_up, n) n),   e^_x = normalise(e_right - g(e_right, n) n - g(e_right, e^_y) e^_y)
 *     (alpha, beta) solve   kappa_1 = alpha Y(k_0, e^_x) + beta Y(k_0, e^_y),   kappa_2 = alpha h(k_0, e^_x) + beta h(k_0, e^_y).
 *     THE OUTPUT is the fractional Stokes pair, its position angle chi measured from e^_x towards e^_y (f = cos chi e^_x + sin chi e^_y):
 *       q = delta (alpha^2 - beta^2) / (alpha^2 + beta^2) = delta cos 2 chi,     u = 2 delta alpha beta / (alpha^2 + beta^2) = delta sin 2 chi.
 *     So turning `up` by psi towards e_right (up' = cos psi up + sin psi right) turns chi by +psi: (q, u) -> delta (cos 2(chi+psi), sin 2(chi+psi)).
 *     A degenerate screen basis (the squared norm of a projected vector <= 4096 eps) or an invalid frame gives NaN in q, u.
 *   Pixels off the disk get NaN in every plane.
 *
 * rtgr_polarization_device_*: the stage alone over planes already on the device — d_hit32 (n), d_state0 and d_state_end (n x 8 each:
 * the rays' start states, rtgr_make_observer_canvas_device_*'s, are READ, never regenerated) — into d_q, d_u (n each) and d_aux (n, may
 * be NULL).  It only enqueues (one small frame kernel, then the polarization kernel) and needs the stream's frame scratch for the
 * observer's record (512 bytes, grow-only).
 * rtgr_trace_polarized_device_* / rtgr_trace_polarized_* (host pointers): the arguments of rtgr_trace_observer_* with `emit` required,
 * plus `pol` and the three planes.  rgb, d_g, every per-ray output and the counters are rtgr_trace_observer_*'s bit for bit; the
 * polarization kernel runs on each batch's window behind the emission kernel.  They only enqueue, with one synchronisation when `ctr` is
 * given; capturable with ctr == NULL once workspace and scratch exist.  The result does not depend on max_batch_rays or on the stream.
 * rtgr_eval_polarization_* (blocking, host pointers): the polarization kernel itself in point mode at n pairs (s0, s_end) under `obs`:
 * kappa (n x 2), f_em (n x 4), aux, delta, q, u (n each), valid (n ints).  Any output may be NULL.
 * rtgr_eval_walker_penrose_* (blocking, host pointers): kappa (n x 2) = (Y(k, f), h(k, f)) at n states s = (x, k) and n vectors f, by
 * the kernel's own Y and h (NaN where the point is on the axis).
 *   RTGR_ERR_BAD_ARG (with a message; the outputs are left untouched): a null pol, emit, obs, d_q, d_u or input plane; an unknown kind;
 * flags or reserved != 0; a non-finite deg0, deg1 or field; deg0 < 0; SCATTER with deg1 <= -1 or a non-zero field; FIELD with a zero
 * field; a scene metric other than RTGR_KS_TRUE or RTGR_MINKOWSKI, with or without RTGR_METRIC_GENERIC (RTGR_KS_REF's radius is not
 * Kerr's: the constants do not exist; likewise RTGR_GRID, RTGR_USER and 4-D grids); everything rtgr_trace_emission_* and
 * rtgr_trace_observer_* refuse.
 *   Out of scope: the plane camera (obs == NULL); anti-aliasing; Q(t), U(t) of the hot spot and polarized spectra (the planes are shaped
 * so that a later change can feed them to the frame reduction in place of the centroid weights); Faraday rotation, circular
 * polarization, limb darkening; grids, RTGR_KS_REF, user metrics; the sharded, frames-in-flight, pixel-array and single-ray entries. */
enum rtgr_polarization_kind { RTGR_POL_SCATTER = 0, RTGR_POL_FIELD = 1 };
typedef struct rtgr_polarization {
    uint32_t kind;        /* rtgr_polarization_kind */
    uint32_t flags;       /* 0 */
    double deg0;          /* degree scale, >= 0 */
    double deg1;          /* SCATTER: delta = deg0 (1 - mu) / (1 + deg1 mu), > -1; FIELD: ignored */
    double field[3];      /* FIELD: B_rho, B_phi, B_z in the emitter's triad (any normalisation); SCATTER: 0 */
    double reserved[2];   /* 0 */
} rtgr_polarization;      /* 64 bytes: kind 0, flags 4, deg0 8, deg1 16, field 24, reserved 48 */
int rtgr_polarization_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol,
                                 const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32 /* n */,
                                 const double* d_state0 /* n x 8 */, const double* d_state_end /* n x 8 */, double* d_q /* n */,
                                 double* d_u /* n */, double* d_aux /* n, may be NULL */, void* stream);
int rtgr_polarization_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol,
                                 const rtgr_observer* obs, uint64_t ni, uint64_t nj, const uint32_t* d_hit32 /* n */,
                                 const float* d_state0 /* n x 8 */, const float* d_state_end /* n x 8 */, float* d_q /* n */,
                                 float* d_u /* n */, float* d_aux /* n, may be NULL */, void* stream);
int rtgr_trace_polarized_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                    uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                    const rtgr_polarization* pol, double* d_rgb, const rtgr_ray_outputs* out, double* d_g /* n, may be NULL */,
                                    double* d_q /* n */, double* d_u /* n */, double* d_aux /* n, may be NULL */, rtgr_counters* ctr,
                                    void* stream);
int rtgr_trace_polarized_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                    uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                                    const rtgr_polarization* pol, float* d_rgb, const rtgr_ray_outputs* out, float* d_g /* n, may be NULL */,
                                    float* d_q /* n */, float* d_u /* n */, float* d_aux /* n, may be NULL */, rtgr_counters* ctr,
                                    void* stream);
int rtgr_trace_polarized_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                             uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                             const rtgr_polarization* pol, double* rgb, const rtgr_ray_outputs* out, double* g /* n, may be NULL */,
                             double* q /* n */, double* u /* n */, double* aux /* n, may be NULL */, rtgr_counters* ctr);
int rtgr_trace_polarized_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                             uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit,
                             const rtgr_polarization* pol, float* rgb, const rtgr_ray_outputs* out, float* g /* n, may be NULL */,
                             float* q /* n */, float* u /* n */, float* aux /* n, may be NULL */, rtgr_counters* ctr);
int rtgr_eval_polarization_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol,
                               const rtgr_observer* obs, const double* s0 /* n x 8 */, const double* s_end /* n x 8 */, uint64_t n,
                               double* kappa /* n x 2 */, double* f_em /* n x 4 */, double* aux /* n */, double* delta /* n */,
                               double* q /* n */, double* u /* n */, int* valid /* n */);
int rtgr_eval_polarization_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_disk_emission* emit, const rtgr_polarization* pol,
                               const rtgr_observer* obs, const float* s0 /* n x 8 */, const float* s_end /* n x 8 */, uint64_t n,
                               float* kappa /* n x 2 */, float* f_em /* n x 4 */, float* aux /* n */, float* delta /* n */,
                               float* q /* n */, float* u /* n */, int* valid /* n */);
int rtgr_eval_walker_penrose_f64(rtgr_context* ctx, const rtgr_scene* scene, const double* s /* n x 8 */, const double* f /* n x 4 */,
                                 uint64_t n, double* kappa /* n x 2 */);
int rtgr_eval_walker_penrose_f32(rtgr_context* ctx, const rtgr_scene* scene, const float* s /* n x 8 */, const float* f /* n x 4 */,
                                 uint64_t n, float* kappa /* n x 2 */);

/* ---- higher-order disk images: follow rays through the disk, order by order ---------------------------------------------------------
 * AN EXTENSION.  The trace ends a ray at its first event, so an emitting disk is an opaque wall.  Here a ray that ends on the emitting
 * disk D = (h, r_in, r_out) is carried through the slab and traced on; where it meets D again is the next ORDER of the image: order 1 is
 * the lensed image of the far side and the underside, order >= 2 the photon ring.  The integrate kernels are untouched: every leg is an
 * ordinary trace of caller-supplied states, and the way through the slab uses two things the library guarantees — a ray traced from a
 * given state is that state's ray to the bit whatever is traced beside it, and a ray that starts inside an object ends with an event
 * where it leaves it.
 *
 * The model (everything in the entry point's scalar type; no operation of the picture is fused).
 *   Leg 0.  The frame of rtgr_trace_observer_* with `emit`: its rgb, state_end, hit32, status and g — or, with `state0` given, the same
 *     of the caller's n = ni nj ray states in place of the observer's (as rtgr_trace_* takes them); `obs` may then be NULL: u_obs is the
 *     static observer at the ray's start, the rule of rtgr_eval_disk_emission_*.
 *   Continuing set after order k.  The pixels whose order-k leg has hit32 == emit->object (the emission kernel's own rule).
 *   Crossing leg.  A trace of those end states in the scene S+ : the caller's metric and exactly ONE object, the inflated disk
 *     D+ = (h + eta, r_in - eta, r_out + eta), eta = `margin` (0: h / 2).  The ray starts inside D+, at distance <= -eta, and ends with an
 *     event on its surface — outside D, at distance eta.  The caller's other objects are NOT in S+: an object that pokes into the slab is
 *     not seen from inside it.  The solver record is the caller's, and every leg runs lambda from lambda0 to lambda1 afresh.
 *     A ray goes on iff its crossing leg ended with status RTGR_RAY_EVENT on object 1; any other ray stops there and contributes no
 *     background (it is absorbed).
 *   Continuation leg.  A trace of the crossing legs' end states in the caller's scene S: its hit32, status and state_end are order k + 1's.
 *   Emission of order k.  "disk emission" above, evaluated by the emission kernel itself on the pair (the pixel's start state, its order-k
 *     end state): g_k = (k_0 . u_obs) / (k_end,k . u_emit), with the e_0 of `obs` when it is given.  rtgr_eval_disk_emission_observer_*
 *     (rtgr_eval_disk_emission_* for obs == NULL) predicts E_k and g_k to the bit.
 *   The picture.  rgb starts as leg 0's (E_0 on the disk, the plain or shaded colour elsewhere); t = T (`transmission`); for
 *     k = 1 .. m_p - 1:  rgb = rgb + t E_k, then t = t T  (m_p: the number of disk crossings found for the pixel, at most max_order + 1);
 *     if the last continuation leg ended somewhere other than the disk:  rgb = rgb + t B,  B the colour the trace gave that end (the
 *     shading kernel applied when `shade` binds that object or the escape).  A pixel that still continues after order max_order stops.
 *     T = 0 reproduces the frame of rtgr_trace_observer_* with `emit`, with one exception: a pixel of the continuing set whose colour
 *     channel is -0 becomes +0 (it has 0 added to it).
 *   Outputs besides rgb (rtgr_order_planes; any member may be NULL).  count: n bytes, m_p.  Per-order planes, order-major, max_order + 1
 *     blocks each: hit32 (n per block), state_end (n x 8), g (n), rgb_order (3 planes of n: the frame's own layout).  Block 0 is leg 0's,
 *     as rtgr_trace_observer_* delivers it, for every pixel.  Block k >= 1: hit32 = emit->object, the end state, g_k and E_k where the
 *     pixel has order k; 0 in hit32 and NaN in the others where it has not.  state0: n x 8, the rays' start states.  One block of these
 *     planes plus state0 is what rtgr_light_curve_device_*, rtgr_spectrum_device_* and rtgr_polarization_device_* take: the Walker-Penrose
 *     constants are conserved across the crossings, so the polarization of order k needs only the start state and the order-k end state.
 *   ctr: the sum over all legs.
 * rtgr_trace_orders_device_*: on the device that holds d_rgb, stream `stream`.  Legs run in chunks of at most obs->max_batch_rays rays
 * (0 or obs == NULL: 2^22) through the stream's frame and batch scratch (grow-only).  The call reads the length of each leg's list back:
 * two synchronisations per order, so it is refused while the stream is captured.  The result does not depend on max_batch_rays or on the
 * stream.  rtgr_trace_orders_*: host pointers, on device 0 of the context.
 *   RTGR_ERR_BAD_ARG (with a message): everything rtgr_trace_observer_* with `emit` refuses (obs == NULL is accepted with state0 only);
 * a null ord, emit or rgb; max_order = 0 or > 8; a margin that is not finite, <= 0 after the default, or >= r_in; a transmission outside
 * [0, 1] or NaN; flags or pad != 0; a stream under capture.
 *   Out of scope: emission integrated through the slab's depth; an angle-dependent optical depth; more than one emitting disk;
 * anti-aliasing; the sharded and frames-in-flight entry points; RTGR_USER metrics and 4-D grids; a light curve summed over orders in one
 * call (the per-order stage calls cover it). */
#define RTGR_MAX_DISK_ORDER 8
typedef struct rtgr_disk_orders {
    uint32_t max_order;    /* N: orders 1 .. N are looked for, 1 <= N <= RTGR_MAX_DISK_ORDER */
    uint32_t flags;        /* 0 */
    double margin;         /* eta; 0: half the disk's half thickness */
    double transmission;   /* T in [0, 1] */
    uint64_t pad;          /* 0 */
} rtgr_disk_orders;        /* 32 bytes: max_order 0, flags 4, margin 8, transmission 16, pad 24 */
typedef struct rtgr_order_planes {
    uint8_t* count;        /* n */
    uint32_t* hit32;       /* (N + 1) x n */
    void* state_end;       /* (N + 1) x n x 8 scalars */
    void* g;               /* (N + 1) x n scalars */
    void* rgb_order;       /* (N + 1) x 3 x n scalars */
    void* state0;          /* n x 8 scalars */
} rtgr_order_planes;       /* 48 bytes; device or host pointers according to the call */
int rtgr_trace_orders_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs /* may be NULL with d_state0 */,
                                 const double* d_state0 /* n x 8, may be NULL */, uint64_t ni, uint64_t nj, const rtgr_shade* shade /* may be NULL */,
                                 const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, double* d_rgb, const rtgr_order_planes* planes /* may be NULL */,
                                 rtgr_counters* ctr, void* stream);
int rtgr_trace_orders_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs /* may be NULL with d_state0 */,
                                 const float* d_state0 /* n x 8, may be NULL */, uint64_t ni, uint64_t nj, const rtgr_shade* shade /* may be NULL */,
                                 const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, float* d_rgb, const rtgr_order_planes* planes /* may be NULL */,
                                 rtgr_counters* ctr, void* stream);
int rtgr_trace_orders_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs /* may be NULL with state0 */,
                          const double* state0 /* n x 8, may be NULL */, uint64_t ni, uint64_t nj, const rtgr_shade* shade /* may be NULL */,
                          const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, double* rgb, const rtgr_order_planes* planes /* may be NULL */,
                          rtgr_counters* ctr);
int rtgr_trace_orders_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs /* may be NULL with state0 */,
                          const float* state0 /* n x 8, may be NULL */, uint64_t ni, uint64_t nj, const rtgr_shade* shade /* may be NULL */,
                          const rtgr_disk_emission* emit, const rtgr_disk_orders* ord, float* rgb, const rtgr_order_planes* planes /* may be NULL */,
                          rtgr_counters* ctr);

/* ---- volume emission: radiative transfer through a hot flow along each ray ------------------------------------------------------------
 * AN EXTENSION.  Every other emitter of the library is a surface: a ray carries no radiation until its first event.  Here a rotating,
 * geometrically thick, optically thin (or grey) flow fills the space around the hole and the intensity is ACCUMULATED along the ray: the
 * pictures whose ring is emission gathered by rays that wind round the photon orbit.  The trace is untouched; one more kernel runs behind
 * it and integrates the transfer equations along each ray's own geodesic, as far as the trace followed that ray.
 *
 * The model (csrc/rtgr_transfer.hpp: ONE device function; everything in the entry point's scalar type; none of its own operations is
 * fused).  The gas is axisymmetric and rotates on cylinders at the equatorial circular-orbit rate, exactly as the disk of "disk
 * emission" does.  At a point x = (t, x, y, z) of a ray with tangent k, started at x_0 with tangent k_0:
 *     rho = hypot(x, y),   r = sqrt(x^2 + y^2 + z^2)                                 (coordinate terms)
 *     density   n = (r / r0)^(-alpha) exp(-z^2 / (2 H^2 rho^2));   a non-finite n counts as 0
 *     flow      RTGR_EMIT_KEPLER: Omega = the orbital rate of "disk emission" at (t, x, y, 0), root `orbit` = +1 / -1 — the same device
 *               function, so at z = 0 the flow's rate is the disk's bit for bit;   RTGR_EMIT_RIGID: Omega = orbit
 *     emitter   xi = (1, -Omega y, Omega x, 0),   n2 = g(x)(xi, xi),   u_f = xi / sqrt(-n2)
 *               the point is VALID iff the orbit exists (B^2 - A C >= 0, C != 0), Omega and n2 are finite and n2 < 0
 *     w = g(x)(k, u_f),   kappa0 = g(x_0)(k_0, u_obs),   gfac = kappa0 / w
 *               u_obs: the e_0 of the observer's frame (rtgr_trace_transfer_*; the hooks with `obs`), or, obs == NULL, the static
 *               observer at x_0 as in rtgr_eval_disk_emission_*
 *   The two transfer equations run along the traced direction, from the camera outwards.  I is the observed specific intensity at the
 *   channel's own frequency, the emissivity j_nu ~ n nu^(-s), the absorption grey:
 *     dtau/dlambda = kappa n w
 *     dI/dlambda   = j0 n w gfac^(3+s) exp(-tau)
 *   Both are 0 where the point is invalid or gfac is not > 0: there is no gas inside the photon orbit's cylinder.  The EMISSION goes to
 *   0 continuously there (w gfac^(3+s) = kappa0 gfac^(2+s), gfac -> 0), with a kink: ~ (rho - rho_ph)^((2+s)/2).
 *   A LIMITATION OF THE MODEL, kappa > 0.  The ABSORPTION does not: n2 -> 0- at the cylinder, so w ~ 1 / sqrt(-n2) and dtau/dlambda =
 *   kappa n w is UNBOUNDED there (integrable, but no adaptive step gets across it at the solver's tolerance).  A Float64 ray that
 *   crosses the cylinder where the density is not negligible ends with a step-size underflow: status 3, I = tau = NaN, and — it was
 *   integrated, so the picture rule applies — rgb = NaN in all three channels.  In the a = 0.9 example at inclination 60 degrees that
 *   is every pixel of the shadow and its rim, 12 % of the frame.  Rays that enter the cylinder far above the plane (n ~ 0), every ray
 *   with kappa = 0, and Float32 (whose coarser steps get across) are not affected.  A dtau that stays bounded at the cylinder would
 *   remove this; that is a change of the model, not made here.
 *   The picture.  rgb_c = rgb_c(traced, shaded, emitted) exp(-tau_end) + gain weight_c I_end.  Three channels of a power law with grey
 *   absorption differ by a constant only, so ONE I and ONE tau are integrated per ray.
 *
 * The integration (transfer_kernel, one lane per ray).  y = (x, k, tau, I), 10 components, from the ray's own start state over
 * [lambda0, lambda_end], lambda_end what the trace reported for that ray.  Tsit5 with the trace's coefficients, the geodesic half the
 * closed right-hand side of the scene's metric (also under RTGR_METRIC_GENERIC); the initial step from the geodesic part, the PI
 * controller of the trace with the rms norm over all 10 components and the solver's abstol / reltol — the step adapts to the emission;
 * the last step is clipped to lambda_end exactly.  It ends earlier
 *   - at the first ACCEPTED step whose end has r < r_stop.  This is not a root-find: CHOOSE r_stop INSIDE THE DARK CYLINDER, where it
 *     cannot change I (it spares a captured ray the steps towards the horizon); 0 for RTGR_MINKOWSKI;
 *   - after opt->max_steps attempts; on a non-finite error estimate; on a step-size underflow.
 * Per-ray status byte: 0 = reached lambda_end, 1 = r_stop, 2 = step cap, 3 = not integrated or not finite (I = tau = NaN).  Status 3
 * has two sources.  Rays the trace ended as RTGR_RAY_NAN, or whose start state or lambda_end is not finite, are NOT INTEGRATED: tsteps
 * = 0, and their rgb is left as traced.  Rays whose integration ended not finite (a non-finite error estimate, a step-size underflow
 * — the kappa > 0 limitation above) WERE integrated: tsteps > 0, and their rgb is NaN.
 *
 * rtgr_trace_transfer_device_* / rtgr_trace_transfer_* (host pointers): the arguments of rtgr_trace_observer_*, plus `flow`, four
 * optional planes — d_I, d_tau (n scalars), d_tstatus (n bytes), d_tsteps (n x uint32: step attempts) — and tctr, the counters of the
 * transfer pass alone (rays integrated, accepted, rejected, rhs_evals, events = rays ended at r_stop, not_finished = status >= 2); ctr
 * stays the trace's.  Every per-ray output of `out`, ctr and d_g are rtgr_trace_observer_*'s bit for bit.  Per batch: the observer
 * trace's work, then the transfer kernel over the batch, reading the start states where the batch left them; lambda_end and the status
 * bytes are borrowed from the stream's frame scratch when `out` does not ask for them (grow-only).  They only enqueue, with one
 * synchronisation when ctr or tctr is given; capturable with ctr == tctr == NULL once workspace and scratch exist.  The result does
 * not depend on max_batch_rays or on the stream.
 * rtgr_eval_transfer_* (blocking, host pointers): the same kernel body over n listed rays (s0, lambda_end): I, tau, tstatus, tsteps
 * and s_end (n x 8: where the integration ended).  Any output may be NULL.  It predicts a pixel of the frame to the bit.
 * rtgr_eval_flow_* (blocking, host pointers): the pointwise model at n points s = (x, k) of rays started at s0: dens, omega,
 * u_f (n x 4), gfac, dtau and dI0 = dI/dlambda at tau = 0.  Any output may be NULL.  An invalid point gives NaN in omega, u_f and
 * gfac and 0 in the two derivatives.
 *   RTGR_ERR_BAD_ARG (with a message that names the field; the outputs are left untouched): a null flow; an unknown emitter;
 * flags != 0; KEPLER with orbit other than +1 / -1; j0 < 0, kappa < 0, r0 <= 0, H <= 0, r_stop < 0, or any parameter NaN or infinite;
 * RTGR_USER metrics; RTGR_GRID and 4-D grids; everything rtgr_trace_observer_* refuses.
 *   Out of scope: grids and user metrics; plunging gas inside the innermost stable orbit (the orbits used there are the unstable
 * circular ones); frequency-dependent absorption and thermal synchrotron emissivities; polarized transfer; anti-aliasing, the sharded
 * and frames-in-flight entries; orders >= 1 of "higher-order disk images" (the flow is integrated along leg 0 only); a per-wave table
 * of Omega(rho) or a persistent refilling kernel, the obvious next steps if the transfer pass is to cost less. */
typedef struct rtgr_flow {
    uint32_t emitter;     /* rtgr_emitter */
    uint32_t flags;       /* 0 */
    double orbit;         /* KEPLER: +1 / -1; RIGID: Omega */
    double j0, kappa;     /* >= 0; kappa = 0: optically thin */
    double r0, alpha, H, s;   /* r0 > 0, H > 0, finite alpha, s */
    double r_stop;        /* >= 0 */
    double gain, weight[3];
} rtgr_flow;  /* 104 bytes: emitter 0, flags 4, orbit 8, j0 16, kappa 24, r0 32, alpha 40, H 48, s 56, r_stop 64, gain 72, weight 80 */
int rtgr_trace_transfer_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                                   const rtgr_flow* flow, double* d_rgb, const rtgr_ray_outputs* out, double* d_g /* n, NULL without emit */,
                                   double* d_I /* n, may be NULL */, double* d_tau /* n, may be NULL */, uint8_t* d_tstatus /* n, may be NULL */,
                                   uint32_t* d_tsteps /* n, may be NULL */, rtgr_counters* ctr, rtgr_counters* tctr, void* stream);
int rtgr_trace_transfer_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                                   uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                                   const rtgr_flow* flow, float* d_rgb, const rtgr_ray_outputs* out, float* d_g /* n, NULL without emit */,
                                   float* d_I /* n, may be NULL */, float* d_tau /* n, may be NULL */, uint8_t* d_tstatus /* n, may be NULL */,
                                   uint32_t* d_tsteps /* n, may be NULL */, rtgr_counters* ctr, rtgr_counters* tctr, void* stream);
int rtgr_trace_transfer_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                            const rtgr_flow* flow, double* rgb, const rtgr_ray_outputs* out, double* g /* n, NULL without emit */,
                            double* I /* n, may be NULL */, double* tau /* n, may be NULL */, uint8_t* tstatus /* n, may be NULL */,
                            uint32_t* tsteps /* n, may be NULL */, rtgr_counters* ctr, rtgr_counters* tctr);
int rtgr_trace_transfer_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_observer* obs, uint64_t ni,
                            uint64_t nj, const rtgr_shade* shade /* may be NULL */, const rtgr_disk_emission* emit /* may be NULL */,
                            const rtgr_flow* flow, float* rgb, const rtgr_ray_outputs* out, float* g /* n, NULL without emit */,
                            float* I /* n, may be NULL */, float* tau /* n, may be NULL */, uint8_t* tstatus /* n, may be NULL */,
                            uint32_t* tsteps /* n, may be NULL */, rtgr_counters* ctr, rtgr_counters* tctr);
int rtgr_eval_transfer_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_flow* flow,
                           const rtgr_observer* obs /* may be NULL: static observer */, const double* s0 /* n x 8 */,
                           const double* lambda_end /* n */, uint64_t n, double* I /* n */, double* tau /* n */, double* s_end /* n x 8 */,
                           uint8_t* tstatus /* n */, uint32_t* tsteps /* n */);
int rtgr_eval_transfer_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_flow* flow,
                           const rtgr_observer* obs /* may be NULL: static observer */, const float* s0 /* n x 8 */,
                           const float* lambda_end /* n */, uint64_t n, float* I /* n */, float* tau /* n */, float* s_end /* n x 8 */,
                           uint8_t* tstatus /* n */, uint32_t* tsteps /* n */);
int rtgr_eval_flow_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_flow* flow, const rtgr_observer* obs /* may be NULL */,
                       const double* s0 /* n x 8 */, const double* s /* n x 8: a point and tangent */, uint64_t n, double* dens /* n */,
                       double* omega /* n */, double* u_f /* n x 4 */, double* gfac /* n */, double* dtau /* n */, double* dI0 /* n */);
int rtgr_eval_flow_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_flow* flow, const rtgr_observer* obs /* may be NULL */,
                       const float* s0 /* n x 8 */, const float* s /* n x 8: a point and tangent */, uint64_t n, float* dens /* n */,
                       float* omega /* n */, float* u_f /* n x 4 */, float* gfac /* n */, float* dtau /* n */, float* dI0 /* n */);

/* ---- camera: make_canvas (src/RayTraceGR.jl:457-478) on the device ------------------------------------------
 * Writes n x 8 ray states (pos, null past-directed 4-velocity) for rows [j0, j1).  Device / host variants. */
int rtgr_make_canvas_device_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni,
                                uint64_t nj, uint64_t j0, uint64_t j1, double* d_state0, void* stream);
int rtgr_make_canvas_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                         uint64_t j0, uint64_t j1, double* state0);
/* T = Float32 (make_canvas is generic in T, :457-462) */
int rtgr_make_canvas_device_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni,
                                uint64_t nj, uint64_t j0, uint64_t j1, float* d_state0, void* stream);
int rtgr_make_canvas_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_camera* cam, uint64_t ni, uint64_t nj,
                         uint64_t j0, uint64_t j1, float* state0);

/* ---- physics kernels exposed for parity tests (test/runtests.jl:12-61 exercises exactly these) -------------
 * Evaluated ON THE DEVICE for n points (host pointers in/out):
 *   g   : n x 16  metric g_ab            (minkowski / kerr_schild, :262-294)
 *   dg  : n x 64  dg[a][b][c] = d_c g_ab (dmetric, :302-313)
 *   Gam : n x 64  Gamma^a_bc             (christoffel, :321-331)
 * Any output may be NULL.  _f32: T = Float32, as the reference's Kerr-Schild testset runs it (test/runtests.jl:37). */
int rtgr_eval_metric_f64(rtgr_context* ctx, const rtgr_scene* scene, const double* x /* n x 4 */, uint64_t n, double* g,
                         double* dg, double* Gam);
int rtgr_eval_metric_f32(rtgr_context* ctx, const rtgr_scene* scene, const float* x /* n x 4 */, uint64_t n, float* g,
                         float* dg, float* Gam);
/* geodesic RHS (src/RayTraceGR.jl:358-370): n x 8 states -> n x 8 derivatives, on the device.
 * path = 0: Kerr–Schild-form closed contraction with IEEE division (the tile kernel's RHS);
 * path = 1: generic dual-number path (RTGR_METRIC_GENERIC, user metrics);
 * path = 2: EXACTLY the function the production integrate loop calls (closed contraction with the fast reciprocal /
 *           reciprocal-square-root sequences, null-congruence shortcuts of the textbook metric). */
int rtgr_eval_geodesic_f64(rtgr_context* ctx, const rtgr_scene* scene, const double* s /* n x 8 */, uint64_t n, int path,
                           double* ds /* n x 8 */);
int rtgr_eval_geodesic_f32(rtgr_context* ctx, const rtgr_scene* scene, const float* s /* n x 8 */, uint64_t n, int path,
                           float* ds /* n x 8 */);
/* objects and the colour rule at n points, on the device (host pointers): `distance(obj, x)` of every object of the scene in scene order
 * (src/RayTraceGR.jl:377-419; user objects: the unit's rtgr_user_distance), `min_distance(objs, s)` (:433-441) and the colouring loop of
 * trace_rays (:513-533: nearest object below opt->hit_threshold, objcolor x omin / length(objs), else opt->miss_rgb) evaluated at x as
 * if a ray had ended there.  x: n x 4;  d: n x nobj;  dmin: n;  hit: n (omin, 0 = miss);  rgb: n x 3 (AoS).  Any output may be NULL. */
int rtgr_eval_objects_f64(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const double* x /* n x 4 */, uint64_t n,
                          double* d, double* dmin, uint8_t* hit, double* rgb);
int rtgr_eval_objects_f32(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const float* x /* n x 4 */, uint64_t n,
                          float* d, float* dmin, uint8_t* hit, float* rgb);
/* the hot loop's reciprocal and reciprocal-square-root sequences (hardware seed + one third-order correction) on n
 * operands; either output may be NULL */
int rtgr_eval_fastmath_f64(rtgr_context* ctx, const double* x, uint64_t n, double* rcp, double* rsq);

/* ---- user metrics: "metric is ANY callable x -> g" (src/RayTraceGR.jl:302-309, :358-370, :457-511) ------------
 * The reference accepts any Julia function as the metric and differentiates it with forward duals.  The native
 * counterpart: the caller writes the metric once as a C++ function template over the scalar type
 *     template <class S> __device__ void rtgr_user_metric(const S x[4], double M, double a, S g[4][4]);
 * (S = double / float for make_canvas' normalisation, S = 4-wide forward dual of either for dmetric), pastes it into
 * raytracegr.jl_amd/csrc/rtgr_user_unit.hip.in, compiles that unit with
 *     hipcc --genco --no-gpu-bundle-output --offload-arch=gfx950 -O3 -std=c++17 -I<csrc> unit.hip -o metric.hsaco
 * and hands the code object to the library, which loads it on every device of the context and returns its id (a hash
 * of the code object: loading the same file twice yields the same id and one resident copy).  A scene selects it with
 * metric = RTGR_USER and user_metric = id, in every entry point that takes a scene (trace, make_canvas, eval_metric,
 * eval_geodesic path 1); M and a of the scene are passed through to the function.  Several metrics may be resident at
 * once.  The Python mirror automates the steps (api.UserMetric).
 *
 * A metric OF KERR–SCHILD FORM, g = eta + f k (x) k with k_t = 1, k null with respect to eta and no t-dependence, may be given
 * by its two ingredients instead of its 16 entries:
 *     template <class S> __device__ void rtgr_user_ks(const S x[4], double M, double a, S& f, S k[3]);
 * (unit built with -DRTGR_USER_KS=1 -DRTGR_USER_NE=3; rtgr_user_metric_compile detects the name in the source text).  The
 * unit derives the 16 entries for make_canvas and the evaluation hooks; its integrate kernels differentiate the four scalars
 * (f, k_x, k_y, k_z) and use the closed contraction of the built-in metrics — no 4x4 solve.
 * rtgr_eval_geodesic_f64(path = 2) on a user scene evaluates exactly that loop RHS. */
int rtgr_user_metric_load(rtgr_context* ctx, const char* code_object_path, uint64_t* id_out);
/* The same in ONE call from source text: `source` (the definition of rtgr_user_metric<S>, as above) is pasted into the unit
 * template, compiled IN-PROCESS and loaded — no hipcc on the box, no child process, ~10 s for a light metric.  The build goes
 * hiprtc (source -> optimised bitcode) -> libamd_comgr (bitcode -> assembly listing -> code object), both resolved with dlopen at
 * first use, with a look at the LISTING in between: the check and repair described below.  stationary != 0 declares that the metric
 * does not depend on t (-DRTGR_USER_NE=3: the integrate kernels carry the three spatial partials only).  A unit whose integrate
 * kernels would spill is rebuilt with more registers per lane.  The unit template and device headers are read from the `csrc`
 * directory next to librtgr_hip.so (or $RTGR_CSRC).  On a compile error the compiler's log is the rtgr_last_error(). */
int rtgr_user_metric_compile(rtgr_context* ctx, const char* source, int stationary, uint64_t* id_out);
/* The build step of rtgr_user_metric_compile on its own: source text -> code object FILE for rtgr_user_metric_load (build once,
 * keep the file, load it in every later process).  Needs no GPU and no context. */
int rtgr_user_metric_build(const char* source, int stationary, const char* code_object_path);
int rtgr_user_metric_unload(rtgr_context* ctx, uint64_t id); /* id 0: all */

/* ---- metrics sampled on a grid: a spacetime that exists only as numbers ------------------------------------------------
 * A numerically computed spacetime (e.g. a binary black hole from a numerical-relativity code) is g_ab sampled on a Cartesian
 * grid; no source text can stand in for it.  A STATIONARY metric (d_t g = 0) sampled on a uniform 3-D grid is handed over as data:
 *   grid->n[3]        samples along x, y, z (each >= 4);  grid->pad = 0
 *   grid->origin[3]   (x, y, z) of sample (0, 0, 0);      grid->spacing[3] > 0 (h_x, h_y, h_z)
 *   g                 n[2]*n[1]*n[0]*10 doubles, x fastest: sample (i, j, k) at g[((k*n[1] + j)*n[0] + i)*10 + c], the 10
 *                     components the upper triangle in row order: tt tx ty tz xx xy xz yy yz zz
 * The call refuses (RTGR_ERR_BAD_ARG, the index of the first bad sample in rtgr_last_error()) any non-finite value and any sample
 * with det g >= 0 (which also catches a transposed layout), and grids of more than RTGR_GRID_MAX_SAMPLES points.  It uploads the
 * samples to every device of the context, in Float64 and in Float32 (the _f32 entry points read the latter), and returns an id; a
 * scene selects the grid with metric = RTGR_GRID, user_metric = id in every entry point that takes a scene.  Grid ids and unit ids
 * never coincide.  M and a of the scene are not read.
 *   Interpolant: tricubic Catmull-Rom (cubic convolution, a = -1/2), separable.  Per axis s = (x - origin)/h, i = clamp(floor(s),
 * 1, n - 3), t = s - i, weights on samples i-1 .. i+2:  (-t^3 + 2t^2 - t)/2, (3t^3 - 5t^2 + 2)/2, (-3t^3 + 4t^2 + t)/2, (t^3 - t^2)/2;
 * derivative weights d/dt of those times 1/h.  It interpolates the samples, g and its first derivatives are continuous across cell
 * faces, quadratics are reproduced exactly, and g and dg come from the same polynomial.  The VALID BOX is s in [1, n - 2] on every
 * axis; outside it the clamped cell's cubic is extrapolated (finite, meaningless).  Every geodesic RHS evaluation reads 4x4x4
 * samples: 16 rows of 4 consecutive x-samples, 40 contiguous doubles each.
 *   Tracing: a step whose scan finds an event ends the ray as RTGR_RAY_EVENT; otherwise an accepted step that ends outside the valid
 * box ends it as RTGR_RAY_OUTSIDE with state_end / lambda_end at the end of that step; a ray that STARTS outside ends as
 * RTGR_RAY_OUTSIDE with 0 accepted steps.  All entry points (device, host-pointer, frames in flight, sharded) and both pass
 * structures (FULL == FAR + NEAR bit for bit) take grid scenes; rtgr_make_canvas_*, the redshift output and rtgr_eval_metric_*
 * evaluate the interpolant (d_t g = 0), rtgr_eval_geodesic_* evaluates the grid RHS for every `path`.  Out of scope: user objects in
 * a grid scene (RTGR_ERR_BAD_ARG), several patches.
 *   Lifetime: rtgr_grid_metric_unload makes the id unknown at once (a scene naming it fails with RTGR_ERR_BAD_ARG), but the device
 * memory is RETIRED, not freed — a hipGraph captured earlier may still replay it — until rtgr_trim / rtgr_destroy. */
#define RTGR_GRID_MAX_SAMPLES (1ull << 28)   /* n[0]*n[1]*n[2] (4-D: n[0]*n[1]*n[2]*n[3]) at most: 21.5 GB in Float64 + 10.7 GB in Float32 per device */
typedef struct rtgr_grid {
    uint32_t n[3];      /* samples along x, y, z; each >= 4 */
    uint32_t pad;       /* 0 */
    double origin[3];   /* (x, y, z) of sample (0,0,0) */
    double spacing[3];  /* > 0 */
} rtgr_grid;            /* 64 bytes */
int rtgr_grid_metric_load(rtgr_context* ctx, const rtgr_grid* grid, const double* g, uint64_t* id_out);
int rtgr_grid_metric_unload(rtgr_context* ctx, uint64_t id);

/* A TIME-DEPENDENT metric sampled on a uniform 4-D grid (an evolving spacetime, slice after slice):
 *   grid->n[4]        samples along t, x, y, z (each >= 4);   grid->origin[4] (t, x, y, z) of sample (0, 0, 0, 0);  grid->spacing[4] > 0
 *   g                 n[0]*n[3]*n[2]*n[1]*10 doubles, TIME SLOWEST: sample (l, k, j, i) — t, z, y, x — at
 *                     g[(((l*n_z + k)*n_y + j)*n_x + i)*10 + c]; every time slice is one block in rtgr_grid_metric_load's layout
 * The same checks as rtgr_grid_metric_load (the flattened index of the first bad sample in rtgr_last_error()), at most
 * RTGR_GRID_MAX_SAMPLES samples in all (n_t n_x n_y n_z), Float64 and Float32 copies on every device; ids come from the same counter,
 * a scene selects the grid the same way (metric = RTGR_GRID, user_metric = id) and rtgr_grid_metric_unload unloads either kind.
 *   Interpolant: the tensor product of the Catmull-Rom weights above on all four axes; d_t g from the time weights' derivatives x 1/h_t,
 * g and all four first derivatives from the same polynomial.  Summation order: per spatial row, the four time slices are blended first,
 * relative to the time-centre slice s_1 — b = (s_1 - ref) + sum_l w_t,l (s_l - s_1), b' = sum_l w'_t,l (s_l - s_1) — and b is then
 * walked like the 3-D stencil (ref = the centre sample of the centre slice).  So a grid whose slices are all equal gives g and
 * d_x,y,z g bit for bit as the 3-D grid of one slice, and d_t g = 0 exactly.  The VALID BOX is s in [1, n - 2] on all four axes:
 * an accepted step that ends outside it — in time too — ends the ray as RTGR_RAY_OUTSIDE, and a ray whose start (camera) time is
 * outside ends as RTGR_RAY_OUTSIDE with 0 accepted steps.  rtgr_make_canvas_*, redshift, rtgr_eval_metric_* and rtgr_eval_geodesic_*
 * evaluate the interpolant at the point's own t. */
typedef struct rtgr_grid4 {
    uint32_t n[4];      /* samples along t, x, y, z; each >= 4 */
    double origin[4];   /* (t, x, y, z) of sample (0,0,0,0) */
    double spacing[4];  /* > 0 */
} rtgr_grid4;           /* 80 bytes: n 0, origin 16, spacing 48 */
int rtgr_grid4_metric_load(rtgr_context* ctx, const rtgr_grid4* grid, const double* g, uint64_t* id_out);

/* ---- user objects: `Object{T}` is an OPEN abstract type (src/RayTraceGR.jl:374-389) ------------------------------------------
 * The reference's second extension point: any `struct MyThing{T} <: Object{T}` with the two methods
 *     distance(obj, pos::SVector{D,T})::T                "zero on the surface, positive outside, negative inside"   (:377-386)
 *     objcolor(obj, pos::SVector{D,T})::SVector{3,T}                                                                 (:387-389)
 * is traced — the ContinuousCallback condition min_distance dispatches on it (:433-441) and so does the colour rule (:518-530).
 * The native counterpart mirrors user metrics: the two methods are written once as device function templates over the scalar
 *     template <class S> __device__ S    rtgr_user_distance(unsigned type, const S x[4], const S p[9]);
 *     template <class S> __device__ void rtgr_user_objcolor(unsigned type, const S x[4], const S p[9], S rgb[3]);
 * (S = double or float; `type` and `p` are the rtgr_object's: one source may define several object types and switch on `type`;
 * the m* helpers of user metrics — msqrt mabs macos matan2 ... — are available), and compiled at run time into the scene's UNIT,
 * the code object that carries every kernel that calls them: ray set-up (the condition's initial sign), the FAR / NEAR / FULL
 * integrate passes (the sample-point scan) and the resolve kernel (event root-find, colour rule).  Objects are independent of
 * the metric in the reference; in compiled code the integrate kernels contain both, so a unit is built for ONE metric variant:
 * its own (the same source also defines rtgr_user_metric / rtgr_user_ks), or a built-in one, named by `built_for` — the scene
 * the unit is meant for: its metric enum, RTGR_METRIC_GENERIC flag and whether a != 0 select the kernels' instantiation; its
 * objects and the values of M and a do not matter — exactly what Julia specialises `solve` on.  A scene whose metric variant
 * differs from the unit's is refused (RTGR_ERR_BAD_ARG), never traced with the wrong kernels.
 *   Optional third function: the FAR pass skips the scan of a step when no object's distance can change sign within the
 * step's reach; for a user object it needs a bound from the source,
 *     template <class S> __device__ S rtgr_user_reach(unsigned type, const S x[4], const S p[9], const S dl[4]);
 * = an upper bound of |distance(x') - distance(x)| over all x' with |x'_q - x_q| <= dl[q].  Without it ("rtgr_user_reach" does
 * not occur in the source) a user object is never provably out of reach and scenes of the unit run the single FULL pass
 * (every accepted step scanned, as the reference does): same results, the FAR pass's saving is lost.
 *   Optional fourth function — a SAMPLE OBJECT per type for the library's own checks:
 *     template <class S> __device__ bool rtgr_user_sample(unsigned type, S p[9]);
 * = true with p filled for an object of `type` about 0.5 across placed around (x, y, z) = (4, 0, 0) — where example2's small sphere
 * stands, in view of the probe's camera —, false for a type the source has none for.  With it the load-time probe (below) traces
 * the unit's OWN objects through its FULL and FAR + NEAR passes, so a distance / reach pair that disagrees on the samples keeps the
 * unit from loading at all; without it the probe's frame holds built-in objects only and a bad bound is left to the scene check.
 *   Whether or not a source brings samples: the FIRST trace of every scene that holds user objects with a reach bound runs
 * rtgr_scene_check's comparison by itself, on a coarse sample of that call's own rays (option "scene_check", default 1; a few
 * milliseconds once per (unit, object list, metric parameters, solver constants, camera), answered from a table afterwards; not
 * during hipGraph capture) — a reach function that is not an upper bound is refused with RTGR_ERR_BAD_ARG instead of losing hits.
 *   Scenes: obj[k].kind = RTGR_USER_OBJECT, .type, .p as the source expects; scene.user_metric = the unit's id.  Built-in
 * objects may stand beside user objects in any order (:518-530's order rule applies to all).  Limits: the tile kernel
 * (option tile = 1) and the packed Float32 kernel know no user objects — scenes of a unit take the pipeline's scalar kernels;
 * the redshift output treats a user object's emitter as the static observer (as for planes and disks).
 * rtgr_user_metric_compile(ctx, source, stationary, id) == rtgr_user_unit_compile(ctx, source, stationary, NULL, id).
 *   Environment: RTGR_UNIT_CACHE=<directory> (opt-in) keeps the code objects rtgr_user_unit_compile / rtgr_user_metric_compile build,
 * keyed by source text + what they are built for + the device headers; a later process with the same inputs loads the file (audited
 * and probed like any other) instead of compiling for seconds.  Within a process the same call again — same context, source,
 * `stationary` and metric variant — is answered at once with the id it gave before, for as long as that unit is resident. */
int rtgr_user_unit_compile(rtgr_context* ctx, const char* source, int stationary, const rtgr_scene* built_for, uint64_t* id_out);
/* ... the build step on its own (no GPU, no context): source -> code object file for rtgr_user_metric_load */
int rtgr_user_unit_build(const char* source, int stationary, const rtgr_scene* built_for, const char* code_object_path);
/* Objects of SEVERAL sources in one scene (the reference puts any mix of Object subtypes into `objs`; compiled code holds a scene's
 * objects in one unit): joins n object sources into ONE source text for rtgr_user_unit_compile / _build.  Source k, which defines
 * ntypes[k] object types (tags 0 .. ntypes[k]-1), is wrapped in a namespace of its own; the joined text's methods dispatch on the tag:
 * type t of source k is type ntypes[0] + ... + ntypes[k-1] + t of the joined text — the caller adds that base to obj[].type.  Where
 * some sources bring rtgr_user_reach and others do not, the joined bound is +infinity for the types of the latter: every
 * step of a scene that holds such an object is scanned (the NEAR pass), scenes without one keep the FAR pass's saving.  A metric's
 * source is not joined: put it before the joined text, as with one family.  Text in, text out — no GPU, no context.
 *   `out` may be NULL (then only *need, the length with its NUL, is written); a buffer shorter than *need is RTGR_ERR_BAD_ARG. */
int rtgr_user_source_join(const char* const* sources, const uint32_t* ntypes, int n, char* out, uint64_t cap, uint64_t* need);
/* What a resident unit was built for. */
typedef struct rtgr_unit_info {
    uint32_t metric;       /* rtgr_metric (| RTGR_METRIC_GENERIC) its kernels are instantiated for; RTGR_USER: its own */
    uint32_t spin;         /* built-in closed-form kernels: 1 = the a != 0 instantiation                               */
    uint32_t has_objects;  /* the source defined rtgr_user_distance / rtgr_user_objcolor                               */
    uint32_t has_reach;    /* ... and rtgr_user_reach: scenes with its objects run FAR + NEAR                          */
    uint32_t far_waves, near_waves, f32_waves; /* waves per SIMD its integrate passes were built for                  */
    uint32_t probe_ok;     /* 1: the load-time probe ran (FULL == FAR + NEAR, two schedules each); 0: skipped (unit_probe = 0) */
} rtgr_unit_info;
int rtgr_user_unit_info(rtgr_context* ctx, uint64_t id, rtgr_unit_info* info);
/* The library's central schedule-invariance property, as a check a caller can run on ITS scene: the FAR + NEAR passes skip the
 * ContinuousCallback scan of a step only where no object's distance can change sign, so they must deliver the frame of the single
 * FULL pass (every accepted step scanned, as the reference does, src/RayTraceGR.jl:488-490).  For built-in objects the bound is the
 * library's; for user objects it is the source's rtgr_user_reach — and a reach function that is NOT an upper bound loses hits
 * silently.  This traces the camera's canvas at ni x nj rays (<= 256 x 256; a coarse canvas of the same camera is the usual call)
 * through both pass structures on device 0 of the context and compares: bit for bit for a built-in metric (with or without user
 * objects), within the load-time probe's bars for a metric given as source.  RTGR_OK, or RTGR_ERR_BAD_ARG with the count of rays
 * that differ in rtgr_last_error().  Blocking; a few milliseconds.  is_f32 must be 0 (Float32 runs one pass structure only). */
int rtgr_scene_check(rtgr_context* ctx, const rtgr_scene* scene, const rtgr_solver* opt, const rtgr_camera* cam, uint64_t ni, uint64_t nj, int is_f32);
/* The EXEC-flip check.  ROCm 7.2's compiler can place a register copy or spill at the top of the FLOW block of a divergent if / else,
 * AHEAD of the instruction that switches EXEC to the `else` lanes; code of that shape computes wrong values in some lanes (DESIGN.md
 * §4.6: the Float64 FULL pass of a heavy metric was wrong from it in round 4).  rtgr_user_metric_compile / _build look for the shape
 * in the listing and rewrite it there (as raytracegr.jl_amd/user_metric.py does on the hipcc route); rtgr_user_metric_load AUDITS
 * every code object it is handed — whatever built it — and refuses one that carries the shape with RTGR_ERR_BAD_ARG and the offending
 * instructions in rtgr_last_error().  rtgr_code_object_audit is that audit on its own (no GPU, no context needed): *found = number
 * of such blocks, their description in `report` (may be NULL).  The file is a gfx950 code object, or a host library that embeds
 * code objects — librtgr_hip.so itself: the build checks audit the kernels the library ships.  RTGR_ERR_BAD_ARG when it is neither,
 * or the disassembler (libamd_comgr) is not on the box. */
int rtgr_code_object_audit(const char* code_object_path, int* found, char* report, uint64_t report_len);
/* … and the check / repair of a gfx950 assembly LISTING (`hipcc -S`), the step rtgr_user_metric_build runs between code generation and
 * the assembler: repaired_path == NULL: *blocks = FLOW blocks that carry the shape; otherwise the listing is rewritten into
 * repaired_path and *blocks = blocks rewritten (RTGR_ERR_BAD_ARG, nothing written, when a block is not of the form the rewrite is
 * proven for).  The same rule as raytracegr.jl_amd/isa_exec.py; the tests hold the two to the same answers. */
int rtgr_listing_repair(const char* listing_path, const char* repaired_path, int* blocks);
/* Every unit that rtgr_user_metric_load / _compile / rtgr_user_unit_compile brings in is checked THREE ways before a scene can use
 * it: (1) ABI version and — when the builder recorded it — a hash of the device headers it was compiled against, which must be the
 * one the library's own kernels were built from (the record layouts the kernels share are not part of this header and move
 * without the ABI version moving); (2) the audit above, on bare code objects and on clang offload bundles alike; an image the
 * audit cannot read is refused, a box without the disassembler loads unaudited; (3) a PROBE: the unit traces a fixed 32 x 32 frame
 * through its single FULL pass and through its FAR + NEAR passes, each under TWO schedules (sixteen waves with one ray per lane;
 * three waves whose lanes refill from the queue — a ray's bits never depend on the schedule), the Float32 FULL pass likewise, and
 * is refused (RTGR_ERR_BAD_ARG, nothing left resident) when the two schedules of one structure differ in any bit or the structures
 * disagree — the symptoms of a mis-compiled unit, whatever the instruction shape (~10-130 ms). */
/* 1 if module `id` is resident (id 0: any module), else 0 */
int rtgr_user_metric_loaded(rtgr_context* ctx, uint64_t id);

/* ---- image output: N0f8 quantisation + transposed PNG layout of `save(file, colorview(...))` (:566-575) ---- */
/* rgb planes (n = ni*nj, device pointer) -> 8-bit interleaved image[j][i][c] (device pointer, 3*n bytes). */
int rtgr_quantize_device_f64(rtgr_context* ctx, const double* d_rgb, uint64_t ni, uint64_t nj, uint8_t* d_img, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RTGR_H */
