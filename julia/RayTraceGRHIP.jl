# RayTraceGRHIP.jl — the reference-side binding a RayTraceGR.jl maintainer would add to route the hot path
# (`trace_rays`, src/RayTraceGR.jl:482-536) through librtgr_hip.so (include/rtgr.h, ABI version 4).
#
# NOT EXECUTED IN THIS REPOSITORY: the build image has no Julia.  What stands in for running it:
#   * tests/c/abi_layout.c — a compiled C caller that passes the same bytes this file would (structs by pointer, an
#     88-byte Pixel array) and whose _Static_asserts pin the table below; tests/test_abi.py runs it on the CPU (layout,
#     symbols) and on the GPU (example2() == sphere2.png through rtgr_trace_pixels_f64 + rtgr_trace_one_f64; a
#     KerrSchild(1, 0.998) + Disk frame through rtgr_trace_f64 with per-ray outputs, against the oracle);
#   * raytracegr.jl_amd/api.py — the same calls through Python ctypes, which every GPU test uses;
#   * tests/test_julia_stub.py — every `ccall` below against the prototypes of include/rtgr.h (symbol declared and exported,
#     as many argument types and arguments as C parameters, pointer / Cint / UInt64 kinds, return type), the structs' field
#     order and the enum constants against the header's, the block structure of this file and of julia/runtests_hip.jl, and
#     that every name runtests_hip.jl uses is defined here.
#   * julia/runtests_hip.jl — the reference's test/runtests.jl:12-79 (incl. the commented-out "rays" test) restated over
#     this module, plus example1() / example2() against the committed goldens: what a maintainer runs first.
#
# fieldoffset table (bytes; Julia lays isbits structs out by the C rules, so `fieldoffset(T, i)` must print exactly this —
# a maintainer can check with `[(fieldname(T,i), fieldoffset(T,i)) for i in 1:fieldcount(T)]`; runtests_hip.jl does):
#
#   RtgrObject       80   kind 0, type 4, p 8
#   RtgrScene      1320   metric 0, nobj 4, M 8, a 16, user_metric 24, obj 32, objects 1312
#   RtgrSolver       72   reltol 0, abstol 8, lambda0 16, lambda1 24, hit_threshold 32, miss_rgb 40, max_steps 64, interp_points 68
#   RtgrCamera      128   pos 0, widthx 32, widthy 64, normal 96
#   RtgrCounters     64   rays 0, accepted 8, rejected 16, rhs_evals 24, events 32, events_interior 40, not_finished 48, reserved 56
#   RtgrRayOutputs   64   state_end 0, lambda_end 8, status 16, hit 24, n_accept 32, n_reject 40, redshift 48, hit32 56
#   RtgrGrid         64   n 0, pad 12, origin 16, spacing 40
#   RtgrGrid4        80   n 0, origin 16, spacing 48
#   RtgrAA           24   k 0, flags 4, contrast 8, max_batch_rays 16
#   RtgrAAStats      32   pixels 0, refined 8, sub_rays 16, batches 24
#   RtgrTextureDesc  16   width 0, height 4, flags 8, pad 12
#   RtgrTextureBind  16   object 0, filter 4, texture 8
#   RtgrShade        24   nbind 0, flags 4, bind 8, r_escape 16
#   RtgrDiskEmission 96   object 0, emitter 4, flags 8, pad 12, orbit 16, T_in 24, p 32, gain 40, theta 48, weight 72
#   RtgrObserver    176   pos 0, vel 32, look 64, up 96, fov_x 128, fov_y 136, orbit 144, kind 152, projection 156, flags 160, pad 164, max_batch_rays 168
#   RtgrHotSpot      80   rho_s 0, phi0 8, sigma 16, cut 24, amp 32, g_power 40, t_start 48, dt 56, nt 64, flags 72, pad 76
#   RtgrSpectrum     80   kind 0, flags 4, nb 8, lo 16, hi 24, amp 32, alpha 40, rho_min 48, rho_max 56, g_power 64, reserved 72
#   RtgrPolarization 64   kind 0, flags 4, deg0 8, deg1 16, field 24, reserved 48
#   RtgrDiskOrders 32   max_order 0, flags 4, margin 8, transmission 16, pad 24
#   RtgrOrderPlanes 48   count 0, hit32 8, state_end 16, g 24, rgb_order 32, state0 40
#   RtgrFlow        104   emitter 0, flags 4, orbit 8, j0 16, kappa 24, r0 32, alpha 40, H 48, s 56, r_stop 64, gain 72, weight 80
#   Pixel{Float64}   88   pos 0, normal 32, rgb 64         (the reference's own type, src/RayTraceGR.jl:446-450)
#   Pixel{Float32}   44   pos 0, normal 16, rgb 32
#
# It is a thin `ccall` layer; host code stays Julia, the metric/object/Pixel signatures of the reference are preserved,
# and anything that cannot cross the C ABI (an arbitrary metric callable, an Object subtype without device source, a scalar
# type other than Float64 / Float32) falls back to the reference's own CPU path — never silently: every such return goes
# through `cpu_fallback`, which emits one `@warn` naming the reason (a 3 ms frame and a 10 s one must not look alike).
#
# Every BASELINE.json configuration from Julia (INTEGRATION.md "Julia" has them spelled out):
#   C1  example1()                                                      minkowski, 200², == scenes/sphere.png
#   C2  example2(ni = 1024, nj = 1024, metric = KerrSchild(1.0, 0.8))   Kerr–Schild a = 0.8, 3 objects
#   C3  render(kerr_schild, objs, cam..., 4096, 4096; ctx = Context(0:7))   rows dealt to 8 GPUs, RGB planes back
#   C4  example2(T = Float32, ni = 2048, nj = 2048, metric = KerrSchild(1.0, 0.8))
#   C5  example_disk(ni = 8192, nj = 8192)                              KerrSchild(1, 0.998) + Disk(0.05, 2, 4)
module RayTraceGRHIP

using RayTraceGR
using StaticArrays

const librtgr = get(ENV, "RTGR_LIB", "librtgr_hip.so")
const RTGR_MAX_OBJECTS = 16      # objects held inline in RtgrScene.obj; a longer `objs` goes through RtgrScene.objects (any length)
const Ctx = Ptr{Cvoid}          # rtgr_context*; C_NULL = the process's default context
const D = RayTraceGR.D          # 4 (src/RayTraceGR.jl:253-254)

# ---- PODs of include/rtgr.h ------------------------------------------------------------------------------------------
struct RtgrObject
    kind::UInt32
    type::UInt32                # RTGR_USER_OBJECT: the tag handed to the unit's rtgr_user_distance / rtgr_user_objcolor
    p::NTuple{9,Float64}
end
struct RtgrScene
    metric::UInt32
    nobj::UInt32
    M::Float64
    a::Float64
    user_metric::UInt64
    obj::NTuple{RTGR_MAX_OBJECTS,RtgrObject}
    objects::Ptr{RtgrObject}    # C_NULL: the list is obj[1:nobj]; otherwise the WHOLE list, nobj objects — `objs` of any length (:433-441)
end
struct RtgrSolver
    reltol::Float64
    abstol::Float64
    lambda0::Float64
    lambda1::Float64
    hit_threshold::Float64
    miss_rgb::NTuple{3,Float64}
    max_steps::UInt32
    interp_points::UInt32
end
struct RtgrCamera
    pos::NTuple{4,Float64}
    widthx::NTuple{4,Float64}
    widthy::NTuple{4,Float64}
    normal::NTuple{4,Float64}
end
struct RtgrCounters
    rays::UInt64; accepted::UInt64; rejected::UInt64; rhs_evals::UInt64
    events::UInt64; events_interior::UInt64; not_finished::UInt64; reserved::UInt64
end
struct RtgrGrid                # a metric sampled on a uniform grid (rtgr_grid_metric_load)
    n::NTuple{3,UInt32}         # samples along x, y, z; each >= 4
    pad::UInt32
    origin::NTuple{3,Float64}   # (x, y, z) of sample (0, 0, 0)
    spacing::NTuple{3,Float64}
end
struct RtgrGrid4               # a time-dependent metric sampled on a uniform 4-D grid (rtgr_grid4_metric_load)
    n::NTuple{4,UInt32}         # samples along t, x, y, z; each >= 4
    origin::NTuple{4,Float64}   # (t, x, y, z) of sample (0, 0, 0, 0)
    spacing::NTuple{4,Float64}
end
struct RtgrAA                  # adaptive anti-aliasing (rtgr_trace_aa_f64 / _f32): k x k sub-rays for the pixels on an edge
    k::UInt32                   # 2..8
    flags::UInt32               # 0
    contrast::Float64           # refine where a colour channel differs from a 4-neighbour's by more than this; < 0: every pixel; Inf: class edges only
    max_batch_rays::UInt64      # sub-rays per batch at most; 0 = default
end
struct RtgrAAStats
    pixels::UInt64; refined::UInt64; sub_rays::UInt64; batches::UInt64
end
struct RtgrTextureDesc         # an image texture (rtgr_texture_load): three planes of height x width doubles, column fastest
    width::UInt32               # 2 .. 16384
    height::UInt32
    flags::UInt32               # 0
    pad::UInt32                 # 0
end
struct RtgrTextureBind         # one texture bound to one object of the list — or to the rays that escape
    object::UInt32              # 1-based index in `objs` (what `hit` holds); 0 = rays that escape
    filter::UInt32              # RTGR_TEX_NEAREST / RTGR_TEX_BILINEAR
    texture::UInt64             # id from load_texture
end
struct RtgrShade               # the binds of a shaded frame (rtgr_trace_shaded_f64 / _f32)
    nbind::UInt32               # 0 .. 16
    flags::UInt32               # 0
    bind::Ptr{RtgrTextureBind}
    r_escape::Float64           # a miss counts as escaped when the Euclidean |x_end| >= r_escape
end
struct RtgrDiskEmission        # an orbiting disk that glows as a black body (rtgr_trace_emission_f64 / _f32)
    object::UInt32              # 1-based index of a Disk in `objs`
    emitter::UInt32             # RTGR_EMIT_KEPLER / RTGR_EMIT_RIGID
    flags::UInt32               # 0 | RTGR_EMIT_INNER_EDGE
    pad::UInt32                 # 0
    orbit::Float64              # KEPLER: +1 = Omega_+ (counter-clockwise seen from +z), -1 = Omega_-; RIGID: Omega itself
    T_in::Float64               # T_em(rho) = T_in (rho / r_in)^(-p)
    p::Float64
    gain::Float64
    theta::NTuple{3,Float64}    # h c / (lambda_c k_B) per channel
    weight::NTuple{3,Float64}
end
struct RtgrObserver            # a pinhole camera carried by an observer (rtgr_trace_observer_f64 / _f32)
    pos::NTuple{4,Float64}      # the event the observer is at
    vel::NTuple{4,Float64}      # RTGR_OBS_VELOCITY: coordinate 4-velocity, any normalisation
    look::NTuple{4,Float64}     # coordinate vectors; only their parts orthogonal to the 4-velocity matter
    up::NTuple{4,Float64}
    fov_x::Float64              # radians
    fov_y::Float64
    orbit::Float64              # RTGR_OBS_CIRCULAR: +1 = Omega_+ (counter-clockwise seen from +z), -1 = Omega_-
    kind::UInt32                # RTGR_OBS_STATIC / RTGR_OBS_VELOCITY / RTGR_OBS_CIRCULAR
    projection::UInt32          # RTGR_PROJ_PERSPECTIVE / RTGR_PROJ_EQUIRECT
    flags::UInt32               # 0
    pad::UInt32                 # 0
    max_batch_rays::UInt64      # rays per batch at most; 0 = default
end
struct RtgrHotSpot             # a rigid Gaussian spot riding in the emitting disk, and its observer times (rtgr_trace_light_curve_f64 / _f32)
    rho_s::Float64              # cylindrical radius of the centre, plane z = 0
    phi0::Float64               # azimuth of the centre at coordinate time 0
    sigma::Float64              # Gaussian width
    cut::Float64                # support in units of sigma
    amp::Float64                # emissivity at the centre
    g_power::Float64            # q of the weight g^q
    t_start::Float64            # tau_k = t_start + k dt
    dt::Float64
    nt::UInt64                  # 1 .. 2^20
    flags::UInt32               # 0
    pad::UInt32                 # 0
end
struct RtgrSpectrum            # a line profile or a thermal spectrum of the emitting disk (rtgr_trace_spectrum_f64 / _f32)
    kind::UInt32                # RTGR_SPEC_LINE / RTGR_SPEC_THERMAL
    flags::UInt32               # 0 | RTGR_SPEC_LOG | RTGR_SPEC_NU3 (thermal only)
    nb::UInt64                  # bins (line) or sample frequencies (thermal): 1 .. 2^16
    lo::Float64                 # line: the bins cover [lo, hi) of g; thermal: theta_0 = lo, theta_(nb-1) = hi
    hi::Float64
    amp::Float64                # line: emissivity at rho_min
    alpha::Float64              # line: (rho / rho_min)^(-alpha)
    rho_min::Float64            # line: the window rho_min <= rho < rho_max
    rho_max::Float64
    g_power::Float64            # line: q of the weight g^q
    reserved::Float64           # 0
end
struct RtgrPolarization        # the emission law of a polarized disk image (rtgr_trace_polarized_f64 / _f32)
    kind::UInt32                # RTGR_POL_SCATTER / RTGR_POL_FIELD
    flags::UInt32               # 0
    deg0::Float64               # degree scale, >= 0
    deg1::Float64               # SCATTER: delta = deg0 (1 - mu) / (1 + deg1 mu), > -1
    field::NTuple{3,Float64}    # FIELD: B_rho, B_phi, B_z in the emitter's triad; SCATTER: 0
    reserved::NTuple{2,Float64} # 0
end
struct RtgrDiskOrders          # how far rays are followed through the emitting disk (rtgr_trace_orders_f64 / _f32)
    max_order::UInt32           # N: orders 1 .. N are looked for, 1 .. 8
    flags::UInt32               # 0
    margin::Float64             # eta; 0: half the disk's half thickness
    transmission::Float64       # T in [0, 1]
    pad::UInt64                 # 0
end
struct RtgrOrderPlanes         # the optional outputs of rtgr_trace_orders_*; C_NULL = not wanted
    count::Ptr{UInt8}           # n
    hit32::Ptr{UInt32}          # (N + 1) x n
    state_end::Ptr{Cvoid}       # (N + 1) x n x 8
    g::Ptr{Cvoid}               # (N + 1) x n
    rgb_order::Ptr{Cvoid}       # (N + 1) x 3 x n
    state0::Ptr{Cvoid}          # n x 8
end
struct RtgrFlow                # a hot, rotating flow that emits and absorbs along each ray (rtgr_trace_transfer_f64 / _f32)
    emitter::UInt32             # RTGR_EMIT_KEPLER / RTGR_EMIT_RIGID
    flags::UInt32               # 0
    orbit::Float64              # KEPLER: +1 / -1; RIGID: Omega
    j0::Float64                 # emissivity scale, >= 0
    kappa::Float64              # grey absorption, >= 0 (0: optically thin)
    r0::Float64                 # density (r / r0)^(-alpha) exp(-z^2 / (2 H^2 rho^2)); r0 > 0
    alpha::Float64
    H::Float64                  # > 0
    s::Float64                  # j_nu ~ nu^(-s)
    r_stop::Float64             # >= 0: a ray's integration ends once it is inside this radius
    gain::Float64
    weight::NTuple{3,Float64}   # rgb_c = rgb_c exp(-tau) + gain weight_c I
end
struct RtgrRayOutputs          # optional per-ray outputs; C_NULL = not wanted
    state_end::Ptr{Cvoid}
    lambda_end::Ptr{Cvoid}
    status::Ptr{UInt8}
    hit::Ptr{UInt8}
    n_accept::Ptr{UInt32}
    n_reject::Ptr{UInt32}
    redshift::Ptr{Cvoid}
    hit32::Ptr{UInt32}          # omin as 32 bits: object lists beyond 255
end

# enum rtgr_metric / rtgr_object_kind / rtgr_ray_status of the header (tests/test_julia_stub.py compares the values)
const RTGR_MINKOWSKI = UInt32(0)
const RTGR_KS_REF = UInt32(1)
const RTGR_KS_TRUE = UInt32(2)
const RTGR_USER = UInt32(3)
const RTGR_GRID = UInt32(4)
const RTGR_METRIC_GENERIC = UInt32(0x100)
const RTGR_PLANE = UInt32(1)
const RTGR_SPHERE = UInt32(2)
const RTGR_DISK = UInt32(3)
const RTGR_USER_OBJECT = UInt32(4)
const RTGR_RAY_EVENT = UInt8(0)
const RTGR_RAY_LAMBDA1 = UInt8(1)
const RTGR_RAY_MAXSTEPS = UInt8(2)
const RTGR_RAY_DTMIN = UInt8(3)
const RTGR_RAY_NAN = UInt8(4)
const RTGR_RAY_OUTSIDE = UInt8(5)
const RTGR_TEX_NEAREST = UInt32(0)
const RTGR_TEX_BILINEAR = UInt32(1)
const RTGR_EMIT_KEPLER = UInt32(0)
const RTGR_EMIT_RIGID = UInt32(1)
const RTGR_EMIT_INNER_EDGE = UInt32(1)
const RTGR_OBS_STATIC = UInt32(0)
const RTGR_OBS_VELOCITY = UInt32(1)
const RTGR_OBS_CIRCULAR = UInt32(2)
const RTGR_PROJ_PERSPECTIVE = UInt32(0)
const RTGR_PROJ_EQUIRECT = UInt32(1)
const RTGR_SPEC_LINE = UInt32(0)
const RTGR_SPEC_THERMAL = UInt32(1)
const RTGR_SPEC_LOG = UInt32(1)
const RTGR_SPEC_NU3 = UInt32(2)
const RTGR_POL_SCATTER = UInt32(0)
const RTGR_POL_FIELD = UInt32(1)

function check(rc)
    rc < 0 && error("librtgr_hip: ", unsafe_string(ccall((:rtgr_last_error, librtgr), Cstring, ())))
    rc
end

"""
    cpu_fallback(what, why)

Every place where a legal call of the reference cannot cross the C ABI and is handed to the reference's own CPU path goes through
here: ONE `@warn` per distinct (entry point, reason) — the CPU path is ~3000 x slower than the device (profiles/r05/cpu_baseline_1024.json),
and a first user must be able to tell the two apart by something better than the clock.  `ENV["RTGR_QUIET_FALLBACK"] = "1"` silences it.
"""
function cpu_fallback(what::AbstractString, why::AbstractString)
    get(ENV, "RTGR_QUIET_FALLBACK", "0") == "1" ||
        @warn "RayTraceGRHIP.$what: $why — running the reference's CPU path (RayTraceGR.$what), not the GPU" maxlog = 1 _id = Symbol(what, hash(why))
    nothing
end

# ---- new scene vocabulary (SURVEY §8 f4): what BASELINE configs 2, 4 and 5 need and the reference does not have -------
"""
    KerrSchild(M, a; textbook = true, generic = false)

The parameterised Kerr–Schild metric the reference's `kerr_schild` hard-wires to `M = 1`, `a = 0  # T(0.8)`
(src/RayTraceGR.jl:275-276).  A callable like every metric of the reference — `KerrSchild(1.0, 0.8)(x)` is the 4x4 `g_ab`
in plain Julia, accepts `Dual`s, works with `RayTraceGR.dmetric / christoffel / make_canvas / trace_rays` on the CPU — and
the C ABI carries it as an enum plus `(M, a)`:
`textbook = true`  → `RTGR_KS_TRUE`, the radius `r² = (q + sqrt(q² + 4a²z²))/2`, `q = ρ² − a²` (a true Kerr black hole);
`textbook = false` → `RTGR_KS_REF`, the radius exactly as written at :284 (not a solution of the field equations for a ≠ 0;
identical for a = 0).  `generic = true` traces with the reference's own formulation of the RHS (4-wide duals, 4x4 inverse,
Christoffel contraction) instead of the closed Kerr–Schild contraction: same results to rounding, ~2.6 x the time.
"""
struct KerrSchild
    M::Float64
    a::Float64
    textbook::Bool
    generic::Bool
end
KerrSchild(M::Real = 1.0, a::Real = 0.0; textbook::Bool = true, generic::Bool = false) =
    KerrSchild(Float64(M), Float64(a), textbook, generic)

basereal(::Type{T}) where {T<:AbstractFloat} = T
basereal(::Type{RayTraceGR.Dual{T,DT}}) where {T,DT} = T             # the reference's Dual mixes with its OWN scalar type only (:55-121)
function (m::KerrSchild)(xx::SVector{4,T}) where {T}             # src/RayTraceGR.jl:274-294 with (M, a) as parameters
    M, a = basereal(T)(m.M), basereal(T)(m.a)
    t, x, y, z = xx
    @assert !any(isnan, (t, x, y, z))                             # :279
    η = @SMatrix T[p == q ? (p == 1 ? -1 : 1) : 0 for p in 1:4, q in 1:4]
    ρ2 = x^2 + y^2 + z^2
    if m.textbook
        q = ρ2 - a^2
        r = sqrt((q + sqrt(q^2 + 4 * a^2 * z^2)) / 2)
    else
        r = sqrt(ρ2 - a^2) / 2 + sqrt(a^2 * z^2 + ((ρ2 - a^2) / 2)^2)   # :284 as written
    end
    f = 2 * M * r^3 / (r^4 + a^2 * z^2)                           # :285
    k = SVector{4,T}(1, (r * x + a * y) / (r^2 + a^2), (r * y - a * x) / (r^2 + a^2), z / r)   # :286-289
    @SMatrix T[η[p, q] + f * k[p] * k[q] for p in 1:4, q in 1:4]   # :291
end

"""
    Disk{T}(half_thickness, r_in, r_out) <: RayTraceGR.Object{T}

Thin accretion disk `|z| <= h`, `r_in <= sqrt(x² + y²) <= r_out` in the equatorial plane (BASELINE config 5; no reference
counterpart).  Obeys the reference's distance contract (:377-383: zero on the surface, positive outside, negative inside),
so the reference's CPU `trace_rays` handles it too through the two methods below; `RTGR_DISK` across the ABI.
"""
struct Disk{T} <: RayTraceGR.Object{T}
    half_thickness::T
    r_in::T
    r_out::T
end
function RayTraceGR.distance(d::Disk{T}, pos::SVector{4,T})::T where {T}
    ϱ = sqrt(pos[2]^2 + pos[3]^2)
    max(abs(pos[4]) - d.half_thickness, d.r_in - ϱ, ϱ - d.r_out)
end
function RayTraceGR.objcolor(d::Disk{T}, pos::SVector{4,T})::SVector{3,T} where {T}   # checkerboard in (radius, azimuth)
    ϱ = sqrt(pos[2]^2 + pos[3]^2)
    ϕ = atan(pos[3], pos[2])
    SVector{3,T}(1, mod(ϱ, 1), mod(12 * ϕ / π, 1))
end

# the objects' own parameters stay Float64 across the ABI (rtgr_object.p); T selects the arithmetic of the path
pack(pl::RayTraceGR.Plane) = RtgrObject(RTGR_PLANE, 0, (Float64(pl.time), 0, 0, 0, 0, 0, 0, 0, 0))
pack(s::RayTraceGR.Sphere) = RtgrObject(RTGR_SPHERE, 0, (Float64.(s.pos)..., Float64.(s.vel)..., Float64(s.radius)))
pack(d::Disk) = RtgrObject(RTGR_DISK, 0, (Float64(d.half_thickness), Float64(d.r_in), Float64(d.r_out), 0, 0, 0, 0, 0, 0))
"""
    DeviceObjects(source)                       a family of NEW Object subtypes, given as device source
    DeviceObject{T}(family, type, fields...)    one object of it: `<: RayTraceGR.Object{T}`, goes into `objs` like a Sphere

The reference's `Object{T}` is an open abstract type (src/RayTraceGR.jl:374-389): a new subtype brings `distance(obj, pos)` and
`objcolor(obj, pos)`.  A Julia method cannot cross the C ABI; the native counterpart is the same two methods as C++ source,

    template <class S> __device__ S    rtgr_user_distance(unsigned type, const S x[4], const S p[9]);
    template <class S> __device__ void rtgr_user_objcolor(unsigned type, const S x[4], const S p[9], S rgb[3]);

(optionally `rtgr_user_reach`: include/rtgr.h "user objects"), compiled at run time — together with the metric the objects are
traced with — into the scene's unit (`rtgr_user_unit_compile`: one ccall, built in-process, no hipcc).  `type` tells the family's
object types apart inside the source, `fields` (up to 9 numbers) are the object's parameters `p`.  DeviceObjects of SEVERAL families
may stand in one `objs` vector when each family says how many types its source defines (`DeviceObjects(source, ntypes = 2)`): their
sources are joined into one (`rtgr_user_source_join`: a namespace per family, type tags renumbered family after family in the order
of first appearance).  An object type WITHOUT device source still takes the reference's CPU path, as before.
"""
struct DeviceObjects
    source::String
    ntypes::UInt32          # how many object types the source defines (0: not stated — enough as long as a scene uses one family)
end
DeviceObjects(source::AbstractString; ntypes::Integer = 0) = DeviceObjects(String(source), UInt32(ntypes))
struct DeviceObject{T} <: RayTraceGR.Object{T}
    family::DeviceObjects
    type::UInt32
    p::NTuple{9,Float64}
end
function DeviceObject{T}(family::DeviceObjects, type::Integer, fields::Real...) where {T}
    length(fields) <= 9 || error("an object has at most 9 scalar fields (rtgr_object.p)")
    DeviceObject{T}(family, UInt32(type), ntuple(i -> i <= length(fields) ? Float64(fields[i]) : 0.0, 9))
end
# (the two methods exist on the device only: the reference's CPU trace_rays cannot evaluate them — say so instead of a MethodError)
RayTraceGR.distance(o::DeviceObject{T}, pos::SVector{4,T}) where {T} =
    error("a DeviceObject carries device source only; give the type Julia methods `distance` / `objcolor` to trace it on the CPU")
RayTraceGR.objcolor(o::DeviceObject{T}, pos::SVector{4,T}) where {T} =
    error("a DeviceObject carries device source only; give the type Julia methods `distance` / `objcolor` to trace it on the CPU")
pack(o::DeviceObject) = RtgrObject(RTGR_USER_OBJECT, o.type, o.p)
pack(o::RayTraceGR.Object) = nothing            # an object type without device source: the CPU path handles it
const NOOBJ = RtgrObject(0, 0, ntuple(_ -> 0.0, 9))

"""
    Context(device_ids) / close(ctx)

All devices one Julia process drives (`rtgr_create`).  `trace_rays(...; ctx)` on a context with several devices deals the
canvas rows cyclically to ALL of them inside the one `ccall` (`rtgr_trace_pixels_f64/_f32`: device k of N takes rows
k, k+N, …, uploads those rows of `c.pixels` over its own PCIe link and writes them straight back into the output array —
nothing is routed through the first device; include/rtgr.h "the hot path, host buffers") — no Distributed.jl, which the
reference tried and abandoned (README.md:129-135).  Without a context the library's default one (ONE device) is used.
Exercised in this repository by the C caller (`tests/c/abi_layout.c --render … 3`) and `tests/test_gpu_context.py`
with a context that lists the GPU several times; between physically different GPUs it has not run yet (no node).
"""
mutable struct Context
    handle::Ctx
    function Context(device_ids::AbstractVector{<:Integer} = Int[])
        h = Ref{Ctx}(C_NULL)
        ids = collect(Cint, device_ids)
        check(ccall((:rtgr_create, librtgr), Cint, (Ptr{Cint}, Cint, Ptr{Ctx}), isempty(ids) ? C_NULL : ids, length(ids), h))
        finalizer(close, new(h[]))
    end
end
function Base.close(c::Context)     # idempotent; also the finalizer
    c.handle == C_NULL && return nothing
    ccall((:rtgr_destroy, librtgr), Cint, (Ctx,), c.handle)
    c.handle = C_NULL
    nothing
end
handle(::Nothing) = C_NULL
handle(c::Context) = c.handle
ndevices(ctx) = Int(check(ccall((:rtgr_context_devices, librtgr), Cint, (Ctx,), handle(ctx))))

"""
    DeviceMetric(code_object; M = 1.0, a = 0.0)

A metric function of the user's own — the native stand-in for passing a new Julia function as `metric` (:302-309) —
given as C++ source text (`DeviceMetric(source = "...")`: built in-process by `rtgr_user_metric_compile`, no hipcc needed) or
as a gfx950 code object built from `rtgr_user_unit.hip.in` (INTEGRATION.md "A new metric").
Several may be resident at once; a scene names its own by id.
"""
struct DeviceMetric
    code_object::String     # path of a code object (rtgr_user_metric_build, or `python -m raytracegr.jl_amd.user_metric`), or "" when `source` is given
    source::String          # C++ source of rtgr_user_metric<S>: built in-process by the library, one ccall
    stationary::Bool
    M::Float64
    a::Float64
end
DeviceMetric(path::AbstractString; M = 1.0, a = 0.0) = DeviceMetric(path, "", false, M, a)
DeviceMetric(; source::AbstractString, stationary = false, M = 1.0, a = 0.0) = DeviceMetric("", source, stationary, M, a)
"""
    build_metric(source, path; stationary = false) -> DeviceMetric(path)

The build step of `DeviceMetric(source = ...)` on its own (`rtgr_user_metric_build`): source text -> code object file, built by the
library in-process — no GPU, no hipcc needed —, to be kept and loaded in later sessions with `DeviceMetric(path)`.
"""
function build_metric(source::AbstractString, path::AbstractString; stationary = false, M = 1.0, a = 0.0)
    check(ccall((:rtgr_user_metric_build, librtgr), Cint, (Cstring, Cint, Cstring), source, stationary, path))
    DeviceMetric(path, "", stationary, M, a)
end

function module_id(m::DeviceMetric, ctx)
    id = Ref{UInt64}(0)
    if isempty(m.source)
        check(ccall((:rtgr_user_metric_load, librtgr), Cint, (Ctx, Cstring, Ptr{UInt64}), handle(ctx), m.code_object, id))
    else
        check(ccall((:rtgr_user_metric_compile, librtgr), Cint, (Ctx, Cstring, Cint, Ptr{UInt64}),
                    handle(ctx), m.source, m.stationary, id))
    end
    id[]
end

"""
    GridMetric(g, origin, spacing)

A metric given as SAMPLES on a uniform grid — a numerically computed spacetime (include/rtgr.h "metrics sampled on a grid"):
stationary, `g` is a 10 x nx x ny x nz Array{Float64} (the upper triangle tt tx ty tz xx xy xz yy yz zz first, then x fastest — the
C layout, column-major), `origin` and `spacing` 3-tuples (x, y, z); time-dependent, `g` is 10 x nx x ny x nz x nt (time slowest) and
`origin` / `spacing` are 4-tuples (t, x, y, z).  Uploaded to the context on first use (`rtgr_grid_metric_load` /
`rtgr_grid4_metric_load`); rays that leave the grid's valid box — in t too — end with status RTGR_RAY_OUTSIDE.  `unload(m, ctx)`
releases the id (`rtgr_grid_metric_unload`).
"""
struct GridMetric{N,A}         # N = 4: stationary (3 axes), N = 5: time-dependent (A = 4 axes)
    g::Array{Float64,N}
    origin::NTuple{A,Float64}
    spacing::NTuple{A,Float64}
    ids::Dict{Ptr{Cvoid},UInt64}
end
function GridMetric(g::AbstractArray{<:Real,5}, origin, spacing)
    size(g, 1) == 10 || error("GridMetric: g must be 10 x nx x ny x nz x nt")
    all(size(g)[2:5] .>= 4) || error("GridMetric: at least 4 samples per axis")
    length(origin) == 4 && length(spacing) == 4 || error("GridMetric: a 4-D grid takes (t, x, y, z) origin and spacing")
    length(g) <= 10 * (1 << 28) || error("GridMetric: more than RTGR_GRID_MAX_SAMPLES (2^28) samples")
    all(v -> v - v == 0, g) || error("GridMetric: non-finite sample")
    all(h -> h > 0, spacing) || error("GridMetric: spacing must be > 0")
    GridMetric(Array{Float64,5}(g), Tuple(Float64.(origin)), Tuple(Float64.(spacing)), Dict{Ptr{Cvoid},UInt64}())
end
function GridMetric(g::AbstractArray{<:Real,4}, origin, spacing)
    size(g, 1) == 10 || error("GridMetric: g must be 10 x nx x ny x nz")
    all(size(g)[2:4] .>= 4) || error("GridMetric: at least 4 samples per axis")
    all(v -> v - v == 0, g) || error("GridMetric: non-finite sample")   # (v - v is NaN for Inf and NaN)
    all(h -> h > 0, spacing) || error("GridMetric: spacing must be > 0")
    GridMetric(Array{Float64,4}(g), Tuple(Float64.(origin)), Tuple(Float64.(spacing)), Dict{Ptr{Cvoid},UInt64}())
end
function module_id(m::GridMetric, ctx)
    id = Ref{UInt64}(get(m.ids, handle(ctx), UInt64(0)))
    if id[] == 0   # first use in this context (or unloaded since): upload
        if length(m.origin) == 4   # time-dependent: n = (nt, nx, ny, nz), the time axis is the array's last
            desc4 = Ref(RtgrGrid4(UInt32.((size(m.g, 5), size(m.g, 2), size(m.g, 3), size(m.g, 4))), m.origin, m.spacing))
            check(ccall((:rtgr_grid4_metric_load, librtgr), Cint, (Ctx, Ptr{RtgrGrid4}, Ptr{Float64}, Ptr{UInt64}), handle(ctx), desc4, m.g, id))
        else
            desc = Ref(RtgrGrid(UInt32.(size(m.g)[2:4]), UInt32(0), m.origin, m.spacing))
            check(ccall((:rtgr_grid_metric_load, librtgr), Cint, (Ctx, Ptr{RtgrGrid}, Ptr{Float64}, Ptr{UInt64}), handle(ctx), desc, m.g, id))
        end
        m.ids[handle(ctx)] = id[]
    end
    id[]
end
function unload(m::GridMetric, ctx = nothing)
    id = get(m.ids, handle(ctx), UInt64(0))
    id == 0 || check(ccall((:rtgr_grid_metric_unload, librtgr), Cint, (Ctx, UInt64), handle(ctx), id))
    m.ids[handle(ctx)] = UInt64(0)
    nothing
end

# (enum, M, a, user_metric id) of a metric argument, or nothing when it cannot cross the ABI
metric_desc(m::GridMetric, ctx) = (RTGR_GRID, 0.0, 0.0, module_id(m, ctx))
metric_desc(m::DeviceMetric, ctx) = (RTGR_USER, m.M, m.a, module_id(m, ctx))
metric_desc(m::KerrSchild, ctx) = ((m.textbook ? RTGR_KS_TRUE : RTGR_KS_REF) | (m.generic ? RTGR_METRIC_GENERIC : UInt32(0)),
                                   m.M, m.a, UInt64(0))
metric_desc(m, ctx) = m === RayTraceGR.minkowski ? (RTGR_MINKOWSKI, 1.0, 0.0, UInt64(0)) :
                      m === RayTraceGR.kerr_schild ? (RTGR_KS_REF, 1.0, 0.0, UInt64(0)) :   # as written: M = 1, a = 0 (:275-276)
                      nothing

# id of the unit that carries the kernels of `family`'s objects for the metric variant of `scene` (rtgr_user_unit_compile reads the
# metric enum, the RTGR_METRIC_GENERIC flag and whether a != 0 off the scene; a DeviceMetric given as source is compiled into the
# same unit) — built once per (context, source, metric variant)
# (no table on this side: rtgr_user_unit_compile answers the same call again — same context, source, `stationary`, metric variant —
#  at once with the id it gave before FOR AS LONG AS THAT UNIT IS RESIDENT, and builds and loads it again after an unload or a
#  refusal by the load-time probe; a Dict here handed out dead ids, ADVICE r5)
function unit_id(family::DeviceObjects, metric, scene, ctx)
    own = metric isa DeviceMetric
    own && isempty(metric.source) && error("DeviceObjects with a DeviceMetric: give the metric as source text too (the two share one unit)")
    source = own ? metric.source * "\n" * family.source : family.source
    id = Ref{UInt64}(0)
    check(ccall((:rtgr_user_unit_compile, librtgr), Cint, (Ctx, Cstring, Cint, Ptr{RtgrScene}, Ptr{UInt64}),
                handle(ctx), source, own && metric.stationary, own ? C_NULL : scene, id))
    id[]
end

# the families of a scene as ONE family (rtgr_user_source_join) and the base each family's type tags move to
const JOINED = Dict{Vector{DeviceObjects},DeviceObjects}()
function join_families(fams::Vector{DeviceObjects})
    all(f -> f.ntypes > 0, fams) ||
        error("DeviceObjects of several families in one scene: say how many object types each source defines — DeviceObjects(source, ntypes = n)")
    bases = UInt32[sum(UInt32[f.ntypes for f in fams[1:k-1]]; init = UInt32(0)) for k in 1:length(fams)]
    joined = get!(JOINED, fams) do
        srcs = Cstring[Base.unsafe_convert(Cstring, f.source) for f in fams]
        nt = UInt32[f.ntypes for f in fams]
        need = Ref{UInt64}(0)
        GC.@preserve fams begin
            check(ccall((:rtgr_user_source_join, librtgr), Cint, (Ptr{Cstring}, Ptr{UInt32}, Cint, Ptr{UInt8}, UInt64, Ptr{UInt64}),
                        srcs, nt, length(fams), C_NULL, 0, need))
            buf = Vector{UInt8}(undef, need[])
            check(ccall((:rtgr_user_source_join, librtgr), Cint, (Ptr{Cstring}, Ptr{UInt32}, Cint, Ptr{UInt8}, UInt64, Ptr{UInt64}),
                        srcs, nt, length(fams), buf, need[], need))
        end
        DeviceObjects(String(buf[1:end-1]), sum(nt))
    end
    joined, bases
end

"""
    Scene

An `rtgr_scene` ready for a `ccall`, together with what its pointers point to: `objs::Vector{Object{T}}` has no length limit in the
reference (src/RayTraceGR.jl:433-441, :483), so a list beyond the 16 inline slots is handed over as an array (`rtgr_scene.objects`)
that must outlive the call.  `ccall(..., (Ptr{RtgrScene}, ...), scene, ...)` roots this object for the duration of the call
(`cconvert` returns it, `unsafe_convert` takes the pointer of the struct inside).
"""
mutable struct Scene
    ref::Base.RefValue{RtgrScene}
    list::Vector{RtgrObject}       # the packed objects when they travel as an array (empty otherwise)
end
Base.cconvert(::Type{Ptr{RtgrScene}}, s::Scene) = s
Base.unsafe_convert(::Type{Ptr{RtgrScene}}, s::Scene) = Base.unsafe_convert(Ptr{RtgrScene}, s.ref)

# (scene, nothing) or (nothing, why it cannot cross the C ABI)
function scene_of(metric, objs, ctx)
    fams = unique(DeviceObjects[o.family for o in objs if o isa DeviceObject])
    family, bases = length(fams) > 1 ? join_families(fams) : (isempty(fams) ? nothing : fams[1], UInt32[0])
    # (a DeviceMetric beside DeviceObjects lives in the objects' unit: its own module is not loaded)
    d = (!isempty(fams) && metric isa DeviceMetric) ? (RTGR_USER, metric.M, metric.a, UInt64(0)) : metric_desc(metric, ctx)
    d === nothing && return nothing, "the metric `$(nameof(typeof(metric)))` is a Julia callable without a device counterpart " *
                                     "(built-ins: minkowski, kerr_schild, KerrSchild(M, a); your own: DeviceMetric(source = ...))"
    po = map(objs) do o
        o isa DeviceObject ? RtgrObject(RTGR_USER_OBJECT, o.type + bases[findfirst(==(o.family), fams)], o.p) : pack(o)
    end
    k = findfirst(isnothing, po)
    k === nothing || return nothing, "objs[$k] is a `$(nameof(typeof(objs[k])))`: an Object subtype without device source " *
                                     "(built-ins: Plane, Sphere, Disk; your own: DeviceObjects(source))"
    list = length(po) > RTGR_MAX_OBJECTS ? RtgrObject[o for o in po] : RtgrObject[]
    packed = ntuple(i -> (isempty(list) && i <= length(po)) ? po[i] : NOOBJ, RTGR_MAX_OBJECTS)
    make(unit) = Scene(Ref(RtgrScene(d[1], length(objs), d[2], d[3], unit, packed, isempty(list) ? Ptr{RtgrObject}(C_NULL) : pointer(list))), list)
    scene = make(d[4])
    isempty(fams) && return scene, nothing
    make(unit_id(family, metric, scene, ctx)), nothing
end
solver_of(::Type{T}) where {T} = begin
    opt = Ref{RtgrSolver}()
    check(ccall((:rtgr_solver_defaults, librtgr), Cint, (Ptr{RtgrSolver}, Cint), opt, T === Float32 ? 1 : 0))
    opt
end
camera_of(pos, widthx, widthy, normal) =
    Ref(RtgrCamera(Tuple(Float64.(pos)), Tuple(Float64.(widthx)), Tuple(Float64.(widthy)), Tuple(Float64.(normal))))

"""
    make_canvas(metric, pos, widthx, widthy, normal, ni, nj; ctx = nothing) -> Canvas{T}

`RayTraceGR.make_canvas` (src/RayTraceGR.jl:457-478) on the device (`rtgr_make_canvas_f64/_f32`: metric at the pixel, `g⁻¹e_t`,
normalisation — one thread per pixel), returned as the reference's own `Canvas{T}` of `Pixel{T}(x, u, zeros)` (:475).
A metric that cannot cross the ABI (or a scalar type other than Float64 / Float32) falls back to the reference's function, with a warning.
"""
function make_canvas(metric, pos::SVector{4,T}, widthx::SVector{4,T}, widthy::SVector{4,T}, normal::SVector{4,T},
                     ni::Int, nj::Int; ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, RayTraceGR.Object{T}[], ctx)
    if scene === nothing
        cpu_fallback("make_canvas", why)
        return RayTraceGR.make_canvas(metric, pos, widthx, widthy, normal, ni, nj)
    end
    cam = camera_of(pos, widthx, widthy, normal)
    st = Array{T}(undef, 8, ni, nj)                 # n x 8 ray states, pixel index i + j*ni (column-major pixels[i,j], :463-464)
    GC.@preserve st begin
        if T === Float64
            check(ccall((:rtgr_make_canvas_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrCamera}, UInt64, UInt64, UInt64, UInt64, Ptr{Float64}),
                        handle(ctx), scene, cam, ni, nj, 0, nj, pointer(st)))
        else
            check(ccall((:rtgr_make_canvas_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrCamera}, UInt64, UInt64, UInt64, UInt64, Ptr{Float32}),
                        handle(ctx), scene, cam, ni, nj, 0, nj, pointer(st)))
        end
    end
    pixels = Array{RayTraceGR.Pixel{T}}(undef, ni, nj)
    for j in 1:nj, i in 1:ni
        pixels[i, j] = RayTraceGR.Pixel{T}(SVector{4,T}(st[1, i, j], st[2, i, j], st[3, i, j], st[4, i, j]),
                                           SVector{4,T}(st[5, i, j], st[6, i, j], st[7, i, j], st[8, i, j]),
                                           zeros(SVector{3,T}))
    end
    RayTraceGR.Canvas{T}(pixels)
end
# `make_canvas` is generic in T (src/RayTraceGR.jl:457-462); the device computes in Float64 and Float32
function make_canvas(metric, pos::SVector{4,T}, widthx::SVector{4,T}, widthy::SVector{4,T}, normal::SVector{4,T},
                     ni::Int, nj::Int; ctx = nothing) where {T}
    cpu_fallback("make_canvas", "the scalar type $T has no device arithmetic (Float64 and Float32 do)")
    RayTraceGR.make_canvas(metric, pos, widthx, widthy, normal, ni, nj)
end

"""
    trace_rays(metric, objs, c::Canvas{T}; ctx = nothing) -> Canvas{T},   T = Float64 | Float32

Drop-in for `RayTraceGR.trace_rays` (src/RayTraceGR.jl:483-484).  Passes `pointer(c.pixels)` — the reference's own
`Pixel{T}` AoS (:446-450; 88 bytes for Float64, 44 for Float32) — across the ABI; returns a new canvas with `rgb`
filled (:532).  The tolerance is `eps(T)^(3/4)` as in the reference (:485).  `ctx = Context(0:7)`: all eight GPUs of a
node work on the canvas (rows dealt cyclically); the result does not depend on the number of devices, bit for bit.
`metric`: `minkowski`, `kerr_schild`, `KerrSchild(M, a)`, a `DeviceMetric`; anything else runs the reference's CPU path.
`objs`: `Plane`, `Sphere`, `Disk`, `DeviceObject`s, in any number (the reference's `Vector{Object{T}}` has no length limit, :433-441,
and neither has the device: the first 16 travel in the kernels' argument block, a longer list in a device table with its spheres
sorted into groups of neighbours that are asked first — 64 objects cost ≈ 1.8 ×, 256 … 512 ≈ 1.5–1.85 × the 3-object frame); any other `Object` subtype runs the reference's CPU path.  Every fall-back says so once (`@warn`).

Where parity ends: on rays that are CAPTURED with |u^t| ≳ 10⁶ the step sequence follows the rounding noise of the RHS formulation;
the closed-form kernels (`kerr_schild`, `KerrSchild(M, a)`) then take up to 27 % fewer steps than the reference and end such rays with
another status at the step cap (INTEGRATION.md "Where parity ends").  `KerrSchild(M, a; generic = true)` traces with the reference's
own formulation of the RHS (0.82 of SURVEY §8(d)'s flop count executed, 1.18·10¹⁰ steps/s) and is the parity-first setting.
"""
function trace_rays(metric, objs::Vector{RayTraceGR.Object{T}}, c::RayTraceGR.Canvas{T}; ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, objs, ctx)
    if scene === nothing
        cpu_fallback("trace_rays", why)
        return RayTraceGR.trace_rays(metric, objs, c)
    end
    opt = solver_of(T)
    ni, nj = size(c.pixels)
    out = similar(c.pixels)
    ctr = Ref{RtgrCounters}()
    GC.@preserve c out begin
        if T === Float64
            check(ccall((:rtgr_trace_pixels_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Cvoid}, UInt64, UInt64, Ptr{Cvoid}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, pointer(c.pixels), ni, nj, pointer(out), ctr))
        else
            check(ccall((:rtgr_trace_pixels_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Cvoid}, UInt64, UInt64, Ptr{Cvoid}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, pointer(c.pixels), ni, nj, pointer(out), ctr))
        end
    end
    RayTraceGR.Canvas{T}(out)
end
# `trace_rays` is generic in T (src/RayTraceGR.jl:483-485): any other scalar type is the reference's own business, loudly
function trace_rays(metric, objs::Vector{RayTraceGR.Object{T}}, c::RayTraceGR.Canvas{T}; ctx = nothing) where {T}
    cpu_fallback("trace_rays", "the scalar type $T has no device arithmetic (Float64 and Float32 do)")
    RayTraceGR.trace_rays(metric, objs, c)
end

"""
    RayDetails{T}

What the reference computes per ray and throws away: `sols.u[i]` (`state_end`, :516), `sol.t[end]` (`lambda_end`, :503), the
solver's return code (`status`, ignored at :502-505), `omin` of the colouring rule (`hit`, :518-526), the accepted / rejected
step counts; plus `redshift` (the frequency ratio observed/emitted from `Sphere.vel`, which the reference stores and never
uses, :411) and the call's `RtgrCounters`.  Arrays are `ni x nj` like `c.pixels` (`state_end`: `8 x ni x nj`).
"""
struct RayDetails{T}
    state_end::Array{T,3}
    lambda_end::Matrix{T}
    status::Matrix{UInt8}
    hit::Matrix{UInt32}             # (rtgr_ray_outputs.hit32: `objs` may hold more than 255 objects)
    n_accept::Matrix{UInt32}
    n_reject::Matrix{UInt32}
    redshift::Matrix{T}
    counters::RtgrCounters
end

"""
    eval_objects(metric, objs, xs::Vector{SVector{4,T}}; ctx = nothing) -> (d, dmin, hit, rgb)

The object side of the path at the points `xs`, on the device (`rtgr_eval_objects_f64/_f32`): `d[o, p]` = `distance(objs[o], xs[p])`
(:377-419; a `DeviceObject`: its unit's `rtgr_user_distance`), `dmin[p]` = `min_distance` (:433-441), and the colouring loop of
`trace_rays` (:513-533) as if a ray had ended at `xs[p]`: `hit[p]` = the object's index (0: nothing within the threshold), `rgb[:, p]`.
What `runtests_hip.jl` holds against the Julia methods of the same object, point by point.
"""
function eval_objects(metric, objs::Vector{RayTraceGR.Object{T}}, xs::Vector{SVector{4,T}}; ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("eval_objects: this scene runs on the reference's CPU path: ", why)
    length(objs) <= 255 || error("eval_objects: `hit` is a byte per point (at most 255 objects)")
    opt = solver_of(T)
    n = length(xs)
    d = Matrix{T}(undef, max(length(objs), 1), n)        # C layout d[p * nobj + o]
    dmin = Vector{T}(undef, n)
    hit = Vector{UInt8}(undef, n)
    rgb = Matrix{T}(undef, 3, n)                         # C layout rgb[3 p + c]
    GC.@preserve xs d dmin hit rgb begin
        if T === Float64
            check(ccall((:rtgr_eval_objects_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Cvoid}, UInt64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Cvoid}),
                        handle(ctx), scene, opt, pointer(xs), n, pointer(d), pointer(dmin), pointer(hit), pointer(rgb)))
        else
            check(ccall((:rtgr_eval_objects_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Cvoid}, UInt64, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}, Ptr{Cvoid}),
                        handle(ctx), scene, opt, pointer(xs), n, pointer(d), pointer(dmin), pointer(hit), pointer(rgb)))
        end
    end
    d, dmin, hit, rgb
end

"""
    check_scene(metric, objs, pos, widthx, widthy, normal; ni = 48, nj = 48, ctx = nothing)

`rtgr_scene_check`: traces a coarse canvas of this camera through the single FULL pass (every accepted step scanned, as the
reference's ContinuousCallback does, :488-490) and through the FAR + NEAR passes, and throws unless the two frames agree (bit for bit
for a built-in metric).  The check to run once on a scene with `DeviceObject`s whose source brings a `rtgr_user_reach` bound: a bound
that is too small loses hits silently, and this is what says so.
"""
function check_scene(metric, objs::Vector{RayTraceGR.Object{T}}, pos, widthx, widthy, normal; ni::Integer = 48, nj::Integer = 48,
                     ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("check_scene: this scene runs on the reference's CPU path (nothing to check): ", why)
    opt = solver_of(Float64)
    cam = camera_of(pos, widthx, widthy, normal)
    check(ccall((:rtgr_scene_check, librtgr), Cint, (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrCamera}, UInt64, UInt64, Cint),
                handle(ctx), scene, opt, cam, ni, nj, 0))
    nothing
end

"""
    render(metric, objs, pos, widthx, widthy, normal, ni, nj; T = Float64, ctx = nothing, details = false)
        -> (R, G, B)  or  ((R, G, B), RayDetails)

`make_canvas` + `trace_rays` in ONE call with the camera on the device (`rtgr_trace_f64/_f32`, `state0 = NULL`): the 88-byte
pixels never exist — nothing goes up, three `ni x nj` planes come back (what `colorview(RGB, R', G', B')` consumes, :566-569).
This is the call for the big screens (4096², 8192²: 5.9 GB of pixels each way otherwise).  All devices of `ctx` take part.
"""
function render(metric, objs, pos, widthx, widthy, normal, ni::Integer, nj::Integer;
                T::Type = Float64, ctx = nothing, details::Bool = false)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("render has no CPU counterpart in the reference (make_canvas + trace_rays are the reference's calls): ", why)
    opt = solver_of(T)
    cam = camera_of(pos, widthx, widthy, normal)
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    ctr = Ref{RtgrCounters}()
    det = details ? RayDetails{T}(Array{T}(undef, 8, ni, nj), Matrix{T}(undef, ni, nj), Matrix{UInt8}(undef, ni, nj),
                                  Matrix{UInt32}(undef, ni, nj), Matrix{UInt32}(undef, ni, nj), Matrix{UInt32}(undef, ni, nj),
                                  Matrix{T}(undef, ni, nj), RtgrCounters(0, 0, 0, 0, 0, 0, 0, 0)) : nothing
    GC.@preserve rgb det begin
        outs = details ? Ref(RtgrRayOutputs(pointer(det.state_end), pointer(det.lambda_end), pointer(det.status), C_NULL,
                                            pointer(det.n_accept), pointer(det.n_reject), pointer(det.redshift), pointer(det.hit))) :
                         Ref(RtgrRayOutputs(C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
        if T === Float64
            check(ccall((:rtgr_trace_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Float64}, Ptr{RtgrCamera}, UInt64, UInt64, UInt64, UInt64,
                         Ptr{Float64}, Ptr{RtgrRayOutputs}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, C_NULL, cam, ni, nj, 0, nj, pointer(rgb), outs, ctr))
        else
            check(ccall((:rtgr_trace_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Float32}, Ptr{RtgrCamera}, UInt64, UInt64, UInt64, UInt64,
                         Ptr{Float32}, Ptr{RtgrRayOutputs}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, C_NULL, cam, ni, nj, 0, nj, pointer(rgb), outs, ctr))
        end
    end
    planes = (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3])
    details || return planes
    planes, RayDetails{T}(det.state_end, det.lambda_end, det.status, det.hit, det.n_accept, det.n_reject, det.redshift, ctr[])
end

"""
    trace_rays_aa(metric, objs, pos, widthx, widthy, normal, ni, nj; k = 4, contrast = 1 / 255, T = Float64, ctx = nothing)
        -> ((R, G, B), refined, RtgrAAStats)

ADAPTIVE ANTI-ALIASING (`rtgr_trace_aa_f64/_f32`) — an extension: the reference traces one ray through each pixel centre, and its
colour rule is discontinuous (the 24-band sawtooth of `objcolor`, :427; the object index; the miss colour, :528).  This is `render`'s
frame with the pixels that differ from a 4-neighbour — in the object hit, in the solver's status, or by more than `contrast` in a colour
channel — traced again with `k x k` sub-rays (the pixels of the `k ni x k nj` canvas of the same camera) and box-filtered; every other
pixel keeps `render`'s bits.  `contrast < 0`: every pixel (uniform supersampling); `Inf`: class edges only.  `refined[i, j]` is 1
where the pixel was refined.  Runs on device 0 of `ctx`.
"""
function trace_rays_aa(metric, objs, pos, widthx, widthy, normal, ni::Integer, nj::Integer;
                       k::Integer = 4, contrast::Real = 1 / 255, T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_rays_aa has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    cam = camera_of(pos, widthx, widthy, normal)
    aa = Ref(RtgrAA(UInt32(k), UInt32(0), Float64(contrast), UInt64(0)))
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    refined = Matrix{UInt8}(undef, ni, nj)
    ctr = Ref{RtgrCounters}()
    stats = Ref{RtgrAAStats}()
    GC.@preserve rgb refined begin
        if T === Float64
            check(ccall((:rtgr_trace_aa_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrCamera}, UInt64, UInt64, Ptr{RtgrAA}, Ptr{Float64},
                         Ptr{RtgrRayOutputs}, Ptr{UInt8}, Ptr{RtgrCounters}, Ptr{RtgrAAStats}),
                        handle(ctx), scene, opt, cam, ni, nj, aa, pointer(rgb), C_NULL, pointer(refined), ctr, stats))
        else
            check(ccall((:rtgr_trace_aa_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrCamera}, UInt64, UInt64, Ptr{RtgrAA}, Ptr{Float32},
                         Ptr{RtgrRayOutputs}, Ptr{UInt8}, Ptr{RtgrCounters}, Ptr{RtgrAAStats}),
                        handle(ctx), scene, opt, cam, ni, nj, aa, pointer(rgb), C_NULL, pointer(refined), ctr, stats))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), refined, stats[]
end

"""
    load_texture(planes; ctx = nothing) -> UInt64

An IMAGE TEXTURE for `trace_rays_shaded` (`rtgr_texture_load`; include/rtgr.h "image textures"): `planes` is a `width x height x 3`
array — the three colour planes, column fastest, which is the layout `render` returns its frame in: a rendered `ni x nj` frame is a
texture as it stands.  Every texel must be finite, `width` and `height` 2 .. 16384.  Uploaded to every device of `ctx`; the id never
coincides with a grid's or a unit's.  `unload_texture(id; ctx)` releases the id (`rtgr_texture_unload`; 0: every texture).
"""
function load_texture(planes; ctx = nothing)
    size(planes, 3) == 3 || error("load_texture: planes must be width x height x 3")
    t = Array{Float64,3}(planes)
    desc = Ref(RtgrTextureDesc(UInt32(size(t, 1)), UInt32(size(t, 2)), UInt32(0), UInt32(0)))
    id = Ref{UInt64}(0)
    check(ccall((:rtgr_texture_load, librtgr), Cint, (Ctx, Ptr{RtgrTextureDesc}, Ptr{Float64}, Ptr{UInt64}), handle(ctx), desc, t, id))
    id[]
end
function unload_texture(id; ctx = nothing)
    check(ccall((:rtgr_texture_unload, librtgr), Cint, (Ctx, UInt64), handle(ctx), id))
    nothing
end

"""
    trace_rays_shaded(metric, objs, pos, widthx, widthy, normal, ni, nj; textures = (), r_escape = 0.0, T = Float64, ctx = nothing)
        -> (R, G, B)

A frame with IMAGE TEXTURES (`rtgr_trace_shaded_f64/_f32`) — an extension: the reference colours by fixed rules (`objcolor`, :420-427;
the miss colour, :528).  This is `render`'s frame with the pixels whose object — or whose escape — has a texture bound coloured by the
texel instead; every other pixel keeps `render`'s bits.  `textures` is a collection of `(object, id, filter)`: `object` the 1-based
index in `objs` (a `Sphere` of either radius sign — the sky `caelum` — or a `Disk`), or 0 for the rays that end without a hit at
`|x| >= r_escape`, which are coloured by the direction they end with; `id` from `load_texture`; `filter` `RTGR_TEX_NEAREST` or
`RTGR_TEX_BILINEAR`.  Runs on device 0 of `ctx`.
"""
function trace_rays_shaded(metric, objs, pos, widthx, widthy, normal, ni::Integer, nj::Integer;
                           textures = (), r_escape::Real = 0.0, T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_rays_shaded has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    cam = camera_of(pos, widthx, widthy, normal)
    binds = RtgrTextureBind[RtgrTextureBind(UInt32(b[1]), UInt32(b[3]), UInt64(b[2])) for b in textures]
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    ctr = Ref{RtgrCounters}()
    GC.@preserve rgb binds begin
        shade = Ref(RtgrShade(UInt32(length(binds)), UInt32(0), pointer(binds), Float64(r_escape)))
        if T === Float64
            check(ccall((:rtgr_trace_shaded_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrCamera}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrAA}, Ptr{Float64},
                         Ptr{RtgrRayOutputs}, Ptr{UInt8}, Ptr{RtgrCounters}, Ptr{RtgrAAStats}),
                        handle(ctx), scene, opt, cam, ni, nj, shade, C_NULL, pointer(rgb), C_NULL, C_NULL, ctr, C_NULL))
        else
            check(ccall((:rtgr_trace_shaded_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrCamera}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrAA}, Ptr{Float32},
                         Ptr{RtgrRayOutputs}, Ptr{UInt8}, Ptr{RtgrCounters}, Ptr{RtgrAAStats}),
                        handle(ctx), scene, opt, cam, ni, nj, shade, C_NULL, pointer(rgb), C_NULL, C_NULL, ctr, C_NULL))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3])
end

"""
    disk_emission(object, T_in; p = 0.75, orbit = 1, emitter = RTGR_EMIT_KEPLER, inner_edge = false, gain = 1.0,
                  wavelengths_nm = (700.0, 546.1, 435.8)) -> RtgrDiskEmission

The parameters of an emitting disk for `trace_rays_emission`: `object` is the 1-based index of a `Disk` in `objs`; the three channels are
Planck's law at `wavelengths_nm`, theta_c = h c / (lambda_c k_B) and weight_c = (546.1 / lambda_c)^5.
"""
function disk_emission(object::Integer, T_in::Real; p::Real = 0.75, orbit::Real = 1, emitter::UInt32 = RTGR_EMIT_KEPLER, inner_edge::Bool = false,
                       gain::Real = 1.0, wavelengths_nm = (700.0, 546.1, 435.8))
    lam = Float64.(Tuple(wavelengths_nm))
    length(lam) == 3 || error("disk_emission: wavelengths_nm needs three wavelengths (r, g, b)")
    RtgrDiskEmission(UInt32(object), emitter, inner_edge ? RTGR_EMIT_INNER_EDGE : UInt32(0), UInt32(0), Float64(orbit), Float64(T_in), Float64(p),
                     Float64(gain), 1.438776877e7 ./ lam, (546.1 ./ lam) .^ 5)
end

"""
    trace_rays_emission(metric, objs, pos, widthx, widthy, normal, ni, nj, emission; T = Float64, ctx = nothing) -> ((R, G, B), g)

A frame with an EMITTING DISK (`rtgr_trace_emission_f64/_f32`) — an extension: `render`'s frame with the pixels that hit the `Disk`
`emission.object` coloured as a black body on the circular orbits of the scene's own metric (include/rtgr.h "disk emission"), shifted by
the frequency ratio `g`, which comes back as an `ni x nj` matrix (NaN off the disk and where no circular orbit exists: black).  Every
other pixel keeps `render`'s bits.  `emission` from `disk_emission`.  Built-in metrics and 3-D grids; runs on device 0 of `ctx`.
"""
function trace_rays_emission(metric, objs, pos, widthx, widthy, normal, ni::Integer, nj::Integer, emission::RtgrDiskEmission;
                             T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_rays_emission has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    cam = camera_of(pos, widthx, widthy, normal)
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    g = Array{T}(undef, ni, nj)
    ctr = Ref{RtgrCounters}()
    emit = Ref(emission)
    GC.@preserve rgb g begin
        if T === Float64
            check(ccall((:rtgr_trace_emission_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrCamera}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{RtgrAA},
                         Ptr{Float64}, Ptr{RtgrRayOutputs}, Ptr{Float64}, Ptr{UInt8}, Ptr{RtgrCounters}, Ptr{RtgrAAStats}),
                        handle(ctx), scene, opt, cam, ni, nj, C_NULL, emit, C_NULL, pointer(rgb), C_NULL, pointer(g), C_NULL, ctr, C_NULL))
        else
            check(ccall((:rtgr_trace_emission_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrCamera}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{RtgrAA},
                         Ptr{Float32}, Ptr{RtgrRayOutputs}, Ptr{Float32}, Ptr{UInt8}, Ptr{RtgrCounters}, Ptr{RtgrAAStats}),
                        handle(ctx), scene, opt, cam, ni, nj, C_NULL, emit, C_NULL, pointer(rgb), C_NULL, pointer(g), C_NULL, ctr, C_NULL))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), g
end

"""
    Observer(pos, look, up, fov_x, fov_y = fov_x; kind = RTGR_OBS_STATIC, vel = (0, 0, 0, 0), orbit = 1,
             projection = RTGR_PROJ_PERSPECTIVE, max_batch_rays = 0) -> RtgrObserver

A pinhole camera at the event `pos`, carried by an observer who is at rest in the slicing (`RTGR_OBS_STATIC`), moves with the coordinate
4-velocity `vel` (`RTGR_OBS_VELOCITY`) or rides the circular geodesic through `pos` (z = 0) of the scene's own metric (`RTGR_OBS_CIRCULAR`,
`orbit` = +1 / -1).  `look` and `up` are coordinate 4-vectors; angles in radians (include/rtgr.h "observer camera").
"""
function Observer(pos, look, up, fov_x::Real, fov_y::Real = fov_x; kind::UInt32 = RTGR_OBS_STATIC, vel = (0.0, 0.0, 0.0, 0.0), orbit::Real = 1,
                  projection::UInt32 = RTGR_PROJ_PERSPECTIVE, max_batch_rays::Integer = 0)
    v4(v) = NTuple{4,Float64}(Float64.(Tuple(v)))
    RtgrObserver(v4(pos), v4(vel), v4(look), v4(up), Float64(fov_x), Float64(fov_y), Float64(orbit), kind, projection, UInt32(0), UInt32(0),
                 UInt64(max_batch_rays))
end

# the frame the library builds from `obs` in `scene` (rtgr_eval_observer_f64/_f32, blocking): (4 x 4 matrix with the COLUMNS e_0, e_right,
# e_up, e_look; Omega) — or an error when the frame is not valid
function observer_frame(scene, obs; T::Type = Float64, ctx = nothing)
    frame = Array{T}(undef, 4, 4)                   # C writes rows e_0, e_right, e_up, e_look: Julia's columns
    omega = Ref{T}(T(0))
    valid = Ref{Cint}(0)
    GC.@preserve frame begin
        if T === Float64
            check(ccall((:rtgr_eval_observer_f64, librtgr), Cint, (Ctx, Ptr{RtgrScene}, Ptr{RtgrObserver}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                        handle(ctx), scene, obs, pointer(frame), omega, valid))
        else
            check(ccall((:rtgr_eval_observer_f32, librtgr), Cint, (Ctx, Ptr{RtgrScene}, Ptr{RtgrObserver}, Ptr{Float32}, Ptr{Float32}, Ptr{Cint}),
                        handle(ctx), scene, obs, pointer(frame), omega, valid))
        end
    end
    valid[] == 0 && error("Observer: no valid frame at this event (a 4-velocity that is not timelike and future-directed, no circular orbit ",
                          "there, or look / up degenerate after projection)")
    frame, omega[]
end

"""
    trace_rays_observer(metric, objs, observer, ni, nj; emission = nothing, T = Float64, ctx = nothing) -> ((R, G, B), g)

A frame seen by an OBSERVER (`rtgr_trace_observer_f64/_f32`) — an extension: the rays of a pinhole at one event, in the orthonormal frame
of a static, moving or orbiting observer (`Observer`), traced as `render` traces caller-supplied states.  With `emission` (from
`disk_emission`) the disk glows and `g`, the frequency ratio against THIS observer's 4-velocity, comes back as an `ni x nj` matrix;
without it `g` is `nothing`.  The frame is asked for first (`rtgr_eval_observer_f64/_f32`): an observer with no valid frame is an error.
Built-in metrics and 3-D grids; runs on device 0 of `ctx`.
"""
function trace_rays_observer(metric, objs, observer::RtgrObserver, ni::Integer, nj::Integer; emission = nothing, T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_rays_observer has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    obs = Ref(observer)
    observer_frame(scene, obs; T = T, ctx = ctx)    # (raises when no frame exists there: the trace itself would only end every ray as NaN)
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    g = Array{T}(undef, ni, nj)
    ctr = Ref{RtgrCounters}()
    emit = emission === nothing ? C_NULL : Ref(emission::RtgrDiskEmission)
    gp = emission === nothing ? Ptr{T}(C_NULL) : pointer(g)
    GC.@preserve rgb g begin
        if T === Float64
            check(ccall((:rtgr_trace_observer_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{Float64},
                         Ptr{RtgrRayOutputs}, Ptr{Float64}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, pointer(rgb), C_NULL, gp, ctr))
        else
            check(ccall((:rtgr_trace_observer_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{Float32},
                         Ptr{RtgrRayOutputs}, Ptr{Float32}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, pointer(rgb), C_NULL, gp, ctr))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), (emission === nothing ? nothing : g)
end

"""
    HotSpot(rho_s, sigma; phi0 = 0, cut = 4, amp = 1, g_power = 4, t_start = 0, dt = 1, nt = 1) -> RtgrHotSpot

A rigid Gaussian spot of width `sigma` that rides in the emitting disk at cylindrical radius `rho_s` with the orbital rate of the disk's
own emitter model, seen at the observer times `t_start + k dt`, `k < nt` (include/rtgr.h "hot-spot light curves").
"""
function HotSpot(rho_s::Real, sigma::Real; phi0::Real = 0, cut::Real = 4, amp::Real = 1, g_power::Real = 4, t_start::Real = 0, dt::Real = 1,
                 nt::Integer = 1)
    RtgrHotSpot(Float64(rho_s), Float64(phi0), Float64(sigma), Float64(cut), Float64(amp), Float64(g_power), Float64(t_start), Float64(dt),
                UInt64(nt), UInt32(0), UInt32(0))
end

# the spot's orbital rate in the disk of `emit` (rtgr_eval_hot_spot_f64/_f32, blocking) — or an error when no valid orbit exists at rho_s
function eval_hot_spot(scene, emit, spot; T::Type = Float64, ctx = nothing)
    omega = Ref{T}(T(0))
    valid = Ref{Cint}(0)
    if T === Float64
        check(ccall((:rtgr_eval_hot_spot_f64, librtgr), Cint,
                    (Ctx, Ptr{RtgrScene}, Ptr{RtgrDiskEmission}, Ptr{RtgrHotSpot}, Ptr{Float64}, UInt64, Ptr{Float64}, Ptr{Cint}, Ptr{Float64}),
                    handle(ctx), scene, emit, spot, C_NULL, 0, omega, valid, C_NULL))
    else
        check(ccall((:rtgr_eval_hot_spot_f32, librtgr), Cint,
                    (Ctx, Ptr{RtgrScene}, Ptr{RtgrDiskEmission}, Ptr{RtgrHotSpot}, Ptr{Float32}, UInt64, Ptr{Float32}, Ptr{Cint}, Ptr{Float64}),
                    handle(ctx), scene, emit, spot, C_NULL, 0, omega, valid, C_NULL))
    end
    valid[] == 0 && error("HotSpot: no valid circular orbit of the disk's emitter at rho_s (none exists there, or it is not timelike)")
    omega[]
end

"""
    light_curve(metric, objs, observer, ni, nj, emission, spot; T = Float64, ctx = nothing) -> ((R, G, B), g, lc, tau)

The LIGHT CURVE of a hot spot (`rtgr_trace_light_curve_f64/_f32`) — an extension: ONE frame of the emitting disk seen by `observer`, as
`trace_rays_observer` with `emission`, reduced on the device over the `nt` observer times of `spot` (from `HotSpot`).  `lc` is
`3 x nt`: the rows F, A, B per observer time `tau[k]`; the image centroid is `(A / F, B / F)` in the pixel coordinates of the frame.  The
picture is the disk without the spot.  The observer's frame and the spot's orbit are asked for first: either being invalid is an error.
"""
function light_curve(metric, objs, observer::RtgrObserver, ni::Integer, nj::Integer, emission::RtgrDiskEmission, spot::RtgrHotSpot;
                     T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("light_curve has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    obs = Ref(observer)
    emit = Ref(emission)
    sp = Ref(spot)
    observer_frame(scene, obs; T = T, ctx = ctx)
    eval_hot_spot(scene, emit, sp; T = T, ctx = ctx)
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    g = Array{T}(undef, ni, nj)
    lc = Array{Float64}(undef, 3, Int(spot.nt))     # C writes nt x 3 row-major: Julia's 3 x nt
    ctr = Ref{RtgrCounters}()
    GC.@preserve rgb g lc begin
        if T === Float64
            check(ccall((:rtgr_trace_light_curve_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{RtgrHotSpot},
                         Ptr{Float64}, Ptr{RtgrRayOutputs}, Ptr{Float64}, Ptr{Float64}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, sp, pointer(rgb), C_NULL, pointer(g), pointer(lc), ctr))
        else
            check(ccall((:rtgr_trace_light_curve_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{RtgrHotSpot},
                         Ptr{Float32}, Ptr{RtgrRayOutputs}, Ptr{Float32}, Ptr{Float64}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, sp, pointer(rgb), C_NULL, pointer(g), pointer(lc), ctr))
        end
    end
    tau = [spot.t_start + k * spot.dt for k in 0:Int(spot.nt)-1]
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), g, lc, tau
end

"""
    Spectrum(kind, lo, hi, nb; amp = 1, alpha = 0, rho_min = 0, rho_max = 0, g_power = 4, log_axis = false, nu3 = false) -> RtgrSpectrum

A spectrum of the emitting disk (include/rtgr.h "disk spectra").  `kind = RTGR_SPEC_LINE`: the profile of a narrow line of rest energy 1,
`nb` bins over `[lo, hi)` of the frequency ratio g, emissivity `amp (rho / rho_min)^(-alpha)` inside `rho_min <= rho < rho_max`, weight
`g^g_power`.  `kind = RTGR_SPEC_THERMAL`: the black-body disk at `nb` sample frequencies theta_k from `lo` to `hi` (the units of the
emission's theta), linear or — `log_axis` — geometric; `nu3` multiplies sample k by theta_k^3.  The line-only fields are sent as 0 then.
"""
function Spectrum(kind::UInt32, lo::Real, hi::Real, nb::Integer; amp::Real = 1, alpha::Real = 0, rho_min::Real = 0, rho_max::Real = 0,
                  g_power::Real = 4, log_axis::Bool = false, nu3::Bool = false)
    if kind == RTGR_SPEC_THERMAL
        return RtgrSpectrum(kind, (log_axis ? RTGR_SPEC_LOG : UInt32(0)) | (nu3 ? RTGR_SPEC_NU3 : UInt32(0)), UInt64(nb), Float64(lo), Float64(hi),
                            0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    end
    RtgrSpectrum(kind, UInt32(0), UInt64(nb), Float64(lo), Float64(hi), Float64(amp), Float64(alpha), Float64(rho_min), Float64(rho_max),
                 Float64(g_power), 0.0)
end

# the spectral axis of `spec` in the disk of `emit` (rtgr_eval_spectrum_f64/_f32, blocking, no points): the bin centres of a line
# profile, the sample frequencies of a thermal spectrum — and every refusal of the record, before anything is traced
function eval_spectrum(scene, emit, spec; T::Type = Float64, ctx = nothing)
    axis = Array{Float64}(undef, Int(spec[].nb))
    GC.@preserve axis begin
        if T === Float64
            check(ccall((:rtgr_eval_spectrum_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrDiskEmission}, Ptr{RtgrSpectrum}, Ptr{Float64}, UInt64, Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}),
                        handle(ctx), scene, emit, spec, C_NULL, 0, pointer(axis), C_NULL, C_NULL))
        else
            check(ccall((:rtgr_eval_spectrum_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrDiskEmission}, Ptr{RtgrSpectrum}, Ptr{Float32}, UInt64, Ptr{Float64}, Ptr{Cvoid}, Ptr{Float64}),
                        handle(ctx), scene, emit, spec, C_NULL, 0, pointer(axis), C_NULL, C_NULL))
        end
    end
    axis
end

"""
    spectrum(metric, objs, observer, ni, nj, emission, spec; T = Float64, ctx = nothing) -> ((R, G, B), g, axis, fab)

The SPECTRUM of an emitting disk (`rtgr_trace_spectrum_f64/_f32`) — an extension: ONE frame of the disk seen by `observer`, as
`trace_rays_observer` with `emission`, reduced on the device to the line profile or the thermal spectrum `spec` names (from `Spectrum`).
`fab` is `3 x nb`: the rows F, A, B per bin or sample of `axis`; the flux centroid there is `(A / F, B / F)` in the pixel coordinates of
the frame.  The observer's frame and the record are asked for first: an invalid frame or a refused record is an error.
"""
function spectrum(metric, objs, observer::RtgrObserver, ni::Integer, nj::Integer, emission::RtgrDiskEmission, spec::RtgrSpectrum;
                  T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("spectrum has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    obs = Ref(observer)
    emit = Ref(emission)
    sp = Ref(spec)
    observer_frame(scene, obs; T = T, ctx = ctx)
    axis = eval_spectrum(scene, emit, sp; T = T, ctx = ctx)
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    g = Array{T}(undef, ni, nj)
    fab = Array{Float64}(undef, 3, Int(spec.nb))    # C writes nb x 3 row-major: Julia's 3 x nb
    ctr = Ref{RtgrCounters}()
    GC.@preserve rgb g fab begin
        if T === Float64
            check(ccall((:rtgr_trace_spectrum_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{RtgrSpectrum},
                         Ptr{Float64}, Ptr{RtgrRayOutputs}, Ptr{Float64}, Ptr{Float64}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, sp, pointer(rgb), C_NULL, pointer(g), pointer(fab), ctr))
        else
            check(ccall((:rtgr_trace_spectrum_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission}, Ptr{RtgrSpectrum},
                         Ptr{Float32}, Ptr{RtgrRayOutputs}, Ptr{Float32}, Ptr{Float64}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, sp, pointer(rgb), C_NULL, pointer(g), pointer(fab), ctr))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), g, axis, fab
end

"""
    Polarization(kind; deg0 = 1, deg1 = 0, field = (0, 0, 0)) -> RtgrPolarization

The emission law of a polarized disk image (include/rtgr.h "polarized disk images").  `kind = RTGR_POL_SCATTER`: an electron-scattering
atmosphere, the electric vector in the disk plane, degree `deg0 (1 - mu) / (1 + deg1 mu)`.  `kind = RTGR_POL_FIELD`: synchrotron emission
in the ordered field `field = (B_rho, B_phi, B_z)` of the emitter's triad, degree `deg0`.
"""
function Polarization(kind::UInt32; deg0::Real = 1, deg1::Real = 0, field = (0.0, 0.0, 0.0))
    RtgrPolarization(kind, UInt32(0), Float64(deg0), Float64(deg1), (Float64(field[1]), Float64(field[2]), Float64(field[3])), (0.0, 0.0))
end

"""
    trace_rays_polarized(metric, objs, observer, ni, nj, emission, pol; T = Float64, ctx = nothing) -> ((R, G, B), g, q, u, aux)

A POLARIZED frame of an emitting disk (`rtgr_trace_polarized_f64/_f32`) — an extension: the frame of `trace_rays_observer` with
`emission`, bit for bit, plus the fractional Stokes pair `(q, u)` by Walker-Penrose transport and `aux` (mu or sin zeta), `ni x nj`
each, NaN off the disk.  The metric must be `KerrSchild(M, a)` with the textbook radius, or flat space.  The observer's frame is asked
for first: an invalid frame or a refused record is an error.
"""
function trace_rays_polarized(metric, objs, observer::RtgrObserver, ni::Integer, nj::Integer, emission::RtgrDiskEmission, pol::RtgrPolarization;
                              T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_rays_polarized has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    obs = Ref(observer)
    emit = Ref(emission)
    pl = Ref(pol)
    observer_frame(scene, obs; T = T, ctx = ctx)
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    g = Array{T}(undef, ni, nj)
    q = Array{T}(undef, ni, nj)
    u = Array{T}(undef, ni, nj)
    aux = Array{T}(undef, ni, nj)
    ctr = Ref{RtgrCounters}()
    GC.@preserve rgb g q u aux begin
        if T === Float64
            check(ccall((:rtgr_trace_polarized_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission},
                         Ptr{RtgrPolarization}, Ptr{Float64}, Ptr{RtgrRayOutputs}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64},
                         Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, pl, pointer(rgb), C_NULL, pointer(g), pointer(q), pointer(u),
                        pointer(aux), ctr))
        else
            check(ccall((:rtgr_trace_polarized_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission},
                         Ptr{RtgrPolarization}, Ptr{Float32}, Ptr{RtgrRayOutputs}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
                         Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, emit, pl, pointer(rgb), C_NULL, pointer(g), pointer(q), pointer(u),
                        pointer(aux), ctr))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), g, q, u, aux
end

"""
    eval_polarization(metric, objs, emission, pol, observer, s0, s_end; ctx = nothing) -> (kappa, f_em, aux, delta, q, u, valid)

The polarization kernel itself at `n` pairs of ray states (`rtgr_eval_polarization_f64/_f32`, blocking): `s0` (`8 x n`) at the camera,
the observer's own states, and `s_end` (`8 x n`) on the disk.  `kappa` is `2 x n`, `f_em` `4 x n`, the others have length `n`.
"""
function eval_polarization(metric, objs, emission::RtgrDiskEmission, pol::RtgrPolarization, observer::RtgrObserver, s0::Matrix{T}, s_end::Matrix{T};
                           ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("eval_polarization: ", why)
    size(s0) == size(s_end) && size(s0, 1) == 8 || error("eval_polarization: s0 and s_end must both be 8 x n")
    n = size(s0, 2)
    obs = Ref(observer)
    emit = Ref(emission)
    pl = Ref(pol)
    observer_frame(scene, obs; T = T, ctx = ctx)
    kappa = Array{T}(undef, 2, n); f_em = Array{T}(undef, 4, n)
    aux = Array{T}(undef, n); delta = Array{T}(undef, n); q = Array{T}(undef, n); u = Array{T}(undef, n)
    valid = Array{Cint}(undef, n)
    GC.@preserve s0 s_end kappa f_em aux delta q u valid begin
        if T === Float64
            check(ccall((:rtgr_eval_polarization_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrDiskEmission}, Ptr{RtgrPolarization}, Ptr{RtgrObserver}, Ptr{Float64}, Ptr{Float64}, UInt64,
                         Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Cint}),
                        handle(ctx), scene, emit, pl, obs, pointer(s0), pointer(s_end), n, pointer(kappa), pointer(f_em), pointer(aux),
                        pointer(delta), pointer(q), pointer(u), pointer(valid)))
        else
            check(ccall((:rtgr_eval_polarization_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrDiskEmission}, Ptr{RtgrPolarization}, Ptr{RtgrObserver}, Ptr{Float32}, Ptr{Float32}, UInt64,
                         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cint}),
                        handle(ctx), scene, emit, pl, obs, pointer(s0), pointer(s_end), n, pointer(kappa), pointer(f_em), pointer(aux),
                        pointer(delta), pointer(q), pointer(u), pointer(valid)))
        end
    end
    kappa, f_em, aux, delta, q, u, map(v -> v != 0, valid)
end

"""
    eval_walker_penrose(metric, s, f; ctx = nothing) -> kappa

The two Walker-Penrose constants `(Y(k, f), h(k, f))` (`2 x n`) at `n` states `s = (x, k)` (`8 x n`) and `n` vectors `f` (`4 x n`), by the
polarization kernel's own Killing-Yano forms (`rtgr_eval_walker_penrose_f64/_f32`, blocking); NaN on the axis.
"""
function eval_walker_penrose(metric, s::Matrix{T}, f::Matrix{T}; ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, RayTraceGR.Object{T}[], ctx)
    scene === nothing && error("eval_walker_penrose: ", why)
    size(s, 1) == 8 && size(f, 1) == 4 && size(s, 2) == size(f, 2) || error("eval_walker_penrose: s must be 8 x n and f 4 x n")
    n = size(s, 2)
    kappa = Array{T}(undef, 2, n)
    GC.@preserve s f kappa begin
        if T === Float64
            check(ccall((:rtgr_eval_walker_penrose_f64, librtgr), Cint, (Ctx, Ptr{RtgrScene}, Ptr{Float64}, Ptr{Float64}, UInt64, Ptr{Float64}),
                        handle(ctx), scene, pointer(s), pointer(f), n, pointer(kappa)))
        else
            check(ccall((:rtgr_eval_walker_penrose_f32, librtgr), Cint, (Ctx, Ptr{RtgrScene}, Ptr{Float32}, Ptr{Float32}, UInt64, Ptr{Float32}),
                        handle(ctx), scene, pointer(s), pointer(f), n, pointer(kappa)))
        end
    end
    kappa
end

"""
    Flow(j0; kappa = 0, r0 = 1, alpha = 1, H = 0.3, s = 0, r_stop = 0, orbit = 1, emitter = RTGR_EMIT_KEPLER, gain = 1, weight = (1, 1, 1)) -> RtgrFlow

A hot, rotating flow that emits and absorbs along each ray (include/rtgr.h "volume emission").  Density `(r / r0)^(-alpha)
exp(-z^2 / (2 H^2 rho^2))`; `emitter = RTGR_EMIT_KEPLER`: gas on cylinders at the circular-orbit rate of the scene's own metric, `orbit`
= +1 or -1; `RTGR_EMIT_RIGID`: Omega = `orbit`.  Emissivity `j0 n nu^(-s)`, grey absorption `kappa n`.  Choose `r_stop` between the
horizon's coordinate radius and the photon orbit's cylinder (0 in flat space).
"""
function Flow(j0::Real; kappa::Real = 0, r0::Real = 1, alpha::Real = 1, H::Real = 0.3, s::Real = 0, r_stop::Real = 0, orbit::Real = 1,
              emitter::UInt32 = RTGR_EMIT_KEPLER, gain::Real = 1, weight = (1.0, 1.0, 1.0))
    RtgrFlow(emitter, UInt32(0), Float64(orbit), Float64(j0), Float64(kappa), Float64(r0), Float64(alpha), Float64(H), Float64(s), Float64(r_stop),
             Float64(gain), (Float64(weight[1]), Float64(weight[2]), Float64(weight[3])))
end

# the solver record of T with lambda1 and / or max_steps replaced (nothing: the default)
function solver_with(::Type{T}, lambda1, max_steps) where {T}
    opt = solver_of(T)
    o = opt[]
    opt[] = RtgrSolver(o.reltol, o.abstol, o.lambda0, lambda1 === nothing ? o.lambda1 : Float64(lambda1), o.hit_threshold, o.miss_rgb,
                       max_steps === nothing ? o.max_steps : UInt32(max_steps), o.interp_points)
    opt
end

"""
    trace_rays_transfer(metric, objs, observer, ni, nj, flow; emission = nothing, lambda1 = nothing, max_steps = nothing, T = Float64, ctx = nothing)
        -> ((R, G, B), I, tau, tstatus, tsteps)

A frame with VOLUME EMISSION (`rtgr_trace_transfer_f64/_f32`) — an extension: the frame of `trace_rays_observer` (with `emission`, an
emitting disk, if given), then the transfer equations of `flow` integrated along every ray as far as the trace followed it:
`rgb = rgb exp(-tau) + gain weight I`.  `I`, `tau` are `ni x nj`; `tstatus` (0 reached the ray's end, 1 r_stop, 2 step cap, 3 not
integrated or not finite: NaN) and `tsteps` (step attempts) likewise.  The observer's frame is asked for first: an invalid frame or a
refused record is an error.
"""
function trace_rays_transfer(metric, objs, observer::RtgrObserver, ni::Integer, nj::Integer, flow::RtgrFlow; emission = nothing, lambda1 = nothing,
                             max_steps = nothing, T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_rays_transfer has no CPU counterpart in the reference: ", why)
    opt = solver_with(T, lambda1, max_steps)
    obs = Ref(observer)
    fl = Ref(flow)
    emit = emission === nothing ? nothing : Ref(emission::RtgrDiskEmission)
    observer_frame(scene, obs; T = T, ctx = ctx)
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    g = Array{T}(undef, ni, nj)
    I = Array{T}(undef, ni, nj)
    tau = Array{T}(undef, ni, nj)
    tstatus = Array{UInt8}(undef, ni, nj)
    tsteps = Array{UInt32}(undef, ni, nj)
    ctr = Ref{RtgrCounters}()
    tctr = Ref{RtgrCounters}()
    GC.@preserve rgb g I tau tstatus tsteps emit begin
        pe = emit === nothing ? Ptr{RtgrDiskEmission}(C_NULL) : Base.unsafe_convert(Ptr{RtgrDiskEmission}, emit)
        pg = emit === nothing ? Ptr{T}(C_NULL) : pointer(g)
        if T === Float64
            check(ccall((:rtgr_trace_transfer_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission},
                         Ptr{RtgrFlow}, Ptr{Float64}, Ptr{RtgrRayOutputs}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{UInt32},
                         Ptr{RtgrCounters}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, pe, fl, pointer(rgb), C_NULL, pg, pointer(I), pointer(tau),
                        pointer(tstatus), pointer(tsteps), ctr, tctr))
        else
            check(ccall((:rtgr_trace_transfer_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission},
                         Ptr{RtgrFlow}, Ptr{Float32}, Ptr{RtgrRayOutputs}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{UInt32},
                         Ptr{RtgrCounters}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, ni, nj, C_NULL, pe, fl, pointer(rgb), C_NULL, pg, pointer(I), pointer(tau),
                        pointer(tstatus), pointer(tsteps), ctr, tctr))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), I, tau, tstatus, tsteps
end

"""
    eval_transfer(metric, objs, flow, s0, lambda_end; lambda1 = nothing, max_steps = nothing, ctx = nothing) -> (I, tau, s_end, tstatus, tsteps)

The transfer kernel itself over `n` listed rays (`rtgr_eval_transfer_f64/_f32`, blocking): `s0` (`8 x n`) their start states,
`lambda_end` (`n`) how far each is integrated; u_obs is the static observer at each ray's start.  `s_end` is `8 x n`.
"""
function eval_transfer(metric, objs, flow::RtgrFlow, s0::Matrix{T}, lambda_end::Vector{T}; lambda1 = nothing, max_steps = nothing,
                       ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("eval_transfer: ", why)
    size(s0, 1) == 8 && size(s0, 2) == length(lambda_end) || error("eval_transfer: s0 must be 8 x n and lambda_end of length n")
    n = size(s0, 2)
    opt = solver_with(T, lambda1, max_steps)
    fl = Ref(flow)
    I = Array{T}(undef, n); tau = Array{T}(undef, n); s_end = Array{T}(undef, 8, n)
    tstatus = Array{UInt8}(undef, n); tsteps = Array{UInt32}(undef, n)
    GC.@preserve s0 lambda_end I tau s_end tstatus tsteps begin
        if T === Float64
            check(ccall((:rtgr_eval_transfer_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrFlow}, Ptr{RtgrObserver}, Ptr{Float64}, Ptr{Float64}, UInt64, Ptr{Float64},
                         Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}, Ptr{UInt32}),
                        handle(ctx), scene, opt, fl, C_NULL, pointer(s0), pointer(lambda_end), n, pointer(I), pointer(tau), pointer(s_end),
                        pointer(tstatus), pointer(tsteps)))
        else
            check(ccall((:rtgr_eval_transfer_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrFlow}, Ptr{RtgrObserver}, Ptr{Float32}, Ptr{Float32}, UInt64, Ptr{Float32},
                         Ptr{Float32}, Ptr{Float32}, Ptr{UInt8}, Ptr{UInt32}),
                        handle(ctx), scene, opt, fl, C_NULL, pointer(s0), pointer(lambda_end), n, pointer(I), pointer(tau), pointer(s_end),
                        pointer(tstatus), pointer(tsteps)))
        end
    end
    I, tau, s_end, tstatus, tsteps
end

"""
    DiskOrders(max_order; transmission = 1, margin = 0) -> RtgrDiskOrders

How far rays are followed through the emitting disk (include/rtgr.h "higher-order disk images"): orders `1 .. max_order` (at most 8) are
looked for; order `k` adds `transmission^k` times its emission to the picture (1: an optically thin disk, 0: the opaque one); `margin`:
how far the disk is inflated for the crossing legs (0: half its half thickness).
"""
function DiskOrders(max_order::Integer; transmission::Real = 1, margin::Real = 0)
    RtgrDiskOrders(UInt32(max_order), UInt32(0), Float64(margin), Float64(transmission), UInt64(0))
end

"""
    trace_rays_orders(metric, objs, observer, ni, nj, emission, orders; T = Float64, ctx = nothing)
        -> ((R, G, B), count, hit32, state_end, g, rgb_order, state0)

The emitting disk seen ORDER BY ORDER (`rtgr_trace_orders_f64/_f32`) — an extension: the frame of `trace_rays_observer` with `emission`
(order 0), then every ray that ended on the disk carried through it and traced on; where it meets the disk again is the next order —
order 1 the lensed far side and underside, order >= 2 the photon ring.  `(R, G, B)` is the sum over orders weighted `transmission^k`;
`count` (`ni x nj`) the disk crossings per pixel; the per-order planes `hit32` (`ni x nj x (N+1)`), `state_end` (`8 x ni x nj x (N+1)`),
`g` (`ni x nj x (N+1)`) and `rgb_order` (`ni x nj x 3 x (N+1)`) hold block 0 = the observer frame and, for `k >= 1`, NaN / 0 where the
pixel has no order `k`; `state0` (`8 x ni x nj`) the rays' start states.  The observer's frame is asked for first: an invalid frame or a
refused record is an error.
"""
function trace_rays_orders(metric, objs, observer::RtgrObserver, ni::Integer, nj::Integer, emission::RtgrDiskEmission, orders::RtgrDiskOrders;
                           T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_rays_orders has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    obs = Ref(observer)
    emit = Ref(emission)
    ord = Ref(orders)
    observer_frame(scene, obs; T = T, ctx = ctx)
    nb = Int(orders.max_order) + 1
    rgb = Array{T}(undef, ni, nj, 3)                # plane-major: rgb[:, :, c] is plane c
    count = Array{UInt8}(undef, ni, nj)
    hit32 = Array{UInt32}(undef, ni, nj, nb)
    state_end = Array{T}(undef, 8, ni, nj, nb)
    g = Array{T}(undef, ni, nj, nb)
    rgb_order = Array{T}(undef, ni, nj, 3, nb)
    state0 = Array{T}(undef, 8, ni, nj)
    ctr = Ref{RtgrCounters}()
    GC.@preserve rgb count hit32 state_end g rgb_order state0 begin
        planes = Ref(RtgrOrderPlanes(pointer(count), pointer(hit32), Ptr{Cvoid}(pointer(state_end)), Ptr{Cvoid}(pointer(g)),
                                     Ptr{Cvoid}(pointer(rgb_order)), Ptr{Cvoid}(pointer(state0))))
        if T === Float64
            check(ccall((:rtgr_trace_orders_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, Ptr{Float64}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission},
                         Ptr{RtgrDiskOrders}, Ptr{Float64}, Ptr{RtgrOrderPlanes}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, C_NULL, ni, nj, C_NULL, emit, ord, pointer(rgb), planes, ctr))
        else
            check(ccall((:rtgr_trace_orders_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{RtgrObserver}, Ptr{Float32}, UInt64, UInt64, Ptr{RtgrShade}, Ptr{RtgrDiskEmission},
                         Ptr{RtgrDiskOrders}, Ptr{Float32}, Ptr{RtgrOrderPlanes}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, obs, C_NULL, ni, nj, C_NULL, emit, ord, pointer(rgb), planes, ctr))
        end
    end
    (rgb[:, :, 1], rgb[:, :, 2], rgb[:, :, 3]), count, hit32, state_end, g, rgb_order, state0
end

"""
    render_frames(metric, objs, cams, ni, nj; T = Float64, ctx = nothing) -> Vector{NTuple{3,Matrix{T}}}

SEVERAL frames of one scene in ONE call (`rtgr_trace_frames_f64/_f32`), two in flight inside the library: frame `k` from the camera
`cams[k] = (pos, widthx, widthy, normal)` (rays generated on the device), returned as its three `ni x nj` planes.  An extension — the
reference renders one frame per call (`example1`, `example2`, src/RayTraceGR.jl:560, :596): a render loop's frames end thin (the last
rays of a pass, the last download), and with two in flight the thin end of one overlaps the start of the next (8-11 % per frame at
1024², INTEGRATION.md "Frames in flight").  Each frame is the frame `render` gives for that camera, bit for bit.
"""
function render_frames(metric, objs, cams::AbstractVector, ni::Integer, nj::Integer; T::Type = Float64, ctx = nothing)
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("render_frames has no CPU counterpart in the reference: ", why)
    opt = solver_of(T)
    K = length(cams)
    packed = RtgrCamera[camera_of(c...)[] for c in cams]
    rgb = [Array{T}(undef, ni, nj, 3) for _ in 1:K]      # plane-major, frame by frame
    ptrs = Ptr{T}[pointer(a) for a in rgb]
    ctrs = Vector{RtgrCounters}(undef, K)
    GC.@preserve rgb begin
        if T === Float64
            check(ccall((:rtgr_trace_frames_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, UInt32, Ptr{RtgrCamera}, Ptr{Ptr{Float64}}, UInt64, UInt64, Ptr{Ptr{Float64}},
                         Ptr{RtgrRayOutputs}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, K, packed, C_NULL, ni, nj, ptrs, C_NULL, ctrs))
        else
            check(ccall((:rtgr_trace_frames_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, UInt32, Ptr{RtgrCamera}, Ptr{Ptr{Float32}}, UInt64, UInt64, Ptr{Ptr{Float32}},
                         Ptr{RtgrRayOutputs}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, K, packed, C_NULL, ni, nj, ptrs, C_NULL, ctrs))
        end
    end
    [(a[:, :, 1], a[:, :, 2], a[:, :, 3]) for a in rgb]
end

"""
    trace_rays_frames(metric, objs, canvases::Vector{Canvas{T}}; ctx = nothing) -> Vector{Canvas{T}}

`trace_rays` over several canvases in one call, two in flight (`rtgr_trace_frames_pixels_f64/_f32`): each canvas's own `Pixel{T}`
array goes across the ABI as in `trace_rays`, all of the same size.  Falls back — loudly — to a loop of the reference's `trace_rays`
where the scene cannot cross the ABI.
"""
function trace_rays_frames(metric, objs::Vector{RayTraceGR.Object{T}}, canvases::Vector{RayTraceGR.Canvas{T}}; ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, objs, ctx)
    if scene === nothing
        cpu_fallback("trace_rays", why)
        return [RayTraceGR.trace_rays(metric, objs, c) for c in canvases]
    end
    isempty(canvases) && return RayTraceGR.Canvas{T}[]
    ni, nj = size(canvases[1].pixels)
    all(c -> size(c.pixels) == (ni, nj), canvases) || error("trace_rays_frames: the canvases must have one size")
    opt = solver_of(T)
    outs = [similar(c.pixels) for c in canvases]
    pin = Ptr{Cvoid}[pointer(c.pixels) for c in canvases]
    pout = Ptr{Cvoid}[pointer(o) for o in outs]
    ctrs = Vector{RtgrCounters}(undef, length(canvases))
    GC.@preserve canvases outs begin
        if T === Float64
            check(ccall((:rtgr_trace_frames_pixels_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, UInt32, Ptr{Ptr{Cvoid}}, UInt64, UInt64, Ptr{Ptr{Cvoid}}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, length(canvases), pin, ni, nj, pout, ctrs))
        else
            check(ccall((:rtgr_trace_frames_pixels_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, UInt32, Ptr{Ptr{Cvoid}}, UInt64, UInt64, Ptr{Ptr{Cvoid}}, Ptr{RtgrCounters}),
                        handle(ctx), scene, opt, length(canvases), pin, ni, nj, pout, ctrs))
        end
    end
    [RayTraceGR.Canvas{T}(o) for o in outs]
end

"""
    trace_ray(metric, objs, cb, p::Pixel{T}; ctx = nothing) -> Pixel{T}

Legacy single-pixel shape (test/runtests.jl:76).  `cb` is ignored: the callback is always
`ContinuousCallback(min_distance(objs, ·), terminate!)` (src/RayTraceGR.jl:488-490).
"""
function trace_ray(metric, objs::Vector{RayTraceGR.Object{T}}, cb, p::RayTraceGR.Pixel{T}; ctx = nothing) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, objs, ctx)
    scene === nothing && error("trace_ray: ", why)
    opt = solver_of(T)
    pos, nrm = Ref(p.pos), Ref(p.normal)
    rgb = Ref(zeros(SVector{3,T})); se = Ref(zeros(SVector{8,T})); st = Ref{UInt8}(0)
    if T === Float64
        check(ccall((:rtgr_trace_one_f64, librtgr), Cint,
                    (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}),
                    handle(ctx), scene, opt, pos, nrm, rgb, se, st))
    else
        check(ccall((:rtgr_trace_one_f32, librtgr), Cint,
                    (Ctx, Ptr{RtgrScene}, Ptr{RtgrSolver}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{UInt8}),
                    handle(ctx), scene, opt, pos, nrm, rgb, se, st))
    end
    RayTraceGR.Pixel{T}(p.pos, p.normal, rgb[])
end

# ---- the reference's unit-test surface on the device (test/runtests.jl:12-61) --------------------------------------------
"""
    dmetric(metric, x::SVector{4,T}; ctx = nothing) -> (g::SMatrix{4,4,T}, dg::SArray{Tuple{4,4,4},T})
    christoffel(metric, x; ctx = nothing) -> Γ::SArray{Tuple{4,4,4},T}
    metric_at(metric, x; ctx = nothing) -> g

`RayTraceGR.dmetric` (:302-313) and `christoffel` (:321-331) evaluated by the device's dual-number path
(`rtgr_eval_metric_f64/_f32`) — what test/runtests.jl:12-61 exercises, `T = Float32` at :37.  The C arrays are row-major
`g[a][b]`, `dg[a][b][c] = ∂_c g_ab`, `Gam[a][b][c] = Γ^a_bc`; Julia's column-major view of the same bytes has the indices
reversed, hence the `permutedims`.
"""
function eval_metric(metric, x::SVector{4,T}, ctx) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, RayTraceGR.Object{T}[], ctx)
    scene === nothing && error("eval_metric: ", why)
    xs = collect(x)
    g = Array{T}(undef, 4, 4); dg = Array{T}(undef, 4, 4, 4); Γ = Array{T}(undef, 4, 4, 4)
    GC.@preserve xs g dg Γ begin
        if T === Float64
            check(ccall((:rtgr_eval_metric_f64, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{Float64}, UInt64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                        handle(ctx), scene, pointer(xs), 1, pointer(g), pointer(dg), pointer(Γ)))
        else
            check(ccall((:rtgr_eval_metric_f32, librtgr), Cint,
                        (Ctx, Ptr{RtgrScene}, Ptr{Float32}, UInt64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                        handle(ctx), scene, pointer(xs), 1, pointer(g), pointer(dg), pointer(Γ)))
        end
    end
    SMatrix{4,4,T}(permutedims(g)), SArray{Tuple{4,4,4},T}(permutedims(dg, (3, 2, 1))), SArray{Tuple{4,4,4},T}(permutedims(Γ, (3, 2, 1)))
end
metric_at(metric, x; ctx = nothing) = eval_metric(metric, x, ctx)[1]
dmetric(metric, x; ctx = nothing) = eval_metric(metric, x, ctx)[1:2]
christoffel(metric, x; ctx = nothing) = eval_metric(metric, x, ctx)[3]

"""
    geodesic(s::SVector{8,T}, metric; ctx = nothing, path = 2) -> ṡ::SVector{8,T}

`RayTraceGR.geodesic(r, metric, λ)` (:358-370) on the device (`rtgr_eval_geodesic_f64/_f32`): `path = 1` is the reference's own
formulation (duals → christoffel → contraction), `path = 2` exactly the function the production integrate loop calls.
"""
function geodesic(s::SVector{8,T}, metric; ctx = nothing, path::Integer = 2) where {T<:Union{Float64,Float32}}
    scene, why = scene_of(metric, RayTraceGR.Object{T}[], ctx)
    scene === nothing && error("geodesic: ", why)
    si = collect(s); so = similar(si)
    GC.@preserve si so begin
        if T === Float64
            check(ccall((:rtgr_eval_geodesic_f64, librtgr), Cint, (Ctx, Ptr{RtgrScene}, Ptr{Float64}, UInt64, Cint, Ptr{Float64}),
                        handle(ctx), scene, pointer(si), 1, path, pointer(so)))
        else
            check(ccall((:rtgr_eval_geodesic_f32, librtgr), Cint, (Ctx, Ptr{RtgrScene}, Ptr{Float32}, UInt64, Cint, Ptr{Float32}),
                        handle(ctx), scene, pointer(si), 1, path, pointer(so)))
        end
    end
    SVector{8,T}(so)
end

# ---- example1() / example2() (src/RayTraceGR.jl:540-612): drop-in twins that write the same PNGs ---------------------------
const outdir = "scenes"

"8-bit image the way `save(file, colorview(RGB, R', G', B'))` quantises it (N0f8: round(clamp(v, 0, 1) * 255), :566-575): `3 x ni x nj`"
quantize(planes) = UInt8[round(UInt8, clamp(planes[c][i, j], 0, 1) * 255) for c in 1:3, i in 1:size(planes[1], 1), j in 1:size(planes[1], 2)]

function save_scene(file, planes)
    # Images / ImageIO are the reference's own dependency for this step (:3-6, :575); loaded here so that `using RayTraceGRHIP`
    # alone does not pull them in
    Images = Base.require(Base.PkgId(Base.UUID("916415d5-f1e6-5110-898d-aaa5f9f070e0"), "Images"))
    T = eltype(planes[1])
    scene = Images.colorview(Images.RGB, T.(planes[1])', T.(planes[2])', T.(planes[3])')     # :566-569
    mkpath(dirname(file))
    rm(file, force = true)
    println("Output file is \"$file\"")
    Images.save(file, scene)                                                                 # :575
end

function example_scene(::Type{T}, which::Int) where {T}
    caelum = RayTraceGR.Sphere{T}(SVector{4,T}(0, 0, 0, 0), SVector{4,T}(1, 0, 0, 0), -10)              # :546, :584
    frustum = RayTraceGR.Plane{T}(-20)                                                                 # :547, :585
    centre = which == 1 ? SVector{4,T}(0, 0, 0, 0) : SVector{4,T}(0, 4, 0, 0)                          # :548, :586
    sphere = RayTraceGR.Sphere{T}(centre, SVector{4,T}(1, 0, 0, 0), T(1) / 2)
    objs = RayTraceGR.Object{T}[caelum, frustum, sphere]
    pos = which == 1 ? SVector{4,T}(0, 0, -2, 0) : SVector{4,T}(0, 4, -2, 0)                           # :554, :592
    objs, pos, SVector{4,T}(0, 1, 0, 0), SVector{4,T}(0, 0, 0, 1), SVector{4,T}(0, 0, 1, 0)            # widthx, widthy, normal
end

"""
    example1(; T = Float64, ni = 200, nj = 200, ctx = nothing, file = "scenes/sphere.png") -> Canvas{T}

`RayTraceGR.example1()` (:542-578) with `make_canvas` and `trace_rays` on the device: Minkowski, caelum + frustum + sphere,
the 200 x 200 screen — BASELINE config 1.  Writes the same PNG (39 855 of 40 000 pixels equal the committed `sphere.png`; the
rest is the silhouette ring, where the reference's own result depends on the last bit of the root-finder — SURVEY §4.2).
"""
function example1(; T::Type = Float64, ni::Int = 200, nj::Int = 200, ctx = nothing, file = joinpath(outdir, "sphere.png"))
    metric = RayTraceGR.minkowski
    objs, pos, widthx, widthy, normal = example_scene(T, 1)
    canvas = make_canvas(metric, pos, widthx, widthy, normal, ni, nj; ctx = ctx)
    canvas = trace_rays(metric, objs, canvas; ctx = ctx)
    file === nothing || save_scene(file, ntuple(c -> T[p.rgb[c] for p in canvas.pixels], 3))
    canvas
end

"""
    example2(; T = Float64, ni = 200, nj = 200, metric = kerr_schild, ctx = nothing, file = "scenes/sphere2.png") -> Canvas{T}

`RayTraceGR.example2()` (:580-612): Kerr–Schild, three objects.  Defaults reproduce the committed `sphere2.png` byte for byte.
BASELINE config 2: `example2(ni = 1024, nj = 1024, metric = KerrSchild(1.0, 0.8))`;
config 4: `example2(T = Float32, ni = 2048, nj = 2048, metric = KerrSchild(1.0, 0.8))`.
"""
function example2(; T::Type = Float64, ni::Int = 200, nj::Int = 200, metric = RayTraceGR.kerr_schild, ctx = nothing,
                  file = joinpath(outdir, "sphere2.png"))
    objs, pos, widthx, widthy, normal = example_scene(T, 2)
    canvas = make_canvas(metric, pos, widthx, widthy, normal, ni, nj; ctx = ctx)
    canvas = trace_rays(metric, objs, canvas; ctx = ctx)
    file === nothing || save_scene(file, ntuple(c -> T[p.rgb[c] for p in canvas.pixels], 3))
    canvas
end

"""
    example_disk(; a = 0.998, ni = 8192, nj = 8192, T = Float64, ctx = nothing, file = "scenes/disk.png") -> (R, G, B)

BASELINE config 5: near-extremal Kerr (`KerrSchild(1.0, a)`, textbook radius) with a thin accretion disk
`Disk(0.05, 2, 4)` in place of example2's small sphere (the camera, at cylindrical radius 4.5, stays outside the disk),
example2's camera, an 8192² screen — through `render` (camera on the device; an `Array{Pixel{Float64}}` of that size would be
5.9 GB each way).  The scene of `bench.py --variant ks_true0998_disk`.
"""
function example_disk(; a::Real = 0.998, ni::Int = 8192, nj::Int = 8192, T::Type = Float64, ctx = nothing,
                      file = joinpath(outdir, "disk.png"))
    objs, pos, widthx, widthy, normal = example_scene(T, 2)
    objs[3] = Disk{T}(T(0.05), T(2), T(4))
    planes = render(KerrSchild(1.0, a), objs, pos, widthx, widthy, normal, ni, nj; T = T, ctx = ctx)
    file === nothing || save_scene(file, planes)
    planes
end

end # module
