"""Host-side mirror of RayTraceGR.jl's interface for the hot path, over the C ABI of include/rtgr.h.

The reference's host language is Julia, which is absent from this image; this module plays the role of the thin
Julia `ccall` layer (julia/RayTraceGRHIP.jl ships the actual Julia stub): same names, argument meaning and error
behaviour as the reference's exported API, so tests read like the reference's own.

    reference (src/RayTraceGR.jl)                       here
    ------------------------------------------------   --------------------------------------------------
    minkowski, kerr_schild            :258-294          minkowski, kerr_schild  (+ KerrSchild(M, a, textbook))
    dmetric, christoffel, geodesic    :298-370          dmetric, christoffel, geodesic   (evaluated on the GPU)
    Object / Plane / Sphere           :374-428          Plane, Sphere (+ Disk); new subtypes: UserObjects(source)(type, fields)
    Pixel / Canvas / make_canvas      :445-478          Pixel (numpy record), Canvas, make_canvas
    trace_rays(metric, objs, canvas)  :482-536          trace_rays(metric, objs, canvas) -> Canvas
    trace_ray(metric, objs, cb, p)    test/runtests.jl:76   trace_ray(metric, objs, cb, p) -> Pixel
    example1(), example2()            :542-612          example1(), example2()  (write scenes/sphere*.png)

Nothing here computes physics on the CPU: every numeric result comes from librtgr_hip.so (HIP kernels).
"""
import ctypes as C
import math
import os

import numpy as np

from . import _abi
from ._abi import rtgr_camera, rtgr_counters, rtgr_ray_outputs, rtgr_scene, rtgr_solver
from .user_metric import UserMetric, UserObject, UserObjects

D = 4  # src/RayTraceGR.jl:253-254


# ---- metrics (callables only as identities: the ABI takes an enum) ---------------------------------
class Metric:
    """A built-in metric: enum + (M, a). Calling it evaluates g_ab(x) on the GPU (src/RayTraceGR.jl:262-294)."""

    def __init__(self, kind, M=1.0, a=0.0, name="metric", generic=False):
        self.kind, self.M, self.a, self.__name__ = int(kind), float(M), float(a), name
        self.generic = bool(generic)  # True: trace with the generic dual-number RHS (RTGR_METRIC_GENERIC)

    def __call__(self, x, dtype=np.float64):
        g, _, _ = _eval_metric(self, x, want=(True, False, False), dtype=dtype)
        return g

    def __repr__(self):
        return f"{self.__name__}(M={self.M}, a={self.a})"


minkowski = Metric(_abi.MINKOWSKI, name="minkowski")          # src/RayTraceGR.jl:262-264
kerr_schild = Metric(_abi.KS_REF, 1.0, 0.0, name="kerr_schild")  # as written: M=1, a=0 (:275-276), r of :284


def KerrSchild(M=1.0, a=0.0, textbook=True, generic=False):
    """Parameterised Kerr–Schild metric the reference describes (README "varying mass and spin") but does not
    have: textbook radius (RTGR_KS_TRUE) or the as-written radius with a != 0 (RTGR_KS_REF).  generic=True traces with
    the reference-style dual-number RHS instead of the closed contraction (same results, ~5x the flops)."""
    return Metric(_abi.KS_TRUE if textbook else _abi.KS_REF, M, a, name="KerrSchild", generic=generic)


_UPPER = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]   # tt tx ty tz xx xy xz yy yz zz


class GridMetric:
    """A metric given as SAMPLES on a uniform grid (RTGR_GRID, include/rtgr.h) — a numerically computed spacetime has no formula.
    Stationary, 3-D: g is a numpy array (nz, ny, nx, 10) of the upper triangle tt tx ty tz xx xy xz yy yz zz, or (nz, ny, nx, 4, 4)
    (the upper triangle is taken); origin = (x, y, z) of sample [0, 0, 0]; spacing = (hx, hy, hz) (a scalar: the same on every axis).
    Time-dependent, 4-D: g is (nt, nz, ny, nx, 10) or (nt, nz, ny, nx, 4, 4), time slowest; origin = (t, x, y, z), spacing =
    (ht, hx, hy, hz) (rtgr_grid4_metric_load).  Values and first derivatives are interpolated on the device (tri- / tetracubic
    Catmull-Rom) inside the integrate loop; rays that leave the valid box — in t too — end with status RAY_OUTSIDE.  Uploaded lazily,
    once per context; calling it evaluates g on the GPU."""
    kind = _abi.GRID
    generic = False   # (grids always take the generic contraction; the scene's metric is plain RTGR_GRID)
    M = a = 0.0

    def __init__(self, g, origin, spacing, name="grid"):
        g = np.asarray(g)
        four = g.ndim == 6 or (g.ndim == 5 and g.shape[-1] == 10)   # (nt, nz, ny, nx, 4, 4) or (nt, nz, ny, nx, 10)
        if g.ndim == (6 if four else 5) and g.shape[-2:] == (4, 4):
            g = np.stack([g[..., p, q] for p, q in _UPPER], axis=-1)
        dims = 4 if four else 3
        if g.ndim != dims + 1 or g.shape[-1] != 10:
            raise ValueError(f"GridMetric: g must have shape (nz, ny, nx, 10), (nz, ny, nx, 4, 4), (nt, nz, ny, nx, 10) or "
                             f"(nt, nz, ny, nx, 4, 4), got {np.shape(g)}")
        if min(g.shape[:dims]) < 4:
            raise ValueError(f"GridMetric: at least 4 samples per axis, got {'(nt, nz, ny, nx)' if four else '(nz, ny, nx)'} = {g.shape[:dims]}")
        if math.prod(g.shape[:dims]) > _abi.RTGR_GRID_MAX_SAMPLES:
            raise ValueError("GridMetric: more than RTGR_GRID_MAX_SAMPLES samples")
        origin = np.broadcast_to(np.asarray(origin, np.float64), (dims,)).copy()
        spacing = np.broadcast_to(np.asarray(spacing, np.float64), (dims,)).copy()
        if not np.all(np.isfinite(origin)) or not np.all(np.isfinite(spacing)) or not np.all(spacing > 0):
            raise ValueError(f"GridMetric: origin must be finite and spacing finite and > 0, got {origin}, {spacing}")
        self.g = np.ascontiguousarray(g, dtype=np.float64)
        if not np.all(np.isfinite(self.g)):
            bad = int(np.flatnonzero(~np.isfinite(self.g).all(axis=-1).ravel())[0])
            raise ValueError(f"GridMetric: sample {bad} (x fastest) holds a non-finite value")
        self.origin, self.spacing, self.__name__ = origin, spacing, name
        self.time_dependent = four
        # in the order of origin / spacing: 3-D (nx, ny, nz), 4-D (nt, nx, ny, nz)
        self.n = ((g.shape[0],) + g.shape[3:0:-1]) if four else g.shape[2::-1]
        self._ids = {}

    def box(self):
        """the valid box, samples 1 .. n-2 of every axis: ((x0, x1), (y0, y1), (z0, z1)), 4-D: ((t0, t1), (x0, x1), (y0, y1), (z0, z1))"""
        return tuple((self.origin[a] + self.spacing[a], self.origin[a] + (self.n[a] - 2) * self.spacing[a]) for a in range(len(self.n)))

    def module_id(self, ctx=None):
        """id of this grid in the context (uploaded on first use)"""
        key = getattr(ctx, "value", ctx)
        gid = self._ids.get(key)
        if gid is not None:
            return gid
        lib = _lib()
        out = C.c_uint64(0)
        if self.time_dependent:
            desc = _abi.rtgr_grid4()
            for a in range(4):
                desc.n[a], desc.origin[a], desc.spacing[a] = self.n[a], self.origin[a], self.spacing[a]
            _abi.check(lib, lib.rtgr_grid4_metric_load(ctx, C.byref(desc), self.g.ctypes.data, C.byref(out)))
        else:
            desc = _abi.rtgr_grid()
            for a in range(3):
                desc.n[a], desc.origin[a], desc.spacing[a] = self.n[a], self.origin[a], self.spacing[a]
            _abi.check(lib, lib.rtgr_grid_metric_load(ctx, C.byref(desc), self.g.ctypes.data, C.byref(out)))
        self._ids[key] = out.value
        return out.value

    def unload(self, ctx=None):
        """release this grid's id in the context (the device memory goes at the next rtgr_trim)"""
        gid = self._ids.pop(getattr(ctx, "value", ctx), None)
        if gid is not None:
            _abi.check(_lib(), _lib().rtgr_grid_metric_unload(ctx, gid))

    def __call__(self, x, dtype=np.float64):
        return _eval_metric(self, x, want=(True, False, False), dtype=dtype)[0]

    def __repr__(self):
        return f"GridMetric({self.__name__}, n={self.n}, origin={tuple(self.origin)}, spacing={tuple(self.spacing)})"


def sample_metric(metric, origin, spacing, n, chunk=1 << 20, t=None):
    """Samples any metric the library evaluates (built-in, UserMetric, GridMetric) on a uniform grid through rtgr_eval_metric_f64:
    n = (nx, ny, nz) points from origin with spacing (scalar or per axis), at t = 0.  Returns the (nz, ny, nx, 10) array GridMetric
    takes.  Evaluated in chunks of `chunk` points.
    t = (t0, ht, nt): a time axis as well — the metric at the 4-D points (t0 + l ht, x, y, z); returns (nt, nz, ny, nx, 10)."""
    nx, ny, nz = (int(v) for v in n)
    origin = np.broadcast_to(np.asarray(origin, np.float64), (3,))
    spacing = np.broadcast_to(np.asarray(spacing, np.float64), (3,))
    z, y, x = np.meshgrid(*(origin[a] + spacing[a] * np.arange(m) for a, m in ((2, nz), (1, ny), (0, nx))), indexing="ij")
    times = [0.0]
    if t is not None:
        t0, ht, nt = float(t[0]), float(t[1]), int(t[2])
        if nt < 1 or not np.isfinite(t0) or not np.isfinite(ht):
            raise ValueError(f"sample_metric: t must be (t0, ht, nt) with nt >= 1, got {t}")
        times = t0 + ht * np.arange(nt)
    out = np.empty((len(times), x.size, 10))
    for l, tl in enumerate(times):
        pts = np.stack([np.full(x.size, tl), x.ravel(), y.ravel(), z.ravel()], axis=1)
        for s0 in range(0, pts.shape[0], chunk):
            g, _, _ = _eval_metric(metric, pts[s0:s0 + chunk], want=(True, False, False))
            g = g.reshape(-1, 4, 4)
            out[l, s0:s0 + chunk] = np.stack([g[:, p, q] for p, q in _UPPER], axis=1)
    if t is None:
        return out[0].reshape(nz, ny, nx, 10)
    return out.reshape(len(times), nz, ny, nx, 10)


# ---- objects (src/RayTraceGR.jl:374-428) ------------------------------------------------------------------------
class Object:
    kind = 0

    def _pack(self):
        raise NotImplementedError("Called distance on abstract object")  # :384-386


class Plane(Object):
    """Plane{T}(time)  src/RayTraceGR.jl:394-397"""
    kind = _abi.PLANE

    def __init__(self, time):
        self.time = float(time)

    def _pack(self):
        return [self.time] + [0.0] * 8


class Sphere(Object):
    """Sphere{T}(pos, vel, radius)  src/RayTraceGR.jl:409-413 (vel is stored and unused, as in the reference)"""
    kind = _abi.SPHERE

    def __init__(self, pos, vel, radius):
        self.pos = [float(v) for v in pos]
        self.vel = [float(v) for v in vel]
        self.radius = float(radius)
        assert len(self.pos) == D and len(self.vel) == D

    def _pack(self):
        return self.pos + self.vel + [self.radius]


class Disk(Object):
    """Thin disk |z| <= h, r_in <= sqrt(x^2+y^2) <= r_out. No reference counterpart (BASELINE config 5)."""
    kind = _abi.DISK

    def __init__(self, half_thickness, r_in, r_out):
        self.h, self.r_in, self.r_out = float(half_thickness), float(r_in), float(r_out)

    def _pack(self):
        return [self.h, self.r_in, self.r_out] + [0.0] * 6


def make_scene(metric, objs, ctx=None, units=True):
    """(metric, objs::Vector{Object}) -> rtgr_scene (order of objs preserved: it matters, :518-530).  A scene of a
    UserMetric and / or of UserObjects carries the id of its run-time unit in `ctx` (built and loaded on first use), so it
    can only ever run with its own kernels — whichever other units are resident.  units=False leaves the id 0 and touches
    neither compiler nor GPU (a scene description for something else than this library: the tests' CPU oracle)."""
    if not isinstance(metric, (Metric, UserMetric, GridMetric)):
        raise TypeError(
            "a metric is one of the built-ins (minkowski, kerr_schild, KerrSchild(M,a)), a UserMetric(source) "
            "compiled for the device or a GridMetric of samples; "
            "a Python callable cannot cross the C ABI (SURVEY §8b)")
    objs = list(objs)
    if len(objs) > _abi.RTGR_OBJECTS_LIMIT:
        raise ValueError(f"at most {_abi.RTGR_OBJECTS_LIMIT} objects")
    # New Object subtypes (src/RayTraceGR.jl:374-389) come as a UserObjects family: its distance / objcolor methods are compiled
    # into ONE unit together with the metric they are traced with (compiled code holds both in the same kernels); the sources of
    # several families are joined into one first (UserObjects.join: type tags renumbered family after family, in the order of
    # first appearance in objs)
    families = list({id(o.family): o.family for o in objs if isinstance(o, UserObject)}.values())
    base = {id(f): 0 for f in families}
    if len(families) > 1:
        joined, bases = UserObjects.join(families)
        base = {id(f): b for f, b in zip(families, bases)}
        families = [joined]
    user_id = 0
    if isinstance(metric, GridMetric) and any(isinstance(o, UserObject) for o in objs):
        raise ValueError("user objects in a scene with a GridMetric are not supported")
    if not units:
        pass
    elif isinstance(metric, GridMetric):
        user_id = metric.module_id(ctx)
    elif families:
        user_id = families[0].unit_id(metric, ctx)
    elif isinstance(metric, UserMetric):
        user_id = metric.module_id(ctx)
    sc = rtgr_scene()
    sc.metric = metric.kind | (_abi.METRIC_GENERIC if metric.generic else 0)
    sc.nobj, sc.M, sc.a = len(objs), metric.M, metric.a
    sc.user_metric = user_id
    # `objs::Vector{Object{T}}` of any length (:433-441): up to RTGR_MAX_OBJECTS in the scene's inline slots, a longer list as one array
    # behind rtgr_scene.objects (kept alive by the scene: sc._keep)
    slots = sc.obj
    if len(objs) > _abi.RTGR_MAX_OBJECTS:
        slots = sc._keep = (_abi.rtgr_object * len(objs))()
        sc.objects = C.cast(slots, C.POINTER(_abi.rtgr_object))
    for o, obj in enumerate(objs):
        slots[o].kind = obj.kind
        slots[o].type = getattr(obj, "type", 0) + (base[id(obj.family)] if isinstance(obj, UserObject) else 0)
        p = obj._pack()
        for q in range(9):
            slots[o].p[q] = p[q]
    return sc


def eval_objects(metric, objs, x, opt=None, dtype=np.float64, ctx=None):
    """distance(obj, x) of every object, min_distance(objs, x) and the colouring rule of trace_rays at the points x [n, 4], on the
    GPU (rtgr_eval_objects_*; src/RayTraceGR.jl:377-441, :513-533) -> dict(d [n, nobj], dmin [n], hit [n], rgb [n, 3])"""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    x = np.ascontiguousarray(x, dtype=dtype).reshape(-1, 4)
    n = x.shape[0]
    opt = opt or solver_defaults(dtype)
    out = dict(d=np.zeros((n, max(sc.nobj, 1)), dtype), dmin=np.zeros(n, dtype), hit=np.zeros(n, np.uint8), rgb=np.zeros((n, 3), dtype))
    fn = lib.rtgr_eval_objects_f64 if dtype == np.float64 else lib.rtgr_eval_objects_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), x.ctypes.data, n, out["d"].ctypes.data, out["dmin"].ctypes.data,
                       out["hit"].ctypes.data, out["rgb"].ctypes.data))
    out["d"] = out["d"][:, :sc.nobj]
    return out


def check_scene(metric, objs, cam, ni=48, nj=48, opt=None, ctx=None):
    """rtgr_scene_check: the FAR + NEAR passes of THIS scene must deliver the frame of the single FULL pass (every accepted step
    scanned, as the reference does) — the check that catches a rtgr_user_reach that is not an upper bound.  `cam`: make_camera
    arguments (dict) or an rtgr_camera.  Raises RtgrError naming the number of rays that differ; returns None when the frames agree."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    camera = _camera(cam)
    opt = opt or solver_defaults()
    _abi.check(lib, lib.rtgr_scene_check(ctx, C.byref(sc), C.byref(opt), C.byref(camera), ni, nj, 0))


def solver_defaults(dtype=np.float64, **over):
    """tol = eps(T)^(3/4), λ∈[0,100], hit threshold 0.01, miss colour (1,0,0)  (src/RayTraceGR.jl:485,:497,:519,:528).
    Pure constants — filled here so that building a solver struct does not need the GPU library."""
    s = rtgr_solver()
    tol = float(np.finfo(dtype).eps) ** 0.75
    s.reltol = s.abstol = tol
    s.lambda0, s.lambda1 = 0.0, 100.0
    s.hit_threshold = 0.01
    s.miss_rgb[0], s.miss_rgb[1], s.miss_rgb[2] = 1.0, 0.0, 0.0
    s.max_steps = 100000
    s.interp_points = 10
    for k, v in over.items():
        if k == "miss_rgb":
            for c in range(3):
                s.miss_rgb[c] = float(v[c])
        else:
            setattr(s, k, v)
    return s


def make_camera(pos, widthx, widthy, normal):
    cam = rtgr_camera()
    for a in range(D):
        cam.pos[a], cam.widthx[a], cam.widthy[a], cam.normal[a] = (float(pos[a]), float(widthx[a]),
                                                                   float(widthy[a]), float(normal[a]))
    return cam


def _camera(cam):
    """make_camera arguments (a dict) or an rtgr_camera -> rtgr_camera"""
    return cam if isinstance(cam, rtgr_camera) else make_camera(**cam)


# ---- Pixel / Canvas (src/RayTraceGR.jl:445-455) -----------------------------------------------------------------
def pixel_dtype(dtype=np.float64):
    """Pixel{T}: pos (4), normal (4), rgb (3) — isbits, 88 bytes for Float64 (:446-450)."""
    return np.dtype([("pos", dtype, 4), ("normal", dtype, 4), ("rgb", dtype, 3)])


def Pixel(pos, normal, rgb=(0.0, 0.0, 0.0), dtype=np.float64):
    p = np.zeros((), dtype=pixel_dtype(dtype))
    p["pos"], p["normal"], p["rgb"] = pos, normal, rgb
    return p


class Canvas:
    """Canvas{T}(pixels::Array{Pixel{T},2}) — `pixels` is stored column-major like Julia: pixels[i, j] with i fastest
    (numpy array of shape (ni, nj), order='F')."""

    def __init__(self, pixels):
        self.pixels = pixels

    @property
    def shape(self):
        return self.pixels.shape

    def rgb_planes(self):
        """(R, G, B) each (ni, nj) — what `T[p.rgb[c] for p in canvas.pixels]` yields (:566-569)."""
        return tuple(np.asfortranarray(self.pixels["rgb"][..., c]) for c in range(3))

    def image_u8(self):
        """8-bit image[j, i, c] as `save(file, colorview(RGB, R', G', B'))` writes it (:566-575; N0f8 rounding)."""
        rgb = np.stack(self.rgb_planes(), axis=-1)  # [i, j, c]
        img = np.rint(np.clip(rgb, 0.0, 1.0) * 255.0).astype(np.uint8)
        return np.ascontiguousarray(np.transpose(img, (1, 0, 2)))


def _lib():
    lib = _abi.load()
    return lib


def _ray_details(res, n, dtype, nobj):
    """`details`: the per-ray output arrays of n rays into `res`, bound into the rtgr_ray_outputs returned (a list of more than 255
    objects: `hit` is 32 bits wide and goes where the library calls it hit32)."""
    outs = rtgr_ray_outputs()
    wide = nobj > 255
    res.update(state_end=np.zeros((n, 8), dtype), lambda_end=np.zeros(n, dtype), status=np.zeros(n, np.uint8),
               hit=np.zeros(n, np.uint32 if wide else np.uint8), n_accept=np.zeros(n, np.uint32), n_reject=np.zeros(n, np.uint32))
    for name in ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject"):
        setattr(outs, "hit32" if (wide and name == "hit") else name, res[name].ctypes.data)
    return outs


def _aa_arg(aa, res, n):
    """The `aa` argument of a frame — None, dict(k=…, contrast=…, max_batch_rays=…) or an rtgr_aa — as the library takes it:
    -> (rtgr_aa, the address of res["refined"] (added here), rtgr_aa_stats), or three None"""
    if aa is None:
        return None, None, None
    aap = aa if isinstance(aa, _abi.rtgr_aa) else _abi.rtgr_aa(k=int(aa.get("k", 4)), flags=0, contrast=float(aa.get("contrast", 1.0 / 255.0)),
                                                                 max_batch_rays=int(aa.get("max_batch_rays", 0)))
    res["refined"] = np.zeros(n, np.uint8)
    return aap, res["refined"].ctypes.data, _abi.rtgr_aa_stats()


def make_canvas(metric, pos, widthx, widthy, normal, ni, nj, dtype=np.float64, ctx=None):
    """make_canvas(metric, pos, widthx, widthy, normal, ni, nj)::Canvas{T}  (src/RayTraceGR.jl:457-478), on the GPU.
    `dtype` plays the reference's type parameter T (np.float64 or np.float32)."""
    lib = _lib()
    sc = make_scene(metric, [], ctx)
    cam = make_camera(pos, widthx, widthy, normal)
    st = np.empty((ni * nj, 8), dtype=dtype)
    fn = lib.rtgr_make_canvas_f64 if dtype == np.float64 else lib.rtgr_make_canvas_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(cam), ni, nj, 0, nj, st.ctypes.data))
    px = np.zeros((ni, nj), dtype=pixel_dtype(dtype), order="F")
    flat = px.reshape(-1, order="F")
    flat["pos"] = st[:, :4]
    flat["normal"] = st[:, 4:]
    return Canvas(px)


def _canvas_scalar(px_dtype):
    for t in (np.float64, np.float32):
        if px_dtype == pixel_dtype(t):
            return t
    raise TypeError("Canvas{Float64} or Canvas{Float32} expected")


def trace_rays(metric, objs, c, opt=None, return_info=False, ctx=None):
    """trace_rays(metric, objs, c::Canvas{T})::Canvas{T}  (src/RayTraceGR.jl:482-536), T = Float64 or Float32.

    Passes the reference's own AoS pixel array across the ABI (rtgr_trace_pixels_f64 / _f32) and returns a NEW canvas
    with pos/normal copied and rgb set (:532).  Pure, like the reference.  The tolerance is eps(T)^(3/4) (:485).
    `ctx`: an rtgr_context handle (_abi.create_context); on a context of several devices the image rows are dealt
    cyclically to ALL of them inside this one call (the reference's `Threads.@threads` loop, across GPUs)."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    ni, nj = c.pixels.shape
    pin = np.asfortranarray(c.pixels)
    t = _canvas_scalar(pin.dtype)
    opt = opt or solver_defaults(t)
    pout = np.empty_like(pin, order="F")
    ctr = rtgr_counters()
    fn = lib.rtgr_trace_pixels_f64 if t == np.float64 else lib.rtgr_trace_pixels_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), pin.ctypes.data, ni, nj, pout.ctypes.data, C.byref(ctr)))
    out = Canvas(pout)
    return (out, ctr.as_dict()) if return_info else out


def trace_frames(metric, objs, cams, ni, nj, opt=None, dtype=np.float64, ctx=None, details=False):
    """SEVERAL frames of one scene in one call, two in flight inside the library (rtgr_trace_frames_f64 / _f32) — an extension: the
    reference renders one frame per call (src/RayTraceGR.jl:560, :596).  cams: a list of make_camera argument dicts (or rtgr_camera);
    rays are generated on the device.  -> list of dict(rgb [3, ni*nj], counters (+ the per-ray outputs when details)), frame by frame:
    each the result of the single call (rtgr_trace_f64), bit for bit."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    K, n = len(cams), ni * nj
    carr = (rtgr_camera * K)(*[_camera(c) for c in cams])
    rgb = [np.zeros((3, n), dtype) for _ in range(K)]
    ptrs = (C.c_void_p * K)(*[r.ctypes.data for r in rgb])
    ctrs = (rtgr_counters * K)()
    outs, per = None, [dict() for _ in range(K)]
    if details:
        outs = (rtgr_ray_outputs * K)(*[_ray_details(per[k], n, dtype, sc.nobj) for k in range(K)])
    fn = lib.rtgr_trace_frames_f64 if dtype == np.float64 else lib.rtgr_trace_frames_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), K, carr, None, ni, nj, ptrs, outs, ctrs))
    return [dict(per[k], rgb=rgb[k], counters=ctrs[k].as_dict()) for k in range(K)]


def trace_aa(metric, objs, cam, ni, nj, k=4, contrast=1.0 / 255.0, opt=None, dtype=np.float64, ctx=None, details=False, max_batch_rays=0):
    """ADAPTIVE ANTI-ALIASING (rtgr_trace_aa_f64 / _f32) — an extension: the plain ni x nj frame of the camera, then k x k sub-rays for
    the pixels that differ from a 4-neighbour in hit, status or by more than `contrast` in a colour channel, averaged (box filter)
    back into the frame; every other pixel keeps the plain frame's bits.  contrast < 0: every pixel (uniform supersampling); math.inf:
    class edges only.  cam: make_camera arguments (dict) or an rtgr_camera.  -> dict(rgb [3, ni*nj], refined [ni*nj] (1 = refined),
    counters (both passes), stats (pixels, refined, sub_rays, batches); details: + the per-ray outputs of the PIXEL-CENTRE rays)."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    camera = _camera(cam)
    n = ni * nj
    res = dict(rgb=np.zeros((3, n), dtype))
    aa, refined, stats = _aa_arg(dict(k=k, contrast=contrast, max_batch_rays=max_batch_rays), res, n)
    outs = _ray_details(res, n, dtype, sc.nobj) if details else None
    ctr = rtgr_counters()
    fn = lib.rtgr_trace_aa_f64 if dtype == np.float64 else lib.rtgr_trace_aa_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), C.byref(camera), ni, nj, C.byref(aa), res["rgb"].ctypes.data, outs, refined,
                       C.byref(ctr), C.byref(stats)))
    res["counters"], res["stats"] = ctr.as_dict(), stats.as_dict()
    return res


# ---- image textures (include/rtgr.h "image textures") -------------------------------------------------------------------------
class Texture:
    """An image texture resident in a context (rtgr_texture_load): `id`, `width`, `height`; `unload()` releases the id (the device
    memory goes at the next rtgr_trim)."""

    def __init__(self, tid, width, height, ctx=None):
        self.id, self.width, self.height, self.ctx = int(tid), int(width), int(height), ctx

    def unload(self):
        texture_unload(self, self.ctx)

    def __repr__(self):
        return f"Texture(id={self.id:#x}, {self.width} x {self.height})"


def texture_load(array, ctx=None):
    """rtgr_texture_load: `array` is (3, height, width) — the three colour planes, column fastest, the layout of every `rgb` output
    (a traced ni x nj frame reshaped (3, nj, ni) is a texture as it stands) — or an image (height, width, 3).  -> Texture"""
    a = np.asarray(array, dtype=np.float64)
    if a.ndim == 3 and a.shape[0] != 3 and a.shape[2] == 3:
        a = np.moveaxis(a, 2, 0)
    if a.ndim != 3 or a.shape[0] != 3:
        raise ValueError(f"texture_load: need (3, height, width) planes or a (height, width, 3) image, got {np.shape(array)}")
    a = np.ascontiguousarray(a)
    lib = _lib()
    desc = _abi.rtgr_texture_desc(width=a.shape[2], height=a.shape[1], flags=0, pad=0)
    out = C.c_uint64(0)
    _abi.check(lib, lib.rtgr_texture_load(ctx, C.byref(desc), a.ctypes.data, C.byref(out)))
    return Texture(out.value, a.shape[2], a.shape[1], ctx)


def texture_unload(texture, ctx=None):
    """rtgr_texture_unload: a Texture or an id; 0: every texture of the context"""
    lib = _lib()
    _abi.check(lib, lib.rtgr_texture_unload(ctx, int(getattr(texture, "id", texture))))


def eval_texture(texture, points, filter=_abi.TEX_BILINEAR, disk_range=None, rgb=None, dtype=np.float64, ctx=None):
    """rtgr_eval_texture_f64 / _f32: the sampler at the points [n, 3] — directions d, or positions whose (x, y) are read when
    disk_range = (r_in, r_out) is given.  rgb [n, 3]: what a "no sample" point (a zero or non-finite d) keeps; default NaN.
    -> rgb [n, 3]"""
    lib = _lib()
    p = np.ascontiguousarray(points, dtype=dtype).reshape(-1, 3)
    n = p.shape[0]
    out = np.full((n, 3), np.nan, dtype) if rgb is None else np.ascontiguousarray(rgb, dtype=dtype).reshape(n, 3).copy()
    rng = None if disk_range is None else np.array(disk_range, dtype=dtype).reshape(2)
    fn = lib.rtgr_eval_texture_f64 if dtype == np.float64 else lib.rtgr_eval_texture_f32
    _abi.check(lib, fn(ctx, int(getattr(texture, "id", texture)), int(filter), p.ctypes.data, n, None if rng is None else rng.ctypes.data,
                       out.ctypes.data))
    return out


def make_shade(textures, r_escape=0.0):
    """{object: (texture, filter)} -> rtgr_shade (object: the 1-based index in the object list, 0 = rays that escape; a bare texture
    means bilinear).  The bind array is kept alive by the struct (sh._keep)."""
    items = list((textures or {}).items())
    binds = (_abi.rtgr_texture_bind * max(len(items), 1))()
    for k, (obj, tf) in enumerate(items):
        tex, filt = tf if isinstance(tf, (tuple, list)) else (tf, _abi.TEX_BILINEAR)
        binds[k].object, binds[k].filter, binds[k].texture = int(obj), int(filt), int(getattr(tex, "id", tex))
    sh = _abi.rtgr_shade(nbind=len(items), flags=0, bind=C.cast(binds, C.POINTER(_abi.rtgr_texture_bind)), r_escape=float(r_escape))
    sh._keep = binds
    return sh


def trace_shaded(metric, objs, cam, ni, nj, textures=None, r_escape=0.0, aa=None, opt=None, dtype=np.float64, ctx=None, details=False):
    """A frame with IMAGE TEXTURES (rtgr_trace_shaded_f64 / _f32) — an extension: the plain ni x nj frame of the camera, then the pixels
    whose object — or whose escape — has a texture bound get the texel's colour; every other pixel keeps the plain frame's bits.
    textures = {omin: (texture, filter), 0: …}: omin is the 1-based index in objs (what `hit` holds), 0 binds the rays that end
    without a hit at |x| >= r_escape (coloured by the direction they end with).  Spheres of either radius sign and Disks take
    textures.  aa: None, or dict(k=…, contrast=…, max_batch_rays=…) / an rtgr_aa — adaptive anti-aliasing of the shaded frame.
    -> dict(rgb [3, ni*nj], counters; aa: + refined, stats; details: + the per-ray outputs of the pixel-centre rays)."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    camera = _camera(cam)
    n = ni * nj
    sh = make_shade(textures, r_escape)
    res = dict(rgb=np.zeros((3, n), dtype))
    aap, refined, stats = _aa_arg(aa, res, n)
    outs = _ray_details(res, n, dtype, sc.nobj) if details else None
    ctr = rtgr_counters()
    fn = lib.rtgr_trace_shaded_f64 if dtype == np.float64 else lib.rtgr_trace_shaded_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), C.byref(camera), ni, nj, C.byref(sh), aap, res["rgb"].ctypes.data, outs, refined,
                       C.byref(ctr), stats))
    res["counters"] = ctr.as_dict()
    if stats is not None:
        res["stats"] = stats.as_dict()
    return res


# ---- disk emission (include/rtgr.h "disk emission") -----------------------------------------------------------------------------
HC_OVER_KB_NM = 1.438776877e7   # h c / k_B in nm K: theta_c = HC_OVER_KB_NM / lambda_c


def DiskEmission(object, T_in, p=0.75, orbit=+1, emitter="kepler", inner_edge=False, gain=1.0, wavelengths_nm=(700.0, 546.1, 435.8)):
    """An orbiting disk that glows as a black body -> rtgr_disk_emission.  object: the 1-based index of a Disk in objs (what `hit`
    holds).  emitter "kepler": gas on the circular geodesics of the scene's own metric, orbit = +1 (counter-clockwise seen from +z) or
    -1; "rigid": Omega = orbit everywhere (0: the static emitter).  T_em(rho) = T_in (rho / r_in)^(-p) [inner_edge: times
    (1 - sqrt(r_in / rho))^(1/4)] in kelvin; the three channels are Planck's law at wavelengths_nm, normalised so that the middle
    wavelength has weight 1: theta_c = h c / (lambda_c k_B), weight_c = (546.1 / lambda_c)^5."""
    kinds = {"kepler": _abi.EMIT_KEPLER, "rigid": _abi.EMIT_RIGID}
    if emitter not in kinds:
        raise ValueError(f"DiskEmission: emitter must be 'kepler' or 'rigid', got {emitter!r}")
    lam = [float(v) for v in wavelengths_nm]
    if len(lam) != 3:
        raise ValueError("DiskEmission: wavelengths_nm needs three wavelengths (r, g, b)")
    return _abi.rtgr_disk_emission(object=int(object), emitter=kinds[emitter], flags=_abi.EMIT_INNER_EDGE if inner_edge else 0, pad=0,
                                   orbit=float(orbit), T_in=float(T_in), p=float(p), gain=float(gain),
                                   theta=(C.c_double * 3)(*[HC_OVER_KB_NM / v for v in lam]),
                                   weight=(C.c_double * 3)(*[(546.1 / v) ** 5 for v in lam]))


def trace_emission(metric, objs, cam, ni, nj, emission, textures=None, r_escape=0.0, aa=None, opt=None, dtype=np.float64, ctx=None, details=False):
    """A frame with an EMITTING DISK (rtgr_trace_emission_f64 / _f32) — an extension: the plain ni x nj frame of the camera, the
    textures (as trace_shaded: {omin: (texture, filter), 0: …}; not on the emitting disk), then the pixels that hit the disk of
    `emission` (a DiskEmission) get the black-body colour of the orbiting gas, shifted by the frequency ratio g; every other pixel
    keeps its bits.  aa: None, or dict(k=…, contrast=…, max_batch_rays=…) / an rtgr_aa — adaptive anti-aliasing of the emitted frame.
    -> dict(rgb [3, ni*nj], g [ni*nj] (NaN off the disk and where nothing emits), counters; aa: + refined, stats; details: + the
    per-ray outputs of the pixel-centre rays)."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    camera = _camera(cam)
    n = ni * nj
    sh = make_shade(textures, r_escape) if textures else None
    res = dict(rgb=np.zeros((3, n), dtype), g=np.zeros(n, dtype))
    aap, refined, stats = _aa_arg(aa, res, n)
    outs = _ray_details(res, n, dtype, sc.nobj) if details else None
    ctr = rtgr_counters()
    fn = lib.rtgr_trace_emission_f64 if dtype == np.float64 else lib.rtgr_trace_emission_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), C.byref(camera), ni, nj, None if sh is None else C.byref(sh), C.byref(emission), aap, res["rgb"].ctypes.data, outs,
                       res["g"].ctypes.data, refined, C.byref(ctr), stats))
    res["counters"] = ctr.as_dict()
    if stats is not None:
        res["stats"] = stats.as_dict()
    return res


def eval_disk_emission(metric, objs, emission, s0, s_end, dtype=np.float64, ctx=None, observer=None):
    """rtgr_eval_disk_emission_f64 / _f32: the emitter model at n pairs of ray states — s0 [n, 8] at the camera (make_canvas' states),
    s_end [n, 8] on the disk.  -> dict(omega [n], u_emit [n, 4], g [n], rgb [n, 3]); a point with no valid emitter gives NaN, NaN,
    NaN and black.  observer (an Observer; rtgr_eval_disk_emission_observer_*): the frequency ratio is taken against ITS 4-velocity, as
    trace_observer does; None: against the static observer at s0."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    a = np.ascontiguousarray(s0, dtype=dtype).reshape(-1, 8)
    e = np.ascontiguousarray(s_end, dtype=dtype).reshape(-1, 8)
    if a.shape != e.shape:
        raise ValueError(f"eval_disk_emission: s0 and s_end must have the same shape, got {a.shape} and {e.shape}")
    n = a.shape[0]
    res = dict(omega=np.zeros(n, dtype), u_emit=np.zeros((n, 4), dtype), g=np.zeros(n, dtype), rgb=np.zeros((n, 3), dtype))
    outs = (res["omega"].ctypes.data, res["u_emit"].ctypes.data, res["g"].ctypes.data, res["rgb"].ctypes.data)
    suf = "f64" if dtype == np.float64 else "f32"
    if observer is None:
        _abi.check(lib, getattr(lib, "rtgr_eval_disk_emission_" + suf)(ctx, C.byref(sc), C.byref(emission), a.ctypes.data, e.ctypes.data, n, *outs))
    else:
        _abi.check(lib, getattr(lib, "rtgr_eval_disk_emission_observer_" + suf)(ctx, C.byref(sc), C.byref(emission), C.byref(observer), a.ctypes.data,
                                                                                 e.ctypes.data, n, *outs))
    return res


# ---- observer camera (include/rtgr.h "observer camera") ---------------------------------------------------------------------------
def Observer(pos, look, up, fov_x, fov_y=None, kind="static", vel=None, orbit=+1, projection="perspective", max_batch_rays=0):
    """A pinhole camera carried by an observer -> rtgr_observer.  pos: the event (t, x, y, z); look, up: coordinate 4-vectors (only
    their parts orthogonal to the observer's 4-velocity matter).  kind "static": at rest in the slicing (make_canvas' observer);
    "velocity": the coordinate 4-velocity `vel`, any normalisation; "circular": on the circular geodesic through pos (z = 0) of the
    scene's own metric, orbit = +1 (counter-clockwise seen from +z) or -1.  projection "perspective": fov_x, fov_y in (0, pi);
    "equirect": a panorama, fov_x <= 2 pi, fov_y <= pi.  Angles in radians; fov_y = None: fov_x for a perspective frame, fov_x / 2
    for a panorama."""
    kinds = {"static": _abi.OBS_STATIC, "velocity": _abi.OBS_VELOCITY, "circular": _abi.OBS_CIRCULAR}
    projs = {"perspective": _abi.PROJ_PERSPECTIVE, "equirect": _abi.PROJ_EQUIRECT}
    if kind not in kinds:
        raise ValueError(f"Observer: kind must be 'static', 'velocity' or 'circular', got {kind!r}")
    if projection not in projs:
        raise ValueError(f"Observer: projection must be 'perspective' or 'equirect', got {projection!r}")
    if kind == "velocity" and vel is None:
        raise ValueError("Observer: kind 'velocity' needs vel")
    if fov_y is None:
        fov_y = fov_x if projection == "perspective" else 0.5 * fov_x
    v4 = lambda v: (C.c_double * 4)(*[float(c) for c in v])
    return _abi.rtgr_observer(pos=v4(pos), vel=v4(vel if vel is not None else (0, 0, 0, 0)), look=v4(look), up=v4(up), fov_x=float(fov_x),
                              fov_y=float(fov_y), orbit=float(orbit), kind=kinds[kind], projection=projs[projection], flags=0, pad=0,
                              max_batch_rays=int(max_batch_rays))


def eval_observer(metric, objs, observer, dtype=np.float64, ctx=None):
    """rtgr_eval_observer_f64 / _f32: the frame the kernels build from `observer` (an Observer) in this scene.
    -> dict(frame [4, 4] (rows e_0, e_right, e_up, e_look), omega (NaN unless circular), valid)."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    frame, omega, valid = np.zeros((4, 4), dtype), np.zeros(1, dtype), C.c_int(0)
    fn = lib.rtgr_eval_observer_f64 if dtype == np.float64 else lib.rtgr_eval_observer_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(observer), frame.ctypes.data, omega.ctypes.data, C.byref(valid)))
    return dict(frame=frame, omega=omega[0], valid=bool(valid.value))


def _valid_observer(metric, objs, observer, dtype, ctx):
    if not eval_observer(metric, objs, observer, dtype, ctx)["valid"]:
        raise ValueError("Observer: no valid frame at this event (a 4-velocity that is not timelike and future-directed, no circular orbit "
                         "there, or look / up degenerate after projection)")


def make_observer_canvas(metric, objs, observer, ni, nj, dtype=np.float64, ctx=None):
    """rtgr_make_observer_canvas_f64 / _f32: the start states [ni*nj, 8] of the observer's rays (pixel i + j ni), which trace_rays
    and rtgr_trace_* take as caller-supplied states.  Raises ValueError for an observer with no valid frame."""
    lib = _lib()
    _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    out = np.zeros((ni * nj, 8), dtype)
    fn = lib.rtgr_make_observer_canvas_f64 if dtype == np.float64 else lib.rtgr_make_observer_canvas_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(observer), ni, nj, 0, nj, out.ctypes.data))
    return out


def trace_observer(metric, objs, observer, ni, nj, emission=None, textures=None, r_escape=0.0, opt=None, dtype=np.float64, ctx=None, details=False):
    """A frame seen by an OBSERVER (rtgr_trace_observer_f64 / _f32) — an extension: a pinhole at one event, carried by a static, moving
    or orbiting observer (an Observer), perspective or equirectangular.  textures as trace_shaded, emission (a DiskEmission) as
    trace_emission — with the frequency ratio taken against THIS observer's 4-velocity.  Raises ValueError for an observer with no
    valid frame.  -> dict(rgb [3, ni*nj], counters; emission: + g [ni*nj]; details: + the per-ray outputs)."""
    lib = _lib()
    _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    n = ni * nj
    sh = make_shade(textures, r_escape) if textures else None
    res = dict(rgb=np.zeros((3, n), dtype))
    if emission is not None:
        res["g"] = np.zeros(n, dtype)
    outs = _ray_details(res, n, dtype, sc.nobj) if details else None
    ctr = rtgr_counters()
    fn = lib.rtgr_trace_observer_f64 if dtype == np.float64 else lib.rtgr_trace_observer_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), C.byref(observer), ni, nj, None if sh is None else C.byref(sh),
                       None if emission is None else C.byref(emission), res["rgb"].ctypes.data, outs,
                       res["g"].ctypes.data if emission is not None else None, C.byref(ctr)))
    res["counters"] = ctr.as_dict()
    return res


# ---- hot-spot light curves (include/rtgr.h "hot-spot light curves") ----------------------------------------------------------------
def HotSpot(rho_s, sigma, t_start=0.0, dt=1.0, nt=1, phi0=0.0, cut=4.0, amp=1.0, g_power=4.0):
    """A rigid Gaussian spot riding in the emitting disk -> rtgr_hot_spot.  rho_s, phi0: its centre at coordinate time 0 (cylindrical
    radius and azimuth in the plane z = 0); sigma: its width, cut: its support in units of sigma; amp: the emissivity at the centre;
    g_power: q of the weight g^q (4 bolometric, 3 the specific intensity of a flat spectrum); the observer times are
    tau_k = t_start + k dt, k < nt."""
    return _abi.rtgr_hot_spot(rho_s=float(rho_s), phi0=float(phi0), sigma=float(sigma), cut=float(cut), amp=float(amp), g_power=float(g_power),
                              t_start=float(t_start), dt=float(dt), nt=int(nt), flags=0, pad=0)


def eval_hot_spot(metric, objs, emission, spot, points=None, dtype=np.float64, ctx=None):
    """rtgr_eval_hot_spot_f64 / _f32: the spot's orbital rate in the disk of `emission` (the emitter model's own, at (rho_s, 0, 0)),
    whether it is valid, and its emissivity j at `points` [n, 3] = (x, y, t): where the spot stands at coordinate time t.
    -> dict(omega_s, valid, j [n] (Float64 whatever dtype))."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    pts = np.ascontiguousarray(points if points is not None else np.zeros((0, 3)), dtype=dtype).reshape(-1, 3)
    n = pts.shape[0]
    omega, valid, j = np.zeros(1, dtype), C.c_int(0), np.zeros(n, np.float64)
    fn = lib.rtgr_eval_hot_spot_f64 if dtype == np.float64 else lib.rtgr_eval_hot_spot_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(emission), C.byref(spot), pts.ctypes.data if n else None, n, omega.ctypes.data, C.byref(valid),
                       j.ctypes.data if n else None))
    return dict(omega_s=omega[0], valid=bool(valid.value), j=j)


def _trace_reduced(name, hook, metric, objs, observer, ni, nj, emission, record, rows, textures, r_escape, opt, dtype, ctx, details):
    """What light_curve and spectrum share: rtgr_trace_<name>_f64 / _f32 on ONE frame of the emitting disk seen by `observer`, reduced on
    the device to `rows` rows of (F, A, B) by `record` (a HotSpot, a Spectrum).  The observer is checked first, then `hook` asks the
    feature's own hook what it must (it raises, or answers).
    -> (dict(rgb [3, ni*nj], g [ni*nj], counters; details: + the per-ray outputs), table [rows, 3], the hook's answer)"""
    lib = _lib()
    _valid_observer(metric, objs, observer, dtype, ctx)
    answer = hook()
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    n = ni * nj
    sh = make_shade(textures, r_escape) if textures else None
    res = dict(rgb=np.zeros((3, n), dtype), g=np.zeros(n, dtype))
    table = np.zeros((int(rows), 3), np.float64)
    outs = _ray_details(res, n, dtype, sc.nobj) if details else None
    ctr = rtgr_counters()
    fn = getattr(lib, f"rtgr_trace_{name}_" + ("f64" if dtype == np.float64 else "f32"))
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), C.byref(observer), ni, nj, None if sh is None else C.byref(sh), C.byref(emission),
                       C.byref(record), res["rgb"].ctypes.data, outs, res["g"].ctypes.data, table.ctypes.data, C.byref(ctr)))
    res["counters"] = ctr.as_dict()
    return res, table, answer


def light_curve(metric, objs, observer, ni, nj, emission, spot, textures=None, r_escape=0.0, opt=None, dtype=np.float64, ctx=None, details=False):
    """The LIGHT CURVE of a hot spot (rtgr_trace_light_curve_f64 / _f32) — an extension: ONE frame of the emitting disk seen by
    `observer` (as trace_observer with `emission`), reduced on the device over the nt observer times of `spot` (a HotSpot).  The
    picture is the disk without the spot.  Raises ValueError for an observer with no valid frame and for a spot with no valid orbit.
    -> dict(rgb [3, ni*nj], g [ni*nj], lc [nt, 3] = (F, A, B) per observer time — the image centroid is (A / F, B / F) in the pixel
    coordinates a, b in (-1, 1) —, tau [nt], counters; details: + the per-ray outputs)."""
    def hook():
        if not eval_hot_spot(metric, objs, emission, spot, None, dtype, ctx)["valid"]:
            raise ValueError("HotSpot: no valid circular orbit of the disk's emitter at rho_s (none exists there, or it is not timelike)")

    res, lc, _ = _trace_reduced("light_curve", hook, metric, objs, observer, ni, nj, emission, spot, spot.nt, textures, r_escape, opt, dtype, ctx, details)
    res.update(lc=lc, tau=spot.t_start + np.arange(int(spot.nt), dtype=np.float64) * spot.dt)
    return res


# ---- disk spectra (include/rtgr.h "disk spectra") ------------------------------------------------------------------------------------
def Spectrum(kind, lo, hi, nb, amp=None, alpha=0.0, rho_min=0.0, rho_max=0.0, g_power=None, log=False, nu3=False):
    """A line profile or a thermal spectrum of the emitting disk -> rtgr_spectrum.  kind "line": nb bins over [lo, hi) of the frequency
    ratio g (a line of rest energy 1), emissivity amp (rho / rho_min)^(-alpha) inside the window rho_min <= rho < rho_max, weight g^g_power
    (amp defaults to 1, g_power to 4).  kind "thermal": nb sample frequencies theta_k from lo to hi in the units of DiskEmission's theta
    (h nu / k_B in kelvin), spaced linearly or, log=True, geometrically; nu3=True multiplies sample k by theta_k^3 (F_nu up to a constant)."""
    kinds = {"line": _abi.SPEC_LINE, "thermal": _abi.SPEC_THERMAL}
    if kind not in kinds:
        raise ValueError(f"Spectrum: kind must be 'line' or 'thermal', got {kind!r}")
    line = kind == "line"
    return _abi.rtgr_spectrum(kind=kinds[kind], flags=(_abi.SPEC_LOG if log else 0) | (_abi.SPEC_NU3 if nu3 else 0), nb=int(nb), lo=float(lo), hi=float(hi),
                              amp=float((1.0 if line else 0.0) if amp is None else amp), alpha=float(alpha), rho_min=float(rho_min), rho_max=float(rho_max),
                              g_power=float((4.0 if line else 0.0) if g_power is None else g_power), reserved=0.0)


def eval_spectrum(metric, objs, emission, spec, points=None, dtype=np.float64, ctx=None):
    """rtgr_eval_spectrum_f64 / _f32: the spectral axis of `spec` (a Spectrum) and, at `points` [n, 3] = (x, y, g), what the reduction
    makes of a pixel that ends there.  -> dict(axis [nb] (line: the bin centres; thermal: theta_k), bin [n] (line: the bin, -1 where the
    point does not count; thermal: 0 or -1), val (line [n]: amp (rho / rho_min)^(-alpha) g^g_power; thermal [n, nb]: c_k / expm1(theta_k tau);
    0 where the point does not count)); Float64 whatever dtype."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    pts = np.ascontiguousarray(points if points is not None else np.zeros((0, 3)), dtype=dtype).reshape(-1, 3)
    n, nb = pts.shape[0], int(spec.nb)
    thermal = spec.kind == _abi.SPEC_THERMAL
    axis, bins = np.zeros(max(nb, 0), np.float64), np.zeros(n, np.int64)
    val = np.zeros((n, nb) if thermal else n, np.float64)
    fn = lib.rtgr_eval_spectrum_f64 if dtype == np.float64 else lib.rtgr_eval_spectrum_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(emission), C.byref(spec), pts.ctypes.data if n else None, n, axis.ctypes.data if nb else None,
                       bins.ctypes.data if n else None, val.ctypes.data if val.size else None))
    return dict(axis=axis, bin=bins, val=val)


def spectrum(metric, objs, observer, ni, nj, emission, spec, textures=None, r_escape=0.0, opt=None, dtype=np.float64, ctx=None, details=False):
    """The SPECTRUM of an emitting disk (rtgr_trace_spectrum_f64 / _f32) — an extension: ONE frame of the disk seen by `observer` (as
    trace_observer with `emission`), reduced on the device to the line profile or the thermal spectrum `spec` (a Spectrum) names.
    Raises ValueError for an observer with no valid frame.  -> dict(rgb [3, ni*nj], g [ni*nj], axis [nb], F [nb], A [nb], B [nb] — the
    flux centroid per bin or sample is (A / F, B / F) in the pixel coordinates a, b in (-1, 1) —, counters; details: + the per-ray outputs)."""
    res, out, axis = _trace_reduced("spectrum", lambda: eval_spectrum(metric, objs, emission, spec, None, dtype, ctx)["axis"], metric, objs, observer, ni, nj,
                              emission, spec, spec.nb, textures, r_escape, opt, dtype, ctx, details)
    res.update(axis=axis, F=out[:, 0].copy(), A=out[:, 1].copy(), B=out[:, 2].copy())
    return res


# ---- polarized disk images (include/rtgr.h "polarized disk images") -------------------------------------------------------------------
def Polarization(kind, deg0=1.0, deg1=0.0, field=(0.0, 0.0, 0.0)):
    """The emission law of a polarized disk image -> rtgr_polarization.  kind "scatter": an electron-scattering atmosphere, the electric
    vector in the disk plane, degree deg0 (1 - mu) / (1 + deg1 mu); "field": synchrotron emission in the ordered field (B_rho, B_phi,
    B_z) of the emitter's triad, degree deg0."""
    kinds = {"scatter": _abi.POL_SCATTER, "field": _abi.POL_FIELD}
    if kind not in kinds:
        raise ValueError(f"Polarization: kind must be 'scatter' or 'field', got {kind!r}")
    return _abi.rtgr_polarization(kind=kinds[kind], flags=0, deg0=float(deg0), deg1=float(deg1), field=(C.c_double * 3)(*[float(c) for c in field]),
                                  reserved=(C.c_double * 2)(0.0, 0.0))


def trace_polarized(metric, objs, observer, ni, nj, emission, polarization, textures=None, r_escape=0.0, opt=None, dtype=np.float64, ctx=None,
                    details=False):
    """A POLARIZED frame of an emitting disk (rtgr_trace_polarized_f64 / _f32) — an extension: trace_observer's frame with emission, bit
    for bit, plus the fractional Stokes pair by Walker-Penrose transport (Kerr with its own radius, or flat space).  Raises ValueError
    for an observer with no valid frame.  -> trace_observer's dict + q, u, aux [ni*nj] (NaN off the disk)."""
    lib = _lib()
    _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    n = ni * nj
    sh = make_shade(textures, r_escape) if textures else None
    res = dict(rgb=np.zeros((3, n), dtype), g=np.zeros(n, dtype), q=np.zeros(n, dtype), u=np.zeros(n, dtype), aux=np.zeros(n, dtype))
    outs = _ray_details(res, n, dtype, sc.nobj) if details else None
    ctr = rtgr_counters()
    fn = lib.rtgr_trace_polarized_f64 if dtype == np.float64 else lib.rtgr_trace_polarized_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), C.byref(observer), ni, nj, None if sh is None else C.byref(sh),
                       None if emission is None else C.byref(emission), None if polarization is None else C.byref(polarization),
                       res["rgb"].ctypes.data, outs, res["g"].ctypes.data, res["q"].ctypes.data, res["u"].ctypes.data, res["aux"].ctypes.data,
                       C.byref(ctr)))
    res["counters"] = ctr.as_dict()
    return res


def eval_polarization(metric, objs, emission, polarization, observer, s0, s_end, dtype=np.float64, ctx=None):
    """rtgr_eval_polarization_f64 / _f32: the polarization kernel at n pairs of ray states — s0 [n, 8] at the camera (the observer's own
    states), s_end [n, 8] on the disk.  Raises ValueError for an observer with no valid frame.
    -> dict(kappa [n, 2], f_em [n, 4], aux, delta, q, u [n], valid [n] bool)."""
    lib = _lib()
    _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    a = np.ascontiguousarray(s0, dtype=dtype).reshape(-1, 8)
    e = np.ascontiguousarray(s_end, dtype=dtype).reshape(-1, 8)
    if a.shape != e.shape:
        raise ValueError(f"eval_polarization: s0 and s_end must have the same shape, got {a.shape} and {e.shape}")
    n = a.shape[0]
    res = dict(kappa=np.zeros((n, 2), dtype), f_em=np.zeros((n, 4), dtype), aux=np.zeros(n, dtype), delta=np.zeros(n, dtype), q=np.zeros(n, dtype),
               u=np.zeros(n, dtype))
    valid = np.zeros(n, np.int32)
    fn = lib.rtgr_eval_polarization_f64 if dtype == np.float64 else lib.rtgr_eval_polarization_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(emission), C.byref(polarization), C.byref(observer), a.ctypes.data, e.ctypes.data, n,
                       res["kappa"].ctypes.data, res["f_em"].ctypes.data, res["aux"].ctypes.data, res["delta"].ctypes.data, res["q"].ctypes.data,
                       res["u"].ctypes.data, valid.ctypes.data))
    res["valid"] = valid != 0
    return res


def eval_walker_penrose(metric, objs, s, f, dtype=np.float64, ctx=None):
    """rtgr_eval_walker_penrose_f64 / _f32: (Y(k, f), h(k, f)) [n, 2] at n states s [n, 8] = (x, k) and n vectors f [n, 4], by the
    polarization kernel's own Killing-Yano forms (NaN on the axis)."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    a = np.ascontiguousarray(s, dtype=dtype).reshape(-1, 8)
    v = np.ascontiguousarray(f, dtype=dtype).reshape(-1, 4)
    if a.shape[0] != v.shape[0]:
        raise ValueError(f"eval_walker_penrose: s and f must have the same length, got {a.shape[0]} and {v.shape[0]}")
    kap = np.zeros((a.shape[0], 2), dtype)
    fn = lib.rtgr_eval_walker_penrose_f64 if dtype == np.float64 else lib.rtgr_eval_walker_penrose_f32
    _abi.check(lib, fn(ctx, C.byref(sc), a.ctypes.data, v.ctypes.data, a.shape[0], kap.ctypes.data))
    return kap


# ---- higher-order disk images (include/rtgr.h "higher-order disk images") ---------------------------------------------------------------
def DiskOrders(max_order, transmission=1.0, margin=0.0):
    """How far rays are followed through the emitting disk -> rtgr_disk_orders.  max_order N (1..8): orders 1 .. N are looked for;
    transmission T in [0, 1]: order k adds T^k times its emission to the picture (1: an optically thin disk, 0: the opaque one);
    margin eta: how far the disk is inflated for the crossing legs (0: half its half thickness)."""
    return _abi.rtgr_disk_orders(max_order=int(max_order), flags=0, margin=float(margin), transmission=float(transmission), pad=0)


def trace_orders(metric, objs, observer, ni, nj, emission, orders, state0=None, textures=None, r_escape=0.0, opt=None, dtype=np.float64, ctx=None):
    """The emitting disk seen ORDER BY ORDER (rtgr_trace_orders_f64 / _f32) — an extension: trace_observer's frame with emission (order 0),
    then every ray that ended on the disk carried through it and traced on; where it meets the disk again is the next order — order 1 the
    lensed far side and underside, order >= 2 the photon ring.  orders: a DiskOrders.  state0 [ni*nj, 8]: the rays are these states in
    place of the observer's, and observer may then be None (the frequency ratio is taken against the static observer at the ray's start).
    Raises ValueError for an observer with no valid frame.
    -> dict(rgb [3, ni*nj] (the sum over orders, weighted T^k), count [ni*nj] uint8 (disk crossings per pixel), the per-order planes
    hit32 [N+1, ni*nj], state_end [N+1, ni*nj, 8], g [N+1, ni*nj], rgb_order [N+1, 3, ni*nj] (block 0: trace_observer's; block k >= 1:
    NaN / 0 where the pixel has no order k), state0 [ni*nj, 8], counters (summed over all legs))."""
    lib = _lib()
    if observer is not None:
        _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    n = ni * nj
    nb = max(int(orders.max_order), 0) + 1 if orders is not None else 1
    sh = make_shade(textures, r_escape) if textures else None
    s0 = None if state0 is None else np.ascontiguousarray(state0, dtype=dtype).reshape(-1, 8)
    if s0 is not None and s0.shape[0] != n:
        raise ValueError(f"trace_orders: state0 must hold ni*nj = {n} states, got {s0.shape[0]}")
    res = dict(rgb=np.zeros((3, n), dtype), count=np.zeros(n, np.uint8), hit32=np.zeros((nb, n), np.uint32), state_end=np.zeros((nb, n, 8), dtype),
               g=np.zeros((nb, n), dtype), rgb_order=np.zeros((nb, 3, n), dtype), state0=np.zeros((n, 8), dtype))
    planes = _abi.rtgr_order_planes(count=res["count"].ctypes.data, hit32=res["hit32"].ctypes.data, state_end=res["state_end"].ctypes.data,
                                    g=res["g"].ctypes.data, rgb_order=res["rgb_order"].ctypes.data, state0=res["state0"].ctypes.data)
    ctr = rtgr_counters()
    fn = lib.rtgr_trace_orders_f64 if dtype == np.float64 else lib.rtgr_trace_orders_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), None if observer is None else C.byref(observer), None if s0 is None else s0.ctypes.data, ni, nj,
                       None if sh is None else C.byref(sh), None if emission is None else C.byref(emission),
                       None if orders is None else C.byref(orders), res["rgb"].ctypes.data, C.byref(planes), C.byref(ctr)))
    res["counters"] = ctr.as_dict()
    return res


def trace_ray(metric, objs, cb, p, opt=None, ctx=None):
    """Legacy single-pixel shape `trace_ray(metric, objs, cb, p)::Pixel` (test/runtests.jl:65-79).
    `cb` is accepted for signature parity and ignored: the callback is always
    ContinuousCallback(min_distance(objs, ·), terminate!) (src/RayTraceGR.jl:488-490)."""
    lib = _lib()
    sc = make_scene(metric, objs, ctx)
    t = _canvas_scalar(p.dtype)
    opt = opt or solver_defaults(t)
    pos = np.ascontiguousarray(p["pos"], dtype=t)
    nrm = np.ascontiguousarray(p["normal"], dtype=t)
    rgb = np.zeros(3, t)
    se = np.zeros(8, t)
    st = C.c_uint8(0)
    fn = lib.rtgr_trace_one_f64 if t == np.float64 else lib.rtgr_trace_one_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), pos.ctypes.data, nrm.ctypes.data, rgb.ctypes.data, se.ctypes.data,
                       C.addressof(st)))
    return Pixel(pos, nrm, rgb, dtype=t)


# ---- physics kernels for the reference's unit tests (test/runtests.jl:12-61), evaluated on the GPU ------------
def _eval_metric(metric, x, want=(True, True, True), dtype=np.float64):
    lib = _lib()
    sc = make_scene(metric, [])
    x = np.ascontiguousarray(x, dtype=dtype).reshape(-1, 4)
    n = x.shape[0]
    g = np.empty((n, 4, 4), dtype) if want[0] else None
    dg = np.empty((n, 4, 4, 4), dtype) if want[1] else None
    G = np.empty((n, 4, 4, 4), dtype) if want[2] else None
    fn = lib.rtgr_eval_metric_f64 if dtype == np.float64 else lib.rtgr_eval_metric_f32
    _abi.check(lib, fn(None, C.byref(sc), x.ctypes.data, n, g.ctypes.data if want[0] else None,
                       dg.ctypes.data if want[1] else None, G.ctypes.data if want[2] else None))
    sq = (lambda v: v[0] if (v is not None and n == 1) else v)
    return sq(g), sq(dg), sq(G)


def dmetric(metric, x, dtype=np.float64):
    """dmetric(metric, x) -> (g[a,b], dg[a,b,c] = ∂_c g_ab)  (src/RayTraceGR.jl:302-313); dtype = the reference's T"""
    g, dg, _ = _eval_metric(metric, x, (True, True, False), dtype)
    return g, dg


def christoffel(metric, x, dtype=np.float64):
    """christoffel(metric, x) -> Γ[a,b,c] = Γ^a_bc  (src/RayTraceGR.jl:321-331)"""
    return _eval_metric(metric, x, (False, False, True), dtype)[2]


def geodesic(s, metric, lam=0.0, path=0, dtype=np.float64):
    """geodesic(s::SVector{8}, metric, λ) -> ṡ  (src/RayTraceGR.jl:367-370); λ is ignored as in the reference.
    path: 0 closed contraction (IEEE division), 1 generic dual numbers, 2 the integrate loop's own RHS."""
    lib = _lib()
    sc = make_scene(metric, [])
    s = np.ascontiguousarray(s, dtype=dtype).reshape(-1, 8)
    ds = np.empty_like(s)
    fn = lib.rtgr_eval_geodesic_f64 if dtype == np.float64 else lib.rtgr_eval_geodesic_f32
    _abi.check(lib, fn(None, C.byref(sc), s.ctypes.data, s.shape[0], path, ds.ctypes.data))
    return ds[0] if ds.shape[0] == 1 else ds


# ---- volume emission (include/rtgr.h "volume emission") -----------------------------------------------------------------------------------
def Flow(j0, kappa=0.0, r0=1.0, alpha=1.0, H=0.3, s=0.0, r_stop=0.0, orbit=+1, emitter="kepler", gain=1.0, weight=(1.0, 1.0, 1.0)):
    """A hot, rotating flow that emits and absorbs along each ray -> rtgr_flow.  Density (r / r0)^(-alpha) exp(-z² / (2 H² rho²));
    emitter "kepler": gas on cylinders at the circular-orbit rate of the scene's own metric, orbit = +1 or -1; "rigid": Omega = orbit.
    Emissivity j0 n nu^(-s), grey absorption kappa n (0: optically thin).  r_stop: the integration of a ray ends once it is inside this
    radius — choose it inside the photon orbit's cylinder, where there is no gas (0 in flat space).  The picture gets gain weight_c I."""
    kinds = {"kepler": _abi.EMIT_KEPLER, "rigid": _abi.EMIT_RIGID}
    if emitter not in kinds:
        raise ValueError(f"Flow: emitter must be 'kepler' or 'rigid', got {emitter!r}")
    w = [float(v) for v in weight]
    if len(w) != 3:
        raise ValueError("Flow: weight needs three channels (r, g, b)")
    return _abi.rtgr_flow(emitter=kinds[emitter], flags=0, orbit=float(orbit), j0=float(j0), kappa=float(kappa), r0=float(r0), alpha=float(alpha),
                          H=float(H), s=float(s), r_stop=float(r_stop), gain=float(gain), weight=(C.c_double * 3)(*w))


def trace_transfer(metric, objs, observer, ni, nj, flow, emission=None, textures=None, r_escape=0.0, opt=None, dtype=np.float64, ctx=None,
                   details=False):
    """A frame with VOLUME EMISSION (rtgr_trace_transfer_f64 / _f32) — an extension: trace_observer's frame, then the transfer equations
    of `flow` (a Flow) integrated along every ray as far as the trace followed it: rgb = rgb exp(-tau) + gain weight I.  Raises
    ValueError for an observer with no valid frame.  -> trace_observer's dict + I, tau [ni*nj], tstatus [ni*nj] (0 reached the ray's
    end, 1 r_stop, 2 step cap, 3 not integrated or not finite), tsteps [ni*nj] (step attempts), transfer_counters."""
    lib = _lib()
    _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    n = ni * nj
    sh = make_shade(textures, r_escape) if textures else None
    res = dict(rgb=np.zeros((3, n), dtype), I=np.zeros(n, dtype), tau=np.zeros(n, dtype), tstatus=np.zeros(n, np.uint8), tsteps=np.zeros(n, np.uint32))
    if emission is not None:
        res["g"] = np.zeros(n, dtype)
    outs = _ray_details(res, n, dtype, sc.nobj) if details else None
    ctr, tctr = rtgr_counters(), rtgr_counters()
    fn = lib.rtgr_trace_transfer_f64 if dtype == np.float64 else lib.rtgr_trace_transfer_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), C.byref(observer), ni, nj, None if sh is None else C.byref(sh),
                       None if emission is None else C.byref(emission), None if flow is None else C.byref(flow), res["rgb"].ctypes.data, outs,
                       res["g"].ctypes.data if emission is not None else None, res["I"].ctypes.data, res["tau"].ctypes.data,
                       res["tstatus"].ctypes.data, res["tsteps"].ctypes.data, C.byref(ctr), C.byref(tctr)))
    res["counters"] = ctr.as_dict()
    res["transfer_counters"] = tctr.as_dict()
    return res


def eval_transfer(metric, objs, flow, s0, lambda_end, observer=None, opt=None, dtype=np.float64, ctx=None):
    """rtgr_eval_transfer_f64 / _f32: the transfer kernel itself over n listed rays — s0 [n, 8] their start states, lambda_end [n] how
    far each is integrated.  observer (an Observer): u_obs is its 4-velocity, as in trace_transfer; None: the static observer at s0.
    -> dict(I, tau [n], s_end [n, 8], tstatus [n], tsteps [n])."""
    lib = _lib()
    if observer is not None:
        _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    opt = opt or solver_defaults(dtype)
    a = np.ascontiguousarray(s0, dtype=dtype).reshape(-1, 8)
    le = np.ascontiguousarray(lambda_end, dtype=dtype).reshape(-1)
    if a.shape[0] != le.shape[0]:
        raise ValueError(f"eval_transfer: s0 and lambda_end must have the same length, got {a.shape[0]} and {le.shape[0]}")
    n = a.shape[0]
    res = dict(I=np.zeros(n, dtype), tau=np.zeros(n, dtype), s_end=np.zeros((n, 8), dtype), tstatus=np.zeros(n, np.uint8), tsteps=np.zeros(n, np.uint32))
    fn = lib.rtgr_eval_transfer_f64 if dtype == np.float64 else lib.rtgr_eval_transfer_f32
    _abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), None if flow is None else C.byref(flow), None if observer is None else C.byref(observer),
                       a.ctypes.data if n else None, le.ctypes.data if n else None, n, *[res[k].ctypes.data if n else None
                                                                                       for k in ("I", "tau", "s_end", "tstatus", "tsteps")]))
    return res


def eval_flow(metric, objs, flow, s0, s, observer=None, dtype=np.float64, ctx=None):
    """rtgr_eval_flow_f64 / _f32: the flow model at n points — s [n, 8] a point and the ray's tangent there, s0 [n, 8] the ray's start
    state (for kappa0).  -> dict(dens, omega [n], u_f [n, 4], gfac, dtau, dI0 [n]); an invalid point gives NaN in omega, u_f and gfac
    and 0 in the two derivatives."""
    lib = _lib()
    if observer is not None:
        _valid_observer(metric, objs, observer, dtype, ctx)
    sc = make_scene(metric, objs, ctx)
    a = np.ascontiguousarray(s0, dtype=dtype).reshape(-1, 8)
    p = np.ascontiguousarray(s, dtype=dtype).reshape(-1, 8)
    if a.shape != p.shape:
        raise ValueError(f"eval_flow: s0 and s must have the same shape, got {a.shape} and {p.shape}")
    n = a.shape[0]
    res = dict(dens=np.zeros(n, dtype), omega=np.zeros(n, dtype), u_f=np.zeros((n, 4), dtype), gfac=np.zeros(n, dtype), dtau=np.zeros(n, dtype),
               dI0=np.zeros(n, dtype))
    fn = lib.rtgr_eval_flow_f64 if dtype == np.float64 else lib.rtgr_eval_flow_f32
    _abi.check(lib, fn(ctx, C.byref(sc), None if flow is None else C.byref(flow), None if observer is None else C.byref(observer),
                       a.ctypes.data if n else None, p.ctypes.data if n else None, n, *[res[k].ctypes.data if n else None
                                                                                      for k in ("dens", "omega", "u_f", "gfac", "dtau", "dI0")]))
    return res


# ---- example scenes (src/RayTraceGR.jl:542-612) -------------------------------------------------------------------
outdir = "scenes"  # :540


def example1_scene():
    """Scene of example1(): Minkowski, sky R=-10, plane t=-20, sphere R=1/2 at the origin; camera (0,0,-2,0)
    (src/RayTraceGR.jl:545-557).  Returns (metric, objs, camera_args)."""
    caelum = Sphere((0, 0, 0, 0), (1, 0, 0, 0), -10)
    frustum = Plane(-20)
    sphere = Sphere((0, 0, 0, 0), (1, 0, 0, 0), 0.5)
    cam = dict(pos=(0, 0, -2, 0), widthx=(0, 1, 0, 0), widthy=(0, 0, 0, 1), normal=(0, 0, 1, 0))
    return minkowski, [caelum, frustum, sphere], cam


def example2_scene(metric=None):
    """Scene of example2(): kerr_schild, sky R=-10, plane t=-20, sphere R=1/2 at (0,4,0,0); camera (0,4,-2,0)
    (src/RayTraceGR.jl:581-593)."""
    caelum = Sphere((0, 0, 0, 0), (1, 0, 0, 0), -10)
    frustum = Plane(-20)
    sphere = Sphere((0, 4, 0, 0), (1, 0, 0, 0), 0.5)
    cam = dict(pos=(0, 4, -2, 0), widthx=(0, 1, 0, 0), widthy=(0, 0, 0, 1), normal=(0, 0, 1, 0))
    return (metric or kerr_schild), [caelum, frustum, sphere], cam


def _run_example(scene, ni, nj, fname, save, ctx=None):
    from .png import write_png
    metric, objs, cam = scene
    canvas = make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], ni, nj, ctx=ctx)
    canvas = trace_rays(metric, objs, canvas, ctx=ctx)
    if save:
        os.makedirs(outdir, exist_ok=True)
        file = os.path.join(outdir, fname)
        if os.path.exists(file):
            os.remove(file)
        print(f'Output file is "{file}"')
        write_png(file, canvas.image_u8())
    return canvas


def example1(ni=200, nj=200, save=True, ctx=None):
    """example1()  src/RayTraceGR.jl:542-576"""
    return _run_example(example1_scene(), ni, nj, "sphere.png", save, ctx)


def example2(ni=200, nj=200, save=True, ctx=None):
    """example2()  src/RayTraceGR.jl:578-612"""
    return _run_example(example2_scene(), ni, nj, "sphere2.png", save, ctx)


__all__ = ["D", "Metric", "UserMetric", "GridMetric", "sample_metric", "UserObjects", "UserObject", "minkowski", "kerr_schild", "KerrSchild", "Object", "Plane", "Sphere", "Disk",
           "make_scene", "check_scene", "eval_objects", "solver_defaults", "make_camera", "Pixel", "pixel_dtype", "Canvas", "make_canvas",
           "trace_rays", "trace_ray", "trace_frames", "trace_aa", "Texture", "texture_load", "texture_unload", "eval_texture", "make_shade", "trace_shaded", "DiskEmission", "trace_emission", "eval_disk_emission", "Observer", "eval_observer", "make_observer_canvas", "trace_observer", "HotSpot", "eval_hot_spot", "light_curve", "Spectrum", "eval_spectrum", "spectrum", "Polarization", "trace_polarized", "eval_polarization", "eval_walker_penrose", "DiskOrders", "trace_orders", "Flow", "trace_transfer", "eval_transfer", "eval_flow", "dmetric", "christoffel", "geodesic", "example1", "example2",
           "example1_scene", "example2_scene"]
