"""Metrics sampled on a grid (RTGR_GRID, include/rtgr.h): a spacetime given as numbers on a uniform 3-D grid, interpolated on the
device (tricubic Catmull-Rom) inside the integrate loop.  The grids here are made with numpy from closed forms, never by the library.
CPU tests: the ABI (header, ctypes, a gcc-compiled caller, the Julia stub) and the Python checks.  GPU tests (`pytest -m gpu`): the
interpolant, tracing through flat and Kerr-Schild grids, the OUTSIDE rule, Float32, every entry point, lifetime."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from scenes import rt, wrap_aware_rgb_err

abi = rt._abi
UPPER = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
ETA = np.array([-1.0, 0, 0, 0, 1, 0, 0, 1, 0, 1])


# ---- closed forms in numpy (the grids' sources) -------------------------------------------------------------------------------
def axes(origin, h, n):
    return [origin[a] + h[a] * np.arange(n[a]) for a in range(3)]


def sample(fn, origin, h, n):
    """(nz, ny, nx, 10) samples of fn(x, y, z) -> (..., 10)"""
    xs, ys, zs = axes(origin, h, n)
    z, y, x = np.meshgrid(zs, ys, xs, indexing="ij")
    return fn(x, y, z)


def flat(x, y, z):
    return np.broadcast_to(ETA, x.shape + (10,)).copy()


def kerr_schild(x, y, z, M=1.0, a=0.8):
    """textbook Kerr-Schild g = eta + f k k (k_t = 1); the ring singularity and its surroundings (rho < 1, deep inside the horizon and
    inside the scenes' central sphere) are replaced by eta: no ray's stencil reaches there"""
    rho2 = x * x + y * y + z * z
    q = rho2 - a * a
    with np.errstate(all="ignore"):
        r = np.sqrt(0.5 * (q + np.sqrt(q * q + 4 * a * a * z * z)))
        f = 2 * M * r ** 3 / (r ** 4 + a * a * z * z)
        k = [np.ones_like(x), (r * x + a * y) / (r * r + a * a), (r * y - a * x) / (r * r + a * a), z / r]
        g = np.stack([ETA[c] + f * k[p] * k[q] for c, (p, q) in enumerate(UPPER)], axis=-1)
    g[rho2 < 1.0] = ETA
    return g


def kerr_schild_island(x, y, z, r0=2.6, r1=3.2):
    """Kerr-Schild's f switched off smoothly between rho = r0 and r1 (a C² quintic step): g = eta + f chi k k, still of Kerr-Schild form
    (det g = -1), and EXACTLY eta beyond r1 — where the interpolant of any grid, extrapolating or not, returns eta to the bit"""
    g = kerr_schild(x, y, z)
    rho = np.sqrt(x * x + y * y + z * z)
    t = np.clip((rho - r0) / (r1 - r0), 0.0, 1.0)
    chi = 1.0 - t ** 3 * (10.0 - 15.0 * t + 6.0 * t * t)
    g = ETA + (g - ETA) * chi[..., None]
    g[rho >= r1] = ETA
    return g


def ks_grid(h, L=6.6, fn=kerr_schild):
    """KerrSchild(1, 0.8) on a grid whose valid box is [-L, L]^3 (samples on multiples of h)"""
    n = int(round(2 * L / h)) + 3
    origin = (-L - h,) * 3
    return rt.GridMetric(sample(fn, origin, (h,) * 3, (n,) * 3), origin, h, name=f"ks h={h}")


def flat_grid(L=11.0, h=1.0):
    n = int(round(2 * L / h)) + 3
    origin = (-L - h,) * 3
    return rt.GridMetric(sample(flat, origin, (h,) * 3, (n,) * 3), origin, h, name="flat")


# ---- the interpolant in numpy (what include/rtgr.h specifies) ---------------------------------------------------------------
def cr_weights(t):
    w = np.stack([(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2], -1)
    dw = np.stack([(-3 * t ** 2 + 4 * t - 1) / 2, (9 * t ** 2 - 10 * t) / 2, (-9 * t ** 2 + 8 * t + 1) / 2, (3 * t ** 2 - 2 * t) / 2], -1)
    return w, dw


def catmull_rom(samples, origin, h, pts):
    """g (n, 10) and dg (n, 3, 10) = d/dx, d/dy, d/dz at spatial points pts (n, 3)"""
    nz, ny, nx, _ = samples.shape
    n = (nx, ny, nz)
    idx, W, DW = [], [], []
    for a in range(3):
        s = (pts[:, a] - origin[a]) / h[a]
        i = np.clip(np.floor(s), 1, n[a] - 3).astype(int)
        w, dw = cr_weights(s - i)
        idx.append(i - 1)
        W.append(w)
        DW.append(dw / h[a])
    g = np.zeros((len(pts), 10))
    dg = np.zeros((len(pts), 3, 10))
    for kz in range(4):
        for ky in range(4):
            for kx in range(4):
                v = samples[idx[2] + kz, idx[1] + ky, idx[0] + kx]
                wx, wy, wz = W[0][:, kx], W[1][:, ky], W[2][:, kz]
                g += (wx * wy * wz)[:, None] * v
                dg[:, 0] += (DW[0][:, kx] * wy * wz)[:, None] * v
                dg[:, 1] += (wx * DW[1][:, ky] * wz)[:, None] * v
                dg[:, 2] += (wx * wy * DW[2][:, kz])[:, None] * v
    return g, dg


def to4(c10):
    """(..., 10) upper triangle -> (..., 4, 4)"""
    out = np.zeros(c10.shape[:-1] + (4, 4))
    for c, (p, q) in enumerate(UPPER):
        out[..., p, q] = out[..., q, p] = c10[..., c]
    return out


# ---- the ABI (no GPU) -------------------------------------------------------------------------------------------------------
def test_header_declares_the_grid_metric():
    txt = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    assert re.search(r"\bRTGR_GRID\s*=\s*4\b", txt) and re.search(r"\bRTGR_RAY_OUTSIDE\s*=\s*5\b", txt)
    assert re.search(r"typedef struct rtgr_grid \{\s*uint32_t n\[3\];.*?uint32_t pad;.*?double origin\[3\];.*?double spacing\[3\];.*?\} rtgr_grid;",
                     txt, re.S)
    assert "int rtgr_grid_metric_load(rtgr_context* ctx, const rtgr_grid* grid, const double* g, uint64_t* id_out);" in txt
    assert "int rtgr_grid_metric_unload(rtgr_context* ctx, uint64_t id);" in txt
    assert re.search(r"#define RTGR_ABI_VERSION 4\b", txt)


def test_ctypes_and_a_c_caller_agree_with_the_header(tmp_path):
    assert abi.GRID == 4 and abi.RAY_OUTSIDE == 5
    assert C.sizeof(abi.rtgr_grid) == 64
    assert (abi.rtgr_grid.n.offset, abi.rtgr_grid.pad.offset, abi.rtgr_grid.origin.offset, abi.rtgr_grid.spacing.offset) == (0, 12, 16, 40)
    assert {"rtgr_grid_metric_load", "rtgr_grid_metric_unload"} <= set(abi.EXPORTS)
    exe = str(tmp_path / "grid_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "grid_layout.c"), "-o", exe, "-ldl"])
    out = subprocess.check_output([exe, abi.LIB_PATH], text=True).split()   # (exit 2: the library does not export the calls)
    assert dict(zip(out[0::2], map(int, out[1::2]))) == {"grid": 64, "n": 0, "pad": 12, "origin": 16, "spacing": 40, "RTGR_GRID": 4,
                                                         "RTGR_RAY_OUTSIDE": 5}
    lib = abi.load()
    assert hasattr(lib, "rtgr_grid_metric_load") and hasattr(lib, "rtgr_grid_metric_unload")


def test_grid_metric_checks_its_arguments_before_any_gpu_call():
    good = np.broadcast_to(ETA, (4, 5, 6, 10))
    with pytest.raises(ValueError, match="shape"):
        rt.GridMetric(np.zeros((4, 5, 6, 9)), (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="shape"):
        rt.GridMetric(np.zeros((4, 5, 10)), (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="at least 4"):
        rt.GridMetric(np.broadcast_to(ETA, (3, 5, 6, 10)), (0, 0, 0), 1.0)
    for bad in (0.0, -1.0, (1.0, 0.0, 1.0), np.nan):
        with pytest.raises(ValueError, match="spacing"):
            rt.GridMetric(good, (0, 0, 0), bad)
    g = good.copy()
    g[2, 3, 4, 7] = np.nan
    with pytest.raises(ValueError, match=f"sample {(2 * 5 + 3) * 6 + 4}"):
        rt.GridMetric(g, (0, 0, 0), 1.0)
    # the 4x4 form: the upper triangle is taken
    m = rt.GridMetric(np.broadcast_to(np.diag([-1.0, 1, 1, 1]), (4, 5, 6, 4, 4)), (0, 0, 0), (1, 2, 3))
    assert np.array_equal(m.g, good) and m.n == (6, 5, 4)


def test_make_scene_with_a_grid_metric_touches_no_gpu():
    m = rt.GridMetric(np.broadcast_to(ETA, (4, 4, 4, 10)), (0, 0, 0), 1.0)
    metric, objs, _ = rt.example1_scene()
    sc = rt.make_scene(m, objs, units=False)
    assert sc.metric == 4 and sc.metric == abi.GRID and sc.user_metric == 0 and sc.nobj == 3


def test_julia_stub_has_the_grid_metric():
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    assert re.search(r"^const RTGR_GRID = UInt32\(4\)$", jl, re.M) and re.search(r"^const RTGR_RAY_OUTSIDE = UInt8\(5\)$", jl, re.M)
    body = re.search(r"^struct RtgrGrid\b.*?\n(.*?)^end", jl, re.M | re.S).group(1)
    fields = re.findall(r"^\s*(\w+)::", body, re.M)
    assert fields == ["n", "pad", "origin", "spacing"]
    assert re.search(r"^#\s+RtgrGrid\s+64\s+n 0, pad 12, origin 16, spacing 40", jl, re.M)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def trace(lib, metric, objs, cam, ni, nj, dtype=np.float64, opt=None, redshift=False, ctx=None):
    sc = rt.make_scene(metric, objs, ctx)
    opt = opt or rt.solver_defaults(dtype)
    n = ni * nj
    out = dict(rgb=np.zeros((3, n), dtype), state_end=np.zeros((n, 8), dtype), lambda_end=np.zeros(n, dtype),
               status=np.zeros(n, np.uint8), hit=np.zeros(n, np.uint8), n_accept=np.zeros(n, np.uint32), n_reject=np.zeros(n, np.uint32))
    if redshift:
        out["redshift"] = np.zeros(n, dtype)
    o = abi.rtgr_ray_outputs()
    for k in ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject", "redshift"):
        if k in out:
            setattr(o, k, out[k].ctypes.data)
    ctr = abi.rtgr_counters()
    fn = lib.rtgr_trace_f64 if dtype == np.float64 else lib.rtgr_trace_f32
    abi.check(lib, fn(ctx, C.byref(sc), C.byref(opt), None, C.byref(cam), ni, nj, 0, nj, out["rgb"].ctypes.data, C.byref(o), C.byref(ctr)))
    out["counters"] = ctr.as_dict()
    return out


def ks_scene(cam_y=-4.5, width=5.0):
    """a compact Kerr-Schild scene inside a sky of radius 6: an opaque sphere of radius 2.2 over the hole, a small sphere in front,
    the far plane; an orthographic camera as the reference's make_canvas builds it"""
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(-20.0), rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), 2.2),
            rt.Sphere((0, 2.0, -3.0, 1.5), (1, 0, 0, 0), 0.6)]
    cam = rt.make_camera(pos=(0, 0, cam_y, 0), widthx=(0, width, 0, 0), widthy=(0, 0, 0, width), normal=(0, 0, 1, 0))
    return objs, cam


@pytest.mark.gpu
def test_quadratics_are_reproduced_exactly(lib):
    """Catmull-Rom reproduces quadratics: g = eta + a small quadratic polynomial per component, sampled, comes back with its exact
    derivatives at random points of the valid box (Float64 to 1e-12, Float32 to 1e-5)."""
    rng = np.random.default_rng(1)
    coef = rng.uniform(-0.02, 0.02, size=(10, 10))   # per component: 1 x y z xx yy zz xy xz yz

    def poly(x, y, z):
        mon = [np.ones_like(x), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z]
        return ETA + np.stack([sum(coef[c, m] * mon[m] for m in range(10)) for c in range(10)], axis=-1)

    def dpoly(x, y, z):
        one, zero = np.ones_like(x), np.zeros_like(x)
        dm = [[zero, one, zero, zero, 2 * x, zero, zero, y, z, zero], [zero, zero, one, zero, zero, 2 * y, zero, x, zero, z],
              [zero, zero, zero, one, zero, zero, 2 * z, zero, x, y]]
        return np.stack([np.stack([sum(coef[c, m] * dm[j][m] for m in range(10)) for c in range(10)], axis=-1) for j in range(3)], axis=1)

    origin, h, n = (-1.3, -0.7, -2.0), (0.25, 0.2, 0.3), (14, 12, 15)
    m = rt.GridMetric(sample(poly, origin, h, n), origin, h)
    lo = np.array([origin[a] + h[a] for a in range(3)])
    hi = np.array([origin[a] + (n[a] - 2) * h[a] for a in range(3)])
    pts = lo + rng.uniform(size=(500, 3)) * (hi - lo)
    x4 = np.concatenate([rng.uniform(-5, 5, size=(500, 1)), pts], axis=1)
    g, dg = rt.dmetric(m, x4)
    assert np.abs(g - to4(poly(*pts.T))).max() < 1e-12
    want = to4(dpoly(*pts.T))            # (n, 3, 4, 4): d_j g_ab
    assert (dg[..., 0] == 0).all()       # stationary
    assert np.abs(np.moveaxis(dg[..., 1:], -1, 1) - want).max() < 1e-12
    g32, dg32 = rt.dmetric(m, x4, dtype=np.float32)
    assert np.abs(g32 - to4(poly(*pts.T))).max() < 1e-5
    assert np.abs(np.moveaxis(dg32[..., 1:], -1, 1) - want).max() < 1e-5


@pytest.mark.gpu
def test_interpolant_is_the_one_specified(lib):
    """On random Lorentzian samples the device's g and dg are the numpy Catmull-Rom of this file to 1e-13 (relative to the data's
    scale), inside the valid box and — extrapolated from the clamped cell — outside it; the Christoffel symbols follow."""
    rng = np.random.default_rng(2)
    origin, h, n = (0.5, -1.0, 2.0), (0.3, 0.35, 0.25), (9, 11, 8)
    samples = ETA + rng.uniform(-0.05, 0.05, size=(n[2], n[1], n[0], 10))
    m = rt.GridMetric(samples, origin, h)
    span = np.array([(n[a] - 1) * h[a] for a in range(3)])
    pts = np.array(origin) + rng.uniform(-0.1, 1.1, size=(400, 3)) * span
    x4 = np.concatenate([np.zeros((400, 1)), pts], axis=1)
    g, dg = rt.dmetric(m, x4)
    gr, dgr = catmull_rom(samples, origin, h, pts)
    assert np.abs(g - to4(gr)).max() <= 1e-13 * np.abs(gr).max()
    d = np.moveaxis(dg[..., 1:], -1, 1)
    assert np.abs(d - to4(dgr)).max() <= 1e-13 * np.abs(dgr).max()
    Gam = rt.christoffel(m, x4)
    gu = np.linalg.inv(to4(gr))
    dd = np.moveaxis(to4(dgr), 1, -1)    # dd[n, a, b, c] = d_c g_ab, c = 1..3
    dd = np.concatenate([np.zeros(dd.shape[:-1] + (1,)), dd], axis=-1)
    G = 0.5 * np.einsum("nad,ndbc->nabc", gu, dd + np.swapaxes(dd, 2, 3) - np.moveaxis(dd, 3, 1))
    assert np.abs(Gam - G).max() <= 1e-10 * max(1.0, np.abs(G).max())   # (through two 4x4 inverses: conditioning, not the interpolant)


@pytest.mark.gpu
def test_flat_grid_is_minkowski(lib):
    """A grid that holds eta: the RHS is exactly 0 on every path, and example1 traced through it is the built-in minkowski frame
    (same hit map, RGB within 1e-9) and passes the sphere.png pin on the same pixels as the built-in path."""
    from raytracegr_jl_amd.png import read_png
    m = flat_grid()
    rng = np.random.default_rng(3)
    s = np.concatenate([np.zeros((64, 1)), rng.uniform(-10, 10, size=(64, 3)), rng.normal(size=(64, 4))], axis=1)
    for path in (0, 1, 2):
        ds = rt.geodesic(s, m, path=path)
        assert np.array_equal(ds[:, :4], s[:, 4:]) and (ds[:, 4:] == 0).all(), path
    metric, objs, cam = rt.example1_scene()
    cam = rt.make_camera(**cam)
    a = trace(lib, metric, objs, cam, 200, 200)
    b = trace(lib, m, objs, cam, 200, 200)
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["status"], b["status"])
    assert np.abs(a["rgb"] - b["rgb"]).max() <= 1e-9
    gold = read_png(os.path.join(ROOT, "tests", "golden", "sphere.png"))
    assert np.array_equal((_image(a["rgb"], 200, 200) == gold).all(axis=2), (_image(b["rgb"], 200, 200) == gold).all(axis=2))


def _image(rgb, ni, nj):
    """rgb[3, ni*nj] -> N0f8 image[j, i, c] (the layout of save(colorview(...)))"""
    a = np.rint(np.clip(rgb, 0, 1) * 255.0).astype(np.uint8).reshape(3, nj, ni)
    return np.ascontiguousarray(np.transpose(a, (1, 2, 0)))


@pytest.fixture(scope="module")
def ks_grids():
    return {0.2: ks_grid(0.2), 0.1: ks_grid(0.1)}


@pytest.mark.gpu
def test_kerr_schild_on_a_grid_converges_to_the_closed_form(lib, ks_grids):
    """KerrSchild(1, 0.8) sampled at h = 0.2 and h = 0.1 against the closed form at 128²: >= 99 % of the hit map agrees, and the max RGB
    error over the pixels that end on the same object falls by >= 3 when h halves (second-order derivatives: about 4)."""
    objs, cam = ks_scene()
    ref = trace(lib, rt.KerrSchild(1.0, 0.8), objs, cam, 128, 128)
    errs = {}
    for h, m in ks_grids.items():
        o = trace(lib, m, objs, cam, 128, 128)
        assert (o["status"] != abi.RAY_OUTSIDE).all()
        same = (o["hit"] == ref["hit"]) & (o["status"] == abi.RAY_EVENT) & (ref["status"] == abi.RAY_EVENT)
        assert np.mean(o["hit"] == ref["hit"]) >= 0.99, (h, np.mean(o["hit"] == ref["hit"]))
        errs[h] = wrap_aware_rgb_err(o["rgb"][:, same], ref["rgb"][:, same], o["hit"][same], nobj=len(objs))
    assert errs[0.2] >= 3 * errs[0.1], errs


@pytest.mark.gpu
def test_full_pass_equals_far_plus_near_on_a_grid(lib, ks_grids):
    objs, cam = ks_scene()
    m = ks_grids[0.2]
    with abi.options(lib, split=0):
        full = trace(lib, m, objs, cam, 96, 96)
    with abi.options(lib, split=1):
        pair = trace(lib, m, objs, cam, 96, 96)
    for k in ("rgb", "state_end", "lambda_end", "status", "hit", "n_accept", "n_reject"):
        assert np.array_equal(full[k], pair[k]), k


@pytest.mark.gpu
def test_rays_that_leave_the_grid_end_outside(lib, ks_grids):
    """A grid smaller than the sky (valid box [-4, 4]^3, the sky at radius 6): rays that leave end RTGR_RAY_OUTSIDE with the miss
    colour and count as not finished; rays that end in an event inside the box are those of a larger grid of the same field; a camera
    outside the box gives OUTSIDE with 0 steps.
    (The field is Kerr-Schild switched off smoothly before rho = 3.2: a step's stages — and a rejected attempt's — may reach beyond the
    small grid's box, where it extrapolates; with the plain Kerr-Schild field the two grids then differ there, the error controller
    takes other steps and the frames differ at the tolerance's level (2.6e-7 in RGB).  With flat space beyond rho = 3.2 both grids
    return eta there exactly.  The larger grid has the same origin and more samples, so inside the small box both compute the same
    cell and fraction from the same samples.)"""
    small = ks_grid(0.2, L=4.0, fn=kerr_schild_island)
    objs, cam = ks_scene(cam_y=-3.5, width=5.0)
    o = trace(lib, small, objs, cam, 96, 96)
    larger = rt.GridMetric(sample(kerr_schild_island, small.origin, (0.2,) * 3, (70, 70, 70)), small.origin, 0.2)
    assert np.array_equal(larger.g[:small.n[2], :small.n[1], :small.n[0]], small.g)
    big = trace(lib, larger, objs, cam, 96, 96)
    out = o["status"] == abi.RAY_OUTSIDE
    assert 0.05 < out.mean() < 0.95
    # coloured like a ray that reached lambda1: the colour rule at the end point — the miss colour, unless the step ended within
    # hit_threshold of an object (a few rays leave through a corner of the box just short of the sky sphere)
    miss = out & (o["hit"] == 0)
    assert miss.sum() >= 0.99 * out.sum() and (o["rgb"][:, miss] == np.array(rt.solver_defaults().miss_rgb)[:, None]).all()
    assert o["counters"]["not_finished"] == int((o["status"] >= abi.RAY_MAXSTEPS).sum())
    assert (np.abs(o["state_end"][out, 1:4]).max(axis=1) > 4.0).all()       # the end of the step that left
    ev = o["status"] == abi.RAY_EVENT
    assert ev.sum() > 1000 and np.array_equal(o["hit"][ev], big["hit"][ev])
    assert np.abs(o["rgb"][:, ev] - big["rgb"][:, ev]).max() <= 1e-12
    assert np.abs(o["lambda_end"][ev] - big["lambda_end"][ev]).max() <= 1e-12
    objs, cam = ks_scene(cam_y=-5.0, width=5.0)
    o = trace(lib, small, objs, cam, 16, 16)
    assert (o["status"] == abi.RAY_OUTSIDE).all() and (o["n_accept"] == 0).all() and o["counters"]["not_finished"] == 256


@pytest.mark.gpu
def test_float32_grid_frame_agrees_with_float64(lib, ks_grids):
    objs, cam = ks_scene()
    m = ks_grids[0.2]
    a = trace(lib, m, objs, cam, 128, 128)
    b = trace(lib, m, objs, cam, 128, 128, dtype=np.float32)
    assert np.mean(a["hit"] == b["hit"]) >= 0.99


@pytest.mark.gpu
def test_every_entry_point_traces_a_grid_scene(lib, ks_grids):
    """device entry, host-pointer entry, frames in flight and the sharded entry over a context of two logical devices give the same
    frame; redshift on the flat grid equals the built-in Minkowski redshift to 1e-12."""
    import torch
    objs, cam = ks_scene()
    m = ks_grids[0.2]
    ni = nj = 64
    host = trace(lib, m, objs, cam, ni, nj)["rgb"]
    sc, opt = rt.make_scene(m, objs), rt.solver_defaults()
    d = torch.zeros((3, ni * nj), dtype=torch.float64, device="cuda")
    abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), ni, nj, 0, nj, d.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), host)
    frames = rt.trace_frames(m, objs, [cam, cam], ni, nj)
    for f in frames:
        assert np.array_equal(f["rgb"], host)
    ctx = abi.create_context(lib, [0, 0])
    try:
        scx = rt.make_scene(m, objs, ctx)
        rgb = np.zeros((3, ni * nj))
        abi.check(lib, lib.rtgr_trace_sharded_f64(ctx, C.byref(scx), C.byref(opt), C.byref(cam), ni, nj, rgb.ctypes.data, None, None))
        assert np.array_equal(rgb, host)
        dd = torch.zeros((3, ni * nj), dtype=torch.float64, device="cuda")
        abi.check(lib, lib.rtgr_trace_sharded_device_f64(ctx, C.byref(scx), C.byref(opt), C.byref(cam), ni, nj, dd.data_ptr(), None, None))
        torch.cuda.synchronize()
        assert np.array_equal(dd.cpu().numpy(), host)
    finally:
        lib.rtgr_destroy(ctx)
    metric, objs1, cam1 = rt.example1_scene()
    cam1 = rt.make_camera(**cam1)
    a = trace(lib, metric, objs1, cam1, 64, 64, redshift=True)
    b = trace(lib, flat_grid(), objs1, cam1, 64, 64, redshift=True)
    ok = np.isfinite(a["redshift"])
    assert ok.sum() > 100 and np.array_equal(ok, np.isfinite(b["redshift"]))
    assert np.abs(a["redshift"][ok] - b["redshift"][ok]).max() <= 1e-12


@pytest.mark.gpu
def test_grid_lifetime_unload_capture_trim(lib):
    """unload -> a scene naming the id fails with RTGR_ERR_BAD_ARG naming it; a hipGraph captured before the unload still replays the
    same frame (the samples were retired, not freed); rtgr_trim then releases them; user objects in a grid scene are refused."""
    import torch
    from raytracegr_jl_amd import sharded
    hook = lib.rtgr_testhook_grid_tables
    hook.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    res, ret = C.c_uint32(), C.c_uint32()
    abi.check(lib, lib.rtgr_trim(None))
    m = ks_grid(0.25, L=6.5)
    objs, cam = ks_scene()
    sc, opt = rt.make_scene(m, objs), rt.solver_defaults()
    gid = sc.user_metric
    ni = nj = 48
    side = torch.cuda.Stream()
    out = {"rgb": torch.zeros((3, ni * nj), dtype=torch.float64, device="cuda")}
    abi.check(lib, lib.rtgr_reserve_workspace(None, out["rgb"].data_ptr(), side.cuda_stream, ni * nj, 0, 0))
    eager = sharded.trace_slab_torch(sc, opt, cam, ni, nj, 0, nj)["rgb"].clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        sharded.trace_slab_torch(sc, opt, cam, ni, nj, 0, nj, out=out)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["rgb"], eager)
    abi.check(lib, hook(None, 0, C.byref(res), C.byref(ret)))
    n_res = res.value
    m.unload()
    abi.check(lib, hook(None, 0, C.byref(res), C.byref(ret)))
    assert (res.value, ret.value) == (n_res - 1, 1)
    rgb = np.zeros((3, ni * nj))
    rc = lib.rtgr_trace_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), ni, nj, 0, nj, rgb.ctypes.data, None, None)
    assert rc == abi.ERR_BAD_ARG and str(gid).encode() in lib.rtgr_last_error()
    out["rgb"].zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["rgb"], eager)
    del g
    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, hook(None, 0, C.byref(res), C.byref(ret)))
    assert ret.value == 0
    assert lib.rtgr_grid_metric_unload(None, gid) == abi.ERR_BAD_ARG
    # user objects beside a grid metric: out of scope, refused with a message
    m2 = flat_grid()
    sc2 = rt.make_scene(m2, objs)
    sc2.obj[3].kind = abi.USER_OBJECT
    rc = lib.rtgr_trace_f64(None, C.byref(sc2), C.byref(opt), None, C.byref(cam), 8, 8, 0, 8, rgb.ctypes.data, None, None)
    assert rc == abi.ERR_BAD_ARG and b"user objects" in lib.rtgr_last_error()
    # bad samples are refused with the index of the first bad one
    bad = m2.g.copy()
    bad[1, 2, 3] = ETA * np.array([1, 0, 0, 0, 1, 0, 0, 1, 0, -1])   # det g > 0
    desc = abi.rtgr_grid()
    for a in range(3):
        desc.n[a], desc.origin[a], desc.spacing[a] = m2.n[a], m2.origin[a], m2.spacing[a]
    gid2 = C.c_uint64()
    assert lib.rtgr_grid_metric_load(None, C.byref(desc), bad.ctypes.data, C.byref(gid2)) == abi.ERR_BAD_ARG
    assert f"sample {(1 * m2.n[1] + 2) * m2.n[0] + 3} ".encode() in lib.rtgr_last_error()


@pytest.mark.gpu
def test_sample_metric_samples_a_builtin_metric(lib):
    origin, h, n = (-3.0, 2.0, -1.0), (0.5, 0.25, 0.4), (5, 6, 4)
    s = rt.sample_metric(rt.KerrSchild(1.0, 0.8), origin, h, n)
    assert s.shape == (4, 6, 5, 10)
    assert np.abs(s - sample(kerr_schild, origin, h, n)).max() < 1e-13
