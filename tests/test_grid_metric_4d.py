"""Time-dependent metrics sampled on a 4-D grid (rtgr_grid4_metric_load, include/rtgr.h): an evolving spacetime given as numbers on a
uniform (t, x, y, z) grid, interpolated on the device (Catmull-Rom on all four axes) at every stage's own t.  CPU tests: the ABI
(header, ctypes, a gcc-compiled caller, the Julia stub) and the Python checks.  GPU tests (`pytest -m gpu`): the interpolant, the
time-constant grid against the 3-D grid bit for bit, convergence to a time-dependent closed form, OUTSIDE on the time axis, both pass
structures, Float32, every entry point, lifetime."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from scenes import rt, wrap_aware_rgb_err
from test_grid_metric import ETA, _image, cr_weights, flat, kerr_schild, ks_grid, ks_scene, sample, to4, trace

abi = rt._abi


def stack_slices(g3, nt):
    """a time-constant 4-D grid: nt copies of one (nz, ny, nx, 10) slice"""
    return np.ascontiguousarray(np.broadcast_to(g3, (nt,) + g3.shape))


def sample4(fn, origin, h, n):
    """(nt, nz, ny, nx, 10) samples of fn(t, x, y, z) -> (..., 10); origin, h, n in the order (t, x, y, z)"""
    ts, xs, ys, zs = (origin[a] + h[a] * np.arange(n[a]) for a in range(4))
    t, z, y, x = np.meshgrid(ts, zs, ys, xs, indexing="ij")
    return fn(t, x, y, z)


def catmull_rom4(samples, origin, h, pts):
    """g (n, 10) and dg (n, 4, 10) = d/dt, d/dx, d/dy, d/dz at 4-D points pts (n, 4): the tensor product of the 1-D weights"""
    nt, nz, ny, nx, _ = samples.shape
    n = (nt, nx, ny, nz)
    idx, W, DW = [], [], []
    for a in range(4):
        s = (pts[:, a] - origin[a]) / h[a]
        i = np.clip(np.floor(s), 1, n[a] - 3).astype(int)
        w, dw = cr_weights(s - i)
        idx.append(i - 1)
        W.append(w)
        DW.append(dw / h[a])
    g = np.zeros((len(pts), 10))
    dg = np.zeros((len(pts), 4, 10))
    for kt in range(4):
        for kz in range(4):
            for ky in range(4):
                for kx in range(4):
                    v = samples[idx[0] + kt, idx[3] + kz, idx[2] + ky, idx[1] + kx]
                    w = [W[0][:, kt], W[1][:, kx], W[2][:, ky], W[3][:, kz]]
                    dw = [DW[0][:, kt], DW[1][:, kx], DW[2][:, ky], DW[3][:, kz]]
                    g += (w[0] * w[1] * w[2] * w[3])[:, None] * v
                    for j in range(4):
                        f = np.prod([dw[a] if a == j else w[a] for a in range(4)], axis=0)
                        dg[:, j] += f[:, None] * v
    return g, dg


def grid4(g3, nt, t0, ht, origin, h, name="grid4"):
    """a time-constant 4-D grid of slice g3 whose time samples start at t0"""
    return rt.GridMetric(stack_slices(g3, nt), (t0,) + tuple(np.broadcast_to(origin, (3,))), (ht,) + tuple(np.broadcast_to(h, (3,))),
                         name=name)


# ---- the ABI (no GPU) -------------------------------------------------------------------------------------------------------
def test_header_declares_the_4d_grid_metric():
    txt = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    assert re.search(r"typedef struct rtgr_grid4 \{\s*uint32_t n\[4\];.*?double origin\[4\];.*?double spacing\[4\];.*?\} rtgr_grid4;", txt, re.S)
    assert "int rtgr_grid4_metric_load(rtgr_context* ctx, const rtgr_grid4* grid, const double* g, uint64_t* id_out);" in txt
    assert re.search(r"#define RTGR_ABI_VERSION 4\b", txt)
    out_of_scope = re.search(r"Out of scope:(.*?)\.", txt, re.S).group(1)
    assert "time-dependent" not in out_of_scope


def test_ctypes_and_a_c_caller_agree_on_rtgr_grid4(tmp_path):
    assert C.sizeof(abi.rtgr_grid4) == 80
    assert (abi.rtgr_grid4.n.offset, abi.rtgr_grid4.origin.offset, abi.rtgr_grid4.spacing.offset) == (0, 16, 48)
    assert "rtgr_grid4_metric_load" in abi.EXPORTS
    exe = str(tmp_path / "grid4_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "grid4_layout.c"), "-o", exe, "-ldl"])
    out = subprocess.check_output([exe, abi.LIB_PATH], text=True).split()   # (exit 2: the library does not export the call)
    assert dict(zip(out[0::2], map(int, out[1::2]))) == {"grid4": 80, "n": 0, "origin": 16, "spacing": 48}
    assert hasattr(abi.load(), "rtgr_grid4_metric_load")


def test_4d_grid_metric_checks_its_arguments_before_any_gpu_call(monkeypatch):
    monkeypatch.setattr(rt.api, "_lib", lambda: pytest.fail("a GPU call"))
    good = np.broadcast_to(ETA, (4, 5, 6, 7, 10))
    m = rt.GridMetric(good, (0, 0, 0, 0), (0.5, 1, 2, 3))
    assert m.time_dependent and m.n == (4, 7, 6, 5) and m.g.shape == (4, 5, 6, 7, 10)
    assert m.box()[0] == (0.5, 1.0)
    with pytest.raises(ValueError, match="shape"):
        rt.GridMetric(np.zeros((4, 5, 6, 7, 9)), (0, 0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="shape"):
        rt.GridMetric(np.zeros((2, 4, 5, 6, 7, 10)), (0, 0, 0, 0), 1.0)
    for shape in ((3, 5, 6, 7, 10), (4, 5, 6, 3, 10)):
        with pytest.raises(ValueError, match="at least 4"):
            rt.GridMetric(np.broadcast_to(ETA, shape), (0, 0, 0, 0), 1.0)
    for bad in (0.0, -1.0, (1.0, 1.0, 0.0, 1.0), (-0.5, 1, 1, 1), np.nan, np.inf):
        with pytest.raises(ValueError, match="spacing"):
            rt.GridMetric(good, (0, 0, 0, 0), bad)
    with pytest.raises(ValueError):
        rt.GridMetric(good, (0, 0, 0), 1.0)            # a 3-component origin for a 4-D grid
    g = good.copy()
    g[2, 3, 4, 5, 7] = np.inf
    with pytest.raises(ValueError, match=f"sample {((2 * 5 + 3) * 6 + 4) * 7 + 5}"):
        rt.GridMetric(g, (0, 0, 0, 0), 1.0)
    big = np.lib.stride_tricks.as_strided(np.zeros(10), shape=(1 << 7, 1 << 7, 1 << 7, 1 << 8, 10), strides=(0, 0, 0, 0, 8))
    with pytest.raises(ValueError, match="RTGR_GRID_MAX_SAMPLES"):
        rt.GridMetric(big, (0, 0, 0, 0), 1.0)
    # the 4x4 form: the upper triangle is taken; 3-D input is what it was
    m = rt.GridMetric(np.broadcast_to(np.diag([-1.0, 1, 1, 1]), (4, 4, 5, 6, 4, 4)), (0, 0, 0, 0), 1.0)
    assert m.time_dependent and np.array_equal(m.g, np.broadcast_to(ETA, (4, 4, 5, 6, 10))) and m.n == (4, 6, 5, 4)
    m3 = rt.GridMetric(np.broadcast_to(ETA, (4, 5, 6, 10)), (0, 0, 0), 1.0)
    assert not m3.time_dependent and m3.n == (6, 5, 4)
    sc = rt.make_scene(m, [], units=False)
    assert sc.metric == abi.GRID and sc.user_metric == 0


def test_julia_stub_has_the_4d_grid_metric():
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    body = re.search(r"^struct RtgrGrid4\b.*?\n(.*?)^end", jl, re.M | re.S).group(1)
    assert re.findall(r"^\s*(\w+)::", body, re.M) == ["n", "origin", "spacing"]
    assert re.search(r"^#\s+RtgrGrid4\s+80\s+n 0, origin 16, spacing 48", jl, re.M)
    assert ":rtgr_grid4_metric_load" in jl and re.search(r"^function GridMetric\(g::AbstractArray\{<:Real,5\}", jl, re.M)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


@pytest.mark.gpu
def test_quadratics_in_t_x_y_z_are_reproduced_exactly(lib):
    """Degree <= 2 in (t, x, y, z), the cross terms t·x, t·y, t·z included: g and all four partials come back exactly at random points
    of the valid box (Float64 to 1e-12, Float32 to 1e-5)."""
    rng = np.random.default_rng(11)
    coef = rng.uniform(-0.02, 0.02, size=(10, 15))   # 1 t x y z tt xx yy zz tx ty tz xy xz yz

    def mono(t, x, y, z):
        return [np.ones_like(x), t, x, y, z, t * t, x * x, y * y, z * z, t * x, t * y, t * z, x * y, x * z, y * z]

    def dmono(t, x, y, z):
        o, z0 = np.ones_like(x), np.zeros_like(x)
        return [[z0, o, z0, z0, z0, 2 * t, z0, z0, z0, x, y, z, z0, z0, z0],
                [z0, z0, o, z0, z0, z0, 2 * x, z0, z0, t, z0, z0, y, z, z0],
                [z0, z0, z0, o, z0, z0, z0, 2 * y, z0, z0, t, z0, x, z0, z],
                [z0, z0, z0, z0, o, z0, z0, z0, 2 * z, z0, z0, t, z0, x, y]]

    def poly(t, x, y, z):
        m = mono(t, x, y, z)
        return ETA + np.stack([sum(coef[c, k] * m[k] for k in range(15)) for c in range(10)], axis=-1)

    origin, h, n = (-2.0, -1.3, -0.7, -2.0), (0.5, 0.25, 0.2, 0.3), (7, 12, 10, 13)
    m = rt.GridMetric(sample4(poly, origin, h, n), origin, h)
    lo = np.array([origin[a] + h[a] for a in range(4)])
    hi = np.array([origin[a] + (n[a] - 2) * h[a] for a in range(4)])
    x4 = lo + rng.uniform(size=(500, 4)) * (hi - lo)
    want_g = to4(poly(*x4.T))
    dm = dmono(*x4.T)
    want_d = np.stack([to4(np.stack([sum(coef[c, k] * dm[j][k] for k in range(15)) for c in range(10)], axis=-1)) for j in range(4)], -1)
    g, dg = rt.dmetric(m, x4)
    assert np.abs(g - want_g).max() < 1e-12 and np.abs(dg - want_d).max() < 1e-12
    assert np.abs(dg[..., 0]).max() > 1e-3                                      # d_t g is really there
    g32, dg32 = rt.dmetric(m, x4, dtype=np.float32)
    assert np.abs(g32 - want_g).max() < 1e-5 and np.abs(dg32 - want_d).max() < 1e-5


@pytest.mark.gpu
def test_4d_interpolant_is_the_one_specified(lib):
    """Random Lorentzian samples: the device's g and four partials are the numpy 4-D Catmull-Rom of this file to 1e-13 relative, inside
    the valid box and extrapolated outside it (t too); the Christoffel symbols (with d_t g) follow."""
    rng = np.random.default_rng(12)
    origin, h, n = (-1.0, 0.5, -1.0, 2.0), (0.7, 0.3, 0.35, 0.25), (6, 9, 8, 7)
    samples = ETA + rng.uniform(-0.05, 0.05, size=(n[0], n[3], n[2], n[1], 10))
    m = rt.GridMetric(samples, origin, h)
    span = np.array([(n[a] - 1) * h[a] for a in range(4)])
    x4 = np.array(origin) + rng.uniform(-0.1, 1.1, size=(400, 4)) * span
    g, dg = rt.dmetric(m, x4)
    gr, dgr = catmull_rom4(samples, origin, h, x4)
    assert np.abs(g - to4(gr)).max() <= 1e-13 * np.abs(gr).max()
    d = np.moveaxis(dg, -1, 1)                                                 # (n, 4, 4, 4): d_j g_ab
    assert np.abs(d - to4(dgr)).max() <= 1e-13 * np.abs(dgr).max()
    Gam = rt.christoffel(m, x4)
    gu = np.linalg.inv(to4(gr))
    dd = np.moveaxis(to4(dgr), 1, -1)                                          # dd[n, a, b, c] = d_c g_ab
    G = 0.5 * np.einsum("nad,ndbc->nabc", gu, dd + np.swapaxes(dd, 2, 3) - np.moveaxis(dd, 3, 1))
    assert np.abs(Gam - G).max() <= 1e-10 * max(1.0, np.abs(G).max())


@pytest.mark.gpu
def test_4d_geodesic_rhs_is_minus_christoffel_u_u_at_the_states_own_t(lib):
    """rtgr_eval_geodesic on a 4-D grid — every path is the integrate loop's own RHS, evaluated at the state's t — against
    (u, −Γ^a_bc u^b u^c) with Γ built from the numpy 4-D Catmull-Rom, ∂_t g included."""
    rng = np.random.default_rng(15)
    origin, h, n = (-1.0, 0.5, -1.0, 2.0), (0.7, 0.3, 0.35, 0.25), (6, 9, 8, 7)
    samples = ETA + rng.uniform(-0.05, 0.05, size=(n[0], n[3], n[2], n[1], 10))
    m = rt.GridMetric(samples, origin, h)
    lo = np.array([origin[a] + h[a] for a in range(4)])
    hi = np.array([origin[a] + (n[a] - 2) * h[a] for a in range(4)])
    x4 = lo + rng.uniform(size=(300, 4)) * (hi - lo)
    u = rng.normal(size=(300, 4))
    gr, dgr = catmull_rom4(samples, origin, h, x4)
    gu = np.linalg.inv(to4(gr))
    dd = np.moveaxis(to4(dgr), 1, -1)                                          # dd[n, a, b, c] = d_c g_ab
    G = 0.5 * np.einsum("nad,ndbc->nabc", gu, dd + np.swapaxes(dd, 2, 3) - np.moveaxis(dd, 3, 1))
    want = -np.einsum("nabc,nb,nc->na", G, u, u)
    assert np.abs(dgr[:, 0]).max() > 1e-3                                      # (d_t g matters)
    s = np.concatenate([x4, u], axis=1)
    scale = np.abs(want).max(axis=1, keepdims=True) + 1e-300
    for path in (0, 1, 2):
        ds = rt.geodesic(s, m, path=path)
        assert np.array_equal(ds[:, :4], u), path
        assert (np.abs(ds[:, 4:] - want) / scale).max() <= 1e-10, path
    # the same states at another t: a different RHS (the time axis is read)
    s2 = s.copy()
    s2[:, 0] = lo[0] + hi[0] - s[:, 0]
    assert np.abs(rt.geodesic(s2, m, path=2)[:, 4:] - rt.geodesic(s, m, path=2)[:, 4:]).max() > 1e-4


@pytest.mark.gpu
def test_the_sample_cap_is_checked_without_overflow(lib):
    """n_t·n_x·n_y·n_z is bounded by RTGR_GRID_MAX_SAMPLES even where the product of four axes of up to 2^20 samples would wrap a
    64-bit integer (2^16 per axis: exactly 2^64).  Load only: the call must refuse before it reads the (tiny) buffer."""
    tiny = np.broadcast_to(ETA, (4, 10)).copy()
    gid = C.c_uint64(0)
    for n in ((1 << 16,) * 4, (1 << 20, 1 << 20, 1 << 20, 16), (16, 1 << 20, 1 << 20, 1 << 20), (1 << 8, 1 << 8, 1 << 8, 1 << 5)):
        desc = abi.rtgr_grid4()
        for a in range(4):
            desc.n[a], desc.origin[a], desc.spacing[a] = n[a], 0.0, 1.0
        assert lib.rtgr_grid4_metric_load(None, C.byref(desc), tiny.ctypes.data, C.byref(gid)) == abi.ERR_BAD_ARG, n
        assert b"RTGR_GRID_MAX_SAMPLES" in lib.rtgr_last_error(), n
        assert gid.value == 0


@pytest.mark.gpu
def test_a_time_constant_grid_is_the_3d_grid_bit_for_bit(lib):
    """Equal slices: pointwise, g and d_x,y,z g are the 3-D grid's bit for bit and d_t g == 0 exactly (the slices are blended relative
    to the centre slice first); traced, the Kerr-Schild scene through both grids has the same status, hit and n_accept and bit-equal
    rgb and state_end; a flat 4-D grid traces example1 like the built-in Minkowski metric."""
    from raytracegr_jl_amd.png import read_png
    rng = np.random.default_rng(13)
    origin, h, n = (0.5, -1.0, 2.0), (0.3, 0.35, 0.25), (9, 11, 8)
    g3 = ETA + rng.uniform(-0.05, 0.05, size=(n[2], n[1], n[0], 10))
    m3 = rt.GridMetric(g3, origin, h)
    m4 = grid4(g3, 5, -3.0, 1.5, origin, h)
    span = np.array([(n[a] - 1) * h[a] for a in range(3)])
    pts = np.array(origin) + rng.uniform(-0.1, 1.1, size=(500, 3)) * span
    x4 = np.concatenate([rng.uniform(-4, 4, size=(500, 1)), pts], axis=1)
    for dtype in (np.float64, np.float32):
        ga, da = rt.dmetric(m3, x4, dtype=dtype)
        gb, db = rt.dmetric(m4, x4, dtype=dtype)
        assert np.array_equal(ga, gb) and np.array_equal(da[..., 1:], db[..., 1:]) and (db[..., 0] == 0).all(), dtype
    # traced
    k3 = ks_grid(0.2)
    k4 = grid4(k3.g, 5, -1000.0, 500.0, k3.origin, k3.spacing)               # valid t in [-500, 500]: every ray stays inside
    objs, cam = ks_scene()
    a, b = trace(lib, k3, objs, cam, 96, 96), trace(lib, k4, objs, cam, 96, 96)
    for k in ("status", "hit", "n_accept", "rgb", "state_end"):
        assert np.array_equal(a[k], b[k]), k
    # flat: example1 as the built-in minkowski frame (same hit map, RGB within 1e-9, the sphere.png pin on the same pixels)
    flat4 = grid4(sample(flat, (-12.0,) * 3, (1.0,) * 3, (25,) * 3), 8, -1000.0, 200.0, (-12.0,) * 3, 1.0, name="flat4")
    metric, objs1, cam1 = rt.example1_scene()
    cam1 = rt.make_camera(**cam1)
    a, b = trace(lib, metric, objs1, cam1, 200, 200), trace(lib, flat4, objs1, cam1, 200, 200)
    assert np.array_equal(a["hit"], b["hit"]) and np.array_equal(a["status"], b["status"])
    assert np.abs(a["rgb"] - b["rgb"]).max() <= 1e-9
    gold = read_png(os.path.join(ROOT, "tests", "golden", "sphere.png"))
    assert np.array_equal((_image(a["rgb"], 200, 200) == gold).all(axis=2), (_image(b["rgb"], 200, 200) == gold).all(axis=2))


H = 0.03


def expanding_grid(h, ht, L=6.6, T0=-32.0, T1=4.0):
    """examples/user_metrics.py:EXPANDING_ISOTROPIC (M = 1, H = 0.03) sampled BY THE LIBRARY from the user metric (sample_metric with a
    time axis) on a grid whose valid box is [-L, L]^3 x [T0, T1]; the singular interior (rho < 1, inside the scene's opaque sphere of
    radius 2.2, out of every stencil's reach) is replaced by eta"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import user_metrics
    user = rt.UserMetric(user_metrics.EXPANDING_ISOTROPIC, M=1.0, a=H)
    n = int(round(2 * L / h)) + 3
    nt = int(round((T1 - T0) / ht)) + 3
    origin = (-L - h,) * 3
    g = rt.sample_metric(user, origin, h, (n,) * 3, t=(T0 - ht, ht, nt))
    x = origin[0] + h * np.arange(n)
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    g[:, (xx * xx + y * y + z * z) < 1.0] = ETA
    return user, rt.GridMetric(g, (T0 - ht,) + origin, (ht, h, h, h), name=f"expanding h={h} ht={ht}")


@pytest.fixture(scope="module")
def expanding():
    user, coarse = expanding_grid(0.4, 4.0)
    _, fine = expanding_grid(0.2, 2.0)
    return user, coarse, fine


@pytest.mark.gpu
def test_a_time_dependent_grid_converges_to_its_closed_form(lib, expanding):
    """EXPANDING_ISOTROPIC sampled at (h, h_t) = (0.4, 4) and (0.2, 2) against the user metric's own frame at 128²: >= 99 % of the
    hit map agrees on the finer grid, and the max RGB error over pixels that end on the same object falls by >= 3 when h and h_t
    halve.  Sensitivity: the t = 0 slice loaded as a 3-D grid (the spacetime frozen) gives a visibly different frame."""
    user, coarse, fine = expanding
    objs, cam = ks_scene()
    ref = trace(lib, user, objs, cam, 128, 128)
    errs = {}
    for m in (coarse, fine):
        o = trace(lib, m, objs, cam, 128, 128)
        assert (o["status"] != abi.RAY_OUTSIDE).all(), m
        same = (o["hit"] == ref["hit"]) & (o["status"] == abi.RAY_EVENT) & (ref["status"] == abi.RAY_EVENT)
        errs[m.spacing[0]] = (np.mean(o["hit"] == ref["hit"]),
                              wrap_aware_rgb_err(o["rgb"][:, same], ref["rgb"][:, same], o["hit"][same], nobj=len(objs)))
    assert errs[2.0][0] >= 0.99, errs
    assert errs[4.0][1] >= 3 * errs[2.0][1], errs
    l0 = int(round((0.0 - fine.origin[0]) / fine.spacing[0]))
    assert fine.origin[0] + l0 * fine.spacing[0] == 0.0
    frozen = rt.GridMetric(fine.g[l0], fine.origin[1:], fine.spacing[1:], name="t = 0 slice")
    bad = trace(lib, frozen, objs, cam, 128, 128)
    ok = (bad["hit"] == ref["hit"]) & (ref["hit"] > 0) & (ref["status"] == abi.RAY_EVENT)
    assert (bad["hit"] != ref["hit"]).mean() > 0.05 or np.abs(bad["state_end"][ok] - ref["state_end"][ok]).max() > 1e-3


@pytest.mark.gpu
def test_rays_that_leave_the_time_range_end_outside(lib):
    """A grid whose valid time range is [-5, 1] — the rays run backwards in t from the camera at t = 0 and most need longer to reach
    the sky: those end RTGR_RAY_OUTSIDE with state_end[0] below -5, the miss colour, counted in not_finished; a camera at a t outside
    the range gives OUTSIDE with 0 steps."""
    k3 = ks_grid(0.25, L=6.5)
    m = grid4(k3.g, 10, -5.75, 0.75, k3.origin, k3.spacing)                 # valid t in [-5, 0.25]: s = 1 .. 8
    t_lo, t_hi = m.box()[0]
    assert t_lo == -5.0 and t_hi >= 0.0
    objs, cam = ks_scene()
    o = trace(lib, m, objs, cam, 96, 96)
    out = o["status"] == abi.RAY_OUTSIDE
    assert 0.05 < out.mean() < 0.95
    assert (o["state_end"][out, 0] < t_lo).all()
    miss = out & (o["hit"] == 0)
    assert miss.sum() >= 0.99 * out.sum() and (o["rgb"][:, miss] == np.array(rt.solver_defaults().miss_rgb)[:, None]).all()
    assert o["counters"]["not_finished"] == int((o["status"] >= abi.RAY_MAXSTEPS).sum())
    ref = trace(lib, k3, objs, cam, 96, 96)                                   # the same field, no time limit
    ev = o["status"] == abi.RAY_EVENT
    assert ev.sum() > 500 and np.array_equal(o["hit"][ev], ref["hit"][ev]) and np.array_equal(o["rgb"][:, ev], ref["rgb"][:, ev])
    late = rt.make_camera(pos=(t_hi + 1.0, 0, -4.5, 0), widthx=(0, 5.0, 0, 0), widthy=(0, 0, 0, 5.0), normal=(0, 0, 1, 0))
    o = trace(lib, m, objs, late, 16, 16)
    assert (o["status"] == abi.RAY_OUTSIDE).all() and (o["n_accept"] == 0).all() and o["counters"]["not_finished"] == 256


@pytest.mark.gpu
def test_full_pass_equals_far_plus_near_and_float32_on_a_4d_grid(lib, expanding):
    _, coarse, _ = expanding
    objs, cam = ks_scene()
    with abi.options(lib, split=0):
        full = trace(lib, coarse, objs, cam, 96, 96)
    with abi.options(lib, split=1):
        pair = trace(lib, coarse, objs, cam, 96, 96)
    for k in ("rgb", "state_end", "lambda_end", "status", "hit", "n_accept", "n_reject"):
        assert np.array_equal(full[k], pair[k]), k
    a = trace(lib, coarse, objs, cam, 128, 128)
    b = trace(lib, coarse, objs, cam, 128, 128, dtype=np.float32)
    assert np.mean(a["hit"] == b["hit"]) >= 0.99


@pytest.mark.gpu
def test_every_entry_point_traces_a_4d_grid_scene(lib, expanding):
    """device entry, host-pointer entry, frames in flight and the sharded entry over a context of two logical devices give the same
    frame on a time-dependent grid; redshift on a flat 4-D grid equals the built-in Minkowski redshift to 1e-12."""
    import torch
    _, coarse, _ = expanding
    objs, cam = ks_scene()
    ni = nj = 64
    host = trace(lib, coarse, objs, cam, ni, nj)["rgb"]
    sc, opt = rt.make_scene(coarse, objs), rt.solver_defaults()
    d = torch.zeros((3, ni * nj), dtype=torch.float64, device="cuda")
    abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), ni, nj, 0, nj, d.data_ptr(), None, None, None))
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), host)
    for f in rt.trace_frames(coarse, objs, [cam, cam], ni, nj):
        assert np.array_equal(f["rgb"], host)
    ctx = abi.create_context(lib, [0, 0])
    try:
        scx = rt.make_scene(coarse, objs, ctx)
        rgb = np.zeros((3, ni * nj))
        abi.check(lib, lib.rtgr_trace_sharded_f64(ctx, C.byref(scx), C.byref(opt), C.byref(cam), ni, nj, rgb.ctypes.data, None, None))
        assert np.array_equal(rgb, host)
        dd = torch.zeros((3, ni * nj), dtype=torch.float64, device="cuda")
        abi.check(lib, lib.rtgr_trace_sharded_device_f64(ctx, C.byref(scx), C.byref(opt), C.byref(cam), ni, nj, dd.data_ptr(), None, None))
        torch.cuda.synchronize()
        assert np.array_equal(dd.cpu().numpy(), host)
    finally:
        lib.rtgr_destroy(ctx)
    flat4 = grid4(sample(flat, (-12.0,) * 3, (1.0,) * 3, (25,) * 3), 8, -1000.0, 200.0, (-12.0,) * 3, 1.0, name="flat4")
    metric, objs1, cam1 = rt.example1_scene()
    cam1 = rt.make_camera(**cam1)
    a = trace(lib, metric, objs1, cam1, 64, 64, redshift=True)
    b = trace(lib, flat4, objs1, cam1, 64, 64, redshift=True)
    ok = np.isfinite(a["redshift"])
    assert ok.sum() > 100 and np.array_equal(ok, np.isfinite(b["redshift"]))
    assert np.abs(a["redshift"][ok] - b["redshift"][ok]).max() <= 1e-12


@pytest.mark.gpu
def test_4d_grid_lifetime_unload_capture_trim(lib):
    """A hipGraph captured on a 4-D grid replays the same frame after the unload (retired, not freed); rtgr_trim then releases it; a
    scene naming the unloaded id gets RTGR_ERR_BAD_ARG; a bad sample is refused with its flattened 4-D index."""
    import torch
    from raytracegr_jl_amd import sharded
    hook = lib.rtgr_testhook_grid_tables
    hook.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    res, ret = C.c_uint32(), C.c_uint32()
    abi.check(lib, lib.rtgr_trim(None))
    k3 = ks_grid(0.25, L=6.5)
    m = grid4(k3.g, 5, -1000.0, 500.0, k3.origin, k3.spacing)
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
    # a bad sample: refused with its flattened index (l, k, j, i) -> ((l n_z + k) n_y + j) n_x + i
    n = (4, 6, 5, 7)                                   # (t, x, y, z)
    bad = np.ascontiguousarray(np.broadcast_to(ETA, (n[0], n[3], n[2], n[1], 10)))
    bad[2, 3, 1, 4] = ETA * np.array([1, 0, 0, 0, 1, 0, 0, 1, 0, -1])   # det g > 0
    desc = abi.rtgr_grid4()
    for a in range(4):
        desc.n[a], desc.origin[a], desc.spacing[a] = n[a], 0.0, 1.0
    gid2 = C.c_uint64()
    assert lib.rtgr_grid4_metric_load(None, C.byref(desc), bad.ctypes.data, C.byref(gid2)) == abi.ERR_BAD_ARG
    assert f"sample {((2 * n[3] + 3) * n[2] + 1) * n[1] + 4} ".encode() in lib.rtgr_last_error()
    desc.n[0] = 3
    assert lib.rtgr_grid4_metric_load(None, C.byref(desc), bad.ctypes.data, C.byref(gid2)) == abi.ERR_BAD_ARG


@pytest.mark.gpu
def test_sample_metric_with_a_time_axis(lib):
    """sample_metric(t=(t0, ht, nt)) evaluates at the 4-D points; without it the output is the t = 0 one of old"""
    origin, h, n = (-3.0, 2.0, -1.0), (0.5, 0.25, 0.4), (5, 6, 4)
    s3 = rt.sample_metric(rt.KerrSchild(1.0, 0.8), origin, h, n)
    s4 = rt.sample_metric(rt.KerrSchild(1.0, 0.8), origin, h, n, t=(-1.0, 0.5, 3))
    assert s4.shape == (3, 4, 6, 5, 10) and all(np.array_equal(s4[l], s3) for l in range(3))   # (stationary)
    assert np.abs(s3 - sample(kerr_schild, origin, h, n)).max() < 1e-13
    rng = np.random.default_rng(14)
    g0 = ETA + rng.uniform(-0.05, 0.05, size=(6, 4, 5, 6, 10))
    m = rt.GridMetric(g0, (-1.0, 0.0, 0.0, 0.0), (0.5, 1.0, 1.0, 1.0))
    s = rt.sample_metric(m, (1.0, 1.0, 1.0), 1.0, (4, 3, 2), t=(-0.5, 0.5, 4))   # the samples of the valid box
    assert np.abs(s - g0[1:5, 1:3, 1:4, 1:5]).max() <= 1e-15                 # the interpolant interpolates (to the ulp of ref + (s - ref))
