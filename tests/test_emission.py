"""An orbiting, glowing disk (rtgr_trace_emission_*, rtgr_eval_disk_emission_*; include/rtgr.h "disk emission").

The reference has no emitters, so the judges are (1) numpy, for the model as the header states it — the metric and its derivatives taken
from the CPU oracle (oracle_lib.eval_metric / metric_plain), the orbital rate also against Kerr's closed form and, through
rtgr_eval_geodesic_f64, against the device's own geodesic equation — and (2) the library's own PLAIN frame, for everything an emitted
trace does around the model:
    emitted rgb  ==  where(hit32 == disk, rtgr_eval_disk_emission(make_canvas states, state_end).rgb, plain rgb)        bit for bit,
g likewise (NaN off the disk), every per-ray output and the counters equal to the plain call's.  With anti-aliasing: uniform == the box
filter of the emitted fine frame, refined == the edge rule on the emitted frame, adaptive == where(refined, uniform, emitted plain).
CPU part: symbols, the struct layout (ctypes and a compiled C caller), no result without a device, the Julia stub.

Recorded on an MI355X (profiles/emission/README.md): see GRID_OMEGA_RECORDED and F32_G_RECORDED below."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from conftest import ROOT
from scenes import rt
from test_textures import OUT_KEYS, _hip_runtime, _outputs, box, edge_mask, same_bits

abi = rt._abi
EMIT_EXPORTS = ("rtgr_trace_emission_device_f64", "rtgr_trace_emission_device_f32", "rtgr_trace_emission_f64", "rtgr_trace_emission_f32",
                "rtgr_eval_disk_emission_f64", "rtgr_eval_disk_emission_f32")
EPS = float(np.finfo(np.float64).eps)
# max |Omega(grid h = 0.2) / Omega(analytic) - 1| over GRID_POINTS, and max relative error of the Float32 hook's g against the Float64
# hook's over the points of the numpy test with u^t <= 4, as measured on an MI355X (profiles/emission/README.md).  The tests assert
# 4 x and 8 x these (and never more than 1e-3 for the latter).
GRID_OMEGA_RECORDED = 1.647e-3
F32_G_RECORDED = 6.743e-7

METRICS = {"ks_true08": lambda: rt.KerrSchild(1, 0.8), "ks_true0998": lambda: rt.KerrSchild(1, 0.998), "ks_true0": lambda: rt.KerrSchild(1, 0.0),
           "ks_ref0": lambda: rt.kerr_schild, "ks_ref08": lambda: rt.KerrSchild(1, 0.8, textbook=False), "mink": lambda: rt.minkowski}
SPIN = {"ks_true08": 0.8, "ks_true0998": 0.998, "ks_true0": 0.0}
RHOS = {"ks_true08": (2.2, 3.0, 6.0), "ks_true0998": (1.6, 2.0, 4.0), "ks_true0": (3.5, 6.0), "ks_ref0": (6.0,), "ks_ref08": (6.0,)}
HOOK_DISK = (0.05, 1.5, 12.0)          # the Disk of the pointwise tests: its r_in = 1.5 enters T_em only
CAM2 = rt.example2_scene()[2]
T_FRAME = 30000.0                      # T_in of the frame tests: with g of 0.2 .. 0.9 the disk's colours are O(0.1 .. 1)


def emission(obj=1, T_in=6000.0, **kw):
    return rt.DiskEmission(obj, T_in, **kw)


# ---- the header's model in numpy (float64), metric and derivatives from the CPU oracle ------------------------------------------------
def inner(g, a, b):
    return np.einsum("np,npq,nq->n", a, g, b)


def np_model(sc, em, s0, se, r_in):
    """-> dict(omega, u_emit, g, rgb, valid, ut): the model of include/rtgr.h at the pairs of states (s0, se) [n, 8]"""
    s0, se = np.asarray(s0, np.float64), np.asarray(se, np.float64)
    n = len(se)
    x, y = se[:, 1], se[:, 2]
    with np.errstate(all="ignore"):
        if em.emitter == abi.EMIT_KEPLER:
            P = np.stack([se[:, 0], x, y, np.zeros(n)], axis=1)
            g, dg, _ = ol.eval_metric(sc, P)
            D = lambda a, b: x * dg[:, a, b, 1] + y * dg[:, a, b, 2]
            gtp = -y * g[:, 0, 1] + x * g[:, 0, 2]
            gpp = y * y * g[:, 1, 1] - 2 * x * y * g[:, 1, 2] + x * x * g[:, 2, 2]
            A = D(0, 0)
            B = (-y * D(0, 1) + x * D(0, 2)) + gtp
            Cc = (y * y * D(1, 1) - 2 * x * y * D(1, 2) + x * x * D(2, 2)) + 2 * gpp
            disc = B * B - A * Cc
            valid = (disc >= 0) & (Cc != 0)
            om = (-B + em.orbit * np.sqrt(disc)) / Cc
        else:
            om, valid = np.full(n, em.orbit), np.ones(n, bool)
        ge, g0 = ol.metric_plain(sc, se[:, :4]), ol.metric_plain(sc, s0[:, :4])
        xi = np.stack([np.ones(n), -om * y, om * x, np.zeros(n)], axis=1)
        n2 = inner(ge, xi, xi)
        valid &= np.isfinite(om) & np.isfinite(n2) & (n2 < 0)
        u = xi / np.sqrt(-n2)[:, None]
        gu = np.linalg.inv(g0)
        t = gu[:, :, 0]
        t2 = inner(g0, t, t)
        tobs = -t / np.sqrt(-t2)[:, None]                      # the static observer of make_canvas, future-directed
        gr = inner(g0, s0[:, 4:], tobs) / inner(ge, se[:, 4:], u)
        valid &= (t2 < 0) & np.isfinite(gr)
        rho = np.hypot(x, y)
        T = em.T_in * (rho / r_in) ** (-em.p)
        if em.flags & abi.EMIT_INNER_EDGE:
            T = T * np.maximum(1 - np.sqrt(r_in / rho), 0.0) ** 0.25
        glow = valid & (gr > 0) & (T > 0)
        theta, weight = np.array(em.theta[:]), np.array(em.weight[:])
        rgb = em.gain * weight[None, :] / np.expm1(theta[None, :] / (gr * T)[:, None])
    rgb = np.where(glow[:, None], rgb, 0.0)
    nan = np.nan
    return dict(omega=np.where(valid, om, nan), u_emit=np.where(valid[:, None], u, nan), g=np.where(glow, gr, nan), rgb=rgb, valid=valid,
                ut=np.where(valid, u[:, 0], nan), T=T)


def kerr_omega(a, rho, sign):
    r = np.sqrt(rho * rho - a * a)
    return 1.0 / (r ** 1.5 + a) if sign > 0 else -1.0 / (r ** 1.5 - a)


def null_end_states(sc, rhos):
    """points at rho, z = +-0.05, two azimuths, each with the two null k_end = +-T + N over a fixed spatial direction"""
    pts, dirs = [], []
    for rho in rhos:
        for phi, z, d in ((0.3, 0.05, (0.2, -0.9, 0.3)), (2.1, -0.05, (-0.7, 0.1, -0.5)), (-1.2, 0.05, (0.5, 0.6, 0.4)), (2.9, -0.05, (0.1, 0.3, -0.9))):
            pts.append([1.5, rho * math.cos(phi), rho * math.sin(phi), z])
            dirs.append(d)
    pts, dirs = np.array(pts), np.array(dirs)
    g = ol.metric_plain(sc, pts)
    # k = +-T + N: T the unit normal of the slicing (g^-1 e_t, timelike everywhere outside the horizon's inside — the ergoregion
    # included, where not every spatial direction has a null vector over it), N the unit vector along d orthogonal to T
    T = np.linalg.inv(g)[:, :, 0]
    T = T / np.sqrt(-inner(g, T, T))[:, None]
    d4 = np.concatenate([np.zeros((len(dirs), 1)), dirs], axis=1)
    N = d4 + inner(g, d4, T)[:, None] * T
    N = N / np.sqrt(inner(g, N, N))[:, None]
    out = []
    for sgn in (1.0, -1.0):
        out.append(np.concatenate([pts, sgn * T + N], axis=1))
    se = np.concatenate(out)
    assert np.abs(inner(ol.metric_plain(sc, se[:, :4]), se[:, 4:], se[:, 4:])).max() < 1e-12
    return se


def hook_cases(name, dev_canvas=None):
    """per orbit sign: (scene, emission, s0, s_end, numpy model) for one metric of the pointwise tests"""
    metric = METRICS[name]()
    sc = rt.make_scene(metric, [rt.Disk(*HOOK_DISK)])
    cases = []
    for sign in (+1, -1):
        se = null_end_states(sc, RHOS[name])
        s0 = canvas_states(metric, 16, 12)[np.arange(len(se)) * 5 % 192]
        probe = np_model(sc, emission(orbit=sign, p=0.0, T_in=1.0), s0, se, HOOK_DISK[1])
        keep = ~probe["valid"] | (probe["g"] > 0)                    # of the two null roots: the one a ray traced from the camera would have
        se, s0 = se[keep], s0[keep]
        for flags in (False, True):
            em = emission(orbit=sign, p=0.75, T_in=1.0, inner_edge=flags)
            m = np_model(sc, em, s0, se, HOOK_DISK[1])
            ok = m["valid"] & np.isfinite(m["g"]) & (m["T"] > 0)
            # T_in so that theta_c / (g T_em) <= 8 at every glowing point: rgb's sensitivity to g stays below 9
            em.T_in = float(max(em.theta[:]) / (8.0 * (m["g"] * m["T"])[ok].min())) if ok.any() else 6000.0
            m = np_model(sc, em, s0, se, HOOK_DISK[1])
            cases.append((metric, sc, em, s0, se, m))
    return cases


_CANVAS = {}


def canvas_states(metric, ni, nj, dtype=np.float64, cam=None):
    """rtgr_make_canvas_* of example2's camera (or `cam`): [ni * nj, 8]; shared, never written to"""
    key = (id(metric), ni, nj, np.dtype(dtype).name, id(cam))
    if key not in _CANVAS:
        lib = abi.load()
        sc = rt.make_scene(metric, [])
        camera = cam if cam is not None else rt.make_camera(**CAM2)
        st = np.zeros((ni * nj, 8), dtype)
        fn = lib.rtgr_make_canvas_f64 if dtype == np.float64 else lib.rtgr_make_canvas_f32
        abi.check(lib, fn(None, C.byref(sc), C.byref(camera), ni, nj, 0, nj, st.ctypes.data))
        st.setflags(write=False)
        _CANVAS[key] = (st, metric, cam)          # (keeps the keyed objects alive)
    return _CANVAS[key][0]


def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(b) else 0.0


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(EMIT_EXPORTS) <= set(abi.EXPORTS)
    lib = abi.load()
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    for s in EMIT_EXPORTS:
        assert hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    for words in ("enum rtgr_emitter { RTGR_EMIT_KEPLER = 0, RTGR_EMIT_RIGID = 1 };", "#define RTGR_EMIT_INNER_EDGE 1u", "plunging gas", "limb darkening",
                  "more than one emitting disk", "Omega_+- = (-B +- sqrt(B^2 - A C)) / C", "BLACK (0, 0, 0) and g = NaN"):
        assert words in hdr, words
    assert "rtgr_emission.hpp" not in open(os.path.join(ROOT, "raytracegr.jl_amd", "build.py")).read().split("KERNEL_HEADERS =")[0]


def _c_caller(tmp_path):
    exe = str(tmp_path / "emission_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "emission_layout.c"), "-o", exe, "-ldl"])
    return exe


def test_struct_layout_in_ctypes_and_in_a_compiled_c_caller(tmp_path):
    e = abi.rtgr_disk_emission
    want = dict(object=0, emitter=4, flags=8, pad=12, orbit=16, T_in=24, p=32, gain=40, theta=48, weight=72)
    assert C.sizeof(e) == 96 and {k: getattr(e, k).offset for k in want} == want
    assert (abi.EMIT_KEPLER, abi.EMIT_RIGID, abi.EMIT_INNER_EDGE) == (0, 1, 1)
    out = subprocess.check_output([_c_caller(tmp_path)], text=True).split()
    assert dict(zip(out[0::2], map(int, out[1::2]))) == dict(want, emission=96)
    em = rt.DiskEmission(3, 6000.0)
    assert (em.object, em.emitter, em.flags, em.pad, em.orbit, em.p, em.gain) == (3, 0, 0, 0, 1.0, 0.75, 1.0)
    assert np.allclose(em.theta[:], [1.438776877e7 / v for v in (700.0, 546.1, 435.8)], rtol=1e-15)
    assert np.allclose(em.weight[:], [(546.1 / v) ** 5 for v in (700.0, 546.1, 435.8)], rtol=1e-15) and em.weight[1] == 1.0
    assert rt.DiskEmission(1, 1.0, emitter="rigid", orbit=0.1, inner_edge=True).flags == abi.EMIT_INNER_EDGE
    with pytest.raises(ValueError):
        rt.DiskEmission(1, 1.0, emitter="static")


def test_no_result_without_a_device(tmp_path):
    """Without a HIP device every new entry FAILS with RTGR_ERR_NO_DEVICE and leaves the caller's arrays alone — from a compiled C caller
    (the host-pointer trace and the hook) and through ctypes (all six)."""
    import torch
    res = subprocess.run([_c_caller(tmp_path), abi.LIB_PATH], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)       # (2: a symbol does not resolve)
    w = res.stdout.split("\n")[1].split()
    got = tuple(int(w[k]) for k in (1, 3, 5))                      # trace, eval, touched
    nd = abi.ERR_NO_DEVICE
    assert got in ((nd, nd, 0), (0, 0, 1)), got
    if torch.cuda.is_available():
        return
    assert got == (nd, nd, 0)
    lib = abi.load()
    sc, opt = rt.make_scene(rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 3.0, 6.0)]), rt.solver_defaults()
    cam, em = rt.make_camera(**CAM2), emission()
    for dtype, suf in ((np.float64, "f64"), (np.float32, "f32")):
        rgb, g = np.full((3, 4), -7.0, dtype), np.full(4, -7.0, dtype)
        rc = getattr(lib, "rtgr_trace_emission_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(cam), 2, 2, None, C.byref(em), None, rgb.ctypes.data, None,
                                                        g.ctypes.data, None, None, None)
        assert rc == nd and b"no CPU fallback" in lib.rtgr_last_error() and (rgb == -7.0).all() and (g == -7.0).all()
        rc = getattr(lib, "rtgr_trace_emission_device_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(cam), 2, 2, None, C.byref(em), None,
                                                               rgb.ctypes.data, None, g.ctypes.data, None, None, None, None)
        assert rc == nd and (rgb == -7.0).all()
        s, out = np.ones((1, 8), dtype), np.full(9, -7.0, dtype)
        rc = getattr(lib, "rtgr_eval_disk_emission_" + suf)(None, C.byref(sc), C.byref(em), s.ctypes.data, s.ctypes.data, 1, out[0:].ctypes.data,
                                                            out[1:].ctypes.data, out[5:].ctypes.data, out[6:].ctypes.data)
        assert rc == nd and (out == -7.0).all()
    with pytest.raises(abi.RtgrError):
        rt.trace_emission(rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 3.0, 6.0)], CAM2, 2, 2, em)
    with pytest.raises(abi.RtgrError):
        rt.eval_disk_emission(rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 3.0, 6.0)], em, np.ones((1, 8)), np.ones((1, 8)))


def test_julia_stub_names_the_symbols_and_the_layout():
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    assert "#   RtgrDiskEmission 96   object 0, emitter 4, flags 8, pad 12, orbit 16, T_in 24, p 32, gain 40, theta 48, weight 72" in jl
    for word in (":rtgr_trace_emission_f64", ":rtgr_trace_emission_f32", "function trace_rays_emission(", "struct RtgrDiskEmission",
                 "const RTGR_EMIT_KEPLER = UInt32(0)", "const RTGR_EMIT_RIGID = UInt32(1)", "const RTGR_EMIT_INNER_EDGE = UInt32(1)"):
        assert word in jl, word


def test_the_numpy_model_reproduces_kerr_and_finds_the_invalid_regions():
    """(CPU: the judge itself — the restated model with the oracle's metric gives Kerr's closed-form rates on the textbook metrics, and
    decides validity where the GPU tests expect it)"""
    for name, a in SPIN.items():
        sc = rt.make_scene(METRICS[name](), [rt.Disk(*HOOK_DISK)])
        for sign in (+1, -1):
            se = null_end_states(sc, RHOS[name])
            far = np.tile([0.0, 10.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0], (len(se), 1))       # (a camera where the static observer exists)
            m = np_model(sc, emission(orbit=sign), far, se, HOOK_DISK[1])
            rho = np.hypot(se[:, 1], se[:, 2])
            v = m["valid"]
            assert rel(m["omega"][v], kerr_omega(a, rho[v], sign)) < 1e-12
            if name == "ks_true08" and sign < 0:
                assert not v[np.isclose(rho, 3.0)].any() and not v[np.isclose(rho, 2.2)].any() and v[np.isclose(rho, 6.0)].all()
            if sign > 0:
                assert v.all()
    sc = rt.make_scene(METRICS["ks_true0"](), [rt.Disk(*HOOK_DISK)])
    for sign in (+1, -1):
        se = null_end_states(sc, (2.5,))
        far = np.tile([0.0, 10.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0], (len(se), 1))
        assert not np_model(sc, emission(orbit=sign), far, se, HOOK_DISK[1])["valid"].any()      # inside the photon orbit: no timelike circle


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ks_true08", "ks_true0998", "ks_true0", "ks_ref0", "ks_ref08"])
def test_hook_against_numpy(lib, name):
    seen_valid = seen_invalid = 0
    for metric, sc, em, s0, se, m in hook_cases(name):
        got = rt.eval_disk_emission(metric, [rt.Disk(*HOOK_DISK)], em, s0, se)
        v = m["valid"]
        assert np.array_equal(np.isfinite(got["omega"]), v) and np.array_equal(np.isfinite(got["u_emit"]).all(axis=1), v)
        assert np.array_equal(np.isfinite(got["g"]), np.isfinite(m["g"]))
        assert (got["rgb"][~v] == 0.0).all() and np.isnan(got["g"][~v]).all()
        glow = np.isfinite(m["g"])
        errs = (rel(got["omega"][v], m["omega"][v]), float(np.max(np.abs(got["u_emit"][v] - m["u_emit"][v]) / np.abs(m["ut"][v])[:, None], initial=0.0)),
                rel(got["g"][glow], m["g"][glow]), rel(got["rgb"][glow], m["rgb"][glow]))
        x = (np.array(em.theta[:])[None, :] / (m["g"] * m["T"])[glow][:, None]) if glow.any() else np.zeros((0, 3))
        print(f"{name} orbit {em.orbit:+.0f} flags {em.flags}: {v.sum()} valid of {len(v)}, u^t <= {np.nanmax(m['ut']) if v.any() else 0:.2f}, "
              f"theta/(g T) <= {x.max(initial=0.0):.2f}; rel err omega {errs[0]:.2e} u_emit {errs[1]:.2e} g {errs[2]:.2e} rgb {errs[3]:.2e}")
        assert x.max(initial=0.0) <= 8.0 * (1 + 1e-12)
        assert errs[0] <= 1e-10 and errs[1] <= 1e-10 and errs[2] <= 1e-10 and errs[3] <= 1e-9
        if name in SPIN:
            rho = np.hypot(se[:, 1], se[:, 2])
            assert rel(got["omega"][v], kerr_omega(SPIN[name], rho[v], em.orbit)) <= 1e-12
        seen_valid += int(v.sum())
        seen_invalid += int((~v).sum())
    assert seen_valid >= 8
    if name == "ks_true08":
        assert seen_invalid >= 4                      # rho = 3 with orbit -1 (and 2.2): no retrograde circular orbit there


@pytest.mark.gpu
def test_no_orbit_is_black_and_nan(lib):
    """Validity decided far from its boundary: Schwarzschild at rho = 2.5 (inside the photon orbit) for both signs, a = 0.8 at rho = 3 retrograde"""
    for name, rhos, signs in (("ks_true0", (2.5,), (+1, -1)), ("ks_true08", (3.0,), (-1,))):
        metric = METRICS[name]()
        sc = rt.make_scene(metric, [rt.Disk(*HOOK_DISK)])
        for sign in signs:
            se = null_end_states(sc, rhos)
            s0 = canvas_states(metric, 16, 12)[:len(se)]
            got = rt.eval_disk_emission(metric, [rt.Disk(*HOOK_DISK)], emission(orbit=sign), s0, se)
            assert np.isnan(got["omega"]).all() and np.isnan(got["u_emit"]).all() and np.isnan(got["g"]).all() and (got["rgb"] == 0.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ks_true08", "ks_true0998", "ks_true0", "ks_ref0", "ks_ref08"])
def test_the_emitter_is_a_geodesic_of_the_devices_own_metric(lib, name):
    """(P, u_emit) at z = 0 through rtgr_eval_geodesic_f64, path 1: the acceleration is -Omega^2 (x, y, 0) (u^t)^2 and u'^t = 0 — which
    pins the sign conventions without anyone having to know them"""
    metric = METRICS[name]()
    rhos = RHOS[name]
    pts = np.array([[0.7, rho * math.cos(phi), rho * math.sin(phi), 0.0] for rho in rhos for phi in (0.3, 2.1)])
    se = np.concatenate([pts, np.tile([-1.0, 0.3, 0.2, 0.1], (len(pts), 1))], axis=1)
    s0 = canvas_states(metric, 16, 12)[:len(se)]
    checked = 0
    for sign in (+1, -1):
        got = rt.eval_disk_emission(metric, [rt.Disk(*HOOK_DISK)], emission(orbit=sign), s0, se)
        v = np.isfinite(got["omega"])
        if not v.any():
            continue
        s = np.concatenate([pts[v], got["u_emit"][v]], axis=1)
        ds = rt.geodesic(s, metric, path=1).reshape(-1, 8)
        om, ut = got["omega"][v], got["u_emit"][v][:, 0]
        want = np.stack([np.zeros(len(om)), -om * om * pts[v][:, 1] * ut * ut, -om * om * pts[v][:, 2] * ut * ut, np.zeros(len(om))], axis=1)
        err = np.abs(ds[:, 4:] - want) / (ut * ut)[:, None]
        print(f"{name} orbit {sign:+d}: {v.sum()} orbits, u^t <= {ut.max():.2f}, max |du - want| / (u^t)^2 = {err.max():.2e}")
        assert same_bits(np.ascontiguousarray(ds[:, :4]), np.ascontiguousarray(got["u_emit"][v]))
        assert err.max() <= 1e-10
        assert (np.sign(om) == sign).all()
        checked += int(v.sum())
    assert checked >= len(pts)


@pytest.mark.gpu
def test_flat_space(lib):
    """Minkowski: Omega = 0 and g = 1, the colour is Planck's at T_em(rho); a rigidly rotating emitter gives special relativity's Doppler factor"""
    metric, disk = rt.minkowski, rt.Disk(0.05, 2.0, 8.0)
    s0 = canvas_states(metric, 16, 12)
    n = len(s0)
    rng = np.random.default_rng(5)
    rho, phi = rng.uniform(2.0, 8.0, n), rng.uniform(-np.pi, np.pi, n)
    se = s0.copy()                                                   # a straight ray keeps its tangent
    se[:, 0], se[:, 1], se[:, 2], se[:, 3] = -7.0, rho * np.cos(phi), rho * np.sin(phi), rng.choice([-0.05, 0.05], n)
    for flags in (False, True):
        em = emission(T_in=1.0e5, p=0.75, gain=0.7, inner_edge=flags)
        got = rt.eval_disk_emission(metric, [disk], em, s0, se)
        assert (got["omega"] == 0.0).all() and np.abs(got["g"] - 1.0).max() <= 8 * EPS
        assert (got["u_emit"] == np.array([1.0, 0.0, 0.0, 0.0])).all()
        T = em.T_in * (rho / 2.0) ** -0.75 * (np.maximum(1 - np.sqrt(2.0 / rho), 0.0) ** 0.25 if flags else 1.0)
        want = 0.7 * np.array(em.weight[:])[None, :] / np.expm1(np.array(em.theta[:])[None, :] / T[:, None])
        err = rel(got["rgb"], want)
        print(f"flat, inner edge {flags}: theta / T <= {(max(em.theta[:]) / T.min()):.2f}, rgb rel err {err / EPS:.1f} eps")
        assert (max(em.theta[:]) / T).max() <= (1.0 if not flags else np.inf)
        if not flags:
            assert err <= 64 * EPS
        else:        # (the edge factor's fourth root costs its own roundings, amplified by theta / T where T is small: judged where theta / T <= 1)
            cool = (max(em.theta[:]) / T) <= 1.0
            assert cool.sum() > n // 4 and rel(got["rgb"][cool], want[cool]) <= 64 * EPS
    # RIGID, Omega = 0.1 at rho = 3: g gamma (1 - v . n) = 1
    se[:, 1], se[:, 2] = 3.0 * np.cos(phi), 3.0 * np.sin(phi)
    got = rt.eval_disk_emission(metric, [disk], emission(emitter="rigid", orbit=0.1), s0, se)
    v = 0.1 * np.stack([-se[:, 2], se[:, 1], np.zeros(n)], axis=1)
    nhat = se[:, 5:8] / se[:, 4:5]
    gamma = 1.0 / math.sqrt(1.0 - 0.09)
    assert (got["omega"] == 0.1).all()
    prod = got["g"] * gamma * (1.0 - np.einsum("ni,ni->n", v, nhat))
    print(f"rigid rotation: max |g gamma (1 - v.n) - 1| = {np.abs(prod - 1).max():.2e}")
    assert np.abs(prod - 1.0).max() <= 1e-13
    assert np.abs(got["u_emit"][:, 0] - gamma).max() <= 4 * EPS * gamma


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
_GRID = {}


def _scene(name):
    """(metric, objs, rtgr_camera, index of the disk)"""
    _, objs, cam = rt.example2_scene()
    if name in ("a0998", "a0"):
        metric = rt.KerrSchild(1, 0.998) if name == "a0998" else rt.KerrSchild(1, 0.0)
        if name not in _GRID:
            _GRID[name] = metric
        return _GRID[name], objs[:2] + [rt.Disk(0.05, 2.0, 4.0)], rt.make_camera(**cam), 3
    if name == "grid":
        from test_grid_metric import ks_grid
        if "grid" not in _GRID:
            _GRID["grid"] = ks_grid(0.2)
        objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(-20.0), rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), 1.9), rt.Disk(0.05, 2.3, 4.0)]
        camera = rt.make_camera(pos=(0, 0, -4.5, 1.5), widthx=(0, 5.0, 0, 0), widthy=(0, 0, 0, 5.0), normal=(0, 0, 1, -0.3))
        return _GRID["grid"], objs, camera, 4
    raise KeyError(name)


_PLAIN = {}


def plain(lib, name, ni, nj, dtype=np.float64):
    """the plain frame (rtgr_trace_f64 / _f32, camera on the device) with every per-ray output: once per (scene, size, dtype), never written to"""
    key = (name, ni, nj, np.dtype(dtype).name)
    if key not in _PLAIN:
        metric, objs, cam, _ = _scene(name)
        sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
        out = dict(_outputs(n, dtype), rgb=np.zeros((3, n), dtype))
        o = abi.rtgr_ray_outputs()
        for k in OUT_KEYS:
            setattr(o, k, out[k].ctypes.data)
        ctr = abi.rtgr_counters()
        fn = lib.rtgr_trace_f64 if dtype == np.float64 else lib.rtgr_trace_f32
        abi.check(lib, fn(None, C.byref(sc), C.byref(opt), None, C.byref(cam), ni, nj, 0, nj, out["rgb"].ctypes.data, C.byref(o), C.byref(ctr)))
        out["counters"] = ctr.as_dict()
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _PLAIN[key] = out
    return _PLAIN[key]


def emitted(lib, name, ni, nj, em, binds=None, dtype=np.float64, aa=None, details=True, counters=True, want_g=True):
    """rtgr_trace_emission_f64 / _f32 (host pointers); binds: None or {object: (Texture, filter)}; aa: None or dict(k, contrast, max_batch_rays)"""
    metric, objs, cam, _ = _scene(name)
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    res = dict(rgb=np.full((3, n), -5.0, dtype))
    if want_g:
        res["g"] = np.full(n, -5.0, dtype)
    o = None
    if details:
        o = abi.rtgr_ray_outputs()
        res.update(_outputs(n, dtype))
        for k in OUT_KEYS:
            setattr(o, k, res[k].ctypes.data)
    sh = rt.make_shade(binds) if binds is not None else None
    aap = refined = stats = None
    if aa is not None:
        aap = C.byref(abi.rtgr_aa(k=aa["k"], flags=0, contrast=aa["contrast"], max_batch_rays=aa.get("max_batch_rays", 0)))
        res["refined"] = np.full(n, 9, np.uint8)
        refined, stats = res["refined"].ctypes.data, abi.rtgr_aa_stats()
    ctr = abi.rtgr_counters() if counters else None
    fn = lib.rtgr_trace_emission_f64 if dtype == np.float64 else lib.rtgr_trace_emission_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(sh) if sh is not None else None, C.byref(em), aap,
                      res["rgb"].ctypes.data, o, res["g"].ctypes.data if want_g else None, refined, C.byref(ctr) if counters else None,
                      C.byref(stats) if stats is not None else None))
    if counters:
        res["counters"] = ctr.as_dict()
    if stats is not None:
        res["stats"] = stats.as_dict()
    return res


def expected(lib, name, ni, nj, em, base, p, dtype):
    """where(hit32 == disk, hook(make_canvas states, state_end), base) -> (rgb, g, mask, hook result on the disk's pixels)"""
    metric, objs, cam, disk = _scene(name)
    mask = p["hit32"] == disk
    idx = np.flatnonzero(mask)
    s0 = canvas_states(metric, ni, nj, dtype, cam=_cam_key(name, cam))
    h = rt.eval_disk_emission(metric, objs, em, s0[idx], p["state_end"][idx], dtype=dtype)
    rgb, g = base.copy(), np.full(ni * nj, np.nan, dtype)
    rgb[:, idx] = h["rgb"].T
    g[idx] = h["g"]
    return rgb, g, mask, h


_CAMS = {}


def _cam_key(name, cam):
    return _CAMS.setdefault(name, cam)      # (one camera object per scene: canvas_states keys on it)


def check_frame(lib, name, ni, nj, em, dtype=np.float64):
    p = plain(lib, name, ni, nj, dtype)
    want_rgb, want_g, mask, h = expected(lib, name, ni, nj, em, p["rgb"], p, dtype)
    got = emitted(lib, name, ni, nj, em, dtype=dtype)
    assert same_bits(got["rgb"], want_rgb)
    assert same_bits(got["g"], want_g)
    for key in OUT_KEYS:
        assert same_bits(got[key], p[key]), key
    assert got["counters"] == p["counters"]
    assert same_bits(got["rgb"][:, ~mask], p["rgb"][:, ~mask]) and np.isnan(got["g"][~mask]).all()
    return p, got, mask, h


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_frames_bit_for_bit(lib, dtype):
    ni, nj = 48, 32
    em = emission(3, T_FRAME)
    # a = 0.998: every disk pixel has an orbit
    p, got, mask, h = check_frame(lib, "a0998", ni, nj, em, dtype)
    valid = np.isfinite(h["omega"])
    print(f"a = 0.998 {np.dtype(dtype).name}: {mask.sum()} disk pixels, {valid.sum()} valid, g in [{np.nanmin(h['g']):.3f}, {np.nanmax(h['g']):.3f}]")
    assert valid.sum() >= 50 and (h["rgb"][valid] > 0).any(axis=1).all()
    # without the detail arrays, the counters or g (the stream's scratch stands in): the same frame
    bare = emitted(lib, "a0998", ni, nj, em, dtype=dtype, details=False, counters=False, want_g=False)
    assert same_bits(bare["rgb"], got["rgb"])
    # a = 0: the disk reaches inside the photon orbit, where nothing emits
    p0, got0, mask0, h0 = check_frame(lib, "a0", ni, nj, em, dtype)
    valid0 = np.isfinite(h0["omega"])
    black = (got0["rgb"][:, mask0] == 0.0).all(axis=0)
    print(f"a = 0 {np.dtype(dtype).name}: {mask0.sum()} disk pixels, {valid0.sum()} valid, {black.sum()} black")
    assert valid0.sum() >= 50 and black.sum() >= 20 and np.array_equal(black, ~valid0 | (h0["rgb"] == 0.0).all(axis=1))
    assert np.isnan(got0["g"][mask0][~valid0]).all()
    print(f"a = 0: g of orbit +1 in [{np.nanmin(h0['g']):.3f}, {np.nanmax(h0['g']):.3f}]")
    assert (h0["g"][valid0] < 1.0).all()
    # the retrograde root at a = 0: gas that runs against the hole's frame is seen blue-shifted where +1 was red-shifted
    retro = emitted(lib, "a0", ni, nj, emission(3, T_FRAME, orbit=-1), dtype=dtype, details=False)
    both = valid0 & np.isfinite(retro["g"][mask0])
    assert both.sum() >= 50 and np.array_equal(np.isfinite(retro["g"][mask0]), valid0)
    print(f"a = 0: g of orbit -1 in [{np.nanmin(retro['g']):.3f}, {np.nanmax(retro['g']):.3f}]")
    assert (retro["g"][mask0][both] > 1.0).all()
    # the Python front end gives the same frame
    metric, objs, _, _ = _scene("a0998")
    front = rt.trace_emission(metric, objs, CAM2, ni, nj, em, dtype=dtype, details=True)
    assert same_bits(front["rgb"], got["rgb"]) and same_bits(front["g"], got["g"]) and same_bits(front["state_end"], p["state_end"])


@pytest.mark.gpu
def test_textures_on_the_sky_with_emission_on_the_disk(lib):
    from test_textures import BILINEAR, texture
    ni, nj = 48, 32
    _, tex = texture("rand32x16")
    em = emission(3, T_FRAME)
    metric, objs, cam, _ = _scene("a0998")
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(), ni * nj
    sh = rt.make_shade({1: (tex, BILINEAR)})
    textured = np.zeros((3, n))
    abi.check(lib, lib.rtgr_trace_shaded_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(sh), None, textured.ctypes.data, None, None,
                                             None, None))
    p = plain(lib, "a0998", ni, nj)
    want_rgb, want_g, mask, _ = expected(lib, "a0998", ni, nj, em, textured, p, np.float64)
    got = emitted(lib, "a0998", ni, nj, em, binds={1: (tex, BILINEAR)})
    assert same_bits(got["rgb"], want_rgb) and same_bits(got["g"], want_g)
    assert same_bits(got["rgb"][:, ~mask], textured[:, ~mask]) and (textured[:, p["hit32"] == 1] != p["rgb"][:, p["hit32"] == 1]).any()
    for key in OUT_KEYS:
        assert same_bits(got[key], p[key]), key


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3])
def test_anti_aliasing_of_an_emitted_frame(lib, k):
    """24 x 16: uniform == the box filter of the emitted (k 24) x (k 16) frame; refined == the edge rule on the EMITTED 24 x 16 frame;
    adaptive == where(refined, uniform, emitted plain); g is the pixel-centre rays'; small batches give the default's bits."""
    ni, nj, contrast, dtype = 24, 16, 0.05, np.float64
    em = emission(3, T_FRAME)
    coarse = emitted(lib, "a0998", ni, nj, em)
    fine = emitted(lib, "a0998", k * ni, k * nj, em, details=False)
    want_uniform = box(fine["rgb"], ni, nj, k)
    uniform = emitted(lib, "a0998", ni, nj, em, aa=dict(k=k, contrast=-1.0))
    assert same_bits(uniform["rgb"], want_uniform) and (uniform["refined"] == 1).all() and same_bits(uniform["g"], coarse["g"])
    assert uniform["stats"] == dict(pixels=ni * nj, refined=ni * nj, sub_rays=k * k * ni * nj, batches=1)
    p = plain(lib, "a0998", ni, nj, dtype)
    mask = edge_mask(coarse["rgb"], p["hit32"], p["status"], ni, nj, contrast)
    by_class = edge_mask(coarse["rgb"], p["hit32"], p["status"], ni, nj, math.inf)
    plain_mask = edge_mask(p["rgb"], p["hit32"], p["status"], ni, nj, contrast)
    print(f"k = {k}: {mask.sum()} refined on the emitted frame, {by_class.sum()} by class, {plain_mask.sum()} on the plain frame")
    assert by_class.sum() <= mask.sum() < ni * nj
    got = emitted(lib, "a0998", ni, nj, em, aa=dict(k=k, contrast=contrast))
    assert np.array_equal(got["refined"], mask.astype(np.uint8))
    assert same_bits(got["rgb"], np.where(mask[None, :], want_uniform, coarse["rgb"])) and same_bits(got["g"], coarse["g"])
    for key in OUT_KEYS:
        assert same_bits(got[key], p[key]), key
    assert got["stats"] == dict(pixels=ni * nj, refined=int(mask.sum()), sub_rays=k * k * int(mask.sum()), batches=1)
    small = emitted(lib, "a0998", ni, nj, em, aa=dict(k=k, contrast=contrast, max_batch_rays=7 * k * k))
    assert small["stats"]["batches"] == -(-int(mask.sum()) // 7)
    assert same_bits(small["rgb"], got["rgb"]) and np.array_equal(small["refined"], got["refined"]) and small["counters"] == got["counters"]


GRID_POINTS = [(rho, phi) for rho in (2.6, 3.0, 3.6) for phi in (0.3, 2.1, -1.2)]


@pytest.mark.gpu
def test_grid_metric(lib):
    """KerrSchild(1, 0.8) sampled at h = 0.2 (tests/test_grid_metric.py's grid): the frame rule holds bit for bit, and the orbital rate of
    the interpolant stays within 4 x the recorded distance from the analytic metric's"""
    ni, nj = 32, 24
    em = emission(4, T_FRAME)
    p, got, mask, h = check_frame(lib, "grid", ni, nj, em)
    valid = np.isfinite(h["omega"])
    print(f"grid: {mask.sum()} disk pixels, {valid.sum()} valid")
    assert valid.sum() >= 20
    grid, objs, _, _ = _scene("grid")
    pts = np.array([[0.0, rho * math.cos(phi), rho * math.sin(phi), z] for (rho, phi) in GRID_POINTS for z in (0.05, -0.05)])
    se = np.concatenate([pts, np.tile([-1.0, 0.3, 0.2, 0.1], (len(pts), 1))], axis=1)
    s0 = np.tile([0.0, 0.0, -4.5, 1.5, -1.0, 0.0, 1.0, 0.0], (len(pts), 1))
    a = rt.eval_disk_emission(grid, objs, em, s0, se)
    b = rt.eval_disk_emission(rt.KerrSchild(1, 0.8), objs, em, s0, se)
    assert np.isfinite(a["omega"]).all() and np.isfinite(b["omega"]).all()
    err = rel(a["omega"], b["omega"])
    print(f"grid h = 0.2 vs analytic: max rel err of Omega {err:.3e} (recorded {GRID_OMEGA_RECORDED})")
    assert GRID_OMEGA_RECORDED is not None, "not measured yet"
    assert err <= 4 * GRID_OMEGA_RECORDED


@pytest.mark.gpu
def test_f32_hook_against_the_f64_hook(lib):
    worst, count = 0.0, 0
    for name in RHOS:
        for metric, sc, em, s0, se, m in hook_cases(name):
            if em.flags:
                continue
            keep = np.isfinite(m["g"]) & (m["ut"] <= 4.0)
            if not keep.any():
                continue
            s0f, sef = s0[keep].astype(np.float32), se[keep].astype(np.float32)
            g64 = rt.eval_disk_emission(metric, [rt.Disk(*HOOK_DISK)], em, s0f.astype(np.float64), sef.astype(np.float64))["g"]
            g32 = rt.eval_disk_emission(metric, [rt.Disk(*HOOK_DISK)], em, s0f, sef, dtype=np.float32)["g"]
            assert g32.dtype == np.float32 and np.isfinite(g32).all() and np.isfinite(g64).all()
            worst = max(worst, rel(g32.astype(np.float64), g64))
            count += int(keep.sum())
    print(f"f32 hook vs f64 hook: {count} points with u^t <= 4, max rel err of g {worst:.3e} (recorded {F32_G_RECORDED})")
    assert count >= 24
    assert F32_G_RECORDED is not None, "not measured yet"
    assert worst <= min(8 * F32_G_RECORDED, 1e-3)


@pytest.mark.gpu
def test_device_entry_on_a_side_stream_equals_the_host_entry(lib):
    import torch
    ni, nj, dtype = 48, 32, np.float64
    em = emission(3, T_FRAME)
    host = emitted(lib, "a0998", ni, nj, em)
    metric, objs, cam, _ = _scene("a0998")
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rgb = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
        g = torch.full((n,), -5.0, dtype=torch.float64, device="cuda")
        dev = _outputs(n, dtype, device=True)
        o = abi.rtgr_ray_outputs()
        for key in OUT_KEYS:
            setattr(o, key, dev[key].data_ptr())
        ctr = abi.rtgr_counters()
        abi.check(lib, lib.rtgr_trace_emission_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, None, C.byref(em), None, rgb.data_ptr(),
                                                          C.byref(o), g.data_ptr(), None, C.byref(ctr), None, side.cuda_stream))
        # … and with nothing but the frame asked for: the stream's scratch holds what the emission kernel reads
        rgb2 = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
        abi.check(lib, lib.rtgr_trace_emission_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, None, C.byref(em), None, rgb2.data_ptr(),
                                                          None, None, None, None, None, side.cuda_stream))
    torch.cuda.synchronize()
    assert rgb.cpu().numpy().tobytes() == host["rgb"].tobytes() and rgb2.cpu().numpy().tobytes() == host["rgb"].tobytes()
    assert g.cpu().numpy().tobytes() == host["g"].tobytes()
    for key in OUT_KEYS:
        assert dev[key].cpu().numpy().tobytes() == host[key].tobytes(), key
    assert ctr.as_dict() == host["counters"]


@pytest.mark.gpu
def test_refusals(lib):
    """Every refusal of the emitted trace and of the hook: RTGR_ERR_BAD_ARG with a message, rgb untouched."""
    import torch
    from test_grid_metric import ETA
    from test_grid_metric_4d import grid4
    from test_textures import NEAREST, texture
    _, tex = texture("rand16x8")
    metric, objs, cam, _ = _scene("a0998")
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ni, nj = 8, 6
    rgb = torch.full((3, ni * nj), -5.0, dtype=torch.float64, device="cuda")
    host = np.full((3, ni * nj), -5.0)
    s = np.ones((1, 8))

    def call(scene=sc, camera=cam, emit=True, binds=None, aa=None, refined=False, stats=False, hook=True, **over):
        em = emission(3, T_FRAME)
        for key, val in over.items():
            if key in ("theta", "weight"):
                setattr(em, key, (C.c_double * 3)(*val))
            else:
                setattr(em, key, val)
        emp = C.byref(em) if emit else None
        sh = rt.make_shade(binds) if binds is not None else None
        shp = C.byref(sh) if sh is not None else None
        campt = C.byref(camera) if camera is not None else None
        aap = C.byref(abi.rtgr_aa(**aa)) if aa else None
        flags = np.zeros(ni * nj, np.uint8)
        dflags = torch.zeros(ni * nj, dtype=torch.uint8, device="cuda")
        st = abi.rtgr_aa_stats()
        rcs = [lib.rtgr_trace_emission_device_f64(None, C.byref(scene), C.byref(opt), campt, ni, nj, shp, emp, aap, rgb.data_ptr(), None, None,
                                                  dflags.data_ptr() if refined else None, None, C.byref(st) if stats else None, None)]
        msgs = [lib.rtgr_last_error()]
        rcs.append(lib.rtgr_trace_emission_f64(None, C.byref(scene), C.byref(opt), campt, ni, nj, shp, emp, aap, host.ctypes.data, None, None,
                                               flags.ctypes.data if refined else None, None, C.byref(st) if stats else None))
        msgs.append(lib.rtgr_last_error())
        if hook:        # the hook shares every check of the parameters and the scene
            out = np.full(3, -3.0)
            rcs.append(lib.rtgr_eval_disk_emission_f64(None, C.byref(scene), emp, s.ctypes.data, s.ctypes.data, 1, None, None, None, out.ctypes.data))
            msgs.append(lib.rtgr_last_error())
            assert rcs[-1] == 0 or (out == -3.0).all()                 # (a refused call leaves the caller's array alone)
        return rcs, msgs

    user = rt.make_scene(metric, objs)
    user.metric = abi.USER
    nan, inf = math.nan, math.inf
    cases = [(dict(emit=False), b"rtgr_disk_emission is NULL"), (dict(camera=None, hook=False), b"camera"),
             (dict(object=0), b"object = 0"), (dict(object=4), b"object = 4"), (dict(object=1), b"Sphere"), (dict(object=2), b"Plane"),
             (dict(binds={3: (tex, NEAREST)}, hook=False), b"one or the other"),
             (dict(emitter=2), b"unknown emitter"), (dict(flags=2), b"flags"), (dict(flags=3), b"flags"), (dict(pad=1), b"pad"),
             (dict(orbit=0.5), b"+1"), (dict(orbit=0.0), b"+1"), (dict(orbit=nan), b"orbit"), (dict(orbit=inf, emitter=1), b"orbit"),
             (dict(T_in=0.0), b"T_in"), (dict(T_in=-1.0), b"T_in"), (dict(T_in=nan), b"T_in"), (dict(gain=0.0), b"gain"), (dict(gain=nan), b"gain"),
             (dict(theta=(1.0, 0.0, 1.0)), b"theta[1]"), (dict(theta=(1.0, 1.0, nan)), b"theta[2]"), (dict(weight=(-1.0, 1.0, 1.0)), b"weight[0]"),
             (dict(weight=(1.0, nan, 1.0)), b"weight[1]"), (dict(p=inf), b"p must be finite"), (dict(p=nan), b"p must be finite"),
             (dict(scene=user), b"RTGR_USER"),
             (dict(refined=True, hook=False), b"must be NULL"), (dict(stats=True, hook=False), b"must be NULL"),
             (dict(aa=dict(k=1, flags=0, contrast=0.1, max_batch_rays=0), hook=False), b"2..8"),
             (dict(aa=dict(k=2, flags=0, contrast=nan, max_batch_rays=0), hook=False), b"NaN")]
    for kw, word in cases:
        rcs, msgs = call(**kw)
        assert rcs == [abi.ERR_BAD_ARG] * len(rcs) and all(word in m for m in msgs), (kw, rcs, msgs)
    # a time-dependent grid is not stationary
    flat4 = grid4(np.broadcast_to(ETA, (6, 6, 6, 10)).copy(), 4, -1.0, 1.0, (-3.0,) * 3, 1.0, name="flat4")
    g4 = rt.make_scene(flat4, [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(-20.0), rt.Disk(0.05, 2.0, 4.0)])
    rcs, msgs = call(scene=g4)
    assert rcs == [abi.ERR_BAD_ARG] * 3 and all(b"4-D" in m for m in msgs), (rcs, msgs)
    torch.cuda.synchronize()
    assert bool((rgb == -5.0).all()) and (host == -5.0).all()
    rcs, _ = call(hook=False)
    torch.cuda.synchronize()
    assert rcs == [0, 0] and rgb.cpu().numpy().tobytes() == host.tobytes() and not (host == -5.0).any()
    # a rigid emitter takes any finite rate, zero included
    assert call(emitter=1, orbit=0.0)[0] == [0, 0, 0]


@pytest.mark.gpu
def test_capture_replay_and_trim(lib):
    """aa == NULL and ctr == NULL: the call is captured once workspace and scratch exist, replays the eager frame, refuses to grow its
    scratch (or to deliver counters) during capture; a scratch that grew afterwards is retired, not freed, so the graph still replays;
    rtgr_trim releases what was retired"""
    import torch
    metric, objs, cam, _ = _scene("a0998")
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    em = emission(3, T_FRAME)
    ni, nj = 24, 16
    n = ni * nj
    side = torch.cuda.Stream()
    hip = _hip_runtime()

    def call(out, g, width=ni, ctr=None):
        return lib.rtgr_trace_emission_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), width, nj, None, C.byref(em), None, out.data_ptr(), None,
                                                  g.data_ptr(), None, C.byref(ctr) if ctr is not None else None, None, side.cuda_stream)

    with torch.cuda.stream(side):
        eager, out = (torch.zeros((3, n), dtype=torch.float64, device="cuda") for _ in range(2))
        g_eager, g_out = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
        wide, g_wide = torch.zeros((3, 2 * n), dtype=torch.float64, device="cuda"), torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    abi.check(lib, call(eager, g_eager))                       # the warm-up: workspace and scratch of this size exist afterwards
    torch.cuda.synchronize()
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc_big = call(wide, g_wide, width=2 * ni)                  # a larger frame: the scratch would have to grow
    msg_big = lib.rtgr_last_error()
    rc_ctr = call(out, g_out, ctr=abi.rtgr_counters())         # counters need a synchronisation
    msg_ctr = lib.rtgr_last_error()
    rc = call(out, g_out)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert rc == 0 and rc_big == abi.ERR_BAD_ARG and b"captured" in msg_big and rc_ctr == abi.ERR_BAD_ARG and b"ctr" in msg_ctr
    assert graph.value and hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and bool((eager != 0).any())
    assert g_out.cpu().numpy().tobytes() == g_eager.cpu().numpy().tobytes() and bool(torch.isfinite(g_eager).any())
    out.zero_()
    torch.cuda.synchronize()
    abi.check(lib, call(wide, g_wide, width=2 * ni))           # the scratch grows: the old one is retired, the graph still replays
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    abi.check(lib, lib.rtgr_trim(None))
    fresh, g_fresh = torch.zeros((3, n), dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    abi.check(lib, call(fresh, g_fresh))
    torch.cuda.synchronize()
    assert torch.equal(fresh, eager)
