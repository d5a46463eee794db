"""The observer camera (rtgr_trace_observer_*, rtgr_make_observer_canvas_*, rtgr_eval_observer_*; include/rtgr.h "observer camera").

The reference has no such camera, so the judges are (1) numpy, for the frame and the pixel rule as the header states them — np_frame /
np_rays below, with the metric from the CPU oracle (a grid: from the device's own rtgr_eval_metric) — and (2) the library's own plain
trace, for everything an observer trace does around them:
    rtgr_trace_observer(obs)  ==  rtgr_trace(state0 = rtgr_make_observer_canvas(obs))                                  bit for bit,
textures and emission laid over it exactly as rtgr_trace_shaded / rtgr_trace_emission lay them over a camera frame, the emission's
frequency ratio taken against the observer's own e_0.
CPU part: symbols, the struct layout (ctypes and a compiled C caller), no result without a device, the numpy model itself.

Recorded on an MI355X (profiles/observer/README.md): see F32_FRAME_RECORDED / F32_STATE_RECORDED below."""
import ctypes as C
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
from conftest import ROOT
from scenes import rt
from test_textures import OUT_KEYS, _hip_runtime, _outputs, same_bits

abi = rt._abi
OBS_EXPORTS = ("rtgr_trace_observer_device_f64", "rtgr_trace_observer_device_f32", "rtgr_trace_observer_f64", "rtgr_trace_observer_f32",
               "rtgr_make_observer_canvas_device_f64", "rtgr_make_observer_canvas_device_f32", "rtgr_make_observer_canvas_f64",
               "rtgr_make_observer_canvas_f32", "rtgr_eval_observer_f64", "rtgr_eval_observer_f32", "rtgr_eval_disk_emission_observer_f64",
               "rtgr_eval_disk_emission_observer_f32")
SIZES = ((48, 32), (37, 19))
# max |frame32 - frame64| / max |frame64| and the same of the canvas states over the observers of the hook test, as measured on an MI355X
# (profiles/observer/README.md).  The test asserts 8 x these: other positions round differently.
F32_FRAME_RECORDED = 4.750e-7
F32_STATE_RECORDED = 2.342e-7
T_FRAME = 30000.0


def observer(kind="static", projection="perspective", pos=(0.5, 5.2, 3.0, 0.0), look=(0.0, -1.0, 0.2, 0.1), up=(0.0, 0.1, 0.0, 1.0), fov=(1.0, 0.7),
             vel=(1.0, 0.1, 0.3, -0.2), orbit=+1, max_batch_rays=0):
    if projection == "equirect" and fov == (1.0, 0.7):
        fov = (2 * math.pi, math.pi)
    return rt.Observer(pos, look, up, fov[0], fov[1], kind=kind, vel=vel if kind == "velocity" else None, orbit=orbit, projection=projection,
                       max_batch_rays=max_batch_rays)


# ---- the header's frame and pixel rule in numpy (float64) ----------------------------------------------------------------------------
def levi_civita():
    eps = np.zeros((4, 4, 4, 4))
    for p in itertools.permutations(range(4)):
        sign = 1.0
        for a in range(4):
            for b in range(a + 1, 4):
                if p[a] > p[b]:
                    sign = -sign
        eps[p] = sign
    return eps


EPS4 = levi_civita()


def np_frame(g, dg, ob):
    """-> dict(frame [4, 4] rows e_0, e_right, e_up, e_look; omega; valid) from g [4, 4] at pos and dg [4, 4, 4] (dg[a, b, c] = d_c g_ab)
    at pos (read by a circular observer only)"""
    pos, look, up = np.array(ob.pos[:]), np.array(ob.look[:]), np.array(ob.up[:])
    ip = lambda a, b: float(a @ g @ b)
    omega, valid = math.nan, True
    with np.errstate(all="ignore"):
        if ob.kind == abi.OBS_STATIC:
            u = -np.linalg.inv(g)[:, 0]
        elif ob.kind == abi.OBS_VELOCITY:
            u = np.array(ob.vel[:])
        else:
            x, y = pos[1], pos[2]
            D = lambda a, b: x * dg[a, b, 1] + y * dg[a, b, 2]
            gtp = -y * g[0, 1] + x * g[0, 2]
            gpp = y * y * g[1, 1] - 2 * x * y * g[1, 2] + x * x * g[2, 2]
            A, B = D(0, 0), (-y * D(0, 1) + x * D(0, 2)) + gtp
            Cc = (y * y * D(1, 1) - 2 * x * y * D(1, 2) + x * x * D(2, 2)) + 2 * gpp
            disc = B * B - A * Cc
            valid = bool(disc >= 0 and Cc != 0)
            omega = (-B + ob.orbit * math.sqrt(disc)) / Cc if valid else math.nan
            u = np.array([1.0, -omega * y, omega * x, 0.0])
        n2 = ip(u, u)
        valid = valid and bool(n2 < 0) and bool(u[0] > 0)
        e0 = u / np.sqrt(-n2)
        l = look + ip(look, e0) * e0
        valid = valid and ip(l, l) > 1e-12 * np.abs(look[:, None] * g * look[None, :]).sum()
        el = l / np.sqrt(ip(l, l))
        w = up + ip(up, e0) * e0 - ip(up, el) * el
        valid = valid and ip(w, w) > 1e-12 * np.abs(up[:, None] * g * up[None, :]).sum()
        eu = w / np.sqrt(ip(w, w))
        lowered = -np.sqrt(-np.linalg.det(g)) * np.einsum("abcd,b,c,d->a", EPS4, e0, el, eu)
        er = np.linalg.inv(g) @ lowered
        frame = np.stack([e0, er, eu, el])
    valid = valid and bool(np.isfinite(frame).all())
    return dict(frame=frame, omega=omega, valid=valid)


def pixel_ab(ni, nj):
    idx = np.arange(ni * nj)
    return 2 * (idx % ni + 0.5) / ni - 1, 2 * (idx // ni + 0.5) / nj - 1


def np_rays(g, frame, ob, ni, nj):
    """the states [ni * nj, 8] of the header's pixel rule"""
    e0, er, eu, el = frame
    a, b = pixel_ab(ni, nj)
    if ob.projection == abi.PROJ_PERSPECTIVE:
        v = el[None, :] + (a * math.tan(ob.fov_x / 2))[:, None] * er[None, :] + (b * math.tan(ob.fov_y / 2))[:, None] * eu[None, :]
        n = v / np.sqrt(np.einsum("np,pq,nq->n", v, g, v))[:, None]
    else:
        al, be = a * ob.fov_x / 2, b * ob.fov_y / 2
        n = np.cos(be)[:, None] * (np.cos(al)[:, None] * el[None, :] + np.sin(al)[:, None] * er[None, :]) + np.sin(be)[:, None] * eu[None, :]
    k = (-e0[None, :] + n) / math.sqrt(2.0)
    return np.concatenate([np.tile(np.array(ob.pos[:]), (ni * nj, 1)), k], axis=1)


ETA4 = np.diag([-1.0, 1.0, 1.0, 1.0])


def rel_max(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - b)) / np.max(np.abs(b)))


def oracle_metric(metric, pos):
    sc = rt.make_scene(metric, [])
    P = np.array([pos])
    g, dg, _ = ol.eval_metric(sc, P)
    return ol.metric_plain(sc, P)[0], dg[0]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(OBS_EXPORTS) <= set(abi.EXPORTS)
    lib = abi.load()
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    for s in OBS_EXPORTS:
        assert hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    for words in ("enum rtgr_observer_kind { RTGR_OBS_STATIC = 0, RTGR_OBS_VELOCITY = 1, RTGR_OBS_CIRCULAR = 2 };",
                  "enum rtgr_projection { RTGR_PROJ_PERSPECTIVE = 0, RTGR_PROJ_EQUIRECT = 1 };", "anti-aliasing with this camera",
                  "a camera path over time", "lenses other than the two projections", "eps_0123 = +1"):
        assert words in hdr, words


def _c_caller(tmp_path):
    exe = str(tmp_path / "observer_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "observer_layout.c"), "-o", exe, "-ldl"])
    return exe


def test_struct_layout_in_ctypes_and_in_a_compiled_c_caller(tmp_path):
    o = abi.rtgr_observer
    want = dict(pos=0, vel=32, look=64, up=96, fov_x=128, fov_y=136, orbit=144, kind=152, projection=156, flags=160, pad=164, max_batch_rays=168)
    assert C.sizeof(o) == 176 and {k: getattr(o, k).offset for k in want} == want
    assert (abi.OBS_STATIC, abi.OBS_VELOCITY, abi.OBS_CIRCULAR, abi.PROJ_PERSPECTIVE, abi.PROJ_EQUIRECT) == (0, 1, 2, 0, 1)
    exe = _c_caller(tmp_path)
    out = subprocess.check_output([exe], text=True).split()
    assert dict(zip(out[0::2], map(int, out[1::2]))) == dict(want, observer=176)
    assert subprocess.run([exe, abi.LIB_PATH]).returncode == 0                     # (2: a symbol does not resolve)
    ob = rt.Observer((0, 1, 2, 0), (0, 1, 0, 0), (0, 0, 0, 1), 1.0, kind="circular", orbit=-1, max_batch_rays=200)
    assert (ob.kind, ob.projection, ob.flags, ob.pad, ob.orbit, ob.fov_x, ob.fov_y, ob.max_batch_rays) == (2, 0, 0, 0, -1.0, 1.0, 1.0, 200)
    assert rt.Observer((0, 1, 2, 0), (0, 1, 0, 0), (0, 0, 0, 1), 2.0, projection="equirect").fov_y == 1.0
    for bad in (dict(kind="orbit"), dict(projection="fisheye"), dict(kind="velocity")):
        with pytest.raises(ValueError):
            rt.Observer((0, 1, 2, 0), (0, 1, 0, 0), (0, 0, 0, 1), 1.0, **bad)


def test_no_result_without_a_device():
    """Without a HIP device every new compute entry FAILS with RTGR_ERR_NO_DEVICE and leaves the caller's arrays alone."""
    import torch
    if torch.cuda.is_available():
        return
    lib, nd = abi.load(), abi.ERR_NO_DEVICE
    sc, opt = rt.make_scene(rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 3.0, 6.0)]), rt.solver_defaults()
    ob, em = observer(), rt.DiskEmission(1, 6000.0)
    for dtype, suf in ((np.float64, "f64"), (np.float32, "f32")):
        rgb, g, st = np.full((3, 4), -7.0, dtype), np.full(4, -7.0, dtype), np.full((4, 8), -7.0, dtype)
        rc = getattr(lib, "rtgr_trace_observer_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(ob), 2, 2, None, C.byref(em), rgb.ctypes.data, None,
                                                        g.ctypes.data, None)
        assert rc == nd and b"no CPU fallback" in lib.rtgr_last_error() and (rgb == -7.0).all() and (g == -7.0).all()
        rc = getattr(lib, "rtgr_trace_observer_device_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(ob), 2, 2, None, None, rgb.ctypes.data, None,
                                                               None, None, None)
        assert rc == nd and (rgb == -7.0).all()
        assert getattr(lib, "rtgr_make_observer_canvas_" + suf)(None, C.byref(sc), C.byref(ob), 2, 2, 0, 2, st.ctypes.data) == nd
        assert getattr(lib, "rtgr_make_observer_canvas_device_" + suf)(None, C.byref(sc), C.byref(ob), 2, 2, 0, 2, st.ctypes.data, None) == nd
        fr, valid = np.full(17, -7.0, dtype), C.c_int(-7)
        assert getattr(lib, "rtgr_eval_observer_" + suf)(None, C.byref(sc), C.byref(ob), fr.ctypes.data, fr[16:].ctypes.data, C.byref(valid)) == nd
        s, out = np.ones((1, 8), dtype), np.full(9, -7.0, dtype)
        rc = getattr(lib, "rtgr_eval_disk_emission_observer_" + suf)(None, C.byref(sc), C.byref(em), C.byref(ob), s.ctypes.data, s.ctypes.data, 1,
                                                                     out[0:].ctypes.data, out[1:].ctypes.data, out[5:].ctypes.data, out[6:].ctypes.data)
        assert rc == nd and (st == -7.0).all() and (fr == -7.0).all() and valid.value == -7 and (out == -7.0).all()
    for call in (lambda: rt.trace_observer(rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 3.0, 6.0)], ob, 2, 2),
                 lambda: rt.make_observer_canvas(rt.KerrSchild(1, 0.5), [], ob, 2, 2), lambda: rt.eval_observer(rt.KerrSchild(1, 0.5), [], ob)):
        with pytest.raises(abi.RtgrError):
            call()


def test_the_numpy_model_is_oriented_orthonormal_and_finds_keplers_rate():
    """(CPU: the judge itself)"""
    # flat space at rest: right = look x up
    ob = observer(pos=(0, 0, -2, 0), look=(0, 0, 1, 0), up=(0, 0, 0, 1))
    m = np_frame(ETA4, None, ob)
    assert m["valid"] and np.abs(m["frame"] - np.array([[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 1, 0]])).max() <= 1e-15
    # KerrSchild(1, 0.8) at rho = 6: an orthonormal frame for every kind, null rays for both projections, Kerr's rate
    metric, pos = rt.KerrSchild(1, 0.8), (0.0, 6.0, 0.0, 0.0)
    g, dg = oracle_metric(metric, pos)
    worst = 0.0
    for kind in ("static", "velocity", "circular"):
        for proj in ("perspective", "equirect"):
            ob = observer(kind, proj, pos=pos)
            m = np_frame(g, dg, ob)
            assert m["valid"]
            worst = max(worst, np.abs(m["frame"] @ g @ m["frame"].T - ETA4).max())
            s = np_rays(g, m["frame"], ob, 37, 19)
            k = s[:, 4:]
            worst = max(worst, np.abs(np.einsum("np,pq,nq->n", k, g, k)).max(), np.abs(k @ g @ m["frame"][0] - 1 / math.sqrt(2)).max())
            assert (k[:, 0] < 0).all()                                 # past-directed
    print(f"numpy model at KerrSchild(1, 0.8), rho = 6: max |g(e_a, e_b) - eta_ab|, |g(k, k)|, |g(k, e_0) - 1/sqrt 2| = {worst:.2e}")
    assert worst <= 1e-14
    om = np_frame(g, dg, observer("circular", pos=pos))["omega"]
    r = math.sqrt(36.0 - 0.64)
    assert abs(om - 1.0 / (r ** 1.5 + 0.8)) <= 1e-14 and abs(om - 0.065357) < 1e-6
    assert abs(np_frame(g, dg, observer("circular", pos=pos, orbit=-1))["omega"] + 1.0 / (r ** 1.5 - 0.8)) <= 1e-14
    # … and it decides validity where the GPU tests expect it
    assert not np_frame(g, dg, observer("velocity", pos=pos, vel=(0, 1, 0, 0)))["valid"]
    assert not np_frame(g, dg, observer(pos=pos, look=(0, 1, 0, 0), up=(0, 2, 0, 0)))["valid"]
    g0, dg0 = oracle_metric(rt.KerrSchild(1, 0.0), (0.0, 2.5, 0.0, 0.0))
    assert not np_frame(g0, dg0, observer("circular", pos=(0.0, 2.5, 0.0, 0.0)))["valid"]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


METRIC_NAMES = ("mink", "ks_ref0", "ks_ref08", "ks_true08", "ks_true08_generic", "grid")
_METRICS = {}


def metric_of(name):
    """(metric, whether it is sampled on a grid); one object per name (the grid: tests/test_emission.py's KerrSchild(1, 0.8) at h = 0.2)"""
    if name not in _METRICS:
        if name == "grid":
            from test_emission import _scene as em_scene
            _METRICS[name] = (em_scene("grid")[0], True)
        else:
            _METRICS[name] = ({"mink": lambda: rt.minkowski, "ks_ref0": lambda: rt.kerr_schild, "ks_ref08": lambda: rt.KerrSchild(1, 0.8, textbook=False),
                               "ks_true08": lambda: rt.KerrSchild(1, 0.8), "ks_true08_generic": lambda: rt.KerrSchild(1, 0.8, generic=True)}[name](), False)
    return _METRICS[name]


def metrics():
    return {name: metric_of(name) for name in METRIC_NAMES}


def hook_observers():
    for kind in ("static", "velocity", "circular"):
        for proj in ("perspective", "equirect"):
            yield observer(kind, proj)
    yield observer("static", pos=(0.5, 4.0, -3.0, 2.0))
    yield observer("velocity", "equirect", pos=(0.5, 4.0, -3.0, 2.0), fov=(3.0, 1.5))
    yield observer("circular", orbit=-1)


def canvas(lib, metric, ob, ni, nj, dtype=np.float64, objs=()):
    sc = rt.make_scene(metric, list(objs))
    st = np.full((ni * nj, 8), -5.0, dtype)
    fn = lib.rtgr_make_observer_canvas_f64 if dtype == np.float64 else lib.rtgr_make_observer_canvas_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(ob), ni, nj, 0, nj, st.ctypes.data))
    return st


@pytest.mark.gpu
def test_hook_against_the_numpy_model(lib):
    """frame, omega and the canvas states for every built-in metric kind and a grid, the three observer kinds, both projections"""
    worst = dict(frame=0.0, omega=0.0, states=0.0, null=0.0)
    for name, (metric, sampled) in metrics().items():
        for ob in hook_observers():
            pos = tuple(ob.pos[:])
            if sampled:                                                  # the interpolant's own g and dg: the device's
                g, dg = rt.dmetric(metric, list(pos))
                g, dg = np.asarray(g).reshape(4, 4), np.asarray(dg).reshape(4, 4, 4)
            else:
                g, dg = oracle_metric(metric, pos)
            m = np_frame(g, dg, ob)
            got = rt.eval_observer(metric, [], ob)
            assert m["valid"] and got["valid"], (name, ob.kind)
            worst["frame"] = max(worst["frame"], rel_max(got["frame"], m["frame"]))
            if ob.kind == abi.OBS_CIRCULAR:
                worst["omega"] = max(worst["omega"], abs(got["omega"] / m["omega"] - 1) if m["omega"] else abs(got["omega"]))
            else:
                assert math.isnan(got["omega"])
            ni, nj = SIZES[1]
            st = canvas(lib, metric, ob, ni, nj)
            worst["states"] = max(worst["states"], rel_max(st, np_rays(g, m["frame"], ob, ni, nj)))
            gd = np.asarray(rt.dmetric(metric, list(pos))[0]).reshape(4, 4)          # the device's own metric at pos
            k = st[:, 4:]
            worst["null"] = max(worst["null"], np.abs(np.einsum("np,pq,nq->n", k, gd, k)).max(), np.abs(k @ gd @ got["frame"][0] - 1 / math.sqrt(2)).max())
            assert (st[:, :4] == np.array(pos)).all()
            # rows [j0, j1) are the rows of the whole canvas
            part = np.zeros((ni * 3, 8))
            sc = rt.make_scene(metric, [])
            abi.check(lib, lib.rtgr_make_observer_canvas_f64(None, C.byref(sc), C.byref(ob), ni, nj, 5, 8, part.ctypes.data))
            assert same_bits(part, st[5 * ni:8 * ni])
    print("hook vs numpy, max relative: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) <= 1e-10


@pytest.mark.gpu
def test_f32_hook_against_the_f64_hook(lib):
    wf = ws = 0.0
    for name, (metric, _) in metrics().items():
        for ob in hook_observers():
            a, b = rt.eval_observer(metric, [], ob), rt.eval_observer(metric, [], ob, dtype=np.float32)
            assert a["valid"] and b["valid"] and b["frame"].dtype == np.float32
            wf = max(wf, rel_max(b["frame"], a["frame"]))
            ni, nj = SIZES[1]
            ws = max(ws, rel_max(canvas(lib, metric, ob, ni, nj, np.float32), canvas(lib, metric, ob, ni, nj)))
    print(f"f32 hook vs f64 hook: max relative difference of the frame {wf:.3e} (recorded {F32_FRAME_RECORDED}), of the states {ws:.3e} "
          f"(recorded {F32_STATE_RECORDED})")
    assert wf <= 8 * F32_FRAME_RECORDED and ws <= 8 * F32_STATE_RECORDED


def trace_observer(lib, metric, objs, ob, ni, nj, dtype=np.float64, emit=None, binds=None, want_g=None, details=True, counters=True, opt=None):
    """rtgr_trace_observer_f64 / _f32 (host pointers), raw: -> (rc, dict)"""
    sc, opt, n = rt.make_scene(metric, objs), opt or rt.solver_defaults(dtype), ni * nj
    res = dict(rgb=np.full((3, n), -5.0, dtype))
    want_g = emit is not None if want_g is None else want_g
    if want_g:
        res["g"] = np.full(n, -5.0, dtype)
    o = None
    if details:
        o = abi.rtgr_ray_outputs()
        res.update(_outputs(n, dtype))
        for k in OUT_KEYS:
            setattr(o, k, res[k].ctypes.data)
    sh = rt.make_shade(binds) if binds is not None else None
    ctr = abi.rtgr_counters() if counters else None
    fn = lib.rtgr_trace_observer_f64 if dtype == np.float64 else lib.rtgr_trace_observer_f32
    rc = fn(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, C.byref(sh) if sh is not None else None, C.byref(emit) if emit is not None else None,
            res["rgb"].ctypes.data, o, res["g"].ctypes.data if want_g else None, C.byref(ctr) if counters else None)
    if counters:
        res["counters"] = ctr.as_dict()
    return rc, res


def trace_states(lib, metric, objs, st, ni, nj, dtype=np.float64):
    """rtgr_trace_f64 / _f32 fed caller-supplied states, every per-ray output"""
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    out = dict(_outputs(n, dtype), rgb=np.zeros((3, n), dtype))
    o = abi.rtgr_ray_outputs()
    for k in OUT_KEYS:
        setattr(o, k, out[k].ctypes.data)
    ctr = abi.rtgr_counters()
    fn = lib.rtgr_trace_f64 if dtype == np.float64 else lib.rtgr_trace_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(opt), st.ctypes.data, None, ni, nj, 0, nj, out["rgb"].ctypes.data, C.byref(o), C.byref(ctr)))
    out["counters"] = ctr.as_dict()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ni,nj", SIZES)
def test_flat_space_pinhole_geometry(lib, ni, nj):
    """Minkowski, example1's objects seen from (0, 0, -2, 0): the sphere of radius 1/2 fills the cone of half angle asin(1/4).

    The solver's event search looks at interp_points points per step (the reference's ContinuousCallback), and the default, 10, is too
    coarse for THIS check: in flat space a step is several units long, and a ray 7.4e-4 rad inside the silhouette is inside the sphere
    for a chord of 0.076 only.  With the default 20 of the 368 pixels inside the cone at 48 x 32 (8 of 221 at 37 x 19; measured on an
    MI355X), all within 2.9e-3 rad of its edge, pass through the sphere between two samples and end on the sky; the CPU oracle, fed the
    numpy model's states, loses 28 (22) the same way.  That is the trace's resolution, not the camera's geometry, which is what is
    under test — so the solver of this test is given the resolution the check needs, from geometry alone: a ray at angle `ang` has
    the impact parameter 2 sin(ang) and the chord 2 sqrt(1/4 - 4 sin²(ang)); its tangent has the spatial length 1 / sqrt(2) per unit
    lambda, so it is inside for sqrt(2) x chord of lambda; no step is longer than lambda1 - lambda0, and the samples of a step are
    (lambda1 - lambda0) / (interp_points - 1) apart at most.  interp_points is the smallest number that puts a sample inside the
    shortest chord of the canvas (about 940 here).  The expectation is the issue's, for every pixel."""
    _, objs, _ = rt.example1_scene()
    fx = math.radians(60.0)
    fy = 2 * math.atan(math.tan(fx / 2) * nj / ni)
    ob = rt.Observer((0, 0, -2, 0), (0, 0, 1, 0), (0, 0, 0, 1), fx, fy)
    a, b = pixel_ab(ni, nj)
    ang = np.arctan(np.hypot(a * math.tan(fx / 2), b * math.tan(fy / 2)))
    margin = np.abs(ang - math.asin(0.25)).min()
    inside = ang < math.asin(0.25)
    opt = rt.solver_defaults()
    chord = 2.0 * np.sqrt(0.25 - 4.0 * np.sin(ang[inside]) ** 2).min()
    opt.interp_points = int(math.ceil((opt.lambda1 - opt.lambda0) / (math.sqrt(2.0) * chord))) + 2
    rc, got = trace_observer(lib, rt.minkowski, objs, ob, ni, nj, opt=opt)
    assert rc == 0
    bad = np.flatnonzero((got["hit32"] == 3) != inside)
    print(f"{ni} x {nj}: {inside.sum()} sphere pixels, the nearest pixel {margin:.2e} rad from the silhouette, shortest chord {chord:.4f}, "
          f"interp_points {opt.interp_points}; {len(bad)} pixels disagree")
    assert margin > 1e-6                                                   # none is left out
    assert (got["status"] == abi.RAY_EVENT).all() and got["counters"]["not_finished"] == 0
    assert inside.sum() > 100
    assert ((got["hit32"] == 3) == inside).all()
    # … and the finer sampling hides no error of the geometry: with the DEFAULT solver a coarse event search can only lose crossings, so
    # every pixel that disagrees lies inside the cone.  (How far from the edge they reach — 2.9e-3 rad measured — follows from the step
    # sizes the controller happened to take; it is printed, not asserted: a bound on it would come from the code under test.)
    rc, coarse = trace_observer(lib, rt.minkowski, objs, ob, ni, nj)
    lost = np.flatnonzero((coarse["hit32"] == 3) != inside)
    print(f"{ni} x {nj}, default solver: {len(lost)} pixels disagree, up to {np.abs(ang[lost] - math.asin(0.25)).max(initial=0.0):.2e} rad from the "
          f"silhouette, {int(inside[lost].sum())} of them inside the cone")
    assert rc == 0 and inside[lost].all() and not (coarse["hit32"][~inside] == 3).any()


@pytest.mark.gpu
def test_aberration(lib):
    """Minkowski, an observer moving along +y at beta = 0.6 and looking along its motion: a ray at theta' from e_look has the coordinate
    direction at theta with cos theta = (cos theta' - beta) / (1 - beta cos theta')"""
    beta = 0.6
    for ni, nj in SIZES:
        ob = rt.Observer((0, 0, -2, 0), (0, 0, 1, 0), (0, 0, 0, 1), 1.4, 1.0, kind="velocity", vel=(1, 0, beta, 0))
        st = canvas(lib, rt.minkowski, ob, ni, nj)
        a, b = pixel_ab(ni, nj)
        cp = 1.0 / np.sqrt(1.0 + (a * math.tan(0.7)) ** 2 + (b * math.tan(0.5)) ** 2)
        got = st[:, 6] / np.abs(st[:, 4])
        err = np.abs(got - (cp - beta) / (1 - beta * cp)).max()
        print(f"aberration {ni} x {nj}: max |cos theta - formula| = {err:.2e}")
        assert err <= 1e-12
        assert np.abs(np.linalg.norm(st[:, 5:8], axis=1) / np.abs(st[:, 4]) - 1).max() <= 1e-12
    assert abs((math.cos(0.7) - beta) / (1 - beta * math.cos(0.7)) - 0.30465) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mink", "ks_ref0", "ks_ref08", "ks_true08", "ks_true08_generic"])
def test_the_orbiting_observer_is_a_geodesic(lib, name):
    """(pos, e_0) of a circular observer through rtgr_eval_geodesic_f64: the acceleration is -Omega^2 (x, y, 0) (u^t)^2; and Omega is the
    emitter's at the same point, to the bit"""
    metric = metric_of(name)[0]
    disk = [rt.Disk(0.05, 1.5, 12.0)]
    checked = 0
    for rho, phi in ((6.0, 0.3), (9.0, 2.1)):
        pos = (0.7, rho * math.cos(phi), rho * math.sin(phi), 0.0)
        for sign in (+1, -1):
            got = rt.eval_observer(metric, [], observer("circular", pos=pos, orbit=sign))
            assert got["valid"]
            om, u = got["omega"], got["frame"][0]
            ds = rt.geodesic(np.concatenate([pos, u]), metric, path=1)
            want = np.array([0.0, -om * om * pos[1] * u[0] ** 2, -om * om * pos[2] * u[0] ** 2, 0.0])
            err = np.abs(ds[4:] - want).max() / u[0] ** 2
            print(f"{name} rho {rho} orbit {sign:+d}: Omega {om:.6f}, max |du - want| / (u^t)^2 = {err:.2e}")
            assert err <= 1e-10
            se = np.array([[*pos, -1.0, 0.3, 0.2, 0.1]])
            s0 = np.array([[0.0, 10.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0]])
            hook = rt.eval_disk_emission(metric, disk, rt.DiskEmission(1, 6000.0, orbit=sign), s0, se)
            assert np.isfinite(hook["omega"]).all()
            assert np.float64(om).tobytes() == hook["omega"][0].tobytes(), (om, hook["omega"][0])
            checked += 1
    assert checked == 4


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def kerr_disk_scene():
    """KerrSchild(1, 0.998) with config 5's disk, inside a sky large enough to hold an observer at rho = 12"""
    return rt.KerrSchild(1, 0.998), [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -20.0), rt.Plane(-60.0), rt.Disk(0.05, 2.0, 4.0)]


def orbiting(projection="perspective", max_batch_rays=0, kind="circular"):
    """at rho = 12 in the equatorial plane, on the prograde circular orbit; perspective: looking at the hole, slightly from above is not
    possible (z = 0), so the view is edge-on with the lensed far side above and below; equirect: the full sky, looking along the motion"""
    if projection == "perspective":
        return rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 1.0, 0.7, kind=kind, orbit=+1, max_batch_rays=max_batch_rays)
    return rt.Observer((0, 0, -12, 0), (0, 1, 0, 0), (0, 0, 0, 1), 2 * math.pi, math.pi, kind=kind, orbit=+1, projection="equirect",
                       max_batch_rays=max_batch_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_frame_rule_bit_for_bit(lib, dtype):
    """rtgr_trace_observer == rtgr_trace(state0 = rtgr_make_observer_canvas), every output and the counters; whatever max_batch_rays"""
    metric, objs = kerr_disk_scene()
    for (ni, nj), proj in zip(SIZES, ("perspective", "equirect")):
        st = canvas(lib, metric, orbiting(proj), ni, nj, dtype)
        want = trace_states(lib, metric, objs, st, ni, nj, dtype)
        assert (want["hit32"] == 3).sum() >= 5 and (want["status"] == abi.RAY_EVENT).sum() > ni * nj // 2
        for batch in (200, 0):
            rc, got = trace_observer(lib, metric, objs, orbiting(proj, batch), ni, nj, dtype)
            assert rc == 0
            assert same_bits(got["rgb"], want["rgb"]), (proj, batch)
            for key in OUT_KEYS:
                assert same_bits(got[key], want[key]), (key, proj, batch)
            assert got["counters"] == want["counters"]
        rc, bare = trace_observer(lib, metric, objs, orbiting(proj, 200), ni, nj, dtype, details=False, counters=False)
        assert rc == 0 and same_bits(bare["rgb"], want["rgb"])


@pytest.mark.gpu
def test_device_entry_on_a_side_stream_equals_the_host_entry(lib):
    import torch
    metric, objs = kerr_disk_scene()
    ni, nj = SIZES[1]
    n = ni * nj
    em = rt.DiskEmission(3, T_FRAME)
    rc, host = trace_observer(lib, metric, objs, orbiting("equirect", 200), ni, nj, emit=em)
    assert rc == 0
    sc, opt, ob = rt.make_scene(metric, objs), rt.solver_defaults(), orbiting("equirect", 200)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rgb = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
        g = torch.full((n,), -5.0, dtype=torch.float64, device="cuda")
        dev = _outputs(n, np.float64, device=True)
        o = abi.rtgr_ray_outputs()
        for key in OUT_KEYS:
            setattr(o, key, dev[key].data_ptr())
        ctr = abi.rtgr_counters()
        abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, C.byref(em), rgb.data_ptr(),
                                                          C.byref(o), g.data_ptr(), C.byref(ctr), side.cuda_stream))
        # … and with nothing but the frame asked for: the stream's scratch holds what the emission kernel reads
        rgb2 = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
        abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, C.byref(em), rgb2.data_ptr(),
                                                          None, None, None, side.cuda_stream))
        st = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        abi.check(lib, lib.rtgr_make_observer_canvas_device_f64(None, C.byref(sc), C.byref(ob), ni, nj, 0, nj, st.data_ptr(), side.cuda_stream))
    torch.cuda.synchronize()
    assert rgb.cpu().numpy().tobytes() == host["rgb"].tobytes() and rgb2.cpu().numpy().tobytes() == host["rgb"].tobytes()
    assert g.cpu().numpy().tobytes() == host["g"].tobytes()
    for key in OUT_KEYS:
        assert dev[key].cpu().numpy().tobytes() == host[key].tobytes(), key
    assert ctr.as_dict() == host["counters"]
    assert st.cpu().numpy().tobytes() == canvas(lib, metric, ob, ni, nj).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_textures(lib, dtype):
    """shaded == where(mask, rtgr_eval_texture(coords), plain observer frame), mask and coords by numpy from the outputs (tests/test_textures.py)"""
    from test_textures import NEAREST, _scene as tex_scene, expected, texture
    metric, objs, _, _ = tex_scene("disk")
    objs = [objs[0], rt.Plane(-60.0), objs[2]]      # (past-directed rays that pass the hole lose coordinate time: the far plane further back)
    binds = {1: (texture("rand32x16")[1], abi.TEX_BILINEAR), 3: (texture("rand16x8")[1], NEAREST)}
    for (ni, nj), batch in zip(SIZES, (0, 200)):
        ob = rt.Observer((0, 4, -6, 1.5), (0, -4, 6, -1.5), (0, 0, 0, 1), 1.2, 0.9, max_batch_rays=batch)
        rc, p = trace_observer(lib, metric, objs, ob, ni, nj, dtype)
        assert rc == 0
        want, mask = expected(p, "disk", binds, 0.0, dtype)
        rc, got = trace_observer(lib, metric, objs, ob, ni, nj, dtype, binds=binds)
        assert rc == 0 and same_bits(got["rgb"], want)
        for key in OUT_KEYS:
            assert same_bits(got[key], p[key]), key
        assert got["counters"] == p["counters"]
        assert (p["hit32"] == 3).sum() >= 10 and (p["hit32"] == 1).sum() >= 100 and (got["rgb"] != p["rgb"]).any(axis=0).sum() >= 100
        rc, bare = trace_observer(lib, metric, objs, ob, ni, nj, dtype, binds=binds, details=False, counters=False)
        assert rc == 0 and same_bits(bare["rgb"], want)


def emission_hook(lib, metric, objs, em, ob, s0, se, dtype=np.float64):
    """rtgr_eval_disk_emission_observer_* (ob = None: the static observer) -> dict(g, rgb)"""
    sc = rt.make_scene(metric, objs)
    n = len(se)
    res = dict(g=np.zeros(n, dtype), rgb=np.zeros((n, 3), dtype))
    fn = lib.rtgr_eval_disk_emission_observer_f64 if dtype == np.float64 else lib.rtgr_eval_disk_emission_observer_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(em), C.byref(ob) if ob is not None else None, np.ascontiguousarray(s0).ctypes.data,
                      np.ascontiguousarray(se).ctypes.data, n, None, None, res["g"].ctypes.data, res["rgb"].ctypes.data))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_emission(lib, dtype):
    """emitted == where(hit32 == disk, hook with this observer, plain) bit for bit; g_obs = g_static g(k_0, e_0) / g(k_0, u_static); a static
    observer gives the unchanged hook's g to the bit; the orbiting observer sees part of the disk blueshifted against the static one"""
    metric, objs = kerr_disk_scene()
    em = rt.DiskEmission(3, T_FRAME)
    (ni, nj), batch = (SIZES[0], 0) if dtype == np.float64 else (SIZES[1], 200)
    for kind in ("circular", "static"):
        ob = orbiting("equirect", batch, kind)
        rc, p = trace_observer(lib, metric, objs, ob, ni, nj, dtype)
        rc2, got = trace_observer(lib, metric, objs, ob, ni, nj, dtype, emit=em)
        assert rc == 0 and rc2 == 0
        mask = p["hit32"] == 3
        idx = np.flatnonzero(mask)
        assert len(idx) >= 5
        st = canvas(lib, metric, ob, ni, nj, dtype)
        h = emission_hook(lib, metric, objs, em, ob, st[idx], p["state_end"][idx], dtype)
        want_rgb, want_g = p["rgb"].copy(), np.full(ni * nj, np.nan, dtype)
        want_rgb[:, idx] = h["rgb"].T
        want_g[idx] = h["g"]
        assert same_bits(got["rgb"], want_rgb) and same_bits(got["g"], want_g)
        for key in OUT_KEYS:
            assert same_bits(got[key], p[key]), key
        assert got["counters"] == p["counters"] and np.isfinite(h["g"]).sum() >= 5
        # the unchanged hook: the static observer at the same pairs of states
        static = rt.eval_disk_emission(metric, objs, em, st[idx], p["state_end"][idx], dtype=dtype)
        assert same_bits(emission_hook(lib, metric, objs, em, None, st[idx], p["state_end"][idx], dtype)["g"], static["g"])
        if kind == "static":
            assert same_bits(h["g"], static["g"])
            continue
        if dtype != np.float64:
            continue
        g0 = ol.metric_plain(rt.make_scene(metric, []), np.array([ob.pos[:]]))[0]
        e0 = rt.eval_observer(metric, [], ob)["frame"][0]
        us = -np.linalg.inv(g0)[:, 0]
        us = us / math.sqrt(-(us @ g0 @ us))
        k0 = st[idx][:, 4:]
        ratio = (k0 @ g0 @ e0) / (k0 @ g0 @ us)
        ok = np.isfinite(h["g"]) & np.isfinite(static["g"])
        err = np.abs(h["g"][ok] / (static["g"][ok] * ratio[ok]) - 1).max()
        brighter = int((ratio[ok] > 1).sum())
        print(f"emission, orbiting observer: {len(idx)} disk pixels, {ok.sum()} glow, identity to {err:.2e}, {brighter} with g above the static observer's")
        assert err <= 1e-10
        assert brighter > 0 and int((h["g"][ok] > static["g"][ok]).sum()) == brighter


@pytest.mark.gpu
def test_invalid_frames(lib):
    """no frame: the hook says so, the Python mirror raises, the raw entry ends every ray as RTGR_RAY_NAN and returns 0"""
    metric0, objs = rt.KerrSchild(1, 0.0), kerr_disk_scene()[1]
    cases = [(metric0, observer("velocity", pos=(0, 6, 0, 0), vel=(0, 1, 0, 0))), (metric0, observer("circular", pos=(0, 2.5, 0, 0))),
             (metric0, observer(pos=(0, 6, 0, 0), look=(0, -1, 0.5, 0), up=(0, -2, 1.0, 0))),
             (metric0, observer("velocity", pos=(0, 6, 0, 0), vel=(-1, 0, 0.1, 0)))]
    g, dg = oracle_metric(metric0, (0.0, 2.5, 0.0, 0.0))
    xi = np.array([1.0, 0.0, 2.5 * math.sqrt(1 / 2.5 ** 3), 0.0])
    assert abs(xi @ g @ xi - 0.2) < 1e-12                                   # (g(xi, xi) = +0.2 inside the photon orbit)
    ni, nj = SIZES[1]
    for metric, ob in cases:
        ob.max_batch_rays = 200
        for dtype in (np.float64, np.float32):
            assert not rt.eval_observer(metric, objs, ob, dtype)["valid"]
            rc, got = trace_observer(lib, metric, objs, ob, ni, nj, dtype)
            assert rc == 0 and (got["status"] == abi.RAY_NAN).all() and got["counters"]["not_finished"] == ni * nj
            assert np.isnan(canvas(lib, metric, ob, ni, nj, dtype, objs)).all()
        with pytest.raises(ValueError):
            rt.trace_observer(metric, objs, ob, ni, nj)
        with pytest.raises(ValueError):
            rt.make_observer_canvas(metric, objs, ob, ni, nj)
    res = rt.trace_observer(*kerr_disk_scene(), orbiting("equirect"), ni, nj, emission=rt.DiskEmission(3, T_FRAME), details=True)
    assert res["counters"]["not_finished"] == 0 and np.isfinite(res["g"]).any() and (res["hit"] == 3).any()


@pytest.mark.gpu
def test_refusals(lib):
    """Every refusal: RTGR_ERR_BAD_ARG with a message, rgb untouched."""
    import torch
    from test_grid_metric import ETA
    from test_grid_metric_4d import grid4
    from test_textures import NEAREST, texture
    metric, objs = kerr_disk_scene()
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ni, nj = 8, 6
    n = ni * nj
    rgb = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
    dg = torch.zeros(n, dtype=torch.float64, device="cuda")
    host, red = np.full((3, n), -5.0), np.zeros(n)

    def call(scene=sc, obs=True, emit=False, binds=None, redshift=False, g=False, w=ni, h=nj, hooks=True, vec=None, **over):
        ob = orbiting()
        for key, val in over.items():
            setattr(ob, key, val)
        for key, val in (vec or {}).items():
            setattr(ob, key, (C.c_double * 4)(*val))
        obp = C.byref(ob) if obs else None
        em = rt.DiskEmission(3, T_FRAME)
        emp = C.byref(em) if emit else None
        sh = rt.make_shade(binds) if binds is not None else None
        shp = C.byref(sh) if sh is not None else None
        o = abi.rtgr_ray_outputs()
        o.redshift = red.ctypes.data
        op = C.byref(o) if redshift else None
        rcs = [lib.rtgr_trace_observer_device_f64(None, C.byref(scene), C.byref(opt), obp, w, h, shp, emp, rgb.data_ptr(), op, dg.data_ptr() if g else None,
                                                  None, None)]
        msgs = [lib.rtgr_last_error()]
        rcs.append(lib.rtgr_trace_observer_f64(None, C.byref(scene), C.byref(opt), obp, w, h, shp, emp, host.ctypes.data, op, red.ctypes.data if g else None,
                                               None))
        msgs.append(lib.rtgr_last_error())
        if hooks:        # the canvas and the frame hook share every check of the record and the scene
            st, fr = np.full((max(w, 1) * max(h, 1), 8), -3.0), np.full(16, -3.0)
            rcs.append(lib.rtgr_make_observer_canvas_f64(None, C.byref(scene), obp, w, h, 0, max(h, 1), st.ctypes.data))
            msgs.append(lib.rtgr_last_error())
            if w and h:
                rcs.append(lib.rtgr_eval_observer_f64(None, C.byref(scene), obp, fr.ctypes.data, None, None))
                msgs.append(lib.rtgr_last_error())
            assert (rcs[2] == 0 or (st == -3.0).all()) and (rcs[-1] == 0 or (fr == -3.0).all())
        return rcs, msgs

    user = rt.make_scene(metric, objs)
    user.metric = abi.USER
    nan, inf = math.nan, math.inf
    _, tex = texture("rand16x8")
    cases = [(dict(obs=False), b"rtgr_observer is NULL"), (dict(kind=3), b"unknown rtgr_observer.kind"), (dict(projection=2), b"unknown rtgr_observer.projection"),
             (dict(flags=1), b"flags"), (dict(pad=1), b"pad"), (dict(vec=dict(pos=(0, nan, -12, 0))), b"pos"), (dict(vec=dict(look=(0, inf, 0, 0))), b"look"),
             (dict(vec=dict(up=(nan, 0, 0, 1))), b"up"), (dict(kind=1, vec=dict(vel=(1, nan, 0, 0))), b"vel"), (dict(fov_x=nan), b"finite"),
             (dict(fov_y=inf), b"finite"), (dict(fov_x=0.0), b"(0, pi)"), (dict(fov_x=math.pi), b"(0, pi)"), (dict(fov_y=-0.1), b"(0, pi)"),
             (dict(fov_y=3.5), b"(0, pi)"), (dict(projection=1, fov_x=6.3), b"2 pi"), (dict(projection=1, fov_y=3.2), b"2 pi"),
             (dict(projection=1, fov_x=0.0), b"2 pi"), (dict(orbit=0.5), b"+1"), (dict(orbit=0.0), b"+1"), (dict(orbit=nan), b"orbit"),
             (dict(vec=dict(pos=(0, 0, -12, 0.5))), b"pos[3]"), (dict(scene=user), b"RTGR_USER"),
             (dict(redshift=True, hooks=False), b"redshift"), (dict(w=0), b"bad canvas"), (dict(h=0), b"bad canvas"), (dict(g=True, hooks=False), b"emit is NULL"),
             (dict(emit=True, binds={3: (tex, NEAREST)}, hooks=False), b"one or the other"),
             (dict(binds={4: (tex, NEAREST)}, hooks=False), b"bind")]
    for kw, word in cases:
        rcs, msgs = call(**kw)
        assert rcs == [abi.ERR_BAD_ARG] * len(rcs) and all(word in m for m in msgs), (kw, rcs, msgs)
    # the emission's own refusals come through
    em_bad = rt.DiskEmission(1, T_FRAME)
    rc = lib.rtgr_trace_observer_f64(None, C.byref(sc), C.byref(opt), C.byref(orbiting()), ni, nj, None, C.byref(em_bad), host.ctypes.data, None, None, None)
    assert rc == abi.ERR_BAD_ARG and b"Sphere" in lib.rtgr_last_error()
    # a time-dependent grid
    flat4 = grid4(np.broadcast_to(ETA, (6, 6, 6, 10)).copy(), 4, -1.0, 1.0, (-3.0,) * 3, 1.0, name="flat4")
    g4 = rt.make_scene(flat4, [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(-20.0), rt.Disk(0.05, 2.0, 4.0)])
    rcs, msgs = call(scene=g4, kind=0, vec=dict(pos=(0, 0, -1, 0)))
    assert rcs == [abi.ERR_BAD_ARG] * 4 and all(b"4-D" in m for m in msgs), (rcs, msgs)
    torch.cuda.synchronize()
    assert bool((rgb == -5.0).all()) and (host == -5.0).all()
    rcs, _ = call()
    torch.cuda.synchronize()
    assert rcs == [0, 0, 0, 0] and rgb.cpu().numpy().tobytes() == host.tobytes() and not (host == -5.0).any()
    # the tile kernel writes whole frames only: more than one batch is refused up front, one batch is served
    with abi.options(lib, tile=1):
        rcs, msgs = call(max_batch_rays=ni, hooks=False)
        assert rcs == [abi.ERR_BAD_ARG] * 2 and all(b"tile = 1" in m and b"observer" in m for m in msgs), (rcs, msgs)
        assert call(hooks=False)[0] == [0, 0]
    # a fov at its upper bound is a panorama's right
    assert call(projection=1, fov_x=2 * math.pi, fov_y=math.pi)[0] == [0, 0, 0, 0]


@pytest.mark.gpu
def test_capture_replay_and_trim(lib):
    """ctr == NULL: the call is captured once workspace and scratch exist (a linear chain of kernels on one stream), replays the eager
    frame, refuses to grow its scratch or to deliver counters during capture; rtgr_trim afterwards, and a fresh call gives the same"""
    import torch
    metric, objs = kerr_disk_scene()
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    em = rt.DiskEmission(3, T_FRAME)
    ni, nj = SIZES[1]
    n = ni * nj
    ob = orbiting("equirect", 200)
    side = torch.cuda.Stream()
    hip = _hip_runtime()

    def call(out, g, width=ni, ctr=None):
        return lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), width, nj, None, C.byref(em), out.data_ptr(), None,
                                                  g.data_ptr(), C.byref(ctr) if ctr is not None else None, side.cuda_stream)

    with torch.cuda.stream(side):
        eager, out = (torch.zeros((3, n), dtype=torch.float64, device="cuda") for _ in range(2))
        g_eager, g_out = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(2))
        wide, g_wide = torch.zeros((3, 4 * n), dtype=torch.float64, device="cuda"), torch.zeros(4 * n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    abi.check(lib, call(eager, g_eager))                       # the warm-up: workspace and scratch of this size exist afterwards
    torch.cuda.synchronize()
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc_big = call(wide, g_wide, width=4 * ni)                  # a wider frame: the scratch would have to grow
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
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    abi.check(lib, lib.rtgr_trim(None))
    fresh, g_fresh = torch.zeros((3, n), dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    abi.check(lib, call(fresh, g_fresh))
    torch.cuda.synchronize()
    assert torch.equal(fresh, eager)
