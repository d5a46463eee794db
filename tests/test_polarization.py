"""Polarized disk images (include/rtgr.h "polarized disk images"): the fractional Stokes pair (q, u) of a thin disk by
Walker-Penrose transport — one kernel around the untouched trace.  The judge is tests/polarization_truth.py: a truth-side parallel
transporter (DOP853 on the symbolic metric) and a numpy restatement of the header's contract.

CPU tests: the symbols, the struct layout (ctypes, a compiled C caller), the transporter's own invariants, the conservation of the two
constants along truth-transported rays, the camera-side solve.  GPU tests: the two hooks against numpy, the end-to-end physics against
the transporter, flat space, Schwarzschild's mirror symmetry, the frame rule bit for bit, the refusals."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import polarization_truth as PT
from conftest import ROOT
from scenes import rt

abi = rt._abi
POL_EXPORTS = ("rtgr_polarization_device_f64", "rtgr_polarization_device_f32", "rtgr_trace_polarized_device_f64", "rtgr_trace_polarized_device_f32",
               "rtgr_trace_polarized_f64", "rtgr_trace_polarized_f32", "rtgr_eval_polarization_f64", "rtgr_eval_polarization_f32",
               "rtgr_eval_walker_penrose_f64", "rtgr_eval_walker_penrose_f32")
SIZES = ((48, 32), (37, 19))
T_FRAME = 30000.0
OUT_KEYS = ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject")
# 12 seeded rays per metric, chosen on the CPU so that none comes within 1.05 r_+ of the hole over 15 units of affine parameter (seed 2
# does, for a = 0 and a = 0.8: replaced)
SEEDS = (0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12)
METRICS = (("ks_true", 0.0), ("ks_true", 0.8), ("ks_true", 0.998), ("mink", 0.0))


def metric_of(kind, a):
    return rt.minkowski if kind == "mink" else rt.KerrSchild(1, a)


@functools.lru_cache(maxsize=None)
def rays(kind, a):
    """the 12 truth-transported rays of one metric: (start (x, k, f), end (x, k, f), r_min), computed once"""
    out = []
    for seed in SEEDS:
        x, k, f = PT.random_ray(seed, kind, 1.0, a)
        y, rmin = PT.transport(kind, 1.0, a, x, k, f, 15.0)
        out.append((np.concatenate([x, k, f]), y, rmin))
    return tuple(out)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(POL_EXPORTS) <= set(abi.EXPORTS) and len(POL_EXPORTS) == 10
    lib = abi.load()
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    for s in POL_EXPORTS:
        assert hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    assert {"Polarization", "trace_polarized", "eval_polarization", "eval_walker_penrose"} <= set(rt.api.__all__)
    # the Julia module: it binds host-pointer entries only (no *_device_* symbol of any feature), so the six host-pointer symbols, each by a
    # ccall (tests/test_julia_stub.py holds every ccall against its C prototype), the record, its constants and the four names
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    for s in POL_EXPORTS:
        assert ("_device_" in s) != (f"ccall((:{s}, librtgr)" in jl), s
    for word in ("struct RtgrPolarization", "const RTGR_POL_SCATTER = UInt32(0)", "const RTGR_POL_FIELD = UInt32(1)", "function Polarization(",
                 "function trace_rays_polarized(", "function eval_polarization(", "function eval_walker_penrose(",
                 "#   RtgrPolarization 64   kind 0, flags 4, deg0 8, deg1 16, field 24, reserved 48"):
        assert word in jl, word


def test_struct_layout_ctypes_and_c(tmp_path):
    s = abi.rtgr_polarization
    assert C.sizeof(s) == 64
    assert [getattr(s, f).offset for f in ("kind", "flags", "deg0", "deg1", "field", "reserved")] == [0, 4, 8, 16, 24, 48]
    exe = str(tmp_path / "polarization_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "polarization_layout.c"), "-o", exe])
    assert subprocess.check_output([exe]).split() == [b"64", b"0", b"4", b"8", b"16", b"24", b"48"]
    p = rt.Polarization("field", 0.7, field=(0, 1, 2))
    assert (p.kind, p.flags, p.deg0, list(p.field), list(p.reserved)) == (abi.POL_FIELD, 0, 0.7, [0, 1, 2], [0, 0])
    with pytest.raises(ValueError):
        rt.Polarization("fields")


@pytest.mark.parametrize("kind,a", METRICS)
def test_truth_transport_conserves_and_the_forms_are_constant(kind, a):
    """The transporter keeps g(k, k) and g(k, f) at <= 1e-10, every ray stays outside 1.05 r_+, and the numpy Y and h conserve kappa_1,
    kappa_2 to <= 1e-9 absolute (9.9e-13 was measured on three such rays; the margin is the integrator's)."""
    rp = 1.0 + np.sqrt(max(1.0 - a * a, 0.0))
    worst = 0.0
    for s, y, rmin in rays(kind, a):
        assert kind == "mink" or rmin > 1.05 * rp, rmin
        g1 = PT.g_at(kind, y[:4], 1.0, a)
        assert abs(PT.inner(g1, y[4:8], y[4:8])) <= 1e-10 and abs(PT.inner(g1, y[4:8], y[8:])) <= 1e-10
        k0, k1 = PT.kappa(s[:4], s[4:8], s[8:], a), PT.kappa(y[:4], y[4:8], y[8:], a)
        worst = max(worst, np.abs(k1 - k0).max())
    print(f"{kind} a = {a}: kappa drift {worst:.2e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("kind,a", METRICS)
def test_the_camera_side_solve_returns_the_screen_components(kind, a):
    """At the far end of each ray stands a static observer; the 2 x 2 solve gives the components of the transported f on (e^_x, e^_y) to
    1e-9, and its matrix has condition number < 1 + 1e-6."""
    for s, y, _ in rays(kind, a):
        x, k, f = y[:4], y[4:8], y[8:]
        g = PT.g_at(kind, x, 1.0, a)
        e0 = np.array([1.0, 0, 0, 0]) / np.sqrt(-g[0][0])
        k = k / (-PT.inner(g, k, e0) * np.sqrt(2.0)) * -1.0   # the library's normalisation: g(k, e_0) = +1/sqrt(2), past-directed
        n = np.sqrt(2.0) * k + e0
        # any frame whose e_right, e_up span the screen: two vectors orthogonal to e_0, fixed by the coordinates
        up = np.array([0.0, 0.1, 0.2, 1.0]); up = up + PT.inner(g, up, e0) * e0
        ri = np.array([0.0, 1.0, -0.3, 0.2]); ri = ri + PT.inner(g, ri, e0) * e0
        frame = np.array([e0, PT.normalise(g, ri), PT.normalise(g, up), n])
        _, ex, ey = PT.screen_basis(g, frame, k)
        kap = PT.kappa(x, k, f, a)
        al, be, Mx = PT.camera_solve(x, k, a, ex, ey, kap)
        assert np.linalg.cond(Mx) < 1 + 1e-6
        assert abs(al - PT.inner(g, f, ex)) <= 1e-9 and abs(be - PT.inner(g, f, ey)) <= 1e-9


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def disk_scene(kind="ks_true", a=0.998):
    """a disk outside every photon orbit, inside a sky large enough to hold an observer at distance 15"""
    return metric_of(kind, a), [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -25.0), rt.Plane(-80.0), rt.Disk(0.05, 4.5, 8.0)]


def inclined(up=(0, 0, 0, 1), pos=(0, 0, -12, 8), max_batch_rays=0):
    return rt.Observer(pos, (0, -pos[1], -pos[2], -pos[3]), up, 1.3, 0.9, max_batch_rays=max_batch_rays)


SCATTER = dict(kind="scatter", deg0=0.12, deg1=0.4)
FIELD = dict(kind="field", deg0=0.7, field=(0.3, 1.0, 0.5))
_FRAMES = {}


def pframe(kind, a, emitter, orbit, law, size=SIZES[0], dtype=np.float64, ob=None, batch=0):
    key = (kind, a, emitter, orbit, tuple(sorted(law.items())), size, np.dtype(dtype).name, batch, None if ob is None else bytes(ob))
    if key not in _FRAMES:
        metric, objs = disk_scene(kind, a)
        o = ob if ob is not None else inclined(max_batch_rays=batch)
        res = rt.trace_polarized(metric, objs, o, size[0], size[1], rt.DiskEmission(3, T_FRAME, emitter=emitter, orbit=orbit), rt.Polarization(**law),
                                 dtype=dtype, details=True)
        res["s0"] = rt.make_observer_canvas(metric, objs, o, size[0], size[1], dtype=dtype)
        res["frame"] = rt.eval_observer(metric, objs, o, dtype=dtype)["frame"]
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FRAMES[key] = res
    return _FRAMES[key]


# Float32 against the Float64 hook, as a RELATIVE error of kappa (per point: |kappa32 - kappa64| / max |kappa64|).  Expected size: each
# form is a sum of terms up to |k||f| r^2 rounded at eps32, so eps32 r^2 / |kappa| if every term were that large and the roundings all
# fell the same way; the terms are mostly smaller than r^2 and their roundings partly cancel, so the measured figure lies below it.
# Measured maximum over the rays of METRICS (profiles/polarization/README.md); asserted at 8 x that.
F32_WP_MEASURED = 3.66e-7
# ... and of rtgr_eval_polarization_f32 against _f64 at pairs of real frames: max |(q, u)32 - (q, u)64| / delta (an angle error: twice the
# relative error of kappa at the two ends, plus the triads').  Measured maximum over CASES x both laws; asserted at 8 x that.
F32_POL_MEASURED = 1.18e-5
# ... and of aux and delta, absolute (both are O(1) or below): measured maximum
F32_AUX_MEASURED = 6.71e-7


@pytest.mark.gpu
@pytest.mark.parametrize("kind,a", METRICS)
def test_walker_penrose_hook_against_numpy_and_conserved(lib, kind, a):
    """rtgr_eval_walker_penrose_f64 at both ends of the truth-transported rays: the numpy forms to 1e-12 (|kappa| + |k||f| r), hence kappa
    conserved to 1e-9 by the DEVICE's forms.  Float32 against the Float64 hook: the relative error of kappa, printed beside its expected
    size eps32 r^2 / |kappa| and asserted at 8 x the measured maximum (F32_WP_MEASURED)."""
    R = rays(kind, a)
    S = np.array([np.concatenate([s[:8], y[:8]]) for s, y, _ in R]).reshape(-1, 8)
    F = np.array([np.concatenate([s[8:], y[8:]]) for s, y, _ in R]).reshape(-1, 4)
    got = rt.eval_walker_penrose(metric_of(kind, a), [], S, F)
    want = np.array([PT.kappa(s[:4], s[4:], f, a) for s, f in zip(S, F)])
    r = np.array([PT.kerr_radius(s[:4], a) for s in S])
    scale = np.abs(want).max(axis=1) + np.linalg.norm(S[:, 4:], axis=1) * np.linalg.norm(F, axis=1) * r
    err = (np.abs(got - want).max(axis=1) / scale).max()
    drift = np.abs(got[0::2] - got[1::2]).max()
    g32 = rt.eval_walker_penrose(metric_of(kind, a), [], S, F, dtype=np.float32)
    kmax = np.abs(got).max(axis=1)
    e32 = (np.abs(g32 - got).max(axis=1) / kmax).max()
    expect = (np.finfo(np.float32).eps * r * r / kmax).max()
    print(f"{kind} a = {a}: device vs numpy {err:.2e}, device drift {drift:.2e}, f32 relative error of kappa {e32:.3e} (expected size eps32 r^2/|kappa| ~ {expect:.2e})")
    assert err <= 1e-12
    assert drift <= 1e-9
    assert e32 <= 8 * F32_WP_MEASURED


CASES = [("ks_true", 0.998, "kepler", +1), ("ks_true", 0.998, "kepler", -1), ("ks_true", 0.0, "kepler", +1), ("ks_true", 0.0, "kepler", -1),
         ("ks_true", 0.998, "rigid", 0.0), ("ks_true", 0.0, "rigid", 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("law", [SCATTER, FIELD], ids=["scatter", "field"])
@pytest.mark.parametrize("kind,a,emitter,orbit", CASES)
def test_polarization_hook_against_the_restatement(lib, kind, a, emitter, orbit, law):
    """Pairs from real frames into the hook and into numpy (the symbolic metric): kappa, f_em, aux, delta, q, u to 1e-10; f_em is a unit
    vector orthogonal to u and k_end to 1e-12."""
    f = pframe(kind, a, emitter, orbit, law, SIZES[1])
    idx = np.flatnonzero(f["hit"] == 3)
    assert len(idx) >= 20
    idx = idx[:: max(1, len(idx) // 40)]
    metric, objs = disk_scene(kind, a)
    em, pol = rt.DiskEmission(3, T_FRAME, emitter=emitter, orbit=orbit), rt.Polarization(**law)
    h = rt.eval_polarization(metric, objs, em, pol, inclined(), f["s0"][idx], f["state_end"][idx])
    assert h["valid"].all()
    worst = ortho = 0.0
    for n, p in enumerate(idx):
        m = PT.model(kind, 1.0, a, f["s0"][p], f["state_end"][p], f["frame"], 0 if emitter == "kepler" else 1, float(orbit), 0 if law["kind"] == "scatter" else 1,
                     law["deg0"], law.get("deg1", 0.0), law.get("field", (0, 0, 0)))
        for got, want in ((h["kappa"][n], m["kappa"]), (h["f_em"][n], m["f_em"]), (h["aux"][n], m["aux"]), (h["delta"][n], m["delta"]),
                          (h["q"][n], m["q"]), (h["u"][n], m["uu"])):
            got, want = np.atleast_1d(got), np.atleast_1d(want)
            worst = max(worst, (np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())
        fe, g = h["f_em"][n], m["g"]
        ortho = max(ortho, abs(PT.inner(g, fe, m["u"])), abs(PT.inner(g, fe, f["state_end"][p][4:])), abs(PT.inner(g, fe, fe) - 1))
        # the frame wrote this pixel from the same kernel: the same bits
        assert h["q"][n] == f["q"][p] and h["u"][n] == f["u"][p] and h["aux"][n] == f["aux"][p]
    # the Float32 hook at the same pairs (rounded to Float32) against the Float64 hook
    h32 = rt.eval_polarization(metric, objs, em, pol, inclined(), f["s0"][idx], f["state_end"][idx], dtype=np.float32)
    assert h32["valid"].all()
    e32 = max(np.abs((h32[k] - h[k]) / h["delta"]).max() for k in ("q", "u"))
    a32 = max(np.abs(h32["aux"] - h["aux"]).max(), np.abs(h32["delta"] - h["delta"]).max())
    print(f"{kind} a = {a} {emitter} {orbit} {law['kind']}: worst {worst:.2e}, orthogonality {ortho:.2e}, f32 (q, u)/delta {e32:.3e}, f32 aux, delta {a32:.3e}")
    assert worst <= 1e-10 and ortho <= 1e-12
    assert e32 <= 8 * F32_POL_MEASURED and a32 <= 8 * F32_AUX_MEASURED


@pytest.mark.gpu
def test_end_to_end_against_truth_transport(lib):
    """Every interior disk pixel of the 48 x 32 a = 0.998 frame: numpy's f_em at the device's s_end, truth-transported BACK along the ray
    from lambda_end to 0, projected on (e^_x, e^_y), against the device's (q, u) / delta to 1e-8.  No pixel is excluded."""
    kind, a = "ks_true", 0.998
    ni, nj = SIZES[0]
    # a wide-angle view of a disk that reaches in to rho = 2 (prograde orbits exist there): some tens of interior pixels, each of which
    # costs one truth-side integration
    metric, objs = metric_of(kind, a), [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -25.0), rt.Plane(-80.0), rt.Disk(0.05, 2.0, 8.0)]
    ob = rt.Observer((0, 0, -12, 8), (0, 0, 12, -8), (0, 0, 0, 1), 2.2, 1.7)
    f = rt.trace_polarized(metric, objs, ob, ni, nj, rt.DiskEmission(3, T_FRAME), rt.Polarization(**FIELD), details=True)
    f["s0"] = rt.make_observer_canvas(metric, objs, ob, ni, nj)
    f["frame"] = rt.eval_observer(metric, objs, ob)["frame"]
    disk = (f["hit"] == 3).reshape(nj, ni)
    inner = disk.copy()
    inner[0, :] = inner[-1, :] = inner[:, 0] = inner[:, -1] = False
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            inner[1:-1, 1:-1] &= disk[1 + dj:nj - 1 + dj, 1 + di:ni - 1 + di]
    idx = np.flatnonzero(inner.ravel())
    assert len(idx) >= 20, len(idx)
    worst = 0.0
    for p in idx:
        s0, se = f["s0"][p], f["state_end"][p]
        E = PT.emitter(kind, 1.0, a, se, 0, 1.0, 1, FIELD["deg0"], 0.0, FIELD["field"])
        y, _ = PT.transport(kind, 1.0, a, se[:4], se[4:], E["f_em"], -float(f["lambda_end"][p]))
        g0 = PT.g_at(kind, s0[:4], 1.0, a)
        _, ex, ey = PT.screen_basis(g0, f["frame"], s0[4:])
        al, be = PT.inner(g0, y[8:], ex), PT.inner(g0, y[8:], ey)
        d = al * al + be * be
        want = np.array([(al * al - be * be) / d, 2 * al * be / d])
        got = np.array([f["q"][p], f["u"][p]]) / E["delta"]
        worst = max(worst, np.abs(got - want).max())
    print(f"{len(idx)} interior pixels, worst |(q, u)/delta - truth| = {worst:.2e}")
    assert worst <= 1e-8


@pytest.mark.gpu
def test_flat_space(lib):
    """Minkowski, RIGID Omega = 0, SCATTER, static observer with up = +z: q = delta, u = 0 to 1e-12 on every disk pixel; up turned by
    psi = 0.3 towards e_right: chi turns by + psi (the header: chi runs from e^_x towards e^_y), exactly delta (cos 2 psi, sin 2 psi) on the
    look axis — asserted there in closed form to 1e-12 — and the restatement's value elsewhere; FIELD with B = e_z gives SCATTER's direction (the contract's cross(p^, B^) is the same
    vector; the issue expected the negated pair, which its own formula does not give)."""
    # the camera looks horizontally from above the disk, so that its e_up IS +z: then e^_y lies in the plane of z and the ray for every
    # pixel, and the disk-plane electric vector is e^_x exactly (an inclined look axis tilts e_up away from z off the frame's centre line)
    level = dict(pos=(0, 0, -12, 5))
    look = lambda up: rt.Observer(level["pos"], (0, 0, 1, 0), up, 1.3, 1.4)
    base = pframe("mink", 0.0, "rigid", 0.0, SCATTER, ob=look((0, 0, 0, 1)))
    d = base["hit"] == 3
    assert d.sum() >= 20
    mu = base["aux"][d]
    delta = SCATTER["deg0"] * (1 - mu) / (1 + SCATTER["deg1"] * mu)
    assert np.abs(base["q"][d] - delta).max() <= 1e-12 and np.abs(base["u"][d]).max() <= 1e-12
    assert np.isnan(base["q"][~d]).all() and np.isnan(base["u"][~d]).all() and np.isnan(base["aux"][~d]).all()
    # the SAME rays under a camera whose up is turned by psi towards e_right: the hook against the restatement to 1e-12, and the sign of
    # the header's convention (chi turns by + psi: u > 0 where it was 0).  Off the frame's centre the projected e_up and e_right are not
    # orthogonal, so the turn of chi equals psi on the look axis only: the exact statement is the restatement's.
    psi = 0.3
    fr = base["frame"]
    up = np.cos(psi) * fr[2] + np.sin(psi) * fr[1]
    metric, objs = disk_scene("mink", 0.0)
    em, pol = rt.DiskEmission(3, T_FRAME, emitter="rigid", orbit=0.0), rt.Polarization(**SCATTER)
    idx = np.flatnonzero(d)
    h = rt.eval_polarization(metric, objs, em, pol, look(tuple(up)), base["s0"][idx], base["state_end"][idx])
    fr2 = rt.eval_observer(metric, objs, look(tuple(up)))["frame"]
    worst = 0.0
    for n, p in enumerate(idx):
        m = PT.model("mink", 1.0, 0.0, base["s0"][p], base["state_end"][p], fr2, 1, 0.0, 0, SCATTER["deg0"], SCATTER["deg1"], (0, 0, 0))
        worst = max(worst, abs(h["q"][n] - m["q"]), abs(h["u"][n] - m["uu"]))
    print(f"flat space, up turned: worst against the restatement {worst:.2e}")
    assert worst <= 1e-12 and (h["u"] > 0).all()
    # THE CLOSED FORM, independent of the restatement: a camera that looks down at the disk point (0, -6, 0) from (0, -12, 8), up = +z, and the
    # ray ON its look axis (n = e_look, so e^_y = e_up, e^_x = e_right exactly).  The disk-plane electric vector there is e_right, so
    # chi = 0 and (q, u) = delta (1, 0); under up' = cos psi up + sin psi right it is cos psi e_right' + sin psi e_up', chi = +psi:
    # (q, u) = delta (cos 2 psi, + sin 2 psi), the sign of the header's convention.  mu = 0.8 is the cosine of the ray to the disk normal.
    pos, lookv = (0, 0, -12, 8), (0, 0, 6, -8)
    cam = lambda up: rt.Observer(pos, lookv, up, 1.3, 0.9)
    fr0 = rt.eval_observer(metric, objs, cam((0, 0, 0, 1)))["frame"]
    delta0 = SCATTER["deg0"] * (1 - 0.8) / (1 + SCATTER["deg1"] * 0.8)
    for ps in (0.0, psi, -0.7):
        upv = np.cos(ps) * fr0[2] + np.sin(ps) * fr0[1]
        fr1 = rt.eval_observer(metric, objs, cam(tuple(upv)))["frame"]
        k0 = (fr1[3] - fr1[0]) / np.sqrt(2.0)
        assert np.abs(fr1[3] - fr0[3]).max() <= 1e-14 and abs(k0[3] + 0.8 / np.sqrt(2.0)) <= 1e-14
        s0 = np.concatenate([pos, k0])
        se = np.concatenate([np.array(pos) + 10 * np.sqrt(2.0) * k0, k0])      # z = 0 at lambda = 10 sqrt 2: the point (0, -6, 0)
        assert abs(se[3]) <= 1e-14 and abs(se[2] + 6) <= 1e-14
        hc = rt.eval_polarization(metric, objs, em, pol, cam(tuple(upv)), s0[None], se[None])
        print(f"flat space, look axis, psi = {ps}: (q, u)/delta = ({hc['q'][0] / delta0:.15f}, {hc['u'][0] / delta0:.15f})")
        assert hc["valid"][0] and abs(hc["aux"][0] - 0.8) <= 1e-12 and abs(hc["delta"][0] - delta0) <= 1e-12
        assert abs(hc["q"][0] - delta0 * np.cos(2 * ps)) <= 1e-12 and abs(hc["u"][0] - delta0 * np.sin(2 * ps)) <= 1e-12
    # FIELD with B = e_z: by the contract f_em = cross(p^, B^) is SCATTER's cross(p^, e_z') — the same vector, the same (q, u) / delta
    fz = pframe("mink", 0.0, "rigid", 0.0, dict(kind="field", deg0=1.0, field=(0, 0, 1)), ob=look((0, 0, 0, 1)))
    assert np.abs(fz["q"][d] - base["q"][d] / delta).max() <= 1e-12 and np.abs(fz["u"][d] - base["u"][d] / delta).max() <= 1e-12


@pytest.mark.gpu
def test_schwarzschild_mirror_symmetry(lib):
    """a = 0, RIGID Omega = 0, observer in the plane x = 0 looking at the origin, up = +z: q(i, j) = q(ni-1-i, j), u(i, j) = -u(ni-1-i, j)
    to 1e-9; pixels whose partner is off the disk are skipped, at most a quarter of the disk's."""
    f = pframe("ks_true", 0.0, "rigid", 0.0, FIELD | dict(field=(0.0, 0.0, 1.0)))
    ni, nj = SIZES[0]
    hit, q, u = (f[k].reshape(nj, ni) for k in ("hit", "q", "u"))
    d = hit == 3
    both = d & d[:, ::-1]
    assert d.sum() >= 20 and (d & ~both).sum() <= d.sum() / 4
    assert np.abs(q - q[:, ::-1])[both].max() <= 1e-9 and np.abs(u + u[:, ::-1])[both].max() <= 1e-9
    assert np.abs(u[both]).max() > 1e-3    # (not trivially zero)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("size", SIZES)
def test_frame_rule_bit_for_bit(lib, dtype, size):
    """The planes are where(hit == disk, hook(canvas states, state_end), NaN); rgb, g, every per-ray output and the counters are
    rtgr_trace_observer_*'s; one row, five rows and the default batch give the same bytes."""
    kind, a = "ks_true", 0.998
    metric, objs = disk_scene(kind, a)
    em, pol = rt.DiskEmission(3, T_FRAME), rt.Polarization(**FIELD)
    f = pframe(kind, a, "kepler", +1, FIELD, size, dtype)
    d = f["hit"] == 3
    assert d.sum() >= 20
    h = rt.eval_polarization(metric, objs, em, pol, inclined(), f["s0"], np.where(d[:, None], f["state_end"], f["s0"]), dtype=dtype)
    for k in ("q", "u", "aux"):
        want = np.where(d, h[k], np.nan)
        assert f[k].tobytes() == want.astype(dtype).tobytes(), k
    plain = rt.trace_observer(metric, objs, inclined(), size[0], size[1], emission=em, dtype=dtype, details=True)
    for k in ("rgb", "g") + OUT_KEYS:
        assert plain[k].tobytes() == f[k].tobytes(), k
    assert plain["counters"] == f["counters"]
    for rows in (1, 5):
        b = pframe(kind, a, "kepler", +1, FIELD, size, dtype, batch=rows * size[0])
        for k in ("rgb", "g", "q", "u", "aux") + OUT_KEYS:
            assert b[k].tobytes() == f[k].tobytes(), (rows, k)


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(lib):
    metric, objs = disk_scene()
    em, ob = rt.DiskEmission(3, T_FRAME), inclined()
    good = dict(kind="scatter", deg0=0.1, deg1=0.5)
    s = np.zeros((4, 8))

    def refused(match, metric=metric, em=em, ob=ob, **over):
        p = rt.Polarization(**(good | {k: v for k, v in over.items() if k in ("kind", "deg0", "deg1", "field")}))
        for k in ("flags",):
            if k in over:
                p.flags = over[k]
        if "reserved" in over:
            p.reserved[1] = over["reserved"]
        with pytest.raises(abi.RtgrError, match=match):
            rt.trace_polarized(metric, objs, ob, 8, 8, em, p)
        with pytest.raises(abi.RtgrError, match=match):
            rt.eval_polarization(metric, objs, em, p, ob, s, s)

    refused("flags", flags=1)
    refused("reserved", reserved=1.0)
    refused("finite", deg0=float("nan"))
    refused("finite", deg1=float("inf"))
    refused("finite", kind="field", field=(0, float("nan"), 1))
    refused("deg0", deg0=-0.1)
    refused("deg1", deg1=-1.0)
    refused("must not be zero", kind="field")
    refused("must be 0", field=(0, 1, 0))
    refused("RTGR_KS_TRUE", metric=rt.KerrSchild(1, 0.5, textbook=False))
    refused("RTGR_KS_TRUE", metric=rt.KerrSchild(1, 0.5, textbook=False, generic=True))
    p = rt.Polarization(**good)
    p.kind = 7
    with pytest.raises(abi.RtgrError, match="unknown rtgr_polarization.kind"):
        rt.trace_polarized(metric, objs, ob, 8, 8, em, p)
    with pytest.raises(abi.RtgrError, match="pol"):
        rt.trace_polarized(metric, objs, ob, 8, 8, em, None)
    with pytest.raises(abi.RtgrError, match="emit"):
        rt.trace_polarized(metric, objs, ob, 8, 8, None, rt.Polarization(**good))
    with pytest.raises(abi.RtgrError, match="RTGR_KS_TRUE"):
        rt.eval_walker_penrose(rt.KerrSchild(1, 0.5, textbook=False), [], s, np.zeros((4, 4)))
    # the C entry leaves its outputs untouched
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    bad = rt.Polarization(**good)
    bad.flags = 2
    n = 64
    rgb, q, u = np.full((3, n), 7.0), np.full(n, 7.0), np.full(n, 7.0)
    rc = lib.rtgr_trace_polarized_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), 8, 8, None, C.byref(em), C.byref(bad), rgb.ctypes.data, None, None,
                                      q.ctypes.data, u.ctypes.data, None, None)
    assert rc == abi.ERR_BAD_ARG and (rgb == 7).all() and (q == 7).all() and (u == 7).all()


@pytest.mark.gpu
def test_invalid_points_give_nan_or_zero_and_no_error(lib):
    """An observer on the axis has no screen the forms can be evaluated on: NaN in q, u on the disk, no error.  An emitter inside the photon
    orbit (a = 0, KEPLER at rho < 3) is invalid: q = u = 0 where delta is finite."""
    metric, objs = disk_scene("ks_true", 0.0)
    em, pol = rt.DiskEmission(3, T_FRAME), rt.Polarization(**SCATTER)
    ob = rt.Observer((0, 0, 0, 14), (0, 0, 0, -1), (0, 0, 1, 0), 1.3, 0.9)
    res = rt.trace_polarized(metric, objs, ob, 16, 12, em, pol)
    d = res["g"] == res["g"]
    assert d.sum() >= 10 and np.isnan(res["q"][d]).all() and np.isnan(res["u"][d]).all() and np.isfinite(res["aux"][d]).all()
    fr = pframe("ks_true", 0.0, "kepler", +1, SCATTER, SIZES[1])
    p = np.flatnonzero(fr["hit"] == 3)[:3]
    se = fr["state_end"][p].copy()
    se[:, 1:3] *= 2.5 / np.hypot(se[:, 1], se[:, 2])[:, None]
    h = rt.eval_polarization(metric, objs, em, rt.Polarization(**FIELD), inclined(), fr["s0"][p], se)   # (FIELD: delta = deg0 is finite)
    assert not h["valid"].any() and (h["q"] == 0).all() and (h["u"] == 0).all()
    # ... and NaN where delta is not finite: SCATTER's mu is taken against the same (non-existent) emitter, so delta is NaN there
    hs = rt.eval_polarization(metric, objs, em, pol, inclined(), fr["s0"][p], se)
    assert not hs["valid"].any() and not np.isfinite(hs["delta"]).any() and np.isnan(hs["q"]).all() and np.isnan(hs["u"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_degenerate_screen_basis_gives_nan(lib, dtype):
    """The 4096 eps rule of the screen basis, both branches, in point mode.  A ray whose direction n is e_up leaves e_up no part orthogonal
    to n (the first test); n = e_right gives e^_y = e_up and leaves e_right none (the second): NaN and valid = 0.  With n turned away
    towards e_look by an angle t the squared norm that the rule looks at is sin^2 t.  The bound 4096 eps is 9.1e-13 in Float64 and 4.9e-4
    in Float32, so t = 1e-2 (Float32: 0.1) is valid and finite with |(q, u)| = delta, and t = 1e-9 (Float32: 1e-3) is NaN again: a factor
    16 on either side of the rule at least.  The end state is a real pixel's."""
    metric, objs = disk_scene("ks_true", 0.998)
    em, pol = rt.DiskEmission(3, T_FRAME), rt.Polarization(**FIELD)
    f = pframe("ks_true", 0.998, "kepler", +1, FIELD, SIZES[1], dtype)
    p = np.flatnonzero(f["hit"] == 3)[7]
    fr = f["frame"].astype(np.float64)
    big, small = (0.1, 1e-3) if dtype == np.float32 else (1e-2, 1e-9)
    tol = 4096 * np.finfo(dtype).eps
    assert np.sin(big) ** 2 > 16 * tol and np.sin(small) ** 2 < tol / 16      # (well on either side of the rule)
    rows = []
    for axis in (2, 1):                            # n = e_up, n = e_right, turned towards e_look
        for t in (0.0, small, -small, big, -big):
            n = np.cos(t) * fr[axis] + np.sin(t) * fr[3]
            rows.append((abs(t), np.concatenate([f["s0"][p][:4], (n - fr[0]) / np.sqrt(2.0)])))
    s0 = np.array([r[1] for r in rows])
    se = np.repeat(f["state_end"][p][None].astype(np.float64), len(rows), axis=0)
    h = rt.eval_polarization(metric, objs, em, pol, inclined(), s0, se, dtype=dtype)
    for (t, _), v, q, u in zip(rows, h["valid"], h["q"], h["u"]):
        if t == big:
            assert v and np.isfinite(q) and np.isfinite(u) and abs(np.hypot(q, u) - FIELD["deg0"]) <= 1e-3, (t, v, q, u)
        else:
            assert not v and np.isnan(q) and np.isnan(u), (t, v, q, u)


# ---- the device entries: streams, a replayed graph, rtgr_trim, the stage alone, every refusal in every entry family -----------------------
PLANES = ("rgb", "g", "q", "u", "aux", "state_end", "hit32")


def _hip_runtime():
    """the HIP runtime already loaded in this process (torch's bundled libamdhip64)"""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return C.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")


class DevFrame:
    """the device buffers of one polarized frame of n pixels, every one filled with `fill` (so an untouched buffer shows)"""

    def __init__(self, n, dtype, fill=7.0):
        import torch
        t = torch.float64 if dtype == np.float64 else torch.float32
        for k, shape in (("rgb", (3, n)), ("g", (n,)), ("q", (n,)), ("u", (n,)), ("aux", (n,)), ("state_end", (n, 8)), ("state0", (n, 8))):
            setattr(self, k, torch.full(shape, fill, dtype=t, device="cuda"))
        self.hit32 = torch.full((n,), int(fill), dtype=torch.int32, device="cuda")
        self.out = abi.rtgr_ray_outputs(state_end=self.state_end.data_ptr(), hit32=self.hit32.data_ptr())
        self.fill = fill
        torch.cuda.synchronize()

    def bytes(self, keys=PLANES):
        return {k: getattr(self, k).cpu().numpy().tobytes() for k in keys}

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((getattr(self, k) == self.fill).all()) for k in PLANES + ("state0",))


def trace_dev(lib, suf, sc, opt, ob, ni, nj, em, pol, F, stream, ctr=None, drop=()):
    ptr = lambda k: None if k in drop else getattr(F, k).data_ptr()
    ref = lambda x: None if x is None else C.byref(x)
    return getattr(lib, "rtgr_trace_polarized_device_" + suf)(None, ref(sc), C.byref(opt), ref(ob), ni, nj, None, ref(em), ref(pol), ptr("rgb"), C.byref(F.out),
                                                              ptr("g"), ptr("q"), ptr("u"), ptr("aux"), ref(ctr), stream)


def stage_dev(lib, suf, sc, ob, ni, nj, em, pol, src, F, stream, drop=()):
    """rtgr_polarization_device_*: hit32, state0, state_end of `src` into q, u, aux of F"""
    ref = lambda x: None if x is None else C.byref(x)
    ptr = lambda o, k: None if k in drop else getattr(o, k).data_ptr()
    return getattr(lib, "rtgr_polarization_device_" + suf)(None, ref(sc), ref(em), ref(pol), ref(ob), ni, nj, ptr(src, "hit32"), ptr(src, "state0"),
                                                           ptr(src, "state_end"), ptr(F, "q"), ptr(F, "u"), ptr(F, "aux"), stream)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_frame_rule_streams_graph_trim_and_the_stage_alone(lib, dtype):
    """rtgr_trace_polarized_device_* gives the bytes of the host entry (whose planes test_frame_rule_bit_for_bit holds against the hook and
    against rtgr_trace_observer_*) on the default stream, on a side stream, in five-row batches, replayed from a straight-line graph
    captured on the side stream, and in a fresh call after rtgr_trim; during capture it refuses counters and a frame whose scratch would
    have to grow, in its own name.  rtgr_polarization_device_*, fed hit32, the canvas states and state_end of that frame, writes the
    same q, u, aux — eager on both streams and replayed from a graph."""
    import torch
    suf = "f64" if dtype == np.float64 else "f32"
    kind, a = "ks_true", 0.998
    ni, nj = SIZES[1]
    n = ni * nj
    metric, objs = disk_scene(kind, a)
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults(dtype)
    em, pol, ob = rt.DiskEmission(3, T_FRAME), rt.Polarization(**FIELD), inclined()
    host = pframe(kind, a, "kepler", +1, FIELD, SIZES[1], dtype)
    want = {k: host[k].tobytes() for k in ("rgb", "g", "q", "u", "aux", "state_end")}
    want["hit32"] = host["hit"].astype(np.int32).tobytes()
    assert (host["hit"] == 3).sum() >= 20
    side = torch.cuda.Stream()
    hip = _hip_runtime()
    F = {k: DevFrame(n, dtype) for k in ("default", "side", "rows5", "graph", "fresh", "wide")}
    wide = DevFrame(4 * n, dtype)
    # eager: the default stream (with counters: the one synchronisation), the side stream, five rows per batch
    ctr = abi.rtgr_counters()
    abi.check(lib, trace_dev(lib, suf, sc, opt, ob, ni, nj, em, pol, F["default"], None, ctr=ctr))
    assert ctr.as_dict() == host["counters"]
    abi.check(lib, trace_dev(lib, suf, sc, opt, ob, ni, nj, em, pol, F["side"], side.cuda_stream))      # (the warm-up of the capture below)
    abi.check(lib, trace_dev(lib, suf, sc, opt, inclined(max_batch_rays=5 * ni), ni, nj, em, pol, F["rows5"], side.cuda_stream))
    torch.cuda.synchronize()
    for k in ("default", "side", "rows5"):
        assert F[k].bytes() == want, k
    # the stage alone, eager on both streams, from the traced frame's own planes and the canvas states
    src = F["default"]
    abi.check(lib, getattr(lib, "rtgr_make_observer_canvas_device_" + suf)(None, C.byref(sc), C.byref(ob), ni, nj, 0, nj, src.state0.data_ptr(), None))
    torch.cuda.synchronize()
    assert src.state0.cpu().numpy().tobytes() == host["s0"].tobytes()
    S = {k: DevFrame(n, dtype) for k in ("default", "side", "graph")}
    abi.check(lib, stage_dev(lib, suf, sc, ob, ni, nj, em, pol, src, S["default"], None))
    abi.check(lib, stage_dev(lib, suf, sc, ob, ni, nj, em, pol, src, S["side"], side.cuda_stream))
    torch.cuda.synchronize()
    three = {k: want[k] for k in ("q", "u", "aux")}
    assert S["default"].bytes(("q", "u", "aux")) == three and S["side"].bytes(("q", "u", "aux")) == three
    # captured on the side stream: a linear chain of kernels; what cannot be captured is refused and leaves the capture alive
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc_big = trace_dev(lib, suf, sc, opt, ob, 4 * ni, nj, em, pol, wide, side.cuda_stream)
    msg_big = lib.rtgr_last_error()
    rc_ctr = trace_dev(lib, suf, sc, opt, ob, ni, nj, em, pol, F["wide"], side.cuda_stream, ctr=abi.rtgr_counters())
    msg_ctr = lib.rtgr_last_error()
    rc = trace_dev(lib, suf, sc, opt, ob, ni, nj, em, pol, F["graph"], side.cuda_stream)
    rc_stage = stage_dev(lib, suf, sc, ob, ni, nj, em, pol, src, S["graph"], side.cuda_stream)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert rc == 0 and rc_stage == 0, lib.rtgr_last_error()
    assert rc_big == abi.ERR_BAD_ARG and b"captured" in msg_big and b"rtgr_trace_polarized" in msg_big, msg_big
    assert rc_ctr == abi.ERR_BAD_ARG and b"ctr" in msg_ctr and b"rtgr_trace_polarized" in msg_ctr, msg_ctr
    assert F["graph"].untouched() and F["wide"].untouched() and wide.untouched()      # (captured, not run; refused, not written)
    assert graph.value and hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert F["graph"].bytes() == want and S["graph"].bytes(("q", "u", "aux")) == three
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    # after rtgr_trim (workspace, scratch and staging released): a fresh call builds them again and gives the same bytes
    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, trace_dev(lib, suf, sc, opt, ob, ni, nj, em, pol, F["fresh"], side.cuda_stream))
    torch.cuda.synchronize()
    assert F["fresh"].bytes() == want
    after = rt.trace_polarized(metric, objs, ob, ni, nj, em, pol, dtype=dtype, details=True)
    assert all(after[k].tobytes() == host[k].tobytes() for k in ("rgb", "g", "q", "u", "aux", "state_end"))


def _copy(x):
    return type(x).from_buffer_copy(x)


def _refusals():
    """(name, what to change, words of the message, the entry families it applies to): every refusal of include/rtgr.h "polarized disk
    images".  Families: host = rtgr_trace_polarized_*, dev = rtgr_trace_polarized_device_*, stage = rtgr_polarization_device_*,
    hook = rtgr_eval_polarization_*, forms = rtgr_eval_walker_penrose_*."""
    rec = ("host", "dev", "stage", "hook")
    every = rec + ("forms",)
    nan, inf = float("nan"), float("inf")

    def pol(**kw):
        def change(c):
            for k, v in kw.items():
                if k == "field":
                    c["pol"].field[:] = v
                elif k == "reserved":
                    c["pol"].reserved[v] = 1.0
                else:
                    setattr(c["pol"], k, v)
        return change

    def metric(m):
        def change(c):
            c["sc"].metric = m
        return change

    def null(k):
        def change(c):
            c[k] = None
        return change

    def drop(k):
        def change(c):
            c["drop"] = (k,)
        return change

    def emit_object(c):
        c["em"].object = 1      # the plane of the scene: not a disk

    def obs_flags(c):
        c["ob"].flags = 1

    def obs_kind(c):
        c["ob"].kind = 9

    def obs_fov(c):
        c["ob"].fov_x = 0.0

    def redshift(c):
        c["redshift"] = True

    return [
        ("pol is NULL", null("pol"), b"pol", rec), ("emit is NULL", null("em"), b"emit", rec), ("obs is NULL", null("ob"), b"obs", rec),
        ("scene is NULL", null("sc"), b"scene", every),
        ("q is NULL", drop("q"), b"q or u", ("host", "dev", "stage")), ("u is NULL", drop("u"), b"q or u", ("host", "dev", "stage")),
        ("rgb is NULL", drop("rgb"), b"rgb", ("host", "dev")),
        ("hit32 is NULL", drop("hit32"), b"hit32", ("stage",)), ("state0 is NULL", drop("state0"), b"state0", ("stage",)),
        ("state_end is NULL", drop("state_end"), b"state_end", ("stage",)),
        ("s0 is NULL", drop("state0"), b"NULL", ("hook", "forms")), ("s_end is NULL", drop("state_end"), b"NULL", ("hook",)),
        ("kappa is NULL", drop("kappa"), b"NULL", ("forms",)),
        ("unknown kind", pol(kind=7), b"unknown rtgr_polarization.kind", rec), ("flags", pol(flags=2), b"flags must be 0", rec),
        ("reserved[0]", pol(reserved=0), b"reserved must be 0", rec), ("reserved[1]", pol(reserved=1), b"reserved must be 0", rec),
        ("deg0 NaN", pol(deg0=nan), b"finite", rec), ("deg0 inf", pol(deg0=inf), b"finite", rec), ("deg1 NaN", pol(deg1=nan), b"finite", rec),
        ("deg1 inf", pol(deg1=-inf), b"finite", rec), ("field NaN", pol(kind=1, field=(0.0, nan, 1.0)), b"field must be finite", rec),
        ("field inf", pol(kind=1, field=(inf, 0.0, 1.0)), b"field must be finite", rec),
        ("deg0 < 0", pol(deg0=-0.1), b"deg0 must be >= 0", rec), ("deg1 = -1", pol(deg1=-1.0), b"deg1 of RTGR_POL_SCATTER must be > -1", rec),
        ("deg1 < -1", pol(deg1=-2.0), b"deg1 of RTGR_POL_SCATTER must be > -1", rec),
        ("FIELD, zero field", pol(kind=1), b"must not be zero", rec), ("SCATTER, a field", pol(field=(0.0, 1.0, 0.0)), b"RTGR_POL_SCATTER must be 0", rec),
        ("RTGR_KS_REF", metric(abi.KS_REF), b"RTGR_KS_TRUE or RTGR_MINKOWSKI", every),
        ("RTGR_KS_REF | GENERIC", metric(abi.KS_REF | abi.METRIC_GENERIC), b"RTGR_KS_TRUE or RTGR_MINKOWSKI", every),
        ("RTGR_GRID (3-D and 4-D grids)", metric(abi.GRID), b"a grid or a user metric", every),
        ("RTGR_GRID | GENERIC", metric(abi.GRID | abi.METRIC_GENERIC), b"a grid or a user metric", every),
        ("RTGR_USER", metric(abi.USER), b"a grid or a user metric", every),
        # what disk emission and the observer camera refuse, one of each kind
        ("the emitter is no disk", emit_object, b"", rec), ("observer flags", obs_flags, b"", rec), ("observer kind", obs_kind, b"", rec),
        ("observer fov", obs_fov, b"", rec), ("redshift asked of an observer trace", redshift, b"redshift", ("host", "dev")),
    ]


@pytest.mark.gpu
def test_every_refusal_in_every_entry_family_leaves_the_outputs_untouched(lib):
    """Each refusal of the header, through each of the five entry families it applies to at the C level (Float64 and Float32): RTGR_ERR_BAD_ARG,
    its message, and every output buffer — host or device — still holds what it held.  The same callers accept the unchanged arguments,
    and RTGR_MINKOWSKI | GENERIC and RTGR_KS_TRUE | GENERIC, so each refusal is the change's."""
    ni = nj = 8
    n = ni * nj
    metric, objs = disk_scene()
    base = dict(sc=rt.make_scene(metric, objs), em=rt.DiskEmission(3, T_FRAME), pol=rt.Polarization(kind="scatter", deg0=0.1, deg1=0.5), ob=inclined(),
                drop=(), redshift=False)
    for dtype, suf in ((np.float64, "f64"), (np.float32, "f32")):
        opt = rt.solver_defaults(dtype)
        D, Src = DevFrame(n, dtype), DevFrame(n, dtype, fill=0.0)
        H = {k: np.full(shape, 7.0, dtype) for k, shape in (("rgb", (3, n)), ("g", n), ("q", n), ("u", n), ("aux", n), ("kappa", (n, 2)), ("f_em", (n, 4)),
                                                         ("delta", n))}
        H["valid"] = np.full(n, 7, np.int32)
        spare = np.zeros(n, dtype)
        s_in, f_in = np.zeros((n, 8), dtype), np.zeros((n, 4), dtype)
        ref = lambda x: None if x is None else C.byref(x)

        def call(family, c):
            hp = lambda k: None if k in c["drop"] else H[k].ctypes.data
            outs = abi.rtgr_ray_outputs(redshift=spare.ctypes.data) if c["redshift"] else None
            if family == "host":
                return getattr(lib, "rtgr_trace_polarized_" + suf)(None, ref(c["sc"]), C.byref(opt), ref(c["ob"]), ni, nj, None, ref(c["em"]), ref(c["pol"]),
                                                                   hp("rgb"), ref(outs), hp("g"), hp("q"), hp("u"), hp("aux"), None)
            if family == "dev":
                if c["redshift"]:
                    D.out.redshift = D.aux.data_ptr()
                try:
                    return trace_dev(lib, suf, c["sc"], opt, c["ob"], ni, nj, c["em"], c["pol"], D, None, drop=c["drop"])
                finally:
                    D.out.redshift = None
            if family == "stage":
                return stage_dev(lib, suf, c["sc"], c["ob"], ni, nj, c["em"], c["pol"], Src, D, None, drop=c["drop"])
            sp = lambda k, arr: None if k in c["drop"] else arr.ctypes.data
            if family == "hook":
                return getattr(lib, "rtgr_eval_polarization_" + suf)(None, ref(c["sc"]), ref(c["em"]), ref(c["pol"]), ref(c["ob"]), sp("state0", s_in),
                                                                     sp("state_end", s_in), n, hp("kappa"), hp("f_em"), hp("aux"), hp("delta"), hp("q"),
                                                                     hp("u"), H["valid"].ctypes.data)
            return getattr(lib, "rtgr_eval_walker_penrose_" + suf)(None, ref(c["sc"]), sp("state0", s_in), f_in.ctypes.data, n, hp("kappa"))

        fresh = lambda: {k: (_copy(v) if isinstance(v, C.Structure) else v) for k, v in base.items()}
        count = 0
        for name, change, words, families in _refusals():
            for family in families:
                c = fresh()
                change(c)
                rc = call(family, c)
                msg = lib.rtgr_last_error()
                assert rc == abi.ERR_BAD_ARG and msg and words in msg, (suf, name, family, rc, msg)
                assert all((v == 7).all() for v in H.values()) and D.untouched(), (suf, name, family)
                count += 1
        assert count >= 130
        # the same callers with nothing changed, and with the generic flag on the two metrics that have the constants: accepted
        for m in (None, abi.KS_TRUE | abi.METRIC_GENERIC, abi.MINKOWSKI | abi.METRIC_GENERIC):
            for family in ("host", "dev", "stage", "hook", "forms"):
                c = fresh()
                if m is not None:
                    c["sc"].metric = m
                assert call(family, c) == 0, (suf, m, family, lib.rtgr_last_error())
