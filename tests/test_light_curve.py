"""Hot-spot light curves (include/rtgr.h "hot-spot light curves"): one traced frame of an emitting disk reduced on the
device over many observer times.  The judge is a numpy restatement of the header's contract — the expanded form of the distance, summed
with math.fsum — fed the planes a trace delivered; the rate Omega_s is held against rtgr_eval_disk_emission_* to the bit.

CPU tests: the symbols, the struct layout (ctypes, a compiled C caller, the Julia stub), the error without a device, the restatement
itself.  GPU tests: the hook, the reduction on real frames and on synthetic planes around the kernel's tile sizes, flat-space physics,
determinism, the untouched trace, the refusals, capture / replay / trim."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from scenes import rt

abi = rt._abi
LC_EXPORTS = ("rtgr_light_curve_device_f64", "rtgr_light_curve_device_f32", "rtgr_trace_light_curve_device_f64", "rtgr_trace_light_curve_device_f32",
              "rtgr_trace_light_curve_f64", "rtgr_trace_light_curve_f32", "rtgr_eval_hot_spot_f64", "rtgr_eval_hot_spot_f32")
SIZES = ((48, 32), (37, 19))
T_FRAME = 30000.0
OUT_KEYS = ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject", "hit32")
# the kernel's tile sizes, as csrc/rtgr_lightcurve.hpp names them (test_the_tile_sizes_are_the_headers holds them against the header)
LC_WAVE, LC_RANGE, LC_LANE_SAMPLES, LC_TILE, LC_MAX_RANGES, LC_PASS = 64, 256, 4, 256, 1024, 1024


# ---- the header's contract in numpy (float64) -----------------------------------------------------------------------------------------
def pixel_ab(ni, nj):
    p = np.arange(ni * nj)
    return 2 * ((p % ni) + 0.5) / ni - 1, 2 * ((p // ni) + 0.5) / nj - 1


def np_weight(ob, ni, nj):
    a, b = pixel_ab(ni, nj)
    if ob is None:
        return np.ones(ni * nj), a, b
    if ob.projection == abi.PROJ_PERSPECTIVE:
        tx, ty = math.tan(0.5 * ob.fov_x), math.tan(0.5 * ob.fov_y)
        return tx * ty * (2 / ni) * (2 / nj) / (1 + a * a * tx * tx + b * b * ty * ty) ** 1.5, a, b
    return np.cos(b * ob.fov_y / 2) * (ob.fov_x / ni) * (ob.fov_y / nj), a, b


def tau_of(spot):
    return spot.t_start + np.arange(int(spot.nt), dtype=np.float64) * spot.dt


def np_active(hit32, se, g, obj, spot):
    se, g = np.asarray(se, np.float64), np.asarray(g, np.float64)
    rho = np.hypot(se[:, 1], se[:, 2])
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((hit32 == obj) & np.isfinite(g) & (g > 0) & np.isfinite(se[:, 0]) & (np.abs(rho - spot.rho_s) < spot.cut * spot.sigma))


def np_d2_expanded(x, y, t, om, spot, tau):
    """d² [n_pixels, nt]: the contract's form, rho_p² + rho_s² - 2 rho_p rho_s (cos gamma cos beta + sin gamma sin beta)"""
    rho, gamma = np.hypot(x, y), np.arctan2(y, x) - spot.phi0 - om * t
    beta = om * tau
    return (rho * rho + spot.rho_s ** 2)[:, None] - 2 * spot.rho_s * rho[:, None] * (np.cos(gamma)[:, None] * np.cos(beta)[None, :] +
                                                                                   np.sin(gamma)[:, None] * np.sin(beta)[None, :])


def np_d2_direct(x, y, t, om, spot, tau):
    ang = spot.phi0 + om * (t[:, None] + tau[None, :])
    return (x[:, None] - spot.rho_s * np.cos(ang)) ** 2 + (y[:, None] - spot.rho_s * np.sin(ang)) ** 2


def np_emissivity(d2, spot):
    e = np.maximum(np.exp(-d2 / (2 * spot.sigma ** 2)) - math.exp(-spot.cut ** 2 / 2), 0.0)
    return spot.amp * np.where(d2 < (spot.cut * spot.sigma) ** 2, e, 0.0)


def np_light_curve(hit32, se, g, obj, om, spot, ob, ni, nj):
    """-> (lc [nt, 3] by math.fsum, the number of active pixels)"""
    se, g = np.asarray(se, np.float64), np.asarray(g, np.float64)
    w, a, b = np_weight(ob, ni, nj)
    idx = np_active(hit32, se, g, obj, spot)
    nt = int(spot.nt)
    if not math.isfinite(om):
        return np.full((nt, 3), np.nan), len(idx)
    j = np_emissivity(np_d2_expanded(se[idx, 1], se[idx, 2], se[idx, 0], float(om), spot, tau_of(spot)), spot)
    terms = (w[idx] * g[idx] ** spot.g_power)[:, None] * j
    lc = np.zeros((nt, 3))
    for k in range(nt):
        lc[k] = (math.fsum(terms[:, k]), math.fsum(terms[:, k] * a[idx]), math.fsum(terms[:, k] * b[idx]))
    return lc, len(idx)


def worst(got, want):
    """max over k and the three columns of |got - want| / F_k.  Where the restatement sees no light at all (F_k = 0: no active pixel within
    the support at that observer time) "within 1e-9 F_k" means exactly none: asserted here."""
    F = want[:, 0]
    lit = F > 0
    assert lit.any() and (F >= 0).all()
    assert (got[~lit] == 0).all() and (want[~lit] == 0).all()
    return float((np.abs(got - want)[lit] / F[lit, None]).max())


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(LC_EXPORTS) <= set(abi.EXPORTS) and len(LC_EXPORTS) == 8
    lib = abi.load()
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    for s in LC_EXPORTS:
        assert hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    for words in ("A spot that shears".lower(), "a frame that shows the spot", "spectra of the spot", "non-stationary", "THE CONTRACT is the expanded form",
                  "#define RTGR_HOT_SPOT_MAX_SAMPLES (1ull << 20)"):
        assert words in hdr, words


def test_the_tile_sizes_are_the_headers():
    # the sizes are the one reduction's (rtgr_reduce.hpp), the record length the light curve's own
    txt = open(os.path.join(ROOT, "raytracegr.jl_amd", "csrc", "rtgr_reduce.hpp")).read()
    for name, val in (("RED_WAVE", LC_WAVE), ("RED_RANGE", LC_RANGE), ("RED_LANE_ITEMS", LC_LANE_SAMPLES), ("RED_MAX_RANGES", LC_MAX_RANGES), ("RED_PASS", LC_PASS)):
        assert re.search(r"constexpr \w+ " + name + r" = " + str(val) + r";", txt), name
    assert "RED_TILE = RED_WAVE * RED_LANE_ITEMS" in txt and LC_TILE == LC_WAVE * LC_LANE_SAMPLES
    lc = open(os.path.join(ROOT, "raytracegr.jl_amd", "csrc", "rtgr_lightcurve.hpp")).read()
    assert re.search(r"constexpr \w+ LC_REC = 6;", lc) and not re.search(r"constexpr \w+ (LC|RED)_(WAVE|RANGE|LANE_\w+|TILE|MAX_RANGES|PASS) =", lc)


def test_struct_layout_in_ctypes_a_compiled_c_caller_and_the_julia_stub(tmp_path):
    s = abi.rtgr_hot_spot
    want = dict(rho_s=0, phi0=8, sigma=16, cut=24, amp=32, g_power=40, t_start=48, dt=56, nt=64, flags=72, pad=76)
    assert C.sizeof(s) == 80 and {k: getattr(s, k).offset for k in want} == want and [n for n, _ in s._fields_] == list(want)
    exe = str(tmp_path / "lightcurve_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "lightcurve_layout.c"), "-o", exe, "-ldl"])
    out = subprocess.check_output([exe], text=True).split()
    assert dict(zip(out[0::2], map(int, out[1::2]))) == dict(want, hot_spot=80)
    assert subprocess.run([exe, abi.LIB_PATH]).returncode == 0                     # (2: a symbol does not resolve)
    sp = rt.HotSpot(4.0, 0.5, t_start=-3.0, dt=0.25, nt=512, phi0=0.3, cut=3.0, amp=2.0, g_power=3.0)
    assert (sp.rho_s, sp.phi0, sp.sigma, sp.cut, sp.amp, sp.g_power, sp.t_start, sp.dt, sp.nt, sp.flags, sp.pad) == (4.0, 0.3, 0.5, 3.0, 2.0, 3.0, -3.0, 0.25, 512, 0, 0)
    # the Julia stub: the struct in the header's order, the fieldoffset table, the three functions, the eight-argument hook asked first
    from test_julia_stub import HDR, JL, c_kind, c_prototypes, ccalls, jl_kind, strip_julia
    text = open(JL).read()
    code = strip_julia(text)
    body = re.search(r"struct RtgrHotSpot[ \t]*\n((?:.|\n)*?)\nend", code).group(1)
    assert re.findall(r"([A-Za-z_0-9]+)::", body) == list(want)
    hdr = re.sub(r"/\*(?:.|\n)*?\*/", " ", open(HDR).read())
    cbody = re.search(r"typedef struct[^{]*\{((?:[^{}]|\{[^{}]*\})*)\}\s*rtgr_hot_spot\s*;", hdr).group(1)
    assert [d.strip().split()[-1] for d in cbody.split(";") if d.strip()] == list(want)
    m = re.search(r"^#\s+RtgrHotSpot\s+(\d+)\s+(.*)$", text, re.M)
    assert m and int(m.group(1)) == 80 and [(n, int(o)) for n, o in re.findall(r"([a-z_A-Z0-9]+) (\d+)", m.group(2))] == list(want.items())
    protos = c_prototypes()
    bound = {c[0]: c for c in ccalls() if "light_curve" in c[0] or "hot_spot" in c[0]}
    assert set(bound) == {"rtgr_trace_light_curve_f64", "rtgr_trace_light_curve_f32", "rtgr_eval_hot_spot_f64", "rtgr_eval_hot_spot_f32"}
    for sym, (_, ret, types, args) in bound.items():
        cret, cparams = protos[sym]
        assert ret == "Cint" and cret == "int" and len(types) == len(args) == len(cparams) == (14 if "trace" in sym else 9)
        assert [jl_kind(t) for t in types] == [c_kind(t) for t in cparams]
        assert "Ptr{RtgrHotSpot}" in [t.strip() for t in types]
    for word in ("function HotSpot(", "function light_curve(", "function eval_hot_spot("):
        assert word in text, word
    fn = code[code.index("function light_curve("):]
    fn = fn[:fn.index("\nend\n")]
    assert 0 < fn.index("observer_frame(scene, obs") < fn.index("eval_hot_spot(scene, emit, sp") < fn.index("ccall(")


def test_no_result_without_a_device():
    """Without a HIP device every new entry FAILS with RTGR_ERR_NO_DEVICE, says so, and leaves the caller's arrays alone."""
    import torch
    if torch.cuda.is_available():
        return
    lib, nd = abi.load(), abi.ERR_NO_DEVICE
    metric, objs = rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 3.0, 6.0)]
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ob, em, sp = rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 1.0), rt.DiskEmission(1, 6000.0), rt.HotSpot(4.0, 0.5, nt=3)
    for dtype, suf in ((np.float64, "f64"), (np.float32, "f32")):
        rgb, g, lc, se, hit = np.full((3, 4), -7.0, dtype), np.full(4, -7.0, dtype), np.full((3, 3), -7.0), np.zeros((4, 8), dtype), np.zeros(4, np.uint32)
        rc = getattr(lib, "rtgr_trace_light_curve_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(ob), 2, 2, None, C.byref(em), C.byref(sp), rgb.ctypes.data,
                                                           None, g.ctypes.data, lc.ctypes.data, None)
        assert rc == nd and b"no CPU fallback" in lib.rtgr_last_error()
        assert getattr(lib, "rtgr_trace_light_curve_device_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(ob), 2, 2, None, C.byref(em), C.byref(sp),
                                                                    rgb.ctypes.data, None, g.ctypes.data, lc.ctypes.data, None, None) == nd
        assert getattr(lib, "rtgr_light_curve_device_" + suf)(None, C.byref(sc), C.byref(em), C.byref(sp), C.byref(ob), 2, 2, hit.ctypes.data, se.ctypes.data,
                                                              g.ctypes.data, lc.ctypes.data, None) == nd
        om, valid, j, pts = np.full(1, -7.0, dtype), C.c_int(-7), np.full(2, -7.0), np.zeros((2, 3), dtype)
        assert getattr(lib, "rtgr_eval_hot_spot_" + suf)(None, C.byref(sc), C.byref(em), C.byref(sp), pts.ctypes.data, 2, om.ctypes.data, C.byref(valid),
                                                         j.ctypes.data) == nd
        assert (rgb == -7.0).all() and (g == -7.0).all() and (lc == -7.0).all() and om[0] == -7.0 and valid.value == -7 and (j == -7.0).all()
    for call in (lambda: rt.light_curve(metric, objs, ob, 2, 2, em, sp), lambda: rt.eval_hot_spot(metric, objs, em, sp)):
        with pytest.raises(abi.RtgrError, match="no CPU fallback"):
            call()


def test_the_numpy_restatement_has_the_orbital_period_and_its_expanded_form_is_the_direct_one():
    """(CPU: the judge itself.)  The expanded form against the direct (x - c_x)² + (y - c_y)² to 1e-12 sigma², on the pairs the reduction can
    ever evaluate an exp for (d within the support) and their surroundings (d <= 2 cut sigma).  The bound is the cancellation error
    eps rho² with room, so it is asked where eps rho² has that room against 1e-12 sigma²: rho <= 20 at sigma = 2, rho <= 12 at sigma = 0.5
    (the GPU tests' case), rho <= 4 at sigma = 0.2.  At the far corner rho = 20, sigma = 0.2 eps rho² = 8.9e-14 already exceeds
    1e-12 sigma² = 4e-14 — no implementation in double meets it there; that figure is printed, not asserted.  F(tau + 2 pi / Omega) = F(tau)."""
    rng = np.random.default_rng(11)
    n = 6000
    psi, t = rng.uniform(-math.pi, math.pi, n), rng.uniform(-60.0, 0.0, n)

    def d2_error(rho_max, rho_s, sigma, om):
        rho = rng.uniform(max(0.05, rho_s - 8 * sigma), min(rho_max, rho_s + 8 * sigma), n)
        x, y = rho * np.cos(psi), rho * np.sin(psi)
        sp = rt.HotSpot(rho_s, sigma, t_start=-7.0, dt=0.37, nt=41, phi0=0.9)
        direct = np_d2_direct(x, y, t, om, sp, tau_of(sp))
        near = direct <= (2 * sp.cut * sigma) ** 2
        assert near.sum() > 1000
        return float(np.abs(np_d2_expanded(x, y, t, om, sp, tau_of(sp)) - direct)[near].max() / sigma ** 2)

    worst_d2 = max(d2_error(20.0, 15.0, 2.0, 0.035), d2_error(12.0, 9.0, 0.5, -0.011), d2_error(12.0, 3.0, 0.5, 0.1), d2_error(4.0, 3.0, 0.2, 0.12))
    print(f"expanded against direct d²: {worst_d2:.2e} sigma²; at the corner rho = 20, sigma = 0.2: {d2_error(20.0, 19.0, 0.2, 0.02):.2e} sigma²")
    assert worst_d2 <= 1e-12
    # the period: a ring of pixels, g = 1, w = 1
    om, m = 0.2, 600
    sp = rt.HotSpot(5.0, 0.5, t_start=1.0, dt=0.9, nt=24, phi0=-0.4)
    rr, pp = rng.uniform(3.2, 6.8, m), rng.uniform(-math.pi, math.pi, m)
    se = np.zeros((m, 8))
    se[:, 0], se[:, 1], se[:, 2] = rng.uniform(-9.0, 0.0, m), rr * np.cos(pp), rr * np.sin(pp)
    hit, g = np.ones(m, np.uint32), np.ones(m)
    a, _ = np_light_curve(hit, se, g, 1, om, sp, None, m, 1)
    later = rt.HotSpot(5.0, 0.5, t_start=1.0 + 2 * math.pi / om, dt=0.9, nt=24, phi0=-0.4)
    b, active = np_light_curve(hit, se, g, 1, om, later, None, m, 1)
    assert active == m and (a[:, 0] > 0).all() and a[:, 0].max() > 1.5 * a[:, 0].min()        # (it does vary within a period)
    assert worst(b, a) <= 1e-12
    half = rt.HotSpot(5.0, 0.5, t_start=1.0 + math.pi / om, dt=0.9, nt=24, phi0=-0.4)
    assert worst(np_light_curve(hit, se, g, 1, om, half, None, m, 1)[0], a) > 0.1          # (and half a period is not one)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def kerr_disk_scene():
    """KerrSchild(1, 0.998) with config 5's disk, inside a sky large enough to hold an observer at rho = 12 (tests/test_observer.py)"""
    return rt.KerrSchild(1, 0.998), [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -20.0), rt.Plane(-60.0), rt.Disk(0.05, 2.0, 4.0)]


def orbiting(projection="perspective", max_batch_rays=0):
    """on the prograde circular orbit at rho = 12, looking at the hole through a narrow window (the disk is seen edge-on: z = 0), so that
    the direct image and the lensed far side cover some tens of pixels even at 37 x 19"""
    return rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 0.8, 0.25, kind="circular", orbit=+1, projection=projection,
                       max_batch_rays=max_batch_rays)


SPOT = dict(rho_s=3.0, sigma=0.5, cut=4.0, phi0=0.7, amp=1.5, g_power=4.0, t_start=-5.0, dt=0.6)
_FRAMES = {}


def frame(proj, size, dtype=np.float64):
    """the emitted frame of the orbiting observer with every per-ray output, by rt.trace_observer: once per (projection, size, dtype), never
    written to"""
    key = (proj, size, np.dtype(dtype).name)
    if key not in _FRAMES:
        metric, objs = kerr_disk_scene()
        res = rt.trace_observer(metric, objs, orbiting(proj), size[0], size[1], emission=rt.DiskEmission(3, T_FRAME), dtype=dtype, details=True)
        res["hit32"] = res["hit"].astype(np.uint32)
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _FRAMES[key] = res
    return _FRAMES[key]


def lc_device(lib, metric, objs, em, spot, ob, ni, nj, hit32, se, g, dtype=np.float64, stream=None, fill=-7.0):
    """rtgr_light_curve_device_f64 / _f32 over planes uploaded as torch tensors -> (rc, lc [nt, 3])"""
    import torch
    sc = rt.make_scene(metric, objs)
    td = torch.float64 if dtype == np.float64 else torch.float32
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        d_hit = torch.from_numpy(np.ascontiguousarray(hit32, np.uint32).view(np.int32).copy()).cuda()
        d_se = torch.from_numpy(np.ascontiguousarray(se, dtype).copy()).cuda()
        d_g = torch.from_numpy(np.ascontiguousarray(g, dtype).copy()).cuda()
        d_lc = torch.full((int(spot.nt), 3), fill, dtype=torch.float64, device="cuda")
        assert d_se.dtype == td and d_se.shape == (ni * nj, 8) and d_hit.shape == (ni * nj,) and d_g.shape == (ni * nj,)
        torch.cuda.synchronize()
        fn = lib.rtgr_light_curve_device_f64 if dtype == np.float64 else lib.rtgr_light_curve_device_f32
        rc = fn(None, C.byref(sc), C.byref(em), C.byref(spot), C.byref(ob) if ob is not None else None, ni, nj, d_hit.data_ptr(), d_se.data_ptr(),
                d_g.data_ptr(), d_lc.data_ptr(), stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    return rc, d_lc.cpu().numpy()


def disk_omega(metric, objs, em, rho_s, dtype=np.float64):
    """rtgr_eval_disk_emission_*'s omega at an end state with (x, y, z) = (rho_s, 0, 0)"""
    s = np.zeros((1, 8), dtype)
    s[0, 1], s[0, 4] = rho_s, 1.0
    s0 = np.array([[0, 30.0, 0, 0, 1, -1, 0, 0]], dtype)       # (a camera far out on the x axis: its static observer is timelike)
    return rt.eval_disk_emission(metric, objs, em, s0, s, dtype=dtype)["omega"][0]


@pytest.mark.gpu
def test_hook_rate_to_the_bit_and_emissivity_against_numpy(lib):
    rng = np.random.default_rng(5)
    objs = [rt.Disk(0.05, 2.0, 9.0)]
    checked = 0
    for name, metric in (("ks_true08", rt.KerrSchild(1, 0.8)), ("ks_true0998", rt.KerrSchild(1, 0.998)), ("ks_true0", rt.KerrSchild(1, 0.0)),
                         ("ks_ref08", rt.KerrSchild(1, 0.8, textbook=False))):
        for orbit in (+1, -1):
            for dtype in (np.float64, np.float32):
                em = rt.DiskEmission(1, T_FRAME, orbit=orbit)
                sp = rt.HotSpot(7.5, 0.6, phi0=0.4, amp=2.5)
                m = 2000
                pts = np.column_stack([rng.uniform(-9, 9, m), rng.uniform(-9, 9, m), rng.uniform(-40, 10, m)]).astype(dtype)
                h = rt.eval_hot_spot(metric, objs, em, sp, pts, dtype=dtype)
                want = disk_omega(metric, objs, em, sp.rho_s, dtype)
                assert h["valid"] and math.isfinite(want) and h["omega_s"].dtype == dtype
                assert np.array([h["omega_s"]]).tobytes() == np.array([want]).tobytes(), (name, orbit, dtype, h["omega_s"], want)
                assert (want > 0) == (orbit > 0)
                p64 = pts.astype(np.float64)
                tau0 = np.zeros(1)
                j = np_emissivity(np_d2_expanded(p64[:, 0], p64[:, 1], p64[:, 2], float(want), sp, tau0), sp)[:, 0]
                err = np.abs(h["j"] - j) / (1e-12 * np.abs(j) + 1e-12 * sp.amp)
                assert (j > 0).sum() >= 20 and err.max() <= 1.0, (name, orbit, dtype, err.max())
                checked += 1
    assert checked == 16
    # RIGID: the rate is emit->orbit itself
    em = rt.DiskEmission(1, T_FRAME, orbit=0.03, emitter="rigid")
    assert rt.eval_hot_spot(rt.minkowski, objs, em, rt.HotSpot(5.0, 0.5))["omega_s"] == 0.03


@pytest.mark.gpu
def test_an_invalid_spot_gives_nan_and_ok(lib):
    """KerrSchild(1, 0): inside the photon orbit (r = 3) the circular orbit is not timelike — valid = 0, every entry of lc NaN, RTGR_OK; the
    Python mirror raises"""
    metric, objs = rt.KerrSchild(1, 0.0), [rt.Disk(0.05, 2.2, 6.0)]
    em, sp = rt.DiskEmission(1, T_FRAME), rt.HotSpot(2.5, 0.3, nt=70, dt=0.5)
    h = rt.eval_hot_spot(metric, objs, em, sp, [[2.5, 0, 0]])
    assert not h["valid"] and math.isnan(h["omega_s"]) and np.isnan(h["j"]).all()
    n = 300
    rng = np.random.default_rng(2)
    se = np.zeros((n, 8))
    se[:, 1], se[:, 2] = rng.uniform(2.2, 3.0, n), rng.uniform(-0.5, 0.5, n)
    rc, lc = lc_device(lib, metric, objs, em, sp, None, n, 1, np.ones(n, np.uint32), se, np.ones(n))
    assert rc == 0 and lc.shape == (70, 3) and np.isnan(lc).all()
    with pytest.raises(ValueError, match="HotSpot"):
        rt.light_curve(metric, [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -20.0), rt.Plane(-60.0)] + objs,
                       rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 0.8), 8, 6, rt.DiskEmission(3, T_FRAME), sp)


@pytest.mark.gpu
@pytest.mark.parametrize("proj,size", [("perspective", SIZES[0]), ("equirect", SIZES[1]), ("perspective", SIZES[1]), ("equirect", SIZES[0])])
def test_reduction_against_the_restatement_on_a_real_frame(lib, proj, size):
    """F, A, B within 1e-9 F_k of numpy's math.fsum over the same planes.  Terms are non-negative; the only amplified error is that of
    d², eps rho² / sigma² <~ 1e-11 at rho <= 12, sigma = 0.5; the rest is a few ulp per term."""
    metric, objs = kerr_disk_scene()
    em, ob = rt.DiskEmission(3, T_FRAME), orbiting(proj)
    ni, nj = size
    f = frame(proj, size)
    om = disk_omega(metric, objs, em, SPOT["rho_s"])
    for nt in (1, 2, 63, 64, 65, 257):
        sp = rt.HotSpot(nt=nt, **SPOT)
        want, active = np_light_curve(f["hit32"], f["state_end"], f["g"], 3, om, sp, ob, ni, nj)
        assert active >= 20, active
        rc, got = lc_device(lib, metric, objs, em, sp, ob, ni, nj, f["hit32"], f["state_end"], f["g"])
        assert rc == 0
        err = worst(got, want)
        print(f"{proj} {ni}x{nj} nt = {nt}: {active} active pixels, worst |lc - numpy| / F_k = {err:.2e}")
        assert err <= 1e-9, (proj, size, nt, err)
    # the traced entry gives the same bytes as the reduction over its own planes, and the Python mirror is that entry
    sp = rt.HotSpot(nt=65, **SPOT)
    res = rt.light_curve(metric, objs, ob, ni, nj, em, sp, details=True)
    rc, again = lc_device(lib, metric, objs, em, sp, ob, ni, nj, f["hit32"], f["state_end"], f["g"])
    assert rc == 0 and res["lc"].tobytes() == again.tobytes() and res["tau"].tobytes() == tau_of(sp).tobytes()
    assert res["g"].tobytes() == f["g"].tobytes() and res["rgb"].tobytes() == f["rgb"].tobytes()


def ring_planes(n, rho_s, reach, seed, t_span=(-6.0, 0.0)):
    """n pixels on a ring of radii within `reach` of rho_s, anywhere in azimuth, met at times in t_span; every one hits object 1 with g = 1"""
    rng = np.random.default_rng(seed)
    rr, pp = rng.uniform(rho_s - reach, rho_s + reach, n), rng.uniform(-math.pi, math.pi, n)
    se = rng.uniform(-1.0, 1.0, (n, 8))
    se[:, 0], se[:, 1], se[:, 2] = rng.uniform(t_span[0], t_span[1], n), rr * np.cos(pp), rr * np.sin(pp)
    return np.ones(n, np.uint32), se, np.ones(n)


RIGID_OMEGA = 0.25
RING = dict(rho_s=3.0, sigma=0.5, cut=4.0, phi0=-1.1, amp=0.8, g_power=3.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nt", [(1, 65), (LC_RANGE - 1, 65), (LC_RANGE, 65), (LC_RANGE + 1, 65), (3 * LC_RANGE + 5, 65), (LC_RANGE - 56, LC_TILE + 44),
                                  (300, LC_PASS + 3), (LC_RANGE * LC_MAX_RANGES + 300, 2)])
def test_synthetic_planes_around_the_tile_sizes(lib, n, nt):
    """Minkowski, a RIGID rotor, g = 1, every pixel on the ring: n around the block's range (LC_RANGE pixels), one pixel, a frame of more
    than LC_RANGE x LC_MAX_RANGES pixels (a block then owns two ranges); nt beyond one tile of LC_TILE samples and beyond one pass of LC_PASS.
    Against numpy to 1e-9 F_k (rho <= 5, sigma = 0.5: eps rho² / sigma² = 2e-14 per term)."""
    objs = [rt.Disk(0.05, 1.0, 6.0)]
    em = rt.DiskEmission(1, T_FRAME, orbit=RIGID_OMEGA, emitter="rigid")
    hit, se, g = ring_planes(n, 3.0, 1.9, seed=n)
    sp = rt.HotSpot(t_start=-2.0, dt=2 * math.pi / RIGID_OMEGA / 61.0, nt=nt, **RING)
    rc, got = lc_device(lib, rt.minkowski, objs, em, sp, None, n, 1, hit, se, g)
    assert rc == 0
    want, active = np_light_curve(hit, se, g, 1, RIGID_OMEGA, sp, None, n, 1)
    assert active == n
    if n == 1:      # one pixel is dark most of the time: where numpy sees light, the same light; where not, exactly none
        lit = want[:, 0] > 0
        assert lit.sum() >= 5 and (got[~lit] == 0).all() and worst(got[lit], want[lit]) <= 1e-9
        return
    assert worst(got, want) <= 1e-9, worst(got, want)


@pytest.mark.gpu
def test_synthetic_planes_symmetries(lib):
    objs = [rt.Disk(0.05, 1.0, 6.0)]
    em = rt.DiskEmission(1, T_FRAME, orbit=RIGID_OMEGA, emitter="rigid")
    n, nt = 3 * LC_RANGE + 5, 97
    hit, se, g = ring_planes(n, 3.0, 1.9, seed=3)
    period = 2 * math.pi / RIGID_OMEGA
    base = dict(dt=period / 61.0, nt=nt, **RING)
    run = lambda sp, planes=(hit, se, g): lc_device(lib, rt.minkowski, objs, em, sp, None, n, 1, *planes)
    rc, ref = run(rt.HotSpot(t_start=-2.0, **base))
    assert rc == 0 and (ref[:, 0] > 0).all()   # (a ring of 773 pixels: light at every observer time)
    # adding delta to every t_end == shifting t_start by delta
    delta = 1.375
    se2 = se.copy()
    se2[:, 0] += delta
    rc1, moved = run(rt.HotSpot(t_start=-2.0, **base), (hit, se2, g))
    rc2, shifted = run(rt.HotSpot(t_start=-2.0 + delta, **base))
    assert rc1 == 0 and rc2 == 0 and worst(moved, shifted) <= 1e-12, worst(moved, shifted)
    assert worst(moved, ref) > 1e-3                                    # (the shift is seen at all)
    # one period later: the same light curve
    rc, later = run(rt.HotSpot(t_start=-2.0 + period, **base))
    assert rc == 0 and worst(later, ref) <= 1e-12, worst(later, ref)
    # dt = 0: nt equal samples, bit for bit
    rc, still = run(rt.HotSpot(t_start=-2.0, dt=0.0, nt=nt, **RING))
    assert rc == 0 and all(still[k].tobytes() == still[0].tobytes() for k in range(nt)) and still[0].tobytes() == ref[0].tobytes()
    # a negative dt walks the same samples backwards
    rc, back = run(rt.HotSpot(t_start=-2.0 + (nt - 1) * base["dt"], dt=-base["dt"], nt=nt, **RING))
    assert rc == 0 and worst(back[::-1], ref) <= 1e-12
    # no active pixel: exactly zero — nothing hits the disk; g is NaN, zero or negative; the ring is out of reach; t_end is not finite
    for planes in ((np.zeros(n, np.uint32), se, g), (hit, se, np.full(n, np.nan)), (hit, se, np.zeros(n)), (hit, se, -g), (hit, se, np.full(n, np.inf)),
                   (hit, se * np.array([1, 5, 5, 1, 1, 1, 1, 1.0]), g), (hit, np.where(np.arange(8) == 0, np.nan, se), g)):
        rc, dark = run(rt.HotSpot(t_start=-2.0, **base), planes)
        assert rc == 0 and (dark == 0).all() and not np.signbit(dark).any()


@pytest.mark.gpu
def test_flat_space_physics(lib):
    """Minkowski, a RIGID rotor, a static observer on the axis 40 above the disk, perspective, square pixels h = 0.25 wide on the disk.  By
    axisymmetry the flux of a rigid circular spot that circles the axis is constant; what remains is pixel sampling: the Gaussian's
    aliasing at sigma = 3 h, exp(-2 pi² 9) ~ 1e-77, and the kink at the cut, (h² / sigma²)(cut exp(-cut² / 2) / 12) = 2e-7 at cut = 5 —
    below the 1e-6 asked for.  The centroid follows the projected circle to half a pixel."""
    ni, nj = SIZES[0]
    z0, h = 40.0, 0.25
    tx, ty = h * ni / 2 / z0, h * nj / 2 / z0
    ob = rt.Observer((0, 0, 0, z0), (0, 0, 0, -1), (0, 0, 1, 0), 2 * math.atan(tx), 2 * math.atan(ty))
    metric, objs = rt.minkowski, [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -60.0), rt.Plane(-200.0), rt.Disk(0.05, 0.001, 8.0)]
    omega = 0.1
    em = rt.DiskEmission(3, T_FRAME, orbit=omega, emitter="rigid")
    sp = rt.HotSpot(0.2, 3 * h, t_start=0.0, dt=2 * math.pi / omega / 32.0, nt=64, cut=5.0, phi0=0.3, g_power=4.0)
    assert sp.rho_s + sp.cut * sp.sigma < h * nj / 2
    # (the event search looks at interp_points points per step, and in flat space a step is many units long: the rays cross the disk,
    # 0.1 thick, within sqrt(2) x 0.1 of lambda — tests/test_observer.py's flat-space check sizes its solver the same way)
    opt = rt.solver_defaults()
    opt.interp_points = int(math.ceil((opt.lambda1 - opt.lambda0) / (math.sqrt(2.0) * 0.1))) + 2
    res = rt.light_curve(metric, objs, ob, ni, nj, em, sp, opt=opt, details=True)
    F, A, B = res["lc"].T
    on_disk = res["hit"] == 3
    assert on_disk.all() and np.isfinite(res["g"]).all()                       # (the whole window looks at the disk)
    ripple = float((F.max() - F.min()) / F.mean())
    print(f"flat space: F constant to {ripple:.2e} over two periods")
    assert F.min() > 0 and ripple <= 1e-6, ripple
    # the projected circle: the spot's centre lies at height 0.05 (the disk's face), seen from z0; its light left at t = -distance
    zf = z0 - 0.05
    t_emit = -math.hypot(zf, sp.rho_s)
    phi = sp.phi0 + omega * (t_emit + res["tau"])
    a_want, b_want = sp.rho_s * np.cos(phi) / zf / tx, sp.rho_s * np.sin(phi) / zf / ty
    da, db = np.abs(A / F - a_want).max(), np.abs(B / F - b_want).max()
    print(f"flat space: centroid off the projected circle by {da * ni:.3f} pixel widths in a, {db * nj:.3f} in b")
    assert da <= 1.0 / ni and db <= 1.0 / nj
    assert np.ptp(A / F) > 1.0 / ni                                                 # (it does move)


def trace_lc_device(lib, metric, objs, ob, ni, nj, em, sp, dtype=np.float64, stream=None, binds=None, want_out=True, want_g=True, want_ctr=True):
    """rtgr_trace_light_curve_device_* with torch planes -> (rc, dict of numpy arrays)"""
    import torch
    from test_textures import _outputs
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    td = torch.float64 if dtype == np.float64 else torch.float32
    sh = rt.make_shade(binds) if binds is not None else None
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        rgb = torch.full((3, n), -5.0, dtype=td, device="cuda")
        g = torch.full((n,), -5.0, dtype=td, device="cuda")
        lc = torch.full((int(sp.nt), 3), -7.0, dtype=torch.float64, device="cuda")
        dev = _outputs(n, dtype, device=True)
        o = abi.rtgr_ray_outputs()
        for key in OUT_KEYS:
            setattr(o, key, dev[key].data_ptr())
        ctr = abi.rtgr_counters()
        torch.cuda.synchronize()
        fn = lib.rtgr_trace_light_curve_device_f64 if dtype == np.float64 else lib.rtgr_trace_light_curve_device_f32
        rc = fn(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, C.byref(sh) if sh is not None else None, C.byref(em), C.byref(sp), rgb.data_ptr(),
                C.byref(o) if want_out else None, g.data_ptr() if want_g else None, lc.data_ptr(), C.byref(ctr) if want_ctr else None,
                stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    res = dict(rgb=rgb.cpu().numpy(), g=g.cpu().numpy(), lc=lc.cpu().numpy(), counters=ctr.as_dict())
    res.update({k: v.cpu().numpy() for k, v in dev.items()})
    return rc, res


@pytest.mark.gpu
def test_determinism_streams_and_batches(lib):
    import torch
    metric, objs = kerr_disk_scene()
    em = rt.DiskEmission(3, T_FRAME)
    ni, nj = SIZES[0]
    sp = rt.HotSpot(nt=130, **SPOT)
    side = torch.cuda.Stream()
    rc, first = trace_lc_device(lib, metric, objs, orbiting(), ni, nj, em, sp)
    assert rc == 0 and (first["lc"][:, 0] > 0).sum() > 60
    for stream, batch, bare in ((None, 0, False), (side, 0, False), (side, 0, True), (None, ni, False), (side, 5 * ni, False), (None, 5 * ni, True)):
        rc, again = trace_lc_device(lib, metric, objs, orbiting(max_batch_rays=batch), ni, nj, em, sp, stream=stream, want_out=not bare, want_g=not bare,
                                    want_ctr=not bare)
        assert rc == 0 and again["lc"].tobytes() == first["lc"].tobytes(), (stream is not None, batch, bare)
    f = frame("perspective", SIZES[0])
    for stream in (None, side, None):
        rc, lc = lc_device(lib, metric, objs, em, sp, orbiting(), ni, nj, f["hit32"], f["state_end"], f["g"], stream=stream)
        assert rc == 0 and lc.tobytes() == first["lc"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("proj,size", [("perspective", SIZES[0]), ("equirect", SIZES[1])])
def test_float32_entry(lib, proj, size):
    """the Float32 entry reduces in double: against the restatement fed the Float32 planes promoted to double (and the Float32 rate promoted),
    to 1e-9 F_k.  Against the Float64 frame: reported."""
    metric, objs = kerr_disk_scene()
    em, ob = rt.DiskEmission(3, T_FRAME), orbiting(proj)
    ni, nj = size
    sp = rt.HotSpot(nt=65, **SPOT)
    rc, got = trace_lc_device(lib, metric, objs, ob, ni, nj, em, sp, dtype=np.float32)
    assert rc == 0 and got["state_end"].dtype == np.float32 and got["lc"].dtype == np.float64
    om = disk_omega(metric, objs, em, sp.rho_s, np.float32)
    assert om.dtype == np.float32
    want, active = np_light_curve(got["hit32"].view(np.uint32), got["state_end"], got["g"], 3, float(om), sp, ob, ni, nj)
    assert active >= 20
    err = worst(got["lc"], want)
    f = frame(proj, size)
    want64, _ = np_light_curve(f["hit32"], f["state_end"], f["g"], 3, disk_omega(metric, objs, em, sp.rho_s), sp, ob, ni, nj)
    print(f"Float32 entry {proj} {ni}x{nj}: {active} active, {err:.2e} F_k off its own planes' restatement; "
          f"{float((np.abs(got['lc'][:, 0] - want64[:, 0])[want64[:, 0] > 0] / want64[want64[:, 0] > 0, 0]).max()):.2e} off the Float64 frame's F")
    assert err <= 1e-9, err
    rc, again = lc_device(lib, metric, objs, em, sp, ob, ni, nj, got["hit32"].view(np.uint32), got["state_end"], got["g"], dtype=np.float32)
    assert rc == 0 and again.tobytes() == got["lc"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_trace_is_untouched(lib, dtype):
    """rgb, g, every per-ray output and the counters of rtgr_trace_light_curve_* == those of rtgr_trace_observer_* with the same emit, bit for
    bit; the host entry likewise; once with textures bound as well"""
    from test_observer import trace_observer
    from test_textures import NEAREST, same_bits, texture
    metric, objs = kerr_disk_scene()
    em = rt.DiskEmission(3, T_FRAME)
    sp = rt.HotSpot(nt=7, **SPOT)
    _, tex = texture("rand16x8")
    for (ni, nj), proj, binds in ((SIZES[0], "perspective", None), (SIZES[1], "equirect", None), (SIZES[1], "perspective", {0: (tex, NEAREST), 1: (tex, NEAREST)})):
        if binds is not None and dtype != np.float64:
            continue
        ob = orbiting(proj, 200)
        rc, want = trace_observer(lib, metric, objs, ob, ni, nj, dtype, emit=em, binds=binds)
        assert rc == 0
        rc, got = trace_lc_device(lib, metric, objs, ob, ni, nj, em, sp, dtype=dtype, binds=binds)
        assert rc == 0
        for key in ("rgb", "g") + OUT_KEYS:
            assert got[key].tobytes() == want[key].tobytes(), (key, proj, dtype)
        assert got["counters"] == want["counters"]
        # the host-pointer entry
        sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
        from test_textures import _outputs
        host = dict(_outputs(n, dtype), rgb=np.zeros((3, n), dtype), g=np.zeros(n, dtype), lc=np.zeros((7, 3)))
        o = abi.rtgr_ray_outputs()
        for key in OUT_KEYS:
            setattr(o, key, host[key].ctypes.data)
        ctr = abi.rtgr_counters()
        sh = rt.make_shade(binds) if binds is not None else None
        fn = lib.rtgr_trace_light_curve_f64 if dtype == np.float64 else lib.rtgr_trace_light_curve_f32
        abi.check(lib, fn(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, C.byref(sh) if sh is not None else None, C.byref(em), C.byref(sp),
                          host["rgb"].ctypes.data, C.byref(o), host["g"].ctypes.data, host["lc"].ctypes.data, C.byref(ctr)))
        for key in ("rgb", "g") + OUT_KEYS:
            assert same_bits(host[key], want[key]), (key, proj, dtype)
        assert ctr.as_dict() == want["counters"] and host["lc"].tobytes() == got["lc"].tobytes()


@pytest.mark.gpu
def test_refusals(lib):
    """Every refusal: RTGR_ERR_BAD_ARG with a message, lc (and rgb) untouched."""
    import torch
    from test_grid_metric import ETA
    from test_grid_metric_4d import grid4
    metric, objs = kerr_disk_scene()
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ni, nj = 8, 6
    n = ni * nj
    rgb = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
    lc = torch.full((4, 3), -7.0, dtype=torch.float64, device="cuda")
    hit = torch.zeros(n, dtype=torch.int32, device="cuda")
    se = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    g = torch.zeros(n, dtype=torch.float64, device="cuda")
    h_rgb, h_lc = np.full((3, n), -5.0), np.full((4, 3), -7.0)
    nan, inf = math.nan, math.inf

    def call(scene=sc, emit=True, spot=True, obs=True, planes=(True, True, True), have_lc=True, em_over=None, ob_over=None, hook=True, **over):
        ob = orbiting()
        for key, val in (ob_over or {}).items():
            setattr(ob, key, val)
        em = rt.DiskEmission(3, T_FRAME)
        for key, val in (em_over or {}).items():
            setattr(em, key, val)
        sp = rt.HotSpot(nt=4, **SPOT)
        for key, val in over.items():
            setattr(sp, key, val)
        emp, spp, obp = C.byref(em) if emit else None, C.byref(sp) if spot else None, C.byref(ob) if obs else None
        rcs, msgs = [], []
        if obs or planes != (True, True, True):      # (the reduction alone takes obs = NULL: the plane camera)
            rcs.append(lib.rtgr_light_curve_device_f64(None, C.byref(scene), emp, spp, obp, ni, nj, hit.data_ptr() if planes[0] else None,
                                                       se.data_ptr() if planes[1] else None, g.data_ptr() if planes[2] else None,
                                                       lc.data_ptr() if have_lc else None, None))
            msgs.append(lib.rtgr_last_error())
        if planes == (True, True, True):
            rcs.append(lib.rtgr_trace_light_curve_device_f64(None, C.byref(scene), C.byref(opt), obp, ni, nj, None, emp, spp, rgb.data_ptr(), None, None,
                                                             lc.data_ptr() if have_lc else None, None, None))
            msgs.append(lib.rtgr_last_error())
            rcs.append(lib.rtgr_trace_light_curve_f64(None, C.byref(scene), C.byref(opt), obp, ni, nj, None, emp, spp, h_rgb.ctypes.data, None, None,
                                                      h_lc.ctypes.data if have_lc else None, None))
            msgs.append(lib.rtgr_last_error())
            if hook and obs and have_lc and not ob_over:
                om, pts, j = np.full(1, -3.0), np.zeros((2, 3)), np.full(2, -3.0)
                rcs.append(lib.rtgr_eval_hot_spot_f64(None, C.byref(scene), emp, spp, pts.ctypes.data, 2, om.ctypes.data, None, j.ctypes.data))
                msgs.append(lib.rtgr_last_error())
                assert rcs[-1] == 0 or (om[0] == -3.0 and (j == -3.0).all())
        return rcs, msgs

    user = rt.make_scene(metric, objs)
    user.metric = abi.USER
    cases = [(dict(emit=False), b"emit"), (dict(spot=False), b"rtgr_hot_spot is NULL"), (dict(have_lc=False), b"lc is NULL"),
             (dict(planes=(False, True, True)), b"hit32 is NULL"), (dict(planes=(True, False, True)), b"state_end is NULL"), (dict(planes=(True, True, False)), b"g is NULL"),
             (dict(nt=0), b"nt"), (dict(nt=(1 << 20) + 1), b"nt"), (dict(sigma=0.0), b"sigma"), (dict(sigma=-1.0), b"sigma"), (dict(sigma=nan), b"sigma"),
             (dict(cut=0.0), b"cut"), (dict(cut=nan), b"cut"), (dict(amp=-0.1), b"amp"), (dict(amp=nan), b"amp"), (dict(rho_s=nan), b"rho_s"),
             (dict(rho_s=inf), b"rho_s"), (dict(phi0=inf), b"phi0"), (dict(g_power=nan), b"g_power"), (dict(t_start=inf), b"t_start"), (dict(dt=nan), b"dt"),
             (dict(rho_s=1.9), b"[r_in, r_out]"), (dict(rho_s=4.1), b"[r_in, r_out]"), (dict(flags=1), b"flags"), (dict(pad=1), b"pad"),
             (dict(scene=user), b"RTGR_USER"), (dict(em_over=dict(object=1)), b"Sphere"), (dict(em_over=dict(orbit=0.5)), b"+1"),
             (dict(em_over=dict(T_in=0.0)), b"T_in"), (dict(ob_over=dict(kind=3)), b"unknown rtgr_observer.kind"), (dict(ob_over=dict(fov_x=4.0)), b"(0, pi)"),
             (dict(ob_over=dict(pad=1)), b"pad")]
    for kw, word in cases:
        rcs, msgs = call(**kw)
        assert rcs and rcs == [abi.ERR_BAD_ARG] * len(rcs) and all(word in m for m in msgs), (kw, rcs, msgs)
    # the traced entries need their observer
    ob_none = call(obs=False)
    assert ob_none[0] == [abi.ERR_BAD_ARG] * 2 and all(b"rtgr_observer is NULL" in m for m in ob_none[1])
    # a time-dependent grid
    flat4 = grid4(np.broadcast_to(ETA, (6, 6, 6, 10)).copy(), 4, -1.0, 1.0, (-3.0,) * 3, 1.0, name="flat4")
    g4 = rt.make_scene(flat4, [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(-20.0), rt.Disk(0.05, 2.0, 4.0)])
    rcs, msgs = call(scene=g4, ob_over=dict(kind=0))
    assert rcs == [abi.ERR_BAD_ARG] * 3 and all(b"4-D" in m for m in msgs), (rcs, msgs)
    torch.cuda.synchronize()
    assert bool((lc == -7.0).all()) and bool((rgb == -5.0).all()) and (h_lc == -7.0).all() and (h_rgb == -5.0).all()
    # … and the same call with nothing wrong is served: at the edges of the Disk's range too
    for rho_s in (2.0, 4.0, 3.0):
        rcs, _ = call(rho_s=rho_s)
        assert rcs == [0, 0, 0, 0]
    torch.cuda.synchronize()
    assert not bool((lc == -7.0).any()) and not (h_lc == -7.0).any() and lc[:, 0].cpu().numpy().tobytes() == h_lc[:, 0].tobytes()


@pytest.mark.gpu
def test_capture_replay_and_trim(lib):
    """ctr == NULL: both device entries are captured once workspace and scratch exist, replay the eager light curve to the bit, refuse to
    grow the scratch or to deliver counters during capture; rtgr_trim afterwards, and a fresh call gives the same"""
    import torch
    from test_textures import _hip_runtime
    metric, objs = kerr_disk_scene()
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    em = rt.DiskEmission(3, T_FRAME)
    ni, nj = SIZES[1]
    n = ni * nj
    ob = orbiting("equirect", 200)
    sp, sp_long = rt.HotSpot(nt=70, **SPOT), rt.HotSpot(nt=3000, **SPOT)
    side = torch.cuda.Stream()
    hip = _hip_runtime()

    def traced(rgb, lc, spot=sp, ctr=None):
        return lib.rtgr_trace_light_curve_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, C.byref(em), C.byref(spot), rgb.data_ptr(),
                                                     None, None, lc.data_ptr(), C.byref(ctr) if ctr is not None else None, side.cuda_stream)

    f = frame("equirect", SIZES[1])
    with torch.cuda.stream(side):
        d_hit = torch.from_numpy(f["hit32"].view(np.int32).copy()).cuda()
        d_se, d_g = torch.from_numpy(f["state_end"].copy()).cuda(), torch.from_numpy(f["g"].copy()).cuda()
        rgb_eager, rgb_out = (torch.zeros((3, n), dtype=torch.float64, device="cuda") for _ in range(2))
        lc_eager, lc_out, lc_alone, lc_fresh = (torch.zeros((70, 3), dtype=torch.float64, device="cuda") for _ in range(4))
        lc_long = torch.zeros((3000, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def alone(lc, spot=sp):
        return lib.rtgr_light_curve_device_f64(None, C.byref(sc), C.byref(em), C.byref(spot), C.byref(ob), ni, nj, d_hit.data_ptr(), d_se.data_ptr(),
                                               d_g.data_ptr(), lc.data_ptr(), side.cuda_stream)

    abi.check(lib, traced(rgb_eager, lc_eager))                # the warm-up: workspace and scratch of this size exist afterwards
    torch.cuda.synchronize()
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc_big = traced(rgb_out, lc_long, spot=sp_long)            # more samples: the scratch would have to grow
    msg_big = lib.rtgr_last_error()
    rc_big2 = alone(lc_long, spot=sp_long)
    msg_big2 = lib.rtgr_last_error()
    rc_ctr = traced(rgb_out, lc_out, ctr=abi.rtgr_counters())  # counters need a synchronisation
    msg_ctr = lib.rtgr_last_error()
    rc = traced(rgb_out, lc_out)
    rc2 = alone(lc_alone)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert rc == 0 and rc2 == 0 and rc_ctr == abi.ERR_BAD_ARG and b"ctr" in msg_ctr
    assert rc_big == abi.ERR_BAD_ARG and b"captured" in msg_big and rc_big2 == abi.ERR_BAD_ARG and b"captured" in msg_big2
    assert graph.value and hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(rgb_out, rgb_eager) and torch.equal(lc_out, lc_eager) and torch.equal(lc_alone, lc_eager) and int((lc_eager[:, 0] > 0).sum()) > 35
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, traced(rgb_out, lc_fresh))
    torch.cuda.synchronize()
    assert torch.equal(lc_fresh, lc_eager)
    want, active = np_light_curve(f["hit32"], f["state_end"], f["g"], 3, disk_omega(metric, objs, em, sp.rho_s), sp, ob, ni, nj)
    assert active >= 20 and worst(lc_fresh.cpu().numpy(), want) <= 1e-9
