"""Disk spectra (include/rtgr.h "disk spectra"): one traced frame of an emitting disk reduced on the device to the
profile of a narrow line (the flux-weighted histogram of the frequency ratio g) or to the spectrum of the black-body disk (the
picture's Planck law at many frequencies).  The judge is a numpy restatement of the header's contract, summed with math.fsum, fed the
planes a trace delivered or synthetic ones.

CPU tests: the symbols, the struct layout (ctypes, a compiled C caller, the Julia stub), the tile constants, the error without a
device, the restatement itself.  GPU tests: the hook, synthetic planes around the kernel's sizes, real frames, identities, flat-space
and Schwarzschild physics, determinism, the untouched trace, the refusals."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from scenes import rt
from test_light_curve import T_FRAME, frame, kerr_disk_scene, np_weight, orbiting

abi = rt._abi
SPEC_EXPORTS = ("rtgr_spectrum_device_f64", "rtgr_spectrum_device_f32", "rtgr_trace_spectrum_device_f64", "rtgr_trace_spectrum_device_f32",
                "rtgr_trace_spectrum_f64", "rtgr_trace_spectrum_f32", "rtgr_eval_spectrum_f64", "rtgr_eval_spectrum_f32")
SIZES = ((48, 32), (37, 19))
OUT_KEYS = ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject", "hit32")
# the kernel's sizes, as csrc/rtgr_spectrum.hpp names them (test_the_tile_sizes_are_the_headers holds them against the header)
SPEC_WAVE, SPEC_RANGE, SPEC_LANE_BINS, SPEC_TILE, SPEC_PASS, SPEC_REC = 64, 256, 4, 256, 1024, 4
LC_MAX_RANGES = 1024
LINE, THERMAL = abi.SPEC_LINE, abi.SPEC_THERMAL


# ---- the header's contract in numpy (float64) -----------------------------------------------------------------------------------------
def np_base(hit32, se, g, obj):
    """-> (mask of the pixels of the common set, rho, g) in double"""
    se, g = np.asarray(se, np.float64), np.asarray(g, np.float64)
    x, y = se[:, 1], se[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (np.asarray(hit32) == obj) & np.isfinite(g) & (g > 0) & np.isfinite(x) & np.isfinite(y)
        rho = np.sqrt(x * x + y * y)
    return ok, rho, g


def np_line_bins(spec, g):
    """the contract's bin: u = (g - lo) * s, s = nb / (hi - lo) -> (counts, bin)"""
    nb = int(spec.nb)
    s = float(nb) / (spec.hi - spec.lo)
    with np.errstate(invalid="ignore"):
        u = (np.asarray(g, np.float64) - spec.lo) * s
        ok = (u >= 0.0) & (u < float(nb))
    return ok, np.where(ok, u, 0.0).astype(np.int64)


def np_line_value(spec, rho, g):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return spec.amp * (rho / spec.rho_min) ** (-spec.alpha) * g ** spec.g_power


def np_temperature(em, r_in, rho):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        T = em.T_in * (rho / r_in) ** (-em.p)
        if em.flags & abi.EMIT_INNER_EDGE:
            T = T * np.sqrt(np.sqrt(np.maximum(1.0 - np.sqrt(r_in / rho), 0.0)))
    return T


def np_theta(spec):
    nb, k = int(spec.nb), np.arange(int(spec.nb), dtype=np.float64)
    if nb == 1:
        return np.array([spec.lo])
    if spec.flags & abi.SPEC_LOG:
        return spec.lo * np.exp(k * math.log(spec.hi / spec.lo) / (nb - 1))
    return spec.lo + k * (spec.hi - spec.lo) / (nb - 1)


def np_axis(spec):
    if spec.kind == THERMAL:
        return np_theta(spec)
    return spec.lo + (np.arange(int(spec.nb)) + 0.5) * (spec.hi - spec.lo) / int(spec.nb)


def np_factor(spec, em, theta):
    return em.gain * (theta * theta * theta) if spec.flags & abi.SPEC_NU3 else np.full_like(theta, em.gain)


def np_spectrum(hit32, se, g, obj, em, r_in, spec, ob, ni, nj):
    """-> (out [nb, 3] by math.fsum, the indices of the counted pixels, per-bin pixel counts (LINE) or None)"""
    ok, rho, g = np_base(hit32, se, g, obj)
    w, a, b = np_weight(ob, ni, nj)
    nb = int(spec.nb)
    out = np.zeros((nb, 3))
    if spec.kind == LINE:
        inb, bins = np_line_bins(spec, g)
        with np.errstate(invalid="ignore"):
            ok = ok & inb & (rho >= spec.rho_min) & (rho < spec.rho_max)
        idx = np.flatnonzero(ok)
        W = w[idx] * np_line_value(spec, rho[idx], g[idx])
        order = np.argsort(bins[idx], kind="stable")
        sb = bins[idx][order]
        cuts = np.searchsorted(sb, np.arange(nb + 1))
        for k in range(nb):
            sel = order[cuts[k]:cuts[k + 1]]
            if len(sel):
                out[k] = (math.fsum(W[sel]), math.fsum(W[sel] * a[idx][sel]), math.fsum(W[sel] * b[idx][sel]))
        return out, idx, np.diff(cuts)
    T = np_temperature(em, r_in, rho)
    with np.errstate(invalid="ignore"):
        ok = ok & (T > 0)
    idx = np.flatnonzero(ok)
    tau = 1.0 / (g[idx] * T[idx])
    theta = np_theta(spec)
    c = np_factor(spec, em, theta)
    wa, wb = w[idx] * a[idx], w[idx] * b[idx]
    for k in range(nb):
        with np.errstate(over="ignore"):
            e = 1.0 / np.expm1(theta[k] * tau)
        out[k] = (c[k] * math.fsum(w[idx] * e), c[k] * math.fsum(wa * e), c[k] * math.fsum(wb * e))
    return out, idx, None


def worst(got, want):
    """max over the bins or samples and the three columns of |got - want| / F.  Where the judge finds nothing (F = 0) "within 1e-9 F"
    means exactly 0: asserted here."""
    F = want[:, 0]
    lit = F > 0
    assert lit.any() and (F >= 0).all()
    assert (got[~lit] == 0).all() and (want[~lit] == 0).all()
    return float((np.abs(got - want)[lit] / F[lit, None]).max())


def merge_pairs(out):
    return out[0::2] + out[1::2]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(SPEC_EXPORTS) <= set(abi.EXPORTS) and len(SPEC_EXPORTS) == 8
    lib = abi.load()
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    for s in SPEC_EXPORTS:
        assert hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    flat = re.sub(r"\s*\n \*\s*", " ", hdr)
    for words in ("u = (g_p - lo) * s", "b = (uint64)u", "rho_min <= rho_p < rho_max", "the same device function", "accumulated as fma(W, e, F)",
                  "applied once, after the sum", "theta_k = lo exp(k log(hi / lo) / (nb - 1))", "pixel order within a fixed range of pixels, then range order",
                  "No floating-point atomics", "n nb > 2^26 is refused",
                  # the out-of-scope list
                  "spectra of the hot spot", "line emissivity other than a power law", "limb darkening", "a colour-matching integral",
                  "linear (two-bin) deposit", "anti-aliasing", "the sharded, frames-in-flight, pixel-array and single-ray entry points",
                  # … and the light curve's own words stay
                  "spectra of the spot",
                  "#define RTGR_SPECTRUM_MAX_BINS (1ull << 16)", "enum rtgr_spectrum_kind { RTGR_SPEC_LINE = 0, RTGR_SPEC_THERMAL = 1 }",
                  "#define RTGR_SPEC_LOG 1u", "#define RTGR_SPEC_NU3 2u"):
        assert words in flat, words
    assert {"Spectrum", "spectrum", "eval_spectrum"} <= set(rt.api.__all__) and all(hasattr(rt, k) for k in ("Spectrum", "spectrum", "eval_spectrum"))


def test_the_tile_sizes_are_the_headers():
    # the sizes are the one reduction's (rtgr_reduce.hpp), the record length the spectra's own
    csrc = os.path.join(ROOT, "raytracegr.jl_amd", "csrc")
    txt = open(os.path.join(csrc, "rtgr_reduce.hpp")).read()
    for name, val in (("RED_WAVE", SPEC_WAVE), ("RED_RANGE", SPEC_RANGE), ("RED_LANE_ITEMS", SPEC_LANE_BINS), ("RED_PASS", SPEC_PASS), ("RED_MAX_RANGES", LC_MAX_RANGES)):
        assert re.search(r"constexpr \w+ " + name + r" = " + str(val) + r";", txt), name
    assert "RED_TILE = RED_WAVE * RED_LANE_ITEMS" in txt and SPEC_TILE == SPEC_WAVE * SPEC_LANE_BINS
    spec = open(os.path.join(csrc, "rtgr_spectrum.hpp")).read()
    assert re.search(r"constexpr \w+ SPEC_REC = " + str(SPEC_REC) + ";", spec) and not re.search(r"constexpr \w+ (SPEC|RED)_(WAVE|RANGE|LANE_\w+|TILE|PASS) =", spec)
    # the pixel weight: its defining body stands in one file of csrc/, the models call it, and no .hip file holds a copy of its expression
    texts = {f: open(os.path.join(csrc, f)).read() for f in os.listdir(csrc) if f.endswith((".hip", ".hpp"))}
    assert [f for f, t in texts.items() if re.search(r"RTGR_DEV double pixel_weight\(", t)] == ["rtgr_reduce.hpp"]
    assert "pixel_weight(" in texts["rtgr_spectrum.hip"] and "pixel_weight(" in texts["rtgr_lightcurve.hip"]
    assert [f for f, t in texts.items() if "W.scale / (s * sqrt(s))" in t] == ["rtgr_reduce.hpp"]


def test_struct_layout_in_ctypes_a_compiled_c_caller_and_the_julia_stub(tmp_path):
    s = abi.rtgr_spectrum
    want = dict(kind=0, flags=4, nb=8, lo=16, hi=24, amp=32, alpha=40, rho_min=48, rho_max=56, g_power=64, reserved=72)
    assert abi.RtgrSpectrum is s
    assert C.sizeof(s) == 80 and {k: getattr(s, k).offset for k in want} == want and [n for n, _ in s._fields_] == list(want)
    exe = str(tmp_path / "spectrum_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "spectrum_layout.c"), "-o", exe, "-ldl"])
    out = subprocess.check_output([exe], text=True).split()
    assert dict(zip(out[0::2], map(int, out[1::2]))) == dict(want, spectrum=80)
    assert subprocess.run([exe, abi.LIB_PATH]).returncode == 0                     # (2: a symbol does not resolve)
    sp = rt.Spectrum("line", 0.1, 1.5, 70, amp=2.0, alpha=3.0, rho_min=2.0, rho_max=4.0, g_power=3.0)
    assert (sp.kind, sp.flags, sp.nb, sp.lo, sp.hi, sp.amp, sp.alpha, sp.rho_min, sp.rho_max, sp.g_power, sp.reserved) == (0, 0, 70, 0.1, 1.5, 2.0, 3.0, 2.0, 4.0, 3.0, 0.0)
    st = rt.Spectrum("thermal", 5.0, 9.0, 4, log=True, nu3=True)
    assert (st.kind, st.flags, st.nb, st.lo, st.hi, st.amp, st.alpha, st.rho_min, st.rho_max, st.g_power, st.reserved) == (1, 3, 4, 5.0, 9.0, 0, 0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="kind"):
        rt.Spectrum("lines", 0, 1, 2)
    # the Julia stub: the struct in the header's order, the fieldoffset table, the three functions, the hook asked before the trace
    from test_julia_stub import HDR, JL, c_kind, c_prototypes, ccalls, jl_kind, strip_julia
    text = open(JL).read()
    code = strip_julia(text)
    body = re.search(r"struct RtgrSpectrum[ \t]*\n((?:.|\n)*?)\nend", code).group(1)
    assert re.findall(r"([A-Za-z_0-9]+)::", body) == list(want)
    hdr = re.sub(r"/\*(?:.|\n)*?\*/", " ", open(HDR).read())
    cbody = re.search(r"typedef struct[^{]*\{((?:[^{}]|\{[^{}]*\})*)\}\s*rtgr_spectrum\s*;", hdr).group(1)
    cfields = [n.strip() for d in cbody.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
    assert cfields == list(want)
    m = re.search(r"^#\s+RtgrSpectrum\s+(\d+)\s+(.*)$", text, re.M)
    assert m and int(m.group(1)) == 80 and [(n, int(o)) for n, o in re.findall(r"([a-z_A-Z0-9]+) (\d+)", m.group(2))] == list(want.items())
    protos = c_prototypes()
    bound = {c[0]: c for c in ccalls() if "spectrum" in c[0]}
    assert set(bound) == {"rtgr_trace_spectrum_f64", "rtgr_trace_spectrum_f32", "rtgr_eval_spectrum_f64", "rtgr_eval_spectrum_f32"}
    for sym, (_, ret, types, args) in bound.items():
        cret, cparams = protos[sym]
        assert ret == "Cint" and cret == "int" and len(types) == len(args) == len(cparams) == (14 if "trace" in sym else 9)
        assert [jl_kind(t) for t in types] == [c_kind(t) for t in cparams]
        assert "Ptr{RtgrSpectrum}" in [t.strip() for t in types]
    for word in ("function Spectrum(", "function spectrum(", "function eval_spectrum(", "const RTGR_SPEC_LINE = UInt32(0)", "const RTGR_SPEC_THERMAL = UInt32(1)",
                 "const RTGR_SPEC_LOG = UInt32(1)", "const RTGR_SPEC_NU3 = UInt32(2)"):
        assert word in text, word
    fn = code[code.index("function spectrum("):]
    fn = fn[:fn.index("\nend\n")]
    assert 0 < fn.index("observer_frame(scene, obs") < fn.index("eval_spectrum(scene, emit, sp") < fn.index("ccall(")


def test_no_result_without_a_device():
    """Without a HIP device every new entry FAILS with RTGR_ERR_NO_DEVICE, says so, and leaves the caller's arrays alone."""
    import torch
    if torch.cuda.is_available():
        return
    lib, nd = abi.load(), abi.ERR_NO_DEVICE
    metric, objs = rt.KerrSchild(1, 0.5), [rt.Disk(0.05, 3.0, 6.0)]
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ob, em = rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 1.0), rt.DiskEmission(1, 6000.0)
    sp = rt.Spectrum("line", 0.0, 1.6, 3, rho_min=3.0, rho_max=6.0)
    for dtype, suf in ((np.float64, "f64"), (np.float32, "f32")):
        rgb, g, out, se, hit = np.full((3, 4), -7.0, dtype), np.full(4, -7.0, dtype), np.full((3, 3), -7.0), np.zeros((4, 8), dtype), np.zeros(4, np.uint32)
        rc = getattr(lib, "rtgr_trace_spectrum_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(ob), 2, 2, None, C.byref(em), C.byref(sp), rgb.ctypes.data,
                                                        None, g.ctypes.data, out.ctypes.data, None)
        assert rc == nd and b"no CPU fallback" in lib.rtgr_last_error()
        assert getattr(lib, "rtgr_trace_spectrum_device_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(ob), 2, 2, None, C.byref(em), C.byref(sp),
                                                                 rgb.ctypes.data, None, g.ctypes.data, out.ctypes.data, None, None) == nd
        assert getattr(lib, "rtgr_spectrum_device_" + suf)(None, C.byref(sc), C.byref(em), C.byref(sp), C.byref(ob), 2, 2, hit.ctypes.data, se.ctypes.data,
                                                           g.ctypes.data, out.ctypes.data, None) == nd
        axis, bins, val, pts = np.full(3, -7.0), np.full(2, -7, np.int64), np.full(2, -7.0), np.zeros((2, 3), dtype)
        assert getattr(lib, "rtgr_eval_spectrum_" + suf)(None, C.byref(sc), C.byref(em), C.byref(sp), pts.ctypes.data, 2, axis.ctypes.data, bins.ctypes.data,
                                                         val.ctypes.data) == nd
        assert (rgb == -7.0).all() and (g == -7.0).all() and (out == -7.0).all() and (axis == -7.0).all() and (bins == -7).all() and (val == -7.0).all()
    for call in (lambda: rt.spectrum(metric, objs, ob, 2, 2, em, sp), lambda: rt.eval_spectrum(metric, objs, em, sp)):
        with pytest.raises(abi.RtgrError, match="no CPU fallback"):
            call()


def synthetic_planes(n, dtype, seed):
    """n pixels of object 1 on a Disk(0.05, 2.0, 8.0): off-disk pixels, NaN / 0 / negative / infinite g, non-finite end points, g
    outside [0.4, 1.2) and none in (0.85, 0.95), rho outside [2.2, 6) and inside r_in (where the inner-edge law has T = 0); pixel 0 — the first three, when there
    are three — is good and shares one g, so one bin holds >= 3 pixels.  Rounded to `dtype` (the entry promotes what it reads)."""
    rng = np.random.default_rng(seed)
    hit = np.where(rng.uniform(size=n) < 0.95, 1, rng.integers(0, 3, n)).astype(np.uint32)
    g = np.where(rng.uniform(size=n) < 0.6, rng.uniform(0.35, 0.85, n), rng.uniform(0.95, 1.25, n))      # (nothing in 0.85 .. 0.95: bins with no pixel)
    bad = rng.uniform(size=n)
    g = np.where(bad < 0.01, np.nan, np.where(bad < 0.02, 0.0, np.where(bad < 0.03, -g, np.where(bad < 0.035, np.inf, g))))
    rho, psi = rng.uniform(1.9, 6.4, n), rng.uniform(-math.pi, math.pi, n)
    se = rng.uniform(-1.0, 1.0, (n, 8))
    se[:, 1], se[:, 2] = rho * np.cos(psi), rho * np.sin(psi)
    pt = rng.uniform(size=n)
    se[:, 1] = np.where(pt < 0.01, np.nan, np.where(pt < 0.015, np.inf, se[:, 1]))
    se[:, 2] = np.where((pt > 0.015) & (pt < 0.025), -np.inf, se[:, 2])
    for k in range(min(3, n)):
        hit[k], g[k] = 1, 0.8125
        se[k, 1], se[k, 2] = 3.0 + 0.25 * k, 0.5
    return hit, se.astype(dtype), g.astype(dtype)


SYN_OBJS = [rt.Disk(0.05, 2.0, 8.0)]
SYN_LINE = dict(lo=0.4, hi=1.2, amp=1.5, alpha=2.5, rho_min=2.2, rho_max=6.0, g_power=3.0)
SYN_THETA = (2.0e3, 6.0e4)


def syn_emission():
    return rt.DiskEmission(1, T_FRAME, orbit=0.0, emitter="rigid", inner_edge=True, gain=0.75)


def syn_canvas(n):
    """(ni, nj, observer): a canvas of two axes with a perspective weight where n factors, one row with w = 1 where it is prime"""
    ni = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    if ni == 1:
        return n, 1, None
    return n // ni, ni, rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 0.9, 0.7)


def test_the_numpy_restatement_against_itself():
    """(CPU: the judge itself.)  LINE with nb bins merged pairwise == LINE with nb / 2 bins: s / 2 is exact, so u / 2 is, and
    floor(u / 2) = floor(u) // 2 — the assignment agrees exactly, the fsums to 1e-12.  THERMAL at g = 1 and a uniform temperature is
    c_k sum(w) / expm1(theta_k / T)."""
    n = 5000
    hit, se, g = synthetic_planes(n, np.float64, 7)
    ni, nj, ob = syn_canvas(n)
    em = syn_emission()
    for nb in (64, 250, 1068 * 2):
        fine, idx, counts = np_spectrum(hit, se, g, 1, em, 2.0, rt.Spectrum("line", nb=nb, **SYN_LINE), ob, ni, nj)
        coarse, idx2, counts2 = np_spectrum(hit, se, g, 1, em, 2.0, rt.Spectrum("line", nb=nb // 2, **SYN_LINE), ob, ni, nj)
        assert len(idx) >= n // 2 and np.array_equal(idx, idx2) and np.array_equal(counts[0::2] + counts[1::2], counts2) and counts.max() >= 3
        assert worst(merge_pairs(fine), coarse) <= 1e-12
        _, b1 = np_line_bins(rt.Spectrum("line", nb=nb, **SYN_LINE), g[idx])
        _, b2 = np_line_bins(rt.Spectrum("line", nb=nb // 2, **SYN_LINE), g[idx])
        assert np.array_equal(b1 // 2, b2)
    # THERMAL: g = 1, p = 0 and no inner edge: T = T_in everywhere
    flat = rt.DiskEmission(1, 9000.0, p=0.0, orbit=0.0, emitter="rigid", gain=0.5)
    ones = np.ones(n)
    for kw in (dict(), dict(log=True), dict(nu3=True), dict(log=True, nu3=True)):
        sp = rt.Spectrum("thermal", 3.0e3, 5.0e4, 17, **kw)
        out, idx, _ = np_spectrum(np.ones(n, np.uint32), se, ones, 1, flat, 2.0, sp, ob, ni, nj)
        w, a, b = np_weight(ob, ni, nj)
        theta = np_theta(sp)
        assert theta[0] == 3.0e3 and abs(theta[-1] - 5.0e4) <= 1e-11 and np.all(np.diff(theta) > 0)
        want = np_factor(sp, flat, theta) * math.fsum(w[idx]) / np.expm1(theta / 9000.0)
        assert len(idx) > 0.9 * n and np.abs(out[:, 0] / want - 1).max() <= 1e-12
    assert np_theta(rt.Spectrum("thermal", 7.0, 9.0, 1)).tolist() == [7.0]
    mid = np_theta(rt.Spectrum("thermal", 1.0, 100.0, 3, log=True))
    assert abs(mid[1] - 10.0) <= 1e-14


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def spec_device(lib, metric, objs, em, spec, ob, ni, nj, hit32, se, g, dtype=np.float64, stream=None, fill=-7.0):
    """rtgr_spectrum_device_f64 / _f32 over planes uploaded as torch tensors -> (rc, out [nb, 3])"""
    import torch
    sc = rt.make_scene(metric, objs)
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        d_hit = torch.from_numpy(np.ascontiguousarray(hit32, np.uint32).view(np.int32).copy()).cuda()
        d_se = torch.from_numpy(np.ascontiguousarray(se, dtype).copy()).cuda()
        d_g = torch.from_numpy(np.ascontiguousarray(g, dtype).copy()).cuda()
        d_out = torch.full((int(spec.nb), 3), fill, dtype=torch.float64, device="cuda")
        assert d_se.shape == (ni * nj, 8) and d_hit.shape == (ni * nj,) and d_g.shape == (ni * nj,)
        torch.cuda.synchronize()
        fn = lib.rtgr_spectrum_device_f64 if dtype == np.float64 else lib.rtgr_spectrum_device_f32
        rc = fn(None, C.byref(sc), C.byref(em), C.byref(spec), C.byref(ob) if ob is not None else None, ni, nj, d_hit.data_ptr(), d_se.data_ptr(),
                d_g.data_ptr(), d_out.data_ptr(), stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    return rc, d_out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_hook_against_numpy(lib, dtype):
    """bin exactly — points ON bin edges included —, val to 1e-12 relative (few-ulp pow / expm1), axis to 1e-14 relative"""
    rng = np.random.default_rng(3)
    em = syn_emission()
    for nb in (1, 7, 64, 1000):
        sp = rt.Spectrum("line", nb=nb, **SYN_LINE)
        edges = [sp.lo + b * (sp.hi - sp.lo) / nb for b in (0, 1, nb - 1, nb)] + [np.nextafter(sp.lo, -np.inf), sp.hi, np.nextafter(sp.hi, 0.0)]
        m = 3000
        g = np.concatenate([edges, rng.uniform(0.3, 1.3, m - len(edges))])
        rho, psi = rng.uniform(1.9, 6.4, m), rng.uniform(-math.pi, math.pi, m)
        rho[:len(edges)] = 3.0
        pts = np.column_stack([rho * np.cos(psi), rho * np.sin(psi), g]).astype(dtype)
        pts[-1, 2], pts[-2, 0], pts[-3, 2], pts[-4, 2] = np.nan, np.inf, 0.0, -0.5
        h = rt.eval_spectrum(rt.minkowski, SYN_OBJS, em, sp, pts, dtype=dtype)
        p64 = pts.astype(np.float64)
        ok, r, gg = np_base(np.ones(m, np.uint32), np.column_stack([np.zeros(m), p64[:, 0], p64[:, 1]]), p64[:, 2], 1)
        inb, bins = np_line_bins(sp, gg)
        with np.errstate(invalid="ignore"):
            counts = ok & inb & (r >= sp.rho_min) & (r < sp.rho_max)
        want_bin = np.where(counts, bins, -1)
        assert h["bin"].dtype == np.int64 and np.array_equal(h["bin"], want_bin), (nb, np.flatnonzero(h["bin"] != want_bin)[:5])
        if dtype == np.float64:      # g = lo opens bin 0, just below lo counts nowhere (rounded to Float32 the edge values move: numpy says where to)
            assert h["bin"][0] == 0 and h["bin"][4] == -1
        assert counts.sum() > m // 2 and (h["val"][~counts] == 0).all()
        want_val = np_line_value(sp, r[counts], gg[counts])
        assert np.abs(h["val"][counts] / want_val - 1).max() <= 1e-12
        assert np.abs(h["axis"] / np_axis(sp) - 1).max() <= 1e-14
    for kw in (dict(), dict(log=True), dict(nu3=True, log=True)):
        sp = rt.Spectrum("thermal", SYN_THETA[0], SYN_THETA[1], 33, **kw)
        m = 500
        rho, psi = rng.uniform(1.5, 6.4, m), rng.uniform(-math.pi, math.pi, m)
        pts = np.column_stack([rho * np.cos(psi), rho * np.sin(psi), rng.uniform(0.3, 1.3, m)]).astype(dtype)
        pts[-1, 2], pts[-2, 1] = -1.0, np.nan
        h = rt.eval_spectrum(rt.minkowski, SYN_OBJS, em, sp, pts, dtype=dtype)
        p64 = pts.astype(np.float64)
        ok, r, gg = np_base(np.ones(m, np.uint32), np.column_stack([np.zeros(m), p64[:, 0], p64[:, 1]]), p64[:, 2], 1)
        T = np_temperature(em, 2.0, r)
        with np.errstate(invalid="ignore"):
            counts = ok & (T > 0)
        assert np.array_equal(h["bin"], np.where(counts, 0, -1)) and 0.5 * m < counts.sum() < m - 20      # (inside r_in: T = 0)
        theta = np_theta(sp)
        want = np_factor(sp, em, theta)[None, :] / np.expm1(theta[None, :] / (gg[counts] * T[counts])[:, None])
        assert h["val"].shape == (m, 33) and (h["val"][~counts] == 0).all()
        assert np.abs(h["val"][counts] / want - 1).max() <= 1e-12
        assert np.abs(h["axis"] / theta - 1).max() <= 1e-14
    one = rt.eval_spectrum(rt.minkowski, SYN_OBJS, em, rt.Spectrum("thermal", 4.0e3, 9.0e3, 1))
    assert one["axis"].tolist() == [4.0e3]


SYN_CASES = ([(n, 65) for n in (1, 255, 256, 257, 773)] + [(773, nb) for nb in (1, 63, 64, 255, 256, 257, SPEC_PASS + 44)] +
             [(SPEC_RANGE * LC_MAX_RANGES + 300, 3), (SPEC_RANGE * LC_MAX_RANGES + 300, 257)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("kind", ["line", "thermal"])
@pytest.mark.parametrize("n,nb", SYN_CASES)
def test_synthetic_planes_around_the_kernels_sizes(lib, n, nb, kind, dtype):
    """n around the block's range of SPEC_RANGE pixels, one pixel, a frame of more than SPEC_RANGE x LC_MAX_RANGES pixels (a block then owns
    two ranges); nb around a sub-tile of SPEC_WAVE, a tile of SPEC_TILE, beyond one pass of SPEC_PASS.  Every F, A, B within 1e-9 F of
    numpy's math.fsum: all terms of F are >= 0, a sequential double sum of N <= 2^19 terms errs by <= N 2^-53 ~ 6e-11 relative, pow and
    expm1 add a few ulp.  A bin or sample the judge finds empty is exactly 0.  (The frame of 2^18 + 300 pixels is judged at 3 and at 257
    bins for LINE and at 3 samples for THERMAL: 257 samples would cost the judge 2e8 terms of math.fsum.)  Precondition: at least half
    the pixels count, and for LINE one bin holds >= 3 pixels (one pixel: that pixel counts)."""
    if kind == "thermal" and n > 100000 and nb > 3:
        nb = 5
    hit, se, g = synthetic_planes(n, dtype, seed=n + nb)
    ni, nj, ob = syn_canvas(n)
    em = syn_emission()
    sp = rt.Spectrum("line", nb=nb, **SYN_LINE) if kind == "line" else rt.Spectrum("thermal", SYN_THETA[0], SYN_THETA[1], nb, log=nb % 2 == 1, nu3=nb % 4 == 1)
    want, idx, counts = np_spectrum(hit, se, g, 1, em, 2.0, sp, ob, ni, nj)
    assert 2 * len(idx) >= n, (len(idx), n)
    if kind == "line":
        assert counts.max() >= min(3, n) and (nb < 16 or (counts == 0).any()), counts      # (several pixels in a bin, and bins with none)
    rc, got = spec_device(lib, rt.minkowski, SYN_OBJS, em, sp, ob, ni, nj, hit, se, g, dtype=dtype)
    assert rc == 0
    err = worst(got, want)
    print(f"{kind} {np.dtype(dtype).name} n = {n} nb = {nb}: {len(idx)} counted pixels, worst |out - numpy| / F = {err:.2e}")
    assert err <= 1e-9, err


REAL_LINE = dict(lo=0.0, hi=1.6, nb=64, rho_min=2.0, rho_max=4.0, alpha=3.0, amp=1.0, g_power=4.0)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("proj,size", [("perspective", SIZES[0]), ("equirect", SIZES[1]), ("perspective", SIZES[1]), ("equirect", SIZES[0])])
def test_reduction_against_the_restatement_on_a_real_frame(lib, proj, size, dtype):
    """the light-curve tests' orbiting observer over KerrSchild(1, 0.998) and Disk(0.05, 2, 4): the stage over the frame's own planes, LINE
    over the whole Disk and THERMAL, judged as the synthetic planes are; the traced entry gives the bytes of the stage over its planes"""
    metric, objs = kerr_disk_scene()
    em, ob = rt.DiskEmission(3, T_FRAME), orbiting(proj)
    ni, nj = size
    f = frame(proj, size, dtype)
    for sp in (rt.Spectrum("line", **REAL_LINE), rt.Spectrum("thermal", 5.0e3, 8.0e4, 65, log=True, nu3=True)):
        want, idx, counts = np_spectrum(f["hit32"], f["state_end"], f["g"], 3, em, 2.0, sp, ob, ni, nj)
        assert len(idx) >= 20, len(idx)
        if sp.kind == LINE:
            assert (counts > 0).sum() >= 5, counts
        rc, got = spec_device(lib, metric, objs, em, sp, ob, ni, nj, f["hit32"], f["state_end"], f["g"], dtype=dtype)
        assert rc == 0
        err = worst(got, want)
        print(f"{proj} {ni}x{nj} {np.dtype(dtype).name} kind {sp.kind}: {len(idx)} counted pixels, "
              f"{(counts > 0).sum() if counts is not None else '-'} bins, worst |out - numpy| / F = {err:.2e}")
        assert err <= 1e-9, err
        res = rt.spectrum(metric, objs, ob, ni, nj, em, sp, dtype=dtype)
        assert np.column_stack([res["F"], res["A"], res["B"]]).tobytes() == got.tobytes() and res["g"].tobytes() == f["g"].tobytes()
        assert res["rgb"].tobytes() == f["rgb"].tobytes() and np.abs(res["axis"] / np_axis(sp) - 1).max() <= 1e-14


@pytest.mark.gpu
def test_identities(lib):
    metric, objs = kerr_disk_scene()
    em = rt.DiskEmission(3, T_FRAME)
    worst_tie = {}
    for proj, size in (("perspective", SIZES[0]), ("equirect", SIZES[1])):
        ni, nj = size
        ob = orbiting(proj)
        f = frame(proj, size)
        planes = (f["hit32"], f["state_end"], f["g"])
        # conservation: sum_b F_b = fsum of W over the counted pixels
        sp64 = rt.Spectrum("line", **REAL_LINE)
        rc, fine = spec_device(lib, metric, objs, em, sp64, ob, ni, nj, *planes)
        ok, rho, g = np_base(*planes, 3)
        w, a, b = np_weight(ob, ni, nj)
        inb, _ = np_line_bins(sp64, g)
        sel = ok & inb & (rho >= 2.0) & (rho < 4.0)
        total = math.fsum(w[sel] * np_line_value(sp64, rho[sel], g[sel]))
        assert rc == 0 and sel.sum() >= 20 and abs(math.fsum(fine[:, 0]) / total - 1) <= 1e-9
        # bin merge: 64 bins merged pairwise against 32 bins, to 1e-12 F
        rc, coarse = spec_device(lib, metric, objs, em, rt.Spectrum("line", **dict(REAL_LINE, nb=32)), ob, ni, nj, *planes)
        assert rc == 0 and worst(merge_pairs(fine), coarse) <= 1e-12
        # NU3 multiplies sample k by theta_k^3
        rc1, plain = spec_device(lib, metric, objs, em, rt.Spectrum("thermal", 5.0e3, 8.0e4, 40, log=True), ob, ni, nj, *planes)
        rc2, cubed = spec_device(lib, metric, objs, em, rt.Spectrum("thermal", 5.0e3, 8.0e4, 40, log=True, nu3=True), ob, ni, nj, *planes)
        theta = rt.eval_spectrum(metric, objs, em, rt.Spectrum("thermal", 5.0e3, 8.0e4, 40, log=True))["axis"]
        assert rc1 == 0 and rc2 == 0 and (plain[:, 0] > 0).all()
        scaled = plain * (theta * theta * theta)[:, None]
        assert (np.abs(cubed - scaled) <= 1e-15 * np.abs(scaled)).all()
        # the picture tie: weight_c F(theta = theta_c) = sum_p w_p rgb[c, p] over the disk
        for dtype in (np.float64, np.float32):
            fd = frame(proj, size, dtype)
            on = (fd["hit32"] == 3) & np.isfinite(fd["g"])
            assert on.sum() >= 20
            for c in range(3):
                rc, one = spec_device(lib, metric, objs, em, rt.Spectrum("thermal", em.theta[c], em.theta[c], 1), ob, ni, nj, fd["hit32"], fd["state_end"],
                                      fd["g"], dtype=dtype)
                want = math.fsum(w[on] * fd["rgb"][c, on].astype(np.float64))
                tie = abs(em.weight[c] * one[0, 0] / want - 1)
                worst_tie[np.dtype(dtype).name] = max(worst_tie.get(np.dtype(dtype).name, 0.0), tie)
                assert rc == 0 and want > 0
    print(f"picture tie: Float64 {worst_tie['float64']:.2e}, Float32 {worst_tie['float32']:.2e}")
    assert worst_tie["float64"] <= 1e-9
    # Float32: the picture evaluates T and expm1 in float.  1 / expm1(x) has the condition number x e^x / (e^x - 1) <= x + 1 <= 11 for
    # x = theta_c / (g T) <= 10 here (theta_b = 33014 K, g T >= 0.2 x 17800 K), x carries ~6 float roundings (pow, two products, a division:
    # 6 x 6e-8), expm1f and the final division a few more: 11 x 4e-7 + 3e-7 ~ 5e-6 per pixel at worst, and a weighted mean of
    # per-pixel errors cannot exceed the worst of them.  Measured: 6.8e-8 (Float64: 2.2e-16); profiles/spectrum/README.md.
    assert worst_tie["float32"] <= 1e-5


def flat_opt():
    """(the event search looks at interp_points points per step, and in flat space a step is many units long: tests/test_light_curve.py's
    flat-space check sizes its solver the same way)"""
    opt = rt.solver_defaults()
    opt.interp_points = int(math.ceil((opt.lambda1 - opt.lambda0) / (math.sqrt(2.0) * 0.1))) + 2
    return opt


@pytest.mark.gpu
def test_flat_space_physics(lib):
    ni, nj = SIZES[0]
    sky = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -60.0), rt.Plane(-200.0)]
    # (a) a static disk of one temperature seen by a static observer: g = 1 everywhere — Planck ratios, and one bin
    z0, h = 40.0, 0.25
    tx, ty = h * ni / 2 / z0, h * nj / 2 / z0
    ob = rt.Observer((0, 0, 0, z0), (0, 0, 0, -1), (0, 0, 1, 0), 2 * math.atan(tx), 2 * math.atan(ty))
    objs = sky + [rt.Disk(0.05, 0.001, 8.0)]
    T0 = 9000.0
    em = rt.DiskEmission(3, T0, p=0.0, orbit=0.0, emitter="rigid")
    th = rt.spectrum(rt.minkowski, objs, ob, ni, nj, em, rt.Spectrum("thermal", 3.0e3, 2.0e4, 12), opt=flat_opt(), details=True)
    assert (th["hit"] == 3).all() and np.isfinite(th["g"]).all() and np.abs(th["g"] - 1).max() <= 1e-13
    planck = 1.0 / np.expm1(th["axis"] / T0)
    assert th["F"][0] > 0 and np.abs((th["F"] / th["F"][0]) / (planck / planck[0]) - 1).max() <= 1e-12
    ln = rt.spectrum(rt.minkowski, objs, ob, ni, nj, em, rt.Spectrum("line", 0.5, 1.5, 5, rho_min=0.5, rho_max=8.0), opt=flat_opt())
    assert ln["F"][2] > 0 and (ln["F"][[0, 1, 3, 4]] == 0).all() and (ln["A"][[0, 1, 3, 4]] == 0).all() and (ln["B"][[0, 1, 3, 4]] == 0).all()
    # (b) a rigid rotor seen at an angle: no frequency ratio outside the special-relativistic bounds of the window's fastest gas
    omega, rho_max = 0.1, 6.0
    v = omega * rho_max
    g_lo, g_hi = math.sqrt((1 - v) / (1 + v)), math.sqrt((1 + v) / (1 - v))
    ob = rt.Observer((0, 0, -30, 8), (0, 0, 30, -8), (0, 0, 0, 1), 0.5, 0.35)
    objs = sky + [rt.Disk(0.05, 1.0, 7.0)]
    em = rt.DiskEmission(3, T0, orbit=omega, emitter="rigid")
    sp = rt.Spectrum("line", 0.0, 3.0, 60, rho_min=2.0, rho_max=rho_max, alpha=2.0)
    res = rt.spectrum(rt.minkowski, objs, ob, ni, nj, em, sp, opt=flat_opt())
    edges = sp.lo + np.arange(61) * (sp.hi - sp.lo) / 60
    outside = (edges[1:] <= g_lo) | (edges[:-1] >= g_hi)
    assert outside.sum() >= 20 and (res["F"][outside] == 0).all() and (res["A"][outside] == 0).all() and (res["B"][outside] == 0).all()
    lit = np.flatnonzero(res["F"] > 0)
    print(f"rigid rotor: flux in bins {lit.min()} .. {lit.max()} of 60 over [0, 3); allowed g in [{g_lo:.3f}, {g_hi:.3f}]")
    assert res["F"].sum() > 0 and len(lit) >= 3      # (the Doppler shift spreads the line at all)


@pytest.mark.gpu
def test_schwarzschild_line_seen_from_the_axis(lib):
    """KerrSchild(1, 0), a static observer ON the axis looking down at the disk, the window [6, 8): every photon through an axis point has
    L_z = 0, so g = sqrt(1 - 3 / rho) / sqrt(1 - 2 / r_o) exactly at z = 0.  (Static: at rest against the Killing field d_t — in the
    library's words an observer of kind "velocity" with vel = d_t; its kind "static" is the observer normal to the Kerr-Schild time
    slices, which falls inwards and sees g = 0.78 .. 0.88 here.)  All flux lies in the bins that overlap that interval widened by
    one bin of width 0.01 on each side (the disk's half thickness was estimated to move g by O(h² / rho²) ~ 7e-5; measured: 8.3e-6)."""
    ni, nj = SIZES[0]
    r_o = 30.0
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -60.0), rt.Plane(-200.0), rt.Disk(0.05, 5.0, 9.0)]
    ob = rt.Observer((0, 0, 0, r_o), (0, 0, 0, -1), (0, 0, 1, 0), 2 * math.atan(9.5 / r_o), 2 * math.atan(9.5 / r_o), kind="velocity", vel=(1, 0, 0, 0))
    em = rt.DiskEmission(3, T_FRAME)
    sp = rt.Spectrum("line", 0.0, 1.6, 160, rho_min=6.0, rho_max=8.0, alpha=3.0)
    res = rt.spectrum(rt.KerrSchild(1, 0.0), objs, ob, ni, nj, em, sp, details=True)
    g_of = lambda rho: math.sqrt(1 - 3 / rho) / math.sqrt(1 - 2 / r_o)
    lo, hi = g_of(6.0) - 0.01, g_of(8.0) + 0.01
    edges = np.arange(161) * 0.01
    allowed = (edges[1:] > lo) & (edges[:-1] < hi)
    rho = np.hypot(res["state_end"][:, 1], res["state_end"][:, 2])
    inwin = (res["hit"] == 3) & np.isfinite(res["g"]) & (rho >= 6.0) & (rho < 8.0)
    shift = np.abs(res["g"][inwin] - np.sqrt(1 - 3 / rho[inwin]) / math.sqrt(1 - 2 / r_o)).max()
    print(f"axis view: {inwin.sum()} pixels in the window, flux in bins {np.flatnonzero(res['F'] > 0).tolist()}, allowed "
          f"{np.flatnonzero(allowed).tolist()}, worst |g - closed form| = {shift:.2e}")
    assert inwin.sum() >= 50 and res["F"].sum() > 0
    assert (res["F"][~allowed] == 0).all() and (res["F"][allowed] > 0).sum() >= 5


def trace_spec_device(lib, metric, objs, ob, ni, nj, em, sp, dtype=np.float64, stream=None, want_out=True, want_g=True, want_ctr=True):
    """rtgr_trace_spectrum_device_* with torch planes -> (rc, dict of numpy arrays)"""
    import torch
    from test_textures import _outputs
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    td = torch.float64 if dtype == np.float64 else torch.float32
    ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
    with ctx:
        rgb = torch.full((3, n), -5.0, dtype=td, device="cuda")
        g = torch.full((n,), -5.0, dtype=td, device="cuda")
        out = torch.full((int(sp.nb), 3), -7.0, dtype=torch.float64, device="cuda")
        dev = _outputs(n, dtype, device=True)
        o = abi.rtgr_ray_outputs()
        for key in OUT_KEYS:
            setattr(o, key, dev[key].data_ptr())
        ctr = abi.rtgr_counters()
        torch.cuda.synchronize()
        fn = lib.rtgr_trace_spectrum_device_f64 if dtype == np.float64 else lib.rtgr_trace_spectrum_device_f32
        rc = fn(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, C.byref(em), C.byref(sp), rgb.data_ptr(), C.byref(o) if want_out else None,
                g.data_ptr() if want_g else None, out.data_ptr(), C.byref(ctr) if want_ctr else None, stream.cuda_stream if stream is not None else None)
    torch.cuda.synchronize()
    res = dict(rgb=rgb.cpu().numpy(), g=g.cpu().numpy(), out=out.cpu().numpy(), counters=ctr.as_dict())
    res.update({k: v.cpu().numpy() for k, v in dev.items()})
    return rc, res


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["line", "thermal"])
def test_determinism_streams_and_batches(lib, kind):
    import torch
    metric, objs = kerr_disk_scene()
    em = rt.DiskEmission(3, T_FRAME)
    ni, nj = SIZES[0]
    sp = rt.Spectrum("line", **REAL_LINE) if kind == "line" else rt.Spectrum("thermal", 5.0e3, 8.0e4, 130, log=True)
    side = torch.cuda.Stream()
    rc, first = trace_spec_device(lib, metric, objs, orbiting(), ni, nj, em, sp)
    assert rc == 0 and (first["out"][:, 0] > 0).sum() >= 5
    for stream, batch, bare in ((None, 0, False), (side, 0, False), (side, 0, True), (None, ni, False), (side, 5 * ni, False), (None, 5 * ni, True)):
        rc, again = trace_spec_device(lib, metric, objs, orbiting(max_batch_rays=batch), ni, nj, em, sp, stream=stream, want_out=not bare, want_g=not bare,
                                      want_ctr=not bare)
        assert rc == 0 and again["out"].tobytes() == first["out"].tobytes(), (stream is not None, batch, bare)
    f = frame("perspective", SIZES[0])
    for stream in (None, side, None):
        rc, out = spec_device(lib, metric, objs, em, sp, orbiting(), ni, nj, f["hit32"], f["state_end"], f["g"], stream=stream)
        assert rc == 0 and out.tobytes() == first["out"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_trace_is_untouched(lib, dtype):
    """rgb, g, every per-ray output and the counters of rt.spectrum(..., details=True) == rt.trace_observer's with the same emit, bit for bit"""
    metric, objs = kerr_disk_scene()
    em = rt.DiskEmission(3, T_FRAME)
    for (ni, nj), proj, sp in ((SIZES[0], "perspective", rt.Spectrum("line", **REAL_LINE)), (SIZES[1], "equirect", rt.Spectrum("thermal", 5.0e3, 8.0e4, 9))):
        ob = orbiting(proj, 200)
        want = rt.trace_observer(metric, objs, ob, ni, nj, emission=em, dtype=dtype, details=True)
        got = rt.spectrum(metric, objs, ob, ni, nj, em, sp, dtype=dtype, details=True)
        keys = [k for k in want if isinstance(want[k], np.ndarray)]
        assert set(keys) >= {"rgb", "g", "state_end", "lambda_end", "status", "hit", "n_accept", "n_reject"}
        for key in keys:
            assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (key, proj, dtype)
        assert got["counters"] == want["counters"] and (got["F"] > 0).any()


@pytest.mark.gpu
def test_refusals(lib):
    """Every refusal: RTGR_ERR_BAD_ARG with a message naming the field, the output (and rgb) untouched."""
    import torch
    from test_grid_metric import ETA
    from test_grid_metric_4d import grid4
    metric, objs = kerr_disk_scene()
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ni, nj = 8, 6
    n = ni * nj
    rgb = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
    out = torch.full((4, 3), -7.0, dtype=torch.float64, device="cuda")
    hit = torch.zeros(n, dtype=torch.int32, device="cuda")
    se = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    g = torch.zeros(n, dtype=torch.float64, device="cuda")
    h_rgb, h_out = np.full((3, n), -5.0), np.full((4, 3), -7.0)
    nan, inf = math.nan, math.inf

    def call(kind="line", scene=sc, emit=True, spec=True, obs=True, planes=(True, True, True), have_out=True, em_over=None, ob_over=None, **over):
        ob = orbiting()
        for key, val in (ob_over or {}).items():
            setattr(ob, key, val)
        em = rt.DiskEmission(3, T_FRAME)
        for key, val in (em_over or {}).items():
            setattr(em, key, val)
        sp = rt.Spectrum("line", **dict(REAL_LINE, nb=4)) if kind == "line" else rt.Spectrum("thermal", 5.0e3, 8.0e4, 4)
        for key, val in over.items():
            setattr(sp, key, val)
        emp, spp, obp = C.byref(em) if emit else None, C.byref(sp) if spec else None, C.byref(ob) if obs else None
        rcs, msgs = [], []
        if obs or planes != (True, True, True):      # (the stage alone takes obs = NULL: the plane camera)
            rcs.append(lib.rtgr_spectrum_device_f64(None, C.byref(scene), emp, spp, obp, ni, nj, hit.data_ptr() if planes[0] else None,
                                                    se.data_ptr() if planes[1] else None, g.data_ptr() if planes[2] else None,
                                                    out.data_ptr() if have_out else None, None))
            msgs.append(lib.rtgr_last_error())
        if planes == (True, True, True):
            rcs.append(lib.rtgr_trace_spectrum_device_f64(None, C.byref(scene), C.byref(opt), obp, ni, nj, None, emp, spp, rgb.data_ptr(), None, None,
                                                          out.data_ptr() if have_out else None, None, None))
            msgs.append(lib.rtgr_last_error())
            rcs.append(lib.rtgr_trace_spectrum_f64(None, C.byref(scene), C.byref(opt), obp, ni, nj, None, emp, spp, h_rgb.ctypes.data, None, None,
                                                   h_out.ctypes.data if have_out else None, None))
            msgs.append(lib.rtgr_last_error())
            if obs and have_out and not ob_over:
                axis, pts, bins, val = np.full(4, -3.0), np.zeros((2, 3)), np.full(2, -3, np.int64), np.full(8, -3.0)
                rcs.append(lib.rtgr_eval_spectrum_f64(None, C.byref(scene), emp, spp, pts.ctypes.data, 2, axis.ctypes.data, bins.ctypes.data, val.ctypes.data))
                msgs.append(lib.rtgr_last_error())
                assert rcs[-1] == 0 or ((axis == -3.0).all() and (bins == -3).all() and (val == -3.0).all())
        return rcs, msgs

    user = rt.make_scene(metric, objs)
    user.metric = abi.USER
    cases = [(dict(emit=False), b"emit"), (dict(spec=False), b"rtgr_spectrum is NULL"), (dict(have_out=False), b"output (spectrum) is NULL"),
             (dict(planes=(False, True, True)), b"hit32 is NULL"), (dict(planes=(True, False, True)), b"state_end is NULL"), (dict(planes=(True, True, False)), b"g is NULL"),
             (dict(nb=0), b"nb"), (dict(nb=(1 << 16) + 1), b"nb"), (dict(flags=4), b"flags"), (dict(flags=abi.SPEC_LOG), b"flags"),
             (dict(flags=abi.SPEC_NU3), b"flags"), (dict(reserved=1.0), b"reserved"), (dict(reserved=nan), b"reserved"),
             (dict(lo=nan), b"lo"), (dict(hi=inf), b"hi"), (dict(amp=nan), b"amp"), (dict(alpha=inf), b"alpha"), (dict(rho_min=nan), b"rho_min"),
             (dict(rho_max=inf), b"rho_max"), (dict(g_power=nan), b"g_power"),
             (dict(amp=-0.1), b"amp"), (dict(rho_min=1.9), b"[r_in, r_out]"), (dict(rho_max=4.1), b"[r_in, r_out]"), (dict(rho_min=3.0, rho_max=3.0), b"rho_min"),
             (dict(rho_min=3.5, rho_max=2.5), b"rho_min"), (dict(rho_min=0.0), b"rho_min"), (dict(rho_min=-1.0), b"rho_min"), (dict(lo=-0.1), b"lo"),
             (dict(lo=1.6), b"lo"), (dict(lo=2.0), b"lo"),
             (dict(kind="thermal", lo=0.0), b"lo"), (dict(kind="thermal", lo=-1.0), b"lo"), (dict(kind="thermal", lo=9.0e4), b"lo"), (dict(kind="thermal", hi=nan), b"hi"),
             (dict(kind="thermal", amp=1.0), b"amp"), (dict(kind="thermal", alpha=1.0), b"alpha"), (dict(kind="thermal", rho_min=2.0), b"rho_min"),
             (dict(kind="thermal", rho_max=4.0), b"rho_max"), (dict(kind="thermal", g_power=4.0), b"g_power"), (dict(kind="thermal", flags=4), b"flags"),
             (dict(kind="thermal", reserved=-1.0), b"reserved"), (dict(kind="thermal", nb=0), b"nb"),
             (dict(scene=user), b"RTGR_USER"), (dict(em_over=dict(object=1)), b"Sphere"), (dict(em_over=dict(orbit=0.5)), b"+1"),
             (dict(em_over=dict(T_in=0.0)), b"T_in"), (dict(ob_over=dict(kind=3)), b"unknown rtgr_observer.kind"), (dict(ob_over=dict(fov_x=4.0)), b"(0, pi)"),
             (dict(ob_over=dict(pad=1)), b"pad")]
    for kw, word in cases:
        rcs, msgs = call(**kw)
        assert rcs and rcs == [abi.ERR_BAD_ARG] * len(rcs) and all(word in m for m in msgs), (kw, rcs, msgs)
    # an unknown kind
    sp = rt.Spectrum("line", **dict(REAL_LINE, nb=4))
    sp.kind = 2
    em, ob = rt.DiskEmission(3, T_FRAME), orbiting()
    assert lib.rtgr_spectrum_device_f64(None, C.byref(sc), C.byref(em), C.byref(sp), C.byref(ob), ni, nj, hit.data_ptr(), se.data_ptr(), g.data_ptr(),
                                        out.data_ptr(), None) == abi.ERR_BAD_ARG and b"rtgr_spectrum.kind" in lib.rtgr_last_error()
    assert lib.rtgr_trace_spectrum_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, C.byref(em), C.byref(sp), h_rgb.ctypes.data, None, None,
                                       h_out.ctypes.data, None) == abi.ERR_BAD_ARG and b"rtgr_spectrum.kind" in lib.rtgr_last_error()
    # the hook's own limit
    pts = np.zeros((3, 3))
    big = rt.Spectrum("thermal", 5.0e3, 8.0e4, 1 << 16)
    assert lib.rtgr_eval_spectrum_f64(None, C.byref(sc), C.byref(em), C.byref(big), pts.ctypes.data, (1 << 10) + 1, None, None, None) == abi.ERR_BAD_ARG
    assert b"2^26" in lib.rtgr_last_error()
    # the traced entries need their observer
    ob_none = call(obs=False)
    assert ob_none[0] == [abi.ERR_BAD_ARG] * 2 and all(b"rtgr_observer is NULL" in m for m in ob_none[1])
    # a time-dependent grid
    flat4 = grid4(np.broadcast_to(ETA, (6, 6, 6, 10)).copy(), 4, -1.0, 1.0, (-3.0,) * 3, 1.0, name="flat4")
    g4 = rt.make_scene(flat4, [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(-20.0), rt.Disk(0.05, 2.0, 4.0)])
    rcs, msgs = call(scene=g4, ob_over=dict(kind=0))
    assert rcs == [abi.ERR_BAD_ARG] * 3 and all(b"4-D" in m for m in msgs), (rcs, msgs)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((rgb == -5.0).all()) and (h_out == -7.0).all() and (h_rgb == -5.0).all()
    # … and the same calls with nothing wrong are served: a window at the edges of the Disk's range, lo = hi for THERMAL
    for kw in (dict(), dict(kind="thermal"), dict(kind="thermal", hi=5.0e3), dict(kind="thermal", flags=3)):
        rcs, _ = call(**kw)
        assert rcs == [0, 0, 0, 0], kw
    torch.cuda.synchronize()
    assert not bool((out == -7.0).any()) and not (h_out == -7.0).any() and out[:, 0].cpu().numpy().tobytes() == h_out[:, 0].tobytes()


@pytest.mark.gpu
def test_capture_replay_and_trim(lib):
    """ctr == NULL: both device entries are captured once workspace and scratch exist, replay the eager spectrum to the bit, refuse to grow
    the scratch or to deliver counters during capture; rtgr_trim afterwards, and a fresh call gives the same"""
    import torch
    from test_textures import _hip_runtime
    metric, objs = kerr_disk_scene()
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    em = rt.DiskEmission(3, T_FRAME)
    ni, nj = SIZES[1]
    n = ni * nj
    ob = orbiting("equirect", 200)
    sp, sp_long = rt.Spectrum("line", **REAL_LINE), rt.Spectrum("line", **dict(REAL_LINE, nb=3000))
    nb = int(sp.nb)
    side = torch.cuda.Stream()
    hip = _hip_runtime()

    def traced(rgb, out, spec=sp, ctr=None):
        return lib.rtgr_trace_spectrum_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, C.byref(em), C.byref(spec), rgb.data_ptr(),
                                                  None, None, out.data_ptr(), C.byref(ctr) if ctr is not None else None, side.cuda_stream)

    f = frame("equirect", SIZES[1])
    with torch.cuda.stream(side):
        d_hit = torch.from_numpy(f["hit32"].view(np.int32).copy()).cuda()
        d_se, d_g = torch.from_numpy(f["state_end"].copy()).cuda(), torch.from_numpy(f["g"].copy()).cuda()
        rgb_eager, rgb_out = (torch.zeros((3, n), dtype=torch.float64, device="cuda") for _ in range(2))
        out_eager, out_graph, out_alone, out_fresh = (torch.zeros((nb, 3), dtype=torch.float64, device="cuda") for _ in range(4))
        out_long = torch.zeros((3000, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def alone(out, spec=sp):
        return lib.rtgr_spectrum_device_f64(None, C.byref(sc), C.byref(em), C.byref(spec), C.byref(ob), ni, nj, d_hit.data_ptr(), d_se.data_ptr(),
                                            d_g.data_ptr(), out.data_ptr(), side.cuda_stream)

    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, traced(rgb_eager, out_eager))                # the warm-up: workspace and scratch of this size exist afterwards
    torch.cuda.synchronize()
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc_big = traced(rgb_out, out_long, spec=sp_long)            # more bins: the scratch would have to grow
    msg_big = lib.rtgr_last_error()
    rc_big2 = alone(out_long, spec=sp_long)
    msg_big2 = lib.rtgr_last_error()
    rc_ctr = traced(rgb_out, out_graph, ctr=abi.rtgr_counters())  # counters need a synchronisation
    msg_ctr = lib.rtgr_last_error()
    rc = traced(rgb_out, out_graph)
    rc2 = alone(out_alone)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert rc == 0 and rc2 == 0 and rc_ctr == abi.ERR_BAD_ARG and b"ctr" in msg_ctr
    assert rc_big == abi.ERR_BAD_ARG and b"captured" in msg_big and rc_big2 == abi.ERR_BAD_ARG and b"captured" in msg_big2
    assert graph.value and hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(rgb_out, rgb_eager) and torch.equal(out_graph, out_eager) and torch.equal(out_alone, out_eager) and int((out_eager[:, 0] > 0).sum()) >= 5
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, traced(rgb_out, out_fresh))
    torch.cuda.synchronize()
    assert torch.equal(out_fresh, out_eager)
    want, idx, _ = np_spectrum(f["hit32"], f["state_end"], f["g"], 3, em, 2.0, sp, ob, ni, nj)
    assert len(idx) >= 20 and worst(out_fresh.cpu().numpy(), want) <= 1e-9
