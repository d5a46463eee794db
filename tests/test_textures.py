"""Image textures for spheres, disks and escaping rays (rtgr_texture_*, rtgr_trace_shaded_*, rtgr_eval_texture_*; include/rtgr.h).

The reference has no textures, so the judges are (1) numpy, for the mapping and the sampler as the header states them, and (2) the
library's own PLAIN frame (which the oracle pins), for everything a shaded trace does around the sampler:
    shaded rgb  ==  where(mask, rtgr_eval_texture(coords), plain rgb)                      bit for bit,
mask and coords computed by numpy from the plain call's state_end / hit32 / status by the header's rule, every per-ray output equal to
the plain call's.  With anti-aliasing: uniform == the box filter of the shaded fine frame, refined == the edge rule on the shaded frame,
adaptive == where(refined, uniform, shaded plain).  CPU part: symbols, struct layouts (ctypes and a compiled C caller), no result
without a device, the Julia stub."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from scenes import many_objects, rt

abi = rt._abi
TEX_EXPORTS = ("rtgr_texture_load", "rtgr_texture_unload", "rtgr_trace_shaded_device_f64", "rtgr_trace_shaded_device_f32",
               "rtgr_trace_shaded_f64", "rtgr_trace_shaded_f32", "rtgr_eval_texture_f64", "rtgr_eval_texture_f32")
OUT_KEYS = ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject", "hit32")
NEAREST, BILINEAR = abi.TEX_NEAREST, abi.TEX_BILINEAR


# ---- the header's formulas in numpy (float64) ---------------------------------------------------------------------------------------------
def coords_direction(d, W, H):
    d = np.asarray(d, np.float64)
    theta = np.arctan2(np.hypot(d[:, 0], d[:, 1]), d[:, 2])
    phi = np.arctan2(d[:, 1], d[:, 0])
    return (phi + np.pi) * W / (2 * np.pi) - 0.5, theta * H / np.pi - 0.5


def coords_disk(x, W, H, r_in, r_out):
    x = np.asarray(x, np.float64)
    phi = np.arctan2(x[:, 1], x[:, 0])
    return (phi + np.pi) * W / (2 * np.pi) - 0.5, (np.hypot(x[:, 0], x[:, 1]) - r_in) / (r_out - r_in) * H - 0.5


def np_nearest(tex, s, v):
    """tex (3, H, W) -> [n, 3]: column floor(s + 1/2) mod W, row clamp(floor(v + 1/2), 0, H - 1)"""
    _, H, W = tex.shape
    q = np.floor(s + 0.5).astype(np.int64) % W
    r = np.clip(np.floor(v + 0.5), 0, H - 1).astype(np.int64)
    return tex[:, r, q].T


def np_bilinear(tex, s, v):
    _, H, W = tex.shape
    q0, r0 = np.floor(s), np.floor(v)
    fx, fy = s - q0, v - r0
    c0, c1 = q0.astype(np.int64) % W, (q0.astype(np.int64) + 1) % W
    ra, rb = np.clip(r0, 0, H - 1).astype(np.int64), np.clip(r0 + 1, 0, H - 1).astype(np.int64)
    t00, t10, t01, t11 = tex[:, ra, c0], tex[:, ra, c1], tex[:, rb, c0], tex[:, rb, c1]
    a = t00 + fx * (t10 - t00)
    b = t01 + fx * (t11 - t01)
    return (a + fy * (b - a)).T


def boundary_distance(s, v):
    """distance (in texels) of (s, v) from the nearest boundary between two texels of the NEAREST rule"""
    fs, fv = (s + 0.5) - np.floor(s + 0.5), (v + 0.5) - np.floor(v + 0.5)
    return np.minimum(np.minimum(fs, 1 - fs), np.minimum(fv, 1 - fv))


def tol_of(tex, dtype):
    """64 max(W, H) eps(R) (max - min): a few ulp of pi from each atan2 and from the affine map move s by about 8 eps W, the interpolant's
    slope in s is at most one neighbour difference, and an 8 x margin on top"""
    _, H, W = tex.shape
    return 64 * max(W, H) * float(np.finfo(dtype).eps) * float(tex.max() - tex.min())


W0, H0, NVEC, SEED = 16, 8, 4096, 28


def sample_vectors(dtype):
    """n = 4096 seeded random unit vectors, the six axis directions (both poles among them) and vectors on either side of the seam
    phi = +-pi, rounded to `dtype`"""
    rng = np.random.default_rng(SEED)
    d = rng.normal(size=(NVEC, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    seam = np.array([[-1.0, sgn * dy, z] for dy in (1e-2, 1e-4, 0.0) for sgn in (1, -1) for z in (0.0, 0.4, -2.0)])
    return np.ascontiguousarray(np.concatenate([d, axes, seam]).astype(dtype))


def random_texture(W, H, seed=3):
    return np.random.default_rng(seed).uniform(0.0, 1.0, size=(3, H, W))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(TEX_EXPORTS) <= set(abi.EXPORTS)
    lib = abi.load()
    for s in TEX_EXPORTS:
        assert hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    for s in TEX_EXPORTS:
        assert s + "(" in hdr, s
    assert "never coincide with grid ids or unit ids" in hdr                        # the header states the id rule …
    for words in ("mip-mapping", "pole-aware bilinear", "planes and user objects", "no asymptotic correction", "dimming is not applied",
                  "comes back to the bit", "not acos"):
        assert words in hdr, words                                                  # … the contract and what is out of scope
    dev = open(os.path.join(ROOT, "raytracegr.jl_amd", "csrc", "rtgr_texture.hpp")).read()
    for words in ("Do not use `acos`: it is ill-conditioned at the poles.", "Column floor(s + ½) mod W.", "clamped at the poles and rims, not reflected",
                  "A constant texture comes back", "no asymptotic correction"):
        assert words in dev, words


def _c_caller(tmp_path):
    exe = str(tmp_path / "texture_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "texture_layout.c"), "-o", exe, "-ldl"])
    return exe


def test_struct_layouts_in_ctypes_and_in_a_compiled_c_caller(tmp_path):
    d, b, s = abi.rtgr_texture_desc, abi.rtgr_texture_bind, abi.rtgr_shade
    assert C.sizeof(d) == 16 and (d.width.offset, d.height.offset, d.flags.offset, d.pad.offset) == (0, 4, 8, 12)
    assert C.sizeof(b) == 16 and (b.object.offset, b.filter.offset, b.texture.offset) == (0, 4, 8)
    assert C.sizeof(s) == 24 and (s.nbind.offset, s.flags.offset, s.bind.offset, s.r_escape.offset) == (0, 4, 8, 16)
    assert abi.RTGR_MAX_TEXTURE_BINDS == 16 and (abi.TEX_NEAREST, abi.TEX_BILINEAR) == (0, 1)
    out = subprocess.check_output([_c_caller(tmp_path)], text=True).split()
    assert dict(zip(out[0::2], map(int, out[1::2]))) == {"desc": 16, "width": 0, "height": 4, "flags": 8, "pad": 12, "bind": 16, "object": 0,
                                                         "filter": 4, "texture": 8, "shade": 24, "nbind": 0, "sflags": 4, "sbind": 8, "r_escape": 16}


def test_no_result_without_a_device(tmp_path):
    """Without a HIP device every new compute entry FAILS with RTGR_ERR_NO_DEVICE and leaves the caller's arrays alone — from a compiled
    C caller (load, the host-pointer trace, the sampler hook) and through ctypes (all eight)."""
    import torch
    res = subprocess.run([_c_caller(tmp_path), abi.LIB_PATH], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)       # (2: a symbol does not resolve)
    w = res.stdout.split("\n")[1].split()
    got = tuple(int(w[k]) for k in (1, 3, 5, 7, 9))                # load, id written, shaded, eval, touched
    nd = abi.ERR_NO_DEVICE
    assert got in ((nd, 0, nd, nd, 0), (0, 1, 0, abi.ERR_BAD_ARG, 1)), got     # (with a device: texture id 0 is unknown to the hook)
    if torch.cuda.is_available():
        return
    assert got == (nd, 0, nd, nd, 0)
    lib = abi.load()
    sc, opt = rt.make_scene(rt.minkowski, []), rt.solver_defaults()
    cam = rt.make_camera(**rt.example1_scene()[2])
    tex = np.zeros((3, 2, 2))
    desc, tid = abi.rtgr_texture_desc(width=2, height=2), C.c_uint64(77)
    assert lib.rtgr_texture_load(None, C.byref(desc), tex.ctypes.data, C.byref(tid)) == nd and tid.value == 77
    assert b"no CPU fallback" in lib.rtgr_last_error()
    assert lib.rtgr_texture_unload(None, 0) == nd
    sh = rt.make_shade({})
    for dtype, suf in ((np.float64, "f64"), (np.float32, "f32")):
        rgb = np.full((3, 4), -7.0, dtype)
        rc = getattr(lib, "rtgr_trace_shaded_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(cam), 2, 2, C.byref(sh), None, rgb.ctypes.data, None, None,
                                                      None, None)
        assert rc == nd and b"no CPU fallback" in lib.rtgr_last_error() and (rgb == -7.0).all()
        rc = getattr(lib, "rtgr_trace_shaded_device_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(cam), 2, 2, C.byref(sh), None, rgb.ctypes.data, None,
                                                             None, None, None, None)
        assert rc == nd and (rgb == -7.0).all()
        p, col = np.ones((1, 3), dtype), np.full((1, 3), -7.0, dtype)
        assert getattr(lib, "rtgr_eval_texture_" + suf)(None, 1, 0, p.ctypes.data, 1, None, col.ctypes.data) == nd and (col == -7.0).all()
    with pytest.raises(abi.RtgrError):
        rt.texture_load(tex)
    with pytest.raises(abi.RtgrError):
        rt.trace_shaded(rt.minkowski, [], rt.example1_scene()[2], 2, 2)


def test_julia_stub_names_the_symbols_and_layouts():
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    for line in ("#   RtgrTextureDesc  16   width 0, height 4, flags 8, pad 12", "#   RtgrTextureBind  16   object 0, filter 4, texture 8",
                 "#   RtgrShade        24   nbind 0, flags 4, bind 8, r_escape 16"):
        assert line in jl, line
    for word in (":rtgr_texture_load", ":rtgr_texture_unload", ":rtgr_trace_shaded_f64", ":rtgr_trace_shaded_f32", "function load_texture(",
                 "function trace_rays_shaded(", "struct RtgrShade", "const RTGR_TEX_BILINEAR = UInt32(1)"):
        assert word in jl, word


def test_the_seed_keeps_the_nearest_filter_under_one_percent():
    """(CPU: the vectors of the NEAREST test and the rule that drops those within 1e-6 texel of a texel boundary)"""
    for dtype in (np.float64, np.float32):
        s, v = coords_direction(sample_vectors(dtype), W0, H0)
        keep = boundary_distance(s, v) >= 1e-6
        assert 0.99 * len(keep) < keep.sum() < len(keep)      # (the axis directions and the seam vectors sit ON boundaries)
        # … and no kept vector is so close that Float32's own rounding of s (a few eps32 W) could decide the texel
        assert boundary_distance(s, v)[keep].min() > 1e-4


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


_TEX = {}


def texture(name):
    """textures the tests share: (planes (3, H, W) float64, Texture), loaded once"""
    if name not in _TEX:
        if name == "rand16x8":
            t = random_texture(W0, H0)
        elif name == "rand32x16":
            t = random_texture(32, 16, seed=5)
        elif name == "const":
            t = np.broadcast_to(np.array([0.1, 1.0 / 3.0, 0.7])[:, None, None], (3, H0, W0)).copy()
        elif name == "ramp":                       # linear in the column index, the same in every row and channel
            t = np.broadcast_to((np.arange(W0) / W0)[None, None, :], (3, H0, W0)).copy()
        else:
            raise KeyError(name)
        t.setflags(write=False)
        _TEX[name] = (t, rt.texture_load(t))
    return _TEX[name]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nearest_is_the_numpy_lookup_bit_for_bit(lib, dtype):
    t, tex = texture("rand16x8")
    d = sample_vectors(dtype)
    s, v = coords_direction(d, W0, H0)
    keep = boundary_distance(s, v) >= 1e-6
    assert keep.sum() > 0.99 * len(keep)
    got = rt.eval_texture(tex, d, NEAREST, dtype=dtype)
    want = np_nearest(t, s, v).astype(dtype)                  # (f32: the texel rounded to float once)
    assert np.isfinite(got).all()                             # every vector is sampled, the dropped ones too
    assert same_bits(np.ascontiguousarray(got[keep]), np.ascontiguousarray(want[keep]))
    # a zero or non-finite d is "no sample": the entry keeps what the caller put there
    bad = np.array([[0, 0, 0], [np.nan, 1, 0], [1, np.inf, 0], [0, 0, -np.inf], [0.0, -0.0, 0.0]], dtype)
    pre = np.full((len(bad), 3), -3.0, dtype)
    for filt in (NEAREST, BILINEAR):
        assert same_bits(rt.eval_texture(tex, bad, filt, rgb=pre, dtype=dtype), pre)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_bilinear_is_the_stated_formula(lib, dtype):
    t, tex = texture("rand16x8")
    d = sample_vectors(dtype)
    s, v = coords_direction(d, W0, H0)
    tol = tol_of(t, dtype)
    got = rt.eval_texture(tex, d, BILINEAR, dtype=dtype)
    err = np.abs(got.astype(np.float64) - np_bilinear(t, s, v)).max()
    print(f"bilinear {np.dtype(dtype).name}: max error {err:.3e}, tol {tol:.3e}")
    assert err <= tol
    # a constant texture comes back exactly
    tc, texc = texture("const")
    got = rt.eval_texture(texc, d, BILINEAR, dtype=dtype)
    assert same_bits(got, np.ascontiguousarray(np.broadcast_to(tc[:, 0, 0].astype(dtype), got.shape)))
    # a texture linear in the column index comes back linear in phi, away from the seam
    tr, texr = texture("ramp")
    got = rt.eval_texture(texr, d, BILINEAR, dtype=dtype).astype(np.float64)
    inner = (s >= 0.0) & (s <= W0 - 1.0)
    assert inner.sum() > 3000
    err = np.abs(got[inner] - (s[inner] / W0)[:, None]).max()
    print(f"ramp {np.dtype(dtype).name}: max error {err:.3e}, tol {tol_of(tr, dtype):.3e}")
    assert err <= tol_of(tr, dtype)
    # continuity across the wrap: just below +pi and just above -pi
    delta = 1e-7 if dtype == np.float64 else 1e-3
    z = np.linspace(-2.0, 2.0, 41)
    up = np.stack([-np.cos(delta) * np.ones_like(z), np.sin(delta) * np.ones_like(z), z], axis=1).astype(dtype)
    dn = up * np.array([1, -1, 1], dtype)
    a, b = rt.eval_texture(tex, up, BILINEAR, dtype=dtype), rt.eval_texture(tex, dn, BILINEAR, dtype=dtype)
    ds = 2 * np.arctan2(up[:, 1].astype(np.float64), -up[:, 0].astype(np.float64)).max() * W0 / (2 * np.pi)     # the pair's distance in s
    assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() <= tol + ds * float(t.max() - t.min())
    assert np.abs(a.astype(np.float64) - b.astype(np.float64)).max() < 1e-2 * float(t.max() - t.min())      # (not a jump across the image)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_disk_mapping(lib, dtype):
    """rho inside, at and outside [r_in, r_out]: the rows clamp at the rims"""
    t, tex = texture("rand16x8")
    r_in, r_out = 2.0, 4.0
    rng = np.random.default_rng(11)
    rho = np.concatenate([rng.uniform(2.0, 4.0, 600), rng.uniform(0.1, 2.0, 100), rng.uniform(4.0, 9.0, 100), [2.0, 4.0, 3.0, 1e-3, 1e6]])
    phi = rng.uniform(-np.pi, np.pi, len(rho))
    x = np.ascontiguousarray(np.stack([rho * np.cos(phi), rho * np.sin(phi), rng.normal(size=len(rho))], axis=1).astype(dtype))
    s, v = coords_disk(x, W0, H0, r_in, r_out)
    assert (v < -0.5).any() and (v > H0 - 0.5).any()
    got = rt.eval_texture(tex, x, BILINEAR, disk_range=(r_in, r_out), dtype=dtype)
    err = np.abs(got.astype(np.float64) - np_bilinear(t, s, v)).max()
    print(f"disk bilinear {np.dtype(dtype).name}: max error {err:.3e}, tol {tol_of(t, dtype):.3e}")
    assert err <= tol_of(t, dtype)
    keep = boundary_distance(s, v) >= (1e-6 if dtype == np.float64 else 1e-4)
    assert keep.sum() > 0.97 * len(keep)
    got = rt.eval_texture(tex, x, NEAREST, disk_range=(r_in, r_out), dtype=dtype)
    assert same_bits(np.ascontiguousarray(got[keep]), np.ascontiguousarray(np_nearest(t, s, v).astype(dtype)[keep]))
    # the z component is not read
    x2 = x.copy()
    x2[:, 2] = np.nan
    assert same_bits(rt.eval_texture(tex, x2, NEAREST, disk_range=(r_in, r_out), dtype=dtype), got)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
def _scene(name):
    """(metric, objs, rtgr_camera, solver overrides)"""
    metric, objs, cam = rt.example2_scene()
    over = {}
    if name == "disk":
        metric, objs = rt.KerrSchild(1.0, 0.8), objs[:2] + [rt.Disk(0.05, 2.0, 4.0)]
    elif name == "ex2_nosky":            # example2 without caelum: the far plane t = -20 still ends every ray (no escape)
        objs, over = objs[1:], dict(miss_rgb=(0.0, 0.0, 0.0))
    elif name == "ex2_open":             # … and without the far plane: rays that miss the sphere run to lambda1 or into the hole
        objs, over = objs[2:], dict(miss_rgb=(0.0, 0.0, 0.0))
    elif name == "many40":               # a 40-object list; object 37 is the sphere many_objects puts in front of the camera
        objs = many_objects(40)
        objs[36], objs[39] = objs[39], objs[36]
    elif name == "mink0":
        metric, objs = rt.minkowski, []
    elif name == "grid":
        from test_grid_metric import kerr_schild_island, ks_grid, ks_scene
        if "grid" not in _GRID:
            _GRID["grid"] = ks_grid(0.2, L=4.0, fn=kerr_schild_island)
        objs, camera = ks_scene(cam_y=-3.5, width=5.0)
        return _GRID["grid"], objs, camera, over
    elif name != "ex2":
        raise KeyError(name)
    return metric, objs, rt.make_camera(**cam), over


_GRID = {}
_PLAIN = {}


def _outputs(n, dtype, device=False):
    import torch
    if device:
        td = torch.float64 if dtype == np.float64 else torch.float32
        z = lambda shape, t: torch.zeros(shape, dtype=t, device="cuda")
        return dict(state_end=z((n, 8), td), lambda_end=z(n, td), status=z(n, torch.uint8), hit=z(n, torch.uint8), n_accept=z(n, torch.int32),
                    n_reject=z(n, torch.int32), hit32=z(n, torch.int32))
    return dict(state_end=np.zeros((n, 8), dtype), lambda_end=np.zeros(n, dtype), status=np.zeros(n, np.uint8), hit=np.zeros(n, np.uint8),
                n_accept=np.zeros(n, np.uint32), n_reject=np.zeros(n, np.uint32), hit32=np.zeros(n, np.uint32))


def plain(lib, name, ni, nj, dtype=np.float64):
    """the plain frame (rtgr_trace_f64 / _f32, camera on the device) with every per-ray output: once per (scene, size, dtype), never
    written to"""
    key = (name, ni, nj, np.dtype(dtype).name)
    if key not in _PLAIN:
        metric, objs, cam, over = _scene(name)
        sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype, **over), ni * nj
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


def shaded(lib, name, ni, nj, binds, r_escape=0.0, dtype=np.float64, aa=None, details=True, counters=True):
    """rtgr_trace_shaded_f64 / _f32 (host pointers); binds: {object: (Texture, filter)}; aa: None or dict(k, contrast, max_batch_rays)"""
    metric, objs, cam, over = _scene(name)
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype, **over), ni * nj
    res = dict(rgb=np.full((3, n), -5.0, dtype))
    o = None
    if details:
        o = abi.rtgr_ray_outputs()
        res.update(_outputs(n, dtype))
        for k in OUT_KEYS:
            setattr(o, k, res[k].ctypes.data)
    sh = rt.make_shade(binds, r_escape)
    aap = refined = stats = None
    if aa is not None:
        aap = C.byref(abi.rtgr_aa(k=aa["k"], flags=0, contrast=aa["contrast"], max_batch_rays=aa.get("max_batch_rays", 0)))
        res["refined"] = np.full(n, 9, np.uint8)
        refined, stats = res["refined"].ctypes.data, abi.rtgr_aa_stats()
    ctr = abi.rtgr_counters() if counters else None
    fn = lib.rtgr_trace_shaded_f64 if dtype == np.float64 else lib.rtgr_trace_shaded_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(sh), aap, res["rgb"].ctypes.data, o, refined,
                      C.byref(ctr) if counters else None, C.byref(stats) if stats is not None else None))
    if counters:
        res["counters"] = ctr.as_dict()
    if stats is not None:
        res["stats"] = stats.as_dict()
    return res


def expected(p, name, binds, r_escape, dtype):
    """where(mask, rtgr_eval_texture(coords), plain rgb) by the header's rule, mask and coords by numpy from the PLAIN call's arrays.
    -> (rgb, mask)"""
    _, objs, _, _ = _scene(name)
    se, hit, st = p["state_end"], p["hit32"], p["status"]
    want, total = p["rgb"].copy(), np.zeros(len(hit), bool)
    for obj, (tex, filt) in binds.items():
        if obj == 0:
            x = se[:, 1:4]
            r = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])        # (in the frame's dtype, unfused, this order)
            assert r.dtype == dtype
            mask = (hit == 0) & ((st == abi.RAY_LAMBDA1) | (st == abi.RAY_OUTSIDE)) & (r >= dtype(r_escape))
            pts, rng = se[:, 5:8], None
        else:
            o = objs[obj - 1]
            mask = hit == obj
            if isinstance(o, rt.Disk):
                pts, rng = se[:, 1:4], (o.r_in, o.r_out)
            else:
                pts, rng = se[:, 1:4] - np.array(o.pos[1:4]).astype(dtype), None
                assert pts.dtype == dtype
        assert not (mask & total).any()
        total |= mask
        idx = np.flatnonzero(mask)
        if len(idx):
            col = rt.eval_texture(tex, np.ascontiguousarray(pts[idx]), filt, disk_range=rng, rgb=np.ascontiguousarray(p["rgb"][:, idx].T), dtype=dtype)
            want[:, idx] = col.T
    return want, total


def check_frame(lib, name, ni, nj, binds, r_escape=0.0, dtype=np.float64):
    p = plain(lib, name, ni, nj, dtype)
    want, mask = expected(p, name, binds, r_escape, dtype)
    got = shaded(lib, name, ni, nj, binds, r_escape, dtype)
    assert same_bits(got["rgb"], want)
    for key in OUT_KEYS:
        assert same_bits(got[key], p[key]), key
    assert got["counters"] == p["counters"]
    assert same_bits(got["rgb"][:, ~mask], p["rgb"][:, ~mask])          # (what is not bound keeps the plain bits)
    changed = (got["rgb"] != p["rgb"]).any(axis=0)
    return p, got, mask, changed


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_example2_sky_and_sphere_textured_plane_untouched(lib, dtype):
    _, tex = texture("rand32x16")
    _, tex2 = texture("rand16x8")
    p, got, mask, changed = check_frame(lib, "ex2", 48, 32, {1: (tex, BILINEAR), 3: (tex2, NEAREST)}, dtype=dtype)
    assert 0 < mask.sum() < len(mask)
    assert (p["hit32"] == 2).sum() > 50 and not mask[p["hit32"] == 2].any()          # the plane is in the picture and keeps its colour
    assert changed[mask].mean() > 0.99 and (p["hit32"][mask] == 1).any() and (p["hit32"][mask] == 3).any()
    # without a detail array asked for (the scratch of the stream stands in) and without counters: the same frame
    bare = shaded(lib, "ex2", 48, 32, {1: (tex, BILINEAR), 3: (tex2, NEAREST)}, dtype=dtype, details=False, counters=False)
    assert same_bits(bare["rgb"], got["rgb"])
    # nbind = 0: the plain frame
    none = shaded(lib, "ex2", 48, 32, {}, dtype=dtype)
    assert same_bits(none["rgb"], p["rgb"]) and none["counters"] == p["counters"]
    for key in OUT_KEYS:
        assert same_bits(none[key], p[key]), key
    # the Python front end gives the same frame
    metric, objs, cam = rt.example2_scene()
    front = rt.trace_shaded(metric, objs, cam, 48, 32, textures={1: (tex, BILINEAR), 3: (tex2, NEAREST)}, dtype=dtype, details=True)
    assert same_bits(front["rgb"], got["rgb"]) and same_bits(front["state_end"], p["state_end"])


@pytest.mark.gpu
def test_kerr_disk_and_sky(lib):
    _, tex = texture("rand32x16")
    _, tex2 = texture("rand16x8")
    p, got, mask, changed = check_frame(lib, "disk", 48, 32, {3: (tex2, BILINEAR), 1: (tex, NEAREST)})
    assert 0 < mask.sum() < len(mask)
    assert (p["hit32"][mask] == 3).sum() > 50 and (p["hit32"][mask] == 1).sum() > 50 and changed[mask].mean() > 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("r_escape", [0.0, 5.0, 62.0])
def test_escapes_of_example2_without_its_sky(lib, r_escape):
    """example2 without caelum, miss_rgb = 0.  As the scene stands the far plane t = -20 still ends every ray (the CPU oracle: 936 plane
    hits, 88 sphere hits, no miss of 1024), so nothing escapes and the shaded frame IS the plain frame; without the plane the rays that
    miss the sphere run to lambda1 at |x| of 57 .. 67 (status RTGR_RAY_LAMBDA1: shaded by their end velocity) or into the hole (status
    RTGR_RAY_MAXSTEPS at |x| = 1.56: never shaded).  r_escape = 0 and 5 select every ray that reached lambda1, 62 about half of them."""
    _, tex = texture("rand32x16")
    p, got, mask, _ = check_frame(lib, "ex2_nosky", 32, 32, {0: (tex, BILINEAR)}, r_escape)
    assert mask.sum() == 0 and (p["hit32"] > 0).all() and same_bits(got["rgb"], p["rgb"])
    p, got, mask, changed = check_frame(lib, "ex2_open", 32, 32, {0: (tex, BILINEAR)}, r_escape)
    assert 0 < mask.sum() < len(mask) and changed[mask].mean() > 0.99
    free = (p["hit32"] == 0) & (p["status"] == abi.RAY_LAMBDA1)
    captured = (p["hit32"] == 0) & (p["status"] != abi.RAY_LAMBDA1)
    assert captured.sum() > 20 and not mask[captured].any() and (p["rgb"][:, captured] == 0.0).all() and (got["rgb"][:, captured] == 0.0).all()
    if r_escape <= 5.0:
        assert np.array_equal(mask, free)
    else:
        assert 0.1 * free.sum() < mask.sum() < 0.9 * free.sum()


@pytest.mark.gpu
def test_rays_that_leave_a_grid_are_shaded(lib):
    _, tex = texture("rand32x16")
    p, got, mask, changed = check_frame(lib, "grid", 16, 16, {0: (tex, BILINEAR)})
    assert 0 < mask.sum() < len(mask) and changed[mask].mean() > 0.99
    assert (p["status"][mask] == abi.RAY_OUTSIDE).sum() > 10


@pytest.mark.gpu
def test_an_object_beyond_the_inline_slots(lib):
    _, tex = texture("rand16x8")
    p, got, mask, changed = check_frame(lib, "many40", 24, 16, {37: (tex, NEAREST)})
    assert 0 < mask.sum() < len(mask) and changed[mask].all() and (p["hit32"][mask] == 37).all()
    assert len(np.unique(p["hit32"])) >= 4


@pytest.mark.gpu
def test_round_trip_a_traced_frame_as_a_texture(lib):
    """a traced 12 x 8 frame loaded as it stands (width = ni, height = nj) and NEAREST-sampled at the texel-centre directions"""
    ni, nj = 12, 8
    p = plain(lib, "ex2", ni, nj)
    tex = rt.texture_load(p["rgb"].reshape(3, nj, ni))
    q, r = np.meshgrid(np.arange(ni), np.arange(nj))
    phi, theta = -np.pi + (q.ravel() + 0.5) * 2 * np.pi / ni, (r.ravel() + 0.5) * np.pi / nj
    d = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
    got = rt.eval_texture(tex, d, NEAREST)
    tex.unload()
    assert same_bits(np.ascontiguousarray(got.T), np.ascontiguousarray(p["rgb"]))


@pytest.mark.gpu
def test_straight_rays_point_where_they_look(lib):
    """Minkowski, nothing to hit, the escapes bound: u' = 0 exactly, so every pixel is the texture at the direction its ray started with"""
    ni, nj = 32, 24
    t, tex = texture("rand32x16")
    got = shaded(lib, "mink0", ni, nj, {0: (tex, BILINEAR)}, details=False)
    cam = rt.example2_scene()[2]
    cv = rt.make_canvas(rt.minkowski, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], ni, nj)
    d = cv.pixels.reshape(-1, order="F")["normal"][:, 1:4]
    s, v = coords_direction(d, 32, 16)
    err = np.abs(got["rgb"].T - np_bilinear(t, s, v)).max()
    print(f"straight rays: max error {err:.3e}, tol {tol_of(t, np.float64):.3e}")
    assert err <= tol_of(t, np.float64)


def box(fine_rgb, ni, nj, k):
    """the box filter of the (k ni) x (k nj) frame as the header states it: per channel 0, plus the k x k sub-pixels with t (rows) outer
    and s (columns) inner, in the frame's dtype, then one division by k*k"""
    dt = fine_rgb.dtype.type
    f = fine_rgb.reshape(3, k * nj, k * ni)
    acc = np.zeros((3, nj, ni), dt)
    for t in range(k):
        for s in range(k):
            acc = acc + f[:, t::k, s::k]
    assert acc.dtype == fine_rgb.dtype
    return (acc / dt(k * k)).reshape(3, ni * nj)


def edge_mask(rgb, hit, st, ni, nj, contrast):
    """the edge rule of rtgr_trace_aa_* on a frame's colours, hit map and status bytes"""
    dt = rgb.dtype.type
    rgb, hit, st = rgb.reshape(3, nj, ni), hit.reshape(nj, ni), st.reshape(nj, ni)
    mask = np.zeros((nj, ni), bool)
    with np.errstate(invalid="ignore"):
        di = (hit[:, 1:] != hit[:, :-1]) | (st[:, 1:] != st[:, :-1]) | (np.abs(rgb[:, :, 1:] - rgb[:, :, :-1]) > dt(contrast)).any(axis=0)
        dj = (hit[1:, :] != hit[:-1, :]) | (st[1:, :] != st[:-1, :]) | (np.abs(rgb[:, 1:, :] - rgb[:, :-1, :]) > dt(contrast)).any(axis=0)
    mask[:, 1:] |= di
    mask[:, :-1] |= di
    mask[1:, :] |= dj
    mask[:-1, :] |= dj
    return mask.reshape(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_anti_aliasing_of_a_shaded_frame(lib, dtype):
    """example2 with caelum textured, 24 x 16, k = 2: uniform == the box filter of the shaded 48 x 32 frame; refined == the edge rule on the
    SHADED 24 x 16 frame; adaptive == where(refined, uniform, shaded plain); batches of 28 sub-rays give the default's bits."""
    ni, nj, k, contrast = 24, 16, 2, 0.2
    _, tex = texture("rand32x16")
    binds = {1: (tex, BILINEAR)}
    coarse = shaded(lib, "ex2", ni, nj, binds, dtype=dtype)
    fine = shaded(lib, "ex2", k * ni, k * nj, binds, dtype=dtype, details=False)
    want_uniform = box(fine["rgb"], ni, nj, k)
    uniform = shaded(lib, "ex2", ni, nj, binds, dtype=dtype, aa=dict(k=k, contrast=-1.0))
    assert same_bits(uniform["rgb"], want_uniform) and (uniform["refined"] == 1).all()
    assert uniform["stats"] == dict(pixels=ni * nj, refined=ni * nj, sub_rays=k * k * ni * nj, batches=1)
    p = plain(lib, "ex2", ni, nj, dtype)
    mask = edge_mask(coarse["rgb"], p["hit32"], p["status"], ni, nj, contrast)
    by_class = edge_mask(coarse["rgb"], p["hit32"], p["status"], ni, nj, math.inf)
    assert by_class.sum() < mask.sum() < ni * nj                      # the texture's own contrast refines pixels the classes would not
    got = shaded(lib, "ex2", ni, nj, binds, dtype=dtype, aa=dict(k=k, contrast=contrast))
    assert np.array_equal(got["refined"], mask.astype(np.uint8))
    assert same_bits(got["rgb"], np.where(mask[None, :], want_uniform, coarse["rgb"]))
    for key in OUT_KEYS:
        assert same_bits(got[key], p[key]), key
    assert got["stats"] == dict(pixels=ni * nj, refined=int(mask.sum()), sub_rays=k * k * int(mask.sum()), batches=1)
    small = shaded(lib, "ex2", ni, nj, binds, dtype=dtype, aa=dict(k=k, contrast=contrast, max_batch_rays=28))
    assert small["stats"]["batches"] == -(-int(mask.sum()) // 7)
    assert same_bits(small["rgb"], got["rgb"]) and np.array_equal(small["refined"], got["refined"]) and small["counters"] == got["counters"]


@pytest.mark.gpu
def test_device_entry_on_a_side_stream_equals_the_host_entry(lib):
    import torch
    ni, nj, dtype = 48, 32, np.float64
    _, tex = texture("rand32x16")
    _, tex2 = texture("rand16x8")
    binds = {1: (tex, BILINEAR), 3: (tex2, NEAREST)}
    host = shaded(lib, "ex2", ni, nj, binds)
    metric, objs, cam, _ = _scene("ex2")
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rgb = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
        dev = _outputs(n, dtype, device=True)
        o = abi.rtgr_ray_outputs()
        for key in OUT_KEYS:
            setattr(o, key, dev[key].data_ptr())
        sh, ctr = rt.make_shade(binds), abi.rtgr_counters()
        abi.check(lib, lib.rtgr_trace_shaded_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(sh), None, rgb.data_ptr(),
                                                        C.byref(o), None, C.byref(ctr), None, side.cuda_stream))
        # … and with nothing but the frame asked for: the stream's scratch holds what the shading kernel reads
        rgb2 = torch.full((3, n), -5.0, dtype=torch.float64, device="cuda")
        abi.check(lib, lib.rtgr_trace_shaded_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(sh), None, rgb2.data_ptr(),
                                                        None, None, None, None, side.cuda_stream))
    torch.cuda.synchronize()
    assert rgb.cpu().numpy().tobytes() == host["rgb"].tobytes() and rgb2.cpu().numpy().tobytes() == host["rgb"].tobytes()
    for key in OUT_KEYS:
        assert dev[key].cpu().numpy().tobytes() == host[key].tobytes(), key
    assert ctr.as_dict() == host["counters"]


@pytest.mark.gpu
def test_refusals(lib):
    """Every refusal of rtgr_texture_load and of the shaded trace: RTGR_ERR_BAD_ARG with a message, rgb untouched."""
    import torch
    t, tex = texture("rand16x8")
    tid = C.c_uint64(0)
    good = np.zeros((3, 4, 4))

    def load(w, h, flags=0, pad=0, texels=good):
        desc = abi.rtgr_texture_desc(width=w, height=h, flags=flags, pad=pad)
        return lib.rtgr_texture_load(None, C.byref(desc), texels.ctypes.data, C.byref(tid)), lib.rtgr_last_error()

    big = np.zeros(3 * 2 * 16385)
    for kw, word in ((dict(w=1, h=4), b"2 .. 16384"), (dict(w=4, h=1), b"2 .. 16384"), (dict(w=16385, h=2, texels=big), b"2 .. 16384"),
                     (dict(w=2, h=16385, texels=big), b"2 .. 16384"), (dict(w=4, h=4, flags=1), b"flags"), (dict(w=4, h=4, pad=1), b"pad")):
        rc, msg = load(**kw)
        assert rc == abi.ERR_BAD_ARG and word in msg, (kw, rc, msg)
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[1, 2, 3] = bad_value
        rc, msg = load(4, 4, texels=bad)
        assert rc == abi.ERR_BAD_ARG and f"texel {(1 * 4 + 2) * 4 + 3} ".encode() in msg, msg
    assert tid.value == 0
    assert lib.rtgr_texture_unload(None, 12345) == abi.ERR_BAD_ARG and b"12345" in lib.rtgr_last_error()

    metric, objs, cam, _ = _scene("ex2")
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ni, nj = 8, 6
    rgb = torch.full((3, ni * nj), -5.0, dtype=torch.float64, device="cuda")
    host = np.full((3, ni * nj), -5.0)

    def call(binds=((1, BILINEAR, tex.id),), scene=sc, camera=cam, shade=True, aa=None, refined=False, stats=False, **over):
        arr = (abi.rtgr_texture_bind * max(len(binds), 1))(*[abi.rtgr_texture_bind(object=o, filter=f, texture=i) for o, f, i in binds])
        args = dict(dict(nbind=len(binds), flags=0, r_escape=0.0), **over)
        sh = abi.rtgr_shade(bind=C.cast(arr, C.POINTER(abi.rtgr_texture_bind)), **args)
        shp = C.byref(sh) if shade else None
        campt = C.byref(camera) if camera is not None else None
        aap = C.byref(abi.rtgr_aa(**aa)) if aa else None
        flags = np.zeros(ni * nj, np.uint8)
        dflags = torch.zeros(ni * nj, dtype=torch.uint8, device="cuda")
        st = abi.rtgr_aa_stats()
        rcs = [lib.rtgr_trace_shaded_device_f64(None, C.byref(scene), C.byref(opt), campt, ni, nj, shp, aap, rgb.data_ptr(), None,
                                                dflags.data_ptr() if refined else None, None, C.byref(st) if stats else None, None)]
        msgs = [lib.rtgr_last_error()]
        rcs.append(lib.rtgr_trace_shaded_f64(None, C.byref(scene), C.byref(opt), campt, ni, nj, shp, aap, host.ctypes.data, None,
                                             flags.ctypes.data if refined else None, None, C.byref(st) if stats else None))
        msgs.append(lib.rtgr_last_error())
        return rcs, msgs

    seventeen = tuple((0, BILINEAR, tex.id) for _ in range(17))
    user = rt.make_scene(metric, objs)
    user.obj[2].kind = abi.USER_OBJECT
    for kw, word in ((dict(shade=False), b"rtgr_shade is NULL"), (dict(camera=None), b"camera"), (dict(flags=1), b"flags"),
                     (dict(binds=seventeen), b"RTGR_MAX_TEXTURE_BINDS"), (dict(binds=((1, BILINEAR, tex.id + 99),)), str(tex.id + 99).encode()),
                     (dict(binds=((1, 2, tex.id),)), b"filter"), (dict(binds=((4, NEAREST, tex.id),)), b"object 4"),
                     (dict(binds=((1, NEAREST, tex.id), (3, NEAREST, tex.id), (1, BILINEAR, tex.id))), b"bound twice"),
                     (dict(binds=((0, NEAREST, tex.id), (0, BILINEAR, tex.id))), b"bound twice"),
                     (dict(binds=((2, NEAREST, tex.id),)), b"Plane"), (dict(binds=((3, NEAREST, tex.id),), scene=user), b"user object"),
                     (dict(r_escape=math.nan), b"r_escape"), (dict(r_escape=-1.0), b"r_escape"),
                     (dict(refined=True), b"must be NULL"), (dict(stats=True), b"must be NULL"),
                     (dict(aa=dict(k=1, flags=0, contrast=0.1, max_batch_rays=0)), b"2..8"),
                     (dict(aa=dict(k=2, flags=0, contrast=math.nan, max_batch_rays=0)), b"NaN")):
        rcs, msgs = call(**kw)
        assert rcs == [abi.ERR_BAD_ARG] * 2 and all(word in m for m in msgs), (kw, rcs, msgs)
    torch.cuda.synchronize()
    assert bool((rgb == -5.0).all()) and (host == -5.0).all()
    rcs, _ = call()
    torch.cuda.synchronize()
    assert rcs == [0, 0] and rgb.cpu().numpy().tobytes() == host.tobytes() and not (host == -5.0).any()
    # the sampler hook
    p, col = np.ones((1, 3)), np.full((1, 3), -3.0)
    assert lib.rtgr_eval_texture_f64(None, tex.id + 99, 0, p.ctypes.data, 1, None, col.ctypes.data) == abi.ERR_BAD_ARG
    assert lib.rtgr_eval_texture_f64(None, tex.id, 2, p.ctypes.data, 1, None, col.ctypes.data) == abi.ERR_BAD_ARG and (col == -3.0).all()


def _hip_runtime():
    """the HIP runtime already loaded in this process (torch's bundled libamdhip64)"""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return C.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")


@pytest.mark.gpu
def test_ids_and_lifetime_capture_unload_replay_trim(lib):
    """texture, grid and unit ids are distinct; a hipGraph captured before rtgr_texture_unload still replays the same frame (the texels
    were retired, not freed), the id is refused for new calls, rtgr_trim releases the memory; scratch growth during capture is refused."""
    import torch
    import sys
    from test_grid_metric import flat_grid
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import user_metrics
    hook = lib.rtgr_testhook_texture_tables
    hook.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    res, ret = C.c_uint32(), C.c_uint32()
    abi.check(lib, lib.rtgr_trim(None))
    t = random_texture(32, 16, seed=9)
    a, b = rt.texture_load(t), rt.texture_load(t)
    grid = flat_grid()
    gid = rt.make_scene(grid, []).user_metric
    uid = rt.make_scene(rt.UserMetric(user_metrics.SCHWARZSCHILD_ISOTROPIC, M=1.0), []).user_metric
    assert len({a.id, b.id, gid, uid}) == 4 and a.id >> 60 == 0x7 and gid >> 60 == 0xA
    assert lib.rtgr_grid_metric_unload(None, a.id) == abi.ERR_BAD_ARG and lib.rtgr_texture_unload(None, gid) == abi.ERR_BAD_ARG
    grid.unload()
    b.unload()
    abi.check(lib, hook(None, 0, C.byref(res), C.byref(ret)))
    n_res = res.value
    assert ret.value == 1

    metric, objs, cam, _ = _scene("ex2")
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ni, nj = 24, 16
    n = ni * nj
    sh = rt.make_shade({1: (a, BILINEAR)})
    side = torch.cuda.Stream()
    hip = _hip_runtime()

    def call(out, width=ni):
        return lib.rtgr_trace_shaded_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), width, nj, C.byref(sh), None, out.data_ptr(), None,
                                                None, None, None, side.cuda_stream)

    with torch.cuda.stream(side):
        eager = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        out = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        wide = torch.zeros((3, 2 * n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    abi.check(lib, call(eager))                                # the warm-up: workspace and scratch of this size exist afterwards
    torch.cuda.synchronize()
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc_big = call(wide, width=2 * ni)                          # a larger frame: the scratch would have to grow
    msg_big = lib.rtgr_last_error()
    rc = call(out)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert rc == 0 and rc_big == abi.ERR_BAD_ARG and b"captured" in msg_big
    assert graph.value and hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and bool((eager != 0).any())
    a.unload()
    abi.check(lib, hook(None, 0, C.byref(res), C.byref(ret)))
    assert (res.value, ret.value) == (n_res - 1, 2)
    fresh = torch.zeros((3, n), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert call(fresh) == abi.ERR_BAD_ARG and str(a.id).encode() in lib.rtgr_last_error()      # the id is unknown at once
    out.zero_()
    torch.cuda.synchronize()
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0                          # … the captured graph still replays
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and bool((fresh == 0).all())
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, hook(None, 0, C.byref(res), C.byref(ret)))
    assert ret.value == 0 and res.value == n_res - 1
    assert lib.rtgr_texture_unload(None, a.id) == abi.ERR_BAD_ARG
