"""Adaptive anti-aliasing (rtgr_trace_aa_*, include/rtgr.h): the plain frame, k x k sub-rays for the pixels on an edge, a box filter.

The reference has no anti-aliasing, so the judge is the library's own PLAIN frame (which the oracle pins): every anti-aliased pixel is
tied to plain frames bit for bit —
    uniform (contrast < 0)  ==  the box filter of the plain (k ni) x (k nj) frame, accumulated by numpy in the same order and dtype
    refined                 ==  the mask numpy computes from the plain frame's hit / status / rgb by the stated rule
    adaptive                ==  where(mask, uniform, plain)
whatever the batch size, the stream, or the entry point.  CPU part: symbols, struct layouts (ctypes and a compiled C caller), no frame
without a device."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from scenes import rt

abi = rt._abi
AA_EXPORTS = ("rtgr_trace_aa_device_f64", "rtgr_trace_aa_device_f32", "rtgr_trace_aa_f64", "rtgr_trace_aa_f32")
OUT_KEYS = ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject")


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------
def test_the_four_entry_points_are_declared_and_exported():
    assert set(AA_EXPORTS) <= set(abi.EXPORTS)
    lib = abi.load()
    for s in AA_EXPORTS:
        assert hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    assert "recursive refinement" in hdr and "jittered samples" in hdr              # the header states what is out of scope


def test_struct_layouts_in_ctypes_and_in_a_compiled_c_caller(tmp_path):
    assert C.sizeof(abi.rtgr_aa) == 24
    assert (abi.rtgr_aa.k.offset, abi.rtgr_aa.flags.offset, abi.rtgr_aa.contrast.offset, abi.rtgr_aa.max_batch_rays.offset) == (0, 4, 8, 16)
    assert C.sizeof(abi.rtgr_aa_stats) == 32
    assert [getattr(abi.rtgr_aa_stats, f).offset for f, _ in abi.rtgr_aa_stats._fields_] == [0, 8, 16, 24]
    exe = str(tmp_path / "aa_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "aa_layout.c"), "-o", exe, "-ldl"])
    out = subprocess.check_output([exe], text=True).split()
    assert dict(zip(out[0::2], map(int, out[1::2]))) == {"aa": 24, "k": 0, "flags": 4, "contrast": 8, "max_batch_rays": 16, "stats": 32,
                                                         "pixels": 0, "refined": 8, "sub_rays": 16, "batches": 24}
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    assert "#   RtgrAA           24   k 0, flags 4, contrast 8, max_batch_rays 16" in jl and ":rtgr_trace_aa_f64" in jl and "function trace_rays_aa(" in jl


def test_no_frame_without_a_device(tmp_path):
    """Without a HIP device the entry points FAIL with RTGR_ERR_NO_DEVICE and leave the caller's arrays alone — from a compiled C caller
    (host-pointer entry) and through ctypes (all four)."""
    import torch
    exe = str(tmp_path / "aa_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "c", "aa_layout.c"), "-o", exe, "-ldl"])
    res = subprocess.run([exe, abi.LIB_PATH], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr)       # (2: a symbol does not resolve)
    words = res.stdout.split("\n")[1].split()
    got = (int(words[1]), int(words[3]))
    assert got in ((abi.ERR_NO_DEVICE, 0), (0, 1)), got
    if torch.cuda.is_available():
        return
    assert got == (abi.ERR_NO_DEVICE, 0)
    lib = abi.load()
    sc, opt = rt.make_scene(rt.minkowski, []), rt.solver_defaults()
    cam = rt.make_camera(**rt.example1_scene()[2])
    aa = abi.rtgr_aa(k=2, flags=0, contrast=1 / 255, max_batch_rays=0)
    for dtype, suf in ((np.float64, "f64"), (np.float32, "f32")):
        rgb = np.full((3, 4), -7.0, dtype)
        rc = getattr(lib, "rtgr_trace_aa_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(cam), 2, 2, C.byref(aa), rgb.ctypes.data, None, None, None, None)
        assert rc == abi.ERR_NO_DEVICE and b"no CPU fallback" in lib.rtgr_last_error() and (rgb == -7.0).all()
        rc = getattr(lib, "rtgr_trace_aa_device_" + suf)(None, C.byref(sc), C.byref(opt), C.byref(cam), 2, 2, C.byref(aa), rgb.ctypes.data, None, None,
                                                        None, None, None)
        assert rc == abi.ERR_NO_DEVICE and (rgb == -7.0).all()
    with pytest.raises(abi.RtgrError):
        rt.trace_aa(rt.minkowski, [], rt.example1_scene()[2], 2, 2)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


_EXTRA = {}   # scenes a test registers under a name of its own


def _scene(name):
    """'ex2': example2's scene; 'disk': KerrSchild(1, 0.8) with the disk; 'mink0': Minkowski, nothing to hit — (metric, objs, camera)"""
    if name in _EXTRA:
        return _EXTRA[name]
    metric, objs, cam = rt.example2_scene()
    if name == "disk":
        metric, objs = rt.KerrSchild(1.0, 0.8), objs[:2] + [rt.Disk(0.05, 2.0, 4.0)]
    elif name == "mink0":
        metric, objs = rt.minkowski, []
    return metric, objs, rt.make_camera(**cam)


_PLAIN = {}


def plain(lib, name, ni, nj, dtype=np.float64):
    """the plain frame (rtgr_trace_f64 / _f32, camera on the device) with every per-ray output and the counters: computed once per
    (scene, size, dtype), shared by the tests, never written to"""
    key = (name, ni, nj, np.dtype(dtype).name)
    if key not in _PLAIN:
        metric, objs, cam = _scene(name)
        sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
        out = dict(rgb=np.zeros((3, n), dtype), state_end=np.zeros((n, 8), dtype), lambda_end=np.zeros(n, dtype), status=np.zeros(n, np.uint8),
                   hit=np.zeros(n, np.uint8), n_accept=np.zeros(n, np.uint32), n_reject=np.zeros(n, np.uint32), hit32=np.zeros(n, np.uint32))
        o = abi.rtgr_ray_outputs()
        for k in OUT_KEYS + ("hit32",):
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


def edge_mask(p, ni, nj, contrast):
    """the edge rule from a plain frame's arrays: a pixel is refined when an in-frame 4-neighbour differs in hit32, in status, or by more
    than `contrast` (rounded to the frame's dtype) in a colour channel; contrast < 0: every pixel"""
    if contrast < 0:
        return np.ones(ni * nj, bool)
    dt = p["rgb"].dtype.type
    rgb, hit, st = p["rgb"].reshape(3, nj, ni), p["hit32"].reshape(nj, ni), p["status"].reshape(nj, ni)
    mask = np.zeros((nj, ni), bool)
    with np.errstate(invalid="ignore"):
        di = (hit[:, 1:] != hit[:, :-1]) | (st[:, 1:] != st[:, :-1]) | (np.abs(rgb[:, :, 1:] - rgb[:, :, :-1]) > dt(contrast)).any(axis=0)
        dj = (hit[1:, :] != hit[:-1, :]) | (st[1:, :] != st[:-1, :]) | (np.abs(rgb[:, 1:, :] - rgb[:, :-1, :]) > dt(contrast)).any(axis=0)
    mask[:, 1:] |= di
    mask[:, :-1] |= di
    mask[1:, :] |= dj
    mask[:-1, :] |= dj
    return mask.reshape(-1)


def aa_host(lib, name, ni, nj, k, contrast, dtype=np.float64, batch=0, details=True):
    """rtgr_trace_aa_f64 / _f32 (host pointers) -> dict(rgb, refined, the per-ray outputs, counters, stats)"""
    metric, objs, cam = _scene(name)
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    res = dict(rgb=np.full((3, n), -5.0, dtype), refined=np.full(n, 9, np.uint8))
    o = None
    if details:
        o = abi.rtgr_ray_outputs()
        res.update(state_end=np.zeros((n, 8), dtype), lambda_end=np.zeros(n, dtype), status=np.zeros(n, np.uint8), hit=np.zeros(n, np.uint8),
                   n_accept=np.zeros(n, np.uint32), n_reject=np.zeros(n, np.uint32))
        for key in OUT_KEYS:
            setattr(o, key, res[key].ctypes.data)
    aa = abi.rtgr_aa(k=k, flags=0, contrast=contrast, max_batch_rays=batch)
    ctr, stats = abi.rtgr_counters(), abi.rtgr_aa_stats()
    fn = lib.rtgr_trace_aa_f64 if dtype == np.float64 else lib.rtgr_trace_aa_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(aa), res["rgb"].ctypes.data, o, res["refined"].ctypes.data,
                      C.byref(ctr), C.byref(stats)))
    res["counters"], res["stats"] = ctr.as_dict(), stats.as_dict()
    return res


def same_bits(a, b):
    """equal bit for bit (NaNs of equal payload included)"""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


FRAMES = [(24, 20), (33, 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("ni,nj", FRAMES)
@pytest.mark.parametrize("name", ["ex2", "disk"])
def test_uniform_supersampling_is_the_box_filter_of_the_fine_frame(lib, name, ni, nj, k, dtype):
    """contrast = -1 refines EVERY pixel: the frame is the k-times finer plain frame, box-filtered — bit for bit.  (k = 3: a reciprocal
    multiply instead of the division would show; any k: a sub-ray that is not make_pixel's of the fine canvas, a sum in another order.)"""
    got = aa_host(lib, name, ni, nj, k, -1.0, dtype, details=False)
    fine = plain(lib, name, k * ni, k * nj, dtype)
    assert np.array_equal(got["rgb"], box(fine["rgb"], ni, nj, k)) and same_bits(got["rgb"], box(fine["rgb"], ni, nj, k))
    assert got["stats"] == dict(pixels=ni * nj, refined=ni * nj, sub_rays=k * k * ni * nj, batches=1)
    assert (got["refined"] == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("contrast", [1.0 / 255.0, math.inf, 0.25])
@pytest.mark.parametrize("name,ni,nj,dtype", [("ex2", 24, 20, np.float64), ("ex2", 33, 17, np.float32), ("disk", 33, 17, np.float64),
                                              ("disk", 24, 20, np.float32), ("disk", 1, 20, np.float64), ("ex2", 24, 1, np.float64),
                                              ("disk", 1, 1, np.float64)])
def test_the_refined_mask_is_the_edge_rule_over_the_plain_frame(lib, name, ni, nj, dtype, contrast):
    """`refined` == the mask numpy computes from the plain frame's hit32 / status / rgb.  ni = 1, nj = 1 (and both): no neighbour outside
    the frame is read — a pixel without neighbours is never refined."""
    p = plain(lib, name, ni, nj, dtype)
    want = edge_mask(p, ni, nj, contrast)
    got = aa_host(lib, name, ni, nj, 2, contrast, dtype, details=False)
    assert np.array_equal(got["refined"], want.astype(np.uint8)), (int(want.sum()), int(got["refined"].sum()))
    assert got["stats"]["refined"] == int(want.sum())
    if min(ni, nj) > 1:
        assert want.sum() > 0                                            # the frames have edges (the silhouettes, at the least)
    if ni * nj == 1:
        assert want.sum() == 0
    if contrast == math.inf and min(ni, nj) > 1:                         # class edges only: flat regions remain, no more than with a colour threshold
        assert want.sum() < ni * nj and want.sum() <= edge_mask(p, ni, nj, 1.0 / 255.0).sum()


def _subray_states(lib, name, ni, nj, k, mask, dtype):
    """the sub-ray states of the masked pixels out of rtgr_make_canvas of the fine canvas, a pixel's k x k block contiguous (t outer)"""
    metric, objs, cam = _scene(name)
    sc = rt.make_scene(metric, objs)
    st = np.zeros((k * ni * k * nj, 8), dtype)
    fn = lib.rtgr_make_canvas_f64 if dtype == np.float64 else lib.rtgr_make_canvas_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(cam), k * ni, k * nj, 0, k * nj, st.ctypes.data))
    st = st.reshape(k * nj, k * ni, 8)
    rows = []
    for idx in np.flatnonzero(mask):
        i, j = idx % ni, idx // ni
        rows.append(st[k * j:k * j + k, k * i:k * i + k].reshape(k * k, 8))
    return np.ascontiguousarray(np.concatenate(rows)) if rows else np.zeros((0, 8), dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name,ni,nj,k,dtype", [("ex2", 24, 20, 4, np.float64), ("disk", 33, 17, 3, np.float64), ("disk", 24, 20, 2, np.float32)])
def test_the_adaptive_frame_selects_between_the_uniform_and_the_plain_frame(lib, name, ni, nj, k, dtype):
    """adaptive == where(mask, uniform, plain) bit for bit; `out` is the plain call's (the pixel-centre rays); ctr == the plain frame's
    counters + those of the sub-rays traced as caller-supplied states; stats.sub_rays == k² mask.sum()."""
    contrast = 1.0 / 255.0
    p = plain(lib, name, ni, nj, dtype)
    mask = edge_mask(p, ni, nj, contrast)
    uniform = box(plain(lib, name, k * ni, k * nj, dtype)["rgb"], ni, nj, k)
    got = aa_host(lib, name, ni, nj, k, contrast, dtype)
    assert same_bits(got["rgb"], np.where(mask[None, :], uniform, p["rgb"]))
    assert np.array_equal(got["refined"], mask.astype(np.uint8))
    for key in OUT_KEYS:
        assert same_bits(got[key], p[key]), key
    assert got["stats"] == dict(pixels=ni * nj, refined=int(mask.sum()), sub_rays=k * k * int(mask.sum()), batches=1)
    # the sub-rays on their own, as ray states
    s0 = _subray_states(lib, name, ni, nj, k, mask, dtype)
    metric, objs, _ = _scene(name)
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults(dtype)
    rgb, ctr = np.zeros((3, s0.shape[0]), dtype), abi.rtgr_counters()
    fn = lib.rtgr_trace_f64 if dtype == np.float64 else lib.rtgr_trace_f32
    abi.check(lib, fn(None, C.byref(sc), C.byref(opt), s0.ctypes.data, None, s0.shape[0], 1, 0, 1, rgb.ctypes.data, None, C.byref(ctr)))
    sub = ctr.as_dict()
    assert sub["rays"] == k * k * int(mask.sum())
    assert got["counters"] == {key: p["counters"][key] + sub[key] for key in sub}


@pytest.mark.gpu
@pytest.mark.parametrize("name,ni,nj,k,dtype", [("disk", 33, 17, 3, np.float64), ("ex2", 24, 20, 2, np.float32)])
def test_batching_changes_nothing(lib, name, ni, nj, k, dtype):
    """max_batch_rays = k² (a pixel per batch), 5 k² + 1 (no multiple of a pixel's block: rounded down to 5 pixels) and the default:
    the same frame bit for bit, the same counters, stats.batches as computed."""
    contrast = 1.0 / 255.0
    count = int(edge_mask(plain(lib, name, ni, nj, dtype), ni, nj, contrast).sum())
    assert count > 10
    ref = aa_host(lib, name, ni, nj, k, contrast, dtype)
    assert ref["stats"]["batches"] == 1
    for batch, want in ((k * k, count), (5 * k * k + 1, -(-count // 5)), (1, count)):   # (1: below one pixel's block — one pixel)
        got = aa_host(lib, name, ni, nj, k, contrast, dtype, batch=batch)
        assert got["stats"] == dict(ref["stats"], batches=want), (batch, got["stats"])
        assert same_bits(got["rgb"], ref["rgb"]) and np.array_equal(got["refined"], ref["refined"]) and got["counters"] == ref["counters"], batch


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_nothing_to_refine(lib, dtype):
    """Minkowski and an empty object list: every ray misses, no pixel differs from a neighbour — no zero-size launch may fail."""
    ni, nj = 24, 20
    p = plain(lib, "mink0", ni, nj, dtype)
    got = aa_host(lib, "mink0", ni, nj, 4, 1.0 / 255.0, dtype)
    assert got["stats"] == dict(pixels=ni * nj, refined=0, sub_rays=0, batches=0)
    assert same_bits(got["rgb"], p["rgb"]) and (got["refined"] == 0).all() and got["counters"] == p["counters"]
    assert (p["hit32"] == 0).all()


def aa_device(lib, name, ni, nj, k, contrast, dtype=np.float64, stream=None, batch=0):
    """rtgr_trace_aa_device_* on torch tensors, on `stream` (default: torch's current one) -> dict of tensors + counters + stats"""
    import torch
    metric, objs, cam = _scene(name)
    sc, opt, n = rt.make_scene(metric, objs), rt.solver_defaults(dtype), ni * nj
    td = torch.float64 if dtype == np.float64 else torch.float32
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        res = dict(rgb=torch.full((3, n), -5.0, dtype=td, device="cuda"), refined=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                   state_end=torch.zeros((n, 8), dtype=td, device="cuda"), lambda_end=torch.zeros(n, dtype=td, device="cuda"),
                   status=torch.zeros(n, dtype=torch.uint8, device="cuda"), hit=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                   n_accept=torch.zeros(n, dtype=torch.int32, device="cuda"), n_reject=torch.zeros(n, dtype=torch.int32, device="cuda"))
        o = abi.rtgr_ray_outputs()
        for key in OUT_KEYS:
            setattr(o, key, res[key].data_ptr())
        aa = abi.rtgr_aa(k=k, flags=0, contrast=contrast, max_batch_rays=batch)
        ctr, stats = abi.rtgr_counters(), abi.rtgr_aa_stats()
        fn = lib.rtgr_trace_aa_device_f64 if dtype == np.float64 else lib.rtgr_trace_aa_device_f32
        abi.check(lib, fn(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(aa), res["rgb"].data_ptr(), C.byref(o),
                          res["refined"].data_ptr(), C.byref(ctr), C.byref(stats), st.cuda_stream))
    res["counters"], res["stats"] = ctr.as_dict(), stats.as_dict()
    return res


def _equal_to_host(dev, host):
    for key in ("rgb", "refined") + OUT_KEYS:
        a = dev[key].cpu().numpy()
        assert a.tobytes() == host[key].tobytes(), key
    assert dev["counters"] == host["counters"] and dev["stats"] == host["stats"]


@pytest.mark.gpu
def test_device_entry_host_twin_and_two_streams(lib):
    """ONE code path: the host-pointer twin gives the device entry's bits (frame, mask, per-ray outputs, counters, stats), on the default
    stream and on two streams of two host threads at the same time (each stream has a scratch of its own)."""
    import threading
    import torch
    jobs = [("ex2", 24, 20, 4, np.float64), ("disk", 33, 17, 3, np.float32)]
    hosts = [aa_host(lib, name, ni, nj, k, 1.0 / 255.0, dtype) for name, ni, nj, k, dtype in jobs]
    for (name, ni, nj, k, dtype), h in zip(jobs, hosts):
        d = aa_device(lib, name, ni, nj, k, 1.0 / 255.0, dtype)
        torch.cuda.synchronize()
        _equal_to_host(d, h)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for rep in range(2):
        outs, errs = [None, None], []

        def run(q):
            try:
                name, ni, nj, k, dtype = jobs[q]
                outs[q] = aa_device(lib, name, ni, nj, k, 1.0 / 255.0, dtype, stream=streams[q], batch=7 * k * k)
            except Exception as e:   # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=run, args=(q,)) for q in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        torch.cuda.synchronize()
        assert not errs, errs
        for d, h in zip(outs, hosts):
            assert d["stats"]["batches"] == -(-h["stats"]["refined"] // 7)
            d["stats"]["batches"] = h["stats"]["batches"]
            _equal_to_host(d, h)


def _hip_runtime():
    """the HIP runtime already loaded in this process (torch's bundled libamdhip64)"""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return C.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")


@pytest.mark.gpu
def test_refusals(lib):
    """k outside 2..8, flags, a NaN contrast, no camera, a scene whose metric is RTGR_USER: RTGR_ERR_BAD_ARG with a message, nothing
    written.  A call during stream capture is refused and leaves the stream usable."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import user_metrics
    metric, objs, cam = _scene("ex2")
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    ni, nj = 8, 6
    rgb = torch.full((3, ni * nj), -5.0, dtype=torch.float64, device="cuda")
    host = np.full((3, ni * nj), -5.0)

    def call(scene=sc, camera=cam, stream=None, **over):
        aa = abi.rtgr_aa(**dict(dict(k=2, flags=0, contrast=1 / 255, max_batch_rays=0), **over))
        campt = C.byref(camera) if camera is not None else None
        rcs = [lib.rtgr_trace_aa_device_f64(None, C.byref(scene), C.byref(opt), campt, ni, nj, C.byref(aa), rgb.data_ptr(), None, None, None, None, stream)]
        msgs = [lib.rtgr_last_error()]
        if stream is None:
            rcs.append(lib.rtgr_trace_aa_f64(None, C.byref(scene), C.byref(opt), campt, ni, nj, C.byref(aa), host.ctypes.data, None, None, None, None))
            msgs.append(lib.rtgr_last_error())
        return rcs, msgs

    user = rt.UserMetric(user_metrics.SCHWARZSCHILD_ISOTROPIC, M=1.0)
    user_scene = rt.make_scene(user, objs)
    assert lib.rtgr_user_metric_loaded(None, user_scene.user_metric) == 1
    for kw, word in ((dict(k=1), b"2..8"), (dict(k=9), b"2..8"), (dict(flags=1), b"flags"), (dict(contrast=math.nan), b"NaN"),
                     (dict(camera=None), b"camera"), (dict(scene=user_scene), b"RTGR_USER")):
        rcs, msgs = call(**kw)
        assert rcs == [abi.ERR_BAD_ARG] * 2 and all(word in m for m in msgs), (kw, rcs, msgs)
    torch.cuda.synchronize()
    assert bool((rgb == -5.0).all()) and (host == -5.0).all()
    # during capture
    hip = _hip_runtime()
    side = torch.cuda.Stream()
    rcs, _ = call(stream=side.cuda_stream)       # (the stream's workspace and scratch exist: growth is not what refuses the next call)
    assert rcs == [0]
    torch.cuda.synchronize()
    good = rgb.clone()
    rgb.fill_(-5.0)
    torch.cuda.synchronize()
    graph = C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rcs, msgs = call(stream=side.cuda_stream)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    if graph.value:
        hip.hipGraphDestroy(graph)
    assert rcs == [abi.ERR_BAD_ARG] and b"captured" in msgs[0]
    torch.cuda.synchronize()
    assert bool((rgb == -5.0).all())
    rcs, _ = call(stream=side.cuda_stream)       # the stream is still usable
    torch.cuda.synchronize()
    assert rcs == [0] and torch.equal(rgb, good)


@pytest.mark.gpu
def test_a_grid_scene_with_rays_that_leave_the_grid(lib):
    """A 3-D grid of KerrSchild(1, 0.8) smaller than the sky (tests/test_grid_metric.py's smallest table), 12 x 10, k = 2: the uniform
    frame is the box filter of the fine frame, and the border between rays that leave the grid (RTGR_RAY_OUTSIDE) and rays that end in
    it is found by the STATUS clause of the edge rule."""
    from test_grid_metric import kerr_schild_island, ks_grid, ks_scene
    ni, nj, k = 12, 10, 2
    objs, cam = ks_scene(cam_y=-3.5, width=5.0)
    scene = "grid"
    _EXTRA[scene] = (ks_grid(0.2, L=4.0, fn=kerr_schild_island), objs, cam)
    p = plain(lib, scene, ni, nj)
    fine = plain(lib, scene, k * ni, k * nj)
    got = aa_host(lib, scene, ni, nj, k, -1.0, details=False)
    assert same_bits(got["rgb"], box(fine["rgb"], ni, nj, k)) and got["stats"]["refined"] == ni * nj
    out = (p["status"] == abi.RAY_OUTSIDE).reshape(nj, ni)
    assert 0 < out.sum() < ni * nj
    edges = aa_host(lib, scene, ni, nj, k, math.inf)
    want = edge_mask(p, ni, nj, math.inf)
    assert np.array_equal(edges["refined"], want.astype(np.uint8))
    st = p["status"].reshape(nj, ni)
    by_status = st[:, 1:] != st[:, :-1]                                    # neighbours the status tells apart
    assert by_status.any() and want.reshape(nj, ni)[:, 1:][by_status].all() and want.reshape(nj, ni)[:, :-1][by_status].all()
    assert same_bits(edges["rgb"], np.where(want[None, :], box(fine["rgb"], ni, nj, k), p["rgb"]))
    assert same_bits(edges["status"], p["status"])
