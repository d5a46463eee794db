"""Contexts, streams, threads, devices (SURVEY §8b "Ownership / Threading", §8e): the library's state lives in an
opaque rtgr_context; calls on different streams / from different host threads / on different (logical) devices must give
the SAME BITS as serial execution, and one host thread must be able to drive every device of a context with one call.
`pytest -m gpu` (one GPU: a context may list the same physical device several times)."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import oracle_lib as O
from conftest import ROOT
from scenes import example, rt, scene_variant

pytestmark = pytest.mark.gpu
abi = rt._abi
OUT_KEYS = ("rgb", "state_end", "lambda_end", "status", "hit", "n_accept", "n_reject")


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def _devices(n):
    """n device ordinals for a context, DISTINCT physical GPUs as far as the box has them (VERDICT r3 #3a: on a node the multi-device
    tests must touch a second GPU — peer copies, per-device PCIe links, modules loaded per device), the calling thread's current
    device first (the tests keep their device-0 tensors there); on a one-GPU box the same ordinal n times: logical devices with
    streams, workspaces and staging of their own."""
    import torch
    cur, count = torch.cuda.current_device(), max(torch.cuda.device_count(), 1)
    return [(cur + k) % count for k in range(n)]


def _trace(sc, opt, cam, ni, nj, ctx=None, stream=None):
    import torch
    from raytracegr_jl_amd import sharded
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        ctr = torch.zeros(8, dtype=torch.int64, device="cuda")   # (zero-filled ON the stream the trace will add on)
        out = sharded.trace_slab_torch(sc, opt, cam, ni, nj, 0, nj, details=True, counters=ctr, ctx=ctx)
    out["ctr"] = ctr
    return out


def _same(a, b):
    import torch
    for k in a:
        x, y = a[k], b[k]
        bad = ~((x == y) | (x.isnan() & y.isnan())) if x.is_floating_point() else (x != y)
        assert not bool(bad.any()), (k, int(bad.sum()), bad.numel(), bad.nonzero()[:8].tolist())


def test_explicit_context_equals_default_context(lib):
    import torch
    sc, cam = example(2)
    opt = rt.solver_defaults()
    ref = _trace(sc, opt, cam, 96, 64)
    torch.cuda.synchronize()
    ctx = abi.create_context(lib, [torch.cuda.current_device()])
    try:
        assert lib.rtgr_context_devices(ctx) == 1
        got = _trace(sc, opt, cam, 96, 64, ctx=ctx)
        torch.cuda.synchronize()
        _same(ref, got)
        # options are per context
        abi.check(lib, lib.rtgr_set_option(ctx, b"split", 0))
        v = C.c_long(7)
        abi.check(lib, lib.rtgr_get_option(None, b"split", C.byref(v)))
        assert v.value == -1
        assert lib.rtgr_set_option(ctx, b"no_such_option", 1) == abi.ERR_BAD_ARG
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_two_streams_in_flight_are_bit_identical_to_serial(lib):
    """Round 1 had ONE process-global workspace: two traces on different streams raced on the same records.  Now every
    (device, stream) owns its workspace and queue heads."""
    import torch
    jobs = [(scene_variant("ks_ref0"), 320, 256), (scene_variant("ks_true0998_disk"), 256, 320)]
    opt = rt.solver_defaults()
    serial = []
    for (sc, cam), ni, nj in jobs:
        serial.append(_trace(sc, opt, cam, ni, nj))
        torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for rep in range(3):
        outs = []
        for ((sc, cam), ni, nj), st in zip(jobs, (s1, s2)):   # both enqueued before either is waited for
            outs.append(_trace(sc, opt, cam, ni, nj, stream=st))
        torch.cuda.synchronize()
        for a, b in zip(serial, outs):
            _same(a, b)


def test_two_host_threads_on_one_context(lib):
    """Re-entrancy: two host threads, each with a stream of its own, drive the same context at the same time."""
    import torch
    jobs = [(scene_variant("ks_ref0"), 200, 160), (scene_variant("ks_true08"), 160, 200)]
    opt = rt.solver_defaults()
    serial = []
    for (sc, cam), ni, nj in jobs:
        serial.append(_trace(sc, opt, cam, ni, nj))
        torch.cuda.synchronize()
    dev = torch.cuda.current_device()
    results, errors = [None, None], []

    def worker(k):
        try:
            torch.cuda.set_device(dev)
            st = torch.cuda.Stream()
            (sc, cam), ni, nj = jobs[k]
            for _ in range(4):
                results[k] = _trace(sc, opt, cam, ni, nj, stream=st)
            st.synchronize()
        except Exception as e:  # noqa: BLE001 - reported below
            errors.append(e)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    for a, b in zip(serial, results):
        _same(a, b)


def test_host_entry_points_from_two_threads(lib):
    """The blocking host-pointer entry points (what a Julia ccall binds) from two threads at once: they share the
    context's staging buffers and must serialise on them, not corrupt them."""
    from test_gpu_parity import hip_trace
    sc, cam = example(2)
    opt = rt.solver_defaults()
    ref = hip_trace(lib, sc, opt, 80, 60, cam=cam)
    got, errors = [None, None], []

    def worker(k):
        try:
            for _ in range(3):
                got[k] = hip_trace(lib, sc, opt, 80, 60, cam=cam)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    th = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    for g in got:
        for k in OUT_KEYS:
            assert np.array_equal(ref[k], g[k]), k
        assert ref["counters"] == g["counters"]


@pytest.mark.parametrize("ndev", [2, 3])
def test_single_process_multi_device_trace(lib, ndev):
    """rtgr_trace_sharded_f64: ONE call from ONE host thread deals the rows cyclically to every device of the context,
    and RGB + status + hit + step counts + end states + lambda_end + counters come back assembled on device 0.  On a
    one-GPU box the context lists the same physical device `ndev` times (logical devices with streams, workspaces and
    peer copies of their own); the frame must equal the single-device frame bit for bit."""
    import torch
    from test_gpu_parity import hip_trace
    sc, cam = scene_variant("ks_true0998_disk")
    opt = rt.solver_defaults()
    ni, nj = 96, 77   # 77 rows: unequal shares
    ref = hip_trace(lib, sc, opt, ni, nj, cam=cam)
    ctx = abi.create_context(lib, _devices(ndev))
    try:
        assert lib.rtgr_context_devices(ctx) == ndev
        n = ni * nj
        rgb = np.zeros((3, n))
        o, arrs = O._outs(n, np.float64, True)
        ctr = abi.rtgr_counters()
        for rep in range(2):
            abi.check(lib, lib.rtgr_trace_sharded_f64(ctx, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj,
                                                      rgb.ctypes.data, C.byref(o), C.byref(ctr)))
            assert np.array_equal(rgb, ref["rgb"])
            for k in OUT_KEYS[1:]:
                assert np.array_equal(arrs[k], ref[k]), k
            assert ctr.as_dict() == ref["counters"]
        # device variant: the frame stays in device-0 memory
        d_rgb = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        d_st = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
        od = abi.rtgr_ray_outputs()
        od.status = d_st.data_ptr()
        abi.check(lib, lib.rtgr_trace_sharded_device_f64(ctx, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj,
                                                         d_rgb.data_ptr(), C.byref(od), None))
        assert np.array_equal(d_rgb.cpu().numpy(), ref["rgb"]) and np.array_equal(d_st.cpu().numpy(), ref["status"])
        # Float32 twin
        opt32 = rt.solver_defaults(np.float32)
        ref32 = hip_trace(lib, sc, opt32, ni, nj, cam=cam, dtype=np.float32)
        rgb32 = np.zeros((3, n), np.float32)
        o32, arrs32 = O._outs(n, np.float32, True)
        abi.check(lib, lib.rtgr_trace_sharded_f32(ctx, C.byref(sc), C.byref(opt32), C.byref(cam), ni, nj, rgb32.ctypes.data,
                                                  C.byref(o32), C.byref(ctr)))
        assert np.array_equal(rgb32, ref32["rgb"]) and ctr.as_dict() == ref32["counters"]
        for k in OUT_KEYS[1:]:
            assert np.array_equal(arrs32[k], ref32[k], equal_nan=True), k
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_device_resident_float32_and_support_entry_points(lib):
    """The entry points the other tests reach only through wrappers or not at all: rtgr_make_canvas_device_f64/_f32
    (== the host variants), rtgr_trace_rows_device_f32 (strided rows == the rows of the full Float32 frame),
    rtgr_trace_sharded_device_f32 (== the single-device frame), rtgr_device_info, rtgr_timing_enable/_read."""
    import torch
    from test_gpu_parity import hip_trace
    sc, cam = scene_variant("ks_true08")
    ni, nj = 64, 48
    n = ni * nj
    stream = torch.cuda.current_stream().cuda_stream
    for suf, td, nd in (("f64", torch.float64, np.float64), ("f32", torch.float32, np.float32)):
        host = np.zeros((n, 8), nd)
        abi.check(lib, getattr(lib, f"rtgr_make_canvas_{suf}")(None, C.byref(sc), C.byref(cam), ni, nj, 0, nj, host.ctypes.data))
        dev = torch.zeros((n, 8), dtype=td, device="cuda")
        abi.check(lib, getattr(lib, f"rtgr_make_canvas_device_{suf}")(None, C.byref(sc), C.byref(cam), ni, nj, 0, nj, dev.data_ptr(), stream))
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), host)
        part = torch.zeros((ni * 5, 8), dtype=td, device="cuda")        # rows [7, 12)
        abi.check(lib, getattr(lib, f"rtgr_make_canvas_device_{suf}")(None, C.byref(sc), C.byref(cam), ni, nj, 7, 12, part.data_ptr(), stream))
        torch.cuda.synchronize()
        assert np.array_equal(part.cpu().numpy(), host[7 * ni:12 * ni])
    opt32 = rt.solver_defaults(np.float32)
    ref = hip_trace(lib, sc, opt32, ni, nj, cam=cam, dtype=np.float32)
    # rows 1, 4, 7, … of the frame, Float32, device-resident, with per-kernel timing on
    abi.check(lib, lib.rtgr_timing_enable(None, 0, 1))
    rows = list(range(1, nj, 3))
    d_rgb = torch.zeros((3, ni * len(rows)), dtype=torch.float32, device="cuda")
    d_st = torch.full((ni * len(rows),), 255, dtype=torch.uint8, device="cuda")
    d_ctr = torch.zeros(8, dtype=torch.int64, device="cuda")
    o = abi.rtgr_ray_outputs()
    o.status = d_st.data_ptr()
    abi.check(lib, lib.rtgr_trace_rows_device_f32(None, C.byref(sc), C.byref(opt32), C.byref(cam), ni, nj, 1, 3, len(rows),
                                                  d_rgb.data_ptr(), C.byref(o), d_ctr.data_ptr(), stream))
    torch.cuda.synchronize()
    want = ref["rgb"].reshape(3, nj, ni)[:, rows, :].reshape(3, -1)
    assert np.array_equal(d_rgb.cpu().numpy(), want)
    assert np.array_equal(d_st.cpu().numpy(), ref["status"].reshape(nj, ni)[rows].reshape(-1))
    assert int(d_ctr[0]) == ni * len(rows)
    ms, launches = (C.c_double * 4)(), (C.c_uint64 * 4)()
    abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms), C.byref(launches)))
    abi.check(lib, lib.rtgr_timing_enable(None, 0, 0))
    assert launches[1] == 1 and launches[2] == 1 and launches[0] >= 1 and launches[3] == 0   # Float32: one FULL pass, no NEAR
    assert all(0.0 < ms[k] < 1e3 for k in (0, 1, 2)) and ms[3] == 0.0
    abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms), C.byref(launches)))            # read = since the previous read
    assert list(launches) == [0, 0, 0, 0]
    # device info
    name = C.create_string_buffer(64)
    cu, mhz, wf = C.c_int(0), C.c_int(0), C.c_int(0)
    abi.check(lib, lib.rtgr_device_info(None, 0, name, 64, C.byref(cu), C.byref(mhz), C.byref(wf)))
    assert name.value and cu.value >= 64 and mhz.value > 500 and wf.value == 64
    assert lib.rtgr_device_info(None, 5, name, 64, C.byref(cu), C.byref(mhz), C.byref(wf)) == abi.ERR_BAD_ARG
    # multi-device, Float32, frame left on device 0
    ctx = abi.create_context(lib, _devices(3))
    try:
        d_full = torch.zeros((3, n), dtype=torch.float32, device="cuda")
        d_hit = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
        od = abi.rtgr_ray_outputs()
        od.hit = d_hit.data_ptr()
        ctr = abi.rtgr_counters()
        abi.check(lib, lib.rtgr_trace_sharded_device_f32(ctx, C.byref(sc), C.byref(opt32), C.byref(cam), ni, nj, d_full.data_ptr(),
                                                         C.byref(od), C.byref(ctr)))
        assert np.array_equal(d_full.cpu().numpy(), ref["rgb"]) and np.array_equal(d_hit.cpu().numpy(), ref["hit"])
        assert ctr.as_dict() == ref["counters"]
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_user_metric_on_a_multi_device_context(lib):
    """A run-time compiled metric is loaded on every device of a context (logical duplicates of one GPU share the
    module); the multi-device frame equals the single-device one, and unload / destroy release it exactly once."""
    import sys
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    import user_metrics
    from test_gpu_parity import hip_trace
    user = rt.UserMetric(user_metrics.SCHWARZSCHILD_ISOTROPIC, M=1.0, stationary=True)
    _, objs, cam = rt.example2_scene()
    opt, camera = rt.solver_defaults(), rt.make_camera(**cam)
    ref = hip_trace(lib, rt.make_scene(user, objs), opt, 48, 33, cam=camera)
    ctx = abi.create_context(lib, _devices(2))
    try:
        sc = rt.make_scene(user, objs, ctx=ctx)          # loads the module into THIS context
        assert lib.rtgr_user_metric_loaded(ctx, sc.user_metric) == 1
        rgb = np.zeros((3, 48 * 33))
        ctr = abi.rtgr_counters()
        abi.check(lib, lib.rtgr_trace_sharded_f64(ctx, C.byref(sc), C.byref(opt), C.byref(camera), 48, 33, rgb.ctypes.data, None, C.byref(ctr)))
        assert np.array_equal(rgb, ref["rgb"]) and ctr.as_dict() == ref["counters"]
        abi.check(lib, lib.rtgr_user_metric_unload(ctx, sc.user_metric))
        assert lib.rtgr_user_metric_loaded(ctx, sc.user_metric) == 0
        assert lib.rtgr_trace_sharded_f64(ctx, C.byref(sc), C.byref(opt), C.byref(camera), 48, 33, rgb.ctypes.data, None, None) == abi.ERR_BAD_ARG
        sc = rt.make_scene(rt.UserMetric(user_metrics.SCHWARZSCHILD_ISOTROPIC, M=1.0, stationary=True), objs, ctx=ctx)   # and again
        abi.check(lib, lib.rtgr_trace_sharded_f64(ctx, C.byref(sc), C.byref(opt), C.byref(camera), 48, 33, rgb.ctypes.data, None, None))
        assert np.array_equal(rgb, ref["rgb"])
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_more_devices_than_rows(lib):
    import torch
    from test_gpu_parity import hip_trace
    sc, cam = example(2)
    opt = rt.solver_defaults()
    ref = hip_trace(lib, sc, opt, 9, 2, cam=cam)
    ctx = abi.create_context(lib, _devices(4))
    try:
        rgb = np.zeros((3, 18))
        abi.check(lib, lib.rtgr_trace_sharded_f64(ctx, C.byref(sc), C.byref(opt), C.byref(cam), 9, 2, rgb.ctypes.data, None, None))
        assert np.array_equal(rgb, ref["rgb"])
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_pixels_entry_point_is_pipelined_in_pieces(lib):
    """rtgr_trace_pixels_f64 — the entry point INTEGRATION.md tells Julia to ccall — cuts the job into transfer pieces
    and compute chunks (H2D || integrate || D2H on three streams).  With tiny pieces (many chunks, ragged last one) the
    returned Array{Pixel} must equal the one-chunk result bit for bit, inputs preserved, in place or not."""
    metric, objs, cam = rt.example2_scene()
    canvas = rt.make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], 60, 45)
    one = rt.trace_rays(metric, objs, canvas)
    with abi.options(lib, host_chunk=256):     # 1024-ray compute chunks = 17 rows of 60; 45 rows -> 3 chunks, pieces of 256
        many = rt.trace_rays(metric, objs, canvas)
        # in place: pixels_out aliases pixels_in
        sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
        px = np.asfortranarray(canvas.pixels.copy())
        abi.check(lib, lib.rtgr_trace_pixels_f64(None, C.byref(sc), C.byref(opt), px.ctypes.data, 60, 45, px.ctypes.data, None))
    for f in ("pos", "normal", "rgb"):
        assert np.array_equal(one.pixels[f], many.pixels[f]), f
        assert np.array_equal(one.pixels[f], px[f]), f
    assert np.array_equal(one.pixels["pos"], canvas.pixels["pos"])
    bad = np.asfortranarray(canvas.pixels.copy())
    bad["normal"][7, 3, 2] = np.nan
    out = np.empty_like(bad)
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    rc = lib.rtgr_trace_pixels_f64(None, C.byref(sc), C.byref(opt), bad.ctypes.data, 60, 45, out.ctypes.data, None)
    assert rc == abi.ERR_NAN_INPUT   # `@assert !any(isnan, …)` (src/RayTraceGR.jl:279), evaluated on the device


@pytest.mark.parametrize("ni,nj,piece", [(37, 53, 64), (64, 40, 200), (19, 120, 100)])
def test_host_pipeline_with_many_chunks_and_every_output(lib, ni, nj, piece):
    """The blocking host entry points cut a job into compute chunks whose D2H is ordered behind the NEXT chunk's set-up
    kernels and lands in two alternating pinned slots: with tiny pieces (9-25 chunks here) and every per-ray output asked
    for, camera rays or caller-supplied states, the result must equal the single-launch device path bit for bit."""
    from test_gpu_parity import hip_trace
    sc, cam = scene_variant("ks_true08")
    opt = rt.solver_defaults()
    ref = hip_trace(lib, sc, opt, ni, nj, cam=cam)        # host_chunk automatic: one chunk at this size
    st0 = np.zeros((ni * nj, 8))
    abi.check(lib, lib.rtgr_make_canvas_f64(None, C.byref(sc), C.byref(cam), ni, nj, 0, nj, st0.ctypes.data))
    with abi.options(lib, host_chunk=piece):
        for state0 in (None, st0):
            got = hip_trace(lib, sc, opt, ni, nj, cam=cam if state0 is None else None, state0=state0)
            for k in OUT_KEYS:
                assert np.array_equal(got[k], ref[k], equal_nan=True), (k, state0 is None)
            assert got["counters"] == ref["counters"]
        # a slab of rows, states supplied
        j0, j1 = nj // 3, nj - 2
        part = hip_trace(lib, sc, opt, ni, nj, j0=j0, j1=j1, state0=st0[j0 * ni:j1 * ni])
        assert np.array_equal(part["rgb"], ref["rgb"].reshape(3, nj, ni)[:, j0:j1].reshape(3, -1))
        assert np.array_equal(part["state_end"], ref["state_end"][j0 * ni:j1 * ni])


def test_float32_canvas_through_the_pixel_entry_points(lib):
    """`Canvas{T}` is generic in T (src/RayTraceGR.jl:452-455; the reference's own tests instantiate T = Float32,
    test/runtests.jl:37): trace_rays on a Canvas{Float32} goes through rtgr_trace_pixels_f32 with 44-byte pixels.  It must
    agree bit for bit with the planar Float32 entry point (same kernels, different packing), preserve pos/normal, work
    in pieces, and trace_ray (rtgr_trace_one_f32) must return the canvas' own pixel."""
    metric, objs, cam = rt.example2_scene()
    ni, nj = 60, 45
    canvas = rt.make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], ni, nj, dtype=np.float32)
    assert canvas.pixels.dtype.itemsize == 44
    out = rt.trace_rays(metric, objs, canvas)
    assert out.pixels.dtype == canvas.pixels.dtype and (canvas.pixels["rgb"] == 0).all()
    for f in ("pos", "normal"):
        assert np.array_equal(out.pixels[f], canvas.pixels[f]), f
    # planar entry point on the same start states
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults(np.float32)
    st = np.concatenate([canvas.pixels["pos"].reshape(-1, 4, order="F"), canvas.pixels["normal"].reshape(-1, 4, order="F")], axis=1)
    st = np.ascontiguousarray(st, np.float32)
    rgb = np.zeros((3, ni * nj), np.float32)
    abi.check(lib, lib.rtgr_trace_f32(None, C.byref(sc), C.byref(opt), st.ctypes.data, None, ni, nj, 0, nj, rgb.ctypes.data, None, None))
    got = out.pixels["rgb"].reshape(-1, 3, order="F")
    assert np.array_equal(got.T, rgb)
    with abi.options(lib, host_chunk=256):
        many = rt.trace_rays(metric, objs, canvas)
    assert np.array_equal(many.pixels["rgb"], out.pixels["rgb"])
    # against the Float64 canvas: same image up to Float32's global error (tests/test_truth.py prices it at <= 5e-4)
    c64 = rt.make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], ni, nj)
    o64 = rt.trace_rays(metric, objs, c64)
    d = np.abs(out.pixels["rgb"].astype(np.float64) - o64.pixels["rgb"])
    assert np.mean(d.max(axis=-1) < 2e-3) > 0.97       # (the rest: silhouette pixels and sawtooth wraps)
    p = rt.trace_ray(metric, objs, None, canvas.pixels[30, 22])
    assert p.dtype == canvas.pixels.dtype and np.array_equal(p["rgb"], out.pixels["rgb"][30, 22])


def _hip_runtime():
    """the HIP runtime already loaded in this process (torch's bundled libamdhip64)"""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return C.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")


def test_workspace_growth_and_stream_capture(lib):
    """(1) A workspace that must grow while its stream is being captured is an ERROR (hipMalloc cannot be captured), not
    a crash.  (2) A graph captured after rtgr_reserve_workspace keeps replaying correctly after the SAME stream's
    workspace has grown for a bigger job: the superseded buffer is retired, never freed under the graph."""
    import torch
    from raytracegr_jl_amd import sharded
    hip = _hip_runtime()
    sc, cam = example(2)
    opt = rt.solver_defaults()
    # (1)
    fresh = torch.cuda.Stream()
    rgb = torch.zeros((3, 64 * 64), dtype=torch.float64, device="cuda")
    graph = C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(fresh.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc = lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), 64, 64, 0, 64, rgb.data_ptr(),
                                   None, None, fresh.cuda_stream)
    msg = lib.rtgr_last_error()
    assert hip.hipStreamEndCapture(C.c_void_p(fresh.cuda_stream), C.byref(graph)) == 0
    if graph.value:
        hip.hipGraphDestroy(graph)
    assert rc == abi.ERR_BAD_ARG and b"rtgr_reserve_workspace" in msg
    # (2)
    ni = nj = 128
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
    with torch.cuda.stream(side):   # the same stream's workspace grows ...
        big = sharded.trace_slab_torch(sc, opt, cam, 512, 512, 0, 512)["rgb"]
    torch.cuda.synchronize()
    out["rgb"].zero_()
    g.replay()                      # ... and the graph, which references the retired buffer, still works
    torch.cuda.synchronize()
    assert torch.equal(out["rgb"], eager) and bool(torch.isfinite(big).all())
    abi.check(lib, lib.rtgr_trim(None))   # frees retired buffers (graph `g` must not be replayed afterwards)


def test_a_long_object_list_and_stream_capture(lib):
    """A list beyond the argument block lives in a device table that is uploaded the first time the list is seen (hipMalloc + a blocking
    copy: neither can be captured).  First sight DURING a capture is an error that says what to do; a list that has been traced once
    is captured and replayed like any scene — the table is found again by content, nothing is allocated."""
    import torch
    from raytracegr_jl_amd import sharded
    hip = _hip_runtime()
    sc, cam = scene_variant("ks_ref0_many64")
    opt = rt.solver_defaults()
    ni = nj = 96
    side = torch.cuda.Stream()
    out = {"rgb": torch.zeros((3, ni * nj), dtype=torch.float64, device="cuda")}
    abi.check(lib, lib.rtgr_reserve_workspace(None, out["rgb"].data_ptr(), side.cuda_stream, ni * nj, 0, 0))
    with abi.options(lib, groups=5):     # (a layout of the list no other test has asked for: its table does not exist yet)
        graph = C.c_void_p(None)
        assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0
        rc = lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), ni, nj, 0, nj, out["rgb"].data_ptr(), None, None,
                                       side.cuda_stream)
        msg = lib.rtgr_last_error()
        assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
        if graph.value:
            hip.hipGraphDestroy(graph)
        assert rc == abi.ERR_BAD_ARG and b"trace the scene once" in msg, msg
        eager = sharded.trace_slab_torch(sc, opt, cam, ni, nj, 0, nj)["rgb"].clone()     # first sight: the table is uploaded
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            sharded.trace_slab_torch(sc, opt, cam, ni, nj, 0, nj, out=out)
        out["rgb"].zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["rgb"], eager) and len(torch.unique(out["rgb"][2])) > 3
    again = sharded.trace_slab_torch(sc, opt, cam, ni, nj, 0, nj)["rgb"]          # (and the default layout gives the same frame)
    torch.cuda.synchronize()
    assert torch.equal(again, eager)


# ---- the reference's OWN call shape over every device of a context (src/RayTraceGR.jl:483-536, :596) -------
def _golden(name):
    from raytracegr_jl_amd.png import read_png
    return read_png(os.path.join(ROOT, "tests", "golden", name))


@pytest.mark.parametrize("ndev", [2, 3])
def test_trace_rays_drop_in_entry_uses_every_device_of_the_context(lib, ndev):
    """`trace_rays(metric, objs, canvas)` binds rtgr_trace_pixels_f64: on a context of N devices the call deals the
    canvas rows cyclically to ALL of them (each device uploads its own rows from the caller's Pixel array and downloads
    them straight back into it), and example2()'s image is still the reference's sphere2.png, 40000/40000 — and the
    Pixel array equals the single-device one bit for bit.  The per-device kernel timers prove that every device
    integrated something."""
    import torch
    metric, objs, cam = rt.example2_scene()
    ctx = abi.create_context(lib, _devices(ndev))
    try:
        canvas = rt.make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], 200, 200, ctx=ctx)
        single, info1 = rt.trace_rays(metric, objs, canvas, return_info=True)                 # default context: one device
        for k in range(ndev):
            abi.check(lib, lib.rtgr_timing_enable(ctx, k, 1))
        multi, infoN = rt.trace_rays(metric, objs, canvas, return_info=True, ctx=ctx)
        assert int((multi.image_u8() != _golden("sphere2.png")).any(axis=2).sum()) == 0
        assert multi.pixels.tobytes() == single.pixels.tobytes()
        assert infoN == info1 and info1["rays"] == 40000
        ms, launches = (C.c_double * 4)(), (C.c_uint64 * 4)()
        for k in range(ndev):
            abi.check(lib, lib.rtgr_timing_read(ctx, k, C.byref(ms), C.byref(launches)))
            assert launches[1] >= 1 and ms[1] > 0.0, f"device entry {k} of the context ran no integrate pass"
            abi.check(lib, lib.rtgr_timing_enable(ctx, k, 0))
        # in place (pixels_out aliases pixels_in) and Float32, ragged shares (77 rows over ndev devices)
        sc = rt.make_scene(metric, objs)
        c32 = rt.make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], 96, 77, dtype=np.float32)
        one32 = rt.trace_rays(metric, objs, c32)
        opt32 = rt.solver_defaults(np.float32)
        px = np.asfortranarray(c32.pixels).copy(order="F")
        ctr = abi.rtgr_counters()
        abi.check(lib, lib.rtgr_trace_pixels_f32(ctx, C.byref(sc), C.byref(opt32), px.ctypes.data, 96, 77, px.ctypes.data, C.byref(ctr)))
        assert px.tobytes() == np.asfortranarray(one32.pixels).tobytes() and ctr.rays == 96 * 77
        # legacy single-ray shape on a multi-device context: one row, one device
        p = canvas.pixels[99, 99]
        assert rt.trace_ray(metric, objs, None, p, ctx=ctx)["rgb"].tobytes() == single.pixels[99, 99]["rgb"].tobytes()
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_an_animated_long_list_starts_its_tables_over(lib):
    """Every distinct list leaves a device table (and the host copy it is found again by) behind until rtgr_trim: a caller that moves
    one object per frame piles them up.  Past OBJECT_TABLES_MAX lists (512) — or OBJECT_TABLES_BYTES (1 GiB: the same branch) — the
    device is synchronised and the tables start over; the frames do not notice.  600 frames of a 41-object list whose last object
    moves where no ray goes: every frame equals the first, bit for bit."""
    from scenes import many_objects
    metric, _, cam = rt.example2_scene()
    objs = many_objects(40)
    camera = rt.make_camera(**cam)
    opt = rt.solver_defaults()
    frames = []
    for k in range(600):
        sc = rt.make_scene(metric, objs + [rt.Sphere((0, 0.0, -400.0 - k, 0.0), (1, 0, 0, 0), 0.5)])   # outside the sky sphere: never seen
        rgb = np.zeros((3, 12 * 12))
        hit = np.zeros(144, np.uint8)
        o = abi.rtgr_ray_outputs()
        o.hit = hit.ctypes.data
        abi.check(lib, lib.rtgr_trace_f64(None, C.byref(sc), C.byref(opt), None, C.byref(camera), 12, 12, 0, 12, rgb.ctypes.data, C.byref(o), None))
        frames.append((rgb, hit))
    for rgb, hit in frames[1:]:
        assert np.array_equal(rgb, frames[0][0]) and np.array_equal(hit, frames[0][1])
    assert len(np.unique(frames[0][1])) > 4 and (frames[0][1] > 0).all() and int(frames[0][1].max()) <= 40
    abi.check(lib, lib.rtgr_trim(None))


def test_a_captured_long_list_keeps_its_table_when_the_tables_start_over(lib):
    """The table of a long list that a hipGraph was captured with is marked kept: when the tables start over (above) it stays, and the
    graph replays the same bits; rtgr_trim frees it with everything else a graph may replay.  The list and the canvas of the test above,
    Float64, on a side stream: traced once, captured, replayed; then OBJECT_TABLES_MAX + 8 = 520 further lists on the default stream, so
    the tables start over at least once; the hook (resident, kept) must show that they did and that the captured one was spared."""
    import torch
    from raytracegr_jl_amd import sharded
    from scenes import many_objects
    hook = lib.rtgr_testhook_object_tables
    hook.restype = C.c_int
    hook.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]

    def tables():
        resident, kept = C.c_uint32(99), C.c_uint32(99)
        abi.check(lib, hook(None, 0, C.byref(resident), C.byref(kept)))
        return resident.value, kept.value

    metric, _, cam = rt.example2_scene()
    objs = many_objects(40)
    camera = rt.make_camera(**cam)
    opt = rt.solver_defaults()
    ni = nj = 12

    def scene(k):
        return rt.make_scene(metric, objs + [rt.Sphere((0, 0.0, -400.0 - k, 0.0), (1, 0, 0, 0), 0.5)])   # outside the sky sphere: never seen

    torch.cuda.synchronize()
    abi.check(lib, lib.rtgr_trim(None))
    assert tables() == (0, 0)
    sc = scene(0)
    side = torch.cuda.Stream()
    out = {"rgb": torch.zeros((3, ni * nj), dtype=torch.float64, device="cuda"), "hit": torch.zeros(ni * nj, dtype=torch.uint8, device="cuda")}
    abi.check(lib, lib.rtgr_reserve_workspace(None, out["rgb"].data_ptr(), side.cuda_stream, ni * nj, 0, 0))
    with torch.cuda.stream(side):
        eager = sharded.trace_slab_torch(sc, opt, camera, ni, nj, 0, nj, hit_only=True)      # first sight: the table is uploaded
    torch.cuda.synchronize()
    eager = {k: v.clone() for k, v in eager.items()}
    assert len(torch.unique(eager["hit"])) > 4                                              # (the list is on screen)
    assert tables() == (1, 0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        sharded.trace_slab_torch(sc, opt, camera, ni, nj, 0, nj, out=out, hit_only=True)
    assert tables() == (1, 1)

    def replay_equals_eager():
        out["rgb"].zero_()
        out["hit"].zero_()
        g.replay()
        torch.cuda.synchronize()
        return torch.equal(out["rgb"], eager["rgb"]) and torch.equal(out["hit"], eager["hit"])

    assert replay_equals_eager()
    other = {}
    for k in range(1, 521):
        sharded.trace_slab_torch(scene(k), opt, camera, ni, nj, 0, nj, out=other, hit_only=True)
    torch.cuda.synchronize()
    assert torch.equal(other["rgb"], eager["rgb"]) and torch.equal(other["hit"], eager["hit"])
    resident, kept = tables()
    assert kept == 1 and resident < 521, (resident, kept)       # the tables started over, and the captured one was spared
    assert replay_equals_eager()
    del g
    torch.cuda.synchronize()
    abi.check(lib, lib.rtgr_trim(None))
    assert tables() == (0, 0)


def test_a_long_object_list_over_every_device_of_a_context(lib):
    """The device table of a long list (and its groups) is per device: a three-device context deals the rows of a 64-object scene
    cyclically, every device uploads its own table on first sight, and the canvas equals the single-device one bit for bit — Float64
    and Float32 (which runs FAR + NEAR from 32 objects on), and again on the second call, when the tables are found by content."""
    from scenes import many_objects
    metric, _, cam = rt.example2_scene()
    objs = many_objects(64)
    ctx = abi.create_context(lib, _devices(3))
    try:
        for dtype in (np.float64, np.float32):
            canvas = rt.make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], 96, 77, dtype=dtype)
            single = rt.trace_rays(metric, objs, canvas)
            for _ in range(2):
                multi, info = rt.trace_rays(metric, objs, canvas, return_info=True, ctx=ctx)
                assert multi.pixels.tobytes() == single.pixels.tobytes() and info["rays"] == 96 * 77
            assert len(np.unique(single.pixels["rgb"][..., 2])) > 8      # (the blue channel is omin / 64: many objects on screen)
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


@pytest.mark.parametrize("ndev", [2, 4])
def test_host_entry_with_caller_rays_and_every_output_over_all_devices(lib, ndev):
    """rtgr_trace_f64 with caller-supplied states (`input_func(i)`, :492-496) and a row slab [j0, j1), every per-ray
    output requested, on an N-device context == the single-device call, bit for bit; likewise from a camera."""
    import torch
    from test_gpu_parity import hip_trace
    sc, cam = scene_variant("ks_true08")
    opt = rt.solver_defaults()
    ni, nj, j0, j1 = 80, 61, 5, 58
    st = np.zeros((ni * nj, 8))
    abi.check(lib, lib.rtgr_make_canvas_f64(None, C.byref(sc), C.byref(cam), ni, nj, 0, nj, st.ctypes.data))
    slab = np.ascontiguousarray(st[j0 * ni:j1 * ni])
    ref_s = hip_trace(lib, sc, opt, ni, nj, j0, j1, state0=slab)
    ref_c = hip_trace(lib, sc, opt, ni, nj, j0, j1, cam=cam)
    ctx = abi.create_context(lib, _devices(ndev))
    try:
        n = ni * (j1 - j0)
        for ref, s0, cm in ((ref_s, slab.ctypes.data, None), (ref_c, None, C.byref(cam))):
            rgb = np.zeros((3, n))
            o, arrs = O._outs(n, np.float64, True)
            ctr = abi.rtgr_counters()
            abi.check(lib, lib.rtgr_trace_f64(ctx, C.byref(sc), C.byref(opt), s0, cm, ni, nj, j0, j1, rgb.ctypes.data,
                                              C.byref(o), C.byref(ctr)))
            assert np.array_equal(rgb, ref["rgb"])
            for k in OUT_KEYS[1:]:
                assert np.array_equal(arrs[k], ref[k]), k
            assert ctr.as_dict() == ref["counters"]
        # a NaN in ONE device's rows is the whole call's error, with the device named (the reference asserts, :279)
        bad = slab.copy()
        bad[3 * ni + 7, 2] = np.nan       # slab row 3 -> device entry 3 % ndev
        rgb = np.zeros((3, n))
        rc = lib.rtgr_trace_f64(ctx, C.byref(sc), C.byref(opt), bad.ctypes.data, None, ni, nj, j0, j1, rgb.ctypes.data, None, None)
        assert rc == abi.ERR_NAN_INPUT and b"entry %d of the context" % (3 % ndev) in lib.rtgr_last_error()
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_gather_without_peer_access_and_peer_option(lib):
    """rtgr_trace_sharded_device_*: option peer = 0 forces the no-peer-access fallback (rows travel device -> pinned host
    -> device 0) — also between entries of one physical device, which is how it is exercised on a one-GPU box; peer = 1
    insists on peer copies.  Same frame, bit for bit, either way."""
    import torch
    from test_gpu_parity import hip_trace
    sc, cam = scene_variant("ks_ref0")
    opt = rt.solver_defaults()
    ni, nj = 72, 50
    n = ni * nj
    ref = hip_trace(lib, sc, opt, ni, nj, cam=cam)
    ctx = abi.create_context(lib, _devices(3))
    try:
        for peer in (0, 1, -1):
            abi.check(lib, lib.rtgr_set_option(ctx, b"peer", peer))
            d_rgb = torch.zeros((3, n), dtype=torch.float64, device="cuda")
            d_se = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
            d_hit = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
            od = abi.rtgr_ray_outputs()
            od.state_end, od.hit = d_se.data_ptr(), d_hit.data_ptr()
            ctr = abi.rtgr_counters()
            abi.check(lib, lib.rtgr_trace_sharded_device_f64(ctx, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj,
                                                             d_rgb.data_ptr(), C.byref(od), C.byref(ctr)))
            assert np.array_equal(d_rgb.cpu().numpy(), ref["rgb"]), peer
            assert np.array_equal(d_se.cpu().numpy(), ref["state_end"]) and np.array_equal(d_hit.cpu().numpy(), ref["hit"])
            assert ctr.as_dict() == ref["counters"]
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def test_trim_while_host_calls_are_in_flight(lib):
    """rtgr_trim frees retired workspaces and the staging BUFFERS; a host-pointer call in flight on another thread holds
    the staging for its whole duration, so trimming must wait for it, not free under it."""
    from test_gpu_parity import hip_trace
    sc, cam = scene_variant("ks_ref0")
    opt = rt.solver_defaults()
    ref = hip_trace(lib, sc, opt, 160, 120, cam=cam)
    stop, errors = threading.Event(), []

    def trimmer():
        while not stop.is_set():
            if lib.rtgr_trim(None) != 0:
                errors.append(lib.rtgr_last_error())

    th = threading.Thread(target=trimmer)
    th.start()
    try:
        for _ in range(6):
            got = hip_trace(lib, sc, opt, 160, 120, cam=cam)
            assert np.array_equal(got["rgb"], ref["rgb"]) and got["counters"] == ref["counters"]
    finally:
        stop.set()
        th.join()
    assert not errors, errors


def test_peer_table_and_exchange_timers(lib):
    """What makes a first multi-GPU run diagnosable (VERDICT r3 #3b): rtgr_peer_access reports, per device of the context, whether
    its rows reach device 0 by peer copy (the same physical GPU counts as one) and why not otherwise; with timing enabled the
    sharded call's exchange is timed per device — rows leaving a device on ITS stream, placement on device 0 — and the option
    peer = 0 (rows through pinned host memory) is timed the same way."""
    import torch
    sc, cam = example(2)
    opt = rt.solver_defaults()
    ni, nj, nd = 128, 96, 3
    ids = _devices(nd)
    ctx = abi.create_context(lib, ids)
    try:
        why = C.create_string_buffer(256)
        for k in range(nd):
            ok = lib.rtgr_peer_access(ctx, k, why, 256)
            assert ok in (0, 1)
            assert ok == 1 or why.value, k                      # no peer access: the reason is recorded
            if ids[k] == ids[0]:
                assert ok == 1
        assert lib.rtgr_peer_access(ctx, nd, why, 256) == abi.ERR_BAD_ARG
        d0 = torch.device("cuda", ids[0])
        d_rgb = torch.zeros((3, ni * nj), dtype=torch.float64, device=d0)
        for peer in (-1, 0):
            abi.check(lib, lib.rtgr_set_option(ctx, b"peer", peer))
            for k in range(nd):
                abi.check(lib, lib.rtgr_timing_enable(ctx, k, 1))
            ctr = abi.rtgr_counters()
            abi.check(lib, lib.rtgr_trace_sharded_device_f64(ctx, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, d_rgb.data_ptr(), None, C.byref(ctr)))
            assert ctr.rays == ni * nj
            for k in range(nd):
                ms, ln = (C.c_double * 2)(), (C.c_uint64 * 2)()
                abi.check(lib, lib.rtgr_timing_read_exchange(ctx, k, C.byref(ms), C.byref(ln)))
                assert ln[0] == (1 if k > 0 else 0) and (ms[0] > 0.0) == (k > 0), (peer, k, ms[0], ln[0])
                assert ln[1] == (nd if k == 0 else 0) and (ms[1] > 0.0) == (k == 0), (peer, k, ms[1], ln[1])
                kms, kln = (C.c_double * 4)(), (C.c_uint64 * 4)()
                abi.check(lib, lib.rtgr_timing_read(ctx, k, C.byref(kms), C.byref(kln)))
                assert kln[1] >= 1 and kms[1] > 0.0             # this device's own FAR pass
                abi.check(lib, lib.rtgr_timing_read_exchange(ctx, k, C.byref(ms), C.byref(ln)))
                assert ln[0] == 0 and ln[1] == 0                # read = reset
                abi.check(lib, lib.rtgr_timing_enable(ctx, k, 0))
    finally:
        abi.check(lib, lib.rtgr_destroy(ctx))


def _cameras(k):
    """k cameras on a short dolly around example2's: every frame another picture"""
    _, _, cam = rt.example2_scene()
    return [dict(cam, pos=(0, 4 + 0.15 * i, -2 - 0.1 * i, 0.05 * i)) for i in range(k)]


@pytest.mark.parametrize("ndev", [0, 3])
def test_frames_in_flight_are_the_single_frames(lib, ndev):
    """rtgr_trace_frames_f64 / _f32: several frames of one scene in ONE blocking call, two in flight inside the library (two
    pipelines per device: staging, streams, workspace) — what a caller with two HIP streams could always do, for the callers of the
    blocking entry points (Julia, C).  No reference counterpart (example1 / example2 render one frame per call,
    src/RayTraceGR.jl:560, :596).  Every frame — RGB and all per-ray outputs, counters — is the frame of the single call, bit for
    bit; on the default context and on one of three (logical) devices, where the rows of EVERY frame are dealt to all devices."""
    from test_gpu_parity import hip_trace
    metric, objs, _ = rt.example2_scene(rt.KerrSchild(1.0, 0.8))
    cams = _cameras(5)
    ctx = abi.create_context(lib, _devices(ndev)) if ndev else None
    try:
        frames = rt.trace_frames(metric, objs, cams, 96, 80, ctx=ctx, details=True)
        sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
        for k, f in enumerate(frames):
            single = hip_trace(lib, sc, opt, 96, 80, cam=rt.make_camera(**cams[k]))
            for key in OUT_KEYS:
                assert np.array_equal(f[key], single[key], equal_nan=True), (k, key)
            assert f["counters"] == single["counters"], k
        assert not np.array_equal(frames[0]["rgb"], frames[3]["rgb"])          # (the cameras differ: so do the frames)
        # Float32, one frame (no second frame to overlap with: the plain call on the first pipeline)
        f32 = rt.trace_frames(metric, objs, cams[:1], 64, 64, dtype=np.float32, ctx=ctx)[0]
        s32 = hip_trace(lib, sc, rt.solver_defaults(np.float32), 64, 64, cam=rt.make_camera(**cams[0]), dtype=np.float32)
        assert np.array_equal(f32["rgb"], s32["rgb"]) or ctx is not None     # (hip_trace runs on the default context: same bits there)
    finally:
        if ctx:
            abi.check(lib, lib.rtgr_destroy(ctx))


def test_frames_in_flight_of_a_long_object_list(lib):
    """Two frames in flight run on two host threads inside the library: both convert the same 64-object list, find (or, the first of
    them, upload) its one device table under the device's lock, and trace.  Five frames of five cameras equal the five single calls."""
    from scenes import many_objects
    from test_gpu_parity import hip_trace
    metric, _, _ = rt.example2_scene()
    objs = many_objects(64, seed=12)                     # (a list no other test has traced: its table is uploaded inside this call)
    cams = _cameras(5)
    frames = rt.trace_frames(metric, objs, cams, 80, 64, details=True)
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    for k, f in enumerate(frames):
        single = hip_trace(lib, sc, opt, 80, 64, cam=rt.make_camera(**cams[k]))
        for key in OUT_KEYS:
            assert np.array_equal(f[key], single[key], equal_nan=True), (k, key)
        assert f["counters"] == single["counters"], k
    assert len(np.unique(frames[0]["hit"])) > 8


def test_frames_of_pixel_arrays_and_the_error_path(lib):
    """The _pixels twin takes the reference's own Array{Pixel{T},2} per frame (src/RayTraceGR.jl:446-450, :532) — three canvases of three
    cameras in one call equal three trace_rays calls; a frame with a NULL array is refused with its number before anything runs."""
    metric, objs, _ = rt.example2_scene()
    cams = _cameras(3)
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    canv = [rt.make_canvas(metric, c["pos"], c["widthx"], c["widthy"], c["normal"], 72, 60) for c in cams]
    want = [rt.trace_rays(metric, objs, c) for c in canv]
    pin = [np.asfortranarray(c.pixels) for c in canv]
    pout = [np.empty_like(p, order="F") for p in pin]
    K = len(pin)
    a_in = (C.c_void_p * K)(*[p.ctypes.data for p in pin])
    a_out = (C.c_void_p * K)(*[p.ctypes.data for p in pout])
    ctrs = (abi.rtgr_counters * K)()
    abi.check(lib, lib.rtgr_trace_frames_pixels_f64(None, C.byref(sc), C.byref(opt), K, a_in, 72, 60, a_out, ctrs))
    for k in range(K):
        assert np.array_equal(pout[k]["rgb"], want[k].pixels["rgb"]) and np.array_equal(pout[k]["pos"], pin[k]["pos"]), k
        assert ctrs[k].rays == 72 * 60
    a_out[1] = None
    assert lib.rtgr_trace_frames_pixels_f64(None, C.byref(sc), C.byref(opt), K, a_in, 72, 60, a_out, None) == abi.ERR_BAD_ARG
    assert "frame 1" in lib.rtgr_last_error().decode()
    rgb = np.zeros((3, 16))
    one = (C.c_void_p * 1)(rgb.ctypes.data)
    assert lib.rtgr_trace_frames_f64(None, C.byref(sc), C.byref(opt), 1, None, None, 4, 4, one, None, None) == abi.ERR_BAD_ARG   # neither cameras nor rays
    assert lib.rtgr_trace_frames_f64(None, C.byref(sc), C.byref(opt), 0, None, None, 4, 4, one, None, None) == abi.ERR_BAD_ARG
