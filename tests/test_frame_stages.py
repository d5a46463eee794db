"""What the frame calls share (csrc/rtgr_frame_host.hip): the layout of a stream's frame scratch, checked by a host-only program built
against csrc/rtgr_internal.hpp alone, and — on the GPU — that ONE frame scratch and ONE batch scratch per stream serve the shaded, emitted,
anti-aliased and observer frames in turn without a captured graph ever losing the scratch it was captured with."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from scenes import rt

abi = rt._abi
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_frame_scratch_layout(tmp_path):
    """every combination of the three borrowed blocks x (plain, anti-aliased, observer) front matter x n in {1, 77, 2496, 1000003} x
    sizeof(R) in {4, 8}: each block 256-aligned, inside the total, disjoint from the others, an absent block no bytes, the head holds
    rtgr_counters and the observer's block ObsFrame<double> (tests/c/frame_layout.cpp).  No device: nothing but the header is linked."""
    exe = str(tmp_path / "frame_layout")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "raytracegr.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "frame_layout.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == f"{4 * 2 * 3 * 8} cases"


def test_reduce_scratch_layout(tmp_path):
    """the reduction scratch of light curves and spectra: n in {1, 77, 2496, 1000003} x sizeof(R) in {4, 8} x head in {0, 1024} x items in
    {1, 1024, 70000} x the 8 combinations of planes the caller gave: every offset equals the formula the two features each wrote out
    before there was one layout, each block 256-aligned, inside the total, disjoint from the others, an absent plane no bytes
    (tests/c/reduce_layout.cpp).  No device: nothing but the headers is linked."""
    exe = str(tmp_path / "reduce_layout")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "raytracegr.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "reduce_layout.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == f"{4 * 2 * 2 * 3 * 8} cases"


def test_the_path_from_a_frame_to_a_table_is_written_once():
    """light curves and spectra share one scratch, one staged copy-out and one layout of the borrowed planes: each of these lines stands
    in exactly one file of csrc/ (the two features' host files hold none of them)"""
    csrc = os.path.join(ROOT, "raytracegr.jl_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp"))}

    def homes(line):
        return [f for f, t in texts.items() if line in t]

    # (the frame scratch of rtgr_frame_host.hip has a refusal of its own, which ends where this one goes on with the advice)
    assert homes("scratch must grow but the stream is being captured") == ["rtgr_frame_host.hip", "rtgr_reduce_host.hip"]
    assert homes('scratch must grow but the stream is being captured: make a "') == ["rtgr_reduce_host.hip"]
    assert homes("hipMemcpyDeviceToHost));   // (staged_frame has synchronised its stream)") == ["rtgr_reduce_host.hip"]
    assert homes("align256((size_t)n * 8 * scalar)") == ["rtgr_internal.hpp"] and homes("align256((size_t)n * 8 * sizeof(R))") == []
    for f in ("rtgr_lightcurve_host.hip", "rtgr_spectrum_host.hip"):
        for word in ("scratch_need", "staged_frame", "align256", "capture_check", "trace_observer_device"):
            assert word not in texts[f], (f, word)


@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


@pytest.mark.gpu
def test_one_scratch_serves_every_entry_and_never_dangles(lib):
    """One side stream, Float64, test_emission.py's a = 0.998 disk scene with a texture on the sky, 24 x 16.  A shaded frame is captured;
    then, eagerly and with no synchronisation in between, the same stream runs an emitted frame twice as wide (the frame scratch grows:
    the captured one is retired, not freed), an observer frame in four batches and an anti-aliased emitted frame (the batch scratch
    serves both).  The graph still replays the eager shaded frame, and after rtgr_trim a fresh call gives it again; each of the three
    other frames is its host entry point's, bit for bit; growing the scratch DURING the capture is refused."""
    import torch
    from test_emission import T_FRAME, _scene, emission, emitted
    from test_observer import trace_observer
    from test_textures import BILINEAR, _hip_runtime, texture
    _, tex = texture("rand32x16")
    binds = {1: (tex, BILINEAR)}
    metric, objs, cam, _ = _scene("a0998")
    sc, opt = rt.make_scene(metric, objs), rt.solver_defaults()
    em, sh = emission(3, T_FRAME), rt.make_shade(binds)
    ob = rt.Observer((0, 0, -8, 1.0), (0, 0, 1, -0.1), (0, 0, 0, 1), 1.0, 0.7, max_batch_rays=96)   # 96 rays: four rows of 24, four batches
    aa = abi.rtgr_aa(k=2, flags=0, contrast=0.05, max_batch_rays=0)
    ni, nj = 24, 16
    n = ni * nj
    # what the host entry points give for the three other frames
    host_em = emitted(lib, "a0998", 2 * ni, nj, em, binds=binds, details=False, counters=False)
    rc, host_ob = trace_observer(lib, metric, objs, ob, ni, nj, emit=em, binds=binds, details=False, counters=False)
    assert rc == 0
    host_aa = emitted(lib, "a0998", ni, nj, em, binds=binds, aa=dict(k=2, contrast=0.05), details=False, counters=False)
    assert 0 < host_aa["stats"]["refined"] < n

    side = torch.cuda.Stream()
    s = side.cuda_stream
    hip = _hip_runtime()
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda")

    def shaded(out):
        return lib.rtgr_trace_shaded_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), ni, nj, C.byref(sh), None, out.data_ptr(), None, None, None,
                                                None, s)

    def emitted_on(out, g, width, aap=None, refined=None, stats=None):
        return lib.rtgr_trace_emission_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), width, nj, C.byref(sh), C.byref(em), aap, out.data_ptr(),
                                                  None, g.data_ptr(), refined.data_ptr() if refined is not None else None, None, stats, s)

    with torch.cuda.stream(side):
        eager, out, fresh, ob_rgb, aa_rgb = (z(3, n) for _ in range(5))
        ob_g, aa_g = z(n), z(n)
        em_rgb, em_g = z(3, 2 * n), z(2 * n)
        refined = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    abi.check(lib, shaded(eager))                              # the warm-up: workspace and scratch of this size exist afterwards
    torch.cuda.synchronize()
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(s), 2) == 0    # hipStreamCaptureModeRelaxed
    rc_big = emitted_on(em_rgb, em_g, 2 * ni)                  # another entry, a larger frame: the shared scratch would have to grow
    msg_big = lib.rtgr_last_error()
    rc = shaded(out)
    assert hip.hipStreamEndCapture(C.c_void_p(s), C.byref(graph)) == 0
    assert rc == 0 and rc_big == abi.ERR_BAD_ARG and b"captured" in msg_big and b"rtgr_trace_emission" in msg_big
    assert graph.value and hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    # three other entries on the same stream, none waited for
    stats = abi.rtgr_aa_stats()
    abi.check(lib, emitted_on(em_rgb, em_g, 2 * ni))
    abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, C.byref(sh), C.byref(em), ob_rgb.data_ptr(), None,
                                                      ob_g.data_ptr(), None, s))
    abi.check(lib, emitted_on(aa_rgb, aa_g, ni, C.byref(aa), refined, C.byref(stats)))
    assert hip.hipGraphLaunch(exe, C.c_void_p(s)) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and bool((eager != 0).any())
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, shaded(fresh))
    torch.cuda.synchronize()
    assert torch.equal(fresh, eager)
    bits = lambda t: t.cpu().numpy().tobytes()
    assert bits(em_rgb) == host_em["rgb"].tobytes() and bits(em_g) == host_em["g"].tobytes()
    assert bits(ob_rgb) == host_ob["rgb"].tobytes() and bits(ob_g) == host_ob["g"].tobytes()
    assert bits(aa_rgb) == host_aa["rgb"].tobytes() and bits(aa_g) == host_aa["g"].tobytes() and bits(refined) == host_aa["refined"].tobytes()
    assert stats.as_dict() == host_aa["stats"]
    # the frames differ from each other: none of the comparisons above is of a frame with itself
    assert not np.array_equal(host_ob["rgb"], host_aa["rgb"]) and not np.array_equal(host_aa["rgb"], eager.cpu().numpy())
