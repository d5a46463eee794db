#!/usr/bin/env python3
"""What image textures cost (rtgr_trace_shaded_device_f64): example2's scene, Float64, the sky sphere `caelum` bound
BILINEAR to a seeded 1024 x 512 texture; per size, ms per frame of
    plain         one ray through each pixel centre, no per-ray output (rtgr_trace_device_f64) — the trace is untouched by this
                  feature, so this IS the frame of the commit before it
    plain+state   the same with state_end, hit32 and status delivered (what the shading kernel reads: the pipeline then carries the
                  44-wide event record and 373 instead of 213 B of workspace per ray)
    shaded        rtgr_trace_shaded_device_f64: plain+state into the stream's scratch, then the shading kernel
the ratios shaded / plain and plain+state / plain, the shading pass by itself (shaded - plain+state, and from the library's kernel timers:
rtgr_timing_read's set-up slot holds the shading kernel beside the ray set-up kernels, so its share is the difference of that slot
between a shaded and a plain+state frame), and the fraction of pixels shaded.

Runs are interleaved (one frame of every rendering per round) and the medians reported with the spread.

    python tools/texture_cost.py [--rounds 9] [--sizes 1024] [--json out.json]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_package():
    name = "raytracegr_jl_amd"
    if name in sys.modules:
        return sys.modules[name]
    pkg = os.path.join(ROOT, "raytracegr.jl_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="1024")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    rt = load_package()
    abi = rt._abi
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    metric, objs, cam = rt.example2_scene()
    cam = rt.make_camera(**cam)
    opt = rt.solver_defaults()
    sc = rt.make_scene(metric, objs)
    tex = rt.texture_load(np.random.default_rng(1).uniform(0.0, 1.0, size=(3, 512, 1024)))
    sh = rt.make_shade({1: (tex, abi.TEX_BILINEAR)})
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "texture": [1024, 512], "rows": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    for N in (int(v) for v in args.sizes.split(",")):
        n = N * N
        rgb = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        state = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        hit32 = torch.zeros(n, dtype=torch.int32, device="cuda")
        status = torch.zeros(n, dtype=torch.uint8, device="cuda")
        o = abi.rtgr_ray_outputs()
        o.state_end, o.hit32, o.status = state.data_ptr(), hit32.data_ptr(), status.data_ptr()

        def plain():
            abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), N, N, 0, N, rgb.data_ptr(), None, None, stream()))

        def plain_state():
            abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), N, N, 0, N, rgb.data_ptr(), C.byref(o), None, stream()))

        def shaded():
            abi.check(lib, lib.rtgr_trace_shaded_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), N, N, C.byref(sh), None, rgb.data_ptr(), None,
                                                            None, None, None, stream()))

        runs = {"plain": plain, "plain_state": plain_state, "shaded": shaded}
        times, wall = {r: [] for r in runs}, {r: [] for r in runs}
        for r in runs:          # warm-up: workspace and scratch
            runs[r]()
        torch.cuda.synchronize()
        fraction = float((hit32 == 1).float().mean())
        for _ in range(args.rounds):   # interleaved
            for r in runs:
                ms, w = timed(runs[r])
                times[r].append(ms)
                wall[r].append(w)
        # one more frame of each under the library's kernel timers
        abi.check(lib, lib.rtgr_timing_enable(None, 0, 1))
        ms4, n4 = (C.c_double * 4)(), (C.c_uint64 * 4)()
        abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms4), C.byref(n4)))
        parts = {}
        for r in runs:
            runs[r]()
            torch.cuda.synchronize()
            abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms4), C.byref(n4)))
            parts[r] = dict(setup_ms=ms4[0], main_ms=ms4[1], resolve_ms=ms4[2], near_ms=ms4[3], launches=[int(v) for v in n4])
        abi.check(lib, lib.rtgr_timing_enable(None, 0, 0))
        med = {r: float(np.median(times[r])) for r in runs}
        row = dict(size=N, shaded_fraction=fraction, ratio_shaded=med["shaded"] / med["plain"], ratio_plain_state=med["plain_state"] / med["plain"],
                   shading_pass_ms=med["shaded"] - med["plain_state"],
                   shading_pass_timer_ms=parts["shaded"]["setup_ms"] - parts["plain_state"]["setup_ms"], kernel_timers=parts)
        for r in runs:
            t = np.array(times[r])
            row[r] = dict(median_ms=med[r], min_ms=float(t.min()), max_ms=float(t.max()), wall_median_ms=float(np.median(wall[r])))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        print(f"example2 {N}², caelum textured ({fraction:.1%} of the pixels): plain {med['plain']:.2f} ms, plain+state {med['plain_state']:.2f} ms, "
              f"shaded {med['shaded']:.2f} ms; shaded / plain = {row['ratio_shaded']:.3f}, plain+state / plain = {row['ratio_plain_state']:.3f}, "
              f"shading pass {row['shading_pass_timer_ms']:.3f} ms by the kernel timers", flush=True)
        del rgb, state, hit32, status
        abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
