#!/usr/bin/env python3
"""What disk emission costs (rtgr_trace_emission_device_f64): BASELINE config 5's scene — KerrSchild(1, 0.998), caelum,
the far plane, Disk(0.05, 2, 4), example2's camera — Float64; per size, ms per frame of
    plain         one ray through each pixel centre, no per-ray output (rtgr_trace_device_f64) — the trace is untouched by this
                  feature, so this IS the frame of the commit before it
    plain+state   the same with state_end and hit32 delivered (what the emission kernel reads)
    emitted       rtgr_trace_emission_device_f64 with d_g: plain+state into the stream's scratch, then the emission kernel
the ratios emitted / plain and plain+state / plain, the emission pass by itself (emitted - plain+state, and from the library's kernel
timers: rtgr_timing_read's set-up slot holds the emission kernel beside the ray set-up kernels, so its share is the difference of that
slot between an emitted and a plain+state frame), and the fraction of pixels on the disk.

Runs are interleaved (one frame of every rendering per round) and the medians reported with the spread.

    python tools/emission_cost.py [--rounds 9] [--sizes 1024] [--json out.json]
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
    _, objs, cam = rt.example2_scene()
    objs = objs[:2] + [rt.Disk(0.05, 2.0, 4.0)]
    cam = rt.make_camera(**cam)
    opt = rt.solver_defaults()
    sc = rt.make_scene(rt.KerrSchild(1.0, 0.998), objs)
    em = rt.DiskEmission(3, 30000.0, inner_edge=True)
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "rows": []}

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
        g = torch.zeros(n, dtype=torch.float64, device="cuda")
        state = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        hit32 = torch.zeros(n, dtype=torch.int32, device="cuda")
        o = abi.rtgr_ray_outputs()
        o.state_end, o.hit32 = state.data_ptr(), hit32.data_ptr()

        def plain():
            abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), N, N, 0, N, rgb.data_ptr(), None, None, stream()))

        def plain_state():
            abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), N, N, 0, N, rgb.data_ptr(), C.byref(o), None, stream()))

        def emitted():
            abi.check(lib, lib.rtgr_trace_emission_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), N, N, None, C.byref(em), None, rgb.data_ptr(),
                                                              None, g.data_ptr(), None, None, None, stream()))

        runs = {"plain": plain, "plain_state": plain_state, "emitted": emitted}
        times, wall = {r: [] for r in runs}, {r: [] for r in runs}
        for r in runs:          # warm-up: workspace and scratch
            runs[r]()
        torch.cuda.synchronize()
        fraction = float((hit32 == 3).float().mean())
        valid = float(torch.isfinite(g).float().mean())
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
        row = dict(size=N, disk_fraction=fraction, emitting_fraction=valid, ratio_emitted=med["emitted"] / med["plain"],
                   ratio_plain_state=med["plain_state"] / med["plain"], emission_pass_ms=med["emitted"] - med["plain_state"],
                   emission_pass_timer_ms=parts["emitted"]["setup_ms"] - parts["plain_state"]["setup_ms"], kernel_timers=parts)
        for r in runs:
            t = np.array(times[r])
            row[r] = dict(median_ms=med[r], min_ms=float(t.min()), max_ms=float(t.max()), wall_median_ms=float(np.median(wall[r])))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        print(f"config 5 {N}², the disk emitting ({fraction:.1%} of the pixels, {valid:.1%} with an orbit): plain {med['plain']:.2f} ms, "
              f"plain+state {med['plain_state']:.2f} ms, emitted {med['emitted']:.2f} ms; emitted / plain = {row['ratio_emitted']:.3f}, "
              f"plain+state / plain = {row['ratio_plain_state']:.3f}, emission pass {row['emission_pass_timer_ms']:.3f} ms by the kernel timers", flush=True)
        del rgb, g, state, hit32
        abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
