#!/usr/bin/env python3
"""What the observer camera costs (rtgr_trace_observer_device_f64): KerrSchild(1, 0.998) with BASELINE config 5's disk
inside a sky sphere of radius 20, seen from the prograde circular orbit at rho = 12 (an equirectangular panorama: the hole and the
disk are in the picture), Float64; per size, ms per frame of
    states        rtgr_trace_device_f64 fed the observer's states as d_state0 (written once, by rtgr_make_observer_canvas_device_f64) —
                  the trace is untouched by this feature, so this IS the path of the commit before it
    observer      rtgr_trace_observer_device_f64: the frame kernel, the ray kernel into the stream's scratch, the same trace
    emitted       the same with the disk emitting and d_g
the ratios observer / states and emitted / states, and the two new kernels by the library's timers (rtgr_timing_read's set-up slot holds
them beside the ray set-up kernels: their share is the difference of that slot between an observer frame and a states frame).

Runs are interleaved (one frame of every rendering per round) and the medians reported with the spread.

    python tools/observer_cost.py [--rounds 9] [--sizes 1024] [--json out.json]
"""
import argparse
import ctypes as C
import importlib.util
import json
import math
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
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -20.0), rt.Plane(-60.0), rt.Disk(0.05, 2.0, 4.0)]
    opt = rt.solver_defaults()
    sc = rt.make_scene(rt.KerrSchild(1.0, 0.998), objs)
    em = rt.DiskEmission(3, 30000.0, inner_edge=True)
    ob = rt.Observer((0, 0, -12, 0), (0, 1, 0, 0), (0, 0, 0, 1), 2 * math.pi, math.pi, kind="circular", projection="equirect")
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
        states = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        hit32 = torch.zeros(n, dtype=torch.int32, device="cuda")
        o = abi.rtgr_ray_outputs()
        o.hit32 = hit32.data_ptr()
        abi.check(lib, lib.rtgr_make_observer_canvas_device_f64(None, C.byref(sc), C.byref(ob), N, N, 0, N, states.data_ptr(), stream()))

        def from_states():
            abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), states.data_ptr(), None, N, N, 0, N, rgb.data_ptr(), None, None, stream()))

        def observer():
            abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, None, rgb.data_ptr(), None, None, None,
                                                              stream()))

        def emitted():
            abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, C.byref(em), rgb.data_ptr(), None,
                                                              g.data_ptr(), None, stream()))

        runs = {"states": from_states, "observer": observer, "emitted": emitted}
        times, wall = {r: [] for r in runs}, {r: [] for r in runs}
        for r in runs:          # warm-up: workspace and scratch
            runs[r]()
        abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), states.data_ptr(), None, N, N, 0, N, rgb.data_ptr(), C.byref(o), None, stream()))
        torch.cuda.synchronize()
        fraction = float((hit32 == 3).float().mean())
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
        row = dict(size=N, disk_fraction=fraction, ratio_observer=med["observer"] / med["states"], ratio_emitted=med["emitted"] / med["states"],
                   new_kernels_timer_ms=parts["observer"]["setup_ms"] - parts["states"]["setup_ms"], kernel_timers=parts)
        for r in runs:
            t = np.array(times[r])
            row[r] = dict(median_ms=med[r], min_ms=float(t.min()), max_ms=float(t.max()), wall_median_ms=float(np.median(wall[r])))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        print(f"observer at rho = 12, {N}² ({fraction:.1%} of the pixels on the disk): states {med['states']:.2f} ms, observer {med['observer']:.2f} ms, "
              f"emitted {med['emitted']:.2f} ms; observer / states = {row['ratio_observer']:.3f}, emitted / states = {row['ratio_emitted']:.3f}, "
              f"frame + ray kernels {row['new_kernels_timer_ms']:.3f} ms by the kernel timers", flush=True)
        del rgb, g, states, hit32
        abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
