#!/usr/bin/env python3
"""What a polarized disk image costs (rtgr_trace_polarized_device_f64): the light-curve cost table's scene —
KerrSchild(1, 0.998) with BASELINE config 5's disk, seen by a static observer at rho = 50, 60 degrees from the axis, through a perspective
window that the disk fills about a tenth of —; Float64; per size, ms of
    plain           rtgr_trace_observer_device_f64 without emission: the trace and the camera's kernels alone
    frame           the same with the disk emitting and every plane the stage reads.  The trace is untouched by this feature: this is the
                    path of the commit before it
    polarized       rtgr_trace_polarized_device_f64: the same frame, plus q, u, aux
    stage           rtgr_polarization_device_f64 alone over the frame's planes (the frame kernel and the polarization kernel)
Beside the wall times (HIP events around each call) the library's own kernel timers (rtgr_timing_read, slot 0: the small kernels) are read
per call: emit_kernel = frame - plain, polarize_kernel = polarized - frame in that slot, and the stage as a multiple of emit_kernel.

Runs are interleaved (one of every call per round) and the medians reported with the spread.

    python tools/polarization_cost.py [--rounds 9] [--sizes 1024] [--json out.json]
"""
import argparse
import ctypes as C
import importlib.util
import json
import math
import os
import sys

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
    metric = rt.KerrSchild(1.0, 0.998)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -80.0), rt.Plane(-300.0), rt.Disk(0.05, 2.0, 4.0)]
    opt = rt.solver_defaults()
    sc = rt.make_scene(metric, objs)
    em = rt.DiskEmission(3, 30000.0, inner_edge=True)
    pol = rt.Polarization("field", 0.7, field=(0.0, 1.0, 0.5))
    inc = math.radians(60.0)
    ob = rt.Observer((0, 50 * math.sin(inc), 0, 50 * math.cos(inc)), (0, -math.sin(inc), 0, -math.cos(inc)), (0, 0, 0, 1), 0.3, 0.3)
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "rows": []}
    abi.check(lib, lib.rtgr_timing_enable(None, 0, 1))

    def timed(fn):
        """(wall ms by HIP events, ms of the small kernels by the library's timers) of one call"""
        ms, launches = (C.c_double * 4)(), (C.c_uint64 * 4)()
        torch.cuda.synchronize()
        abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms), C.byref(launches)))     # (drop what came before)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms), C.byref(launches)))
        return e0.elapsed_time(e1), ms[0]

    for N in (int(v) for v in args.sizes.split(",")):
        n = N * N
        rgb = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        g, q, u, aux = (torch.zeros(n, dtype=torch.float64, device="cuda") for _ in range(4))
        se, s0 = (torch.zeros((n, 8), dtype=torch.float64, device="cuda") for _ in range(2))
        hit32 = torch.zeros(n, dtype=torch.int32, device="cuda")
        o = abi.rtgr_ray_outputs()
        o.hit32, o.state_end = hit32.data_ptr(), se.data_ptr()
        abi.check(lib, lib.rtgr_make_observer_canvas_device_f64(None, C.byref(sc), C.byref(ob), N, N, 0, N, s0.data_ptr(), stream()))

        def plain():
            abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, None, rgb.data_ptr(), C.byref(o), None,
                                                              None, stream()))

        def frame():
            abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, C.byref(em), rgb.data_ptr(), C.byref(o),
                                                              g.data_ptr(), None, stream()))

        def polarized():
            abi.check(lib, lib.rtgr_trace_polarized_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, C.byref(em), C.byref(pol),
                                                               rgb.data_ptr(), C.byref(o), g.data_ptr(), q.data_ptr(), u.data_ptr(), aux.data_ptr(), None,
                                                               stream()))

        def stage():
            abi.check(lib, lib.rtgr_polarization_device_f64(None, C.byref(sc), C.byref(em), C.byref(pol), C.byref(ob), N, N, hit32.data_ptr(), s0.data_ptr(),
                                                            se.data_ptr(), q.data_ptr(), u.data_ptr(), aux.data_ptr(), stream()))

        runs = {"plain": plain, "frame": frame, "polarized": polarized, "stage": stage}
        for r in ("plain", "polarized", "frame", "stage"):          # warm-up: workspace and scratch
            runs[r]()
        torch.cuda.synchronize()
        wall, small = {r: [] for r in runs}, {r: [] for r in runs}
        for _ in range(args.rounds):   # interleaved
            for r in runs:
                w, s = timed(runs[r])
                wall[r].append(w)
                small[r].append(s)
        row = dict(size=N, pixels=n, on_disk=int((hit32 == 3).sum()), finite_q=int(torch.isfinite(q).sum()))
        for r in runs:
            row[r] = dict(median_ms=float(np.median(wall[r])), min_ms=float(min(wall[r])), max_ms=float(max(wall[r])),
                          small_kernels_ms=float(np.median(small[r])))
        emit_ms = float(np.median(np.array(small["frame"]) - np.array(small["plain"])))
        pol_ms = float(np.median(np.array(small["polarized"]) - np.array(small["frame"])))
        row.update(emit_kernel_ms=emit_ms, polarize_kernel_ms=pol_ms, stage_over_emit=pol_ms / emit_ms,
                   polarized_over_frame=row["polarized"]["median_ms"] / row["frame"]["median_ms"])
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        print(f"{N}²: {row['on_disk']} pixels on the disk ({row['on_disk'] / n:.1%}); frame {row['frame']['median_ms']:.2f} ms, polarized "
              f"{row['polarized']['median_ms']:.2f} ms ({row['polarized_over_frame']:.4f} x); emit_kernel {emit_ms:.4f} ms, polarize_kernel {pol_ms:.4f} ms "
              f"= {row['stage_over_emit']:.2f} x emit_kernel; the stage alone {row['stage']['median_ms']:.3f} ms wall", flush=True)
        del rgb, g, q, u, aux, se, s0, hit32
        abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
