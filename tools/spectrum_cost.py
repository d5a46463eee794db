#!/usr/bin/env python3
"""What a disk spectrum costs (rtgr_spectrum_device_f64): the light-curve cost table's scene — KerrSchild(1, 0.998) with
BASELINE config 5's disk, seen by a static observer at rho = 50, 60 degrees from the axis, through a perspective window that the disk
fills about a tenth of —; Float64; per size, ms of
    frame           rtgr_trace_observer_device_f64 with the disk emitting and every plane the stage reads — ONE frame.  The trace is
                    untouched by this feature: this is the path of the commit before it
    line nb         rtgr_spectrum_device_f64, RTGR_SPEC_LINE over the whole disk, nb bins over g in [0, 1.6)
    cull nb         the same call with the bins moved to g in [10, 11.6), where no pixel falls: every tile culls every pixel and walks
                    nothing — what of `line nb` is the cull, which is repeated per tile of 256 bins
    thermal nb      rtgr_spectrum_device_f64, RTGR_SPEC_THERMAL at nb frequencies
with bins x pixels per second (LINE: what the cull sweeps), records per second of the walk, pairs (counted pixels x nb) per second
(THERMAL).

Runs are interleaved (one of every call per round) and the medians reported with the spread.

    python tools/spectrum_cost.py [--rounds 9] [--sizes 1024] [--line 64,1024,16384] [--thermal 64,1024] [--json out.json]
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
    ap.add_argument("--line", default="64,1024,16384")
    ap.add_argument("--thermal", default="64,1024")
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
    inc = math.radians(60.0)
    ob = rt.Observer((0, 50 * math.sin(inc), 0, 50 * math.cos(inc)), (0, -math.sin(inc), 0, -math.cos(inc)), (0, 0, 0, 1), 0.3, 0.3)
    line_nbs = [int(v) for v in args.line.split(",")]
    thermal_nbs = [int(v) for v in args.thermal.split(",")]
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "rows": []}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for N in (int(v) for v in args.sizes.split(",")):
        n = N * N
        rgb = torch.zeros((3, n), dtype=torch.float64, device="cuda")
        g = torch.zeros(n, dtype=torch.float64, device="cuda")
        se = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
        hit32 = torch.zeros(n, dtype=torch.int32, device="cuda")
        specs = {f"line{nb}": rt.Spectrum("line", 0.0, 1.6, nb, alpha=3.0, rho_min=2.0, rho_max=4.0) for nb in line_nbs}
        specs.update({f"cull{nb}": rt.Spectrum("line", 10.0, 11.6, nb, alpha=3.0, rho_min=2.0, rho_max=4.0) for nb in line_nbs})
        specs.update({f"thermal{nb}": rt.Spectrum("thermal", 2.0e3, 2.0e5, nb, log=True, nu3=True) for nb in thermal_nbs})
        outs = {k: torch.zeros((int(s.nb), 3), dtype=torch.float64, device="cuda") for k, s in specs.items()}
        o = abi.rtgr_ray_outputs()
        o.hit32, o.state_end = hit32.data_ptr(), se.data_ptr()

        def frame():
            abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, C.byref(em), rgb.data_ptr(), C.byref(o),
                                                              g.data_ptr(), None, stream()))

        def stage(key):
            return lambda: abi.check(lib, lib.rtgr_spectrum_device_f64(None, C.byref(sc), C.byref(em), C.byref(specs[key]), C.byref(ob), N, N, hit32.data_ptr(),
                                                                       se.data_ptr(), g.data_ptr(), outs[key].data_ptr(), stream()))

        runs = {"frame": frame}
        runs.update({key: stage(key) for key in specs})
        for r in runs:          # warm-up: workspace and scratch
            runs[r]()
        torch.cuda.synchronize()
        rho = torch.hypot(se[:, 1], se[:, 2])
        base = (hit32 == 3) & torch.isfinite(g) & (g > 0) & torch.isfinite(se[:, 1]) & torch.isfinite(se[:, 2])
        counted_line = int((base & (g < 1.6) & (rho >= 2.0) & (rho < 4.0)).sum())
        counted_thermal = int((base & (rho > 2.0)).sum())      # (the inner-edge law: T > 0 iff rho > r_in)
        times = {r: [] for r in runs}
        for _ in range(args.rounds):   # interleaved
            for r in runs:
                times[r].append(timed(runs[r]))
        med = {r: float(np.median(times[r])) for r in runs}
        row = dict(size=N, pixels=n, on_disk=int((hit32 == 3).sum()), counted_line=counted_line, counted_thermal=counted_thermal)
        for r in runs:
            row[r] = dict(median_ms=med[r], min_ms=float(min(times[r])), max_ms=float(max(times[r])))
        for nb in line_nbs:
            row[f"line{nb}"].update(bins_pixels_per_s=nb * n / (med[f"line{nb}"] * 1e-3), cull_ms=med[f"cull{nb}"],
                                    walk_ms=med[f"line{nb}"] - med[f"cull{nb}"], conserved=float(outs[f"line{nb}"][:, 0].sum()))
        for nb in thermal_nbs:
            row[f"thermal{nb}"].update(pairs=counted_thermal * nb, pairs_per_s=counted_thermal * nb / (med[f"thermal{nb}"] * 1e-3))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        print(f"{N}²: {row['on_disk'] / n:.1%} of the pixels on the disk, {counted_line} counted by LINE, {counted_thermal} by THERMAL; one emitted frame "
              f"{med['frame']:.2f} ms", flush=True)
        for nb in line_nbs:
            c = row[f"line{nb}"]
            print(f"   line nb = {nb}: {c['median_ms']:.3f} ms (min {c['min_ms']:.3f}, max {c['max_ms']:.3f}), {c['bins_pixels_per_s']:.3e} bins x pixels/s; "
                  f"cull alone {c['cull_ms']:.3f} ms, walk and the rest {c['walk_ms']:.3f} ms", flush=True)
        for nb in thermal_nbs:
            c = row[f"thermal{nb}"]
            print(f"   thermal nb = {nb}: {c['median_ms']:.3f} ms (min {c['min_ms']:.3f}, max {c['max_ms']:.3f}), {c['pairs_per_s']:.3e} pairs/s", flush=True)
        del rgb, g, se, hit32, outs
        abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
