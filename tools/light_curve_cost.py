#!/usr/bin/env python3
"""What a hot-spot light curve costs (rtgr_light_curve_device_f64): KerrSchild(1, 0.998) with BASELINE config 5's disk,
seen by a static observer at rho = 50, 60 degrees from the axis, through a perspective window that the disk fills about a tenth of;
a spot at rho_s = 3 (sigma = 0.5, cut = 4: its ring covers the whole disk), two orbital periods; Float64; per size, ms of
    frame         rtgr_trace_observer_device_f64 with the disk emitting and every plane the reduction reads — ONE frame.  The trace is
                  untouched by this feature: this is the path of the commit before it, whose only way to a light curve of nt samples is nt
                  such frames (had its emitter a clock)
    lc nt         rtgr_light_curve_device_f64 over that frame's planes, for each nt: the seed kernel, the emission kernel on one point, the
                  reduction and the sum
with the pairs (active pixels x nt) per second, the share of the pixels culled, and frame x nt / lc.

Runs are interleaved (one of every call per round) and the medians reported with the spread.

    python tools/light_curve_cost.py [--rounds 9] [--sizes 1024] [--nts 64,1024,4096] [--json out.json]
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
    ap.add_argument("--nts", default="64,1024,4096")
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
    rho_s, sigma, cut = 3.0, 0.5, 4.0
    omega = float(rt.eval_hot_spot(metric, objs, em, rt.HotSpot(rho_s, sigma))["omega_s"])
    period = 2 * math.pi / omega
    nts = [int(v) for v in args.nts.split(",")]
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "omega_s": omega, "rows": []}

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
        lcs = {nt: torch.zeros((nt, 3), dtype=torch.float64, device="cuda") for nt in nts}
        spots = {nt: rt.HotSpot(rho_s, sigma, t_start=0.0, dt=2 * period / nt, nt=nt, cut=cut) for nt in nts}
        o = abi.rtgr_ray_outputs()
        o.hit32, o.state_end = hit32.data_ptr(), se.data_ptr()

        def frame():
            abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, C.byref(em), rgb.data_ptr(), C.byref(o),
                                                              g.data_ptr(), None, stream()))

        def reduction(nt):
            return lambda: abi.check(lib, lib.rtgr_light_curve_device_f64(None, C.byref(sc), C.byref(em), C.byref(spots[nt]), C.byref(ob), N, N, hit32.data_ptr(),
                                                                          se.data_ptr(), g.data_ptr(), lcs[nt].data_ptr(), stream()))

        runs = {"frame": frame}
        runs.update({f"lc{nt}": reduction(nt) for nt in nts})
        for r in runs:          # warm-up: workspace and scratch
            runs[r]()
        torch.cuda.synchronize()
        rho = torch.hypot(se[:, 1], se[:, 2])
        active = int(((hit32 == 3) & torch.isfinite(g) & (g > 0) & torch.isfinite(se[:, 0]) & ((rho - rho_s).abs() < cut * sigma)).sum())
        on_disk = int((hit32 == 3).sum())
        times = {r: [] for r in runs}
        for _ in range(args.rounds):   # interleaved
            for r in runs:
                times[r].append(timed(runs[r]))
        med = {r: float(np.median(times[r])) for r in runs}
        row = dict(size=N, pixels=n, on_disk=on_disk, active=active, culled_share=1.0 - active / n,
                   frame=dict(median_ms=med["frame"], min_ms=float(min(times["frame"])), max_ms=float(max(times["frame"]))))
        for nt in nts:
            t = times[f"lc{nt}"]
            F = lcs[nt][:, 0]
            row[f"lc{nt}"] = dict(median_ms=med[f"lc{nt}"], min_ms=float(min(t)), max_ms=float(max(t)), pairs=active * nt,
                                  pairs_per_s=active * nt / (med[f"lc{nt}"] * 1e-3), frames_instead_ms=med["frame"] * nt,
                                  speedup=med["frame"] * nt / med[f"lc{nt}"], lit_share=float((F > 0).float().mean()), F_max_over_min=float(F.max() / F.min()))
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        print(f"{N}²: {on_disk / n:.1%} of the pixels on the disk, {active} active ({row['culled_share']:.1%} culled); one emitted frame {med['frame']:.2f} ms", flush=True)
        for nt in nts:
            c = row[f"lc{nt}"]
            print(f"   nt = {nt}: {c['median_ms']:.3f} ms (min {c['min_ms']:.3f}, max {c['max_ms']:.3f}), {c['pairs_per_s']:.3e} pairs/s; {nt} frames would "
                  f"take {c['frames_instead_ms']:.0f} ms: x {c['speedup']:.0f}", flush=True)
        del rgb, g, se, hit32, lcs
        abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
