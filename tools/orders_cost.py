#!/usr/bin/env python3
"""What the higher orders of a disk image cost (rtgr_trace_orders_device_f64): the Kerr scene of tests/test_orders.py —
KerrSchild(1, 0.9), sky R = -30, Disk(0.05, 3, 12), a static observer at (0, 0, -18, 9) looking at the origin —; Float64; per size, ms of
    frame    rtgr_trace_observer_device_f64 with the disk emitting and the planes leg 0 keeps: the emitted observer frame.  The trace
             is untouched by this feature: this is the path of the commit before it
    orders   rtgr_trace_orders_device_f64, N orders, every plane asked for
and the rays of each leg, from the planes: leg 0 the frame, then per order the crossing leg and the continuation leg.  The call holds
two synchronisations per order, so its wall time is taken by the host clock around the call and a device synchronisation.

Runs are interleaved (one of every call per round) and the medians reported with the spread.

    python tools/orders_cost.py [--rounds 9] [--sizes 1024] [--orders 2] [--json out.json]
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
    ap.add_argument("--orders", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    rt = load_package()
    abi = rt._abi
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    metric = rt.KerrSchild(1.0, 0.9)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -30.0), rt.Disk(0.05, 3.0, 12.0)]
    opt = rt.solver_defaults(max_steps=4000, lambda1=200.0)
    sc = rt.make_scene(metric, objs)
    em = rt.DiskEmission(2, 30000.0)
    orders = rt.DiskOrders(args.orders, 0.5)
    ob = rt.Observer((0, 0, -18, 9), (0, 0, 18, -9), (0, 0, 0, 1), 1.4, 1.05)
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "orders": args.orders, "rows": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for N in (int(v) for v in args.sizes.split(",")):
        n, nb = N * N, args.orders + 1
        f64 = dict(dtype=torch.float64, device="cuda")
        rgb, g, se, s0 = torch.zeros((3, n), **f64), torch.zeros((nb, n), **f64), torch.zeros((nb, n, 8), **f64), torch.zeros((n, 8), **f64)
        rgbo = torch.zeros((nb, 3, n), **f64)
        hit32 = torch.zeros((nb, n), dtype=torch.int32, device="cuda")
        count = torch.zeros(n, dtype=torch.uint8, device="cuda")
        o = abi.rtgr_ray_outputs()
        o.hit32, o.state_end = hit32.data_ptr(), se.data_ptr()
        planes = abi.rtgr_order_planes(count=count.data_ptr(), hit32=hit32.data_ptr(), state_end=se.data_ptr(), g=g.data_ptr(),
                                       rgb_order=rgbo.data_ptr(), state0=s0.data_ptr())

        def frame():
            abi.check(lib, lib.rtgr_trace_observer_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), N, N, None, C.byref(em), rgb.data_ptr(), C.byref(o),
                                                              g.data_ptr(), None, stream()))

        def traced_orders():
            abi.check(lib, lib.rtgr_trace_orders_device_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), None, N, N, None, C.byref(em), C.byref(orders),
                                                            rgb.data_ptr(), C.byref(planes), None, stream()))

        runs = {"frame": frame, "orders": traced_orders}
        for r in runs:          # warm-up: workspace and scratch
            runs[r]()
        torch.cuda.synchronize()
        wall = {r: [] for r in runs}
        for _ in range(args.rounds):   # interleaved; `orders` last, so the planes hold its results
            for r in runs:
                wall[r].append(timed(runs[r]))
        per_order = [int((hit32[k] == 2).sum()) for k in range(nb)]
        legs = [n] + [m for k in range(1, nb) for m in (per_order[k - 1], per_order[k - 1])]   # (every crossing leg of this scene goes on)
        row = dict(size=N, pixels=n, pixels_per_order=per_order, rays_per_leg=legs)
        for r in runs:
            row[r] = dict(median_ms=float(np.median(wall[r])), min_ms=float(min(wall[r])), max_ms=float(max(wall[r])))
        row["orders_over_frame"] = row["orders"]["median_ms"] / row["frame"]["median_ms"]
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
        print(f"{N}²: pixels per order {per_order}, rays per leg {legs}; frame {row['frame']['median_ms']:.2f} ms, {args.orders} orders "
              f"{row['orders']['median_ms']:.2f} ms = {row['orders_over_frame']:.3f} x", flush=True)
        del rgb, g, se, s0, rgbo, hit32, count
        abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
