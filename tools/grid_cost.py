#!/usr/bin/env python3
"""What a metric sampled on a grid costs (RTGR_GRID): ms per frame of example2's scene with KerrSchild(1, 0.8) sampled
on a grid, against the closed form traced through the generic contraction (KerrSchild(1, 0.8, generic=True)), at 1024² and 2048².

Two spacings: one grid whose Float64 samples fit the 256 MiB Infinity Cache (h = 0.15: 140³ points, 209 MiB) and one that does not
(h = 0.075: 278³ points, 1.6 GiB).  The grids are sampled with numpy from the textbook formula.  Runs are interleaved (one frame of every
configuration per round) and the medians reported, with the spread; the frames are checked against the closed form's hit map.

    python tools/grid_cost.py [--rounds 7] [--sizes 1024,2048] [--json out.json]
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


UPPER = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
ETA = np.array([-1.0, 0, 0, 0, 1, 0, 0, 1, 0, 1])


def kerr_schild_samples(h, L, M=1.0, a=0.8):
    """(n, n, n, 10) samples of textbook Kerr-Schild on a grid whose valid box is [-L, L]^3; rho < 1 (around the ring singularity,
    which example2's rays never approach) holds eta.  Sampled slab by slab (z) to bound the temporaries."""
    n = int(round(2 * L / h)) + 3
    origin = -L - h
    c = origin + h * np.arange(n)
    y, x = np.meshgrid(c, c, indexing="ij")
    out = np.empty((n, n, n, 10))
    for k in range(n):
        z = np.full_like(x, c[k])
        rho2 = x * x + y * y + z * z
        q = rho2 - a * a
        with np.errstate(all="ignore"):
            r = np.sqrt(0.5 * (q + np.sqrt(q * q + 4 * a * a * z * z)))
            f = 2 * M * r ** 3 / (r ** 4 + a * a * z * z)
            kv = [np.ones_like(x), (r * x + a * y) / (r * r + a * a), (r * y - a * x) / (r * r + a * a), z / r]
            for ci, (p, qq) in enumerate(UPPER):
                out[k, :, :, ci] = ETA[ci] + f * kv[p] * kv[qq]
        out[k][rho2 < 1.0] = ETA
    return out, (origin,) * 3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--spacings", default="0.15,0.075")
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
    L = 10.3   # the sky is a sphere of radius 10 around the origin
    configs = {"closed_generic": rt.make_scene(rt.KerrSchild(1.0, 0.8, generic=True), objs)}
    grids = {}
    for h in (float(v) for v in args.spacings.split(",")):
        t0 = time.time()
        g, origin, n = kerr_schild_samples(h, L)
        grids[h] = rt.GridMetric(g, origin, h, name=f"h={h}")
        del g
        configs[f"grid_h{h}"] = rt.make_scene(grids[h], objs)
        print(f"grid h={h}: {n}^3 samples, {n ** 3 * 80 / 2 ** 20:.0f} MiB Float64, sampled + uploaded in {time.time() - t0:.1f} s", flush=True)
    sizes = [int(v) for v in args.sizes.split(",")]
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "scene": "example2 objects, KerrSchild(1, 0.8)", "rows": []}
    for N in sizes:
        rgb = {k: torch.zeros((3, N * N), dtype=torch.float64, device="cuda") for k in configs}
        hit = {k: torch.zeros(N * N, dtype=torch.uint8, device="cuda") for k in configs}
        times = {k: [] for k in configs}

        def run(k, record):
            o = abi.rtgr_ray_outputs()
            o.hit = hit[k].data_ptr()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(configs[k]), C.byref(opt), None, C.byref(cam), N, N, 0, N,
                                                     rgb[k].data_ptr(), C.byref(o), None, torch.cuda.current_stream().cuda_stream))
            e1.record()
            e1.synchronize()
            if record:
                times[k].append(e0.elapsed_time(e1))

        for k in configs:   # warm-up: workspace, first-touch of the grid
            run(k, False)
        for _ in range(args.rounds):   # interleaved
            for k in configs:
                run(k, True)
        ref = hit["closed_generic"].cpu().numpy()
        for k in configs:
            t = np.array(times[k])
            agree = float(np.mean(hit[k].cpu().numpy() == ref))
            row = dict(size=N, config=k, median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), hit_agree=agree)
            result["rows"].append(row)
            print(f"{N}² {k:16s} median {row['median_ms']:8.2f} ms  [{row['min_ms']:.2f} .. {row['max_ms']:.2f}]  hit map vs closed form {agree:.4f}",
                  flush=True)
        base = np.median(times["closed_generic"])
        for k in configs:
            if k != "closed_generic":
                print(f"{N}² {k}: {np.median(times[k]) / base:.2f} x the closed form (generic contraction)", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
