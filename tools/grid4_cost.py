#!/usr/bin/env python3
"""What a TIME-DEPENDENT grid costs (rtgr_grid4_metric_load): ms per frame of example2's scene with KerrSchild(1, 0.8)
traced three ways at the same spatial spacing h = 0.15 — the closed form through the generic contraction, the 3-D grid (RTGR_GRID) and a
4-D grid of n_t time slices (the same field in every slice: the cost does not depend on the values, and the frames must then agree with
the 3-D grid's bit for bit) — at 1024² and 2048².  Runs are interleaved (one frame of every configuration per round) and the medians
reported, with the spread, as tools/grid_cost.py does.

    python tools/grid4_cost.py [--rounds 7] [--sizes 1024,2048] [--nt 10] [--json out.json]
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
    ap.add_argument("--h", type=float, default=0.15)
    ap.add_argument("--nt", type=int, default=10, help="time slices of the 4-D grid (valid t range [-200, 10])")
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
    h = args.h
    t0 = time.time()
    g, origin, n = kerr_schild_samples(h, L)
    g3 = rt.GridMetric(g, origin, h, name=f"3-D h={h}")
    ht = 210.0 / (args.nt - 3)    # valid t in [-200, 10]: example2's rays run backwards from t = 0 and end long before t = -200
    g4 = rt.GridMetric(np.broadcast_to(g, (args.nt,) + g.shape), (-200.0 - ht,) + origin, (ht, h, h, h), name=f"4-D h={h} nt={args.nt}")
    del g
    configs = {"closed_generic": rt.make_scene(rt.KerrSchild(1.0, 0.8, generic=True), objs), "grid3": rt.make_scene(g3, objs),
               "grid4": rt.make_scene(g4, objs)}
    print(f"h={h}: {n}^3 samples ({n ** 3 * 80 / 2 ** 20:.0f} MiB Float64), 4-D x {args.nt} slices "
          f"({args.nt * n ** 3 * 80 / 2 ** 20:.0f} MiB); sampled + uploaded in {time.time() - t0:.1f} s", flush=True)
    sizes = [int(v) for v in args.sizes.split(",")]
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "h": h, "nt": args.nt,
              "scene": "example2 objects, KerrSchild(1, 0.8)", "rows": []}
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
        same = bool(torch.equal(rgb["grid3"], rgb["grid4"]))
        for k in configs:
            t = np.array(times[k])
            agree = float(np.mean(hit[k].cpu().numpy() == ref))
            row = dict(size=N, config=k, median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), hit_agree=agree)
            result["rows"].append(row)
            print(f"{N}² {k:16s} median {row['median_ms']:8.2f} ms  [{row['min_ms']:.2f} .. {row['max_ms']:.2f}]  hit map vs closed form {agree:.4f}",
                  flush=True)
        b3, b4 = np.median(times["grid3"]), np.median(times["grid4"])
        result["rows"].append(dict(size=N, grid4_over_grid3=float(b4 / b3), grid4_frame_equals_grid3=same))
        print(f"{N}² grid4 / grid3 = {b4 / b3:.2f}, grid3 / closed = {b3 / np.median(times['closed_generic']):.1f}; "
              f"4-D frame bit-equal to the 3-D frame: {same}", flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
