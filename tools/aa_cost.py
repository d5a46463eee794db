#!/usr/bin/env python3
"""What adaptive anti-aliasing costs (rtgr_trace_aa_device_f64): per scene and size, ms per frame of
    plain      one ray through each pixel centre (rtgr_trace_device_f64)
    adaptive   k = 4, contrast = 1/255: the plain frame + 16 sub-rays for the pixels on an edge
    uniform    the plain frame at k ni x k nj (what a caller had to render and average before) — for sizes up to --uniform-max
the refined fraction f, adaptive / plain beside the prediction 1 + f k², the library's own kernel timers for one adaptive frame
(rtgr_timing_read: set-up incl. the three anti-aliasing kernels, FAR / FULL pass, resolve, NEAR pass), and the mean absolute 8-bit error
of the plain and of the adaptive frame against a k = 8 uniform frame (sizes up to --error-max).

Scenes: example2's, and KerrSchild(1, 0.8) with example2's objects.  Runs are interleaved (one frame of every rendering per round) and
the medians reported with the spread.

    python tools/aa_cost.py [--rounds 7] [--sizes 1024,4096] [--uniform-max 1024] [--error-max 1024] [--json out.json]
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default="1024,4096")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--uniform-max", type=int, default=1024)
    ap.add_argument("--error-max", type=int, default=1024)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    rt = load_package()
    abi = rt._abi
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    _, objs, cam = rt.example2_scene()
    cam = rt.make_camera(**cam)
    opt = rt.solver_defaults()
    scenes = {"example2": rt.make_scene(rt.kerr_schild, objs), "ks_true08": rt.make_scene(rt.KerrSchild(1.0, 0.8), objs)}
    k = args.k
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    result = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "k": k, "contrast": 1.0 / 255.0, "rows": []}

    def plain(sc, N, rgb):
        abi.check(lib, lib.rtgr_trace_device_f64(None, C.byref(sc), C.byref(opt), None, C.byref(cam), N, N, 0, N, rgb.data_ptr(), None, None, stream()))

    def aa(sc, N, rgb, kk, contrast):
        a = abi.rtgr_aa(k=kk, flags=0, contrast=contrast, max_batch_rays=0)
        stats = abi.rtgr_aa_stats()
        abi.check(lib, lib.rtgr_trace_aa_device_f64(None, C.byref(sc), C.byref(opt), C.byref(cam), N, N, C.byref(a), rgb.data_ptr(), None, None, None,
                                                    C.byref(stats), stream()))
        return stats.as_dict()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, out

    def u8(t):
        return torch.round(torch.clamp(t, 0.0, 1.0) * 255.0)

    for name, sc in scenes.items():
        for N in (int(v) for v in args.sizes.split(",")):
            rgb = torch.zeros((3, N * N), dtype=torch.float64, device="cuda")
            fine = torch.zeros((3, k * N * k * N), dtype=torch.float64, device="cuda") if N <= args.uniform_max else None
            runs = {"plain": lambda: plain(sc, N, rgb), "adaptive": lambda: aa(sc, N, rgb, k, 1.0 / 255.0)}
            if fine is not None:
                runs["uniform"] = lambda: plain(sc, k * N, fine)
            times, wall, stats = {r: [] for r in runs}, {r: [] for r in runs}, None
            for r in runs:          # warm-up: workspace and scratch
                runs[r]()
            torch.cuda.synchronize()
            for _ in range(args.rounds):   # interleaved
                for r in runs:
                    ms, w, out = timed(runs[r])
                    times[r].append(ms)
                    wall[r].append(w)
                    if r == "adaptive":
                        stats = out
            # one more adaptive frame under the library's kernel timers
            abi.check(lib, lib.rtgr_timing_enable(None, 0, 1))
            ms4, n4 = (C.c_double * 4)(), (C.c_uint64 * 4)()
            abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms4), C.byref(n4)))
            parts = {}
            for r in ("plain", "adaptive"):
                runs[r]()
                torch.cuda.synchronize()
                abi.check(lib, lib.rtgr_timing_read(None, 0, C.byref(ms4), C.byref(n4)))
                parts[r] = dict(setup_ms=ms4[0], main_ms=ms4[1], resolve_ms=ms4[2], near_ms=ms4[3], launches=[int(v) for v in n4])
            abi.check(lib, lib.rtgr_timing_enable(None, 0, 0))
            f = stats["refined"] / stats["pixels"]
            med = {r: float(np.median(times[r])) for r in runs}
            row = dict(scene=name, size=N, refined_fraction=f, stats=stats, predicted_ratio=1.0 + f * k * k, ratio=med["adaptive"] / med["plain"],
                       kernel_timers=parts)
            for r in runs:
                t = np.array(times[r])
                row[r] = dict(median_ms=med[r], min_ms=float(t.min()), max_ms=float(t.max()), wall_median_ms=float(np.median(wall[r])))
            if N <= args.error_max:   # against a k = 8 uniform frame (the adaptive entry with contrast < 0: every pixel refined)
                truth = torch.zeros_like(rgb)
                aa(sc, N, truth, 8, -1.0)
                plain(sc, N, rgb)
                torch.cuda.synchronize()
                row["err8_plain"] = float((u8(rgb) - u8(truth)).abs().mean())
                aa(sc, N, rgb, k, 1.0 / 255.0)
                torch.cuda.synchronize()
                row["err8_adaptive"] = float((u8(rgb) - u8(truth)).abs().mean())
                if fine is not None:
                    aa(sc, N, rgb, k, -1.0)
                    torch.cuda.synchronize()
                    row["err8_uniform"] = float((u8(rgb) - u8(truth)).abs().mean())
                del truth
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
            print(f"{name} {N}²: f = {f:.4f}; plain {med['plain']:.2f} ms, adaptive {med['adaptive']:.2f} ms"
                  + (f", uniform {med['uniform']:.2f} ms" if "uniform" in med else "")
                  + f"; adaptive / plain = {row['ratio']:.2f} (1 + f k² = {row['predicted_ratio']:.2f})", flush=True)
            del rgb, fine
            abi.check(lib, lib.rtgr_trim(None))
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
