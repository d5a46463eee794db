#!/usr/bin/env python3
"""The bits of the two reductions of a traced frame — hot-spot light curves and disk spectra (§4.17) — as sha256 of every
output, so that two builds of the library can be held against each other on one machine: a refactor of the reduction changes no hash.

    python tools/reduce_bits.py [--tree PATH] [--json out.json]

--tree: the checkout whose package and library are loaded (default: this one; a `git worktree` of another revision, built there).  Only
the public Python and ctypes API is used, so any revision that has the two features can be asked.  Each run wants a fresh process.

Asked: rtgr_light_curve_device_* and rtgr_spectrum_device_* (LINE and THERMAL) over the synthetic planes of tests/test_light_curve.py
(ring_planes) and tests/test_spectrum.py (synthetic_planes), same generators and seeds — n in {1, 255, 256, 257, 773} at 65 items, n = 773
at {1, 257, 1068} items, n = 2^18 + 300 at 2 (light curve) or 3 (spectra) items; Float64 and Float32 planes; with and without an
observer's pixel weight —, one traced call of each feature on the 37 x 19 frame of the tests' orbiting observer, and the two hooks at 64
points."""
import argparse
import ctypes as C
import hashlib
import importlib.util
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_FRAME = 30000.0
SHAPES = [(n, 65) for n in (1, 255, 256, 257, 773)] + [(773, items) for items in (1, 257, 1068)]
BIG = 256 * 1024 + 300


def load_package(tree):
    name = "raytracegr_jl_amd"
    pkg = os.path.join(tree, "raytracegr.jl_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def ring_planes(n, rho_s, reach, seed, t_span=(-6.0, 0.0)):
    rng = np.random.default_rng(seed)
    rr, pp = rng.uniform(rho_s - reach, rho_s + reach, n), rng.uniform(-math.pi, math.pi, n)
    se = rng.uniform(-1.0, 1.0, (n, 8))
    se[:, 0], se[:, 1], se[:, 2] = rng.uniform(t_span[0], t_span[1], n), rr * np.cos(pp), rr * np.sin(pp)
    return np.ones(n, np.uint32), se, np.ones(n)


def synthetic_planes(n, dtype, seed):
    rng = np.random.default_rng(seed)
    hit = np.where(rng.uniform(size=n) < 0.95, 1, rng.integers(0, 3, n)).astype(np.uint32)
    g = np.where(rng.uniform(size=n) < 0.6, rng.uniform(0.35, 0.85, n), rng.uniform(0.95, 1.25, n))
    bad = rng.uniform(size=n)
    g = np.where(bad < 0.01, np.nan, np.where(bad < 0.02, 0.0, np.where(bad < 0.03, -g, np.where(bad < 0.035, np.inf, g))))
    rho, psi = rng.uniform(1.9, 6.4, n), rng.uniform(-math.pi, math.pi, n)
    se = rng.uniform(-1.0, 1.0, (n, 8))
    se[:, 1], se[:, 2] = rho * np.cos(psi), rho * np.sin(psi)
    pt = rng.uniform(size=n)
    se[:, 1] = np.where(pt < 0.01, np.nan, np.where(pt < 0.015, np.inf, se[:, 1]))
    se[:, 2] = np.where((pt > 0.015) & (pt < 0.025), -np.inf, se[:, 2])
    for k in range(min(3, n)):
        hit[k], g[k] = 1, 0.8125
        se[k, 1], se[k, 2] = 3.0 + 0.25 * k, 0.5
    return hit, se.astype(dtype), g.astype(dtype)


def canvas(rt, n, weighted):
    """(ni, nj, observer): two axes and a perspective weight where asked for and n factors, else one row with w = 1"""
    ni = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    if not weighted or ni == 1:
        return n, 1, None
    return n // ni, ni, rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 0.9, 0.7)


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    rt = load_package(os.path.abspath(args.tree))
    abi = rt._abi
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    out = {}

    def device_call(name, dtype, metric, objs, em, record, rows, ob, ni, nj, hit, se, g):
        sc = rt.make_scene(metric, objs)
        d_hit = torch.from_numpy(np.ascontiguousarray(hit, np.uint32).view(np.int32).copy()).cuda()
        d_se = torch.from_numpy(np.ascontiguousarray(se, dtype).copy()).cuda()
        d_g = torch.from_numpy(np.ascontiguousarray(g, dtype).copy()).cuda()
        d_out = torch.full((int(rows), 3), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        fn = getattr(lib, f"rtgr_{name}_device_" + ("f64" if dtype == np.float64 else "f32"))
        abi.check(lib, fn(None, C.byref(sc), C.byref(em), C.byref(record), C.byref(ob) if ob is not None else None, ni, nj, d_hit.data_ptr(), d_se.data_ptr(),
                          d_g.data_ptr(), d_out.data_ptr(), None))
        torch.cuda.synchronize()
        return sha(d_out.cpu().numpy())

    # ---- the stages over synthetic planes -------------------------------------------------------------------------------------------
    ring = dict(rho_s=3.0, sigma=0.5, cut=4.0, phi0=-1.1, amp=0.8, g_power=3.0)
    line = dict(lo=0.4, hi=1.2, amp=1.5, alpha=2.5, rho_min=2.2, rho_max=6.0, g_power=3.0)
    for dtype in (np.float64, np.float32):
        dn = np.dtype(dtype).name
        for weighted in (False, True):
            wn = "weighted" if weighted else "plain"
            for n, items in SHAPES + [(BIG, 2)]:
                ni, nj, ob = canvas(rt, n, weighted)
                hit, se, g = ring_planes(n, 3.0, 1.9, seed=n)
                em = rt.DiskEmission(1, T_FRAME, orbit=0.25, emitter="rigid")
                sp = rt.HotSpot(t_start=-2.0, dt=2 * math.pi / 0.25 / 61.0, nt=items, **ring)
                out[f"light_curve {dn} {wn} n={n} nt={items}"] = device_call("light_curve", dtype, rt.minkowski, [rt.Disk(0.05, 1.0, 6.0)], em, sp, items, ob,
                                                                             ni, nj, hit, se, g)
            for n, items in SHAPES + [(BIG, 3)]:
                ni, nj, ob = canvas(rt, n, weighted)
                hit, se, g = synthetic_planes(n, dtype, seed=n + items)
                em = rt.DiskEmission(1, T_FRAME, orbit=0.0, emitter="rigid", inner_edge=True, gain=0.75)
                for kind, sp in (("line", rt.Spectrum("line", nb=items, **line)),
                                 ("thermal", rt.Spectrum("thermal", 2.0e3, 6.0e4, items, log=items % 2 == 1, nu3=items % 4 == 1))):
                    out[f"spectrum {kind} {dn} {wn} n={n} nb={items}"] = device_call("spectrum", dtype, rt.minkowski, [rt.Disk(0.05, 2.0, 8.0)], em, sp, items, ob,
                                                                                     ni, nj, hit, se, g)

    # ---- one traced call of each feature on the real frame, and the hooks ---------------------------------------------------------------
    metric = rt.KerrSchild(1, 0.998)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -20.0), rt.Plane(-60.0), rt.Disk(0.05, 2.0, 4.0)]
    ob = rt.Observer((0, 0, -12, 0), (0, 0, 1, 0), (0, 0, 0, 1), 0.8, 0.25, kind="circular", orbit=+1, projection="perspective")
    em = rt.DiskEmission(3, T_FRAME)
    spot = rt.HotSpot(nt=65, rho_s=3.0, sigma=0.5, cut=4.0, phi0=0.7, amp=1.5, g_power=4.0, t_start=-5.0, dt=0.6)
    for dtype in (np.float64, np.float32):
        dn = np.dtype(dtype).name
        res = rt.light_curve(metric, objs, ob, 37, 19, em, spot, dtype=dtype, details=True)
        out[f"traced light_curve {dn}"] = sha(res["lc"], res["rgb"], res["g"], res["state_end"], res["hit"])
        for kind, sp in (("line", rt.Spectrum("line", 0.0, 1.6, 64, rho_min=2.0, rho_max=4.0, alpha=3.0)),
                         ("thermal", rt.Spectrum("thermal", 2.0e3, 2.0e5, 33, log=True, nu3=True))):
            res = rt.spectrum(metric, objs, ob, 37, 19, em, sp, dtype=dtype, details=True)
            out[f"traced spectrum {kind} {dn}"] = sha(res["F"], res["A"], res["B"], res["axis"], res["rgb"], res["g"], res["state_end"], res["hit"])
        rng = np.random.default_rng(11)
        pts = np.column_stack([rng.uniform(-4, 4, 64), rng.uniform(-4, 4, 64), rng.uniform(-40, 10, 64)]).astype(dtype)
        h = rt.eval_hot_spot(metric, objs, em, spot, pts, dtype=dtype)
        out[f"eval_hot_spot {dn}"] = sha(np.array([h["omega_s"]]), h["j"])
        pts[:, 2] = rng.uniform(0.3, 1.3, 64)
        for kind, sp in (("line", rt.Spectrum("line", 0.0, 1.6, 64, rho_min=2.0, rho_max=4.0, alpha=3.0)),
                         ("thermal", rt.Spectrum("thermal", 2.0e3, 2.0e5, 33, log=True, nu3=True))):
            h = rt.eval_spectrum(metric, objs, em, sp, pts, dtype=dtype)
            out[f"eval_spectrum {kind} {dn}"] = sha(h["axis"], h["bin"], h["val"])

    for k, v in out.items():
        print(f"{v}  {k}")
    print(f"{sha(np.frombuffer(''.join(out.values()).encode(), np.uint8))}  all {len(out)} outputs")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
