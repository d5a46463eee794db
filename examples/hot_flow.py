#!/usr/bin/env python3
"""A hot, geometrically thick flow round the a = 0.9 hole, optically thin and grey side by side (rt.trace_transfer; include/rtgr.h
"volume emission").

    python examples/hot_flow.py [ni nj]

KerrSchild(1, 0.9) inside a dark sky at r = 60, seen by a static observer at r = 40, inclination 60 degrees.  The gas rotates on
cylinders at the circular-orbit rate, density (r / 4)^(-1.5) exp(-z² / (2 0.4² rho²)); the transfer equations are integrated along every
ray behind the trace.  The ring is emission gathered by rays that wind round the photon orbit.  r_stop = 1.75 lies between the horizon's
coordinate radius (at most 1.70) and the dark cylinder (rho < 1.80).  With kappa > 0 a ray that crosses the photon orbit's cylinder
inside the gas meets an unbounded dtau/dlambda and ends not finite (status 3): those pixels are drawn black.  Prints the status counts
and the step attempts of both frames; writes scenes/hot_flow_thin.png and scenes/hot_flow_grey.png.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def main():
    ni = int(sys.argv[1]) if len(sys.argv) > 1 else 320
    nj = int(sys.argv[2]) if len(sys.argv) > 2 else 3 * ni // 4
    metric = rt.KerrSchild(1.0, 0.9)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -60.0)]
    inc = np.radians(60.0)
    pos = (0.0, 40 * np.sin(inc), 0.0, 40 * np.cos(inc))
    obs = rt.Observer(pos, (0, -pos[1], -pos[2], -pos[3]), (0, 0, 0, 1), 0.6, 0.45)
    opt = rt.solver_defaults(max_steps=4000, lambda1=400.0)
    flow = dict(j0=0.027, r0=4.0, alpha=1.5, H=0.4, s=0.5, r_stop=1.75, weight=(1.0, 0.6, 0.3))
    import importlib
    write_png = importlib.import_module(rt.__name__ + ".png").write_png
    os.makedirs("scenes", exist_ok=True)
    frames = {"thin": rt.trace_transfer(metric, objs, obs, ni, nj, rt.Flow(kappa=0.0, **flow), opt=opt),
              "grey": rt.trace_transfer(metric, objs, obs, ni, nj, rt.Flow(kappa=0.028, **flow), opt=opt)}
    scale = max(float(np.nanmax(frames["thin"]["I"])), 1e-30)
    for name, f in frames.items():
        c = f["transfer_counters"]
        print(f"{name}: status counts (end, r_stop, step cap, not finite) {np.bincount(f['tstatus'], minlength=4).tolist()}, "
              f"{c['accepted'] + c['rejected']} step attempts, max I {np.nanmax(f['I']):.3f}, max tau {np.nanmax(f['tau']):.3f}")
        img = np.clip(np.nan_to_num(f["rgb"]) / scale, 0, 1).reshape(3, nj, ni)
        write_png(os.path.join("scenes", f"hot_flow_{name}.png"), np.ascontiguousarray((255 * np.moveaxis(img, 0, -1)[::-1]).astype(np.uint8)))
        print(f"wrote scenes/hot_flow_{name}.png")


if __name__ == "__main__":
    main()
