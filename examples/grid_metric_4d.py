#!/usr/bin/env python3
"""An evolving spacetime that exists only as numbers: a time-dependent metric sampled on a 4-D grid (rtgr_grid4_metric_load).

This example samples a spacetime we DO know, examples/user_metrics.py:EXPANDING_ISOTROPIC (a mass in a universe expanding at H = 0.03),
through api.sample_metric with a time axis, and traces a compact scene through the grid and through the user metric itself:

    python examples/grid_metric_4d.py [ni]     # prints the hit-map agreement and the max RGB difference; default 96

A caller with simulation data builds the same GridMetric from its own (nt, nz, ny, nx, 10) array (time slowest, each slice in the 3-D
layout), origin (t0, x0, y0, z0) and spacing (ht, h, h, h).  Rays that leave the valid box — in t too — end with status RAY_OUTSIDE.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from __graft_entry__ import load_package

import user_metrics

rt = load_package()
ETA = np.array([-1.0, 0, 0, 0, 1, 0, 0, 1, 0, 1])


def main():
    ni = int(sys.argv[1]) if len(sys.argv) > 1 else 96
    user = rt.UserMetric(user_metrics.EXPANDING_ISOTROPIC, M=1.0, a=0.03)
    h, ht, L, T0, T1 = 0.2, 2.0, 6.6, -32.0, 4.0            # valid box [-L, L]^3 x [T0, T1]
    n, nt = int(round(2 * L / h)) + 3, int(round((T1 - T0) / ht)) + 3
    origin = (-L - h,) * 3
    g = rt.sample_metric(user, origin, h, (n,) * 3, t=(T0 - ht, ht, nt))
    x = origin[0] + h * np.arange(n)
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    g[:, (xx * xx + y * y + z * z) < 1.0] = ETA              # the singular interior: inside the opaque sphere below, out of every ray's reach
    grid = rt.GridMetric(g, (T0 - ht,) + origin, (ht, h, h, h), name="expanding")
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(-20.0), rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), 2.2),
            rt.Sphere((0, 2.0, -3.0, 1.5), (1, 0, 0, 0), 0.6)]
    cam = dict(pos=(0, 0, -4.5, 0), widthx=(0, 5.0, 0, 0), widthy=(0, 0, 0, 5.0), normal=(0, 0, 1, 0))
    a = rt.trace_frames(grid, objs, [rt.make_camera(**cam)], ni, ni)[0]
    b = rt.trace_frames(user, objs, [rt.make_camera(**cam)], ni, ni)[0]
    print(f"{grid}: hit map agrees on {np.mean(a['hit'] == b['hit']):.4f} of {ni}x{ni} pixels, "
          f"max RGB difference {np.abs(a['rgb'] - b['rgb']).max():.2e}")


if __name__ == "__main__":
    main()
