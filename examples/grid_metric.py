#!/usr/bin/env python3
"""A spacetime that exists only as numbers: the metric sampled on a grid (RTGR_GRID, GridMetric).

A numerically computed spacetime — coalescing black holes from a numerical-relativity code — is g_ab on a Cartesian grid, with no
formula behind it.  This example makes such a grid from a spacetime we DO know, KerrSchild(1, 0.8) sampled with api.sample_metric,
traces example2's objects through it, and renders the closed form beside it:

    python examples/grid_metric.py [ni [h]]    # writes scenes/grid_metric.png: grid (left) | closed form (right), default 200, h = 0.15

A caller with simulation data builds the same GridMetric from its own (nz, ny, nx, 10) array (upper triangle tt tx ty tz xx xy xz yy
yz zz, x fastest) or (nz, ny, nx, 4, 4) array, origin and spacing.  Rays that leave the grid's valid box end with status RAY_OUTSIDE.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def main():
    ni = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    h = float(sys.argv[2]) if len(sys.argv) > 2 else 0.15
    closed = rt.KerrSchild(1.0, 0.8)
    L = 10.3                                       # the sky below is a sphere of radius 10: the valid box is [-L, L]^3
    n = int(round(2 * L / h)) + 3
    origin = (-L - h,) * 3
    g = rt.sample_metric(closed, origin, h, (n, n, n))
    # around the ring singularity (x² + y² = a², z = 0) the samples are huge or infinite; example2's rays never come within 3 of the
    # hole, so that region is simply filled with flat space
    c = origin[0] + h * np.arange(n)
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    g[x * x + y * y + z * z < 1.0] = [-1, 0, 0, 0, 1, 0, 0, 1, 0, 1]
    grid = rt.GridMetric(g, origin, h, name=f"KerrSchild(1, 0.8) at h = {h}")
    print(f"{grid}: {n ** 3} samples, {g.nbytes / 2 ** 20:.0f} MiB")
    caelum = rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -10)
    frustum = rt.Plane(-20)
    sphere = rt.Sphere((0, 4, 0, 0), (1, 0, 0, 0), 0.5)
    objs = [caelum, frustum, sphere]
    cam = dict(pos=(0, 4, -2, 0), widthx=(0, 1, 0, 0), widthy=(0, 0, 0, 1), normal=(0, 0, 1, 0))
    images = []
    for metric in (grid, closed):
        canvas = rt.make_canvas(metric, cam["pos"], cam["widthx"], cam["widthy"], cam["normal"], ni, ni)
        out, info = rt.trace_rays(metric, objs, canvas, return_info=True)
        images.append(out.image_u8())
        print(f"{metric}: {info}")
    diff = np.abs(images[0].astype(int) - images[1].astype(int)).max(axis=2)
    print(f"pixels that differ by more than 2/255: {int((diff > 2).sum())} of {ni * ni}")
    from raytracegr_jl_amd.png import write_png
    os.makedirs(rt.api.outdir, exist_ok=True)
    path = os.path.join(rt.api.outdir, "grid_metric.png")
    write_png(path, np.concatenate(images, axis=1))
    print("wrote", path)


if __name__ == "__main__":
    main()
