#!/usr/bin/env python3
"""The polarized image of a thin ring around the a = 0.998 hole, seen 20 degrees from the axis (rt.trace_polarized; include/rtgr.h
"polarized disk images").

    python examples/polarized_ring.py [ni nj]

A ring Disk(0.05, 4.5, 6) of synchrotron-emitting gas in an ordered field, once VERTICAL (B = e_z') and once TOROIDAL (B = e_phi'), seen
by a static observer at rho = 40.  The electric vector is perpendicular to the field as the gas sees the ray, carried to the camera by
the Walker-Penrose constants: a vertical field gives the azimuthal ("tangential") pattern, a toroidal one the radial pattern, each
twisted by aberration and by the hole's frame dragging.  Prints the position angle around the ring; draws the ticks over the picture
into scenes/polarized_ring.png when matplotlib is there.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def main():
    ni = int(sys.argv[1]) if len(sys.argv) > 1 else 240
    nj = int(sys.argv[2]) if len(sys.argv) > 2 else ni
    metric = rt.KerrSchild(1.0, 0.998)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -80.0), rt.Plane(-300.0), rt.Disk(0.05, 4.5, 6.0)]   # the ring is object 3
    opt = rt.solver_defaults(lambda1=300.0)
    emission = rt.DiskEmission(3, 30000.0)
    inc = math.radians(20.0)
    fov = 0.42
    obs = rt.Observer((0, 0, -40 * math.sin(inc), 40 * math.cos(inc)), (0, 0, math.sin(inc), -math.cos(inc)), (0, 0, 0, 1), fov,
                      2 * math.atan(math.tan(fov / 2) * nj / ni))
    fields = {"vertical": (0.0, 0.0, 1.0), "toroidal": (0.0, 1.0, 0.0)}
    frames = {}
    for name, field in fields.items():
        f = rt.trace_polarized(metric, objs, obs, ni, nj, emission, rt.Polarization("field", 0.7, field=field), opt=opt)
        frames[name] = f
        q, u = f["q"].reshape(nj, ni), f["u"].reshape(nj, ni)
        on = np.isfinite(q)
        chi = 0.5 * np.arctan2(u, q)              # from e^_x (screen right) towards e^_y (screen up)
        jj, ii = np.nonzero(on)
        theta = np.arctan2(jj - (nj - 1) / 2, ii - (ni - 1) / 2)     # the pixel's own direction from the frame's centre
        # the angle between the tick and the radial direction of the picture, folded to [0, 90] degrees: 90 = tangential, 0 = radial
        off = np.degrees(np.abs((chi[on] - theta + math.pi / 2) % math.pi - math.pi / 2))
        print(f"{name:9s} field: {int(on.sum())} pixels on the ring, degree {np.hypot(q[on], u[on]).mean():.3f}; tick against the radial direction: "
              f"median {np.median(off):5.1f} degrees (10 % .. 90 %: {np.percentile(off, 10):5.1f} .. {np.percentile(off, 90):5.1f})")
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        print("(matplotlib is not installed: no picture)")
        return
    fig, axes = plt.subplots(1, 2, figsize=(10, 5))
    step = max(1, ni // 30)
    for ax, (name, f) in zip(axes, frames.items()):
        img = np.clip(np.moveaxis(f["rgb"].reshape(3, nj, ni), 0, -1), 0, 1)
        ax.imshow(img / max(img.max(), 1e-30), origin="lower")
        q, u = f["q"].reshape(nj, ni), f["u"].reshape(nj, ni)
        jj, ii = np.mgrid[step // 2:nj:step, step // 2:ni:step]
        qq, uu = q[jj, ii], u[jj, ii]
        ok = np.isfinite(qq)
        chi, deg = 0.5 * np.arctan2(uu[ok], qq[ok]), np.hypot(qq[ok], uu[ok])
        ax.quiver(ii[ok], jj[ok], deg * np.cos(chi), deg * np.sin(chi), color="w", headwidth=0, headlength=0, headaxislength=0, pivot="middle",
                  scale=0.7 * ni / step, width=0.004)
        ax.set_title(f"{name} field")
        ax.set_axis_off()
    os.makedirs("scenes", exist_ok=True)
    fig.savefig(os.path.join("scenes", "polarized_ring.png"), dpi=120, bbox_inches="tight")
    print("wrote scenes/polarized_ring.png")


if __name__ == "__main__":
    main()
