#!/usr/bin/env python3
"""The photon ring of an optically thin disk around the a = 0.9 hole (rt.trace_orders; include/rtgr.h "higher-order disk images").

    python examples/photon_ring.py [ni nj]

KerrSchild(1, 0.9) with Disk(0.05, 3, 12), seen by a static observer at (0, 0, -18, 9) looking at the origin.  The trace ends a ray
where it first meets the disk; rt.trace_orders carries it through and traces on, order by order: order 1 is the lensed image of the
disk's far side and underside, order 2 the photon ring.  With transmission T = 1 the picture is the sum of all orders.  Prints how many
pixels have each order; writes the sum and the order-1 and order-2 planes on their own into scenes/photon_ring*.png.
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
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -30.0), rt.Disk(0.05, 3.0, 12.0)]   # the disk is object 2
    opt = rt.solver_defaults(max_steps=4000, lambda1=200.0)
    obs = rt.Observer((0, 0, -18, 9), (0, 0, 18, -9), (0, 0, 0, 1), 1.4, 1.05)
    f = rt.trace_orders(metric, objs, obs, ni, nj, rt.DiskEmission(2, 30000.0), rt.DiskOrders(3, transmission=1.0), opt=opt)
    for k in range(4):
        on = f["hit32"][k] == 2
        g = f["g"][k][on]
        print(f"order {k}: {int(on.sum()):6d} pixels" + (f", frequency ratio {g.min():.3f} .. {g.max():.3f}" if on.any() else ""))
    print("disk crossings per pixel (0, 1, 2, ...):", np.bincount(f["count"]).tolist())
    import importlib
    write_png = importlib.import_module(rt.__name__ + ".png").write_png
    os.makedirs("scenes", exist_ok=True)
    scale = max(float(np.nanmax(f["rgb_order"][0][:, f["hit32"][0] == 2], initial=0.0)), 1e-30)
    pictures = {"photon_ring.png": f["rgb"], "photon_ring_order1.png": f["rgb_order"][1], "photon_ring_order2.png": f["rgb_order"][2]}
    for name, planes in pictures.items():
        img = np.clip(np.nan_to_num(planes) / scale, 0, 1).reshape(3, nj, ni)
        write_png(os.path.join("scenes", name), np.ascontiguousarray((255 * np.moveaxis(img, 0, -1)[::-1]).astype(np.uint8)))
        print("wrote scenes/" + name)


if __name__ == "__main__":
    main()
