#!/usr/bin/env python3
"""Disk emission: the a = 0.998 hole with a thin disk that GLOWS (rt.trace_emission; include/rtgr.h "disk emission").

    python examples/accretion_disk.py [ni nj] [--aa K] [--sky] [--retrograde] [--T kelvin]

writes scenes/accretion_disk.png: BASELINE config 5's scene — KerrSchild(1, 0.998), the sky sphere `caelum`, the far plane and
Disk(0.05, 2, 4) seen from example2's camera — with the disk emitting as a black body on the circular orbits of the metric: the side
that moves towards the camera is blue-shifted and bright, the receding side red and dim, and the gravitational redshift darkens the
inner rim.  --sky puts a seeded star field on `caelum` (an image texture, as in examples/textured_sky.py); --aa K anti-aliases the frame
(K x K sub-rays for the pixels on an edge of the EMITTED frame); --retrograde lets the gas orbit against the hole's spin (most of this
disk then lies inside the innermost retrograde circular orbit and stays black).  The frequency ratio g of every disk pixel is printed
as a range.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def main():
    argv, aa, T_in = list(sys.argv), None, 30000.0
    if "--aa" in argv:
        at = argv.index("--aa")
        aa = dict(k=int(argv[at + 1]), contrast=1.0 / 255.0)
        del argv[at:at + 2]
    if "--T" in argv:
        at = argv.index("--T")
        T_in = float(argv[at + 1])
        del argv[at:at + 2]
    sky, retro = "--sky" in argv, "--retrograde" in argv
    argv = [a for a in argv if a not in ("--sky", "--retrograde")]
    ni = int(argv[1]) if len(argv) > 1 else 400
    nj = int(argv[2]) if len(argv) > 2 else ni
    from raytracegr_jl_amd.png import write_png
    _, objs, cam = rt.example2_scene()                 # [caelum, frustum, sphere]
    objs = objs[:2] + [rt.Disk(0.05, 2.0, 4.0)]        # the disk is object 3 of the list: what `hit` holds for the rays that end on it
    emission = rt.DiskEmission(3, T_in, p=0.75, orbit=-1 if retro else +1, inner_edge=True, gain=0.6)
    textures = None
    if sky:
        from textured_sky import stars
        textures = {1: (rt.texture_load(stars()), rt._abi.TEX_BILINEAR)}
    res = rt.trace_emission(rt.KerrSchild(1.0, 0.998), objs, cam, ni, nj, emission, textures=textures, aa=aa)
    g = res["g"][np.isfinite(res["g"])]
    print(f"{np.isfinite(res['g']).sum()} emitting pixels" + (f", g in [{g.min():.3f}, {g.max():.3f}]" if len(g) else ""))
    img = np.rint(np.clip(res["rgb"].reshape(3, nj, ni), 0.0, 1.0) * 255.0).astype(np.uint8)
    os.makedirs(rt.api.outdir, exist_ok=True)
    file = os.path.join(rt.api.outdir, "accretion_disk.png")
    write_png(file, np.ascontiguousarray(np.transpose(img, (1, 2, 0))))
    print(f'Output file is "{file}"  ({res["counters"]["rays"]} rays)')
    if textures:
        textures[1][0].unload()


if __name__ == "__main__":
    main()
