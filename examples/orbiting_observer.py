#!/usr/bin/env python3
"""The observer camera: the a = 0.998 hole and its glowing disk seen from a circular orbit (rt.trace_observer; include/rtgr.h "observer
camera").

    python examples/orbiting_observer.py [ni nj] [--retrograde] [--static] [--T kelvin]

writes scenes/orbiting_observer.png and scenes/orbiting_observer_sky.png: BASELINE config 5's hole and disk — KerrSchild(1, 0.998),
Disk(0.05, 2, 4) — inside a sky sphere of radius 30, seen by an observer on the prograde circular geodesic at rho = 12 in the equatorial
plane.  The first image is a perspective frame (60 degrees wide) looking at the hole: the disk edge-on, its far side lifted above and
below the hole by lensing, the colours shifted by the disk's motion AND the observer's own.  The second is the full sky as an
equirectangular panorama (twice as wide as high) centred on the direction of motion: aberration crowds the sky towards that direction.
--static puts the observer at rest at the same event instead, --retrograde on the other circular orbit.  The frame the library built is
printed: Omega, the observer's 4-velocity, and the range of the frequency ratio g over the disk's pixels.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def main():
    argv, T_in = list(sys.argv), 30000.0
    if "--T" in argv:
        at = argv.index("--T")
        T_in = float(argv[at + 1])
        del argv[at:at + 2]
    static, retro = "--static" in argv, "--retrograde" in argv
    argv = [a for a in argv if a not in ("--static", "--retrograde")]
    ni = int(argv[1]) if len(argv) > 1 else 400
    nj = int(argv[2]) if len(argv) > 2 else ni * 2 // 3
    from raytracegr_jl_amd.png import write_png
    metric = rt.KerrSchild(1.0, 0.998)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -30.0), rt.Plane(-100.0), rt.Disk(0.05, 2.0, 4.0)]   # the disk is object 3
    opt = rt.solver_defaults(lambda1=200.0)
    emission = rt.DiskEmission(3, T_in, p=0.75, inner_edge=True, gain=0.6)
    kind = "static" if static else "circular"
    pos, up = (0.0, 0.0, -12.0, 0.0), (0, 0, 0, 1)
    motion = (0, -1, 0, 0) if retro else (0, 1, 0, 0)           # the direction the orbit moves in at pos
    views = {"orbiting_observer.png": (rt.Observer(pos, (0, 0, 1, 0), up, math.radians(60.0), 2 * math.atan(math.tan(math.radians(30.0)) * nj / ni),
                                                   kind=kind, orbit=-1 if retro else +1), ni, nj),
             "orbiting_observer_sky.png": (rt.Observer(pos, motion, up, 2 * math.pi, math.pi, kind=kind, orbit=-1 if retro else +1,
                                                       projection="equirect"), ni, ni // 2)}
    os.makedirs(rt.api.outdir, exist_ok=True)
    for name, (obs, w, h) in views.items():
        frame = rt.eval_observer(metric, objs, obs)
        res = rt.trace_observer(metric, objs, obs, w, h, emission=emission, opt=opt)
        g = res["g"][np.isfinite(res["g"])]
        print(f"{name}: Omega = {frame['omega']:.6f}, u = {np.array2string(frame['frame'][0], precision=4)}, {len(g)} emitting pixels"
              + (f", g in [{g.min():.3f}, {g.max():.3f}]" if len(g) else ""))
        img = np.rint(np.clip(res["rgb"].reshape(3, h, w), 0.0, 1.0) * 255.0).astype(np.uint8)
        file = os.path.join(rt.api.outdir, name)
        write_png(file, np.ascontiguousarray(np.transpose(img, (1, 2, 0))))
        print(f'Output file is "{file}"  ({res["counters"]["rays"]} rays, {res["counters"]["not_finished"]} not finished)')


if __name__ == "__main__":
    main()
