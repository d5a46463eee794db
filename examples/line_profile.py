#!/usr/bin/env python3
"""The relativistic line profile and the thermal spectrum of the disk of the a = 0.998 hole, each from ONE traced frame
(rt.spectrum; include/rtgr.h "disk spectra").

    python examples/line_profile.py [ni nj] [--nb bins] [--T kelvin]

BASELINE config 5's hole and disk — KerrSchild(1, 0.998), Disk(0.05, 2, 4) — seen by a static observer at rho = 50, 30 and 75 degrees
from the axis.  The line: rest energy 1, emissivity rho^-3 over the whole disk, weight g^4, nb bins over g in [0, 1.6): the broad red
wing of the gravitational redshift at both inclinations, the blue horn of the approaching side at 75 degrees.  The thermal spectrum:
theta^3 / expm1(theta / (g T)) summed over the image at 16 frequencies, geometrically spaced.  Prints both as tables; plots them into
scenes/line_profile.png when matplotlib is there.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def main():
    argv, T_in, nb = list(sys.argv), 30000.0, 32
    for flag in ("--T", "--nb"):
        if flag in argv:
            at = argv.index(flag)
            if flag == "--T":
                T_in = float(argv[at + 1])
            else:
                nb = int(argv[at + 1])
            del argv[at:at + 2]
    ni = int(argv[1]) if len(argv) > 1 else 400
    nj = int(argv[2]) if len(argv) > 2 else ni * 2 // 3
    metric = rt.KerrSchild(1.0, 0.998)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -80.0), rt.Plane(-300.0), rt.Disk(0.05, 2.0, 4.0)]   # the disk is object 3
    opt = rt.solver_defaults(lambda1=300.0)
    emission = rt.DiskEmission(3, T_in, p=0.75, inner_edge=True)
    line = rt.Spectrum("line", 0.0, 1.6, nb, alpha=3.0, rho_min=2.0, rho_max=4.0, g_power=4.0)
    thermal = rt.Spectrum("thermal", 2.0e3, 2.0e5, 16, log=True, nu3=True)
    fov_x = 0.3
    profiles, spectra = {}, {}
    for deg in (30.0, 75.0):
        inc = math.radians(deg)
        obs = rt.Observer((0, 50 * math.sin(inc), 0, 50 * math.cos(inc)), (0, -math.sin(inc), 0, -math.cos(inc)), (0, 0, 0, 1), fov_x,
                          2 * math.atan(math.tan(fov_x / 2) * nj / ni))
        profiles[deg] = rt.spectrum(metric, objs, obs, ni, nj, emission, line, opt=opt)
        spectra[deg] = rt.spectrum(metric, objs, obs, ni, nj, emission, thermal, opt=opt)
        g = profiles[deg]["g"]
        print(f"{deg:.0f} degrees: {int(np.isfinite(g).sum())} emitting pixels, g from {np.nanmin(g):.3f} to {np.nanmax(g):.3f}")
    print("\nline profile: F per bin of g, normalised to its peak")
    print("      g     " + "".join(f"{deg:>10.0f}°" for deg in profiles))
    for b in range(nb):
        print(f"  {profiles[30.0]['axis'][b]:7.4f}   " + "".join(f"{p['F'][b] / p['F'].max():11.4f}" for p in profiles.values()))
    print("\nthermal spectrum: theta = h nu / k_B in kelvin, theta^3 sum w / expm1(theta / (g T)), normalised to its peak")
    print("   theta    " + "".join(f"{deg:>10.0f}°" for deg in spectra))
    for k in range(int(thermal.nb)):
        print(f"  {spectra[30.0]['axis'][k]:9.1f} " + "".join(f"{s['F'][k] / s['F'].max():11.4f}" for s in spectra.values()))
    try:
        import matplotlib
    except ImportError:
        return
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    os.makedirs(rt.api.outdir, exist_ok=True)
    fig, (a0, a1) = plt.subplots(1, 2, figsize=(9, 3.5))
    for deg in profiles:
        a0.step(profiles[deg]["axis"], profiles[deg]["F"] / profiles[deg]["F"].max(), where="mid", label=f"{deg:.0f}°")
        a1.loglog(spectra[deg]["axis"], spectra[deg]["F"] / spectra[deg]["F"].max(), "o-", label=f"{deg:.0f}°")
    a0.set_xlabel("g = E_obs / E_rest")
    a1.set_xlabel("h nu / k_B  [K]")
    a0.legend()
    file = os.path.join(rt.api.outdir, "line_profile.png")
    fig.savefig(file, dpi=120, bbox_inches="tight")
    print(f'Output file is "{file}"')


if __name__ == "__main__":
    main()
