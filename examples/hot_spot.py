#!/usr/bin/env python3
"""A hot spot in the disk of the a = 0.998 hole: its light curve and the track of its image centroid from ONE traced frame
(rt.light_curve; include/rtgr.h "hot-spot light curves").

    python examples/hot_spot.py [ni nj] [--nt samples] [--T kelvin]

BASELINE config 5's hole and disk — KerrSchild(1, 0.998), Disk(0.05, 2, 4) — seen by a static observer at rho = 50, 60 degrees from
the axis.  A Gaussian spot (sigma = 0.4) rides in the disk at rho_s = 4 with the orbital rate of the disk's own gas; two orbital periods
are sampled at 512 observer times.  Writes scenes/hot_spot.png (the frame: the disk without the spot — the picture does not depend on the
observer time), scenes/hot_spot_lc.npy ([nt, 4]: tau, F, A, B) and scenes/hot_spot_track.txt (tau, F / max F, the centroid A / F, B / F in
the frame's pixel coordinates a, b in (-1, 1)).  The frame is traced once; the nt observer times cost one reduction on the device.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def main():
    argv, T_in, nt = list(sys.argv), 30000.0, 512
    for flag in ("--T", "--nt"):
        if flag in argv:
            at = argv.index(flag)
            if flag == "--T":
                T_in = float(argv[at + 1])
            else:
                nt = int(argv[at + 1])
            del argv[at:at + 2]
    ni = int(argv[1]) if len(argv) > 1 else 400
    nj = int(argv[2]) if len(argv) > 2 else ni * 2 // 3
    from raytracegr_jl_amd.png import write_png
    metric = rt.KerrSchild(1.0, 0.998)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -80.0), rt.Plane(-300.0), rt.Disk(0.05, 2.0, 4.0)]   # the disk is object 3
    opt = rt.solver_defaults(lambda1=300.0)
    emission = rt.DiskEmission(3, T_in, p=0.75, inner_edge=True, gain=0.6)
    inc = math.radians(60.0)
    fov_x = 0.3
    obs = rt.Observer((0, 50 * math.sin(inc), 0, 50 * math.cos(inc)), (0, -math.sin(inc), 0, -math.cos(inc)), (0, 0, 0, 1), fov_x,
                      2 * math.atan(math.tan(fov_x / 2) * nj / ni))
    omega = rt.eval_hot_spot(metric, objs, emission, rt.HotSpot(4.0, 0.4))["omega_s"]
    period = 2 * math.pi / omega
    spot = rt.HotSpot(4.0, 0.4, t_start=0.0, dt=2 * period / nt, nt=nt, cut=4.0, g_power=4.0)
    res = rt.light_curve(metric, objs, obs, ni, nj, emission, spot, opt=opt)
    tau, (F, A, B) = res["tau"], res["lc"].T
    lit = F > 0
    print(f"Omega_s = {omega:.6f} (period {period:.3f}), {int(np.isfinite(res['g']).sum())} emitting pixels, {nt} observer times over two periods")
    print(f"F: max / min = {F.max() / max(F[lit].min(), 1e-300):.2f} (Doppler beaming and lensing), brightest at tau = {tau[F.argmax()]:.2f}")
    os.makedirs(rt.api.outdir, exist_ok=True)
    img = np.rint(np.clip(res["rgb"].reshape(3, nj, ni), 0.0, 1.0) * 255.0).astype(np.uint8)
    file = os.path.join(rt.api.outdir, "hot_spot.png")
    write_png(file, np.ascontiguousarray(np.transpose(img, (1, 2, 0))))
    print(f'Output file is "{file}"  ({res["counters"]["rays"]} rays, {res["counters"]["not_finished"]} not finished)')
    np.save(os.path.join(rt.api.outdir, "hot_spot_lc.npy"), np.column_stack([tau, F, A, B]))
    track = np.full((nt, 4), np.nan)
    track[:, 0], track[:, 1] = tau, F / F.max()
    track[lit, 2], track[lit, 3] = A[lit] / F[lit], B[lit] / F[lit]
    np.savetxt(os.path.join(rt.api.outdir, "hot_spot_track.txt"), track, header="tau  F / max F  centroid a  centroid b")
    print(f'Light curve and centroid track: "{os.path.join(rt.api.outdir, "hot_spot_lc.npy")}", "hot_spot_track.txt"')


if __name__ == "__main__":
    main()
