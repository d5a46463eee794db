#!/usr/bin/env python3
"""Image textures: example2's black hole in front of a sky that shows a PICTURE (rt.trace_shaded; include/rtgr.h "image textures").

    python examples/textured_sky.py [ni nj] [--aa K] [--stars]

writes two frames of example2's scene (src/RayTraceGR.jl:578-612):
    scenes/textured_sky.png       the sky sphere `caelum` (radius -10) wears a texture instead of the reference's 24-band sawtooth; the small
                                  sphere and the far plane keep the reference's colours
    scenes/textured_escape.png    `caelum` and the far plane removed: the texture is bound to the rays that ESCAPE, coloured by the
                                  direction they end with; rays that end in the hole stay black (miss_rgb = 0)
The texture is made here with numpy — a checkerboard over (theta, phi) with a coloured meridian band, or with --stars a seeded star
field; no image file is read.  --aa K anti-aliases both frames (K x K sub-rays for the pixels on an edge — of the SHADED frame, so the
checker's own edges are refined too).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from __graft_entry__ import load_package

rt = load_package()


def checker(W=512, H=256, cells=16):
    """(3, H, W): a checkerboard of `cells` squares from pole to pole, red towards phi = 0 and blue towards phi = +-pi"""
    q, r = np.meshgrid(np.arange(W), np.arange(H))
    on = ((q * 2 * cells // W) + (r * cells // H)) % 2 == 0
    phi = -np.pi + (q + 0.5) * 2 * np.pi / W
    t = np.empty((3, H, W))
    t[0] = np.where(on, 0.9, 0.1) * (0.55 + 0.45 * np.cos(phi))
    t[1] = np.where(on, 0.9, 0.1) * 0.8
    t[2] = np.where(on, 0.9, 0.1) * (0.55 - 0.45 * np.cos(phi))
    return t


def stars(W=1024, H=512, n=4000, seed=4):
    """(3, H, W): n seeded stars, uniform on the sphere, each a small Gaussian blob of a random warm / cold tint"""
    rng = np.random.default_rng(seed)
    t = np.zeros((3, H, W))
    z = rng.uniform(-1.0, 1.0, n)
    q0 = rng.uniform(0, W, n)
    r0 = np.arccos(z) / np.pi * H
    tint = rng.uniform(0.6, 1.0, (n, 3)) * rng.uniform(0.3, 1.0, (n, 1))
    for k in range(n):
        rr, qq = np.arange(int(r0[k]) - 3, int(r0[k]) + 4), np.arange(int(q0[k]) - 3, int(q0[k]) + 4)
        w = np.exp(-((rr[:, None] - r0[k]) ** 2 + (qq[None, :] - q0[k]) ** 2) / 1.5)
        ok = (rr >= 0) & (rr < H)
        t[:, rr[ok][:, None], qq[None, :] % W] += tint[k][:, None, None] * w[ok][None]
    return np.clip(t, 0.0, 1.0)


def main():
    argv, aa = list(sys.argv), None
    if "--aa" in argv:
        at = argv.index("--aa")
        aa = dict(k=int(argv[at + 1]), contrast=1.0 / 255.0)
        del argv[at:at + 2]
    star_field = "--stars" in argv
    argv = [a for a in argv if a != "--stars"]
    ni = int(argv[1]) if len(argv) > 1 else 400
    nj = int(argv[2]) if len(argv) > 2 else ni
    from raytracegr_jl_amd.png import write_png
    metric, objs, cam = rt.example2_scene()            # [caelum, frustum, sphere]
    tex = rt.texture_load(stars() if star_field else checker())
    os.makedirs(rt.api.outdir, exist_ok=True)

    def save(res, name):
        img = np.rint(np.clip(res["rgb"].reshape(3, nj, ni), 0.0, 1.0) * 255.0).astype(np.uint8)
        file = os.path.join(rt.api.outdir, name)
        write_png(file, np.ascontiguousarray(np.transpose(img, (1, 2, 0))))
        print(f'Output file is "{file}"  ({res["counters"]["rays"]} rays)')

    # the sky is object 1 of the list: what `hit` holds for the rays that end on it
    save(rt.trace_shaded(metric, objs, cam, ni, nj, textures={1: (tex, rt._abi.TEX_BILINEAR)}, aa=aa), "textured_sky.png")
    # no sky and no far plane (it would end every ray at t = -20): the rays that reach lambda1 far out are the ones that escape
    black = rt.solver_defaults(miss_rgb=(0.0, 0.0, 0.0))
    save(rt.trace_shaded(metric, objs[2:], cam, ni, nj, textures={0: (tex, rt._abi.TEX_BILINEAR)}, r_escape=20.0, aa=aa, opt=black), "textured_escape.png")
    tex.unload()


if __name__ == "__main__":
    main()
