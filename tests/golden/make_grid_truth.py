#!/usr/bin/env python3
"""Generates tests/golden/truth_grid_<name>.npz for name in quad3, quad4, quad3_box, quad4_box: 64 rays through the polynomial
field of tests/grid_truth.py — the field a grid kernel integrates EXACTLY when it is loaded with that field's samples — as
tests/truth.py integrates them (symbolic derivatives, d_t g included, scipy DOP853 at rtol 1e-13).  Per ray: state0, state_end,
lambda_end, hit, rgb, clearance, self_err (against rtol 1e-11), lambda_exit and state_exit (the first λ outside the grid's valid box, inf: never, and the state there)
and `marked`: rays left out of the tests' statistics — clearance below the hit threshold or another object hit by the looser run (a grazing ray), or an
object met AFTER leaving the box.  Also the coefficient table and the grid's description; the samples are not stored (grid_truth.samples rebuilds
them).

    python tests/golden/make_grid_truth.py [name ...]         # ≈ 1 min on 8 cores
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def one(job):
    import grid_truth as G
    import truth
    name, i, j = job
    coef = G.field_table(G.GRIDS[name]["dim"])
    sc, cam = G.truth_scene(name)
    s0 = truth.pixel_state(sc, cam, G.FRAME[0], G.FRAME[1], i, j, metric_fn=G.metric_at(coef))
    r = G.trace_truth(name, coef, s0)
    loose = G.trace_truth(name, coef, s0, rtol=1e-11, atol=1e-13)
    self_err = np.abs(r["state_end"] - loose["state_end"]).max() if loose["hit"] == r["hit"] else np.inf
    return s0, r["state_end"], r["lambda_end"], r["hit"], r["rgb"], r["clearance"], self_err, r["lambda_exit"], r["state_exit"]


def main(names):
    import grid_truth as G
    from scenes import rt
    ij = G.pixels()
    threshold = rt.solver_defaults().hit_threshold
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for name in names:
            grid = G.GRIDS[name]
            res = pool.map(one, [(name, int(i), int(j)) for i, j in ij], chunksize=2)
            col = lambda k, **kw: np.array([r[k] for r in res], **kw)
            hit, lam_end, lam_exit, clearance = col(3, dtype=np.uint8), col(2), col(7), col(5)
            late = (hit > 0) & (lam_end > lam_exit)              # an object met after leaving the valid box
            marked = (clearance < threshold) | late | ~np.isfinite(col(6))
            out = os.path.join(HERE, f"truth_grid_{name}.npz")
            np.savez_compressed(out, n=np.array(G.FRAME), ij=ij, state0=col(0), state_end=col(1), lambda_end=lam_end, hit=hit, rgb=col(4),
                                clearance=clearance, self_err=col(6), lambda_exit=lam_exit, state_exit=col(8), marked=marked,
                                coef=G.field_table(grid["dim"]), origin=np.array(grid["origin"]), spacing=np.array(grid["spacing"]),
                                grid_n=np.array(grid["n"]))
            se = col(6)
            print(name, os.path.getsize(out), "bytes; hit classes", np.bincount(hit, minlength=5), "left the box", int(np.isfinite(lam_exit).sum()),
                  "marked", int(marked.sum()), "(late %d)" % int(late.sum()), "self_err max %.1e" % se.max(),
                  "lambda_end max %.2f, t_end min %.2f" % (lam_end.max(), col(1)[:, 0].min()), flush=True)


if __name__ == "__main__":
    import grid_truth
    main(sys.argv[1:] or list(grid_truth.NAMES))
