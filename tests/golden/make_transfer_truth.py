"""Generates tests/golden/truth_transfer.npz (CPU only, no product code): rays of a static observer through the flow of "volume emission",
each with the DOP853 truth of (I, tau, s_end), the Tsit5 twin's in Float64 and Float32, and the twin's error against the truth
(tests/transfer_truth.py).

    python tests/golden/make_transfer_truth.py [--jobs N]

Rays.  A KS_TRUE M = 1, a = 0.9 scene: the observer static at r = 40, inclination 60 deg, a sky at r = 60 (lambda_end is where the ray
reaches it).  A ray leaves along (towards the hole) + (b / 40) e, e a unit vector across the line of sight — so b is the impact
parameter: one far miss, rays through the flow's bulk on either side of the spin, two that graze the photon orbit (b 0.2 % outside the
critical value found by bisection: the longest paths), and captured ones (they end at r_stop, inside the dark cylinder).  Four rays
of the as-written KS_REF a = 0 scene the same way.

r_stop.  The library's rays are past-directed, and in ingoing Kerr-Schild coordinates a past-directed captured ray never crosses the
horizon: it creeps up to it.  The horizon's coordinate radius sqrt(r_+² + a² sin² theta) is 1.44 .. 1.70 for a = 0.9, so a
sphere of radius 1.5 is reached by no captured ray near the equator.  r_stop must lie between the horizon and the
dark cylinder (rho < 1.80 for a = 0.9 prograde; rho < 2.25 in the as-written a = 0 metric, whose horizon is at 1.56): 1.75 and 2.0 here.
Each ray is run optically thin (kappa = 0) and with kappa > 0; j0 is chosen so that
the largest I is of order 1, kappa so that the largest tau is."""
import multiprocessing
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import transfer_truth as tt  # noqa: E402

R_OBS, R_SKY, INCL, LAMBDA1 = 40.0, 60.0, np.radians(60.0), 400.0
R_STOP = {"ks_true09": 1.75, "ks_ref0": 2.0}
FLOW = dict(emitter=tt.KEPLER, orbit=1.0, r0=4.0, alpha=1.5, H=0.4, s=0.5)
SCENES = {"ks_true09": ("ks_true", 1.0, 0.9), "ks_ref0": ("ks_ref", 1.0, 0.0)}
TOL64, TOL32 = tt.EPS64 ** 0.75, tt.EPS32 ** 0.75


def opt_of(tol):
    return dict(reltol=tol, abstol=tol, lambda0=0.0, lambda1=LAMBDA1, max_steps=100000)


def geometry():
    pos = np.array([0.0, R_OBS * np.sin(INCL), 0.0, R_OBS * np.cos(INCL)])
    rad = -pos[1:] / R_OBS
    ey = np.array([0.0, 1.0, 0.0])
    e2 = np.cross(rad, ey)
    return pos, rad, ey, e2


def state(scene, b, e):
    pos, rad, _, _ = geometry()
    return tt.camera_state(scene, pos, rad + (b / R_OBS) * e)


def critical_b(args):
    name, sign = args
    scene = tt.Scene(*SCENES[name])
    _, _, ey, _ = geometry()
    lo, hi = 1.0, 12.0      # captured, escapes
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        if tt.escape_lambda(scene, state(scene, mid, sign * ey), R_SKY, LAMBDA1, R_STOP[name]) is None:
            lo = mid
        else:
            hi = mid
    return hi


def run(args):
    name, s0, lam_end, fl = args
    scene = tt.Scene(*SCENES[name])
    try:
        tr = tt.truth(scene, fl, s0, lam_end)
    except AssertionError as e:
        # dtau/dlambda = kappa n w is unbounded where a ray crosses the photon orbit's cylinder with kappa > 0 (w ~ 1 / sqrt(-n2): integrable,
        # but DOP853 at rtol 1e-13 gives up on it): no truth for that run; the tests leave it out by its NaN and say so
        print("no truth:", name, fl["kappa"], lam_end, e, flush=True)
        tr = dict(I=np.nan, tau=np.nan, s_end=np.full(8, np.nan), lam=np.nan, stopped=lam_end == LAMBDA1)
    t64 = tt.twin(scene, fl, s0, lam_end, opt_of(TOL64), dt=np.float64)
    t32 = tt.twin(scene, fl, s0.astype(np.float32), np.float32(lam_end), opt_of(TOL32), dt=np.float32)
    # THE TWIN'S ERROR is recorded over a small ensemble: the run above and eight more whose start state is one ulp off in one component.
    # The integrand has a kink where the gas begins (w gfac^(3+s) ~ (rho - rho_ph)^(5/4)), and where the steps fall across it decides an
    # error of 1e-10 or of 1e-13: a single run's figure is a draw, not a size (ray 15: 2.0e-13 unperturbed, up to 1.3e-10 one ulp away,
    # while the true I moves by a few ulp).  The maximum over the ensemble is what a solver of this kind and tolerance delivers.
    for t, dt in ((t64, np.float64), (t32, np.float32)):
        ens = [t] + [tt.twin(scene, fl, nudged(s0.astype(dt), c, up), dt(lam_end), opt_of(TOL64 if dt is np.float64 else TOL32), dt=dt)
                     for c, up in ENSEMBLE]
        for q in ("I", "tau"):
            t["err_" + q] = float(np.max([abs(float(e[q]) - float(tr[q])) for e in ens]))
        # … and so is a step count: how far the ensemble's counts lie from the unperturbed run's is the twin's own step noise
        t["steps_spread"] = int(max(abs(int(e["steps"]) - int(t["steps"])) for e in ens))
    return tr, t64, t32


ENSEMBLE = ((5, True), (5, False), (6, True), (6, False), (7, True), (7, False), (1, True), (2, False))


def nudged(s0, comp, up):
    s = s0.copy()
    s[comp] = np.nextafter(s[comp], s.dtype.type(np.inf if up else -np.inf))
    return s


def main():
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else min(32, os.cpu_count() or 4)
    _, _, ey, e2 = geometry()
    with multiprocessing.Pool(jobs) as pool:
        bc = pool.map(critical_b, [("ks_true09", +1), ("ks_true09", -1), ("ks_ref0", +1)])
        print("critical b: ks_true09 +y %.6f, -y %.6f; ks_ref0 %.6f" % tuple(bc), flush=True)
        rays = [("ks_true09", 20.0, ey), ("ks_true09", 12.0, -ey), ("ks_true09", 8.0, ey), ("ks_true09", 8.0, -ey), ("ks_true09", 6.5, e2),
                ("ks_true09", 10.0, -e2), ("ks_true09", 5.0, ey), ("ks_true09", 7.5, -e2), ("ks_true09", bc[0] * 1.002, ey),
                ("ks_true09", bc[1] * 1.002, -ey), ("ks_true09", 1.0, ey), ("ks_true09", 2.0, -e2),
                ("ks_ref0", 20.0, ey), ("ks_ref0", 8.0, -ey), ("ks_ref0", bc[2] * 1.002, ey), ("ks_ref0", 1.0, ey)]
        scenes = {k: tt.Scene(*v) for k, v in SCENES.items()}
        s0 = [state(scenes[n], b, e) for n, b, e in rays]
        lam = pool.starmap(tt.escape_lambda, [(scenes[n], s, R_SKY, LAMBDA1, R_STOP[n]) for (n, _, _), s in zip(rays, s0)])
        captured = np.array([v is None for v in lam])
        lam_end = np.array([LAMBDA1 if v is None else v for v in lam])
        print("lambda_end:", np.round(lam_end, 2), "captured:", captured.astype(int), flush=True)
        # scale: the twin at j0 = kappa = 1 (tau does not depend on j0) and at j0 = 1, kappa = 0 (I is linear in j0)
        probe = pool.map(run_twin, [(n, s, le, dict(FLOW, j0=1.0, kappa=kap, r_stop=R_STOP[n])) for kap in (0.0, 1.0) for (n, _, _), s, le in zip(rays, s0, lam_end)])
        nr = len(rays)
        imax = max(float(p["I"]) for p in probe[:nr])
        taumax = max(float(p["tau"]) for p in probe[nr:])
        j0 = float("%.2g" % (1.0 / imax))
        kappa = float("%.2g" % (1.0 / taumax))
        print(f"max I at j0 = 1: {imax:.4g} -> j0 = {j0}; max tau at kappa = 1: {taumax:.4g} -> kappa = {kappa}", flush=True)
        kappas = (0.0, kappa)
        res = pool.map(run, [(n, s, le, dict(FLOW, j0=j0, kappa=kap, r_stop=R_STOP[n])) for kap in kappas for (n, _, _), s, le in zip(rays, s0, lam_end)])
    shape = (2, nr)
    col = lambda which, key, dt=np.float64: np.array([r[which][key] for r in res], dt).reshape(shape + np.shape(res[0][which][key]))
    out = dict(scene=np.array([n for n, _, _ in rays]), b=np.array([b for _, b, _ in rays]), s0=np.array(s0), lambda_end=lam_end, captured=captured,
               kappas=np.array(kappas), j0=j0, flow=np.array([FLOW[k] for k in ("orbit", "r0", "alpha", "H", "s")]), r_stop=np.array([R_STOP[n] for n, _, _ in rays]),
               lambda1=LAMBDA1, tol64=TOL64, tol32=TOL32,
               truth_I=col(0, "I"), truth_tau=col(0, "tau"), truth_s_end=col(0, "s_end"), truth_stopped=col(0, "stopped", bool))
    for tag, which, dt in (("twin64", 1, np.float64), ("twin32", 2, np.float32)):
        out.update({f"{tag}_I": col(which, "I", dt), f"{tag}_tau": col(which, "tau", dt), f"{tag}_s_end": col(which, "s_end", dt),
                    f"{tag}_status": col(which, "status", np.uint8), f"{tag}_steps": col(which, "steps", np.uint32)})
        out[f"{tag}_err_I"], out[f"{tag}_err_tau"] = col(which, "err_I"), col(which, "err_tau")      # (over the ensemble: see run)
        out[f"{tag}_steps_spread"] = col(which, "steps_spread", np.uint32)
        out[f"{tag}_err1_tau"] = np.abs(out[f"{tag}_tau"].astype(np.float64) - out["truth_tau"])
        out[f"{tag}_err1_I"] =np.abs(out[f"{tag}_I"].astype(np.float64) - out["truth_I"])              # (the unperturbed run alone)
    for k in ("truth_I", "truth_tau", "twin64_err_I", "twin64_err_tau", "twin32_err_I", "twin32_err_tau", "twin64_steps", "twin32_steps", "twin64_status"):
        print(k, out[k], flush=True)
    path = os.path.join(HERE, "truth_transfer.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


def run_twin(args):
    name, s0, lam_end, fl = args
    return tt.twin(tt.Scene(*SCENES[name]), fl, s0, lam_end, opt_of(TOL64), dt=np.float64)


if __name__ == "__main__":
    main()
