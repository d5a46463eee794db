"""The truth side of tests/test_transfer.py (include/rtgr.h "volume emission"), in numpy / scipy — TEST-SIDE ONLY, no product code:

  * flow_point(...)   the flow model of the header's contract at one point, restated in numpy from truth._metric_fn's symbolic g and dg
                      (dtype-generic: the arithmetic runs in the dtype of its inputs);
  * truth(...)        the 10-vector (x, k, tau, I) integrated by DOP853 at rtol 1e-13, atol 1e-15, max_step 0.05, on truth.rhs(scene);
  * twin(...)         a plain numpy restatement of the Tsit5 + PI loop of the contract on the 10 components, float64 or float32: what a
                      solver of the transfer kernel's kind and tolerance delivers, and so the yardstick of the kernel's own error;
  * camera_state(...) the start state of a ray of a static observer (k_0 = (-e_0 + n) / sqrt 2, past-directed), and the rays of the
                      fixture tests/golden/truth_transfer.npz (golden/make_transfer_truth.py).

Nothing here knows the device code: the formulas are typed from the header's contract."""
import functools

import numpy as np

import truth as T

KEPLER, RIGID = 0, 1
EPS64, EPS32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)


class Scene:
    """what truth.rhs / truth._kind read of an rtgr_scene: kind 'mink' | 'ks_ref' | 'ks_true' (the values of enum rtgr_metric)"""
    def __init__(self, kind, M=1.0, a=0.0):
        self.metric, self.user_metric, self.M, self.a = {"mink": 0, "ks_ref": 1, "ks_true": 2}[kind], 0, float(M), float(a)


_kind = T._kind


def flow_params(emitter=KEPLER, orbit=1.0, j0=1.0, kappa=0.0, r0=1.0, alpha=1.0, H=0.3, s=0.0, r_stop=0.0):
    return dict(emitter=emitter, orbit=orbit, j0=j0, kappa=kappa, r0=r0, alpha=alpha, H=H, s=s, r_stop=r_stop)


@functools.lru_cache(maxsize=None)
def _ks_parts(kind):
    """truth.metric_expr(kind) = eta + f k k^T taken apart SYMBOLICALLY — f = g_tt + 1, k_i = g_ti / f (k_t = 1) — with sympy's own
    derivatives of f and k: 16 small expressions instead of the 64 entries of the expanded dg, which cost 1.3 ms a call.  The DOP853
    truth makes 40 000 calls per ray; tests/test_transfer.py holds this function to truth._metric_fn at random points."""
    import sympy as sp
    (x, y, z, M, a), g = T.metric_expr(kind)
    f = g[0, 0] + 1
    k = [g[0, i] / f for i in (1, 2, 3)]
    exprs = [f] + k + [sp.diff(f, v) for v in (x, y, z)] + [sp.diff(ki, v) for v in (x, y, z) for ki in k]
    return sp.lambdify((x, y, z, M, a), exprs, modules="math", cse=True)


ETA = np.diag([-1.0, 1.0, 1.0, 1.0])


def _metric64(kind, M, a, p):
    if kind == "mink":
        return ETA.copy(), np.zeros((3, 4, 4))
    try:
        v = _ks_parts(kind)(float(p[1]), float(p[2]), float(p[3]), float(M), float(a))
    except (ZeroDivisionError, ValueError, OverflowError):   # (the math module raises where numpy gives inf or NaN: on the ring, at the origin)
        return np.full((4, 4), np.nan), np.full((3, 4, 4), np.nan)
    f, k = v[0], np.array([1.0, v[1], v[2], v[3]])
    df = v[4:7]
    dk = np.zeros((3, 4))
    dk[:, 1:] = np.array(v[7:16]).reshape(3, 3)
    kk = np.outer(k, k)
    dg = np.empty((3, 4, 4))
    for j in range(3):
        o = np.outer(dk[j], k)
        dg[j] = df[j] * kk + f * (o + o.T)
    return ETA + f * kk, dg


def _metric(kind, M, a, p, dt):
    """g [4, 4] and dg [3, 4, 4] (d/dx, d/dy, d/dz) at p = (t, x, y, z), evaluated in dtype dt: float64 through _ks_parts, any other
    dtype through truth._metric_fn's lambdas on scalars of that dtype"""
    if dt is np.float64:
        return _metric64(kind, M, a, p)
    c = lambda v: dt(v)
    g, dg = T._metric_fn(kind)(c(p[1]), c(p[2]), c(p[3]), c(M), c(a))
    return g.astype(dt), dg.astype(dt)


def static_observer(g):
    t = np.linalg.inv(g)[:, 0]
    t2 = t @ g @ t
    return -t / np.sqrt(-t2), bool(t2 < 0)


def kappa0_of(scene, s0, u_obs=None, dt=np.float64):
    g0, _ = _metric(_kind(scene), scene.M, scene.a, s0[:4], dt)
    if u_obs is None:
        u_obs, _ = static_observer(g0)
    return dt(s0[4:].astype(dt) @ g0 @ u_obs.astype(dt))


def orbit_rate(kind, M, a, x, y, orbit, dt=np.float64):
    """(Omega, ok) of the equatorial circular orbit through (x, y, 0): the root `orbit` of C Omega² + 2 B Omega + A = 0"""
    g, dg = _metric(kind, M, a, (0.0, x, y, 0.0), dt)
    D = x * dg[0] + y * dg[1]
    gtp = x * g[0, 2] - y * g[0, 1]
    gpp = y * y * g[1, 1] - 2 * x * y * g[1, 2] + x * x * g[2, 2]
    A = D[0, 0]
    B = (x * D[0, 2] - y * D[0, 1]) + gtp
    C = (y * y * D[1, 1] - 2 * x * y * D[1, 2] + x * x * D[2, 2]) + 2 * gpp
    disc = B * B - A * C
    with np.errstate(all="ignore"):
        return (orbit * np.sqrt(disc) - B) / C, bool(disc >= 0 and C != 0)


def flow_point(scene, fl, kappa0, s, dt=np.float64):
    """-> dict(dens, omega, u_f, gfac, valid, dtau, dI0) at s = (x, k)"""
    kind, M, a = _kind(scene), scene.M, scene.a
    s = np.asarray(s, dt)
    x, y, z = s[1], s[2], s[3]
    f = {k: (dt(v) if k != "emitter" else v) for k, v in fl.items()}
    with np.errstate(all="ignore"):
        rho = np.hypot(x, y)
        r = np.sqrt(x * x + y * y + z * z)
        dens = (r / f["r0"]) ** (-f["alpha"]) * np.exp(-(z * z) / (dt(2) * f["H"] * f["H"] * rho * rho))
        if not np.isfinite(dens):
            dens = dt(0)
        if fl["emitter"] == KEPLER:
            om, ok = orbit_rate(kind, M, a, x, y, f["orbit"], dt)
        else:
            om, ok = f["orbit"], True
        g, _ = _metric(kind, M, a, s[:4], dt)
        xi = np.array([dt(1), -(om * y), om * x, dt(0)], dt)
        n2 = xi @ g @ xi
        ok = bool(ok and np.isfinite(om) and np.isfinite(n2) and n2 < 0)
        uf = xi / np.sqrt(-n2)
        w = s[4:] @ g @ uf
        gf = dt(kappa0) / w
        dtau = dI0 = dt(0)
        if ok and gf > 0:
            dtau = f["kappa"] * dens * w
            dI0 = f["j0"] * dens * w * gf ** (dt(3) + f["s"])
    return dict(dens=dens, omega=om, u_f=uf, gfac=gf, valid=ok, dtau=dtau, dI0=dI0)


def rhs10(scene, fl, kappa0, dt=np.float64):
    kind, M, a = _kind(scene), scene.M, scene.a

    def geo(y):   # truth.rhs(scene)'s lowered form on _metric's g and dg (tests/test_transfer.py holds the two against each other)
        g, dgs = _metric(kind, M, a, y[:4], dt)
        dg = np.zeros((4, 4, 4), dt)
        dg[1:] = dgs
        u = y[4:8]
        low = np.einsum("bac,b,c->a", dg, u, u) - dt(0.5) * np.einsum("abc,b,c->a", dg, u, u)
        return np.concatenate([u, -np.linalg.solve(g, low)])

    def f(_lam, y):
        y = np.asarray(y, dt)
        p = flow_point(scene, fl, kappa0, y[:8], dt)
        with np.errstate(all="ignore"):
            return np.concatenate([geo(y), [p["dtau"], p["dI0"] * np.exp(-y[8])]]).astype(dt)
    return f


def truth(scene, fl, s0, lam_end, lam0=0.0, u_obs=None, rtol=1e-13, atol=1e-15, max_step=0.05):
    """-> dict(I, tau, s_end, lam, stopped): DOP853 on (x, k, tau, I) over [lam0, lam_end]; ends earlier where r = r_stop (an event)"""
    from scipy.integrate import solve_ivp
    k0 = kappa0_of(scene, np.asarray(s0, np.float64), u_obs)
    ev = None
    if fl["r_stop"] > 0:
        ev = lambda lam, y: y[1] * y[1] + y[2] * y[2] + y[3] * y[3] - fl["r_stop"] ** 2
        ev.terminal, ev.direction = True, -1
    y0 = np.concatenate([np.asarray(s0, np.float64), [0.0, 0.0]])
    if not lam_end > lam0:
        return dict(I=0.0, tau=0.0, s_end=y0[:8], lam=lam0, stopped=False)
    sol = solve_ivp(rhs10(scene, fl, k0), (lam0, float(lam_end)), y0, method="DOP853", rtol=rtol, atol=atol, max_step=max_step, events=ev)
    assert sol.success, sol.message
    return dict(I=sol.y[9, -1], tau=sol.y[8, -1], s_end=sol.y[:8, -1], lam=sol.t[-1], stopped=sol.status == 1)


# ---- the twin: Tsit5 + PI on 10 components, as the header's contract states it -------------------------------------------------------------
A21 = 0.161
A3 = (-0.008480655492356989, 0.335480655492357)
A4 = (2.8971530571054935, -6.359448489975075, 4.3622954328695815)
A5 = (5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525)
A6 = (5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383)
A7 = (0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774)
BT = (-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552, -0.45808210592918697,
      0.015151515151515152)
ROWS = ((A21,), A3, A4, A5, A6, A7)


def _rms(v):
    return np.sqrt(np.mean(v * v, dtype=v.dtype))


def _initial_dt(f, y, f0, abstol, reltol, dtmax, dt):
    """Hairer's initial step on the geodesic part (8 components); one more evaluation of the right-hand side"""
    y8, f8 = y[:8], f0[:8]
    sk = dt(1) / (np.abs(y8) * reltol + abstol)
    d0, d1 = _rms(y8 * sk), _rms(f8 * sk)
    dt0 = dt(1e-6) if (d0 < 1e-5 or d1 < 1e-5) else (d0 / d1) * dt(0.01)
    dt0 = min(dt0, dtmax)
    f1 = f(0.0, np.concatenate([y8 + dt0 * f8, y[8:]]).astype(dt))[:8]
    d2 = _rms((f1 - f8) * sk) / dt0
    md = max(d1, d2)
    dt1 = max(dt(1e-6), dt0 * dt(1e-3)) if md <= 1e-15 else dt(10) ** (-(dt(2) + np.log10(md)) * dt(0.2))
    return dt(min(min(dt(100) * dt0, dt1), dtmax))


def twin(scene, fl, s0, lam_end, opt, u_obs=None, dt=np.float64):
    """opt: dict(reltol, abstol, lambda0, lambda1, max_steps).  -> dict(I, tau, s_end, status, steps)"""
    dt = np.dtype(dt).type
    reltol, abstol = dt(opt["reltol"]), dt(opt["abstol"])
    t, t1, dtmax = dt(opt["lambda0"]), dt(lam_end), dt(opt["lambda1"]) - dt(opt["lambda0"])
    y = np.concatenate([np.asarray(s0, dt), [dt(0), dt(0)]]).astype(dt)
    nan = dt(np.nan)
    if not (np.isfinite(y).all() and np.isfinite(t1)):
        return dict(I=nan, tau=nan, s_end=y[:8], status=3, steps=0)
    if not t < t1:
        return dict(I=dt(0), tau=dt(0), s_end=y[:8], status=0, steps=0)
    f = rhs10(scene, fl, kappa0_of(scene, np.asarray(s0, dt), u_obs, dt), dt)
    beta1, beta2, igamma, qmin_inv, qmax_inv, qoldinit = dt(0.14), dt(0.08), dt(1) / dt(0.9), dt(5), dt(0.1), dt(1e-4)
    rstop2 = dt(fl["r_stop"]) ** 2
    k = [f(0.0, y)] + [None] * 6
    h = _initial_dt(f, y, k[0], abstol, reltol, dtmax, dt)
    qold, nacc, nrej, status = qoldinit, 0, 0, 0
    with np.errstate(all="ignore"):
        while True:
            if not t < t1:
                status = 0
                break
            if nacc + nrej >= opt["max_steps"]:
                status = 2
                break
            last = not h < t1 - t
            h = min(h, t1 - t)
            for s_, row in enumerate(ROWS):
                acc = sum(dt(c) * k[l] for l, c in enumerate(row))
                k[s_ + 1] = f(0.0, (y + h * acc).astype(dt))
            yn = (y + h * sum(dt(c) * k[l] for l, c in enumerate(A7))).astype(dt)
            ut = h * sum(dt(c) * k[l] for l, c in enumerate(BT))
            res = ut / (np.maximum(np.abs(y), np.abs(yn)) * reltol + abstol)
            E = _rms(res.astype(dt))
            if not np.isfinite(E):
                status = 3
                break
            q11 = dt(0)
            if E == 0:
                q = qmax_inv
            else:
                q11 = E ** beta1
                q = max(qmax_inv, min(qmin_inv, q11 / qold ** beta2 * igamma))
            if E <= 1:
                nacc += 1
                qold = max(E, qoldinit)
                hnew = h / q
                t = t1 if last else dt(t + h)
                y, k[0] = yn, k[6]
                if y[1] * y[1] + y[2] * y[2] + y[3] * y[3] < rstop2:
                    status = 1
                    break
                h = min(dtmax, hnew)
                if t < t1 and not t + h > t:
                    status = 3
                    break
            else:
                nrej += 1
                h = h / min(qmin_inv, q11 * igamma)
                if not t + h > t:
                    status = 3
                    break
    good = status != 3 and np.isfinite(y[8]) and np.isfinite(y[9])
    return dict(I=y[9] if good else nan, tau=y[8] if good else nan, s_end=y[:8], status=status if good else 3, steps=nacc + nrej)


# ---- rays of a static observer ---------------------------------------------------------------------------------------------------------------
def camera_state(scene, pos, direction):
    """the start state of the ray a static observer at `pos` = (t, x, y, z) sends along the spatial `direction` (3-vector, any length):
    k_0 = (-e_0 + n) / sqrt 2, n the unit vector over `direction` orthogonal to e_0 — past-directed and null, as the library's rays are"""
    pos = np.asarray(pos, np.float64)
    g, _ = _metric(_kind(scene), scene.M, scene.a, pos, np.float64)
    e0, ok = static_observer(g)
    assert ok
    d = np.concatenate([[0.0], np.asarray(direction, np.float64)])
    n = d + (d @ g @ e0) * e0
    n = n / np.sqrt(n @ g @ n)
    k = (-e0 + n) / np.sqrt(2.0)
    assert abs(k @ g @ k) < 1e-13
    return np.concatenate([pos, k])


def escape_lambda(scene, s0, r_sky, lam1, r_capture):
    """(lambda at which the ray reaches r = r_sky, or None if it comes within r_capture first): the geodesic alone, DOP853"""
    from scipy.integrate import solve_ivp
    sky = lambda lam, s: s[1] * s[1] + s[2] * s[2] + s[3] * s[3] - r_sky ** 2
    sky.terminal, sky.direction = True, 1
    cap = lambda lam, s: s[1] * s[1] + s[2] * s[2] + s[3] * s[3] - r_capture ** 2
    cap.terminal, cap.direction = True, -1
    geo = rhs10(scene, flow_params(j0=0.0), 1.0)
    sol = solve_ivp(lambda lam, s: geo(lam, np.concatenate([s, [0.0, 0.0]]))[:8], (0.0, lam1), s0, method="DOP853", rtol=1e-13, atol=1e-15,
                    max_step=0.25, events=[sky, cap])
    if len(sol.t_events[0]):
        return float(sol.t_events[0][0])
    return None
