"""An independent, much-tighter solution of the same physics — TEST-SIDE ONLY (like oracle/, never imported by the product).

Why it exists.  The oracle restates OrdinaryDiffEq's Tsit5 + PI controller + ContinuousCallback from their published
algorithms, and the only artefacts of the reference that pin it are two 8-bit images: everything below
1/255 would otherwise be HIP-vs-oracle only.  This module removes the shared assumptions: it knows nothing of Tsit5,
dual numbers, the closed contraction or the event machinery —

  * the metric is typed as a sympy expression (same formulas as `kerr_schild`, src/RayTraceGR.jl:283-291, and the
    textbook radius), its derivative is SYMBOLIC (`sympy.diff`), both are lambdified;
  * the geodesic equation (:358-370) is evaluated from them with a linear solve (no Christoffel symbols, no inverse);
  * the integrator is scipy's DOP853 (8th order) at rtol 1e-13 / atol 1e-15 — three to four orders tighter than the
    path's own tolerance 2⁻³⁹ ≈ 1.8·10⁻¹² — with its own dense-output root finder for the object events;
  * `make_canvas` (:457-478) and the colouring rule (:513-533, :402-404, :420-428) are restated in numpy.

So `|x_oracle − x_truth|` and `|x_hip − x_truth|` measure each path's GLOBAL integration error.  The reference (same
method, same tolerances) has a global error of the same size, which is what turns "within 1e-6 RGB of the Julia reference"
(BASELINE.json north_star) from an untestable statement into a bounded one: two solutions that are each within ε of the
true geodesic are within 2ε of each other, whatever the controller details.
"""
import functools

import numpy as np

KERR_BL_MARKER = 0x300   # rtgr_scene.user_metric of a test scene that means "the Boyer–Lindquist example" to this module


def metric_expr(kind):
    """kind: 'mink' | 'ks_ref' (r as written, :284) | 'ks_true' (textbook r) | 'schw_iso' (the user-metric example; a scene
    of kind RTGR_USER is taken to be that one) | 'kerr_bl'.  Returns ((x, y, z, M, a), g): the sympy symbols and the 4x4 matrix
    g_ab — the ONE place the formulas are typed (the double-precision lambdas below and the 50-digit reference of
    golden/make_rhs_edges.py are both made from it)."""
    import sympy as sp
    x, y, z, M, a = sp.symbols("x y z M a", real=True)
    eta = sp.diag(-1, 1, 1, 1)
    if kind == "mink":
        g = eta
    elif kind == "schw_iso":   # Schwarzschild in isotropic coordinates (examples/user_metrics.py: a run-time compiled metric)
        m = M / (2 * sp.sqrt(x * x + y * y + z * z))
        g = sp.diag(-((1 - m) / (1 + m)) ** 2, (1 + m) ** 4, (1 + m) ** 4, (1 + m) ** 4) + 0 * a * eta
    elif kind == "kerr_bl":    # Kerr in Boyer–Lindquist coordinates on the plain spherical map (examples/user_metrics.py
        # KERR_BOYER_LINDQUIST); written here WITHOUT inverse trigonometric functions: cosθ = z/r, sinθ = ϖ/r, …
        r = sp.sqrt(x * x + y * y + z * z)
        pw = sp.sqrt(x * x + y * y)
        ct, st, cp, sphi = z / r, pw / r, x / pw, y / pw
        Sig = r * r + a * a * ct * ct
        Del = r * r - 2 * M * r + a * a
        w = 2 * M * r / Sig
        gBL = {"tt": w - 1, "tp": -a * w * st ** 2, "rr": Sig / Del, "hh": Sig, "pp": (r * r + a * a + a * a * w * st ** 2) * st ** 2}
        dr = sp.Matrix([0, st * cp, st * sphi, ct])
        dth = sp.Matrix([0, ct * cp / r, ct * sphi / r, -st / r])
        dph = sp.Matrix([0, -sphi / (r * st), cp / (r * st), 0])
        dt = sp.Matrix([1, 0, 0, 0])
        g = (gBL["tt"] * dt * dt.T + gBL["tp"] * (dt * dph.T + dph * dt.T) + gBL["rr"] * dr * dr.T + gBL["hh"] * dth * dth.T
             + gBL["pp"] * dph * dph.T)
    else:
        rho2 = x * x + y * y + z * z
        q = rho2 - a * a
        if kind == "ks_ref":
            r = sp.sqrt(q) / 2 + sp.sqrt(a * a * z * z + (q / 2) ** 2)
        else:
            r = sp.sqrt((q + sp.sqrt(q * q + 4 * a * a * z * z)) / 2)
        f = 2 * M * r ** 3 / (r ** 4 + a * a * z * z)
        k = sp.Matrix([1, (r * x + a * y) / (r * r + a * a), (r * y - a * x) / (r * r + a * a), z / r])
        g = eta + f * k * k.T
    return (x, y, z, M, a), g


@functools.lru_cache(maxsize=None)
def _metric_fn(kind):
    """Returns f(x, y, z, M, a) -> (g[4][4], dg[3][4][4]) of metric_expr(kind) in double precision, with dg[j] = ∂g/∂x_j,
    j = x,y,z (every metric here is stationary: ∂_t g = 0)."""
    import sympy as sp
    (x, y, z, M, a), g = metric_expr(kind)
    dg = [sp.diff(g, v) for v in (x, y, z)]
    fn = sp.lambdify((x, y, z, M, a), [g.tolist(), [d.tolist() for d in dg]], modules="numpy", cse=True)

    def call(px, py, pz, m, sa):
        gg, dd = fn(px, py, pz, m, sa)
        return np.array(gg, dtype=np.float64), np.array(dd, dtype=np.float64)
    return call


def _kind(scene):
    from conftest import load_package
    abi = load_package()._abi
    k = scene.metric & ~abi.METRIC_GENERIC
    if k == abi.USER and scene.user_metric == KERR_BL_MARKER:
        return "kerr_bl"
    return {abi.MINKOWSKI: "mink", abi.KS_REF: "ks_ref", abi.KS_TRUE: "ks_true", abi.USER: "schw_iso"}[k]


def metric(scene, pos):
    return _metric_fn(_kind(scene))(pos[1], pos[2], pos[3], scene.M, scene.a)[0]


def rhs(scene):
    """s = (x^a, u^a) -> (u^a, u̇^a),  g_ad u̇^d = −(∂_b g_ac − ½ ∂_a g_bc) u^b u^c  (the lowered form of :358-370)."""
    fn, M, a = _metric_fn(_kind(scene)), scene.M, scene.a

    def f(_lam, s):
        g, dgs = fn(s[1], s[2], s[3], M, a)
        dg = np.zeros((4, 4, 4))        # dg[b][a][c] = ∂_b g_ac
        dg[1:] = dgs
        u = s[4:]
        low = np.einsum("bac,b,c->a", dg, u, u) - 0.5 * np.einsum("abc,b,c->a", dg, u, u)
        return np.concatenate([u, -np.linalg.solve(g, low)])
    return f


def object_distance(o, pos):
    """distance(obj, pos): Plane :399-401, Sphere :415-419 (signed by the radius' sign), Disk (no reference)."""
    from conftest import load_package
    abi = load_package()._abi
    p = o.p
    if o.kind == abi.PLANE:
        return pos[0] - p[0]
    if o.kind == abi.SPHERE:
        d2 = sum((pos[i] - p[i]) ** 2 for i in (1, 2, 3))
        return np.sign(p[8]) * (d2 - p[8] ** 2)
    if o.kind == abi.USER_OBJECT:      # the two Object subtypes of examples/user_objects.py, restated from their DEFINITION
        c = np.array([pos[1] - p[0], pos[2] - p[1], pos[3] - p[2]])
        if o.type == 0:                # torus around z: squared distance from the circle of radius p[3], minus the tube radius squared
            return (np.hypot(c[0], c[1]) - p[3]) ** 2 + c[2] ** 2 - p[4] ** 2
        return float(np.sum((c / np.array([p[3], p[4], p[5]])) ** 2) - 1.0)
    rc = np.hypot(pos[1], pos[2])
    return max(abs(pos[3]) - p[0], p[1] - rc, rc - p[2])


def object_colour(o, pos):
    from conftest import load_package
    abi = load_package()._abi
    if o.kind == abi.PLANE:
        return np.array([0.0, 0.5, 0.0])
    if o.kind == abi.SPHERE:
        d = np.array([pos[i] - o.p[i] for i in (1, 2, 3)])
        th = np.arccos(d[2] / np.linalg.norm(d))
        ph = np.arctan2(d[1], d[0])
        return np.array([np.mod(12 * th / np.pi, 1.0), np.mod(12 * ph / np.pi, 1.0), 1.0])
    if o.kind == abi.USER_OBJECT:
        p = o.p
        c = np.array([pos[1] - p[0], pos[2] - p[1], pos[3] - p[2]])
        if o.type == 0:
            w = np.hypot(c[0], c[1]) - p[3]
            return np.array([np.mod(6 * np.arctan2(c[1], c[0]) / np.pi, 1.0), np.mod(6 * np.arctan2(c[2], w) / np.pi, 1.0), 0.5])
        q = c / np.array([p[3], p[4], p[5]])
        return np.array([np.mod(12 * np.arccos(q[2] / np.linalg.norm(q)) / np.pi, 1.0), 0.5, np.mod(12 * np.arctan2(q[1], q[0]) / np.pi, 1.0)])
    rc = np.hypot(pos[1], pos[2])
    return np.array([1.0, np.mod(rc, 1.0), np.mod(12 * np.arctan2(pos[2], pos[1]) / np.pi, 1.0)])


def pixel_state(scene, cam, ni, nj, i, j, metric_fn=None):
    """make_canvas for pixel (i, j), 0-based (:463-476).  `metric_fn(pos) -> g[4][4]`: a field other than the scene's own
    (tests/grid_truth.py)."""
    dx = (i + 0.5) / ni - 0.5
    dy = (j + 0.5) / nj - 0.5
    pos = np.array(cam.pos) + dx * np.array(cam.widthx) + dy * np.array(cam.widthy)
    n = np.array(cam.normal) + dx * np.array(cam.widthx) + dy * np.array(cam.widthy)
    g = metric(scene, pos) if metric_fn is None else metric_fn(pos)
    t = np.linalg.solve(g, np.array([1.0, 0, 0, 0]))
    u = (t / np.sqrt(-t @ g @ t) + n / np.sqrt(n @ g @ n)) / np.sqrt(2.0)
    return np.concatenate([pos, u])


def box_margin(box, pos):
    """> 0 inside `box`, < 0 outside: the smallest distance of pos[a] to the two faces of its axis.  box[a] = (lo, hi) for
    the axes (x, y, z), or (t, x, y, z) for a box with a time range."""
    first = 4 - len(box)
    return min(min(pos[first + a] - lo, hi - pos[first + a]) for a, (lo, hi) in enumerate(box))


def trace_ray(scene, opt, s0, rtol=1e-13, atol=1e-15, max_step=0.2, rhs_fn=None, box=None, guard=None):
    """-> dict(state_end, lambda_end, hit (1-based object, 0 = nothing), rgb, nfev, clearance, lambda_exit, state_exit).

    `rhs_fn`: the right-hand side of another field than the scene's metric (tests/grid_truth.py: a polynomial, ∂_t g included).
    `box`: the first λ at which the ray leaves it is recorded as lambda_exit (inf: never) by an event that is NOT terminal —
    the ray goes on, so that an object met after leaving is seen as well.  `guard`: a radius at which a ray that has met
    nothing ends (a scene without a sky: the field need not be a spacetime at any distance); not an object, hit = 0.

    `max_step`: scipy looks for an event only between the END POINTS of its steps, and an 8th-order method crosses flat
    space in a handful of them; 0.2 (objects here are ≥ 0.5 across, |ẋ| ≈ 1) keeps a chord from being stepped over.

    `clearance`: the smallest |distance| to any object OTHER than the one hit, over the whole ray, relative to that
    object's size scale — rays with a tiny clearance graze an object, and whether the reference's sampled sign test sees
    the graze is decided by where its steps happen to fall; callers exclude them from tolerance statistics."""
    from scipy.integrate import solve_ivp
    objs = [scene.obj[k] for k in range(scene.nobj)]
    events = []
    for o in objs:
        ev = (lambda o: lambda lam, s: object_distance(o, s))(o)
        ev.terminal = True
        events.append(ev)
    if guard is not None:
        ev = lambda lam, s: guard * guard - s[1] * s[1] - s[2] * s[2] - s[3] * s[3]
        ev.terminal = True
        events.append(ev)
    if box is not None:
        ev = lambda lam, s: box_margin(box, s)
        ev.terminal, ev.direction = False, -1
        events.append(ev)
    sol = solve_ivp(rhs_fn or rhs(scene), (opt.lambda0, opt.lambda1), s0, method="DOP853", rtol=rtol, atol=atol, events=events,
                    dense_output=True, max_step=max_step)
    lam_exit, s_exit = np.inf, np.full(8, np.nan)
    if box is not None:
        if box_margin(box, s0) < 0:
            lam_exit, s_exit = opt.lambda0, np.array(s0)
        elif len(sol.t_events[-1]):
            lam_exit, s_exit = sol.t_events[-1][0], sol.y_events[-1][0]
    hit_events = [k for k, te in enumerate(sol.t_events[:len(objs) + (guard is not None)]) if len(te)]
    if hit_events:
        k = hit_events[0]
        lam_end, s_end = sol.t_events[k][0], sol.y_events[k][0]
    else:
        lam_end, s_end = sol.t[-1], sol.y[:, -1]
    # colouring rule (:518-530): the object of smallest signed distance below the threshold
    omin, dmin = 0, opt.hit_threshold
    for k, o in enumerate(objs):
        d = object_distance(o, s_end)
        if d < dmin:
            omin, dmin = k + 1, d
    rgb = np.array(opt.miss_rgb[:]) if omin == 0 else object_colour(objs[omin - 1], s_end) * omin / len(objs)
    lam = np.linspace(opt.lambda0, lam_end, 400)
    path = sol.sol(lam)
    clearance = np.inf
    for k, o in enumerate(objs):
        if k + 1 == omin:
            continue
        clearance = min(clearance, min(abs(object_distance(o, path[:, m])) for m in range(path.shape[1])))
    return dict(state_end=s_end, lambda_end=lam_end, hit=omin, rgb=rgb, nfev=sol.nfev, clearance=clearance, lambda_exit=lam_exit,
                state_exit=s_exit)
