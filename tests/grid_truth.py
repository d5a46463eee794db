"""A field whose Catmull-Rom interpolant is the field itself, and its true geodesics — TEST-SIDE ONLY (like truth.py).

Catmull-Rom interpolation reproduces polynomials of degree <= 2 in each variable exactly (to rounding), with any spacing, origin
and number of samples, and also where the clamped outer cell extrapolates.  So a metric whose ten components are quadratic
polynomials in (x, y, z) — or (t, x, y, z) — sampled on ANY grid is, on the device, that polynomial everywhere, and the geodesics
of the polynomial are the true geodesics of what a grid kernel integrates: a smooth-field problem that truth.py's DOP853 solves to
rounding, so the grid traces can be held to test_truth.py's absolute bars.

One coefficient table defines the field: g_c = eta_c + sum_m coef[c, m] * monomial_m for the ten components c = tt tx ty tz xx xy
xz yy yz zz and the monomials MONOMIALS (the first ten for a stationary field).  From it come a sympy expression (differentiated
symbolically for the truth's right-hand side, d_t g included), a numpy evaluator (the grids' samples) and — through
oracle_lib.set_polynomial — the CPU oracle's metric.  The scenes, grids and pixels of the four fixtures
tests/golden/truth_grid_<name>.npz are described here as well; tests/golden/make_grid_truth.py writes them.
"""
import functools

import numpy as np

import truth

POLY_MARKER = 0x202   # rtgr_scene.user_metric of a kind-USER scene that means "the polynomial field" to the oracle (RTGR_ORACLE_POLY)
MONOMIALS = ("1", "x", "y", "z", "xx", "yy", "zz", "xy", "xz", "yz", "t", "tt", "tx", "ty", "tz")
UPPER = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]
ETA = np.array([-1.0, 0, 0, 0, 1, 0, 0, 1, 0, 1])
N_RAYS = 64
FRAME = (45, 35)      # the fixtures' pixels are pixels of a 45 x 35 frame; pixel (5 i + 2, 5 j + 2) is pixel (i, j) of SMALL_FRAME
SMALL_FRAME = (9, 7)
GUARD = 9.0           # box scenes have no sky: a true ray that has met nothing ends at this radius


def monomials(t, x, y, z):
    return [1 + 0 * x, x, y, z, x * x, y * y, z * z, x * y, x * z, y * z, t + 0 * x, t * t + 0 * x, t * x, t * y, t * z]


def field_table(dim):
    """(10, 15) coefficients.  g_tt = -(1 - 2 Phi) with Phi a tilted, anisotropic, off-centre well of depth 0.3; the other nine
    components from a seeded generator: constants <= 0.05, linear <= 0.01, quadratic <= 0.004.  dim = 4 adds the terms in t."""
    rng = np.random.default_rng(20261021)
    c = np.zeros((10, 15))
    c[:, 0] = rng.uniform(-0.05, 0.05, 10)
    c[:, 1:4] = rng.uniform(-0.01, 0.01, (10, 3))
    c[:, 4:10] = rng.uniform(-0.004, 0.004, (10, 6))
    #            1     x      y      z       xx     yy     zz     xy     xz    yz
    c[0, :10] = [-0.6, 0.010, 0.004, -0.008, 0.008, 0.005, 0.007, 0.004, 0.0, -0.003]
    if dim == 4:
        c[:, 10] = rng.uniform(-0.004, 0.004, 10)
        c[:, 11] = rng.uniform(-1e-4, 1e-4, 10)
        c[:, 12:15] = rng.uniform(-6e-4, 6e-4, (10, 3))
        c[0, 10:12] = [0.008, 2e-4]
    return c


def field_np(coef):
    """fn(t, x, y, z) -> (..., 10): the samples' source"""
    def fn(t, x, y, z):
        mon = monomials(t, x, y, z)
        return np.stack([ETA[c] + sum(coef[c, m] * mon[m] for m in range(15) if coef[c, m] != 0.0) for c in range(10)], axis=-1)
    return fn


def field_expr(coef):
    """((t, x, y, z), g): sympy symbols and the 4 x 4 matrix g_ab"""
    import sympy as sp
    t, x, y, z = sp.symbols("t x y z", real=True)
    mon = [sp.Integer(1), x, y, z, x * x, y * y, z * z, x * y, x * z, y * z, t, t * t, t * x, t * y, t * z]
    g = sp.zeros(4, 4)
    for c, (p, q) in enumerate(UPPER):
        g[p, q] = g[q, p] = sp.Float(float(ETA[c])) + sum(sp.Float(float(coef[c, m])) * mon[m] for m in range(15))
    return (t, x, y, z), g


@functools.lru_cache(maxsize=None)
def _field_fn(key):
    import sympy as sp
    coef = np.frombuffer(key, np.float64).reshape(10, 15)
    v, g = field_expr(coef)
    dg = [sp.diff(g, s) for s in v]                       # d_t g too
    fn = sp.lambdify(v, [g.tolist(), [d.tolist() for d in dg]], modules="numpy", cse=True)

    def call(pos):
        gg, dd = fn(pos[0], pos[1], pos[2], pos[3])
        return np.array(gg, dtype=np.float64), np.array(dd, dtype=np.float64)
    return call


def field_fn(coef):
    """fn(pos[4]) -> (g[4][4], dg[4][4][4]) with dg[b] = d_b g, b = t, x, y, z, from the SYMBOLIC derivative"""
    return _field_fn(np.ascontiguousarray(coef, np.float64).tobytes())


def metric_at(coef):
    fn = field_fn(coef)
    return lambda pos: fn(pos)[0]


def rhs(coef, stretch=None):
    """truth.rhs for the polynomial field, d_t g included.  `stretch` = (axis of (t, x, y, z), origin, factor): the field a grid
    loaded with that axis' spacing declared `factor` times too large represents, g'(x) = g(origin + (x - origin) / factor)."""
    fn = field_fn(coef)

    def f(_lam, s):
        pos = s[:4]
        if stretch is not None:
            pos = np.array(pos)
            pos[stretch[0]] = stretch[1] + (pos[stretch[0]] - stretch[1]) / stretch[2]
        g, dg = fn(pos)                                  # dg[b][a][c] = d_b g_ac
        if stretch is not None:
            dg[stretch[0]] /= stretch[2]
        u = s[4:]
        low = np.einsum("bac,b,c->a", dg, u, u) - 0.5 * np.einsum("abc,b,c->a", dg, u, u)
        return np.concatenate([u, -np.linalg.solve(g, low)])
    return f


def signature_range(coef, box, per_axis=9, radius=None):
    """over a lattice of the box ((t0, t1),)? (x0, x1), (y0, y1), (z0, z1) — `radius`: its points within that distance of the
    origin —: (min, max) of the lowest eigenvalue and (min, max) of the three others"""
    ax = [np.linspace(lo, hi, per_axis) for lo, hi in box]
    if len(box) == 3:
        ax = [np.zeros(1)] + ax
    t, x, y, z = np.meshgrid(*ax, indexing="ij")
    keep = np.ones(x.size, bool) if radius is None else (x * x + y * y + z * z).ravel() <= radius * radius
    g10 = field_np(coef)(t.ravel()[keep], x.ravel()[keep], y.ravel()[keep], z.ravel()[keep])
    g = np.zeros((g10.shape[0], 4, 4))
    for c, (p, q) in enumerate(UPPER):
        g[:, p, q] = g[:, q, p] = g10[:, c]
    ev = np.linalg.eigvalsh(g)
    return (ev[:, 0].min(), ev[:, 0].max()), (ev[:, 1:].min(), ev[:, 1:].max())


# ---- the four fixtures: grids, scenes, pixels ------------------------------------------------------------------------------------
# Spacings, origins and counts differ on every axis, and every number is a binary fraction: the camera's centre (0, 0, -2.75, 1.875)
# is a grid node exactly — x sample 15, y sample 10, z sample 14 of the lens grids, t sample 12 of the 4-D one — so the rays of the centre row and
# column start with an integer cell coordinate.  origin / spacing / n in the order (x, y, z), 4-D: (t, x, y, z).
GRIDS = {
    # valid box x [-7, 7], y [-6.6875, 6.875], z [-6.25, 6.25]: the whole sky sphere of radius 6
    "quad3": dict(dim=3, origin=(-7.5, -7.125, -6.875), spacing=(0.5, 0.4375, 0.625), n=(31, 34, 23)),
    # ... and t in [-8.25, 0.75]: every ray ends by the plane t = -6.85
    "quad4": dict(dim=4, origin=(-9.0, -7.5, -7.125, -6.875), spacing=(0.75, 0.5, 0.4375, 0.625), n=(15, 31, 34, 23)),
    # valid box x [-3.5, 2.5], y [-4.0625, 3.375], z [-2.5, 3.125]: smaller than the rays' reach, different on every axis
    "quad3_box": dict(dim=3, origin=(-4.0, -4.5, -3.125), spacing=(0.5, 0.4375, 0.625), n=(15, 20, 12)),
    # ... and t in [-3, 0.75]: the time range ends before the slower rays have left the spatial box
    "quad4_box": dict(dim=4, origin=(-3.75, -4.0, -4.5, -3.125), spacing=(0.75, 0.5, 0.4375, 0.625), n=(8, 15, 20, 12)),
}
NAMES = tuple(GRIDS)
LENS, BOX = ("quad3", "quad4"), ("quad3_box", "quad4_box")
CAMERA = dict(pos=(0, 0, -2.75, 1.875), widthx=(0, 3.0, 0, 0), widthy=(0, 0, 1.8, 2.4), normal=(0, 0, 2.4, -1.8))
PLANE_T = -6.85


def valid_box(grid):
    return tuple((o + h, o + (n - 2) * h) for o, h, n in zip(grid["origin"], grid["spacing"], grid["n"]))


def objects(name):
    """Object 2 is the plane in every scene, as in scenes.scene_variant: test_truth._check_against_truth holds the rays that end on
    object 2 to the captured-ray bars and all others to the sphere bar.  The box scenes have no sky, and every object lies strictly
    inside the valid box; their plane is at a time no ray reaches, so it never ends one."""
    from scenes import rt
    if name in LENS:
        return [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -6.0), rt.Plane(PLANE_T), rt.Sphere((0, 0.5, -1.5, 1.0), (1, 0, 0, 0), 0.9),
                rt.Disk(0.2, 1.2, 2.6)]
    return [rt.Sphere((0, 0.3, -0.9, 0.5), (1, 0, 0, 0), 0.9), rt.Plane(-1000.0), rt.Sphere((0, -0.9, -1.6, 1.3), (1, 0, 0, 0), 0.6),
            rt.Disk(0.2, 1.1, 2.2)]


def truth_scene(name, coef=None):
    """(scene, camera): kind USER with POLY_MARKER, which is the polynomial field to the oracle (after oracle_lib.set_polynomial)
    and means nothing to the library — nothing is compiled or loaded"""
    from scenes import rt
    sc = rt.make_scene(rt.minkowski, objects(name), units=False)
    sc.metric, sc.user_metric = rt._abi.USER, POLY_MARKER
    return sc, rt.make_camera(**CAMERA)


def pixels():
    """64 distinct pixels of FRAME, seeded: 16 that are also pixels of SMALL_FRAME (the centre pixel, which starts on a grid node,
    among them), then 48 others"""
    rng = np.random.default_rng(20261022)
    small = [(4, 3)] + [(int(k % 9), int(k // 9)) for k in rng.permutation(63) if (k % 9, k // 9) != (4, 3)][:15]
    ij = [(5 * i + 2, 5 * j + 2) for i, j in small]
    for k in rng.permutation(FRAME[0] * FRAME[1]):
        p = (int(k % FRAME[0]), int(k // FRAME[0]))
        if p not in ij and len(ij) < N_RAYS:
            ij.append(p)
    return np.array(ij, dtype=np.int64)


def samples(grid, coef):
    """the grid's samples, rebuilt from the coefficients: (nz, ny, nx, 10) or (nt, nz, ny, nx, 10)"""
    ax = [o + h * np.arange(n) for o, h, n in zip(grid["origin"], grid["spacing"], grid["n"])]
    if grid["dim"] == 3:
        z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        return field_np(coef)(0.0 * x, x, y, z)
    t, z, y, x = np.meshgrid(ax[0], ax[3], ax[2], ax[1], indexing="ij")
    return field_np(coef)(t, x, y, z)


def trace_truth(name, coef, s0, rtol=1e-13, atol=1e-15, stretch=None, lambda1=None):
    """truth.trace_ray through the polynomial field in the scene of fixture `name`.  lambda1: integrate to that λ with no events
    (the state of the true geodesic there)."""
    from scenes import rt
    opt = rt.solver_defaults()
    sc, _ = truth_scene(name)
    if lambda1 is not None:
        opt.lambda1 = lambda1
        sc.nobj = 0
        return truth.trace_ray(sc, opt, s0, rtol=rtol, atol=atol, rhs_fn=rhs(coef, stretch))
    box = valid_box(GRIDS[name])
    return truth.trace_ray(sc, opt, s0, rtol=rtol, atol=atol, rhs_fn=rhs(coef, stretch), box=box, guard=None if name in LENS else GUARD)
