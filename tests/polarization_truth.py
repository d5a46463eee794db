"""The truth side of tests/test_polarization.py (include/rtgr.h "polarized disk images"), in numpy / scipy, double precision:

  * transport(...)      a null geodesic and a vector f parallel-transported along it, integrated together by DOP853 with Christoffel
                        symbols from truth._metric_fn's symbolic g and dg;
  * forms / kappa       the numpy restatement of the Killing-Yano form Y and its dual h in Kerr-Schild coordinates, and the two
                        Walker-Penrose constants kappa_1 = Y(k, f), kappa_2 = h(k, f);
  * screen_basis / camera_solve   the observer-side 2 x 2 solve;
  * emitter / model     the emitter's triad, the two emission laws, and the whole chain of one pixel.

Nothing here knows the device code: the formulas are typed from the header's contract."""
import numpy as np

import truth

EPS = 2.220446049250313e-16
TOL = 4096 * EPS


def metric_fn(kind):
    return truth._metric_fn(kind)


def g_at(kind, x, M, a):
    return metric_fn(kind)(x[1], x[2], x[3], M, a)[0]


def christoffel(kind, x, M, a):
    """Gamma[a][b][c] = Gamma^a_bc at x, from the symbolic g and dg."""
    g, dgs = metric_fn(kind)(x[1], x[2], x[3], M, a)
    dg = np.zeros((4, 4, 4))      # dg[b][a][c] = d_b g_ac
    dg[1:] = dgs
    low = 0.5 * (np.einsum("bac->abc", dg) + np.einsum("cab->abc", dg) - dg)   # Gamma_abc
    return np.linalg.solve(g, low.reshape(4, 16)).reshape(4, 4, 4)


def transport(kind, M, a, x0, k0, f0, lam1, rtol=1e-12, atol=1e-14, max_step=0.25):
    """(x, k, f) from affine parameter 0 to lam1 (either sign): dx = k, dk = -Gamma(k, k), df = -Gamma(k, f).  Returns the 12-vector at
    lam1 and the smallest Kerr radius met; the integration stops where the ray comes within 1.05 r_+ (the caller replaces such a ray)."""
    from scipy.integrate import solve_ivp

    rmin = [np.inf]
    r_stop = 1.05 * (M + np.sqrt(max(M * M - a * a, 0.0))) if kind != "mink" else 1e-3

    def near(_lam, s):
        return kerr_radius(s[:4], a) - r_stop
    near.terminal = True

    def rhs(_lam, s):
        G = christoffel(kind, s[:4], M, a)
        k, f = s[4:8], s[8:12]
        return np.concatenate([k, -np.einsum("abc,b,c->a", G, k, k), -np.einsum("abc,b,c->a", G, k, f)])

    s0 = np.concatenate([x0, k0, f0]).astype(np.float64)
    sol = solve_ivp(rhs, (0.0, float(lam1)), s0, method="DOP853", rtol=rtol, atol=atol, max_step=max_step, events=near)
    assert sol.success, sol.message
    rmin[0] = min(kerr_radius(sol.y[:4, i], a) for i in range(sol.y.shape[1]))
    return sol.y[:, -1], rmin[0]


def kerr_radius(x, a):
    q = x[1] ** 2 + x[2] ** 2 + x[3] ** 2 - a * a
    return np.sqrt(0.5 * (q + np.sqrt(q * q + 4 * a * a * x[3] ** 2)))


def forms(x, a):
    """(dr, w1, dc, w2, r, c) at x: covectors on (dt, dx, dy, dz); None where the point is on the axis."""
    X, Y, Z = x[1], x[2], x[3]
    q = X * X + Y * Y + Z * Z - a * a
    r2 = 0.5 * (q + np.sqrt(q * q + 4 * a * a * Z * Z))
    r = np.sqrt(r2)
    dr = np.array([0.0, 2 * r2 * X, 2 * r2 * Y, 2 * r2 * Z + 2 * a * a * Z]) / (4 * r2 * r - 2 * q * r)
    c = Z / r
    dc = np.array([0.0, 0.0, 0.0, 1.0 / r]) - (Z / r2) * dr
    s2 = 1.0 - c * c
    pw2 = X * X + Y * Y
    ra = r2 + a * a
    if pw2 <= TOL * ra:
        return None
    A = np.array([0.0, -Y, X, 0.0])                       # x dy - y dx
    dt = np.array([1.0, 0.0, 0.0, 0.0])
    w1 = dt - a * (A / ra + a * s2 * dr / ra)
    w2 = ra * A / pw2 - a * dt          # (r^2 + a^2) dphi~ - a dt - a dr: the a dr of dphi~ cancels
    return dr, w1, dc, w2, r, c


def kappa(x, k, f, a):
    """(kappa_1, kappa_2) = (Y_ab k^a f^b, h_ab k^a f^b);  Y = -a c dr^w1 + r dc^w2,  h = -r dr^w1 - a c dc^w2."""
    F = forms(x, a)
    if F is None:
        return np.array([np.nan, np.nan])
    dr, w1, dc, w2, r, c = F
    A = (dr @ k) * (w1 @ f) - (dr @ f) * (w1 @ k)         # (dr ^ w1)(k, f)
    B = (dc @ k) * (w2 @ f) - (dc @ f) * (w2 @ k)         # (dc ^ w2)(k, f)
    return np.array([-a * c * A + r * B, -r * A - a * c * B])


def inner(g, v, w):
    return float(v @ g @ w)


def normalise(g, v):
    return v / np.sqrt(inner(g, v, v))


def cross(g, u, v, w):
    """cross(v, w)_a = -sqrt(-det g) eps_abcd u^b v^c w^d (eps_0123 = +1), raised with g^{-1}."""
    lo = np.zeros(4)
    m = np.array([u, v, w])
    for i in range(4):
        cols = [j for j in range(4) if j != i]
        lo[i] = (-1) ** i * np.linalg.det(m[:, cols])
    lo *= -np.sqrt(-np.linalg.det(g))
    return np.linalg.solve(g, lo)


def screen_basis(g0, frame, k0):
    """(n, e^_x, e^_y) at the camera from the frame record (rows e_0, e_right, e_up, e_look) and the ray's k_0."""
    e0, er, eu = frame[0], frame[1], frame[2]
    n = np.sqrt(2.0) * k0 + e0
    ey = normalise(g0, eu - inner(g0, eu, n) * n)
    ex = normalise(g0, er - inner(g0, er, n) * n - inner(g0, er, ey) * ey)
    return n, ex, ey


def camera_solve(x0, k0, a, ex, ey, kap):
    """(alpha, beta, matrix): kappa = matrix (alpha, beta)."""
    kx, ky = kappa(x0, k0, ex, a), kappa(x0, k0, ey, a)
    Mx = np.array([[kx[0], ky[0]], [kx[1], ky[1]]])
    al, be = np.linalg.solve(Mx, kap)
    return al, be, Mx


def orbit_rate(kind, M, a, x, y, orbit):
    g, dgs = metric_fn(kind)(x, y, 0.0, M, a)
    D = x * dgs[0] + y * dgs[1]
    gtp = x * g[0][2] - y * g[0][1]
    gpp = y * y * g[1][1] - 2 * x * y * g[1][2] + x * x * g[2][2]
    A = D[0][0]
    B = (x * D[0][2] - y * D[0][1]) + gtp
    C = (y * y * D[1][1] - 2 * x * y * D[1][2] + x * x * D[2][2]) + 2 * gpp
    return (orbit * np.sqrt(B * B - A * C) - B) / C


def emitter(kind, M, a, se, emitter_kind, orbit, law, deg0, deg1, field):
    """The emitter side at the end state se = (x_end, k_end): dict with u, f_em, aux, delta, kappa, valid."""
    x, k = se[:4], se[4:]
    g = g_at(kind, x, M, a)
    Om = orbit_rate(kind, M, a, x[1], x[2], orbit) if emitter_kind == 0 else orbit
    xi = np.array([1.0, -Om * x[2], Om * x[1], 0.0])
    u = xi / np.sqrt(-inner(g, xi, xi))
    dz = np.array([0.0, 0.0, 0.0, 1.0])
    ez = normalise(g, dz + inner(g, dz, u) * u)
    pw = np.hypot(x[1], x[2])
    v = np.array([0.0, x[1], x[2], 0.0]) / pw
    v = v + inner(g, v, u) * u
    v = v - inner(g, v, ez) * ez
    erho = normalise(g, v)
    ephi = cross(g, u, ez, erho)
    p = k + inner(g, k, u) * u
    ph = p / np.sqrt(inner(g, p, p))
    if law == 0:
        w = cross(g, u, ph, ez)
        mu = abs(inner(g, ph, ez))
        delta = deg0 * (1 - mu) / (1 + deg1 * mu)
        aux = mu
    else:
        B = field[0] * erho + field[1] * ephi + field[2] * ez
        B = normalise(g, B)
        w = cross(g, u, ph, B)
        delta = deg0
        aux = None
    n2 = inner(g, w, w)
    if law == 1:
        aux = np.sqrt(n2)
    valid = n2 > TOL
    f = w / np.sqrt(n2)
    return dict(u=u, f_em=f, aux=aux, delta=delta, kappa=kappa(x, k, f, a), valid=valid, g=g, ez=ez, erho=erho, ephi=ephi, phat=ph)


def model(kind, M, a, s0, se, frame, emitter_kind, orbit, law, deg0, deg1, field):
    """One pixel by Walker-Penrose: the emitter side, then the camera-side solve.  Returns the emitter's dict plus q, u, alpha, beta."""
    E = emitter(kind, M, a, se, emitter_kind, orbit, law, deg0, deg1, field)
    g0 = g_at(kind, s0[:4], M, a)
    _, ex, ey = screen_basis(g0, frame, s0[4:])
    al, be, Mx = camera_solve(s0[:4], s0[4:], a, ex, ey, E["kappa"])
    d = al * al + be * be
    E.update(alpha=al, beta=be, q=E["delta"] * (al * al - be * be) / d, uu=2 * E["delta"] * al * be / d, matrix=Mx, ex=ex, ey=ey)
    return E


def random_ray(seed, kind, M, a):
    """A seeded ray for the conservation tests: x_0 at coordinate radius in [5, 8], k_0 = (-u + n)/sqrt(2) null and past-directed (u the
    static observer, n a random unit direction of its rest space), f_0 a random unit vector orthogonal to u and n — so g(k_0, f_0) = 0."""
    rng = np.random.default_rng(seed)
    rad, ct, ph = rng.uniform(5.0, 8.0), rng.uniform(-0.9, 0.9), rng.uniform(0.0, 2 * np.pi)
    st = np.sqrt(1 - ct * ct)
    x = np.array([0.0, rad * st * np.cos(ph), rad * st * np.sin(ph), rad * ct])
    g = g_at(kind, x, M, a)
    u = np.array([1.0, 0.0, 0.0, 0.0]) / np.sqrt(-g[0][0])
    n = np.concatenate([[0.0], rng.normal(size=3)])
    n = normalise(g, n + inner(g, n, u) * u)
    f = np.concatenate([[0.0], rng.normal(size=3)])
    f = f + inner(g, f, u) * u
    f = normalise(g, f - inner(g, f, n) * n)
    return x, (n - u) / np.sqrt(2.0), f
