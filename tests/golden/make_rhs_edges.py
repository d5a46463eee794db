#!/usr/bin/env python3
"""Generates tests/golden/rhs_edges.npz: the geodesic right-hand side u̇, the metric g, its derivative ∂g and the Christoffel
symbols Γ at the EDGES of the Kerr–Schild coordinates, evaluated in 50 digits, for tests/test_rhs_edges.py.  TEST-SIDE ONLY.

The reference.  tests/truth.py types the metric as a sympy expression (truth.metric_expr).  Here that expression and its
SYMBOLIC derivatives are lambdified with modules="mpmath" and evaluated at mp.dps = 50; Γ is ½ g⁻¹(∂g + ∂g − ∂g) with a
50-digit inverse, and u̇ solves the lowered equation g_ad u̇^d = −(∂_b g_ac − ½ ∂_a g_bc) u^b u^c (no formula is restated).
Inputs are the stored doubles (or floats), converted exactly.  Every Float64 reference value is stored as hi (the nearest
double) + lo (the remainder, kept as a float: 53 + 24 bits, so that errors far below 1e-16 stay measurable); the Float32
references — whose bars sit at 1e-5 … 1e-3 — as the nearest double.

Next to each Float64 reference: the error of the oracle's own double arithmetic at that state (oracle_lib.geodesic,
oracle_lib.eval_metric), measured as the tests measure the device (rel_err below).  The Float64 bars of the tests are
multiples of THAT — they never come from what the device gives.

Variants (VARIANTS): the six of test_gpu_parity.METRICS, then a nearly absent spin, a negative one, the extremal one and the
whole problem scaled by 2^∓10.  Families (FAMILIES), 32 states each, positions in units of M; t and u are seeded normals:

  axis      x = y = 0 exactly, z = ±{2.5, 7, 40} M
  equator   z = 0 exactly, cylindrical radius {2.5, 6, 30} M, eleven azimuths
  coord     (±ρ, 0, 0) and (0, ±ρ, 0), ρ = {2.5, 6, 30} M
  tiny_z    |z| = {1e-12, 1e-150, 1e-300, 5e-324} at cylindrical radius 3 M        (Float32: {1e-12, 1e-30, 1e-45})
  tiny_xy   x = −y of the same sizes at z = ±3 M
  horizon   points of the Kerr–Schild spheroids r = r₊(1 ± 1e-6) and r₊(1 + 1e-2), r₊ = M + sqrt(M² − a²), polar angles
            {0.2, 1.0, 1.5}
  far       |x| = {1e2, 1e3, 1e4, 1e6} M in seeded directions                       (Float32: {1e2, 1e3, 1e4})
  null      positions taken in turn from the seven families above; u null and past-directed as make_canvas builds it
            (src/RayTraceGR.jl:466-476) from the seeded spatial direction

The tensors g, ∂g, Γ (80 independent components, two words each) are stored for the first N_TENSOR states of every family —
those walk through every distinct position class of the family — so that the file stays below the size limit for committed
files; u̇ is stored for all 32.

The traced edge (TRACE_SCENES): 64 rays per scene with z = u^z = 0 exactly (48) or x = y = u^x = u^y = 0 exactly (16), half
aimed past the hole and half into it, chosen HERE, on the CPU, such that the oracle's frame shows the hit class of the true
geodesic (truth.trace_ray) and ends within 3e-11 of it; the truth's end states are stored.

    python tests/golden/make_rhs_edges.py            # ≈ 5 min on 8 cores
"""
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
OUT = os.path.join(HERE, "rhs_edges.npz")

#            name          (truth kind, M, a)
VARIANTS = {"ks_ref0": ("ks_ref", 1.0, 0.0), "ks_ref08": ("ks_ref", 1.0, 0.8), "ks_true0": ("ks_true", 1.0, 0.0),
            "ks_true08": ("ks_true", 1.0, 0.8), "ks_true0998": ("ks_true", 1.2, 0.998), "tiny_spin": ("ks_true", 1.0, 1e-9),
            "neg_spin": ("ks_true", 1.0, -0.8), "extremal": ("ks_true", 1.0, 1.0),
            "scaled_down": ("ks_true", 2.0 ** -10, 0.8 * 2.0 ** -10), "scaled_up": ("ks_true", 2.0 ** 10, 0.8 * 2.0 ** 10)}
FAMILIES = ["axis", "equator", "coord", "tiny_z", "tiny_xy", "horizon", "far", "null"]
N = 32           # states per family and variant
N_TENSOR = 4     # … of which the first N_TENSOR carry g, ∂g, Γ
SEED = 20261019
TINY = {np.float64: [1e-12, 1e-150, 1e-300, 5e-324], np.float32: [1e-12, 1e-30, 1e-45]}
FAR = {np.float64: [1e2, 1e3, 1e4, 1e6], np.float32: [1e2, 1e3, 1e4]}
SYM = [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]   # packed symmetric pairs
TRACE_SCENES = ["ks_true08", "ks_ref0"]
TRUTH_TOL = 3e-11
# A past-directed ray aimed into the hole never crosses the horizon of these ingoing coordinates: it hovers above it, neighbouring
# geodesics separating exponentially, until the far plane t = −20 ends it.  Started at t = −14 it meets the plane while still
# falling, and its end state is as well conditioned as an escaping ray's.
T_START = {0: 0.0, 1: -14.0, 2: 0.0, 3: -14.0}


def metric_params(name, dtype):
    """(kind, M, a) as the device sees them: a Float32 scene holds M and a rounded to float"""
    kind, M, a = VARIANTS[name]
    return kind, float(dtype(M)), float(dtype(a))


# ---- states ---------------------------------------------------------------------------------------------------------
def _positions(family, M, a, dtype, rng):
    k = np.arange(N)
    P = np.zeros((N, 3))
    tiny, far = np.array(TINY[dtype]), np.array(FAR[dtype])
    sign = np.array([1.0, -1.0])
    phi = 0.37 + k * 2 * np.pi / 11
    if family == "axis":
        P[:, 2] = np.array([2.5, -2.5, 7, -7, 40, -40])[k % 6] * M
    elif family == "equator":
        R = np.array([2.5, 6, 30])[k % 3] * M
        P[:, 0], P[:, 1] = R * np.cos(phi), R * np.sin(phi)
    elif family == "coord":
        rho = np.array([2.5, 6, 30])[(k // 4) % 3] * M
        d = np.array([(1, 0), (-1, 0), (0, 1), (0, -1)], float)[k % 4]
        P[:, 0], P[:, 1] = rho * d[:, 0], rho * d[:, 1]
    elif family == "tiny_z":
        P[:, 0], P[:, 1] = 3 * M * np.cos(phi), 3 * M * np.sin(phi)
        P[:, 2] = tiny[k % len(tiny)] * sign[(k // len(tiny)) % 2]
    elif family == "tiny_xy":
        e = tiny[k % len(tiny)] * sign[(k // len(tiny)) % 2]
        P[:, 0], P[:, 1], P[:, 2] = e, -e, 3 * M * sign[(k // (2 * len(tiny))) % 2]
    elif family == "horizon":
        rp = M + np.sqrt(max(M * M - a * a, 0.0))
        r = rp * np.array([1 - 1e-6, 1 + 1e-6, 1 + 1e-2])[k % 3]
        th = np.array([0.2, 1.0, 1.5])[(k // 3) % 3]
        w = np.sqrt(r * r + a * a) * np.sin(th)
        P[:, 0], P[:, 1], P[:, 2] = w * np.cos(phi), w * np.sin(phi), r * np.cos(th)
    elif family == "far":
        d = rng.normal(size=(N, 3))
        P[:] = d / np.linalg.norm(d, axis=1, keepdims=True) * (far[k % len(far)] * M)[:, None]
    else:
        raise KeyError(family)
    return P


def _null_u(kind, M, a, pos, n3):
    """make_canvas' ray direction (src/RayTraceGR.jl:466-476) at pos for the spatial direction n3: null, past-directed"""
    import truth
    g = truth._metric_fn(kind)(pos[0], pos[1], pos[2], M, a)[0]
    t = np.linalg.solve(g, np.array([1.0, 0, 0, 0]))
    n = np.concatenate([[0.0], n3])
    return (t / np.sqrt(-t @ g @ t) + n / np.sqrt(n @ g @ n)) / np.sqrt(2.0)


def states(name, dtype=np.float64):
    """-> s [len(FAMILIES), N, 8] of dtype.  Seeded per (variant, family, precision); no look at any solver's output."""
    kind, M, a = metric_params(name, dtype)
    out = np.zeros((len(FAMILIES), N, 8), dtype)
    vi = list(VARIANTS).index(name)
    for fi, fam in enumerate(FAMILIES):
        rng = np.random.default_rng([SEED, vi, fi, 32 if dtype == np.float32 else 64])
        s = np.zeros((N, 8))
        s[:, 0] = rng.normal(size=N) * 5
        s[:, 4:] = rng.normal(size=(N, 4))
        if fam == "null":
            for k in range(N):
                src = k % (len(FAMILIES) - 1)
                s[k, 1:4] = out[src, k, 1:4]
                s[k, 4:] = _null_u(kind, M, a, s[k, 1:4], s[k, 5:])
        else:
            s[:, 1:4] = _positions(fam, M, a, dtype, rng)
        out[fi] = s.astype(dtype)
        x, y, z = (out[fi, :, c].astype(np.float64) for c in (1, 2, 3))
        assert (x * x + y * y + z * z > a * a).all() if kind == "ks_ref" else ((x * x + y * y + z * z > a * a) | (z != 0)).all(), (name, fam)
    return out


# ---- the 50-digit reference -----------------------------------------------------------------------------------------
_FN = {}


def _mp_fn(kind):
    if kind not in _FN:
        import mpmath
        import sympy as sp
        import truth
        mpmath.mp.dps = 50
        syms, g = truth.metric_expr(kind)
        dg = [sp.diff(g, v) for v in syms[:3]]
        _FN[kind] = sp.lambdify(syms, [g.tolist(), [d.tolist() for d in dg]], modules="mpmath", cse=True)
    return _FN[kind]


def reference(kind, M, a, s, tensors=True):
    """s: 8 numbers (converted exactly).  -> (u̇[4], g[10], dg[3][10], Γ[4][10]) as mpmath numbers, packed over SYM."""
    import mpmath as mp
    mp.mp.dps = 50
    x = [mp.mpf(float(v)) for v in s]
    G, DG = _mp_fn(kind)(x[1], x[2], x[3], mp.mpf(M), mp.mpf(a))
    zero = mp.mpf(0)

    def d(c, p, q):     # ∂_c g_pq
        return zero if c == 0 else mp.mpf(DG[c - 1][p][q])
    g = mp.matrix(4, 4)
    for p in range(4):
        for q in range(4):
            g[p, q] = mp.mpf(G[p][q])
    u = x[4:]
    low = mp.matrix(4, 1)
    for p in range(4):
        low[p] = -sum((d(b, p, c) - d(p, b, c) / 2) * u[b] * u[c] for b in range(4) for c in range(4))
    ud = mp.lu_solve(g, low)
    if not tensors:
        return [ud[p] for p in range(4)], None, None, None
    gi = mp.inverse(g)
    Gam = [[sum(gi[p, e] * (d(b, e, c) + d(c, e, b) - d(e, b, c)) for e in range(4)) / 2 for (b, c) in SYM] for p in range(4)]
    return ([ud[p] for p in range(4)], [g[p, q] for (p, q) in SYM], [[d(c, p, q) for (p, q) in SYM] for c in (1, 2, 3)], Gam)


def split(v):
    """50-digit numbers -> (hi: nearest double, lo: the remainder as a float)"""
    import mpmath as mp
    v = np.array(v, dtype=object)
    hi = np.array([float(e) for e in v.ravel()]).reshape(v.shape)
    lo = np.array([float(e - mp.mpf(float(e))) for e in v.ravel()], dtype=np.float32).reshape(v.shape)
    return hi, lo


def rel_err(got, hi, lo=None):
    """|got − (hi + lo)| over the trailing axes of one state, relative to the reference's largest component there:
    the measure of every bar in test_rhs_edges.py.  got − hi is exact for neighbours, so the result resolves errors below
    the spacing of doubles.  got, hi [n, …] -> [n]"""
    got, hi = np.asarray(got, np.float64), np.asarray(hi, np.float64)
    n = hi.shape[0]
    dlt = got - hi
    if lo is not None:
        dlt = dlt - np.asarray(lo, np.float64)
    scale = np.abs(hi).reshape(n, -1).max(axis=1)
    e = np.abs(dlt).reshape(n, -1).max(axis=1)
    return np.where(scale > 0, e / np.where(scale > 0, scale, 1.0), e)


def unpack_g(p):
    """[n, 10] -> [n, 4, 4] symmetric"""
    g = np.zeros(p.shape[:-1] + (4, 4), p.dtype)
    for i, (a, b) in enumerate(SYM):
        g[..., a, b] = g[..., b, a] = p[..., i]
    return g


def unpack_dg(p):
    """[n, 3, 10] (∂_x, ∂_y, ∂_z of the packed pairs) -> dg[n, a, b, c] = ∂_c g_ab, ∂_t ≡ 0"""
    dg = np.zeros(p.shape[:-2] + (4, 4, 4), p.dtype)
    for c in range(3):
        dg[..., c + 1] = unpack_g(p[..., c, :])
    return dg


def unpack_gamma(p):
    """[n, 4, 10] -> Γ[n, a, b, c] = Γ^a_bc"""
    return unpack_g(p)


def _one(job):
    name, prec, fi, k, s = job
    dtype = np.float32 if prec == 32 else np.float64
    kind, M, a = metric_params(name, dtype)
    return reference(kind, M, a, s, tensors=k < N_TENSOR)


def variant_arrays(pool, name, dtype):
    """every array of one variant and precision, keyed as in the file"""
    from scenes import rt
    import oracle_lib as O
    prec = 32 if dtype == np.float32 else 64
    kind, M, a = metric_params(name, dtype)
    s = states(name, dtype)
    jobs = [(name, prec, fi, k, s[fi, k]) for fi in range(len(FAMILIES)) for k in range(N)]
    res = pool.map(_one, jobs, chunksize=4)
    nf = len(FAMILIES)
    ud = np.array([r[0] for r in res], dtype=object).reshape(nf, N, 4)
    ten = [r for r in res if r[1] is not None]
    g = np.array([r[1] for r in ten], dtype=object).reshape(nf, N_TENSOR, 10)
    dg = np.array([r[2] for r in ten], dtype=object).reshape(nf, N_TENSOR, 3, 10)
    Gm = np.array([r[3] for r in ten], dtype=object).reshape(nf, N_TENSOR, 4, 10)
    pre = f"f{prec}_{name}_"
    out = {pre + "s": s}
    for key, v in (("ud", ud), ("g", g), ("dg", dg), ("G", Gm)):
        hi, lo = split(v)
        out[pre + key + "_hi"] = hi
        if prec == 64:
            out[pre + key + "_lo"] = lo
    if prec == 64:   # the oracle's own double arithmetic at the same states, measured as the tests measure the device
        sc = rt.make_scene(rt.KerrSchild(M, a, textbook=kind == "ks_true"), [], units=False)
        flat = s.reshape(-1, 8)
        e = rel_err(O.geodesic(sc, flat)[:, 4:], out[pre + "ud_hi"].reshape(-1, 4), out[pre + "ud_lo"].reshape(-1, 4))
        out[pre + "ud_oracle_err"] = e.reshape(nf, N)
        out[pre + "ud_oracle_ld_err"] = rel_err(O.geodesic(sc, flat, long_double=True)[:, 4:], out[pre + "ud_hi"].reshape(-1, 4),
                                                out[pre + "ud_lo"].reshape(-1, 4)).reshape(nf, N)
        out[pre + "tensor_oracle_err"] = oracle_tensor_err(sc, s, out, pre)
    return out


def oracle_tensor_err(sc, s, arrs, pre):
    """[families, N_TENSOR, 3]: rel_err of the oracle's g, ∂g, Γ"""
    import oracle_lib as O
    nf = len(FAMILIES)
    x = np.ascontiguousarray(s[:, :N_TENSOR, :4]).reshape(-1, 4)
    go, dgo, Go = O.eval_metric(sc, x)
    e = np.zeros((nf * N_TENSOR, 3))
    for i, (got, key, unpack) in enumerate(((go, "g", unpack_g), (dgo, "dg", unpack_dg), (Go, "G", unpack_gamma))):
        hi = unpack(arrs[pre + key + "_hi"].reshape((nf * N_TENSOR,) + arrs[pre + key + "_hi"].shape[2:]))
        lo = unpack(arrs[pre + key + "_lo"].reshape((nf * N_TENSOR,) + arrs[pre + key + "_lo"].shape[2:]))
        e[:, i] = rel_err(got, hi, lo)
    return e.reshape(nf, N_TENSOR, 3)


# ---- the traced edge --------------------------------------------------------------------------------------------------
def trace_scene(name):
    """(scene, solver options) of a traced-edge scene: ks_true08 with the disk of config 5, ks_ref0 with example 2's objects"""
    from scenes import rt
    _, objs, _ = rt.example2_scene()
    if name == "ks_true08":
        return rt.make_scene(rt.KerrSchild(1, 0.8), objs[:2] + [rt.Disk(0.05, 2.0, 4.0)], units=False), rt.solver_defaults()
    return rt.make_scene(rt.kerr_schild, objs, units=False), rt.solver_defaults()


def trace_candidates(name):
    """[(group, state0)]: group 0 plane rays aimed past the hole, 1 plane rays into it, 2 axis rays past (outwards), 3 axis
    rays into it.  Seeded; more candidates than are kept (24 + 24 + 8 + 8)."""
    import truth
    sc, _ = trace_scene(name)
    kind = "ks_true" if name == "ks_true08" else "ks_ref"
    rng = np.random.default_rng([SEED, 99, TRACE_SCENES.index(name)])
    cands = []
    for g in (0, 1):
        for _ in range(48):
            phi, R = rng.uniform(0, 2 * np.pi), rng.uniform(5.0, 8.0)
            pos = np.array([R * np.cos(phi), R * np.sin(phi), 0.0])
            b = rng.uniform(5.5, 9.0) * rng.choice([-1.0, 1.0]) if g == 0 else rng.uniform(-1.5, 1.5)   # impact parameter
            inward = -pos / R
            side = np.array([-inward[1], inward[0], 0.0])
            n3 = inward * np.sqrt(max(R * R - b * b, 0.0)) + side * b
            if g == 0 and abs(b) >= R:
                n3 = side * np.sign(b)
            n3[2] = 0.0
            u = _null_u(kind, sc.M, sc.a, pos, n3)
            u[3] = 0.0
            cands.append((g, np.concatenate([[T_START[g]], pos, u])))
    for g in (2, 3):
        for _ in range(16):
            z = rng.uniform(4.0, 8.0) * rng.choice([-1.0, 1.0])
            pos = np.array([0.0, 0.0, z])
            n3 = np.array([0.0, 0.0, np.sign(z) if g == 2 else -np.sign(z)])
            u = _null_u(kind, sc.M, sc.a, pos, n3)
            u[1] = u[2] = 0.0
            cands.append((g, np.concatenate([[T_START[g]], pos, u])))
    return cands


def _trace_one(job):
    import truth
    name, s0 = job
    sc, opt = trace_scene(name)
    r = truth.trace_ray(sc, opt, s0)
    return r["state_end"], r["lambda_end"], r["hit"], r["rgb"]


def traced_edge(pool, name):
    import oracle_lib as O
    sc, opt = trace_scene(name)
    cands = trace_candidates(name)
    s0 = np.array([c[1] for c in cands])
    grp = np.array([c[0] for c in cands])
    orc = O.trace(sc, opt, len(cands), 1, state0=s0)
    res = pool.map(_trace_one, [(name, s) for s in s0], chunksize=2)
    end = np.array([r[0] for r in res])
    hit = np.array([r[2] for r in res], dtype=np.uint8)
    ok = (orc["hit"] == hit) & (np.abs(orc["state_end"] - end).max(axis=1) <= TRUTH_TOL)
    keep = []
    for g, want in ((0, 24), (1, 24), (2, 8), (3, 8)):
        idx = np.flatnonzero(ok & (grp == g))
        assert len(idx) >= want, (name, g, len(idx))
        keep += list(idx[:want])
    keep = np.array(keep)
    pre = f"trace_{name}_"
    return {pre + "state0": s0[keep], pre + "group": grp[keep].astype(np.uint8), pre + "truth_end": end[keep],
            pre + "truth_lambda": np.array([res[i][1] for i in keep]), pre + "truth_hit": hit[keep],
            pre + "truth_rgb": np.array([res[i][3] for i in keep])}


def _save(arrs):
    np.savez_compressed(OUT, families=np.array(FAMILIES), variants=np.array(list(VARIANTS)), **arrs)
    print(os.path.getsize(OUT), "bytes", flush=True)


if __name__ == "__main__":
    trace_only = sys.argv[1:] == ["trace"]       # `make_rhs_edges.py trace`: choose the traced-edge rays again, keep the rest
    arrs = {}
    if trace_only:
        with np.load(OUT) as f:
            arrs = {k: f[k] for k in f.files if k.startswith("f64_") or k.startswith("f32_")}
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        for name in ([] if trace_only else VARIANTS):
            for dtype in (np.float64, np.float32):
                arrs.update(variant_arrays(pool, name, dtype))
            e = arrs[f"f64_{name}_ud_oracle_err"].max(axis=1)
            print(name, "oracle u̇ error per family", " ".join("%.1e" % v for v in e), flush=True)
        for name in TRACE_SCENES:
            arrs.update(traced_edge(pool, name))
            print("traced edge", name, np.bincount(arrs[f"trace_{name}_truth_hit"], minlength=4), flush=True)
    _save(arrs)
