"""The geodesic right-hand side and the metric hooks at the EDGES of the Kerr–Schild coordinates, against a 50-digit reference.

tests/golden/rhs_edges.npz (made by tests/golden/make_rhs_edges.py: the sympy metric of tests/truth.py, its symbolic
derivatives and a linear solve, all in mpmath at 50 digits) holds, for ten metric variants x eight families of 32 states — polar
axis, equatorial plane, coordinate axes, |z| and |x| = |y| down to the smallest denormal, both sides of the horizon, radii up to
10⁶ M, null directions — the exact u̇ (and g, ∂g, Γ at the first states of each family) as double-double pairs, and next to
them the error of the ORACLE's own double arithmetic at the same states.

The bars.  Float64: the device's error against the 50-digit value, relative to the largest component at that state, maximum
over a family, must stay within max(16 x the oracle's recorded error over that family, 64 eps).  Oracle and device are different
groupings of the same rational function, each a few dozen roundings long: a factor 16 allows another grouping and cannot hide a
wrong term (test_geodesic_rhs_matches_oracle's 5e-12 is a thousand times looser).  The bar is a property of the reference side
alone.  Float32: the project's stated F32_RHS_TOL per path and the reference testset's 4 eps^¾ / 16 eps^¾ (test/runtests.jl:38).

The identities (reflection, symmetry planes, t-independence, the homogeneity u -> 2⁷u) hold to the BIT for any fixed IEEE
instruction sequence, fused or not; they are asserted for the oracle on the CPU and for the three device paths on the GPU.

mpmath runs in the CPU tests only (a sample of the fixture is regenerated to the bit); the GPU tests read the fixture.
"""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O
from conftest import ROOT
from scenes import rt

abi = rt._abi


def _generator():
    spec = importlib.util.spec_from_file_location("make_rhs_edges", os.path.join(ROOT, "tests", "golden", "make_rhs_edges.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _generator()
VARIANTS, FAMILIES, NT = list(G.VARIANTS), G.FAMILIES, G.N_TENSOR
NF = len(FAMILIES)
EPS = float(np.finfo(np.float64).eps)
EPS32_34 = float(np.finfo(np.float32).eps) ** 0.75
_FIX = {}


def fix(key):
    if not _FIX:
        with np.load(os.path.join(ROOT, "tests", "golden", "rhs_edges.npz")) as f:
            _FIX.update({k: f[k] for k in f.files})
    return _FIX[key]


def metric_of(name):
    kind, M, a = G.VARIANTS[name]
    return rt.KerrSchild(M, a, textbook=kind == "ks_true")


def oracle_scene(name):
    return rt.make_scene(metric_of(name), [], units=False)


def f64_bar(oracle_err):
    """[families, n] recorded oracle errors -> [families] bars"""
    return np.maximum(16.0 * oracle_err.max(axis=1), 64 * EPS)


def tensors(name, prec):
    """the reference's g [F*NT, 4, 4], dg [.., 4, 4, 4], Γ [.., 4, 4, 4] as (hi, lo or None) pairs, and the positions"""
    out = []
    for key, unpack in (("g", G.unpack_g), ("dg", G.unpack_dg), ("G", G.unpack_gamma)):
        hi = fix(f"f{prec}_{name}_{key}_hi")
        hi = unpack(hi.reshape((NF * NT,) + hi.shape[2:]))
        lo = None
        if prec == 64:
            lo = fix(f"f{prec}_{name}_{key}_lo")
            lo = unpack(lo.reshape((NF * NT,) + lo.shape[2:]))
        out.append((hi, lo))
    x = np.ascontiguousarray(fix(f"f{prec}_{name}_s")[:, :NT, :4]).reshape(-1, 4)
    return x, out


def report(err, bar, what):
    """err, bar [families]: one assertion that names every family over its bar, with the figures"""
    bar = np.broadcast_to(bar, err.shape)
    lines = [f"{FAMILIES[i]:8s} {err[i]:.2e} (bar {bar[i]:.2e})" for i in range(len(err))]
    print(what, "|", "; ".join(lines))
    bad = [lines[i] for i in range(len(err)) if not err[i] <= bar[i]]
    assert not bad, f"{what}: " + "; ".join(bad)


# ---- the identities, for any implementation f(s [n, 8]) -> ṡ [n, 8] ---------------------------------------------------
def identity_violations(f, s, dtype, M, a):
    """M, a: the metric's, for the domain of the states MADE here by zeroing coordinates (kept where ρ² >= a² + M²).
    -> list of (identity, number of states violating it).  Zeros compare equal whatever their sign (a sum of a +0 and a −0 is
    +0 on both sides of a reflection); everything else is compared as bits (==)."""
    s = np.ascontiguousarray(s, dtype)
    tiny_normal = 2.0 ** (-100 if dtype == np.float32 else -1000)
    bad = []
    base = f(s)
    assert np.isfinite(base).all()

    def count(name, ok):
        if not ok.all():
            bad.append((name, int((~ok).sum())))
    # z -> −z, u^z -> −u^z
    m = s.copy(); m[:, 3] = -m[:, 3]; m[:, 7] = -m[:, 7]
    want = base.copy(); want[:, 7] = -want[:, 7]; want[:, 3] = -want[:, 3]
    count("reflection", (f(m) == want).all(axis=1))
    # in the plane / on the axis
    def inside(v):
        v = v.astype(np.float64)
        return v[:, 1] ** 2 + v[:, 2] ** 2 + v[:, 3] ** 2 >= a * a + M * M
    p = s.copy(); p[:, 3] = 0; p[:, 7] = 0
    fp = f(p[inside(p)])
    count("plane", (fp[:, 7] == 0) & np.isfinite(fp).all(axis=1))
    x = s.copy(); x[:, 1] = x[:, 2] = 0; x[:, 5] = x[:, 6] = 0
    fx = f(x[inside(x)])
    assert len(fp) >= len(s) // 2 and len(fx) >= len(s) // 4
    count("axis", (fx[:, 5] == 0) & (fx[:, 6] == 0))
    # t
    for t in (1e30 if dtype == np.float32 else 1e300, -3.0):
        q = s.copy(); q[:, 0] = t
        count("time", (f(q)[:, 4:] == base[:, 4:]).all(axis=1))
    # u -> 2⁷ u: u̇ -> 2¹⁴ u̇ (compared where neither side leaves the normal range)
    h = s.copy(); h[:, 4:] *= 128
    fh = f(h)[:, 4:].astype(np.float64)
    b = base[:, 4:].astype(np.float64)
    defined = ((np.abs(b) >= tiny_normal) & np.isfinite(fh)) | ((b == 0) & (fh == 0))
    count("homogeneity", ((fh == b * 2.0 ** 14) | ~defined).all(axis=1))
    return bad


def identity_states(name, prec):
    """every fourth state of every family of a variant: 64 states"""
    return fix(f"f{prec}_{name}_s").reshape(-1, 8)[::4]


# ---- CPU -----------------------------------------------------------------------------------------------------------------
def test_fixture_layout_and_states_regenerate():
    assert list(fix("families")) == FAMILIES and list(fix("variants")) == VARIANTS
    for name in VARIANTS:
        for dtype, prec in ((np.float64, 64), (np.float32, 32)):
            s = fix(f"f{prec}_{name}_s")
            assert s.dtype == dtype and s.shape == (NF, G.N, 8) and np.isfinite(s).all()
            assert G.states(name, dtype).tobytes() == s.tobytes()
    ax, eq = FAMILIES.index("axis"), FAMILIES.index("equator")
    s = fix("f64_ks_true08_s")
    assert (s[ax, :, 1:3] == 0).all() and (s[eq, :, 3] == 0).all() and np.abs(s[FAMILIES.index("tiny_z"), :, 3]).min() == 5e-324
    # null: g(u, u) = 0 to rounding and past-directed
    import truth
    kind, M, a = G.VARIANTS["ks_true08"]
    for v in s[FAMILIES.index("null")]:
        g = truth._metric_fn(kind)(v[1], v[2], v[3], M, a)[0]
        assert abs(v[4:] @ g @ v[4:]) < 1e-13 * (v[4:] @ v[4:]) and v[4] < 0


@pytest.mark.parametrize("name", ["ks_ref08", "extremal", "scaled_down"])
def test_fixture_reference_regenerates_to_the_bit(name):
    """One state per family with its tensors in Float64 and one in Float32, evaluated again in 50 digits (≈ 1 s)."""
    for fi in range(NF):
        for dtype, prec, k in ((np.float64, 64, (fi + 1) % NT), (np.float32, 32, NT + fi)):
            kind, M, a = G.metric_params(name, dtype)
            ref = G.reference(kind, M, a, fix(f"f{prec}_{name}_s")[fi, k], tensors=k < NT)
            for key, v in zip(("ud", "g", "dg", "G"), ref):
                if v is None:
                    continue
                hi, lo = G.split(v)
                assert hi.tobytes() == fix(f"f{prec}_{name}_{key}_hi")[fi, k].tobytes(), (fi, key)
                assert prec == 32 or lo.tobytes() == fix(f"f{prec}_{name}_{key}_lo")[fi, k].tobytes(), (fi, key)


@pytest.mark.parametrize("name", VARIANTS)
def test_oracle_error_is_the_recorded_one(name):
    """The bars of the GPU tests are multiples of these numbers: they must be what the oracle gives here."""
    sc = oracle_scene(name)
    s = fix(f"f64_{name}_s")
    hi, lo = fix(f"f64_{name}_ud_hi").reshape(-1, 4), fix(f"f64_{name}_ud_lo").reshape(-1, 4)
    ds = O.geodesic(sc, s.reshape(-1, 8))
    assert np.isfinite(ds).all()
    assert np.array_equal(G.rel_err(ds[:, 4:], hi, lo).reshape(NF, G.N), fix(f"f64_{name}_ud_oracle_err"))
    ld = G.rel_err(O.geodesic(sc, s.reshape(-1, 8), long_double=True)[:, 4:], hi, lo).reshape(NF, G.N)
    assert np.array_equal(ld, fix(f"f64_{name}_ud_oracle_ld_err"))
    assert ld.max() <= 16 * EPS                      # the reference and the long-double chain agree far below every bar
    arrs = {k: fix(k) for k in _FIX if k.startswith(f"f64_{name}_")}
    assert np.array_equal(G.oracle_tensor_err(sc, s, arrs, f"f64_{name}_"), fix(f"f64_{name}_tensor_oracle_err"))
    # what the bars come to
    assert f64_bar(fix(f"f64_{name}_ud_oracle_err")).max() < 5e-12


@pytest.mark.parametrize("name", ["ks_ref0", "ks_ref08", "ks_true0", "ks_true08"])
def test_oracle_satisfies_the_exact_identities(name):
    sc = oracle_scene(name)
    assert identity_violations(lambda s: O.geodesic(sc, s), identity_states(name, 64), np.float64, *G.VARIANTS[name][1:]) == []


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("path", [0, 1, 2])
def test_rhs_f64_at_the_edges(lib, name, path):
    s = fix(f"f64_{name}_s").reshape(-1, 8)
    got = rt.geodesic(s, metric_of(name), path=path)
    assert np.array_equal(got[:, :4], s[:, 4:]) and np.isfinite(got).all()
    err = G.rel_err(got[:, 4:], fix(f"f64_{name}_ud_hi").reshape(-1, 4), fix(f"f64_{name}_ud_lo").reshape(-1, 4))
    report(err.reshape(NF, G.N).max(axis=1), f64_bar(fix(f"f64_{name}_ud_oracle_err")), f"f64 rhs {name} path {path}")


def _hooks(metric, x, dtype):
    """rtgr_eval_metric_f64 / _f32 through the two public calls: (g, ∂g, Γ)"""
    g, dg = rt.dmetric(metric, x, dtype=dtype)
    return g, dg, rt.christoffel(metric, x, dtype=dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
def test_metric_hooks_f64_at_the_edges(lib, name):
    x, ref = tensors(name, 64)
    got = _hooks(metric_of(name), x, np.float64)
    orc = fix(f"f64_{name}_tensor_oracle_err")
    for i, what in enumerate(("g", "dg", "Gamma")):
        assert np.isfinite(got[i]).all()
        err = G.rel_err(got[i], *ref[i]).reshape(NF, NT).max(axis=1)
        report(err, f64_bar(orc[:, :, i]), f"f64 {what} {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("path", [0, 1, 2])
def test_rhs_f32_at_the_edges(lib, name, path):
    from test_gpu_parity import F32_RHS_TOL
    s = fix(f"f32_{name}_s").reshape(-1, 8)
    got = rt.geodesic(s, metric_of(name), path=path, dtype=np.float32)
    assert got.dtype == np.float32 and np.array_equal(got[:, :4], s[:, 4:]) and np.isfinite(got).all()
    err = G.rel_err(got[:, 4:], fix(f"f32_{name}_ud_hi").reshape(-1, 4))
    report(err.reshape(NF, G.N).max(axis=1), F32_RHS_TOL[path], f"f32 rhs {name} path {path}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", VARIANTS)
def test_metric_hooks_f32_at_the_edges(lib, name):
    x, ref = tensors(name, 32)
    got = _hooks(metric_of(name), x, np.float32)
    for i, (what, bar) in enumerate((("g", 4 * EPS32_34), ("dg", 4 * EPS32_34), ("Gamma", 16 * EPS32_34))):
        assert got[i].dtype == np.float32 and np.isfinite(got[i]).all()
        report(G.rel_err(got[i], ref[i][0]).reshape(NF, NT).max(axis=1), bar, f"f32 {what} {name}")


@pytest.mark.gpu
def test_minkowski_at_the_edges(lib):
    """the sixth of test_gpu_parity.METRICS: g = η, ∂g = Γ = 0 and u̇ = 0 exactly, at the same states, on every path"""
    for dtype, prec in ((np.float64, 64), (np.float32, 32)):
        s = fix(f"f{prec}_ks_true08_s").reshape(-1, 8)
        for path in (0, 1, 2):
            got = rt.geodesic(s, rt.minkowski, path=path, dtype=dtype)
            assert np.array_equal(got[:, :4], s[:, 4:]) and (got[:, 4:] == 0).all()
        g, dg, Gam = _hooks(rt.minkowski, s[:, :4], dtype)
        assert (g == np.diag([-1.0, 1, 1, 1])).all() and (dg == 0).all() and (Gam == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ks_ref0", "ks_ref08", "ks_true0", "ks_true08", "tiny_spin", "extremal"])
@pytest.mark.parametrize("prec", [64, 32])
def test_exact_identities_on_the_device(lib, name, prec):
    dtype = np.float64 if prec == 64 else np.float32
    m = metric_of(name)
    bad = {path: identity_violations(lambda s: rt.geodesic(s, m, path=path, dtype=dtype).reshape(-1, 8),
                                     identity_states(name, prec), dtype, *G.VARIANTS[name][1:]) for path in (0, 1, 2)}
    assert all(v == [] for v in bad.values()), bad


def _scalable(s, k):
    """states whose position survives a scaling by 2^k and back unchanged (zeros do; the smallest denormals do not)"""
    p = s[:, 1:4]
    with np.errstate(over="ignore", under="ignore"):
        return ((p * 2.0 ** k) * 2.0 ** -k == p).all(axis=1) & np.isfinite(p * 2.0 ** k).all(axis=1) & \
            ((np.abs(p) >= 2.0 ** -900) | (p == 0)).all(axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ks_true0", "ks_true08"])
@pytest.mark.parametrize("path", [0, 1, 2])
def test_scaling_the_whole_problem_scales_the_rhs_to_the_bit(lib, name, path):
    """(x, M, a) -> 2^±10 (x, M, a): u̇ -> 2^∓10 u̇ exactly for the textbook radius — every operand of a reciprocal square root
    scales by an even power of two, so seed, correction and every product scale with it.  (The as-written radius r = ρ/2 + …
    mixes ρ and ρ² and is not homogeneous.)"""
    kind, M, a = G.VARIANTS[name]
    s = fix(f"f64_{name}_s").reshape(-1, 8)
    base = rt.geodesic(s, rt.KerrSchild(M, a), path=path)[:, 4:]
    for k in (10, -10):
        keep = _scalable(s, k)
        assert keep.sum() >= 0.7 * len(s)
        t = s[keep].copy()
        t[:, 1:4] *= 2.0 ** k
        got = rt.geodesic(t, rt.KerrSchild(M * 2.0 ** k, a * 2.0 ** k), path=path)[:, 4:]
        differ = (got != base[keep] * 2.0 ** -k).any(axis=1)
        assert not differ.any(), (k, int(differ.sum()), np.flatnonzero(keep)[differ][:8])


def rhs_operands():
    """every operand the four ks_field branches (and accel_spin_true's fused seed) hand to rcp_ / sqrt_inv at the fixture's
    Float64 positions, in numpy: ρ², q, the two radicands, r, r², r² + a², r⁴ + a²z² (1 + ρ and r²(r² + a²)² for a = 0 as
    written and the production textbook form)"""
    ops = []
    for name in VARIANTS:
        kind, M, a = G.VARIANTS[name]
        x, y, z = (fix(f"f64_{name}_s")[..., c].ravel() for c in (1, 2, 3))
        a2 = a * a
        rho2 = x * x + y * y + z * z
        q = rho2 - a2
        if kind == "ks_ref":
            rad = a2 * z * z + (0.5 * q) ** 2
            r = 0.5 * np.sqrt(q) + np.sqrt(rad)
            ops += [q, rad, 1 + np.sqrt(rho2)]
        else:
            rad = q * q + 4 * a2 * z * z
            r = np.sqrt(0.5 * (q + np.sqrt(rad)))
            ops += [rad, r * r * (r * r + a2) ** 2]
        ops += [rho2, r, r * r, r * r + a2, r ** 4 + a2 * z * z]
    ops = np.concatenate(ops)
    assert np.isfinite(ops).all() and (ops > 0).all()
    return ops


@pytest.mark.gpu
def test_fast_reciprocal_and_rsqrt_over_the_range_the_rhs_uses(lib):
    """frcp / frsq (rtgr_physics.hpp): <= 1.5e-16 / 2.0e-16 relative against long double, at every operand the RHS forms at the
    fixture's positions and at 2^20 log-uniform operands spanning their range (2^-55 … 2^180; test_fast_reciprocal_and_rsqrt_accuracy
    covers 2^-10 … 2^10)."""
    ops = rhs_operands()
    lo, hi = np.log2(ops.min()), np.log2(ops.max())
    assert lo < -35 and hi > 170
    rng = np.random.default_rng(4)
    x = np.ascontiguousarray(np.concatenate([ops, np.exp2(rng.uniform(lo, hi, size=1 << 20))]))
    rcp, rsq = np.empty_like(x), np.empty_like(x)
    abi.check(lib, lib.rtgr_eval_fastmath_f64(None, x.ctypes.data, x.size, rcp.ctypes.data, rsq.ctypes.data))
    xl = x.astype(np.longdouble)
    e_rcp = np.abs(rcp.astype(np.longdouble) * xl - 1)
    e_rsq = np.abs(rsq.astype(np.longdouble) * np.sqrt(xl) - 1)
    print("frcp", float(e_rcp.max()), "frsq", float(e_rsq.max()), "range 2^%.1f .. 2^%.1f" % (lo, hi))
    assert e_rcp.max() <= 1.5e-16 and e_rsq.max() <= 2.0e-16, (float(e_rcp.max()), float(x[e_rcp.argmax()]), float(e_rsq.max()), float(x[e_rsq.argmax()]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.TRACE_SCENES)
def test_traced_edge_rays_stay_in_their_symmetry_set(lib, name):
    """64 rays that start EXACTLY in the equatorial plane (z = u^z = 0) or on the polar axis (x = y = u^x = u^y = 0), half of
    each aimed past the hole and half into it: the plane and the axis are invariant sets of the flow AND of every device
    formulation's arithmetic (the identities above), so the end state has z ≡ 0 / x = y ≡ 0 exactly; the frame passes compare()
    against the oracle with no class flip and ends within 3e-11 of the true geodesics stored by the generator."""
    from test_gpu_parity import F32_FLIP_FRAC, F32_RGB_TOL, compare, hip_trace
    from scenes import wrap_aware_rgb_err
    s0, grp = fix(f"trace_{name}_state0"), fix(f"trace_{name}_group")
    assert s0.shape == (64, 8) and list(np.bincount(grp)) == [24, 24, 8, 8]
    plane, axis = grp < 2, grp >= 2
    assert (s0[plane, 3] == 0).all() and (s0[plane, 7] == 0).all() and (s0[axis][:, [1, 2, 5, 6]] == 0).all()
    sc_o, opt = G.trace_scene(name)
    sc = _device_scene(name)
    gpu = hip_trace(lib, sc, opt, 64, 1, state0=s0)
    ref = O.trace(sc_o, opt, 64, 1, state0=s0)
    assert (gpu["state_end"][plane][:, [3, 7]] == 0).all() and (gpu["state_end"][axis][:, [1, 2, 5, 6]] == 0).all()
    # (step attempts: the project's allowance for these two scenes, test_example2_matches_oracle_and_golden_png and
    #  test_variant_crops_match_oracle — ±1 as written, ±2 with spin)
    compare(gpu, ref, nobj=sc.nobj, sc=sc, max_class_flips=0, max_step_diff=1 if name == "ks_ref0" else 2)
    assert (gpu["hit"] == fix(f"trace_{name}_truth_hit")).all()
    d = np.abs(gpu["state_end"] - fix(f"trace_{name}_truth_end")).max(axis=1)
    print("traced edge", name, "max |end − truth|", d.max(), "oracle", np.abs(ref["state_end"] - fix(f"trace_{name}_truth_end")).max())
    assert d.max() <= G.TRUTH_TOL, d.max()
    # Float32: the same rays, rounded (zeros stay zeros), at the project's Float32 bars against the Float32 oracle
    opt32 = rt.solver_defaults(np.float32)
    s32 = s0.astype(np.float32)
    g32 = hip_trace(lib, sc, opt32, 64, 1, state0=s32, dtype=np.float32)
    r32 = O.trace(sc_o, opt32, 64, 1, state0=s32, dtype=np.float32)
    assert (g32["state_end"][plane][:, [3, 7]] == 0).all() and (g32["state_end"][axis][:, [1, 2, 5, 6]] == 0).all()
    flips = g32["hit"] != r32["hit"]
    assert flips.mean() <= F32_FLIP_FRAC, flips.mean()
    assert wrap_aware_rgb_err(g32["rgb"][:, ~flips].astype(float), r32["rgb"][:, ~flips].astype(float), g32["hit"][~flips], sc=sc) < F32_RGB_TOL


def _device_scene(name):
    _, objs, _ = rt.example2_scene()
    if name == "ks_true08":
        return rt.make_scene(rt.KerrSchild(1, 0.8), objs[:2] + [rt.Disk(0.05, 2.0, 4.0)])
    return rt.make_scene(rt.kerr_schild, objs)


def test_traced_edge_fixture_is_what_the_oracle_and_the_truth_give():
    """On the CPU: the stored rays are the generator's (seeded), the oracle shows the truth's hit class on every one and ends
    within 3e-11 of it, and a true geodesic of each group integrates again to the stored end state."""
    import truth
    for name in G.TRACE_SCENES:
        s0, grp = fix(f"trace_{name}_state0"), fix(f"trace_{name}_group")
        cands = G.trace_candidates(name)
        pool = {c[1].tobytes() for c in cands}
        assert all(v.tobytes() in pool for v in s0)
        sc, opt = G.trace_scene(name)
        ref = O.trace(sc, opt, 64, 1, state0=s0)
        assert (ref["hit"] == fix(f"trace_{name}_truth_hit")).all()
        assert np.abs(ref["state_end"] - fix(f"trace_{name}_truth_end")).max() <= G.TRUTH_TOL
        assert (ref["state_end"][grp < 2][:, [3, 7]] == 0).all() and (ref["state_end"][grp >= 2][:, [1, 2, 5, 6]] == 0).all()
        hits = fix(f"trace_{name}_truth_hit")
        assert len(set(hits[grp == 0]) | set(hits[grp == 2])) >= 1 and (hits > 0).all()
        for g in ((0, 3) if name == G.TRACE_SCENES[0] else (1, 2)):     # (≈ 1 s each)
            k = int(np.flatnonzero(grp == g)[0])
            r = truth.trace_ray(sc, opt, s0[k])
            assert r["hit"] == hits[k] and np.abs(r["state_end"] - fix(f"trace_{name}_truth_end")[k]).max() < 1e-12
