"""The FAR pass's reach test with its rounding floor folded into host-made constants (rtgr_objects.hpp: sphere_reach, plane_reach;
rtgr_args.hpp: reach_guard2, DevObject::nR2 / ::floor_; rtgr_scene_host.hip: object_constants).

The kernels decide "this step cannot reach the object" by
    sphere         RN(|D0| − g2 B)  > F        group / run of groups   RN(D0 − g2 B) > F        plane   RN(|d| − g2 δ_t) > Fp
(one fma, one compare; RN: rounding to nearest in the kernels' scalar type).  The frame stays what it was because each of these IMPLIES
the term-by-term criterion it replaces,
    |D0| > guard B + e (|D0| + 2R²)            D0 > guard B + e (|D0| + 2R²)                    |d| > guard δ_t + e (|x_t| + |p0|),
e = 256 ulp: the FAR pass then hands over every ray it handed over before, and a ray handed over is redone by the NEAR pass from its exact
pre-step state.  CPU part (no GPU): that implication, for the constants AS THE LIBRARY'S HOST FUNCTION ROUNDS THEM (a test hook returns
them), the new side evaluated exactly as the device does (exact rational arithmetic, one rounding), the old side in 40-digit arithmetic.
GPU part: FULL pass against FAR + NEAR, bit for bit, on 64 x 64 frames that lean on the floor."""
import ctypes as C
import decimal
import math
from fractions import Fraction

import numpy as np
import pytest

from scenes import example, rt

abi = rt._abi
D40 = decimal.Context(prec=40)


def reach_constants(objs, f32):
    """[(nR2, floor)] of the objects and (e, guard, g2), as the kernels of the scalar type get them (rtgr_testhook_reach_constants)"""
    lib = abi.load()
    n = len(objs)
    arr = (abi.rtgr_object * n)()
    for k, (kind, p0, radius) in enumerate(objs):
        arr[k].kind = kind
        arr[k].p[0], arr[k].p[8] = p0, radius
    rows, consts = np.zeros((n, 2)), np.zeros(3)
    fn = lib.rtgr_testhook_reach_constants
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(abi.rtgr_object), C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    assert fn(arr, n, int(f32), rows.ctypes.data, consts.ctypes.data) == 0
    return rows, consts


def rn(y, ty):
    """the value of type ty nearest to the rational y (ties to even): what one fma delivers"""
    f = float(y)                       # (int / int true division: correctly rounded)
    if ty is np.float64:
        return f
    c = np.float32(f)                  # a second rounding: look at the neighbours
    best = None
    for v in (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(v):
            continue
        d = abs(Fraction(float(v)) - y)
        even = (int(np.float32(v).view(np.uint32)) & 1) == 0
        if best is None or d < best[0] or (d == best[0] and even):
            best = (d, float(v))
    return best[1]


def new_says_out(lhs0, g2, move, floor, ty):
    """RN(lhs0 − g2 move) > floor, every operand a value of type ty"""
    return rn(Fraction(lhs0) - Fraction(g2) * Fraction(move), ty) > floor


def old_says_out(lhs0, guard, move, e, mag_terms):
    """lhs0 > guard move + e (Σ mag_terms) in 40-digit arithmetic"""
    d = lambda v: decimal.Decimal(v)   # (exact: a binary float is a finite decimal)
    mag = d(0)
    for m in mag_terms:
        mag = D40.add(mag, m if isinstance(m, decimal.Decimal) else d(m))
    return D40.compare(d(lhs0), D40.add(D40.multiply(d(guard), d(move)), D40.multiply(d(e), mag))) > 0


def moves(rng, n, ty):
    """δ from 0 to 10 per axis: uniform, log-uniform down to 1e-12, and exactly 0"""
    kind = rng.integers(0, 3, (n, 1))
    dl = np.where(kind == 0, rng.uniform(0, 10, (n, 3)), np.where(kind == 1, 10.0 ** rng.uniform(-12, 1, (n, 3)), 0.0))
    return dl.astype(ty)


N_RANDOM = 33000      # per criterion and scalar type: 3 x 2 x 33000 = 2e5 evaluated cases in all, ~1e5 per type
N_NEAR = 400


@pytest.mark.parametrize("ty", [np.float64, np.float32], ids=["f64", "f32"])
def test_sphere_and_group_criteria_imply_the_termwise_ones(ty):
    f32 = ty is np.float32
    rng = np.random.default_rng(20 + f32)
    n = N_RANDOM
    R = (10.0 ** rng.uniform(-3, 4, n) * rng.choice([-1.0, 1.0], n)).astype(ty)
    rows, (e, guard, g2) = reach_constants([(abi.SPHERE, 0.0, float(r)) for r in R], f32)
    nR2, F = rows[:, 0], rows[:, 1]
    # the host's constants: −R² is the kernels' own RN(R·R), the floor is no smaller than 2 e R² (1 + 2e) and within a few ulp of it
    assert np.array_equal(nR2.astype(ty), -(R * R))
    assert e == (2.0 ** -15 if f32 else 2.0 ** -44) and guard == float(ty(1) + ty(1e-6)) and ty(g2) == g2
    assert Fraction(g2) >= Fraction(guard) * (1 + 2 * Fraction(e)) * (1 - Fraction(1, 2 ** (23 if f32 else 52)))
    for k in range(0, n, 97):
        exact = 2 * Fraction(e) * Fraction(float(R[k])) ** 2 * (1 + 2 * Fraction(e))
        assert exact <= Fraction(F[k]) <= exact * (1 + Fraction(8, 2 ** (23 if f32 else 52))) and ty(F[k]) == F[k]
    # positions: |D0| from 1e-14 R² to 1e6, outside and (where the sphere is large enough) inside; D0 and B as the kernel's type holds them
    R2 = R.astype(np.float64) ** 2
    mag = 10.0 ** rng.uniform(np.log10(1e-14 * R2), 6.0)
    inside = (rng.random(n) < 0.4) & (mag < 0.99 * R2)
    rad = np.sqrt(R2 + np.where(inside, -mag, mag))
    d = rng.normal(size=(n, 3))
    X = (d / np.linalg.norm(d, axis=1)[:, None] * rad[:, None]).astype(ty)
    dl = moves(rng, n, ty)
    D0 = ((X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]).astype(ty) + (X[:, 2] * X[:, 2] + nR2.astype(ty)).astype(ty)).astype(ty)
    D0 = np.where(rng.random(n) < 0.5, (np.where(inside, -mag, mag)).astype(ty), D0)     # half: the drawn value itself (no cancellation noise)
    B = (dl * (ty(2) * np.abs(X) + dl)).sum(axis=1).astype(ty)
    # … and cases a few ulp on either side of the floor: no move at all, and a move with D0 set next to g2 B + F
    kk = rng.integers(0, n, N_NEAR)
    near_R, near_F, near_B = R[kk], F[kk], np.where(rng.random(N_NEAR) < 0.5, 0.0, B[kk].astype(np.float64)).astype(ty)
    near_D = np.array([rn(Fraction(float(g2)) * Fraction(float(b)) + Fraction(float(f)), ty) for b, f in zip(near_B, near_F)], ty)
    steps = rng.integers(-4, 5, N_NEAR)
    for s in range(1, 5):
        near_D = np.where(steps >= s, np.nextafter(near_D, ty(np.inf)), np.where(steps <= -s, np.nextafter(near_D, ty(0)), near_D))
    near_D = near_D * rng.choice([-1.0, 1.0], N_NEAR).astype(ty)
    R, F, D0, B = np.concatenate([R, near_R]), np.concatenate([F, near_F]), np.concatenate([D0, near_D]), np.concatenate([B, near_B])
    said = {"sphere": [0, 0, 0], "group": [0, 0, 0]}
    for r, f, d0, b in zip(R.tolist(), F.tolist(), D0.tolist(), B.tolist()):
        if not (math.isfinite(d0) and math.isfinite(b)):
            continue
        two_r2 = D40.multiply(decimal.Decimal(2), D40.multiply(decimal.Decimal(r), decimal.Decimal(r)))
        for form, lhs0 in (("sphere", abs(d0)), ("group", d0)):
            new = new_says_out(lhs0, g2, b, f, ty)
            old = old_says_out(lhs0, guard, b, e, (abs(d0), two_r2))
            assert old or not new, (form, r, d0, b, f)
            said[form][0] += new
            said[form][1] += old
            said[form][2] += 1
    for form, (new, old, total) in said.items():      # neither side is vacuous, and the folded floor gives little away
        assert 0.05 * total < new <= old < 0.95 * total, (form, said)
        assert old - new < 0.01 * total, (form, said)


@pytest.mark.parametrize("ty", [np.float64, np.float32], ids=["f64", "f32"])
def test_plane_criterion_implies_the_termwise_one(ty):
    f32 = ty is np.float32
    rng = np.random.default_rng(30 + f32)
    n = N_RANDOM
    p0 = np.where(rng.random(n) < 0.05, 0.0, 10.0 ** rng.uniform(-9, 4, n) * rng.choice([-1.0, 1.0], n)).astype(ty)
    rows, (e, guard, g2) = reach_constants([(abi.PLANE, float(p), 0.0) for p in p0], f32)
    Fp = rows[:, 1]
    assert (rows[:, 0] == 0).all()
    for k in range(0, n, 97):
        exact = 2 * Fraction(e) * abs(Fraction(float(p0[k]))) * (1 + 2 * Fraction(e))
        assert exact <= Fraction(Fp[k]) and ty(Fp[k]) == Fp[k]
        assert Fraction(Fp[k]) <= exact * (1 + Fraction(8, 2 ** (23 if f32 else 52))) + Fraction(float(np.finfo(ty).tiny)) * 4
    dist = 10.0 ** rng.uniform(np.log10(np.maximum(1e-14 * np.abs(p0.astype(np.float64)), 1e-20)), 6.0) * rng.choice([-1.0, 1.0], n)
    x0 = (p0.astype(np.float64) + dist).astype(ty)
    dt = moves(rng, n, ty)[:, 0]
    kk = rng.integers(0, n, N_NEAR)          # … and a few ulp on either side of the floor: x0 next to p0 ± (g2 δ + Fp)
    near = np.array([rn(Fraction(float(p0[k])) + Fraction(float(g2)) * Fraction(float(dt[k])) + Fraction(float(Fp[k])), ty) for k in kk], ty)
    steps = rng.integers(-4, 5, N_NEAR)
    for s in range(1, 5):
        near = np.where(steps >= s, np.nextafter(near, ty(np.inf)), np.where(steps <= -s, np.nextafter(near, ty(-np.inf)), near))
    p0, Fp, x0, dt = np.concatenate([p0, p0[kk]]), np.concatenate([Fp, Fp[kk]]), np.concatenate([x0, near]), np.concatenate([dt, dt[kk]])
    d = (x0 - p0).astype(ty)                 # the kernel's own, rounded, difference
    new_n = old_n = total = 0
    for p, f, x, dd, t in zip(p0.tolist(), Fp.tolist(), x0.tolist(), d.tolist(), dt.tolist()):
        if not math.isfinite(dd):
            continue
        new = new_says_out(abs(dd), g2, t, f, ty)
        old = old_says_out(abs(dd), guard, t, e, (abs(x), abs(p)))
        assert old or not new, (p, x, dd, t, f)
        new_n, old_n, total = new_n + new, old_n + old, total + 1
    assert 0.05 * total < new_n <= old_n < 0.95 * total and old_n - new_n < 0.01 * total, (new_n, old_n, total)


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU: the single FULL pass (every accepted step scanned against every object, option split = 0) against FAR + NEAR, bit for bit
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def _spiral(n):
    """n small spheres (radius 0.2-0.45) on a spiral of radius 3-7.5 around the hole: the geometry of the benchmark's long lists"""
    out = []
    for k in range(n):
        t, rad = 0.7 * (k + 2), 3.0 + 4.5 * k / max(n, 1)
        out.append(rt.Sphere((0.0, rad * math.cos(t), rad * math.sin(t) + 1.5, 1.2 * math.sin(2.3 * t)), (1, 0, 0, 0), 0.2 + 0.25 * abs(math.sin(1.1 * t))))
    return out


def _cases():
    metric, objs, cam = rt.example2_scene()
    sky, plane, ball = objs
    tiny_cam = dict(cam, widthx=(0, 6e-3, 0, 0), widthy=(0, 0, 0, 6e-3))      # a 6 mm screen: rays 0.1 R apart around a sphere of R = 1e-3
    return {
        "example2": (objs, cam, {}),
        "plus17": (objs + _spiral(17), cam, {}),                                # 20 objects: a device table, groups of <= 4
        "plus61": (objs + _spiral(61), cam, {}),                                # 64 objects: groups of <= 8
        "plus61_runs": (objs + _spiral(61), cam, dict(groups=2)),               # … in groups of <= 2: 31 groups, in runs of groups
        "grazed_1e-3": ([sky, plane, rt.Sphere((0, 4, -1.95, 0), (1, 0, 0, 0), 1e-3)], tiny_cam, {}),
        "plane_-1e-9": ([sky, rt.Plane(-1e-9), ball], cam, {}),
    }


KEYS = ("rgb", "status", "hit", "n_accept", "n_reject")


@pytest.mark.gpu
@pytest.mark.parametrize("case,ty", [("example2", np.float64), ("example2", np.float32), ("plus17", np.float64), ("plus61", np.float64),
                                     ("plus61_runs", np.float64), ("grazed_1e-3", np.float64), ("plane_-1e-9", np.float64)],
                         ids=lambda v: v if isinstance(v, str) else np.dtype(v).name)
def test_full_pass_equals_far_plus_near_where_the_floor_matters(lib, case, ty):
    from test_gpu_parity import hip_trace
    objs, cam, knobs = _cases()[case]
    sc, camera, opt = rt.make_scene(rt.kerr_schild, objs), rt.make_camera(**cam), rt.solver_defaults(ty)
    with abi.options(lib, **knobs):
        pair = hip_trace(lib, sc, opt, 64, 64, cam=camera, dtype=ty)
    with abi.options(lib, split=0, **knobs):
        full = hip_trace(lib, sc, opt, 64, 64, cam=camera, dtype=ty)
    for k in KEYS:
        assert np.array_equal(pair[k], full[k], equal_nan=pair[k].dtype.kind == "f"), (case, k, int((pair[k] != full[k]).sum()))
    hits = set(np.unique(pair["hit"]).tolist())
    if case == "grazed_1e-3":      # the tiny sphere is on the frame, and so is its edge
        assert {1, 3} <= hits and 20 < int((pair["hit"] == 3).sum()) < 64 * 64 - 20, hits
    elif case == "plane_-1e-9":    # every ray starts 1e-9 from the plane
        assert 2 in hits and int((pair["hit"] == 2).sum()) > 64 * 64 // 2, hits
    else:
        assert len(hits) >= (3 if case == "example2" else 5), hits
