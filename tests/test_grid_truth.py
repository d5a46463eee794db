"""Traces through grid-sampled metrics (RTGR_GRID, 3-D and 4-D) against TRUE geodesics.

The oracle has no grid metric, so the other grid tests compare grid kernels with each other, with a closed form under refinement,
or on flat space.  Here the sampled field is a quadratic polynomial per component (tests/grid_truth.py), which the Catmull-Rom
interpolant reproduces to rounding on any grid — inside the valid box and where the clamped outer cell extrapolates.  The device's
field IS the polynomial, its true geodesics come from tests/truth.py's DOP853 (symbolic derivatives, d_t g included), and every bar
below is one of test_truth.py's, imported.  The grids are anisotropic, non-cubic and off-centre, with the camera's centre on a node.

tests/golden/truth_grid_{quad3,quad4}.npz: the lens scenes (sky, plane, sphere, disk; the box holds every ray).
tests/golden/truth_grid_{quad3,quad4}_box.npz: the same field on a grid whose valid box — different on every axis, and ending early
in t — is smaller than the rays' reach, all objects strictly inside and no sky: a ray ends in an event exactly when its true
geodesic meets an object before it leaves the box, wherever the steps fall (an accepted step is scanned for events first).

Measured maxima are recorded in profiles/grid_truth/README.md.
"""
import functools
import os

import numpy as np
import pytest

import grid_truth as G
from conftest import ROOT
from scenes import rt
from test_grid_metric import catmull_rom
from test_grid_metric_4d import catmull_rom4
from test_truth import F32_BARS, PLANE, TOL_SPHERE, _check_against_truth

abi = rt._abi
OUTPUTS = ("rgb", "state_end", "lambda_end", "status", "hit", "n_accept", "n_reject")
STRETCH = 1e-6              # the teeth tests: one spacing declared this much (relative) too large
TEETH_RAYS = 8


@functools.lru_cache(maxsize=None)
def fixture(name):
    with np.load(os.path.join(ROOT, "tests", "golden", f"truth_grid_{name}.npz")) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def grid_samples(name):
    f = fixture(name)
    s = G.samples(G.GRIDS[name], f["coef"])
    s.setflags(write=False)
    return s


def subset(got, f, sel, got_sel=None):
    """(got, f) as _check_against_truth takes them — a 'frame' of len(sel) x 1 pixels: the rays `sel` of fixture f, and the rays
    `got_sel` (default: the same) of a traced result"""
    sel = np.flatnonzero(sel) if np.asarray(sel).dtype == bool else np.asarray(sel)
    got_sel = sel if got_sel is None else np.asarray(got_sel)
    fs = {k: f[k][sel] for k in ("hit", "state_end", "lambda_end", "rgb", "clearance")}
    fs["n"], fs["ij"] = len(sel), np.stack([np.arange(len(sel)), np.zeros(len(sel), int)], axis=1)
    gs = {k: got[k][got_sel] for k in ("hit", "state_end", "lambda_end")}
    gs["rgb"] = got["rgb"][:, got_sel]
    return gs, fs


def margin(name, pos):
    """> 0 inside the valid box of the fixture's grid, < 0 outside (pos: a 4-position)"""
    import truth
    return truth.box_margin(G.valid_box(G.GRIDS[name]), pos)


# ---- CPU: the fixtures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.NAMES)
def test_fixtures_meet_their_conditions(name):
    f, grid = fixture(name), G.GRIDS[name]
    dim = grid["dim"]
    assert np.array_equal(f["coef"], G.field_table(dim)) and np.array_equal(f["ij"], G.pixels())
    assert tuple(f["origin"]) == grid["origin"] and tuple(f["spacing"]) == grid["spacing"] and tuple(f["grid_n"]) == grid["n"]
    assert len(set(grid["spacing"])) == dim and len(set(grid["origin"])) == dim and len(set(grid["n"][-3:])) == 3
    box = G.valid_box(grid)
    sc, cam = G.truth_scene(name)
    # Lorentzian over every box a ray or a stage can be in: the valid box, a cell beyond it, and — box scenes — out to the guard
    wide = [(lo - h, hi + h) for (lo, hi), h in zip(box, grid["spacing"])]
    if name in G.BOX:
        wide = wide[:dim - 3] + [(-G.GUARD, G.GUARD)] * 3
        if dim == 4:
            wide[0] = (f["state_end"][:, 0].min(), wide[0][1])
    (t_lo, t_hi), (s_lo, s_hi) = G.signature_range(f["coef"], wide, per_axis=13, radius=None if name in G.LENS else G.GUARD)
    assert t_hi < -0.1 and s_lo > 0.1, ((t_lo, t_hi), (s_lo, s_hi))
    if dim == 4:    # the time dependence matters at the 1e-9 level by a wide margin: g changes by >= 1e-2 over the rays' time range
        fn = G.field_np(f["coef"])
        ends = f["state_end"] if name in G.LENS else f["state_exit"][np.isfinite(f["lambda_exit"])]
        x, y, z = ends[:, 1], ends[:, 2], ends[:, 3]
        assert np.abs(fn(ends[:, 0].min(), x, y, z) - fn(0.0, x, y, z)).max(axis=1).min() >= 1e-2
    # the camera's centre is a grid node of the lens grids: the centre pixel starts with integer cell coordinates
    lens = G.GRIDS[G.LENS[dim - 3]]
    cell = (np.array(G.CAMERA["pos"])[4 - dim:] - np.array(lens["origin"])) / np.array(lens["spacing"])
    assert np.array_equal(cell, np.round(cell)) and tuple(f["ij"][0]) == (22, 17)
    assert np.array_equal(f["state0"][0, :4], G.CAMERA["pos"])
    # marked rays: a grazing ray (clearance below the hit threshold, or the truth's looser run ended on another object: a chord
    # shorter than its step) or an object met after leaving the box; at most 10 %
    threshold = rt.solver_defaults().hit_threshold
    late = (f["hit"] > 0) & (f["lambda_end"] > f["lambda_exit"])
    assert np.array_equal(f["marked"], (f["clearance"] < threshold) | late | ~np.isfinite(f["self_err"]))
    assert f["marked"].sum() <= 0.1 * G.N_RAYS
    se = f["self_err"][~f["marked"]]
    assert se.max() < 1e-10
    counts = np.bincount(f["hit"], minlength=5)
    if name in G.LENS:
        assert counts[0] == 0 and (counts[1:] >= 5).all(), counts
        assert np.isinf(f["lambda_exit"]).all()                       # the valid box holds every ray, the sky and the time range
        assert all(lo < -6.0 and hi > 6.0 for lo, hi in box[-3:])
        assert (np.abs(f["state0"][:, :4]).max() < 6.0) and min(margin(name, s) for s in f["state0"]) > 0
    else:
        ev = (f["hit"] > 0) & ~f["marked"]
        assert ev.sum() >= 15 and (f["hit"] == 0).sum() >= 15, counts
        assert np.isfinite(f["lambda_exit"][f["hit"] == 0]).all() and counts[PLANE] == 0
        assert len({(round(lo, 6), round(hi, 6)) for lo, hi in box[-3:]} | {(-hi, -lo) for lo, hi in box[-3:]}) == 6   # differs on every axis
        # every object strictly inside the box (spheres: centre +- radius; the disk: +- r_out, +- h)
        for o in (sc.obj[k] for k in range(sc.nobj)):
            if o.kind == abi.SPHERE:
                ext = [(o.p[1 + a] - abs(o.p[8]), o.p[1 + a] + abs(o.p[8])) for a in range(3)]
            elif o.kind == abi.DISK:
                ext = [(-o.p[2], o.p[2]), (-o.p[2], o.p[2]), (-o.p[0], o.p[0])]
            else:
                assert o.kind == abi.PLANE and o.p[0] < f["state_end"][:, 0].min() - 100      # a time no ray reaches
                continue
            assert all(lo < e0 and e1 < hi for (lo, hi), (e0, e1) in zip(box[-3:], ext)), (o.kind, ext)
        if dim == 4:   # the time range ends early: some rays leave through it, inside the spatial box
            import truth
            assert sum(truth.box_margin(box[1:], s) > 1e-6 for s in f["state_exit"][f["hit"] == 0]) >= 5


@pytest.mark.parametrize("name", G.NAMES)
def test_grid_truth_fixture_regenerates(name):
    """Three rays of each fixture integrated again (test_truth_fixture_regenerates' bars): the committed vectors are what
    tests/grid_truth.py computes, and the stored start states are truth.pixel_state's for the stored pixels."""
    import truth
    f = fixture(name)
    sc, cam = G.truth_scene(name)
    for k in (0, 27, 60):
        i, j = (int(v) for v in f["ij"][k])
        s0 = truth.pixel_state(sc, cam, int(f["n"][0]), int(f["n"][1]), i, j, metric_fn=G.metric_at(f["coef"]))
        assert np.abs(s0 - f["state0"][k]).max() < 1e-15
        r = G.trace_truth(name, f["coef"], s0)
        assert r["hit"] == f["hit"][k]
        assert np.abs(r["state_end"] - f["state_end"][k]).max() < 1e-12
        assert np.abs(r["rgb"] - f["rgb"][k]).max() < 1e-12
        assert r["lambda_exit"] == f["lambda_exit"][k] or abs(r["lambda_exit"] - f["lambda_exit"][k]) < 1e-12


@pytest.mark.parametrize("name", G.NAMES)
def test_the_interpolant_of_the_samples_is_the_polynomial(name):
    """The statement that makes the polynomial's geodesics the truth of the interpolated field: the numpy Catmull-Rom that
    include/rtgr.h specifies (and test_interpolant_is_the_one_specified pins the device to), applied to the rebuilt samples, equals
    the polynomial and its symbolic derivatives to 1e-13 x the data's scale — inside the valid box, and with one axis up to three
    cells outside it (beyond the table's last sample), where the clamped cell extrapolates.
    The data's scale: max |g| for the values; max |g| / min h for the derivatives, which are sums of samples times weights / h —
    their rounding error follows the samples' size, not the (here small) derivative's.
    One axis at a time: three cells out the four weights are -18, 57, -62, 24 — the sum cancels to 1 from a magnitude of 161, and
    every further extrapolating axis multiplies the rounding error by that (all four axes three cells out: 1e-9, in numpy as on
    the device); a ray's stages leave the box by a fraction of a step, the field itself is exact there as anywhere."""
    f, grid = fixture(name), G.GRIDS[name]
    dim = grid["dim"]
    rng = np.random.default_rng(31)
    box = np.array(G.valid_box(grid))
    h = np.array(grid["spacing"])
    n = 300
    pts = box[:, 0] + rng.uniform(size=(n, dim)) * (box[:, 1] - box[:, 0])
    ax = rng.integers(dim, size=n)
    out = rng.uniform(0, 3, size=n) * h[ax]
    side = rng.integers(2, size=n)
    moved = np.where(side == 0, box[ax, 0] - out, box[ax, 1] + out)
    pts[n // 3:][np.arange(n - n // 3), ax[n // 3:]] = moved[n // 3:]
    assert (np.abs(pts[:, -3:]).max(axis=0) > np.abs(np.array(grid["origin"][-3:]) + (np.array(grid["n"][-3:]) - 1) * h[-3:]).min()).any()
    x4 = pts if dim == 4 else np.concatenate([np.zeros((n, 1)), pts], axis=1)
    fn = G.field_fn(f["coef"])
    want = [fn(p) for p in x4]
    g = np.array([w[0] for w in want])
    dg = np.array([w[1] for w in want])                      # dg[n, b, a, c] = d_b g_ac
    if dim == 3:
        got_g, got_dg = catmull_rom(grid_samples(name), grid["origin"], grid["spacing"], pts)
        dg = dg[:, 1:]
    else:
        got_g, got_dg = catmull_rom4(grid_samples(name), grid["origin"], grid["spacing"], pts)
        assert np.abs(dg[:, 0]).max() > 1e-3
    for c, (p, q) in enumerate(G.UPPER):
        assert np.abs(got_g[:, c] - g[:, p, q]).max() <= 1e-13 * np.abs(g).max(), (c, np.abs(got_g[:, c] - g[:, p, q]).max())
        assert np.abs(got_dg[:, :, c] - dg[:, :, p, q]).max() <= 1e-13 * np.abs(g).max() / h.min(), (c, np.abs(got_dg[:, :, c] - dg[:, :, p, q]).max())


def test_oracle_rhs_of_the_polynomial_is_the_symbolic_one():
    """The oracle's dual-number chain on the polynomial (d_t g included) against grid_truth.rhs at random states."""
    import oracle_lib as O
    coef = G.field_table(4)
    O.set_polynomial(coef)
    sc, _ = G.truth_scene("quad4")
    rng = np.random.default_rng(32)
    s = np.concatenate([rng.uniform(-7, 0, (64, 1)), rng.uniform(-5, 5, (64, 3)), rng.uniform(-1, 1, (64, 4))], axis=1)
    ref = O.geodesic(sc, s, long_double=True)
    f = G.rhs(coef)
    got = np.array([f(0.0, v) for v in s])
    assert (np.abs(got - ref) / np.abs(ref).max(axis=1, keepdims=True)).max() < 1e-12
    frozen = coef.copy()
    frozen[:, 10:] = 0
    f0 = G.rhs(frozen)
    assert np.abs(np.array([f0(0.0, v) for v in s]) - ref).max() > 1e-4          # (the terms in t are felt)


@pytest.mark.parametrize("name", G.NAMES)
def test_oracle_on_the_polynomial_against_true_geodesics(name):
    """The same algorithm the kernels run (Tsit5 at 2^-39, the sampled event scan) on the same field, without a grid: its global
    error on these rays is inside test_truth.py's bars — shown before any GPU run.  The oracle knows no box, so in the box scenes
    only the rays whose true geodesic ends in an event (before leaving) are traced."""
    import oracle_lib as O
    f = fixture(name)
    O.set_polynomial(f["coef"])
    sc, _ = G.truth_scene(name)
    sel = np.flatnonzero(~f["marked"] & (f["hit"] > 0))
    r = O.trace(sc, rt.solver_defaults(), len(sel), 1, state0=f["state0"][sel])
    assert (r["status"] == abi.RAY_EVENT).all()
    worst = _check_against_truth(name, *subset(r, f, sel, np.arange(len(sel))), min_sphere_rays=30 if name in G.LENS else 15, nobj=sc.nobj)
    print(f"[grid truth] oracle {name}: max |state_end - truth| {worst[0]:.2e}, rgb {worst[1]:.2e} (bar {TOL_SPHERE:.0e})")


# ---- the teeth: what a wrong axis would do --------------------------------------------------------------------------------------------
def stretched(name):
    """(axis of (t, x, y, z), origin, factor): fixture `name`'s grid with its y spacing (3-D) or its time spacing (4-D) declared
    1e-6 too large"""
    grid = G.GRIDS[name]
    ax = 2 if grid["dim"] == 3 else 0
    return ax, grid["origin"][ax - (4 - grid["dim"])], 1.0 + STRETCH


@functools.lru_cache(maxsize=None)
def stretched_truth(name):
    """the first TEETH_RAYS unmarked sky-sphere rays of a lens fixture through the STRETCHED polynomial: (ray indices, end states)"""
    f = fixture(name)
    rays = np.flatnonzero(~f["marked"] & (f["hit"] == 1))[:TEETH_RAYS]
    ends = []
    for k in rays:
        r = G.trace_truth(name, f["coef"], f["state0"][k], stretch=stretched(name))
        assert r["hit"] == 1
        ends.append(r["state_end"])
    return rays, np.array(ends)


@pytest.mark.parametrize("name", G.LENS)
def test_a_spacing_wrong_by_1e_6_moves_the_true_rays_by_100_bars(name):
    f = fixture(name)
    rays, ends = stretched_truth(name)
    moved = np.abs(ends - f["state_end"][rays]).max(axis=1)
    print(f"[grid truth] {name}: a spacing 1e-6 too large moves the end states by {moved.min():.2e} .. {moved.max():.2e}")
    assert (moved >= 100 * TOL_SPHERE).sum() > len(rays) // 2, moved


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


@functools.lru_cache(maxsize=None)
def grid_metric(name, wrong=False):
    grid = G.GRIDS[name]
    spacing = list(grid["spacing"])
    if wrong:
        spacing[stretched(name)[0] - (4 - grid["dim"])] *= stretched(name)[2]
    return rt.GridMetric(grid_samples(name), grid["origin"], spacing, name=name + (" (stretched)" if wrong else ""))


def ragged(state0):
    """the 64 rays and a 65th — a copy of the first: a lane pair and a wave are both half-filled"""
    return np.concatenate([state0, state0[:1]], axis=0)


def hip_rays(lib, name, dtype=np.float64, split=None, state0=None, wrong=False):
    """the fixture's rays (ragged) through the fixture's grid, by state0"""
    from test_gpu_parity import hip_trace
    s0 = ragged(fixture(name)["state0"]) if state0 is None else state0
    sc = rt.make_scene(grid_metric(name, wrong), G.objects(name))
    opt = rt.solver_defaults(dtype)
    if split is None:
        return hip_trace(lib, sc, opt, len(s0), 1, state0=s0, dtype=dtype)
    with abi.options(lib, split=split):
        return hip_trace(lib, sc, opt, len(s0), 1, state0=s0, dtype=dtype)


_F64_LENS = {}


def f64_lens(lib, name, split):
    if (name, split) not in _F64_LENS:
        _F64_LENS[name, split] = hip_rays(lib, name, split=split)
    return _F64_LENS[name, split]


def check_copy(r):
    """the 65th ray is the first one to the bit"""
    for k in OUTPUTS:
        a = r[k][:, 64] if k == "rgb" else r[k][64]
        b = r[k][:, 0] if k == "rgb" else r[k][0]
        assert np.array_equal(a, b), k


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 1])
@pytest.mark.parametrize("name", G.LENS)
def test_hip_grid_global_error_against_true_geodesics(lib, name, split):
    """tu_f64_grid / tu_f64_grid4, FULL (split = 0) and FAR + NEAR (split = 1): every ray ends in an event, none OUTSIDE; hit, end
    state, lambda_end and RGB within test_truth.py's bars of the true geodesics."""
    f = fixture(name)
    r = f64_lens(lib, name, split)
    assert (r["status"] == abi.RAY_EVENT).all()
    check_copy(r)
    worst = _check_against_truth(name, *subset(r, f, ~f["marked"]), nobj=4)
    print(f"[grid truth] f64 {name} split={split}: max |state_end - truth| {worst[0]:.2e}, rgb {worst[1]:.2e} (bar {TOL_SPHERE:.0e})")


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.LENS)
def test_hip_grid_pass_structures_give_identical_bits(lib, name):
    full, pair = f64_lens(lib, name, 0), f64_lens(lib, name, 1)
    for k in OUTPUTS:
        assert np.array_equal(full[k], pair[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.LENS)
def test_hip_float32_grid_global_error_against_true_geodesics(lib, name):
    """tu_f32_grid / tu_f32_grid4 with the Float32 tables, at tol = eps(Float32)^(3/4): the bars of
    test_hip_float32_global_error_against_true_geodesics."""
    f = fixture(name)
    r = hip_rays(lib, name, dtype=np.float32)
    assert (r["status"] == abi.RAY_EVENT).all()
    check_copy(r)
    worst = _check_against_truth(name, *subset(r, f, ~f["marked"]), nobj=4, **F32_BARS)
    print(f"[grid truth] f32 {name}: max |state_end - truth| {worst[0]:.2e}, rgb {worst[1]:.2e} (bar {F32_BARS['tol_sphere']:.0e})")


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.LENS)
def test_hip_camera_on_an_anisotropic_grid(lib, name):
    """The prepare kernel's camera on a sampled metric: a ragged 9 x 7 frame through `cam` whose pixels shared with the fixture (16 or more)
    start where the fixture's rays start (1e-15 x scale), end within the bars of their true geodesics, and whose traced outputs
    are, bit for bit, those of the same start states traced through state0."""
    from test_gpu_parity import hip_trace
    f = fixture(name)
    ni, nj = G.SMALL_FRAME
    m = grid_metric(name)
    c = rt.make_canvas(m, ni=ni, nj=nj, **G.CAMERA)
    st = np.concatenate([c.pixels.reshape(-1, order="F")["pos"], c.pixels.reshape(-1, order="F")["normal"]], axis=1)
    shared = [k for k in range(G.N_RAYS) if f["ij"][k, 0] % 5 == 2 and f["ij"][k, 1] % 5 == 2]
    p = np.array([(f["ij"][k, 0] - 2) // 5 + ni * ((f["ij"][k, 1] - 2) // 5) for k in shared])
    assert len(shared) >= 16 and len(set(p)) == len(shared)
    assert np.abs(st[p] - f["state0"][shared]).max() <= 1e-15 * np.abs(f["state0"][shared]).max()
    sc, opt = rt.make_scene(m, G.objects(name)), rt.solver_defaults()
    by_cam = hip_trace(lib, sc, opt, ni, nj, cam=rt.make_camera(**G.CAMERA))
    by_state = hip_trace(lib, sc, opt, ni * nj, 1, state0=st)
    for k in OUTPUTS:
        assert np.array_equal(by_cam[k], by_state[k]), k
    keep = np.array([not f["marked"][k] for k in shared])
    assert keep.sum() >= 12
    _check_against_truth(name, *subset(by_cam, f, np.array(shared)[keep], p[keep]), min_sphere_rays=8, nobj=4)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", G.BOX)
def test_hip_grid_box_rule_against_true_geodesics(lib, name, dtype):
    """The `inside` rule after an accepted step, on a box that differs on every axis (and ends early in t): on the unmarked rays the
    status is RAY_EVENT exactly where the true geodesic meets an object before it leaves, within the bars; every other ray ends
    RAY_OUTSIDE, not before the true geodesic leaves, with its end outside the box on some axis; the end of that last step — whose
    stages read the clamped outer cells and extrapolate — is the true geodesic at the device's own lambda_end to the sphere bar."""
    f = fixture(name)
    bars = {} if dtype == np.float64 else F32_BARS
    tol = bars.get("tol_sphere", TOL_SPHERE)
    r = hip_rays(lib, name, dtype=dtype)
    check_copy(r)
    assert r["counters"]["not_finished"] == int((r["status"] == abi.RAY_OUTSIDE).sum())
    r = {k: (v[:, :64] if k == "rgb" else v[:64]) if isinstance(v, np.ndarray) else v for k, v in r.items()}
    ok = ~f["marked"]
    event = f["hit"] > 0
    assert np.isin(r["status"], (abi.RAY_EVENT, abi.RAY_OUTSIDE)).all()
    assert np.array_equal(r["status"][ok] == abi.RAY_EVENT, event[ok]), np.flatnonzero(ok & ((r["status"] == abi.RAY_EVENT) != event))
    worst = _check_against_truth(name, *subset(r, f, ok & event), min_sphere_rays=15, nobj=4, **bars)
    out = r["status"] == abi.RAY_OUTSIDE
    print(f"[grid truth] {np.dtype(dtype).name} {name}: min (lambda_end - true lambda_exit) {(r['lambda_end'][out] - f['lambda_exit'][out]).min():.3e}")
    assert (r["lambda_end"][out] >= f["lambda_exit"][out]).all()
    assert all(margin(name, s.astype(np.float64)) < 0 for s in r["state_end"][out])
    errs = []
    for k in np.flatnonzero(out & ok)[::max(1, int((out & ok).sum()) // 8)][:8]:
        t = G.trace_truth(name, f["coef"], f["state0"][k], lambda1=float(r["lambda_end"][k]))
        errs.append(np.abs(r["state_end"][k] - t["state_end"]).max())
    assert len(errs) == 8 and max(errs) <= tol, errs
    print(f"[grid truth] {np.dtype(dtype).name} {name}: events max |state_end - truth| {worst[0]:.2e}, rgb {worst[1]:.2e}; "
          f"OUTSIDE ends {max(errs):.2e} (bar {tol:.0e}); {int(out.sum())} OUTSIDE")
    # a start outside the box — in t for the 4-D grid — ends before its first step
    box = G.valid_box(G.GRIDS[name])
    s0 = np.repeat(f["state0"][:1], 3, axis=0)
    s0[1, 1] = box[-3][1] + 0.25
    if len(box) == 4:
        s0[2, 0] = box[0][1] + 0.25
    else:
        s0[2, 3] = box[-1][0] - 0.25
    o = hip_rays(lib, name, dtype=dtype, state0=s0)
    assert o["status"][0] == r["status"][0] and o["n_accept"][0] == r["n_accept"][0] > 0
    assert (o["status"][1:] == abi.RAY_OUTSIDE).all() and (o["n_accept"][1:] == 0).all() and o["counters"]["not_finished"] >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", G.LENS)
def test_hip_grid_check_has_teeth(lib, name):
    """The same samples loaded with one spacing (y; the time axis of the 4-D grid) declared 1e-6 too large: the device's field is
    the polynomial stretched along that axis.  Its rays follow the STRETCHED truth to the bar, and the check against the fixture
    then fails on the rays that the CPU test above shows to move by >= 100 bars."""
    f = fixture(name)
    rays, ends = stretched_truth(name)
    r = hip_rays(lib, name, wrong=True)
    assert np.abs(r["state_end"][rays] - ends).max() <= TOL_SPHERE
    off = np.abs(r["state_end"][rays] - f["state_end"][rays]).max(axis=1)
    assert (off > TOL_SPHERE).sum() > len(rays) // 2, off
    with pytest.raises(AssertionError):
        _check_against_truth(name, *subset(r, f, ~f["marked"]), nobj=4)
