"""Volume emission (include/rtgr.h "volume emission"): the flow model, the transfer integration and the frame rule.

CPU: the symbols and the layout, the truth side held to itself (tests/transfer_truth.py: the DOP853 truth, the Tsit5 twin) and to the
fixture tests/golden/truth_transfer.npz, and three exact statements.  GPU: rtgr_eval_flow_* against the numpy restatement,
rtgr_eval_transfer_* against the truth with the twin's own error as the yardstick, the identities on the device, frame == hook ==
observer trace bit for bit, composition with an emitting disk, capture, the contract of the arrays, the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import transfer_truth as tt
import truth as T
from conftest import ROOT
from scenes import rt

abi = rt._abi
EXPORTS = tuple(f"rtgr_{n}_{s}" for n in ("trace_transfer_device", "trace_transfer", "eval_transfer", "eval_flow") for s in ("f64", "f32"))
EPS64, EPS32 = tt.EPS64, tt.EPS32
FIXTURE = os.path.join(ROOT, "tests", "golden", "truth_transfer.npz")
FLOOR = 3e-11          # the project's true-geodesic bound (tests/test_truth.py), relative to max |truth|
TWIN_FACTOR = 4.0      # DESIGN.md §4.19's rule: the kernel may err 4 x what a solver of its own kind does
REL_STEP_DIFF = 0.015  # tests/test_gpu_parity.py: the step margin of HIP against its CPU restatement
MODEL_RTOL = 1e-10     # tests/test_emission.py: Omega and u_emit of the hook against numpy


def fixture():
    return np.load(FIXTURE)


def fx_flow(fx, kap, i):
    orbit, r0, alpha, H, s = fx["flow"]
    return dict(emitter=tt.KEPLER, orbit=float(orbit), j0=float(fx["j0"]), kappa=float(fx["kappas"][kap]), r0=float(r0), alpha=float(alpha), H=float(H),
                s=float(s), r_stop=float(fx["r_stop"][i]))


def rt_flow(fl, **kw):
    d = dict(fl)
    d["emitter"] = {tt.KEPLER: "kepler", tt.RIGID: "rigid"}[d["emitter"]]
    d.update(kw)
    return rt.Flow(**d)


def fx_scene(name):
    return {"ks_true09": (tt.Scene("ks_true", 1.0, 0.9), rt.KerrSchild(1, 0.9)), "ks_ref0": (tt.Scene("ks_ref", 1.0, 0.0), rt.kerr_schild)}[name]


def opt_dict(tol, lambda1, max_steps=100000):
    return dict(reltol=tol, abstol=tol, lambda0=0.0, lambda1=lambda1, max_steps=max_steps)


def rt_opt(dtype, lambda1, max_steps=None):
    o = rt.solver_defaults(dtype)
    o.lambda1 = lambda1
    if max_steps is not None:
        o.max_steps = max_steps
    return o


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_declared_and_exported():
    assert set(EXPORTS) <= set(abi.EXPORTS) and len(EXPORTS) == 8
    lib = abi.load()
    hdr = open(os.path.join(ROOT, "include", "rtgr.h")).read()
    for s in EXPORTS:
        assert hasattr(lib, s), s
        assert s + "(" in hdr, s
    assert "#define RTGR_ABI_VERSION 4" in hdr and lib.rtgr_abi_version() == 4     # additive: no existing layout moved
    assert {"Flow", "trace_transfer", "eval_transfer", "eval_flow"} <= set(rt.api.__all__)
    # the Julia module binds the host-pointer entries of the frame and of the listed rays, each by a ccall (tests/test_julia_stub.py holds
    # every ccall against its C prototype), the record and the three names
    jl = open(os.path.join(ROOT, "julia", "RayTraceGRHIP.jl")).read()
    for s in ("rtgr_trace_transfer_f64", "rtgr_trace_transfer_f32", "rtgr_eval_transfer_f64", "rtgr_eval_transfer_f32"):
        assert f"ccall((:{s}, librtgr)" in jl, s
    assert "_device_" not in "".join(l for l in jl.splitlines() if "rtgr_trace_transfer" in l)
    for word in ("struct RtgrFlow", "function Flow(", "function trace_rays_transfer(", "function eval_transfer(",
                 "#   RtgrFlow        104   emitter 0, flags 4, orbit 8, j0 16, kappa 24, r0 32, alpha 40, H 48, s 56, r_stop 64, gain 72, weight 80"):
        assert word in jl, word
    body = jl.split("struct RtgrFlow", 1)[1].split("\nend", 1)[0]
    import re
    assert re.findall(r"^\s+([A-Za-z_0-9]+)::", body, re.M) == [n for n, _ in abi.rtgr_flow._fields_]
    for words in ("volume emission", "dtau/dlambda = kappa n w", "A LIMITATION OF THE MODEL, kappa > 0", "their rgb is NaN", "CHOOSE r_stop INSIDE THE DARK CYLINDER", "plunging gas", "polarized transfer",
                  "104 bytes: emitter 0, flags 4, orbit 8, j0 16, kappa 24, r0 32, alpha 40, H 48, s 56, r_stop 64, gain 72, weight 80"):
        assert words in hdr, words


def test_struct_layout_ctypes_and_c(tmp_path):
    s = abi.rtgr_flow
    names = ("emitter", "flags", "orbit", "j0", "kappa", "r0", "alpha", "H", "s", "r_stop", "gain", "weight")
    want = [0, 4, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80]
    assert C.sizeof(s) == 104 and [getattr(s, f).offset for f in names] == want
    exe = str(tmp_path / "transfer_layout")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "transfer_layout.c"), "-o", exe])
    assert [int(v) for v in subprocess.check_output([exe]).split()] == [104] + want
    f = rt.Flow(0.5, kappa=0.1, r0=4, alpha=1.5, H=0.4, s=0.5, r_stop=1.75, orbit=-1, weight=(1, 2, 3))
    assert (f.emitter, f.flags, f.orbit, f.j0, f.kappa, f.r0, f.alpha, f.H, f.s, f.r_stop, f.gain, list(f.weight)) == \
        (abi.EMIT_KEPLER, 0, -1.0, 0.5, 0.1, 4.0, 1.5, 0.4, 0.5, 1.75, 1.0, [1, 2, 3])
    with pytest.raises(ValueError):
        rt.Flow(1.0, emitter="keplerian")


@pytest.mark.parametrize("kind,a", [("ks_true", 0.9), ("ks_ref", 0.0), ("ks_ref", 0.8)])
def test_the_fast_metric_is_truths_symbolic_metric(kind, a):
    """transfer_truth._metric64 takes truth.metric_expr apart as eta + f k k^T (16 small derivatives instead of 64 expanded ones); it
    and the geodesic right-hand side built on it are truth._metric_fn's and truth.rhs's to rounding"""
    rng = np.random.default_rng(5)
    sc = tt.Scene(kind, 1.0, a)
    geo, f10 = T.rhs(sc), tt.rhs10(sc, tt.flow_params(j0=0.0), 1.0)
    for _ in range(20):
        p = np.concatenate([[0.3], rng.uniform(-1, 1, 3) * rng.uniform(2.5, 30)])
        g, dg = tt._metric(kind, 1.0, a, p, np.float64)
        g2, dg2 = T._metric_fn(kind)(p[1], p[2], p[3], 1.0, a)
        assert np.abs(g - g2).max() <= 64 * EPS64 * np.abs(g2).max() and np.abs(dg - dg2).max() <= 256 * EPS64 * np.abs(dg2).max()
        y = np.concatenate([p, rng.uniform(-1, 1, 4)])
        r1, r2 = f10(0.0, np.concatenate([y, [0.0, 0.0]]))[:8], geo(0.0, y)
        assert np.abs(r1 - r2).max() <= 1e-12 * max(1.0, np.abs(r2).max())


def test_the_fixture_holds_what_the_issue_lists_and_is_small():
    fx = fixture()
    assert os.path.getsize(FIXTURE) < 1 << 20
    names = list(fx["scene"])
    assert names.count("ks_true09") == 12 and names.count("ks_ref0") == 4
    cap = fx["captured"]
    assert cap[np.array(names) == "ks_true09"].sum() >= 1 and fx["truth_stopped"][0][cap].all() and not fx["truth_stopped"][0][~cap].any()
    assert fx["kappas"][0] == 0.0 and fx["kappas"][1] > 0.0
    assert 0.3 <= np.nanmax(fx["truth_I"]) <= 3.0, "j0 makes max I of order 1"
    assert (fx["truth_tau"][0] == 0.0).all() and 0.3 <= np.nanmax(fx["truth_tau"][1]) <= 3.0
    # kappa > 0 on a ray that crosses the photon orbit's cylinder inside the gas: dtau/dlambda = kappa n w is unbounded there (w ~ 1 / sqrt(-n2),
    # integrable), DOP853 gives up at rtol 1e-13 and the twin's step underflows (status 3).  Those runs have no truth; every other run has one
    no_truth = np.isnan(fx["truth_I"])
    assert not no_truth[0].any() and np.array_equal(no_truth[1], fx["twin64_status"][1] == 3) and 1 <= no_truth[1].sum() <= 6
    assert no_truth[1][cap].sum() >= 2 and not no_truth[1][[0, 1, 2, 3, 12, 13]].any()
    # the two grazing rays are the longest of those that escape
    lam = np.where(cap, 0.0, fx["lambda_end"])[:12]
    assert set(np.argsort(lam)[-2:]) == {8, 9}
    # the twin is a solver of the tolerance it was given: its error is small against the truth, and not zero
    scale = np.nanmax(np.abs(fx["truth_I"]))
    assert 0 < np.nanmax(fx["twin64_err_I"]) <= 1e-7 * scale and np.nanmax(fx["twin32_err_I"]) <= 3e-2 * scale
    assert (fx["twin64_status"][0, cap] == 1).all() and (fx["twin64_status"][0, ~cap] == 0).all()
    # … recorded over the ensemble of start states one ulp apart, which holds the unperturbed run
    for tag in ("twin64", "twin32"):
        has = np.isfinite(fx["truth_I"])
        assert (fx[f"{tag}_err_I"][has] >= fx[f"{tag}_err1_I"][has]).all()


@pytest.mark.parametrize("i,kap", [(0, 0), (2, 1), (12, 0), (13, 1)])
def test_the_fixture_is_what_the_truth_side_computes(i, kap):
    """two rays of each scene recomputed: the DOP853 truth and both twins give the recorded numbers"""
    fx = fixture()
    name = str(fx["scene"][i])
    sc, _ = fx_scene(name)
    fl, s0, le = fx_flow(fx, kap, i), fx["s0"][i], float(fx["lambda_end"][i])
    tr = tt.truth(sc, fl, s0, le)
    assert abs(tr["I"] - fx["truth_I"][kap, i]) <= 1e-13 * max(1.0, abs(tr["I"])) and abs(tr["tau"] - fx["truth_tau"][kap, i]) <= 1e-13
    assert np.abs(tr["s_end"] - fx["truth_s_end"][kap, i]).max() <= 1e-11
    t64 = tt.twin(sc, fl, s0, le, opt_dict(float(fx["tol64"]), float(fx["lambda1"])))
    assert abs(t64["I"] - fx["twin64_I"][kap, i]) <= 1e-13 and abs(t64["tau"] - fx["twin64_tau"][kap, i]) <= 1e-13
    assert abs(int(t64["steps"]) - int(fx["twin64_steps"][kap, i])) <= 1
    t32 = tt.twin(sc, fl, s0.astype(np.float32), np.float32(le), opt_dict(float(fx["tol32"]), float(fx["lambda1"])), dt=np.float32)
    assert abs(float(t32["I"]) - float(fx["twin32_I"][kap, i])) <= 1e-6 and abs(int(t32["steps"]) - int(fx["twin32_steps"][kap, i])) <= 1


# a straight ray through flat space: from (t, x, y, z) = (0, 9, -3, 0.4) along a null direction that passes the axis at rho ~ 1.3
FLAT_S0 = np.array([0.0, 9.0, -3.0, 0.4, -1.0, -0.9, 0.42, -0.03])
FLAT_S0[4] = -np.linalg.norm(FLAT_S0[5:])
FLAT_END = 18.0


def flat_integrand(fl, kappa0):
    """dI/dlambda at tau = 0 along FLAT_S0 in closed special-relativistic form: u_f = gamma (1, -Omega y, Omega x, 0), gamma =
    1 / sqrt(1 - Omega² rho²), w = -k^t gamma + gamma Omega (x k^y - y k^x)"""
    om = fl["orbit"]

    def f(lam):
        x = FLAT_S0[1:4] + lam * FLAT_S0[5:8]
        rho2 = x[0] ** 2 + x[1] ** 2
        if not om * om * rho2 < 1:
            return 0.0
        gam = 1 / np.sqrt(1 - om * om * rho2)
        w = gam * (-FLAT_S0[4] + om * (x[0] * FLAT_S0[6] - x[1] * FLAT_S0[5]))
        n = (np.sqrt(rho2 + x[2] ** 2) / fl["r0"]) ** (-fl["alpha"]) * np.exp(-x[2] ** 2 / (2 * fl["H"] ** 2 * rho2))
        gf = kappa0 / w
        return fl["j0"] * n * w * gf ** (3 + fl["s"]) if gf > 0 else 0.0
    return f


FLAT_RIGID0 = tt.flow_params(emitter=tt.RIGID, orbit=0.0, j0=0.7, kappa=0.3, r0=2.0, alpha=1.2, H=0.5, s=0.8)
FLAT_THIN = tt.flow_params(emitter=tt.RIGID, orbit=0.05, j0=0.7, kappa=0.0, r0=2.0, alpha=1.2, H=0.5, s=0.8)


def flat_quad(fl):
    from scipy.integrate import quad
    k0 = tt.kappa0_of(tt.Scene("mink"), FLAT_S0)
    val, err = quad(flat_integrand(fl, k0), 0.0, FLAT_END, epsabs=1e-14, epsrel=1e-14, limit=400)
    return val


def test_three_exact_statements_on_the_truth_and_the_twin():
    sc = tt.Scene("mink")
    o = opt_dict(EPS64 ** 0.75, 100.0)
    # flat space, gas at rest, any s: w is constant and gfac = 1, so dI = (j0 / kappa) exp(-tau) dtau
    for res, tol in ((tt.truth(sc, FLAT_RIGID0, FLAT_S0, FLAT_END), 1e-12), (tt.twin(sc, FLAT_RIGID0, FLAT_S0, FLAT_END, o), 1e-9)):
        assert res["tau"] > 0.1
        want = FLAT_RIGID0["j0"] / FLAT_RIGID0["kappa"] * -np.expm1(-res["tau"])
        assert abs(res["I"] - want) <= tol * want
    # kappa = 0: tau stays 0 exactly
    thin_truth, thin_twin = tt.truth(sc, FLAT_THIN, FLAT_S0, FLAT_END), tt.twin(sc, FLAT_THIN, FLAT_S0, FLAT_END, o)
    assert thin_truth["tau"] == 0.0 and thin_twin["tau"] == 0.0
    # flat space, rigid rotation: the integral of the closed integrand
    want = flat_quad(FLAT_THIN)
    assert want > 0.05 and abs(thin_truth["I"] - want) <= 1e-12 * want and abs(thin_twin["I"] - want) <= 1e-9 * want


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


def model_points(sc, a):
    """~200 points s = (x, k) and the start states of their rays: a shell of random points, the plane z = 0, the axis, the origin, rho just
    inside and outside the prograde photon orbit's cylinder, r = 1e4"""
    rng = np.random.default_rng(11)
    pts = []
    for _ in range(150):
        r = rng.uniform(1.2, 30.0)
        v = rng.normal(size=3)
        pts.append(r * v / np.linalg.norm(v))
    # (rings in the plane z = 0: 2 and 3 lie inside the retrograde orbit's dark cylinder, rho < 4.01, the other four outside both)
    for rho in (2.0, 3.0, 4.5, 6.0, 9.0, 15.0):
        for phi in (0.3, 2.1, -1.2):
            pts.append([rho * np.cos(phi), rho * np.sin(phi), 0.0])
    rph = 2 * (1 + np.cos(2 / 3 * np.arccos(-a)))
    cyl = np.sqrt(rph * rph + a * a)
    pts += [[0, 0, 2.5], [0, 0, -7.0], [0, 0, 0], [cyl - 0.01, 0, 0.3], [cyl + 0.01, 0, 0.3], [0, cyl - 0.01, 0], [0, cyl + 0.01, 0], [6e3, 8e3, 10.0],
            [1e4, 0, 0], [0.4, 0.3, 1.9], [0.5, -0.2, 0.1]]
    pts = np.array(pts, np.float64)
    pos = np.array([0, 40 * np.sin(np.pi / 3), 0, 40 * np.cos(np.pi / 3)])
    s0 = np.array([tt.camera_state(sc, pos, -pos[1:] / 40 + 0.2 * rng.normal(size=3)) for _ in pts])
    s = np.concatenate([np.full((len(pts), 1), 0.7), pts, s0[:, 4:] * rng.uniform(0.5, 2.0, (len(pts), 1))], axis=1)
    return s0, s


@pytest.mark.gpu
@pytest.mark.parametrize("orbit", [+1, -1])
def test_model_pointwise_against_numpy_and_the_disks_rate(lib, orbit):
    a = 0.9
    sc, metric = tt.Scene("ks_true", 1.0, a), rt.KerrSchild(1, a)
    s0, s = model_points(sc, a)
    fl = tt.flow_params(orbit=float(orbit), j0=0.6, kappa=0.2, r0=4.0, alpha=1.5, H=0.4, s=0.5)
    got = rt.eval_flow(metric, [], rt_flow(fl), s0, s)
    want = [tt.flow_point(sc, fl, tt.kappa0_of(sc, s0[i]), s[i]) for i in range(len(s))]
    valid = np.array([w["valid"] for w in want])
    assert 100 <= valid.sum() < len(s)     # (the retrograde orbit's dark cylinder is the wider one)
    assert np.array_equal(np.isfinite(got["omega"]), valid) and np.array_equal(np.isfinite(got["u_f"]).all(axis=1), valid), "invalid points are flagged exactly"
    assert np.array_equal(np.isfinite(got["gfac"]), valid) and (got["dtau"][~valid] == 0).all() and (got["dI0"][~valid] == 0).all()
    col = lambda k: np.array([w[k] for w in want], np.float64)
    rel = lambda g_, w_: float(np.max(np.abs(g_ - w_) / np.abs(w_))) if len(w_) else 0.0
    uf = np.array([w["u_f"] for w in want])
    errs = dict(omega=rel(got["omega"][valid], col("omega")[valid]), u_f=float(np.max(np.abs(got["u_f"][valid] - uf[valid]) / np.abs(uf[valid][:, :1]))),
                gfac=rel(got["gfac"][valid], col("gfac")[valid]))
    dens = col("dens")
    pos_d = dens > 0
    errs["dens"] = rel(got["dens"][pos_d], dens[pos_d])
    glow = valid & (col("dI0") > 0)
    errs["dtau"], errs["dI0"] = rel(got["dtau"][glow], col("dtau")[glow]), rel(got["dI0"][glow], col("dI0")[glow])
    print(f"orbit {orbit:+d}: {valid.sum()} valid of {len(s)}, {glow.sum()} glow; rel err " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert (got["dens"][~pos_d] == 0).all() and glow.sum() >= 80
    assert all(errs[k] <= MODEL_RTOL for k in ("omega", "u_f", "gfac", "dens")) and errs["dtau"] <= 10 * MODEL_RTOL and errs["dI0"] <= 10 * MODEL_RTOL
    # at z = 0 the flow's rate and 4-velocity are the disk's, bit for bit
    flat = (s[:, 3] == 0.0) & valid
    assert flat.sum() >= 12
    em = rt.DiskEmission(1, 6000.0, orbit=orbit)
    disk = rt.eval_disk_emission(metric, [rt.Disk(0.05, 1.5, 2e4)], em, s0[flat], s[flat])
    assert disk["omega"].tobytes() == got["omega"][flat].tobytes() and disk["u_emit"].tobytes() == got["u_f"][flat].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_integration_against_the_truth(lib, dtype):
    """|I - I_truth| <= max(3e-11 max|I_truth| [x eps32 / eps64 in Float32], 4 x the twin's recorded error), likewise tau; the step
    attempts within the suite's relative margin of the twin's, or the twin's own step noise where that is larger.  The twin's recorded error is its largest over a nine-member ensemble
    (start states one ulp apart: golden/make_transfer_truth.py says why a single run's figure is a draw).  With the single run's figure
    the Float64 kernel missed the bound on ONE ray, the captured ray of the as-written a = 0 scene: |I - I_truth| = 7.9e-11 against
    max(3.05e-11, 4 x 2.0e-13), where the twin itself errs by up to 1.3e-10 one ulp away.  Measured maxima: profiles/transfer/README.md."""
    fx = fixture()
    f32 = dtype == np.float32
    tag, floor = ("twin32", FLOOR * EPS32 / EPS64) if f32 else ("twin64", FLOOR)
    names = np.array([str(v) for v in fx["scene"]])
    worst = {}
    for name in ("ks_true09", "ks_ref0"):
        sel = np.flatnonzero(names == name)
        _, metric = fx_scene(name)
        for kap in (0, 1):
            fl = rt_flow(fx_flow(fx, kap, sel[0]))
            got = rt.eval_transfer(metric, [], fl, fx["s0"][sel], fx["lambda_end"][sel], opt=rt_opt(dtype, float(fx["lambda1"])), dtype=dtype)
            for q in ("I", "tau"):
                has = np.isfinite(fx["truth_I"][kap, sel])     # (kappa > 0 across the photon orbit's cylinder: no truth, see the fixture's test)
                tr, terr = fx[f"truth_{q}"][kap, sel][has], fx[f"{tag}_err_{q}"][kap, sel][has]
                err = np.abs(got[q].astype(np.float64)[has] - tr)
                bound = np.maximum(floor * np.nanmax(np.abs(fx[f"truth_{q}"][kap])), TWIN_FACTOR * terr)
                worst[(name, kap, q)] = (float(err.max()), float((err / bound).max()))
                print(f"{np.dtype(dtype).name} {name} kappa {fx['kappas'][kap]:g} {q}: max err {err.max():.3e} (twin {terr.max():.3e}), max err / bound {(err / bound).max():.3f}")
                assert (err <= bound).all(), (name, kap, q, err, bound)
                # … and where the ensemble does not exceed the unperturbed run fourfold — the smooth rays — that run's own figure binds, so
                # the wider yardstick of the kink rays hides no regression elsewhere
                err1 = fx[f"{tag}_err1_{q}"][kap, sel][has]
                stable = terr <= 4 * err1
                bound1 = np.maximum(floor * np.nanmax(np.abs(fx[f"truth_{q}"][kap])), TWIN_FACTOR * err1)
                print(f"      single-run yardstick on {stable.sum()} of {len(err)} rays: max err / bound {(err[stable] / bound1[stable]).max(initial=0):.3f}")
                assert (err[stable] <= bound1[stable]).all(), (name, kap, q, err, bound1, stable)
            steps_ref = fx[f"{tag}_steps"][kap, sel].astype(np.int64)
            sd = np.abs(got["tsteps"].astype(np.int64) - steps_ref)
            print(f"   steps {got['tsteps']} twin {steps_ref} status {got['tstatus']}")
            # Step attempts, both types: within max(2, rel_step_diff x steps, the twin's own step noise) of the twin's.  The noise is the
            # largest distance of the twin's count from itself over the fixture's ensemble (start states one ulp apart): a ray that winds
            # round the photon orbit follows another sequence of steps after any rounding difference (Float32 grazing ray: the twin alone
            # moves by 8, the kernel is 6 away).  Left out: the runs without a truth — across an unbounded dtau/dlambda a step count is
            # where the underflow (Float64) or the luck of the steps (Float32) says, in the twin as in the kernel.
            fine = has & (fx[f"{tag}_status"][kap, sel] != 3)
            allowed = np.maximum(np.maximum(2, np.floor(REL_STEP_DIFF * steps_ref)), fx[f"{tag}_steps_spread"][kap, sel].astype(np.int64))
            assert (sd[fine] <= allowed[fine]).all(), (got["tsteps"], steps_ref, allowed)
            # the status is the twin's on every ray — also where there is no truth: Float64 ends those with a step underflow (3, NaN), the
            # coarser Float32 steps get across the integrable singularity
            assert np.array_equal(got["tstatus"], fx[f"{tag}_status"][kap, sel])
            assert np.isnan(got["I"][got["tstatus"] == 3]).all() and np.isfinite(got["I"][got["tstatus"] != 3]).all()
            assert f32 or (got["tstatus"][~has] == 3).all()
            if kap == 0:
                assert (got["tstatus"][fx["captured"][sel]] == 1).all(), "a captured ray ends at r_stop"
            if kap == 0:
                assert (got["tau"] == 0).all()


def mink_eval(fl, dtype=np.float64, s0=FLAT_S0, lam_end=FLAT_END, **kw):
    return rt.eval_transfer(rt.minkowski, [], rt_flow(fl), np.atleast_2d(s0), np.atleast_1d(lam_end), dtype=dtype, **kw)


@pytest.mark.gpu
def test_identities_on_the_device(lib):
    r = mink_eval(FLAT_RIGID0)
    want = FLAT_RIGID0["j0"] / FLAT_RIGID0["kappa"] * -np.expm1(-r["tau"][0])
    assert r["tstatus"][0] == 0 and r["tau"][0] > 0.1 and abs(r["I"][0] - want) <= 1e-9 * want
    thin = mink_eval(FLAT_THIN)
    want = flat_quad(FLAT_THIN)
    assert thin["tau"][0] == 0.0 and abs(thin["I"][0] - want) <= 1e-9 * want
    assert abs(thin["s_end"][0, 1:4] - (FLAT_S0[1:4] + FLAT_END * FLAT_S0[5:8])).max() <= 1e-12
    # lambda_end = lambda0: nothing integrated
    z = mink_eval(FLAT_THIN, lam_end=0.0)
    assert z["I"][0] == 0 and z["tau"][0] == 0 and z["tstatus"][0] == 0 and z["tsteps"][0] == 0 and np.array_equal(z["s_end"][0], FLAT_S0)
    # the step cap
    o = rt.solver_defaults(np.float64)
    o.max_steps = 3
    c = mink_eval(FLAT_THIN, opt=o)
    assert c["tstatus"][0] == 2 and c["tsteps"][0] == 3
    # a NaN start state
    bad = FLAT_S0.copy()
    bad[2] = np.nan
    n = mink_eval(FLAT_THIN, s0=bad)
    assert n["tstatus"][0] == 3 and np.isnan(n["I"][0]) and np.isnan(n["tau"][0]) and n["tsteps"][0] == 0


KERR = dict(metric=lambda: rt.KerrSchild(1, 0.9), objs=lambda: [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -60.0)])
KERR_POS = (0.0, 40 * np.sin(np.pi / 3), 0.0, 40 * np.cos(np.pi / 3))
KERR_FLOW = dict(j0=0.027, kappa=0.0, r0=4.0, alpha=1.5, H=0.4, s=0.5, r_stop=1.75, gain=1.5, weight=(1.0, 0.6, 0.3))
LAMBDA1 = 400.0
OUT_KEYS = ("state_end", "lambda_end", "status", "hit", "n_accept", "n_reject")
T_KEYS = ("I", "tau", "tstatus", "tsteps")


def kerr_observer(max_batch_rays=0):
    return rt.Observer(KERR_POS, (0, -KERR_POS[1], -KERR_POS[2], -KERR_POS[3]), (0, 0, 0, 1), 0.5, 0.4, projection="equirect", max_batch_rays=max_batch_rays)


def kerr_opt(dtype=np.float64):
    # (the captured rays of this sky-only scene creep up to the horizon until the trace's step cap ends them: a small cap keeps the test quick)
    return rt_opt(dtype, LAMBDA1, max_steps=3000)


@pytest.mark.gpu
@pytest.mark.parametrize("size,rows", [((16, 12), 0), ((37, 19), 5)])
def test_frame_is_the_hook_and_the_observer_trace(lib, size, rows):
    ni, nj = size
    metric, objs = KERR["metric"](), KERR["objs"]()
    fl, opt = rt.Flow(**KERR_FLOW), kerr_opt()
    ob = kerr_observer(rows * ni)
    f = rt.trace_transfer(metric, objs, ob, ni, nj, fl, opt=opt, details=True)
    o = rt.trace_observer(metric, objs, ob, ni, nj, opt=opt, details=True)
    assert all(o[k].tobytes() == f[k].tobytes() for k in OUT_KEYS) and o["counters"] == f["counters"]
    s0 = rt.make_observer_canvas(metric, objs, ob, ni, nj)
    e = rt.eval_transfer(metric, objs, fl, s0, f["lambda_end"], observer=ob, opt=opt)
    skipped = f["status"] == abi.RAY_NAN
    assert not skipped.any()
    assert all(e[k].tobytes() == f[k].tobytes() for k in T_KEYS)
    assert (f["tstatus"] == 1).sum() >= 2 and (f["tstatus"] == 0).sum() >= ni * nj // 2 and np.nanmax(f["I"]) > 0.05
    # THE PICTURE, optically thin: numpy's expression TO THE LAST BIT.  tau is exactly 0, so the attenuation is exp(-0) = 1 in any exp; the
    # two products and the sum are single IEEE operations on the device (no contraction in the picture rule) as in numpy.
    w = np.array(KERR_FLOW["weight"])[:, None]
    assert (f["tau"] == 0).all()
    want = o["rgb"] * np.exp(-f["tau"]) + KERR_FLOW["gain"] * w * f["I"]
    assert f["rgb"].tobytes() == want.tobytes()
    # … and grey: to the last bit WITH AN ATTENUATION WITHIN ONE ULP OF numpy's, because exp differs — the device's exp is the ROCm math
    # library's, numpy's the host libm's, each within an ulp of the true value.  So the statement is not "rgb within an ulp" (an
    # attenuation one ulp off moves the product by an ulp of itself and the rounded sum by up to two of its own: measured, 5 % of the
    # entries differ, by at most 2 ulp) but the sharper one: for every pixel ONE attenuation among numpy's exp(-tau) and its two
    # neighbours reproduces all three channels bit for bit.  Pixels whose integration ended not finite (the kappa > 0 limitation of the
    # model: include/rtgr.h) are NaN in both.
    grey_flow = dict(KERR_FLOW, kappa=0.028)
    gf = rt.trace_transfer(metric, objs, ob, ni, nj, rt.Flow(**grey_flow), opt=opt)
    bad = gf["tstatus"] == 3
    assert np.isnan(gf["rgb"][:, bad]).all() and np.isnan(gf["I"][bad]).all() and (gf["tsteps"][bad] > 0).all()
    ok = ~bad
    assert ok.sum() >= ni * nj // 2 and (gf["tau"][ok] > 0).any()
    att0 = np.exp(-gf["tau"][ok])
    emitted = KERR_FLOW["gain"] * w * gf["I"][ok]
    exact = {k: ((o["rgb"][:, ok] * a + emitted) == gf["rgb"][:, ok]).all(axis=0)
             for k, a in ((0, att0), (-1, np.nextafter(att0, -np.inf)), (+1, np.nextafter(att0, np.inf)))}
    print(f"{ni} x {nj} grey: {bad.sum()} pixels not finite; of {ok.sum()} finite pixels {exact[0].sum()} exact with numpy's exp, "
          f"{(~exact[0] & (exact[-1] | exact[1])).sum()} with a neighbour of it, {(~(exact[0] | exact[-1] | exact[1])).sum()} with neither")
    assert (exact[0] | exact[-1] | exact[1]).all()
    assert f["transfer_counters"]["accepted"] + f["transfer_counters"]["rejected"] == int(f["tsteps"].sum())
    assert f["transfer_counters"]["rays"] == ni * nj and f["transfer_counters"]["events"] == int((f["tstatus"] == 1).sum())
    # independent of the batch size
    for batch in (ni, 5 * ni, ni * nj):
        b = rt.trace_transfer(metric, objs, kerr_observer(batch), ni, nj, fl, opt=opt, details=True)
        assert all(b[k].tobytes() == f[k].tobytes() for k in T_KEYS + OUT_KEYS + ("rgb",)), batch
    # nothing emitted, nothing absorbed: the observer's picture (-0 may become +0)
    dark = rt.trace_transfer(metric, objs, ob, ni, nj, rt.Flow(**dict(KERR_FLOW, j0=0.0, kappa=0.0)), opt=opt)
    assert np.array_equal(dark["rgb"], o["rgb"]) and (dark["I"] == 0).all() and (dark["tau"] == 0).all()


def _hip_runtime():
    import importlib.util
    spec = importlib.util.find_spec("torch")
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return C.CDLL(cand if os.path.exists(cand) else "libamdhip64.so")


class DevFrame:
    """the device buffers of one transfer frame of n pixels, every one filled so that an untouched buffer shows"""
    PLANES = ("rgb", "I", "tau", "tstatus", "tsteps", "state_end", "lambda_end", "status")

    def __init__(self, n, dtype):
        import torch
        t = torch.float64 if dtype == np.float64 else torch.float32
        for k, shape in (("rgb", (3, n)), ("I", (n,)), ("tau", (n,)), ("state_end", (n, 8)), ("lambda_end", (n,))):
            setattr(self, k, torch.full(shape, 7.0, dtype=t, device="cuda"))
        self.tstatus = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        self.status = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        self.tsteps = torch.full((n,), 7, dtype=torch.int32, device="cuda")
        self.out = abi.rtgr_ray_outputs(state_end=self.state_end.data_ptr(), lambda_end=self.lambda_end.data_ptr(), status=self.status.data_ptr())
        torch.cuda.synchronize()

    def bytes(self, keys=None):
        return {k: getattr(self, k).cpu().numpy().tobytes() for k in (keys or self.PLANES)}

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all(bool((getattr(self, k) == 7).all()) for k in self.PLANES)


def trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F, stream, ctr=None, tctr=None, drop=(), out=True):
    ptr = lambda k: None if k in drop else getattr(F, k).data_ptr()
    ref = lambda x: None if x is None else C.byref(x)
    return getattr(lib, "rtgr_trace_transfer_device_" + suf)(None, ref(sc), C.byref(opt), ref(ob), ni, nj, None, None, ref(fl), ptr("rgb"),
                                                             C.byref(F.out) if out else None, None, ptr("I"), ptr("tau"), ptr("tstatus"), ptr("tsteps"),
                                                             ref(ctr), ref(tctr), stream)


@pytest.mark.gpu
def test_device_entry_streams_batches_capture_and_trim(lib):
    """rtgr_trace_transfer_device_f64 gives the host entry's bytes on the default stream (with both counters), on a side stream, in
    five-row batches, with every optional plane and `out` omitted (lambda_end and status then borrowed from the frame scratch), replayed
    once from a graph captured with ctr = tctr = NULL, and after rtgr_trim; during capture it refuses either counter in its own name"""
    import torch
    dtype, suf = np.float64, "f64"
    ni, nj = 37, 19
    n = ni * nj
    metric, objs = KERR["metric"](), KERR["objs"]()
    sc, opt, fl, ob = rt.make_scene(metric, objs), kerr_opt(), rt.Flow(**KERR_FLOW), kerr_observer()
    host = rt.trace_transfer(metric, objs, ob, ni, nj, fl, opt=opt, details=True)
    want = {k: host[k].tobytes() for k in ("rgb", "I", "tau", "tstatus", "state_end", "lambda_end", "status")}
    want["tsteps"] = host["tsteps"].astype(np.int32).tobytes()
    side, hip = torch.cuda.Stream(), _hip_runtime()
    F = {k: DevFrame(n, dtype) for k in ("default", "side", "rows5", "bare", "graph", "refused", "fresh")}
    ctr, tctr = abi.rtgr_counters(), abi.rtgr_counters()
    abi.check(lib, trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F["default"], None, ctr=ctr, tctr=tctr))
    assert ctr.as_dict() == host["counters"] and tctr.as_dict() == host["transfer_counters"]
    abi.check(lib, trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F["side"], side.cuda_stream))
    abi.check(lib, trace_dev(lib, suf, sc, opt, kerr_observer(5 * ni), ni, nj, fl, F["rows5"], side.cuda_stream))
    only_t = abi.rtgr_counters()
    abi.check(lib, trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F["bare"], side.cuda_stream, tctr=only_t, drop=("I", "tau", "tstatus", "tsteps"), out=False))
    torch.cuda.synchronize()
    for k in ("default", "side", "rows5"):
        assert F[k].bytes() == want, k
    assert only_t.as_dict() == host["transfer_counters"] and F["bare"].bytes(("rgb",)) == {"rgb": want["rgb"]}
    assert all(bool((getattr(F["bare"], k) == 7).all()) for k in ("I", "tau", "tstatus", "tsteps", "state_end", "lambda_end", "status"))
    graph, exe = C.c_void_p(None), C.c_void_p(None)
    assert hip.hipStreamBeginCapture(C.c_void_p(side.cuda_stream), 2) == 0   # hipStreamCaptureModeRelaxed
    rc_ctr = trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F["refused"], side.cuda_stream, ctr=abi.rtgr_counters())
    msg_ctr = lib.rtgr_last_error()
    rc_tctr = trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F["refused"], side.cuda_stream, tctr=abi.rtgr_counters())
    msg_tctr = lib.rtgr_last_error()
    rc = trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F["graph"], side.cuda_stream)
    assert hip.hipStreamEndCapture(C.c_void_p(side.cuda_stream), C.byref(graph)) == 0
    assert rc == 0, lib.rtgr_last_error()
    assert rc_ctr == abi.ERR_BAD_ARG and b"ctr" in msg_ctr and b"rtgr_trace_transfer" in msg_ctr, msg_ctr
    assert rc_tctr == abi.ERR_BAD_ARG and b"tctr" in msg_tctr and b"rtgr_trace_transfer" in msg_tctr, msg_tctr
    assert F["graph"].untouched() and F["refused"].untouched()
    assert graph.value and hip.hipGraphInstantiate(C.byref(exe), graph, None, None, C.c_size_t(0)) == 0
    assert hip.hipGraphLaunch(exe, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    assert F["graph"].bytes() == want
    hip.hipGraphExecDestroy(exe)
    hip.hipGraphDestroy(graph)
    abi.check(lib, lib.rtgr_trim(None))
    abi.check(lib, trace_dev(lib, suf, sc, opt, ob, ni, nj, fl, F["fresh"], side.cuda_stream))
    torch.cuda.synchronize()
    assert F["fresh"].bytes() == want


@pytest.mark.gpu
def test_composition_with_an_emitting_disk(lib):
    """Schwarzschild, an emitting disk and a sky: a pixel that ends on the disk shows the disk's colour times exp(-tau) plus the flow's
    term, a sky pixel the sky's colour attenuated"""
    metric = rt.KerrSchild(1, 0.0)
    objs = [rt.Sphere((0, 0, 0, 0), (1, 0, 0, 0), -25.0), rt.Plane(-80.0), rt.Disk(0.05, 4.5, 8.0)]
    pos = (0, 0, -12, 8)
    ob = rt.Observer(pos, (0, 0, 12, -8), (0, 0, 0, 1), 1.3, 0.9)
    em = rt.DiskEmission(3, 30000.0)
    flow = dict(j0=0.05, kappa=0.05, r0=4.0, alpha=1.5, H=0.4, s=0.5, r_stop=2.5, gain=0.8, weight=(1.0, 0.5, 0.25))
    opt = rt_opt(np.float64, 100.0, max_steps=3000)
    f = rt.trace_transfer(metric, objs, ob, 24, 16, rt.Flow(**flow), emission=em, opt=opt, details=True)
    o = rt.trace_observer(metric, objs, ob, 24, 16, emission=em, opt=opt, details=True)
    assert f["g"].tobytes() == o["g"].tobytes() and f["hit"].tobytes() == o["hit"].tobytes()
    disk, sky = o["hit"] == 3, o["hit"] == 1
    assert disk.sum() >= 20 and sky.sum() >= 50 and (o["rgb"][:, disk].max(axis=0) > 0).all()
    att, w = np.exp(-f["tau"]), np.array(flow["weight"])[:, None]
    want = o["rgb"] * att + flow["gain"] * w * f["I"]
    for sel in (disk, sky):
        ok = sel & (f["tstatus"] != 3)
        assert ok.sum() >= 20 and (f["tau"][ok] > 0).all() and (att[ok] < 1).all()
        assert np.abs(f["rgb"][:, ok] - want[:, ok]).max() <= 4 * EPS64 * np.abs(want[:, ok]).max()
        assert (f["rgb"][:, ok] >= o["rgb"][:, ok] * att[ok] * (1 - 4 * EPS64)).all()


# ---- the contract of the arrays -----------------------------------------------------------------------------------------------------------
GUARD = 64


class Guarded:
    """a host array of `count` elements with GUARD bytes of 0xA5 behind it"""

    def __init__(self, count, dtype):
        nbytes = count * np.dtype(dtype).itemsize
        self.raw = np.full(nbytes + GUARD, 0xA5, np.uint8)
        self.view = self.raw[:nbytes].view(dtype)
        self.nbytes = nbytes

    @property
    def ptr(self):
        return self.raw.ctypes.data

    def intact(self):
        return bool((self.raw[self.nbytes:] == 0xA5).all())

    def written(self):
        return not bool((self.raw[:self.nbytes] == 0xA5).all())


def _hook_cases(n):
    rng = np.random.default_rng(3)
    sc = tt.Scene("ks_true", 1.0, 0.9)
    pos = np.array(KERR_POS)
    s0 = np.array([tt.camera_state(sc, pos, -pos[1:] / 40 + 0.3 * rng.normal(size=3)) for _ in range(max(n, 1))])[:n]
    return s0.reshape(n, 8), np.full(n, 30.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 257])
def test_the_hooks_keep_to_their_arrays(lib, n):
    """guard bytes behind every output, each optional output omitted in turn, n = 0, n = 257 (more than one workgroup, a partial one)"""
    sc = rt.make_scene(rt.KerrSchild(1, 0.9), [])
    opt, fl = rt_opt(np.float64, LAMBDA1), rt.Flow(**KERR_FLOW)
    s0, le = _hook_cases(n)
    s = s0.copy()
    s[:, 1:4] *= 0.2
    t_spec = (("I", n, np.float64), ("tau", n, np.float64), ("s_end", 8 * n, np.float64), ("tstatus", n, np.uint8), ("tsteps", n, np.uint32))
    f_spec = (("dens", n, np.float64), ("omega", n, np.float64), ("u_f", 4 * n, np.float64), ("gfac", n, np.float64), ("dtau", n, np.float64),
              ("dI0", n, np.float64))
    p = lambda a: a.ctypes.data if n else None
    full = {}
    for hook, spec in (("transfer", t_spec), ("flow", f_spec)):
        for omit in (None,) + tuple(k for k, _, _ in spec):
            bufs = {k: Guarded(c, d) for k, c, d in spec}
            args = [None if k == omit else bufs[k].ptr for k, _, _ in spec]
            if hook == "transfer":
                rc = lib.rtgr_eval_transfer_f64(None, C.byref(sc), C.byref(opt), C.byref(fl), None, p(s0), p(le), n, *args)
            else:
                rc = lib.rtgr_eval_flow_f64(None, C.byref(sc), C.byref(fl), None, p(s0), p(s), n, *args)
            assert rc == 0, lib.rtgr_last_error()
            for k, c, _ in spec:
                assert bufs[k].intact(), (hook, omit, k)
                if k == omit or n == 0:
                    assert not bufs[k].written(), (hook, omit, k)
                elif omit is None:
                    full[(hook, k)] = bufs[k].view.tobytes()
                else:
                    assert bufs[k].view.tobytes() == full[(hook, k)], (hook, omit, k)


@pytest.mark.gpu
def test_the_host_entrys_extra_planes_keep_to_their_arrays(lib):
    ni, nj = 16, 12
    n = ni * nj
    metric, objs = KERR["metric"](), KERR["objs"]()
    sc, opt, fl, ob = rt.make_scene(metric, objs), kerr_opt(), rt.Flow(**KERR_FLOW), kerr_observer()
    spec = (("I", n, np.float64), ("tau", n, np.float64), ("tstatus", n, np.uint8), ("tsteps", n, np.uint32))
    full = {}
    for omit in (None,) + tuple(k for k, _, _ in spec):
        rgb = Guarded(3 * n, np.float64)
        bufs = {k: Guarded(c, d) for k, c, d in spec}
        rc = lib.rtgr_trace_transfer_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, None, C.byref(fl), rgb.ptr, None, None,
                                         *[None if k == omit else bufs[k].ptr for k, _, _ in spec], None, None)
        assert rc == 0, lib.rtgr_last_error()
        assert rgb.intact() and all(b.intact() for b in bufs.values())
        for k, _, _ in spec + (("rgb", 0, 0),):
            b = rgb if k == "rgb" else bufs[k]
            if k == omit:
                assert not b.written()
            elif omit is None:
                full[k] = b.view.tobytes()
            else:
                assert b.view.tobytes() == full[k], (omit, k)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _refusals():
    ok = dict(KERR_FLOW)
    nan, inf = float("nan"), float("inf")
    cases = [(dict(ok, emitter="rigid", orbit=nan), b"orbit"), (dict(ok, orbit=0.5), b"orbit"), (dict(ok, j0=-1.0), b"j0"), (dict(ok, j0=nan), b"j0"),
             (dict(ok, kappa=-0.1), b"kappa"), (dict(ok, kappa=inf), b"kappa"), (dict(ok, r0=0.0), b"r0"), (dict(ok, r0=nan), b"r0"), (dict(ok, alpha=nan), b"alpha"),
             (dict(ok, H=0.0), b"H"), (dict(ok, H=-1.0), b"H"), (dict(ok, s=inf), b".s"), (dict(ok, r_stop=-1.0), b"r_stop"), (dict(ok, r_stop=nan), b"r_stop"),
             (dict(ok, gain=nan), b"gain"), (dict(ok, weight=(1.0, nan, 1.0)), b"weight[1]")]
    flows = [(rt.Flow(**kw), word) for kw, word in cases]
    bad = rt.Flow(**ok)
    bad.emitter = 7
    flows.append((bad, b"emitter"))
    bad = rt.Flow(**ok)
    bad.flags = 1
    flows.append((bad, b"flags"))
    return flows


@pytest.mark.gpu
def test_every_refusal_names_its_field_and_leaves_the_outputs_untouched(lib):
    ni, nj = 8, 6
    n = ni * nj
    metric, objs = KERR["metric"](), KERR["objs"]()
    sc, opt, ob = rt.make_scene(metric, objs), kerr_opt(), kerr_observer()
    s0, le = _hook_cases(4)
    good = rt.Flow(**KERR_FLOW)

    def all_three(scene, flow, word, observer=ob):
        ref = lambda x: None if x is None else C.byref(x)
        rgb, I = np.full(3 * n, 7.0), np.full(n, 7.0)
        rc = lib.rtgr_trace_transfer_f64(None, C.byref(scene), C.byref(opt), ref(observer), ni, nj, None, None, ref(flow), rgb.ctypes.data, None, None,
                                         I.ctypes.data, None, None, None, None, None)
        msg = lib.rtgr_last_error()
        assert rc == abi.ERR_BAD_ARG and word in msg, (word, msg)
        assert (rgb == 7).all() and (I == 7).all()
        if observer is None:
            return
        out = np.full(4, 7.0)
        rc = lib.rtgr_eval_transfer_f64(None, C.byref(scene), C.byref(opt), ref(flow), None, s0.ctypes.data, le.ctypes.data, 4, out.ctypes.data, None, None, None, None)
        msg = lib.rtgr_last_error()
        assert rc == abi.ERR_BAD_ARG and word in msg and (out == 7).all(), (word, msg)
        rc = lib.rtgr_eval_flow_f64(None, C.byref(scene), ref(flow), None, s0.ctypes.data, s0.ctypes.data, 4, out.ctypes.data, None, None, None, None, None)
        msg = lib.rtgr_last_error()
        assert rc == abi.ERR_BAD_ARG and word in msg and (out == 7).all(), (word, msg)

    all_three(sc, None, b"flow")
    for flow, word in _refusals():
        all_three(sc, flow, word)
    # metrics without a closed right-hand side here: the user's own, grids
    for m, word in ((abi.USER, b"RTGR_USER"), (abi.GRID, b"grid"), (abi.GRID + 1, b"grid")):
        other = rt.make_scene(metric, objs)
        other.metric = m
        all_three(other, good, word)
    # what the observer trace refuses: no observer, a bad canvas, redshift asked of an observer frame
    all_three(sc, good, b"obs", observer=None)
    rgb = np.full(3 * n, 7.0)
    rc = lib.rtgr_trace_transfer_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), 0, nj, None, None, C.byref(good), rgb.ctypes.data, None, None,
                                     None, None, None, None, None, None)
    assert rc == abi.ERR_BAD_ARG and b"canvas" in lib.rtgr_last_error() and (rgb == 7).all()
    g = np.full(n, 7.0)
    rc = lib.rtgr_trace_transfer_f64(None, C.byref(sc), C.byref(opt), C.byref(ob), ni, nj, None, None, C.byref(good), rgb.ctypes.data, None, g.ctypes.data,
                                     None, None, None, None, None, None)
    assert rc == abi.ERR_BAD_ARG and b"emit" in lib.rtgr_last_error() and (rgb == 7).all() and (g == 7).all()
