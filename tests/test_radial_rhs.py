"""The a = 0 closed-form RHS (rtgr_physics.hpp: accel_radial) with the cancelling pair of terms left out — λ = κP + ½ q f κ K²,
|k|² − 1 and k♯·L from t1 = ρ²/r (tools/check_identities_radial.py holds the algebra to 40 digits) — at the fixture of
test_rhs_edges.py: tests/golden/rhs_edges.npz, 8 families x 32 states per variant against 50-digit values.

CPU: the operation sequence restated in numpy (plain IEEE double, no fused multiply-add, true division for the reciprocals) stays
within the fixture's own Float64 bar, max(16 x the oracle's recorded error over a family, 64 eps) — test_rhs_edges.f64_bar, a property of
the reference side alone — for every a = 0 variant of the fixture, and is finite at every state.

GPU: path 2 (the function the integrate kernels call) against path 0 (ks_field + ksform_accel, the general contraction, which does not
know that k is a gradient).  Each is within the bar of the 50-digit value (test_rhs_edges.py asserts that), so the two differ by at most
twice the bar, family by family; and path 2 keeps the exact identities of test_rhs_edges.identity_violations.
"""
import numpy as np
import pytest

from scenes import rt
from test_rhs_edges import FAMILIES, G, NF, f64_bar, fix, identity_states, identity_violations, metric_of, report

RADIAL = [name for name, (kind, M, a) in G.VARIANTS.items() if a == 0.0]


def accel_radial_numpy(s, kind, M):
    """s [n, 8] Float64 states -> u̇ [n, 4]: accel_radial's operations in its order, one rounding each"""
    x, y, z = s[:, 1], s[:, 2], s[:, 3]
    ut, ux, uy, uz = s[:, 4], s[:, 5], s[:, 6], s[:, 7]
    rho2 = x * x + (y * y + z * z)
    ir = 1.0 / np.sqrt(rho2)
    if kind == "ks_ref":
        rho = rho2 * ir
        invr = 2.0 * ir * (1.0 / (1.0 + rho))
        rq2 = 0.5 * ir + 1.0
    else:
        invr, rq2 = ir, ir
    f = (2.0 * M) * invr
    xu = x * ux + (y * uy + z * uz)
    uu = ux * ux + (uy * uy + uz * uz)
    D = rq2 * xu
    Ku = invr * xu
    K = ut + Ku
    fi = f * invr
    P = fi * (-D * (K + Ku) + uu)
    lam = invr * P + (rq2 * (fi * K)) * (0.5 * K)
    t1 = rho2 * invr
    S = f * (1.0 / (f * (t1 * invr - 1.0) + 1.0)) if kind == "ks_ref" else f
    kL = t1 * lam - P
    SkL = S * kL
    g = SkL * invr - lam
    return np.stack([P - SkL, x * g, y * g, z * g], axis=1)


def test_the_a0_variants_of_the_fixture_are_the_two_radii():
    assert sorted(RADIAL) == ["ks_ref0", "ks_true0"], RADIAL


@pytest.mark.parametrize("name", RADIAL)
def test_operation_sequence_in_numpy_is_within_the_f64_bar(name):
    kind, M, a = G.VARIANTS[name]
    s = fix(f"f64_{name}_s").reshape(-1, 8)
    with np.errstate(all="raise", under="ignore"):
        got = accel_radial_numpy(s, kind, M)
    assert np.isfinite(got).all()
    err = G.rel_err(got, fix(f"f64_{name}_ud_hi").reshape(-1, 4), fix(f"f64_{name}_ud_lo").reshape(-1, 4))
    report(err.reshape(NF, G.N).max(axis=1), f64_bar(fix(f"f64_{name}_ud_oracle_err")), f"numpy restatement {name}")


# ---- GPU -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    abi = rt._abi
    lib = abi.load()
    abi.check(lib, lib.rtgr_init(-1))
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("name", RADIAL)
def test_production_path_against_the_general_contraction(lib, name):
    s = fix(f"f64_{name}_s").reshape(-1, 8)
    m = metric_of(name)
    general, radial = rt.geodesic(s, m, path=0), rt.geodesic(s, m, path=2)
    assert np.isfinite(general).all() and np.isfinite(radial).all() and np.array_equal(radial[:, :4], s[:, 4:])
    hi = fix(f"f64_{name}_ud_hi").reshape(-1, 4)
    scale = np.abs(hi).max(axis=1)
    d = np.abs(radial[:, 4:] - general[:, 4:]).max(axis=1)
    d = np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), d)            # (the measure of make_rhs_edges.rel_err)
    report(d.reshape(NF, G.N).max(axis=1), 2.0 * f64_bar(fix(f"f64_{name}_ud_oracle_err")), f"path 2 - path 0 {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", RADIAL)
@pytest.mark.parametrize("prec", [64, 32])
def test_production_path_keeps_the_exact_identities(lib, name, prec):
    dtype = np.float64 if prec == 64 else np.float32
    m = metric_of(name)
    bad = identity_violations(lambda s: rt.geodesic(s, m, path=2, dtype=dtype).reshape(-1, 8), identity_states(name, prec), dtype,
                              *G.VARIANTS[name][1:])
    assert bad == [], bad
    assert len(FAMILIES) == NF
