"""The identities the a = 0 closed-form RHS is built on (rtgr_physics.hpp: accel_radial) — k = x/r(ρ) is a gradient field, so the
antisymmetric part of the general contraction's L_i vanishes and L_i = x_i (κP + ½ q f κ K²) — and the acceleration against the
Christoffel contraction of the 4x4 metric (src/RayTraceGR.jl:321-331, :358-370), for r = ρ and for the as-written r = (ρ + ρ²)/2,
in 40-digit arithmetic: tools/check_identities_radial.py, run here so that the derivation in the kernel source is a test."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_radial_identities_hold_to_40_digits_for_both_radii():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_identities_radial.py"), "--points", "8", "--digits", "40"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all identities hold" in r.stdout
    assert r.stdout.count("ok  ") == 8 and "FAIL" not in r.stdout, r.stdout   # (1), ∇r = q x, (2), (3) for each radius
    for kind in ("rho", "as_written"):
        assert r.stdout.count(kind) == 4, r.stdout
