// rtgr_polarization.hpp — linear polarization of a thin disk by Walker–Penrose transport (include/rtgr.h "polarized disk images").  The
// device functions of ONE kernel (rtgr_polarize.hip: polarize_kernel), which serves the traced frame, the stage alone and the two hooks,
// so a hook predicts a pixel to the bit.
//
// THE CONTRACT (everything in the scalar type R of the entry point; coordinates are the library's Kerr–Schild (t, x, y, z); the metric is
// RTGR_KS_TRUE with the scene's a — the forms do not contain M —, RTGR_MINKOWSKI the same code with a = 0).
//   pw² = x² + y²,  q = x² + y² + z² − a²,  r² = (q + sqrt(q² + 4 a² z²)) / 2  (the textbook Kerr radius).
//   dr  = (2 r² x, 2 r² y, 2 r² z + 2 a² z) / (4 r³ − 2 q r)  on (dx, dy, dz);   c = z / r,  dc = dz / r − (z / r²) dr,  s² = 1 − c²
//   dφ~ = (x dy − y dx)/pw² + a dr/(r² + a²)
//   ω¹  = dt − a s² dφ~,  evaluated as dt − a [(x dy − y dx)/(r² + a²) + (a s²/(r² + a²)) dr]       (regular on the axis)
//   ω²  = (r² + a²) dφ~ − a dt − a dr = (r² + a²)(x dy − y dx)/pw² − a dt                             (the only 1/pw²)
//   Y = −a c dr∧ω¹ + r dc∧ω²  (Killing–Yano),   h = −r dr∧ω¹ − a c dc∧ω²  (conformal Killing–Yano).
//   κ₁ = Y_ab k^a f^b, κ₂ = h_ab k^a f^b are constant along a null geodesic with tangent k for f parallel-transported, g(k, f) = 0;
//   adding a multiple of k to f changes neither; the traced ray's own past-directed tangent is used at both ends as it is.
//   A point with pw² <= 4096 eps (r² + a²) is INVALID (the disk is never there; an observer there gets NaN).
// The emitter's triad at the ray's end: u = the emitter of rtgr_emission.hpp (circular_orbit_rate, KEPLER or RIGID);
//   cross(v, w)_a = −sqrt(−det g) ε_abcd u^b v^c w^d (ε_0123 = +1), raised with g⁻¹ — rtgr_observer.hpp's e_right = look × up;
//   e_z' = normalise(∂_z + g(∂_z, u) u);  e_ρ' = normalise of (0, x, y, 0)/pw made orthogonal to u and e_z';  e_φ' = cross(e_z', e_ρ');
//   p = k_end + g(k_end, u) u,  p^ = p / sqrt(g(p, p)).
// The emission law:  SCATTER  f_em = normalise(cross(p^, e_z')), μ = |g(p^, e_z')|, δ = deg0 (1 − μ)/(1 + deg1 μ), aux = μ;
//                    FIELD    B^ = normalise(B_ρ e_ρ' + B_φ e_φ' + B_z e_z'), f_em = normalise(cross(p^, B^)), δ = deg0, aux = |cross(p^, B^)|.
//   INVALID if the emitter is invalid or |cross|² <= 4096 eps: q = u = 0 there if δ is finite, else NaN.  aux, κ, f_em and δ are written
//   before validity is known: at an invalid point they hold whatever the formulas give (a division by pw = 0 included — such a point
//   fails the axis rule) and mean nothing.
// At the camera (state x_0, k_0 = (−e_0 + n)/sqrt(2); frame record e_0, e_right, e_up, e_look with its metric g):
//   n = sqrt(2) k_0 + e_0,  e^_y = normalise(e_up − g(e_up, n) n),  e^_x = normalise(e_right − g(e_right, n) n − g(e_right, e^_y) e^_y);
//   κ₁ = α Y(k_0, e^_x) + β Y(k_0, e^_y),  κ₂ = α h(k_0, e^_x) + β h(k_0, e^_y);
//   q = δ (α² − β²)/(α² + β²),  u = 2 δ α β/(α² + β²): the position angle runs from e^_x towards e^_y; no atan.
//   A degenerate screen basis (squared norm of a projected vector <= 4096 eps sum |v g v|, the rule of observer_frame) or an invalid
//   frame gives NaN.
// Out of scope: the plane camera, anti-aliasing, Q(t) / U(t) and polarized spectra, Faraday rotation, circular polarization, limb
// darkening, grids, RTGR_KS_REF and user metrics.
//
// No operation of these functions is fused (fp contract off), as in rtgr_emission.hpp and rtgr_observer.hpp; the metric code they call
// is the library's.
#pragma once
#include "rtgr_observer.hpp"

namespace rtgr {

// the four covectors on (dt, dx, dy, dz) and the two scalars of Y and h at one point
template <class R>
struct PolForms {
    R dr[4], w1[4], dc[4], w2[4];
    R r, ac;
    bool ok;   // off the axis
};

template <class R>
RTGR_DEV void pol_forms(R a, const R x[4], PolForms<R>& F) {
#pragma clang fp contract(off)
    const R X = x[1], Y = x[2], Z = x[3];
    const R a2 = a * a;
    const R q = X * X + Y * Y + Z * Z - a2;
    const R r2 = R(0.5) * (q + rsqrt_(q * q + R(4) * a2 * Z * Z));
    const R r = rsqrt_(r2);
    const R den = R(4) * r2 * r - R(2) * q * r;
    F.dr[0] = R(0);
    F.dr[1] = R(2) * r2 * X / den;
    F.dr[2] = R(2) * r2 * Y / den;
    F.dr[3] = (R(2) * r2 * Z + R(2) * a2 * Z) / den;
    const R c = Z / r, zr2 = Z / r2;
    F.dc[0] = R(0);
    F.dc[1] = -(zr2 * F.dr[1]);
    F.dc[2] = -(zr2 * F.dr[2]);
    F.dc[3] = R(1) / r - zr2 * F.dr[3];
    const R s2 = R(1) - c * c, pw2 = X * X + Y * Y, ra = r2 + a2;
    F.ok = pw2 > R(4096) * obs_eps<R>() * ra;
    const R e = a * s2 / ra;
    F.w1[0] = R(1);
    F.w1[1] = -(a * (e * F.dr[1] - Y / ra));
    F.w1[2] = -(a * (e * F.dr[2] + X / ra));
    F.w1[3] = -(a * (e * F.dr[3]));
    const R h = ra / pw2;
    F.w2[0] = -a;
    F.w2[1] = -(h * Y);
    F.w2[2] = h * X;
    F.w2[3] = R(0);
    F.r = r;
    F.ac = a * c;
}

template <class R>
RTGR_DEV R pol_dot(const R w[4], const R v[4]) {
#pragma clang fp contract(off)
    return ((w[0] * v[0] + w[1] * v[1]) + w[2] * v[2]) + w[3] * v[3];
}

// (κ₁, κ₂) = (Y(k, f), h(k, f))
template <class R>
RTGR_DEV void pol_kappa(const PolForms<R>& F, const R k[4], const R f[4], R kap[2]) {
#pragma clang fp contract(off)
    const R A = pol_dot<R>(F.dr, k) * pol_dot<R>(F.w1, f) - pol_dot<R>(F.dr, f) * pol_dot<R>(F.w1, k);   // (dr∧ω¹)(k, f)
    const R B = pol_dot<R>(F.dc, k) * pol_dot<R>(F.w2, f) - pol_dot<R>(F.dc, f) * pol_dot<R>(F.w2, k);   // (dc∧ω²)(k, f)
    kap[0] = F.r * B - F.ac * A;
    kap[1] = -(F.r * A) - F.ac * B;
}

// cross(v, c) in the rest space of u: w = −sqrt(−det g), gu = g⁻¹ (observer_frame's e_right, with (u, v, c) for (e_0, e_look, e_up))
template <class R>
RTGR_DEV void pol_cross(R w, const R gu[4][4], const R u[4], const R v[4], const R c[4], R out[4]) {
#pragma clang fp contract(off)
    R lo[4];
    lo[0] = w * obs_det3<R>(u[1], u[2], u[3], v[1], v[2], v[3], c[1], c[2], c[3]);
    lo[1] = -(w * obs_det3<R>(u[0], u[2], u[3], v[0], v[2], v[3], c[0], c[2], c[3]));
    lo[2] = w * obs_det3<R>(u[0], u[1], u[3], v[0], v[1], v[3], c[0], c[1], c[3]);
    lo[3] = -(w * obs_det3<R>(u[0], u[1], u[2], v[0], v[1], v[2], c[0], c[1], c[2]));
#pragma unroll
    for (int p = 0; p < 4; p++) out[p] = gu[p][0] * lo[0] + gu[p][1] * lo[1] + gu[p][2] * lo[2] + gu[p][3] * lo[3];
}

// The emitter side at the end state se: κ, f_em, aux, δ.  Returns whether the point is valid; everything is always written.
template <class R>
RTGR_DEV bool pol_emitter(const DevScene<R>& sc, R a, const DevEmission<R>& E, const DevPolarization<R>& P, const R se[8], R kap[2], R fem[4],
                          R& aux, R& delta) {
#pragma clang fp contract(off)
    const R x = se[1], y = se[2];
    bool ok = true;
    R Om;
    if (E.emitter == RTGR_EMIT_KEPLER) Om = circular_orbit_rate<R>(sc, se[0], x, y, E.orbit, ok);
    else Om = E.orbit;
    R g[4][4], gu[4][4], u[4];
    metric_plain<R>(sc, se, g);
    const R xi[4] = {R(1), -(Om * y), Om * x, R(0)};
    const R n2 = inner<R>(g, xi, xi);   // (disk_emission's own expression for u_emit)
    ok = ok && rfinite(Om) && rfinite(n2) && n2 < R(0);
    const R sc_u = R(1) / rsqrt_(-n2);
#pragma unroll
    for (int c = 0; c < 4; c++) u[c] = xi[c] * sc_u;
    const R det = obs_det4<R>(g);
    ok = ok && det < R(0);
    const R w = -rsqrt_(-det);
    inv4sym<R>(g, gu);
    const R tol = R(4096) * obs_eps<R>();
    // e_z'
    R ez[4];
    {
        const R dz[4] = {R(0), R(0), R(0), R(1)};
        const R b = obs_inner<R>(g, dz, u);
        R v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = dz[c] + b * u[c];
        const R s = R(1) / rsqrt_(obs_inner<R>(g, v, v));
#pragma unroll
        for (int c = 0; c < 4; c++) ez[c] = v[c] * s;
    }
    // p^
    R ph[4];
    {
        const R b = obs_inner<R>(g, se + 4, u);
        R v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = se[4 + c] + b * u[c];
        const R s = R(1) / rsqrt_(obs_inner<R>(g, v, v));
#pragma unroll
        for (int c = 0; c < 4; c++) ph[c] = v[c] * s;
    }
    R cr[4];
    bool field = P.kind == RTGR_POL_FIELD;
    if (field) {
        R er[4], ep[4], B[4];
        const R pw = rsqrt_(x * x + y * y);
        R v[4] = {R(0), x / pw, y / pw, R(0)};
        const R b = obs_inner<R>(g, v, u);
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = v[c] + b * u[c];
        const R d = obs_inner<R>(g, v, ez);
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = v[c] - d * ez[c];
        const R s = R(1) / rsqrt_(obs_inner<R>(g, v, v));
#pragma unroll
        for (int c = 0; c < 4; c++) er[c] = v[c] * s;
        pol_cross<R>(w, gu, u, ez, er, ep);
#pragma unroll
        for (int c = 0; c < 4; c++) B[c] = P.field[0] * er[c] + P.field[1] * ep[c] + P.field[2] * ez[c];
        const R sb = R(1) / rsqrt_(obs_inner<R>(g, B, B));
#pragma unroll
        for (int c = 0; c < 4; c++) B[c] = B[c] * sb;
        pol_cross<R>(w, gu, u, ph, B, cr);
        delta = P.deg0;
    } else {
        pol_cross<R>(w, gu, u, ph, ez, cr);
        const R mu = rabs<R>(obs_inner<R>(g, ph, ez));
        delta = P.deg0 * (R(1) - mu) / (R(1) + P.deg1 * mu);
        aux = mu;
    }
    const R c2 = obs_inner<R>(g, cr, cr);
    if (field) aux = rsqrt_(c2);
    ok = ok && c2 > tol;
    const R s = R(1) / rsqrt_(c2);
#pragma unroll
    for (int c = 0; c < 4; c++) fem[c] = cr[c] * s;
    PolForms<R> F;
    pol_forms<R>(a, se, F);
    ok = ok && F.ok;
    pol_kappa<R>(F, se + 4, fem, kap);
    return ok;
}

// The camera side: (α, β) from κ under frame Fr at the start state s0.  Returns whether the screen basis and the frame are usable.
template <class R>
RTGR_DEV bool pol_camera(R a, const ObsFrame<R>& Fr, const R s0[8], const R kap[2], R& al, R& be) {
#pragma clang fp contract(off)
    const R tol = R(4096) * obs_eps<R>();
    bool ok = Fr.valid != 0u;
    R n[4], ex[4], ey[4], er[4], eu[4];
    const R s2 = rsqrt_(R(2));
#pragma unroll
    for (int c = 0; c < 4; c++) { n[c] = s2 * s0[4 + c] + Fr.e[0][c]; er[c] = Fr.e[1][c]; eu[c] = Fr.e[2][c]; }
    {
        const R b = obs_inner<R>(Fr.g, eu, n);
        R v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = eu[c] - b * n[c];
        const R q = obs_inner<R>(Fr.g, v, v);
        ok = ok && q > tol * obs_scale<R>(Fr.g, eu);
        const R s = R(1) / rsqrt_(q);
#pragma unroll
        for (int c = 0; c < 4; c++) ey[c] = v[c] * s;
    }
    {
        const R b = obs_inner<R>(Fr.g, er, n), d = obs_inner<R>(Fr.g, er, ey);
        R v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = er[c] - b * n[c] - d * ey[c];
        const R q = obs_inner<R>(Fr.g, v, v);
        ok = ok && q > tol * obs_scale<R>(Fr.g, er);
        const R s = R(1) / rsqrt_(q);
#pragma unroll
        for (int c = 0; c < 4; c++) ex[c] = v[c] * s;
    }
    PolForms<R> F;
    pol_forms<R>(a, s0, F);
    ok = ok && F.ok;
    R kx[2], ky[2];
    pol_kappa<R>(F, s0 + 4, ex, kx);
    pol_kappa<R>(F, s0 + 4, ey, ky);
    const R det = kx[0] * ky[1] - ky[0] * kx[1];
    al = (kap[0] * ky[1] - ky[0] * kap[1]) / det;
    be = (kx[0] * kap[1] - kx[1] * kap[0]) / det;
    return ok;
}

}  // namespace rtgr
