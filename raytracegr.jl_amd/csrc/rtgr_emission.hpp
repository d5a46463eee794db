// rtgr_emission.hpp — an orbiting, glowing disk (include/rtgr.h "disk emission"): the emitter's orbital rate from the metric's own
// derivatives, the frequency ratio between the camera's static observer and that emitter, and the black-body colour it gives.  ONE device
// function, disk_emission<R>, which the emission kernel applies to the pixels of a frame and — the same kernel — to the points of the
// hook rtgr_eval_disk_emission_* (rtgr_emit.hip), so an emitted pixel and the hook at the same pair of states give the same bits.
//
// THE MODEL (everything in the scalar type R of the entry point; s0 = (x_0, k_0) the ray's state at the camera, se = (x_end, k_end) its
// state on the disk).
//
// The orbital rate.  The metric is stationary, axisymmetric about z and symmetric under z -> -z.  With psi = (0, -y, x, 0) the orbit of
// xi = d_t + Omega psi is a geodesic iff the gradient of g(xi, xi) vanishes at fixed Omega; by the symmetries only its radial component
// survives.  At the equatorial projection P = (t, x_end, y_end, 0), with D = x d_x + y d_y acting on the metric's components:
//     g_tpsi = -y g_tx + x g_ty                      g_psipsi = y² g_xx - 2 x y g_xy + x² g_yy
//     A = D g_tt       B = (-y D g_tx + x D g_ty) + g_tpsi       C = (y² D g_xx - 2 x y D g_xy + x² D g_yy) + 2 g_psipsi
//     C Omega² + 2 B Omega + A = 0:    Omega_± = (-B ± sqrt(B² - A C)) / C
// RTGR_EMIT_KEPLER takes the root `orbit` = ±1 names (+1: counter-clockwise seen from +z for a > 0); RTGR_EMIT_RIGID takes Omega = orbit.
// g and dg at P come from dmetric_dev (the built-in metrics, through forward duals) or sampled_metric (a 3-D grid): no closed form of
// Kerr's is used, so the rate is right for the reference's own metric (whose radius is not Kerr's) and for grids.
//
// The emitter.  xi = (1, -Omega y_end, Omega x_end, 0) at x_end itself (the disk has a thickness: it rotates on cylinders at the
// equatorial rate), n² = g(x_end)(xi, xi), u_emit = xi / sqrt(-n²).  VALID iff B² - A C >= 0, C != 0, Omega and n² finite, n² < 0.
//
// The frequency ratio.  g = (k_0 · u_obs) / (k_end · u_emit), u_obs the static observer at x_0 as in redshift_body (rtgr_camera.hpp),
// every inner product with the metric at the point where its vectors live.  A camera whose static observer is not timelike, or a g
// that is not finite, makes the point invalid as well.
//
// The colour.  A black body's I_nu / nu³ is invariant, so the observed spectrum is Planck's at g T_em:
//     rho = hypot(x_end, y_end)      T_em = T_in (rho / r_in)^(-p)      [RTGR_EMIT_INNER_EDGE: x sqrt(sqrt(max(1 - sqrt(r_in / rho), 0)))]
//     rgb_c = gain weight_c / expm1(theta_c / (g T_em))
// An invalid point, g <= 0 or a T_em that is not > 0 gives black and g = NaN; an invalid point also Omega = NaN and u_emit = NaN.
//
// The function's own expressions are not fused (fp contract off).  The metric code it calls — dmetric_dev's dual numbers, a grid's
// interpolant — is the library's, compiled as everywhere else; the function is therefore inlined into ONE kernel only (rtgr_emit.hip:
// emit_kernel, which serves the frame and the hook), so that a pixel and the hook cannot differ in what the compiler fused around it.
#pragma once
#include "rtgr_host.hpp"      // (DevEmission: the parameters as the host converted them)
#include "rtgr_tile.hpp"     // (rpow; it brings rtgr_camera.hpp)
#include "rtgr_texture.hpp"   // (rhypot, rfinite)

namespace rtgr {

template <class R> RTGR_DEV R rexpm1(R x);
template <> RTGR_DEV double rexpm1<double>(double x) { return expm1(x); }
template <> RTGR_DEV float rexpm1<float>(float x) { return expm1f(x); }

// g and dg of a stationary scene (a built-in metric or a 3-D grid) at x
template <class R>
RTGR_DEV void emission_dmetric(const DevScene<R>& sc, const R x[4], R g[4][4], R dg[4][4][4]) {
    if (sampled_on(sc.metric, 3)) sampled_metric<R, 3>(sc.grid, x, g, dg);
    else dmetric_dev<R>(sc.metric, sc.M, sc.a, x, g, dg);
}

// The orbital rate of the model above at the equatorial point (t, x, y, 0): the root `orbit` = ±1 names of C Omega² + 2 B Omega + A = 0.
// ok: B² - A C >= 0 and C != 0.  ONE function for the emitter (disk_emission) and for an observer on a circular orbit
// (rtgr_observer.hpp: observer_frame), so the two rates at one point are the same bits.
template <class R>
RTGR_DEV R circular_orbit_rate(const DevScene<R>& sc, R t, R x, R y, R orbit, bool& ok) {
#pragma clang fp contract(off)
    const R P[4] = {t, x, y, R(0)};
    R g[4][4], dg[4][4][4];
    emission_dmetric<R>(sc, P, g, dg);
    const R Dtt = x * dg[0][0][1] + y * dg[0][0][2], Dtx = x * dg[0][1][1] + y * dg[0][1][2], Dty = x * dg[0][2][1] + y * dg[0][2][2];
    const R Dxx = x * dg[1][1][1] + y * dg[1][1][2], Dxy = x * dg[1][2][1] + y * dg[1][2][2], Dyy = x * dg[2][2][1] + y * dg[2][2][2];
    const R gtp = x * g[0][2] - y * g[0][1];
    const R gpp = y * y * g[1][1] - R(2) * x * y * g[1][2] + x * x * g[2][2];
    const R A = Dtt;
    const R B = (x * Dty - y * Dtx) + gtp;
    const R C = (y * y * Dxx - R(2) * x * y * Dxy + x * x * Dyy) + R(2) * gpp;
    const R disc = B * B - A * C;
    ok = disc >= R(0) && C != R(0);
    return (orbit * rsqrt_(disc) - B) / C;   // (orbit = ±1 picks the root)
}

// The temperature law of the model above at cylindrical radius rho.  ONE function for the picture (disk_emission) and for the disk's
// thermal spectrum (rtgr_spectrum.hpp, in double); no operation is fused.
template <class R>
RTGR_DEV R emission_temperature(const DevEmission<R>& E, R rho) {
#pragma clang fp contract(off)
    R T = E.T_in * rpow<R>(rho / E.r_in, -E.p);
    if (E.flags & RTGR_EMIT_INNER_EDGE) {
        R edge = R(1) - rsqrt_(E.r_in / rho);
        edge = edge > R(0) ? edge : R(0);
        T = T * rsqrt_(rsqrt_(edge));
    }
    return T;
}

// The model above at one pair of states.  Returns whether the emitter is valid (and the frequency ratio finite); omega, uem, gred and
// rgb are always written.  obs (may be null): the frame of an observer camera (rtgr_observer.hpp) — u_obs is then its e_0 instead of
// the static observer at x_0.
template <class R>
RTGR_DEV bool disk_emission(const DevScene<R>& sc, const DevEmission<R>& E, const R s0[8], const R se[8], R& omega, R uem[4], R& gred, R rgb[3],
                            const ObsFrame<R>* obs = nullptr) {
#pragma clang fp contract(off)
    const R nan = R(__builtin_nan(""));
    const R x = se[1], y = se[2];
    bool ok = true;
    R Om;
    if (E.emitter == RTGR_EMIT_KEPLER) Om = circular_orbit_rate<R>(sc, se[0], x, y, E.orbit, ok);
    else Om = E.orbit;
    R ge[4][4], g0[4][4], tobs[4];
    metric_plain<R>(sc, se, ge);
    const R xi[4] = {R(1), -(Om * y), Om * x, R(0)};
    const R n2 = inner<R>(ge, xi, xi);
    ok = ok && rfinite(Om) && rfinite(n2) && n2 < R(0);
    const R sc_u = R(1) / rsqrt_(-n2);
    for (int c = 0; c < 4; c++) uem[c] = xi[c] * sc_u;
    bool ok0;
    metric_plain<R>(sc, s0, g0);
    if (obs) {
        ok0 = obs->valid != 0u;
        for (int c = 0; c < 4; c++) tobs[c] = obs->e[0][c];
    } else {
        static_observer<R>(g0, tobs, ok0);
    }
    const R num = inner<R>(g0, s0 + 4, tobs), den = inner<R>(ge, se + 4, uem);
    R gr = num / den;
    ok = ok && ok0 && rfinite(gr);
    rgb[0] = rgb[1] = rgb[2] = R(0);
    if (!ok) {
        omega = nan; gred = nan;
        for (int c = 0; c < 4; c++) uem[c] = nan;
        return false;
    }
    omega = Om;
    const R rho = rhypot<R>(x, y);
    const R T = emission_temperature<R>(E, rho);
    if (!(gr > R(0)) || !(T > R(0))) { gred = nan; return true; }
    gred = gr;
    const R gT = gr * T;
    for (int c = 0; c < 3; c++) rgb[c] = E.gain * E.weight[c] / rexpm1<R>(E.theta[c] / gT);
    return true;
}

}  // namespace rtgr
