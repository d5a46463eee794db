// rtgr_observer.hpp — the observer camera (include/rtgr.h "observer camera"): a pinhole at ONE event, carried by an observer who is at
// rest in the slicing, moves with a given 4-velocity or rides a circular orbit.  Two device functions: observer_frame<R>, which builds
// the observer's orthonormal frame from the caller's record, and observer_ray<R>, the state of pixel (i, j) in that frame.  Both are
// inlined into ONE kernel each (rtgr_observer.hip), which the traced frame, rtgr_make_observer_canvas_* and the hook rtgr_eval_observer_*
// all run: the hook predicts a traced ray's start state to the bit.
//
// THE FRAME (everything in the scalar type R of the entry point; every inner product with g = the metric at pos, metric_plain).
//   u        RTGR_OBS_STATIC    static_observer(g) of rtgr_camera.hpp — -g^{-1} e_t, normalised, future-directed — taken as e_0 as it is
//            RTGR_OBS_VELOCITY  the caller's vel;  e_0 = vel / sqrt(-g(vel, vel))
//            RTGR_OBS_CIRCULAR  xi = (1, -Omega y, Omega x, 0), Omega = circular_orbit_rate (rtgr_emission.hpp: the emitter's own function)
//                               at (t, x, y, 0), root `orbit`;  e_0 = xi / sqrt(-g(xi, xi))
//   e_look   = normalise(look + g(look, e_0) e_0)
//   e_up     = normalise(up + g(up, e_0) e_0 - g(up, e_look) e_look)
//   e_right  (lowered)_a = -sqrt(-det g) eps_{abcd} e_0^b e_look^c e_up^d, eps_0123 = +1, raised with g^{-1}: "right = look x up" at rest
//            in flat space (u = d_t, look = +y, up = +z gives +x).
// VALID iff u is timelike and future-directed (u^t > 0: t is a time function of every metric the library traces), for CIRCULAR
// B² - A C >= 0, C != 0 and g(xi, xi) < 0, det g < 0, the projected look and up are not degenerate — the squared norm of the projected
// vector exceeds 4096 eps(R) times sum |v^a g_ab v^b| of the vector given — and every entry of the frame is finite.
//
// THE PIXEL.  a = 2 (i + 1/2) / ni - 1, b = 2 (j + 1/2) / nj - 1 (i along e_right, j along e_up, 0-based).
//   RTGR_PROJ_PERSPECTIVE  v = e_look + a hx e_right + b hy e_up, hx = tan(fov_x / 2), hy = tan(fov_y / 2);  n = v / sqrt(g(v, v))
//   RTGR_PROJ_EQUIRECT     alpha = a hx, beta = b hy, hx = fov_x / 2, hy = fov_y / 2;
//                          n = cos beta (cos alpha e_look + sin alpha e_right) + sin beta e_up
//   state: x = pos, k = (-e_0 + n) / sqrt(2) — null, past-directed, make_canvas' normalisation (src/RayTraceGR.jl:474).
// An invalid frame gives NaN in all eight scalars of every ray; prepare_kernel ends such a ray as RTGR_RAY_NAN.
//
// No operation of the two functions is fused (fp contract off).  static_observer and the metric code behind circular_orbit_rate are
// the library's, compiled as everywhere else.
#pragma once
#include "rtgr_emission.hpp"

namespace rtgr {

template <class R> RTGR_DEV R rsin(R x);
template <> RTGR_DEV double rsin<double>(double x) { return sin(x); }
template <> RTGR_DEV float rsin<float>(float x) { return sinf(x); }
template <class R> RTGR_DEV R rcos(R x);
template <> RTGR_DEV double rcos<double>(double x) { return cos(x); }
template <> RTGR_DEV float rcos<float>(float x) { return cosf(x); }
template <class R> RTGR_DEV R obs_eps();
template <> RTGR_DEV double obs_eps<double>() { return 2.220446049250313e-16; }
template <> RTGR_DEV float obs_eps<float>() { return 1.1920929e-7f; }

// g(a, b) with nothing fused (rtgr_camera.hpp's inner is compiled with the library's contraction)
template <class R>
RTGR_DEV R obs_inner(const R g[4][4], const R a[4], const R b[4]) {
#pragma clang fp contract(off)
    R acc = R(0);
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc += a[p] * g[p][q] * b[q];
    return acc;
}
// sum |a^p g_pq a^q|: the scale a squared norm is held against
template <class R>
RTGR_DEV R obs_scale(const R g[4][4], const R a[4]) {
#pragma clang fp contract(off)
    R acc = R(0);
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) acc += rabs<R>(a[p] * g[p][q] * a[q]);
    return acc;
}
template <class R>
RTGR_DEV R obs_det3(R a0, R a1, R a2, R b0, R b1, R b2, R c0, R c1, R c2) {
#pragma clang fp contract(off)
    return a0 * (b1 * c2 - b2 * c1) - a1 * (b0 * c2 - b2 * c0) + a2 * (b0 * c1 - b1 * c0);
}
// det of a 4 x 4 matrix by the 2 x 2 minors inv4sym uses
template <class R>
RTGR_DEV R obs_det4(const R m[4][4]) {
#pragma clang fp contract(off)
    const R s0 = m[0][0] * m[1][1] - m[1][0] * m[0][1], s1 = m[0][0] * m[1][2] - m[1][0] * m[0][2];
    const R s2 = m[0][0] * m[1][3] - m[1][0] * m[0][3], s3 = m[0][1] * m[1][2] - m[1][1] * m[0][2];
    const R s4 = m[0][1] * m[1][3] - m[1][1] * m[0][3], s5 = m[0][2] * m[1][3] - m[1][2] * m[0][3];
    const R c5 = m[2][2] * m[3][3] - m[3][2] * m[2][3], c4 = m[2][1] * m[3][3] - m[3][1] * m[2][3];
    const R c3 = m[2][1] * m[3][2] - m[3][1] * m[2][2], c2 = m[2][0] * m[3][3] - m[3][0] * m[2][3];
    const R c1 = m[2][0] * m[3][2] - m[3][0] * m[2][2], c0 = m[2][0] * m[3][1] - m[3][0] * m[2][1];
    return s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
}

// The frame of the header comment.  F is always written in full; F.valid says whether it may be used.
template <class R>
RTGR_DEV void observer_frame(const DevScene<R>& sc, const DevObserver<R>& ob, ObsFrame<R>& F) {
#pragma clang fp contract(off)
    const R nan = R(__builtin_nan(""));
    R g[4][4], e0[4], el[4], eu[4], er[4];
    metric_plain<R>(sc, ob.pos, g);
    bool ok = true;
    R Om = nan;
    if (ob.kind == RTGR_OBS_STATIC) {
        static_observer<R>(g, e0, ok);
    } else {
        R u[4];
        if (ob.kind == RTGR_OBS_CIRCULAR) {
            Om = circular_orbit_rate<R>(sc, ob.pos[0], ob.pos[1], ob.pos[2], ob.orbit, ok);
            u[0] = R(1); u[1] = -(Om * ob.pos[2]); u[2] = Om * ob.pos[1]; u[3] = R(0);
            ok = ok && rfinite(Om);
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++) u[c] = ob.vel[c];
        }
        const R n2 = obs_inner<R>(g, u, u);
        ok = ok && rfinite(n2) && n2 < R(0);
        const R s = R(1) / rsqrt_(-n2);
#pragma unroll
        for (int c = 0; c < 4; c++) e0[c] = u[c] * s;
    }
    ok = ok && e0[0] > R(0);
    // look and up, projected and normalised
    const R tol = R(4096) * obs_eps<R>();
    {
        const R a = obs_inner<R>(g, ob.look, e0);
        R v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = ob.look[c] + a * e0[c];
        const R q = obs_inner<R>(g, v, v);
        ok = ok && q > tol * obs_scale<R>(g, ob.look);
        const R s = R(1) / rsqrt_(q);
#pragma unroll
        for (int c = 0; c < 4; c++) el[c] = v[c] * s;
    }
    {
        const R a = obs_inner<R>(g, ob.up, e0), b = obs_inner<R>(g, ob.up, el);
        R v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = ob.up[c] + a * e0[c] - b * el[c];
        const R q = obs_inner<R>(g, v, v);
        ok = ok && q > tol * obs_scale<R>(g, ob.up);
        const R s = R(1) / rsqrt_(q);
#pragma unroll
        for (int c = 0; c < 4; c++) eu[c] = v[c] * s;
    }
    // e_right: lowered by the volume form, raised by g^{-1}.  eps_{abcd} A^b B^c C^d = (-1)^a det of (A, B, C) without column a.
    {
        const R det = obs_det4<R>(g);
        ok = ok && det < R(0);
        const R w = -rsqrt_(-det);
        R lo[4], gu[4][4];
        lo[0] = w * obs_det3<R>(e0[1], e0[2], e0[3], el[1], el[2], el[3], eu[1], eu[2], eu[3]);
        lo[1] = -(w * obs_det3<R>(e0[0], e0[2], e0[3], el[0], el[2], el[3], eu[0], eu[2], eu[3]));
        lo[2] = w * obs_det3<R>(e0[0], e0[1], e0[3], el[0], el[1], el[3], eu[0], eu[1], eu[3]);
        lo[3] = -(w * obs_det3<R>(e0[0], e0[1], e0[2], el[0], el[1], el[2], eu[0], eu[1], eu[2]));
        inv4sym<R>(g, gu);
#pragma unroll
        for (int p = 0; p < 4; p++) er[p] = gu[p][0] * lo[0] + gu[p][1] * lo[1] + gu[p][2] * lo[2] + gu[p][3] * lo[3];
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        ok = ok && rfinite(ob.pos[c]) && rfinite(e0[c]) && rfinite(er[c]) && rfinite(eu[c]) && rfinite(el[c]);
        F.pos[c] = ob.pos[c];
        F.e[0][c] = e0[c]; F.e[1][c] = er[c]; F.e[2][c] = eu[c]; F.e[3][c] = el[c];
#pragma unroll
        for (int q = 0; q < 4; q++) F.g[c][q] = g[c][q];
    }
    F.omega = Om; F.hx = ob.hx; F.hy = ob.hy;
    F.valid = ok ? 1u : 0u;
    F.projection = ob.projection;
}

// The state of pixel (i, j), 0-based, of the ni x nj canvas in frame F.
template <class R>
RTGR_DEV void observer_ray(const ObsFrame<R>& F, uint64_t ni, uint64_t nj, uint64_t i, uint64_t j, R s[8]) {
#pragma clang fp contract(off)
    if (!F.valid) {
        // The NaN goes through a vector register: as eight wave-uniform constants the compiler keeps them in scalar pairs and writes
        // the Float64 ones with `s_mov_b64 s[..], 0x7ff8000000000000` — a 32-bit literal, which lands in the LOW half: a denormal, not a
        // NaN, came out in x (ROCm 7.2, gfx950; found by tests/test_observer.py's invalid frames).
        R nanv = R(__builtin_nan(""));
        asm volatile("" : "+v"(nanv));
#pragma unroll
        for (int c = 0; c < 8; c++) s[c] = nanv;
        return;
    }
    const R a = R(2) * (R(i) + R(0.5)) / R(ni) - R(1);
    const R b = R(2) * (R(j) + R(0.5)) / R(nj) - R(1);
    R n[4];
    if (F.projection == RTGR_PROJ_EQUIRECT) {
        const R al = a * F.hx, be = b * F.hy;
        const R ca = rcos<R>(al), sa = rsin<R>(al), cb = rcos<R>(be), sb = rsin<R>(be);
#pragma unroll
        for (int c = 0; c < 4; c++) n[c] = cb * (ca * F.e[3][c] + sa * F.e[1][c]) + sb * F.e[2][c];
    } else {
        const R ax = a * F.hx, by = b * F.hy;
        R v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) v[c] = F.e[3][c] + ax * F.e[1][c] + by * F.e[2][c];
        const R sn = rsqrt_(obs_inner<R>(F.g, v, v));
#pragma unroll
        for (int c = 0; c < 4; c++) n[c] = v[c] / sn;
    }
    const R s2 = rsqrt_(R(2));
#pragma unroll
    for (int c = 0; c < 4; c++) {
        s[c] = F.pos[c];
        s[4 + c] = (n[c] - F.e[0][c]) / s2;
    }
}

}  // namespace rtgr
