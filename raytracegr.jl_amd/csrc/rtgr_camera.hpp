// rtgr_camera.hpp — make_canvas' pixel -> ray state (src/RayTraceGR.jl:457-478) and the redshift between observer and emitter
#pragma once
#include "rtgr_objects.hpp"

namespace rtgr {

// metric(x) with plain scalars (no duals): what make_canvas calls (:469).  NE says which sampled metric this instantiation can meet
// (Sampled<R, METRIC>::NE where the metric is a template parameter, by sampled_on(sc.metric, ·) where it is read at run time): 4 is the
// instantiation FOR a time-dependent grid — no other carries the 4-D interpolant —, 3 every other one, which finds a 3-D grid like a built-in.
template <class R, int NE = 3>
RTGR_DEV void metric_plain(const DevScene<R>& sc, const R x[4], R g[4][4]) {
#pragma clang fp contract(off)   // see make_pixel
    if constexpr (NE == 4) {
        R dg[4][4][4];   // (not read)
        sampled_metric<R, 4>(sc.grid, x, g, dg);
        return;
    }
#ifdef RTGR_USER_METRIC
    if (sc.metric == (uint32_t)RTGR_USER) {
        rtgr_user_metric<R>(x, (double)sc.M, (double)sc.a, g);
        return;
    }
#endif
    if (sampled_on(sc.metric, NE)) {
        R dg[4][4][4];   // (not read: the camera needs g only)
        sampled_metric<R, NE>(sc.grid, x, g, dg);
        return;
    }
    // built-ins are η + f k k
    R f = R(0), kk[4] = {R(1), R(0), R(0), R(0)};
    if (sc.metric != RTGR_MINKOWSKI) {
        KSField<R> F;
        if (sc.metric == RTGR_KS_REF) ks_field<R, RTGR_KS_REF, true>(x[1], x[2], x[3], sc.M, sc.a, F);
        else ks_field<R, RTGR_KS_TRUE, true>(x[1], x[2], x[3], sc.M, sc.a, F);
        f = F.f; kk[1] = F.k[0]; kk[2] = F.k[1]; kk[3] = F.k[2];
    }
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) g[p][q] = (p == q ? (p == 0 ? R(-1) : R(1)) : R(0)) + f * kk[p] * kk[q];
}

// ---- make_canvas pixel (src/RayTraceGR.jl:464-476): state (x, u) of pixel (i, j), 0-based -------------------------
template <class R, int NE = 3>
RTGR_DEV void make_pixel(const DevScene<R>& sc, const DevCamera<R>& cam, uint64_t ni, uint64_t nj, uint64_t i0,
                         uint64_t j0, R s[8]) {
    // No implicit contraction in the camera (here, metric_plain, ks_field, inv4sym): this function is inlined into
    // prepare_kernel — next to the RHS of the same point — AND into canvas_kernel, and -ffp-contract=fast decides fusions by
    // use counts after inlining and CSE: a product shared with the neighbouring code (a², ρ²) fused in one kernel and not in
    // the other, and the camera ray generated inside the pipeline differed from rtgr_make_canvas' in the last bit (round 3:
    // found by test_host_pipeline_with_many_chunks_and_every_output when the spin RHS changed).  Explicit rfma() stay FMAs.
#pragma clang fp contract(off)
    const R dx = (R(i0 + 1) - R(0.5)) / R(ni) - R(0.5);                               // :465
    const R dy = (R(j0 + 1) - R(0.5)) / R(nj) - R(0.5);                               // :466
    R x[4], n[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        x[c] = cam.pos[c] + dx * cam.widthx[c] + dy * cam.widthy[c];                  // :467
        n[c] = cam.normal[c] + dx * cam.widthx[c] + dy * cam.widthy[c];               // :468
    }
    R g[4][4];
    metric_plain<R, NE>(sc, x, g);                                                 // :469
    R gu[4][4];
    inv4sym<R>(g, gu);                                                                // :470
    R t[4];
#pragma unroll
    for (int p = 0; p < 4; p++) t[p] = gu[p][0];                                      // gu * e_t   :471
    R t2 = R(0), n2 = R(0);
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            t2 += t[p] * g[p][q] * t[q];                                              // :472
            n2 += n[p] * g[p][q] * n[q];                                              // :473
        }
    const R st = rsqrt_(-t2), sn = rsqrt_(n2), s2 = rsqrt_(R(2));
#pragma unroll
    for (int p = 0; p < 4; p++) {
        s[p] = x[p];
        s[4 + p] = (t[p] / st + n[p] / sn) / s2;                                      // :474
    }
}

// ---- redshift (rtgr_ray_outputs.redshift; SURVEY §8 f4: "Doppler/redshift via the unused Sphere.vel", :411, :416) --------
// g = (k·u_obs) / (k·u_emit): the ratio observed / emitted frequency of the light that reaches a pixel.
//   k      = tangent of the traced ray (an affinely parametrised null geodesic, so k is parallel-transported and the
//            ratio does not depend on its normalisation or on the direction the ray was traced in)
//   u_obs  = the static observer make_canvas builds every ray from, future-directed: −g^{-1} e_t / sqrt(−g(t,t)) at the
//            pixel (:471-472; the reference uses the past-directed sign because it traces rays backwards in time)
//   u_emit = Sphere: its `vel` (coordinate 4-velocity as stored in the reference's struct) normalised with the metric at
//            the hit point; Plane / Disk: the static observer t̂ there
//   ·      = the metric at the respective end of the ray — ANY metric: built-in or run-time compiled, Float64 or Float32
// NaN where nothing is hit, or where u_emit is not timelike (a static emitter inside the ergoregion, vel = 0, …).
template <class R>
RTGR_DEV void static_observer(const R g[4][4], R t[4], bool& ok) {
    R gu[4][4];
    inv4sym<R>(g, gu);
    R t2 = R(0);
    for (int p = 0; p < 4; p++) t[p] = gu[p][0];
    for (int p = 0; p < 4; p++)
        for (int q = 0; q < 4; q++) t2 += t[p] * g[p][q] * t[q];
    ok = t2 < R(0);
    const R s = R(-1) / rsqrt_(-t2);   // g^{-1} e_t points to the past (make_canvas builds past-directed rays from it); −: future
    for (int p = 0; p < 4; p++) t[p] *= s;
}
template <class R>
RTGR_DEV R inner(const R g[4][4], const R a[4], const R b[4]) {
    R acc = R(0);
    for (int p = 0; p < 4; p++)
        for (int q = 0; q < 4; q++) acc += a[p] * g[p][q] * b[q];
    return acc;
}
// one thread per ray; a body function so that run-time compiled metric units wrap it in kernels of their own (metric_plain
// dispatches to the unit's rtgr_user_metric there)
template <class R, int NE = 3>
RTGR_DEV void redshift_body(const DevScene<R>& sc, const DevCamera<R>& cam, const R* state0, uint64_t ni, uint64_t nj, uint64_t j0,
                            uint64_t jstride, uint64_t n, uint64_t out_offset, const R* state_end, const uint8_t* hit, const uint32_t* hit32, R* red) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const uint64_t idx = out_offset + w;
    const R nan = R(__builtin_nan(""));
    const uint32_t h = hit32 ? hit32[idx] : (uint32_t)hit[idx];
    if (h == 0 || h > sc.nobj) { red[idx] = nan; return; }
    R s0[8], se[8];
    if (state0) for (int c = 0; c < 8; c++) s0[c] = state0[w * 8 + c];
    else make_pixel<R, NE>(sc, cam, ni, nj, w % ni, j0 + (w / ni) * jstride, s0);
    for (int c = 0; c < 8; c++) se[c] = state_end[idx * 8 + c];
    R g0[4][4], ge[4][4], tobs[4], uem[4];
    bool ok0, oke;
    metric_plain<R, NE>(sc, s0, g0);
    static_observer<R>(g0, tobs, ok0);
    metric_plain<R, NE>(sc, se, ge);
    uint32_t pos = 0;                      // the hit map holds indices of the CALLER's list: find the object in the regrouped one
    for_each_object<R>(sc, [&](const DevObject<R>& o_, uint32_t o) { if (o_.orig + 1u == h) pos = o; });
    const DevObject<R>& ob = object_at<R>(sc, pos);
    if (ob.kind == RTGR_SPHERE) {
        const R v[4] = {ob.p[4], ob.p[5], ob.p[6], ob.p[7]};
        const R v2 = inner<R>(ge, v, v);
        oke = v2 < R(0);
        const R s = R(1) / rsqrt_(-v2);
        for (int p = 0; p < 4; p++) uem[p] = v[p] * s;
    } else {
        static_observer<R>(ge, uem, oke);
    }
    const R num = inner<R>(g0, s0 + 4, tobs), den = inner<R>(ge, se + 4, uem);
    red[idx] = (ok0 && oke) ? num / den : nan;
}

}  // namespace rtgr
