// rtgr_resolve.hpp — the resolve kernel, one thread per ray: root of cond(x(θ)) on [0, top], end state, colouring rule, stores
#pragma once
#include "rtgr_objects.hpp"

#ifndef RTGR_ROOT_SHORTCUT
#define RTGR_ROOT_SHORTCUT 1
#endif

namespace rtgr {

template <class R, bool SEL = false>
RTGR_DEV R cond_poly(const DevScene<R>& sc, const R x0[4], const R c[4][4], R th, ObjSel sel = ObjSel{}) {
    R x[4];
    poly_pos<R>(x0, c, th, x);
    return min_distance<R, SEL>(sc, x, sel);
}

// LONG LISTS.  The root-find below evaluates the condition — the minimum over ALL objects' distances (:433-441) — some ten times per
// event, and the colour rule once more: with N objects, ~10 N distances per ray, of which all but one or two are of objects nowhere
// near the step the event lies in.  For a list beyond the argument block the wave first narrows the list down: over the event's step
// every object's distance stays within d_i(0) ± B_i (the bounds of the FAR pass's reach test, from the box |x_q(θ) − x_q(0)| <= δ_q,
// θ in [0, top], that the step's polynomial spans), so the minimum never exceeds U = min_i (d_i(0) + B_i), and an object with
// d_i(0) − B_i > U is never the minimum — neither its value nor its index can enter a result, at any θ of the bracket.  The objects
// that SOME lane of the wave cannot leave out form the selection (one bit per object up to 64, per 2^shift neighbours beyond); the
// rays of a wave are neighbours on the canvas, so the selection is a handful of objects.  Same frame bit for bit (under test with
// option groups = 0, which switches this off too).  Guards as in the reach test: 1e-6 relative on the bound, a floor of 256 ulp of the
// operands' magnitude; a NaN anywhere keeps the object in.
template <class R>
RTGR_DEV ObjSel select_objects(const DevScene<R>& sc, const R x0[4], const R c[4][4], R top, bool event) {
    ObjSel sel{0ull, objsel_shift(sc.nobj), 0u, 0u};
    R dl[4];
#pragma unroll
    for (int q = 0; q < 4; q++) dl[q] = top * rfma(top, rfma(top, rfma(top, rabs(c[3][q]), rabs(c[2][q])), rabs(c[1][q])), rabs(c[0][q]));
    R U = R(__builtin_huge_val());
    auto upper = [&](const DevObject<R>& ob, uint32_t) {
        R lo, up;
        distance_bounds<R>(ob, x0, dl, &lo, &up);
        U = up < U ? up : U;
    };
    if (sc.ngroups == 0u) {   // a list without groups: every object twice
        for_each_object<R>(sc, upper);
        for_each_object<R>(sc, [&](const DevObject<R>& ob, uint32_t o) {
            R lo, up;
            distance_bounds<R>(ob, x0, dl, &lo, &up);
            if (__ballot(event && !(lo > U)) != 0ull) sel.add(o);
        });
        return sel;
    }
    // A grouped list (DevScene): the bound U may come from ANY objects — from a sample first (one member of every group, the loose
    // spheres, the other kinds).  A group whose bounding sphere stays farther than sqrt(U) away for the whole step holds no member
    // that can be the minimum: with m = |X_g| − R_g − |δ| > sqrt(U) >= 0 every member has |X_i(θ)| − r_i >= m, so its distance
    // (|X_i| − r_i)(|X_i| + r_i) >= m² > U (members have r_i >= 0: the host leaves inside-out spheres loose).  Such groups — and
    // runs of groups — are passed over when every lane agrees; the members that remain tighten the bound (U2: the minimum over the
    // sample AND over everything that passed, which holds the object the full list's bound comes from), and a last walk over what
    // passed keeps what the tight bound cannot leave out: the same selection as two walks over the whole list give.
    for_each_sample<R>(sc, upper);
    const R eps = sizeof(R) == 8 ? R(2.220446049250313e-16) : R(1.1920929e-7);
    const R guard = R(1) + R(1e-6);
    const R reach = guard * (rsqrt_(rfma(dl[1], dl[1], rfma(dl[2], dl[2], dl[3] * dl[3]))) + (U > R(0) ? rsqrt_(U) : R(0)));
    R U2 = U;
    auto member = [&](const DevObject<R>& ob, uint32_t o) {
        R lo, up;
        distance_bounds<R>(ob, x0, dl, &lo, &up);
        const bool in = !(lo > U);
        U2 = (in && up < U2) ? up : U2;
        if (__ballot(event && in) != 0ull) sel.add(o);
    };
    for_each_within_reach<R>(sc,
        [&](const DevObject<R>& G, int) -> bool {
            const R X0 = x0[1] - G.p[1], X1 = x0[2] - G.p[2], X2 = x0[3] - G.p[3];
            const R S = rfma(X0, X0, rfma(X1, X1, X2 * X2));
            const R t = G.p[8] + reach;
            const R rhs = t * t;
            const bool far_away = S > rfma(guard, rhs, R(256) * eps * (S + rhs));
            return __ballot(event && !far_away) != 0ull;
        },
        member, member);
    ObjSel fin{0ull, sel.shift, 0u, 0u};
    for_each_selected<R>(sc, sel, [&](const DevObject<R>& ob, uint32_t o) {
        R lo, up;
        distance_bounds<R>(ob, x0, dl, &lo, &up);
        if (__ballot(event && !(lo > U2)) != 0ull) fin.add(o);
    });
    return fin;
}

// Bracketed root of g(θ) = ps·cond(x(θ)) on [0, top], g(0) > 0 >= g(top).  Ridders' method: every iterate stays inside
// the bracket, the estimate x4 converges quadratically (the bracket WIDTH only halves per iteration, so convergence is
// judged on successive estimates).  Once the estimate has settled, probes 16 ulp before and after it pin the crossing:
// the result is a point with g >= 0 within ~32 ulp of it — the reference's prevfloat(find_zero(...))
// up to a few ulp (a 512-ulp window, 1e-13 in θ, for the rays whose distance is too noisy for that).  If the probes fail
// (estimate was off) the loop simply continues on the tightened bracket; the bisection point `mid` guarantees progress.
// -DRTGR_ROOT_STATS builds report the iteration count of every ray through lambda_end.
template <class R, bool SEL = false>
RTGR_DEV R event_root(const DevScene<R>& sc, const R x0[4], const R c[4][4], R ps, R top, int* iters = nullptr, ObjSel sel = ObjSel{}) {
    R lo = R(0), hi = top;
    R fhi = cond_poly<R, SEL>(sc, x0, c, hi, sel) * ps;
    R flo = cond_poly<R, SEL>(sc, x0, c, R(0), sel) * ps;
    R result = R(0);
    bool done = false;
    if (fhi == R(0)) { result = hi; done = true; }
    else if (!(flo > R(0)) || !(fhi < R(0))) { result = R(0); done = true; }
    const R eps = sizeof(R) == 8 ? R(2.220446049250313e-16) : R(1.1920929e-7);
    R est_prev = R(-1);
    for (int it = 0; it < 96 && !done; it++) {
        if (iters) *iters = it + 1;
        const R width = hi - lo;
        const R mid = rfma(R(0.5), width, lo);
        if (!(width > R(2) * eps * hi) || !(mid > lo && mid < hi)) {
            result = lo; done = true;
        } else {
            const R fm = cond_poly<R, SEL>(sc, x0, c, mid, sel) * ps;
            const R rad = rfma(fm, fm, -flo * fhi);  // > 0 since flo > 0 > fhi
            // Ridders' estimate.  When one end of the bracket already sits on the root (|g(lo)| ~ 1e-17 after a lucky
            // iterate) the formula returns that end itself: the point to EVALUATE is then the midpoint (progress), but the
            // ESTIMATE is the end — without this distinction such rays never "settled" and bisected 45 more times
            // (0.3 % of the rays, 13-50 iterations; their waves waited: 4 iterations per ray, 10.5 per wave).
            const R xr = rfma((mid - lo) * fm, frsq<R>(rad), mid);
            const bool inside = xr > lo && xr < hi;
            const R x4 = inside ? xr : mid;
            const R est = inside ? xr : (xr <= lo ? lo : (xr >= hi ? hi : mid));
            const R f4 = (x4 == mid) ? fm : cond_poly<R, SEL>(sc, x0, c, x4, sel) * ps;
            // An exact zero is common (a plane at a representable time makes g vanish on a whole ulp-interval of θ):
            // "directly at zero" is an accepted result, so stop there.
            if (fm == R(0)) { result = mid; done = true; }
            else if (f4 == R(0)) { result = x4; done = true; }
            const R a = rmin(mid, x4), b = rmax(mid, x4);
            const R fa = (mid <= x4) ? fm : f4, fb = (mid <= x4) ? f4 : fm;
            if (fa > R(0)) {
                lo = a; flo = fa;
                if (fb > R(0)) { lo = b; flo = fb; } else { hi = b; fhi = fb; }
            } else {
                hi = a; fhi = fa;
            }
            // two successive estimates within 256 ulp: converged down to the rounding noise of the distance itself
            // (ulp of max(θ, top/16): the noise is absolute in θ — λ = t + hθ is what matters — so a root near θ = 0
            //  must not be chased to ITS ulp)
            const R scale = rmax(est, R(0.0625) * top);
            const bool settled = RTGR_ROOT_SHORTCUT && (rabs(est - est_prev) <= R(256) * eps * scale);
            est_prev = est;
            if (settled && !done) {
                // Verify the settled estimate two-sidedly: 16 ulp before and after; if the sign change is not in there
                // (the distance is evaluated with a rounding noise of ~10 ulp of θ, which makes the estimates jitter and
                // can push the crossing out), 512 ulp.  Rays that never pass fall back to ~50 bisection steps on the
                // one-sided Ridders bracket, and their whole wave waits for them (measured with an 8-ulp settle test
                // and the 16-ulp window only: mean 5.4 iterations per ray, 15.7 per wave).
#pragma unroll 1
                for (int pass = 0; pass < 2 && !done; pass++) {
                    const R wd = (pass == 0 ? R(16) : R(512)) * eps;
                    const R pm = rmax(rfma(-wd, scale, est), lo), pp = rmin(rfma(wd, scale, est), hi);
                    const R fpm = (pm > lo) ? cond_poly<R, SEL>(sc, x0, c, pm, sel) * ps : flo;
                    const R fpp = (pp < hi) ? cond_poly<R, SEL>(sc, x0, c, pp, sel) * ps : fhi;
                    if (!(fpm < R(0)) && !(fpp > R(0))) {
                        result = pm; done = true;  // the sign change (or an exact zero at pm) is inside [pm, pp]
                    } else if (fpp == R(0)) {
                        result = pp; done = true;
                    } else {
                        // the crossing is elsewhere: tighten the bracket with what was learnt
                        if (fpm > R(0)) { lo = pm; flo = fpm; } else { hi = pm; fhi = fpm; }
                        if (fpp > R(0)) { if (pp > lo) { lo = pp; flo = fpp; } } else if (pp < hi) { hi = pp; fhi = fpp; }
                    }
                }
                if (!done) est_prev = R(-1);
            }
        }
    }
    return done ? result : lo;
}
#ifdef RTGR_ROOT_STATS
#define RTGR_ROOT_STATS_ARG , &root_iters
#else
#define RTGR_ROOT_STATS_ARG , nullptr
#endif

// the stores of one resolved ray
template <class R>
RTGR_DEV void resolve_store(const ResolveArgs<R>& A, uint64_t w, const RecRef<const R>& rec, const R xe[4], R Theta, R t, R h, const R col[3],
                            uint32_t hit, R ps, int root_iters) {
    (void)root_iters;
    const uint64_t idx = A.offset + w;
    A.rgb[idx] = col[0];
    A.rgb[A.n_slab + idx] = col[1];
    A.rgb[2 * A.n_slab + idx] = col[2];
    const uint32_t* mt = A.meta + w * 3;
    if (A.state_end) {
        R* se = A.state_end + idx * 8;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            se[q] = xe[q];
            R ue = rec[REC_U + q];
            if (ps != R(0)) {
                const R* cu = rec.tail + (REC_CU - HAND_W);
                ue = rfma(Theta, rfma(Theta, rfma(Theta, rfma(Theta, cu[12 + q], cu[8 + q]), cu[4 + q]), cu[q]), ue);
            }
            se[4 + q] = ue;
        }
    }
#ifdef RTGR_ROOT_STATS
    if (A.lambda_end) A.lambda_end[idx] = (R)root_iters;  // debug build: iterations of the root find
#else
    if (A.lambda_end) A.lambda_end[idx] = rfma(h, Theta, t);
#endif
    if (A.status) A.status[idx] = (uint8_t)(mt[2] & 0xffu);
    if (A.hit) A.hit[idx] = (uint8_t)hit;
    if (A.hit32) A.hit32[idx] = hit;
    if (A.n_accept) A.n_accept[idx] = mt[0];
    if (A.n_reject) A.n_reject[idx] = mt[1];
}
// resolve_body (below) with the list narrowed down first (select_objects): lists beyond the argument block
template <class R>
RTGR_DEV void resolve_body_selected(const ResolveArgs<R>& A) {
    const uint64_t w0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = w0 < A.n;
    const uint64_t w = live ? w0 : A.n - 1;   // (every lane of the wave takes part in the selection's ballots; the spare ones repeat the last ray, silently)
    const RecRef<const R> rec{A.hand + w * HAND_W, A.rec + w * (uint64_t)A.recw};
    R x0[4], xe[4];
#pragma unroll
    for (int q = 0; q < 4; q++) xe[q] = x0[q] = rec[REC_X + q];
    const R ps = rec[REC_PS], top = rec[REC_TOP], t = rec[REC_T], h = rec[REC_H];
    R Theta = R(0);
    int root_iters = 0;
    (void)root_iters;
    const bool event = ps != R(0);
    R c[4][4];
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
        for (int q = 0; q < 4; q++) c[m][q] = event ? rec[REC_C + 4 * m + q] : R(0);
    ObjSel sel = select_objects<R>(A.sc, x0, c, event ? top : R(0), event);
    if (event) {
        Theta = event_root<R, true>(A.sc, x0, c, ps, top RTGR_ROOT_STATS_ARG, sel);
        poly_pos<R>(x0, c, Theta, xe);
    }
    // (a ray without an event is coloured where it stopped: nothing is known about that point — every object is asked)
    if (__ballot(!event) != 0ull) { sel.mask = ~0ull; sel.count = 65u; }
    R col[3];
    const uint32_t hit = colour_pixel<R, true>(A.sc, A.opt, xe, col, sel);
    if (live) resolve_store<R>(A, w, rec, xe, Theta, t, h, col, hit, ps, root_iters);
}
// (a body function: a unit with user objects wraps it in a resolve kernel of its own — the root-find evaluates the objects'
//  distances and the colour rule their objcolor)
template <class R>
RTGR_DEV void resolve_body(const ResolveArgs<R>& A) {
    if (__builtin_expect(A.select != 0u && A.sc.nobj > (uint32_t)RTGR_MAX_OBJECTS && A.n != 0, 0)) { resolve_body_selected<R>(A); return; }
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= A.n) return;
    const RecRef<const R> rec{A.hand + w * HAND_W, A.rec + w * (uint64_t)A.recw};
    R x0[4], xe[4];
#pragma unroll
    for (int q = 0; q < 4; q++) xe[q] = x0[q] = rec[REC_X + q];
    const R ps = rec[REC_PS], top = rec[REC_TOP], t = rec[REC_T], h = rec[REC_H];
    R Theta = R(0);
    int root_iters = 0;
    (void)root_iters;
    if (ps != R(0)) {  // an event: the polynomial part of the record is valid
        R c[4][4];
#pragma unroll
        for (int m = 0; m < 4; m++)
#pragma unroll
            for (int q = 0; q < 4; q++) c[m][q] = rec[REC_C + 4 * m + q];
        Theta = event_root<R>(A.sc, x0, c, ps, top RTGR_ROOT_STATS_ARG);
        poly_pos<R>(x0, c, Theta, xe);
    }
    R col[3];
    const uint32_t hit = colour_pixel<R>(A.sc, A.opt, xe, col);
    resolve_store<R>(A, w, rec, xe, Theta, t, h, col, hit, ps, root_iters);
}
template <class R>
__global__ __launch_bounds__(256) void resolve_kernel(const ResolveArgs<R> A) {
    resolve_body<R>(A);
}

}  // namespace rtgr
