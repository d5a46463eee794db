// rtgr_tile.hpp — the simple tile kernel (trace_kernel, knob tile = 1): device-side Tsit5 + PI controller + ContinuousCallback for one ray per lane.
//
// Replaces, for the call site src/RayTraceGR.jl:510-511
//     solve(probs, Tsit5(), callback=cb, trajectories=N, reltol=tol, abstol=tol)
// the un-vendored third-party machinery the reference leans on (OrdinaryDiffEq 5.38.3 Tsit5 step + PI controller +
// Hairer initial dt; DiffEqBase 6.35.2 ContinuousCallback with 10 interpolation points; Roots bracketing
// root-find), as restated in SURVEY.md App. A/B.  One wavefront lane owns one ray; state, the 7 stage derivatives
// and the RHS temporaries all live in VGPRs.
#pragma once
#include "rtgr_camera.hpp"

namespace rtgr {

template <class R>
struct Tsit5C {
    static constexpr R a21 = R(0.161L);
    static constexpr R a31 = R(-0.008480655492356989L), a32 = R(0.335480655492357L);
    static constexpr R a41 = R(2.8971530571054935L), a42 = R(-6.359448489975075L), a43 = R(4.3622954328695815L);
    static constexpr R a51 = R(5.325864828439257L), a52 = R(-11.748883564062828L), a53 = R(7.4955393428898365L),
                       a54 = R(-0.09249506636175525L);
    static constexpr R a61 = R(5.86145544294642L), a62 = R(-12.92096931784711L), a63 = R(8.159367898576159L),
                       a64 = R(-0.071584973281401L), a65 = R(-0.028269050394068383L);
    static constexpr R a71 = R(0.09646076681806523L), a72 = R(0.01L), a73 = R(0.4798896504144996L),
                       a74 = R(1.379008574103742L), a75 = R(-3.290069515436081L), a76 = R(2.324710524099774L);
    static constexpr R bt1 = R(-0.00178001105222577714L), bt2 = R(-0.0008164344596567469L),
                       bt3 = R(0.007880878010261995L), bt4 = R(-0.1447110071732629L), bt5 = R(0.5823571654525552L),
                       bt6 = R(-0.45808210592918697L), bt7 = R(0.015151515151515152L);
    // dense output rows r[i][m]: b_i(θ) = Σ_m r[i][m] θ^(m+1)
    static constexpr R r[7][4] = {
        {R(1.0L), R(-2.763706197274826L), R(2.9132554618219126L), R(-1.0530884977290216L)},
        {R(0), R(0.13169999999999998L), R(-0.2234L), R(0.1017L)},
        {R(0), R(3.9302962368947516L), R(-5.941033872131505L), R(2.490627285651252793L)},
        {R(0), R(-12.411077166933676L), R(30.33818863028232L), R(-16.548102889244902L)},
        {R(0), R(37.50931341651104L), R(-88.1789048947664L), R(47.37952196281928L)},
        {R(0), R(-27.896526289197286L), R(65.09189467479366L), R(-34.87065786149661L)},
        {R(0), R(1.5L), R(-4.0L), R(2.5L)}};
};

template <class R> RTGR_DEV R rpow(R x, R y);
template <> RTGR_DEV double rpow<double>(double x, double y) { return pow(x, y); }
template <> RTGR_DEV float rpow<float>(float x, float y) { return powf(x, y); }
template <class R> RTGR_DEV R rlog10(R x);
template <> RTGR_DEV double rlog10<double>(double x) { return log10(x); }
template <> RTGR_DEV float rlog10<float>(float x) { return log10f(x); }

template <class R>
RTGR_DEV R rms8(const R v[8]) {  // ODE_DEFAULT_NORM, SURVEY App. B.1
    R acc = R(0);
#pragma unroll
    for (int i = 0; i < 8; i++) acc = rfma(v[i], v[i], acc);
    return rsqrt_(acc * R(0.125));
}

// b_i(θ), i = 0..6
template <class R>
RTGR_DEV void dense_weights(R th, R b[7]) {
    using C = Tsit5C<R>;
#pragma unroll
    for (int i = 0; i < 7; i++) b[i] = th * rfma(th, rfma(th, rfma(th, C::r[i][3], C::r[i][2]), C::r[i][1]), C::r[i][0]);
}

// position part of the dense output: x(θ) = y0[0..3] + h Σ b_i k_i[0..3]
template <class R>
RTGR_DEV void dense_pos(const R y[8], R h, const R k[7][8], R th, R x[4]) {
    R b[7];
    dense_weights<R>(th, b);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        R acc = b[0] * k[0][c];
#pragma unroll
        for (int i = 1; i < 7; i++) acc = rfma(b[i], k[i][c], acc);
        x[c] = rfma(h, acc, y[c]);
    }
}

template <class R>
RTGR_DEV void dense_full(const R y[8], R h, const R k[7][8], R th, R out[8]) {
    R b[7];
    dense_weights<R>(th, b);
#pragma unroll
    for (int c = 0; c < 8; c++) {
        R acc = b[0] * k[0][c];
#pragma unroll
        for (int i = 1; i < 7; i++) acc = rfma(b[i], k[i][c], acc);
        out[c] = rfma(h, acc, y[c]);
    }
}

struct RayStats {
    uint32_t nacc, nrej, nrhs;
    uint8_t status, interior;
};

// Hairer initial step, SURVEY App. B.3.  f0 = f(y) on entry; uses one more RHS evaluation.
template <class R, int METRIC, bool SPIN>
RTGR_DEV R initial_dt(const R y[8], const R f0[8], R M, R a, R abstol, R reltol, R dtmax) {
    R sk[8], tmp[8];
#pragma unroll
    for (int i = 0; i < 8; i++) sk[i] = R(1) / rfma(rabs(y[i]), reltol, abstol);
#pragma unroll
    for (int i = 0; i < 8; i++) tmp[i] = y[i] * sk[i];
    const R d0 = rms8(tmp);
#pragma unroll
    for (int i = 0; i < 8; i++) tmp[i] = f0[i] * sk[i];
    const R d1 = rms8(tmp);
    R dt0 = (d0 < R(1e-5) || d1 < R(1e-5)) ? R(1e-6) : (d0 / d1) * R(0.01);
    dt0 = rmin(dt0, dtmax);
    R u1[8], f1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) u1[i] = rfma(dt0, f0[i], y[i]);
    rhs<R, METRIC, SPIN>(u1, M, a, f1);
#pragma unroll
    for (int i = 0; i < 8; i++) tmp[i] = (f1[i] - f0[i]) * sk[i];
    const R d2 = rms8(tmp) / dt0;
    const R md = rmax(d1, d2);
    R dt1;
    if (md <= R(1e-15)) dt1 = rmax(R(1e-6), dt0 * R(1e-3));
    else dt1 = rpow<R>(R(10), -(R(2) + rlog10<R>(md)) * R(0.2));
    return rmin(rmin(R(100) * dt0, dt1), dtmax);
}

// One full trajectory.  Returns the end state (`sol[end]`) and λ_end (`sol.t[end]`, src/RayTraceGR.jl:503-504).
template <class R, int METRIC, bool SPIN>
RTGR_DEV RayStats integrate_ray(const DevScene<R>& sc, const DevSolver<R>& opt, const R s0[8], R s_end[8], R& lam_end) {
    using C = Tsit5C<R>;
    const R M = sc.M, a = sc.a;
    const R reltol = opt.reltol, abstol = opt.abstol;
    const R t1 = opt.lambda1;
    const R dtmax = opt.lambda1 - opt.lambda0;
    const R beta1 = R(0.14L), beta2 = R(0.08L), igamma = R(1) / R(0.9L);
    const R qmin_inv = R(5), qmax_inv = R(0.1L), qoldinit = R(1e-4L);
    RayStats st{0, 0, 0, RTGR_RAY_LAMBDA1, 0};

    R y[8], k[7][8];
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = s0[i];
    R t = opt.lambda0;
    rhs<R, METRIC, SPIN>(y, M, a, k[0]);
    R dt = initial_dt<R, METRIC, SPIN>(y, k[0], M, a, abstol, reltol, dtmax);
    st.nrhs = 2;
    R qold = qoldinit;
    R prev_cond = min_distance<R>(sc, y);
    const int npts = (int)opt.interp_points;
    const R dth = npts > 1 ? R(1) / R(npts - 1) : R(1);

    for (;;) {
        if (!(t < t1)) { st.status = RTGR_RAY_LAMBDA1; break; }
        if (st.nacc + st.nrej >= opt.max_steps) { st.status = RTGR_RAY_MAXSTEPS; break; }
        dt = rmin(dt, t1 - t);
        // ---- Tsit5 attempt --------------------------------------------------------------
        R Y[8], yn[8];
        const R h = dt;
#pragma unroll
        for (int i = 0; i < 8; i++) Y[i] = rfma(h * C::a21, k[0][i], y[i]);
        rhs<R, METRIC, SPIN>(Y, M, a, k[1]);
#pragma unroll
        for (int i = 0; i < 8; i++) Y[i] = rfma(h, rfma(C::a32, k[1][i], C::a31 * k[0][i]), y[i]);
        rhs<R, METRIC, SPIN>(Y, M, a, k[2]);
#pragma unroll
        for (int i = 0; i < 8; i++)
            Y[i] = rfma(h, rfma(C::a43, k[2][i], rfma(C::a42, k[1][i], C::a41 * k[0][i])), y[i]);
        rhs<R, METRIC, SPIN>(Y, M, a, k[3]);
#pragma unroll
        for (int i = 0; i < 8; i++)
            Y[i] = rfma(h, rfma(C::a54, k[3][i], rfma(C::a53, k[2][i], rfma(C::a52, k[1][i], C::a51 * k[0][i]))), y[i]);
        rhs<R, METRIC, SPIN>(Y, M, a, k[4]);
#pragma unroll
        for (int i = 0; i < 8; i++)
            Y[i] = rfma(h, rfma(C::a65, k[4][i], rfma(C::a64, k[3][i], rfma(C::a63, k[2][i],
                        rfma(C::a62, k[1][i], C::a61 * k[0][i])))), y[i]);
        rhs<R, METRIC, SPIN>(Y, M, a, k[5]);
#pragma unroll
        for (int i = 0; i < 8; i++)
            yn[i] = rfma(h, rfma(C::a76, k[5][i], rfma(C::a75, k[4][i], rfma(C::a74, k[3][i], rfma(C::a73, k[2][i],
                         rfma(C::a72, k[1][i], C::a71 * k[0][i]))))), y[i]);
        rhs<R, METRIC, SPIN>(yn, M, a, k[6]);
        st.nrhs += 6;
        R acc = R(0);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const R ut = h * rfma(C::bt7, k[6][i], rfma(C::bt6, k[5][i], rfma(C::bt5, k[4][i], rfma(C::bt4, k[3][i],
                             rfma(C::bt3, k[2][i], rfma(C::bt2, k[1][i], C::bt1 * k[0][i]))))));
            const R res = ut / rfma(rmax(rabs(y[i]), rabs(yn[i])), reltol, abstol);
            acc = rfma(res, res, acc);
        }
        const R EEst = rsqrt_(acc * R(0.125));
        if (EEst != EEst) { st.status = RTGR_RAY_NAN; break; }
        // ---- PI controller --------------------------------------------------------------
        R q, q11 = R(0);
        if (EEst == R(0)) q = qmax_inv;
        else {
            q11 = rpow<R>(EEst, beta1);
            q = q11 / rpow<R>(qold, beta2);
            q = rmax(qmax_inv, rmin(qmin_inv, q * igamma));
        }
        if (EEst <= R(1)) {
            st.nacc++;
            qold = rmax(EEst, qoldinit);
            const R dtnew = dt / q;
            R tnew = t + dt;
            if (rabs(tnew - t1) < R(10) * R(sizeof(R) == 8 ? 2.220446049250313e-16 : 1.1920929e-7) * rmax(rabs(tnew), rabs(t1)))
                tnew = t1;
            // ---- ContinuousCallback -----------------------------------------------------
            const R next_cond = min_distance<R>(sc, yn);
            const R ps = rsign(prev_cond);
            bool event = false;
            R top = R(1);
            if (ps != R(0)) {
                if (ps * rsign(next_cond) <= R(0)) {
                    event = true;
                } else {
                    for (int i = 2; i <= npts; i++) {
                        const R th = R(i - 1) * dth;
                        R xi[4];
                        dense_pos<R>(y, h, k, th, xi);
                        if (ps * rsign(min_distance<R>(sc, xi)) < R(0)) {
                            event = true;
                            top = th;
                            st.interior = (i != npts);
                            break;
                        }
                    }
                }
            }
            if (event) {
                // bracketed root of cond(dense(θ)) on [0, top]; Θ ends on the pre-crossing side (prevfloat)
                R lo = R(0), hi = top, xi[4];
                dense_pos<R>(y, h, k, hi, xi);
                R Theta;
                if (min_distance<R>(sc, xi) == R(0)) Theta = hi;
                else {
                    for (int it = 0; it < 200; it++) {
                        const R mid = rfma(R(0.5), hi - lo, lo);
                        if (!(mid > lo && mid < hi)) break;
                        dense_pos<R>(y, h, k, mid, xi);
                        const R sg = rsign(min_distance<R>(sc, xi));
                        if (sg * ps > R(0)) lo = mid; else hi = mid;
                    }
                    Theta = lo;
                }
                dense_full<R>(y, h, k, Theta, s_end);
                lam_end = rfma(h, Theta, t);
                st.status = RTGR_RAY_EVENT;
                return st;
            }
            prev_cond = next_cond;
#pragma unroll
            for (int i = 0; i < 8; i++) { y[i] = yn[i]; k[0][i] = k[6][i]; }
            t = tnew;
            dt = rmin(dtmax, dtnew);
            if (t < t1 && !(t + dt > t)) { st.status = RTGR_RAY_DTMIN; break; }
        } else {
            st.nrej++;
            dt = dt / rmin(qmin_inv, q11 * igamma);
            if (!(t + dt > t)) { st.status = RTGR_RAY_DTMIN; break; }
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) s_end[i] = y[i];
    lam_end = t;
    return st;
}

// One lane = one ray.  A wave owns an 8x8 pixel tile (lock-step efficiency 0.90 vs 0.45 for 64 consecutive
// pixels); a 256-thread workgroup owns 4 horizontally adjacent tiles.  The simple variant (knob tile = 1):
// whole adaptive loop + event finder + colouring inline — an independent formulation kept for A/B and cross-checks.
template <class R, int METRIC, bool SPIN>
__global__ __launch_bounds__(256) void trace_kernel(const TraceArgs<R> A) {
    const uint64_t tiles_i = (A.ni + 7) >> 3;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t ti = wave % tiles_i, tj = wave / tiles_i;
    const uint64_t i = ti * 8 + (lane & 7), jl = tj * 8 + (lane >> 3);
    const bool valid = (i < A.ni) && (jl < A.nrows);
    const uint64_t n = A.ni * A.nrows;
    const uint64_t idx = i + jl * A.ni;

    RayStats st{0, 0, 0, 0, 0};
    bool ev = false;
    if (valid) {
        R s0[8], se[8], lam, col[3];
        if (A.state0) {
#pragma unroll
            for (int c = 0; c < 8; c++) s0[c] = A.state0[idx * 8 + c];
        } else {
            make_pixel<R>(A.sc, A.cam, A.ni, A.nj, i, A.j0 + jl * A.jstride, s0);
        }
        st = integrate_ray<R, METRIC, SPIN>(A.sc, A.opt, s0, se, lam);
        const uint32_t hit = colour_pixel<R>(A.sc, A.opt, se, col);
        A.rgb[idx] = col[0];
        A.rgb[n + idx] = col[1];
        A.rgb[2 * n + idx] = col[2];
        if (A.state_end) {
#pragma unroll
            for (int c = 0; c < 8; c++) A.state_end[idx * 8 + c] = se[c];
        }
        if (A.lambda_end) A.lambda_end[idx] = lam;
        if (A.status) A.status[idx] = st.status;
        if (A.hit) A.hit[idx] = (uint8_t)hit;
        if (A.hit32) A.hit32[idx] = hit;
        if (A.n_accept) A.n_accept[idx] = st.nacc;
        if (A.n_reject) A.n_reject[idx] = st.nrej;
        ev = (st.status == RTGR_RAY_EVENT);
    }
    if (A.counters) {
        const unsigned long long c0 = wave_sum(valid ? 1ull : 0ull), c1 = wave_sum(st.nacc), c2 = wave_sum(st.nrej),
                                 c3 = wave_sum(st.nrhs), c4 = wave_sum(ev ? 1ull : 0ull),
                                 c5 = wave_sum(st.interior), c6 = wave_sum((valid && st.status >= RTGR_RAY_MAXSTEPS) ? 1ull : 0ull);
        if (lane == 0) {
            atomicAdd(&A.counters[0], c0);
            atomicAdd(&A.counters[1], c1);
            atomicAdd(&A.counters[2], c2);
            atomicAdd(&A.counters[3], c3);
            atomicAdd(&A.counters[4], c4);
            atomicAdd(&A.counters[5], c5);
            atomicAdd(&A.counters[6], c6);
        }
    }
}

}  // namespace rtgr
