// rtgr_transfer.hpp — volume emission (include/rtgr.h "volume emission"): radiative transfer through a hot, rotating flow, integrated
// along each ray BEHIND the trace.  The trace's kernels are untouched: this header holds the flow model (ONE device function,
// flow_point<R>), the integrator of the 10-vector (x, k, tau, I) and the kernel that runs it, one lane per ray.
//
// THE MODEL (everything in the scalar type R of the entry point; flow_point's own expressions are not fused).  At a point
// x = (t, x, y, z) of a ray with tangent k, started at x_0 with tangent k_0:
//     rho = hypot(x, y)        r = sqrt(x² + y² + z²)                                   (coordinate terms)
//     n   = (r / r0)^(-alpha) exp(-z² / (2 H² rho²))                                     a non-finite n counts as 0
//     Omega = circular_orbit_rate(sc, t, x, y, orbit, ok)   [RTGR_EMIT_KEPLER: rtgr_emission.hpp's, the disk's own rate at z = 0]
//           = orbit                                          [RTGR_EMIT_RIGID]
//     xi = (1, -Omega y, Omega x, 0)       n² = g(x)(xi, xi)       u_f = xi / sqrt(-n²)
//     VALID iff ok, Omega and n² finite, n² < 0
//     w = g(x)(k, u_f)         kappa0 = g(x_0)(k_0, u_obs)         gfac = kappa0 / w
//     dtau/dlambda = kappa n w             dI/dlambda = j0 n w gfac^(3+s) exp(-tau)
// both 0 where the point is invalid or gfac is not > 0.  u_obs is the e_0 of the observer's frame record, or, without one, the static
// observer at x_0 (disk_emission's rule).
//
// THE INTEGRATION.  Tsit5 (Tsit5C's coefficients) on y = (x, k, tau, I) from the ray's own start state over [lambda0, lambda_end]:
// the geodesic half is rhs<R, METRIC, SPIN>, the closed right-hand side of the tile kernel; initial_dt on the geodesic part; the PI
// controller of integrate_ray with the rms norm over all 10 components, so the step adapts to the emission; the last step clipped to
// lambda_end exactly.  It ends earlier at the first ACCEPTED step whose end has r < r_stop (no root-find: r_stop belongs inside the
// dark cylinder, where nothing is emitted), after opt.max_steps attempts, on a non-finite error estimate or on dt underflow.
// Status byte: 0 reached lambda_end, 1 r_stop, 2 step cap, 3 not integrated or not finite (I = tau = NaN).
// With kappa > 0, dtau/dlambda is unbounded at the photon orbit's cylinder (w ~ 1 / sqrt(-n²)): a Float64 ray that crosses it inside
// the gas ends with a step underflow, status 3, and its pixel becomes NaN (include/rtgr.h states this limitation of the model).
//
// THE KERNEL.  transfer_kernel<R, METRIC, SPIN>, one lane per ray, no LDS, no floating-point atomic, no lane reads another's data.
// Frame mode (ni > 0): 8 x 8 pixel tiles over the batch's rows as trace_kernel maps them; the start states are the batch's, lambda_end
// and the trace's status the frame's window; rays the trace ended as RTGR_RAY_NAN are not integrated and keep their colour; every other
// pixel becomes rgb_c exp(-tau_end) + gain weight_c I_end.  List mode (ni == 0; rtgr_eval_transfer_*): n listed rays, linear index,
// the same body.  The step counters go through a wave sum and one integer atomic per wave.
#pragma once
#include "rtgr_host.hpp"
#include "rtgr_emission.hpp"
#include "rtgr_tile.hpp"

namespace rtgr {

template <class R>
struct FlowPoint {
    R dens, omega, uf[4], gfac;
    bool valid;
};

// kappa0 of the model above.  ok: the observer is timelike there (the frame record valid)
template <class R>
RTGR_DEV R flow_kappa0(const DevScene<R>& sc, const R s0[8], const ObsFrame<R>* obs, bool& ok) {
#pragma clang fp contract(off)
    R g0[4][4], tobs[4];
    metric_plain<R>(sc, s0, g0);
    if (obs) {
        ok = obs->valid != 0u;
        for (int c = 0; c < 4; c++) tobs[c] = obs->e[0][c];
    } else {
        static_observer<R>(g0, tobs, ok);
    }
    return inner<R>(g0, s0 + 4, tobs);
}

// The model above at one point s = (x, k).  dens, omega, uf, gfac as they come out of the formulas (the hook masks them); dtau and
// dI0 (dI/dlambda at tau = 0) are the derivatives the integrator uses.
template <class R>
RTGR_DEV void flow_point(const DevScene<R>& sc, const DevFlow<R>& F, R kappa0, const R s[8], FlowPoint<R>& P, R& dtau, R& dI0) {
#pragma clang fp contract(off)
    const R x = s[1], y = s[2], z = s[3];
    const R rho = rhypot<R>(x, y);
    const R r = rsqrt_(x * x + y * y + z * z);
    R dens = rpow<R>(r / F.r0, -F.alpha) * mexp(-(z * z) / (R(2) * F.H * F.H * rho * rho));
    if (!rfinite(dens)) dens = R(0);
    bool ok = true;
    R Om;
    if (F.emitter == RTGR_EMIT_KEPLER) Om = circular_orbit_rate<R>(sc, s[0], x, y, F.orbit, ok);
    else Om = F.orbit;
    R g[4][4];
    metric_plain<R>(sc, s, g);
    const R xi[4] = {R(1), -(Om * y), Om * x, R(0)};
    const R n2 = inner<R>(g, xi, xi);
    ok = ok && rfinite(Om) && rfinite(n2) && n2 < R(0);
    const R sc_u = R(1) / rsqrt_(-n2);
    for (int c = 0; c < 4; c++) P.uf[c] = xi[c] * sc_u;
    const R w = inner<R>(g, s + 4, P.uf);
    const R gf = kappa0 / w;
    P.dens = dens; P.omega = Om; P.gfac = gf; P.valid = ok;
    dtau = R(0); dI0 = R(0);
    if (ok && gf > R(0)) {
        dtau = F.kappa * dens * w;
        dI0 = F.j0 * dens * w * rpow<R>(gf, R(3) + F.s);
    }
}

template <class R, int METRIC, bool SPIN>
RTGR_DEV void transfer_rhs(const DevScene<R>& sc, const DevFlow<R>& F, R kappa0, const R y[10], R dy[10]) {
    rhs<R, METRIC, SPIN>(y, sc.M, sc.a, dy);
    FlowPoint<R> P;
    R dtau, dI0;
    flow_point<R>(sc, F, kappa0, y, P, dtau, dI0);
    dy[8] = dtau;
    dy[9] = dI0 * mexp(-y[8]);
}

struct TransferStats {
    uint32_t nacc, nrej, nrhs;
    uint8_t status;
};

enum TransferStatus : uint8_t { TR_END = 0, TR_RSTOP = 1, TR_MAXSTEPS = 2, TR_NAN = 3 };

// One ray.  y: (x, k, 0, 0) on entry, the state where the integration ended on exit.
template <class R, int METRIC, bool SPIN>
RTGR_DEV TransferStats transfer_ray(const DevScene<R>& sc, const DevSolver<R>& opt, const DevFlow<R>& F, R kappa0, R lam_end, R y[10]) {
    using C = Tsit5C<R>;
    const R reltol = opt.reltol, abstol = opt.abstol;
    const R t1 = lam_end;
    const R dtmax = opt.lambda1 - opt.lambda0;
    const R beta1 = R(0.14L), beta2 = R(0.08L), igamma = R(1) / R(0.9L);
    const R qmin_inv = R(5), qmax_inv = R(0.1L), qoldinit = R(1e-4L);
    const R rstop2 = F.r_stop * F.r_stop;
    TransferStats st{0, 0, 0, TR_END};
    R t = opt.lambda0;
    if (!(t < t1)) return st;
    R k[7][10];
    transfer_rhs<R, METRIC, SPIN>(sc, F, kappa0, y, k[0]);
    R dt = initial_dt<R, METRIC, SPIN>(y, k[0], sc.M, sc.a, abstol, reltol, dtmax);
    st.nrhs = 2;
    R qold = qoldinit;
    for (;;) {
        if (!(t < t1)) { st.status = TR_END; break; }
        if (st.nacc + st.nrej >= opt.max_steps) { st.status = TR_MAXSTEPS; break; }
        const bool last = !(dt < t1 - t);
        dt = rmin(dt, t1 - t);
        R Y[10], yn[10];
        const R h = dt;
#pragma unroll
        for (int i = 0; i < 10; i++) Y[i] = rfma(h * C::a21, k[0][i], y[i]);
        transfer_rhs<R, METRIC, SPIN>(sc, F, kappa0, Y, k[1]);
#pragma unroll
        for (int i = 0; i < 10; i++) Y[i] = rfma(h, rfma(C::a32, k[1][i], C::a31 * k[0][i]), y[i]);
        transfer_rhs<R, METRIC, SPIN>(sc, F, kappa0, Y, k[2]);
#pragma unroll
        for (int i = 0; i < 10; i++) Y[i] = rfma(h, rfma(C::a43, k[2][i], rfma(C::a42, k[1][i], C::a41 * k[0][i])), y[i]);
        transfer_rhs<R, METRIC, SPIN>(sc, F, kappa0, Y, k[3]);
#pragma unroll
        for (int i = 0; i < 10; i++)
            Y[i] = rfma(h, rfma(C::a54, k[3][i], rfma(C::a53, k[2][i], rfma(C::a52, k[1][i], C::a51 * k[0][i]))), y[i]);
        transfer_rhs<R, METRIC, SPIN>(sc, F, kappa0, Y, k[4]);
#pragma unroll
        for (int i = 0; i < 10; i++)
            Y[i] = rfma(h, rfma(C::a65, k[4][i], rfma(C::a64, k[3][i], rfma(C::a63, k[2][i], rfma(C::a62, k[1][i], C::a61 * k[0][i])))), y[i]);
        transfer_rhs<R, METRIC, SPIN>(sc, F, kappa0, Y, k[5]);
#pragma unroll
        for (int i = 0; i < 10; i++)
            yn[i] = rfma(h, rfma(C::a76, k[5][i], rfma(C::a75, k[4][i], rfma(C::a74, k[3][i], rfma(C::a73, k[2][i],
                         rfma(C::a72, k[1][i], C::a71 * k[0][i]))))), y[i]);
        transfer_rhs<R, METRIC, SPIN>(sc, F, kappa0, yn, k[6]);
        st.nrhs += 6;
        R acc = R(0);
#pragma unroll
        for (int i = 0; i < 10; i++) {
            const R ut = h * rfma(C::bt7, k[6][i], rfma(C::bt6, k[5][i], rfma(C::bt5, k[4][i], rfma(C::bt4, k[3][i],
                             rfma(C::bt3, k[2][i], rfma(C::bt2, k[1][i], C::bt1 * k[0][i]))))));
            const R res = ut / rfma(rmax(rabs(y[i]), rabs(yn[i])), reltol, abstol);
            acc = rfma(res, res, acc);
        }
        const R EEst = rsqrt_(acc * R(0.1L));
        if (!rfinite(EEst)) { st.status = TR_NAN; break; }
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
            t = last ? t1 : t + dt;
#pragma unroll
            for (int i = 0; i < 10; i++) { y[i] = yn[i]; k[0][i] = k[6][i]; }
            if (rfma(y[1], y[1], rfma(y[2], y[2], y[3] * y[3])) < rstop2) { st.status = TR_RSTOP; break; }
            dt = rmin(dtmax, dtnew);
            if (t < t1 && !(t + dt > t)) { st.status = TR_NAN; break; }
        } else {
            st.nrej++;
            dt = dt / rmin(qmin_inv, q11 * igamma);
            if (!(t + dt > t)) { st.status = TR_NAN; break; }
        }
    }
    return st;
}

template <class R, int METRIC, bool SPIN>
__global__ __launch_bounds__(256) void transfer_kernel(const TransferArgs<R> A) {
    const uint32_t lane = threadIdx.x & 63;
    bool valid;
    uint64_t idx;
    if (A.ni) {   // frame mode: a wave owns an 8 x 8 tile, a workgroup four horizontally adjacent tiles
        const uint64_t tiles_i = (A.ni + 7) >> 3;
        const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        const uint64_t ti = wave % tiles_i, tj = wave / tiles_i;
        const uint64_t i = ti * 8 + (lane & 7), jl = tj * 8 + (lane >> 3);
        valid = (i < A.ni) && (jl < A.nrows);
        idx = i + jl * A.ni;
    } else {
        idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        valid = idx < A.n;
    }
    TransferStats st{0, 0, 0, TR_NAN};
    bool ran = false;
    if (valid) {
        R nanv = R(__builtin_nan(""));
        asm volatile("" : "+v"(nanv));   // (through a vector register: see observer_ray, rtgr_observer.hpp)
        R y[10];
#pragma unroll
        for (int c = 0; c < 8; c++) y[c] = A.state0[idx * 8 + c];
        y[8] = R(0); y[9] = R(0);
        const R lam_end = A.lambda_end[idx];
        const bool skip = A.status && A.status[idx] == RTGR_RAY_NAN;
        bool fin = rfinite(lam_end);
#pragma unroll
        for (int c = 0; c < 8; c++) fin = fin && rfinite(y[c]);
        if (!skip && fin) {
            bool ok0;
            const R kappa0 = flow_kappa0<R>(A.sc, y, A.obs, ok0);
            st = transfer_ray<R, METRIC, SPIN>(A.sc, A.opt, A.fl, ok0 ? kappa0 : nanv, lam_end, y);
            ran = true;
        }
        const bool good = st.status != TR_NAN && rfinite(y[8]) && rfinite(y[9]);
        if (!good) st.status = TR_NAN;
        const R tau = good ? y[8] : nanv, I = good ? y[9] : nanv;
        if (A.I) A.I[idx] = I;
        if (A.tau) A.tau[idx] = tau;
        if (A.tstatus) A.tstatus[idx] = st.status;
        if (A.tsteps) A.tsteps[idx] = st.nacc + st.nrej;
        if (A.s_end)
#pragma unroll
            for (int c = 0; c < 8; c++) A.s_end[idx * 8 + c] = y[c];
        if (A.rgb && ran) {   // (a ray that was not integrated keeps its colour; one whose integration ended not finite gets NaN)
#pragma clang fp contract(off)
            const R att = mexp(-tau);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                const R was = A.rgb[ch * A.plane_stride + idx];
                A.rgb[ch * A.plane_stride + idx] = was * att + A.fl.gain * A.fl.weight[ch] * I;
            }
        }
    }
    if (A.counters) {
        const unsigned long long c0 = wave_sum(ran ? 1ull : 0ull), c1 = wave_sum(st.nacc), c2 = wave_sum(st.nrej), c3 = wave_sum(st.nrhs),
                                 c4 = wave_sum((ran && st.status == TR_RSTOP) ? 1ull : 0ull),
                                 c6 = wave_sum((ran && st.status >= TR_MAXSTEPS) ? 1ull : 0ull);
        if (lane == 0) {
            atomicAdd(&A.counters[0], c0);
            atomicAdd(&A.counters[1], c1);
            atomicAdd(&A.counters[2], c2);
            atomicAdd(&A.counters[3], c3);
            atomicAdd(&A.counters[4], c4);
            atomicAdd(&A.counters[6], c6);
        }
    }
}

// the pointwise hook's kernel: the model at n points s = (x, k) of rays started at s0
template <class R>
__global__ __launch_bounds__(256) void flow_kernel(const FlowArgs<R> A) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.n) return;
    R nanv = R(__builtin_nan(""));
    asm volatile("" : "+v"(nanv));
    R s0[8], s[8];
#pragma unroll
    for (int c = 0; c < 8; c++) { s0[c] = A.state0[idx * 8 + c]; s[c] = A.state[idx * 8 + c]; }
    bool ok0;
    const R kappa0 = flow_kappa0<R>(A.sc, s0, A.obs, ok0);
    FlowPoint<R> P;
    R dtau, dI0;
    flow_point<R>(A.sc, A.fl, ok0 ? kappa0 : nanv, s, P, dtau, dI0);
    if (A.dens) A.dens[idx] = P.dens;
    if (A.omega) A.omega[idx] = P.valid ? P.omega : nanv;
    if (A.u_f)
#pragma unroll
        for (int c = 0; c < 4; c++) A.u_f[idx * 4 + c] = P.valid ? P.uf[c] : nanv;
    if (A.gfac) A.gfac[idx] = P.valid ? P.gfac : nanv;
    if (A.dtau) A.dtau[idx] = dtau;
    if (A.dI0) A.dI0[idx] = dI0;
}

// ---- host side of the two kernel units (tu_transfer_f64.hip, tu_transfer_f32.hip instantiate these for their scalar type) -------------
template <class R, int METRIC, bool SPIN>
static int transfer_launch_as(const TransferArgs<R>& A, hipStream_t st) {
    // frame mode: four tiles of 8 x 8 pixels per workgroup; list mode: 256 rays per workgroup
    const uint64_t blocks = A.ni ? (((A.ni + 7) / 8) * ((A.nrows + 7) / 8) + 3) / 4 : (A.n + 255) / 256;
    if (blocks == 0) return RTGR_OK;
    if (blocks > 0x7fffffffull) return fail(RTGR_ERR_BAD_ARG, "volume emission: too many rays for one launch");
    hipLaunchKernelGGL((transfer_kernel<R, METRIC, SPIN>), dim3((unsigned)blocks), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}

template <class R>
int transfer_launch(const TransferArgs<R>& A, hipStream_t st) {
    const bool spin = A.sc.a != R(0);
    switch (A.sc.metric) {
        case RTGR_MINKOWSKI: return transfer_launch_as<R, RTGR_MINKOWSKI, false>(A, st);
        case RTGR_KS_REF: return spin ? transfer_launch_as<R, RTGR_KS_REF, true>(A, st) : transfer_launch_as<R, RTGR_KS_REF, false>(A, st);
        case RTGR_KS_TRUE: return spin ? transfer_launch_as<R, RTGR_KS_TRUE, true>(A, st) : transfer_launch_as<R, RTGR_KS_TRUE, false>(A, st);
        default: return fail(RTGR_ERR_BAD_ARG, "volume emission: no transfer kernel for this metric");   // (the host has refused it already)
    }
}

template <class R>
int flow_launch(const FlowArgs<R>& A, hipStream_t st) {
    if (A.n == 0) return RTGR_OK;
    hipLaunchKernelGGL(flow_kernel<R>, dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}

}  // namespace rtgr
