// rtgr_lightcurve.hip — the kernels of hot-spot light curves (include/rtgr.h "hot-spot light curves"; the spot model: rtgr_lightcurve.hpp;
// host side: rtgr_lightcurve_host.hip):
//   lc_seed_kernel<R>     one wave, once per call: the synthetic pair of states and observer record at (0, rho_s, 0, 0) that the emission
//                         kernel (rtgr_emit.hip), launched in point mode behind it, turns into Omega_s in the scratch's head
//   LcModel<R>            the light curve as a model of THE reduction (rtgr_reduce.hpp: reduce_kernel, reduce_sum_kernel): the items are
//                         the observer times; NaN everywhere for an invalid spot
//   lc_points_kernel<R>   the hook: j at n triples (x, y, t), one lane each, from the same device functions
#include "rtgr_lightcurve.hpp"

namespace rtgr {

template <class R>
__global__ __launch_bounds__(64) void lc_seed_kernel(R rho_s, char* __restrict__ head) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    // the ray "ends" on the disk at (0, rho_s, 0, 0) and "starts" there too, k = d_t at both ends; u_obs = d_t of a record that is valid
    // by decree: every test of the emitter model then depends on the emitter alone (rtgr_emission.hpp: disk_emission)
    R* s0 = (R*)(head + LC_HEAD_S0);
    R* se = (R*)(head + LC_HEAD_SE);
    for (int c = 0; c < 8; c++) s0[c] = se[c] = R(0);
    s0[1] = se[1] = rho_s;
    s0[4] = se[4] = R(1);
    ObsFrame<R> F;
    for (int a = 0; a < 4; a++) {
        F.pos[a] = s0[a];
        for (int b = 0; b < 4; b++) { F.g[a][b] = R(0); F.e[a][b] = a == b ? R(1) : R(0); }
    }
    F.omega = R(0); F.hx = R(0); F.hy = R(0);
    F.valid = 1u; F.projection = 0u;
    *(ObsFrame<R>*)(head + LC_HEAD_FRAME) = F;
}

// The model (rtgr_reduce.hpp).  The head's word is Omega_s; an item is observer sample k.  CULL: the lanes read (t, x, y) of their end
// state and leave unless they lie on the ring.  WALK: a pair is a multiply, an FMA, an add and a compare unless it lies inside the support.
template <class R>
struct LcModel {
    typedef R Scalar;
    typedef LcSpot Spec;
    static constexpr unsigned REC = LC_REC;
    struct Block { double Om; };
    struct Items { double cb[RED_LANE_ITEMS], sb[RED_LANE_ITEMS]; };
    static RTGR_DEV bool begin(const LcSpot&, const void* head, Block& B) {
        B.Om = (double)*(const R*)head;
        return finite_f64(B.Om);   // (an invalid spot)
    }
    static RTGR_DEV void item(const LcSpot& S, const Block& B, uint64_t k, Items& it, unsigned s) {
        const double tau = S.t_start + (double)k * S.dt;
        sincos(B.Om * tau, &it.sb[s], &it.cb[s]);
    }
    static RTGR_DEV PixelRecord<REC - 3> cull(const ReduceArgs<R, LcSpot>& A, const Block& B, uint64_t p, double g, uint64_t) {
        PixelRecord<REC - 3> px;
        const R* se = A.P.state_end + p * 8;
        px.act = lc_record(A.S, B.Om, (double)se[0], (double)se[1], (double)se[2], px.key);
        if (px.act) px.w = A.S.amp * pixel_weight(A.W, p, A.P.ni, A.P.nj, px.a, px.b) * pow(g, A.S.q);
        return px;
    }
    static RTGR_DEV void walk(const LcSpot& S, const double* P, double w, double wa, double wb, const Items& it, unsigned s, bool live, unsigned,
                              double& F, double& Fa, double& Fb) {
        if (live) {
            const double d2 = lc_d2(P[0], P[1], P[2], it.cb[s], it.sb[s]);
            if (d2 < S.r2_cut) {   // (outside: e = 0, and adding w x 0 changes no sum)
                const double e = lc_inside(S, d2);
                F = fma(w, e, F);
                Fa = fma(wa, e, Fa);
                Fb = fma(wb, e, Fb);
            }
        }
    }
    static RTGR_DEV void finish(const LcSpot&, uint64_t, double*) {}
};

// the hook: tau = 0 (cos beta = 1, sin beta = 0) — the spot as it stands at the point's own coordinate time
template <class R>
__global__ __launch_bounds__(256) void lc_points_kernel(const R* __restrict__ xyt, uint64_t n, LcSpot S, const R* __restrict__ omega, double* __restrict__ j) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const double Om = (double)*omega;
    double v = __builtin_nan("");
    if (finite_f64(Om)) {
        double P[3];
        v = 0.0;
        if (lc_record(S, Om, (double)xyt[idx * 3 + 2], (double)xyt[idx * 3 + 0], (double)xyt[idx * 3 + 1], P)) {
            const double d2 = lc_d2(P[0], P[1], P[2], 1.0, 0.0);
            if (d2 < S.r2_cut) v = S.amp * lc_inside(S, d2);
        }
    }
    j[idx] = v;
}

template <class R>
int lc_seed_launch(R rho_s, char* d_head, hipStream_t st) {
    hipLaunchKernelGGL(lc_seed_kernel<R>, dim3(1), dim3(64), 0, st, rho_s, d_head);
    CHECK_LAUNCH();
    return RTGR_OK;
}

template <class R>
int lc_reduce_launch(const ReducePlanes<R>& P, const LcSpot& S, const PixelWeight& W, uint64_t nt, const char* d_head, double* d_partial, double* d_lc,
                     hipStream_t st) {
    return reduce_launch<LcModel<R>>(P, S, W, nt, d_head + LC_HEAD_OMEGA, d_partial, d_lc, st);
}

template <class R>
int lc_points_launch(const R* d_xyt, uint64_t n, const LcSpot& S, const char* d_head, double* d_j, hipStream_t st) {
    if (n == 0) return RTGR_OK;
    hipLaunchKernelGGL(lc_points_kernel<R>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_xyt, n, S, (const R*)(d_head + LC_HEAD_OMEGA), d_j);
    CHECK_LAUNCH();
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(lc_seed_launch);
RTGR_INSTANTIATE_F64_F32(lc_reduce_launch);
RTGR_INSTANTIATE_F64_F32(lc_points_launch);

}  // namespace rtgr
