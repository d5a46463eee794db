// rtgr_spectrum.hip — the kernels of disk spectra (include/rtgr.h "disk spectra"; the spectral model: rtgr_spectrum.hpp; host side:
// rtgr_spectrum_host.hip):
//   SpecModel<R, KIND>       a line profile and a thermal spectrum as models of THE reduction (rtgr_reduce.hpp: reduce_kernel,
//                            reduce_sum_kernel): the items are the bins or the sample frequencies; THERMAL's sum is scaled by c_k
//   spec_points_kernel<R>    the hook: the axis, and bin and val at n triples (x, y, g), one lane each, from the same device functions
#include "rtgr_spectrum.hpp"

namespace rtgr {

// The models (rtgr_reduce.hpp).  No head.  CULL: LINE leaves unless the pixel's bin lies in THIS block's tile — so every record belongs
// to exactly one tile and the walk's cost per record does not grow with nb; the others read (x, y) of their end state and leave unless
// the mode's condition holds.  The record's key: LINE the bin within the tile, THERMAL tau.  WALK: LINE adds the record into the one of
// the lane's bins whose index it names — plain additions; THERMAL adds it, times 1 / expm1(theta tau), into each of the lane's samples.
template <class R, int KIND>
struct SpecModel {
    typedef R Scalar;
    typedef SpecDev Spec;
    static constexpr unsigned REC = SPEC_REC;
    struct Block {};
    struct Items { double th[RED_LANE_ITEMS]; };   // (THERMAL: the sample frequencies; LINE: nothing)
    static RTGR_DEV bool begin(const SpecDev&, const void*, Block&) { return true; }
    static RTGR_DEV void item(const SpecDev& S, const Block&, uint64_t k, Items& it, unsigned s) {
        if (KIND == RTGR_SPEC_THERMAL) it.th[s] = spec_theta(S, k);
    }
    static RTGR_DEV PixelRecord<REC - 3> cull(const ReduceArgs<R, SpecDev>& A, const Block&, uint64_t p, double g, uint64_t tile0) {
        PixelRecord<REC - 3> px;
        uint64_t bin = 0;
        px.key[0] = 0.0;
        if (KIND == RTGR_SPEC_THERMAL || (spec_line_bin(A.S, g, bin) && bin >= tile0 && bin - tile0 < RED_TILE)) {
            const R* se = A.P.state_end + p * 8;
            double rho, v = 1.0;
            if (spec_rho((double)se[1], (double)se[2], rho)) {
                if (KIND == RTGR_SPEC_THERMAL) {
                    px.act = spec_thermal_tau(A.S, rho, g, px.key[0]);
                } else {
                    px.act = spec_line_value(A.S, rho, g, v);
                    px.key[0] = (double)(bin - tile0);
                }
                if (px.act) px.w = pixel_weight(A.W, p, A.P.ni, A.P.nj, px.a, px.b) * v;
            }
        }
        return px;
    }
    static RTGR_DEV void walk(const SpecDev&, const double* key, double w, double wa, double wb, const Items& it, unsigned s, bool live, unsigned slot,
                              double& F, double& Fa, double& Fb) {
        if (KIND == RTGR_SPEC_THERMAL) {
            if (live) {
                const double e = spec_planck(it.th[s], key[0]);
                F = fma(w, e, F);
                Fa = fma(wa, e, Fa);
                Fb = fma(wb, e, Fb);
            }
        } else if ((unsigned)key[0] == slot) {
            F = F + w;
            Fa = Fa + wa;
            Fb = Fb + wb;
        }
    }
    static RTGR_DEV void finish(const SpecDev& S, uint64_t k, double* v) {
        if (KIND == RTGR_SPEC_THERMAL) {
            const double c = spec_factor(S, spec_theta(S, k));
            v[0] = c * v[0]; v[1] = c * v[1]; v[2] = c * v[2];
        }
    }
};

// the hook: lane idx serves entry idx of the axis (idx < nb) and point idx (idx < n); a point that does not count: bin -1, val 0
template <class R>
__global__ __launch_bounds__(256) void spec_points_kernel(const R* __restrict__ xyg, uint64_t n, SpecDev S, double* __restrict__ axis,
                                                          int64_t* __restrict__ bin, double* __restrict__ val) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (axis && idx < S.nb) axis[idx] = S.kind == RTGR_SPEC_THERMAL ? spec_theta(S, idx) : spec_line_centre(S, idx);
    if (idx >= n) return;
    const double x = (double)xyg[idx * 3 + 0], y = (double)xyg[idx * 3 + 1], g = (double)xyg[idx * 3 + 2];
    double rho = 0.0;
    const bool ok = g > 0.0 && finite_f64(g) && spec_rho(x, y, rho);
    if (S.kind == RTGR_SPEC_THERMAL) {
        double tau = 0.0;
        const bool counts = ok && spec_thermal_tau(S, rho, g, tau);
        if (bin) bin[idx] = counts ? 0 : -1;
        if (val)
            for (uint64_t k = 0; k < S.nb; k++) {
                const double th = spec_theta(S, k);
                val[idx * S.nb + k] = counts ? spec_factor(S, th) * spec_planck(th, tau) : 0.0;
            }
    } else {
        uint64_t b = 0;
        double v = 0.0;
        const bool counts = ok && spec_line_bin(S, g, b) && spec_line_value(S, rho, g, v);
        if (bin) bin[idx] = counts ? (int64_t)b : -1;
        if (val) val[idx] = counts ? v : 0.0;
    }
}

template <class R>
int spec_reduce_launch(const ReducePlanes<R>& P, const SpecDev& S, const PixelWeight& W, double* d_partial, double* d_out, hipStream_t st) {
    if (S.kind == RTGR_SPEC_THERMAL) return reduce_launch<SpecModel<R, RTGR_SPEC_THERMAL>>(P, S, W, S.nb, nullptr, d_partial, d_out, st);
    return reduce_launch<SpecModel<R, RTGR_SPEC_LINE>>(P, S, W, S.nb, nullptr, d_partial, d_out, st);
}

template <class R>
int spec_points_launch(const R* d_xyg, uint64_t n, const SpecDev& S, double* d_axis, int64_t* d_bin, double* d_val, hipStream_t st) {
    const uint64_t m = n > S.nb ? n : S.nb;
    hipLaunchKernelGGL(spec_points_kernel<R>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_xyg, n, S, d_axis, d_bin, d_val);
    CHECK_LAUNCH();
    return RTGR_OK;
}

RTGR_INSTANTIATE_F64_F32(spec_reduce_launch);
RTGR_INSTANTIATE_F64_F32(spec_points_launch);

}  // namespace rtgr
