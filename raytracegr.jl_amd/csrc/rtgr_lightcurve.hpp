// rtgr_lightcurve.hpp — hot-spot light curves (include/rtgr.h "hot-spot light curves"): the spot model, i.e. the device functions of the
// reduction of ONE traced frame over many observer times (the reduction itself and its sizes: rtgr_reduce.hpp; its model and the other
// kernels: rtgr_lightcurve.hip; host side: rtgr_lightcurve_host.hip).
//
// THE MODEL, restated (everything in double; the planes of a Float32 entry are promoted on read).  A rigid Gaussian spot rides in the
// emitting disk at radius rho_s with the rate Omega_s of the disk's own emitter model there — which is NOT computed here: the emission
// kernel (rtgr_emit.hip) evaluates it in point mode on one synthetic pair of states, so the metric code stays inlined into that one
// kernel and Omega_s is rtgr_eval_disk_emission_*'s `omega` to the bit.  Observer sample k is the camera shifted by
// tau_k = t_start + k dt; pixel p, whose ray met the disk at (t_p, x_p, y_p), then sees the disk at coordinate time t_p + tau_k, where
// the spot's centre stands at azimuth phi0 + Omega_s (t_p + tau_k).
//
// THE CONTRACT is the expanded form of the distance, split into a factor per pixel and a factor per sample:
//     theta_p = phi0 + Omega_s t_p                       beta_k = Omega_s tau_k
//     P0 = (x_p² + y_p²) + rho_s²       P1 = -2 rho_s (x_p cos theta_p + y_p sin theta_p)       P2 = -2 rho_s (y_p cos theta_p - x_p sin theta_p)
//     d² = P0 + (P1 cos beta_k + P2 sin beta_k)          [= rho_p² + rho_s² - 2 rho_p rho_s cos(gamma_p - beta_k), gamma_p = psi_p - theta_p]
//     e  = d² < (cut sigma)² ? max(exp(-d² / (2 sigma²)) - exp(-cut² / 2), 0) : 0            j = amp e
// (a pair costs two FMAs and a compare, and an exp only inside the support; the cancellation error of d² is eps rho², eps rho² / sigma²
// relative in e).  A pixel is ACTIVE iff hit32 == the disk, g finite and > 0, (t, x, y) finite and |rho_p - rho_s| < cut sigma — no other
// pixel can ever have d < cut sigma.  With the pixel's (a, b) and weight w (pixel_weight, rtgr_reduce.hpp), W = amp w g^q:
//     F_k = sum_p W e_pk      A_k = sum_p (W a) e_pk      B_k = sum_p (W b) e_pk
#pragma once
#include "rtgr_reduce.hpp"   // (finite_f64, pixel_weight, the skeleton)

namespace rtgr {

constexpr unsigned LC_REC = 6;              // doubles per record: P0, P1, P2, W, W a, W b

// the per-pixel factors P[3] of a point (t, x, y) of the disk; false: the point is not finite, or it lies off the ring the spot sweeps
RTGR_DEV bool lc_record(const LcSpot& S, double Om, double t, double x, double y, double P[3]) {
    const double rho2 = x * x + y * y;
    const double rho = sqrt(rho2);
    if (!finite_f64(t) || !(fabs(rho - S.rho_s) < S.cut_sigma)) return false;   // (a NaN or infinite radius fails the compare)
    const double theta = S.phi0 + Om * t;
    double st, ct;
    sincos(theta, &st, &ct);
    P[0] = rho2 + S.rho_s * S.rho_s;
    P[1] = -2.0 * S.rho_s * (x * ct + y * st);
    P[2] = -2.0 * S.rho_s * (y * ct - x * st);
    return true;
}

// d² of the contract for one (pixel, sample) pair, and e for a pair inside the support (d² < r2_cut; e = 0 outside, which the callers
// do not evaluate: the hot loop's pair is a multiply, an FMA, an add and a compare unless it lies inside)
RTGR_DEV double lc_d2(double P0, double P1, double P2, double cb, double sb) { return P0 + fma(P2, sb, P1 * cb); }
RTGR_DEV double lc_inside(const LcSpot& S, double d2) {
    const double e = exp(-(d2 * S.inv_2s2)) - S.e_cut;
    return e > 0.0 ? e : 0.0;
}

}  // namespace rtgr
