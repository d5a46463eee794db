// rtgr_spectrum.hpp — disk spectra (include/rtgr.h "disk spectra"): the spectral model, i.e. the device functions of the reduction of ONE
// traced frame of an emitting disk to a line profile or a thermal spectrum (the reduction itself and its sizes: rtgr_reduce.hpp; its
// models and the hook's kernel: rtgr_spectrum.hip; host side: rtgr_spectrum_host.hip).
//
// THE MODEL, restated (everything in double; the planes of a Float32 entry are promoted on read).  Pixel p takes part iff
// hit32[p] == the disk, g_p finite and > 0, (x_p, y_p) of its end state finite, and the mode's own condition holds; rho_p = sqrt(x² + y²).
// Its weight w_p and its (a_p, b_p) are the light curve's (rtgr_reduce.hpp: pixel_weight).
//   LINE     s = nb / (hi - lo) from the host;  u = (g_p - lo) * s;  counts iff 0 <= u < nb and rho_min <= rho_p < rho_max;  b = (uint64)u
//            W_p = w_p [amp (rho_p / rho_min)^(-alpha) g_p^q]        (the bracket: the hook's val)
//            F_b = sum W_p      A_b = sum (W_p a_p)      B_b = sum (W_p b_p)      — plain additions
//   THERMAL  theta_k = lo + k (hi - lo) / (nb - 1)   [RTGR_SPEC_LOG: lo exp(k log(hi / lo) / (nb - 1))]   (nb = 1: lo)
//            T_p = emission_temperature(rho_p) (rtgr_emission.hpp, in double);  counts iff T_p > 0;  tau_p = 1 / (g_p T_p)
//            e = 1 / expm1(theta_k tau_p);  F_k = fma(w_p, e, F_k), A_k = fma(w_p a_p, e, A_k), B_k = fma(w_p b_p, e, B_k)
//            c_k = gain [RTGR_SPEC_NU3: gain theta_k³], applied once after the sum over the ranges
// No expression of these functions is fused (fp contract off) except the accumulation the contract names.
#pragma once
#include "rtgr_reduce.hpp"     // (finite_f64, pixel_weight, the skeleton)
#include "rtgr_emission.hpp"   // (emission_temperature)

namespace rtgr {

constexpr unsigned SPEC_REC = 4;             // doubles per record: LINE (bin - tile base, W, W a, W b), THERMAL (tau, W, W a, W b)

// rho of an end point; false: the point is not finite
RTGR_DEV bool spec_rho(double x, double y, double& rho) {
#pragma clang fp contract(off)
    rho = sqrt(x * x + y * y);
    return finite_f64(x) && finite_f64(y);
}

// LINE: the bin of a frequency ratio; false: outside [lo, hi)
RTGR_DEV bool spec_line_bin(const SpecDev& S, double g, uint64_t& b) {
#pragma clang fp contract(off)
    const double u = (g - S.lo) * S.s;
    if (!(u >= 0.0 && u < (double)S.nb)) return false;
    b = (uint64_t)u;
    return true;
}

// LINE: amp (rho / rho_min)^(-alpha) g^q; false: rho outside the window
RTGR_DEV bool spec_line_value(const SpecDev& S, double rho, double g, double& v) {
#pragma clang fp contract(off)
    if (!(rho >= S.rho_min && rho < S.rho_max)) return false;
    v = S.amp * pow(rho / S.rho_min, -S.alpha) * pow(g, S.q);
    return true;
}
RTGR_DEV double spec_line_centre(const SpecDev& S, uint64_t b) {
#pragma clang fp contract(off)
    return S.lo + ((double)b + 0.5) * (S.hi - S.lo) / (double)S.nb;
}

// THERMAL: sample frequency k, its factor c_k, tau of a pixel (false: T is not > 0) and Planck's 1 / expm1
RTGR_DEV double spec_theta(const SpecDev& S, uint64_t k) {
#pragma clang fp contract(off)
    if (S.nb == 1) return S.lo;
    const double f = (double)k * S.span / (double)(S.nb - 1);
    return (S.flags & RTGR_SPEC_LOG) ? S.lo * exp(f) : S.lo + f;
}
RTGR_DEV double spec_factor(const SpecDev& S, double theta) {
#pragma clang fp contract(off)
    return (S.flags & RTGR_SPEC_NU3) ? S.em.gain * (theta * theta * theta) : S.em.gain;
}
RTGR_DEV bool spec_thermal_tau(const SpecDev& S, double rho, double g, double& tau) {
#pragma clang fp contract(off)
    const double T = emission_temperature<double>(S.em, rho);
    if (!(T > 0.0)) return false;
    tau = 1.0 / (g * T);
    return true;
}
RTGR_DEV double spec_planck(double theta, double tau) {
#pragma clang fp contract(off)
    return 1.0 / expm1(theta * tau);
}

}  // namespace rtgr
