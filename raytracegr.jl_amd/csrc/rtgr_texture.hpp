// rtgr_texture.hpp — image textures (include/rtgr.h "image textures"): the mapping from a direction or a disk position to texture
// coordinates and the sampler.  ONE device function, tex_sample<R>, used by the shading kernel and by the pointwise hook
// rtgr_eval_texture_* (rtgr_shade.hip), so a shaded pixel and the hook at the same point give the same bits.
//
// THE CONTRACT (W = width, H = height of the texture; everything in the scalar type R of the entry point).
//
// From a 3-vector d (direction mapping):
// - θ = atan2(hypot(d_x, d_y), d_z). Do not use `acos`: it is ill-conditioned at the poles.
// - φ = atan2(d_y, d_x).
// - s = (φ + π)·W/(2π) − ½.
// - v = θ·H/π − ½.
// - Column q has its centre at φ = −π + (q + ½)·2π/W. Row r has its centre at θ = (r + ½)·π/H.
// - These are the θ, φ of the reference's `objcolor(::Sphere)`.
// - A zero or non-finite d means "no sample": the pixel keeps its colour.
//
// Disk mapping, from a position x with r_in and r_out of the disk:
// - φ and s as above, from (x, y).
// - v = (hypot(x, y) − r_in)/(r_out − r_in)·H − ½.
//
// NEAREST:
// - Column floor(s + ½) mod W.
// - Row clamp(floor(v + ½), 0, H − 1).
// - The result is the texel's stored value, bit for bit.
//
// BILINEAR:
// - q₀ = floor(s), f_x = s − q₀. Columns are q₀ mod W and (q₀ + 1) mod W, so the seam at φ = ±π wraps.
// - r₀ = floor(v), f_y = v − r₀. Rows are clamp(r₀, 0, H − 1) and clamp(r₀ + 1, 0, H − 1): clamped at the poles and rims, not reflected.
// - Per channel: a = t₀₀ + f_x (t₁₀ − t₀₀), b = t₀₁ + f_x (t₁₁ − t₀₁), result = a + f_y (b − a).
// - This form is written relative to a corner, like the grid interpolant relative to its centre sample. A constant texture comes back
//   to the bit: t₁₀ − t₀₀ = 0 exactly, f_x · 0 = 0, t₀₀ + 0 = t₀₀, and the same in y.
//
// What the contract leaves open, fixed here: the affine maps are evaluated as (φ + π)·(W / (2π)) − ½ and θ·(H / π) − ½, with π rounded to
// R; no operation is fused (fp contract off: the bits do not depend on the kernel the function is inlined into); a disk position with a
// non-finite x or y, or a v that is not finite (r_out = r_in), is "no sample" too.  The escape direction of a shaded frame is the
// coordinate velocity at the ray's end, with no asymptotic correction; the colour is the texel as sampled, without the reference's
// omin / length(objs) dimming (rtgr_shade.hip).
//
// Device layout of a texture: row after row, column fastest, FOUR scalars per texel (r, g, b, 0) — a corner is one aligned 32-byte
// (Float64) or 16-byte (Float32) load.  Out of scope: mip-mapping or any minification filter (anti-aliasing is the answer to
// minification), pole-aware bilinear.
#pragma once
#include "rtgr_objects.hpp"

namespace rtgr {

enum TexMapping : uint32_t { TEX_MAP_DIRECTION = 0, TEX_MAP_DISK = 1 };

template <class R> struct TexVec;   // one texel: four scalars, loaded as one vector
template <> struct alignas(32) TexVec<double> { double c[4]; };
template <> struct alignas(16) TexVec<float> { float c[4]; };

template <class R> RTGR_DEV R rhypot(R x, R y);
template <> RTGR_DEV double rhypot<double>(double x, double y) { return hypot(x, y); }
template <> RTGR_DEV float rhypot<float>(float x, float y) { return hypotf(x, y); }
template <class R> RTGR_DEV bool rfinite(R x) { return x - x == R(0); }   // false for ±Inf and NaN

// column index of a (possibly out-of-range by a period) column number: q mod W for q in [-W, 2W)
RTGR_DEV uint32_t tex_wrap(int q, int W) { return (uint32_t)(q < 0 ? q + W : (q >= W ? q - W : q)); }

// The sampler: p = d (TEX_MAP_DIRECTION) or a position whose x, y are read (TEX_MAP_DISK, with r_in / r_out).  Returns false — col
// untouched — for "no sample".
template <class R>
RTGR_DEV bool tex_sample(const R* tex, uint32_t W, uint32_t H, uint32_t filter, uint32_t mapping, R px, R py, R pz, R r_in, R r_out, R col[3]) {
#pragma clang fp contract(off)
    const R PI = R(3.14159265358979323846), HALF = R(0.5);
    R v;
    if (mapping == TEX_MAP_DISK) {
        if (!rfinite(px) || !rfinite(py)) return false;
        v = (rhypot<R>(px, py) - r_in) / (r_out - r_in) * R(H) - HALF;
    } else {
        if (!rfinite(px) || !rfinite(py) || !rfinite(pz) || (px == R(0) && py == R(0) && pz == R(0))) return false;
        const R theta = ratan2<R>(rhypot<R>(px, py), pz);
        v = theta * (R(H) / PI) - HALF;
    }
    if (!rfinite(v)) return false;
    const R phi = ratan2<R>(py, px);
    const R s = (phi + PI) * (R(W) / (R(2) * PI)) - HALF;
    const R rmax = R(H - 1u);
    const TexVec<R>* t = (const TexVec<R>*)tex;
    if (filter == RTGR_TEX_NEAREST) {
        const int q = (int)rfloor<R>(s + HALF);                       // in [0, W]
        R r = rfloor<R>(v + HALF);
        r = r < R(0) ? R(0) : (r > rmax ? rmax : r);
        const TexVec<R> a = t[(size_t)(uint32_t)r * W + tex_wrap(q, (int)W)];
        col[0] = a.c[0]; col[1] = a.c[1]; col[2] = a.c[2];
        return true;
    }
    const R q0 = rfloor<R>(s), r0 = rfloor<R>(v);                         // q0 in [-1, W - 1]
    const R fx = s - q0, fy = v - r0;
    const uint32_t c0 = tex_wrap((int)q0, (int)W), c1 = tex_wrap((int)q0 + 1, (int)W);
    const R ra = r0 < R(0) ? R(0) : (r0 > rmax ? rmax : r0);
    const R r1 = r0 + R(1);
    const R rb = r1 < R(0) ? R(0) : (r1 > rmax ? rmax : r1);
    const size_t row0 = (size_t)(uint32_t)ra * W, row1 = (size_t)(uint32_t)rb * W;
    const TexVec<R> t00 = t[row0 + c0], t10 = t[row0 + c1], t01 = t[row1 + c0], t11 = t[row1 + c1];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const R a = t00.c[c] + fx * (t10.c[c] - t00.c[c]);
        const R b = t01.c[c] + fx * (t11.c[c] - t01.c[c]);
        col[c] = a + fy * (b - a);
    }
    return true;
}

}  // namespace rtgr
