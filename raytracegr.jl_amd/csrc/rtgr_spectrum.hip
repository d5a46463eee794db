// rtgr_spectrum.hip — the kernels of disk spectra (include/rtgr.h "disk spectra"; model and sizes: rtgr_spectrum.hpp; host side:
// rtgr_spectrum_host.hip):
//   spec_reduce_kernel<R, KIND>   the hot path: blocks of one wave over (ranges of pixels) x (tiles of bins or samples) -> partial sums
//   spec_sum_kernel               the partial sums of a pass added in range order, times c_k for THERMAL -> the output
//   spec_points_kernel<R>         the hook: the axis, and bin and val at n triples (x, y, g), one lane each, from the same device functions
// No floating-point atomics and no cross-lane reduction: a lane OWNS its bins or samples and adds the pixels of its block's range in
// pixel order, so a sum's order of operations is fixed by (n, nb) alone — the result is the same bits on every run and every stream.
#include "rtgr_spectrum.hpp"

namespace rtgr {

// what the reduction kernel reads: everything wave-uniform sits in the argument block (scalar loads)
template <class R>
struct SpecArgs {
    LcPlanes<R> P;
    SpecDev S;
    LcWeight W;
    double* partial;     // [3][blocks][nbp]
    uint64_t chunk;      // pixels per block along the pixel axis
    uint64_t k0, nbp;    // this pass: bins or samples k0 .. k0 + nbp - 1
};

// Block (bx, by): the pixels [bx chunk, (bx + 1) chunk) x the bins or samples k0 + by SPEC_TILE + s SPEC_WAVE + lane, s < SPEC_LANE_BINS.
// CULL: hit32 is read coalesced; a lane whose pixel is not on the disk is done after that one load, one whose g is no positive finite
// number after a second; LINE also leaves unless the pixel's bin lies in THIS block's tile — so every record belongs to exactly one
// tile and the walk's cost per record does not grow with nb; the others read (x, y) of their end state and leave unless the mode's
// condition holds.  COMPACT: the active lanes of a round of SPEC_WAVE pixels write their records to LDS behind those of the rounds
// before, in pixel order (ballot + count of the lanes below).  WALK: every lane reads record after record — one address for the whole
// wave, which LDS broadcasts — LINE: and adds it into the one of its bins whose index the record names; THERMAL: and adds it, times
// 1 / expm1(theta tau), into each of its samples.
template <class R, int KIND>
__global__ __launch_bounds__(SPEC_WAVE) void spec_reduce_kernel(SpecArgs<R> A) {
    __shared__ double rec[SPEC_RANGE * SPEC_REC];
    const unsigned lane = threadIdx.x;
    const uint64_t kt = (uint64_t)blockIdx.y * SPEC_TILE;   // first bin or sample of the tile, within the pass
    const uint64_t tile0 = A.k0 + kt;                       // … and on the whole axis
    const unsigned left = (unsigned)(A.nbp - kt < SPEC_TILE ? A.nbp - kt : SPEC_TILE);
    const unsigned ns = (left + SPEC_WAVE - 1) / SPEC_WAVE;   // live sub-tiles: wave-uniform
    double th[SPEC_LANE_BINS], F[SPEC_LANE_BINS], Fa[SPEC_LANE_BINS], Fb[SPEC_LANE_BINS];
#pragma unroll
    for (unsigned s = 0; s < SPEC_LANE_BINS; s++) {
        th[s] = KIND == RTGR_SPEC_THERMAL ? spec_theta(A.S, tile0 + s * SPEC_WAVE + lane) : 0.0;
        F[s] = Fa[s] = Fb[s] = 0.0;
    }
    const uint64_t p0 = (uint64_t)blockIdx.x * A.chunk;
    const uint64_t p1 = p0 + A.chunk < A.P.n ? p0 + A.chunk : A.P.n;
    for (uint64_t base = p0; base < p1; base += SPEC_RANGE) {
        unsigned cnt = 0;
#pragma unroll 1
        for (unsigned r = 0; r < SPEC_RANGE / SPEC_WAVE; r++) {
            const uint64_t p = base + r * SPEC_WAVE + lane;
            bool act = false;
            double key = 0.0, w = 0.0, a = 0.0, b = 0.0;
            if (p < p1 && A.P.hit32[p] == A.P.object) {
                const double g = (double)A.P.g[p];
                if (g > 0.0 && lc_finite(g)) {
                    uint64_t bin = 0;
                    if (KIND == RTGR_SPEC_THERMAL || (spec_line_bin(A.S, g, bin) && bin >= tile0 && bin - tile0 < SPEC_TILE)) {
                        const R* se = A.P.state_end + p * 8;
                        double rho, v = 1.0;
                        if (spec_rho((double)se[1], (double)se[2], rho)) {
                            if (KIND == RTGR_SPEC_THERMAL) {
                                act = spec_thermal_tau(A.S, rho, g, key);
                            } else {
                                act = spec_line_value(A.S, rho, g, v);
                                key = (double)(bin - tile0);
                            }
                            if (act) w = lc_pixel_weight(A.W, p, A.P.ni, A.P.nj, a, b) * v;
                        }
                    }
                }
            }
            const unsigned long long m = __ballot(act);
            if (act) {
                const unsigned slot = cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                double* q = rec + slot * SPEC_REC;
                q[0] = key; q[1] = w; q[2] = w * a; q[3] = w * b;
            }
            cnt += (unsigned)__builtin_popcountll(m);
        }
        __syncthreads();
        for (unsigned i = 0; i < cnt; i++) {
            const double* q = rec + i * SPEC_REC;
            const double key = q[0], w = q[1], wa = q[2], wb = q[3];
            if (KIND == RTGR_SPEC_THERMAL) {
#pragma unroll
                for (unsigned s = 0; s < SPEC_LANE_BINS; s++) {
                    if (s < ns) {
                        const double e = spec_planck(th[s], key);
                        F[s] = fma(w, e, F[s]);
                        Fa[s] = fma(wa, e, Fa[s]);
                        Fb[s] = fma(wb, e, Fb[s]);
                    }
                }
            } else {
                const unsigned rel = (unsigned)key;
#pragma unroll
                for (unsigned s = 0; s < SPEC_LANE_BINS; s++) {
                    if (rel == s * SPEC_WAVE + lane) {
                        F[s] = F[s] + w;
                        Fa[s] = Fa[s] + wa;
                        Fb[s] = Fb[s] + wb;
                    }
                }
            }
        }
        __syncthreads();   // (the next round of this block overwrites the records)
    }
    const uint64_t plane = (uint64_t)gridDim.x * A.nbp;
#pragma unroll
    for (unsigned s = 0; s < SPEC_LANE_BINS; s++) {
        const uint64_t kk = kt + s * SPEC_WAVE + lane;
        if (kk < A.nbp) {
            double* q = A.partial + (uint64_t)blockIdx.x * A.nbp + kk;
            q[0] = F[s]; q[plane] = Fa[s]; q[2 * plane] = Fb[s];
        }
    }
}

// one lane per bin or sample of the pass: the partial sums of the `blocks` ranges added in range order (reads coalesced along the axis),
// then c_k once (THERMAL)
__global__ __launch_bounds__(256) void spec_sum_kernel(SpecDev S, const double* __restrict__ partial, uint64_t blocks, uint64_t k0, uint64_t nbp,
                                                       double* __restrict__ out) {
    const uint64_t kk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (kk >= nbp) return;
    const uint64_t plane = blocks * nbp;
    double v[3] = {0.0, 0.0, 0.0};
#pragma unroll 16   // (the loads of sixteen ranges in flight; the additions stay in range order)
    for (uint64_t bx = 0; bx < blocks; bx++) {
        const double* q = partial + bx * nbp + kk;
        v[0] += q[0]; v[1] += q[plane]; v[2] += q[2 * plane];
    }
    if (S.kind == RTGR_SPEC_THERMAL) {
        const double c = spec_factor(S, spec_theta(S, k0 + kk));
        v[0] = c * v[0]; v[1] = c * v[1]; v[2] = c * v[2];
    }
    double* o = out + (k0 + kk) * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// the hook: lane idx serves entry idx of the axis (idx < nb) and point idx (idx < n); a point that does not count: bin -1, val 0
template <class R>
__global__ __launch_bounds__(256) void spec_points_kernel(const R* __restrict__ xyg, uint64_t n, SpecDev S, double* __restrict__ axis,
                                                          int64_t* __restrict__ bin, double* __restrict__ val) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (axis && idx < S.nb) axis[idx] = S.kind == RTGR_SPEC_THERMAL ? spec_theta(S, idx) : spec_line_centre(S, idx);
    if (idx >= n) return;
    const double x = (double)xyg[idx * 3 + 0], y = (double)xyg[idx * 3 + 1], g = (double)xyg[idx * 3 + 2];
    double rho = 0.0;
    const bool ok = g > 0.0 && lc_finite(g) && spec_rho(x, y, rho);
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

#define CHECK_LAUNCH()                                     \
    do {                                                   \
        hipError_t e_ = hipGetLastError();                 \
        if (e_ != hipSuccess) return fail(RTGR_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

size_t spec_partial_bytes(uint64_t n, uint64_t nb) {
    const uint64_t nbp = nb < SPEC_PASS ? nb : SPEC_PASS;
    return align256((size_t)(3 * lc_blocks(n) * nbp * sizeof(double)));
}

template <class R>
int spec_reduce_launch(const LcPlanes<R>& P, const SpecDev& S, const LcWeight& W, double* d_partial, double* d_out, hipStream_t st) {
    SpecArgs<R> A;
    A.P = P; A.S = S; A.W = W;
    A.partial = d_partial;
    A.chunk = lc_chunk(P.n);
    const uint64_t blocks = lc_blocks(P.n);
    for (uint64_t k0 = 0; k0 < S.nb; k0 += SPEC_PASS) {
        A.k0 = k0;
        A.nbp = S.nb - k0 < SPEC_PASS ? S.nb - k0 : SPEC_PASS;
        const dim3 grid((unsigned)blocks, (unsigned)((A.nbp + SPEC_TILE - 1) / SPEC_TILE));
        if (S.kind == RTGR_SPEC_THERMAL) hipLaunchKernelGGL((spec_reduce_kernel<R, RTGR_SPEC_THERMAL>), grid, dim3(SPEC_WAVE), 0, st, A);
        else hipLaunchKernelGGL((spec_reduce_kernel<R, RTGR_SPEC_LINE>), grid, dim3(SPEC_WAVE), 0, st, A);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(spec_sum_kernel, dim3((unsigned)((A.nbp + 255) / 256)), dim3(256), 0, st, S, (const double*)d_partial, blocks, k0, A.nbp, d_out);
        CHECK_LAUNCH();
    }
    return RTGR_OK;
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
