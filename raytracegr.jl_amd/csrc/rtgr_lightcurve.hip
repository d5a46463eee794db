// rtgr_lightcurve.hip — the kernels of hot-spot light curves (include/rtgr.h "hot-spot light curves"; model and sizes: rtgr_lightcurve.hpp;
// host side: rtgr_lightcurve_host.hip):
//   lc_seed_kernel<R>     one wave, once per call: the synthetic pair of states and observer record at (0, rho_s, 0, 0) that the emission
//                         kernel (rtgr_emit.hip), launched in point mode behind it, turns into Omega_s in the scratch's head
//   lc_reduce_kernel<R>   the hot path: blocks of one wave over (ranges of pixels) x (tiles of time samples) -> partial sums
//   lc_sum_kernel         the partial sums of a pass added in range order -> lc; NaN everywhere for an invalid spot
//   lc_points_kernel<R>   the hook: j at n triples (x, y, t), one lane each, from the same device functions
// No floating-point atomics and no cross-lane reduction: a lane OWNS its time samples and adds the pixels of its block's range in pixel
// order, so a sum's order of operations is fixed by (n, nt) alone — the result is the same bits on every run and every stream.
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

// what the reduction kernel reads: everything wave-uniform sits in the argument block (scalar loads)
template <class R>
struct LcArgs {
    LcPlanes<R> P;
    LcSpot S;
    LcWeight W;
    const R* omega;      // the head's Omega_s
    double* partial;     // [3][blocks][ntp]
    uint64_t chunk;      // pixels per block along the pixel axis
    uint64_t k0, ntp;    // this pass: samples k0 .. k0 + ntp - 1
};

// Block (bx, by): the pixels [bx chunk, (bx + 1) chunk) x the samples k0 + by LC_TILE + s LC_WAVE + lane, s < LC_LANE_SAMPLES.
// CULL: hit32 is read coalesced; a lane whose pixel is not on the disk is done after that one load, one whose g is no positive finite
// number after a second; the others read (t, x, y) of their end state and leave unless they lie on the ring.  COMPACT: the active
// lanes of a round of LC_WAVE pixels write their records to LDS behind those of the rounds before, in pixel order (ballot + count of the
// lanes below).  WALK: every lane reads record after record — one address for the whole wave, which LDS broadcasts without a bank
// conflict — and adds it into the F, A, B of each of its samples, in registers.
template <class R>
__global__ __launch_bounds__(LC_WAVE) void lc_reduce_kernel(LcArgs<R> A) {
    __shared__ double rec[LC_RANGE * LC_REC];
    const double Om = (double)*A.omega;
    if (!lc_finite(Om)) return;   // (an invalid spot: lc_sum_kernel writes NaN and reads no partial sum)
    const unsigned lane = threadIdx.x;
    const uint64_t kt = (uint64_t)blockIdx.y * LC_TILE;   // first sample of the tile, within the pass
    const unsigned left = (unsigned)(A.ntp - kt < LC_TILE ? A.ntp - kt : LC_TILE);
    const unsigned ns = (left + LC_WAVE - 1) / LC_WAVE;   // live sub-tiles: wave-uniform
    double cb[LC_LANE_SAMPLES], sb[LC_LANE_SAMPLES], F[LC_LANE_SAMPLES], Fa[LC_LANE_SAMPLES], Fb[LC_LANE_SAMPLES];
#pragma unroll
    for (unsigned s = 0; s < LC_LANE_SAMPLES; s++) {
        const uint64_t k = A.k0 + kt + s * LC_WAVE + lane;
        const double tau = A.S.t_start + (double)k * A.S.dt;
        sincos(Om * tau, &sb[s], &cb[s]);
        F[s] = Fa[s] = Fb[s] = 0.0;
    }
    const uint64_t p0 = (uint64_t)blockIdx.x * A.chunk;
    const uint64_t p1 = p0 + A.chunk < A.P.n ? p0 + A.chunk : A.P.n;
    for (uint64_t base = p0; base < p1; base += LC_RANGE) {
        unsigned cnt = 0;
#pragma unroll 1
        for (unsigned r = 0; r < LC_RANGE / LC_WAVE; r++) {
            const uint64_t p = base + r * LC_WAVE + lane;
            bool act = false;
            double P[3], w = 0.0, a = 0.0, b = 0.0;
            if (p < p1 && A.P.hit32[p] == A.P.object) {
                const double g = (double)A.P.g[p];
                if (g > 0.0 && lc_finite(g)) {
                    const R* se = A.P.state_end + p * 8;
                    act = lc_record(A.S, Om, (double)se[0], (double)se[1], (double)se[2], P);
                    if (act) w = A.S.amp * lc_pixel_weight(A.W, p, A.P.ni, A.P.nj, a, b) * pow(g, A.S.q);
                }
            }
            const unsigned long long m = __ballot(act);
            if (act) {
                const unsigned slot = cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                double* q = rec + slot * LC_REC;
                q[0] = P[0]; q[1] = P[1]; q[2] = P[2]; q[3] = w; q[4] = w * a; q[5] = w * b;
            }
            cnt += (unsigned)__builtin_popcountll(m);
        }
        __syncthreads();
        for (unsigned i = 0; i < cnt; i++) {
            const double* q = rec + i * LC_REC;
            const double P0 = q[0], P1 = q[1], P2 = q[2], w = q[3], wa = q[4], wb = q[5];
#pragma unroll
            for (unsigned s = 0; s < LC_LANE_SAMPLES; s++) {
                if (s < ns) {
                    const double d2 = lc_d2(P0, P1, P2, cb[s], sb[s]);
                    if (d2 < A.S.r2_cut) {   // (outside: e = 0, and adding w x 0 changes no sum)
                        const double e = lc_inside(A.S, d2);
                        F[s] = fma(w, e, F[s]);
                        Fa[s] = fma(wa, e, Fa[s]);
                        Fb[s] = fma(wb, e, Fb[s]);
                    }
                }
            }
        }
        __syncthreads();   // (the next round of this block overwrites the records)
    }
    const uint64_t plane = (uint64_t)gridDim.x * A.ntp;
#pragma unroll
    for (unsigned s = 0; s < LC_LANE_SAMPLES; s++) {
        const uint64_t kk = kt + s * LC_WAVE + lane;
        if (kk < A.ntp) {
            double* q = A.partial + (uint64_t)blockIdx.x * A.ntp + kk;
            q[0] = F[s]; q[plane] = Fa[s]; q[2 * plane] = Fb[s];
        }
    }
}

// one lane per sample of the pass: the partial sums of the `blocks` ranges added in range order (reads coalesced along the samples)
template <class R>
__global__ __launch_bounds__(256) void lc_sum_kernel(const R* __restrict__ omega, const double* __restrict__ partial, uint64_t blocks, uint64_t k0,
                                                     uint64_t ntp, double* __restrict__ lc) {
    const uint64_t kk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (kk >= ntp) return;
    double v[3];
    if (!lc_finite((double)*omega)) {
        v[0] = v[1] = v[2] = __builtin_nan("");
    } else {
        const uint64_t plane = blocks * ntp;
        v[0] = v[1] = v[2] = 0.0;
#pragma unroll 16   // (the loads of sixteen ranges in flight; the additions stay in range order)
        for (uint64_t bx = 0; bx < blocks; bx++) {
            const double* q = partial + bx * ntp + kk;
            v[0] += q[0]; v[1] += q[plane]; v[2] += q[2 * plane];
        }
    }
    double* o = lc + (k0 + kk) * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// the hook: tau = 0 (cos beta = 1, sin beta = 0) — the spot as it stands at the point's own coordinate time
template <class R>
__global__ __launch_bounds__(256) void lc_points_kernel(const R* __restrict__ xyt, uint64_t n, LcSpot S, const R* __restrict__ omega, double* __restrict__ j) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const double Om = (double)*omega;
    double v = __builtin_nan("");
    if (lc_finite(Om)) {
        double P[3];
        v = 0.0;
        if (lc_record(S, Om, (double)xyt[idx * 3 + 2], (double)xyt[idx * 3 + 0], (double)xyt[idx * 3 + 1], P)) {
            const double d2 = lc_d2(P[0], P[1], P[2], 1.0, 0.0);
            if (d2 < S.r2_cut) v = S.amp * lc_inside(S, d2);
        }
    }
    j[idx] = v;
}

#define CHECK_LAUNCH()                                     \
    do {                                                   \
        hipError_t e_ = hipGetLastError();                 \
        if (e_ != hipSuccess) return fail(RTGR_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e_)); \
    } while (0)

size_t lc_partial_bytes(uint64_t n, uint64_t nt) {
    const uint64_t ntp = nt < LC_PASS ? nt : LC_PASS;
    return align256((size_t)(3 * lc_blocks(n) * ntp * sizeof(double)));
}

template <class R>
int lc_seed_launch(R rho_s, char* d_head, hipStream_t st) {
    hipLaunchKernelGGL(lc_seed_kernel<R>, dim3(1), dim3(64), 0, st, rho_s, d_head);
    CHECK_LAUNCH();
    return RTGR_OK;
}

template <class R>
int lc_reduce_launch(const LcPlanes<R>& P, const LcSpot& S, const LcWeight& W, uint64_t nt, const char* d_head, double* d_partial, double* d_lc,
                     hipStream_t st) {
    LcArgs<R> A;
    A.P = P; A.S = S; A.W = W;
    A.omega = (const R*)(d_head + LC_HEAD_OMEGA);
    A.partial = d_partial;
    A.chunk = lc_chunk(P.n);
    const uint64_t blocks = lc_blocks(P.n);
    for (uint64_t k0 = 0; k0 < nt; k0 += LC_PASS) {
        A.k0 = k0;
        A.ntp = nt - k0 < LC_PASS ? nt - k0 : LC_PASS;
        const unsigned tiles = (unsigned)((A.ntp + LC_TILE - 1) / LC_TILE);
        hipLaunchKernelGGL(lc_reduce_kernel<R>, dim3((unsigned)blocks, tiles), dim3(LC_WAVE), 0, st, A);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(lc_sum_kernel<R>, dim3((unsigned)((A.ntp + 255) / 256)), dim3(256), 0, st, A.omega, (const double*)d_partial, blocks, k0, A.ntp, d_lc);
        CHECK_LAUNCH();
    }
    return RTGR_OK;
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
