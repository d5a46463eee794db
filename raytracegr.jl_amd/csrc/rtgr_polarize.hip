// rtgr_polarize.hip — the kernel of polarized disk images (include/rtgr.h "polarized disk images"; host side:
// rtgr_polarization_host.hip; the model: rtgr_polarization.hpp):
//   polarize_kernel<R>   POL_FRAME   over a traced frame (or a batch's window of it): the pixels that hit the emitting disk get the
//                                    fractional Stokes pair (q, u) and aux; every other pixel NaN in every plane
//                        POL_POINTS  the same at n caller-supplied pairs of states, every output of the model delivered
//                                    (rtgr_eval_polarization_*)
//                        POL_FORMS   (Y(k, f), h(k, f)) at n states and vectors (rtgr_eval_walker_penrose_*)
// One lane per pixel / point, blocks of 256, 64-bit indices, no LDS, no atomics.  ONE kernel for all uses, for rtgr_emit.hip's reason:
// one copy of the model, so a hook predicts a pixel to the bit.  The start states are read, never regenerated.
#include "rtgr_host.hpp"
#include "rtgr_polarization.hpp"

namespace rtgr {

static inline unsigned nblk(uint64_t n) { return (unsigned)((n + 255) / 256); }

// Scene, emission record, polarization record and the pointer to the observer's frame record sit in the argument block: wave-uniform,
// read with scalar loads.  A lane whose hit32 is not the disk writes NaN and leaves after that one coalesced load; the others read
// their start and end state (8 scalars each, AoS).
template <class R>
__global__ __launch_bounds__(256) void polarize_kernel(PolArgs<R> A) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.n) return;
    R nanv = R(__builtin_nan(""));
    asm volatile("" : "+v"(nanv));   // (through a vector register: see observer_ray, rtgr_observer.hpp)
    const R a = A.sc.metric == (uint32_t)RTGR_MINKOWSKI ? R(0) : A.sc.a;
    if (A.mode == POL_FORMS) {
        R s[8], f[4], kap[2];
#pragma unroll
        for (int c = 0; c < 8; c++) s[c] = A.state0[idx * 8 + c];
#pragma unroll
        for (int c = 0; c < 4; c++) f[c] = A.fvec[idx * 4 + c];
        PolForms<R> F;
        pol_forms<R>(a, s, F);
        pol_kappa<R>(F, s + 4, f, kap);
        A.kappa[idx * 2 + 0] = F.ok ? kap[0] : nanv;
        A.kappa[idx * 2 + 1] = F.ok ? kap[1] : nanv;
        return;
    }
    if (A.hit32 && A.hit32[idx] != A.em.object) {
        if (A.q) A.q[idx] = nanv;
        if (A.u) A.u[idx] = nanv;
        if (A.aux) A.aux[idx] = nanv;
        return;
    }
    R s0[8], se[8];
#pragma unroll
    for (int c = 0; c < 8; c++) s0[c] = A.state0[idx * 8 + c];
#pragma unroll
    for (int c = 0; c < 8; c++) se[c] = A.state_end[idx * 8 + c];
    // the emitter side first: what stays live across to the camera side is kappa, delta, aux and the flag
    R kap[2], fem[4], aux, delta;
    const bool okE = pol_emitter<R>(A.sc, a, A.em, A.pol, se, kap, fem, aux, delta);
    if (A.kappa) { A.kappa[idx * 2 + 0] = kap[0]; A.kappa[idx * 2 + 1] = kap[1]; }
    if (A.f_em)
#pragma unroll
        for (int c = 0; c < 4; c++) A.f_em[idx * 4 + c] = fem[c];
    if (A.delta) A.delta[idx] = delta;
    if (A.aux) A.aux[idx] = aux;
    R al, be;
    const bool okC = pol_camera<R>(a, *A.obs, s0, kap, al, be);
    R q, u;
    {
#pragma clang fp contract(off)
        const R a2 = al * al, b2 = be * be, d = a2 + b2;
        q = delta * (a2 - b2) / d;
        u = R(2) * delta * al * be / d;
    }
    if (!okC) { q = nanv; u = nanv; }
    else if (!okE) { q = rfinite(delta) ? R(0) : nanv; u = q; }
    if (A.q) A.q[idx] = q;
    if (A.u) A.u[idx] = u;
    if (A.valid) A.valid[idx] = okE && okC ? 1 : 0;
}

template <class R>
int polarize_launch(const PolArgs<R>& A, hipStream_t st) {
    if (A.n == 0) return RTGR_OK;
    hipLaunchKernelGGL(polarize_kernel<R>, dim3(nblk(A.n)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(polarize_launch);

}  // namespace rtgr
