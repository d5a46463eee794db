// rtgr_emit.hip — the kernel of disk emission (include/rtgr.h "disk emission"; host side: rtgr_emission_host.hip):
//   emit_kernel<R>   frame mode: over a traced frame, the pixels that hit the emitting disk get the black-body colour of the orbiting emitter
//                    point mode: the same at n caller-supplied pairs of states, every output of the model delivered (rtgr_eval_disk_emission_*)
// One lane per pixel / point, blocks of 256, 64-bit indices, no LDS, no atomics.
//
// ONE kernel for both uses, on purpose: the hook must predict a pixel to the bit, and the model (rtgr_emission.hpp: disk_emission) goes
// through dmetric_dev's dual numbers and, for a grid, the interpolant — code that is compiled with the library's usual contraction,
// where what gets fused depends on the code around it after inlining.  Two kernels would inline it next to different neighbours; one
// kernel holds one copy.  (Switching contraction off for the whole unit instead is no way out: make_pixel must give rtgr_make_canvas'
// bits, and on a grid its interpolant is contracted there.)
#include "rtgr_host.hpp"
#include "rtgr_emission.hpp"

namespace rtgr {

static inline unsigned nblk(uint64_t n) { return (unsigned)((n + 255) / 256); }

// Frame mode (hit32 given): hit32 is read coalesced; a lane whose ray did not end on the disk writes NaN to the ratio plane (when there
// is one) and exits.  The others — a few per cent of a frame — read their end state (8 scalars, AoS) and their camera state: state0 when
// the rays were caller-supplied states (the sub-rays of anti-aliasing), else make_pixel of the camera, exactly as redshift_body does.
// Point mode (hit32 null): every lane evaluates its pair of states.  The colour goes to rgb[ch * plane_stride + idx * pixel_stride]:
// planes for a frame, n x 3 for the hook.  Scene, camera and emission parameters sit in the argument block: wave-uniform, read with
// scalar loads.
template <class R>
__global__ __launch_bounds__(256) void emit_kernel(EmitArgs<R> A) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.n) return;
    if (A.hit32 && A.hit32[idx] != A.em.object) {
        if (A.g) A.g[idx] = R(__builtin_nan(""));
        return;
    }
    R s0[8], se[8];
    if (A.state0) for (int c = 0; c < 8; c++) s0[c] = A.state0[idx * 8 + c];
    else make_pixel<R>(A.sc, A.cam, A.ni, A.nj, idx % A.ni, idx / A.ni, s0);
    for (int c = 0; c < 8; c++) se[c] = A.state_end[idx * 8 + c];
    R omega, uem[4], g, col[3];
    disk_emission<R>(A.sc, A.em, s0, se, omega, uem, g, col, A.obs);
    if (A.omega) A.omega[idx] = omega;
    if (A.u_emit) for (int c = 0; c < 4; c++) A.u_emit[idx * 4 + c] = uem[c];
    if (A.g) A.g[idx] = g;
    if (A.rgb)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) A.rgb[ch * A.plane_stride + idx * A.pixel_stride] = col[ch];
}

template <class R>
int emit_launch(const EmitArgs<R>& A, hipStream_t st) {
    if (A.n == 0) return RTGR_OK;
    hipLaunchKernelGGL(emit_kernel<R>, dim3(nblk(A.n)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(emit_launch);

}  // namespace rtgr
