// rtgr_observer.hip — the kernels of the observer camera (include/rtgr.h "observer camera"; host side: rtgr_observer_host.hip):
//   observer_frame_kernel<R>   one wave, once per call: the observer's frame (rtgr_observer.hpp: observer_frame) into a record in the
//                              stream's scratch
//   observer_rays_kernel<R>    one lane per pixel, blocks of 256, 64-bit indices: the n x 8 start states of a batch of pixels
// No LDS, no atomics.  The frame kernel is the only place observer_frame is inlined into, the ray kernel the only one of observer_ray:
// the traced frame, rtgr_make_observer_canvas_* and rtgr_eval_observer_* run these two kernels and see the same bits.
#include "rtgr_host.hpp"
#include "rtgr_observer.hpp"

namespace rtgr {

static inline unsigned nblk(uint64_t n) { return (unsigned)((n + 255) / 256); }

// Scene and observer sit in the argument block.  Lane 0 computes and writes the record (a few hundred bytes); the other lanes of the
// wave have nothing to do.
template <class R>
__global__ __launch_bounds__(64) void observer_frame_kernel(DevScene<R> sc, DevObserver<R> ob, ObsFrame<R>* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    ObsFrame<R> F;
    observer_frame<R>(sc, ob, F);
    *out = F;
}

// The frame record is read through a wave-uniform address that nothing in the kernel writes: scalar loads.  Each lane writes its eight
// scalars (AoS, 64 bytes in Float64: what trace_device reads as state0).
template <class R>
__global__ __launch_bounds__(256) void observer_rays_kernel(const ObsFrame<R>* __restrict__ frame, uint64_t ni, uint64_t nj, uint64_t first, uint64_t n,
                                                           R* __restrict__ state0) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const uint64_t idx = first + w;
    R s[8];
    observer_ray<R>(*frame, ni, nj, idx % ni, idx / ni, s);
#pragma unroll
    for (int c = 0; c < 8; c++) state0[w * 8 + c] = s[c];
}

template <class R>
int observer_frame_launch(const DevScene<R>& sc, const DevObserver<R>& ob, ObsFrame<R>* d_frame, hipStream_t st) {
    hipLaunchKernelGGL(observer_frame_kernel<R>, dim3(1), dim3(64), 0, st, sc, ob, d_frame);
    CHECK_LAUNCH();
    return RTGR_OK;
}
template <class R>
int observer_rays_launch(const ObsFrame<R>* d_frame, uint64_t ni, uint64_t nj, uint64_t first, uint64_t n, R* d_state0, hipStream_t st) {
    if (n == 0) return RTGR_OK;
    hipLaunchKernelGGL(observer_rays_kernel<R>, dim3(nblk(n)), dim3(256), 0, st, d_frame, ni, nj, first, n, d_state0);
    CHECK_LAUNCH();
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(observer_frame_launch);
RTGR_INSTANTIATE_F64_F32(observer_rays_launch);

}  // namespace rtgr
