// rtgr_aa.hip — the small kernels of adaptive anti-aliasing (include/rtgr.h "adaptive anti-aliasing"; host side: rtgr_aa_host.hip):
//   aa_flag_kernel<R>      the edge rule over a traced frame -> flag bytes + the list of flagged pixels
//   aa_subrays_kernel<R>   the k x k sub-rays of the listed pixels: make_pixel of the k-times finer canvas, as canvas_kernel writes them
//   aa_reduce_kernel<R>    the sub-rays' colours averaged into the listed pixels of the frame
// All three are memory-bound and tiny next to the trace between them: one thread per pixel / sub-ray, 64-bit indices, nothing clever.
#include "rtgr_host.hpp"
#include "rtgr_camera.hpp"

namespace rtgr {

static inline unsigned nblk(uint64_t n) { return (unsigned)((n + 255) / 256); }

// does pixel p differ from its neighbour q (both inside the frame)?
template <class R>
RTGR_DEV bool aa_differs(const R* rgb, const uint32_t* hit32, const uint8_t* status, uint64_t n, uint64_t p, uint64_t q, R contrast) {
    if (hit32[p] != hit32[q] || status[p] != status[q]) return true;
    R d = R(0);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        R e = rgb[c * n + p] - rgb[c * n + q];
        e = e < R(0) ? -e : e;
        d = e > d ? e : d;   // (a NaN difference never wins: not an edge)
    }
    return d > contrast;
}

// One thread per pixel, idx = i + j ni.  Neighbours are read only where they are inside the frame (ni = 1 / nj = 1: none on that axis).
// The list is appended with ONE atomic per wave: the flagged lanes are counted with a ballot, lane 0 reserves the wave's range and
// every flagged lane writes at its rank inside it.  The order of the list is whatever order the waves' atomics arrive in; nothing
// downstream depends on it (a listed pixel's result is a function of the pixel alone).
template <class R>
__global__ __launch_bounds__(256) void aa_flag_kernel(const R* rgb, const uint32_t* hit32, const uint8_t* status, uint64_t ni, uint64_t nj,
                                                      R contrast, int all, uint8_t* flag, uint64_t* list, unsigned long long* count) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t n = ni * nj;
    bool f = false;
    if (idx < n) {
        f = all != 0;
        if (!f) {
            const uint64_t i = idx % ni, j = idx / ni;
            if (i > 0) f = f || aa_differs<R>(rgb, hit32, status, n, idx, idx - 1, contrast);
            if (i + 1 < ni) f = f || aa_differs<R>(rgb, hit32, status, n, idx, idx + 1, contrast);
            if (j > 0) f = f || aa_differs<R>(rgb, hit32, status, n, idx, idx - ni, contrast);
            if (j + 1 < nj) f = f || aa_differs<R>(rgb, hit32, status, n, idx, idx + ni, contrast);
        }
        if (flag) flag[idx] = f ? 1 : 0;
    }
    // (no lane has left: the whole wave takes part in the ballot and lane 0 is there to reserve the range)
    const unsigned long long mask = __ballot(f);
    const unsigned lane = threadIdx.x & 63u;
    unsigned long long base = 0;
    if (lane == 0 && mask != 0) base = atomicAdd(count, (unsigned long long)__popcll(mask));
    base = __shfl(base, 0);
    if (f) list[base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull))] = idx;
}

// One thread per sub-ray w = p k² + t k + s of listed pixel p = (i, j): the camera ray of pixel (k i + s, k j + t) of the (k ni) x (k nj)
// canvas — make_pixel, the function every camera ray of the library comes from, with canvas_kernel's switch for a time-dependent grid.
template <class R>
__global__ __launch_bounds__(256) void aa_subrays_kernel(DevScene<R> sc, DevCamera<R> cam, uint64_t ni, uint64_t nj, uint32_t k,
                                                         const uint64_t* list, uint64_t nsub, R* state0) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nsub) return;
    const uint32_t kk = k * k;
    const uint64_t p = w / kk;
    const uint32_t r = (uint32_t)(w - p * kk), t = r / k, s = r - t * k;
    const uint64_t idx = list[p], i = idx % ni, j = idx / ni;
    R st[8];
    if (sampled_on(sc.metric, 4)) make_pixel<R, 4>(sc, cam, k * ni, k * nj, k * i + s, k * j + t, st);
    else make_pixel<R>(sc, cam, k * ni, k * nj, k * i + s, k * j + t, st);
#pragma unroll
    for (int c = 0; c < 8; c++) state0[w * 8 + c] = st[c];
}

// One thread per listed pixel: per channel 0 + the k² sub-colours in their stored order (t outer, s inner), one IEEE division by k².
template <class R>
__global__ __launch_bounds__(256) void aa_reduce_kernel(const R* sub, const uint64_t* list, uint64_t npix, uint32_t k, R* rgb, uint64_t n) {
#pragma clang fp contract(off)
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const uint32_t kk = k * k;
    const uint64_t nsub = npix * kk, idx = list[p];
    const R den = R(kk);
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const R* v = sub + c * nsub + p * kk;
        R acc = R(0);
        for (uint32_t q = 0; q < kk; q++) acc = acc + v[q];
        rgb[c * n + idx] = acc / den;
    }
}

template <class R>
int aa_flag(const R* d_rgb, const uint32_t* d_hit32, const uint8_t* d_status, uint64_t ni, uint64_t nj, R contrast, bool all, uint8_t* d_flag,
            uint64_t* d_list, unsigned long long* d_count, hipStream_t st) {
    hipLaunchKernelGGL(aa_flag_kernel<R>, dim3(nblk(ni * nj)), dim3(256), 0, st, d_rgb, d_hit32, d_status, ni, nj, contrast, all ? 1 : 0,
                       d_flag, d_list, d_count);
    CHECK_LAUNCH();
    return RTGR_OK;
}
template <class R>
int aa_subrays(const DevScene<R>& sc, const DevCamera<R>& cam, uint64_t ni, uint64_t nj, uint32_t k, const uint64_t* d_list, uint64_t npix,
               R* d_state0, hipStream_t st) {
    const uint64_t nsub = npix * k * k;
    hipLaunchKernelGGL(aa_subrays_kernel<R>, dim3(nblk(nsub)), dim3(256), 0, st, sc, cam, ni, nj, k, d_list, nsub, d_state0);
    CHECK_LAUNCH();
    return RTGR_OK;
}
template <class R>
int aa_reduce(const R* d_sub, const uint64_t* d_list, uint64_t npix, uint32_t k, R* d_rgb, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(aa_reduce_kernel<R>, dim3(nblk(npix)), dim3(256), 0, st, d_sub, d_list, npix, k, d_rgb, n);
    CHECK_LAUNCH();
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(aa_flag);
RTGR_INSTANTIATE_F64_F32(aa_subrays);
RTGR_INSTANTIATE_F64_F32(aa_reduce);

}  // namespace rtgr
