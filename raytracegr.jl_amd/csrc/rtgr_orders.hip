// rtgr_orders.hip — the small kernels of higher-order disk images (include/rtgr.h "higher-order disk images"; host side:
// rtgr_orders_host.hip; argument blocks: rtgr_orders.hpp):
//   orders_select_kernel       a leg's hit32 / status -> the list of the rays that go on (slot and pixel of each) and its length
//   orders_gather_kernel<R>    the listed rays' states into a compact array
//   orders_fill_kernel<R>      0 / NaN into the per-order planes of orders >= 1
//   orders_scatter_kernel<R>   a continuation leg's compact results into the picture and into one block of the per-order planes
// One lane per pixel or per listed ray, blocks of 256, 64-bit indices, no LDS, no floating-point atomics: the only atomic is the one
// integer add per wave that reserves the wave's range of the list.  All four are memory-bound and tiny next to the legs between them.
#include "rtgr_host.hpp"
#include "rtgr_orders.hpp"

namespace rtgr {

static inline unsigned nblk(uint64_t n) { return (unsigned)((n + 255) / 256); }

// One lane per ray of the leg.  The list is appended with ONE atomic per wave, as aa_flag_kernel does: the lanes that go on are counted
// with a ballot, lane 0 reserves the wave's range and every such lane writes at its rank inside it.  A lane beyond m_in takes part in
// the ballot with `false` (no lane leaves before it).  The list holds at most m_in entries: slot and pix are m_in long.
__global__ __launch_bounds__(256) void orders_select_kernel(OrdersSelectArgs A) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool f = false;
    if (i < A.m_in) {
        f = A.hit32[i] == A.object && (!A.need_event || A.status[i] == 0 /* RTGR_RAY_EVENT */);
        if (A.count_plane) A.count_plane[i] = f ? 1 : 0;
    }
    const unsigned long long mask = __ballot(f);
    const unsigned lane = threadIdx.x & 63u;
    unsigned long long base = 0;
    if (lane == 0 && mask != 0) base = atomicAdd(A.count, (unsigned long long)__popcll(mask));
    base = __shfl(base, 0);
    if (f) {
        const unsigned long long at = base + (unsigned long long)__popcll(mask & ((1ull << lane) - 1ull));
        A.slot[at] = i;
        A.pix[at] = A.src_pix ? A.src_pix[i] : i;
    }
}

template <class R>
__global__ __launch_bounds__(256) void orders_gather_kernel(OrdersGatherArgs<R> A) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= A.m) return;
    const uint64_t s = A.idx[j];
#pragma unroll
    for (int c = 0; c < 8; c++) A.dst[j * 8 + c] = A.src[s * 8 + c];
}

// One lane per entry of the g plane; the other planes in the same lane: hit32 likewise, 8 scalars of state_end, 3 of rgb_order (every
// scalar of its blocks is NaN, so the lane fills entries 3 q .. 3 q + 2 whatever plane they lie in).
template <class R>
__global__ __launch_bounds__(256) void orders_fill_kernel(OrdersFillArgs<R> A) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= A.per) return;
    const R nan = R(__builtin_nan(""));
    if (A.hit32) A.hit32[q] = 0u;
    if (A.g) A.g[q] = nan;
    if (A.state_end)
#pragma unroll
        for (int c = 0; c < 8; c++) A.state_end[q * 8 + c] = nan;
    if (A.rgb_order)
#pragma unroll
        for (int c = 0; c < 3; c++) A.rgb_order[q * 3 + c] = nan;
}

// One lane per listed ray.  A pixel is on a list at most once, so no two lanes write the same pixel.
template <class R>
__global__ __launch_bounds__(256) void orders_scatter_kernel(OrdersScatterArgs<R> A) {
#pragma clang fp contract(off)
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.m) return;
    const uint64_t p = A.pix[i];
    R col[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        col[c] = A.rgb_leg[c * A.m + i];
        const R add = A.t * col[c];
        A.rgb[c * A.n + p] = A.rgb[c * A.n + p] + add;
    }
    if (A.hit32[i] != A.object) return;
    if (A.count) A.count[p] = (uint8_t)(A.count[p] + 1);
    if (A.hit32_k) A.hit32_k[p] = A.object;
    if (A.g_k) A.g_k[p] = A.g[i];
    if (A.state_end_k)
#pragma unroll
        for (int c = 0; c < 8; c++) A.state_end_k[p * 8 + c] = A.state_end[i * 8 + c];
    if (A.rgb_order_k)
#pragma unroll
        for (int c = 0; c < 3; c++) A.rgb_order_k[c * A.n + p] = col[c];
}

int orders_select_launch(const OrdersSelectArgs& A, hipStream_t st) {
    if (A.m_in == 0) return RTGR_OK;
    hipLaunchKernelGGL(orders_select_kernel, dim3(nblk(A.m_in)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}
template <class R>
int orders_gather_launch(const OrdersGatherArgs<R>& A, hipStream_t st) {
    if (A.m == 0) return RTGR_OK;
    hipLaunchKernelGGL(orders_gather_kernel<R>, dim3(nblk(A.m)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}
template <class R>
int orders_fill_launch(const OrdersFillArgs<R>& A, hipStream_t st) {
    if (A.per == 0) return RTGR_OK;
    hipLaunchKernelGGL(orders_fill_kernel<R>, dim3(nblk(A.per)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}
template <class R>
int orders_scatter_launch(const OrdersScatterArgs<R>& A, hipStream_t st) {
    if (A.m == 0) return RTGR_OK;
    hipLaunchKernelGGL(orders_scatter_kernel<R>, dim3(nblk(A.m)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(orders_gather_launch);
RTGR_INSTANTIATE_F64_F32(orders_fill_launch);
RTGR_INSTANTIATE_F64_F32(orders_scatter_launch);

}  // namespace rtgr
