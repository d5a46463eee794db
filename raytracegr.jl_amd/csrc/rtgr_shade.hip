// rtgr_shade.hip — the kernels of image textures (include/rtgr.h "image textures"; host side: rtgr_texture_host.hip):
//   shade_kernel<R>          over a traced frame: the pixels whose object — or whose escape — has a texture bound get the texel's colour
//   eval_texture_kernel<R>   the same sampler (rtgr_texture.hpp: tex_sample) at n caller-supplied points: rtgr_eval_texture_*
// Both are memory-bound and tiny next to the trace in front of them: one lane per pixel / point, 64-bit indices, no LDS, no atomics.
#include "rtgr_host.hpp"
#include "rtgr_texture.hpp"

namespace rtgr {

static inline unsigned nblk(uint64_t n) { return (unsigned)((n + 255) / 256); }

// One lane per pixel.  hit32 and status are read coalesced; of the ray's end state (8 scalars, AoS) only the three scalars the pixel's
// bind needs — the position for an object, the velocity for an escape (and the position again for the |x_end| >= r_escape test).  The
// bind table sits in the argument block: wave-uniform, read with scalar loads as DevScene's inline objects are, and walked by a
// wave-uniform index only (a per-lane index into it would make the compiler copy the block into every lane's scratch).  A pixel matches
// one bind at most (the host refuses an object bound twice), so the lanes first pick their bind's parameters and the sampler runs once.
// The texel gathers are the only irregular traffic; every other pixel is not written.
template <class R>
__global__ __launch_bounds__(256) void shade_kernel(ShadeArgs<R> A) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A.n) return;
    const uint32_t hit = A.hit32[idx];
    const uint32_t status = A.status[idx];
    const bool ended_free = hit == 0u && (status == RTGR_RAY_LAMBDA1 || status == RTGR_RAY_OUTSIDE);
    const R* tex = nullptr;
    uint32_t W = 0, H = 0, filter = 0, kind = 0;
    R a = R(0), b = R(0), c = R(0);
#pragma unroll 1
    for (uint32_t k = 0; k < A.desc.nbind; k++) {
        const DevTexBind<R>& B = A.desc.bind[k];
        if (B.object == 0u ? ended_free : hit == B.object) {
            tex = B.tex; W = B.W; H = B.H; filter = B.filter; kind = B.kind;
            a = B.a; b = B.b; c = B.c;
        }
    }
    if (!tex) return;
    const R* se = A.state_end + idx * 8;
    R px = se[1], py = se[2], pz = se[3];
    uint32_t mapping = TEX_MAP_DIRECTION;
    if (kind == 0u) {                 // an escape: far enough out?  then the direction the ray ends with
        {
#pragma clang fp contract(off)
            const R r2 = px * px + py * py + pz * pz;
            if (!(rsqrt_<R>(r2) >= A.desc.r_escape)) return;
        }
        px = se[5]; py = se[6]; pz = se[7];
    } else if (kind == RTGR_DISK) {
        mapping = TEX_MAP_DISK;       // (a = r_in, b = r_out)
    } else {                          // a sphere of either radius sign: from its centre
        px = px - a; py = py - b; pz = pz - c;
    }
    R col[3];
    if (!tex_sample<R>(tex, W, H, filter, mapping, px, py, pz, a, b, col)) return;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) A.rgb[ch * A.plane_stride + idx] = col[ch];
}

// One lane per point: p n x 3, rgb n x 3 (AoS); a "no sample" point keeps what rgb holds.
template <class R>
__global__ __launch_bounds__(256) void eval_texture_kernel(const R* tex, uint32_t W, uint32_t H, uint32_t filter, uint32_t mapping, R r_in, R r_out,
                                                           const R* p, uint64_t n, R* rgb) {
    const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    R col[3];
    if (!tex_sample<R>(tex, W, H, filter, mapping, p[idx * 3], p[idx * 3 + 1], p[idx * 3 + 2], r_in, r_out, col)) return;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) rgb[idx * 3 + ch] = col[ch];
}

template <class R>
int shade_launch(const ShadeArgs<R>& A, hipStream_t st) {
    if (A.n == 0 || A.desc.nbind == 0) return RTGR_OK;
    hipLaunchKernelGGL(shade_kernel<R>, dim3(nblk(A.n)), dim3(256), 0, st, A);
    CHECK_LAUNCH();
    return RTGR_OK;
}
template <class R>
int eval_texture_launch(const R* d_tex, uint32_t W, uint32_t H, uint32_t filter, bool disk, R r_in, R r_out, const R* d_p, uint64_t n, R* d_rgb,
                        hipStream_t st) {
    if (n == 0) return RTGR_OK;
    hipLaunchKernelGGL(eval_texture_kernel<R>, dim3(nblk(n)), dim3(256), 0, st, d_tex, W, H, filter,
                       (uint32_t)(disk ? TEX_MAP_DISK : TEX_MAP_DIRECTION), r_in, r_out, d_p, n, d_rgb);
    CHECK_LAUNCH();
    return RTGR_OK;
}
RTGR_INSTANTIATE_F64_F32(shade_launch);
RTGR_INSTANTIATE_F64_F32(eval_texture_launch);

}  // namespace rtgr
