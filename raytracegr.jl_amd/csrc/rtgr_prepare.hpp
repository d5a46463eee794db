// rtgr_prepare.hpp — the pipeline ahead of the integrate kernel: ray set-up, the per-launch reset, the longest-expected-first queue order
#pragma once
#include "rtgr_camera.hpp"

namespace rtgr {

// ---------------------------------------------------------------------------------------------------------------------
// ray ordering: longest-expected-first (LPT) queue order
//
// Rays need 27…991 step attempts and a lane processes its rays one after another, so with few rays per lane (small
// screens, or one slab of an 8-GPU split: ~10 rays per lane) the kernel time is set by the lanes that happen to draw a
// long ray LAST: greedy scheduling in natural order runs 1.24x (10 rays/lane) … 1.46x (5 rays/lane) over the ideal.
// The rays that get long are the ones aimed at the hole, so the queue is ordered by the angle α between the ray and the
// direction to the origin (sin α = impact parameter / distance): a 256-bucket counting sort, ascending.  Simulated
// makespan over ideal with that order: 1.02-1.03.  The order only changes WHEN a ray is integrated, never its result.
// ---------------------------------------------------------------------------------------------------------------------
template <class R>
RTGR_DEV void order_key(const R x4[4], const R u4[4], bool valid, uint64_t w, uint8_t* keys, uint32_t* hist) {
    __shared__ uint32_t lh[256];  // called by every thread of a 256-thread block (prepare_kernel)
    lh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t b = 0xffffffffu;
    if (valid) {
        const R x = x4[1], y = x4[2], z = x4[3], ux = u4[1], uy = u4[2], uz = u4[3];
        const R xx = x * x + y * y + z * z, uu = ux * ux + uy * uy + uz * uz, xu = x * ux + y * uy + z * uz;
        float sin2 = 1.0f;
        if (xu < R(0) && xx > R(0) && uu > R(0)) sin2 = fmaxf(0.0f, 1.0f - (float)(xu * xu / (xx * uu)));
        b = (uint32_t)fminf(255.0f, 256.0f * __builtin_sqrtf(sin2));  // moving away -> last bucket
        keys[w] = (uint8_t)b;
    }
    // neighbouring rays share a handful of buckets: one LDS atomic per distinct bucket per wave, not one per ray
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t b0 = __shfl(b, (int)leader, 64);
        const unsigned long long m = __ballot(valid && b == b0);
        if ((threadIdx.x & 63) == leader) atomicAdd(&lh[b0], (uint32_t)__builtin_popcountll(m));
        todo &= ~m;
    }
    __syncthreads();
    if (lh[threadIdx.x]) atomicAdd(&hist[threadIdx.x], lh[threadIdx.x]);
}

// Ray set-up, one thread per ray: the camera ray itself when the caller gave a camera instead of states (make_canvas,
// :457-478 — the state never goes through HBM), its key for the longest-first queue (see "ray ordering" below), u̇(y0), the Hairer initial step (d0, d1, one Euler probe, d2; the
// norms in f32 like the controller's), sign(min_distance(y0)) for the ContinuousCallback (App. B.4) and the controller's
// q_old = 1e-4 (App. B.2) -> the ray's 16-scalar start record.  2 RHS evaluations per ray (counted by the integrate
// kernel's counters).  A body function for the same reason as integrate_body.
template <class R, int METRIC, bool SPIN>
RTGR_DEV void prepare_body(const IntegrateArgs<R>& A) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = w < A.n;
    const MetricK<R> MK = scene_consts<R, METRIC>(A.sc);
    const R reltol = A.opt.reltol, abstol = A.opt.abstol, dtmax = A.opt.lambda1 - A.opt.lambda0;
    R x[4] = {R(0), R(1), R(0), R(0)}, u[4] = {R(-1), R(0), R(1), R(0)}, k1[4], k2[4];
    if (valid) {
        if (A.state0) {
            const R* s0 = A.state0 + w * 8;
            bool bad = false;
#pragma unroll
            for (int q = 0; q < 4; q++) { x[q] = s0[q]; u[q] = s0[4 + q]; bad = bad || x[q] != x[q] || u[q] != u[q]; }
            // `@assert !any(isnan, xx)` of kerr_schild (src/RayTraceGR.jl:279): evaluated here, where every caller-supplied
            // state is read anyway; the host entry points turn the flag into RTGR_ERR_NAN_INPUT
            if (bad && A.nan_flag) atomicOr(A.nan_flag, 1u);
        } else {  // make_canvas (src/RayTraceGR.jl:457-478) for this pixel, straight into registers
            R s[8];
            const uint64_t idx = A.first + w;
            make_pixel<R, Sampled<R, METRIC>::NE>(A.sc, A.cam, A.ni, A.nj, idx % A.ni, A.j0 + (idx / A.ni) * A.jstride, s);
#pragma unroll
            for (int q = 0; q < 4; q++) { x[q] = s[q]; u[q] = s[4 + q]; }
        }
    }
    if (A.keys) order_key<R>(x, u, valid, w, A.keys, A.hist);  // block-wide (LDS histogram): before any early exit
    if (!valid) return;
    // The ray's state is a VALUE from here on, whichever way it was obtained: without this barrier the compiler contracts
    // the last product of make_pixel (u = (…)·1/√2) into the first sum of the RHS (k_a u^a = u^t + …) when the camera ray
    // is generated in this kernel, and cannot when the same ray is loaded from the caller's array — camera and state0
    // frames then differ in the last bit of u̇(y0) (found by test_host_pipeline_with_many_chunks_and_every_output).
#pragma unroll
    for (int q = 0; q < 4; q++) { asm volatile("" : "+v"(x[q])); asm volatile("" : "+v"(u[q])); }
    accel<R, METRIC, SPIN, true>(x + 1, u, MK, k1, x[0]);      // f0 = (u, k1)
    float acc0 = 0.0f, acc1 = 0.0f;
    float iskx[4], isku[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        iskx[q] = __builtin_amdgcn_rcpf((float)rfma(rabs(x[q]), reltol, abstol));
        isku[q] = __builtin_amdgcn_rcpf((float)rfma(rabs(u[q]), reltol, abstol));
        const float a0 = (float)x[q] * iskx[q], b0 = (float)u[q] * isku[q];
        const float a1 = (float)u[q] * iskx[q], b1 = (float)k1[q] * isku[q];
        acc0 = __builtin_fmaf(a0, a0, __builtin_fmaf(b0, b0, acc0));
        acc1 = __builtin_fmaf(a1, a1, __builtin_fmaf(b1, b1, acc1));
    }
    const float d0f = __builtin_sqrtf(acc0 * 0.125f), d1f = __builtin_sqrtf(acc1 * 0.125f);
    const float dt0f = (d0f < 1e-5f || d1f < 1e-5f) ? 1e-6f : (d0f / d1f) * 0.01f;
    const R dt0 = rmin((R)dt0f, dtmax);
    R X[3], U[4];                                              // y0 + dt0 f0
#pragma unroll
    for (int q = 0; q < 4; q++) U[q] = rfma(dt0, k1[q], u[q]);
#pragma unroll
    for (int q = 0; q < 3; q++) X[q] = rfma(dt0, u[1 + q], x[1 + q]);
    accel<R, METRIC, SPIN, true>(X, U, MK, k2, rfma(dt0, u[0], x[0]));          // f1 − f0 = (dt0·k1, k2 − k1)
    float acc2 = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const float a2 = (float)(dt0 * k1[q]) * iskx[q], b2 = (float)(k2[q] - k1[q]) * isku[q];
        acc2 = __builtin_fmaf(a2, a2, __builtin_fmaf(b2, b2, acc2));
    }
    const float d2f = __builtin_sqrtf(acc2 * 0.125f) / (float)dt0;
    const float md = fmaxf(d1f, d2f);
    // dt1 = 10^(-(2 + log10 md)/5) = 2^(-(2 log2 10 + log2 md)/5)
    const float dt1f = (md <= 1e-15f) ? fmaxf(1e-6f, (float)dt0 * 1e-3f) : fexp2(-0.2f * (6.643856189774724f + flog2(md)));
    const R dt_init = rmin(rmin(R(100) * dt0, (R)dt1f), dtmax);
    R* hd = A.hand + w * HAND_W;
#pragma unroll
    for (int q = 0; q < 4; q++) { hd[q] = x[q]; hd[4 + q] = u[q]; hd[8 + q] = k1[q]; }
    hd[12] = A.opt.lambda0;
    hd[13] = dt_init;
    hd[14] = rsign(min_distance<R>(A.sc, x));
    hd[15] = R(-13.287712379549449);                           // log2(qoldinit = 1e-4)
}

template <class R, int METRIC, bool SPIN>
__global__ __launch_bounds__(256) void prepare_kernel(const IntegrateArgs<R> A) {
    prepare_body<R, METRIC, SPIN>(A);
}

// Per-launch reset of the queue heads and of the ordering histogram.  A kernel rather than hipMemsetAsync: memset nodes
// of a captured HIP graph were observed not to re-run on later replays (ROCm 7.0 runtime bundled with PyTorch), which
// left stale queue heads / histograms and sent the scatter out of bounds; kernel nodes replay reliably.
static __global__ __launch_bounds__(256) void reset_kernel(unsigned long long* ctrl, uint32_t* hist512) {
    if (threadIdx.x < 8) ctrl[threadIdx.x] = 0ull;
    if (hist512) { hist512[threadIdx.x] = 0u; hist512[256 + threadIdx.x] = 0u; }
}

// exclusive prefix sum of the 256-bin histogram (one block) -> running offsets used by the scatter
static __global__ __launch_bounds__(256) void order_scan_kernel(const uint32_t* hist, uint32_t* offsets) {
    __shared__ uint32_t sh[256];
    sh[threadIdx.x] = hist[threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int b = 0; b < 256; b++) { const uint32_t c = sh[b]; sh[b] = acc; acc += c; }
    }
    __syncthreads();
    offsets[threadIdx.x] = sh[threadIdx.x];
}
// order[offset(bucket)++] = ray index.  Ranks inside a 256-ray block come from LDS atomics; each block then claims its
// range of every non-empty bucket with ONE global atomic (neighbouring rays share a handful of buckets).
static __global__ __launch_bounds__(256) void order_scatter_kernel(const uint8_t* keys, uint64_t n, uint32_t* offsets, uint32_t* order) {
    __shared__ uint32_t lcount[256], gbase[256];
    lcount[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = w < n;
    const uint32_t b = valid ? keys[w] : 0xffffffffu;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t r = 0;
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {  // one LDS atomic per distinct bucket per wave; lanes rank themselves inside the ballot mask
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t b0 = __shfl(b, (int)leader, 64);
        const unsigned long long m = __ballot(valid && b == b0);
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(&lcount[b0], (uint32_t)__builtin_popcountll(m));
        base = __shfl(base, (int)leader, 64);
        if (valid && b == b0) r = base + mask_rank(m, lane);
        todo &= ~m;
    }
    __syncthreads();
    if (lcount[threadIdx.x]) gbase[threadIdx.x] = atomicAdd(&offsets[threadIdx.x], lcount[threadIdx.x]);
    __syncthreads();
    if (valid) order[gbase[b] + r] = (uint32_t)w;
}

}  // namespace rtgr
