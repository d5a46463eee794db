// rtgr_reduce.hpp — THE reduction of one traced frame of an emitting disk to a table of (F, A, B) rows, one row per ITEM of an axis: the
// observer times of a hot-spot light curve (rtgr_lightcurve.hpp / .hip), the bins of a line profile and the sample frequencies of a thermal
// spectrum (rtgr_spectrum.hpp / .hip).  Here: the sizes, the records every reduction reads, the two kernels and their launch, each once;
// what differs between the reductions is a MODEL (below), and the kernels are instantiated per model in the unit that holds it.
//
// THE KERNEL'S SIZES.  A block is one wave (RED_WAVE lanes).  Along the pixel axis a block owns a fixed range of `chunk` pixels —
// RED_RANGE pixels while the frame has at most RED_RANGE x RED_MAX_RANGES of them, a multiple of RED_RANGE beyond — which it compacts,
// RED_RANGE at a time and in pixel order, into records of M::REC doubles in LDS (RED_RANGE x REC x 8 bytes: 12 KB for REC = 6, 8 KB for 4).
// Along the item axis a block owns RED_TILE = RED_WAVE x RED_LANE_ITEMS items, each lane RED_LANE_ITEMS of them in registers; the host
// walks the axis in passes of RED_PASS items.  So the partial sums of a pass are at most RED_MAX_RANGES x RED_PASS x 3 doubles =
// 25 165 824 bytes (24 MiB), whatever the frame and the number of items.
//
// No floating-point atomics and no cross-lane reduction: a lane OWNS its items and adds the pixels of its block's range in pixel order,
// so a sum's order of operations is fixed by (n, items) alone — the result is the same bits on every run and every stream.
//
// Included by the two kernel units and by the host code of the reductions (rtgr_reduce_host.hip and the two features' host files); no
// run-time unit and no kernel of the trace includes it.
#pragma once
#include "rtgr_host.hpp"
#include "rtgr_physics.hpp"   // (RTGR_DEV)

namespace rtgr {

constexpr unsigned RED_WAVE = 64;            // lanes per block: one wave
constexpr unsigned RED_RANGE = 256;          // pixels compacted into LDS at a time; the range of a block in a frame of <= RED_RANGE x RED_MAX_RANGES pixels
constexpr unsigned RED_LANE_ITEMS = 4;       // items a lane owns
constexpr unsigned RED_TILE = RED_WAVE * RED_LANE_ITEMS;   // items a block owns
constexpr unsigned RED_MAX_RANGES = 1024;    // blocks along the pixel axis at most
constexpr uint64_t RED_PASS = 1024;          // items per pass of the host

// pixels per block and blocks along the pixel axis for a frame of n pixels; the bytes of the partial sums of one pass ([3][blocks][pass])
inline uint64_t reduce_chunk(uint64_t n) {
    const uint64_t ranges = (n + RED_RANGE - 1) / RED_RANGE;
    return ((ranges + RED_MAX_RANGES - 1) / RED_MAX_RANGES) * RED_RANGE;
}
inline uint64_t reduce_blocks(uint64_t n) { const uint64_t c = reduce_chunk(n); return c ? (n + c - 1) / c : 0; }
inline size_t reduce_partial_bytes(uint64_t n, uint64_t items) {
    const uint64_t pass = items < RED_PASS ? items : RED_PASS;
    return align256((size_t)(3 * reduce_blocks(n) * pass * sizeof(double)));
}

// the planes of a traced frame a reduction reads: n = ni nj pixels, `object` what hit32 holds on the emitting disk
template <class R>
struct ReducePlanes {
    const uint32_t* hit32;
    const R* state_end;
    const R* g;
    uint64_t n, ni, nj;
    uint32_t object, pad;
};
// the pixel weight: proj 0: w = 1 (no observer); 1: perspective, hx, hy = tan(fov / 2), scale = hx hy (2 / ni)(2 / nj); 2: equirectangular,
// hy = fov_y / 2, scale = (fov_x / ni)(fov_y / nj)
struct PixelWeight {
    uint32_t proj, pad;
    double hx, hy, scale;
};

RTGR_DEV bool finite_f64(double x) { return x - x == 0.0; }

// pixel p of the ni x nj frame: its (a, b) and its weight
RTGR_DEV double pixel_weight(const PixelWeight& W, uint64_t p, uint64_t ni, uint64_t nj, double& a, double& b) {
    const uint64_t i = p % ni, j = p / ni;
    a = 2.0 * ((double)i + 0.5) / (double)ni - 1.0;
    b = 2.0 * ((double)j + 0.5) / (double)nj - 1.0;
    if (W.proj == 1u) {
        const double ax = a * W.hx, by = b * W.hy, s = 1.0 + ax * ax + by * by;
        return W.scale / (s * sqrt(s));
    }
    if (W.proj == 2u) return cos(b * W.hy) * W.scale;
    return 1.0;
}

// what a model makes of one pixel: whether it counts, and then the keys of its record, its weight W and its (a, b)
template <unsigned KEYS>
struct PixelRecord {
    bool act = false;
    double key[KEYS], w = 0.0, a = 0.0, b = 0.0;
};

// what the kernels read: everything wave-uniform sits in the argument block (scalar loads).  Spec: the model's own record
template <class R, class Spec>
struct ReduceArgs {
    ReducePlanes<R> P;
    Spec S;
    PixelWeight W;
    double* partial;     // [3][blocks][items]
    uint64_t chunk;      // pixels per block along the pixel axis
    uint64_t k0, items;  // this pass: items k0 .. k0 + items - 1
    const void* head;    // the model's word of the stream's scratch head (the light curve: Omega_s), or null.  (Last: in front of
                         // `partial` it moved the spectra's scalar loads and cost LINE 36 bytes of scratch)
};

// A MODEL M — static RTGR_DEV functions and constants only, so that every choice is made when the kernel is compiled:
//   Scalar, Spec         the scalar type of the planes; the model's record in the argument block
//   REC                  doubles per record in LDS: REC - 3 keys of the model's, then W, W a, W b
//   Block                what the model reads once per block;  bool begin(S, head, Block&) — false: nothing to sum (the reduction kernel
//                        returns, the sum kernel writes NaN and reads no partial sum)
//   Items                the per-lane state of the lane's RED_LANE_ITEMS items (arrays over s);  void item(S, B, k, Items&, s) for item
//                        k of the whole axis, the lane's s-th
//   PixelRecord<REC - 3> cull(A, B, p, g, tile0)   pixel p (on the disk, g finite and > 0) into whether it counts and, if so, the keys, the
//                        weight W and (a, b) of its record; tile0: the first item of the block's tile, on the whole axis.  (Returned by
//                        value: with the outputs as reference parameters the compiler merged THERMAL's two conditional regions and took
//                        172 registers for 170 — profiles/reduce/README.md)
//   void walk(S, key, w, wa, wb, it, s, live, slot, F, Fa, Fb)     one record (its keys; W, W a, W b) against the lane's s-th item: `live`
//                        whether the item's sub-tile has any item of the pass (wave-uniform), `slot` the item's place in the tile, (F, Fa,
//                        Fb) its sums
//   void finish(S, k, v) what is applied to the summed (F, A, B) of item k once
//
// Block (bx, by): the pixels [bx chunk, (bx + 1) chunk) x the items k0 + by RED_TILE + s RED_WAVE + lane, s < RED_LANE_ITEMS.
// CULL: hit32 is read coalesced; a lane whose pixel is not on the disk is done after that one load, one whose g is no positive finite
// number after a second; the others go through the model's cull.  COMPACT: the active lanes of a round of RED_WAVE pixels write their
// records to LDS behind those of the rounds before, in pixel order (ballot + count of the lanes below).  WALK: every lane reads record
// after record — one address for the whole wave, which LDS broadcasts without a bank conflict — and walks it against each of its items,
// whose sums stay in registers.
template <class M>
__global__ __launch_bounds__(RED_WAVE) void reduce_kernel(ReduceArgs<typename M::Scalar, typename M::Spec> A) {
    constexpr unsigned KEYS = M::REC - 3;
    __shared__ double rec[RED_RANGE * M::REC];
    typename M::Block B;
    if (!M::begin(A.S, A.head, B)) return;
    const unsigned lane = threadIdx.x;
    const uint64_t kt = (uint64_t)blockIdx.y * RED_TILE;   // first item of the tile, within the pass
    const uint64_t tile0 = A.k0 + kt;                      // … and on the whole axis
    const unsigned left = (unsigned)(A.items - kt < RED_TILE ? A.items - kt : RED_TILE);
    const unsigned ns = (left + RED_WAVE - 1) / RED_WAVE;   // live sub-tiles: wave-uniform
    typename M::Items it;
    double F[RED_LANE_ITEMS], Fa[RED_LANE_ITEMS], Fb[RED_LANE_ITEMS];
#pragma unroll
    for (unsigned s = 0; s < RED_LANE_ITEMS; s++) {
        M::item(A.S, B, tile0 + s * RED_WAVE + lane, it, s);
        F[s] = Fa[s] = Fb[s] = 0.0;
    }
    const uint64_t p0 = (uint64_t)blockIdx.x * A.chunk;
    const uint64_t p1 = p0 + A.chunk < A.P.n ? p0 + A.chunk : A.P.n;
    for (uint64_t base = p0; base < p1; base += RED_RANGE) {
        unsigned cnt = 0;
#pragma unroll 1
        for (unsigned r = 0; r < RED_RANGE / RED_WAVE; r++) {
            const uint64_t p = base + r * RED_WAVE + lane;
            bool act = false;
            PixelRecord<KEYS> px;
            if (p < p1 && A.P.hit32[p] == A.P.object) {
                const double g = (double)A.P.g[p];
                if (g > 0.0 && finite_f64(g)) {
                    px = M::cull(A, B, p, g, tile0);
                    act = px.act;
                }
            }
            const unsigned long long m = __ballot(act);
            if (act) {
                const unsigned slot = cnt + __builtin_popcountll(m & ((1ull << lane) - 1ull));
                double* q = rec + slot * M::REC;
#pragma unroll
                for (unsigned c = 0; c < KEYS; c++) q[c] = px.key[c];
                q[KEYS] = px.w; q[KEYS + 1] = px.w * px.a; q[KEYS + 2] = px.w * px.b;
            }
            cnt += (unsigned)__builtin_popcountll(m);
        }
        __syncthreads();
        for (unsigned i = 0; i < cnt; i++) {
            const double* q = rec + i * M::REC;
            double key[KEYS];
#pragma unroll
            for (unsigned c = 0; c < KEYS; c++) key[c] = q[c];
            const double w = q[KEYS], wa = q[KEYS + 1], wb = q[KEYS + 2];
#pragma unroll
            for (unsigned s = 0; s < RED_LANE_ITEMS; s++) M::walk(A.S, key, w, wa, wb, it, s, s < ns, s * RED_WAVE + lane, F[s], Fa[s], Fb[s]);
        }
        __syncthreads();   // (the next round of this block overwrites the records)
    }
    const uint64_t plane = (uint64_t)gridDim.x * A.items;
#pragma unroll
    for (unsigned s = 0; s < RED_LANE_ITEMS; s++) {
        const uint64_t kk = kt + s * RED_WAVE + lane;
        if (kk < A.items) {
            double* q = A.partial + (uint64_t)blockIdx.x * A.items + kk;
            q[0] = F[s]; q[plane] = Fa[s]; q[2 * plane] = Fb[s];
        }
    }
}

// one lane per item of the pass: the partial sums of the `blocks` ranges added in range order (reads coalesced along the items), then
// the model's finish
template <class M>
__global__ __launch_bounds__(256) void reduce_sum_kernel(typename M::Spec S, const void* head, const double* __restrict__ partial, uint64_t blocks,
                                                         uint64_t k0, uint64_t items, double* __restrict__ out) {
    const uint64_t kk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (kk >= items) return;
    double v[3];
    typename M::Block B;
    if (!M::begin(S, head, B)) {
        v[0] = v[1] = v[2] = __builtin_nan("");
    } else {
        const uint64_t plane = blocks * items;
        v[0] = v[1] = v[2] = 0.0;
#pragma unroll 16   // (the loads of sixteen ranges in flight; the additions stay in range order)
        for (uint64_t bx = 0; bx < blocks; bx++) {
            const double* q = partial + bx * items + kk;
            v[0] += q[0]; v[1] += q[plane]; v[2] += q[2 * plane];
        }
        M::finish(S, k0 + kk, v);
    }
    double* o = out + (k0 + kk) * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// THE launch: items x 3 doubles into d_out, pass by pass over the item axis — the partial sums of a pass in d_partial
// (reduce_partial_bytes), then their sum in range order
template <class M>
int reduce_launch(const ReducePlanes<typename M::Scalar>& P, const typename M::Spec& S, const PixelWeight& W, uint64_t items, const void* d_head,
                  double* d_partial, double* d_out, hipStream_t st) {
    ReduceArgs<typename M::Scalar, typename M::Spec> A;
    A.P = P; A.S = S; A.W = W;
    A.head = d_head;
    A.partial = d_partial;
    A.chunk = reduce_chunk(P.n);
    const uint64_t blocks = reduce_blocks(P.n);
    for (uint64_t k0 = 0; k0 < items; k0 += RED_PASS) {
        A.k0 = k0;
        A.items = items - k0 < RED_PASS ? items - k0 : RED_PASS;
        const unsigned tiles = (unsigned)((A.items + RED_TILE - 1) / RED_TILE);
        hipLaunchKernelGGL(reduce_kernel<M>, dim3((unsigned)blocks, tiles), dim3(RED_WAVE), 0, st, A);
        CHECK_LAUNCH();
        hipLaunchKernelGGL(reduce_sum_kernel<M>, dim3((unsigned)((A.items + 255) / 256)), dim3(256), 0, st, S, d_head, (const double*)d_partial, blocks, k0,
                           A.items, d_out);
        CHECK_LAUNCH();
    }
    return RTGR_OK;
}

}  // namespace rtgr
