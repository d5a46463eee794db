// rtgr_orders.hpp — higher-order disk images (include/rtgr.h "higher-order disk images"): what the small kernels of rtgr_orders.hip read,
// and the two rules they apply.  No kernel of the trace includes this header; the legs themselves are ordinary traces.
//
// A LEG's rays are either the pixels of the frame (leg 0: slot = pixel) or a compact list (every later leg): entry i of the list is the
// ray in slot i of the leg's arrays and belongs to pixel pix[i].  The list order is whatever order the waves' atomics arrive in; every
// result is scattered back by pixel index, so nothing depends on it.
#pragma once
#include <cstdint>

#include "rtgr_args.hpp"

namespace rtgr {

// Select: from a leg's hit32 (and status, when the rule asks for an event), the rays that go on.  Entry j of the new list: slot[j] = the
// ray's slot in the leg's arrays, pix[j] = its pixel.  count_plane (leg 0 only, may be null): 1 where the pixel is on the list, else 0.
struct OrdersSelectArgs {
    const uint32_t* hit32;      // m_in
    const uint8_t* status;      // m_in, or null: the status is not asked
    const uint64_t* src_pix;    // m_in: the pixel of slot i, or null: slot i is pixel i
    uint64_t m_in;
    uint32_t object;            // the rays with hit32 == object go on …
    uint32_t need_event;        // … if, when this is set, their status is RTGR_RAY_EVENT
    uint64_t* slot;             // out, *count entries
    uint64_t* pix;              // out, likewise
    unsigned long long* count;  // the caller zeroes it on the stream
    uint8_t* count_plane;       // m_in bytes, or null
};

// Gather: dst[j] = src[idx[j]], 8 scalars each — the end states of the listed rays, or (idx = pix) their start states.
template <class R>
struct OrdersGatherArgs {
    const R* src;
    const uint64_t* idx;
    uint64_t m;
    R* dst;
};

// Fill: blocks 1 .. N of the per-order planes before anything is scattered into them: 0 in hit32, NaN in the others.  Any plane may be
// null.  `per` = N n entries of hit32 and g, 8 per of state_end, 3 per of rgb_order.
template <class R>
struct OrdersFillArgs {
    uint32_t* hit32;
    R* state_end;
    R* g;
    R* rgb_order;
    uint64_t per;
};

// Scatter and composite: a continuation leg's compact results (m rays, colour planes m apart) into the picture (planes n apart) and into
// block k of the per-order planes.  c = the leg's colour of the ray — E_k where it ended on the disk (the emission kernel has written
// it), else the background B (plain or shaded):  rgb = rgb + t c  either way, unfused.  Where it ended on the disk the pixel has order k.
template <class R>
struct OrdersScatterArgs {
    const uint64_t* pix;       // m
    const uint32_t* hit32;     // m
    const R* state_end;        // m x 8
    const R* g;                // m (NaN off the disk)
    const R* rgb_leg;          // 3 planes of m
    uint64_t m, n;
    uint32_t object, pad;
    R t;
    R* rgb;                    // 3 planes of n
    uint8_t* count;            // n, or null
    uint32_t* hit32_k;         // block k of the planes, each may be null
    R* state_end_k;
    R* g_k;
    R* rgb_order_k;
};

// the launches (rtgr_orders.hip), each a no-op for an empty list
int orders_select_launch(const OrdersSelectArgs& A, hipStream_t st);
template <class R> int orders_gather_launch(const OrdersGatherArgs<R>& A, hipStream_t st);
template <class R> int orders_fill_launch(const OrdersFillArgs<R>& A, hipStream_t st);
template <class R> int orders_scatter_launch(const OrdersScatterArgs<R>& A, hipStream_t st);

}  // namespace rtgr
