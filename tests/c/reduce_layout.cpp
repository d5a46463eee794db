// The reduction scratch of a stream (reduce_layout, csrc/rtgr_internal.hpp; the partial sums' size: reduce_partial_bytes, csrc/rtgr_reduce.hpp)
// over every combination of planes the caller gave, with and without a head: a host-only program, built against the headers alone
// (tests/test_frame_stages.py).  Every offset is held against the formula the light-curve and spectrum entries each wrote out before
// there was one layout, restated here.  Prints the number of cases and exits 0, or names the first case that breaks a rule and exits 1.
#include <cstdio>

#include "rtgr_internal.hpp"
#include "rtgr_reduce.hpp"

using namespace rtgr;

struct Block { const char* name; size_t at, bytes; };

static size_t a256(size_t b) { return (b + 255) & ~(size_t)255; }

// the partial sums of one pass, as lc_partial_bytes and spec_partial_bytes both had it: 3 planes x blocks x min(items, 1024) doubles
static size_t old_partial_bytes(uint64_t n, uint64_t items) {
    const uint64_t ranges = (n + 256 - 1) / 256;
    const uint64_t chunk = ((ranges + 1024 - 1) / 1024) * 256;
    const uint64_t blocks = chunk ? (n + chunk - 1) / chunk : 0;
    const uint64_t pass = items < 1024 ? items : 1024;
    return a256((size_t)(3 * blocks * pass * sizeof(double)));
}

static int bad(const char* what, const char* block, uint64_t n, size_t scalar, size_t head, uint64_t items, const ReduceGiven& given) {
    std::printf("%s (%s): n = %llu, scalar = %zu, head = %zu, items = %llu, given: state_end %d hit32 %d g %d\n", what, block, (unsigned long long)n, scalar,
                head, (unsigned long long)items, given.state_end, given.hit32, given.g);
    return 1;
}

int main() {
    const uint64_t sizes[] = {1, 77, 2496, 1000003};
    const size_t scalars[] = {4, 8};
    const size_t heads[] = {0, 1024};
    const uint64_t item_counts[] = {1, 1024, 70000};
    int cases = 0;
    for (uint64_t n : sizes)
        for (size_t scalar : scalars)
            for (size_t head : heads)
                for (uint64_t items : item_counts)
                    for (int g = 0; g < 8; g++) {
                        ReduceGiven given;
                        given.state_end = g & 1; given.hit32 = g & 2; given.g = g & 4;
                        const size_t partial = reduce_partial_bytes(n, items);
                        if (partial != old_partial_bytes(n, items)) return bad("the partial sums changed size", "partial", n, scalar, head, items, given);
                        const ReduceLayout at = reduce_layout(head, partial, n, scalar, given);
                        // the formula of the two entries, restated: the head, the partial sums, then what is borrowed, in this order
                        const size_t b_state = given.state_end ? 0 : a256((size_t)n * 8 * scalar), b_hit = given.hit32 ? 0 : a256((size_t)n * sizeof(uint32_t)),
                                     b_g = given.g ? 0 : a256((size_t)n * scalar);
                        const size_t off_borrow = head + old_partial_bytes(n, items);
                        if (at.partial != head) return bad("offset differs from the old formula", "partial", n, scalar, head, items, given);
                        if (at.state_end != off_borrow) return bad("offset differs from the old formula", "state_end", n, scalar, head, items, given);
                        if (at.hit32 != off_borrow + b_state) return bad("offset differs from the old formula", "hit32", n, scalar, head, items, given);
                        if (at.g != off_borrow + b_state + b_hit) return bad("offset differs from the old formula", "g", n, scalar, head, items, given);
                        if (at.bytes != off_borrow + b_state + b_hit + b_g) return bad("total differs from the old formula", "total", n, scalar, head, items, given);
                        // the bytes a block must hold when it is there; what the layout gives it: up to the next offset
                        const uint64_t pass = items < 1024 ? items : 1024;
                        const Block blocks[] = {{"head", 0, head},
                                                {"partial", at.partial, (size_t)(3 * reduce_blocks(n) * pass * sizeof(double))},
                                                {"state_end", at.state_end, given.state_end ? 0 : (size_t)n * 8 * scalar},
                                                {"hit32", at.hit32, given.hit32 ? 0 : (size_t)n * sizeof(uint32_t)},
                                                {"g", at.g, given.g ? 0 : (size_t)n * scalar}};
                        const int nb = sizeof blocks / sizeof blocks[0];
                        if (at.bytes % 256) return bad("the total is not 256-aligned", "total", n, scalar, head, items, given);
                        for (int b = 0; b < nb; b++) {
                            const size_t next = b + 1 < nb ? blocks[b + 1].at : at.bytes;
                            if (blocks[b].at % 256) return bad("not 256-aligned", blocks[b].name, n, scalar, head, items, given);
                            if (next < blocks[b].at || next > at.bytes) return bad("out of order or beyond the total", blocks[b].name, n, scalar, head, items, given);
                            const size_t room = next - blocks[b].at;
                            if (blocks[b].bytes == 0 && room != 0) return bad("an absent block takes bytes", blocks[b].name, n, scalar, head, items, given);
                            if (room < blocks[b].bytes) return bad("too small", blocks[b].name, n, scalar, head, items, given);
                            if (room >= blocks[b].bytes + 256) return bad("more than one alignment unit of slack", blocks[b].name, n, scalar, head, items, given);
                            for (int c = 0; c < b; c++)   // disjoint from every other block that is there
                                if (blocks[c].bytes && blocks[b].bytes && blocks[c].at + blocks[c].bytes > blocks[b].at)
                                    return bad("overlaps an earlier block", blocks[b].name, n, scalar, head, items, given);
                        }
                        cases++;
                    }
    std::printf("%d cases\n", cases);
    return 0;
}
