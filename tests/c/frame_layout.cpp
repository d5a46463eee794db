// The frame scratch of a stream (frame_layout, csrc/rtgr_internal.hpp) over every combination of borrowed blocks and front matter: a host-only
// program, built against the header alone (tests/test_frame_stages.py).  Prints the number of cases and exits 0, or names the first
// case that breaks a rule and exits 1.
#include <cstdio>

#include "rtgr_internal.hpp"

using namespace rtgr;

struct Block { const char* name; size_t at, bytes; };

static int bad(const char* what, const char* block, uint64_t n, size_t scalar, const FrameNeeds& need) {
    std::printf("%s (%s): n = %llu, scalar = %zu, state_end %d hit32 %d status %d list %d obs %d\n", what, block, (unsigned long long)n, scalar,
                need.state_end, need.hit32, need.status, need.list, need.obs);
    return 1;
}

int main() {
    const uint64_t sizes[] = {1, 77, 2496, 1000003};
    const size_t scalars[] = {4, 8};
    const bool front[3][2] = {{false, false}, {true, false}, {false, true}};   // (list, obs): a plain, an anti-aliased, an observer frame
    int cases = 0;
    for (uint64_t n : sizes)
        for (size_t scalar : scalars)
            for (const bool* f : front)
                for (int borrowed = 0; borrowed < 8; borrowed++) {
                    FrameNeeds need;
                    need.state_end = borrowed & 1; need.hit32 = borrowed & 2; need.status = borrowed & 4;
                    need.list = f[0]; need.obs = f[1];
                    const FrameLayout at = frame_layout(n, scalar, need);
                    // the bytes a block must hold when it is there; what the layout gives it: up to the next offset
                    const Block blocks[] = {{"head", 0, sizeof(rtgr_counters) + sizeof(unsigned long long)},
                                            {"obs", at.obs, need.obs ? sizeof(ObsFrame<double>) : 0},
                                            {"list", at.list, need.list ? n * sizeof(uint64_t) : 0},
                                            {"state_end", at.state_end, need.state_end ? n * 8 * scalar : 0},
                                            {"hit32", at.hit32, need.hit32 ? n * sizeof(uint32_t) : 0},
                                            {"status", at.status, need.status ? n : 0}};
                    const int nb = sizeof blocks / sizeof blocks[0];
                    if (at.bytes % 256) return bad("the total is not 256-aligned", "total", n, scalar, need);
                    for (int b = 0; b < nb; b++) {
                        const size_t next = b + 1 < nb ? blocks[b + 1].at : at.bytes;
                        if (blocks[b].at % 256) return bad("not 256-aligned", blocks[b].name, n, scalar, need);
                        if (next < blocks[b].at || next > at.bytes) return bad("out of order or beyond the total", blocks[b].name, n, scalar, need);
                        const size_t room = next - blocks[b].at;
                        if (blocks[b].bytes == 0 && room != 0) return bad("an absent block takes bytes", blocks[b].name, n, scalar, need);
                        if (room < blocks[b].bytes) return bad("too small", blocks[b].name, n, scalar, need);
                        if (room >= blocks[b].bytes + 256 && b != 0 && b != 1) return bad("more than one alignment unit of slack", blocks[b].name, n, scalar, need);
                        // disjoint from every other block that is there
                        for (int c = 0; c < b; c++)
                            if (blocks[c].bytes && blocks[b].bytes && blocks[c].at + blocks[c].bytes > blocks[b].at)
                                return bad("overlaps an earlier block", blocks[b].name, n, scalar, need);
                    }
                    if (blocks[0].at != 0 || at.obs < sizeof(rtgr_counters)) return bad("the head does not hold rtgr_counters", "head", n, scalar, need);
                    cases++;
                }
    std::printf("%d cases\n", cases);
    return 0;
}
