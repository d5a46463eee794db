// The bookkeeping of a device's id-named tables (Resident<T>, csrc/rtgr_host.hpp) for both kinds, GridTable and TextureTable: a host-only
// program, built against the header alone (tests/test_tables.py).  The "device pointers" are made-up numbers: the container never looks at
// them, it only hands them back to be freed.  Prints the number of checks and exits 0, or names the first one that fails and exits 1.
#include <algorithm>
#include <cstdio>

#include "rtgr_host.hpp"

using namespace rtgr;

static int checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        checks++;                                                                \
        if (!(cond)) { std::printf("%s: line %d: %s\n", kind, __LINE__, #cond); return 1; } \
    } while (0)

template <class T>
static T table(uint64_t id) {   // the pointers of table id: 16 id and 16 id + 8
    T t;
    t.id = id;
    t.d64 = (void*)(uintptr_t)(16 * id);
    t.d32 = (void*)(uintptr_t)(16 * id + 8);
    return t;
}
// whether `got` holds exactly the two pointers of each of `ids`, each once
static bool pointers_of(std::vector<void*> got, std::vector<uint64_t> ids) {
    std::vector<void*> want;
    for (uint64_t id : ids) { want.push_back((void*)(uintptr_t)(16 * id)); want.push_back((void*)(uintptr_t)(16 * id + 8)); }
    std::sort(got.begin(), got.end());
    std::sort(want.begin(), want.end());
    return got == want;
}

template <class T>
static int run(const char* kind) {
    const uint64_t ids[] = {0x7000000000000001ull, 0xA000000000000002ull, 3, 4, 5};
    Resident<T> r;
    // retire on an empty set: "all" reports true (the texture rule), id 0 without it and any other id false (the grid rule)
    CHECK(r.retire(0, true));
    CHECK(!r.retire(0, false));
    CHECK(!r.retire(3, true) && !r.retire(3, false));
    CHECK(r.n_resident() == 0 && r.n_retired() == 0 && r.drain(true).empty());
    // published ids are found, with their own pointers; an unknown id is not, and its retire reports false
    for (uint64_t id : ids) r.publish(table<T>(id));
    for (uint64_t id : ids) CHECK(r.find(id) && r.find(id)->id == id && r.find(id)->d64 == table<T>(id).d64 && r.find(id)->d32 == table<T>(id).d32);
    CHECK(!r.find(6) && !r.find(0));
    CHECK(!r.retire(6, false) && !r.retire(6, true));
    CHECK(!r.retire(0, false));
    CHECK(r.n_resident() == 5 && r.n_retired() == 0);
    // retire(id) moves exactly that entry, after which the id is unknown (a second retire reports false)
    CHECK(r.retire(3, false));
    CHECK(!r.find(3) && !r.retire(3, false) && !r.retire(3, true));
    for (uint64_t id : ids) CHECK(id == 3 || r.find(id));
    CHECK(r.n_resident() == 4 && r.n_retired() == 1);
    CHECK(r.retire(ids[0], true));   // (zero_means_all changes nothing for an id that is not 0)
    CHECK(r.n_resident() == 3 && r.n_retired() == 2);
    // draining the retired entries: each retired pointer exactly once, the resident entries left alone; a second drain gives nothing
    CHECK(pointers_of(r.drain(false), {3, ids[0]}));
    CHECK(r.drain(false).empty());
    CHECK(r.n_resident() == 3 && r.n_retired() == 0);
    CHECK(r.find(ids[1]) && r.find(4) && r.find(5) && !r.find(3) && !r.find(ids[0]));
    // retire(0) with zero_means_all moves everything
    CHECK(r.retire(4, false));
    CHECK(r.retire(0, true));
    CHECK(r.n_resident() == 0 && r.n_retired() == 3);
    CHECK(!r.find(ids[1]) && !r.find(4) && !r.find(5));
    // draining all: every pointer exactly once — retired and resident — and the set is empty
    r.publish(table<T>(7));
    r.publish(table<T>(8));
    CHECK(pointers_of(r.drain(true), {ids[1], 4, 5, 7, 8}));
    CHECK(r.n_resident() == 0 && r.n_retired() == 0 && !r.find(7) && r.drain(true).empty());
    return 0;
}

int main() {
    if (run<GridTable>("GridTable") || run<TextureTable>("TextureTable")) return 1;
    std::printf("%d checks\n", checks);
    return 0;
}
