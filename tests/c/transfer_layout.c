/* pins sizeof(rtgr_flow) and the offsets of its members at compile time, and prints them as a C compiler lays them out
   (tests/test_transfer.py holds the ctypes mirror to the same numbers) */
#include <stddef.h>
#include <stdio.h>

#include "rtgr.h"

_Static_assert(sizeof(rtgr_flow) == 104, "rtgr_flow is 104 bytes");
_Static_assert(offsetof(rtgr_flow, emitter) == 0 && offsetof(rtgr_flow, flags) == 4 && offsetof(rtgr_flow, orbit) == 8, "emitter, flags, orbit");
_Static_assert(offsetof(rtgr_flow, j0) == 16 && offsetof(rtgr_flow, kappa) == 24, "j0, kappa");
_Static_assert(offsetof(rtgr_flow, r0) == 32 && offsetof(rtgr_flow, alpha) == 40 && offsetof(rtgr_flow, H) == 48 && offsetof(rtgr_flow, s) == 56,
               "r0, alpha, H, s");
_Static_assert(offsetof(rtgr_flow, r_stop) == 64 && offsetof(rtgr_flow, gain) == 72 && offsetof(rtgr_flow, weight) == 80, "r_stop, gain, weight");

int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtgr_flow), offsetof(rtgr_flow, emitter), offsetof(rtgr_flow, flags),
           offsetof(rtgr_flow, orbit), offsetof(rtgr_flow, j0), offsetof(rtgr_flow, kappa), offsetof(rtgr_flow, r0), offsetof(rtgr_flow, alpha),
           offsetof(rtgr_flow, H), offsetof(rtgr_flow, s), offsetof(rtgr_flow, r_stop), offsetof(rtgr_flow, gain), offsetof(rtgr_flow, weight));
    return 0;
}
